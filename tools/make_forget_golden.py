"""Writes tests/golden/csm1b_forget.pt: the ORACLE's greedy codes of a two-turn conversation at CSM-1B shapes that FORGETS rows [190, 490) of
its history between the turns, for tests/test_session_forget_gpu.py (include/csm_hip.h csm_session_forget, sesameai/sessions.py
Conversation.forget_rows).  oracle/csm_ref.py is imported unchanged; nothing of the product runs here.

The checkpoint is csm1b_decisive_copy.pt's long-lag one (`decisive_copy:3:700`: c0 of a frame names the last code of the row 700 back, read
out of layer 3's cached K / V).  Turn 1 is that golden's 1,334-row prompt and FRAMES frames.  Then the oracle's backbone cache is EDITED the
way csm_session_forget is defined -- rows below 190 untouched; rows from 490 on moved down by 300, V as it is, K rotated back by 300
positions with (cos, sin)(300 theta) computed in float64 and rounded to float, fp32 arithmetic on the bf16 values, one rounding -- and turn 2
(the EOS row, a user segment, the reply's text: 24 rows) runs on it.  Per weight format (bf16, fp8-dequantised) it is checked here that

  * the edited-cache oracle's codes of turn 2, the cold oracle's codes of the TRIMMED prompt and `decisive_copy_expected_codes` of the
    trimmed prompt are equal bit for bit;
  * the smallest top-1 / top-2 margin of turn 2 is at least 4 x the largest logit difference between the edited-cache and the cold run;
  * frame 0 of turn 2 reads a MOVED row: 190 <= S' - 1 - 700 < the rows held after the forget.

The file holds the new rows, the codes of both turns, the margins and the gap.

    python tools/make_forget_golden.py            # CSM-1B, several minutes of CPU
    python tools/make_forget_golden.py --tiny     # the tiny shapes, seconds, nothing written
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import csm_ref as C                                                     # noqa: E402
from oracle.make_golden import DECISIVE_CHECKSUM_NAMES, bench_prompt, toy_prompt    # noqa: E402

FRAMES = 6


def user_turn(shape, seed):
    """The rows that are new in turn 2: the user's segment (6 text rows, 8 audio frames + EOS) and the reply's text (8 rows)."""
    g = torch.Generator().manual_seed(seed)
    ids = lambda k: torch.randint(0, shape.text_vocab_size, (k,), generator=g).tolist()
    return C.build_prompt([(ids(6), torch.randint(0, 2048, (shape.audio_num_codebooks, 8), generator=g)), (ids(8), None)])


@torch.inference_mode()
def run(om, tok, msk, start, n):
    """Rows [start, S) of the prompt, then n greedy frames, on the backbone cache as it is: (codes (n, 32) int32, logits (n, 32, V) fp32)."""
    S = tok.shape[0]
    cur_t, cur_m, pos = tok[start:].unsqueeze(0), msk[start:].unsqueeze(0), torch.arange(start, S).unsqueeze(0)
    codes, logits = [], []
    for _ in range(n):
        tr = C.FrameTrace()
        fr = om.generate_frame(cur_t, cur_m, pos, 1.0, 1, greedy=True, trace=tr)
        codes.append(fr[0].to(torch.int32)); logits.append(torch.stack(tr.logits)[:, 0].float())
        cur_t = torch.cat([fr.long(), torch.zeros(1, 1).long()], dim=1).unsqueeze(1)
        cur_m = torch.cat([torch.ones_like(fr).bool(), torch.zeros(1, 1).bool()], dim=1).unsqueeze(1)
        pos = pos[:, -1:] + 1
    return torch.stack(codes), torch.stack(logits)


def forget_in_cache(om, a, b, held):
    """csm_session_forget on the oracle's backbone cache, rows [0, held)."""
    s, d = om.shape.backbone, b - a
    ang = float(d) * C.llama3_scaled_rope_theta(s.head_dim, s.rope_base, s.scale_factor).double()
    c, sn = torch.cos(ang).float(), torch.sin(ang).float()
    for k, v in zip(om.backbone.k, om.backbone.v):
        x = k[0, :, b:held].float().unflatten(-1, (-1, 2))
        x0, x1 = x[..., 0], x[..., 1]
        k[0, :, a:held - d] = torch.stack([x0 * c + x1 * sn, x1 * c - x0 * sn], dim=-1).flatten(-2).to(k.dtype)
        v[0, :, a:held - d] = v[0, :, b:held].clone()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiny", action="store_true", help="tiny shapes, nothing written")
    args = ap.parse_args()
    seed = 1234
    if args.tiny:
        shape, flavour, (a, b) = C.csm_tiny(), "decisive_copy:1:40", (20, 50)
        first = toy_prompt(shape, 12, 20, 120)
    else:
        shape, (a, b) = C.csm_1b(), (190, 490)
        first = bench_prompt(shape, 5000, segments=10, ctx_text=30, ctx_frames=100)
        flavour = f"decisive_copy:3:{(first[0].shape[0] * 21) // 40}"          # csm1b_decisive_copy.pt's s1334
    layer, lag = C.copy_flavour_params(shape, flavour)
    w = C.make_weights(shape, seed=seed, flavour=flavour)
    names = [n for n in DECISIVE_CHECKSUM_NAMES + [f"backbone.layers.{layer}.attn.{t}_proj.weight" for t in ("q", "k", "v", "output")] if n in w]
    new = user_turn(shape, 7202)
    gold = dict(weight_seed=seed, flavour=flavour, frames=FRAMES, prompt_rows=first[0].shape[0], prompt_seed=5000, forget=(a, b), lag=lag,
                new_tokens=new[0].to(torch.int32), new_mask=new[1],
                weight_checksums=(names, torch.stack([w[n].view(torch.int16).to(torch.int64).sum() for n in names])))
    eos = C.audio_rows(torch.zeros(shape.audio_num_codebooks, 0, dtype=torch.long))
    for tag in ("bf16", "fp8"):
        ww = w if tag == "bf16" else C.fp8_dequantized(w)
        om = C.OracleModel(shape, ww)
        om.setup_caches(1)
        t0 = time.time()
        S = first[0].shape[0]
        codes1, _ = run(om, first[0], first[1], 0, FRAMES)
        assert torch.equal(codes1, C.decisive_copy_expected_codes(shape, seed, first[0], first[1], FRAMES, lag)), "turn 1 left the copy trajectory"
        ft, fm = C.audio_rows(codes1.long().t())
        hist = torch.cat([first[0], ft[:-1]]), torch.cat([first[1], fm[:-1]])          # the mirror: the prompt and the frames, no closing EOS row yet
        held = S + FRAMES - 1
        forget_in_cache(om, a, b, held)
        held -= b - a
        trimmed = tuple(torch.cat([h[:a], h[b:], e, x]) for h, e, x in zip(hist, eos, new))
        S2 = trimmed[0].shape[0]
        assert a <= S2 - 1 - lag < held, "frame 0 of turn 2 does not read a moved row"
        codes2, log_e = run(om, trimmed[0], trimmed[1], held, FRAMES)
        om.reset_caches()
        cold2, log_c = run(om, trimmed[0], trimmed[1], 0, FRAMES)
        want = C.decisive_copy_expected_codes(shape, seed, trimmed[0], trimmed[1], FRAMES, lag)
        assert torch.equal(codes2, want), "the edited-cache oracle leaves the analytic codes of the trimmed prompt"
        assert torch.equal(cold2, want), "the cold oracle leaves the analytic codes of the trimmed prompt"
        margin = min(float((lg.topk(2, dim=-1).values[..., 0] - lg.topk(2, dim=-1).values[..., 1]).min()) for lg in (log_e, log_c))
        gap = float((log_e - log_c).abs().max())
        assert margin >= 4 * gap, f"{tag}: margin {margin} < 4 x gap {gap}"
        print(f"  {tag}: turn 1 {S} rows, forget [{a}, {b}), turn 2 {S2} rows ({S2 - held} after the {held} held), {FRAMES} frames each; "
              f"margin {margin:.3f}, edited-vs-cold gap {gap:.4f}, ratio {margin / gap:.1f}; {time.time() - t0:.0f}s", flush=True)
        gold[tag] = dict(codes1=codes1.to(torch.int16), codes2=codes2.to(torch.int16), full_rows2=S2, held2=held, margin=margin, gap=gap)
    if args.tiny:
        print("tiny: ok (nothing written)")
        return
    out = os.path.join(ROOT, "tests", "golden", "csm1b_forget.pt")
    torch.save(gold, out)
    print(f"wrote {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
