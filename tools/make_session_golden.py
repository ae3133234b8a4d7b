"""Writes tests/golden/csm1b_sessions.pt: the ORACLE's cold greedy codes of a three-turn conversation at CSM-1B shapes, for
tests/test_sessions_gpu.py (conversation sessions: include/csm_hip.h csm_session_*, sesameai/sessions.py).  oracle/csm_ref.py is imported
unchanged.

The checkpoint is the long-lag history-dependent decisive one of csm1b_decisive_copy.pt (`decisive_copy:3:700`: c0 of a frame names the
last code of the row 700 back, read out of layer 3's cached K / V).  Turn 1's prompt is that golden's 1,334-row prompt; turns 2 and 3 add a
short user segment and the reply's text; every reply is FRAMES frames (the copy trajectory never samples EOS, so every reply is cut at
its limit).  Per weight format (bf16, fp8-dequantised) and turn the file holds the rows that are new in that turn, the number of rows of
the cold prompt, and the cold codes -- each asserted to be the trajectory the construction implies.

It also holds the oracle-only proof that the golden can SEE a fault in the rows a session carries: after the cold prompt of turns 2 and 3
has run, the copy layer's K / V rows [0, held) -- held = the rows a session's pages hold at that point -- are zeroed, or their V rows are
moved one position late (each key then finds its neighbour's value), and the frames after frame 0 (which the prompt's own call computed)
are generated again: they must differ from the cold codes (`faults_changed`: how many of them do).  A golden that these faults leave
alone would be no test of a load.  (K and V moved TOGETHER cannot be seen by this checkpoint: a key carries its position in its rotation,
so the copy finds the same row wherever it lies.  That fault is the copy-kernel tests' business: a loaded slot equals its source bit for bit.)

    python tools/make_session_golden.py            # CSM-1B, several minutes of CPU
    python tools/make_session_golden.py --tiny     # the tiny shapes, seconds: checks this file's frame loop against oracle.csm_ref.generate_codes
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

FRAMES = 12
FAULTS = ("zero", "shift_v")


def user_turn(shape, seed):
    """The rows that are new in a later turn: the user's segment (6 text rows, 8 audio frames + EOS) and the reply's text (8 rows)."""
    g = torch.Generator().manual_seed(seed)
    ids = lambda k: torch.randint(0, shape.text_vocab_size, (k,), generator=g).tolist()
    return C.build_prompt([(ids(6), torch.randint(0, 2048, (shape.audio_num_codebooks, 8), generator=g)), (ids(8), None)])


def frame_rows(codes):
    """Generated frames (n, 32) as prompt rows WITHOUT the closing EOS row."""
    t, m = C.audio_rows(codes.t())
    return t[:-1], m[:-1]


@torch.inference_mode()
def run_turn(om, layer, tok, msk, n, held):
    """The cold greedy codes (n, 32) of the prompt, and per fault the codes with the copy layer's carried rows [0, held) faulted after the
    prompt's call (held = 0: no fault runs)."""
    om.reset_caches()
    S = tok.shape[0]
    f0 = om.generate_frame(tok.unsqueeze(0), msk.unsqueeze(0), torch.arange(S).unsqueeze(0), 1.0, 1, greedy=True)
    k, v = om.backbone.k[layer], om.backbone.v[layer]
    snap = (k[:, :, :S].clone(), v[:, :, :S].clone())

    def rest():
        frames, cur = [f0], f0
        for f in range(1, n):
            t = torch.cat([cur.long(), torch.zeros(1, 1).long()], dim=1).unsqueeze(1)
            mk = torch.cat([torch.ones_like(cur).bool(), torch.zeros(1, 1).bool()], dim=1).unsqueeze(1)
            cur = om.generate_frame(t, mk, torch.tensor([[S + f - 1]]), 1.0, 1, greedy=True)
            frames.append(cur)
        return torch.cat(frames).to(torch.int32)

    cold = rest()
    faulted = {}
    for name in FAULTS if held else ():
        k[:, :, :S], v[:, :, :S] = snap[0], snap[1]
        if name == "zero":
            k[:, :, :held] = 0; v[:, :, :held] = 0
        else:
            v[:, :, 1:held] = snap[1][:, :, :held - 1]
        faulted[name] = rest()
    return cold, faulted


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiny", action="store_true", help="tiny shapes, nothing written: this file's loop against oracle.csm_ref.generate_codes")
    args = ap.parse_args()
    seed = 1234
    if args.tiny:
        shape, flavour = C.csm_tiny(), "decisive_copy:1:40"
        first = toy_prompt(shape, 12, 20, 60)
    else:
        shape = C.csm_1b()
        first = bench_prompt(shape, 5000, segments=10, ctx_text=30, ctx_frames=100)
        flavour = f"decisive_copy:3:{(first[0].shape[0] * 21) // 40}"          # oracle/make_golden.py copy_long_flavour: csm1b_decisive_copy.pt's s1334
    layer, lag = C.copy_flavour_params(shape, flavour)
    w = C.make_weights(shape, seed=seed, flavour=flavour)
    names = [n for n in DECISIVE_CHECKSUM_NAMES + [f"backbone.layers.{layer}.attn.{t}_proj.weight" for t in ("q", "k", "v", "output")] if n in w]
    gold = dict(weight_seed=seed, flavour=flavour, frames=FRAMES, prompt_rows=first[0].shape[0], prompt_seed=5000,
                weight_checksums=(names, torch.stack([w[n].view(torch.int16).to(torch.int64).sum() for n in names])))
    news = [first, user_turn(shape, 7102), user_turn(shape, 7103)]
    for tag in ("bf16", "fp8"):
        om = C.OracleModel(shape, w if tag == "bf16" else C.fp8_dequantized(w))
        om.setup_caches(1)
        hist_t, hist_m, held, turns = first[0][:0], first[1][:0], 0, []
        for k, (nt, nm) in enumerate(news):
            t0 = time.time()
            if k:                                               # the EOS row that closes the last reply's audio
                e_t, e_m = C.audio_rows(torch.zeros(shape.audio_num_codebooks, 0, dtype=torch.long))
                hist_t, hist_m = torch.cat([hist_t, e_t]), torch.cat([hist_m, e_m])
            tok, msk = torch.cat([hist_t, nt]), torch.cat([hist_m, nm])
            S = tok.shape[0]
            codes, faulted = run_turn(om, layer, tok, msk, FRAMES, held)
            assert torch.equal(codes, C.decisive_copy_expected_codes(shape, seed, tok, msk, FRAMES, lag)), "the oracle left the trajectory the construction implies"
            assert not bool((codes == 0).all(dim=1).any()), "an all-zero (EOS) frame"
            if args.tiny:
                ref = torch.cat(C.generate_codes(om, tok, msk, FRAMES * 80, 1.0, 1, greedy=True, max_seq_len=shape.backbone.max_seq_len)).to(torch.int32)
                assert torch.equal(ref, codes), "this file's frame loop is not oracle.csm_ref.generate_codes's"
            changed = {name: int((got[1:] != codes[1:]).any(dim=1).sum()) for name, got in faulted.items()}
            if k:
                assert S - 1 - lag < held, "frame 1 does not read a carried row"
                assert all(changed[name] > 0 for name in FAULTS), f"turn {k + 1}: a fault in the carried rows leaves the codes alone: {changed}"
            print(f"  {tag} turn {k + 1}: {S} rows ({S - held} after the {held} carried), {FRAMES} frames in {time.time() - t0:.0f}s; "
                  f"frames 1.. changed by faults in the carried rows: {changed}", flush=True)
            turns.append(dict(new_tokens=nt.to(torch.int32) if k else None, new_mask=nm if k else None, full_rows=S, held=held,
                              codes=codes.to(torch.int16), faults_changed=changed))
            f_t, f_m = frame_rows(codes.long())
            hist_t, hist_m = torch.cat([tok, f_t]), torch.cat([msk, f_m])
            held = S + FRAMES - 1                               # cut at its limit: the last frame's row is not in the cache (sesameai/sessions.py)
        gold[tag] = turns
    if args.tiny:
        print("tiny: ok (nothing written)")
        return
    out = os.path.join(ROOT, "tests", "golden", "csm1b_sessions.pt")
    torch.save(gold, out)
    print(f"wrote {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
