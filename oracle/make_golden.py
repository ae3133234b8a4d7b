"""Generates the committed golden vectors under tests/golden/ from the oracle.

TEST INFRASTRUCTURE ONLY.  Run here (CPU, minutes):  python -m oracle.make_golden [--only ...]
Nothing in this script reads /root/reference; the vectors are functions of the oracle code,
the seeds below and torch's CPU generator.

Files (all torch.save'd dicts of small tensors):
  csm1b_frames.pt   CSM-1B shapes, seeded weights (seed 1234), config-1 prompt (16 text tokens):
                    the oracle's greedy trajectory for N frames, and for every frame/codebook
                    the top-8 (value, index) of the bf16 logits, teacher-forced on that
                    trajectory, plus the bf16-vs-fp32 oracle logit gap (the rounding-noise floor
                    any bf16 implementation lives in).
  tiny_frames.pt    same for the tiny shapes with a 2-segment prompt, full logits kept.
  sampler_cases.pt  sample_topk inputs/outputs incl. tie cases and supplied Exp(1) noise.
  prompt_layout.pt  (tokens, mask) of a 2-segment toy prompt (generator.py:63-109 layout).
  mimi_*.pt         Mimi decode of a seeded (1,32,10) code block: whole and stateless chunks.
  csm1b_cfg2.pt     CSM-1B, BASELINE config 2's prompt (bench.py's seeded S=190 prompt: 40 text + 125 audio + EOS + 24 text
                    rows): 6 greedy frames, top-8 logits, margins, bf16-vs-fp32 gap.
  csm1b_cfg3.pt     the same shape at B=32 (bench.py's prompts of utterances 0..31): 2 frames of the batched oracle, top-8
                    logits and margins per (frame, codebook, utterance).
  csm1b_cfg5.pt     BASELINE config 5: fp8-e4m3-dequantised weights (oracle.csm_ref.fp8_dequantized), S=1334 prompt (10
                    segments), 2 frames; and a 1700-row prompt: the prompt frame (p = 1699) and one step frame (p = 1700).
  csm1b_cfg5b.pt    config 5 batched at B = 4 (four different 1334-row prompts), 2 frames of the batched oracle.
  csm1b_cfg5c.pt    config 5 at B = 32 (the batch SURVEY.md 8d names): top-8 logits / codes / margins only, prompts by seed.
  csm1b_decisive.pt CSM-1B with the DECISIVE synthetic checkpoint (oracle.csm_ref.decisive_weights): the oracle's FREE-RUNNING greedy
                    codes -- 64 frames at B = 1 for the 190-row and the 1334-row prompt, 16 frames at B = 32, twelve utterances of mixed
                    lengths for the refilled batch -- each with bf16 and with fp8-dequantised weights, every row's top-1 / top-2 margin
                    asserted >= 4 x the oracle's bf16-vs-fp32 gap on that run; + the Mimi oracle's PCM of the first clip.
  tiny_decisive.pt  the same for the tiny shapes (full logits of the first frames kept).
  csm1b_decisive_copy.pt / tiny_decisive_copy.pt
                    the HISTORY-DEPENDENT decisive checkpoint (oracle.csm_ref.decisive_copy_weights: c0 of a frame names the last code of
                    the row `lag` positions back, read through one backbone layer's cached K / V): free-running greedy codes for the
                    190-row prompt (copy layer 8, lag 3: from frame 4 on the rows read are the ones the frame steps appended), for the
                    1334-row prompt (copy layer 3, lag 700: a key in the middle of the split key range) and at B = 32; bf16 and
                    fp8-dequantised; margin >= 4 x gap on every row, the implied trajectory asserted, and KV faults injected into the
                    oracle (stale rows, a wrong RoPE position, a dropped key range, zeroed prompt rows) asserted to CHANGE the codes.
  csm1b_decisive_dcopy.pt / tiny_decisive_dcopy.pt   (--only dcopy; dcopytiny / dcopyfull: one of the two)
                    the DECODER-side copy checkpoint (oracle.csm_ref.decisive_dcopy_variant: step p of a frame names the code `lag` decoder
                    positions back, read through one decoder layer's cached K / V): 8 free-running frames at B = 1, 4 of a batch whose
                    utterances have last text tokens of their own, the twelve utterances of the refilled batch; per-row margins and gaps,
                    checksums of every tensor; KV faults in that decoder layer asserted to CHANGE the codes, the same faults in another
                    decoder layer, in the backbone, and on the two flavours above asserted to change nothing.
  csm1b_possweep.pt CSM-1B bench checkpoint, ONE 2046-row prompt cut at S in POSSWEEP_S: for every S the prompt frame and two teacher-forced
                    steps at positions S and S + 1 (top-8 logits, codes, margins, the bf16-vs-fp32 gap), bf16 and fp8-dequantised; plus 64
                    CONSECUTIVE teacher-forced steps after a 740-row prompt (positions 740..803: across the one-launch backbone layer's
                    switch from one CU per head to the key range split over 8 CUs at 768).
  csm1b_norms.pt    CSM-1B checkpoints whose RMSNorm scales are not 1 (oracle.csm_ref.norm_test_weights, seed 1234: `jitter` and
                    `outlier`), legs A-F of NORMS_LEGS (bf16 / fp8-dequantised, config-2 and config-5 prompts): top-8 logits, codes,
                    margins and the bf16-vs-fp32 gap per frame; for legs A and E the move of the logits (at the golden's top-8
                    indices, frame 0) under each scale fault of oracle.csm_ref.NORM_FAULTS that clears 1.5 x the leg's gap.
                    About 2 minutes on 8 CPU threads.
  mimi_long.pt      full-size Mimi (seed 4321 weights) at real clip lengths (MIMI_LONG): the oracle's PCM of seeded 126 / 150 / 300 / 1125-frame
                    clips (every 16th sample + head / tail windows; the codes are a function of the stored seeds), the oracle's codes of a 5 s and a
                    10.4 s voice prompt, and per clip how far the compared samples move when the oracle's attention window is 249, 251 or unbounded
                    or its RoPE angle is taken modulo the stream pool's ring (270): each asserted >= 10 x the 2e-5-of-peak bound of the GPU test
                    wherever the fault touches the clip; for the prompts the frames whose codes change, and the share of frames a 1e-6 nudge of
                    the latent leaves alone (the inputs do not sit on quantiser ties).  The wall time of every oracle run is stored beside it.
"""
from __future__ import annotations

import argparse
import os
import time

import torch

from . import csm_ref as C
from . import mimi_ref as M

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


def toy_prompt(shape: C.CsmShape, seed: int, n_text: int, ctx_frames: int):
    g = torch.Generator().manual_seed(seed)
    segs = []
    if ctx_frames:
        ids = torch.randint(0, shape.text_vocab_size, (n_text,), generator=g).tolist()
        codes = torch.randint(0, 2048, (shape.audio_num_codebooks, ctx_frames), generator=g)
        segs.append((ids, codes))
    ids = torch.randint(0, shape.text_vocab_size, (n_text,), generator=g).tolist()
    segs.append((ids, None))
    return C.build_prompt(segs)


@torch.inference_mode()
def frames_golden(shape: C.CsmShape, weights, prompt, n_frames: int, keep_full: bool, with_fp32: bool, quiet: bool = False, w32=None):
    tok, msk = prompt
    m = C.OracleModel(shape, weights)
    m.setup_caches(1)
    m32 = None
    if with_fp32:
        m32 = C.OracleModel(shape, w32 if w32 is not None else {k: v.float() for k, v in weights.items()}, dtype=torch.float32)
        m32.setup_caches(1)
    cur_t, cur_m = tok.unsqueeze(0), msk.unsqueeze(0)
    pos = torch.arange(tok.size(0)).unsqueeze(0)
    codes, top_v, top_i, full, gap, margin = [], [], [], [], [], []
    for f in range(n_frames):
        t0 = time.time()
        tr = C.FrameTrace()
        # greedy frame; the oracle feeds back its own choice == teacher forcing on its trajectory
        s = m.generate_frame(cur_t, cur_m, pos, 1.0, 1, greedy=True, trace=tr)
        lg = torch.stack(tr.logits, 0)[:, 0]                     # (32, V) bf16
        v, i = torch.topk(lg.float(), 8, dim=-1)
        codes.append(s[0]); top_v.append(v.to(torch.bfloat16)); top_i.append(i.to(torch.int16))
        margin.append((v[:, 0] - v[:, 1]))
        if keep_full:
            full.append(lg)
        if m32 is not None:
            tr32 = C.FrameTrace()
            m32.generate_frame(cur_t, cur_m, pos, 1.0, 1, greedy=True, forced=s, trace=tr32)
            lg32 = torch.stack(tr32.logits, 0)[:, 0]
            gap.append((lg.float() - lg32).abs().max(dim=-1)[0])
        cur_t = torch.cat([s.long(), torch.zeros(1, 1).long()], dim=1).unsqueeze(1)
        cur_m = torch.cat([torch.ones_like(s).bool(), torch.zeros(1, 1).bool()], dim=1).unsqueeze(1)
        pos = pos[:, -1:] + 1
        if not quiet:
            print(f"  frame {f}: {time.time() - t0:.1f}s  c0..3={s[0, :4].tolist()}", flush=True)
    out = dict(prompt_tokens=tok, prompt_mask=msk, codes=torch.stack(codes), top_v=torch.stack(top_v),
               top_i=torch.stack(top_i), margin=torch.stack(margin))
    if keep_full:
        out["logits"] = torch.stack(full)
    if gap:
        out["bf16_vs_fp32_gap"] = torch.stack(gap)
    return out


def bench_prompt(shape: C.CsmShape, seed: int, segments: int = 1, ctx_text: int = 40, ctx_frames: int = 125, gen_text: int = 24):
    """bench.py::synthetic_prompt for one utterance (same generator call order), restated here so the golden files do
    not depend on the benchmark script; tests assert the two agree."""
    g = torch.Generator().manual_seed(seed)
    rows = segments * (ctx_text + ctx_frames + 1) + gen_text
    t = torch.zeros(rows, 33, dtype=torch.long)
    m = torch.zeros(rows, 33, dtype=torch.bool)
    r = 0
    for _ in range(segments):
        t[r:r + ctx_text, 32] = torch.randint(0, shape.text_vocab_size, (ctx_text,), generator=g); m[r:r + ctx_text, 32] = True
        r += ctx_text
        t[r:r + ctx_frames, :32] = torch.randint(0, 2048, (ctx_frames, 32), generator=g); m[r:r + ctx_frames + 1, :32] = True
        r += ctx_frames + 1
    t[r:r + gen_text, 32] = torch.randint(0, shape.text_vocab_size, (gen_text,), generator=g); m[r:r + gen_text, 32] = True
    return t, m


@torch.inference_mode()
def frames_golden_batch(shape: C.CsmShape, weights, toks, msks, n_frames: int):
    """Batched oracle (B utterances of equal length), greedy, teacher-forced on its own trajectory: per frame the codes
    [B][32], top-8 logits [32][B][8] and the top-1/top-2 margin [32][B]."""
    B = toks.shape[0]
    m = C.OracleModel(shape, weights)
    m.setup_caches(B)
    cur_t, cur_m = toks, msks
    pos = torch.arange(toks.size(1)).unsqueeze(0).repeat(B, 1)
    codes, top_v, top_i, margin = [], [], [], []
    for f in range(n_frames):
        t0 = time.time()
        tr = C.FrameTrace()
        s = m.generate_frame(cur_t, cur_m, pos, 1.0, 1, greedy=True, trace=tr)
        lg = torch.stack(tr.logits, 0)                           # (32, B, V) bf16
        v, i = torch.topk(lg.float(), 8, dim=-1)
        codes.append(s.clone()); top_v.append(v.to(torch.bfloat16)); top_i.append(i.to(torch.int16)); margin.append(v[..., 0] - v[..., 1])
        cur_t = torch.cat([s.long(), torch.zeros(B, 1).long()], dim=1).unsqueeze(1)
        cur_m = torch.cat([torch.ones_like(s).bool(), torch.zeros(B, 1).bool()], dim=1).unsqueeze(1)
        pos = pos[:, -1:] + 1
        print(f"  batch frame {f}: {time.time() - t0:.1f}s", flush=True)
    return dict(prompt_tokens=toks, prompt_mask=msks, codes=torch.stack(codes), top_v=torch.stack(top_v), top_i=torch.stack(top_i),
                margin=torch.stack(margin))


@torch.inference_mode()
def free_run(shape: C.CsmShape, weights, toks, msks, n_frames: int, what: str, keep_rows: bool = False):
    """The oracle's FREE-RUNNING greedy loop (generator.py:283-294 with topk = 1) on B equal-length prompts, beside an fp32 oracle that is
    fed the bf16 oracle's codes: codes [n][B][32], the smallest top-1 / top-2 margin and the largest bf16-vs-fp32 logit gap per frame.
    Asserts what the decisive checkpoint is for: every decision's margin >= 4 x the gap, and the trajectory the construction implies."""
    if toks.dim() == 2:
        toks, msks = toks.unsqueeze(0), msks.unsqueeze(0)
    B = toks.shape[0]
    m = C.OracleModel(shape, weights); m.setup_caches(B)
    m32 = C.OracleModel(shape, {k: v.float() for k, v in weights.items()}, dtype=torch.float32); m32.setup_caches(B)
    cur_t, cur_m = toks.long(), msks
    pos = torch.arange(toks.size(1)).unsqueeze(0).repeat(B, 1)
    codes, margins, gaps, rows = [], [], [], []
    t0 = time.time()
    for f in range(n_frames):
        tr, tr32 = C.FrameTrace(), C.FrameTrace()
        s = m.generate_frame(cur_t, cur_m, pos, 1.0, 1, greedy=True, trace=tr)
        m32.generate_frame(cur_t, cur_m, pos, 1.0, 1, greedy=True, forced=s, trace=tr32)
        lg, lg32 = torch.stack(tr.logits, 0).float(), torch.stack(tr32.logits, 0)       # [32][B][V]
        top2 = torch.topk(lg, 2, dim=-1)[0]
        margin, gap = (top2[..., 0] - top2[..., 1]), (lg - lg32).abs().amax(dim=-1)
        assert bool((margin >= 4.0 * gap.max()).all()), f"{what} frame {f}: margin {float(margin.min()):.3f} < 4 x gap {float(gap.max()):.4f}"
        assert not bool((s == 0).all(dim=1).any()), "an all-zero (EOS) frame"
        codes.append(s.clone()); margins.append(margin.min()); gaps.append(gap.max()); rows.append((margin, gap))
        cur_t = torch.cat([s.long(), torch.zeros(B, 1).long()], dim=1).unsqueeze(1)
        cur_m = torch.cat([torch.ones_like(s).bool(), torch.zeros(B, 1).bool()], dim=1).unsqueeze(1)
        pos = pos[:, -1:] + 1
    codes = torch.stack(codes)
    print(f"  {what}: {n_frames} frames x {B} in {time.time() - t0:.0f}s, smallest margin {float(min(margins)):.3f}, largest gap "
          f"{float(max(gaps)):.4f} ({float(min(margins)) / float(max(gaps)):.0f} x)", flush=True)
    out = dict(codes=codes.to(torch.int16), min_margin=torch.stack(margins), max_gap=torch.stack(gaps))
    if keep_rows:           # per (frame, codebook, utterance)
        out["margin"], out["gap"] = torch.stack([r[0] for r in rows]), torch.stack([r[1] for r in rows])
    return out


def decisive_many_prompts(shape: C.CsmShape):
    """Twelve prompts of mixed lengths and per-utterance frame limits for the continuously refilled batch of 8."""
    spec = [(2100 + i, (8 + 5 * i) % 37 + 4, (17 * i) % 90 + 6, 6 + i % 5, 12 + (7 * i) % 23) for i in range(12)]
    return [(bench_prompt(shape, seed, 1, ct, cf, gt), lim) for seed, ct, cf, gt, lim in spec]


def decisive_golden(shape: C.CsmShape, seed: int, full: bool):
    gold = dict(weight_seed=seed)
    w = C.make_weights(shape, seed=seed, flavour="decisive")
    for tag, wts in (("bf16", w), ("fp8", None)):
        if wts is None:
            wts = C.fp8_dequantized(w)
        if full:
            n1, n32 = 64, 16
            p190 = bench_prompt(shape, 2025)
            p1334 = bench_prompt(shape, 5000, segments=10, ctx_text=30, ctx_frames=100)
            b32 = [bench_prompt(shape, 2025 + b) for b in range(32)]
        else:
            n1, n32 = 24, 8
            p190 = toy_prompt(shape, 11, 6, 5)
            p1334 = toy_prompt(shape, 12, 20, 60)
            b32 = [toy_prompt(shape, 100 + b, 6, 5) for b in range(5)]
        for name, (tok, msk) in (("s190", p190), ("s1334", p1334)):
            g = free_run(shape, wts, tok, msk, n1, f"{tag} {name}")
            want = C.decisive_expected_codes(shape, seed, int(tok[-1, 32]), n1)
            assert torch.equal(g["codes"][:, 0].to(torch.int32), want), "the oracle left the trajectory the construction implies"
            g["prompt_rows"] = tok.shape[0]
            gold[f"{tag}_{name}"] = g
        gold[f"{tag}_b32"] = free_run(shape, wts, torch.stack([p[0] for p in b32]), torch.stack([p[1] for p in b32]), n32, f"{tag} b32")
        if tag == "bf16":
            many = []
            for i, ((tok, msk), lim) in enumerate(decisive_many_prompts(shape)):
                g = free_run(shape, wts, tok, msk, lim, f"{tag} many[{i}] S={tok.shape[0]}")
                many.append(g["codes"][:, 0].clone())
            gold["bf16_many"] = many
    return decisive_finish(gold, w, full)


DECISIVE_CHECKSUM_NAMES = ["text_embeddings.weight", "audio_embeddings.weight", "codebook0_head.weight", "audio_head", "projection.weight",
                           "backbone.layers.7.attn.output_proj.weight", "backbone.layers.15.mlp.w2.weight", "decoder.layers.3.mlp.w2.weight"]


def decisive_finish(gold, w, full: bool):
    """What the golden carries beside the codes: checksums of the re-derived tensors (the GPU test builds the checkpoint with the
    product's own generator and must get the same ones) and, full size, the Mimi oracle's PCM of the first clip -- whole
    (generator.py:299) and as the stateless 10-frame chunks generate_stream yields (generator.py:119-210; every 4th sample kept)."""
    names = [n for n in DECISIVE_CHECKSUM_NAMES if n in w]
    gold["weight_checksum_names"] = names
    gold["weight_checksum"] = torch.stack([w[n].view(torch.int16).to(torch.int64).sum() for n in names])    # exact, order-free
    if full:
        s = M.mimi_full()
        mw = M.make_weights(s, seed=4321)
        codes = gold["bf16_s190"]["codes"][:, 0].long().t().unsqueeze(0)            # (1, 32, T)
        gold["pcm_s190"] = M.decode(s, mw, codes)[0, 0].clone()
        gold["pcm_chunks_stride"] = 4
        gold["pcm_s190_chunks"] = M.decode_stateless_chunks(s, mw, codes, 10)[0, 0][::4].clone()
        # the long prompt's clip too (round 6: it was checked against the HIP codec on the oracle's codes -- HIP vs HIP): every 4th sample
        codes = gold["bf16_s1334"]["codes"][:, 0].long().t().unsqueeze(0)
        gold["pcm_s1334_stride4"] = M.decode(s, mw, codes)[0, 0][::4].clone()
        codes = gold["fp8_s1334"]["codes"][:, 0].long().t().unsqueeze(0)
        gold["pcm_fp8_s1334_stride4"] = M.decode(s, mw, codes)[0, 0][::4].clone()
        gold["mimi_weight_seed"] = 4321
    return gold


# ---- the history-dependent decisive checkpoint ----------------------------------------------------------------------------------
COPY_SHORT = "decisive_copy"            # middle layer, lag 3
COPY_FAULTS = ({"kind": "stale"}, {"kind": "shift_rope", "delta": 1}, {"kind": "zero_prompt"})


def copy_long_flavour(shape: C.CsmShape, rows: int) -> str:
    """the long-prompt variant: an early layer, a lag of about half the prompt (a key in the middle of the key range)."""
    return f"decisive_copy:{min(3, shape.backbone.num_layers - 1)}:{max(4, (rows * 21) // 40)}"


@torch.inference_mode()
def copy_fault_check(shape: C.CsmShape, weights, flavour: str, tok, msk, want, n: int = 8):
    """The point of the flavour: faults in the copy layer's KV cache CHANGE the free-running codes (and the unfaulted run is `want`)."""
    layer, lag = C.copy_flavour_params(shape, flavour)
    S = tok.shape[0]
    # (decode-step faults show once a frame reads a row that a step appended: frame lag + 1 on -- the long-lag variant reads prompt rows only)
    faults = [f for f in COPY_FAULTS if f["kind"] == "zero_prompt" or lag + 1 < n] + [{"kind": "drop_keys", "lo": max(0, S - 1 - lag), "hi": S + n - lag}]
    changed = []
    try:
        for fault in faults:
            C.KV_FAULT = dict(fault, stack="backbone", layer=layer)
            m = C.OracleModel(shape, weights); m.setup_caches(1)
            got = torch.cat(C.generate_codes(m, tok, msk, n * 80, 1.0, 1, greedy=True, max_seq_len=shape.backbone.max_seq_len))
            changed.append(int((got != want[:n]).any(dim=1).sum()))
            assert changed[-1] > 0, f"{flavour}: the fault {fault} in the copy layer's cache does not change the codes"
    finally:
        C.KV_FAULT = None
    print(f"  {flavour}: KV faults {[f['kind'] for f in faults]} change {changed} of the first {n} frames", flush=True)
    return torch.tensor(changed)


def decisive_copy_golden(shape: C.CsmShape, seed: int, full: bool):
    gold = dict(weight_seed=seed)
    if full:
        n1, n32 = 64, 16
        p190 = bench_prompt(shape, 2025)
        p1334 = bench_prompt(shape, 5000, segments=10, ctx_text=30, ctx_frames=100)
        b32 = [bench_prompt(shape, 2025 + b) for b in range(32)]
    else:
        n1, n32 = 24, 8
        p190 = toy_prompt(shape, 11, 6, 5)
        p1334 = toy_prompt(shape, 12, 20, 60)
        b32 = [toy_prompt(shape, 100 + b, 6, 5) for b in range(5)]
    long_flavour = copy_long_flavour(shape, p1334[0].shape[0])
    gold["flavours"] = dict(s190=COPY_SHORT, b32=COPY_SHORT, s1334=long_flavour)
    sums = {}
    for flavour, runs in ((COPY_SHORT, (("s190", p190), ("b32", b32))), (long_flavour, (("s1334", p1334),))):
        layer, lag = C.copy_flavour_params(shape, flavour)
        w = C.make_weights(shape, seed=seed, flavour=flavour)
        names = [n for n in DECISIVE_CHECKSUM_NAMES + [f"backbone.layers.{layer}.attn.{t}_proj.weight" for t in ("q", "k", "v", "output")] if n in w]
        sums[flavour] = (names, torch.stack([w[n].view(torch.int16).to(torch.int64).sum() for n in names]))
        for tag in ("bf16", "fp8"):
            wts = w if tag == "bf16" else C.fp8_dequantized(w)
            for name, prompt in runs:
                if name == "b32":
                    toks, msks = torch.stack([p[0] for p in prompt]), torch.stack([p[1] for p in prompt])
                    g = free_run(shape, wts, toks, msks, n32, f"{flavour} {tag} b32")
                    for b in range(toks.shape[0]):
                        want = C.decisive_copy_expected_codes(shape, seed, toks[b], msks[b], n32, lag)
                        assert torch.equal(g["codes"][:, b].to(torch.int32), want), "the batched oracle left the trajectory the construction implies"
                else:
                    tok, msk = prompt
                    g = free_run(shape, wts, tok, msk, n1, f"{flavour} {tag} {name}")
                    want = C.decisive_copy_expected_codes(shape, seed, tok, msk, n1, lag)
                    assert torch.equal(g["codes"][:, 0].to(torch.int32), want), "the oracle left the trajectory the construction implies"
                    g["prompt_rows"] = tok.shape[0]
                    g["faults_changed"] = copy_fault_check(shape, wts, flavour, tok, msk, want)
                gold[f"{tag}_{name}"] = g
        del w
    gold["weight_checksums"] = sums
    return gold


# ---- the decoder-side copy checkpoint -----------------------------------------------------------------------------------------------
DCOPY = dict(
    full=dict(variants=("decisive_dcopy:0:1", "decisive_dcopy:3:2", "decisive_dcopy:1:7"), fp8=("decisive_dcopy:3:2",),
              batched=("decisive_dcopy:0:1", "decisive_dcopy:1:7"), many=("decisive_dcopy:0:1",), batch=32, cross_frames=2),
    tiny=dict(variants=("decisive_dcopy:0:1", "decisive_dcopy:1:3"), fp8=(), batched=("decisive_dcopy:0:1", "decisive_dcopy:1:3"), many=(),
              batch=5, cross_frames=4),
    frames=8, frames_batched=4)


def dcopy_prompts(shape: C.CsmShape, full: bool):
    """(the B = 1 prompt, the batch's prompts): config 2's 190-row prompt and config 3's 32, or their toy counterparts.  In the batch the
    last text token of utterance b is 5000 + b (tiny: 500 + b): frame 0's first code follows from that token alone, and two of 32 seeded
    tokens name the same code one time in four -- those two utterances would then run the same trajectory."""
    if full:
        one, batch, t0 = bench_prompt(shape, 2025), [bench_prompt(shape, 2025 + b) for b in range(DCOPY["full"]["batch"])], 5000
    else:
        one, batch, t0 = toy_prompt(shape, 11, 6, 5), [toy_prompt(shape, 100 + b, 6, 5) for b in range(DCOPY["tiny"]["batch"])], 500
    for b, (tok, _) in enumerate(batch):
        tok[-1, 32] = t0 + b
    return one, batch


def dcopy_many_prompts(shape: C.CsmShape):
    """decisive_many_prompts' twelve prompts with limits of 3..7 frames: every frame is 31 decoder steps on a cache that starts empty."""
    return [(p, 3 + (7 * i) % 5) for i, (p, _) in enumerate(decisive_many_prompts(shape))]


def dcopy_decoder_faults(shape: C.CsmShape, lag: int):
    """The KV faults of oracle.csm_ref.KV_FAULT for the decoder's cache: `zero_prompt` zeroes what the 2-row first call (positions 0, 1)
    wrote, `drop_keys` hides the positions that are copied from (p - lag for p = lag + 1 .. 31)."""
    return [{"kind": "stale"}, {"kind": "shift_rope", "delta": 1}, {"kind": "shift_rope", "delta": -1}, {"kind": "shift_write", "delta": -1},
            {"kind": "zero_prompt"}, {"kind": "drop_keys", "lo": 1, "hi": shape.audio_num_codebooks - lag}]


def dcopy_backbone_faults(rows: int, n: int):
    return [{"kind": "stale"}, {"kind": "shift_rope", "delta": 1}, {"kind": "shift_write", "delta": -1}, {"kind": "zero_prompt"},
            {"kind": "drop_keys", "lo": rows - 4, "hi": rows + n}]


def fault_name(fault: dict) -> str:
    return fault["kind"] + (f"{fault['delta']:+d}" if "delta" in fault else "")


@torch.inference_mode()
def faulted_frames(model: C.OracleModel, shape: C.CsmShape, tok, msk, want, stack: str, layer: int, faults) -> torch.Tensor:
    """Per fault: how many of the first len(want) free-running frames leave `want` with that fault in (stack, layer)."""
    n = want.shape[0]
    changed = []
    try:
        for fault in faults:
            C.KV_FAULT = dict(fault, stack=stack, layer=layer)
            got = torch.cat(C.generate_codes(model, tok, msk, n * 80, 1.0, 1, greedy=True, max_seq_len=shape.backbone.max_seq_len))
            changed.append(int((got != want).any(dim=1).sum()) if got.shape == want.shape else n)
    finally:
        C.KV_FAULT = None
    return torch.tensor(changed)


def dcopy_fault_matrix(shape: C.CsmShape, weights, flavour: str, tok, msk, want, backbone: bool = True):
    """What the flavour is for, asserted on the oracle: every KV fault in the copy layer of the DECODER changes the free-running codes;
    the same faults in another decoder layer, and KV faults in a backbone layer, change nothing."""
    layer, lag = C.dcopy_flavour_params(shape, flavour)
    other = (layer + 1) % shape.decoder.num_layers
    faults = dcopy_decoder_faults(shape, lag)
    m = C.OracleModel(shape, weights); m.setup_caches(1)
    assert torch.equal(faulted_frames(m, shape, tok, msk, want, "decoder", layer, [{"kind": "none"}]), torch.tensor([0]))
    out = dict(kinds=[fault_name(f) for f in faults], other_layer=other,
               faults_changed=faulted_frames(m, shape, tok, msk, want, "decoder", layer, faults),
               other_layer_changed=faulted_frames(m, shape, tok, msk, want, "decoder", other, faults))
    assert bool((out["faults_changed"] > 0).all()), f"{flavour}: a fault in the copy layer's cache leaves the codes alone: {out}"
    assert not bool(out["other_layer_changed"].any()), f"{flavour}: a fault in decoder layer {other} moves the codes: {out}"
    if backbone:
        bb = shape.backbone.num_layers // 2
        out["backbone_layer"] = bb
        out["backbone_changed"] = faulted_frames(m, shape, tok, msk, want, "backbone", bb, dcopy_backbone_faults(tok.shape[0], want.shape[0]))
        assert not bool(out["backbone_changed"].any()), f"{flavour}: a backbone KV fault moves the codes: {out}"
    print(f"  {flavour}: decoder KV faults {out['kinds']} change {out['faults_changed'].tolist()} of {want.shape[0]} frames in layer {layer}, "
          f"{out['other_layer_changed'].tolist()} in layer {other}" + (f"; backbone faults {out['backbone_changed'].tolist()}" if backbone else ""), flush=True)
    return out


def dcopy_cross_check(shape: C.CsmShape, seed: int, tok, msk, n: int, decoder_layers):
    """The gap this flavour closes: the decoder faults leave the free-running codes of `decisive` and `decisive_copy` as they are."""
    out = {}
    for flavour in ("decisive", "decisive_copy"):
        w = C.make_weights(shape, seed=seed, flavour=flavour)
        m = C.OracleModel(shape, w); m.setup_caches(1)
        want = torch.cat(C.generate_codes(m, tok, msk, n * 80, 1.0, 1, greedy=True, max_seq_len=shape.backbone.max_seq_len))
        assert want.shape[0] == n
        changed = torch.stack([faulted_frames(m, shape, tok, msk, want, "decoder", layer, dcopy_decoder_faults(shape, 2)) for layer in decoder_layers])
        assert not bool(changed.any()), f"{flavour} sees a decoder KV fault: {changed.tolist()}"
        out[flavour] = dict(decoder_layers=list(decoder_layers), changed=changed)
        print(f"  {flavour}: decoder KV faults in layers {list(decoder_layers)} change {changed.tolist()} of {n} frames", flush=True)
        del w, m
    return out


def weight_checksums(w):
    names = sorted(w)
    return names, torch.stack([w[k].view(torch.int16).to(torch.int64).sum() for k in names])       # exact, order-free


def dcopy_expected(shape: C.CsmShape, seed: int, tok, n: int, lag: int) -> torch.Tensor:
    return C.decisive_dcopy_expected_codes(shape, seed, int(tok[-1, 32]), n, lag)


def decisive_dcopy_golden(shape: C.CsmShape, seed: int, full: bool, path: str):
    """Writes `path` after every variant (the CSM-1B oracle runs take a quarter of an hour on 8 CPU threads)."""
    cfg = DCOPY["full" if full else "tiny"]
    n1, nb = DCOPY["frames"], DCOPY["frames_batched"]
    (tok, msk), batch = dcopy_prompts(shape, full)
    btok, bmsk = torch.stack([p[0] for p in batch]), torch.stack([p[1] for p in batch])
    gold = dict(weight_seed=seed, variants=[], prompt_rows=tok.shape[0], weight_checksums={}, runs={})
    layers = sorted({C.dcopy_flavour_params(shape, f)[0] for f in cfg["variants"]}) if not full else [shape.decoder.num_layers - 1]
    gold["cross"] = dcopy_cross_check(shape, seed, tok, msk, cfg["cross_frames"], layers)
    w = C.make_weights(shape, seed=seed)
    base = C.decisive_dcopy_base(shape, w, seed)
    for flavour in cfg["variants"]:
        layer, lag = C.dcopy_flavour_params(shape, flavour)
        wts = C.decisive_dcopy_variant(shape, base, w, seed, layer, lag)
        gold["weight_checksums"][flavour] = weight_checksums(wts)
        runs = {}
        for tag in ("bf16",) + (("fp8",) if flavour in cfg["fp8"] else ()):
            wt = wts if tag == "bf16" else C.fp8_dequantized(wts)
            g = free_run(shape, wt, tok, msk, n1, f"{flavour} {tag} B=1", keep_rows=True)
            want = dcopy_expected(shape, seed, tok, n1, lag)
            assert torch.equal(g["codes"][:, 0].to(torch.int32), want), "the oracle left the trajectory the construction implies"
            g.update(dcopy_fault_matrix(shape, wt, flavour, tok, msk, want, backbone=tag == "bf16"))
            runs[f"{tag}_s190"] = g
        if flavour in cfg["batched"]:
            g = free_run(shape, wts, btok, bmsk, nb, f"{flavour} bf16 B={btok.shape[0]}", keep_rows=True)
            for b in range(btok.shape[0]):
                assert torch.equal(g["codes"][:, b].to(torch.int32), dcopy_expected(shape, seed, btok[b], nb, lag)), "the batched oracle left the implied trajectory"
            first = g["codes"][0]
            assert all(not torch.equal(first[i], first[j]) for i in range(first.shape[0]) for j in range(i)), "two utterances of the batch share a first frame"
            g["prompt_checksum"] = btok.sum(dim=(1, 2))
            runs["bf16_b32"] = g
        if flavour in cfg["many"]:
            many = []
            for i, ((t_, m_), lim) in enumerate(dcopy_many_prompts(shape)):
                g = free_run(shape, wts, t_, m_, lim, f"{flavour} bf16 many[{i}] S={t_.shape[0]}")
                assert torch.equal(g["codes"][:, 0].to(torch.int32), dcopy_expected(shape, seed, t_, lim, lag))
                many.append(dict(codes=g["codes"][:, 0].clone(), min_margin=g["min_margin"], max_gap=g["max_gap"]))
            runs["bf16_many"] = many
        gold["runs"][flavour] = runs
        gold["variants"].append(flavour)
        torch.save(gold, path + ".part")
        os.replace(path + ".part", path)
        del wts
    return gold


# ---- position sweep on the bench checkpoint -------------------------------------------------------------------------------------------
POSSWEEP_S = (63, 64, 65, 511, 512, 766, 767, 768, 769, 775, 1023, 1024, 1535, 2046)
POSSWEEP_PROMPT = dict(seed=7000, segments=15, ctx_text=30, ctx_frames=100, gen_text=81)          # 15 x 131 + 81 = 2046 rows
CONSEC_S, CONSEC_FRAMES = 740, 64


def possweep_prompt(shape: C.CsmShape):
    a = POSSWEEP_PROMPT
    return bench_prompt(shape, a["seed"], a["segments"], a["ctx_text"], a["ctx_frames"], a["gen_text"])


@torch.inference_mode()
def possweep_golden(shape: C.CsmShape, weights, sizes, consec_s: int, consec_frames: int):
    """For each S: the first S rows of the prompt prefilled in one call (the reference's way: generator.py:283 with the whole prompt),
    the prompt frame, then two teacher-forced steps -- greedy, fed the bf16 oracle's own codes -- at positions S and S + 1 (one step when
    S + 1 is the last position).  Per (S, frame): codes [32], top-8 logits, margin [32], bf16-vs-fp32 gap [32]."""
    tok, msk = possweep_prompt(shape)
    assert tok.shape[0] == 2046
    w32 = {k: v.float() for k, v in weights.items()}
    out = dict(sizes=torch.tensor(sizes), per_size=[])
    for S in list(sizes) + [None]:
        t0 = time.time()
        n_frames = 3 if S is not None else consec_frames + 1
        S_ = S if S is not None else consec_s
        n_frames = min(n_frames, shape.backbone.max_seq_len - S_ + 1)
        g = frames_golden(shape, weights, (tok[:S_], msk[:S_]), n_frames, keep_full=False, with_fp32=True, quiet=True, w32=w32)
        del g["prompt_tokens"], g["prompt_mask"]
        g["rows"] = S_
        print(f"  possweep S={S_}: {n_frames} frames in {time.time() - t0:.0f}s, max gap {float(g['bf16_vs_fp32_gap'].max()):.4f}, "
              f"rows with margin < gap/2: {int((g['margin'] < 0.5 * g['bf16_vs_fp32_gap'].max()).sum())} of {g['margin'].numel()}", flush=True)
        if S is None:
            out["consecutive"] = g
        else:
            out["per_size"].append(g)
    return out


# ---- norm-test checkpoints (RMSNorm scales != 1) ---------------------------------------------------------------------------------------
NORMS_PROMPTS = dict(cfg2=dict(seed=2025), cfg5=dict(seed=5000, segments=10, ctx_text=30, ctx_frames=100))     # config 2 (S = 190), config 5 (S = 1334)
NORMS_LEGS = (          # leg, checkpoint, weights, prompt, teacher-forced frames
    ("A", "jitter", "bf16", "cfg2", 4),
    ("B", "jitter", "fp8", "cfg2", 4),
    ("C", "jitter", "bf16", "cfg5", 2),
    ("D", "jitter", "fp8", "cfg5", 2),
    ("E", "outlier", "bf16", "cfg2", 4),
    ("F", "outlier", "fp8", "cfg2", 2),
)
NORMS_FAULT_LEGS = ("A", "E")
NORMS_FAULT_MIN = 1.5   # a stored fault moves the logits by at least this many x its leg's gap
NORMS_SEED = 1234


def norms_prompt(shape: C.CsmShape, name: str):
    return bench_prompt(shape, **NORMS_PROMPTS[name])


@torch.inference_mode()
def norm_fault_delta(shape: C.CsmShape, weights, gold, tok, msk, fault: str) -> torch.Tensor:
    """Frame 0, teacher-forced on the golden codes, with a scale fault edited into the weights: max |dlogit| at the golden's top-8
    indices against the golden's top-8 values -- the statistic the GPU test asserts on."""
    m = C.OracleModel(shape, C.norm_fault_weights(shape, weights, fault))
    m.setup_caches(1)
    tr = C.FrameTrace()
    m.generate_frame(tok.unsqueeze(0), msk.unsqueeze(0), torch.arange(tok.shape[0]).unsqueeze(0), 1.0, 1, greedy=True,
                     forced=gold["codes"][0].unsqueeze(0), trace=tr)
    lg = torch.stack(tr.logits, 0)[:, 0].float()
    return (torch.gather(lg, 1, gold["top_i"][0].long()) - gold["top_v"][0].float()).abs().max()


def norms_golden(shape: C.CsmShape):
    """Legs A-F (NORMS_LEGS) in frames_golden's layout, and for legs A and E the four scale faults of C.NORM_FAULTS on frame 0.
    Every fault kept moves the logits by >= NORMS_FAULT_MIN x the leg's gap; the piece permutation must clear it on A or on E."""
    gold = dict(weight_seed=NORMS_SEED, prompts={k: dict(v) for k, v in NORMS_PROMPTS.items()}, prompt_checksum={}, legs={})
    prompts = {k: norms_prompt(shape, k) for k in NORMS_PROMPTS}
    for k, (tok, msk) in prompts.items():
        gold["prompt_checksum"][k] = torch.stack([tok.sum(), msk.sum(), torch.tensor(tok.shape[0])])
    for variant in ("jitter", "outlier"):
        w = C.norm_test_weights(shape, seed=NORMS_SEED, outliers=variant == "outlier")
        w8 = None
        for leg, v, dtype, pname, n in NORMS_LEGS:
            if v != variant:
                continue
            t0 = time.time()
            if dtype == "fp8" and w8 is None:
                w8 = C.fp8_dequantized(w)
            wts = w8 if dtype == "fp8" else w
            tok, msk = prompts[pname]
            g = frames_golden(shape, wts, (tok, msk), n, keep_full=False, with_fp32=True, quiet=True)
            del g["prompt_tokens"], g["prompt_mask"]
            g.update(checkpoint=v, weights=dtype, prompt=pname, rows=tok.shape[0])
            if dtype == "fp8":
                g["deq_checksum"] = torch.stack([w8["backbone.layers.3.mlp.w2.weight"].float().abs().sum(),
                                                 w8["decoder.layers.1.attn.q_proj.weight"].float().abs().sum(), w8["audio_head"].float().abs().sum()])
            gap = float(g["bf16_vs_fp32_gap"].max())
            msg = f"  leg {leg} ({v}, {dtype}, S={tok.shape[0]}, {n} frames): gap {gap:.4f}"
            if leg in NORMS_FAULT_LEGS:
                faults = {f: norm_fault_delta(shape, wts, g, tok, msk, f) for f in C.NORM_FAULTS}
                msg += "; faults " + ", ".join(f"{f} {float(d):.3f} ({float(d) / gap:.1f} x)" for f, d in faults.items())
                g["faults"] = {f: d for f, d in faults.items() if float(d) >= NORMS_FAULT_MIN * gap}
            print(msg + f"  [{time.time() - t0:.0f}s]", flush=True)
            gold["legs"][leg] = g
        del w, w8
    for leg in NORMS_FAULT_LEGS:
        kept = gold["legs"][leg]["faults"]
        assert leg != "A" or all(f in kept for f in C.NORM_FAULTS if f != "bb7_sa_pieces"), f"leg A: a scale fault is within {NORMS_FAULT_MIN} x gap"
    assert any("bb7_sa_pieces" in gold["legs"][leg]["faults"] for leg in NORMS_FAULT_LEGS), "the piece permutation clears 1.5 x gap on neither leg A nor E"
    return gold


# ---- full-size Mimi at real clip lengths ----------------------------------------------------------------------------------------------
MIMI_LONG = dict(
    weight_seed=4321,
    decode=((126, 9126), (150, 9150), (300, 9300), (1125, 91125)),              # (frames, code seed): 252 / 300 / 600 / 2250 transformer tokens
    encode=((1920 * 126 + 777, 7126), (1920 * 260 + 5, 7260)),                  # (samples, wav seed): a 5 s and a 10.4 s voice prompt
    stride=16, window=2048, last_frames=10,
    bound=2e-5,                 # of the clip's peak: what tests/test_mimi_long_gpu.py allows between the HIP codec and these vectors
    fault_factor=10.0,          # an injected fault moves the compared samples by at least this many bounds
    pool_ring=270,              # tr_context + 2 * max_chunk_frames of open_streams(n, max_chunk_frames=10)
    tie_nudge=1e-6, tie_unchanged_min=0.97, enc_changed_min=0.10,
    # graded against the live oracle by the GPU test (no golden): a batch of two prompts, and lengths around one hop
    encode_b2=(1920 * 40 + 300, 7340), encode_edges=((1919, 7301), (1920, 7302), (1921, 7303), (9600, 7304)),
    longest_oracle_seconds=9.9)     # M.decode of the 1125-frame clip, 8 CPU threads, measured when the fixture was first generated
MIMI_LONG_FAULTS = (("ctx249", dict(context=249)), ("ctx251", dict(context=251)), ("nowindow", dict(context=M.NO_WINDOW)),
                    ("rope_mod_ring", dict(rope_mod=270)))


def mimi_long_codes(seed: int, frames: int, rows: int = 1) -> torch.Tensor:
    return torch.randint(0, 2048, (rows, 32, frames), generator=torch.Generator().manual_seed(seed))


def mimi_long_wav(seed: int, samples: int, rows: int = 1) -> torch.Tensor:
    return torch.randn(rows, 1, samples, generator=torch.Generator().manual_seed(seed)) * 0.3


def mimi_long_views(pcm: torch.Tensor):
    """The samples of a clip (.., hop * T) that the fixture keeps and the GPU test compares: name -> view."""
    a = MIMI_LONG
    s16 = pcm[..., ::a["stride"]]
    return dict(stride16=s16, head=pcm[..., :a["window"]], tail=pcm[..., -a["window"]:],
                last_stride16=s16[..., -a["last_frames"] * 1920 // a["stride"]:])


def mimi_long_fault_applies(fault: str, tokens: int) -> bool:
    """Does the fault change anything a clip of this many transformer tokens computes?"""
    kw = dict(MIMI_LONG_FAULTS)[fault]
    if "rope_mod" in kw:
        return tokens > kw["rope_mod"]
    return tokens > 250          # some query's window starts above 0: the last key of a 251-token window / the first of a 250-token one exists


def mimi_long_move(got: torch.Tensor, want: torch.Tensor) -> float:
    """max over the compared views of max|got - want| / the view's peak: the statistic the GPU test bounds per view."""
    g, w = mimi_long_views(got), mimi_long_views(want)
    return max(float((g[k] - w[k]).abs().max() / w[k].abs().max()) for k in w)


def mimi_long_tie_unchanged(s, w, z: torch.Tensor, codes: torch.Tensor, seed: int) -> float:
    """Share of frames whose 32 codes all survive a nudge of the latent by tie_nudge x its peak (seeded noise)."""
    noise = torch.randn(z.shape, generator=torch.Generator().manual_seed(seed + 1))
    return float((M.quantize(s, w, z + MIMI_LONG["tie_nudge"] * z.abs().max() * noise) == codes).all(dim=1).float().mean())


def mimi_long_golden():
    a = MIMI_LONG
    s = M.mimi_full()
    w = M.make_weights(s, seed=a["weight_seed"], encoder=True)
    need = a["fault_factor"] * a["bound"]
    gold = dict(weight_seed=a["weight_seed"], bound=a["bound"], fault_factor=a["fault_factor"], pool_ring=a["pool_ring"],
                stride=a["stride"], window=a["window"], longest_oracle_seconds=a["longest_oracle_seconds"], decode=[], encode=[])
    for frames, seed in a["decode"]:
        codes = mimi_long_codes(seed, frames)
        t0 = time.time()
        pcm = M.decode(s, w, codes)
        secs = time.time() - t0
        v = mimi_long_views(pcm)
        moves = {}
        for fault, kw in MIMI_LONG_FAULTS:
            moves[fault] = mimi_long_move(M.decode(s, w, codes, **kw), pcm) if mimi_long_fault_applies(fault, 2 * frames) else 0.0
            assert not mimi_long_fault_applies(fault, 2 * frames) or moves[fault] >= need, \
                f"{frames} frames: the fault {fault} moves the compared samples by {moves[fault]:.3g} of peak < {need:.3g}"
        print(f"  mimi_long decode {frames} frames: oracle {secs:.1f}s, peak {float(pcm.abs().max()):.3g}, fault moves (of peak) "
              + ", ".join(f"{k} {x:.3g}" for k, x in moves.items()), flush=True)
        gold["decode"].append(dict(frames=frames, code_seed=seed, code_checksum=int((codes[0] * torch.arange(1, frames + 1)).sum()),
                                   pcm_stride16=v["stride16"].clone(), pcm_head=v["head"].clone(), pcm_tail=v["tail"].clone(),
                                   fault_moves=moves))
    for samples, seed in a["encode"]:
        wav = mimi_long_wav(seed, samples)
        t0 = time.time()
        z = M.encode_latent(s, w, wav)
        codes = M.quantize(s, w, z)
        secs = time.time() - t0
        T = codes.shape[-1]
        past = torch.arange(T) >= 125                   # frames whose last token (2t + 1) has a window that starts above 0
        changed = {}
        for fault, kw in MIMI_LONG_FAULTS[:3]:
            diff = (M.encode(s, w, wav, **kw) != codes).any(dim=1)[0]
            assert not bool(diff[:124].any()), "a window fault reached frames whose windows all start at 0"
            changed[fault] = int(diff.sum())
        unchanged = mimi_long_tie_unchanged(s, w, z, codes, seed)
        assert unchanged >= a["tie_unchanged_min"], f"{samples} samples: only {unchanged:.3f} of the frames survive a {a['tie_nudge']} nudge"
        print(f"  mimi_long encode {samples} samples ({T} frames, {int(past.sum())} past the window): oracle {secs:.1f}s, frames changed "
              + ", ".join(f"{k} {x}" for k, x in changed.items()) + f", unchanged under the nudge {unchanged:.3f}", flush=True)
        gold["encode"].append(dict(samples=samples, wav_seed=seed, wav_checksum=float(wav.double().abs().sum()), codes=codes.to(torch.int16),
                                   frames_past_window=int(past.sum()), frames_changed=changed, tie_unchanged=unchanged))
    mimi_long_check_encode_faults(gold["encode"])
    return gold


def mimi_long_check_encode_faults(enc) -> None:
    """Every window fault changes the codes of >= enc_changed_min of the frames past the window: over the prompts together, and on its
    own in every prompt that has at least 1 / enc_changed_min such frames (the 5 s prompt has 2: 254 tokens against a window of 250)."""
    need = MIMI_LONG["enc_changed_min"]
    for fault, _ in MIMI_LONG_FAULTS[:3]:
        total, past = sum(e["frames_changed"][fault] for e in enc), sum(e["frames_past_window"] for e in enc)
        assert total >= need * past, f"the fault {fault} changes {total} of the {past} frames past the window"
        for e in enc:
            if e["frames_past_window"] * need >= 1:
                assert e["frames_changed"][fault] >= need * e["frames_past_window"], \
                    f"{e['samples']} samples: the fault {fault} changes {e['frames_changed'][fault]} of the {e['frames_past_window']} frames past the window"


def sampler_cases():
    g = torch.Generator().manual_seed(77)
    V = 2051
    logits = (torch.randn(48, V, generator=g) * 3).to(torch.bfloat16)
    logits[3, 100:160] = logits[3].max()                       # a 60-way tie at the top
    logits[4, :] = 0.5                                         # all equal
    logits[5, 7] = 40.0                                        # one dominant logit
    kth = torch.topk(logits[6].float(), 50)[0][-1]
    logits[6, 2000:2010] = kth.to(torch.bfloat16)              # ties exactly at the kth value
    cases = []
    for (T, k) in ((0.9, 50), (0.7, 30), (1.0, 2051), (0.8, 1), (1.3, 5)):
        q = torch.empty(48, V, dtype=torch.bfloat16).exponential_(1, generator=g)
        out = C.sample_topk(logits, k, T, q=q, greedy_lowest_index=(k == 1))
        cases.append(dict(temperature=T, topk=k, noise=q, out=out[:, 0].clone()))
    return dict(logits=logits, cases=cases)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--frames", type=int, default=12)
    a = ap.parse_args()
    os.makedirs(OUT, exist_ok=True)
    want = lambda n: (not a.only) or (n in a.only.split(","))

    if want("prompt"):
        shape = C.csm_tiny()
        tok, msk = toy_prompt(shape, 5, 4, 3)
        torch.save(dict(tokens=tok, mask=msk, seed=5, n_text=4, ctx_frames=3), os.path.join(OUT, "prompt_layout.pt"))
    if want("sampler"):
        torch.save(sampler_cases(), os.path.join(OUT, "sampler_cases.pt"))
    if want("tiny"):
        shape = C.csm_tiny()
        w = C.make_weights(shape, seed=1234)
        gold = frames_golden(shape, w, toy_prompt(shape, 11, 6, 5), 6, keep_full=True, with_fp32=True)
        gold.update(weight_seed=1234, prompt_seed=11)
        torch.save(gold, os.path.join(OUT, "tiny_frames.pt"))
    if want("mimi"):
        for name, s in (("tiny", M.mimi_tiny()), ("full", M.mimi_full())):
            w = M.make_weights(s, seed=4321)
            codes = torch.randint(0, s.codebook_size, (1, 32, 10 if name == "full" else 23),
                                  generator=torch.Generator().manual_seed(9))
            whole = M.decode(s, w, codes)
            chunks = M.decode_stateless_chunks(s, w, codes, 10)
            # keep every 16th sample of the full-size clip + exact head/tail windows (small file)
            torch.save(dict(codes=codes, weight_seed=4321, pcm=whole if name == "tiny" else None,
                            pcm_stride16=whole[..., ::16].clone(), pcm_head=whole[..., :4096].clone(),
                            pcm_tail=whole[..., -4096:].clone(),
                            chunks_stride16=chunks[..., ::16].clone(),
                            rms=whole.pow(2).mean().sqrt()), os.path.join(OUT, f"mimi_{name}.pt"))
    if want("mimilong"):
        torch.save(mimi_long_golden(), os.path.join(OUT, "mimi_long.pt"))
    if want("tinydecisive"):
        torch.save(decisive_golden(C.csm_tiny(), 1234, full=False), os.path.join(OUT, "tiny_decisive.pt"))
    if want("decisive"):
        torch.save(decisive_golden(C.csm_1b(), 1234, full=True), os.path.join(OUT, "csm1b_decisive.pt"))
    if want("tinycopy"):
        torch.save(decisive_copy_golden(C.csm_tiny(), 1234, full=False), os.path.join(OUT, "tiny_decisive_copy.pt"))
    if want("copy"):
        torch.save(decisive_copy_golden(C.csm_1b(), 1234, full=True), os.path.join(OUT, "csm1b_decisive_copy.pt"))
    if want("dcopy") or a.only == "dcopytiny":      # "dcopytiny" / "dcopyfull": one of the two files alone
        decisive_dcopy_golden(C.csm_tiny(), 1234, False, os.path.join(OUT, "tiny_decisive_dcopy.pt"))
    if want("dcopy") or a.only == "dcopyfull":
        decisive_dcopy_golden(C.csm_1b(), 1234, True, os.path.join(OUT, "csm1b_decisive_dcopy.pt"))
    if a.only == "copyx":
        # more copy layers / lags on the 190-row prompt, added to the existing file: the FIRST layer with lag 1 (layer 0 normalises the embedding
        # sum itself; lag 1 reads the row the immediately preceding frame step appended -- from frame 2 on) and the LAST layer with lag 7 (its
        # finisher applies the stack's final norm)
        shape = C.csm_1b()
        path = os.path.join(OUT, "csm1b_decisive_copy.pt")
        gold = torch.load(path)
        seed = int(gold["weight_seed"])
        tok, msk = bench_prompt(shape, 2025)
        for name, flavour in (("s190_first", "decisive_copy:0:1"), ("s190_last", f"decisive_copy:{shape.backbone.num_layers - 1}:7")):
            layer, lag = C.copy_flavour_params(shape, flavour)
            w = C.make_weights(shape, seed=seed, flavour=flavour)
            names = [n for n in DECISIVE_CHECKSUM_NAMES + [f"backbone.layers.{layer}.attn.{t}_proj.weight" for t in ("q", "k", "v", "output")] if n in w]
            gold["weight_checksums"][flavour] = (names, torch.stack([w[n].view(torch.int16).to(torch.int64).sum() for n in names]))
            gold["flavours"][name] = flavour
            for tag in ("bf16", "fp8"):
                wts = w if tag == "bf16" else C.fp8_dequantized(w)
                g = free_run(shape, wts, tok, msk, 32, f"{flavour} {tag} {name}")
                want_codes = C.decisive_copy_expected_codes(shape, seed, tok, msk, 32, lag)
                assert torch.equal(g["codes"][:, 0].to(torch.int32), want_codes), "the oracle left the trajectory the construction implies"
                g["prompt_rows"] = tok.shape[0]
                g["faults_changed"] = copy_fault_check(shape, wts, flavour, tok, msk, want_codes, n=max(8, lag + 5))
                gold[f"{tag}_{name}"] = g
            del w
        torch.save(gold, path)
    if a.only == "copymany":
        # the twelve utterances of the continuously refilled batch of 8 (decisive_many_prompts) on the copy checkpoint: a refill writes a prompt's K/V
        # into ONE slot of a live batch, and every slot then steps at its own position -- what the free-running codes read back
        shape = C.csm_1b()
        path = os.path.join(OUT, "csm1b_decisive_copy.pt")
        gold = torch.load(path)
        seed = int(gold["weight_seed"])
        _, lag = C.copy_flavour_params(shape, COPY_SHORT)
        w = C.make_weights(shape, seed=seed, flavour=COPY_SHORT)
        many = []
        for i, ((tok, msk), lim) in enumerate(decisive_many_prompts(shape)):
            g = free_run(shape, w, tok, msk, lim, f"{COPY_SHORT} bf16 many[{i}] S={tok.shape[0]}")
            assert torch.equal(g["codes"][:, 0].to(torch.int32), C.decisive_copy_expected_codes(shape, seed, tok, msk, lim, lag))
            many.append(g["codes"][:, 0].clone())
        gold["bf16_many"] = many
        torch.save(gold, path)
    if a.only == "cfg4":
        # BASELINE config 4 = batch 256 sharded over 8 GPUs: 32 utterances per rank, rank r's prompts are bench.py's seeds 4000 + 32 r .. (batch32_leg).
        # No 8-GPU node has been available to this build; what CAN be checked on one GPU is that a shard -- here the LAST rank's, seeds 4224..4255 --
        # computes what the batched oracle computes for those prompts: top-8 logits / codes / margins of 2 teacher-forced frames + the bf16-vs-fp32 gap.
        shape = C.csm_1b()
        w = C.make_weights(shape, seed=1234)
        rank, seed0 = 7, 4000 + 32 * 7
        ps = [bench_prompt(shape, seed0 + b) for b in range(32)]
        toks, msks = torch.stack([p[0] for p in ps]), torch.stack([p[1] for p in ps])
        gold = frames_golden_batch(shape, w, toks, msks, 2)
        B = 32
        gaps = []
        with torch.inference_mode():
            m32 = C.OracleModel(shape, {k: v.float() for k, v in w.items()}, dtype=torch.float32); m32.setup_caches(B)
            cur_t, cur_m = toks, msks
            pos = torch.arange(toks.size(1)).unsqueeze(0).repeat(B, 1)
            mb = C.OracleModel(shape, w); mb.setup_caches(B)
            for f in range(2):
                tr, tr32 = C.FrameTrace(), C.FrameTrace()
                s_ = mb.generate_frame(cur_t, cur_m, pos, 1.0, 1, greedy=True, trace=tr)
                assert torch.equal(s_, gold["codes"][f])
                m32.generate_frame(cur_t, cur_m, pos, 1.0, 1, greedy=True, forced=s_, trace=tr32)
                gaps.append((torch.stack(tr.logits, 0).float() - torch.stack(tr32.logits, 0)).abs().max(dim=-1)[0])
                cur_t = torch.cat([s_.long(), torch.zeros(B, 1).long()], dim=1).unsqueeze(1)
                cur_m = torch.cat([torch.ones_like(s_).bool(), torch.zeros(B, 1).bool()], dim=1).unsqueeze(1)
                pos = pos[:, -1:] + 1
        gold["bf16_vs_fp32_gap"] = torch.stack(gaps)
        gold.update(weight_seed=1234, rank=rank, prompt_seed=seed0, prompt_checksum=gold["prompt_tokens"].sum(dim=(1, 2)))
        del gold["prompt_tokens"], gold["prompt_mask"]
        torch.save(gold, os.path.join(OUT, "csm1b_cfg4_rank7.pt"))
    if want("possweep"):
        shape = C.csm_1b()
        w = C.make_weights(shape, seed=1234)
        gold = dict(weight_seed=1234, prompt=dict(POSSWEEP_PROMPT), consec_rows=CONSEC_S)
        gold["bf16"] = possweep_golden(shape, w, POSSWEEP_S, CONSEC_S, CONSEC_FRAMES)
        torch.save(gold, os.path.join(OUT, "csm1b_possweep.pt"))                 # (kept if the fp8 half is interrupted)
        gold["fp8"] = possweep_golden(shape, C.fp8_dequantized(w), POSSWEEP_S, CONSEC_S, CONSEC_FRAMES)
        torch.save(gold, os.path.join(OUT, "csm1b_possweep.pt"))
        del w
    if want("norms"):
        torch.save(norms_golden(C.csm_1b()), os.path.join(OUT, "csm1b_norms.pt"))
    if a.only == "decisivefinish":          # re-derive the checksums / PCM of existing files without re-running the trajectories
        for fname, shape, full in (("tiny_decisive.pt", C.csm_tiny(), False), ("csm1b_decisive.pt", C.csm_1b(), True)):
            path = os.path.join(OUT, fname)
            gold = torch.load(path)
            torch.save(decisive_finish(gold, C.make_weights(shape, seed=int(gold["weight_seed"]), flavour="decisive"), full), path)
    if want("csm1b"):
        shape = C.csm_1b()
        t0 = time.time()
        w = C.make_weights(shape, seed=1234)
        print(f"weights: {time.time() - t0:.0f}s", flush=True)
        gold = frames_golden(shape, w, toy_prompt(shape, 2025, 16, 0), a.frames, keep_full=False, with_fp32=True)
        gold.update(weight_seed=1234, prompt_seed=2025)
        torch.save(gold, os.path.join(OUT, "csm1b_frames.pt"))
    for name, fname, fp8 in (("cfg3gap", "csm1b_cfg3.pt", False), ("cfg5cgap", "csm1b_cfg5c.pt", True)):
        if not want(name):
            continue
        # The oracle's own bf16-vs-fp32 logit gap ON THE ROWS OF A BATCHED GOLDEN (32 utterances x 32 codebooks x 2 frames): the gap stored
        # with config 2 / config 5 is a maximum over 192 / 64 rows of ONE utterance, the batched tests compare 2,048 rows -- a maximum over
        # ten times the samples (round 4: tests/test_frame_gpu.py holds the B = 32 paths to 1x THIS gap).  Added to the existing file; its
        # codes must be reproduced on this host.
        shape = C.csm_1b()
        w = C.make_weights(shape, seed=1234)
        if fp8:
            w = C.fp8_dequantized(w)
        path = os.path.join(OUT, fname)
        gold = torch.load(path)
        if "prompt_tokens" in gold:
            toks, msks = gold["prompt_tokens"].long(), gold["prompt_mask"]
        else:
            ps = [bench_prompt(shape, int(gold["prompt_seed"]) + b, segments=10, ctx_text=30, ctx_frames=100) for b in range(gold["codes"].shape[1])]
            toks, msks = torch.stack([p[0] for p in ps]), torch.stack([p[1] for p in ps])
        B = toks.shape[0]
        gaps = []
        with torch.inference_mode():
            mb = C.OracleModel(shape, w); mb.setup_caches(B)
            m32 = C.OracleModel(shape, {k: v.float() for k, v in w.items()}, dtype=torch.float32); m32.setup_caches(B)
            cur_t, cur_m = toks, msks
            pos = torch.arange(toks.size(1)).unsqueeze(0).repeat(B, 1)
            for f in range(gold["codes"].shape[0]):
                t0 = time.time()
                tr, tr32 = C.FrameTrace(), C.FrameTrace()
                s = mb.generate_frame(cur_t, cur_m, pos, 1.0, 1, greedy=True, trace=tr)
                assert torch.equal(s, gold["codes"][f]), "the stored trajectory is not reproduced on this host"
                m32.generate_frame(cur_t, cur_m, pos, 1.0, 1, greedy=True, forced=s, trace=tr32)
                lg, lg32 = torch.stack(tr.logits, 0).float(), torch.stack(tr32.logits, 0)
                gaps.append((lg - lg32).abs().max(dim=-1)[0])               # [32 codebooks][B]
                cur_t = torch.cat([s.long(), torch.zeros(B, 1).long()], dim=1).unsqueeze(1)
                cur_m = torch.cat([torch.ones_like(s).bool(), torch.zeros(B, 1).bool()], dim=1).unsqueeze(1)
                pos = pos[:, -1:] + 1
                print(f"  {name} frame {f}: {time.time() - t0:.1f}s max {float(gaps[-1].max()):.4f}", flush=True)
        gold["bf16_vs_fp32_gap"] = torch.stack(gaps)
        torch.save(gold, path)
        del w, mb, m32
    if want("cfg2") or want("cfg3") or want("cfg5") or want("cfg5b") or want("cfg5c"):
        shape = C.csm_1b()
        w = C.make_weights(shape, seed=1234)
        if want("cfg2"):
            gold = frames_golden(shape, w, bench_prompt(shape, 2025), 6, keep_full=False, with_fp32=True)
            gold.update(weight_seed=1234, prompt_seed=2025)
            torch.save(gold, os.path.join(OUT, "csm1b_cfg2.pt"))
        if want("cfg3"):
            ps = [bench_prompt(shape, 2025 + b) for b in range(32)]
            gold = frames_golden_batch(shape, w, torch.stack([p[0] for p in ps]), torch.stack([p[1] for p in ps]), 2)
            gold.update(weight_seed=1234, prompt_seed=2025)
            gold["prompt_tokens"] = gold["prompt_tokens"].to(torch.int32)
            torch.save(gold, os.path.join(OUT, "csm1b_cfg3.pt"))
        if want("cfg5"):
            w8 = C.fp8_dequantized(w)
            del w
            g5 = frames_golden(shape, w8, bench_prompt(shape, 5000, segments=10, ctx_text=30, ctx_frames=100), 2, keep_full=False, with_fp32=True)
            tok, msk = bench_prompt(shape, 5001, segments=12, ctx_text=30, ctx_frames=100, gen_text=128)      # 12 x 131 + 128 = 1700 rows
            gl = frames_golden(shape, w8, (tok, msk), 2, keep_full=False, with_fp32=True)
            gold = dict(weight_seed=1234, s1334=g5, s1700=gl,
                        deq_checksum=torch.stack([w8["backbone.layers.3.mlp.w2.weight"].float().abs().sum(),
                                                  w8["decoder.layers.1.attn.q_proj.weight"].float().abs().sum(),
                                                  w8["audio_head"].float().abs().sum()]))
            for d in (g5, gl):
                d["prompt_tokens"] = d["prompt_tokens"].to(torch.int32)
            torch.save(gold, os.path.join(OUT, "csm1b_cfg5.pt"))
        if want("cfg5b"):
            # BASELINE config 5, batched (SURVEY.md 8d lists B = 32; B = 4 keeps the fixture small): 4 different 1334-row prompts,
            # fp8-dequantised weights, 2 teacher-forced frames of the BATCHED oracle
            w8 = C.fp8_dequantized(w)
            ps = [bench_prompt(shape, 6000 + b, segments=10, ctx_text=30, ctx_frames=100) for b in range(4)]
            gold = frames_golden_batch(shape, w8, torch.stack([p[0] for p in ps]), torch.stack([p[1] for p in ps]), 2)
            gold.update(weight_seed=1234, prompt_seed=6000)
            gold["prompt_tokens"] = gold["prompt_tokens"].to(torch.int32)
            torch.save(gold, os.path.join(OUT, "csm1b_cfg5b.pt"))
        if want("cfg5c"):
            # BASELINE config 5 at the batch SURVEY.md 8d lists for it: B = 32 x the 1334-row prompt (bench.py's config5_b32 leg: seeds
            # 6000..6031), fp8-dequantised weights, 2 teacher-forced frames of the batched oracle.  Only the top-8 logits, the codes and
            # the margins are kept (the prompts are a function of the seeds: the test rebuilds them with bench.synthetic_prompt).
            w8 = C.fp8_dequantized(w)
            ps = [bench_prompt(shape, 6000 + b, segments=10, ctx_text=30, ctx_frames=100) for b in range(32)]
            gold = frames_golden_batch(shape, w8, torch.stack([p[0] for p in ps]), torch.stack([p[1] for p in ps]), 2)
            gold.update(weight_seed=1234, prompt_seed=6000, prompt_checksum=gold["prompt_tokens"].sum(dim=(1, 2)))
            del gold["prompt_tokens"], gold["prompt_mask"]
            torch.save(gold, os.path.join(OUT, "csm1b_cfg5c.pt"))


if __name__ == "__main__":
    main()
