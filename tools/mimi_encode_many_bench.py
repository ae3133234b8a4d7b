#!/usr/bin/env python3
"""Ragged Mimi encode on an MI355X: one mimi_encode_many call for N clips of different lengths against the way the same work was done
before it existed -- N mimi_encode calls, one launch chain per clip -- and what that does to building the prompts of a full batch.

Full-size codec (synthetic weights), N = 1, 2, 4, 8, 32 clips of 1 .. 6 s (seeded lengths, not multiples of the hop).  Times are GPU
times between HIP events on the launching stream, per round (one ragged call / N single calls), medians; the two ways alternate round
by round in one process, after warm-up rounds of both, on wavs already on the device (the C ABI alone: no packing, no int64 copy).
Before timing, the ragged codes are compared with the single encodes' (bit-identical).  The break-even N is the smallest N at which the
ragged call's median is below the N single calls': it becomes sesameai/generator.py's ENCODE_MANY_MIN_CLIPS.

Prompt building: wall time (host clock around a synchronised call) of Generator._build_prompts for 64 requests x 4 audio segments of
1 .. 6 s, every tensor distinct, through the ragged path and through today's per-segment encode calls.

    python tools/mimi_encode_many_bench.py --out profiles/encode_many/encode_many.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "sesameai-tts_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def lengths(n, seed):
    g = torch.Generator().manual_seed(seed)
    return [int(x) for x in torch.randint(24000, 6 * 24000 + 1, (n,), generator=g)]


def ragged_vs_singles(codec, N, rounds, warmup):
    from sesameai._abi import check, lib
    dev, hop, K = codec.device, codec.args.hop, codec.args.num_codebooks
    lens = lengths(N, 500 + N)
    g = torch.Generator().manual_seed(900 + N)
    packed = (torch.randn(sum(lens), generator=g) * 0.3).to(dev)
    offs = [sum(lens[:k]) for k in range(N)]
    frames = [-(-n // hop) for n in lens]
    F = sum(frames)
    assert F <= codec.max_frames
    many = torch.empty(K, F, dtype=torch.int32, device=dev)
    single = [torch.empty(1, K, f, dtype=torch.int32, device=dev) for f in frames]
    c_offs, c_lens = (C.c_long * N)(*offs), (C.c_long * N)(*lens)
    st = lambda: torch.cuda.current_stream().cuda_stream

    def run_many():
        check(lib.mimi_encode_many(codec._h, packed.data_ptr(), c_offs, c_lens, N, many.data_ptr(), st()), codec._h, mimi=True)

    def run_singles():
        for i in range(N):
            check(lib.mimi_encode(codec._h, packed.data_ptr() + 4 * offs[i], lens[i], 0, 1, single[i].data_ptr(), st()), codec._h, mimi=True)

    run_many(); run_singles()
    torch.cuda.synchronize()
    same = all(torch.equal(m, s[0]) for m, s in zip(many.split(frames, dim=1), single))
    t_many, t_single = [], []
    for r in range(warmup + rounds):
        a, b = timed(run_many), timed(run_singles)
        if r >= warmup:
            t_many.append(a); t_single.append(b)
    med_m, med_s = statistics.median(t_many), statistics.median(t_single)
    return dict(n=N, samples=lens, frames=F, bit_identical=same, ragged_ms=round(med_m, 4), singles_ms=round(med_s, 4),
                ragged_min_ms=round(min(t_many), 4), singles_min_ms=round(min(t_single), 4), speedup=round(med_s / med_m, 3), rounds=rounds)


def prompt_building(codec, requests, segs, rounds):
    from sesameai import generator as G
    from sesameai.generator import Generator, Segment
    gen = Generator.__new__(Generator)
    gen.device, gen._text_tokenizer, gen._audio_tokenizer = codec.device, None, codec
    lens = lengths(requests * segs, 77)
    g = torch.Generator().manual_seed(78)
    clips = [(torch.randn(n, generator=g) * 0.3).to(codec.device) for n in lens]
    contexts = [[Segment(j % 2, [5, 6, 7], audio=clips[r * segs + j]) for j in range(segs)] for r in range(requests)]
    texts, speakers = [[11, 12, 13]] * requests, [0] * requests

    def wall(min_clips):
        keep = G.ENCODE_MANY_MIN_CLIPS
        G.ENCODE_MANY_MIN_CLIPS = min_clips
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = gen._build_prompts(texts, speakers, contexts)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, out
        finally:
            G.ENCODE_MANY_MIN_CLIPS = keep

    t_r, t_s, same = [], [], True
    for r in range(1 + rounds):
        a, pa = wall(2)
        b, pb = wall(10 ** 9)
        same = same and all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(pa, pb))
        if r:
            t_r.append(a); t_s.append(b)
    return dict(requests=requests, segments_per_request=segs, clips=len(clips), frames=sum(-(-n // codec.args.hop) for n in lens),
                prompts_equal=same, ragged_wall_ms=round(statistics.median(t_r), 2), per_segment_wall_ms=round(statistics.median(t_s), 2),
                speedup=round(statistics.median(t_s) / statistics.median(t_r), 3), rounds=rounds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--prompt-rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from sesameai.mimi import MimiArgs, MimiCodec, synthetic_state_dict
    codec = MimiCodec(MimiArgs(), synthetic_state_dict(MimiArgs(), seed=4321), max_frames=2400)
    res = dict(device=torch.cuda.get_device_name(0), encode=[], prompts=None)
    for N in (1, 2, 4, 8, 32):
        res["encode"].append(ragged_vs_singles(codec, N, a.rounds, a.warmup))
        print(json.dumps(res["encode"][-1]), flush=True)
    wins = [e["n"] for e in res["encode"] if e["ragged_ms"] < e["singles_ms"]]
    res["break_even_n"] = min(wins) if wins else None
    res["prompts"] = prompt_building(codec, 64, 4, a.prompt_rounds)
    print(json.dumps(res["prompts"]), flush=True)
    print(json.dumps(dict(break_even_n=res["break_even_n"])))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
