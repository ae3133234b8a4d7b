#!/usr/bin/env python3
"""The device watermark pool on an MI355X (mimi_wm_pool_feed / mimi_wm_pool_detect): what a call costs beside the Mimi decode it follows and
beside the NumPy rule on the host.

  feed      one feed of 32 streams x 19,200 samples (one chunk of 10 Mimi frames a stream: ten blocks each; open clips, steady state).
            "gpu_ms": between HIP events around the library call on a packed device buffer (its one kernel); "pool_feed_wall_ms":
            WatermarkPool.feed as a caller makes it, up to a synchronise; "mimi_pool_decode_gpu_ms": between HIP events around
            MimiStreamPool.decode of the same chunk (32 streams x 10 frames, full-size codec); "numpy_rule_wall_ms": the same chunk through
            tests/watermark_ref.py's streams on the host.  Alternating round by round.
  detect    64 clips x 10 s over 4,096 offsets in one call, and one 10 s clip over the full period: gpu_ms between HIP events;
            "numpy_rule_wall_s": ONE 10 s clip over 4,096 offsets through tests/watermark_ref.py (once).

    python tools/wm_bench.py --out profiles/watermark/watermark.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "sesameai-tts_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

STREAMS, CHUNK = 32, 19200
P = 1920 * 56


def stats(v):
    return {"median": statistics.median(v), "mean": statistics.fmean(v), "min": min(v), "max": max(v), "n": len(v)}


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def speechlike(n, seed):
    t = np.arange(n) / 24000.0
    rng = np.random.default_rng(seed)
    f0 = 110.0 + 110.0 * rng.random()
    x = sum(np.sin(2 * np.pi * f0 * h * t + h * h) / h for h in range(1, 12)) * (0.55 + 0.45 * np.sin(2 * np.pi * 3.0 * t + seed))
    return (0.15 * x + 0.003 * rng.standard_normal(n)).astype(np.float32)


def raw_feed(pool, N, n):
    """-> a function that times ONE mimi_wm_pool_feed of N streams x n samples between HIP events"""
    from sesameai import _abi
    packed = torch.from_numpy(np.concatenate([speechlike(n, 40 + i) for i in range(N)])).cuda()
    out = torch.empty(N * (n + 1920), dtype=torch.float32, device="cuda")
    ids = (C.c_int32 * N)(*range(N))
    offs, lens = (C.c_long * N)(*[i * n for i in range(N)]), (C.c_long * N)(*[n] * N)
    fin, n_out = (C.c_int32 * N)(*[0] * N), (C.c_long * N)()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def gpu():
        e0.record()
        rc = _abi.lib.mimi_wm_pool_feed(pool._h, ids, offs, lens, fin, N, packed.data_ptr(), 0, out.data_ptr(), n_out, torch.cuda.current_stream().cuda_stream)
        e1.record()
        assert rc == 0
        e1.synchronize()
        return e0.elapsed_time(e1), int(sum(n_out))
    return gpu


def feed_leg(rounds, warmup):
    import watermark_ref as W
    from sesameai.mimi import MimiArgs, MimiCodec, synthetic_state_dict
    from sesameai.watermarking import WatermarkPool
    pool = WatermarkPool(STREAMS)
    gpu = raw_feed(pool, STREAMS, CHUNK)
    caller = WatermarkPool(STREAMS)
    host = [speechlike(CHUNK, 40 + i) for i in range(STREAMS)]
    chunks = [torch.from_numpy(h).cuda() for h in host]
    refs = [W.StreamEmbed() for _ in range(STREAMS)]
    codec = MimiCodec(MimiArgs(), synthetic_state_dict(MimiArgs(), seed=4321), max_frames=160)
    dec = codec.open_streams(STREAMS, max_chunk_frames=10)
    codes = torch.randint(0, 2048, (STREAMS, 32, 10), dtype=torch.int32, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def decode(r):
        if r % 12 == 0:
            dec.reset(list(range(STREAMS)))                       # (a stream holds at most max_frames)
        e0.record(); dec.decode(list(range(STREAMS)), codes); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1)

    def numpy_rule():
        t = time.perf_counter()
        for r, h in zip(refs, host):
            r.feed(h)
        return (time.perf_counter() - t) * 1e3

    t_gpu, t_feed, t_dec, t_np, given = [], [], [], [], 0
    for r in range(warmup + rounds):
        (a, given), b, c = gpu(), wall(lambda: caller.feed(range(STREAMS), chunks)), decode(r)
        d = numpy_rule() if r % 10 == 0 else None
        if r >= warmup:
            t_gpu.append(a); t_feed.append(b); t_dec.append(c)
            if d is not None:
                t_np.append(d)
    return {"streams": STREAMS, "samples_in_per_stream": CHUNK, "samples_out_last_call": given, "gpu_ms": stats(t_gpu), "pool_feed_wall_ms": stats(t_feed),
            "mimi_pool_decode_gpu_ms": stats(t_dec), "numpy_rule_wall_ms": stats(t_np),
            "feed_over_decode_gpu": statistics.median(t_gpu) / statistics.median(t_dec)}


def raw_detect(pool, clips, n_off):
    from sesameai import _abi
    from sesameai.watermarking import ALL_MASK, symbol_bits, CSM_1B_GH_WATERMARK
    N, n = len(clips), len(clips[0])
    packed = torch.from_numpy(np.concatenate(clips)).cuda()
    L, U = C.c_long * N, C.c_uint64 * N
    offs, lens, o0, noff = L(*[i * n for i in range(N)]), L(*[n] * N), L(*[0] * N), L(*[n_off] * N)
    ex, mk = U(*[symbol_bits(CSM_1B_GH_WATERMARK)] * N), U(*[ALL_MASK] * N)
    scores = torch.empty(N * n_off, dtype=torch.int32, device="cuda")
    rows = torch.empty(N, 64, dtype=torch.int64, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def gpu():
        e0.record()
        rc = _abi.lib.mimi_wm_pool_detect(pool._h, offs, lens, o0, noff, ex, mk, N, packed.data_ptr(), 0, scores.data_ptr(), rows.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream)
        e1.record()
        assert rc == 0
        e1.synchronize()
        return e0.elapsed_time(e1), rows[:, :4].cpu().tolist()
    return gpu


def detect_leg(rounds, warmup):
    import watermark_ref as W
    from sesameai.watermarking import WatermarkPool
    pool = WatermarkPool(1)
    marked = [W.embed(speechlike(240000 + 1000, 70 + i))[1000:] for i in range(64)]       # cut by 1,000 samples: found at offset 1,000
    many, one = raw_detect(pool, marked, 4096), raw_detect(pool, marked[:1], P)
    t_many, t_one, rows = [], [], None
    for r in range(warmup + rounds):
        (a, rows), (b, row1) = many(), one()
        if r >= warmup:
            t_many.append(a); t_one.append(b)
    assert all(r[1] == 1000 and r[2] == 56 for r in rows) and row1[0][1] == 1000, (rows[:2], row1)
    t = time.perf_counter()
    ref = W.detect(marked[0], W.DEFAULT_PAYLOAD, o0=0, n_off=4096)
    t_np = time.perf_counter() - t
    assert ref[1] == 1000 and ref[2] == 56
    return {"clips_64_x_10s_over_4096_offsets_gpu_ms": stats(t_many), "one_10s_clip_over_the_full_period_gpu_ms": stats(t_one),
            "numpy_rule_one_10s_clip_over_4096_offsets_wall_s": t_np, "every_clip_found_at": 1000, "score": 56}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("wm_bench: needs a GPU (there is nothing to measure without one)")
    res = {"command": "python tools/wm_bench.py " + " ".join(sys.argv[1:]), "device": torch.cuda.get_device_name(0),
           "what": "gpu_ms: between HIP events; wall: host clock up to a synchronise; statistics over alternating rounds", "rounds": args.rounds, "warmup": args.warmup}
    res["feed"] = feed_leg(args.rounds, args.warmup)
    print(json.dumps({"feed": res["feed"]}), flush=True)
    res["detect"] = detect_leg(max(args.rounds // 3, 3), 2)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
