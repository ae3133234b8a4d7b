#!/usr/bin/env python3
"""The device voice-activity pool on an MI355X (mimi_vad_pool_feed): what one call costs beside the Mimi encode it precedes and beside the
NumPy rule on the host.

  feed      one feed of 32 streams x 19,200 samples (one pump of 10 Mimi frames a stream: 80 detector frames each; open clips, steady
            state).  "gpu_ms": between HIP events around the library call on a packed device buffer (its two kernels);
            "pool_feed_wall_ms": VadPool.feed as a caller makes it, up to a synchronise; "mimi_enc_pool_encode_gpu_ms": between HIP events
            around MimiEncodeStreamPool.encode of the same chunk (32 streams x 10 frames, full-size codec);
            "numpy_rule_wall_ms": the same chunk through tests/vad_ref.py's streams on the host.  Alternating round by round.
  detect    64 clips x 10 s in one call with ``final``: gpu_ms between HIP events.

    python tools/vad_bench.py --out profiles/vad/vad.json
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


def stats(v):
    return {"median": statistics.median(v), "mean": statistics.fmean(v), "min": min(v), "max": max(v), "n": len(v)}


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def speechlike(n, seed):
    """a voice that comes and goes over hiss: the detector has something to decide"""
    t = np.arange(n) / 24000.0
    rng = np.random.default_rng(seed)
    f0 = 110.0 + 110.0 * rng.random()
    x = sum(np.sin(2 * np.pi * f0 * h * t + h * h) / h for h in range(1, 12)) * (np.sin(2 * np.pi * 0.7 * t + seed) > 0)
    return (0.15 * x + 0.002 * rng.standard_normal(n)).astype(np.float32)


def raw_feed(pool, N, n, final):
    """-> a function that times ONE mimi_vad_pool_feed of N streams x n samples between HIP events"""
    from sesameai import _abi
    packed = torch.from_numpy(np.concatenate([speechlike(n, 40 + i) for i in range(N)])).cuda()
    ids = (C.c_int32 * N)(*range(N))
    offs, lens = (C.c_long * N)(*[i * n for i in range(N)]), (C.c_long * N)(*[n] * N)
    fin, n_fr = (C.c_int32 * N)(*[int(final)] * N), (C.c_long * N)()
    K = N * (n // 240 + 1)
    flags, lag = torch.empty(K, dtype=torch.uint8, device="cuda"), torch.empty(K, dtype=torch.int16, device="cuda")
    power, floor = torch.empty(K, dtype=torch.int64, device="cuda"), torch.empty(K, dtype=torch.int64, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def gpu():
        e0.record()
        rc = _abi.lib.mimi_vad_pool_feed(pool._h, ids, offs, lens, fin, N, packed.data_ptr(), 0, flags.data_ptr(), lag.data_ptr(), power.data_ptr(),
                                         floor.data_ptr(), n_fr, torch.cuda.current_stream().cuda_stream)
        e1.record()
        assert rc == 0
        e1.synchronize()
        return e0.elapsed_time(e1), int(sum(n_fr))
    return gpu


def feed_leg(rounds, warmup):
    import vad_ref as V
    from sesameai.mimi import MimiArgs, MimiCodec, synthetic_state_dict
    from sesameai.vad import VadPool
    pool = VadPool(STREAMS)
    gpu = raw_feed(pool, STREAMS, CHUNK, False)
    caller = VadPool(STREAMS)
    host = [speechlike(CHUNK, 40 + i) for i in range(STREAMS)]
    chunks = [torch.from_numpy(h).cuda() for h in host]
    refs = [V.StreamRef() for _ in range(STREAMS)]
    codec = MimiCodec(MimiArgs(), synthetic_state_dict(MimiArgs(), seed=4321), max_frames=160)
    enc = codec.open_encode_streams(STREAMS, max_chunk_frames=10)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def encode():
        e0.record(); enc.encode(list(range(STREAMS)), chunks); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1)

    def numpy_rule():
        t = time.perf_counter()
        for r, h in zip(refs, host):
            r.feed(h)
        return (time.perf_counter() - t) * 1e3

    t_gpu, t_feed, t_enc, t_np, frames = [], [], [], [], 0
    for r in range(warmup + rounds):
        (a, frames), b, c = gpu(), wall(lambda: caller.feed(range(STREAMS), chunks)), encode()
        d = numpy_rule() if r % 10 == 0 else None                 # (about a second a round: every tenth)
        if r >= warmup:
            t_gpu.append(a); t_feed.append(b); t_enc.append(c)
            if d is not None:
                t_np.append(d)
    return {"streams": STREAMS, "samples_in_per_stream": CHUNK, "frames_last_call": frames, "gpu_ms": stats(t_gpu), "pool_feed_wall_ms": stats(t_feed),
            "mimi_enc_pool_encode_gpu_ms": stats(t_enc), "numpy_rule_wall_ms": stats(t_np),
            "feed_over_encode_gpu": statistics.median(t_gpu) / statistics.median(t_enc)}


def detect_leg(rounds, warmup):
    from sesameai.vad import VadPool
    N, n = 64, 240000
    pool = VadPool(N)
    gpu = raw_feed(pool, N, n, True)
    t, frames = [], 0
    for r in range(warmup + rounds):
        a, frames = gpu()
        if r >= warmup:
            t.append(a)
    return {"clips": N, "seconds_per_clip": 10, "frames": frames, "gpu_ms": stats(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("vad_bench: needs a GPU (there is nothing to measure without one)")
    res = {"command": "python tools/vad_bench.py " + " ".join(sys.argv[1:]), "device": torch.cuda.get_device_name(0),
           "what": "gpu_ms: between HIP events; wall_ms: host clock up to a synchronise; statistics over alternating rounds", "rounds": args.rounds, "warmup": args.warmup}
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
