#!/usr/bin/env python3
"""The device loudness pool and the levelling finisher on an MI355X: what they cost beside the float64 meter on the host and beside the
finisher without a target.

  measure   64 clips x 10 s metered in one go (mimi_ld_pool_feed with ``final``, then mimi_ld_pool_integrate): "gpu_ms" between HIP events
            around the two library calls on a packed device buffer (three kernels); "feed_gpu_ms" the feed alone (6,400 hops through
            k_ld_energy, then k_ld_scan); "host_float64_wall_ms": the same 64 clips through a float64 BS.1770 meter on the host
            (scipy.signal.lfilter biquads, 400 ms blocks, both gates).
  feed      one feed of 32 open streams x 19,200 samples (a live batch's decode call: 8 hops a stream), metering only.
  finish    64 ragged clips (0.4 .. 12 s) through SegmentFinisher.finish with a target on every clip (meter + mimi_fin_segments_ld, five
            kernels) against the same clips without one (mimi_fin_segments, two kernels): gpu_ms between HIP events, alternating.
"fir" puts the energy kernel's time beside its dot2 and LDS counts.

    python tools/loudness_bench.py --out profiles/loudness/loudness.json
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

H, T = 2400, 512
DOT2_PER_HOP = H * T // 2                 # 614,400
LDS_READS_PER_HOP = 256 * 5 * (T // 2)    # 327,680 four-byte reads (every thread walks five output pairs, the idle fifth included)
# MI355X: 256 CUs x 4 SIMDs x 16 lanes at 2.4 GHz, one v_dot2_i32_i16 a lane a clock; LDS: 128 bytes a clock a CU
PEAK_DOT2_PER_S = 256 * 64 * 2.4e9
PEAK_LDS_BYTES_PER_S = 256 * 128 * 2.4e9


def stats(v):
    return {"median": statistics.median(v), "mean": statistics.fmean(v), "min": min(v), "max": max(v), "n": len(v)}


def speechlike(n, seed):
    t = np.arange(n) / 24000.0
    rng = np.random.default_rng(seed)
    f0 = 110.0 + 110.0 * rng.random()
    x = sum(np.sin(2 * np.pi * f0 * h * t + h * h) / h for h in range(1, 12)) * (np.sin(2 * np.pi * 0.7 * t + seed) > 0)
    return ((0.05 + 0.2 * rng.random()) * x + 0.002 * rng.standard_normal(n)).astype(np.float32)


def raw(pool, N, n, final, integrate):
    """-> a function that times ONE mimi_ld_pool_feed of N streams x n samples (and the integrate behind it) between HIP events"""
    from sesameai import _abi
    packed = torch.from_numpy(np.concatenate([speechlike(n, 40 + i) for i in range(N)])).cuda()
    ids = (C.c_int32 * N)(*range(N))
    offs, lens = (C.c_long * N)(*[i * n for i in range(N)]), (C.c_long * N)(*[n] * N)
    fin, n_h = (C.c_int32 * N)(*[int(final)] * N), (C.c_long * N)()
    energy = torch.empty(N * (n // H + 1), dtype=torch.int64, device="cuda")
    rows = torch.empty((N, 4), dtype=torch.int64, device="cuda")
    e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))

    def gpu():
        s = torch.cuda.current_stream().cuda_stream
        e0.record()
        rc = _abi.lib.mimi_ld_pool_feed(pool._h, ids, offs, lens, fin, N, packed.data_ptr(), 0, energy.data_ptr(), n_h, s)
        e1.record()
        if integrate:
            rc |= _abi.lib.mimi_ld_pool_integrate(pool._h, ids, N, rows.data_ptr(), s)
        e2.record()
        assert rc == 0
        e2.synchronize()
        return e0.elapsed_time(e1), e0.elapsed_time(e2), int(sum(n_h))
    return gpu, packed


def host_meter(clips):
    """the float64 BS.1770 meter of tests/test_loudness_oracle.py, timed"""
    from scipy.signal import lfilter

    import loudness_ref as L
    shelf, hp = L.loudness_taps.biquads(24000)
    t = time.perf_counter()
    out = []
    for x in clips:
        y = lfilter(hp[0], hp[1], lfilter(shelf[0], shelf[1], x.astype(np.float64)))
        nb = (y.shape[0] - 4 * H) // H + 1
        c = np.concatenate([[0.0], np.cumsum(y * y)])
        z = (c[4 * H:4 * H + nb * H:H] - c[0:nb * H:H]) / (4 * H)
        keep = z > 10 ** ((-70 + 0.691) / 10)
        if keep.any():
            keep &= z > z[keep].mean() / 10
        out.append(-0.691 + 10 * np.log10(z[keep].mean()) if keep.any() else float("-inf"))
    return (time.perf_counter() - t) * 1e3, out


def measure_leg(rounds, warmup):
    from sesameai.loudness import LoudnessPool
    N, n = 64, 240000
    pool = LoudnessPool(N)
    gpu, packed = raw(pool, N, n, True, True)
    t_feed, t_all, hops = [], [], 0
    for r in range(warmup + rounds):
        a, b, hops = gpu()
        if r >= warmup:
            t_feed.append(a); t_all.append(b)
    host = packed.cpu().numpy().reshape(N, n)
    t_host = [host_meter(host)[0] for _ in range(3)]
    sec = statistics.median(t_feed) * 1e-3
    fir = {"hops": hops, "dot2": hops * DOT2_PER_HOP, "lds_read_bytes": hops * LDS_READS_PER_HOP * 4,
           "dot2_fraction_of_peak": hops * DOT2_PER_HOP / sec / PEAK_DOT2_PER_S,
           "lds_fraction_of_peak": hops * LDS_READS_PER_HOP * 4 / sec / PEAK_LDS_BYTES_PER_S,
           "note": "from feed_gpu_ms, which also holds k_ld_scan and the launch gaps: a lower bound on the kernel's own fractions"}
    return {"clips": N, "seconds_per_clip": 10, "hops": hops, "gpu_ms": stats(t_all), "feed_gpu_ms": stats(t_feed),
            "host_float64_wall_ms": stats(t_host), "fir": fir}


def feed_leg(rounds, warmup):
    from sesameai.loudness import LoudnessPool
    N, n = 32, 19200
    gpu, _ = raw(LoudnessPool(N), N, n, False, False)
    t, hops = [], 0
    for r in range(warmup + rounds):
        a, _, hops = gpu()
        if r >= warmup:
            t.append(a)
    return {"streams": N, "samples_in_per_stream": n, "hops_last_call": hops, "gpu_ms": stats(t)}


def finish_leg(rounds, warmup):
    from sesameai.finish import SegmentFinish, SegmentFinisher
    rng = np.random.default_rng(3)
    clips = [torch.from_numpy(speechlike(int(v), 7 + i)).cuda() for i, v in enumerate(rng.integers(9600, 288000, 64))]
    fin = SegmentFinisher()
    plain, level = SegmentFinish(), SegmentFinish(loudness=-19.0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def run(how):
        e0.record(); fin.finish(clips, how); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1)
    t_plain, t_level = [], []
    for r in range(warmup + rounds):
        a, b = run(plain), run(level)
        if r >= warmup:
            t_plain.append(a); t_level.append(b)
    return {"clips": 64, "samples": int(sum(c.shape[0] for c in clips)), "mimi_fin_segments_gpu_ms": stats(t_plain),
            "meter_and_mimi_fin_segments_ld_gpu_ms": stats(t_level),
            "note": "between HIP events around SegmentFinisher.finish: the host's packing of the clips for the meter lies inside the second figure"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("loudness_bench: needs a GPU (there is nothing to measure without one)")
    res = {"command": "python tools/loudness_bench.py " + " ".join(sys.argv[1:]), "device": torch.cuda.get_device_name(0),
           "what": "gpu_ms: between HIP events; wall_ms: host clock; statistics over rounds after warm-up", "rounds": args.rounds, "warmup": args.warmup}
    res["measure"] = measure_leg(args.rounds, args.warmup)
    print(json.dumps({"measure": res["measure"]}), flush=True)
    res["feed"] = feed_leg(args.rounds, args.warmup)
    res["finish"] = finish_leg(args.rounds, args.warmup)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
