"""Times the log-mel pool (sesameai/mel.py) on the device, feed + finish, by HIP events (median of ``--iters`` calls after ``--warmup``):
  (a) 64 clips x 30 s in one shot;  (b) a live-shaped call: 32 open streams x 1,280 new samples;  (c) the END-of-turn tail: one stream's
  final 1,280 samples of a 10 s turn plus ``finish``.
Beside them what a caller does today for one 10 s turn, wall time: device -> host copy, host resample 24 -> 16 kHz, transformers'
WhisperFeatureExtractor on at most 16 CPU threads, host -> device copy of the features; and the extractor's ``device="cuda"`` path.
Those two need transformers (and the first scipy) and are skipped with a note where it is absent.  Prints one JSON line.
  python tools/mel_bench.py [--iters 30] [--warmup 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sesameai-tts_amd"), os.path.join(ROOT, "tests")]

PEAK_F32_MFMA = 157.3e12          # FLOP/s, the chip's fp32 matrix peak


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "iters": iters}


def wall(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "iters": iters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import mel_ref as R
    from sesameai.mel import MelPool
    dev = torch.device("cuda")
    n_mels = 80
    pool = MelPool(64, n_mels, device=dev)
    speech = torch.from_numpy(R.signal("speech", 7, 480000)).to(dev)
    res = {"n_mels": n_mels, "threads": min(16, os.cpu_count() or 1)}

    clips = [speech.roll(977 * k) for k in range(64)]
    ids = list(range(64))

    def one_shot():
        pool.reset(ids)
        return pool.finish(pool.feed(ids, clips, True))
    res["a_64x30s_feed_finish"] = timed(one_shot, max(5, args.iters // 3), 2)
    tiles = 64 * 94
    flop = tiles * (2 * 32 * 400 * 448 + 2 * 32 * 224 * 32 * ((n_mels + 31) // 32))

    def feed_only():
        pool.reset(ids)
        return pool.feed(ids, clips, True)
    res["a_64x30s_feed_only"] = timed(feed_only, max(5, args.iters // 3), 2)
    res["a_mfma_flop"] = flop
    res["a_mfma_fraction_of_peak"] = flop / (res["a_64x30s_feed_only"]["median_ms"] * 1e-3) / PEAK_F32_MFMA

    live = list(range(32))
    pool.reset(live)
    pool.feed(live, [speech[:16000]] * 32, False)
    chunk = [speech[16000 + 40 * k:16000 + 40 * k + 1280] for k in range(32)]
    res["b_32_streams_x_1280"] = timed(lambda: pool.feed(live, chunk, False), args.iters, args.warmup)      # (the streams run on: 30 x 80 ms stay far under the cap)

    held = {}

    def tail_setup():
        pool.reset([40])
        held["rows"] = pool.feed([40], [speech[:160000 - 1280]], False)[0].clone()

    def tail():
        (rows,) = pool.feed([40], [speech[160000 - 1280:160000]], True)
        return pool.finish([torch.cat([held["rows"], rows])])
    ms = []
    for k in range(args.warmup + args.iters):
        tail_setup()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        tail()
        b.record()
        b.synchronize()
        if k >= args.warmup:
            ms.append(a.elapsed_time(b))
    res["c_end_of_turn_tail"] = {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "iters": args.iters}

    # what a caller does today for one 10 s turn at 24 kHz that lies on the device
    turn24 = torch.from_numpy(R.signal("speech", 8, 240000)).to(dev)
    torch.set_num_threads(res["threads"])
    try:
        from scipy.signal import resample_poly
        from transformers import WhisperFeatureExtractor
        fe = WhisperFeatureExtractor(feature_size=n_mels)

        def today_cpu():
            x = turn24.cpu().numpy()
            y = resample_poly(x, 2, 3).astype("float32")
            f = fe(y, sampling_rate=16000, return_tensors="pt").input_features
            return f.to(dev)
        res["today_cpu_extractor_10s_wall"] = wall(today_cpu, args.iters, args.warmup)

        def today_cuda():
            x = turn24.cpu().numpy()
            y = resample_poly(x, 2, 3).astype("float32")
            f = fe(y, sampling_rate=16000, return_tensors="pt", device="cuda").input_features
            return f.to(dev)
        res["today_cuda_extractor_10s_wall"] = wall(today_cuda, args.iters, args.warmup)
    except Exception as e:                                   # transformers or scipy absent: the comparison is not taken here
        res["today_skipped"] = f"{type(e).__name__}: {e}"

    from sesameai.mel import TurnFeatures
    tf = TurnFeatures(1, src_rate=24000, n_mels=n_mels, device=dev)

    def ours_whole_turn():
        tf.feed([0], [turn24], True)
        return tf.take(0)
    res["ours_10s_turn_resample_feed_finish_wall"] = wall(ours_whole_turn, args.iters, args.warmup)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
