#!/usr/bin/env python3
"""The device resampler pool on an MI355X (mimi_rs_pool_feed): what one launch costs, against the only way there was before -- scipy's
resample_poly on the host, whole clip at a time, plus the upload -- and what it adds to a TurnStreams.pump.

  feed      one feed of N = 1 / 8 / 32 streams x 0.8 s at 48 kHz -> 24 kHz (open clips, steady state), and one 10 s clip at 44.1 kHz -> 24 kHz
            (one shot, final).  "gpu_ms": between HIP events around the library call on a packed device buffer (the kernel);
            "pool_feed_wall_ms": ResamplerPool.feed as a caller makes it (packing, output allocation, the launch) up to a synchronise;
            "host_resample_poly_plus_upload_wall_ms": the same samples through scipy.signal.resample_poly (fp32) on the host and .cuda(),
            up to a synchronise, in the same process, alternating round by round.
  pump      TurnStreams.pump for 8 microphones x 0.8 s, full-size codec: at 24 kHz without a resampler, at 48 kHz int16 with one; wall ms up
            to a synchronise, alternating.

    python tools/resample_bench.py --out profiles/resample/resample.json
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


def stats(v):
    return {"median": statistics.median(v), "mean": statistics.fmean(v), "min": min(v), "max": max(v), "n": len(v)}


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def feed_leg(rounds, warmup):
    from scipy.signal import resample_poly
    from sesameai import _abi
    from sesameai.resample import ResamplerPool
    out = []
    for src, dst, N, seconds, final in ((48000, 24000, 1, 0.8, False), (48000, 24000, 8, 0.8, False), (48000, 24000, 32, 0.8, False), (44100, 24000, 1, 10.0, True)):
        n = int(src * seconds)
        pool = ResamplerPool(src, dst, N)
        host = [(torch.randn(n, generator=torch.Generator().manual_seed(40 + i)) * 0.3) for i in range(N)]
        chunks = [h.cuda() for h in host]
        packed = torch.cat(chunks)
        ids = list(range(N))
        arr_ids, offs, lens = (C.c_int32 * N)(*ids), (C.c_long * N)(*[i * n for i in range(N)]), (C.c_long * N)(*[n] * N)
        fin, n_out = (C.c_int32 * N)(*[int(final)] * N), (C.c_long * N)()
        buf = torch.empty(N * (n * pool.up // pool.down + 64), device="cuda")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        up, down = pool.up, pool.down

        def gpu():
            e0.record()
            rc = _abi.lib.mimi_rs_pool_feed(pool._h, arr_ids, offs, lens, fin, N, packed.data_ptr(), 0, buf.data_ptr(), 0, n_out, torch.cuda.current_stream().cuda_stream)
            e1.record()
            assert rc == 0
            e1.synchronize()
            return e0.elapsed_time(e1)

        def host_way():
            return [torch.from_numpy(resample_poly(h.numpy(), up, down)).cuda() for h in host]

        t_gpu, t_feed, t_host = [], [], []
        for r in range(warmup + rounds):                            # the three alternate round by round
            a, b, c = gpu(), wall(lambda: pool.feed(ids, chunks, final)), wall(host_way)
            if r >= warmup:
                t_gpu.append(a); t_feed.append(b); t_host.append(c)
        out.append({"src_rate": src, "dst_rate": dst, "streams": N, "seconds_per_stream": seconds, "samples_in_per_stream": n, "final": final,
                    "samples_out_last_call": int(sum(n_out)), "gpu_ms": stats(t_gpu), "pool_feed_wall_ms": stats(t_feed),
                    "host_resample_poly_plus_upload_wall_ms": stats(t_host),
                    "host_over_pool_feed_wall": statistics.median(t_host) / statistics.median(t_feed)})
        print(json.dumps(out[-1]), flush=True)
        del pool
    return out


def pump_leg(rounds, warmup):
    from sesameai.mimi import MimiArgs, MimiCodec, synthetic_state_dict
    from sesameai.resample import ResamplerPool
    from sesameai.turns import TurnStreams
    codec = MimiCodec(MimiArgs(), synthetic_state_dict(MimiArgs(), seed=4321), max_frames=160)
    N, hop = 8, codec.args.hop
    plain = TurnStreams(codec.open_encode_streams(N, max_chunk_frames=10), hop, 10)
    fast = TurnStreams(codec.open_encode_streams(N, max_chunk_frames=10), hop, 10, resampler=ResamplerPool(48000, 24000, N))
    x24 = [(torch.randn(10 * hop, generator=torch.Generator().manual_seed(60 + i)) * 0.3).cuda() for i in range(N)]
    x48 = [((torch.randn(20 * hop, generator=torch.Generator().manual_seed(80 + i)) * 0.3).clamp(-1, 1) * 32767).round().to(torch.int16).cuda() for i in range(N)]
    t_plain, t_fast, frames = [], [], []

    def go(ts, xs):
        for s, x in enumerate(xs):
            ts.feed(s, x)
        frames.append(ts.pump())

    for r in range(warmup + rounds):
        a, b = wall(lambda: go(plain, x24)), wall(lambda: go(fast, x48))
        if r >= warmup:
            t_plain.append(a); t_fast.append(b)
    return {"streams": N, "seconds_per_stream": 0.8, "frames_per_pump": sorted(set(frames)), "pump_24k_fp32_no_resampler_wall_ms": stats(t_plain),
            "pump_48k_int16_with_resampler_wall_ms": stats(t_fast), "added_ms": statistics.median(t_fast) - statistics.median(t_plain)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("resample_bench: needs a GPU (there is nothing to measure without one)")
    res = {"command": "python tools/resample_bench.py " + " ".join(sys.argv[1:]), "device": torch.cuda.get_device_name(0),
           "what": "gpu_ms: between HIP events; wall_ms: host clock up to a synchronise; medians over alternating rounds", "rounds": args.rounds, "warmup": args.warmup}
    res["feed"] = feed_leg(args.rounds, args.warmup)
    res["pump"] = pump_leg(args.rounds, args.warmup)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
