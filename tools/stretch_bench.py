#!/usr/bin/env python3
"""The device time-stretch pool on an MI355X (mimi_ts_pool_feed): what one launch costs beside the Mimi decode it follows and beside the
NumPy rule on the host, and what ``speed=`` costs a live batch.

  feed      one feed of 32 streams x 19,200 samples (one live-batch chunk of 10 frames; open clips, steady state) at 1.2 x.  "gpu_ms": between
            HIP events around the library call on a packed device buffer (the kernel); "pool_feed_wall_ms": TimeStretchPool.feed as a caller
            makes it, up to a synchronise; "mimi_pool_decode_gpu_ms": between HIP events around MimiStreamPool.decode of the same chunk (32
            streams x 10 frames, full-size codec); "numpy_rule_wall_ms": the same chunk through tests/stretch_ref.py's streams on the host.
            Alternating round by round.
  one_shot  64 clips x 10 s in one call with ``final``: gpu_ms between HIP events.
  live      ``generate_many_stream`` for 96 requests over 32 slots (full-size model and codec, synthetic weights, seeded limits of 25 .. 125
            frames, own seeds) with ``speed=1.2`` and with ``speed=None``, alternating in one process: generated frames / wall seconds up
            to the last chunk.  ``--live-only-none`` runs the ``None`` leg alone (also on a tree that has no ``speed=`` keyword).

    python tools/stretch_bench.py --out profiles/speed/speed.json
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

STREAMS, CHUNK, SPEED = 32, 19200, 1.2
REQUESTS, SLOTS = 96, 32
TEMP, TOPK = 0.8, 40


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
    f0 = 110.0 + 60.0 * rng.random()
    x = sum(np.sin(2 * np.pi * f0 * h * t + h) / h for h in range(1, 9)) * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t))
    return (0.2 * x + 0.01 * rng.standard_normal(n)).astype(np.float32)


def raw_feed(pool, N, n, final):
    """-> a function that times ONE mimi_ts_pool_feed of N streams x n samples between HIP events"""
    from sesameai import _abi
    packed = torch.from_numpy(np.concatenate([speechlike(n, 40 + i) for i in range(N)])).cuda()
    ids = (C.c_int32 * N)(*range(N))
    offs, lens = (C.c_long * N)(*[i * n for i in range(N)]), (C.c_long * N)(*[n] * N)
    fin, n_out = (C.c_int32 * N)(*[int(final)] * N), (C.c_long * N)()
    buf = torch.empty(N * (int(n / 0.5) + 4096), device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def gpu():
        e0.record()
        rc = _abi.lib.mimi_ts_pool_feed(pool._h, ids, offs, lens, fin, N, packed.data_ptr(), buf.data_ptr(), n_out, None, torch.cuda.current_stream().cuda_stream)
        e1.record()
        assert rc == 0
        e1.synchronize()
        return e0.elapsed_time(e1), int(sum(n_out))
    return gpu


def feed_leg(rounds, warmup):
    import stretch_ref as S
    from sesameai.mimi import MimiArgs, MimiCodec, synthetic_state_dict
    from sesameai.stretch import TimeStretchPool
    pool = TimeStretchPool(STREAMS)
    pool.reset(range(STREAMS), SPEED)
    gpu = raw_feed(pool, STREAMS, CHUNK, False)
    caller = TimeStretchPool(STREAMS)
    caller.reset(range(STREAMS), SPEED)
    host = [speechlike(CHUNK, 40 + i) for i in range(STREAMS)]
    chunks = [torch.from_numpy(h).cuda() for h in host]
    refs = [S.StreamRef(S.to_pm(SPEED)) for _ in range(STREAMS)]
    codec = MimiCodec(MimiArgs(), synthetic_state_dict(MimiArgs(), seed=4321), max_frames=160)
    mimi = codec.open_streams(STREAMS, max_chunk_frames=10)
    codes = torch.randint(0, 2048, (STREAMS, 32, 10), generator=torch.Generator().manual_seed(3), dtype=torch.int32).cuda()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def decode():
        e0.record(); mimi.decode(list(range(STREAMS)), codes); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1)

    def numpy_rule():
        t = time.perf_counter()
        for r, h in zip(refs, host):
            r.feed(h)
        return (time.perf_counter() - t) * 1e3

    t_gpu, t_feed, t_dec, t_np, outs = [], [], [], [], 0
    for r in range(warmup + rounds):
        (a, outs), b, c = gpu(), wall(lambda: caller.feed(range(STREAMS), chunks)), decode()
        d = numpy_rule() if r % 5 == 0 else None                  # (a tenth of a second a round: every fifth)
        if r >= warmup:
            t_gpu.append(a); t_feed.append(b); t_dec.append(c)
            if d is not None:
                t_np.append(d)
    return {"streams": STREAMS, "samples_in_per_stream": CHUNK, "speed": SPEED, "samples_out_last_call": outs, "blocks_per_stream": outs // STREAMS // 512,
            "gpu_ms": stats(t_gpu), "pool_feed_wall_ms": stats(t_feed), "mimi_pool_decode_gpu_ms": stats(t_dec), "numpy_rule_wall_ms": stats(t_np),
            "feed_over_decode_gpu": statistics.median(t_gpu) / statistics.median(t_dec)}


def one_shot_leg(rounds, warmup):
    from sesameai.stretch import TimeStretchPool
    N, n = 64, 240000
    pool = TimeStretchPool(N)
    pool.reset(range(N), SPEED)
    gpu = raw_feed(pool, N, n, True)
    t, outs = [], 0
    for r in range(warmup + rounds):
        a, outs = gpu()
        if r >= warmup:
            t.append(a)
    return {"clips": N, "seconds_per_clip": 10, "speed": SPEED, "samples_out": outs, "gpu_ms": stats(t)}


def live_leg(rounds, warmup, only_none):
    from sesameai.generator import Generator, Segment
    from sesameai.mimi import MimiArgs, MimiCodec, synthetic_state_dict as mimi_sd
    from sesameai.models import Model, csm_1b_args, synthetic_state_dict
    codec = MimiCodec(MimiArgs(), mimi_sd(MimiArgs(), seed=4321), max_frames=160)
    gen = Generator(Model(csm_1b_args(), synthetic_state_dict(csm_1b_args(), seed=1234), max_frames=256, max_prefill_rows=2048),
                    audio_tokenizer=codec, max_batch_size=SLOTS)
    g = torch.Generator().manual_seed(77)
    texts = [torch.randint(0, 128_256, (12,), generator=g).tolist() for _ in range(REQUESTS)]
    ctxs = [[Segment(speaker=1, text=torch.randint(0, 128_256, (20,), generator=g).tolist(), audio_codes=torch.randint(0, 2048, (32, 40), generator=g))]
            for _ in range(REQUESTS)]
    limits = [int(x) for x in torch.randint(25, 126, (REQUESTS,), generator=g)]
    seeds = [9000 + i for i in range(REQUESTS)]

    def run(**kw):
        gen._model.seed(7)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        frames = samples = 0
        for _i, pcm, fr, _last in gen.generate_many_stream(texts, [1] * REQUESTS, ctxs, max_audio_length_ms=[n * 80 for n in limits],
                                                           temperature=TEMP, topk=TOPK, seed=seeds, **kw):
            frames += fr.shape[0]; samples += pcm.shape[0]
        torch.cuda.synchronize()
        return frames / (time.perf_counter() - t0), frames, samples

    legs = {"none": {}} if only_none else {"speed_1.2": {"speed": SPEED}, "none": {}}
    fps = {k: [] for k in legs}
    counts = {}
    for r in range(warmup + rounds):
        for k, kw in legs.items():
            f, frames, samples = run(**kw)
            counts[k] = (frames, samples)
            print(json.dumps({"round": r, "leg": k, "frames_per_s": f, "frames": frames, "samples": samples}), flush=True)
            if r >= warmup:
                fps[k].append(f)
    out = {"requests": REQUESTS, "slots": SLOTS, "limits_frames_total": sum(limits), "sampling": [TEMP, TOPK],
           **{k: {"frames_per_s": stats(v), "frames": counts[k][0], "samples": counts[k][1]} for k, v in fps.items()}}
    if not only_none:
        out["speed_over_none_frames_per_s"] = statistics.median(fps["speed_1.2"]) / statistics.median(fps["none"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--live-rounds", type=int, default=3)
    ap.add_argument("--live-only-none", action="store_true")
    ap.add_argument("--skip-live", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("stretch_bench: needs a GPU (there is nothing to measure without one)")
    res = {"command": "python tools/stretch_bench.py " + " ".join(sys.argv[1:]), "device": torch.cuda.get_device_name(0),
           "what": "gpu_ms: between HIP events; wall_ms: host clock up to a synchronise; statistics over alternating rounds", "rounds": args.rounds, "warmup": args.warmup}
    if not args.live_only_none:
        res["feed"] = feed_leg(args.rounds, args.warmup)
        print(json.dumps({"feed": res["feed"]}), flush=True)
        res["one_shot"] = one_shot_leg(max(args.rounds // 3, 3), 2)
        print(json.dumps({"one_shot": res["one_shot"]}), flush=True)
    if not args.skip_live:
        res["live"] = live_leg(args.live_rounds, 1, args.live_only_none)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
