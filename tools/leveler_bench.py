#!/usr/bin/env python3
"""The live leveler on an MI355X (mimi_ld_pool_level_*): what levelling costs beside metering the same samples, and what it costs a
served live batch.

  feed      one live-shaped call of 32 open streams x 19,200 fp32 samples (8 hops a stream): mimi_ld_pool_level_feed (three kernels:
            k_ld_energy, k_ld_level_scan, k_ld_apply) against mimi_ld_pool_feed (two: k_ld_energy, k_ld_scan) on the same packed buffer,
            alternating, "gpu_ms" between HIP events around the ONE library call.
  level     64 clips x 10 s on fresh streams with ``final``: mimi_ld_pool_level_feed against mimi_ld_pool_feed + mimi_ld_pool_integrate
            (what ``measure`` makes), alternating.  "apply" puts the difference beside the bytes k_ld_apply moves (8 a sample in fp32):
            a LOWER bound on its rate, for the difference also holds the scan's gain walk.
  live      ``generate_many_stream`` for 96 requests over 32 slots (full-size model and codec, synthetic weights, seeded limits of
            25 .. 125 frames) with and without ``loudness=-19``, alternating: frames per second on the host clock up to a synchronise.
Kernel times proper come from a kernel trace of this tool with --skip-live, in a run of its own (docs/experiments/leveler.md).

    python tools/leveler_bench.py --out profiles/leveler/leveler.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "sesameai-tts_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from loudness_bench import speechlike, stats  # noqa: E402

H = 2400
HBM_BYTES_PER_S = 8.0e12                  # MI355X: HBM3E peak
SLOTS, REQUESTS, TEMP, TOPK = 32, 96, 0.9, 50


def pair(N, n, final, integrate):
    """-> a function that times ONE metering call and ONE levelling call of N streams x n samples between HIP events"""
    from sesameai import _abi
    from sesameai.loudness import Level, LoudnessPool
    meter, lev = LoudnessPool(N), LoudnessPool(N)
    lev.level_reset(range(N), Level(-19.0))
    packed = torch.from_numpy(np.concatenate([speechlike(n, 40 + i) for i in range(N)])).cuda()
    out = torch.empty_like(packed)
    ids = (C.c_int32 * N)(*range(N))
    offs, lens = (C.c_long * N)(*[i * n for i in range(N)]), (C.c_long * N)(*[n] * N)
    fin, n_h = (C.c_int32 * N)(*[int(final)] * N), (C.c_long * N)()
    hops_max = N * (n // H + 1)
    energy = torch.empty(hops_max, dtype=torch.int64, device="cuda")
    gain = torch.empty(hops_max + 2 * N, dtype=torch.int32, device="cuda")
    rows = torch.empty((N, 4), dtype=torch.int64, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def run(level):
        s = torch.cuda.current_stream().cuda_stream
        e0.record()
        if level:
            rc = _abi.lib.mimi_ld_pool_level_feed(lev._h, ids, offs, lens, fin, N, packed.data_ptr(), 0, out.data_ptr(), energy.data_ptr(),
                                                  gain.data_ptr(), n_h, s)
        else:
            rc = _abi.lib.mimi_ld_pool_feed(meter._h, ids, offs, lens, fin, N, packed.data_ptr(), 0, energy.data_ptr(), n_h, s)
            if integrate:
                rc |= _abi.lib.mimi_ld_pool_integrate(meter._h, ids, N, rows.data_ptr(), s)
        e1.record()
        assert rc == 0
        e1.synchronize()
        return e0.elapsed_time(e1), int(sum(n_h))
    return run


def pair_leg(N, n, final, integrate, rounds, warmup):
    run = pair(N, n, final, integrate)
    t = {False: [], True: []}
    hops = 0
    for r in range(warmup + rounds):
        for level in (False, True):
            ms, hops = run(level)
            if r >= warmup:
                t[level].append(ms)
    extra = (statistics.median(t[True]) - statistics.median(t[False])) * 1e-3
    nbytes = N * n * 8
    return {"streams": N, "samples_per_stream": n, "hops_last_call": hops, "meter_gpu_ms": stats(t[False]), "level_gpu_ms": stats(t[True]),
            "level_over_meter": statistics.median(t[True]) / statistics.median(t[False]),
            "apply": {"bytes": nbytes, "extra_ms": extra * 1e3, "bytes_per_s_lower_bound": nbytes / extra if extra > 0 else None,
                      "fraction_of_hbm_peak_lower_bound": nbytes / extra / HBM_BYTES_PER_S if extra > 0 else None,
                      "note": "level - meter also holds the scan's gain walk and one more launch: a lower bound on k_ld_apply's own rate"}}


def live_leg(rounds, warmup):
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

    legs = {"loudness_-19": {"loudness": -19.0}, "none": {}}
    fps, counts = {k: [] for k in legs}, {}
    for r in range(warmup + rounds):
        for k, kw in legs.items():
            f, frames, samples = run(**kw)
            counts[k] = (frames, samples)
            print(json.dumps({"round": r, "leg": k, "frames_per_s": f, "frames": frames, "samples": samples}), flush=True)
            if r >= warmup:
                fps[k].append(f)
    return {"requests": REQUESTS, "slots": SLOTS, "limits_frames_total": sum(limits), "sampling": [TEMP, TOPK],
            **{k: {"frames_per_s": stats(v), "frames": counts[k][0], "samples": counts[k][1]} for k, v in fps.items()},
            "loudness_over_none_frames_per_s": statistics.median(fps["loudness_-19"]) / statistics.median(fps["none"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--live-rounds", type=int, default=3)
    ap.add_argument("--skip-live", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("leveler_bench: needs a GPU (there is nothing to measure without one)")
    res = {"command": "python tools/leveler_bench.py " + " ".join(sys.argv[1:]), "device": torch.cuda.get_device_name(0),
           "what": "gpu_ms: between HIP events, medians over alternating rounds after warm-up; frames_per_s: host clock up to a synchronise",
           "rounds": args.rounds, "warmup": args.warmup}
    res["feed"] = pair_leg(32, 19200, False, False, args.rounds, args.warmup)
    print(json.dumps({"feed": res["feed"]}), flush=True)
    res["level"] = pair_leg(64, 240000, True, True, args.rounds, args.warmup)
    print(json.dumps({"level": res["level"]}), flush=True)
    if not args.skip_live:
        res["live"] = live_leg(args.live_rounds, 1)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
