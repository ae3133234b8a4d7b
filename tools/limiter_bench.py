#!/usr/bin/env python3
"""The look-ahead limiter on an MI355X (mimi_lim_pool_*): what limiting costs beside levelling the same samples, and what it costs a
served live batch.

  feed      one live-shaped call of 32 open streams x 19,200 fp32 samples: mimi_lim_pool_feed (two kernels: k_lim_carry, k_lim_apply)
            against mimi_ld_pool_level_feed (three: k_ld_energy, k_ld_level_scan, k_ld_apply) on the same packed buffer, alternating,
            "gpu_ms" between HIP events around the ONE library call.  The limiter's streams are open (fed once before the clock starts), so
            every call reads its carry and holds its look-ahead back, as a live call does.
  clips     64 clips x 10 s on fresh streams with ``final``, the same pair.  "halo" puts beside the ratio what the rule makes a tile
            restage: (TILE + K + 2 L) required gains for TILE outputs.
  shapes    the 64 clips through the limiter alone at four (look-ahead, release) pairs from (1 sample, K = 1) to (480, K = 8192),
            alternating: what the halo and the minimum's passes cost.
  live      ``generate_many_stream`` for 96 requests over 32 slots (full-size model and codec, synthetic weights, seeded limits of
            25 .. 125 frames) with and without ``limiter=True``, alternating: frames per second on the host clock up to a synchronise.
  true_peak the "feed" and "clips" shapes once more, sample-peak streams against true-peak streams (``Limit(true_peak=True)``) of two
            pools on the same packed buffer, alternating; the yardstick is the sample-peak feed of the same run.  At drive_shift 2, as
            the legs above (samples of 2^15 and more: the taps in 64 bits), and at drive_shift 0 ("narrow": int16 pairs).  For the clips also
            mimi_tp_measure (one memset, one kernel) against mimi_ld_pool_feed (the loudness meter's energies) on the same clips.
            --only-true-peak runs these two alone.
Kernel times proper come from a kernel trace of this tool with --skip-live, in a run of its own (docs/experiments/limiter.md).

    python tools/limiter_bench.py --out profiles/limiter/limiter.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "sesameai-tts_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import leveler_bench  # noqa: E402
from loudness_bench import speechlike, stats  # noqa: E402

H = 2400
TILE = 4096
HBM_BYTES_PER_S = 8.0e12                  # MI355X: HBM3E peak


def pair(N, n, final, drive_shift):
    """-> a function that times ONE levelling call and ONE limiting call of N streams x n samples between HIP events"""
    from sesameai import _abi
    from sesameai.limiter import Limit, LimiterPool
    from sesameai.loudness import Level, LoudnessPool
    lev, lim = LoudnessPool(N), LimiterPool(N)
    lev.level_reset(range(N), Level(-19.0))
    limit = Limit(drive_shift=drive_shift)
    lim.reset(range(N), limit)
    packed = torch.from_numpy(np.concatenate([speechlike(n, 40 + i) for i in range(N)])).cuda()
    out = torch.empty(N * n + 16, dtype=packed.dtype, device="cuda")
    ids = (C.c_int32 * N)(*range(N))
    offs, lens = (C.c_long * N)(*[i * n for i in range(N)]), (C.c_long * N)(*[n] * N)
    fin, n_h, n_out = (C.c_int32 * N)(*[int(final)] * N), (C.c_long * N)(), (C.c_long * N)()
    hops_max = N * (n // H + 1)
    energy = torch.empty(hops_max, dtype=torch.int64, device="cuda")
    gain = torch.empty(hops_max + 2 * N, dtype=torch.int32, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if not final:                             # open streams: the look-ahead is held from here on
        assert _abi.lib.mimi_lim_pool_feed(lim._h, ids, offs, lens, fin, N, packed.data_ptr(), out.data_ptr(), n_out, 0,
                                           torch.cuda.current_stream().cuda_stream) == 0

    def run(limiting):
        s = torch.cuda.current_stream().cuda_stream
        e0.record()
        if limiting:
            rc = _abi.lib.mimi_lim_pool_feed(lim._h, ids, offs, lens, fin, N, packed.data_ptr(), out.data_ptr(), n_out, 0, s)
        else:
            rc = _abi.lib.mimi_ld_pool_level_feed(lev._h, ids, offs, lens, fin, N, packed.data_ptr(), 0, out.data_ptr(), energy.data_ptr(),
                                                  gain.data_ptr(), n_h, s)
        e1.record()
        assert rc == 0
        e1.synchronize()
        return e0.elapsed_time(e1)

    def limited():
        return [int(v) for v in lim.state(range(N)).cpu()[:, 2].tolist()], limit.params()
    return run, limited


def min_passes(L):
    """passes of k_lim_apply's step 3: the window doubles while it can, then one pass joins two windows to L + 1"""
    span, passes = 1, 0
    while span < L + 1:
        span += min(span, L + 1 - span)
        passes += 1
    return passes


def pair_leg(N, n, final, drive_shift, rounds, warmup):
    run, limited = pair(N, n, final, drive_shift)
    t = {False: [], True: []}
    for r in range(warmup + rounds):
        for limiting in (False, True):
            ms = run(limiting)
            if r >= warmup:
                t[limiting].append(ms)
    counts, (_, L, rho, _) = limited()
    K = -(-65536 // rho)
    nbytes = N * n * 8
    med = statistics.median(t[True]) * 1e-3
    return {"streams": N, "samples_per_stream": n, "final": bool(final), "drive_shift": drive_shift, "lookahead": L, "rho": rho, "K": K,
            "samples_limited_per_stream_since_fresh": [min(counts), max(counts)],
            "level_gpu_ms": stats(t[False]), "limit_gpu_ms": stats(t[True]),
            "limit_over_level": statistics.median(t[True]) / statistics.median(t[False]),
            "bytes": nbytes, "limit_bytes_per_s": nbytes / med, "limit_fraction_of_hbm_peak": nbytes / med / HBM_BYTES_PER_S,
            "halo": {"tile": TILE, "staged_per_tile": TILE + K + 2 * L, "staged_over_tile": (TILE + K + 2 * L) / TILE,
                     "minimum_passes_over_staged": min_passes(L), "scan_passes_over_staged": 3}}


def shapes_leg(rounds, warmup):
    """64 clips x 10 s through the limiter alone at four (look-ahead, release) pairs, alternating: what the halo (K + 2 L staged beside a
    tile) and the minimum's passes (log2 of L + 1) add to a limiter that has next to neither"""
    from sesameai import _abi
    from sesameai.limiter import Limit, LimiterPool
    N, n = 64, 240000
    shapes = {"L=1 K=1": Limit(lookahead=1, release_ms=1.0 / 24, drive_shift=2), "L=120 K=1": Limit(lookahead=120, release_ms=1.0 / 24, drive_shift=2),
              "L=120 K=2428": Limit(drive_shift=2), "L=480 K=8192": Limit(lookahead=480, release_ms=1e9, drive_shift=2)}
    pool = LimiterPool(N)
    packed = torch.from_numpy(np.concatenate([speechlike(n, 40 + i) for i in range(N)])).cuda()
    out = torch.empty(N * n + 16, dtype=packed.dtype, device="cuda")
    ids, offs, lens = (C.c_int32 * N)(*range(N)), (C.c_long * N)(*[i * n for i in range(N)]), (C.c_long * N)(*[n] * N)
    fin, n_out = (C.c_int32 * N)(*[1] * N), (C.c_long * N)()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t = {k: [] for k in shapes}
    for r in range(warmup + rounds):
        for k, limit in shapes.items():
            pool.reset(range(N), limit)                                   # (host arithmetic)
            e0.record()
            rc = _abi.lib.mimi_lim_pool_feed(pool._h, ids, offs, lens, fin, N, packed.data_ptr(), out.data_ptr(), n_out, 0,
                                             torch.cuda.current_stream().cuda_stream)
            e1.record()
            assert rc == 0
            e1.synchronize()
            if r >= warmup:
                t[k].append(e0.elapsed_time(e1))
    res = {}
    for k, limit in shapes.items():
        _, L, rho, _ = limit.params()
        K = -(-65536 // rho)
        res[k] = {"gpu_ms": stats(t[k]), "staged_over_tile": (TILE + K + 2 * L) / TILE, "minimum_passes": min_passes(L),
                  "lds_bytes_per_workgroup": 4 * (2 * (TILE + K + 2 * L + 1) + TILE)}
    return res


def true_peak_leg(N, n, final, drive_shift, rounds, warmup, meter):
    """sample-peak against true-peak limiting of N streams x n samples, alternating; with ``meter`` also the stateless true-peak meter
    against the loudness meter's feed on the same clips"""
    from sesameai import _abi
    from sesameai.limiter import Limit, LimiterPool
    from sesameai.loudness import LoudnessPool
    lib = _abi.lib
    pools = {"sample": LimiterPool(N), "true_peak": LimiterPool(N)}
    pools["sample"].reset(range(N), Limit(drive_shift=drive_shift))
    pools["true_peak"].reset(range(N), Limit(drive_shift=drive_shift, true_peak=True))
    ld = LoudnessPool(N)
    packed = torch.from_numpy(np.concatenate([speechlike(n, 40 + i) for i in range(N)])).cuda()
    out = torch.empty(N * n + 16, dtype=packed.dtype, device="cuda")
    ids = (C.c_int32 * N)(*range(N))
    offs, lens = (C.c_long * N)(*[i * n for i in range(N)]), (C.c_long * N)(*[n] * N)
    fin, ones, n_out, n_h = (C.c_int32 * N)(*[int(final)] * N), (C.c_int32 * N)(*[1] * N), (C.c_long * N)(), (C.c_long * N)()
    energy = torch.empty(N * (n // H + 1), dtype=torch.int64, device="cuda")
    rows = torch.empty((N, 4), dtype=torch.int64, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if not final:                             # open streams: the latency is held from here on
        for pool in pools.values():
            assert lib.mimi_lim_pool_feed(pool._h, ids, offs, lens, fin, N, packed.data_ptr(), out.data_ptr(), n_out, 0,
                                          torch.cuda.current_stream().cuda_stream) == 0

    def run(leg):
        s = torch.cuda.current_stream().cuda_stream
        if leg == "ld_feed":
            assert lib.mimi_ld_pool_reset(ld._h, ids, N) == 0          # (host arithmetic, outside the clock)
        e0.record()
        if leg in pools:
            rc = lib.mimi_lim_pool_feed(pools[leg]._h, ids, offs, lens, fin, N, packed.data_ptr(), out.data_ptr(), n_out, 0, s)
        elif leg == "tp_measure":
            rc = lib.mimi_tp_measure(packed.data_ptr(), offs, lens, N, 0, rows.data_ptr(), s)
        else:
            rc = lib.mimi_ld_pool_feed(ld._h, ids, offs, lens, ones, N, packed.data_ptr(), 0, energy.data_ptr(), n_h, s)
        e1.record()
        assert rc == 0
        e1.synchronize()
        return e0.elapsed_time(e1)

    legs = ["sample", "true_peak"] + (["ld_feed", "tp_measure"] if meter else [])
    t = {k: [] for k in legs}
    for r in range(warmup + rounds):
        for k in legs:
            ms = run(k)
            if r >= warmup:
                t[k].append(ms)
    limited = {k: [int(v) for v in pool.state(range(N)).cpu()[:, 2].tolist()] for k, pool in pools.items()}
    res = {"streams": N, "samples_per_stream": n, "final": bool(final), "drive_shift": drive_shift,
           "samples_limited_per_stream_since_fresh": {k: [min(v), max(v)] for k, v in limited.items()},
           "sample_gpu_ms": stats(t["sample"]), "true_peak_gpu_ms": stats(t["true_peak"]),
           "true_peak_over_sample": statistics.median(t["true_peak"]) / statistics.median(t["sample"])}
    if meter:
        res.update({"ld_feed_gpu_ms": stats(t["ld_feed"]), "tp_measure_gpu_ms": stats(t["tp_measure"]),
                    "tp_measure_over_ld_feed": statistics.median(t["tp_measure"]) / statistics.median(t["ld_feed"]),
                    "true_peak_over_sample_peak_db": [float(20 * np.log10(max(r[1], 1) / max(r[0], 1))) for r in rows.cpu().tolist()][:4]})
    return res


def live_leg(rounds, warmup):
    """the leveler tool's own live leg with ``limiter=True`` in the place of its loudness target"""
    import time

    from sesameai.generator import Generator, Segment
    from sesameai.mimi import MimiArgs, MimiCodec, synthetic_state_dict as mimi_sd
    from sesameai.models import Model, csm_1b_args, synthetic_state_dict
    SLOTS, REQUESTS, TEMP, TOPK = leveler_bench.SLOTS, leveler_bench.REQUESTS, leveler_bench.TEMP, leveler_bench.TOPK
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

    legs = {"limiter": {"limiter": True}, "none": {}}
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
            "limiter_over_none_frames_per_s": statistics.median(fps["limiter"]) / statistics.median(fps["none"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--live-rounds", type=int, default=3)
    ap.add_argument("--skip-live", action="store_true")
    ap.add_argument("--only-true-peak", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("limiter_bench: needs a GPU (there is nothing to measure without one)")
    res = {"command": "python tools/limiter_bench.py " + " ".join(sys.argv[1:]), "device": torch.cuda.get_device_name(0),
           "what": "gpu_ms: between HIP events, medians over alternating rounds after warm-up; frames_per_s: host clock up to a synchronise",
           "rounds": args.rounds, "warmup": args.warmup}
    if not args.only_true_peak:
        res["feed"] = pair_leg(32, 19200, False, 2, args.rounds, args.warmup)
        print(json.dumps({"feed": res["feed"]}), flush=True)
        res["clips"] = pair_leg(64, 240000, True, 2, args.rounds, args.warmup)
        print(json.dumps({"clips": res["clips"]}), flush=True)
        res["shapes"] = shapes_leg(args.rounds, args.warmup)
        print(json.dumps({"shapes": res["shapes"]}), flush=True)
    # drive_shift 2, as the legs above: samples of 2^15 and more, the 64-bit taps; drive_shift 0: int16 pairs
    res["true_peak"] = {"feed": true_peak_leg(32, 19200, False, 2, args.rounds, args.warmup, False),
                        "clips": true_peak_leg(64, 240000, True, 2, args.rounds, args.warmup, True),
                        "feed_narrow": true_peak_leg(32, 19200, False, 0, args.rounds, args.warmup, False),
                        "clips_narrow": true_peak_leg(64, 240000, True, 0, args.rounds, args.warmup, False)}
    print(json.dumps({"true_peak": res["true_peak"]}), flush=True)
    if not args.skip_live and not args.only_true_peak:
        res["live"] = live_leg(args.live_rounds, 1)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
