#!/usr/bin/env python3
"""Multi-stream Mimi decode on an MI355X: one pool call for N streams (mimi_pool_decode) against the way the same work was done
before the pool existed -- N single-stream handles, each running one stateful 10-frame chunk decode (decode_stream) -- and what a
32-stream pool call per 10 frame steps on the side stream costs the B = 32 frame loop.  And the ragged call (mimi_pool_decode_ragged)
against the uniform calls it replaces: 32 streams of which 24 have a full chunk and 8 end with 1..8 frames -- one ragged call against one
uniform call of 24 plus eight calls of one -- and all 32 at 10 frames against the one uniform call (the price of the table lookup).

Full-size codec (synthetic weights), 10-frame chunks, N = 1, 8, 32.  Times are GPU times between HIP events on the launching
stream, per round (one pool call / N single-stream calls); the two ways alternate round by round in one process, after warm-up
rounds of both.  Before timing, the pool's PCM is compared with the handles' PCM on the same codes (it is bit-identical).

    python tools/mimi_streams_bench.py --out profiles/r07/mimi_streams.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "sesameai-tts_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

CHUNK = 10


class SingleStream:
    """One more single-stream handle on the codec's device weights (what a server without the pool would hold per caller)."""

    def __init__(self, codec, max_frames):
        from sesameai._abi import check, lib
        self.lib, self.check, self.hop, self.h = lib, check, codec.args.hop, C.c_void_p(None)
        cfg, w = codec._cfg_w
        check(lib.mimi_create(C.byref(cfg), C.byref(w), max_frames, 0, C.byref(self.h)), None, mimi=True)

    def reset(self):
        self.check(self.lib.mimi_reset_stream(self.h, torch.cuda.current_stream().cuda_stream), self.h, mimi=True)

    def decode_stream(self, codes, pcm):                       # codes (32, T) int32 device, pcm (hop*T,) fp32 device
        self.check(self.lib.mimi_decode_strided(self.h, codes.data_ptr(), 1, codes.shape[1], 0, codes.stride(0), codes.stride(1), pcm.data_ptr(), 1,
                                                torch.cuda.current_stream().cuda_stream), self.h, mimi=True)

    def close(self):
        self.lib.mimi_destroy(self.h)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def pool_vs_singles(codec, N, rounds, warmup, per_reset=4):
    dev = codec.device
    g = torch.Generator().manual_seed(100 + N)
    codes = torch.randint(0, 2048, (N, 32, CHUNK * per_reset), generator=g).to(device=dev, dtype=torch.int32)
    pool = codec.open_streams(N, max_chunk_frames=CHUNK)
    singles = [SingleStream(codec, CHUNK * per_reset) for _ in range(N)]
    ids = list(range(N))
    pcm1 = torch.empty(N, codec.args.hop * CHUNK, dtype=torch.float32, device=dev)
    out = {}

    def run_pool(k):
        out["pool"] = pool.decode(ids, codes[:, :, k * CHUNK:(k + 1) * CHUNK])

    def run_singles(k):
        for i, h in enumerate(singles):
            h.decode_stream(codes[i, :, k * CHUNK:(k + 1) * CHUNK], pcm1[i])

    t_pool, t_single, same = [], [], True
    for r in range(warmup + rounds):
        k = r % per_reset
        if k == 0:                                              # a single handle carries max_frames frames: start both ways afresh (untimed)
            pool.reset()
            for h in singles:
                h.reset()
            torch.cuda.synchronize()
        a, b = timed(lambda: run_pool(k)), timed(lambda: run_singles(k))
        same = same and torch.equal(out["pool"][:, 0], pcm1)
        if r >= warmup:
            t_pool.append(a); t_single.append(b)
    for h in singles:
        h.close()
    med = statistics.median
    return {"streams": N, "chunk_frames": CHUNK, "rounds": rounds,
            "pool_call_ms": {"median": med(t_pool), "mean": statistics.fmean(t_pool), "min": min(t_pool), "max": max(t_pool)},
            "single_stream_handles_ms": {"median": med(t_single), "mean": statistics.fmean(t_single), "min": min(t_single), "max": max(t_single)},
            "singles_over_pool": med(t_single) / med(t_pool), "pcm_bit_identical": bool(same)}


def timed_both(fn):
    """(GPU ms between HIP events, host ms the calls took to return) of fn()."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter(); fn(); t1 = time.perf_counter()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), (t1 - t0) * 1e3


def _stats(v):
    return {"median": statistics.median(v), "mean": statistics.fmean(v), "min": min(v), "max": max(v)}


def ragged_leg(codec, rounds, warmup, N=32):
    """One ragged call against the uniform calls it replaces, on twin pools (same codes, same schedule, PCM compared), alternating round by
    round after warm-up rounds of both.  `endings`: 24 streams x 10 frames and 8 streams with 1..8 frames; `all_full`: 32 x 10."""
    dev = codec.device
    codes = torch.randint(0, 2048, (N, 32, CHUNK), generator=torch.Generator().manual_seed(300 + N)).to(device=dev, dtype=torch.int32)
    ids = list(range(N))
    res = {"streams": N, "rounds": rounds}
    for name, lens in (("endings", [CHUNK] * (N - 8) + list(range(1, 9))), ("all_full", [CHUNK] * N)):
        rag_pool, uni_pool = codec.open_streams(N, max_chunk_frames=CHUNK), codec.open_streams(N, max_chunk_frames=CHUNK)
        groups = {}
        for i, T in enumerate(lens):
            groups.setdefault(T, []).append(i)
        out = {}

        def run_ragged():
            out["rag"] = rag_pool.decode_ragged(ids, codes, lens)

        def run_grouped():                                     # today's grouping: one uniform call per distinct length
            out["uni"] = {T: uni_pool.decode(g, codes[g[0]:g[-1] + 1, :, :T]) for T, g in sorted(groups.items(), reverse=True)}

        t = {"ragged_gpu": [], "ragged_host": [], "grouped_gpu": [], "grouped_host": []}
        same = True
        for r in range(warmup + rounds):
            a, b = timed_both(run_ragged), timed_both(run_grouped)
            same = same and all(torch.equal(out["rag"][i][0], out["uni"][T][g.index(i), 0]) for T, g in groups.items() for i in g)
            if r >= warmup:
                t["ragged_gpu"].append(a[0]); t["ragged_host"].append(a[1]); t["grouped_gpu"].append(b[0]); t["grouped_host"].append(b[1])
        res[name] = {"frames": lens, "uniform_calls_replaced": len(groups), "pcm_bit_identical": bool(same),
                     "one_ragged_call_gpu_ms": _stats(t["ragged_gpu"]), "one_ragged_call_host_ms": _stats(t["ragged_host"]),
                     "uniform_calls_gpu_ms": _stats(t["grouped_gpu"]), "uniform_calls_host_ms": _stats(t["grouped_host"]),
                     "uniform_over_ragged_gpu": statistics.median(t["grouped_gpu"]) / statistics.median(t["ragged_gpu"]),
                     "uniform_over_ragged_host": statistics.median(t["grouped_host"]) / statistics.median(t["ragged_host"])}
    return res


def frame_loop_leg(codec, steps, reps):
    """B = 32 frame steps of the 1B model with and without one 32-stream pool call per 10 steps on a side stream; ms per step."""
    import bench
    from sesameai.models import Model, csm_1b_args, synthetic_state_dict
    dev = codec.device
    margs = csm_1b_args()
    a = types.SimpleNamespace(ctx_text=40, ctx_frames=125, gen_text=24)
    B, T, K = 32, 0.9, 50
    tok, msk = bench.synthetic_prompt(a, B, margs.text_vocab_size, seed0=4000)
    S = tok.shape[1]
    m = Model(margs, synthetic_state_dict(margs, seed=1234), device=str(dev), max_frames=2 * reps * steps + 128, max_prefill_rows=B * S)
    m.setup_caches(B); m.seed(77)
    pos = torch.arange(S).unsqueeze(0).repeat(B, 1)
    m.reset_caches(); m.prefill(tok.to(dev), msk.to(dev), pos.to(dev)); m.depth(B, T, K, commit=True)
    pool = codec.open_streams(B, max_chunk_frames=CHUNK)
    codes = torch.randint(0, 2048, (B, 32, CHUNK), generator=torch.Generator().manual_seed(9)).to(device=dev, dtype=torch.int32)
    side = torch.cuda.Stream(device=dev)
    ids = list(range(B))
    for _ in range(10):
        m.step(B, T, K)
    with torch.cuda.stream(side):
        pool.decode(ids, codes)
    torch.cuda.synchronize()

    def with_decodes():
        st = torch.cuda.current_stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(st)
        for i in range(steps):
            m.step(B, T, K)
            if i % CHUNK == CHUNK - 1:                          # the block's steps are queued; the decode of the previous block runs beside them
                with torch.cuda.stream(side):
                    pool.decode(ids, codes)
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps

    plain, mixed = [], []
    for _ in range(reps):                                       # alternating
        plain.append(bench.timed_steps(m, B, steps, T, K))
        mixed.append(with_decodes())
    m.read_frames(B, m.num_frames() - 1, 1)                     # raises if a launch gave up
    return {"batch": B, "steps_per_rep": steps, "reps": reps, "prompt_rows": S,
            "step_ms_undisturbed": plain, "step_ms_with_a_32_stream_pool_call_per_10_steps": mixed,
            "median_undisturbed": statistics.median(plain), "median_with_decodes": statistics.median(mixed),
            "slowdown": statistics.median(mixed) / statistics.median(plain)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-frame-loop", action="store_true")
    ap.add_argument("--skip-ragged", action="store_true", help="(a library built before mimi_pool_decode_ragged, named by CSM_HIP_LIB, has no such leg)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mimi_streams_bench: needs a GPU (there is nothing to measure without one)")
    from sesameai.mimi import MimiArgs, MimiCodec, synthetic_state_dict
    codec = MimiCodec(MimiArgs(), synthetic_state_dict(MimiArgs(), seed=4321, encoder=False), max_frames=32)
    res = {"command": "python tools/mimi_streams_bench.py " + " ".join(sys.argv[1:]), "device": torch.cuda.get_device_name(0),
           "what": "GPU ms (HIP events) of one mimi_pool_decode of N streams x 10 frames vs N single-stream handles each running one stateful 10-frame decode",
           "pool_vs_singles": [pool_vs_singles(codec, N, args.rounds, args.warmup) for N in (1, 8, 32)]}
    print(json.dumps(res["pool_vs_singles"]), flush=True)
    if not args.skip_ragged:
        res["ragged_vs_uniform_calls"] = ragged_leg(codec, args.rounds, args.warmup)
        print(json.dumps(res["ragged_vs_uniform_calls"]), flush=True)
    if not args.skip_frame_loop:
        res["frame_loop_b32"] = frame_loop_leg(codec, args.steps, args.reps)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
