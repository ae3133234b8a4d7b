#!/usr/bin/env python3
"""Mimi encode streams on an MI355X (mimi_enc_pool_encode): what one pool call costs, what streaming a turn buys on the response path and
what it costs in total, and whether the kernels the pool shares with the rest of the codec kept their times.

Full-size codec (synthetic weights), 10-frame chunks.  Times are GPU ms between HIP events on the launching stream; the ways that are
compared alternate round by round in one process after warm-up rounds of both; medians, with min and max beside them.

  pool_call     one pool call for N = 1 / 8 / 32 streams x 10 frames
  turns         a 3 s and a 10 s turn: "last sample -> codes ready" is the FINAL pool call (what is left when the turn ends, its earlier
                chunks having been encoded as they arrived) against the whole-clip mimi_encode of the turn; "total" is every pool call of the
                turn against that one encode.  The streamed codes are compared with the whole-clip codes first (bit-identical).
  shared        mimi_encode (3 s), mimi_encode_many (four clips) and the decode pool's uniform call (32 x 10): the launches whose kernels the
                encode pool instantiates anew.  With --parent-lib PATH this leg runs in child processes, alternating the library named (a build
                of the parent commit) and this build, twice each: the parent's own two repeats give the spread a difference has to pass.

    python tools/enc_stream_bench.py --out profiles/enc_stream/enc_stream.json [--parent-lib /path/to/parent/libcsm_hip.so]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "sesameai-tts_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

CHUNK, HOP, RATE = 10, 1920, 24000


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(v):
    return {"median": statistics.median(v), "mean": statistics.fmean(v), "min": min(v), "max": max(v), "n": len(v)}


def clip(seed, n, dev):
    return (torch.randn(n, generator=torch.Generator().manual_seed(seed)) * 0.3).to(dev)


def new_codec(max_frames):
    from sesameai.mimi import MimiArgs, MimiCodec, synthetic_state_dict
    return MimiCodec(MimiArgs(), synthetic_state_dict(MimiArgs(), seed=4321), max_frames=max_frames)


def pool_call_leg(codec, rounds, warmup):
    out = []
    for N in (1, 8, 32):
        pool = codec.open_encode_streams(N, max_chunk_frames=CHUNK)
        wavs = [clip(700 + i, CHUNK * HOP, codec.device) for i in range(N)]
        ids = list(range(N))
        t = [timed(lambda: pool.encode(ids, wavs)) for _ in range(warmup + rounds)][warmup:]
        out.append({"streams": N, "chunk_frames": CHUNK, "pool_call_ms": stats(t)})
        del pool
    return out


def turns_leg(codec, rounds, warmup):
    out = []
    for seconds in (3, 10):
        n = seconds * RATE
        x = clip(800 + seconds, n, codec.device)
        pool = codec.open_encode_streams(1, max_chunk_frames=CHUNK)
        step = CHUNK * HOP
        n_whole = (n - 1) // step                                   # chunks encoded while the turn is spoken; the rest waits for its end
        pieces = [x[k * step:(k + 1) * step] for k in range(n_whole)] + [x[n_whole * step:]]
        want = codec.encode(x.view(1, 1, -1))[0]
        res = {}

        def whole():
            res["whole"] = codec.encode(x.view(1, 1, -1))

        t_last, t_total, t_whole, same = [], [], [], True
        for r in range(warmup + rounds):
            pool.reset()
            torch.cuda.synchronize()
            got, ts = [], []
            for pc in pieces:
                ts.append(timed(lambda: got.extend(pool.encode([0], [pc]))))
            w = timed(whole)
            same = same and torch.equal(torch.cat(got, dim=1), want)
            if r >= warmup:
                t_last.append(ts[-1]); t_total.append(sum(ts)); t_whole.append(w)
        out.append({"turn_seconds": seconds, "samples": n, "frames": int(want.shape[1]), "pool_calls": len(pieces),
                    "frames_in_the_final_call": -(-int(pieces[-1].shape[0]) // HOP), "codes_bit_identical": bool(same),
                    "last_sample_to_codes_ms": {"final_pool_call": stats(t_last), "whole_clip_mimi_encode": stats(t_whole)},
                    "total_gpu_ms_per_turn": {"all_pool_calls": stats(t_total), "whole_clip_mimi_encode": stats(t_whole)},
                    "whole_over_final_call": statistics.median(t_whole) / statistics.median(t_last),
                    "streamed_total_over_whole": statistics.median(t_total) / statistics.median(t_whole)})
    return out


def shared_leg(codec, rounds, warmup):
    dev = codec.device
    x3 = clip(900, 3 * RATE, dev).view(1, 1, -1)
    many = [clip(901 + i, n, dev) for i, n in enumerate((3 * RATE, RATE, 2 * RATE + 777, 5 * HOP))]
    dpool = codec.open_streams(32, max_chunk_frames=CHUNK)
    codes = torch.randint(0, 2048, (32, 32, CHUNK), generator=torch.Generator().manual_seed(9)).to(device=dev, dtype=torch.int32)
    ids = list(range(32))
    ways = {"mimi_encode_3s": lambda: codec.encode(x3), "mimi_encode_many_4_clips": lambda: codec.encode_many(many),
            "mimi_pool_decode_32x10": lambda: dpool.decode(ids, codes)}
    t = {k: [] for k in ways}
    for r in range(warmup + rounds):
        for k, fn in ways.items():                                  # the three alternate round by round
            v = timed(fn)
            if r >= warmup:
                t[k].append(v)
    return {k: stats(v) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--leg", choices=("all", "shared"), default="all")
    ap.add_argument("--parent-lib", default=None, help="libcsm_hip.so built from the parent commit: the `shared` leg then alternates it with this build")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("enc_stream_bench: needs a GPU (there is nothing to measure without one)")
    if args.leg == "shared":
        print(json.dumps(shared_leg(new_codec(160), args.rounds, args.warmup)))
        return
    codec = new_codec(160)
    res = {"command": "python tools/enc_stream_bench.py " + " ".join(sys.argv[1:]), "device": torch.cuda.get_device_name(0),
           "what": "GPU ms between HIP events; medians over alternating rounds", "rounds": args.rounds, "warmup": args.warmup}
    res["pool_call"] = pool_call_leg(codec, args.rounds, args.warmup)
    print(json.dumps(res["pool_call"]), flush=True)
    res["turns"] = turns_leg(codec, args.rounds, args.warmup)
    print(json.dumps(res["turns"]), flush=True)
    if args.parent_lib:
        del codec
        torch.cuda.synchronize()
        runs = []
        for which in ("parent", "this", "parent", "this"):          # fresh child processes, one at a time
            env = dict(os.environ)
            env.pop("CSM_HIP_LIB", None)
            if which == "parent":
                env["CSM_HIP_LIB"] = os.path.abspath(args.parent_lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", "shared", "--rounds", str(args.rounds), "--warmup", str(args.warmup)],
                               env=env, capture_output=True, text=True, timeout=400)
            if r.returncode != 0:
                sys.exit(f"enc_stream_bench: the `shared` leg on the {which} build failed ({r.returncode}):\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
            runs.append({"build": which, **json.loads(r.stdout.strip().splitlines()[-1])})
            print(json.dumps(runs[-1]), flush=True)
        keys = [k for k in runs[0] if k != "build"]
        res["shared_kernels_parent_vs_this"] = {"runs": runs, "median_ms": {
            k: {"parent": [r[k]["median"] for r in runs if r["build"] == "parent"], "this": [r[k]["median"] for r in runs if r["build"] == "this"]} for k in keys}}
    else:
        res["shared_kernels_this_build"] = shared_leg(codec, args.rounds, args.warmup)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
