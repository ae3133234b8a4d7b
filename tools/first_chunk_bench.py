#!/usr/bin/env python3
"""Time to first audio in the live batch on an MI355X: ``generate_many_stream`` with ``first_chunk_frames`` = None / 2 / 4.

Full-size model and codec (synthetic weights).  96 requests of one registered voice (a 1,294-row prefix in the prefix store + a 40-row
suffix of their own) through 32 slots, seeds of their own (the same codes for every setting), limits of 40..80 frames, sampled 0.9 / 50.
Per request: host-clock time from the moment the scheduler gives it its slot (its refill's last call has returned: live_batch.py makes its
_Utterance) to the moment its first chunk's PCM is in host memory.  Per run: the frames of all requests per second of wall time -- what
the shorter blocks' extra read_frames waits cost.  The settings alternate run by run in one process after one untimed run of each.

    python tools/first_chunk_bench.py --out profiles/pool_ragged/first_chunk.json
"""
import argparse
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

from prefix_bench import PREFIX, SUFFIX, prompt  # noqa: E402

REQUESTS, SLOTS = 96, 32
SETTINGS = (None, 2, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("first_chunk_bench: needs a GPU (there is nothing to measure without one)")
    from sesameai import live_batch
    from sesameai.generator import Generator
    from sesameai.mimi import MimiArgs, MimiCodec, synthetic_state_dict as mimi_sd
    from sesameai.models import Model, csm_1b_args, synthetic_state_dict
    codec = MimiCodec(MimiArgs(), mimi_sd(MimiArgs(), seed=4321, encoder=False), max_frames=32)
    m = Model(csm_1b_args(), synthetic_state_dict(csm_1b_args(), seed=1234), max_frames=128, max_prefill_rows=2048)
    gen = Generator(m, audio_tokenizer=codec, max_batch_size=SLOTS)
    m.seed(7)
    tok, msk = prompt()
    g = torch.Generator().manual_seed(3)
    reqs = []
    for i in range(REQUESTS):
        t = tok.clone()
        t[PREFIX:, 32] = torch.randint(0, 128_256, (SUFFIX,), generator=g).cuda()
        reqs.append((t, msk))
    limits = [40 + (i * 13) % 41 for i in range(REQUESTS)]
    seeds = [5000 + i for i in range(REQUESTS)]
    handle = gen.cache_prefix(tok[:PREFIX], msk[:PREFIX])
    gen._build_prompts = lambda texts, speakers, contexts: reqs         # the requests are prompts already

    # the moment a request gets its slot: the scheduler makes its _Utterance
    given = {}

    class Stamped(live_batch._Utterance):
        def __init__(self, index, *rest, **kw):
            super().__init__(index, *rest, **kw)
            given[index] = time.perf_counter()
    live_batch._Utterance = Stamped

    def run(k):
        given.clear()
        first, frames, sizes = {}, 0, {}
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for i, pcm, fr, last in gen.generate_many_stream([0] * REQUESTS, [0] * REQUESTS, [[]] * REQUESTS, max_audio_length_ms=[n * 80 for n in limits],
                                                         temperature=0.9, topk=50, seed=seeds, first_chunk_frames=k):
            frames += fr.shape[0]
            if i not in first and fr.shape[0]:
                host = pcm.cpu()                                       # (the side stream is synchronised already; this is the copy)
                first[i] = time.perf_counter() - given[i]
                sizes[i] = fr.shape[0]
                del host
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        ms = sorted(1e3 * v for v in first.values())
        return {"first_audio_ms_median": statistics.median(ms), "first_audio_ms_worst": ms[-1], "first_audio_ms_best": ms[0],
                "first_chunk_frames_median": statistics.median(sizes.values()), "frames": frames, "frames_per_s": frames / wall, "requests_with_audio": len(ms)}

    runs = {str(k): [] for k in SETTINGS}
    for r in range(a.rounds + 1):
        for k in SETTINGS:                                              # alternating; round 0 warms every shape and is dropped
            v = run(k)
            if r:
                runs[str(k)].append(v)
                print(json.dumps({"first_chunk_frames": k, **v}), flush=True)
    gen.drop_prefix(handle)
    res = {"command": "python tools/first_chunk_bench.py " + " ".join(sys.argv[1:]), "device": torch.cuda.get_device_name(0),
           "requests": REQUESTS, "slots": SLOTS, "prompt_rows": PREFIX + SUFFIX, "prefix_rows": PREFIX, "limits": "40..80 frames", "sampling": "0.9 / 50, own seeds",
           "rounds": a.rounds, "runs": runs,
           "summary": {k: {name: {"median_of_runs": statistics.median(x[name] for x in v), "min": min(x[name] for x in v), "max": max(x[name] for x in v)}
                           for name in ("first_audio_ms_median", "first_audio_ms_worst", "frames_per_s")} for k, v in runs.items()}}
    print(json.dumps(res["summary"]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
