#!/usr/bin/env python3
"""Refilling several slots with one ragged prefill on an MI355X: what the group saves over one refill after the other.

Full-size model (synthetic weights), 1,334-row prompts = a 1,294-row voice prefix (copied: the prefix store) + a 40-row suffix.  GPU
times are taken between HIP events on the launching stream, the two ways alternate round by round in one process after a warm-up
round of both, and the medians are reported.  The baseline is one refill at a time (``refill_group=1``: csm_refill_begin).

  initial_fill 32 slots: one apply + 32 suffix refills one after the other, against one apply + ONE group of 32 suffixes
  refill       B = 32, k = 1, 4, 8 slots retired together: frame steps from retirement until the LAST of them has its frame 0, and
               ms per step while refilling, at the default budget (refill_row_layers = 600) with the scheduler's arithmetic
  throughput   generate_codes_continuous, 64 requests of one voice, 8 slots, limits 40..80 frames, sampled 0.9 / 50: frames per second
               of wall time for refill_group = 1, 4, 8

    python tools/group_refill_bench.py --out profiles/r09/group_refill.json
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

from prefix_bench import BUDGET, PREFIX, SUFFIX, med, prompt, suffix_refill, timed, whole_refill  # noqa: E402


def group_refill(m, slots, tok, msk):
    m.refill_group_begin(slots, [(tok[PREFIX:], msk[PREFIX:])] * len(slots), starts=[PREFIX] * len(slots))
    while not m.refill_group_advance(16):
        pass


def bench_fill(m, pf, tok, msk, rounds):
    B = m._max_batch
    one, grp = [], []

    def fill_one_by_one():
        m.apply_prefix(pf, list(range(B)))
        for s_ in range(B):
            suffix_refill(m, s_, tok, msk)

    def fill_group():
        m.apply_prefix(pf, list(range(B)))
        group_refill(m, list(range(B)), tok, msk)
    for r in range(rounds + 1):
        m.reset_caches(); a = timed(fill_one_by_one)
        m.reset_caches(); b = timed(fill_group)
        if r:
            one.append(a); grp.append(b)
    return dict(slots=B, suffix_rows=SUFFIX, one_by_one_ms=med(one), one_group_ms=med(grp))


def bench_refill(m, pf, tok, msk, rounds):
    """k retired slots of a live B = 32 batch on the scheduler's own schedule (live_batch.py): after each frame step one bounded piece of
    refill work, budget * (1 + slots still waiting) // rows layers per call."""
    B, L = m._max_batch, m.bb.num_layers
    m.reset_caches()
    m.apply_prefix(pf, list(range(B)))
    group_refill(m, list(range(B)), tok, msk)
    for _ in range(8):
        m.step(B, 0.9, 50)
    plain = [timed(lambda: m.step(B, 0.9, 50)) for _ in range(20)]
    suffix = (tok[PREFIX:], msk[PREFIX:])

    def one(k, grouped):
        retired = list(range(3, 3 + k))
        m.reset_slots(retired)
        free, ms, steps = list(retired), [], 0
        state = {"pending": None}                                    # (rows of the refill in flight, slots it fills)

        def step_and_feed():
            m.step(B, 0.9, 50)
            if state["pending"] is None:
                take = [free.pop(0) for _ in range(min(k if grouped else 1, len(free)))]
                m.apply_prefix(pf, take)
                if grouped:
                    m.refill_group_begin(take, [suffix] * len(take), starts=[PREFIX] * len(take))
                else:
                    m.refill_begin(take[0], *suffix, start=PREFIX)
                state["pending"] = SUFFIX * len(take)
            per_call = max(1, min(BUDGET * (1 + len(free)) // state["pending"], L))
            if (m.refill_group_advance if grouped else m.refill_advance)(per_call):
                state["pending"] = None
        while free or state["pending"] is not None:
            ms.append(timed(step_and_feed)); steps += 1
        m.step(B, 0.9, 50)                                           # this step samples the last new utterance's frame 0
        return steps + 1, ms
    out = dict(step_ms_no_refill=med(plain))
    for k in (1, 4, 8):
        res = {False: ([], []), True: ([], [])}
        for r in range(rounds + 1):
            for grouped in (False, True):
                steps, ms = one(k, grouped)
                if r:
                    res[grouped][0].append(steps); res[grouped][1].extend(ms)
        out[f"retired_{k}"] = {name: dict(steps_to_last_frame0=int(statistics.median(res[g][0])), step_ms_while_refilling=med(res[g][1]))
                               for name, g in (("one_by_one", False), ("one_group", True))}
    m.read_frames(B, max(m.num_frames() - 1, 0), 1)                   # (raises if anything went wrong on the way)
    return out


def bench_throughput(sd, tok, msk, rounds):
    from sesameai.generator import Generator
    from sesameai.models import Model, csm_1b_args
    m = Model(csm_1b_args(), sd, max_frames=128, max_prefill_rows=2048)
    gen = Generator(m, max_batch_size=8)
    m.seed(7)
    g = torch.Generator().manual_seed(3)
    reqs = []
    for i in range(64):
        t = tok.clone()
        t[PREFIX:, 32] = torch.randint(0, 128_256, (SUFFIX,), generator=g).cuda()
        reqs.append((t, msk))
    limits = [40 + (i * 13) % 41 for i in range(64)]
    h = gen.cache_prefix(tok[:PREFIX], msk[:PREFIX])

    def run(group):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = gen.generate_codes_continuous(reqs, limits, 0.9, 50, refill_group=group)
        torch.cuda.synchronize()
        return sum(o.shape[0] for o in out) / (time.perf_counter() - t0)
    res = {1: [], 4: [], 8: []}
    for r in range(rounds + 1):
        for group in res:
            v = run(group)
            if r:
                res[group].append(v)
    gen.drop_prefix(h)
    return dict(requests=64, slots=8, limits="40..80 frames", sampling="0.9 / 50",
                **{f"frames_per_s_refill_group_{k}": round(statistics.median(v), 1) for k, v in res.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    from sesameai.models import Model, csm_1b_args, synthetic_state_dict
    sd = synthetic_state_dict(csm_1b_args(), seed=1234)
    tok, msk = prompt()
    m = Model(csm_1b_args(), sd, max_frames=64, max_prefill_rows=2048)
    m.setup_caches(32)
    m.seed(7)
    m.reset_caches()
    whole_refill(m, 0, tok, msk)
    pf = m.capture_prefix(0, PREFIX)
    res = dict(device=torch.cuda.get_device_name(0), prompt_rows=PREFIX + SUFFIX, prefix_rows=PREFIX, rounds=a.rounds)
    res["initial_fill"] = bench_fill(m, pf, tok, msk, a.rounds)
    print(json.dumps({"initial_fill": res["initial_fill"]}), flush=True)
    res["refill_beside_the_loop_b32"] = bench_refill(m, pf, tok, msk, a.rounds)
    print(json.dumps({"refill": res["refill_beside_the_loop_b32"]}), flush=True)
    del pf, m
    res["throughput"] = bench_throughput(sd, tok, msk, max(a.rounds // 2, 1))
    print(json.dumps({"throughput": res["throughput"]}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
