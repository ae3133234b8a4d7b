#!/usr/bin/env python3
"""The prefix store on an MI355X: what copying a voice prompt's K/V costs, and what it saves the continuously refilled batch.

Full-size model (synthetic weights), 1,334-row prompts = a 1,294-row voice prefix + a 40-row suffix.  GPU times are taken between
HIP events on the launching stream, the two ways alternate round by round in one process after a warm-up round of both, and the
medians are reported.

  apply        csm_prefix_apply for n = 1, 8, 32 slots (ms, GB/s written) against the same bytes moved run by run: one device copy
               per (layer, K|V, kv head, slot) run through torch's ``copy_``, which issues one hipMemcpyAsync for a contiguous run
  initial_fill 32 slots filled with whole prompts (what the loop did before) against one apply + 32 suffix refills
  refill       B = 32, one slot retired: frame steps until the new utterance's frame 0, and ms per step while the refill runs,
               at the default budget (refill_row_layers = 600), whole prompt against apply + suffix
  throughput   generate_codes_continuous, 64 requests of one voice, 8 slots, limits 40..80 frames: frames per second of wall time

    python tools/prefix_bench.py --out profiles/r08/prefix_store.json
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

PREFIX, SUFFIX = 1294, 40
BUDGET = 600


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def med(xs):
    return round(statistics.median(xs), 4)


def prompt():
    import bench
    from types import SimpleNamespace
    a = SimpleNamespace(ctx_text=40, ctx_frames=125, gen_text=24)
    t, m = bench.synthetic_prompt(a, 1, 128_256, seed0=5000, segments=10, ctx_text=30, ctx_frames=100)
    assert t.shape[1] == PREFIX + SUFFIX
    return t[0].cuda(), m[0].cuda()


def whole_refill(m, slot, tok, msk):
    m.refill_begin(slot, tok, msk)
    while not m.refill_advance(16):
        pass


def suffix_refill(m, slot, tok, msk):
    m.refill_begin(slot, tok[PREFIX:], msk[PREFIX:], start=PREFIX)
    while not m.refill_advance(16):
        pass


def bench_apply(m, pf, rounds):
    """The kernel against per-run device copies into a buffer of the caches' layout (the caches themselves are the engine's)."""
    L, KV, hd, smax, B = m.bb.num_layers, m.bb.num_kv_heads, m.bb.head_dim, m.bb.max_seq_len, m._max_batch
    snap = pf.read().cuda()                                        # [L][2][KV][rows][hd]
    cache = torch.empty(2, L, B, KV, smax, hd, dtype=torch.bfloat16, device="cuda")
    out = {}
    for n in (1, 8, 32):
        slots = list(range(n))

        def by_memcpy():
            for l in range(L):
                for w in range(2):
                    for h in range(KV):
                        src = snap[l, w, h]
                        for s_ in slots:
                            cache[w, l, s_, h, :pf.rows].copy_(src)
        ker, cpy = [], []
        for r in range(rounds + 1):
            a = timed(lambda: m.apply_prefix(pf, slots))
            b = timed(by_memcpy)
            if r:
                ker.append(a); cpy.append(b)
        gb = pf.bytes * n / 1e9
        out[f"n{n}"] = dict(bytes_written=pf.bytes * n, kernel_ms=med(ker), kernel_gbps=round(gb / (med(ker) / 1e3), 1),
                            memcpy_per_run_ms=med(cpy), memcpy_per_run_gbps=round(gb / (med(cpy) / 1e3), 1), copies=L * 2 * KV * n)
    return out


def bench_fill(m, pf, tok, msk, rounds):
    B = m._max_batch
    whole, store = [], []

    def fill_whole():
        for s_ in range(B):
            whole_refill(m, s_, tok, msk)

    def fill_store():
        m.apply_prefix(pf, list(range(B)))
        for s_ in range(B):
            suffix_refill(m, s_, tok, msk)
    for r in range(rounds + 1):
        m.reset_caches(); a = timed(fill_whole)
        m.reset_caches(); b = timed(fill_store)
        if r:
            whole.append(a); store.append(b)
    return dict(slots=B, whole_prompts_ms=med(whole), apply_plus_suffixes_ms=med(store))


def bench_refill(m, pf, tok, msk, rounds):
    """One retired slot of a live B = 32 batch, the generator's own schedule: after each frame step up to BUDGET // rows layers."""
    B, L = m._max_batch, m.bb.num_layers
    m.reset_caches()
    m.apply_prefix(pf, list(range(B)))
    for s_ in range(B):
        suffix_refill(m, s_, tok, msk)
    for _ in range(8):
        m.step(B, 0.9, 50)
    plain = [timed(lambda: m.step(B, 0.9, 50)) for _ in range(20)]

    def one(store):
        m.reset_slots([5])
        steps, ms = 0, []
        rows = SUFFIX if store else PREFIX + SUFFIX
        per_call = max(1, min(BUDGET // rows, L))
        state = {"begun": False, "done": False}

        def step_and_feed():
            m.step(B, 0.9, 50)
            if not state["begun"]:
                if store:
                    m.apply_prefix(pf, [5])
                    m.refill_begin(5, tok[PREFIX:], msk[PREFIX:], start=PREFIX)
                else:
                    m.refill_begin(5, tok, msk)
                state["begun"] = True
            state["done"] = m.refill_advance(per_call)
        while not state["done"]:
            ms.append(timed(step_and_feed)); steps += 1
        m.step(B, 0.9, 50)                                           # this step samples the new utterance's frame 0
        return steps + 1, ms
    res = {"whole": ([], []), "store": ([], [])}
    for r in range(rounds + 1):
        for key, store in (("whole", False), ("store", True)):
            steps, ms = one(store)
            if r:
                res[key][0].append(steps); res[key][1].extend(ms)
    m.read_frames(B, max(m.num_frames() - 1, 0), 1)                   # (raises if anything went wrong on the way)
    return dict(step_ms_no_refill=med(plain),
                whole_prompt=dict(steps_to_frame0=int(statistics.median(res["whole"][0])), step_ms_while_refilling=med(res["whole"][1])),
                apply_plus_suffix=dict(steps_to_frame0=int(statistics.median(res["store"][0])), step_ms_while_refilling=med(res["store"][1])))


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

    def run():
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = gen.generate_codes_continuous(reqs, limits, 0.9, 50)
        torch.cuda.synchronize()
        return sum(o.shape[0] for o in out) / (time.perf_counter() - t0)
    whole, store = [], []
    for r in range(rounds + 1):
        a = run()
        h = gen.cache_prefix(tok[:PREFIX], msk[:PREFIX])
        b = run()
        gen.drop_prefix(h)
        if r:
            whole.append(a); store.append(b)
    return dict(requests=64, slots=8, limits="40..80 frames", frames_per_s_whole_prompts=round(statistics.median(whole), 1),
                frames_per_s_with_store=round(statistics.median(store), 1))


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
    res = dict(device=torch.cuda.get_device_name(0), prompt_rows=PREFIX + SUFFIX, prefix_rows=PREFIX, prefix_bytes=pf.bytes, rounds=a.rounds)
    res["apply"] = bench_apply(m, pf, a.rounds)
    print(json.dumps({"apply": res["apply"]}), flush=True)
    res["initial_fill"] = bench_fill(m, pf, tok, msk, a.rounds)
    print(json.dumps({"initial_fill": res["initial_fill"]}), flush=True)
    res["refill_beside_the_loop_b32"] = bench_refill(m, pf, tok, msk, a.rounds)
    print(json.dumps({"refill": res["refill_beside_the_loop_b32"]}), flush=True)
    res["describe"] = m.describe()
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
