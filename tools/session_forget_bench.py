#!/usr/bin/env python3
"""Forgetting a session's oldest turns in place on an MI355X: what the one launch costs, and what it saves a turn whose window is full.

Full-size model (CSM-1B shapes, seeded weights, 64-row pages).  A conversation has grown to 1,334 rows; rows [190, 490) -- the oldest turns
after a 190-row voice prompt -- are forgotten, which rewrites the 906 rows from row 128 (the start of the cut's page) on into fresh pages;
the next turn adds 40 rows.  Every figure is the median over ``--rounds`` rounds after one warm-up round, with the smallest and largest
beside it; the ways compared alternate inside each round in one process.

  copies   GPU time between HIP events of ONE csm_session_forget, beside ONE csm_session_load of a session of as many rows as the forget
           rewrites (906), and their ratio; GB/s counts the bytes written
  b1       host time from the first call to frame 0 on the host at batch 1: forget + load + the 40-row suffix, against what a caller had
           to do before -- a new session, the trimmed 1,074-row history run cold
  b32      a live batch of 32, one slot retired: frame steps and host time to the step that samples the new utterance's frame 0, refill
           beside the loop at the default budget: forget + load + suffix against the cold trimmed history

    python tools/session_forget_bench.py --out profiles/session_forget/session_forget.json
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

HELD, A, B_, NEW, PAGE = 1334, 190, 490, 40, 64
KEPT = HELD - (B_ - A)                       # 1,034 rows after the forget
FIRST = A // PAGE * PAGE                     # 128: the first rewritten row
BUDGET = 600


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stat(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4), n=len(xs))


def prompts():
    """(the 1,334-row history, the trimmed history + the 40 new rows: 1,074 rows)."""
    import bench
    from types import SimpleNamespace
    a = SimpleNamespace(ctx_text=40, ctx_frames=125, gen_text=24)
    t, m = bench.synthetic_prompt(a, 1, 128_256, seed0=5000, segments=10, ctx_text=30, ctx_frames=100)
    assert t.shape[1] == HELD
    g = torch.Generator().manual_seed(11)
    nt = torch.zeros(NEW, 33, dtype=t.dtype); nm = torch.zeros(NEW, 33, dtype=torch.bool)
    nt[:, 32] = torch.randint(0, 128_256, (NEW,), generator=g); nm[:, 32] = True
    trimmed = torch.cat([t[0][:A], t[0][B_:], nt]).cuda(), torch.cat([m[0][:A], m[0][B_:], nm]).cuda()
    return (t[0].cuda(), m[0].cuda()), trimmed


def refresh(m, s):
    """The session holds HELD rows again (whatever slot 0 holds: only the time of the copies is measured)."""
    s.truncate(0)
    m.save_session(s, 0, HELD)
    torch.cuda.synchronize()


def bench_copies(m, s, rounds):
    ref = m.open_session()
    m.save_session(ref, 0, KEPT - FIRST)                            # as many rows as the forget rewrites
    row_bytes = m.bb.num_layers * 2 * m.bb.num_kv_heads * m.bb.head_dim * 2
    res = {"forget": [], "load_same_rows": []}
    for r in range(rounds + 1):
        refresh(m, s)
        a = timed(lambda: s.forget(A, B_))
        b = timed(lambda: m.load_sessions([ref], [1]))
        assert s.rows == KEPT
        if r:
            res["forget"].append(a); res["load_same_rows"].append(b)
    ref.close()
    nbytes = (KEPT - FIRST) * row_bytes
    out = {k: dict(ms=stat(v), rows=KEPT - FIRST, bytes_written=nbytes, gbps=round(nbytes / 1e9 / (statistics.median(v) / 1e3), 1)) for k, v in res.items()}
    out["forget_over_load"] = round(statistics.median(res["forget"]) / statistics.median(res["load_same_rows"]), 3)
    out["rows_moved_and_rotated"], out["rows_copied_verbatim"] = KEPT - A, A - FIRST
    out["fresh_pages"], out["describe"] = (KEPT + PAGE - 1) // PAGE - A // PAGE, m.describe().split("session_forgets=")[1].split(";")[0]
    return out


def bench_b1(m, s, trimmed, rounds):
    t3, m3 = trimmed[0].unsqueeze(0), trimmed[1].unsqueeze(0)

    def frame0():
        m.depth(1, 0.9, 50, commit=True)
        m.read_frames(1, 0, 1)

    def forget():
        s.forget(A, B_)
        m.reset_caches()
        m.load_sessions([s], [0])
        m.prefill_prompt(t3, m3, start=KEPT)
        frame0()

    def cold():
        m.reset_caches()
        m._kv_prompt = None
        m.prefill_prompt(t3, m3)
        frame0()
    res = {"forget_load_suffix": [], "new_session_cold": []}
    for r in range(rounds + 1):
        refresh(m, s)
        t0 = time.perf_counter(); forget(); a = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        t0 = time.perf_counter(); cold(); b = (time.perf_counter() - t0) * 1e3
        if r:
            res["forget_load_suffix"].append(a); res["new_session_cold"].append(b)
    S = trimmed[0].shape[0]
    return dict(prompt_rows=S, rows_run=dict(forget_load_suffix=S - KEPT, new_session_cold=S), ms_to_frame0={k: stat(v) for k, v in res.items()})


def bench_b32(m, s, full, trimmed, rounds):
    B, L = m._max_batch, m.bb.num_layers
    tok, msk = trimmed
    S = tok.shape[0]
    m.reset_caches()
    for slot in range(B):
        m.refill_begin(slot, *full)
        while not m.refill_advance(L):
            pass
    for _ in range(8):
        m.step(B, 0.9, 50)

    def one(session):
        m.reset_slots([5])
        m.step(B, 0.9, 50)
        if session:
            refresh(m, s)
        rows = S - KEPT if session else S
        per_call = max(1, min(BUDGET // rows, L))
        torch.cuda.synchronize(); t0 = time.perf_counter()
        if session:
            s.forget(A, B_)
            m.load_sessions([s], [5])
            m.refill_begin(5, tok[KEPT:], msk[KEPT:], start=KEPT)
        else:
            m.refill_begin(5, tok, msk)
        steps = 0
        while True:
            done = m.refill_advance(per_call)
            m.step(B, 0.9, 50); steps += 1
            if done:
                break
        m.read_frames(B, m.num_frames() - 1, 1)                        # the step that sampled frame 0 has run
        return steps, (time.perf_counter() - t0) * 1e3
    res = {"forget_load_suffix": ([], []), "new_session_cold": ([], [])}
    for r in range(rounds + 1):
        for key in res:
            steps, ms = one(key == "forget_load_suffix")
            if r:
                res[key][0].append(steps); res[key][1].append(ms)
    return {k: dict(steps_to_frame0=int(statistics.median(v[0])), ms_to_frame0=stat(v[1])) for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("session_forget_bench needs a GPU: there is nothing to measure without one")
    from sesameai.models import Model, csm_1b_args, synthetic_state_dict
    sd = synthetic_state_dict(csm_1b_args(), seed=1234)
    full, trimmed = prompts()
    res = dict(device=torch.cuda.get_device_name(0), held_rows=HELD, forgotten=[A, B_], new_rows=NEW, page_rows=PAGE, rounds=a.rounds)
    for B, key in ((2, "copies"), (1, "b1"), (32, "b32")):
        m = Model(csm_1b_args(), sd, max_frames=64, max_prefill_rows=2048)
        m.setup_caches(B)
        m.seed(7)
        m.open_session_store(64, PAGE)
        m.reset_caches()
        m.refill_slot(0, *full, 0.9, 50)
        s = m.open_session()
        m.save_session(s, 0, HELD)
        res[key] = bench_copies(m, s, a.rounds) if key == "copies" else bench_b1(m, s, trimmed, a.rounds) if key == "b1" else bench_b32(m, s, full, trimmed, a.rounds)
        print(json.dumps({key: res[key]}), flush=True)
        s.close()
        del m
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
