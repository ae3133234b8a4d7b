#!/usr/bin/env python3
"""Conversation sessions on an MI355X: what carrying a dialogue's K/V in pages costs, and what it saves a turn.

Full-size model (CSM-1B shapes, seeded weights).  A conversation has grown to 1,334 rows; the next turn adds 40 (the last reply's closing
rows, the user's segment, the reply's text): a cold prompt of 1,374 rows against a load of 1,334 and a prefill of 40.  Every figure is the
median over ``--rounds`` rounds after one warm-up round, with the smallest and largest beside it; the two ways alternate inside each round.

  copies   GPU time between HIP events of ONE load of the 1,334 rows into 1 slot and into 8 slots (8 sessions, one launch), of ONE save of
           a turn's 52 new rows (40 prompt rows + 12 frames) and of a first save of all 1,334 -- for pages of 32, 64 and 128 rows; GB/s
           counts the bytes written.  Beside them csm_prefix_apply of the same rows (the dense snapshot's copy).
  b1       host time from ``reset_caches`` to frame 0 on the host at batch 1 (load + suffix prefill + depth pass + read) against the cold
           prompt (nothing reused: another conversation held the slot in between) and against today's previous-prompt reuse (the slot
           still holds this conversation's last PROMPT: the 12 generated frames and the new rows run)
  b32      a live batch of 32, one slot retired: frame steps and host time from the begin call to the step that samples the new
           utterance's frame 0, refill beside the loop at the default budget, session (load + 40 rows) against the cold 1,374 rows

    python tools/session_bench.py --out profiles/sessions/sessions.json
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

HELD, NEW, FRAMES = 1334, 40, 12
BUDGET = 600


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def wall(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def stat(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4), n=len(xs))


def prompt():
    import bench
    from types import SimpleNamespace
    a = SimpleNamespace(ctx_text=40, ctx_frames=125, gen_text=24)
    t, m = bench.synthetic_prompt(a, 1, 128_256, seed0=5000, segments=10, ctx_text=30, ctx_frames=100)
    assert t.shape[1] == HELD
    g = torch.Generator().manual_seed(11)
    nt = torch.zeros(NEW, 33, dtype=t.dtype); nm = torch.zeros(NEW, 33, dtype=torch.bool)
    nt[:, 32] = torch.randint(0, 128_256, (NEW,), generator=g); nm[:, 32] = True
    return torch.cat([t[0], nt]).cuda(), torch.cat([m[0], nm]).cuda()


def bench_copies(sd, tok, msk, page_rows, rounds):
    from sesameai.models import Model, csm_1b_args
    m = Model(csm_1b_args(), sd, max_frames=16, max_prefill_rows=2048)
    m.setup_caches(8)
    m.reset_caches()
    m.refill_slot(0, tok, msk, 1.0, 1)                               # slot 0 holds 1,374 rows
    pages = (HELD + NEW + FRAMES + page_rows - 1) // page_rows
    m.open_session_store(8 * pages + 8, page_rows)
    ss = [m.open_session() for _ in range(8)]
    for s in ss:
        m.save_session(s, 0, HELD)
    pf = m.capture_prefix(0, HELD)
    row_bytes = pf.bytes // HELD
    res = {k: [] for k in ("load_1", "load_8", "save_turn", "save_all", "prefix_apply_1", "prefix_apply_8")}
    for r in range(rounds + 1):
        got = dict(load_1=timed(lambda: m.load_sessions(ss[:1], [1])), prefix_apply_1=timed(lambda: m.apply_prefix(pf, [1])),
                   load_8=timed(lambda: m.load_sessions(ss, list(range(8)))), prefix_apply_8=timed(lambda: m.apply_prefix(pf, list(range(8)))),
                   save_turn=timed(lambda: m.save_session(ss[0], 0, HELD + NEW + FRAMES)))
        ss[0].truncate(0)
        got["save_all"] = timed(lambda: m.save_session(ss[0], 0, HELD))
        if r:
            for k, v in got.items():
                res[k].append(v)
    rows = dict(load_1=HELD, load_8=8 * HELD, save_turn=NEW + FRAMES, save_all=HELD, prefix_apply_1=HELD, prefix_apply_8=8 * HELD)
    out = {k: dict(ms=stat(v), bytes_written=rows[k] * row_bytes, gbps=round(rows[k] * row_bytes / 1e9 / (statistics.median(v) / 1e3), 1)) for k, v in res.items()}
    out["pages_per_session"], out["page_bytes"], out["describe"] = ss[1].pages, page_rows * row_bytes, m.describe().split("session_store=")[1].split(";")[0]
    return out


def bench_b1(m, s, tok, msk, rounds):
    S = tok.shape[0]
    t3, m3 = tok.unsqueeze(0), msk.unsqueeze(0)
    prev_t, prev_m = tok[:HELD - FRAMES].unsqueeze(0), msk[:HELD - FRAMES].unsqueeze(0)      # the last turn's PROMPT: what today's reuse finds in slot 0

    def frame0():
        m.depth(1, 0.9, 50, commit=True)
        m.read_frames(1, 0, 1)

    def session():
        m.reset_caches()
        m.load_sessions([s], [0])
        m.prefill_prompt(t3, m3, start=HELD)
        frame0()

    def cold():
        m.reset_caches()
        m._kv_prompt = None
        m.prefill_prompt(t3, m3)
        frame0()

    def reuse():
        m.reset_caches()
        m.prefill_prompt(t3, m3)
        frame0()
    res = {"session": [], "cold": [], "previous_prompt_reuse": []}
    for r in range(rounds + 1):
        a = wall(session)
        b = wall(cold)
        m.reset_caches(); m._kv_prompt = None; m.prefill_prompt(prev_t, prev_m); torch.cuda.synchronize()
        c = wall(reuse)
        assert m.last_prefill_rows == S - (HELD - FRAMES)
        if r:
            res["session"].append(a); res["cold"].append(b); res["previous_prompt_reuse"].append(c)
    return dict(prompt_rows=S, rows_run=dict(session=S - HELD, cold=S, previous_prompt_reuse=S - (HELD - FRAMES)), ms_to_frame0={k: stat(v) for k, v in res.items()})


def bench_b32(m, s, tok, msk, rounds):
    B, L = m._max_batch, m.bb.num_layers
    S = tok.shape[0]
    m.reset_caches()
    for slot in range(B):
        m.load_sessions([s], [slot])
        m.refill_begin(slot, tok[HELD:], msk[HELD:], start=HELD)
        while not m.refill_advance(L):
            pass
    for _ in range(8):
        m.step(B, 0.9, 50)

    def one(session):
        m.reset_slots([5])
        m.step(B, 0.9, 50)
        rows = S - HELD if session else S
        per_call = max(1, min(BUDGET // rows, L))
        torch.cuda.synchronize(); t0 = time.perf_counter()
        if session:
            m.load_sessions([s], [5])
            m.refill_begin(5, tok[HELD:], msk[HELD:], start=HELD)
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
    res = {"session": ([], []), "cold": ([], [])}
    for r in range(rounds + 1):
        for key in ("session", "cold"):
            steps, ms = one(key == "session")
            if r:
                res[key][0].append(steps); res[key][1].append(ms)
    return {k: dict(steps_to_frame0=int(statistics.median(v[0])), ms_to_frame0=stat(v[1])) for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--page-rows", type=int, nargs="+", default=[32, 64, 128])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("session_bench needs a GPU: there is nothing to measure without one")
    from sesameai.models import Model, csm_1b_args, synthetic_state_dict
    sd = synthetic_state_dict(csm_1b_args(), seed=1234)
    tok, msk = prompt()
    res = dict(device=torch.cuda.get_device_name(0), held_rows=HELD, new_rows=NEW, rounds=a.rounds, copies={})
    for pr in a.page_rows:
        res["copies"][f"page_rows_{pr}"] = bench_copies(sd, tok, msk, pr, a.rounds)
        print(json.dumps({f"copies_{pr}": res["copies"][f"page_rows_{pr}"]}), flush=True)
    for B, fn, key in ((1, bench_b1, "b1"), (32, bench_b32, "b32")):
        m = Model(csm_1b_args(), sd, max_frames=64, max_prefill_rows=2048)
        m.setup_caches(B)
        m.seed(7)
        m.open_session_store(24, 64)
        m.reset_caches()
        m.refill_slot(0, tok[:HELD], msk[:HELD], 0.9, 50)
        s = m.open_session()
        m.save_session(s, 0, HELD)
        res[key] = fn(m, s, tok, msk, a.rounds)
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
