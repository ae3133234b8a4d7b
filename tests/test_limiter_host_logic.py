"""Host logic around the live limiter (no GPU): SlotStreams (sesameai/live_batch.py, through Generator.generate_many_stream) against
recording fake pools.  The fake limiter delays each stream by its look-ahead and scales it, as the real one delays; what is checked is the
bookkeeping: ``limiter=None`` makes today's calls and imports nothing; a slot is reset with its request's ``Limit``; ONE ``feed`` per pool
call, after the leveler and before the mark and the resampler, ``final`` travelling with the same chunk through every stage; a None
request never touches the pool; the look-ahead moves from a request's first chunk to its last, also to a closing chunk that is empty at
24 kHz; ``loudness=`` with ``limiter=`` hands both pools the pair of ``paired``; and ``Limit`` and ``paired`` against tests/limiter_ref.py
and tests/leveler_ref.py."""
import importlib
import math
import sys

import pytest
import torch

import leveler_ref as LR
import limiter_ref as R
import test_leveler_host_logic as H
from test_host_logic import _ScriptedSlots, _ScriptedSlotsBeside
from test_leveler_host_logic import EVENTS, LENS, SPEEDS, _FakeLeveler
from test_stretch_host_logic import LOOK
from test_watermark_host_logic import KEY

SCALE = 0.25


class _FakeLimiter:
    def __init__(self, n=3, device="cpu"):
        self.n_streams, self.calls, self.resets = n, [], []
        self._limit, self._held = [None] * n, [None] * n

    def reset(self, ids, limits):
        ids = [int(i) for i in ids]
        assert len(ids) == len(limits) >= 1
        self.resets.append(list(zip(ids, limits)))
        for i, lm in zip(ids, limits):
            self._limit[i], self._held[i] = lm, torch.empty(0)

    def feed(self, ids, chunks, final=False):
        ids = [int(i) for i in ids]
        fin = [bool(final)] * len(ids) if isinstance(final, bool) else [bool(f) for f in final]
        assert len(set(ids)) == len(ids) == len(chunks) == len(fin) >= 1 and all(0 <= i < self.n_streams for i in ids)
        assert all(self._held[i] is not None for i in ids), "a stream is fed only after its reset"
        self.calls.append([(i, int(c.shape[0]), f) for i, c, f in zip(ids, chunks, fin)])
        EVENTS.append(("limit", self.calls[-1]))
        out = []
        for i, c, f in zip(ids, chunks, fin):
            assert c.dim() == 1 and c.dtype == torch.float32
            data = torch.cat([self._held[i], c.cpu()])
            n = data.shape[0] if f else max(0, data.shape[0] - int(self._limit[i].lookahead))
            out.append(data[:n] * SCALE)
            self._held[i] = None if f else data[n:]
        return out


def _run(model_cls, lens, limit, monkeypatch, **kw):
    made = []
    if kw.get("limiter") is not None:
        lim_mod = importlib.import_module("sesameai.limiter")             # (the one ``from .limiter import`` will find)
        monkeypatch.setattr(lim_mod, "LimiterPool", lambda *a, **k: made.append(_FakeLimiter(*a, **k)) or made[-1])
    chunks, pool, others = H._run(model_cls, lens, limit, monkeypatch, **kw)
    others["limit"] = made
    return chunks, pool, others


def _limits():
    from sesameai.limiter import Limit
    # (beside H._levels(): request 1 has a limit and no level, request 9 a level and no limit, requests 5 and 8 neither)
    return [Limit(drive_shift=1), True, True, Limit(lookahead=480), Limit(-3.0, 24), None, Limit(), Limit(lookahead=1), None, None, True]


def _want(limits):
    from sesameai.limiter import Limit
    return [None if v is None else Limit() if v is True else v for v in limits]


@pytest.mark.parametrize("model_cls", [_ScriptedSlots, _ScriptedSlotsBeside])
def test_no_limiter_makes_todays_calls_and_imports_nothing(model_cls, monkeypatch):
    plain, pool0, _ = _run(model_cls, LENS, 30, monkeypatch)
    import sesameai
    if hasattr(sesameai, "limiter"):                                    # put back, afterwards, the module the other tests hold
        monkeypatch.setattr(sesameai, "limiter", sesameai.limiter)
    monkeypatch.delitem(sys.modules, "sesameai.limiter", raising=False)
    got, pool1, made = _run(model_cls, LENS, 30, monkeypatch, limiter=None)
    assert "sesameai.limiter" not in sys.modules, "limiter=None imports nothing"
    assert made["limit"] == [] and EVENTS == []
    assert pool1.log == pool0.log and len(got) == len(plain)
    assert all(a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and a[3] == b[3] for a, b in zip(plain, got))
    got, pool2, made = _run(model_cls, LENS, 30, monkeypatch, limiter=[None] * len(LENS))
    assert made["limit"] == [] and EVENTS == [] and pool2.log == pool0.log, "nobody asks: no pool is built"
    got, pool3, made = _run(model_cls, LENS, 30, monkeypatch, loudness=-19.0)             # the leveler alone: Levels as given, no limiter
    assert "limit" not in {k for k, _ in EVENTS} and made["limit"] == [] and all(lv.ceiling_db == -1.0 for call in made["level"][0].resets for _, lv in call)


@pytest.mark.parametrize("first", [None, 3])
@pytest.mark.parametrize("model_cls", [_ScriptedSlots, _ScriptedSlotsBeside])
def test_slot_streams_limit_every_decode_call_once_and_a_none_request_skips_the_pool(model_cls, first, monkeypatch):
    from sesameai.limiter import Limit
    kw = {} if first is None else {"first_chunk_frames": first}
    limits = _limits()
    want = _want(limits)
    plain, pool0, _ = _run(model_cls, LENS, 30, monkeypatch, **kw)
    got, pool1, made = _run(model_cls, LENS, 30, monkeypatch, limiter=limits, **kw)
    assert len(made["limit"]) == 1 and made["limit"][0].n_streams == 3 and made["level"] == [] and made["stretch"] == [] and made["mark"] == []
    lm = made["limit"][0]
    assert pool1.log == pool0.log, "the decode pool sees the calls it saw"
    # the resets: every limited request that held a slot, once, with ITS Limit
    resets = [r for call in lm.resets for r in call]
    left = [l for _, l in resets]
    for i, l in enumerate(want):
        if l is not None and min(LENS[i], 30) > 0:
            left.remove(l)                                              # (ValueError: a request with audio took its slot without a reset)
    assert all(0 <= slot < 3 and isinstance(l, Limit) for slot, l in resets) and len(left) <= 1
    # one feed per decode call that holds a limited request, over exactly those slots and the PCM of that call
    decodes = [e for e in pool1.log if e[0] in ("decode", "decode_ragged")]
    with_pcm = [c for c in lm.calls if any(n for _, n, _ in c)]
    assert 0 < len(with_pcm) <= len(decodes) and len(decodes) > 10
    k = 0
    for e in decodes:
        sizes = {i: 1920 * (e[2] if e[0] == "decode" else e[2][j]) for j, i in enumerate(e[1])}
        if k < len(with_pcm) and all(i in sizes and sizes[i] == n for i, n, _ in with_pcm[k]):
            k += 1
    assert k == len(with_pcm), "every limiter call takes the PCM of ONE decode call"
    assert all(f for c in lm.calls if not any(n for _, n, _ in c) for _, _, f in c), "an empty feed is only ever a closing one"
    assert sum(f for c in lm.calls for _, _, f in c) == len(resets), "final exactly once per limited request that held a slot"
    bare = 0
    for i in range(len(LENS)):
        a = [c for c in plain if c[0] == i]
        b = [c for c in got if c[0] == i]
        assert [c[3] for c in b] == [False] * (len(b) - 1) + [True] and len(a) == len(b)
        assert all(torch.equal(x[2], y[2]) for x, y in zip(a, b)), "frames and last flags are the plain run's"
        if want[i] is None:
            assert all(torch.equal(x[1], y[1]) for x, y in zip(a, b)), "a request without a limit is not touched"
            continue
        assert torch.equal(torch.cat([y[1] for y in b]), torch.cat([x[1] for x in a]) * SCALE), f"request {i} went through ITS stream"
        # the chunk lengths differ only by the look-ahead, which moves from the first chunk(s) to the last
        la, lb, L = [x[1].shape[0] for x in a], [y[1].shape[0] for y in b], int(want[i].lookahead)
        taken = given = 0
        for j in range(len(la)):
            taken += la[j]
            ready = taken if j == len(la) - 1 else max(0, taken - L)
            assert lb[j] == ready - given, (i, j, la, lb)
            given = ready
        assert lb[-1] == la[-1] + min(L, sum(la[:-1])) and sum(lb) == sum(la), (i, la, lb)
        bare += la[-1] == 0 and lb[-1] > 0
    assert bare > 0, "a closing chunk that is empty at 24 kHz carries the look-ahead"


def test_the_order_is_stretch_level_limit_mark_resample_and_final_travels_through(monkeypatch):
    import test_watermark_host_logic as W
    from sesameai.limiter import paired
    from sesameai.loudness import Level
    monkeypatch.setattr(W, "EVENTS", EVENTS)                                # the fake marker logs where the others do
    levels, limits = H._levels(), _limits()
    got, pool, made = _run(_ScriptedSlots, LENS, 30, monkeypatch, first_chunk_frames=3, speed=SPEEDS, out_sample_rate=48000, watermark=KEY,
                           loudness=levels, limiter=limits)
    lv, lm, ts, wm, rs = made["level"][0], made["limit"][0], made["stretch"][0], made["mark"][0], made["resample"][0]
    assert min(len(lv.calls), len(lm.calls), len(ts.calls), len(wm.calls), len(rs.calls)) > 5
    order = {"stretch": 0, "level": 1, "limit": 2, "mark": 3, "resample": 4}
    per_slot = {}
    for kind, call in EVENTS:
        for i, n, f in call:
            per_slot.setdefault(i, []).append((kind, n, f))
    assert sorted(per_slot) == [0, 1, 2]
    shapes = set()
    for i, seq in per_slot.items():
        at = 0
        while at < len(seq):                                            # a pool call's group: ascending stages up to the resampler
            end = at
            while seq[end][0] != "resample":
                end += 1
            group = seq[at:end + 1]
            kinds = [k for k, _, _ in group]
            assert kinds == sorted(set(kinds), key=order.get) and kinds[-2:] == ["mark", "resample"], (i, group)
            assert len({f for _, _, f in group}) == 1, "final travels with the same chunk through every stage"
            if "limit" in kinds and "stretch" in kinds and group[0][1] == 0:
                assert group[0][2] and group[kinds.index("limit")][1] == LOOK, "a bare ending: the limiter gets the stretch's tail, with final"
                shapes.add("bare")
            shapes.add(tuple(kinds))
            at = end + 1
    assert ("stretch", "level", "limit", "mark", "resample") in shapes and ("level", "limit", "mark", "resample") in shapes and "bare" in shapes
    assert {("mark", "resample"), ("stretch", "mark", "resample")} & shapes, "requests with neither skip both pools"
    assert {("limit", "mark", "resample"), ("stretch", "limit", "mark", "resample")} & shapes, "a limit without a level"
    assert {("level", "mark", "resample"), ("stretch", "level", "mark", "resample")} & shapes, "a level without a limit"
    # with both, each pool got its half of the pair; with one, what was given
    as_level = [None if v is None else v if isinstance(v, Level) else Level(float(v)) for v in levels]
    pairs = [paired(a, b) if a is not None and b is not None else (a, b) for a, b in zip(as_level, _want(limits))]
    given_lv, given_lm = [l for call in lv.resets for _, l in call], [l for call in lm.resets for _, l in call]
    for i, (a, b) in enumerate(pairs):
        if min(LENS[i], 30) > 0:
            if a is not None:
                given_lv.remove(a)
            if b is not None:
                given_lm.remove(b)
    assert len(given_lv) <= 1 and len(given_lm) <= 1
    assert sum(f for c in lm.calls for _, _, f in c) == sum(len(c) for c in lm.resets)


def test_limit_and_paired_against_the_references_numbers():
    from sesameai.limiter import Limit, paired, per_request_limits
    from sesameai.loudness import Level
    assert Limit().params() == tuple(R.params()) == (29203, 120, 27, 0)
    for kw in (dict(ceiling_db=-3.0), dict(lookahead=1), dict(lookahead=480), dict(release_ms=50.0), dict(release_ms=1e9), dict(release_ms=1.0 / 24),
               dict(drive_shift=4), dict(ceiling_db=0.0, lookahead=24, release_ms=250.0, drive_shift=2)):
        assert Limit(**kw).params() == tuple(R.params(**kw)), kw
    assert Limit(release_ms=1e9).params()[2] == 8 and Limit(release_ms=1.0 / 24).params()[2] == 65536
    for bad in (dict(lookahead=0), dict(lookahead=481), dict(lookahead=2.5), dict(drive_shift=-1), dict(drive_shift=5), dict(headroom_shift=5),
                dict(headroom_shift=-1), dict(release_ms=0.0), dict(release_ms=-5.0), dict(release_ms=0.04), dict(ceiling_db=0.5)):
        with pytest.raises(ValueError):
            Limit(**bad).params()
    assert per_request_limits(None, 2) == [None, None] and per_request_limits(True, 2) == [Limit()] * 2
    assert per_request_limits([Limit(-3.0), None, True], 3) == [Limit(-3.0), None, Limit()]
    for bad in ([True], [True, 5.0, None], "yes"):
        with pytest.raises(ValueError):
            per_request_limits(bad, 3)
    # the pair: the leveler h doublings lower under a 0 dB ceiling, the limiter driven by exactly 2^h
    for level, limit in ((Level(-19.0), Limit()), (Level(-16.0, start_gain=0.5, max_gain_db=12.0), Limit(-3.0, 24, 50.0, 0, 1)),
                         (Level(-23.0, slew_shift=2), Limit(headroom_shift=0)), (Level(-14.0, max_gain_db=36.0), Limit(headroom_shift=4))):
        h = limit.headroom_shift
        lo, lm = paired(level, limit)
        assert lm == limit._replace(drive_shift=h) and lm.params() == tuple(R.params(limit.ceiling_db, limit.lookahead, limit.release_ms, h))
        p0 = LR.params(level.loudness, level.ceiling_db, level.start_gain, level.max_gain_db, level.slew_shift)
        want = LR.params(level.loudness - h * 20.0 * math.log10(2.0), 0.0, level.start_gain / 2.0 ** h, level.max_gain_db - 6.0 * h, level.slew_shift)
        assert lo.params() == tuple(want) and want.C == 32767 and want.sh == p0.sh
        assert want.g0 << h == p0.g0 and want.gmax << h == p0.gmax and abs(want.P_T * 4 ** h - p0.P_T) <= 2 * 4 ** h      # rint, then 4^h
    with pytest.raises(ValueError):
        paired(Level(-19.0, start_gain=2.0 ** -16), Limit())                # the lowered start gain leaves the library's range
    with pytest.raises(ValueError):
        paired(Level(-60.0), Limit(headroom_shift=4))                       # the lowered target leaves -70 .. 0 LUFS
