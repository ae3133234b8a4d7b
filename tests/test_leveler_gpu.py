"""The device leveler (include/mimi_hip.h mimi_ld_pool_level_*, sesameai/loudness.py) against the rule (tests/leveler_ref.py): every
comparison is np.array_equal -- samples, boundary gains, hop energies and state rows; fp32 and int16; one-shot and over chunk schedules
that split inside a hop, on a hop edge, with an empty chunk and at an odd offset; three streams with different Levels in any company and
order; a ring that wraps; the cap, gmax, the absolute gate, a start gain, NaN and Inf, in place; integrate on a leveler stream; the
refusals; and the metering feed, bit for bit what it was."""
import numpy as np
import pytest
import torch

import leveler_ref as R
import loudness_ref as L
from test_loudness_oracle import clip, speechlike

pytestmark = pytest.mark.gpu
_cache = {}
SCHEDULE = [1, 2399, 2400, 2401, 511, 0]          # then the rest


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _pool(n=8, ring=0):
    from sesameai.loudness import LoudnessPool
    if ("pool", n, ring) not in _cache:
        _cache[("pool", n, ring)] = LoudnessPool(n, ring=ring)
    return _cache[("pool", n, ring)]


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def _level(**kw):
    from sesameai.loudness import Level
    lv = Level(**kw)
    p = R.params(kw["loudness"], kw.get("ceiling_db", -1.0), kw.get("start_gain", 1.0), kw.get("max_gain_db", 24.0), kw.get("slew_shift", 4))
    assert lv.params() == tuple(p)
    return lv, p


def _clips():
    """three clips of 2.5 .. 6 s (25 .. 60 hops, none a whole number of hops) with their Levels, and the rule's answers, kept"""
    if "clips" not in _cache:
        xs = [clip("speech 0.9")[:3 * 24000 + 777], clip("plosive")[24000:24000 + 60000 + 1], clip("sine 1 kHz")[:100007]]
        lvs = [_level(loudness=-19.0), _level(loudness=-16.0, ceiling_db=-3.0, slew_shift=2), _level(loudness=-23.0, start_gain=0.5, max_gain_db=12.0)]
        _cache["clips"] = xs, lvs
    return _cache["clips"]


def _ref(x, p, ring=L.RING):
    key = ("ref", x.dtype.str, x.shape[0], hash(x.tobytes()), p, ring)
    if key not in _cache:
        _cache[key] = R.level_ref(x, p, ring)
    return _cache[key]


def _as(x, kind):
    return x if kind == "fp32" else L.to_s(x).astype(np.int16)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _cuts(N, schedule):
    out, a = [], 0
    for c in schedule:
        c = min(c, N - a)
        out.append((a, a + c)); a += c
    out.append((a, N))
    return out


def _streamed(pool, ids, xs, levels, plans):
    """every clip through its own stream on its own schedule, the streams sharing the calls, `final` with each stream's last chunk
    -> per stream (samples, energies, gains joined over the calls without the repeated boundaries, state row)"""
    pool.level_reset(ids, levels)
    dev = [_t(x).cuda() for x in xs]
    ys, es, gs = [[] for _ in ids], [[] for _ in ids], [[] for _ in ids]
    for t in range(max(len(p) for p in plans)):
        live = [j for j in range(len(ids)) if t < len(plans[j])]
        fin = [t == len(plans[j]) - 1 for j in live]
        out = pool.level_feed([ids[j] for j in live], [dev[j][plans[j][t][0]:plans[j][t][1]] for j in live], fin)
        for a, j in enumerate(live):
            assert out[a].shape[0] == plans[j][t][1] - plans[j][t][0]                       # n_out == n_in on every call
            ys[j].append(out[a]); es[j].append(pool.last_energies[a])
            g = pool.last_gains[a].cpu().numpy().astype(np.int64)
            assert g.shape[0] == pool.last_energies[a].shape[0] + 2
            if gs[j]:
                assert np.array_equal(np.concatenate(gs[j])[-2:], g[:2])                    # the open hop's boundaries come again
                g = g[2:]
            gs[j].append(g)
    rows = [tuple(r) for r in pool.level_state(ids).cpu().tolist()]
    return [(torch.cat(ys[j]).cpu().numpy(), torch.cat(es[j]).cpu().numpy(), np.concatenate(gs[j]), rows[j]) for j in range(len(ids))]


def _check(got, want, what):
    y, e, g, row = got
    assert _same(y, want.y), (what, int(np.count_nonzero(y != want.y)))
    assert np.array_equal(e, want.energies) and np.array_equal(g, want.gains), what
    assert row == want.row, (what, row, want.row)


@pytest.mark.parametrize("kind", ["fp32", "int16"])
def test_three_streams_one_shot_alone_and_reversed(kind):
    _need_gpu()
    xs, lvs = _clips()
    xs = [_as(x, kind) for x in xs]
    pool = _pool()
    whole = [[(0, x.shape[0])] for x in xs]
    together = _streamed(pool, [0, 1, 2], xs, [lv for lv, _ in lvs], whole)
    for j in range(3):
        _check(together[j], _ref(xs[j], lvs[j][1]), (kind, "together", j))
        alone = _streamed(pool, [5], [xs[j]], [lvs[j][0]], [whole[j]])[0]
        _check(alone, _ref(xs[j], lvs[j][1]), (kind, "alone", j))
    back = _streamed(pool, [7, 3, 6], xs[::-1], [lv for lv, _ in lvs][::-1], whole[::-1])
    for j in range(3):
        _check(back[j], _ref(xs[2 - j], lvs[2 - j][1]), (kind, "reversed", j))
    assert all(len(set(_ref(xs[j], lvs[j][1]).gains.tolist())) > 1 for j in range(3))             # no identity passes


@pytest.mark.parametrize("kind", ["fp32", "int16"])
def test_chunk_schedules_give_the_one_shot_result(kind):
    _need_gpu()
    xs, lvs = _clips()
    xs = [_as(x, kind) for x in xs]
    N = [x.shape[0] for x in xs]
    frames = [(0, 3840)] + [(a, min(a + 1920, N[2])) for a in range(3840, N[2], 1920)]
    plans = [_cuts(N[0], SCHEDULE), [(0, N[1])], frames]
    got = _streamed(_pool(), [2, 0, 1], xs, [lv for lv, _ in lvs], plans)
    for j in range(3):
        _check(got[j], _ref(xs[j], lvs[j][1]), (kind, j))


@pytest.mark.parametrize("kind", ["fp32", "int16"])
def test_odd_offsets_heads_tails_and_in_place(kind):
    """chunks at odd element offsets of the packed buffer (the 16-byte lines are ragged at both ends), out on another 16-byte phase than
    in (no vector path), and in == out"""
    _need_gpu()
    xs, lvs = _clips()
    pool = _pool()
    x = _as(xs[0], kind)
    want = _ref(x, lvs[0][1])
    lens = [1, 3, 5, 7, 9, 2401, 4099, 8197]
    plan = _cuts(x.shape[0], lens)                                  # every chunk but one starts at an odd offset of the CLIP
    for in_place in (False, True):
        pool.level_reset([4, 1], [lvs[0][0], lvs[1][0]])
        ys = []
        for a, b in plan:                                           # stream 1's 1-, 3- .. sample chunks in front shift stream 4's offset in the buffer
            out = pool.level_feed([1, 4], [_t(_as(xs[1], kind)[:len(ys) * 2 + 1]).cuda(), _t(x[a:b]).cuda()], in_place=in_place)
            ys.append(out[1])
        assert _same(torch.cat(ys).cpu().numpy(), want.y), (kind, in_place)
    # the C ABI directly: out = a buffer whose address differs from in's by 4 (fp32) or 2 (int16) bytes modulo 16
    import ctypes as C
    from sesameai.loudness import _stream
    src = _t(x).cuda()
    dst = torch.zeros(x.shape[0] + 9, dtype=src.dtype, device="cuda")
    pool.level_reset([2], lvs[0][0])
    hops = x.shape[0] // L.H
    energy = torch.empty(hops, dtype=torch.int64, device="cuda")
    gain = torch.empty(hops + 2, dtype=torch.int32, device="cuda")
    n_hops = (C.c_long * 1)()
    rc = pool._lib.mimi_ld_pool_level_feed(pool._h, (C.c_int32 * 1)(2), (C.c_long * 1)(0), (C.c_long * 1)(x.shape[0]), (C.c_int32 * 1)(1), 1,
                                           src.data_ptr(), int(kind == "int16"), dst.data_ptr() + src.element_size(), energy.data_ptr(),
                                           gain.data_ptr(), n_hops, _stream())
    assert rc == 0 and n_hops[0] == hops
    got = dst.cpu().numpy()
    assert _same(got[1:1 + x.shape[0]], want.y) and not got[0] and not got[1 + x.shape[0]:].any()      # and nothing outside it
    assert np.array_equal(gain.cpu().numpy(), want.gains) and np.array_equal(energy.cpu().numpy(), want.energies)


def test_a_ring_of_8_against_25_hops():
    _need_gpu()
    pool = _pool(2, ring=8)
    x = clip("loud then quiet")[60000:120000 + 100]                 # 25 hops across the drop of 38 dB
    lv, p = _level(loudness=-19.0)
    want = _ref(x, p, 8)
    assert not np.array_equal(want.gains, _ref(x, p).gains)         # the ring is seen
    for plan in ([(0, x.shape[0])], _cuts(x.shape[0], [31000, 9000])):
        _check(_streamed(pool, [1], [x], [lv], [plan])[0], want, plan)


def test_cap_gmax_the_gate_and_a_start_gain():
    _need_gpu()
    pool = _pool()
    lv, p = _level(loudness=-19.0)
    plosive = clip("plosive")[:60000 + 5]
    quiet = speechlike(6.0, 0.05, 2)[:60000] * np.float32(0.25)
    silent = speechlike(3.0, 1.0, 5) * np.float32(10 ** (-75 / 20))
    half, ph = _level(loudness=-19.0, start_gain=0.5)
    fast, pf = _level(loudness=-19.0, slew_shift=1, max_gain_db=12.0)
    xs, lvs, ps = [plosive, quiet, silent, plosive, quiet], [lv, fast, lv, half, half], [p, pf, p, ph, ph]
    got = _streamed(pool, [0, 1, 2, 3, 4], xs, lvs, [[(0, x.shape[0])] for x in xs])
    for j in range(5):
        _check(got[j], _ref(xs[j], ps[j]), j)
    w = _ref(plosive, p)
    assert w.row[2] > 0 and np.abs(L.to_s(w.y)).max() <= p.C and any(g == cap for g, (_, _, _, cap) in zip(w.gains[2:], w.trace))     # the cap binds
    assert _ref(quiet, pf).gains[-1] == pf.gmax                                                             # gmax binds
    assert L.measure_ref(silent)[1] == 0 and set(_ref(silent, p).gains.tolist()) == {p.g0}                  # under the absolute gate: g0
    assert _ref(plosive, ph).gains[0] == 32768 and not np.array_equal(_ref(plosive, ph).y, w.y)


def test_nan_and_inf_touch_nothing_else():
    _need_gpu()
    xs, lvs = _clips()
    pool = _pool()
    x = xs[0].copy()
    x[40000], x[40001], x[50001] = np.nan, np.inf, -np.inf
    want, clean = _ref(x, lvs[0][1]), _ref(xs[0], lvs[0][1])
    assert np.isnan(want.y[40000]) and want.y[40001] == np.float32(lvs[0][1].C) / 32768 and want.y[50001] == -want.y[40001]
    assert np.array_equal(want.y[:38400], clean.y[:38400]) and np.array_equal(want.gains[:18], clean.gains[:18])       # the hops in front
    plans = [_cuts(x.shape[0], [1920 * 5] * 6), [(0, xs[1].shape[0])], [(0, xs[2].shape[0])]]
    got = _streamed(pool, [0, 1, 2], [x, xs[1], xs[2]], [lv for lv, _ in lvs], plans)
    _check(got[0], want, "the stream with NaN and Inf")
    _check(got[1], _ref(xs[1], lvs[1][1]), "its neighbour")
    _check(got[2], _ref(xs[2], lvs[2][1]), "its neighbour")
    _check(_streamed(pool, [0], [xs[0]], [lvs[0][0]], [[(0, xs[0].shape[0])]])[0], clean, "the next call")


def test_integrate_sees_the_input_of_a_leveler_stream():
    _need_gpu()
    xs, lvs = _clips()
    pool = _pool()
    pool.level_reset([0, 1], [lvs[0][0], lvs[1][0]])
    pool.level_feed([0, 1], [_t(xs[0][:30000]), _t(xs[1][:1000])])
    pool.level_feed([0, 1], [_t(xs[0][30000:]), _t(xs[1][1000:])], final=True)
    rows = [tuple(r) for r in pool.integrate([0, 1]).cpu().tolist()]
    assert rows == [L.measure_ref(xs[0]), L.measure_ref(xs[1])]


def test_refusals_move_nothing():
    _need_gpu()
    from sesameai._abi import CsmError
    from sesameai.loudness import Level
    xs, lvs = _clips()
    pool = _pool()
    x, (lv, p) = xs[0], lvs[0]
    st = R.LevelerRef(p)
    pool.reset([6])
    pool.level_reset([0, 3], lv)
    assert [tuple(r) for r in pool.level_state([0, 3]).cpu().tolist()] == [(p.g0, 0, 0, 0)] * 2          # reset and not fed
    y0 = pool.level_feed([0], [_t(x[:5000])])[0].cpu().numpy()
    assert _same(y0, st.feed(x[:5000])[0])
    with pytest.raises(CsmError):                                   # a leveler stream at the metering feed
        pool.feed([0], [_t(x[5000:9000])])
    with pytest.raises(CsmError):                                   # a metering stream at the leveler's feed, in company
        pool.level_feed([0, 6], [_t(x[5000:9000])] * 2)
    with pytest.raises(CsmError):
        pool.level_state([6])
    for ids in ([], [0, 0], [8], [-1]):
        with pytest.raises(CsmError):
            pool.level_feed(ids, [_t(x[:10])] * len(ids))
    for bad in (dict(max_gain_db=37.0), dict(start_gain=0.0), dict(start_gain=17.0), dict(slew_shift=0), dict(slew_shift=17), dict(ceiling_db=1.0)):
        with pytest.raises(ValueError):
            pool.level_reset([0], Level(-19.0, **bad))
    with pytest.raises(ValueError):
        pool.level_reset([0], Level(-80.0))
    import ctypes as C
    one, pt = (C.c_int32 * 1)(0), (C.c_long * 1)(p.P_T)
    i32 = lambda v: (C.c_int32 * 1)(v)
    for args in ((pt, i32(0), i32(65536), i32(65536), i32(4)), ((C.c_long * 1)(0), i32(100), i32(65536), i32(65536), i32(4)),
                 (pt, i32(100), i32(65537), i32(65536), i32(4)), (pt, i32(100), i32(65536), i32((1 << 22) + 1), i32(4)),
                 (pt, i32(100), i32(65536), i32(65536), i32(17))):
        assert pool._lib.mimi_ld_pool_level_reset(pool._h, one, *args, 1) == -1
    # nothing moved: the rule's continuation, and stream 6 still meters
    y1 = pool.level_feed([0], [_t(x[5000:])], final=True)[0].cpu().numpy()
    assert _same(y1, st.feed(x[5000:], final=True)[0])
    assert tuple(pool.level_state([0]).cpu().tolist()[0]) == st.row == _ref(x, p).row
    e = pool.feed([6], [_t(x)], final=True)[0].cpu().numpy()
    assert np.array_equal(e, L.hop_energies(L.to_s(x)))
    pool.reset([0])                                                 # back to metering
    assert np.array_equal(pool.feed([0], [_t(x)], final=True)[0].cpu().numpy(), e)


def test_the_metering_feed_is_what_it_was():
    """k_ld_energy with its new, null pointer: the existing inputs' energies and rows, and the one-shot ``level`` beside ``measure``"""
    _need_gpu()
    from sesameai.loudness import level, measure
    names = ["plosive", "speech 0.9", "sine 60 Hz", "square 3 kHz", "loud then quiet"]
    xs = [clip(n)[:60001] for n in names]
    pool = _pool()
    pool.reset(list(range(5)))
    es = pool.feed(list(range(5)), [_t(x) for x in xs], final=True)
    rows = [tuple(r) for r in pool.integrate(list(range(5))).cpu().tolist()]
    for j, x in enumerate(xs):
        assert np.array_equal(es[j].cpu().numpy(), L.hop_energies(L.to_s(x))) and rows[j] == L.measure_ref(x), names[j]
    assert [tuple(m) for m in measure([_t(x) for x in xs])] == [L.measure_ref(x) for x in xs]
    ys = level([_t(x) for x in xs], [-19.0, -23.0, -16.0, -19.0, -30.0])
    for j, (x, t) in enumerate(zip(xs, [-19.0, -23.0, -16.0, -19.0, -30.0])):
        assert _same(ys[j].cpu().numpy(), _ref(x, R.params(t)).y), names[j]
