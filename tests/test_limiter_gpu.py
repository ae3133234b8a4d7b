"""The device limiter (include/mimi_hip.h mimi_lim_pool_*, sesameai/limiter.py) against the rule (tests/limiter_ref.py): every comparison
is np.array_equal -- samples, emitted counts and state rows; fp32 and int16; lengths around the look-ahead, the history and the tile;
every corner of the parameter ranges; peaks at both ends, on both sides of a tile edge, L apart and K apart; chunk schedules that split
inside and around L, sample by sample over a tile edge, with empty chunks and an empty final; 64 streams in one call; alone, in company
and in reversed order; NaN and Inf; the one-shot ``limit``; the refusals.  Every case but the named pass-through is limited somewhere BY
THE REFERENCE, so no identity passes."""
import numpy as np
import pytest
import torch

import limiter_ref as R

pytestmark = pytest.mark.gpu
_cache = {}
TILE = 4096                 # LIM_TILE
ONE = R.ONE


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _pool(n=64):
    from sesameai.limiter import LimiterPool
    if ("pool", n) not in _cache:
        _cache[("pool", n)] = LimiterPool(n)
    return _cache[("pool", n)]


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def _limit(p: R.Params):
    """the ``Limit`` whose integers are p: release_ms is chosen so that rint(65536 / (release_ms 24)) is p.rho"""
    from sesameai.limiter import Limit
    db = 0.0 if p.C == 32767 else 20.0 * np.log10((p.C + 0.5) / 32767.0)
    lm = Limit(ceiling_db=db, lookahead=p.L, release_ms=65536.0 / (24.0 * p.rho), drive_shift=p.hr)
    assert lm.params() == tuple(p), (lm.params(), p)
    return lm


def _clip(N, p: R.Params, kind, seed=0, spikes=()):
    """noise well inside full scale after the drive, with full-scale negative spikes where asked (a = 32768 > every C)"""
    rng = np.random.default_rng(seed * 7919 + N)
    x = (np.clip(rng.standard_normal(N) * 0.2, -0.9, 0.9) * 2.0 ** -p.hr).astype(np.float32)
    for s in spikes:
        if 0 <= s < N:
            x[s] = -(2.0 ** -p.hr)
    return x if kind == "fp32" else np.clip(np.rint(x * 32768.0), -32768, 32767).astype(np.int16)


def _ref(x, p):
    key = ("ref", x.dtype.str, x.shape[0], hash(x.tobytes()), p)
    if key not in _cache:
        _cache[key] = R.limit_ref(x, p)
    return _cache[key]


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _cuts(N, schedule):
    out, a = [], 0
    for c in schedule:
        c = min(c, N - a)
        out.append((a, a + c)); a += c
    out.append((a, N))
    return out


def _streamed(pool, ids, xs, ps, plans, empty_final=False):
    """every clip through its own stream on its own schedule, the streams sharing the calls; `final` with each stream's last chunk, or
    with an empty chunk behind it -> per stream (samples, state row); the emitted counts are checked against the rule call by call"""
    pool.reset(ids, [_limit(p) for p in ps])
    assert [tuple(r) for r in pool.state(ids).cpu().tolist()] == [(ONE, 0, 0, 0)] * len(ids)                 # reset and not fed
    dev = [_t(x).cuda() for x in xs]
    plans = [pl + [(pl[-1][1], pl[-1][1])] for pl in plans] if empty_final else plans
    ys, refs = [[] for _ in ids], [R.LimiterRef(p) for p in ps]
    for t in range(max(len(pl) for pl in plans)):
        live = [j for j in range(len(ids)) if t < len(plans[j])]
        fin = [t == len(plans[j]) - 1 for j in live]
        want = [refs[j].out_count(plans[j][t][1] - plans[j][t][0], f) for j, f in zip(live, fin)]
        assert [pool.out_count(ids[j], plans[j][t][1] - plans[j][t][0], f) for j, f in zip(live, fin)] == want
        out = pool.feed([ids[j] for j in live], [dev[j][plans[j][t][0]:plans[j][t][1]] for j in live], fin)
        for a, j in enumerate(live):
            assert out[a].shape[0] == want[a], (t, j)
            refs[j].E += want[a]; refs[j].R += plans[j][t][1] - plans[j][t][0]               # (the counts only: the samples are checked whole)
            ys[j].append(out[a])
    rows = [tuple(r) for r in pool.state(ids).cpu().tolist()]
    return [(torch.cat(ys[j]).cpu().numpy(), rows[j]) for j in range(len(ids))]


def _check(got, want, what, limited=True):
    y, row = got
    assert _same(y, want.y), (what, int(np.count_nonzero(y != want.y)), np.nonzero(y != want.y)[0][:8])
    assert row == want.row, (what, row, want.row)
    assert (want.limited > 0) == limited, (what, "the reference limits nothing here" if limited else "the pass-through is limited")


def _lengths(p):
    H = p.K + 2 * p.L
    return [0, 1, p.L, p.L + 1, H - 1, H + 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5]


@pytest.mark.parametrize("kind", ["fp32", "int16"])
@pytest.mark.parametrize("L,rho", [(L, rho) for L in (1, 120, 480) for rho in (8, 27, 65536)])
def test_lengths_and_parameters_one_shot(L, rho, kind):
    """ten lengths a call, (hr, C) going round all six pairs; a spike at sample 0 and one at the last sample of every clip"""
    _need_gpu()
    corners = [(hr, C) for hr in (0, 2) for C in (1, 29204, 32767)]
    ps = [R.Params(corners[(j + L + rho) % 6][1], L, rho, corners[(j + L + rho) % 6][0]) for j in range(10)]
    Ns = _lengths(ps[0])
    xs = [_clip(N, p, kind, j, spikes=(0, N - 1)) for j, (N, p) in enumerate(zip(Ns, ps))]
    got = _streamed(_pool(), list(range(10)), xs, ps, [[(0, N)] for N in Ns])
    for j in range(10):
        if Ns[j] == 0:
            assert got[j][0].shape[0] == 0 and got[j][1] == (ONE, 0, 0, 0)
        else:
            _check(got[j], _ref(xs[j], ps[j]), (kind, L, rho, Ns[j], ps[j]))


@pytest.mark.parametrize("kind", ["fp32", "int16"])
def test_peaks_at_the_ends_on_a_tile_edge_L_apart_and_K_apart(kind):
    _need_gpu()
    cases = []
    for p in (R.Params(29204, 120, 27, 2), R.Params(1000, 480, 8, 0), R.Params(32767, 1, 65536, 0), R.Params(9000, 7, 27, 1)):
        N = 2 * TILE + p.K + 700
        for name, spikes in (("sample 0", (0,)), ("the last sample", (N - 1,)), ("before the tile edge", (TILE - 1,)),
                             ("behind the tile edge", (TILE,)), ("both sides of it", (TILE - 1, TILE)), ("L apart", (3000, 3000 + p.L)),
                             ("L + 1 apart", (3000, 3001 + p.L)), ("K apart", (600, 600 + p.K)), ("K + L apart", (600, 600 + p.K + p.L))):
            x = np.zeros(N, np.float32 if kind == "fp32" else np.int16)                      # lone spikes after silence
            for s in spikes:
                x[s] = -(2.0 ** -p.hr) if kind == "fp32" else -(32768 >> p.hr)
            cases.append((name, x, p))
    got = _streamed(_pool(), list(range(len(cases))), [c[1] for c in cases], [c[2] for c in cases], [[(0, c[1].shape[0])] for c in cases])
    for g, (name, x, p) in zip(got, cases):
        w = _ref(x, p)
        _check(g, w, (kind, name, p))
        s, a = int(np.nonzero(x)[0][0]), 32768                                             # (the spike is full scale AFTER the drive)
        peak = abs(float(g[0][s])) * (32768 if kind == "fp32" else 1)
        assert p.C - 1 - (a >> 16) <= peak <= p.C, (kind, name, p, peak)                   # the peak is met, not cut
    x = np.zeros(2000, np.int16)
    x[1000] = -32768
    assert _streamed(_pool(), [5], [x], [R.Params(29204, 120, 27, 2)], [[(0, 2000)]])[0][0][1000] == -29204


SCHEDULES = {"inside L": lambda L: [L // 2, 1, L - L // 2 - 1, 1, 1], "around L": lambda L: [L - 1, 2, L + 1, L, L + 1],
             "sample by sample over a tile edge": lambda L: [TILE + L - 2, 1, 1, 1, 1], "empty chunks": lambda L: [500, 0, 0, 700, 0],
             "frames": lambda L: [3840] + [1920] * 4}


@pytest.mark.parametrize("kind", ["fp32", "int16"])
@pytest.mark.parametrize("empty_final", [False, True])
def test_chunk_schedules_give_the_one_shot_result(kind, empty_final):
    """five schedules x four parameter sets in the same calls, and the streams reused for a second clip after `final`"""
    _need_gpu()
    ps = [R.Params(29204, 120, 27, 0), R.Params(1, 1, 65536, 2), R.Params(32767, 480, 8, 2), R.Params(9000, 7, 1000, 1)]
    xs, pp, plans = [], [], []
    for a, p in enumerate(ps):
        N = 3 * TILE + 5 + 100 * a
        for b, (name, steps) in enumerate(SCHEDULES.items()):
            xs.append(_clip(N, p, kind, 10 * a + b, spikes=(0, TILE + p.L, TILE + p.L + 1, N - 1)))
            pp.append(p); plans.append(_cuts(N, steps(p.L)))
    ids = list(range(len(xs)))[::-1]
    for clip_no in range(2):
        got = _streamed(_pool(), ids, xs, pp, plans, empty_final)
        for j in range(len(xs)):
            _check(got[j], _ref(xs[j], pp[j]), (kind, empty_final, clip_no, j, pp[j]))


@pytest.mark.parametrize("kind", ["fp32", "int16"])
def test_64_streams_alone_in_company_and_reversed(kind):
    _need_gpu()
    rng = np.random.default_rng(5)
    Ls, rhos, Cs = [1, 7, 120, 333, 480], [8, 27, 100, 1000, 65536], [1, 100, 9000, 29204, 32767]
    ps = [R.Params(Cs[j % 5], Ls[(j // 5) % 5], rhos[(j * 3) % 5], (j // 3) % 5) for j in range(64)]
    Ns = [int(rng.integers(1, 3 * TILE)) for _ in range(64)]
    xs = [_clip(N, p, kind, j, spikes=(N // 2,)) for j, (N, p) in enumerate(zip(Ns, ps))]
    whole = [[(0, N)] for N in Ns]
    pool = _pool()
    together = _streamed(pool, list(range(64)), xs, ps, whole)
    for j in range(64):
        _check(together[j], _ref(xs[j], ps[j]), (kind, "together", j, ps[j]))
    back = _streamed(pool, list(range(64))[::-1], xs, ps, whole)                          # other stream ids, the same list order
    flipped = _streamed(pool, list(range(64)), xs[::-1], ps[::-1], whole[::-1])           # the reversed list
    for j in range(64):
        assert _same(back[j][0], together[j][0]) and back[j][1] == together[j][1]
        assert _same(flipped[63 - j][0], together[j][0]) and flipped[63 - j][1] == together[j][1]
    for j in (0, 17, 63):
        alone = _streamed(pool, [9], [xs[j]], [ps[j]], [whole[j]])[0]
        assert _same(alone[0], together[j][0]) and alone[1] == together[j][1]
    # ragged schedules in company: every stream its own chunk length
    plans = [_cuts(N, [1 + (37 * j) % 900] * 3 + [TILE]) for j, N in enumerate(Ns)]
    ragged = _streamed(pool, list(range(64)), xs, ps, plans)
    for j in range(64):
        assert _same(ragged[j][0], together[j][0]) and ragged[j][1] == together[j][1], (kind, "ragged", j)


@pytest.mark.parametrize("kind", ["fp32", "int16"])
def test_a_clip_under_the_ceiling_passes_untouched(kind):
    """the named pass-through: nothing is limited, the output is the input, delayed by nothing once concatenated"""
    _need_gpu()
    p = R.Params(32000, 120, 27, 0)
    x = _clip(2 * TILE + 77, p, kind, 3)
    assert np.abs(x.astype(np.float64)).max() * (32768 if kind == "fp32" else 1) < p.C
    for plan in ([(0, x.shape[0])], _cuts(x.shape[0], [60, 60, 1, 4000])):
        got = _streamed(_pool(), [2], [x], [p], [plan])[0]
        _check(got, _ref(x, p), (kind, plan), limited=False)
        assert _same(got[0], x) and got[1] == (ONE, x.shape[0], 0, 0)


def test_nan_and_inf_touch_nothing_else():
    _need_gpu()
    p, q = R.Params(29204, 120, 27, 0), R.Params(20000, 480, 8, 1)
    clean = _clip(3 * TILE, p, "fp32", 4, spikes=(100,))
    x = clean.copy()
    x[3000], x[5000], x[TILE + 1], x[2 * TILE - 1] = np.nan, np.inf, -np.inf, 1e30
    other = _clip(2 * TILE + 9, q, "fp32", 6, spikes=(5000,))
    want, cw = _ref(x, p), _ref(clean, p)
    Cf = np.float32(p.C) / np.float32(32768)
    assert np.isnan(want.y[3000]) and want.y[5000] == Cf and want.y[TILE + 1] == -Cf and want.y[2 * TILE - 1] == Cf and want.row[3] == 3
    first = TILE + 1 - p.L                                                                               # where the first Inf begins to pull the gain
    assert np.array_equal(np.delete(want.y[:first], 3000), np.delete(cw.y[:first], 3000))                 # the NaN moved nothing
    assert np.array_equal(want.g[:first], cw.g[:first]) and want.g[first] < cw.g[first]
    for plans in ([[(0, x.shape[0])], [(0, other.shape[0])]], [_cuts(x.shape[0], [3001, 1999, 1, 95]), _cuts(other.shape[0], [1920] * 3)]):
        got = _streamed(_pool(), [0, 1], [x, other], [p, q], plans)
        _check(got[0], want, "the stream with NaN and Inf")
        _check(got[1], _ref(other, q), "its neighbour")
    _check(_streamed(_pool(), [0], [clean], [p], [[(0, clean.shape[0])]])[0], cw, "the next clip on that stream")


@pytest.mark.parametrize("kind", ["fp32", "int16"])
def test_limit_with_64_clips(kind):
    _need_gpu()
    from sesameai.limiter import Limit, limit
    rng = np.random.default_rng(8)
    ps = [R.params(ceiling_db=-1.0 - (j % 4), lookahead=(24, 120, 480)[j % 3], release_ms=(50.0, 100.0, 250.0)[j % 3], drive_shift=1 + j % 2)
          for j in range(64)]
    lms = [Limit(-1.0 - (j % 4), (24, 120, 480)[j % 3], (50.0, 100.0, 250.0)[j % 3], 1 + j % 2) for j in range(64)]
    assert [lm.params() for lm in lms] == [tuple(p) for p in ps]
    Ns = [int(rng.integers(1, 2 * TILE)) for _ in range(64)]
    xs = [_clip(N, R.Params(hr=0), kind, 100 + j, spikes=(N // 2,)) for j, N in enumerate(Ns)]            # 6 .. 12 dB hot after the drive
    ys = limit([_t(x) for x in xs], lms)
    for j in range(64):
        w = _ref(xs[j], ps[j])
        assert _same(ys[j].cpu().numpy(), w.y) and w.limited > 0, (kind, j)
    one = limit([_t(xs[0])], Limit(drive_shift=2))[0].cpu().numpy()                                       # one Limit for all
    assert _same(one, _ref(xs[0], R.params(drive_shift=2)).y)
    with pytest.raises(ValueError):
        limit([], Limit())
    with pytest.raises(ValueError):
        limit([_t(xs[0])] * 65, Limit())


def test_refusals_move_nothing():
    _need_gpu()
    import ctypes as C
    from sesameai._abi import CsmError
    from sesameai.limiter import Limit, LimiterPool
    pool = LimiterPool(4)
    p = R.Params(9000, 120, 27, 1)
    x = _clip(TILE + 900, p, "fp32", 12, spikes=(700, 4000))
    with pytest.raises(CsmError, match="without parameters"):                              # a new pool's streams have none
        pool.feed([0], [_t(x[:10])])
    pool.reset([0, 3], _limit(p))
    st = R.LimiterRef(p)
    y0 = pool.feed([0], [_t(x[:1000])])[0].cpu().numpy()
    assert _same(y0, st.feed(x[:1000]))
    for ids in ([], [0, 0], [4], [-1]):
        with pytest.raises(CsmError):
            pool.feed(ids, [_t(x[:10])] * len(ids))
    with pytest.raises(CsmError, match="without parameters"):
        pool.feed([0, 1], [_t(x[1000:1100])] * 2)                                          # in company: stream 0 does not move either
    with pytest.raises(CsmError, match="other format"):
        pool.feed([0], [_t(np.zeros(10, np.int16))])                                       # it holds fp32 samples
    for bad in (dict(lookahead=0), dict(lookahead=481), dict(drive_shift=5), dict(drive_shift=-1), dict(headroom_shift=5), dict(release_ms=0.0),
                dict(release_ms=0.001), dict(ceiling_db=1.0), dict(lookahead=1.5)):
        with pytest.raises(ValueError):
            pool.reset([0], Limit(**bad))
    one, i32 = (C.c_int32 * 1)(0), lambda v: (C.c_int32 * 1)(v)
    for args in ((0, 120, 27, 0), (32768, 120, 27, 0), (100, 0, 27, 0), (100, 481, 27, 0), (100, 120, 7, 0), (100, 120, 65537, 0),
                 (100, 120, 27, -1), (100, 120, 27, 5)):
        assert pool._lib.mimi_lim_pool_reset(pool._h, one, *[i32(v) for v in args], 1) == -1
    buf = torch.zeros(64, device="cuda")
    n_out = (C.c_long * 1)()
    head = (pool._h, one, (C.c_long * 1)(0), (C.c_long * 1)(16), i32(0), 1)
    assert pool._lib.mimi_lim_pool_feed(*head, buf.data_ptr(), buf.data_ptr(), n_out, 0, None) == -1 and b"overlap" in pool._lib.mimi_lim_pool_last_error(pool._h)
    assert pool._lib.mimi_lim_pool_feed(*head, buf.data_ptr(), None, n_out, 0, None) == -1
    assert pool._lib.mimi_lim_pool_feed(*head, buf.data_ptr() + 2, buf.data_ptr() + 128, n_out, 0, None) == -1
    assert pool._lib.mimi_lim_pool_feed(*head, buf.data_ptr(), buf.data_ptr() + 128, n_out, 2, None) == -1
    assert pool.out_count(0, 5) == 5 and pool.out_count(0, 5, True) == 125 and pool.out_count(3, 120) == 0 and pool.out_count(3, 121) == 1
    with pytest.raises(CsmError):
        pool.out_count(1, 5)
    # nothing moved: the rule's continuation
    y1 = pool.feed([0], [_t(x[1000:])], final=True)[0].cpu().numpy()
    assert _same(y1, st.feed(x[1000:], final=True))
    assert tuple(pool.state([0]).cpu().tolist()[0]) == st.row == _ref(x, p).row and st.row[2] > 0
    assert pool.poll([0, 3])[1] == (ONE, 0, 0, 0) and pool.poll([0])[0].limited == st.row[2]
