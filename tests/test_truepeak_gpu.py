"""The device's true-peak detection (include/mimi_hip.h mimi_lim_pool_reset_tp and mimi_tp_measure; sesameai/limiter.py, sesameai/truepeak.py)
against the rule (tests/truepeak_ref.py): every comparison is np.array_equal -- samples, emitted counts, state rows and meter rows; fp32 and
int16; lengths around T, the latency L + T and the tile; L in {1, 120, 480} with rho, hr and C going round; true peaks that lie between a
tile's last sample and the next tile's first; a lone inter-sample peak whose 16-tap window straddles a tile edge, a chunk edge, the clip's
first sample and its last; samples of 2^15 and more (the 64-bit path), NaN and Inf, clips that mix narrow and wide tiles; chunk schedules
with chunks shorter than T; 64 streams of both modes in one call, alone, in company and reversed, reused after ``final``; the meter for 64
ragged clips; the refusals.

A condition, not a measurement: every clip of two samples or more, in every case but the named pass-through, has a_tp > a somewhere BY THE
REFERENCE and a true-peak output that differs from the sample-peak output, so no case passes on sample-peak arithmetic.  (A clip of 0 or 1
samples cannot: the largest tap is 14693 < 2^14, so a lone sample's inter-sample magnitudes stay below it.  Those lengths ride in calls
whose other clips meet the condition.)"""
import numpy as np
import pytest
import torch

import limiter_ref as R
import truepeak_ref as P

pytestmark = pytest.mark.gpu
_cache = {}
TILE = 4096                 # LIM_TILE
ONE = R.ONE
T = P.T


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


def _limit(p: R.Params, tp=True):
    """the ``Limit`` whose integers are p"""
    from sesameai.limiter import Limit
    db = 0.0 if p.C == 32767 else 20.0 * np.log10((p.C + 0.5) / 32767.0)
    lm = Limit(ceiling_db=db, lookahead=p.L, release_ms=65536.0 / (24.0 * p.rho), drive_shift=p.hr, true_peak=tp)
    assert lm.params() == tuple(p) and lm.latency == p.L + (T if tp else 0), (lm.params(), p)
    return lm


def _clip(N, p: R.Params, kind, seed=0, scale=1.0):
    """an fs/4 tone at 45 degrees (+ + - - ..: every second interval carries a true peak 3 dB over its samples), each sample 0.95 .. 1 of
    ``scale`` x full scale after the drive"""
    rng = np.random.default_rng(seed * 7919 + N)
    sign = np.where((np.arange(N) // 2) % 2 == 0, 1.0, -1.0)
    x = sign * (1.0 - 0.05 * rng.random(N)) * scale * 2.0 ** -p.hr
    return x.astype(np.float32) if kind == "fp32" else np.clip(np.rint(x * 32767.0), -32768, 32767).astype(np.int16)


def _key(x, p):
    return (x.dtype.str, x.shape[0], hash(x.tobytes()), p)


def _ref(x, p, tp=True):
    key = ("ref", tp) + _key(x, p)
    if key not in _cache:
        _cache[key] = P.limit_tp_ref(x, p) if tp else R.limit_ref(x, p)
    return _cache[key]


def _matters(x, p):
    """the condition: a_tp > a somewhere, and the true-peak output is not the sample-peak output"""
    a_tp, a = P.magnitude_tp(x, p.hr), R.magnitude(x, p.hr)
    return bool((a_tp > a).any()) and not np.array_equal(_ref(x, p).y, _ref(x, p, False).y, equal_nan=True)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _cuts(N, schedule):
    out, a = [], 0
    for c in schedule:
        c = min(c, N - a)
        out.append((a, a + c)); a += c
    out.append((a, N))
    return out


def _streamed(pool, ids, xs, ps, plans, tps=None, empty_final=False):
    """every clip through its own stream on its own schedule, the streams sharing the calls (tps: which detect true peaks; None: all);
    `final` with each stream's last chunk, or with an empty chunk behind it -> per stream (samples, state row); the emitted counts are
    checked against the rule call by call"""
    tps = [True] * len(ids) if tps is None else tps
    pool.reset(ids, [_limit(p, tp) for p, tp in zip(ps, tps)])
    assert [tuple(r) for r in pool.state(ids).cpu().tolist()] == [(ONE, 0, 0, 0)] * len(ids)                 # reset and not fed
    dev = [_t(x).cuda() for x in xs]
    plans = [pl + [(pl[-1][1], pl[-1][1])] for pl in plans] if empty_final else plans
    ys, refs = [[] for _ in ids], [P.TruePeakLimiterRef(p) if tp else R.LimiterRef(p) for p, tp in zip(ps, tps)]
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


def _check(got, x, p, what, tp=True, matters=True):
    y, row = got
    want = _ref(x, p, tp)
    assert _same(y, want.y), (what, int(np.count_nonzero(y != want.y)), np.nonzero(y != want.y)[0][:8])
    assert row == want.row, (what, row, want.row)
    if tp and x.shape[0] >= 2:
        assert _matters(x, p) == matters, (what, "true peaks change nothing here" if matters else "the pass-through is limited")


def _lengths(L):
    return [0, 1, T - 1, T, T + 1, 2 * T, L + T, L + T + 1, TILE - 1, TILE, TILE + 1, 12293]


@pytest.mark.parametrize("kind", ["fp32", "int16"])
@pytest.mark.parametrize("L", [1, 120, 480])
def test_lengths_and_parameters_one_shot(L, kind):
    """twelve lengths a call; rho goes round {8, 27, 65536} and (hr, C) round all six pairs"""
    _need_gpu()
    corners = [(hr, C) for hr in (0, 2) for C in (1, 29204, 32767)]
    ps = [R.Params(corners[(j + L) % 6][1], L, (8, 27, 65536)[(j + L) % 3], corners[(j + L) % 6][0]) for j in range(12)]
    Ns = _lengths(L)
    xs = [_clip(N, p, kind, j) for j, (N, p) in enumerate(zip(Ns, ps))]
    got = _streamed(_pool(), list(range(12)), xs, ps, [[(0, N)] for N in Ns])
    for j in range(12):
        if Ns[j] == 0:
            assert got[j][0].shape[0] == 0 and got[j][1] == (ONE, 0, 0, 0)
        else:
            _check(got[j], xs[j], ps[j], (kind, L, Ns[j], ps[j]))


def _pair(N, at, p, kind):
    """silence but for two equal samples at ``at`` and ``at + 1``, each just under C after the drive: no sample passes the ceiling, the
    interval between them does (1.25 x) -- a lone inter-sample peak"""
    s = ((p.C - 3) >> p.hr)
    x = np.zeros(N, np.int16)
    x[at:at + 2] = s
    return x if kind == "int16" else (x.astype(np.float32) / np.float32(32768.0)).astype(np.float32)


@pytest.mark.parametrize("kind", ["fp32", "int16"])
def test_true_peaks_on_tile_edges_chunk_edges_and_the_clip_ends(kind):
    _need_gpu()
    N = 2 * TILE + 700
    cases = []
    for p in (R.Params(29204, 120, 27, 0), R.Params(20000, 1, 65536, 1), R.Params(32000, 480, 8, 2)):
        # the fs/4 tone at 1.3 x full scale (int16: at full scale), whole and cut one sample either side of every tile edge of the outputs
        x = _clip(N, p, kind, 3, scale=1.3 if kind == "fp32" else 1.0)
        cases.append(("tone", x, p, [(0, N)]))
        cases.append(("tone cut at the tile", x, p, _cuts(N, [TILE + p.L + T - 1, 1, 1, TILE - 2, 1, 1])))
        # the lone peak: its window straddles the clip's first sample, its last, a tile edge (the pair before it, across it, behind it; the
        # edge of the outputs lies at TILE one shot and L + T later in the input when streamed) and a chunk edge
        for at in (0, N - 2, TILE - 9, TILE - 2, TILE - 1, TILE, TILE + 6, TILE + p.L + T - 1, 2 * TILE - 1):
            x = _pair(N, at, p, kind)
            cases.append((("pair", at), x, p, [(0, N)]))
            cut = min(max(at + 1, 1), N - 1)
            cases.append((("pair cut inside", at), x, p, _cuts(N, [cut - 5, 5, 1, 2, 6]) if cut > 5 else _cuts(N, [cut, 3, 5])))
    for lo in range(0, len(cases), 64):
        part = cases[lo:lo + 64]
        got = _streamed(_pool(), list(range(len(part))), [c[1] for c in part], [c[2] for c in part], [c[3] for c in part])
        for g, (name, x, p, _) in zip(got, part):
            _check(g, x, p, (kind, name, p))
            if name[0].startswith("pair"):
                assert _ref(x, p, False).limited == 0 and _ref(x, p).limited > 0, "no sample passes the ceiling; the interval does"


@pytest.mark.parametrize("kind", ["fp32", "int16"])
def test_samples_of_2_to_the_15_and_more_take_the_wide_path_and_give_the_rules_integers(kind):
    _need_gpu()
    N = 3 * TILE + 5
    if kind == "int16":
        ps = [R.Params(29204, 120, 27, 4), R.Params(1000, 480, 8, 4), R.Params(32767, 1, 65536, 1)]
        xs = [_clip(N, R.Params(hr=0), kind, 1), _clip(N, R.Params(hr=0), kind, 2), _clip(N, R.Params(hr=0), kind, 3)]      # |v| up to 2^19; 2^16
        mixed = _clip(N, R.Params(hr=0), kind, 4)
        mixed[:TILE + 300] //= 4                                             # narrow tiles, then wide ones (hr = 1: |v| < 2^15 needs |s| < 2^14)
        mixed[2 * TILE + 900:] //= 4
        ps.append(R.Params(20000, 120, 27, 1)); xs.append(mixed)
        assert np.abs(mixed[:TILE].astype(np.int64) << 1).max() < 2 ** 15 <= np.abs(mixed[TILE + 300:2 * TILE].astype(np.int64) << 1).max()
    else:
        ps = [R.Params(29204, 120, 27, 0), R.Params(1000, 480, 8, 2), R.Params(32767, 1, 65536, 0), R.Params(20000, 120, 27, 0), R.Params(29204, 7, 100, 0)]
        xs = [_clip(N, ps[0], kind, 1, scale=9.0), _clip(N, ps[1], kind, 2, scale=9.0), _clip(N, ps[2], kind, 3, scale=1.5)]
        mixed = _clip(N, ps[3], kind, 4, scale=0.99)
        mixed[TILE + 300:2 * TILE + 900] *= np.float32(9.0)
        xs.append(mixed)
        assert np.abs(P.signed(mixed[:TILE], 0)).max() < 2 ** 15 < np.abs(P.signed(mixed, 0)).max()
        odd = _clip(N, ps[4], kind, 5, scale=1.2)
        odd[3000], odd[5000], odd[TILE + 1], odd[2 * TILE - 1], odd[2 * TILE], odd[N - 1] = np.nan, np.inf, -np.inf, 1e30, np.nan, -1e30
        xs.append(odd)
    ids = list(range(len(xs)))
    for plans in ([[(0, N)]] * len(xs), [_cuts(N, [3001, 1999, 1, 95, TILE - 3, 7])] * len(xs)):
        got = _streamed(_pool(), ids, xs, ps, plans)
        for j in ids:
            _check(got[j], xs[j], ps[j], (kind, j, ps[j], len(plans[0])))
    if kind == "fp32":
        w = _ref(xs[4], ps[4])
        assert np.isnan(w.y[3000]) and np.isnan(w.y[2 * TILE]) and w.row[3] == 4                # the NaN stay, the four absurd samples are clamped
        clean = _clip(N, ps[4], kind, 5, scale=1.2)
        assert np.array_equal(w.g[:3000 - ps[4].L - T - ps[4].K], _ref(clean, ps[4]).g[:3000 - ps[4].L - T - ps[4].K])
        _check(_streamed(_pool(), [4], [clean], [ps[4]], [[(0, N)]])[0], clean, ps[4], "the next clip on that stream")


SCHEDULES = {"shorter than T": lambda L: [1, 2, 3, 4, 5, 6, 7] * 12 + [TILE], "around the latency": lambda L: [L + T - 1, 2, L + T + 1, L + T, L + 1],
             "sample by sample over a tile edge": lambda L: [TILE + L + T - 2, 1, 1, 1, 1], "empty chunks": lambda L: [5, 0, 0, 700, 0, 3, 0],
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
            xs.append(_clip(N, p, kind, 10 * a + b))
            pp.append(p); plans.append(_cuts(N, steps(p.L)))
    ids = list(range(len(xs)))[::-1]
    for clip_no in range(2):
        got = _streamed(_pool(), ids, xs, pp, plans, empty_final=empty_final)
        for j in range(len(xs)):
            _check(got[j], xs[j], pp[j], (kind, empty_final, clip_no, j, pp[j]))


@pytest.mark.parametrize("kind", ["fp32", "int16"])
def test_64_streams_of_both_modes_alone_in_company_and_reversed(kind):
    _need_gpu()
    rng = np.random.default_rng(5)
    Ls, rhos, Cs = [1, 7, 120, 333, 480], [8, 27, 100, 1000, 65536], [1, 100, 9000, 29204, 32767]
    ps = [R.Params(Cs[j % 5], Ls[(j // 5) % 5], rhos[(j * 3) % 5], (j // 3) % 3) for j in range(64)]
    tps = [j % 3 != 1 for j in range(64)]                                                 # 21 sample-peak streams among them
    Ns = [int(rng.integers(2, 3 * TILE)) for _ in range(64)]
    xs = [_clip(N, p, kind, j) for j, (N, p) in enumerate(zip(Ns, ps))]
    whole = [[(0, N)] for N in Ns]
    pool = _pool()
    together = _streamed(pool, list(range(64)), xs, ps, whole, tps)
    for j in range(64):
        _check(together[j], xs[j], ps[j], (kind, "together", j, ps[j], tps[j]), tp=tps[j])      # (sample mode: bit-identical to limit_ref)
        assert _matters(xs[j], ps[j]), j
    back = _streamed(pool, list(range(64))[::-1], xs, ps, whole, tps)                    # other stream ids (and the other mode's banks), the same list order
    flipped = _streamed(pool, list(range(64)), xs[::-1], ps[::-1], whole[::-1], tps[::-1])          # the reversed list
    for j in range(64):
        assert _same(back[j][0], together[j][0]) and back[j][1] == together[j][1]
        assert _same(flipped[63 - j][0], together[j][0]) and flipped[63 - j][1] == together[j][1]
    for j in (0, 1, 17, 63):
        alone = _streamed(pool, [9], [xs[j]], [ps[j]], [whole[j]], [tps[j]])[0]
        assert _same(alone[0], together[j][0]) and alone[1] == together[j][1]
    # ragged schedules in company: every stream its own chunk length, the streams reused after `final`
    plans = [_cuts(N, [1 + (37 * j) % 900] * 3 + [TILE]) for j, N in enumerate(Ns)]
    ragged = _streamed(pool, list(range(64)), xs, ps, plans, tps)
    for j in range(64):
        assert _same(ragged[j][0], together[j][0]) and ragged[j][1] == together[j][1], (kind, "ragged", j)
    # the one-shot ``limit`` with one Limit per clip
    from sesameai.limiter import limit
    ys = limit([_t(x) for x in xs], [_limit(p, tp) for p, tp in zip(ps, tps)])
    assert all(_same(ys[j].cpu().numpy(), together[j][0]) for j in range(64))


@pytest.mark.parametrize("kind", ["fp32", "int16"])
def test_a_clip_whose_true_peak_is_under_the_ceiling_passes_untouched(kind):
    """the named pass-through: nothing is limited, the output is the input"""
    _need_gpu()
    p = R.Params(32000, 120, 27, 0)
    x = _clip(2 * TILE + 77, p, kind, 3, scale=0.6)
    assert P.measure_tp(x)[0] < P.measure_tp(x)[1] < p.C
    for plan in ([(0, x.shape[0])], _cuts(x.shape[0], [60, 60, 1, 7, 4000])):
        got = _streamed(_pool(), [2], [x], [p], [plan])[0]
        _check(got, x, p, (kind, plan), matters=False)
        assert _same(got[0], x) and got[1] == (ONE, x.shape[0], 0, 0)


@pytest.mark.parametrize("kind", ["fp32", "int16"])
def test_the_meter_for_64_ragged_clips(kind):
    _need_gpu()
    from sesameai.truepeak import TruePeak, true_peak, true_peak_db, true_peak_rows
    rng = np.random.default_rng(11)
    Ns = [0, 1, 2, T, TILE - 1, TILE, TILE + 1, 3 * TILE + 5] + [int(rng.integers(1, 3 * TILE)) for _ in range(56)]
    xs = [_clip(N, R.Params(), kind, 40 + j, scale=(0.5, 1.0, 9.0)[j % 3] if kind == "fp32" else (0.5, 1.0)[j % 2]) for j, N in enumerate(Ns)]
    quiet = np.zeros(2 * TILE + 10, xs[0].dtype)
    first, last, edge = quiet.copy(), quiet.copy(), quiet.copy()
    first[0] = last[-2:] = 1000                                                           # the peak is the first interval's; the last one's
    edge[TILE - 1:TILE + 1] = -1000                                                       # the interval across a tile edge
    tie = quiet.copy()
    tie[100:102] = tie[TILE + 100:TILE + 102] = tie[2 * TILE:2 * TILE + 2] = 500          # the same true peak in three tiles: the first wins
    xs[8:13] = [first, last, edge, tie, quiet]
    want = [P.measure_tp(x) for x in xs]
    assert want[0] == (0, 0, 0, 0) and want[8][2] == 0 and want[9][2] in (quiet.shape[0] - 2, quiet.shape[0] - 1) and want[10][2] == TILE - 1
    assert want[11][2] == 100 and want[11][1] > want[11][0] and want[12] == (0, 0, 0, quiet.shape[0])
    assert sum(w[1] > w[0] for w in want) > 50 and (kind == "int16" or max(w[1] for w in want) > 2 ** 18)
    rows = true_peak_rows([_t(x) for x in xs])
    assert rows.is_cuda and rows.dtype == torch.int64 and [tuple(r) for r in rows.cpu().tolist()] == want
    got = true_peak([_t(x).cuda() for x in xs[::-1]])                                    # reversed, from the device
    assert [tuple(g) for g in got] == want[::-1] and isinstance(got[0], TruePeak)
    assert true_peak([_t(xs[7])])[0] == want[7]                                          # alone
    assert abs(got[-8].true_peak_db - 20 * np.log10(want[7][1] / 32768.0)) < 1e-9 and true_peak_db(0) == float("-inf")
    with pytest.raises(ValueError):
        true_peak([])
    with pytest.raises(ValueError):
        true_peak([_t(xs[1])] * 65)


def test_refusals_move_nothing():
    _need_gpu()
    import ctypes as C
    from sesameai._abi import CsmError, lib
    from sesameai.limiter import Limit, LimiterPool
    pool = LimiterPool(4)
    p = R.Params(9000, 120, 27, 1)
    x = _clip(TILE + 900, p, "fp32", 12)
    pool.reset([0, 3], _limit(p))
    st = P.TruePeakLimiterRef(p)
    y0 = pool.feed([0], [_t(x[:1000])])[0].cpu().numpy()
    assert _same(y0, st.feed(x[:1000])) and y0.shape[0] == 1000 - p.L - T
    one, i32 = (C.c_int32 * 1)(0), lambda v: (C.c_int32 * 1)(v)
    for args in ((100, 120, 27, 0, 2), (100, 120, 27, 0, -1), (0, 120, 27, 0, 1), (100, 481, 27, 0, 1), (100, 120, 7, 0, 1), (100, 120, 27, 5, 1)):
        assert pool._lib.mimi_lim_pool_reset_tp(pool._h, one, *[i32(v) for v in args], 1) == -1
    assert pool._lib.mimi_lim_pool_reset_tp(pool._h, one, *[i32(v) for v in (100, 120, 27, 0, 2)], 1) == -1
    assert b"neither 0 nor 1" in pool._lib.mimi_lim_pool_last_error(pool._h)
    assert pool._lib.mimi_lim_pool_reset_tp(pool._h, one, i32(100), i32(120), i32(27), i32(0), None, 1) == -1
    with pytest.raises(CsmError, match="other format"):
        pool.feed([0], [_t(np.zeros(10, np.int16))])                                       # it holds fp32 samples
    with pytest.raises(CsmError):
        pool.feed([0, 1], [_t(x[1000:1100])] * 2)                                          # stream 1 has no parameters: stream 0 does not move
    with pytest.raises(ValueError):
        pool.reset([0], Limit(lookahead=481, true_peak=True))
    assert pool.out_count(0, 5) == 5 and pool.out_count(0, 5, True) == 5 + p.L + T and pool.out_count(3, p.L + T) == 0 and pool.out_count(3, p.L + T + 1) == 1
    # the meter: nothing written
    rows = torch.full((2, 4), 7, dtype=torch.int64, device="cuda")
    buf = torch.zeros(64, device="cuda")
    off, ln = (C.c_long * 2)(0, 8), (C.c_long * 2)(8, 8)
    for args, text in (((None, off, ln, 2, 0, rows.data_ptr(), None), b"null pointer"), ((buf.data_ptr(), off, ln, 2, 0, None, None), b"null pointer"),
                       ((buf.data_ptr(), off, ln, 2, 2, rows.data_ptr(), None), b"unknown format"), ((buf.data_ptr() + 2, off, ln, 2, 0, rows.data_ptr(), None), b"misaligned"),
                       ((buf.data_ptr(), off, ln, 2, 0, rows.data_ptr() + 4, None), b"misaligned"), ((buf.data_ptr(), off, ln, 0, 0, rows.data_ptr(), None), b"1 .. 64 clips"),
                       ((buf.data_ptr(), off, ln, 65, 0, rows.data_ptr(), None), b"1 .. 64 clips"),
                       ((buf.data_ptr(), off, (C.c_long * 2)(8, -1), 2, 0, rows.data_ptr(), None), b"negative length"),
                       ((buf.data_ptr(), (C.c_long * 2)(-1, 8), ln, 2, 0, rows.data_ptr(), None), b"negative offset")):
        assert lib.mimi_tp_measure(*args) == -1 and text in lib.mimi_tp_last_error(), text
    assert bool((rows == 7).all())
    # nothing moved: the rule's continuation
    y1 = pool.feed([0], [_t(x[1000:])], final=True)[0].cpu().numpy()
    assert _same(y1, st.feed(x[1000:], final=True))
    assert tuple(pool.state([0]).cpu().tolist()[0]) == st.row == _ref(x, p).row and st.row[2] > 0
    assert pool.poll([0, 3])[1] == (ONE, 0, 0, 0)
