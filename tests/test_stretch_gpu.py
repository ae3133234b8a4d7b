"""The device time-stretch pool (include/mimi_hip.h mimi_ts_pool_*, sesameai/stretch.py) against the rule (tests/stretch_ref.py): every check
is np.array_equal, for the samples AND for the offsets d_k the search picked -- one-shot, streamed over the oracle test's schedules, in any
company, order and stream id, on the clips where the tie-break and the 32-bit score are decisive, and with non-finite samples."""
import ctypes as C

import numpy as np
import pytest
import torch

import stretch_ref as S
from test_stretch_oracle import LENGTHS, PMS, noise, schedules, square, tie_clip, voiced

pytestmark = pytest.mark.gpu
_cache = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _clip(N):
    if N not in _cache:
        _cache[N] = voiced(N, N) if N % 2 else noise(N, N)
    return _cache[N]


def _ref(x, pm):
    return S.stretch_ref(x, pm)


def _pool(n=64):
    from sesameai.stretch import TimeStretchPool
    if ("pool", n) not in _cache:
        _cache[("pool", n)] = TimeStretchPool(n)
    return _cache[("pool", n)]


def _same(y, d, want, what):
    wy, wd = want
    assert np.array_equal(d.cpu().numpy(), wd), (what, "d", d.cpu().numpy().tolist(), wd.tolist())
    got = y.cpu().numpy()
    assert got.shape == wy.shape, (what, got.shape, wy.shape)
    assert np.array_equal(got, wy, equal_nan=True), (what, "y", int(np.count_nonzero(~((got == wy) | (np.isnan(got) & np.isnan(wy))))))


def _stretch(clips, speeds):
    from sesameai.stretch import stretch
    return stretch([torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in clips], speeds, want_offsets=True)


def _streamed(pool, ids, pms, clips, scheds):
    """Every clip through its own stream on its own schedule, all streams sharing the calls: step t feeds every stream that still has a
    chunk; what is left of a clip (maybe nothing) goes with final.  out_count is checked against every feed."""
    pool.reset(ids, [pm / 1000.0 for pm in pms])
    clips = [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in clips]
    cuts = [S.cut(c.shape[0], s) for c, s in zip(clips, scheds)]
    ys, ds = [[] for _ in ids], [[] for _ in ids]
    for t in range(max(len(p) for p, _ in cuts) + 1):
        live = [j for j in range(len(ids)) if t <= len(cuts[j][0])]
        fin = [t == len(cuts[j][0]) for j in live]
        chunks = [clips[j][cuts[j][1]:] if f else clips[j][cuts[j][0][t][0]:cuts[j][0][t][1]] for j, f in zip(live, fin)]
        counts = [pool.out_count(ids[j], c.shape[0], f) for j, c, f in zip(live, chunks, fin)]
        y, d = pool.feed([ids[j] for j in live], chunks, fin, want_offsets=True)
        assert [int(v.shape[0]) for v in y] == counts
        for j, yy, dd in zip(live, y, d):
            ys[j].append(yy); ds[j].append(dd)
    return [torch.cat(v) for v in ys], [torch.cat(v) for v in ds]


@pytest.mark.parametrize("pm", [500, 1200, 2000])
def test_one_shot_is_the_rule(pm):
    _need_gpu()
    clips = [_clip(N) for N in LENGTHS]
    ys, ds = _stretch(clips, pm / 1000.0)
    for N, x, y, d in zip(LENGTHS, clips, ys, ds):
        _same(y, d, _ref(x, pm), (pm, N))


def test_64_clips_with_their_own_speeds_and_no_regard_for_company():
    _need_gpu()
    rng = np.random.default_rng(5)
    lens = [int(v) for v in rng.integers(0, 6000, 64)]
    lens[:4] = [0, 1, 1280, 5999]
    pms = [int(v) for v in rng.integers(500, 2001, 64)]
    pms[:4] = [500, 2000, 1000, 1999]
    clips = [noise(n, 100 + i) for i, n in enumerate(lens)]
    ys, ds = _stretch(clips, [pm / 1000.0 for pm in pms])
    want = [_ref(x, pm) for x, pm in zip(clips, pms)]
    for i in range(64):
        _same(ys[i], ds[i], want[i], ("all 64", i))
    # a few of them again: other stream ids, reversed order, other company
    pool = _pool()
    pick = [63, 40, 3, 17, 0]
    ids = [5, 62, 9, 0, 33]
    pool.reset(ids, [pms[i] / 1000.0 for i in pick])
    y2, d2 = pool.feed(ids, [torch.from_numpy(clips[i]) for i in pick], final=True, want_offsets=True)
    for i, y, d in zip(pick, y2, d2):
        _same(y, d, want[i], ("subset", i))


@pytest.mark.parametrize("pm", PMS)
def test_streamed_over_any_schedule_is_the_one_shot_result(pm):
    _need_gpu()
    pool = _pool()
    jobs = [(N, name, sch) for N in (0, 1, 1279, 1281, 5000, 20011) for name, sch in schedules(N, N + pm).items()]
    ids = list(range(3, 3 + len(jobs)))
    ys, ds = _streamed(pool, ids, [pm] * len(jobs), [_clip(N) for N, _, _ in jobs], [sch for _, _, sch in jobs])
    for (N, name, _), y, d in zip(jobs, ys, ds):
        _same(y, d, _ref(_clip(N), pm), (pm, N, name))


def test_the_tie_break_the_full_scale_square_and_silence():
    _need_gpu()
    clips = [tie_clip(), square(), np.zeros(5000, dtype=np.float32)]
    pms = [1250, 1000, 1200]
    ys, ds = _stretch(clips, [pm / 1000.0 for pm in pms])
    for i in range(3):
        _same(ys[i], ds[i], _ref(clips[i], pms[i]), i)
    assert (ds[2][1:] == -S.D).all()
    wrong = S.stretch_ref(clips[0], 1250, tie="last")[1]
    assert (ds[0].cpu().numpy()[1:] != wrong[1:]).all()                  # a last-index argmax would differ in every block
    assert S.stretch_ref(clips[1], 1000, want_scores=True)[2] == 512 * 2047 * 2047
    # the same three streamed in 1,920-sample chunks
    y2, d2 = _streamed(_pool(), [0, 1, 2], pms, clips, [[1920] * 8] * 3)
    for i in range(3):
        _same(y2[i], d2[i], _ref(clips[i], pms[i]), ("streamed", i))


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_sample_enters_no_decision_and_stays_where_it_is_mixed(bad):
    _need_gpu()
    x = noise(6000, 2)
    xb = x.copy(); xb[3000] = bad
    xz = x.copy(); xz[3000] = 0.0
    other = noise(4000, 3)
    pool = _pool()
    ys, ds = _streamed(pool, [7, 8], [1200, 800], [xb, other], [[1920, 1920], [4000]])
    want = _ref(xb, 1200)
    _same(ys[0], ds[0], want, "the clip with the bad sample")
    assert np.array_equal(ds[0].cpu().numpy(), _ref(xz, 1200)[1])
    assert 1 <= int(np.count_nonzero(~np.isfinite(want[0]))) <= 2
    _same(ys[1], ds[1], _ref(other, 800), "its neighbour")
    # the pool's next call, on the same streams
    ys, ds = _streamed(pool, [7, 8], [1200, 800], [x, other], [[100, 3000], [7]])
    _same(ys[0], ds[0], _ref(x, 1200), "the stream after the bad clip")
    _same(ys[1], ds[1], _ref(other, 800), "its neighbour after the bad clip")


def test_a_reset_forgets_an_open_clip_and_final_leaves_the_speed():
    _need_gpu()
    pool = _pool()
    a, b = noise(5000, 8), noise(3000, 9)
    pool.reset([2], 1.5)
    pool.feed([2], [torch.from_numpy(a)])                             # an open clip: blocks out, carry and c on the device
    pool.reset([2], 0.73)
    y, d = pool.feed([2], [torch.from_numpy(b)], final=True, want_offsets=True)
    _same(y[0], d[0], _ref(b, 730), "after a reset")
    y, d = pool.feed([2], [torch.from_numpy(a)], final=True, want_offsets=True)       # final left the stream fresh at the same speed
    _same(y[0], d[0], _ref(a, 730), "after final")


def test_every_refusal_leaves_the_pool_usable():
    _need_gpu()
    from sesameai import _abi
    from sesameai.stretch import TimeStretchPool, stretch
    with pytest.raises(_abi.CsmError):
        TimeStretchPool(0)
    with pytest.raises(_abi.CsmError):
        TimeStretchPool(65)
    pool = TimeStretchPool(4)
    x = torch.from_numpy(noise(3000, 4))
    pool.reset([1], 1.2)
    first = pool.feed([1], [x[:2000]])[0].clone()
    for ids, speeds in (([0, 0], [1.2, 1.2]), ([4], [1.2]), ([-1], [1.2]), ([0], [0.499]), ([0], [2.001]), ([], []), ([0, 1, 2, 3, 0], [1.0] * 5)):
        with pytest.raises(_abi.CsmError):
            pool.reset(ids, speeds)
    for ids in ([1, 1], [4], [-1], [], [0, 1, 2, 3, 1]):
        with pytest.raises(_abi.CsmError):
            pool.feed(ids, [x[:10]] * len(ids))
    with pytest.raises(_abi.CsmError):
        pool.out_count(4, 10)
    with pytest.raises(_abi.CsmError):
        pool.out_count(0, -1)
    lib, h = _abi.lib, pool._h
    one, off, ln, fin, no = (C.c_int32 * 1)(1), (C.c_long * 1)(0), (C.c_long * 1)(10), (C.c_int32 * 1)(0), (C.c_long * 1)(0)
    buf = torch.zeros(16, device="cuda")
    assert lib.mimi_ts_pool_feed(h, one, off, ln, fin, 1, None, buf.data_ptr(), no, None, None) == -1
    assert lib.mimi_ts_pool_feed(h, one, off, ln, fin, 1, buf.data_ptr(), None, no, None, None) == -1
    assert lib.mimi_ts_pool_feed(h, one, (C.c_long * 1)(-1), ln, fin, 1, buf.data_ptr(), buf.data_ptr(), no, None, None) == -1
    assert lib.mimi_ts_pool_feed(h, one, off, (C.c_long * 1)(-1), fin, 1, buf.data_ptr(), buf.data_ptr(), no, None, None) == -1
    assert lib.mimi_ts_pool_feed(h, one, off, (C.c_long * 1)(2 ** 30 + 1), fin, 1, buf.data_ptr(), buf.data_ptr(), no, None, None) == -1
    assert b"2^30" in lib.mimi_ts_pool_last_error(h)
    with pytest.raises(ValueError):
        stretch([], 1.2)
    with pytest.raises(ValueError):
        stretch([x] * 65, 1.2)
    # stream 1 went on as if nothing had happened: no refusal moved its state
    rest = pool.feed([1], [x[2000:]], final=True)[0]
    assert np.array_equal(torch.cat([first, rest]).cpu().numpy(), _ref(x.numpy(), 1200)[0])
