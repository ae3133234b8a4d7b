"""The device resampler pool (include/mimi_hip.h mimi_rs_pool_*, sesameai/resample.py) against the float64 definition
(tests/resample_ref.py) and against itself: streamed == one-shot bit for bit, whatever the chunk schedule, the company and the order.

Bound against the reference, per output: (taps + 3) * 2^-24 * sum|h_phase| * max|x| -- the fp32 fmaf chain's first-order bound plus one
rounding of each tap; at most 61 taps and sum|h| <= 2.25 put it below 9e-6 of the peak.  No sample is excused."""
import ctypes as C

import numpy as np
import pytest
import torch

import resample_ref as R
from test_resample_oracle import GPU_PAIRS, schedule

pytestmark = pytest.mark.gpu
LENS = [1, 7, 333, 1000, 4097]
_cache = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _clips(lens=LENS, seed=0):
    key = ("clips", tuple(lens), seed)
    if key not in _cache:
        g = torch.Generator().manual_seed(seed)
        _cache[key] = [torch.randn(n, generator=g) for n in lens]
    return _cache[key]


def _oneshot(src, dst, lens=LENS, seed=0):
    """The clips' one-shot results (ONE call), computed once per pair and shared."""
    from sesameai.resample import resample
    key = ("oneshot", src, dst, tuple(lens), seed)
    if key not in _cache:
        _cache[key] = [y.clone() for y in resample([c.cuda() for c in _clips(lens, seed)], src, dst)]
    return _cache[key]


def _pool(src, dst, n=64, **kw):
    from sesameai.resample import ResamplerPool
    key = ("pool", src, dst, n, tuple(kw.items()))
    if key not in _cache:
        _cache[key] = ResamplerPool(src, dst, n, **kw)
    _cache[key].reset()
    return _cache[key]


def _streamed(pool, ids, clips, schedules):
    """Every clip through its own stream on its own schedule, all streams sharing the calls: step t feeds every stream that still has a
    chunk; what is left of a clip (maybe nothing) goes with final."""
    clips = [c.to(pool.device) for c in clips]
    at = [0] * len(ids)
    out = [[] for _ in ids]
    for t in range(max(len(s) for s in schedules) + 1):
        live = [j for j in range(len(ids)) if t <= len(schedules[j])]
        chunks = [clips[j][at[j]:at[j] + schedules[j][t]] if t < len(schedules[j]) else clips[j][at[j]:] for j in live]
        for j, y in zip(live, pool.feed([ids[j] for j in live], chunks, [t == len(schedules[j]) for j in live])):
            out[j].append(y)                                  # (every call returns views into a buffer of its own)
            at[j] += schedules[j][t] if t < len(schedules[j]) else 0
    return [torch.cat(o) for o in out]


@pytest.mark.parametrize("src, dst", GPU_PAIRS)
def test_taps_are_the_rounded_float64_filter(src, dst):
    _need_gpu()
    pool = _pool(src, dst)
    up, down, half = R.rates(src, dst)
    assert (pool.up, pool.down, pool.half) == (up, down, half)
    want = R.taps(up, down).astype(np.float32)
    got = pool.taps().numpy()
    assert got.shape == want.shape and np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64))


@pytest.mark.parametrize("src, dst", GPU_PAIRS)
def test_one_shot_against_the_float64_definition(src, dst):
    _need_gpu()
    worst = 0.0
    for x, y in zip(_clips(), _oneshot(src, dst)):
        want, bound = R.resample_ref(x.numpy(), src, dst, with_bound=True)
        got = y.cpu().numpy().astype(np.float64)
        assert got.shape == want.shape
        err = np.abs(got - want)
        worst = max(worst, float((err / bound).max()))
        print(f"{src}->{dst} N={x.shape[0]}: max|err|={err.max():.3g} max bound={bound.max():.3g} worst err/bound={float((err / bound).max()):.3f}")
        assert bound.max() < 9e-6 * float(x.abs().max())
        assert np.all(err <= bound), f"N={x.shape[0]}: {int((err > bound).sum())} outputs outside the bound, worst ratio {(err / bound).max()}"
    assert worst > 0.0, "fp32 cannot be exact here: the comparison compared nothing"


@pytest.mark.parametrize("name", ["ones", "uneven", "short", "tail_alone"])
@pytest.mark.parametrize("src, dst", GPU_PAIRS)
def test_streamed_is_bit_for_bit_the_one_shot_result(src, dst, name):
    _need_gpu()
    pool = _pool(src, dst)
    want = _oneshot(src, dst)
    got = _streamed(pool, [5, 0, 63, 17, 2], _clips(), [schedule(name, n, src, dst) for n in LENS])
    for n, a, b in zip(LENS, got, want):
        assert a.shape == b.shape and torch.equal(a, b), f"{name}, N={n}"


@pytest.mark.parametrize("src, dst", GPU_PAIRS)
def test_company_order_and_stream_id_do_not_matter(src, dst):
    _need_gpu()
    from sesameai.resample import resample
    lens = [1 + (997 * i) % 2400 for i in range(64)]
    clips = [c.cuda() for c in _clips(lens, seed=7)]
    all64 = _oneshot(src, dst, lens, seed=7)
    rev = resample(clips[::-1], src, dst)[::-1]
    assert all(torch.equal(a, b) for a, b in zip(all64, rev)), "64 streams, reversed"
    three = resample(clips[10:13], src, dst)
    assert all(torch.equal(a, b) for a, b in zip(three, all64[10:13])), "3 streams"
    three_rev = resample(clips[10:13][::-1], src, dst)[::-1]
    assert all(torch.equal(a, b) for a, b in zip(three_rev, all64[10:13])), "3 streams, reversed"
    for k in (0, 11, 63):
        (alone,) = resample([clips[k]], src, dst)
        assert torch.equal(alone, all64[k]), f"clip {k} alone"
    # and cut in two at different places, on other stream ids, in one pool
    pool = _pool(src, dst)
    got = _streamed(pool, list(range(63, -1, -1)), clips, [[(7 * i) % (n + 1)] for i, n in enumerate(lens)])
    assert all(torch.equal(a, b) for a, b in zip(got, all64)), "64 streams, each cut once"


@pytest.mark.parametrize("src, dst", [(48000, 24000), (24000, 44100)])
def test_formats(src, dst):
    _need_gpu()
    g = torch.Generator().manual_seed(3)
    s16 = torch.randint(-32768, 32768, (1000,), generator=g).to(torch.int16)
    s16[:4] = torch.tensor([-32768, 32767, 0, -1], dtype=torch.int16)
    pool = _pool(src, dst, 4)
    (a,) = pool.feed([1], [s16.cuda()], True)
    (b,) = pool.feed([2], [(s16.float() / 32768.0).cuda()], True)
    assert a.dtype == torch.float32 and torch.equal(a, b), "int16 in = fp32 in of s / 32768"
    # streamed int16 == one-shot int16
    parts = [pool.feed([3], [s16[:77].cuda()])[0].clone(), pool.feed([3], [s16[77:].cuda()], True)[0]]
    assert torch.equal(torch.cat(parts), a)
    x = 0.6 * torch.randn(1000, generator=g)             # some of it beyond +-1: the clamp works
    x[500] = float("nan")
    (y,) = pool.feed([0], [x.cuda()], True)
    p16 = _pool(src, dst, 4, out_dtype=torch.int16)
    (q,) = p16.feed([0], [x.cuda()], True)
    want = torch.round(torch.clamp(y, -1.0, 1.0) * 32767.0)
    want = torch.where(torch.isnan(y), torch.zeros_like(want), want).to(torch.int16)
    assert q.dtype == torch.int16 and torch.equal(q, want)
    assert int((y.abs() > 1).sum()) > 0 and int(torch.isnan(y).sum()) > 0 and int((q.abs() == 32767).sum()) > 0
    (qq,) = p16.feed([1], [s16.cuda()], True)            # int16 -> int16
    assert torch.equal(qq, torch.round(torch.clamp(a, -1.0, 1.0) * 32767.0).to(torch.int16))


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("src, dst", GPU_PAIRS)
def test_a_non_finite_sample_reaches_exactly_the_outputs_that_cover_it(src, dst, bad):
    _need_gpu()
    pool = _pool(src, dst)
    clips = _clips([333, 1000, 333], seed=5)
    clean = _oneshot(src, dst, [333, 1000, 333], seed=5)
    dirty = [clips[0], clips[1].clone(), clips[2]]
    dirty[1][500] = bad
    for scheds in ([[], [], []], [[100], [7, 333, 1, 159, 1], [300]]):        # one-shot, and cut (the bad sample ends a chunk)
        got = _streamed(pool, [0, 1, 2], dirty, scheds)
        assert torch.equal(got[0], clean[0]) and torch.equal(got[2], clean[2]), "the other streams are untouched"
        lo, hi = R.contaminated(1000, src, dst, 500)
        nonfinite = ~torch.isfinite(got[1]).cpu()
        want = torch.zeros_like(nonfinite); want[lo:hi] = True
        assert hi > lo and torch.equal(nonfinite, want), f"contaminated {nonfinite.nonzero().flatten()[[0, -1]].tolist()} vs [{lo}, {hi})"
        assert torch.equal(got[1][~nonfinite.cuda()], clean[1][~nonfinite.cuda()]), "the rest is bit-identical"
    # a stream that holds the bad sample in its history, reset: clean
    pool.feed([1], [dirty[1][:501].cuda()])
    pool.reset([1])
    (again,) = pool.feed([1], [clips[1].cuda()], True)
    assert torch.equal(again, clean[1]), "clean after reset"
    # ... and after a final, without a reset
    pool.feed([1], [dirty[1][:501].cuda()], True)
    (again,) = pool.feed([1], [clips[1].cuda()], True)
    assert torch.equal(again, clean[1]), "clean after final"


def test_out_count_and_empty_feeds():
    _need_gpu()
    src, dst = 44100, 24000
    up, down, half = R.rates(src, dst)
    pool = _pool(src, dst, 4)
    x = _clips([1000], seed=9)[0].cuda()
    N = 0
    outs = []
    for m in (0, 1, half // up - 1, 3, 0, 500, 1000 - 500 - 3 - (half // up - 1) - 1):
        want = R.emitted(N + m, up, down, half, False) - R.emitted(N, up, down, half, False)
        assert pool.out_count(2, m, False) == want
        (y,) = pool.feed([2], [x[N:N + m]])
        assert y.shape[0] == want
        outs.append(y.clone()); N += m
    assert N == 1000 and pool.out_count(2, 0, True) == R.emitted(N, up, down, half, True) - R.emitted(N, up, down, half, False)
    outs.append(pool.feed([2], [x[:0]], True)[0])
    from sesameai.resample import resample
    assert torch.equal(torch.cat(outs), resample([x], src, dst)[0])
    assert pool.out_count(2, 0, True) == 0, "final left the stream fresh"


def test_refusals_leave_the_pool_usable():
    _need_gpu()
    from sesameai import _abi
    from sesameai.resample import ResamplerPool, resample
    lib = _abi.lib
    h = C.c_void_p(None)
    for src, dst, n in [(24000, 24000, 4), (0, 24000, 4), (24000, -5, 4), (24000, 24001, 4), (321, 1, 4), (1, 321, 4), (48000, 24000, 0), (48000, 24000, 65)]:
        assert lib.mimi_rs_pool_create(src, dst, n, C.byref(h)) == -1 and not h.value and lib.mimi_rs_pool_last_error(None), (src, dst, n)
    with pytest.raises(_abi.CsmError):
        ResamplerPool(24000, 24000, 2)
    src, dst = 48000, 24000
    pool = ResamplerPool(src, dst, 4)
    x = _clips([1000], seed=9)[0].cuda()
    (want,) = resample([x], src, dst)
    out = torch.empty(4096, device="cuda")
    n_out = (C.c_long * 4)(-7, -7, -7, -7)
    i32, lng = (lambda *v: (C.c_int32 * len(v))(*v)), (lambda *v: (C.c_long * len(v))(*v))

    def refused(ids, offs, lens, fin, n, inp=x.data_ptr(), in_fmt=0, outp=out.data_ptr(), out_fmt=0, counts=n_out):
        rc = lib.mimi_rs_pool_feed(pool._h, ids, offs, lens, fin, n, inp, in_fmt, outp, out_fmt, counts, None)
        assert rc == -1 and lib.mimi_rs_pool_last_error(pool._h), "not refused"

    got = [pool.feed([1], [x[:300]])[0].clone()]
    refused(i32(1), lng(0), lng(10), i32(0), 0)
    refused(i32(0, 1, 2, 3, 0), lng(0, 0, 0, 0, 0), lng(1, 1, 1, 1, 1), i32(0, 0, 0, 0, 0), 5)
    refused(i32(1, 1), lng(0, 0), lng(10, 10), i32(0, 0), 2)
    refused(i32(4), lng(0), lng(10), i32(0), 1)
    refused(i32(-1), lng(0), lng(10), i32(0), 1)
    refused(i32(0, 1), lng(0, 0), lng(10, -1), i32(0, 0), 2)
    refused(i32(0, 1), lng(0, -1), lng(10, 10), i32(0, 1), 2)
    refused(None, lng(0), lng(10), i32(0), 1)
    refused(i32(1), None, lng(10), i32(0), 1)
    refused(i32(1), lng(0), None, i32(0), 1)
    refused(i32(1), lng(0), lng(10), None, 1)
    refused(i32(1), lng(0), lng(10), i32(1), 1, inp=None)
    refused(i32(1), lng(0), lng(10), i32(1), 1, outp=None)
    refused(i32(1), lng(0), lng(10), i32(1), 1, counts=None)
    refused(i32(1), lng(0), lng(10), i32(1), 1, in_fmt=2)
    refused(i32(1), lng(0), lng(10), i32(1), 1, out_fmt=-1)
    assert lib.mimi_rs_pool_reset(pool._h, i32(4), 1) == -1 and lib.mimi_rs_pool_reset(pool._h, None, 1) == -1 and lib.mimi_rs_pool_reset(pool._h, i32(1), 0) == -1
    assert lib.mimi_rs_pool_out_count(pool._h, 4, 10, 0) == -1 and lib.mimi_rs_pool_out_count(pool._h, 1, -1, 0) == -1
    assert list(n_out) == [-7] * 4, "a refused call writes no count"
    with pytest.raises(_abi.CsmError):
        pool.feed([1, 1], [x[:5], x[:5]])
    got.append(pool.feed([1], [x[300:]], True)[0])
    assert torch.equal(torch.cat(got), want), "no refused call moved the stream"
