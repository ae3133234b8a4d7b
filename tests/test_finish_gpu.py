"""The device segment finisher (include/mimi_hip.h mimi_fin_*, sesameai/finish.py) against the rule's oracle (tests/finish_ref.py): every
comparison is ``np.array_equal`` / ``torch.equal`` -- the rule is integer-valued and fully specified, no sample is excused.  Lead, tail and
fade are given in SAMPLES: the wrapper converts ``sample_rate * ms // 1000``, so at ``sample_rate=1000`` a millisecond is a sample."""
import ctypes as C

import numpy as np
import pytest
import torch

from finish_ref import finish_ref, quantise

LENS = [0, 1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8193]
PARAMS = [(0, 0, 0), (12000, 2400, 1200), (1, 0, 1), (0, 1, 5), (3, 2, 1_000_000), (2, 1, 4)]
_cache = {}


def _fin():
    from sesameai.finish import SegmentFinisher
    if "fin" not in _cache:
        _cache["fin"] = SegmentFinisher("cuda")
    return _cache["fin"]


def _clips(lens=tuple(LENS), seed=0, amp=0.3):
    key = ("clips", lens, seed, amp)
    if key not in _cache:
        g = torch.Generator().manual_seed(seed)
        _cache[key] = [torch.randn(n, generator=g) * amp for n in lens]
    return _cache[key]


def _big():
    """The seeded 300,001-sample clip at amplitude 0.2."""
    if "big" not in _cache:
        _cache["big"] = torch.randn(300_001, generator=torch.Generator().manual_seed(7)) * 0.2
    return _cache["big"]


def _run(clips, params):
    """One wrapper call -> one int16 NumPy array per clip; params: one (lead, tail, fade) in samples for all clips, or one per clip."""
    from sesameai.finish import SegmentFinish
    how = SegmentFinish(*params) if isinstance(params, tuple) else [SegmentFinish(*p) for p in params]
    out = _fin().finish([c.cuda() for c in clips], how, sample_rate=1000)
    torch.cuda.synchronize()
    assert all(y.dtype == torch.int16 and y.is_cuda for y in out)
    return [y.cpu().numpy() for y in out]


def _same(got, clips, params):
    per = [params] * len(clips) if isinstance(params, tuple) else params
    assert len(got) == len(clips)
    for k, (y, c, p) in enumerate(zip(got, clips, per)):
        want = finish_ref(c.numpy(), *p)
        assert y.shape == want.shape, (k, len(c), p)
        assert np.array_equal(y, want), (k, len(c), p, int((y != want).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("params", PARAMS)
def test_every_length_in_one_call(params):
    """All the lengths around the tiles of both kernels in ONE call: the segments' M are odd and even in turn, so most start at an odd element."""
    clips = _clips()
    got = _run(clips, params)
    _same(got, clips, params)
    assert any((sum(len(y) for y in got[:k]) & 1) for k in range(len(got)))          # some segment does start odd


@pytest.mark.gpu
def test_the_long_clip_is_bit_exact():
    big = _big()
    got = _run([big], (12000, 2400, 1200))
    _same(got, [big], (12000, 2400, 1200))
    got = _run([big, big[:5]], (0, 0, 0))                                             # no fade, odd M: the raw quantisation
    _same(got, [big, big[:5]], (0, 0, 0))
    assert int(np.abs(got[0]).max()) == 32767


def test_a_reciprocal_multiply_would_show():
    """No GPU needed: the oracle's correctly rounded division and a multiply by 1 / peak differ on the long clip, so its bit-exact comparison
    above is decisive for the kernel's division."""
    x = _big().numpy()
    a, b = quantise(x), quantise(x, reciprocal=True)
    assert int((a != b).sum()) >= 1
    assert not np.array_equal(finish_ref(x, 12000, 2400, 1200), finish_ref(x, 12000, 2400, 1200, reciprocal=True))


@pytest.mark.gpu
def test_where_the_peak_sits():
    """9,000 samples = two whole peak tiles and a partial one; the peak first, last, inside the last partial tile, and negative."""
    base = (torch.randn(9000, generator=torch.Generator().manual_seed(3)) * 0.1).clamp(-0.5, 0.5)
    clips, at = [], [0, 8999, 8500, 4100]
    for k, i in enumerate(at):
        c = base.clone()
        c[i] = -0.9 if k == 3 else 0.9
        clips.append(c)
    got = _run(clips, (0, 0, 0))
    _same(got, clips, (0, 0, 0))
    for k, i in enumerate(at):
        assert int(got[k][i]) == (-32767 if k == 3 else 32767) and int(np.abs(np.delete(got[k], i)).max()) < 32767
    got = _run(clips, (7, 0, 50))
    _same(got, clips, (7, 0, 50))


@pytest.mark.gpu
def test_the_floor():
    zero = torch.zeros(5000)
    tiny = torch.full((5000,), 1e-7)
    tiny[::2] = -1e-7
    for params in [(0, 0, 0), (3, 4, 100)]:
        got = _run([zero, tiny], params)
        _same(got, [zero, tiny], params)
    assert not got[0].any() and int(np.abs(_run([tiny], (0, 0, 0))[0]).max()) == 3276        # 1e-7 / 1e-6 * 32767, truncated


def _varied(n, seed=11):
    g = torch.Generator().manual_seed(seed)
    lens = [0 if k % 9 == 4 else int(torch.randint(1, 6000, (1,), generator=g)) for k in range(n)]
    clips = [torch.randn(m, generator=g) * (0.05 + 0.01 * k) for k, m in enumerate(lens)]
    params = [(k % 5 * 37, k % 3 * 101, [0, 1, 50, 1200, 100000][k % 5]) for k in range(n)]
    return clips, params


@pytest.mark.gpu
def test_64_segments_each_with_its_own_parameters():
    clips, params = _varied(64)
    _same(_run(clips, params), clips, params)


@pytest.mark.gpu
def test_65_segments_take_two_calls(monkeypatch):
    from sesameai import finish as F
    clips, params = _varied(65, seed=12)
    calls = []
    real = F.lib

    class Spy:                                   # the library, with the segments of every mimi_fin_segments call noted
        def __getattr__(self, name):
            fn = getattr(real, name)
            if name != "mimi_fin_segments":
                return fn
            return lambda *a: calls.append(a[6]) or fn(*a)

    monkeypatch.setattr(F, "lib", Spy())
    got = _run(clips, params)
    assert calls == [64, 1]
    _same(got, clips, params)
    # the 65 segments are still views of one packed buffer, back to back
    out = _fin().finish([c.cuda() for c in clips], [F.SegmentFinish(*p) for p in params], sample_rate=1000)
    assert all(a.data_ptr() + 2 * a.numel() == b.data_ptr() for a, b in zip(out, out[1:]))


@pytest.mark.gpu
def test_raw_abi_refusals():
    from sesameai._abi import lib
    fin = _fin()
    x = torch.zeros(8, device="cuda")
    out = torch.full((64,), 77, dtype=torch.int16, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def call(n, n_in, lead=0):
        m = max(len(n_in), 1)
        ptrs = (C.c_void_p * m)(*[x.data_ptr()] * len(n_in))
        z = (C.c_int32 * m)()
        off, cnt = (C.c_long * m)(), (C.c_long * m)()
        rc = lib.mimi_fin_segments(fin._h, ptrs, (C.c_long * m)(*n_in), (C.c_int32 * m)(*[lead] * len(n_in)), z, z, n, out.data_ptr(), off, cnt, s)
        return rc, (lib.mimi_fin_last_error(fin._h) or b"").decode()

    rc, msg = call(0, [])
    assert rc == -1 and "1 .. 64" in msg
    rc, msg = call(65, [1] * 65)
    assert rc == -1 and "1 .. 64" in msg
    rc, msg = call(2, [4, -1])
    assert rc == -1 and "negative length" in msg
    rc, msg = call(1, [4], lead=-3)
    assert rc == -1 and "negative" in msg
    rc, msg = call(1, [(1 << 30) + 1])
    assert rc == -1 and "2^30" in msg
    torch.cuda.synchronize()
    assert bool((out == 77).all())                                                   # nothing was enqueued
    assert lib.mimi_fin_out_count(5, 12000, 2400) == 14405 and lib.mimi_fin_out_count(-1, 0, 0) == -1 and lib.mimi_fin_out_count(1 << 30, 1, 0) == -1
    rc, _ = call(1, [8])                                                              # the handle is still usable
    torch.cuda.synchronize()
    assert rc == 0 and not bool(out[:8].any()) and bool((out[8:] == 77).all())


@pytest.mark.gpu
def test_company_and_order_change_nothing():
    """Each of 8 segments: alone, among 63 others, and in a reversed list."""
    clips, params = _varied(64, seed=13)
    among = _run(clips, params)
    rev = _run(clips[::-1], params[::-1])[::-1]
    for k in range(0, 64, 8):
        alone = _run([clips[k]], [params[k]])[0]
        assert np.array_equal(alone, among[k]) and np.array_equal(alone, rev[k]), k
    for a, b in zip(among, rev):
        assert np.array_equal(a, b)


@pytest.mark.gpu
def test_non_finite_samples_stay_where_they_are():
    clips, params = _varied(6, seed=14)
    clips = [c.clone() for c in clips]
    clips[2] = torch.randn(5000, generator=torch.Generator().manual_seed(15)) * 0.2
    clean = _run(clips, params)
    bad = [c.clone() for c in clips]
    bad[2][[10, 4096, 4999]] = torch.tensor([float("nan"), float("inf"), float("-inf")])
    got = _run(bad, params)
    _same(got, bad, params)                                                           # the oracle: 0 there, the peak from the finite samples
    lead = params[2][0]
    plain = _run([bad[2]], (0, 0, 0))[0]
    assert plain[[10, 4096, 4999]].tolist() == [0, 0, 0] and int(np.abs(plain).max()) == 32767
    keep = np.ones(5000, bool); keep[[10, 4096, 4999]] = False
    assert np.array_equal(plain[keep], finish_ref(clips[2].numpy(), 0, 0, 0)[keep])   # (the three were not the peak: all others as without them)
    assert len(got[2]) == lead + 5000 + params[2][1]
    for k in (0, 1, 3, 4, 5):
        assert np.array_equal(got[k], clean[k])                                       # the other segments of the call
    again = _run(clips, params)                                                       # the handle's next call
    for a, b in zip(again, clean):
        assert np.array_equal(a, b)
