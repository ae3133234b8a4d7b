"""The time-stretch rule (tests/stretch_ref.py) graded on the CPU: the streamed restatement equals the whole-clip rule for every schedule the
GPU tests use, the carry fits its 2,560 floats for every speed, the counts follow the formulas, and the two things that make the rule what
it is -- the alignment search and the first-index tie-break -- are each shown to matter on signals where getting them wrong is gross."""
import numpy as np
import pytest

import stretch_ref as S

PMS = [500, 730, 1200, 1999, 2000]
LENGTHS = [0, 1, 511, 512, 513, 1279, 1280, 1281, 2047, 5000, 20011]
CHUNKS = [0, 1, 7, 255, 512, 1280, 1920, 4000]


def noise(n, seed=0, amp=0.3):
    return (np.random.default_rng(seed).standard_normal(n) * amp).astype(np.float32)


def voiced(n, seed=0):
    """a speech-like test signal: a 140 Hz pulse train's harmonics under a slow envelope, plus a little noise"""
    t = np.arange(n) / 24000.0
    x = sum(np.sin(2 * np.pi * 140.0 * h * t + h) / h for h in range(1, 9)) * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t))
    return (0.2 * x + 0.01 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def schedules(N, seed):
    """three chunk schedules of a clip of N samples: random draws from CHUNKS, all at once, and final alone after everything"""
    rng = np.random.default_rng(seed)
    rand = [int(rng.choice(CHUNKS)) for _ in range(64)]
    return {"random": rand, "whole_then_final_alone": [N], "ones_and_zeros": [0, 1, 0, 1279, 1, 0, 0, 512]}


def tie_clip(N=6000, seed=11):
    """a period-64 sine on the 1/2048 grid plus noise below 2^-14: q is exactly periodic, x is not"""
    base = np.rint(np.sin(2 * np.pi * np.arange(N) / 64.0) * 0.4 * 2048.0) / 2048.0
    return (base + np.random.default_rng(seed).uniform(-1.0, 1.0, N) * 2.0 ** -15).astype(np.float32)


def square(N=4000):
    return np.where((np.arange(N) // 50) % 2 == 0, 4.0, -4.0).astype(np.float32)


@pytest.mark.parametrize("pm", PMS)
def test_chunked_equals_one_shot(pm):
    for N in LENGTHS:
        x = voiced(N, N) if N % 2 else noise(N, N)
        want_y, want_d = S.stretch_ref(x, pm)
        assert want_y.shape[0] == S.out_len(N, pm) and want_d.shape[0] == -(-want_y.shape[0] // S.H)
        for name, sch in schedules(N, N + pm).items():
            y, d = S.stretch_streamed(x, pm, sch)
            assert np.array_equal(y, want_y) and np.array_equal(d, want_d), (pm, N, name)


def test_the_carry_fits_for_every_speed():
    worst = max(S.history_needed(pm) for pm in range(S.PM_MIN, S.PM_MAX + 1))
    assert worst == 2559 < S.CARRY


@pytest.mark.parametrize("pm", PMS)
def test_lengths_and_counts_follow_the_formulas(pm):
    for N in list(range(0, 3000, 37)) + LENGTHS:
        M = S.out_len(N, pm)
        assert (M - 1) * pm < N * 1000 <= M * pm or N == M == 0
        e = S.emitted(N, pm, False)
        # block k is out exactly when a_k + D + 2H <= N, and every such block lies whole inside the final output
        assert all(S.a_of(k, pm) + S.LOOK <= N for k in range(e)) and S.a_of(e, pm) + S.LOOK > N
        assert e * S.H <= M and e <= S.emitted(N, pm, True) == -(-M // S.H)
        assert S.out_count(0, 0, pm, N, False) == e * S.H and S.out_count(0, 0, pm, N, True) == M
    # a stream's counts add up over any split
    s = S.StreamRef(pm)
    got = sum(s.feed(noise(n, n))[0].shape[0] for n in (1279, 1, 0, 1920, 4000))
    assert got == S.emitted(7200, pm, False) * S.H
    assert got + s.feed(noise(5), final=True)[0].shape[0] == S.out_len(7205, pm)
    assert (s.R, s.k) == (0, 0)


def _envelope_min(y, lo, hi, win=240):
    e = [np.abs(y[i:i + win]).max() for i in range(lo, hi - win, 16)]
    return min(e)


@pytest.mark.parametrize("pm", [1200, 800])
def test_the_search_keeps_a_sine_whole(pm):
    x = (0.5 * np.sin(2 * np.pi * 200.0 * np.arange(24000) / 24000.0)).astype(np.float32)
    y, d = S.stretch_ref(x, pm)
    y0, d0 = S.stretch_ref(x, pm, search=False)
    assert not d0.any() and d[1:].any()
    lo, hi = 1024, y.shape[0] - 2048                         # (away from the clip's ends, where the zero extension is mixed in)
    with_search, without = _envelope_min(y, lo, hi), _envelope_min(y0, lo, hi)
    print(f"pm={pm}: envelope minimum {with_search:.4f} with the search, {without:.4f} with d = 0")
    assert with_search >= 0.49 and without < 0.46


def test_the_zero_crossing_rate_of_a_voiced_signal_stays():
    x = voiced(24000, 1)
    zc = lambda v: int(np.count_nonzero(np.signbit(v[1:]) != np.signbit(v[:-1])))
    y, _ = S.stretch_ref(x, 1200)
    rate_in, rate_out = zc(x) / x.shape[0], zc(y) / y.shape[0]
    assert abs(rate_out - rate_in) < 0.1 * rate_in             # the pitch stays


def test_the_tie_break_is_decisive():
    x = tie_clip()
    q = S.quant(x)
    assert np.array_equal(q[:-64], q[64:]) and not np.array_equal(x[:-64], x[64:])
    y, d = S.stretch_ref(x, 1250)
    y2, d2 = S.stretch_ref(x, 1250, tie="last")
    blocks = int(np.count_nonzero(d[1:] != d2[1:]))
    moved = int(np.count_nonzero(y != y2))
    print(f"last-index argmax: {blocks} of {d.shape[0] - 1} blocks pick another d, {moved} samples change")
    assert blocks == d.shape[0] - 1 == 9 and moved > 2000


def test_a_full_scale_square_reaches_the_largest_score():
    y, d, top = S.stretch_ref(square(), 1000, want_scores=True)
    assert top == 512 * 2047 * 2047 == 2145387008 < 2 ** 31
    assert S.quant(np.array([4.0, -4.0, 0.99999, np.inf, -np.inf, np.nan, 2.0 ** -11 * 1.5, 2.0 ** -11 * 2.5], dtype=np.float32)).tolist() == \
        [2047, -2047, 2047, 0, 0, 0, 2, 2]                   # clamp; non-finite -> 0; halves round to even


def test_silence_picks_the_first_candidate():
    y, d = S.stretch_ref(np.zeros(5000, dtype=np.float32), 1200)
    assert not y.any() and d[0] == 0 and (d[1:] == -S.D).all() and d.shape[0] > 5


def test_a_non_finite_sample_enters_no_decision():
    x = noise(6000, 2)
    bad = x.copy(); bad[3000] = np.nan
    zero = x.copy(); zero[3000] = 0.0
    y, d = S.stretch_ref(bad, 1200)
    yz, dz = S.stretch_ref(zero, 1200)
    assert np.array_equal(d, dz)
    nan = np.isnan(y)
    assert 1 <= nan.sum() <= 2 and np.array_equal(y[~nan], yz[~nan])
