"""The limiter's rule on its own (tests/limiter_ref.py; include/mimi_hip.h, mimi_lim_pool_*), no GPU: the recursion of the release equals
its windowed form, the gain never exceeds what a sample requires, nothing finite leaves above the ceiling and the clamp stays idle, a clip
under the ceiling passes untouched, a lone spike is met exactly with the gain falling from L samples ahead of it, a stream over any chunk
schedule is the one-shot result, NaN and Inf touch nothing else, and the meter tests' own speech 12 dB hot is limited and stays under C."""
import numpy as np
import pytest

import limiter_ref as R
from test_loudness_oracle import speechlike

ONE = R.ONE
TILE = 4096                                                   # the device's tile: the schedules split around its edge
GRID = [(L, rho, hr, C) for L in (1, 7, 120, 480) for rho in (8, 27, 1000, 65536) for hr in (0, 2) for C in (1, 1000, 29204, 32767)]


def noise(N, seed, scale=1.0, kind="fp32"):
    rng = np.random.default_rng(seed)
    x = np.clip(rng.standard_normal(N) * scale * rng.choice([0.02, 0.3, 1.0], N), -0.999, 0.999).astype(np.float32)
    return x if kind == "fp32" else np.clip(np.rint(x * 32768.0), -32768, 32767).astype(np.int16)


def peak_i16(y):
    return np.abs(y.astype(np.float64)).max(initial=0.0) * (32768.0 if y.dtype == np.float32 else 1.0)


def test_the_defaults():
    assert R.params() == R.Params(29203, 120, 27, 0) and R.Params().K == 2428 and R.Params(rho=8).K == 8192 and R.Params(rho=65536).K == 1
    assert R.params(release_ms=1e6).rho == 8 and R.params(release_ms=50.0).rho == 55 and R.params(ceiling_db=0.0).C == 32767
    for bad in (dict(lookahead=0), dict(lookahead=481), dict(drive_shift=5), dict(drive_shift=-1), dict(release_ms=0.04 / 24)):
        with pytest.raises(AssertionError):
            R.params(**bad)


@pytest.mark.parametrize("L,rho", [(1, 8), (7, 27), (120, 1000), (480, 65536), (120, 27), (480, 8)])
def test_the_recursion_equals_the_windowed_form(L, rho):
    for seed, N in enumerate((0, 1, L, 700, 3000)):
        m = R.required(noise(N, seed), R.Params(9000, L, rho, 1))
        w = R.window_min(np.concatenate([np.full(L, ONE), m, np.full(L, ONE)]).astype(np.int64), L)
        e = R.release_recursive(w, rho)
        assert np.array_equal(e, R.release(w, rho)) and np.array_equal(e, R.release_windowed(w, rho)), (L, rho, N)
        assert np.array_equal(R.gains(m, R.Params(9000, L, rho, 1), R.release_recursive), R.gains(m, R.Params(9000, L, rho, 1)))


@pytest.mark.parametrize("kind", ["fp32", "int16"])
def test_the_gain_never_exceeds_the_need_and_nothing_leaves_above_the_ceiling(kind):
    limited = 0
    for k, (L, rho, hr, C) in enumerate(GRID):
        p = R.Params(C, L, rho, hr)
        x = noise(int(np.random.default_rng(k).integers(0, 2500)), k, 2.0 ** -hr, kind)            # |x 2^hr| < 32768
        w = R.limit_ref(x, p)
        assert (w.g <= w.m).all() and (w.g >= 0).all() and w.y.dtype == x.dtype and w.y.shape == x.shape
        assert peak_i16(w.y) <= C and w.row[3] == 0, p                                              # without the clamp
        assert w.row == (int(w.g.min()) if x.shape[0] else ONE, x.shape[0], int((w.g < ONE).sum()), 0)
        limited += w.limited
    assert limited > 0


@pytest.mark.parametrize("kind", ["fp32", "int16"])
def test_a_clip_under_the_ceiling_passes_untouched(kind):
    x = noise(9000, 3, 0.25, kind)
    p = R.Params(int(peak_i16(x)) + 1, 120, 27, 0)
    w = R.limit_ref(x, p)
    assert np.array_equal(w.y, x) and w.row == (ONE, 9000, 0, 0)
    st = R.LimiterRef(p)
    ys = [st.feed(x[a:b]) for a, b in ((0, 100), (100, 5000), (5000, 9000))] + [st.feed(x[:0], final=True)]
    assert [y.shape[0] for y in ys] == [0, 4880, 4000, 120] and np.array_equal(np.concatenate(ys), x)


@pytest.mark.parametrize("L,rho,hr,C", [(120, 27, 2, 29204), (1, 27, 0, 29204), (480, 1000, 0, 1), (7, 65536, 2, 32767), (120, 8, 0, 1000)])
def test_a_lone_spike_is_met_exactly_and_from_L_samples_ahead(L, rho, hr, C):
    p = R.Params(C, L, rho, hr)
    at, N = 600, 600 + p.K + 2 * L + 50
    for x in (np.zeros(N, np.int16), np.zeros(N, np.float32)):
        x[at] = -32768 if x.dtype == np.int16 else -1.0
        w = R.limit_ref(x, p)
        a = 32768 << hr
        assert C - 1 - (a >> 16) <= peak_i16(w.y[at:at + 1]) <= C and w.row[3] == 0
        low = np.nonzero(w.g < ONE)[0]
        assert low[0] == at - L and low[-1] <= at + p.K + 2 * L and w.g[at] == w.m[at] == (C << 16) // a
        assert (np.diff(w.g[at - L:at + 1]) <= 0).all() and (np.diff(w.g[at + L:]) >= 0).all()      # down to the peak, up after the hold
    x = np.zeros(2000, np.int16)
    x[1000] = -32768
    assert R.limit_ref(x, R.Params(29204, 120, 27, 2)).y[1000] == -29204                            # exactly -C


def schedules(N, L):
    return {"inside L": [L // 2, 1, L - L // 2 - 1, 1, 1], "around L": [L - 1, 2, L + 1, L, L + 1],
            "sample by sample over a tile edge": [TILE + L - 2, 1, 1, 1, 1], "an empty chunk": [500, 0, 0, 700, 0],
            "frames": [3840] + [1920] * 3, "one": [N]}


@pytest.mark.parametrize("kind", ["fp32", "int16"])
@pytest.mark.parametrize("L,rho", [(120, 27), (1, 65536), (480, 8), (7, 1000)])
def test_stream_equals_one_shot(L, rho, kind):
    p = R.Params(9000, L, rho, 1)
    for N in (0, 1, L, L + 1, 3000, TILE + L + 700):
        x = noise(N, N + L, 0.5, kind)
        want = R.limit_ref(x, p)
        for name, steps in schedules(N, L).items():
            for closing in ("with the last chunk", "with an empty chunk"):
                st = R.LimiterRef(p)
                ys, a = [], 0
                for c in steps + [N]:
                    c = min(c, N - a)
                    last = a + c == N and closing == "with the last chunk"
                    assert st.out_count(c, last) == (N if last else max(0, a + c - L)) - st.E
                    ys.append(st.feed(x[a:a + c], final=last))
                    a += c
                    if last:
                        break
                if closing == "with an empty chunk":
                    ys.append(st.feed(x[:0], final=True))
                    assert ys[-1].shape[0] == min(L, N)                                    # the latency: L samples
                y = np.concatenate(ys)
                assert y.dtype == x.dtype and np.array_equal(y, want.y) and st.row == want.row, (N, name, closing)
                assert (st.R, st.E) == (0, 0)                                               # fresh, with the same parameters
                assert np.array_equal(st.feed(x, final=True), want.y) and st.row == want.row, "the next clip on the same stream"
    assert R.limit_ref(noise(3000, 3000 + L, 0.5, kind), p).limited > 0


def test_nan_and_inf_touch_nothing_else():
    p = R.Params(29204, 120, 27, 0)
    clean = noise(9000, 11, 0.3)
    x = clean.copy()
    x[3000], x[5000], x[7000], x[8000] = np.nan, np.inf, -np.inf, 1e30
    w, c = R.limit_ref(x, p), R.limit_ref(clean, p)
    Cf = np.float32(p.C) / np.float32(32768)
    assert np.isnan(w.y[3000]) and w.y[5000] == Cf and w.y[7000] == -Cf and w.y[8000] == Cf and w.row[3] == 3
    assert w.m[3000] == ONE and w.m[5000] == w.m[7000] == w.m[8000] == (p.C << 16) >> 30
    assert np.array_equal(w.g[:5000 - 120], c.g[:5000 - 120]) and np.array_equal(np.delete(w.y[:4880], 3000), np.delete(c.y[:4880], 3000))
    assert np.isfinite(np.delete(w.y, 3000)).all() and peak_i16(np.delete(w.y, 3000)) <= p.C
    st = R.LimiterRef(p)
    y = np.concatenate([st.feed(x[:3001]), st.feed(x[3001:5001]), st.feed(x[5001:], final=True)])
    assert np.array_equal(y, w.y, equal_nan=True) and st.row == w.row


@pytest.mark.parametrize("kind", ["fp32", "int16"])
def test_speech_12_dB_hot_is_limited_and_stays_under_the_ceiling(kind):
    x = speechlike(6.0, 0.9, 1)
    x = x if kind == "fp32" else np.rint(x * 32767.0).astype(np.int16)
    p = R.params(drive_shift=2)                                                              # 12.04 dB of drive
    w = R.limit_ref(x, p)
    print(f"speech 12 dB hot ({kind}): {w.limited} of {x.shape[0]} samples limited, min gain {w.row[0] / ONE:.3f}, peak out {peak_i16(w.y):.0f}")
    assert w.limited > 0 and peak_i16(w.y) <= p.C and w.row[3] == 0 and w.row[0] < ONE // 2
    assert peak_i16(x) * 4 > 2 * p.C                                                         # what a clamp would have flattened
