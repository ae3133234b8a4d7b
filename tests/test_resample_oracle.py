"""The resampler's oracle (tests/resample_ref.py) on the CPU: the written-out definition IS scipy.signal.resample_poly, the streamed
restatement equals the whole-clip one for the schedules the GPU tests use, and each way of breaking the streamed form moves some output
by at least 100 x the bound the GPU tests hold the kernel to -- so a kernel that passes them has none of these faults."""
import numpy as np
import pytest

import resample_ref as R

GPU_PAIRS = [(48000, 24000), (44100, 24000), (16000, 24000), (24000, 48000), (24000, 44100), (24000, 8000)]
SCHEDULES = {"ones": None, "uneven": [7, 333, 1, 659], "short": "look-ahead", "tail_alone": "all"}


def _noise(n, seed=0):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32).astype(np.float64)


def schedule(name, N, src, dst):
    """Chunk lengths of a clip of N samples; what is left over (maybe nothing) goes with ``final``."""
    up, down, half = R.rates(src, dst)
    if name == "ones":
        return [1] * N
    if name == "uneven":
        out, left = [], N
        for m in [7, 333, 1, 659]:
            out.append(min(m, left)); left -= out[-1]
        return out
    if name == "short":                                     # every chunk shorter than the look-ahead
        m = max(half // up - 1, 1)
        return [m] * (N // m)
    if name == "tail_alone":                                # everything, then n_in = 0 with final
        return [N]
    raise KeyError(name)


@pytest.mark.parametrize("src, dst", R.PAIRS)
def test_the_definition_is_scipys_resample_poly(src, dst):
    from scipy.signal import firwin, resample_poly
    up, down, half = R.rates(src, dst)
    want_h = firwin(2 * half + 1, 1.0 / max(up, down), window=("kaiser", 5.0)) * up
    assert np.abs(R.taps(up, down) - want_h).max() < 1e-15 * up
    for N in (1, 7, 333, 1000):
        x = _noise(N, N)
        want = resample_poly(x, up, down)
        got = R.resample_ref(x, src, dst)
        assert got.shape == want.shape and np.abs(got - want).max() < 1e-12, (N, np.abs(got - want).max())


@pytest.mark.parametrize("src, dst", R.PAIRS)
def test_the_streaming_count_is_what_the_look_ahead_allows(src, dst):
    up, down, half = R.rates(src, dst)
    assert half // up <= 30 and 2 * half // up + 1 <= 61
    for N in range(0, 400):
        e = R.emitted(N, up, down, half, False)
        # output n is free once its newest sample floor((n down + half) / up) has arrived: exactly the first e outputs
        assert all((n * down + half) // up <= N - 1 for n in range(max(e - 3, 0), e))
        assert (e * down + half) // up > N - 1
        assert e <= R.emitted(N, up, down, half, True) == -(-N * up // down)


@pytest.mark.parametrize("name", list(SCHEDULES))
@pytest.mark.parametrize("src, dst", GPU_PAIRS)
def test_streamed_equals_whole_clip(src, dst, name):
    for N in (1, 7, 333, 1000, 4097):
        if name == "ones" and N > 1000:                     # (single-sample feeds: 1000 of them pass every state the 4097 would)
            continue
        x = _noise(N, N + 1)
        want = R.resample_ref(x, src, dst)
        got = R.resample_streamed(x, src, dst, schedule(name, N, src, dst))
        assert got.shape == want.shape and np.abs(got - want).max() < 1e-13, (N, name)


def test_a_long_stream_keeps_small_numbers():
    s = R.StreamRef(44100, 24000)
    x = _noise(20000, 5)
    got = np.concatenate([s.feed(x[a:a + 1921]) for a in range(0, 20000, 1921)])
    assert 0 <= s.n_in <= s.down + s.H and 0 <= s.n_out <= 2 * s.up + s.down and s.k0 < -19000
    want = R.resample_ref(x, 44100, 24000)
    assert np.abs(got - want[:got.shape[0]]).max() < 1e-13 and got.shape[0] == R.emitted(20000, s.up, s.down, s.half, False)


def test_contaminated_range_is_where_a_nan_goes():
    for src, dst in GPU_PAIRS:
        x = _noise(333, 9)
        clean = R.resample_ref(x, src, dst)
        x[100] = np.nan
        y = R.resample_ref(x, src, dst)
        lo, hi = R.contaminated(333, src, dst, 100)
        bad = np.isnan(y)
        assert bad[lo:hi].all() and not bad[:lo].any() and not bad[hi:].any() and hi > lo
        assert np.array_equal(y[~bad], clean[~bad])


# ---- fault detectors: on the oracle alone ----------------------------------------------------------------------------------------------

def _bound(x, src, dst):
    return R.resample_ref(x, src, dst, with_bound=True)[1].max()


@pytest.mark.parametrize("src, dst", GPU_PAIRS)
@pytest.mark.parametrize("fault", ["shift", "phase", "half", "drop_history", "no_tail"])
def test_each_fault_moves_an_output_by_100_bounds(src, dst, fault):
    N = 1000
    x = _noise(N, 3)
    want = R.resample_ref(x, src, dst)
    got = R.resample_streamed(x, src, dst, schedule("uneven", N, src, dst), fault=fault)
    if fault == "no_tail":
        assert got.shape[0] < want.shape[0], "the tail is missing"
        got = np.concatenate([got, np.zeros(want.shape[0] - got.shape[0])])
    err = np.abs(got - want).max()
    assert err >= 100 * _bound(x, src, dst), (fault, err)
    assert _bound(x, src, dst) < 9e-6 * np.abs(x).max()


def test_an_input_shifted_by_one_sample_is_most_of_the_peak():
    x = _noise(1000, 3)
    want = R.resample_ref(x, 48000, 24000)
    got = R.resample_ref(np.concatenate([x[1:], [0.0]]), 48000, 24000)
    assert np.abs(got - want).max() > 0.5 * np.abs(want).max()


@pytest.mark.parametrize("src, dst", GPU_PAIRS)
def test_history_kept_across_a_reset_is_seen(src, dst):
    a, b = _noise(333, 4), _noise(333, 5)
    want = R.resample_ref(b, src, dst)
    for fault in (None, "stale_history"):
        s = R.StreamRef(src, dst, fault)
        R.resample_streamed(a, src, dst, [333], stream=s)            # clip a, ended: the history memory still holds its last samples
        s.feed(a[:50]); s.reset()                                    # ... and an open clip, reset
        got = R.resample_streamed(b, src, dst, [7, 100], stream=s)
        err = np.abs(got - want).max()
        assert (err < 1e-13) if fault is None else (err >= 100 * _bound(b, src, dst)), (fault, err)
