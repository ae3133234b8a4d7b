"""The integer loudness rule (tests/loudness_ref.py; include/mimi_hip.h, mimi_ld_pool_* and mimi_fin_segments_ld) against an independent
float64 ITU-R BS.1770-4 meter written here with scipy.signal.lfilter: the two biquads as IIR filters, 400 ms blocks with 75 % overlap, the
absolute and the relative gate.  The bound is +-0.1 LU: EBU Tech 3341's tolerance for a meter, not a measured number.  With T = 512 taps at
Q = 14 bits the rule stayed within 0.003 LU on the speech-like inputs, 0.004 on the square and 0.087 on the 60 Hz sine (the tight case: the
high-pass has the longest tail; T = 256 misses it by 0.46).  Also: that the relative gate is seen, the accumulator bound, the tap table
regenerated and compared, the chunk-schedule invariance of the reference itself, and the clip gain of the finisher."""
import math
import os

import numpy as np
import pytest

import finish_ref
import loudness_ref as L

scipy_signal = pytest.importorskip("scipy.signal")

RATE = 24000
BOUND = 0.1                 # LU, EBU Tech 3341


def speechlike(seconds=6.0, peak=0.9, seed=0):
    """band-limited noise (100 Hz .. 4 kHz) in syllable-like bursts, fp32"""
    rng = np.random.default_rng(seed)
    n = int(seconds * RATE)
    spec = np.fft.rfft(rng.standard_normal(n))
    f = np.fft.rfftfreq(n, 1.0 / RATE)
    spec[(f < 100) | (f > 4000)] = 0
    spec *= 1.0 / np.maximum(f, 100.0)                       # a falling spectrum
    x = np.fft.irfft(spec, n)
    t = np.arange(n) / RATE
    env = np.clip(np.sin(2 * np.pi * 3.1 * t + rng.uniform(0, 6)) + 0.3, 0, 1) * (np.sin(2 * np.pi * 0.4 * t) > -0.7)
    x = x * env
    return (x * (peak / np.abs(x).max())).astype(np.float32)


def sine(freq, seconds=5.0, db=-6.0):
    t = np.arange(int(seconds * RATE)) / RATE
    return (10 ** (db / 20) * np.sin(2 * np.pi * freq * t)).astype(np.float32)


def square(freq=3000.0, seconds=5.0):
    t = np.arange(int(seconds * RATE)) / RATE
    return np.where(np.sin(2 * np.pi * freq * t) >= 0, 1.0, -1.0).astype(np.float32)


def loud_then_quiet(seconds=8.0):
    x = speechlike(seconds, 0.9, seed=3).copy()
    x[x.shape[0] // 2:] *= np.float32(10 ** (-38 / 20))
    return x


def plosive():
    """a quiet sentence with one hard plosive: its peak says nothing about its loudness"""
    x = speechlike(6.0, 0.05, 2).copy()
    x[30000:30040] = np.float32(0.9) * np.hanning(40).astype(np.float32)
    return x


INPUTS = {
    "plosive": plosive,
    "speech 0.9": lambda: speechlike(6.0, 0.9, 1),
    "speech 0.05": lambda: speechlike(6.0, 0.05, 2),
    "sine 1 kHz": lambda: sine(1000.0),
    "sine 60 Hz": lambda: sine(60.0),
    "square 3 kHz": square,
    "loud then quiet": loud_then_quiet,
}
_made = {}


def clip(name):
    if name not in _made:
        _made[name] = INPUTS[name]()
    return _made[name]


def float_meter(x, relative=True):
    """BS.1770-4 integrated loudness of a mono clip at 24 kHz, float64, the filters as IIR biquads"""
    shelf, hp = L.loudness_taps.biquads(RATE)
    y = scipy_signal.lfilter(hp[0], hp[1], scipy_signal.lfilter(shelf[0], shelf[1], np.asarray(x, np.float64)))
    nb = (y.shape[0] - 4 * L.H) // L.H + 1
    z = np.array([np.mean(y[j * L.H:j * L.H + 4 * L.H] ** 2) for j in range(max(nb, 0))])
    with np.errstate(divide="ignore"):
        l = -0.691 + 10 * np.log10(z)
    keep = l > -70.0
    if relative and keep.any():
        keep &= l > -0.691 + 10 * np.log10(z[keep].mean()) - 10.0
    return -0.691 + 10 * np.log10(z[keep].mean()) if keep.any() else float("-inf")


def rule_lufs(x, relative=True):
    S, n, _, _ = L.measure_ref(x, relative=relative)
    return L.lufs(S, n)


def test_the_biquads_at_48_khz_are_the_standards():
    """the re-derivation, run at 48 kHz, gives the coefficients BS.1770-4 prints"""
    shelf, hp = L.loudness_taps.biquads(48000)
    assert np.allclose(shelf[0], [1.53512485958697, -2.69169618940638, 1.19839281085285], atol=1e-8, rtol=0)
    assert np.allclose(shelf[1], [1.0, -1.69065929318241, 0.73248077421585], atol=1e-8, rtol=0)
    assert hp[0] == [1.0, -2.0, 1.0]
    assert np.allclose(hp[1], [1.0, -1.99004745483398, 0.99007225036621], atol=1e-8, rtol=0)


def test_the_taps_are_the_generators_and_the_accumulator_cannot_overflow():
    hq = L.loudness_taps.taps()
    assert len(hq) == L.T == 512 and L.Q == 14 and np.array_equal(L.HQ, hq)
    assert all(-32768 <= v <= 32767 for v in hq)
    assert sum(abs(v) for v in hq) * 32768 < 2 ** 31
    # the cut impulse response IS scipy's, rounded
    shelf, hp = L.loudness_taps.biquads(RATE)
    imp = np.zeros(L.T); imp[0] = 1.0
    h = scipy_signal.lfilter(hp[0], hp[1], scipy_signal.lfilter(shelf[0], shelf[1], imp))
    assert np.abs(np.asarray(hq) - h * 2 ** L.Q).max() <= 0.5 + 1e-6
    # the worst input reaches the bound's neighbourhood and stays inside int32
    worst = np.where(np.asarray(hq[::-1]) >= 0, 32767, -32768).astype(np.int64)
    assert abs(int(np.dot(worst, np.asarray(hq[::-1], np.int64)))) + (1 << 13) < 2 ** 31


def test_the_library_holds_the_generated_table():
    text = open(L.loudness_taps.HEADER).read()
    assert text == L.loudness_taps.header_text()
    assert L.loudness_taps.parse_header(text) == L.loudness_taps.taps()
    plan = open(os.path.join(os.path.dirname(L.loudness_taps.HEADER), "loudness_plan.h")).read()
    assert f"#define LD_GATE_ABS {L.GATE_ABS}L" in plan and f"#define LD_H {L.H}" in plan and f"#define LD_RING_DEFAULT {L.RING}" in plan


@pytest.mark.parametrize("name", list(INPUTS))
def test_the_integer_rule_is_a_bs1770_meter(name):
    x = clip(name)
    want, got = float_meter(x), rule_lufs(x)
    print(f"{name}: float64 meter {want:.4f} LUFS, integer rule {got:.4f} LUFS, difference {got - want:+.4f} LU")
    assert abs(got - want) <= BOUND


def test_half_the_taps_miss_the_60_hz_sine():
    """the comparison tells T = 512 from T = 256"""
    x = clip("sine 60 Hz")
    hq = L.HQ[:256]
    e = L.hop_energies(L.to_s(x), hq)
    S, n = L.gate(e)
    assert abs(L.lufs(S, n) - float_meter(x)) > BOUND


def test_the_relative_gate_is_seen():
    x = clip("loud then quiet")
    assert float_meter(x, relative=False) < float_meter(x) - 2.0               # the float64 meter moves by 2.8 LU without the gate
    assert abs(rule_lufs(x, relative=False) - rule_lufs(x)) > BOUND
    assert abs(rule_lufs(x, relative=False) - float_meter(x, relative=False)) <= BOUND
    S, n, _, hops = L.measure_ref(x)
    Sa, na = L.gate(L.hop_energies(L.to_s(x)), relative=False)
    assert 0 < n < na <= hops - 3


def test_the_absolute_gate_and_short_clips():
    assert L.measure_ref(np.zeros(24000, np.float32)) == (0, 0, 0, 10)
    quiet = (speechlike(2.0, 1.0, 5) * np.float32(10 ** (-75 / 20)))
    S, n, peak, hops = L.measure_ref(quiet)
    assert (S, n) == (0, 0) and peak > 0 and hops == 20                         # nothing above -70 LUFS
    for N in (0, 1, 2399, 2400, 9599):
        S, n, peak, hops = L.measure_ref(clip("speech 0.9")[5000:5000 + N])
        assert (S, n, hops) == (0, 0, N // L.H)                                 # no block of 400 ms
    assert L.measure_ref(clip("speech 0.9")[5000:5000 + 9600])[1] == 1
    bad = np.array([np.nan, np.inf, -np.inf] * 4000, np.float32)
    assert L.measure_ref(bad) == (0, 0, 0, 5)
    assert L.measure_ref(np.full(3, -1.0, np.float32))[2] == 32768


SCHEDULES = {"one": None, "1": 1, "2399": 2399, "2401": 2401, "1920": 1920, "3840": 3840, "7": 7}


def cuts(N, step):
    if step is None:
        return [(0, N)]
    if step == 1:           # sample by sample across the first two hop edges only, the rest at once
        a = [(i, i + 1) for i in range(2396, min(2404, N))] if N > 2396 else []
        head = [(0, min(2396, N))]
        tail = [(min(2404, N), N)] if N > 2404 else []
        return head + a + tail
    return [(i, min(i + step, N)) for i in range(0, N, step)] or [(0, 0)]


@pytest.mark.parametrize("N", [0, 1, 510, 511, 2399, 2400, 2401, 9599, 9600, 9601, 24007])
def test_the_reference_does_not_depend_on_the_chunk_schedule(N):
    x = np.concatenate([clip("speech 0.9")[3000:], clip("square 3 kHz")])[:N]
    want_e = L.hop_energies(L.to_s(x))
    want = L.measure_ref(x)
    for name, step in SCHEDULES.items():
        st = L.StreamRef()
        got = []
        for a, b in cuts(N, step):
            got.append(st.feed(x[a:b]))
        got.append(st.feed(x[:0]))                            # an empty chunk
        got.append(st.feed(x[:0], final=True))
        assert np.array_equal(np.concatenate(got), want_e), (N, name)
        assert st.integrate() == want, (N, name)
        assert st.R == 0 and st.k == 0


def test_a_small_ring_holds_the_last_hops():
    x = clip("loud then quiet")[:60000]
    st = L.StreamRef(ring=8)
    st.feed(x[:31000]); st.feed(x[31000:], final=True)
    e = L.hop_energies(L.to_s(x))
    S, n = L.gate(e[-8:], 8)
    assert st.integrate() == (S, n, int(np.abs(L.to_s(x)).max()), 25) and (S, n) != L.gate(e)


def test_the_lufs_conversions():
    assert L.target_ms(-0.691) == 2 ** 30
    assert L.target_ms(-19) == int(round(2 ** 30 * 10 ** (-1.8309)))
    assert L.ceiling_i16(0) == 32767 and L.ceiling_i16(-1.0) == 29203 and L.ceiling_i16(-200) == 1
    # a full-scale 1 kHz sine reads -3.01 + the shelf's gain at 1 kHz: -3.0 LUFS within the bound, as BS.1770 has it for 997 Hz
    S, n, _, _ = L.measure_ref(sine(1000.0, db=0.0))
    assert abs(L.lufs(S, n) - float_meter(sine(1000.0, db=0.0))) <= BOUND and abs(L.lufs(S, n) + 3.0) < 0.2


def test_the_clip_gain_reaches_the_target_or_stops_at_the_ceiling():
    P_T, C = L.target_ms(-19.0), L.ceiling_i16(-1.0)
    seen = set()
    for name in ("speech 0.9", "speech 0.05", "square 3 kHz", "loud then quiet", "plosive"):
        x = clip(name)
        S, n, peak, _ = L.measure_ref(x)
        g, bound = L.clip_gain(S, n, peak, P_T, C)
        seen.add(bound)
        y = L.finish_ld_ref(x, 0, 0, 0, P_T, C)
        assert y.dtype == np.int16 and y.shape == x.shape and int(np.abs(y.astype(np.int64)).max()) <= C + 1
        S2, n2, peak2, _ = L.measure_ref(y)
        print(f"{name}: {L.lufs(S, n):.3f} LUFS, gain {float(g):.5f} ({'ceiling' if bound else 'target'}), then {L.lufs(S2, n2):.3f} LUFS, peak {peak2}")
        if bound:
            assert L.lufs(S2, n2) < -19.0 and abs(peak2 - C) <= 2
        else:
            assert abs(L.lufs(S2, n2) + 19.0) <= BOUND
    assert seen == {True, False}, "both a ceiling-limited and a target-limited clip must occur"
    # a louder target on the same speech clip: the ceiling binds
    S, n, peak, _ = L.measure_ref(clip("speech 0.9"))
    assert L.clip_gain(S, n, peak, L.target_ms(-5.0), C)[1] and not L.clip_gain(S, n, peak, L.target_ms(-30.0), C)[1]


def test_without_a_gated_block_the_finisher_keeps_the_peak_rule():
    P_T, C = L.target_ms(-19.0), L.ceiling_i16(-1.0)
    for x in (clip("speech 0.9")[:9599], np.zeros(20000, np.float32), clip("speech 0.9")[:0],
              speechlike(2.0, 1.0, 5) * np.float32(10 ** (-75 / 20))):
        assert L.measure_ref(x)[1] == 0
        assert np.array_equal(L.finish_ld_ref(x, 120, 50, 30, P_T, C), finish_ref.finish_ref(x, 120, 50, 30))
    x = clip("speech 0.9")
    assert np.array_equal(L.finish_ld_ref(x, 120, 50, 30, 0, C), finish_ref.finish_ref(x, 120, 50, 30))
    assert not np.array_equal(L.finish_ld_ref(x, 120, 50, 30, P_T, C), finish_ref.finish_ref(x, 120, 50, 30))
    assert math.isinf(L.lufs(0, 0))
