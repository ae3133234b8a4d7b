"""The true-peak rule itself (tests/truepeak_ref.py), on the CPU: the committed taps against their generator and their check values; the
meter against the float64 values of inputs band-limited to 8 kHz on a 32x grid, and against a 32x resample_poly, with bounds computed here
from the taps; the limiter's properties on
five inputs (an fs/4 tone at 45 degrees, a 3 kHz square, white noise, noise band-limited to 11 kHz, speech-like bursts); the stream form
against the one-shot rule; and the finisher's clip gain with the true peak in the place of the sample peak.

Measured on these five inputs (dB by which the limiter's OUTPUT passes the ceiling in its own integer true peak -- not exact, because the
gain moves between samples; docs/experiments/true_peak.md): at the defaults L = 120 the worst is +0.0048 dB (the noise to 11 kHz), at
L = 480 +0.0009 dB, at L = 1 +0.34 dB.  At the defaults the test asserts 4 x the measured worst; at L = 1 it only reports."""
import math

import numpy as np
import pytest

import limiter_ref as R
import loudness_ref as LD
import truepeak_ref as P

RATE = 24000
T = P.T
WORST_AT_DEFAULTS_DB = 0.0048          # measured here, on ``table()``; the assertion allows 4 x
_cache = {}


def _speechlike(seconds, seed=0):
    """tests/test_loudness_oracle.py ``speechlike`` without its module's SciPy: band-limited noise (100 Hz .. 4 kHz) in syllable-like bursts"""
    rng = np.random.default_rng(seed)
    n = int(seconds * RATE)
    spec = np.fft.rfft(rng.standard_normal(n))
    f = np.fft.rfftfreq(n, 1.0 / RATE)
    spec[(f < 100) | (f > 4000)] = 0
    spec *= 1.0 / np.maximum(f, 100.0)
    x = np.fft.irfft(spec, n)
    t = np.arange(n) / RATE
    x = x * np.clip(np.sin(2 * np.pi * 3.1 * t + rng.uniform(0, 6)) + 0.3, 0, 1) * (np.sin(2 * np.pi * 0.4 * t) > -0.7)
    return x * (0.9 / np.abs(x).max())


def table(seconds=2.0):
    """the five inputs, fp32, as hot as the issue's table has them"""
    if "table" not in _cache:
        rng = np.random.default_rng(0)
        n = int(seconds * RATE)
        t = np.arange(n)
        spec = np.fft.rfft(rng.standard_normal(n))
        spec[np.fft.rfftfreq(n, 1.0 / RATE) > 11000] = 0
        band = np.fft.irfft(spec, n)
        _cache["table"] = {
            "fs/4 sine, 45 degrees, 1.3 x full scale": (1.3 * np.sin(np.pi / 2 * t + np.pi / 4)).astype(np.float32),
            "3 kHz square": np.where((t // 4) % 2 == 0, 1.0, -1.0).astype(np.float32),
            "white noise, sigma 0.5": (0.5 * rng.standard_normal(n)).astype(np.float32),
            "noise to 11 kHz, 3 x full scale": (3.0 * band / np.abs(band).max()).astype(np.float32),
            "speechlike, 12 dB hot": (_speechlike(seconds) * 10 ** (12 / 20)).astype(np.float32),
        }
    return _cache["table"]


def _db(a, b):
    return 20.0 * math.log10(a / b)


def test_the_committed_taps_are_the_generators_and_have_the_check_values():
    tt = P.truepeak_taps
    assert open(tt.HEADER).read() == tt.header_text()
    H = tt.parse_header(open(tt.HEADER).read())
    assert H == tt.taps() and np.array_equal(np.array(H), P.H) and P.H.shape == (3, 2 * T) and (tt.T, tt.Q, tt.OS) == (8, 14, 4)
    assert [int(r.sum()) for r in P.H] == [16385, 16388, 16385]
    assert [int(np.abs(r).sum()) for r in P.H] == [27451, 31572, 27451]
    assert int(P.H.max()) == 14693 and np.array_equal(P.H[0], P.H[2][::-1]) and np.array_equal(P.H[1], P.H[1][::-1])
    assert 31572 * 2 ** 15 < 2 ** 30 and ((31572 << 30) + (1 << 13)) >> 14 < 2 ** 31          # the narrow accumulator; a_tp fits 31 bits
    # the definition, spelled out once more: H[p][k + 7] = rint(h(p - 4 k) 2^14)
    h = lambda n: float(np.sinc(n / 4.0) * np.kaiser(63, 8.0)[n + 31]) if -31 <= n <= 31 else 0.0
    assert all(P.H[p - 1][k + 7] == int(np.rint(h(p - 4 * k) * 2 ** 14)) for p in (1, 2, 3) for k in range(-7, 9))


def _passband_error(f_max=8000.0):
    """the largest |H_p(w) - e^{j w p / 4}| over the three phases and w up to f_max: what the committed taps do to a tone, relative to it"""
    w = 2 * np.pi * np.linspace(0.0, f_max, 801) / RATE
    k = np.arange(-(T - 1), T + 1)                                   # tap k + 7 multiplies sample i - 1 + k; the point lies p / 4 behind i - 1
    worst = 0.0
    for p in (1, 2, 3):
        resp = (P.H[p - 1][None, :] / 2.0 ** P.Q * np.exp(1j * w[:, None] * k[None, :])).sum(axis=1)
        worst = max(worst, float(np.abs(resp - np.exp(1j * w * p / 4.0)).max()))
    return worst


N_TONES, LO, HI = 6000, 500, 5500       # samples of a case; the stretch that is measured, away from the ends, where the clip is not band-limited


def _tone_cases():
    """sums of tones of 8 kHz and less: single tones at three phases, and six sums of twelve"""
    rng = np.random.default_rng(3)
    cases = [[(f, 0.5, ph)] for f in (50.0, 1000.0, 3000.0, 6000.0, 7999.0, 8000.0) for ph in (0.0, 0.3, math.pi / 4)]
    return cases + [[(float(rng.uniform(20, 8000)), float(a), float(rng.uniform(0, 6.28))) for a in rng.uniform(0.01, 0.08, 12)] for _ in range(6)]


def _value(tones, t):
    return sum(a * np.sin(2 * np.pi * f * t / RATE + ph) for f, a, ph in tones)


def _meter_and_bounds(tones):
    """-> (the meter's reading of samples LO .. HI - 1, whose intervals LO .. HI span the times LO - 1 .. HI; the largest error the issue
    allows it on either side, in int16 units: the taps' pass-band error times the sum of the amplitudes -- the error of a sum of tones --
    and 2.5 for the integers: a sample is rounded up by less than 1, which is less than sum |H| / 2^14 < 2 behind the taps, and U's own
    rounding is 0.5)"""
    x = _value(tones, np.arange(N_TONES)).astype(np.float32)
    amps = sum(a for _, a, _ in tones) * 32768.0
    return x, float(P.magnitude_tp(x, 0)[LO:HI].max()), _passband_error() * amps + 2.5


GRID = math.cos(math.pi * 8000.0 / 96000.0)        # what the spacing of the 4x grid can hide of a peak at 8 kHz: 0.30 dB


def test_the_meter_against_the_float64_values_of_tones_of_8_khz_and_less():
    """The inputs' exact values between the samples are known, on the 32x grid over exactly the times the meter's stretch spans.  The
    under-read is at most the spacing of the 4x grid plus the taps' pass-band error, the over-read at most that error; both computed from
    the committed taps, nothing else added."""
    assert 0.29 < -20.0 * math.log10(GRID) < 0.31 and _passband_error() < 2e-3
    worst_under = worst_over = 0.0
    for tones in _tone_cases():
        x, got, slack = _meter_and_bounds(tones)
        true_peak = float(np.abs(_value(tones, np.arange((LO - 1) * 32, HI * 32 + 1) / 32.0)).max()) * 32768.0
        assert true_peak * GRID - slack <= got <= true_peak + slack, (tones[0], true_peak, got, slack)
        worst_under, worst_over = max(worst_under, (true_peak - got) / true_peak), max(worst_over, (got - true_peak) / slack)
    print(f"taps' pass-band error to 8 kHz {_passband_error():.2e}; worst under-read {worst_under:.4f} of the peak (the grid allows {1 - GRID:.4f}); "
          f"worst over-read {worst_over:.2f} of what the taps' error and the integers allow")
    # the fs/4 tone at 45 degrees reads +3.01 dB over its sample peak, within the taps' error AT fs/4 (and the integers)
    t = np.arange(4000)
    x = np.sin(np.pi / 2 * t + np.pi / 4).astype(np.float32) * np.float32(0.9)
    sp, tp = int(R.magnitude(x, 0)[100:3900].max()), int(P.magnitude_tp(x, 0)[100:3900].max())          # (away from the tone's onset and end)
    assert abs(_db(tp, sp) - 3.0103) <= _db(1 + _passband_error(6000.0), 1) + _db(sp + 3, sp), _db(tp, sp)


def test_the_meter_against_a_float64_32x_resample_poly():
    """The same cases and the same bounds against scipy.signal.resample_poly(x, 32, 1) over the same times.  That measure has an error
    of its own -- its filter's, measured here against the tones themselves -- and only that is added."""
    sig = pytest.importorskip("scipy.signal")
    worst_ref = 0.0
    for tones in _tone_cases():
        x, got, slack = _meter_and_bounds(tones)
        ref32 = sig.resample_poly(x.astype(np.float64), 32, 1)[(LO - 1) * 32:HI * 32 + 1]
        ref_err = float(np.abs(ref32 - _value(tones, np.arange((LO - 1) * 32, HI * 32 + 1) / 32.0)).max()) * 32768.0
        true_peak = float(np.abs(ref32).max()) * 32768.0
        assert true_peak * GRID - slack - ref_err <= got <= true_peak + slack + ref_err, (tones[0], true_peak, got, slack, ref_err)
        worst_ref = max(worst_ref, ref_err / (sum(a for _, a, _ in tones) * 32768.0))
    print(f"the 32x reference's own error: {worst_ref:.2e} of the amplitudes")


def test_the_limiters_properties_on_the_five_inputs():
    report = {}
    for name, x in table().items():
        a, a_tp = R.magnitude(x, 0), P.magnitude_tp(x, 0)
        assert (a_tp >= a).all() and (a_tp > a).any(), name
        for L in (120, 1, 480):
            p = R.Params(29203, L, 27, 0)
            tp, sm = P.limit_tp_ref(x, p), R.limit_ref(x, p)
            assert (tp.m <= sm.m).all() and (tp.g <= sm.g).all() and (tp.g < sm.g).any(), (name, L)      # never above the sample-peak gain
            assert np.abs(tp.y.astype(np.float64)).max() * 32768.0 <= p.C, (name, L)                      # |y| <= C still holds exactly
            q = np.clip(np.rint(x.astype(np.float64) * 8192.0), -32768, 32767).astype(np.int16)           # the same through int16, hr = 2
            ti = P.limit_tp_ref(q, p._replace(hr=2))
            assert np.abs(ti.y.astype(np.int64)).max() <= p.C and (ti.g <= R.limit_ref(q, p._replace(hr=2)).g).all()
            over = _db(P.measure_tp(tp.y)[1], p.C)
            report[(name, L)] = (over, _db(P.measure_tp(sm.y)[1], p.C))
    for (name, L), (over, plain) in sorted(report.items(), key=lambda kv: kv[0][1]):
        print(f"L = {L:3d}  {name:42s} output true peak {over:+.4f} dB over C (sample-peak limiter: {plain:+.3f} dB)")
    worst = max(v[0] for (name, L), v in report.items() if L == 120)
    assert worst <= 4 * WORST_AT_DEFAULTS_DB, worst
    assert all(v[1] > v[0] for v in report.values()), "the sample-peak limiter leaves more over the ceiling on every input"
    assert max(v[1] for v in report.values()) > 3.0                                                        # ... +3 dB on the fs/4 tone


def test_a_clip_whose_true_peak_is_under_the_ceiling_comes_out_as_it_went_in():
    p = R.params()
    for name, x in table().items():
        quiet = (x * np.float32(0.5 * p.C / P.measure_tp(x)[1])).astype(np.float32)
        assert P.measure_tp(quiet)[1] < p.C
        w = P.limit_tp_ref(quiet, p)
        assert np.array_equal(w.y, quiet) and w.row == (R.ONE, quiet.shape[0], 0, 0), name
        st = P.TruePeakLimiterRef(p)
        first = st.feed(quiet[:1000])
        assert first.shape[0] == 1000 - p.L - T and np.array_equal(first, quiet[:1000 - p.L - T])          # delayed by L + T
        assert np.array_equal(np.concatenate([first, st.feed(quiet[1000:], final=True)]), quiet)


SCHEDULES = {"whole": [], "shorter than T": [1, 2, 3, 4, 5, 6, 7] * 30, "single samples across a tile edge": [4096 + 120 + T - 3] + [1] * 8,
             "empty chunks": [5, 0, 0, 700, 0, 1, 0, 0, 4000], "around the latency": [127, 1, 1, 128, 129, 7, 8, 9]}


@pytest.mark.parametrize("kind", ["fp32", "int16"])
def test_the_stream_form_equals_the_one_shot_rule(kind):
    rng = np.random.default_rng(7)
    for p in (R.Params(), R.Params(9000, 1, 65536, 1), R.Params(20000, 480, 8, 0), R.Params(1000, 7, 1000, 2)):
        N = 9000
        x = (rng.standard_normal(N) * 0.5 * 2.0 ** -p.hr).astype(np.float32)
        if kind == "int16":
            x = np.clip(np.rint(x * 32768.0), -32768, 32767).astype(np.int16)
        want = P.limit_tp_ref(x, p)
        assert want.limited > 0 and not np.array_equal(want.y, R.limit_ref(x, p).y)
        st = P.TruePeakLimiterRef(p)
        for name, steps in SCHEDULES.items():
            for empty_final in (False, True):                        # ... and the stream reused after `final` every time
                ys, at, R_, E_ = [], 0, 0, 0
                for c in steps:
                    c = min(c, N - at)
                    assert st.out_count(c) == max(0, R_ + c - p.L - T) - E_
                    ys.append(st.feed(x[at:at + c]))
                    at, R_, E_ = at + c, R_ + c, E_ + ys[-1].shape[0]
                ys.append(st.feed(x[at:], final=not empty_final))
                if empty_final:
                    assert ys[-1].shape[0] == max(0, N - p.L - T) - E_
                    ys.append(st.feed(x[:0], final=True))
                y = np.concatenate(ys)
                assert y.dtype == x.dtype and np.array_equal(y, want.y) and st.row == want.row, (kind, p, name, empty_final)
    st = P.TruePeakLimiterRef(R.Params())
    assert st.feed(np.zeros(0, np.float32), final=True).shape[0] == 0 and st.out_count(128) == 0 and st.out_count(129) == 1


def test_measure_tp_names_the_first_position_of_the_true_peak():
    x = np.zeros(500, np.int16)
    assert P.measure_tp(x) == (0, 0, 0, 500) and P.measure_tp(x[:0]) == (0, 0, 0, 0)
    x[100:102] = x[300:302] = 1000
    sp, tp, at, n = P.measure_tp(x)
    assert (sp, at, n) == (1000, 100, 500) and tp == (2 * 10269 * 1000 + 8192) >> 14
    x[0] = -32768
    assert P.measure_tp(x) == (32768, 32768, 0, 500)
    f = np.array([np.nan, 0.5, 0.5, np.inf, -np.inf], np.float32)
    assert P.signed(f, 0).tolist() == [0, 16384, 16384, 2 ** 30, -2 ** 30] and P.measure_tp(f)[0] == 2 ** 30


def test_the_finisher_keeps_the_true_peak_under_the_ceiling_only_with_the_flag():
    """Each input at half of full scale, brought to 0 LUFS under -1 dB: the ceiling binds.  With the true peak in the place of the peak
    the finished clip's own true peak is at most C + 1 (int16 rounding); with the sample peak it passes C."""
    C, P_T = LD.ceiling_i16(-1.0), LD.target_ms(0.0)
    for name, x in table().items():
        x = (x * np.float32(0.5 / np.abs(x).max())).astype(np.float32)
        S, n, peak, _ = LD.measure_ref(x)
        true_peak = P.measure_tp(x)[1]
        assert n > 0 and true_peak > peak and LD.clip_gain(S, n, true_peak, P_T, C)[1], (name, "the ceiling does not bind")
        with_flag = P.finish_tp_ref(x, 0, 0, 0, P_T, C)
        without = LD.finish_ld_ref(x, 0, 0, 0, P_T, C)
        assert P.measure_tp(with_flag)[1] <= C + 1 < P.measure_tp(without)[1], (name, P.measure_tp(with_flag), P.measure_tp(without))
        assert np.array_equal(P.finish_tp_ref(x, 12000, 2400, 1200, P_T, C)[12000 + 1200:-2400 - 1200], with_flag[1200:-1200])
        assert np.array_equal(P.finish_tp_ref(x, 5, 7, 3, 0, C), LD.finish_ld_ref(x, 5, 7, 3, 0, C))      # no target: the peak rule, as before
