"""The voice-activity rule (tests/vad_ref.py) graded on the CPU: the streamed restatement equals the whole-clip rule for every schedule the
GPU tests use, with a carry of at most 879 samples and positions relative to its base; and each part of the rule -- the first-crossing lag,
the block-floating shift, the hysteresis, the voicing test, min_on, hang, the 64-bit bounds -- is shown to decide something on an input
where the rule alone holds.  The figures in the comments are what this file measured; every one of them is asserted."""
import numpy as np
import pytest

import vad_ref as V

LENGTHS = [0, 1, 239, 240, 241, 879, 880, 881, 2400, 24000, 50011]
CHUNKS = [0, 1, 7, 239, 240, 1920, 4000]
QUICK = V.Params(min_on=4, hang=20, hold=10)           # events inside a one-second clip
_cache = {}


def noise(n, seed=0, amp=0.1):
    return (np.random.default_rng(seed).standard_normal(n) * amp).astype(np.float32)


def voice(n, f0=150.0, amp=0.3, seed=0, hiss=0.002):
    """a synthetic voice: 11 harmonics of f0 at 1/h with fixed phases, peak ``amp``, plus white noise at ``hiss``"""
    t = np.arange(n) / 24000.0
    x = sum(np.sin(2 * np.pi * f0 * h * t + h * h) / h for h in range(1, 12))
    x = x / max(np.abs(x).max(), 1e-9) * amp if n else x
    return (x + np.random.default_rng(seed).standard_normal(n) * hiss).astype(np.float32)


def talk(N, seed=0, f0=150.0, amp=0.3, spans=((0.15, 0.55),), hiss=0.002):
    """hiss all along, the voice inside ``spans`` (fractions of the clip)"""
    x = noise(N, seed, hiss)
    for a, b in spans:
        lo, hi = int(a * N), int(b * N)
        x[lo:hi] += voice(hi - lo, f0, amp, seed + 1, 0.0)
    return x


def clip(N):
    if N not in _cache:
        _cache[N] = talk(N, N, (110.0, 150.0, 220.0)[N % 3])
    return _cache[N]


def ref(N, prm=QUICK):
    if ("ref", N, prm) not in _cache:
        _cache[("ref", N, prm)] = V.vad_ref(clip(N), prm)
    return _cache[("ref", N, prm)]


def schedules(N, seed):
    """three chunk schedules of a clip of N samples: random draws from CHUNKS, all at once with final alone after everything, and single
    samples around a frame edge"""
    rng = np.random.default_rng(seed)
    rand = [int(rng.choice(CHUNKS)) for _ in range(64)]
    return {"random": rand, "whole_then_final_alone": [N], "around_a_frame_edge": [238, 1, 1, 1, 0, 1, 477, 1, 1, 1, 1, 640, 239, 1, 1]}


def same(got, want, what):
    for f in ("flags", "lag", "power", "floor", "summary"):
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == b.dtype and np.array_equal(a, b), (what, f)
    assert got.events == want.events, (what, "events")


@pytest.mark.parametrize("N", LENGTHS)
def test_streamed_equals_whole_clip(N):
    want = ref(N)
    assert want.flags.shape[0] == N // V.F
    assert V.events(want.flags, QUICK) == want.events
    for name, sch in schedules(N, N + 1).items():
        same(V.vad_streamed(clip(N), QUICK, sch), want, (N, name))
    if N >= 24000:
        assert [e[0] for e in want.events] == ["start", "end"], "the clips hold a whole turn"
        a, b = want.events[0][1] * V.F, want.events[1][1] * V.F
        assert abs(a - int(0.15 * N)) <= 3 * V.F and abs(b - int(0.55 * N)) <= 3 * V.F, "stamped where the voice starts and stops"


def test_the_stream_keeps_at_most_879_samples_and_the_five_state_words():
    s = V.StreamRef(QUICK)
    rng = np.random.default_rng(3)
    x = clip(50011)
    at, worst = 0, 0
    while at < x.shape[0]:
        n = int(rng.choice(CHUNKS))
        s.feed(x[at:at + n])
        at += n
        worst = max(worst, s.carry.shape[0])
        assert s.carry.shape[0] == min(s.R, V.HIST + s.R % V.F)
    assert 640 < worst <= V.CARRY - 1 == 879
    s.feed(x[:V.F - 1 - s.R % V.F])                             # one sample short of a frame: the most a stream ever keeps
    assert s.carry.shape[0] == 879
    assert set(vars(s.scan)) == {"prm", "N", "speech", "run", "quiet", "since", "k", "last_start", "last_end", "n_start", "n_end"}
    # final discards the partial frame and leaves the stream fresh with the same parameters
    s.feed(x[:100], final=True)
    assert (s.R, s.scan.k, s.carry.shape[0], s.scan.prm) == (0, 0, 0, QUICK)
    same(V.vad_streamed(x[:5000], QUICK, [1920, 1920]), V.vad_ref(x[:5000], QUICK), "after final")


def test_int16_and_fp32_of_the_same_clip_agree():
    x = clip(24000)
    i16 = V.to_s(x).astype(np.int16)
    same(V.vad_ref(i16, QUICK), ref(24000), "int16")
    assert V.to_s(np.array([1.0, -1.0, 0.99999, np.inf, -np.inf, np.nan, 1.5 / 32768, 2.5 / 32768, -4.0], dtype=np.float32)).tolist() == \
        [32767, -32768, 32767, 0, 0, 0, 2, 2, -32768]          # clamp; non-finite -> 0; halves round to even


def test_the_first_crossing_lag_is_not_the_best_lag():
    x = voice(12000, 220.0, 0.3, seed=1, hiss=0.002)
    first = V.vad_ref(x).lag[10:]
    best = V.vad_ref(x, pick="argmax").lag[10:]
    differ = int(np.count_nonzero(first != best))
    print(f"220 Hz: first-crossing lags {sorted(set(first.tolist()))}, arg-max lags {sorted(set(best.tolist()))}, {differ} of {first.shape[0]} frames differ")
    assert differ == first.shape[0] == 40                       # every frame
    assert set(best.tolist()) == {109} and 100 <= first.min() and first.max() <= 108 and (first < best).all()


def pulses(n, f0=150.0, amp=0.003, seed=2, hiss=0.0003):
    """a voice as a pulse train: 11 harmonics of equal weight and zero phase, peak ``amp``, plus white noise at ``hiss``"""
    t = np.arange(n) / 24000.0
    x = sum(np.cos(2 * np.pi * f0 * h * t) for h in range(1, 12))
    return (x / np.abs(x).max() * amp + np.random.default_rng(seed).standard_normal(n) * hiss).astype(np.float32)


def test_the_block_floating_shift_keeps_a_quiet_voice_voiced():
    """A 150 Hz pulse train whose peak is 0.003 (98 of 32,768) over hiss a tenth of that: with the block-floating shift (0 here) every frame
    is voiced; a fixed shift of 6 leaves two bits of the pulses and none of what lies between them, and loses frames (93 of 98 stay).
    Measured beside it and NOT asserted: without any noise a periodic signal stays periodic under any shift, so both give 98 of 98; and for
    the 1/h voice of ``voice`` with hiss at 0.001 the fixed shift calls MORE frames voiced than the rule (26 against 6 of 48), because the arithmetic
    shift's bias of -1/2 adds the same constant to R and E and so inflates the normalised correlation."""
    x = pulses(24000)
    block = V.vad_ref(x).flags[2:]
    fixed = V.vad_ref(x, shift=6).flags[2:]
    nb, nf = int(np.count_nonzero(block & 2)), int(np.count_nonzero(fixed & 2))
    print(f"150 Hz at 0.003: {nb} of {block.shape[0]} frames voiced with the block-floating shift, {nf} with a fixed shift of 6")
    assert nb == block.shape[0] == 98 and nf < nb


def _level(n, amp, seed):
    return voice(n, 150.0, amp, seed, hiss=0.0)


def test_between_3x_and_8x_of_the_floor_a_turn_goes_on_but_none_starts():
    # the floor rests at n_min = (240 * 8)^2: a voice whose power is 5 x that
    def p_of(amp):
        return V.power(V.to_s(_level(2400, amp, 0))[1200:1440])
    amp = 0.3
    while p_of(amp) > 5 * V.Params().n_min:
        amp *= 0.98
    ratio = p_of(amp) / V.Params().n_min
    assert 3.5 < ratio < 7.5, ratio
    quiet, mid, loud = np.zeros(4800, dtype=np.float32), _level(48000, amp, 1), _level(4800, 0.3, 2)
    alone = V.vad_ref(np.concatenate([quiet, mid]))
    after = V.vad_ref(np.concatenate([quiet, loud, mid]))
    print(f"level {amp:.5f}: power / floor {ratio:.2f}; alone {alone.events}, after a loud start {after.events}")
    assert alone.events == [] and int(np.count_nonzero(alone.flags & 2)) > 190      # voiced all along, never loud enough to start
    # ... but loud enough to keep a running turn alive (frame 20 is the first loud one; its window is half silence and not yet voiced)
    assert after.events == [("start", 21)] and after.summary[0] == 1
    assert (after.flags[60:] & 8).all()


def test_white_noise_is_never_voiced():
    r = V.vad_ref(noise(480000, 7, 0.1))
    n = int(np.count_nonzero(r.flags & 2))
    print(f"20 s of white noise at 0.1: {n} of {r.flags.shape[0]} frames voiced")
    assert r.flags.shape[0] == 2000 and n == 0 and r.events == [] and (r.lag == 0).all()


def test_a_noise_burst_and_clicks_start_no_turn():
    x = noise(72000, 8, 0.001)
    x[12000:19200] += noise(7200, 9, 0.3)                       # 0.3 s of loud noise
    for at in (30000, 36000, 36500, 50000):
        x[at:at + 20] += 0.5                                    # 20-sample clicks
    r = V.vad_ref(x)
    loud = int(np.count_nonzero(r.flags & 1))
    print(f"burst and clicks: {loud} loud frames, {int(np.count_nonzero(r.flags & 4))} active, events {r.events}")
    assert loud >= 30 and r.events == [] and r.summary[5] == 0


def test_two_bursts_300_ms_apart_are_one_turn_at_hang_70_and_two_at_hang_20():
    x = talk(72000, 10, 150.0, 0.3, spans=((0.1, 0.3), (0.4, 0.6)))      # voiced 0.3 .. 0.9 s and 1.2 .. 1.8 s of 3 s
    one = V.vad_ref(x, V.Params(hang=70))
    two = V.vad_ref(x, V.Params(hang=20))
    print(f"hang 70: {one.events}; hang 20: {two.events}")
    assert [e[0] for e in one.events] == ["start", "end"] and one.summary[5:7].tolist() == [1, 1]
    assert [e[0] for e in two.events] == ["start", "end", "start", "end"] and two.summary[5:7].tolist() == [2, 2]
    assert abs(one.events[0][1] - 30) <= 2 and abs(one.events[1][1] - 180) <= 3
    assert abs(two.events[1][1] - 90) <= 3 and abs(two.events[2][1] - 120) <= 2


def full_scale_square(N=4800):
    return np.where((np.arange(N) // 60) % 2 == 0, 1.0, -1.0).astype(np.float32)


def test_a_full_scale_square_reaches_the_bounds_inside_64_bits():
    x = full_scale_square()
    s = V.to_s(x)
    assert set(s.tolist()) == {32767, -32768}
    i16 = np.where((np.arange(4800) // 60) % 2 == 0, -32768, -32768).astype(np.int16)      # all -32768: the largest |s| there is
    P = V.power(V.to_s(i16)[:240])
    assert P == 0                                               # DC-free
    P = V.power(s[240:480])
    assert P == 240 * (120 * 32767 ** 2 + 120 * 32768 ** 2) - (120 * 32767 - 120 * 32768) ** 2 and P < 2 ** 46
    buf = V._ext(s, 4 * V.F - V.W - V.TMAX, V.W + V.TMAX)
    R, E, E0 = V.correlations(buf)
    assert np.abs(buf >> 6).max() == 512 and E0 == 480 * 511 * 511 + 240 * (512 * 512 - 511 * 511) and int(np.abs(R).max()) < 2 ** 29
    lag, top = V.lag_of(buf, want_bounds=True)
    # a square's autocorrelation falls off as 1 - 4 d / 120 around its period: the first lag above 0.707 is 120 - 8
    assert top < 2 ** 59 and lag == 112
    r = V.vad_ref(x)
    assert (r.lag[4:] == 112).all() and r.floor.max() < 2 ** 47
    assert np.abs(V.to_s(i16) >> 6).max() == 512 and int(V.correlations(V.to_s(i16)[:880])[0].max()) == 480 * 512 * 512 < 2 ** 29


def test_silence_has_no_lag():
    r = V.vad_ref(np.zeros(4800, dtype=np.float32))
    assert (r.lag == 0).all() and not r.flags.any() and (r.power == 0).all() and (r.floor == V.Params().n_min).all()
    assert r.summary.tolist() == [0, 20, -1, -1, 0, 0, 0, 0]


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_sample_is_a_zero_sample(bad):
    x = clip(24000)[:12000].copy()
    xb = x.copy(); xb[5000] = bad
    xz = x.copy(); xz[5000] = 0.0
    same(V.vad_ref(xb, QUICK), V.vad_ref(xz, QUICK), bad)


def test_parameters_outside_their_ranges_are_refused():
    for p in (V.Params(on_q4=4096), V.Params(off_q4=15), V.Params(on_q4=40, off_q4=48), V.Params(min_on=0), V.Params(min_on=1001),
              V.Params(hang=0), V.Params(hang=10001), V.Params(hold=-1), V.Params(hold=10001), V.Params(n_min=0), V.Params(n_min=2 ** 40 + 1)):
        with pytest.raises(ValueError):
            V.check(p)
    V.check(V.Params(4095, 16, 1000, 10000, 10000, 2 ** 40)); V.check(V.Params(16, 16, 1, 1, 0, 1))
