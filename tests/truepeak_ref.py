"""NumPy statement of true-peak detection (include/mimi_hip.h, mimi_lim_pool_reset_tp and mimi_tp_measure): the limiter of
tests/limiter_ref.py with the magnitude of a sample replaced by the largest magnitude the 4x oversampled signal reaches on the sample and
in the two intervals beside it.  Exact integers throughout, so the device is held to this bit for bit.

Taps.  T = 8; three fractional phases p = 1, 2, 3 of 2 T = 16 taps in Q14, H[p][k + 7] for k = -7 .. 8 (tools/truepeak_taps.py makes
them: a 63-tap Kaiser windowed sinc); phase 0 is the sample itself.

  a. signed sample v[r], an integer.  int16: v = s << hr.  fp32: v = sign(x) a[r] with a of step 1 of the limiter's rule: a NaN gives 0,
     |v| <= 2^30.  v = 0 outside the clip.
  b. inter-sample magnitude.  Interval i lies between samples i - 1 and i (i = 0 .. N for a clip of N samples).
     acc = sum_{k = -7 .. 8} H[p][k + 7] v[i - 1 + k];  U[i][p] = (|acc| + 2^13) >> 14.  |acc| <= 31572 * 2^30 < 2^45: int64.
  c. true-peak magnitude of sample r of the clip: a_tp[r] = max(a[r], U[r][1 .. 3], U[r + 1][1 .. 3]) < 2^31.
  d. step 2 of the limiter reads a_tp in the place of a: m[r] = ONE if a_tp[r] <= C else (C << 16) // a_tp[r]; m = ONE outside the clip
     as before.  Steps 3 to 6 and the state row are the limiter's.
  e. streaming: m[r] needs v up to r + T, so the latency is L + T: with R received and E emitted a call emits max(0, R - L - T) - E, or
     R - E at ``final``.
``limit_tp_ref`` is the definition, one shot; ``TruePeakLimiterRef`` is a stream that keeps, beside the required gains of the K + 2 L
positions in front of the last T, the last 2 T signed samples and up to L + T held samples, and must give the same.
``measure_tp`` is the stateless meter: (sample peak, true peak, first r with a_tp[r] == true peak, n), hr = 0."""
import importlib.util
import os

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

import limiter_ref as R
from limiter_ref import ONE, Limited, Params

_spec = importlib.util.spec_from_file_location(
    "truepeak_taps", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "truepeak_taps.py"))
truepeak_taps = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(truepeak_taps)

T = truepeak_taps.T
Q = truepeak_taps.Q
H = np.array(truepeak_taps.taps(), dtype=np.int64)               # (3, 16)
ROW = 4


def signed(x: np.ndarray, hr: int) -> np.ndarray:
    """step a -> int64"""
    x = np.asarray(x).reshape(-1)
    if x.dtype == np.int16:
        return x.astype(np.int64) << hr
    a = R.magnitude(x, hr)                                       # (0 for a NaN)
    return np.where(np.signbit(x), -a, a)


def intersample(v: np.ndarray) -> np.ndarray:
    """step b for v[0 .. n) with T zeros-or-neighbours already in place on either side: window w reads v[w .. w + 2 T), which is interval
    i = w + T of v's own indices -> the largest of the three phases, one value per window (len(v) - 2 T + 1 of them)"""
    if v.shape[0] < 2 * T:
        return np.zeros(0, np.int64)
    acc = sliding_window_view(v.astype(np.int64), 2 * T) @ H.T
    return ((np.abs(acc) + (1 << (Q - 1))) >> Q).max(axis=1)


def magnitude_tp(x: np.ndarray, hr: int) -> np.ndarray:
    """step c for a whole clip -> int64, one per sample"""
    v = signed(x, hr)
    if v.shape[0] == 0:
        return v
    U = intersample(np.concatenate([np.zeros(T, np.int64), v, np.zeros(T, np.int64)]))          # intervals 0 .. N
    return np.maximum(np.abs(v), np.maximum(U[:-1], U[1:]))


def need(a: np.ndarray, C: int) -> np.ndarray:
    return np.where(a <= C, ONE, (C << 16) // np.maximum(a, 1))


def required_tp(x: np.ndarray, p: Params) -> np.ndarray:
    return need(magnitude_tp(x, p.hr), p.C)


def limit_tp_ref(x, p: Params) -> Limited:
    """One clip, one shot."""
    R.check(p)
    x = np.asarray(x).reshape(-1)
    m = required_tp(x, p)
    g = R.gains(m, p)
    y, clamped = R.apply_gains(x, g, p)
    return Limited(y, g, m, R.row_of(g, clamped))


def measure_tp(x) -> tuple:
    """(sample peak, true peak, first position r with a_tp[r] == true peak, n); an empty clip: four zeros"""
    x = np.asarray(x).reshape(-1)
    if x.shape[0] == 0:
        return (0, 0, 0, 0)
    a_tp = magnitude_tp(x, 0)
    return (int(np.abs(signed(x, 0)).max()), int(a_tp.max()), int(np.argmax(a_tp)), int(x.shape[0]))


def true_peak_db(tp: int) -> float:
    """a true peak in dB relative to full scale (2^15)"""
    return 20.0 * np.log10(max(int(tp), 1) / 32768.0)


class TruePeakLimiterRef:
    """The rule the way the pool keeps a true-peak stream."""

    def __init__(self, p: Params):
        R.check(p)
        self.p, self.H = p, p.K + 2 * p.L
        self.row = (ONE, 0, 0, 0)
        self._fresh()

    def _fresh(self):
        self.R = self.E = 0
        self.hist = np.full(self.H, ONE, np.int64)               # m of the positions R - T - H .. R - T
        self.pend = np.zeros(2 * T, np.int64)                    # v of the positions R - 2 T .. R
        self.held = None

    def out_count(self, n_in: int, final: bool = False) -> int:
        Rn = self.R + n_in
        return (Rn if final else max(0, Rn - self.p.L - T)) - self.E

    def feed(self, x, final: bool = False) -> np.ndarray:
        p, x = self.p, np.asarray(x).reshape(-1)
        n = x.shape[0]
        if self.R == 0:
            self.row = (ONE, 0, 0, 0)
        nh, n_out = self.R - self.E, self.out_count(n, final)
        xs = x if self.held is None or not nh else np.concatenate([self.held, x])          # positions -nh ..
        assert xs.dtype == x.dtype, "a stream that holds samples keeps their format"
        vs = np.concatenate([self.pend, signed(x, p.hr), np.zeros(T if final else 0, np.int64)])           # positions -2 T ..
        U = intersample(vs)                                                                # intervals -T .. n - T (.. n at final)
        a_tp = np.maximum(np.abs(vs[T:T + U.shape[0] - 1]), np.maximum(U[:-1], U[1:]))     # positions -T .. n - T (.. n at final)
        q = np.arange(-T, -T + a_tp.shape[0])
        m_new = np.where(q < -self.R, ONE, need(a_tp, p.C))                                # in front of the clip: silence
        m = np.concatenate([self.hist, m_new, np.full(p.L if final else 0, ONE, np.int64)])          # positions -T - H ..
        lo = self.H + T - nh - p.K - p.L                                                   # >= 0: nh <= L + T
        g = box_g(m[lo:lo + n_out + p.K + 2 * p.L], p) if n_out else np.zeros(0, np.int64)
        assert g.shape[0] == n_out
        y, clamped = R.apply_gains(xs[:n_out], g, p)
        self.row = R.row_of(g, clamped, self.row)
        self.R, self.E = self.R + n, self.E + n_out
        self.hist, self.pend, self.held = m[n:n + self.H], vs[n:n + 2 * T], xs[n_out:]
        if final:
            self._fresh()
        return y


def box_g(m: np.ndarray, p: Params) -> np.ndarray:
    """steps 3 to 5 over required gains that start K + L in front of the first output and end L behind the last"""
    return R.box(R.release(R.window_min(m, p.L), p.rho)[p.K:], p.L)


def finish_tp_ref(x: np.ndarray, lead: int, tail: int, fade: int, P_T: int, C: int) -> np.ndarray:
    """tests/loudness_ref.py ``finish_ld_ref`` with the clip's true peak in the place of its sample peak: ``SegmentFinish(loudness=,
    true_peak=True)``.  One gain per clip is linear, so the finished clip's true peak is the input's times the gain."""
    import finish_ref
    import loudness_ref as LD
    x = np.asarray(x, np.float32).reshape(-1)
    S, n, _, _ = LD.measure_ref(x)
    if P_T <= 0 or n == 0:
        return finish_ref.finish_ref(x, lead, tail, fade)
    g, _ = LD.clip_gain(S, n, measure_tp(x)[1], P_T, C)
    q = LD.quantise_ld(x, g)
    y = np.concatenate([np.zeros(int(lead), np.int16), q, np.zeros(int(tail), np.int16)])
    m = min(int(fade), len(y) // 2)
    if m > 0:
        r = finish_ref.ramp(m)
        y[:m] = np.trunc(y[:m].astype(np.float32) * r).astype(np.int16)
        y[len(y) - m:] = np.trunc(y[len(y) - m:].astype(np.float32) * r[::-1]).astype(np.int16)
    return y
