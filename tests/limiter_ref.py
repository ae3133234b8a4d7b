"""NumPy statement of the look-ahead peak limiter (include/mimi_hip.h, mimi_lim_pool_*): a gain that starts to fall L samples ahead of
a peak, is what the peak requires exactly on it, and recovers at rho per sample.  Every number that decides a sample is an exact integer,
or a spelled-out fp32 operation, so the device is held to this bit for bit.  Sample peaks only.

Per stream, set when the stream is made fresh: C (ceiling, 1 .. 32767), L (look-ahead, 1 .. 480 samples), rho (release step, Q16 per
sample, 8 .. 65536), hr (drive shift, 0 .. 4: the input is multiplied by exactly 2^hr in front of the limiter).  ONE = 65536,
K = ceil(ONE / rho) <= 8192.  A stream is preceded and followed by silence: m[r] = ONE for r < 0 and for r >= the clip's length.

  1. magnitude a[r], an integer.  int16: a = |s << hr|.  fp32: t = fl(|x| * 2^(15 + hr)), an exact scaling; a = 0 for a NaN, a = 2^30 if
     t >= 2^30 (an infinite sample too), else a = int(ceil(t)).
  2. required gain, Q16: m[r] = ONE if a[r] <= C else (C << 16) // a[r].
  3. look-ahead minimum: w[r] = min(m[r .. r + L]), for r >= -L.
  4. release: e[r] = min(w[r], e[r - 1] + rho), e = ONE before r = -L.  Equivalently, and exactly,
     e[r] = min over j in [r - K, r] of (w[j] + (r - j) rho): terms further back cannot win, because w <= ONE.
  5. attack smoothing: g[r] = (e[r - L] + .. + e[r]) // (L + 1).  Every e[r - k] <= w[r - k] <= m[r], so g[r] <= m[r].
  6. output, in the input's format.  int16: y = ((s << hr) g + 2^15) >> 16.  fp32: y = fl(fl(x * 2^hr) * gf), gf = float(g) * 2^-16
     (exact), not fused; then y > Cf -> Cf and y < -Cf -> -Cf with Cf = float(C) * 2^-15.  A NaN stays a NaN.
  7. streaming: sample r comes out once the stream has received r + L + 1 samples, or at ``final``, which leaves the stream fresh with the
     same parameters.  With R received and E emitted a call emits max(0, R - L) - E, or R - E at ``final``.
  8. state row since the stream was fresh: {min g emitted (ONE while none), samples emitted, samples with g < ONE, samples the clamp
     changed}.
``limit_ref`` is the definition, one shot, from the recursion of step 4 in its closed form over the whole clip; ``LimiterRef`` is a
stream that keeps only the last K + 2 L required gains and the held samples, and must give the same."""
import math
from typing import NamedTuple

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

ONE = 65536
A_MAX = 1 << 30
ROW = 4


class Params(NamedTuple):
    C: int = 29203
    L: int = 120
    rho: int = 27
    hr: int = 0

    @property
    def K(self) -> int:
        return -(-ONE // self.rho)


def ceiling_i16(ceiling_db: float) -> int:
    return max(1, min(32767, int(math.floor(32767.0 * 10.0 ** (float(ceiling_db) / 20.0)))))


def params(ceiling_db=-1.0, lookahead=120, release_ms=100.0, drive_shift=0) -> Params:
    """What ``sesameai.limiter.Limit`` turns into: rho = max(8, rint(65536 / (release_ms * 24)))."""
    p = Params(ceiling_i16(ceiling_db), int(lookahead), max(8, int(round(65536.0 / (float(release_ms) * 24.0)))), int(drive_shift))
    check(p)
    return p


def check(p: Params) -> None:
    assert 1 <= p.C <= 32767 and 1 <= p.L <= 480 and 8 <= p.rho <= 65536 and 0 <= p.hr <= 4, p


def magnitude(x: np.ndarray, hr: int) -> np.ndarray:
    """step 1 -> int64"""
    if x.dtype == np.int16:
        return np.abs(x.astype(np.int64) << hr)
    assert x.dtype == np.float32
    with np.errstate(all="ignore"):
        t = (np.abs(x) * np.float32(2.0 ** (15 + hr))).astype(np.float32)
        big = t >= np.float32(A_MAX)
        a = np.ceil(np.where(big | np.isnan(t), np.float32(0), t)).astype(np.int64)
    return np.where(big, A_MAX, a)


def required(x: np.ndarray, p: Params) -> np.ndarray:
    """step 2 -> int64"""
    a = magnitude(x, p.hr)
    return np.where(a <= p.C, ONE, (p.C << 16) // np.maximum(a, 1))


def window_min(m: np.ndarray, L: int) -> np.ndarray:
    """min(m[i .. i + L]) for every i with i + L < len(m)"""
    return sliding_window_view(m, L + 1).min(axis=1) if m.shape[0] > L else np.zeros(0, np.int64)


def release_recursive(w: np.ndarray, rho: int) -> np.ndarray:
    """step 4 as stated: e = ONE before w[0]"""
    e, prev = np.empty_like(w), ONE
    for i in range(w.shape[0]):
        prev = min(int(w[i]), prev + rho)
        e[i] = prev
    return e


def release_windowed(w: np.ndarray, rho: int) -> np.ndarray:
    """step 4 over the last K + 1 values only; w = ONE in front of w[0]"""
    K = -(-ONE // rho)
    ext = np.concatenate([np.full(K, ONE, np.int64), w])
    tilt = (K - np.arange(K + 1, dtype=np.int64)) * rho                      # (r - j) rho for j = r - K .. r
    return (sliding_window_view(ext, K + 1) + tilt).min(axis=1)


def release(w: np.ndarray, rho: int) -> np.ndarray:
    """step 4 in closed form over everything given: i rho + the running minimum of (w[j] - j rho)"""
    tilt = np.arange(w.shape[0], dtype=np.int64) * rho
    return np.minimum.accumulate(w - tilt) + tilt if w.shape[0] else w


def box(e: np.ndarray, L: int) -> np.ndarray:
    """(e[i] + .. + e[i + L]) // (L + 1) for every i with i + L < len(e)"""
    c = np.concatenate([np.zeros(1, np.int64), np.cumsum(e, dtype=np.int64)])
    return (c[L + 1:] - c[:-(L + 1)]) // (L + 1) if e.shape[0] > L else np.zeros(0, np.int64)


def gains(m: np.ndarray, p: Params, how=release) -> np.ndarray:
    """steps 3 to 5 for a whole clip with required gains m -> g, one per sample"""
    m = np.asarray(m, np.int64)
    w = window_min(np.concatenate([np.full(p.L, ONE, np.int64), m, np.full(p.L, ONE, np.int64)]), p.L)      # w[-L .. N)
    return box(how(w, p.rho), p.L)


def apply_gains(x: np.ndarray, g: np.ndarray, p: Params):
    """step 6 -> (y in x's format, samples the clamp changed)"""
    if x.dtype == np.int16:
        return (((x.astype(np.int64) << p.hr) * g + (1 << 15)) >> 16).astype(np.int16), 0
    gf = g.astype(np.float32) * np.float32(2.0 ** -16)
    Cf = np.float32(p.C) * np.float32(2.0 ** -15)
    with np.errstate(all="ignore"):
        y = ((x * np.float32(2.0 ** p.hr)).astype(np.float32) * gf).astype(np.float32)
        hi, lo = y > Cf, y < -Cf
    return np.where(hi, Cf, np.where(lo, -Cf, y)).astype(np.float32), int(np.count_nonzero(hi | lo))


def row_of(g: np.ndarray, clamped: int, before=(ONE, 0, 0, 0)) -> tuple:
    return (min(before[0], int(g.min()) if g.shape[0] else ONE), before[1] + int(g.shape[0]), before[2] + int(np.count_nonzero(g < ONE)),
            before[3] + clamped)


class Limited(NamedTuple):
    y: np.ndarray            # the output, in the input's format
    g: np.ndarray            # the gain of every sample, Q16, int64
    m: np.ndarray            # the required gain of every sample
    row: tuple

    @property
    def limited(self) -> int:
        return self.row[2]


def limit_ref(x, p: Params) -> Limited:
    """One clip, one shot."""
    check(p)
    x = np.asarray(x).reshape(-1)
    m = required(x, p)
    g = gains(m, p)
    y, clamped = apply_gains(x, g, p)
    return Limited(y, g, m, row_of(g, clamped))


class LimiterRef:
    """The rule the way the pool keeps a stream: the required gains of the last K + 2 L positions, the held samples, the row."""

    def __init__(self, p: Params):
        check(p)
        self.p, self.H = p, p.K + 2 * p.L
        self.row = (ONE, 0, 0, 0)
        self._fresh()

    def _fresh(self):
        self.R = self.E = 0
        self.hist = np.full(self.H, ONE, np.int64)
        self.held = None

    def out_count(self, n_in: int, final: bool = False) -> int:
        R = self.R + n_in
        return (R if final else max(0, R - self.p.L)) - self.E

    def feed(self, x, final: bool = False) -> np.ndarray:
        p, x = self.p, np.asarray(x).reshape(-1)
        if self.R == 0:
            self.row = (ONE, 0, 0, 0)
        nh, n_out = self.R - self.E, self.out_count(x.shape[0], final)
        xs = x if self.held is None or not nh else np.concatenate([self.held, x])          # positions -nh ..
        assert xs.dtype == x.dtype, "a stream that holds samples keeps their format"
        m = np.concatenate([self.hist, required(x, p), np.full(p.L if final else 0, ONE, np.int64)])      # positions -H ..
        # output t is position t - nh: its box reads e from L behind, those the scan's K more, and w reaches L ahead
        lo = self.H - nh - p.K - p.L                                                         # >= 0: nh <= L
        g = box(release(window_min(m[lo:lo + n_out + p.K + 2 * p.L], p.L), p.rho)[p.K:], p.L) if n_out else np.zeros(0, np.int64)
        assert g.shape[0] == n_out
        y, clamped = apply_gains(xs[:n_out], g, p)
        self.row = row_of(g, clamped, self.row)
        self.R, self.E = self.R + x.shape[0], self.E + n_out
        self.hist, self.held = m[:self.H + x.shape[0]][-self.H:], xs[n_out:]
        if final:
            self._fresh()
        return y
