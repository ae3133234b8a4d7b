"""NumPy statement of the live leveler (include/mimi_hip.h, mimi_ld_pool_level_*), built on the meter's rule (tests/loudness_ref.py): a
causal gain that follows the gated loudness measured so far, hop by hop, with nothing held back -- n_out == n_in on every call.  Every
number that decides a sample is an exact integer, or a spelled-out float64 / fp32 operation on integers, so the device is held to this bit
for bit.  Samples s, hop energies e[h] (H = 2400) and gate() are the meter's.

Per stream, set when the stream is made fresh: P_T (target mean square, 1 .. 2^31), C (ceiling, 1 .. 32767), g0 (start gain, Q16,
1 .. gmax), gmax (largest gain, Q16, 1 .. 2^22), sh (slew shift, 1 .. 16).

  1. pk[h] = max |s| over hop h; P[h] = max(pk[0 .. h]) since the stream was fresh (the ring does not limit it; a partial hop has none).
  2. boundary gains, Q16: A[0] = A[1] = g0; for j >= 1, from hops <= j - 1 only:
         (S, n) = gate(e[max(0, j - ring) .. j - 1])
         T = A[j] if n == 0 else int(min(f64(gmax), trunc(sqrt((f64(P_T * 4H) * f64(n)) / f64(S)) * 65536.0)))      (float64, as clip_gain)
         d = max(1, A[j] >> sh);  B = min(max(T, A[j] - d), A[j] + d);  cap = (C << 16) // max(P[j - 1], 1)
         A[j + 1] = max(1, min(B, cap, gmax))
  3. the sample at stream position r, j = r // H, i = r % H:  gi = (A[j] (H - i) + A[j + 1] i) // H  (64-bit).
  4. int16: v = (s gi + 2^15) >> 16, y = clamp(v, -C, C).  fp32: y = fl(x * gf), gf = float(gi) * 2^-16 (exact), then y > Cf -> Cf and
     y < -Cf -> -Cf with Cf = float(C) * 2^-15: a NaN stays a NaN, an infinite sample becomes +-Cf.  clipped counts the samples the
     clamp changed.
  5. final ends the clip: a trailing partial hop is levelled like any other sample (its gains were known), then the stream is fresh
     with the same parameters.
The state row is {A[k + 1], k, clipped, P[k - 1]} for k complete hops: the gain the open hop ends on, the hops, the samples clamped and
the running peak of the complete hops (0 while there is none)."""
from typing import NamedTuple

import numpy as np

import loudness_ref as L
from vad_ref import to_s

H = L.H
GMAX_LIMIT = 1 << 22
ROW = 4


class Params(NamedTuple):
    P_T: int
    C: int
    g0: int = 65536
    gmax: int = 16 * 65536
    sh: int = 4


def params(loudness, ceiling_db=-1.0, start_gain=1.0, max_gain_db=24.0, slew_shift=4) -> Params:
    """What ``sesameai.loudness.Level`` turns into: the gains in Q16, 6 dB a doubling (24 dB is 16 x 65536)."""
    gmax = int(round(65536.0 * 2.0 ** (float(max_gain_db) / 6.0)))
    p = Params(L.target_ms(loudness), L.ceiling_i16(ceiling_db), int(round(float(start_gain) * 65536.0)), gmax, int(slew_shift))
    check(p)
    return p


def check(p: Params) -> None:
    assert 1 <= p.P_T <= 2 ** 31 and 1 <= p.C <= 32767 and 1 <= p.gmax <= GMAX_LIMIT and 1 <= p.g0 <= p.gmax and 1 <= p.sh <= 16, p


def target_gain(S: int, n: int, p: Params) -> int:
    """T of step 2 for n > 0"""
    g = np.sqrt((np.float64(p.P_T * 4 * H) * np.float64(n)) / np.float64(S))
    return int(min(np.float64(p.gmax), np.trunc(g * np.float64(65536.0))))


def next_gain(A: int, S: int, n: int, P: int, p: Params):
    """(A[j + 1], T, d, cap) from A[j], the gated hops <= j - 1 and P[j - 1]; T is None while nothing has passed the gates"""
    T = A if n == 0 else target_gain(S, n, p)
    d = max(1, A >> p.sh)
    B = min(max(T, A - d), A + d)
    cap = (p.C << 16) // max(P, 1)
    return max(1, min(B, cap, p.gmax)), (None if n == 0 else T), d, cap


def boundary_gains(e, pk, p: Params, ring: int = L.RING):
    """A[0 .. K + 1] for K complete hops with energies e and peaks pk; also the trace [(j, T, d, cap)] of step 2"""
    K = len(e)
    A, trace, P = [p.g0, p.g0], [], 0
    for j in range(1, K + 1):
        P = max(P, int(pk[j - 1]))
        S, n = L.gate(e[max(0, j - ring):j], ring)
        a, T, d, cap = next_gain(A[j], S, n, P, p)
        A.append(a)
        trace.append((j, T, d, cap))
    return A, trace


def sample_gains(A, r0: int, n: int, k0: int = 0) -> np.ndarray:
    """gi for stream positions r0 .. r0 + n, A[0] being the boundary of hop k0"""
    A = np.asarray(A, np.int64)
    r = r0 + np.arange(n, dtype=np.int64)
    j, i = r // H - k0, r % H
    return (A[j] * (H - i) + A[j + 1] * i) // H if n else np.zeros(0, np.int64)


def apply_gains(x: np.ndarray, gi: np.ndarray, C: int):
    """step 4 -> (y in x's format, samples the clamp changed)"""
    x = np.asarray(x).reshape(-1)
    if x.dtype == np.int16:
        v = (x.astype(np.int64) * gi + (1 << 15)) >> 16
        y = np.clip(v, -C, C)
        return y.astype(np.int16), int(np.count_nonzero(y != v))
    assert x.dtype == np.float32
    gf = gi.astype(np.float32) * np.float32(2.0 ** -16)          # gi < 2^24: exact
    Cf = np.float32(C) * np.float32(2.0 ** -15)
    with np.errstate(all="ignore"):
        y = (x * gf).astype(np.float32)
        hi, lo = y > Cf, y < -Cf
    y = np.where(hi, Cf, np.where(lo, -Cf, y)).astype(np.float32)
    return y, int(np.count_nonzero(hi | lo))


def hop_peaks(s: np.ndarray) -> np.ndarray:
    k = s.shape[0] // H
    return np.abs(s[:k * H]).reshape(k, H).max(axis=1) if k else np.zeros(0, np.int64)


class Levelled(NamedTuple):
    y: np.ndarray            # the output, in the input's format
    gains: np.ndarray        # A[0 .. K + 1], int64
    energies: np.ndarray     # e[0 .. K), int64
    row: tuple               # {A[K + 1], K, clipped, P[K - 1]}
    trace: list


def level_ref(x, p: Params, ring: int = L.RING) -> Levelled:
    """One clip, one shot."""
    check(p)
    x = np.asarray(x).reshape(-1)
    s = to_s(x)
    e = L.hop_energies(s)
    pk = hop_peaks(s)
    A, trace = boundary_gains([int(v) for v in e], pk, p, ring)
    y, clipped = apply_gains(x, sample_gains(A, 0, x.shape[0]), p.C)
    return Levelled(y, np.asarray(A, np.int64), e, (A[-1], len(e), clipped, int(pk.max()) if len(pk) else 0), trace)


class LevelerRef:
    """The rule the way the pool keeps a stream: the meter's StreamRef beside {A[k], A[k + 1], P, clipped} and the open hop's peak."""

    def __init__(self, p: Params, ring: int = L.RING):
        check(p)
        self.p, self.ring_size = p, ring
        self.meter = L.StreamRef(ring)
        self.row = (p.g0, 0, 0, 0)
        self._fresh()

    def _fresh(self):
        self.R, self.k, self.a_cur, self.a_next, self.P, self.clipped, self.open_pk = 0, 0, self.p.g0, self.p.g0, 0, 0, 0
        self.e = []

    def feed(self, x, final: bool = False):
        """-> (y, the hop energies this chunk completes, A[k0 .. k0 + nf + 1])"""
        x = np.asarray(x).reshape(-1)
        s = to_s(x)
        e_new = self.meter.feed(x, final)
        k0, r0 = self.k, self.R
        A = [self.a_cur, self.a_next]
        at = 0                                                  # samples of the chunk behind the hops walked so far
        for m in range(len(e_new)):
            end = (k0 + m + 1) * H - r0                         # the chunk's sample behind hop k0 + m
            pk = max(self.open_pk, int(np.abs(s[at:end]).max()) if end > at else 0)
            at, self.open_pk = end, 0
            self.e = (self.e + [int(e_new[m])])[-self.ring_size:]
            self.P = max(self.P, pk)
            S, n = L.gate(self.e, self.ring_size)
            A.append(next_gain(A[-1], S, n, self.P, self.p)[0])
        if s.shape[0] > at:
            self.open_pk = max(self.open_pk, int(np.abs(s[at:]).max()))
        y, c = apply_gains(x, sample_gains(A, r0, x.shape[0], k0), self.p.C)
        self.R, self.k, self.a_cur, self.a_next, self.clipped = r0 + x.shape[0], k0 + len(e_new), A[-2], A[-1], self.clipped + c
        self.row = (self.a_next, self.k, self.clipped, self.P)
        if final:
            self._fresh()
        return y, e_new, np.asarray(A, np.int64)


def reach(A, trace, p: Params):
    """the first hop that STARTS on its target, or None: j + 1 for the first j with a target T and |T - A[j]| <= d, where the slew no
    longer binds and A[j + 1] = min(T, cap, gmax)"""
    for j, T, d, cap in trace:
        if T is not None and abs(T - A[j]) <= d:
            return j + 1
    return None


def lufs_after(y, from_hop: int) -> float:
    S, n, _, _ = L.measure_ref(np.asarray(y).reshape(-1)[from_hop * H:])
    return L.lufs(S, n)

