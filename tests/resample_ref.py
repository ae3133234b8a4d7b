"""float64 numpy statement of the resampler's definition (include/mimi_hip.h, mimi_rs_pool_*): scipy.signal.resample_poly's default filter
written out, the whole-clip sum, the streaming count, and a streamed restatement that works the way the device pool does -- a history of
2 * half / up + 1 samples, two running totals reduced by whole periods, zero in front of the clip by INDEX -- with switches that break it in
the ways a kernel could be broken (tests/test_resample_oracle.py shows each of them far above the GPU tests' bound).  No scipy in here."""
from math import gcd

import numpy as np

PAIRS = [(48000, 24000), (44100, 24000), (32000, 24000), (22050, 24000), (16000, 24000), (8000, 24000),
         (24000, 48000), (24000, 44100), (24000, 16000), (24000, 8000)]
U = 2.0 ** -24              # fp32 unit round-off


def rates(src, dst):
    """(up, down, half)"""
    g = gcd(src, dst)
    up, down = dst // g, src // g
    return up, down, 10 * max(up, down)


def taps(up, down):
    """firwin(2 * half + 1, 1 / max(up, down), window=('kaiser', 5.0)) * up, float64, h[0 .. 2 * half]"""
    mx = max(up, down)
    half = 10 * mx
    m = np.arange(-half, half + 1, dtype=np.float64)
    h = np.sinc(m / mx) / mx
    h *= np.i0(5.0 * np.sqrt(np.clip(1.0 - (m / half) ** 2, 0.0, None))) / np.i0(5.0)
    return h / h.sum() * up


def emitted(N, up, down, half, final):
    """Outputs a stream has emitted after N samples in all."""
    if final:
        return -(-N * up // down)
    a = N * up - 1 - half
    return 0 if a < 0 else a // down + 1


def _sum(x, h, up, down, half, n, k_first=0):
    """y[n] for the output indices ``n`` (an int64 array) of the clip x[0 .. N) whose first sample has index ``k_first`` <= 0 ... that is,
    x[j] is sample k_first + j; also the number of taps of each output's phase and the sum of their magnitudes (for the fp32 bound)."""
    N = x.shape[0]
    c = n * down + half
    klo = -((-(c - 2 * half)) // up)
    y = np.zeros(n.shape[0])
    cnt = np.zeros(n.shape[0], dtype=np.int64)
    mag = np.zeros(n.shape[0])
    for j in range(2 * half // up + 1):
        k = klo + j
        t = c - k * up
        ok = t >= 0
        hv = np.where(ok, h[np.clip(t, 0, 2 * half)], 0.0)
        cnt += ok
        mag += np.abs(hv)
        inside = ok & (k - k_first >= 0) & (k - k_first < N)
        y += np.where(inside, hv * x[np.clip(k - k_first, 0, max(N - 1, 0))] if N else 0.0, 0.0)
    return y, cnt, mag


def resample_ref(x, src, dst, with_bound=False):
    """The definition: x (N,) -> y (ceil(N up / down),) float64.  with_bound: also the GPU tests' per-output bound
    (taps + 3) * 2^-24 * sum|h_phase| * max|x| (the fp32 fmaf chain's first-order error plus one rounding of each tap)."""
    x = np.asarray(x, dtype=np.float64)
    up, down, half = rates(src, dst)
    n = np.arange(emitted(x.shape[0], up, down, half, True), dtype=np.int64)
    y, cnt, mag = _sum(x, taps(up, down), up, down, half, n)
    if not with_bound:
        return y
    finite = x[np.isfinite(x)]
    return y, (cnt + 3) * U * mag * (np.abs(finite).max() if finite.size else 0.0)


def contaminated(N, src, dst, k_bad):
    """The outputs [lo, hi) of a clip of N samples whose tap range covers sample k_bad."""
    up, down, half = rates(src, dst)
    M = emitted(N, up, down, half, True)
    lo = max(0, -((-(k_bad * up - half)) // down))          # n * down + half - k * up >= 0
    hi = min(M, (k_bad * up + half) // down + 1)            # n * down + half - k * up <= 2 * half
    return lo, max(hi, lo)


class StreamRef:
    """One stream the way the pool keeps it.  ``fault`` names one way of getting it wrong:
    'shift' (the chunk is read one sample late), 'phase' (tap index + 1), 'half' (tap index - 1: half off by one), 'drop_history' (history
    not carried over a cut), 'stale_history' (no index rule: a reset stream reads what the last clip left), 'no_tail' (final emits as an
    open clip does)."""

    def __init__(self, src, dst, fault=None):
        self.up, self.down, self.half = rates(src, dst)
        self.h = taps(self.up, self.down)
        self.H = 2 * self.half // self.up + 1
        self.hist = np.zeros(self.H)
        self.fault = fault
        self.reset()

    def reset(self):
        self.n_in = self.n_out = self.k0 = 0

    def feed(self, chunk, final=False):
        up, down, half, H = self.up, self.down, self.half, self.H
        chunk = np.asarray(chunk, dtype=np.float64)
        if self.fault == "shift" and chunk.shape[0]:
            chunk = np.concatenate([chunk[1:], [0.0]])
        m = chunk.shape[0]
        e = max(emitted(self.n_in + m, up, down, half, final and self.fault != "no_tail"), self.n_out)
        hist = np.zeros(H) if self.fault == "drop_history" else self.hist
        buf = np.concatenate([hist, chunk])                  # buf[H + d] = sample k_base + d
        n = np.arange(self.n_out, e, dtype=np.int64)
        c = n * down + half + {"phase": 1, "half": -1}.get(self.fault, 0)
        klo = -((-(c - 2 * half)) // up)
        y = np.zeros(n.shape[0])
        k_first = self.n_in - H if self.fault == "stale_history" else max(self.k0, self.n_in - H)
        for j in range(H + 1):
            k = klo + j
            t = c - k * up
            ok = (t >= 0) & (t <= 2 * half) & (k >= k_first) & (k < self.n_in + m)
            idx = np.clip(H + k - self.n_in, 0, H + m - 1)
            y += np.where(ok, self.h[np.clip(t, 0, 2 * half)] * buf[idx], 0.0)
        self.hist = buf[m:]                                  # the last H samples
        if final:
            self.reset()
        else:
            self.n_in += m
            self.n_out = e
            q = min(self.n_in // down, self.n_out // up)     # whole periods: every difference n * down - k * up stays
            self.n_in -= q * down
            self.n_out -= q * up
            self.k0 -= q * down
        return y


def resample_streamed(x, src, dst, schedule, fault=None, stream=None):
    """x cut into chunks of the lengths in ``schedule`` (the rest, maybe empty, goes with final) through one StreamRef."""
    x = np.asarray(x, dtype=np.float64)
    s = stream if stream is not None else StreamRef(src, dst, fault)
    out, at = [], 0
    for m in schedule:
        out.append(s.feed(x[at:at + m]))
        at += m
    out.append(s.feed(x[at:], final=True))
    return np.concatenate(out)
