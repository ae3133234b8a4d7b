"""NumPy statement of the time-stretch rule (include/mimi_hip.h, mimi_ts_pool_*): WSOLA with a 512-sample block and hop, a +-256-sample
alignment search on 12-bit search samples scored in exact integers, the first-index argmax, and an fp32 crossfade of two multiplies and one
add.  Every decision is integer arithmetic, so the device is held to this bit for bit.  ``stretch_ref`` is the whole-clip rule;
``StreamRef`` restates it the way the pool keeps a stream -- a carry of fewer than 2,560 samples, the last block's position, positions
relative to the carry's base -- and ``emitted`` / ``out_count`` are the host's counts.  ``search=False`` (d = 0 everywhere: overlap-add
without alignment) and ``tie='last'`` are the two ways of getting the rule wrong that tests/test_stretch_oracle.py shows to matter."""
import numpy as np

H = 512                     # block and hop
D = 256                     # search radius
CARRY = 2560                # floats a stream keeps between calls
PM_MIN, PM_MAX = 500, 2000
LOOK = D + 2 * H            # block k comes out once a_k + LOOK samples are in


def to_pm(speed):
    return int(round(float(speed) * 1000))


def quant(x):
    """q[i] = clamp(rint(x[i] * 2048), -2047, 2047) as int64; a non-finite sample gives 0."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(all="ignore"):
        v = np.clip(np.rint(x * np.float32(2048.0)), -2047.0, 2047.0)
    return np.where(np.isfinite(x), v, 0.0).astype(np.int64)


def out_len(N, pm):
    return (N * 1000 + pm - 1) // pm


def a_of(k, pm):
    return (k * H * pm) // 1000


def emitted(R, pm, final):
    """Blocks a stream has emitted after R samples in all."""
    if final:
        return -(-out_len(R, pm) // H)
    T = R - LOOK
    return 0 if T < 0 else ((T + 1) * 1000 - 1) // (H * pm) + 1


def out_count(R, k, pm, n_in, final):
    """Samples a feed of n_in samples gives a stream that holds R samples and has emitted k blocks."""
    e = emitted(R + n_in, pm, final)
    return out_len(R + n_in, pm) - k * H if final else (e - k) * H


def _ext(v, lo, n):
    """v zero-extended, [lo, lo + n)"""
    out = np.zeros(n, dtype=v.dtype)
    a, b = max(lo, 0), min(lo + n, v.shape[0])
    if b > a:
        out[a - lo:b - lo] = v[a:b]
    return out


def scores(q, a, b):
    """S(d) for d = -D .. D as exact int64: sum_j q[a + d + j] * q[b + j] on the zero-extended q."""
    t = _ext(q, b, H)
    r = _ext(q, a - D, 2 * H)
    return np.correlate(r, t, mode="valid")                  # 2H - H + 1 = 513 values, [e] = sum_j r[e + j] t[j]


_RAMP = (np.arange(H, dtype=np.float32) / np.float32(H)).astype(np.float32)
_RAMP1 = (np.float32(1.0) - _RAMP).astype(np.float32)


def mix(xc, xb):
    """fl(fl(xc * r) + fl(xb * (1 - r))): two fp32 multiplies and one fp32 add"""
    with np.errstate(all="ignore"):
        return (xc * _RAMP).astype(np.float32) + (xb * _RAMP1).astype(np.float32)


def pick(S, tie="first"):
    return int(np.argmax(S)) if tie == "first" else int(S.shape[0] - 1 - np.argmax(S[::-1]))


def stretch_ref(x, pm, search=True, tie="first", want_scores=False):
    """x (N,) fp32, pm in [500, 2000] -> (y (M,) fp32, d (K,) int32 with d[0] = 0)[, the largest score met]"""
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
    assert PM_MIN <= pm <= PM_MAX
    N = x.shape[0]
    M = out_len(N, pm)
    K = -(-M // H)
    q = quant(x)
    y = np.zeros(K * H, dtype=np.float32)
    d = np.zeros(K, dtype=np.int32)
    c, top = 0, 0
    if K:
        y[:H] = _ext(x, 0, H)
    for k in range(1, K):
        a, b = a_of(k, pm), c + H
        if search:
            S = scores(q, a, b)
            top = max(top, int(S.max()))
            d[k] = pick(S, tie) - D
        c = a + int(d[k])
        y[k * H:(k + 1) * H] = mix(_ext(x, c, H), _ext(x, b, H))
    return (y[:M], d, top) if want_scores else (y[:M], d)


def history_needed(pm, kmax=4000):
    """The most samples a stream must keep after a feed: R - max(0, a_(k'-1) - D) just before block k' may come out."""
    worst = LOOK - 1                                           # k' = 0: everything so far
    for k in range(1, kmax):
        worst = max(worst, a_of(k, pm) + LOOK - 1 - max(0, a_of(k - 1, pm) - D))
    return worst


class StreamRef:
    """One stream the way the pool keeps it: {pm, R, k} on the host; the carry (from ``base`` = max(0, a_(k-1) - D) on) and c of the last
    block, relative to the base, on the 'device'."""

    def __init__(self, pm):
        self.reset(pm)
        self.carry = np.zeros(0, dtype=np.float32)
        self.c = 0

    def reset(self, pm):
        assert PM_MIN <= pm <= PM_MAX
        self.pm, self.R, self.k = pm, 0, 0

    def _base(self, k):
        return max(0, a_of(k - 1, self.pm) - D) if k >= 1 else 0

    def feed(self, chunk, final=False):
        chunk = np.asarray(chunk, dtype=np.float32)
        pm, k0 = self.pm, self.k
        base = self._base(k0)
        buf = np.concatenate([self.carry if k0 or self.R else self.carry[:0], chunk])      # buf[p] = sample base + p
        assert buf.shape[0] == self.R + chunk.shape[0] - base
        R1 = self.R + chunk.shape[0]
        k1 = emitted(R1, pm, final)
        n_out = out_count(self.R, k0, pm, chunk.shape[0], final)
        q = quant(buf)
        y = np.zeros(max(k1 - k0, 0) * H, dtype=np.float32)
        d = np.zeros(max(k1 - k0, 0), dtype=np.int32)
        c = self.c
        for k in range(k0, k1):
            i = k - k0
            if k == 0:
                y[:H] = _ext(buf, 0, H)
                c = 0
                continue
            a, b = a_of(k, pm) - base, c + H
            d[i] = pick(scores(q, a, b)) - D
            c = a + int(d[i])
            y[i * H:(i + 1) * H] = mix(_ext(buf, c, H), _ext(buf, b, H))
        if final:
            self.carry, self.c = buf[:0], 0
            self.reset(pm)
        else:
            shift = self._base(k1) - base
            self.carry, self.c = buf[shift:].copy(), c - shift
            assert self.carry.shape[0] < CARRY and (k1 == 0 or self.c >= 0)
            self.R, self.k = R1, k1
        return y[:n_out], d


def cut(N, schedule):
    """Chunk bounds of a clip of N samples: the schedule's lengths while they fit; what is left (maybe nothing) goes with final."""
    out, at = [], 0
    for m in schedule:
        m = min(m, N - at)
        out.append((at, at + m))
        at += m
    return out, at


def stretch_streamed(x, pm, schedule):
    x = np.asarray(x, dtype=np.float32)
    s = StreamRef(pm)
    ys, ds = [], []
    parts, at = cut(x.shape[0], schedule)
    for lo, hi in parts:
        y, d = s.feed(x[lo:hi])
        ys.append(y); ds.append(d)
    y, d = s.feed(x[at:], final=True)
    ys.append(y); ds.append(d)
    return np.concatenate(ys), np.concatenate(ds)
