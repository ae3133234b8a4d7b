"""Host reference of the device watermark (include/mimi_hip.h, mimi_wm_pool_*): THE RULE in plain NumPy with int64 arithmetic, written from
its statement and not from the kernels.  A keyed spread-spectrum mark with host-interference cancellation: every 1920-sample block of a
stream carries one of 56 symbols (a sync byte, five payload bytes, their CRC-8); a block whose own correlation with the key's chips does
not already say its bit with margin gets the smallest chip-shaped push that makes it say so.

  samples   q = clamp(rint(x * 32768), -32768, 32767) for fp32, a non-finite x gives 0; an int16 sample is its own q
  symbols   b_k = +1 / -1 for k = 0 .. 55: 0xB2, the payload's five bytes, CRC-8 (poly 0x07, init 0) of those five; MSB first
  chips     c[p] = 1 - 2 * ((w >> (p & 31)) & 1), w = philox4x32_10((p >> 7, 0, 0, 0x574D), (secret_lo, secret_hi))[(p >> 5) & 3], p in [0, P)
  embed     block J = n // S of a stream carries symbol k = J % K with chips c[n % P]; over a COMPLETE block E = sum q^2, r = sum q c,
            T = (isqrt(E) * t_q4) >> 4, u = b_k r; u >= T: D = 0, else D = b_k (T - u); a = |D| // S, rem = |D| % S,
            d[m] = sgn(D) c[m] (a + (m < rem)); fp32: y = x + float32(d) * 2^-15 where d != 0 and x is finite, else y = x (bit for bit);
            int16: y = clamp(q + d).  A trailing partial block is left as it is.
  detect    see ``detect``."""
import math

import numpy as np

from philox_ref import philox4x32_10

S, K = 1920, 56
P = S * K
SYNC = 0xB2
DOMAIN = 0x574D
DEFAULT_PAYLOAD = (212, 211, 146, 56, 201)
ALL = (1 << K) - 1
SYNC_MASK = 0xFF
ROW = 64


def crc8(data) -> int:
    c = 0
    for v in data:
        c ^= int(v) & 0xFF
        for _ in range(8):
            c = ((c << 1) ^ 0x07) & 0xFF if c & 0x80 else (c << 1) & 0xFF
    return c


def symbol_bits(payload=DEFAULT_PAYLOAD) -> int:
    """The 56 symbols as one word: bit k (LSB = symbol 0) is 1 where b_k = +1."""
    data = [int(v) & 0xFF for v in payload]
    assert len(data) == 5
    word = 0
    for j, byte in enumerate([SYNC] + data + [crc8(data)]):
        for i in range(8):
            word |= ((byte >> (7 - i)) & 1) << (8 * j + i)
    return word


def symbols(payload=DEFAULT_PAYLOAD) -> np.ndarray:
    w = symbol_bits(payload)
    return np.array([1 if (w >> k) & 1 else -1 for k in range(K)], dtype=np.int64)


def default_secret(payload=DEFAULT_PAYLOAD) -> int:
    return int.from_bytes(bytes(int(v) & 0xFF for v in payload), "big")


_CHIPS = {}


def chips(secret=None) -> np.ndarray:
    """c[0 .. P) as int64 +-1."""
    secret = default_secret() if secret is None else int(secret) & (2 ** 64 - 1)
    if secret not in _CHIPS:
        p = np.arange(P, dtype=np.uint64)
        w4 = philox4x32_10((np.arange(P >> 7, dtype=np.uint64), 0, 0, DOMAIN), (secret & 0xFFFFFFFF, secret >> 32))
        w = np.stack(w4, 1).reshape(-1).astype(np.uint64)                       # word (p >> 7) * 4 + ((p >> 5) & 3) = p >> 5
        _CHIPS[secret] = (1 - 2 * ((w[p >> np.uint64(5)] >> (p & np.uint64(31))) & np.uint64(1)).astype(np.int64))
    return _CHIPS[secret]


def quant(x: np.ndarray) -> np.ndarray:
    x = np.asarray(x)
    if x.dtype == np.int16:
        return x.astype(np.int64)
    assert x.dtype == np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        y = np.clip(np.rint(x * np.float32(32768.0)), -32768.0, 32767.0)
    return np.where(np.isfinite(x), y, 0).astype(np.int64)


def block_push(q: np.ndarray, c: np.ndarray, b: int, t_q4: int, spread: bool = True):
    """One complete block: (d[0 .. S), D)."""
    E, r = int((q * q).sum()), int((q * c).sum())
    T = (math.isqrt(E) * int(t_q4)) >> 4
    u = b * r
    D = 0 if u >= T else b * (T - u)
    a, rem = abs(D) // S, abs(D) % S
    sg = (D > 0) - (D < 0)
    d = sg * c * (a + ((np.arange(S) < rem) if spread else 0))
    return d.astype(np.int64), D


def apply_push(x: np.ndarray, d: np.ndarray) -> np.ndarray:
    if x.dtype == np.int16:
        return np.clip(x.astype(np.int64) + d, -32768, 32767).astype(np.int16)
    with np.errstate(invalid="ignore", over="ignore"):
        y = x + d.astype(np.float32) * np.float32(2.0 ** -15)
    return np.where((d != 0) & np.isfinite(x), y, x).astype(np.float32)


def embed(x: np.ndarray, payload=DEFAULT_PAYLOAD, secret=None, t_q4: int = 8, start: int = 0) -> np.ndarray:
    """A whole clip whose sample 0 is stream position ``start`` (a multiple of S)."""
    assert start % S == 0
    x = np.asarray(x)
    c, b, q = chips(default_secret(payload) if secret is None else secret), symbols(payload), quant(x)
    y = x.copy()
    for i in range(len(x) // S):
        J = start // S + i
        k = J % K
        d, _ = block_push(q[i * S:(i + 1) * S], c[k * S:(k + 1) * S], int(b[k]), t_q4)
        y[i * S:(i + 1) * S] = apply_push(x[i * S:(i + 1) * S], d)
    return y


class StreamEmbed:
    """The streamed restatement: a carry of fewer than S raw samples and the position."""

    def __init__(self, payload=DEFAULT_PAYLOAD, secret=None, t_q4: int = 8):
        self.payload, self.secret, self.t_q4 = payload, default_secret(payload) if secret is None else secret, t_q4
        self.carry, self.pos = None, 0                                  # pos: stream position of the carry's first sample

    def feed(self, chunk: np.ndarray, final: bool = False) -> np.ndarray:
        chunk = np.asarray(chunk)
        have = chunk if self.carry is None else np.concatenate([self.carry, chunk])
        n = len(have) // S * S
        out = embed(have[:n], self.payload, self.secret, self.t_q4, start=self.pos)
        if final:
            out = np.concatenate([out, have[n:]])
            self.carry, self.pos = None, 0
        else:
            self.carry, self.pos = have[n:].copy(), self.pos + n
            assert len(self.carry) < S
        return out


def correlations(q: np.ndarray, c: np.ndarray, offsets: np.ndarray):
    """For every candidate offset: R[K] int64 and cov[K], and the number of complete blocks."""
    N, C = len(q), len(offsets)
    offsets = np.asarray(offsets, dtype=np.int64)
    first = (-offsets) % S
    nb = np.where(N >= first, (N - first) // S, 0)
    R, cov = np.zeros((C, K), dtype=np.int64), np.zeros((C, K), dtype=np.int64)
    if N == 0 or nb.max(initial=0) == 0:
        return R, cov, nb
    cext = np.resize(c, P + N)                                           # (repeats the period)
    win = np.lib.stride_tricks.sliding_window_view(cext, N)              # win[o][j] = c[(o + j) % P]
    step = max(1, 4_000_000 // N)
    nbm = int(nb.max())
    for lo in range(0, C, step):
        o, f, n_ = offsets[lo:lo + step], first[lo:lo + step], nb[lo:lo + step]
        cs = np.concatenate([np.zeros((len(o), 1), dtype=np.int64), np.cumsum(q[None, :] * win[o], axis=1)], axis=1)
        i = np.arange(nbm)[None, :]
        ok = i < n_[:, None]
        a = np.where(ok, f[:, None] + i * S, 0)
        r = np.where(ok, np.take_along_axis(cs, np.where(ok, a + S, 0), 1) - np.take_along_axis(cs, a, 1), 0)
        k = (((o + f) // S)[:, None] + i) % K
        rows = np.broadcast_to(np.arange(len(o))[:, None], k.shape)
        np.add.at(R[lo:lo + step], (rows[ok], k[ok]), r[ok])
        np.add.at(cov[lo:lo + step], (rows[ok], k[ok]), 1)
    return R, cov, nb


def score_rows(R: np.ndarray, cov: np.ndarray, expect: int, mask: int):
    b = np.array([1 if (expect >> k) & 1 else -1 for k in range(K)], dtype=np.int64)
    m = np.array([(mask >> k) & 1 for k in range(K)], dtype=bool)
    on = m[None, :] & (cov > 0)
    return (on & (np.sign(R) == b[None, :])).sum(1), on.sum(1)


def detect(x: np.ndarray, payload=None, secret=None, o0: int = 0, n_off: int = P, expect=None, mask=None) -> np.ndarray:
    """-> the 64 int64 of one clip: best i, its offset, score, covered, complete blocks, decoded payload (40 bits), CRC flag, 0, R_0 .. R_55.
    Candidate i says "clip sample 0 is stream position (o0 + i) % P".  payload None: the sync byte alone (of the default payload's word).
    The CRC flag: every symbol 8 .. 55 has a block and a non-zero R, and the CRC-8 of the five decoded bytes is the decoded sixth."""
    if expect is None:
        expect = symbol_bits(DEFAULT_PAYLOAD if payload is None else payload)
    if mask is None:
        mask = SYNC_MASK if payload is None else ALL
    if secret is None:
        secret = default_secret(DEFAULT_PAYLOAD if payload is None else payload)
    q = quant(x)
    offsets = (int(o0) + np.arange(int(n_off), dtype=np.int64)) % P
    R, cov, nb = correlations(q, chips(secret), offsets)
    score, covered = score_rows(R, cov, expect, mask)
    i = int(np.argmax(score))                                            # the first of the highest
    row = np.zeros(ROW, dtype=np.int64)
    bits = [int(R[i, k] > 0) for k in range(K)]
    data = [sum(bits[8 * j + t] << (7 - t) for t in range(8)) for j in range(1, 7)]
    decided = all(cov[i, k] > 0 and R[i, k] != 0 for k in range(8, K))
    row[:8] = [i, offsets[i], score[i], covered[i], nb[i], int.from_bytes(bytes(data[:5]), "big"), int(decided and crc8(data[:5]) == data[5]), 0]
    row[8:] = R[i]
    return row


def verify_row(row) -> bool:
    """The decision of ``sesameai.watermarking.verify`` on a detect row: covered >= 16 and at most covered // 8 of them wrong."""
    score, covered = int(row[2]), int(row[3])
    return covered >= 16 and covered - score <= covered // 8


def synthetic_voice(seconds: float = 10.0, seed: int = 0) -> np.ndarray:
    """19 harmonics of 140 Hz under a 3 Hz envelope, peak about 0.4, plus hiss at 0.003."""
    n = int(seconds * 24000)
    t = np.arange(n) / 24000.0
    g = np.random.default_rng(seed)
    v = sum(np.sin(2 * np.pi * 140.0 * h * t + g.uniform(0, 2 * np.pi)) / h for h in range(1, 20))
    v = v * (0.55 + 0.45 * np.sin(2 * np.pi * 3.0 * t))
    v = 0.4 * v / np.abs(v).max()
    return (v + 0.003 * g.standard_normal(n)).astype(np.float32)
