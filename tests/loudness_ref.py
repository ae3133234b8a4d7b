"""NumPy statement of the loudness rule (include/mimi_hip.h, mimi_ld_pool_* and mimi_fin_segments_ld): ITU-R BS.1770-4 / EBU R 128 for one
channel at 24 kHz, made integer, and the clip gain the finisher takes from it.  Every number that decides a sample is an exact integer, or
a spelled-out float64 / fp32 formula on integers, so the device is held to this bit for bit.

  1. samples s[i] as the VAD reads them (``vad_ref.to_s``); K-weighting as an integer FIR of T = 512 taps at Q = 14 bits
     (tools/loudness_taps.py makes them): z[i] = (sum_j hq[j] s[i - j] + 2^13) >> 14, s zero in front of the clip.
  2. hop h covers samples [h H, (h + 1) H), H = 2400: e[h] = sum z^2, an exact integer; a trailing partial hop has none.
  3. blocks E[j] = e[j] + .. + e[j + 3] over the HELD hops (the last ``ring`` ones); absolute gate E > GATE_ABS (-70 LUFS); relative gate
     10 n_abs E > S_abs (10 LU under the mean of the absolutely gated blocks); S, n = sum and count of the blocks behind both gates;
     peak = max |s| over every sample taken.
  4. clip gain g = fp32(min(sqrt((f64(P_T * 4H) * f64(n)) / f64(S)), f64(C) / f64(peak))), q = clamp(trunc(fp32(fp32(x * g) * 32767)),
     +-32767); a clip with n == 0, or without a target, takes the finisher's peak rule (tests/finish_ref.py)."""
import importlib.util
import math
import os

import numpy as np

import finish_ref
from vad_ref import to_s

_spec = importlib.util.spec_from_file_location(
    "loudness_taps", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "loudness_taps.py"))
loudness_taps = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(loudness_taps)

T = 512
Q = 14
H = 2400
RING = 4096
GATE_ABS = 1208568          # floor(4 H 2^30 10^((-70 + 0.691) / 10))
CARRY = T - 1 + H           # int16 values a stream keeps between calls, at most CARRY - 1 = 2910

HQ = np.array(loudness_taps.taps(T, Q), dtype=np.int64)
assert int(np.abs(HQ).sum()) * 32768 < 2 ** 31, "an int32 accumulation could overflow"
assert GATE_ABS == math.floor(4 * H * 2 ** 30 * 10 ** ((-70 + 0.691) / 10))


def kweight(s: np.ndarray, hq: np.ndarray = HQ, q: int = Q) -> np.ndarray:
    """z for every sample of s (int64), s zero in front"""
    s = np.asarray(s, np.int64)
    if s.shape[0] == 0:
        return s.copy()
    acc = np.convolve(s, hq)[:s.shape[0]]                     # exact: |acc| < 2^31
    return (acc + (1 << (q - 1))) >> q


def hop_energies(s: np.ndarray, hq: np.ndarray = HQ, q: int = Q) -> np.ndarray:
    """e[h] for the complete hops of s, int64"""
    z = kweight(s, hq, q)
    k = z.shape[0] // H
    return (z[:k * H] ** 2).reshape(k, H).sum(axis=1)


def gate(e, ring: int = RING, relative: bool = True):
    """(S, n) by exact two-pass gating over the last ``ring`` hops of e; Python integers"""
    e = [int(v) for v in e][-ring:] if len(e) else []
    E = [e[j] + e[j + 1] + e[j + 2] + e[j + 3] for j in range(len(e) - 3)]
    a = [v for v in E if v > GATE_ABS]
    if not relative:
        return sum(a), len(a)
    s_abs, n_abs = sum(a), len(a)
    assert 10 * n_abs * max(a, default=0) < 2 ** 63
    r = [v for v in a if 10 * n_abs * v > s_abs]
    return sum(r), len(r)


def measure_ref(x, ring: int = RING, relative: bool = True):
    """x: fp32 or int16 clip -> (S, n, peak, hops)"""
    s = to_s(np.asarray(x).reshape(-1))
    e = hop_energies(s)
    S, n = gate(e, ring, relative)
    return S, n, int(np.abs(s).max()) if s.shape[0] else 0, int(e.shape[0])


def lufs(S: int, n: int) -> float:
    """the integrated loudness, for display: -inf where nothing passed the gates"""
    return -0.691 + 10.0 * math.log10(S / (n * 4.0 * H * 32768.0 ** 2)) if n > 0 and S > 0 else float("-inf")


def target_ms(loudness: float) -> int:
    """P_T: the K-weighted mean square, in int16 units, of a signal at ``loudness`` LUFS"""
    return int(round(2.0 ** 30 * 10.0 ** ((float(loudness) + 0.691) / 10.0)))


def ceiling_i16(ceiling_db: float) -> int:
    """C: the sample ceiling, in int16 units"""
    return max(1, min(32767, int(math.floor(32767.0 * 10.0 ** (float(ceiling_db) / 20.0)))))


def clip_gain(S: int, n: int, peak: int, P_T: int, C: int):
    """(g as fp32, whether the ceiling bound it)"""
    g1 = np.sqrt((np.float64(P_T * 4 * H) * np.float64(n)) / np.float64(S))
    g2 = np.float64(C) / np.float64(peak)
    return np.float32(min(g1, g2)), bool(g2 < g1)


def quantise_ld(x: np.ndarray, g: np.float32) -> np.ndarray:
    x = np.asarray(x, np.float32).reshape(-1)
    xs = np.where(np.isfinite(x), x, np.float32(0.0)).astype(np.float32)
    with np.errstate(all="ignore"):
        u = ((xs * np.float32(g)).astype(np.float32) * np.float32(32767.0)).astype(np.float32)
        return np.clip(np.trunc(u), -32767.0, 32767.0).astype(np.int16)


def finish_ld_ref(x: np.ndarray, lead: int, tail: int, fade: int, P_T: int = 0, C: int = 32767, ring: int = RING) -> np.ndarray:
    """finish_ref with the clip gain in the place of the peak rule; P_T == 0, or a clip that passes no block, is finish_ref itself"""
    x = np.asarray(x, np.float32).reshape(-1)
    S, n, peak, _ = measure_ref(x, ring)
    if P_T <= 0 or n == 0:
        return finish_ref.finish_ref(x, lead, tail, fade)
    g, _ = clip_gain(S, n, peak, P_T, C)
    q = quantise_ld(x, g)
    y = np.concatenate([np.zeros(int(lead), np.int16), q, np.zeros(int(tail), np.int16)])
    m = min(int(fade), len(y) // 2)
    if m > 0:
        r = finish_ref.ramp(m)
        y[:m] = np.trunc(y[:m].astype(np.float32) * r).astype(np.int16)
        y[len(y) - m:] = np.trunc(y[len(y) - m:].astype(np.float32) * r[::-1]).astype(np.int16)
    return y


class StreamRef:
    """The rule the way the pool keeps a stream: a carry of at most 2910 samples, a ring of hop energies, the peak so far."""

    def __init__(self, ring: int = RING):
        self.ring_size = ring
        self.reset()

    def reset(self):
        self.R, self.k, self.peak = 0, 0, 0
        self.carry = np.zeros(0, np.int64)
        self.ring = {}

    def feed(self, x, final: bool = False) -> np.ndarray:
        """-> the hop energies this chunk completes"""
        s = to_s(np.asarray(x).reshape(-1))
        buf = np.concatenate([self.carry, s])                  # from max(k H - (T - 1), 0) on
        base = max(self.k * H - (T - 1), 0)
        lead = base - (self.k * H - (T - 1))                   # rule zeros in front
        w = np.concatenate([np.zeros(lead, np.int64), buf])
        self.R += s.shape[0]
        nf = self.R // H - self.k
        out = np.zeros(nf, np.int64)
        for i in range(nf):
            win = w[i * H:i * H + H + T - 1]
            acc = np.convolve(win, HQ)[T - 1:T - 1 + H]
            z = (acc + (1 << (Q - 1))) >> Q
            out[i] = int((z * z).sum())
            self.ring[(self.k + i) % self.ring_size] = int(out[i])
        if s.shape[0]:
            self.peak = max(self.peak, int(np.abs(s).max()))
        self.k += nf
        self.last = (self.k, self.peak, dict(self.ring))
        if final:
            self.R, self.k, self.peak, self.carry, self.ring = 0, 0, 0, np.zeros(0, np.int64), {}
        else:
            keep = min(self.R, T - 1 + self.R % H)
            self.carry = buf[buf.shape[0] - keep:]
            assert keep < CARRY
        return out

    def integrate(self):
        """(S, n, peak, hops) as of the last call"""
        k, peak, ring = self.last
        held = [ring[h % self.ring_size] for h in range(max(0, k - self.ring_size), k)]
        S, n = gate(held, self.ring_size)
        return S, n, peak, k
