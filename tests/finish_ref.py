"""The finishing rule of a segment (include/mimi_hip.h, mimi_fin_*), written once in NumPy fp32: the oracle the device finisher is graded against.

One clip ``x`` (fp32, N >= 0 samples) with lead L, tail T and fade F, in samples:
  1. peak = max(max |x_i| over the finite samples, float32(1e-6));
  2. q_i = trunc((x_i / peak) * 32767.0f), every operation in fp32, ``/`` the IEEE division; a non-finite x_i gives 0;
  3. y = L zeros ++ q ++ T zeros, M = L + N + T;
  4. n = min(F, M // 2); ramp r_j = float32(j * (1.0 / (n - 1))) in float64, r_(n-1) = 1, r_0 = 0 for n == 1;
     y[j] = trunc(float32(y[j]) * r_j), y[M - n + j] = trunc(float32(y[M - n + j]) * r_(n-1-j)).
This is the arithmetic of ``tts_service.TTS.generate_audio_segment`` (tests/test_finish_oracle.py holds the two together)."""
import numpy as np

PEAK_FLOOR = np.float32(1e-6)


def ms_to_samples(ms: int, sample_rate: int) -> int:
    return sample_rate * int(ms) // 1000


def ramp(n: int) -> np.ndarray:
    """r_0 .. r_(n-1) by the formula of step 4 (NOT by np.linspace: the tests compare the two)."""
    if n <= 0:
        return np.zeros(0, np.float32)
    if n == 1:
        return np.zeros(1, np.float32)
    step = 1.0 / float(n - 1)
    r = (np.arange(n, dtype=np.float64) * step).astype(np.float32)
    r[n - 1] = np.float32(1.0)
    return r


def peak_of(x: np.ndarray) -> np.float32:
    x = np.asarray(x, np.float32).reshape(-1)
    a = np.abs(x[np.isfinite(x)])
    return np.maximum(a.max() if a.size else np.float32(0.0), PEAK_FLOOR).astype(np.float32)


def quantise(x: np.ndarray, reciprocal: bool = False) -> np.ndarray:
    """Steps 1 and 2.  ``reciprocal=True`` is the WRONG variant x * (1 / peak): the tests use it to show that the comparison tells the two apart."""
    x = np.asarray(x, np.float32).reshape(-1)
    peak = peak_of(x)
    fin = np.isfinite(x)
    xs = np.where(fin, x, np.float32(0.0)).astype(np.float32)
    scaled = xs * (np.float32(1.0) / peak) if reciprocal else xs / peak
    assert scaled.dtype == np.float32
    q = (scaled * np.float32(32767.0)).astype(np.float32)
    return np.trunc(q).astype(np.int16)


def finish_ref(x: np.ndarray, lead: int, tail: int, fade: int, reciprocal: bool = False) -> np.ndarray:
    """-> int16 (lead + N + tail,); lead, tail, fade in samples."""
    q = quantise(x, reciprocal)
    y = np.concatenate([np.zeros(int(lead), np.int16), q, np.zeros(int(tail), np.int16)])
    n = min(int(fade), len(y) // 2)
    if n > 0:
        r = ramp(n)
        y[:n] = np.trunc(y[:n].astype(np.float32) * r).astype(np.int16)
        y[len(y) - n:] = np.trunc(y[len(y) - n:].astype(np.float32) * r[::-1]).astype(np.int16)
    return y


def finish_ref_ms(x: np.ndarray, lead_ms: int = 500, tail_ms: int = 100, fade_ms: int = 50, sample_rate: int = 24000) -> np.ndarray:
    return finish_ref(x, ms_to_samples(lead_ms, sample_rate), ms_to_samples(tail_ms, sample_rate), ms_to_samples(fade_ms, sample_rate))
