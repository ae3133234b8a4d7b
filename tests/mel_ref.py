"""The Whisper log-mel feature rule in float64 NumPy, restated so that a stream can follow it (include/mimi_hip.h, mimi_mel_pool_*).

Signal: s is 480,000 samples at 16 kHz, the clip's first min(L, 480000) and zeros behind them (int16 is x 2^-15).  It is padded by
reflection with 200 samples at both ends.  Frame t = 0 .. 2999 reads p[160 t .. 160 t + 399], times the PERIODIC Hann window;
P[k] = |DFT_400|^2 for k = 0 .. 200; mel[m] = sum_k F[k][m] P[k] with F the Slaney-scale, Slaney-normalised triangular bank over
0 .. 8000 Hz; raw[t][m] = log10(max(mel, 1e-10)).  Features: (max(raw, max(raw) - 8) + 4) / 4 as (n_mels, 3000) fp32.

Streaming: a frame is emitted as soon as every sample it reads has been received, or is known to be zero or reflected -- which only
`final` or the cap of 480,000 samples settle.  ``variant`` switches ONE ingredient to a plausible wrong one; the oracle test shows that
each moves the features far outside the bound the device is held to."""
import numpy as np

RATE, NFFT, HOP, PAD, CAP, FRAMES, BINS = 16000, 400, 160, 200, 480000, 3000, 201
LOG_FLOOR = -10.0


def window(symmetric=False):
    n = np.arange(NFFT, dtype=np.float64)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * n / (NFFT - 1 if symmetric else NFFT))


def hz_to_mel(hz, htk=False):
    hz = np.asarray(hz, dtype=np.float64)
    if htk:
        return 2595.0 * np.log10(1.0 + hz / 700.0)
    return np.where(hz >= 1000.0, 15.0 + np.log(np.maximum(hz, 1e-30) / 1000.0) * (27.0 / np.log(6.4)), 3.0 * hz / 200.0)


def mel_to_hz(mel, htk=False):
    mel = np.asarray(mel, dtype=np.float64)
    if htk:
        return 700.0 * (10.0 ** (mel / 2595.0) - 1.0)
    return np.where(mel >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (mel - 15.0)), 200.0 * mel / 3.0)


def bank(n_mels, htk=False):
    """(201, n_mels): triangles between n_mels + 2 edges evenly spaced in mel, each scaled by 2 / (upper edge - lower edge) in Hz."""
    edges = mel_to_hz(np.linspace(hz_to_mel(0.0, htk), hz_to_mel(RATE / 2.0, htk), n_mels + 2), htk)
    f = np.linspace(0.0, RATE / 2.0, BINS)[:, None]
    up = (f - edges[None, :-2]) / (edges[1:-1] - edges[:-2])[None]
    down = (edges[None, 2:] - f) / (edges[2:] - edges[1:-1])[None]
    return np.maximum(0.0, np.minimum(up, down)) * (2.0 / (edges[2:] - edges[:-2]))[None]


def basis():
    """(400, 201) cos and -sin of 2 pi n k / 400, the angle reduced in integers."""
    a = 2.0 * np.pi * ((np.arange(NFFT)[:, None] * np.arange(BINS)[None]) % NFFT) / NFFT
    return np.cos(a), -np.sin(a)


def as_float(x):
    x = np.asarray(x)
    return x.astype(np.float64) / 32768.0 if x.dtype == np.int16 else x.astype(np.float64)


def frames_needed(R, final):
    """Frames that R <= CAP received samples settle."""
    if final:
        return min(FRAMES, -(-(R + PAD) // HOP))
    if R >= CAP:
        return FRAMES
    return 0 if R <= PAD else (R - PAD) // HOP + 1


def _rows(s, t0, t1, n_mels, variant=None):
    """raw rows t0 .. t1 - 1 of the clip whose samples so far are ``s`` (float64, len <= CAP; zeros behind them)."""
    if t1 <= t0:
        return np.zeros((0, n_mels))
    hop = 159 if variant == "hop159" else HOP
    full = np.zeros(CAP)
    full[:len(s)] = s
    p = np.pad(full, PAD, mode="constant" if variant == "zero_pad_left" else "reflect")
    if variant == "zero_pad_left":
        p[-PAD:] = full[-2:-PAD - 2:-1]
    w, (c, ms), fb = window(variant == "symmetric"), basis(), bank(n_mels, variant == "htk")
    mel = np.empty((t1 - t0, n_mels))
    for t in range(t0, t1):              # frame by frame, each with the same three products: a row does not depend on its company
        fr = p[t * hop:t * hop + NFFT] * w
        mel[t - t0] = ((fr @ c) ** 2 + (fr @ ms) ** 2) @ fb
    mel = np.maximum(mel, 1e-10)
    return np.log(mel) if variant == "ln" else np.log10(mel)


def finish(raw, n_mels, variant=None):
    """raw: (K <= 3000, n_mels) -> (n_mels, 3000) fp32; the frames behind K are the constant."""
    full = np.full((FRAMES, n_mels), np.log(1e-10) if variant == "ln" else LOG_FLOOR)
    full[:len(raw)] = raw
    top = full.max(axis=1, keepdims=True) if variant == "frame_max" else full.max()
    return ((np.maximum(full, top - 8.0) + 4.0) / 4.0).T.astype(np.float32)


def raw_rows(x, n_mels=80, variant=None):
    """One shot: the clip's live rows (min(3000, ceil((L + 200) / 160)), n_mels), float64."""
    s = as_float(x)[:CAP]
    return _rows(s, 0, frames_needed(len(s), True), n_mels, variant)


def log_mel(x, n_mels=80, variant=None):
    return finish(raw_rows(x, n_mels, variant), n_mels, variant)


class MelStream:
    """Fed in chunks; the rows it returns, concatenated, are ``raw_rows`` of everything fed."""

    def __init__(self, n_mels=80):
        self.n_mels = n_mels
        self.reset()

    def reset(self):
        self.s, self.frames, self.dropped = np.zeros(0), 0, 0

    def frame_count(self, n_in, final=False):
        return frames_needed(min(len(self.s) + n_in, CAP), final) - self.frames

    def feed(self, chunk, final=False):
        chunk = as_float(chunk)
        use = min(len(chunk), CAP - len(self.s))
        self.dropped += len(chunk) - use
        self.s = np.concatenate([self.s, chunk[:use]])
        upto = frames_needed(len(self.s), final)
        # a frame emitted before `final` reads received samples only: computing it from what is in so far IS its final value
        rows = _rows(self.s, self.frames, upto, self.n_mels)
        self.frames = upto
        if final:
            self.reset()
        return rows


# ---- the seeded test signals (tools/mel_golden.py stores the transformers extractor's features of them in tests/golden/mel.pt) ----
def signal(name, seed, length):
    """(length,) float32 in [-1, 1], or int16 for the names that end in ``_i16``."""
    rng = np.random.RandomState(seed)
    t = np.arange(length, dtype=np.float64) / RATE
    if name.startswith("speech"):
        # harmonic bursts (a gliding pitch, 24 harmonics at 1 / h, two formant-like bumps) with pauses, over a noise floor 60 dB below
        f0 = 110.0 + 40.0 * np.sin(2.0 * np.pi * 0.7 * t + rng.uniform(0, 6.28))
        phase = 2.0 * np.pi * np.cumsum(f0) / RATE
        x = np.zeros(length)
        for h in range(1, 25):
            bump = 1.0 + 3.0 * np.exp(-((h * 130.0 - 700.0) / 300.0) ** 2) + 2.0 * np.exp(-((h * 130.0 - 2300.0) / 400.0) ** 2)
            x += bump / h * np.sin(h * phase + rng.uniform(0, 6.28))
        env = ((t % 0.45) < 0.3).astype(np.float64) * (0.5 - 0.5 * np.cos(2.0 * np.pi * np.minimum((t % 0.45) / 0.3, 1.0)))
        x = 0.3 * x / max(np.abs(x).max(), 1e-9) * env + 0.3e-3 * rng.standard_normal(length)
        if "quiet" in name:
            x = x * 0.01                                        # the same 40 dB quieter
    elif name.startswith("sine_silence_noise"):
        a, b = int(0.4 * length), int(0.7 * length)            # a 1 kHz sine, then silence, then faint noise: the clamp holds most frames
        x = np.zeros(length)
        x[:a] = 0.5 * np.sin(2.0 * np.pi * 1000.0 * t[:a])
        x[b:] = 1e-4 * rng.standard_normal(length - b)
    else:
        raise ValueError(name)
    if name.endswith("_i16"):
        return np.round(x * 32767.0).astype(np.int16)
    return x.astype(np.float32)


# (generator name, seed, length, n_mels): the fixture's inputs, in its order
GOLDEN_INPUTS = [
    ("speech", 11, 32000, 80), ("speech_quiet", 11, 32000, 80), ("sine_silence_noise", 12, 40000, 80), ("speech_i16", 13, 24000, 128),
    ("speech", 14, 1, 80), ("speech", 15, 200, 80), ("speech", 16, 201, 80), ("speech", 17, 360, 128), ("speech", 18, 361, 80),
    ("speech", 19, 5000, 80), ("speech", 20, 48077, 128),
    ("speech", 21, 479801, 80), ("speech", 22, 480000, 80), ("speech", 23, 481000, 80),
]


def golden_frames(length):
    """The frames of a clip whose extractor features the fixture stores: all the live ones, but for the three 30 s clips (3000 frames of
    80 fp32 each would pass the size a committed file may have): their first 8, every 61st, and their last 40."""
    live = frames_needed(min(length, CAP), True)
    if live < 1000:
        return np.arange(live)
    return np.unique(np.concatenate([np.arange(8), np.arange(0, live, 61), np.arange(live - 40, live)]))
