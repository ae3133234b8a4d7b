"""The speech-to-text front end on the device: a pool of stateful Whisper log-mel streams (include/mimi_hip.h, mimi_mel_pool_*).

Every Whisper-family recogniser takes the same input: an 80- or 128-band log-mel spectrogram of 30 s at 16 kHz.  It is a pure function of
the samples and causal but for a final clamp, so a stream computes it WHILE the turn is spoken, as the codes are: ``MelPool.feed`` gives
the raw rows each stream completes (two launches whatever the streams and their chunk lengths; a 400-point DFT per frame as an fp32
matrix product on the matrix cores), ``finish`` turns a clip's rows into the ``(n_mels, 3000)`` features.  A stream's rows, concatenated
over any chunk schedule, are bit for bit its one-shot rows (tests/mel_ref.py states the rule in float64).  ``TurnFeatures`` puts a
resampler in front, for ``TurnStreams(features=)``.  All arithmetic is the library's; this file marshals.

Not built: turns longer than 30 s (Whisper's long-form windows: samples past 480,000 are counted and dropped), the recogniser's decoder
(its encoder is sesameai/whisper_enc.py), ``generate_stream`` at B = 1, a C-host example."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch

from ._stream_pool import StreamPool, _stream, int16_if_all, pack, shared_pool, split

MAX_STREAMS = 64                 # MIMI_MEL_MAX_STREAMS
SAMPLE_RATE = 16000
FRAMES = 3000                    # MIMI_MEL_FRAMES
CAP = 480000                     # MIMI_MEL_CAP
BINS_PAD, BASIS_COLS, MAX_MELS = 224, 448, 128


class MelPool(StreamPool):
    """``n`` independent log-mel streams of ``n_mels`` (80 or 128) bands.  ``feed(ids, chunks, final)`` gives every listed stream its new
    samples at 16 kHz, fp32 or int16, and returns the raw rows ``(K_i, n_mels)`` each completes: two launches, no host-to-device copy of a
    plan, no synchronisation.  Samples past 480,000 are counted (``dropped``) and dropped.  ``final`` ends a stream's clip and leaves it
    fresh; ``reset(ids)`` is host arithmetic.  ``finish(raws)`` -> the ``(n_mels, 3000)`` features of up to 64 clips: two launches."""

    def __init__(self, n: int, n_mels: int = 80, device: Union[str, torch.device] = "cuda"):
        self.n_mels = int(n_mels)
        super().__init__("mimi_mel_pool", n, device, int(n_mels), int(n))

    def tables(self) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """For tests: the fp32 tables the device holds: window (400,), basis (400, 448), bank (224, 128)."""
        w, b, f = torch.empty(400), torch.empty(400, BASIS_COLS), torch.empty(BINS_PAD, MAX_MELS)
        self._check(self._lib.mimi_mel_pool_tables(self._h, w.data_ptr(), b.data_ptr(), f.data_ptr()))
        return w, b, f

    def frame_count(self, sid: int, n_in: int, final: bool = False) -> int:
        """Rows a feed of ``n_in`` samples would give stream ``sid`` now (host arithmetic)."""
        return self._count("frame_count", sid, n_in, final)

    def dropped(self, sid: int) -> int:
        """Samples of stream ``sid`` that fell behind the cap since it was fresh (host arithmetic)."""
        n = int(self._lib.mimi_mel_pool_dropped(self._h, int(sid)))
        if n < 0:
            self._check(-1)
        return n

    def reset(self, ids: Optional[Sequence[int]] = None) -> None:
        """Start the listed streams (default: all) afresh.  No launch."""
        ids = [int(i) for i in (range(self.n_streams) if ids is None else ids)]
        self._check(self._lib.mimi_mel_pool_reset(self._h, (C.c_int32 * max(len(ids), 1))(*ids), len(ids)))

    @torch.inference_mode()
    def feed(self, ids: Sequence[int], chunks: Sequence[torch.Tensor], final: Union[bool, Sequence[bool]] = False) -> List[torch.Tensor]:
        """ids: n distinct stream ids; chunks[i]: (n_i,) fp32 or int16 at 16 kHz, n_i >= 0, CPU or device (int16 only if every chunk is);
        final: one flag, or one per stream -> per stream its new raw rows (K_i, n_mels) fp32, views of one buffer."""
        p = pack(chunks, self.device, int16_if_all, ids, final)
        raw = torch.empty((max(sum(self._counts("frame_count", p)), 1), self.n_mels), dtype=torch.float32, device=self.device)
        n_frames = (C.c_long * p.m)()
        self._check(self._lib.mimi_mel_pool_feed(self._h, *p.head, int(p.dtype == torch.int16), raw.data_ptr(), n_frames, _stream()))
        return split(raw, n_frames[:len(p.ids)])

    @torch.inference_mode()
    def finish(self, raws: Sequence[torch.Tensor]) -> List[torch.Tensor]:
        """raws[i]: (K_i <= 3000, n_mels) fp32, a clip's raw rows -> [(n_mels, 3000) fp32], views of one buffer."""
        return finish(raws, self.n_mels, self.device)


@torch.inference_mode()
def finish(raws: Sequence[torch.Tensor], n_mels: int, device: Union[str, torch.device]) -> List[torch.Tensor]:
    """The stateless finisher (mimi_mel_finish): the clip's maximum, clamp, shift, scale, transpose; the frames a clip lacks get the
    constant.  Up to 64 clips, two launches."""
    from . import _abi
    n = len(raws)
    assert all(r.dim() == 2 and r.shape[1] == n_mels for r in raws), "every clip's rows must be (K, n_mels)"
    rows = [r.to(device=device, dtype=torch.float32) for r in raws]
    lens = [int(r.shape[0]) for r in rows]
    packed = torch.cat(rows) if sum(lens) else torch.zeros((1, n_mels), dtype=torch.float32, device=device)
    offs = [sum(lens[:k]) * n_mels for k in range(n)]
    m = max(n, 1)
    out = torch.empty((m, n_mels, FRAMES), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        rc = _abi.lib.mimi_mel_finish(packed.data_ptr(), (C.c_long * m)(*offs), (C.c_long * m)(*lens), n, int(n_mels), out.data_ptr(), _stream())
    if rc != 0:
        raise _abi.CsmError(rc, (_abi.lib.mimi_mel_last_error() or b"").decode())
    return list(out[:n].unbind(0))


_POOLS: Dict[tuple, MelPool] = {}          # log_mel()'s pools, made on first use and kept


@torch.inference_mode()
def log_mel(wavs: Sequence[torch.Tensor], n_mels: int = 80, device: Union[str, torch.device, None] = None) -> List[torch.Tensor]:
    """Up to 64 clips of different lengths, each (n_i,) fp32 or int16 at 16 kHz -> each the ``(n_mels, 3000)`` Whisper features, the way a
    live stream computes them: on fresh streams with ``final``, in ONE feed and one finish."""
    if not 1 <= len(wavs) <= MAX_STREAMS:
        raise ValueError(f"log_mel takes 1 .. {MAX_STREAMS} clips a call")
    pool = shared_pool(_POOLS, device, wavs[0], lambda dev: (str(dev), int(n_mels)), lambda dev: MelPool(MAX_STREAMS, int(n_mels), device=dev))
    ids = list(range(len(wavs)))
    pool.reset(ids)
    return pool.finish(pool.feed(ids, wavs, final=True))


class TurnFeatures:
    """The features of ``n`` spoken turns, computed while they are spoken: a ``ResamplerPool(src_rate, 16000, n)`` in front of a
    ``MelPool``.  ``feed(ids, chunks, final)`` takes each listed stream's new samples at ``src_rate`` -- one resampler call and one mel
    call -- and holds its raw rows; at ``final`` the turn's rows are finished and wait for ``take(sid) -> (features (n_mels, 3000),
    n_frames)``, oldest turn first.  The features are bit for bit ``log_mel([resample(the whole turn, src_rate, 16000)])``."""

    def __init__(self, n: int, src_rate: int = 24000, n_mels: int = 80, device: Union[str, torch.device] = "cuda"):
        self.n_streams, self.src_rate, self.n_mels = int(n), int(src_rate), int(n_mels)
        self.mel = MelPool(n, n_mels, device=device)
        self.resampler = None
        if self.src_rate != SAMPLE_RATE:
            from .resample import ResamplerPool
            self.resampler = ResamplerPool(self.src_rate, SAMPLE_RATE, n, device=device)
        self._rows: Dict[int, List[torch.Tensor]] = {s: [] for s in range(self.n_streams)}
        self._ready: Dict[int, List[Tuple[torch.Tensor, int]]] = {s: [] for s in range(self.n_streams)}

    def reset(self, ids: Optional[Sequence[int]] = None) -> None:
        """The listed streams (default: all) start a new turn; what they held of the running one is dropped."""
        ids = [int(i) for i in (range(self.n_streams) if ids is None else ids)]
        if self.resampler is not None:
            self.resampler.reset(ids)
        self.mel.reset(ids)
        for s in ids:
            self._rows[s] = []

    def feed(self, ids: Sequence[int], chunks: Sequence[torch.Tensor], final: Union[bool, Sequence[bool]] = False) -> None:
        ids = [int(i) for i in ids]
        fin = [bool(final)] * len(ids) if isinstance(final, (bool, int)) else [bool(f) for f in final]
        if self.resampler is not None:
            chunks = self.resampler.feed(ids, chunks, fin)
        done = []
        for s, rows, f in zip(ids, self.mel.feed(ids, chunks, fin), fin):
            if rows.shape[0]:
                self._rows[s].append(rows)
            if f:
                done.append(s)
        if done:
            raws = [torch.cat(self._rows[s]) if self._rows[s] else torch.empty((0, self.n_mels), device=self.mel.device) for s in done]
            for s, raw, feats in zip(done, raws, self.mel.finish(raws)):
                self._ready[s].append((feats, int(raw.shape[0])))
                self._rows[s] = []

    def pending(self, sid: int) -> int:
        """Ended turns of stream ``sid`` whose features wait for ``take``."""
        return len(self._ready[int(sid)])

    def take(self, sid: int) -> Tuple[torch.Tensor, int]:
        """The oldest ended turn of stream ``sid``: (features (n_mels, 3000) fp32, the frames that hold samples)."""
        if not self._ready[int(sid)]:
            raise ValueError(f"stream {int(sid)}: no ended turn")
        return self._ready[int(sid)].pop(0)
