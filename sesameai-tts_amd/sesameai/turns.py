"""The user's spoken turns of several conversations, encoded WHILE they are spoken (the reference's voice chat puts the user's turn into the
context as ``Segment(text=user_msg, speaker=1, audio=user_aud)``, ogwebapp.py:76-125, and can only encode it after the turn has ended).

``TurnStreams`` sits on a pool of stateful Mimi encode streams (``MimiCodec.open_encode_streams``): ``feed`` buffers a microphone's new
samples, ``pump`` encodes every stream's whole frames in ONE pool call, and ``finish`` encodes what is left of a turn -- the partial last
frame included -- and hands back a ``Segment`` with ``audio_codes``: bit for bit the codes ``MimiCodec.encode`` gives the whole turn.  When
the turn ends, all of it but the last call's frames is already on the device.  With a ``resampler`` (a ``ResamplerPool`` from the
microphones' rate to the codec's, sesameai/resample.py) the samples come at the microphones' rate, fp32 or int16: the codes are then those
of ``encode(resample(the whole turn))``.  Host logic only; the arithmetic is the pools'."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Union

import torch


class TurnStreams:
    def __init__(self, pool, hop: int, chunk_frames: int = 10, resampler=None):
        """pool: anything with ``n_streams``, ``encode(ids, wavs) -> [(32, T_i)]`` and ``reset(ids)`` (``MimiEncodeStreamPool``);
        chunk_frames: the most frames one stream gives one call (at most the pool's ``max_chunk_frames``);
        resampler: None (samples come at 24 kHz: today's calls exactly), or anything with ``feed(ids, chunks, final) -> [(m_i,)]`` and
        ``reset(ids)`` over at least ``pool.n_streams`` streams (``ResamplerPool``)."""
        assert chunk_frames >= 1 and hop >= 1
        self.pool, self.hop, self.chunk_frames, self.resampler = pool, int(hop), int(chunk_frames), resampler
        self._buf: Dict[int, Optional[torch.Tensor]] = {s: None for s in range(pool.n_streams)}     # samples not yet encoded
        self._codes: Dict[int, List[torch.Tensor]] = {s: [] for s in range(pool.n_streams)}         # the turn's codes so far
        self._raw: Dict[int, List[torch.Tensor]] = {s: [] for s in range(pool.n_streams)}           # (resampler) samples not yet resampled
        self._fed: Dict[int, bool] = {s: False for s in range(pool.n_streams)}                      # (resampler) the turn has had samples

    def buffered(self, sid: int) -> int:
        """Samples of stream ``sid`` at the codec's rate that wait for their encode."""
        b = self._buf[int(sid)]
        return 0 if b is None else int(b.shape[0])

    def frames(self, sid: int) -> int:
        """Frames of stream ``sid``'s running turn that are already encoded."""
        return sum(int(c.shape[1]) for c in self._codes[int(sid)])

    def feed(self, sid: int, samples: torch.Tensor) -> None:
        """(n,) fp32 @ 24 kHz, n >= 0: the microphone's next samples -- with a resampler: fp32 or int16 at the microphone's rate.
        Nothing is launched."""
        sid = int(sid)
        assert samples.dim() == 1, "samples must be (n,)"
        if self.resampler is not None:
            if samples.shape[0]:
                self._raw[sid].append(samples)
                self._fed[sid] = True
            return
        self._append(sid, samples)

    def _append(self, sid: int, samples: torch.Tensor) -> None:
        b = self._buf[sid]
        self._buf[sid] = samples if b is None else torch.cat([b, samples.to(b.device)])

    def _take(self, sid: int, n: int) -> torch.Tensor:
        b = self._buf[sid]
        self._buf[sid] = b[n:] if n < b.shape[0] else None
        return b[:n]

    def _raw_chunk(self, sid: int) -> torch.Tensor:
        """Stream ``sid``'s samples that wait for the resampler, as one chunk (int16 only if all of them are)."""
        raw, self._raw[sid] = self._raw[sid], []
        if len(raw) == 1:
            return raw[0]
        if not raw:
            return torch.empty(0, dtype=torch.float32)
        if any(r.dtype != torch.int16 for r in raw):
            raw = [r.float() / 32768.0 if r.dtype == torch.int16 else r.float() for r in raw]
        return torch.cat([r.to(raw[0].device) for r in raw])

    def pump(self) -> int:
        """With a resampler, first ONE resampler call for every stream that has new samples.  Then ONE pool call for every stream that holds
        at least one whole frame: each gives its whole frames, at most ``chunk_frames``; the remainder stays buffered.  Returns the number
        of frames encoded (0: no encode call)."""
        if self.resampler is not None:
            new = [s for s in sorted(self._raw) if self._raw[s]]
            if new:
                for s, y in zip(new, self.resampler.feed(new, [self._raw_chunk(s) for s in new], False)):
                    self._append(s, y)
        ids = [s for s in sorted(self._buf) if self.buffered(s) >= self.hop]
        if not ids:
            return 0
        wavs = [self._take(s, min(self.chunk_frames, self.buffered(s) // self.hop) * self.hop) for s in ids]
        total = 0
        for s, c in zip(ids, self.pool.encode(ids, wavs)):
            self._codes[s].append(c)
            total += int(c.shape[1])
        return total

    def finish(self, sid: int, speaker: int, text: Union[str, Sequence[int]]):
        """Ends stream ``sid``'s turn: with a resampler, ends the stream's clip there (its last samples and the filter's tail come out);
        then encodes what is buffered, the partial last frame included, in the fewest calls ``chunk_frames`` allows, resets the stream and
        returns ``Segment(speaker, text, audio=None, audio_codes=(32, T))`` of the whole turn."""
        from .generator import Segment
        sid = int(sid)
        if self.resampler is not None and self._fed[sid]:
            (y,) = self.resampler.feed([sid], [self._raw_chunk(sid)], True)
            self._append(sid, y)
            self._fed[sid] = False
        full = self.chunk_frames * self.hop
        while self.buffered(sid) > 0:
            (c,) = self.pool.encode([sid], [self._take(sid, min(full, self.buffered(sid)))])
            self._codes[sid].append(c)
        codes, self._codes[sid] = self._codes[sid], []
        if not codes:
            raise ValueError(f"stream {sid}: a turn without samples")
        self.pool.reset([sid])
        return Segment(speaker=speaker, text=text, audio=None, audio_codes=torch.cat(codes, dim=1))
