"""The user's spoken turns of several conversations, encoded WHILE they are spoken (the reference's voice chat puts the user's turn into the
context as ``Segment(text=user_msg, speaker=1, audio=user_aud)``, ogwebapp.py:76-125, and can only encode it after the turn has ended).

``TurnStreams`` sits on a pool of stateful Mimi encode streams (``MimiCodec.open_encode_streams``): ``feed`` buffers a microphone's new
samples, ``pump`` encodes every stream's whole frames in ONE pool call, and ``finish`` encodes what is left of a turn -- the partial last
frame included -- and hands back a ``Segment`` with ``audio_codes``: bit for bit the codes ``MimiCodec.encode`` gives the whole turn.  When
the turn ends, all of it but the last call's frames is already on the device.  Host logic only; the arithmetic is the pool's."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Union

import torch


class TurnStreams:
    def __init__(self, pool, hop: int, chunk_frames: int = 10):
        """pool: anything with ``n_streams``, ``encode(ids, wavs) -> [(32, T_i)]`` and ``reset(ids)`` (``MimiEncodeStreamPool``);
        chunk_frames: the most frames one stream gives one call (at most the pool's ``max_chunk_frames``)."""
        assert chunk_frames >= 1 and hop >= 1
        self.pool, self.hop, self.chunk_frames = pool, int(hop), int(chunk_frames)
        self._buf: Dict[int, Optional[torch.Tensor]] = {s: None for s in range(pool.n_streams)}     # samples not yet encoded
        self._codes: Dict[int, List[torch.Tensor]] = {s: [] for s in range(pool.n_streams)}         # the turn's codes so far

    def buffered(self, sid: int) -> int:
        """Samples of stream ``sid`` that wait for their encode."""
        b = self._buf[int(sid)]
        return 0 if b is None else int(b.shape[0])

    def frames(self, sid: int) -> int:
        """Frames of stream ``sid``'s running turn that are already encoded."""
        return sum(int(c.shape[1]) for c in self._codes[int(sid)])

    def feed(self, sid: int, samples: torch.Tensor) -> None:
        """(n,) fp32 @ 24 kHz, n >= 0: the microphone's next samples.  Nothing is launched."""
        sid = int(sid)
        assert samples.dim() == 1, "samples must be (n,)"
        b = self._buf[sid]
        self._buf[sid] = samples if b is None else torch.cat([b, samples.to(b.device)])

    def _take(self, sid: int, n: int) -> torch.Tensor:
        b = self._buf[sid]
        self._buf[sid] = b[n:] if n < b.shape[0] else None
        return b[:n]

    def pump(self) -> int:
        """ONE pool call for every stream that holds at least one whole frame: each gives its whole frames, at most ``chunk_frames``;
        the remainder stays buffered.  Returns the number of frames encoded (0: no call)."""
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
        """Ends stream ``sid``'s turn: encodes what is buffered, the partial last frame included, in the fewest calls ``chunk_frames``
        allows, resets the stream and returns ``Segment(speaker, text, audio=None, audio_codes=(32, T))`` of the whole turn."""
        from .generator import Segment
        sid = int(sid)
        full = self.chunk_frames * self.hop
        while self.buffered(sid) > 0:
            (c,) = self.pool.encode([sid], [self._take(sid, min(full, self.buffered(sid)))])
            self._codes[sid].append(c)
        codes, self._codes[sid] = self._codes[sid], []
        if not codes:
            raise ValueError(f"stream {sid}: a turn without samples")
        self.pool.reset([sid])
        return Segment(speaker=speaker, text=text, audio=None, audio_codes=torch.cat(codes, dim=1))
