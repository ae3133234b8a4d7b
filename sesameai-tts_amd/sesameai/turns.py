"""The user's spoken turns of several conversations, encoded WHILE they are spoken (the reference's voice chat puts the user's turn into the
context as ``Segment(text=user_msg, speaker=1, audio=user_aud)``, ogwebapp.py:76-125, and can only encode it after the turn has ended).

``TurnStreams`` sits on a pool of stateful Mimi encode streams (``MimiCodec.open_encode_streams``): ``feed`` buffers a microphone's new
samples, ``pump`` encodes every stream's whole frames in ONE pool call, and ``finish`` encodes what is left of a turn -- the partial last
frame included -- and hands back a ``Segment`` with ``audio_codes``: bit for bit the codes ``MimiCodec.encode`` gives the whole turn.  When
the turn ends, all of it but the last call's frames is already on the device.  With a ``resampler`` (a ``ResamplerPool`` from the
microphones' rate to the codec's, sesameai/resample.py) the samples come at the microphones' rate, fp32 or int16: the codes are then those
of ``encode(resample(the whole turn))``.  With a ``vad`` (a ``VadPool``, sesameai/vad.py) the streams listen all the time and the
detector says where a turn starts and ends; ``ReplyOnPause`` turns its events into calls.  With ``features`` (a ``TurnFeatures``,
sesameai/mel.py) the turn's speech-to-text input -- Whisper's log-mel features of exactly the samples the segment's codes encode -- is
computed while the turn is spoken too, and ``take_features`` has it when the turn ends.  Host logic only; the arithmetic is the pools'."""
from __future__ import annotations

from collections import deque
from typing import Callable, Deque, Dict, List, Optional, Sequence, Tuple, Union

import torch


class TurnStreams:
    VAD_FRAME = 240                  # the detector's frame at 24 kHz: events are stamped in frames

    def __init__(self, pool, hop: int, chunk_frames: int = 10, resampler=None, vad=None, pre_roll: int = 4800, post_roll: int = 4800,
                 features=None):
        """pool: anything with ``n_streams``, ``encode(ids, wavs) -> [(32, T_i)]`` and ``reset(ids)`` (``MimiEncodeStreamPool``);
        chunk_frames: the most frames one stream gives one call (at most the pool's ``max_chunk_frames``);
        resampler: None (samples come at 24 kHz: today's calls exactly), or anything with ``feed(ids, chunks, final) -> [(m_i,)]`` and
        ``reset(ids)`` over at least ``pool.n_streams`` streams (``ResamplerPool``);
        vad: None (a turn is what lies between two ``finish`` calls: today's calls exactly), or anything with ``feed(ids, chunks, final)
        -> [frames with .flags and .first]``, ``events(frames, params, in_speech) -> [("start" | "end", frame)]`` and ``params[sid]`` with
        ``min_on`` and ``hang`` over at least ``pool.n_streams`` streams (``VadPool``).  ``pump`` then makes ONE ``vad.feed`` call over the
        streams that received samples at the codec's rate -- the very samples that go to the encoder, behind the resampler -- in front of
        the encode call, and the turn is gated: in silence nothing is encoded and only the last ``pre_roll`` samples (plus the ``min_on -
        1`` frames a START reaches back, plus the unjudged ones) are kept; at START the turn begins at ``a = max(previous cut,
        start_frame * 240 - pre_roll)`` and is encoded as it comes; at END its audio ends at ``end = end_frame * 240 + post_roll`` (never
        past what has been received), the codes of frames past ``T = ceil((end - a) / hop)`` are dropped -- the encoder is causal, so the
        segment is bit for bit ``encode(samples[a : a + T * hop])`` -- and the stream goes on listening.  ``poll_events`` hands out
        ``(sid, "start" | "end", sample)``; after an "end", ``finish`` returns that turn's segment.
        features: None (today's calls exactly), or anything with ``feed(ids, chunks, final)``, ``reset(ids)`` and ``take(sid) ->
        (features, n_frames)`` over at least ``pool.n_streams`` streams that takes samples at the codec's rate (``TurnFeatures``).  Without
        a vad every sample range handed to ``pool.encode`` is handed to ``features.feed`` too, one call per pump over the same ids, and
        the turn's last range goes with ``final``.  With a vad the codes of an ended turn are cut where the detector says, up to ``hang``
        frames behind what was already encoded, and features cannot be cut afterwards: so ``features.feed`` follows the encoder only up to
        where a coming END may still cut (one call per pump), and the rest, up to the last sample the segment's codes encode, goes with
        ``final`` when the turn is closed.  Either way the features are those of EXACTLY the samples ``[a, b)`` that the codes encode."""
        assert chunk_frames >= 1 and hop >= 1
        self.pool, self.hop, self.chunk_frames, self.resampler = pool, int(hop), int(chunk_frames), resampler
        self._buf: Dict[int, Optional[torch.Tensor]] = {s: None for s in range(pool.n_streams)}     # samples not yet encoded
        self._codes: Dict[int, List[torch.Tensor]] = {s: [] for s in range(pool.n_streams)}         # the turn's codes so far
        self._raw: Dict[int, List[torch.Tensor]] = {s: [] for s in range(pool.n_streams)}           # (resampler) samples not yet resampled
        self._fed: Dict[int, bool] = {s: False for s in range(pool.n_streams)}                      # (resampler) the turn has had samples
        self.vad, self.pre_roll, self.post_roll = vad, int(pre_roll), int(post_roll)
        self.features = features
        self._fsent: Dict[int, int] = {s: 0 for s in range(pool.n_streams)}       # (features, vad) the next sample of the turn they lack
        if vad is not None:
            assert pre_roll >= 0 and post_roll >= 0
            ids = range(pool.n_streams)
            self._new: Dict[int, List[torch.Tensor]] = {s: [] for s in ids}       # samples at the codec's rate that no pump has seen
            self._hist: Dict[int, Optional[torch.Tensor]] = {s: None for s in ids}      # the samples from _h0 on that may still be needed
            self._h0: Dict[int, int] = {s: 0 for s in ids}
            self._recv: Dict[int, int] = {s: 0 for s in ids}                      # samples received since the stream opened
            self._judged: Dict[int, int] = {s: 0 for s in ids}                    # frames the detector has judged
            self._speech: Dict[int, bool] = {s: False for s in ids}               # the detector's state
            self._cut: Dict[int, int] = {s: 0 for s in ids}                       # where the last turn's audio ended
            self._turn: Dict[int, Optional[List[int]]] = {s: None for s in ids}   # the running turn: [a, next sample to encode]
            self._ready: Dict[int, Deque[torch.Tensor]] = {s: deque() for s in ids}     # ended turns' codes that wait for finish
            self._events: List[Tuple[int, str, int]] = []

    def buffered(self, sid: int) -> int:
        """Samples of stream ``sid`` at the codec's rate that wait for their encode."""
        if self.vad is not None:
            t = self._turn[int(sid)]
            return 0 if t is None else self._recv[int(sid)] - t[1]
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
        if self.vad is not None:
            if samples.shape[0]:
                self._new[sid].append(samples)
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
        of frames encoded (0: no encode call).  With a vad: see the class."""
        if self.vad is not None:
            return self._pump_vad()
        if self.resampler is not None:
            new = [s for s in sorted(self._raw) if self._raw[s]]
            if new:
                for s, y in zip(new, self.resampler.feed(new, [self._raw_chunk(s) for s in new], False)):
                    self._append(s, y)
        ids = [s for s in sorted(self._buf) if self.buffered(s) >= self.hop]
        if not ids:
            return 0
        wavs = [self._take(s, min(self.chunk_frames, self.buffered(s) // self.hop) * self.hop) for s in ids]
        if self.features is not None:
            self.features.feed(ids, wavs, False)
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
        if self.vad is not None:
            if not self._ready[sid]:
                if self._turn[sid] is None:
                    raise ValueError(f"stream {sid}: a turn without samples")
                self._close(sid, self._recv[sid])                        # no END yet: the caller ends the turn where the samples end
            return Segment(speaker=speaker, text=text, audio=None, audio_codes=self._ready[sid].popleft())
        if self.resampler is not None and self._fed[sid]:
            (y,) = self.resampler.feed([sid], [self._raw_chunk(sid)], True)
            self._append(sid, y)
            self._fed[sid] = False
        full = self.chunk_frames * self.hop
        ended = False                                                    # (features) the turn's last range has gone with final
        while self.buffered(sid) > 0:
            wav = self._take(sid, min(full, self.buffered(sid)))
            (c,) = self.pool.encode([sid], [wav])
            self._codes[sid].append(c)
            if self.features is not None:
                ended = self.buffered(sid) == 0
                self.features.feed([sid], [wav], ended)
        codes, self._codes[sid] = self._codes[sid], []
        if not codes:
            raise ValueError(f"stream {sid}: a turn without samples")
        if self.features is not None and not ended:                      # every sample was encoded by a pump: an empty last range
            self.features.feed([sid], [torch.empty(0, dtype=torch.float32)], True)
        self.pool.reset([sid])
        return Segment(speaker=speaker, text=text, audio=None, audio_codes=torch.cat(codes, dim=1))

    def take_features(self, sid: int):
        """The oldest ended turn of stream ``sid`` whose features have not been taken: ``(features (n_mels, 3000), n_frames)``."""
        assert self.features is not None, "TurnStreams without features"
        return self.features.take(int(sid))

    # -- with a voice-activity detector ---------------------------------------------------------------
    def poll_events(self) -> List[Tuple[int, str, int]]:
        """The events since the last poll, in order: ``(sid, "start", a)`` -- a turn runs from sample ``a`` of the stream on -- and
        ``(sid, "end", end)`` -- it ended at sample ``end`` and ``finish(sid, ..)`` has its segment.  Samples count at the codec's rate
        from the stream's first sample."""
        ev, self._events = self._events, []
        return ev

    def _samples(self, sid: int, lo: int, hi: int) -> torch.Tensor:
        return self._hist[sid][lo - self._h0[sid]:hi - self._h0[sid]]

    def _close(self, sid: int, end: int) -> None:
        """Ends the running turn at sample ``end``: encodes what its T frames still lack (the stream alone, in the fewest calls), drops the
        codes past them, resets the encode stream."""
        a, sent = self._turn[sid]
        end = min(max(end, a + 1), self._recv[sid])
        T = -(-(end - a) // self.hop)
        b = min(a + T * self.hop, self._recv[sid])
        while self.frames(sid) < T:
            n = min(self.chunk_frames * self.hop, b - sent)
            (c,) = self.pool.encode([sid], [self._samples(sid, sent, sent + n)])
            self._codes[sid].append(c)
            sent += n
        codes, self._codes[sid] = self._codes[sid], []
        self.pool.reset([sid])
        if self.features is not None:                                    # what the turn's features lack of [a, b), and the end of the clip
            self.features.feed([sid], [self._samples(sid, self._fsent[sid], b)], True)
        self._ready[sid].append(torch.cat(codes, dim=1)[:, :T])
        self._turn[sid], self._cut[sid] = None, end
        self._events.append((sid, "end", end))

    def _pump_vad(self) -> int:
        F = self.VAD_FRAME
        got: Dict[int, torch.Tensor] = {}
        if self.resampler is not None:
            new = [s for s in sorted(self._raw) if self._raw[s]]
            if new:
                got = dict(zip(new, self.resampler.feed(new, [self._raw_chunk(s) for s in new], False)))
        else:
            for s in sorted(self._new):
                if self._new[s]:
                    parts, self._new[s] = self._new[s], []
                    got[s] = parts[0] if len(parts) == 1 else torch.cat([p.to(parts[0].device) for p in parts])
        ids = [s for s in sorted(got) if got[s].shape[0]]
        if ids:
            for s, y, fr in zip(ids, [got[s] for s in ids], self.vad.feed(ids, [got[s] for s in ids], False)):
                h = self._hist[s]
                self._hist[s] = y if h is None else torch.cat([h, y.to(h.device)])
                self._recv[s] += int(y.shape[0])
                prm = self.vad.params[s]
                for kind, f in self.vad.events(fr, prm, self._speech[s]):
                    self._speech[s] = kind == "start"
                    if kind == "start" and self._turn[s] is None:
                        a = max(self._cut[s], f * F - self.pre_roll, self._h0[s], 0)
                        self._turn[s] = [a, a]
                        self._fsent[s] = a
                        self._events.append((s, "start", a))
                    elif kind == "end" and self._turn[s] is not None:        # (None: finish has ended the turn by hand)
                        self._close(s, f * F + self.post_roll)
                self._judged[s] = int(fr.first) + int(fr.flags.shape[0])
                # what may still be needed: a turn's samples not yet encoded and, from where a coming END may cut, the next turn's
                # pre-roll; in silence, from where a coming START may reach back to
                t = self._turn[s]
                if t is not None:
                    keep = min(t[1], max((self._judged[s] - prm.hang + 1) * F + self.post_roll, 0))
                    if self.features is not None:
                        keep = min(keep, self._fsent[s])
                else:
                    keep = max(self._cut[s], (self._judged[s] - prm.min_on + 1) * F - self.pre_roll, 0)
                keep = min(max(keep, self._h0[s]), self._recv[s])
                self._hist[s], self._h0[s] = self._hist[s][keep - self._h0[s]:], keep
        ids = [s for s in sorted(self._turn) if self._turn[s] is not None and self.buffered(s) >= self.hop]
        if not ids:
            return 0
        if self.features is not None:
            self._feed_features_vad(ids)
        wavs = []
        for s in ids:
            t = self._turn[s]
            n = min(self.chunk_frames, self.buffered(s) // self.hop) * self.hop
            wavs.append(self._samples(s, t[1], t[1] + n))
            t[1] += n
        total = 0
        for s, c in zip(ids, self.pool.encode(ids, wavs)):
            self._codes[s].append(c)
            total += int(c.shape[1])
        return total


    def _feed_features_vad(self, ids: List[int]) -> None:
        """ONE ``features.feed`` over the streams about to be encoded: each turn's samples up to where this pump's encode call will stand,
        but no further than a coming END may still cut -- END frame f >= judged - hang + 1 ends the audio at f * 240 + post_roll."""
        F, fids, chunks = self.VAD_FRAME, [], []
        for s in ids:
            t = self._turn[s]
            upto = t[1] + min(self.chunk_frames, self.buffered(s) // self.hop) * self.hop
            safe = min(upto, max((self._judged[s] - self.vad.params[s].hang + 1) * F + self.post_roll, 0))
            if safe > self._fsent[s]:
                fids.append(s)
                chunks.append(self._samples(s, self._fsent[s], safe))
                self._fsent[s] = safe
        if fids:
            self.features.feed(fids, chunks, False)


class ReplyOnPause:
    """The reference's ``ReplyOnPause(respond, can_interrupt=True)`` over a ``TurnStreams`` with a vad: ``receive(sid, samples)`` feeds a
    microphone and pumps; at every END ``respond(sid, segment)`` is called, where ``segment(speaker, text)`` gives the turn's ``Segment``
    (``TurnStreams.finish``), and the stream's reply counts as in flight until ``reply_done(sid)``; a START that arrives meanwhile calls
    ``on_interrupt(sid)`` once (barge-in) and ends the flight.  With ``stt`` (a callable ``(features, n_frames) -> str``, such as
    ``sesameai.stt.WhisperSTT``, over ``TurnStreams(features=)``) an END calls ``respond(sid, segment, text)`` with the transcribed
    text, and ``segment(speaker, text=None)`` puts it into the ``Segment`` unless another is given.  Host logic only."""

    def __init__(self, turns: TurnStreams, respond: Callable, on_interrupt: Optional[Callable] = None, stt: Optional[Callable] = None):
        assert turns.vad is not None, "ReplyOnPause needs TurnStreams with a vad"
        assert stt is None or turns.features is not None, "stt needs TurnStreams with features"
        self.turns, self.respond, self.on_interrupt, self.stt = turns, respond, on_interrupt, stt
        self.in_flight: Dict[int, bool] = {}

    def reply_done(self, sid: int) -> None:
        """The reply to stream ``sid`` has been played to its end: a START from now on interrupts nothing."""
        self.in_flight[int(sid)] = False

    def receive(self, sid: int, samples: torch.Tensor) -> int:
        """-> the number of events handled"""
        self.turns.feed(sid, samples)
        self.turns.pump()
        events = self.turns.poll_events()
        for s, kind, _ in events:
            if kind == "start":
                if self.in_flight.get(s) and self.on_interrupt is not None:
                    self.on_interrupt(s)
                self.in_flight[s] = False
            else:
                self.in_flight[s] = True
                if self.stt is None:
                    self.respond(s, lambda speaker, text, s=s: self.turns.finish(s, speaker, text))
                else:
                    said = self.stt(*self.turns.take_features(s))
                    self.respond(s, lambda speaker, text=None, s=s, said=said: self.turns.finish(s, speaker, said if text is None else text), said)
        return len(events)
