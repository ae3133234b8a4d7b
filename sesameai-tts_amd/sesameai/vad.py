"""Voice activity on the device: a pool of stateful streams that say when a speaker starts and when they have stopped
(include/mimi_hip.h, mimi_vad_pool_*).

The reference's voice chat hands a turn to the model when fastrtc's ``ReplyOnPause`` hears a pause (ogwebapp.py:169), with a downloaded
neural detector.  Here the decision is a rule in exact integers per 10 ms frame -- a DC-free power against a slow noise floor with
hysteresis, and a first-crossing autocorrelation lag that tells a voice from noise, clicks and bursts -- for up to 64 microphones with two
launches per call, with state: a stream's frames, concatenated over any chunk schedule, are bit for bit the one-shot result.  All
arithmetic is the library's; this file marshals, and ``events`` reads the per-frame flags on the host."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

import torch

from ._stream_pool import StreamPool, _stream, int16_if_all, pack, shared_pool, split

MAX_STREAMS = 64                 # MIMI_VAD_MAX_STREAMS
FRAME = 240                      # F: samples per frame at 24 kHz
SAMPLE_RATE = 24000
SUMMARY = 8                      # MIMI_VAD_SUMMARY


class VadParams(NamedTuple):
    """Per-stream parameters (set by ``reset``).  on_q4 / off_q4: how far above the noise floor a frame's power must lie to count as loud
    in silence / in speech, in sixteenths (128 = x 8); min_on: active frames that start a turn; hang: quiet frames that end it; hold:
    frames a loud stretch stays active after its last voiced frame; n_min: the floor's floor."""
    on_q4: int = 128
    off_q4: int = 48
    min_on: int = 8
    hang: int = 70
    hold: int = 30
    n_min: int = 3686400


class _CParams(C.Structure):      # mimi_vad_params
    _fields_ = [("on_q4", C.c_int32), ("off_q4", C.c_int32), ("min_on", C.c_int32), ("hang", C.c_int32), ("hold", C.c_int32),
                ("reserved", C.c_int32), ("n_min", C.c_int64)]


class VadFrames(NamedTuple):
    """One stream's frames of one call: (K,) uint8 / int16 / int64 / int64 on the device, and the index of the first of them."""
    flags: torch.Tensor
    lag: torch.Tensor
    power: torch.Tensor
    floor: torch.Tensor
    first: int


class VadSummary(NamedTuple):
    in_speech: bool
    frames: int
    last_start: int
    last_end: int
    quiet: int
    starts: int
    ends: int


def events(frames: Union[VadFrames, Sequence[int], torch.Tensor], params: VadParams = VadParams(), in_speech: bool = False,
           first: Optional[int] = None) -> List[Tuple[str, int]]:
    """The events in a run of per-frame flags, on the host: [("start" | "end", frame)].  Bit 3 is the state after the frame; a START is
    stamped ``min_on - 1`` frames before the frame that turns the state to speech, an END ``hang - 1`` frames before the one that turns it
    back.  in_speech: the state in front of the run; first: its first frame's index (a ``VadFrames`` carries its own)."""
    if isinstance(frames, VadFrames):
        first = frames.first if first is None else first
        frames = frames.flags
    if isinstance(frames, torch.Tensor):
        frames = frames.cpu().tolist()
    first = 0 if first is None else int(first)
    out, was = [], bool(in_speech)
    for i, f in enumerate(frames):
        now = bool(f & 8)
        if now != was:
            out.append(("start", first + i - params.min_on + 1) if now else ("end", first + i - params.hang + 1))
        was = now
    return out


class VadPool(StreamPool):
    """``n`` independent voice-activity streams.  ``reset(ids, params)`` starts the listed streams afresh with their parameters (host
    arithmetic, no launch); ``feed(ids, chunks, final)`` gives every listed stream its new samples at 24 kHz, fp32 or int16, and returns
    the frames each completed: at most two launches, no host-to-device copy of a plan, no synchronisation.  ``final`` ends a stream's clip:
    a partial frame is discarded and the stream is fresh (same parameters).  ``poll()`` reads every stream's summary (one small copy, the
    call's only synchronisation)."""

    def __init__(self, n: int, device: Union[str, torch.device] = "cuda"):
        super().__init__("mimi_vad_pool", n, device, int(n))
        self.params: Dict[int, VadParams] = {s: VadParams() for s in range(self.n_streams)}
        self._k: Dict[int, int] = {s: 0 for s in range(self.n_streams)}          # frames judged since the stream was fresh
        self._summary = torch.zeros(self.n_streams * SUMMARY, dtype=torch.int64, device=self.device)

    events = staticmethod(events)

    def frame_count(self, sid: int, n_in: int, final: bool = False) -> int:
        """Frames a feed of ``n_in`` samples would complete for stream ``sid`` now (host arithmetic)."""
        return self._count("frame_count", sid, n_in, final)

    def reset(self, ids: Sequence[int], params: Union[None, VadParams, Sequence[VadParams]] = None) -> None:
        """Start the listed streams afresh; ``params``: None (the defaults), one set for all, or one per id."""
        ids = [int(i) for i in ids]
        ps = [params or VadParams()] * len(ids) if params is None or isinstance(params, VadParams) else [VadParams(*p) for p in params]
        assert len(ps) == len(ids), "one parameter set per id"
        m = max(len(ids), 1)
        arr = (_CParams * m)(*[_CParams(p.on_q4, p.off_q4, p.min_on, p.hang, p.hold, 0, p.n_min) for p in ps])
        self._check(self._lib.mimi_vad_pool_reset(self._h, (C.c_int32 * m)(*ids), arr, len(ids)))
        for i, p in zip(ids, ps):
            self.params[i], self._k[i] = p, 0

    @torch.inference_mode()
    def feed(self, ids: Sequence[int], chunks: Sequence[torch.Tensor], final: Union[bool, Sequence[bool]] = False) -> List[VadFrames]:
        """ids: n distinct stream ids; chunks[i]: (n_i,) fp32 or int16 at 24 kHz, n_i >= 0, CPU or device, the new samples of stream
        ids[i] (int16 only if every chunk is); final: one flag, or one per stream -> one ``VadFrames`` per stream (views into four
        buffers), K_i >= 0 frames each."""
        p = pack(chunks, self.device, int16_if_all, ids, final)
        K = max(sum(self._counts("frame_count", p)), 1)
        flags = torch.empty(K, dtype=torch.uint8, device=self.device)
        lag = torch.empty(K, dtype=torch.int16, device=self.device)
        power = torch.empty(K, dtype=torch.int64, device=self.device)
        floor = torch.empty(K, dtype=torch.int64, device=self.device)
        n_frames = (C.c_long * p.m)()
        self._check(self._lib.mimi_vad_pool_feed(self._h, *p.head, int(p.dtype == torch.int16), flags.data_ptr(), lag.data_ptr(),
                                                 power.data_ptr(), floor.data_ptr(), n_frames, _stream()))
        got = [int(x) for x in n_frames[:len(p.ids)]]
        cols = [split(t, got) for t in (flags, lag, power, floor)]
        out = []
        for j, (i, g, f) in enumerate(zip(p.ids, got, p.fin)):
            out.append(VadFrames(cols[0][j], cols[1][j], cols[2][j], cols[3][j], self._k[i]))
            self._k[i] = 0 if f else self._k[i] + g
        return out

    @torch.inference_mode()
    def poll(self) -> List[VadSummary]:
        """Every stream's summary as of its last call (counts since the stream was last fresh)."""
        self._check(self._lib.mimi_vad_pool_summary(self._h, self._summary.data_ptr(), _stream()))
        rows = self._summary.view(self.n_streams, SUMMARY).cpu().tolist()
        return [VadSummary(bool(r[0]), *r[1:7]) for r in rows]


_POOLS: Dict[str, VadPool] = {}       # detect()'s pools, made on first use and kept


@torch.inference_mode()
def detect(wavs: Sequence[torch.Tensor], params: Union[None, VadParams, Sequence[VadParams]] = None,
           device: Union[str, torch.device, None] = None, want_summary: bool = False):
    """Up to 64 clips of different lengths, each (n_i,) fp32 or int16 at 24 kHz -> one ``VadFrames`` per clip (n_i // 240 frames), on
    fresh streams with ``final``.  want_summary: also every clip's ``VadSummary``."""
    if not 1 <= len(wavs) <= MAX_STREAMS:
        raise ValueError(f"detect takes 1 .. {MAX_STREAMS} clips a call")
    pool = shared_pool(_POOLS, device, wavs[0], str, lambda dev: VadPool(MAX_STREAMS, device=dev))
    ids = list(range(len(wavs)))
    pool.reset(ids, params)            # (host arithmetic: also covers a stream that an earlier call, interrupted, left open)
    frames = pool.feed(ids, wavs, final=True)
    return (frames, pool.poll()[:len(wavs)]) if want_summary else frames
