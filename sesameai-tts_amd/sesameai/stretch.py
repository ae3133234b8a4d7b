"""Speech rate on the device: a pool of stateful WSOLA time-stretch streams (include/mimi_hip.h, mimi_ts_pool_*).

The reference's web chat plays every sentence at 1.2 x (utils/web_base.py ``speed_factor``; utils/tts_base.py applies pydub's ``speedup``,
which drops a slice of every 150 ms and crossfades over the cut wherever it falls).  Here each 512-sample joint is placed where the
waveforms agree (a +-256-sample search on 12-bit samples, scored in exact integers), as ONE launch per call for up to 64 streams, with
state: a stream's chunks, concatenated, are bit for bit the one-shot result of its concatenated samples, so a live batch's audio can be
stretched chunk by chunk beside the frame loop.  All arithmetic is the library's; this file marshals."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Union

import torch

from ._stream_pool import StreamPool, _stream, fp32_unscaled, pack, shared_pool, split

MAX_STREAMS = 64                 # MIMI_TS_MAX_STREAMS
BLOCK = 512                      # H: samples per block, one d per block
PM_MIN, PM_MAX = 500, 2000

def speed_pm(speed: Union[None, float, int]) -> Optional[int]:
    """A speed factor as the integer permille the library takes; ``None`` for no stretch at all (``None`` or exactly 1.0)."""
    if speed is None:
        return None
    pm = int(round(float(speed) * 1000))
    if pm == 1000:
        return None
    if not PM_MIN <= pm <= PM_MAX:
        raise ValueError(f"speed must lie in 0.5 .. 2.0, got {speed!r}")
    return pm


def per_request(speed, n: int) -> List[Optional[float]]:
    """``speed=`` of an entry point -- None, one factor, or one factor or None per request -- as one checked factor or None per request."""
    if speed is None or isinstance(speed, (int, float)):
        speed = [speed] * n
    speed = list(speed)
    if len(speed) != n:
        raise ValueError(f"speed: one value, or one per request ({n})")
    pms = [speed_pm(s) for s in speed]
    return [None if pm is None else pm / 1000.0 for pm in pms]


class TimeStretchPool(StreamPool):
    """``n`` independent time-stretch streams.  ``reset(ids, speeds)`` starts the listed streams afresh at their speeds (host arithmetic, no
    launch); ``feed(ids, chunks, final)`` gives every listed stream its new fp32 samples and returns what each may emit now: ONE launch, no
    host-to-device copy of a plan, no synchronisation.  ``final`` ends a stream's clip: the tail comes out and the stream is fresh (at the
    same speed).  Streams start fresh at speed 1.0."""

    def __init__(self, n: int, device: Union[str, torch.device] = "cuda"):
        super().__init__("mimi_ts_pool", n, device, int(n))

    def out_count(self, sid: int, n_in: int, final: bool = False) -> int:
        """Samples a feed of ``n_in`` samples would give stream ``sid`` now (host arithmetic)."""
        return self._count("out_count", sid, n_in, final)

    def reset(self, ids: Sequence[int], speeds: Union[float, int, Sequence[Union[float, int]]]) -> None:
        """Start the listed streams afresh; ``speeds``: one factor for all, or one per id (0.5 .. 2.0; 1.0 is a legal stream speed)."""
        ids = [int(i) for i in ids]
        sp = [speeds] * len(ids) if isinstance(speeds, (int, float)) else list(speeds)
        assert len(sp) == len(ids), "one speed per id"
        pm = [int(round(float(s) * 1000)) for s in sp]
        m = max(len(ids), 1)
        self._check(self._lib.mimi_ts_pool_reset(self._h, (C.c_int32 * m)(*ids), (C.c_int32 * m)(*pm), len(ids)))

    @torch.inference_mode()
    def feed(self, ids: Sequence[int], chunks: Sequence[torch.Tensor], final: Union[bool, Sequence[bool]] = False, want_offsets: bool = False):
        """ids: n distinct stream ids; chunks[i]: (n_i,) fp32, n_i >= 0, CPU or device, the new samples of stream ids[i]; final: one flag, or
        one per stream -> one (m_i,) fp32 tensor per stream (views into one buffer), m_i >= 0.  want_offsets: also, per stream, the int32
        offsets d_k of its ceil(m_i / 512) emitted blocks (device; 0 for a clip's first block)."""
        p = pack(chunks, self.device, fp32_unscaled, ids, final)
        counts = self._counts("out_count", p)
        out = torch.empty(max(sum(counts), 1), dtype=torch.float32, device=self.device)
        d = torch.empty(max(sum(-(-c // BLOCK) for c in counts), 1), dtype=torch.int32, device=self.device) if want_offsets else None
        n_out = (C.c_long * p.m)()
        self._check(self._lib.mimi_ts_pool_feed(self._h, *p.head, out.data_ptr(), n_out, d.data_ptr() if want_offsets else None, _stream()))
        got = [int(x) for x in n_out[:len(p.ids)]]
        if not want_offsets:
            return split(out, got)
        return split(out, got), split(d, [-(-g // BLOCK) for g in got])


_POOLS: Dict[str, TimeStretchPool] = {}       # stretch()'s pools, made on first use and kept


@torch.inference_mode()
def stretch(wavs: Sequence[torch.Tensor], speed: Union[float, int, Sequence[Union[float, int]]], device: Union[str, torch.device, None] = None,
            want_offsets: bool = False):
    """Up to 64 clips of different lengths, each (n_i,) fp32, at ``speed`` (one factor, or one per clip; 0.5 .. 2.0) -> each
    (ceil(n_i / speed_i),) fp32, in ONE launch on fresh streams with ``final``."""
    if not 1 <= len(wavs) <= MAX_STREAMS:
        raise ValueError(f"stretch takes 1 .. {MAX_STREAMS} clips a call")
    pool = shared_pool(_POOLS, device, wavs[0], str, lambda dev: TimeStretchPool(MAX_STREAMS, device=dev))
    ids = list(range(len(wavs)))
    pool.reset(ids, speed)             # (host arithmetic: also covers a stream that an earlier call, interrupted, left open)
    return pool.feed(ids, wavs, final=True, want_offsets=want_offsets)
