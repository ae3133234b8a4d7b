"""Finished segments on the device (include/mimi_hip.h, mimi_fin_*): decoded fp32 clips -> the int16 segments a WAV holds.

The reference finishes every sentence on the host with pydub (peak-normalise -> int16, lead and tail silence, fade in and out,
tts_service.py:288-306); ``tts_service.TTS.generate_audio_segment`` does the same with a float32 copy to the host and five NumPy passes per
clip.  Here all the clips that are ready together go through ONE launch chain (two kernels) and leave the device as int16, bit for bit the
same samples.  All arithmetic is the library's; this file marshals."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Sequence, Union

import torch

from . import _abi
from ._abi import lib

MAX_SEGMENTS = 64                # MIMI_FIN_MAX_SEGMENTS


@dataclass(frozen=True)
class SegmentFinish:
    """How a clip becomes a segment; the defaults are the reference's (tts_service.py:260-262).  Milliseconds become samples as
    ``sample_rate * ms // 1000``."""
    lead_ms: int = 500
    tail_ms: int = 100
    fade_ms: int = 50

    def samples(self, sample_rate: int):
        if min(self.lead_ms, self.tail_ms, self.fade_ms) < 0:
            raise ValueError("lead_ms, tail_ms and fade_ms must be >= 0")
        return tuple(int(sample_rate) * int(ms) // 1000 for ms in (self.lead_ms, self.tail_ms, self.fade_ms))


def per_clip(finish: Union[SegmentFinish, Sequence[SegmentFinish]], n: int) -> List[SegmentFinish]:
    """One ``SegmentFinish`` for all n clips, or one per clip -> one per clip."""
    if isinstance(finish, SegmentFinish):
        return [finish] * n
    finish = list(finish)
    if len(finish) != n or not all(isinstance(f, SegmentFinish) for f in finish):
        raise ValueError(f"finish: one SegmentFinish, or one per clip ({n})")
    return finish


class SegmentFinisher:
    """``finish(clips, finish)``: every clip (n_i,) fp32, n_i >= 0 -> its segment (lead + n_i + tail,) int16 on the device, views of one packed
    buffer.  Up to 64 clips are one library call (two launches on the current torch stream, no synchronisation); more run in several."""

    def __init__(self, device: Union[str, torch.device] = "cuda"):
        self.device = torch.device(device)
        self._h = C.c_void_p(None)
        with torch.cuda.device(self.device):
            rc = lib.mimi_fin_create(C.byref(self._h))
        if rc != 0:
            raise _abi.CsmError(rc, (lib.mimi_fin_last_error(None) or b"").decode())

    def _check(self, rc: int) -> None:
        if rc != 0:
            raise _abi.CsmError(rc, (lib.mimi_fin_last_error(self._h) or b"").decode())

    @torch.inference_mode()
    def finish(self, clips: Sequence[torch.Tensor], finish: Union[SegmentFinish, Sequence[SegmentFinish]] = SegmentFinish(),
               sample_rate: int = 24000) -> List[torch.Tensor]:
        n = len(clips)
        params = [f.samples(sample_rate) for f in per_clip(finish, n)]
        if n == 0:
            return []
        # (kept alive until the launches are made; the stream orders their release behind the kernels)
        parts = [c.reshape(-1).to(device=self.device, dtype=torch.float32).contiguous() for c in clips]
        counts = [int(lib.mimi_fin_out_count(int(c.shape[0]), L, T)) for c, (L, T, _) in zip(parts, params)]
        if min(counts) < 0:
            raise ValueError("a segment of more than 2^30 samples")
        out = torch.empty(max(sum(counts), 1), dtype=torch.int16, device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        res: List[torch.Tensor] = []
        base = 0
        for lo in range(0, n, MAX_SEGMENTS):
            sub, par = parts[lo:lo + MAX_SEGMENTS], params[lo:lo + MAX_SEGMENTS]
            m = len(sub)
            ptrs = (C.c_void_p * m)(*[c.data_ptr() if c.shape[0] else None for c in sub])
            off, n_out = (C.c_long * m)(), (C.c_long * m)()
            with torch.cuda.device(self.device):
                self._check(lib.mimi_fin_segments(self._h, ptrs, (C.c_long * m)(*[int(c.shape[0]) for c in sub]),
                                                  (C.c_int32 * m)(*[p[0] for p in par]), (C.c_int32 * m)(*[p[1] for p in par]),
                                                  (C.c_int32 * m)(*[p[2] for p in par]), m, out.data_ptr() + 2 * base, off, n_out, stream))
            res.extend(out[base + off[k]:base + off[k] + n_out[k]] for k in range(m))
            base += sum(n_out[:m])
        return res

    def __del__(self):
        try:
            if self._h:
                lib.mimi_fin_destroy(self._h)
        except Exception:
            pass
