"""Finished segments on the device (include/mimi_hip.h, mimi_fin_*): decoded fp32 clips -> the int16 segments a WAV holds.

The reference finishes every sentence on the host with pydub (peak-normalise -> int16, lead and tail silence, fade in and out,
tts_service.py:288-306); ``tts_service.TTS.generate_audio_segment`` does the same with a float32 copy to the host and five NumPy passes per
clip.  Here all the clips that are ready together go through ONE launch chain (two kernels) and leave the device as int16, bit for bit the
same samples.  All arithmetic is the library's; this file marshals."""
from __future__ import annotations

import ctypes as C
import itertools
from dataclasses import dataclass
from typing import List, Optional, Sequence, Union

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
    loudness: Optional[float] = None     # LUFS: the clip is brought to this integrated loudness (BS.1770) instead of to its own peak
    ceiling_db: float = -1.0             # ... but no sample above this, dB relative to full scale (only read with ``loudness``)
    true_peak: bool = False              # ... the ceiling holds for the 4x oversampled waveform, dBTP (only read with ``loudness``)

    def samples(self, sample_rate: int):
        if min(self.lead_ms, self.tail_ms, self.fade_ms) < 0:
            raise ValueError("lead_ms, tail_ms and fade_ms must be >= 0")
        return tuple(int(sample_rate) * int(ms) // 1000 for ms in (self.lead_ms, self.tail_ms, self.fade_ms))

    def level(self):
        """(P_T, C) of mimi_fin_segments_ld; P_T == 0: the peak rule"""
        if self.loudness is None:
            return 0, 32767
        from .loudness import ceiling_i16, target_ms
        return target_ms(self.loudness), ceiling_i16(self.ceiling_db)


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
    buffer.  Up to 64 clips are one library call (two launches on the current torch stream, no synchronisation); more run in several.
    Where a clip's ``SegmentFinish`` names a ``loudness``, the call's clips are metered first (sesameai/loudness.py, three more launches)
    and the call is mimi_fin_segments_ld; where none does, the calls are exactly those made without the keyword.  Where such a clip also
    asks for ``true_peak``, the buffer the clips were packed into for the loudness meter also goes through mimi_tp_measure
    (sesameai/truepeak.py: a memset of 32 bytes a clip and one launch), and one small device copy per run of clips that ask puts their
    true peaks in the place of the sample peaks in the meter rows: one gain per clip is linear, so the finished clip's true peak is the
    input's times the gain.  No synchronisation."""

    def __init__(self, device: Union[str, torch.device] = "cuda"):
        self.device = torch.device(device)
        self._h = C.c_void_p(None)
        self.last_meter = None       # (m, 4) int64 on the device: {S, n, peak, hops} of the last call's clips that went through the meter
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
        each = per_clip(finish, n)
        params = [f.samples(sample_rate) for f in each]
        levels = [f.level() for f in each]
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
            sub, par, lev = parts[lo:lo + MAX_SEGMENTS], params[lo:lo + MAX_SEGMENTS], levels[lo:lo + MAX_SEGMENTS]
            m = len(sub)
            ptrs = (C.c_void_p * m)(*[c.data_ptr() if c.shape[0] else None for c in sub])
            off, n_out = (C.c_long * m)(), (C.c_long * m)()
            head = (self._h, ptrs, (C.c_long * m)(*[int(c.shape[0]) for c in sub]), (C.c_int32 * m)(*[p[0] for p in par]),
                    (C.c_int32 * m)(*[p[1] for p in par]), (C.c_int32 * m)(*[p[2] for p in par]))
            with torch.cuda.device(self.device):
                if any(pt for pt, _ in lev):       # a clip of the call asks for a loudness: meter them all (three launches), then finish
                    from .loudness import measure_rows
                    want = [f.true_peak and f.loudness is not None for f in each[lo:lo + MAX_SEGMENTS]]
                    if any(want):                  # one packed buffer for both meters; the true peaks into the peak column of the clips that ask
                        from .loudness import pack_clips
                        from .truepeak import ROW, measure_packed
                        p = pack_clips(sub, self.device)
                        self.last_meter = meter = measure_rows(sub, self.device, packed=p)
                        peaks = torch.empty((m, ROW), dtype=torch.int64, device=self.device)
                        measure_packed(_abi.lib, p.packed, p.c_offs, p.c_lens, m, peaks)
                        at = 0
                        for asks, run in itertools.groupby(want):
                            k = len(list(run))
                            if asks:
                                meter[at:at + k, 2] = peaks[at:at + k, 1]
                            at += k
                    else:
                        self.last_meter = meter = measure_rows(sub, self.device)
                    self._check(lib.mimi_fin_segments_ld(*head, (C.c_long * m)(*[pt for pt, _ in lev]), (C.c_int32 * m)(*[c for _, c in lev]),
                                                         meter.data_ptr(), m, out.data_ptr() + 2 * base, off, n_out, stream))
                else:
                    self._check(lib.mimi_fin_segments(*head, m, out.data_ptr() + 2 * base, off, n_out, stream))
            res.extend(out[base + off[k]:base + off[k] + n_out[k]] for k in range(m))
            base += sum(n_out[:m])
        return res

    def __del__(self):
        try:
            if self._h:
                lib.mimi_fin_destroy(self._h)
        except Exception:
            pass
