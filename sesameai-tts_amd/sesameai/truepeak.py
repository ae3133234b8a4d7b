"""A true-peak meter on the device (include/mimi_hip.h, mimi_tp_measure): the largest magnitude a clip's 4x oversampled waveform reaches,
which a 24 kHz sample peak can miss by 3 dB and a resampler behind it makes real.  Exact integers (tests/truepeak_ref.py states the rule):
the detector of ``sesameai.limiter.Limit(true_peak=True)`` and of ``SegmentFinish(true_peak=True)``.  All arithmetic is the library's;
this file marshals."""
from __future__ import annotations

import math
from typing import List, NamedTuple, Sequence, Union

import torch

from ._stream_pool import _stream, one_format, pack

MAX_CLIPS = 64                   # MIMI_TP_MAX_CLIPS
ROW = 4                          # MIMI_TP_ROW
FULL_SCALE = 32768


class TruePeak(NamedTuple):
    """One clip's row: the sample peak and the true peak in int16 units (fp32: |x| * 32768, rounded up), the first sample whose own
    magnitude or one of the two intervals beside it reaches the true peak, the clip's length."""
    sample_peak: int
    true_peak: int
    position: int
    n: int

    @property
    def true_peak_db(self) -> float:
        return true_peak_db(self.true_peak)

    @property
    def sample_peak_db(self) -> float:
        return true_peak_db(self.sample_peak)


def true_peak_db(peak: Union[int, float]) -> float:
    """A peak in int16 units -> dB relative to full scale (dBTP for a true peak); silence gives -inf."""
    return 20.0 * math.log10(float(peak) / FULL_SCALE) if peak > 0 else -math.inf


def measure_packed(lib, buf: torch.Tensor, c_offs, c_lens, n: int, out: torch.Tensor) -> None:
    """``mimi_tp_measure`` on clips already packed in ``buf`` (fp32 or int16, on the device), rows into ``out`` ((n, 4) int64 on the
    device): one memset, one launch, no synchronisation."""
    rc = lib.mimi_tp_measure(buf.data_ptr(), c_offs, c_lens, int(n), int(buf.dtype == torch.int16), out.data_ptr(), _stream())
    if rc != 0:
        from . import _abi
        raise _abi.CsmError(rc, (lib.mimi_tp_last_error() or b"").decode())


@torch.inference_mode()
def true_peak_rows(wavs: Sequence[torch.Tensor], device: Union[str, torch.device, None] = None) -> torch.Tensor:
    """Up to 64 clips of different lengths, each (n_i,) fp32 or int16 at 24 kHz (one format a call) -> (len(wavs), 4) int64 ON THE DEVICE:
    {sample peak, true peak, position, n} per clip; an empty clip gives zeros."""
    from . import _abi
    if not 1 <= len(wavs) <= MAX_CLIPS:
        raise ValueError(f"true_peak takes 1 .. {MAX_CLIPS} clips a call")
    if device is None:
        device = wavs[0].device if wavs[0].is_cuda else torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    p = pack(wavs, device, one_format, noun="clip")
    out = torch.empty((len(wavs), ROW), dtype=torch.int64, device=device)
    with torch.cuda.device(device):
        measure_packed(_abi.lib, p.packed, p.c_offs, p.c_lens, len(wavs), out)
    return out


def true_peak(wavs: Sequence[torch.Tensor], device: Union[str, torch.device, None] = None) -> List[TruePeak]:
    """``true_peak_rows`` read back (one small copy, the call's only synchronisation)."""
    return [TruePeak(*r) for r in true_peak_rows(wavs, device).cpu().tolist()]
