"""Audio at any sample rate, on the device: a pool of stateful polyphase resampler streams (include/mimi_hip.h, mimi_rs_pool_*).

The reference resamples every context clip with ``torchaudio.functional.resample`` before Mimi sees it (tts_service.py:161-166,
ogwebapp.py:44-47).  Here the filter is ``scipy.signal.resample_poly``'s default -- the one ``tts_service.load_audio`` and the watermarker
already use on the host -- as ONE launch per call for up to 64 streams, with state: a stream's chunks, concatenated, are bit for bit the
one-shot result of its concatenated samples, so a microphone at 48 kHz or a telephone at 8 kHz can be followed while it runs.  All
arithmetic is the library's; this file marshals."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch

from ._stream_pool import StreamPool, _stream, int16_if_all, pack, shared_pool, split

MAX_STREAMS = 64                 # MIMI_RS_MAX_STREAMS
_FMT = {torch.float32: 0, torch.int16: 1}


class ResamplerPool(StreamPool):
    """``n`` independent resampler streams ``src_rate`` -> ``dst_rate``.  ``feed(ids, chunks, final)`` gives every listed stream its new
    samples -- fp32, or int16 (``s / 32768``) -- and returns what each may emit now, as ``out_dtype`` (fp32, or int16:
    ``round(clamp(y, -1, 1) * 32767)``): ONE launch, no host-to-device copy of a plan, no synchronisation.  ``final`` ends a stream's clip:
    the tail comes out and the stream is fresh.  ``reset`` is host arithmetic only.  Streams start fresh."""

    def __init__(self, src_rate: int, dst_rate: int, n: int, device: Union[str, torch.device] = "cuda", out_dtype: torch.dtype = torch.float32):
        if out_dtype not in _FMT:
            raise ValueError("out_dtype must be torch.float32 or torch.int16")
        self.src_rate, self.dst_rate, self.out_dtype = int(src_rate), int(dst_rate), out_dtype
        super().__init__("mimi_rs_pool", n, device, self.src_rate, self.dst_rate, int(n))
        up, down, half = C.c_int(0), C.c_int(0), C.c_int(0)
        self._check(self._lib.mimi_rs_pool_taps(self._h, None, C.byref(up), C.byref(down), C.byref(half)))
        self.up, self.down, self.half = up.value, down.value, half.value

    def taps(self) -> torch.Tensor:
        """For tests: the fp32 taps the device holds, h[0 .. 2 * half]."""
        out = torch.empty(2 * self.half + 1, dtype=torch.float32)
        self._check(self._lib.mimi_rs_pool_taps(self._h, out.data_ptr(), None, None, None))
        return out

    def out_count(self, sid: int, n_in: int, final: bool = False) -> int:
        """Samples a feed of ``n_in`` samples would give stream ``sid`` now (host arithmetic)."""
        return self._count("out_count", sid, n_in, final)

    def reset(self, ids: Optional[Sequence[int]] = None) -> None:
        """Start the listed streams (default: all) afresh.  No launch."""
        ids = [int(i) for i in (range(self.n_streams) if ids is None else ids)]
        self._check(self._lib.mimi_rs_pool_reset(self._h, (C.c_int32 * max(len(ids), 1))(*ids), len(ids)))

    @torch.inference_mode()
    def feed(self, ids: Sequence[int], chunks: Sequence[torch.Tensor], final: Union[bool, Sequence[bool]] = False) -> List[torch.Tensor]:
        """ids: n distinct stream ids; chunks[i]: (n_i,) fp32 or int16, n_i >= 0, CPU or device, the new samples of stream ids[i];
        final: one flag, or one per stream -> one (m_i,) ``out_dtype`` tensor per stream (views into one buffer), m_i >= 0."""
        p = pack(chunks, self.device, int16_if_all, ids, final)
        out = torch.empty(max(sum(self._counts("out_count", p)), 1), dtype=self.out_dtype, device=self.device)
        n_out = (C.c_long * p.m)()
        self._check(self._lib.mimi_rs_pool_feed(self._h, *p.head, _FMT[p.dtype], out.data_ptr(), _FMT[self.out_dtype], n_out, _stream()))
        return split(out, n_out[:len(p.ids)])


_POOLS: Dict[Tuple[int, int, str, torch.dtype], ResamplerPool] = {}       # resample()'s pools, made on first use and kept


@torch.inference_mode()
def resample(wavs: Sequence[torch.Tensor], src_rate: int, dst_rate: int, device: Union[str, torch.device, None] = None,
             out_dtype: torch.dtype = torch.float32) -> List[torch.Tensor]:
    """Up to 64 clips of different lengths, each (n_i,) fp32 or int16 at ``src_rate`` -> each (ceil(n_i * up / down),) at ``dst_rate``, in ONE
    launch on fresh streams with ``final``: per clip what ``scipy.signal.resample_poly(clip, up, down)`` computes, in fp32."""
    if not 1 <= len(wavs) <= MAX_STREAMS:
        raise ValueError(f"resample takes 1 .. {MAX_STREAMS} clips a call")
    pool = shared_pool(_POOLS, device, wavs[0], lambda dev: (int(src_rate), int(dst_rate), str(dev), out_dtype),
                       lambda dev: ResamplerPool(src_rate, dst_rate, MAX_STREAMS, device=dev, out_dtype=out_dtype))
    ids = list(range(len(wavs)))
    pool.reset(ids)                    # (host arithmetic: covers a stream that an earlier call, interrupted, left open)
    return pool.feed(ids, wavs, final=True)
