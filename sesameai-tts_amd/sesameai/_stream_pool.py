"""What the pools of stateful audio streams share on the Python side (resample, stretch, vad, watermarking; include/mimi_hip.h,
mimi_rs_pool_* / mimi_ts_pool_* / mimi_vad_pool_* / mimi_wm_pool_*): the handle and its errors, the packing of a call's chunks into one
device buffer with the host arrays the library reads, and the pools that the one-shot functions make on first use and keep.  All
arithmetic is the library's; this file marshals."""
from __future__ import annotations

import ctypes as C
from typing import Callable, Dict, Hashable, List, NamedTuple, Optional, Sequence, Tuple, Union

import torch


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


# The dtype rules of a call: (chunks, device) -> (the call's dtype, the chunks in it on the device).

def int16_if_all(chunks: Sequence[torch.Tensor], device: torch.device) -> Tuple[torch.dtype, List[torch.Tensor]]:
    """int16 only if every chunk is int16; otherwise fp32, and a stray int16 chunk is scaled by 1 / 32768 (resampler, VAD, detect)."""
    dt = torch.int16 if len(chunks) and all(c.dtype == torch.int16 for c in chunks) else torch.float32
    return dt, [c.to(device) if c.dtype == dt else (c.to(device).float() / 32768.0 if c.dtype == torch.int16 else c.to(device, dt))
                for c in chunks]


def one_format(chunks: Sequence[torch.Tensor], device: torch.device) -> Tuple[torch.dtype, List[torch.Tensor]]:
    """int16 or fp32, and a call that mixes them is refused (watermark feed: a marked stream keeps its format)."""
    i16 = len(chunks) > 0 and all(c.dtype == torch.int16 for c in chunks)
    assert i16 or all(c.dtype != torch.int16 for c in chunks), "fp32 and int16 chunks in one call"
    dt = torch.int16 if i16 else torch.float32
    return dt, [c.to(device, dt) for c in chunks]


def fp32_unscaled(chunks: Sequence[torch.Tensor], device: torch.device) -> Tuple[torch.dtype, List[torch.Tensor]]:
    """Everything to fp32 as ``.to`` converts it (stretcher, Mimi encode)."""
    return torch.float32, [c.to(device=device, dtype=torch.float32) for c in chunks]


class Packed(NamedTuple):
    """One call's chunks as the library takes them.  ``head`` = (ids, offsets, lengths, final flags, n, the packed buffer's address): the
    arguments every ``*_pool_feed`` starts with behind its handle.  ``m`` = max(n, 1): the length of every host array of the call."""
    ids: List[int]
    fin: List[bool]
    lens: List[int]
    offs: List[int]
    packed: torch.Tensor
    dtype: torch.dtype
    c_offs: C.Array
    c_lens: C.Array
    head: tuple
    m: int


def pack(chunks: Sequence[torch.Tensor], device: torch.device, rule: Callable, ids: Optional[Sequence[int]] = None,
         final: Union[bool, Sequence[bool]] = False, noun: str = "chunk") -> Packed:
    """Chunks (or clips), each (n_i,), n_i >= 0, CPU or device -> one device buffer, chunk after chunk, in the dtype ``rule`` chooses, with
    their offsets and lengths in it; ``ids`` and ``final`` (one flag, or one per id) as a feed call lists them (None: a call without
    streams).  An empty call still hands the library real memory -- a 1-element zero buffer, 1-element arrays -- so that ITS check refuses
    the call."""
    n = len(chunks)
    if ids is not None:
        ids = [int(i) for i in ids]
        n = len(ids)
        assert len(chunks) == n, "one chunk per id"
    assert all(c.dim() == 1 for c in chunks), f"every {noun} must be (n,)"
    fin = [bool(final)] * n if isinstance(final, (bool, int)) else [bool(f) for f in final]
    assert len(fin) == n, "one final flag per id"
    dt, parts = rule(chunks, device)
    lens = [int(c.shape[0]) for c in parts]
    offs = [sum(lens[:k]) for k in range(n)]
    packed = torch.cat(parts) if sum(lens) else torch.zeros(1, dtype=dt, device=device)
    m = max(n, 1)
    c_ids, c_offs, c_lens, c_fin = (C.c_int32 * m)(*(ids or [])), (C.c_long * m)(*offs), (C.c_long * m)(*lens), (C.c_int32 * m)(*[int(f) for f in fin])
    return Packed(ids or [], fin, lens, offs, packed, dt, c_offs, c_lens, (c_ids, c_offs, c_lens, c_fin, n, packed.data_ptr()), m)


def split(buf: torch.Tensor, counts: Sequence[int]) -> List[torch.Tensor]:
    """The packed results of a call, one view per stream."""
    counts = [int(c) for c in counts]
    return list(buf[:sum(counts)].split(counts))


class StreamPool:
    """The handle of one pool: ``api`` names the library's functions (``api + "_create"``, ...), ``create_args`` are what its create takes
    in front of the handle's address.  The library is resolved here, not at import."""

    def __init__(self, api: str, n: int, device: Union[str, torch.device], *create_args):
        from . import _abi
        self._abi, self._lib, self._api = _abi, _abi.lib, api
        self.n_streams, self.device = int(n), torch.device(device)
        self._h = C.c_void_p(None)
        with torch.cuda.device(self.device):
            rc = self._fn("create")(*create_args, C.byref(self._h))
        if rc != 0:
            raise _abi.CsmError(rc, (self._fn("last_error")(None) or b"").decode())

    def _fn(self, name: str):
        return getattr(self._lib, f"{self._api}_{name}")

    def _check(self, rc: int) -> None:
        if rc != 0:
            raise self._abi.CsmError(rc, (self._fn("last_error")(self._h) or b"").decode())

    def _count(self, name: str, sid: int, n_in: int, final: bool) -> int:
        """``*_out_count`` / ``*_frame_count`` (host arithmetic): -1 means ask ``last_error``."""
        n = int(self._fn(name)(self._h, int(sid), int(n_in), int(bool(final))))
        if n < 0:
            self._check(-1)
        return n

    def _counts(self, name: str, p: Packed) -> List[int]:
        """What the call ``p`` will give each listed stream.  (An id the library will refuse counts as 0 here: the feed is what refuses it.)"""
        return [max(int(self._fn(name)(self._h, i, k, int(f))), 0) for i, k, f in zip(p.ids, p.lens, p.fin)]

    def __del__(self):
        try:
            if self._h:
                self._fn("destroy")(self._h)
        except Exception:
            pass


def shared_pool(pools: Dict[Hashable, StreamPool], device: Union[str, torch.device, None], like: Optional[torch.Tensor],
                key: Callable[[torch.device], Hashable], make: Callable[[torch.device], StreamPool]):
    """The pool a one-shot function keeps per ``key(device)``, made on first use.  ``device`` None: ``like``'s if it lives on one, else the
    current one; a device without an index is the current one."""
    if device is None:
        device = like.device if like is not None and like.is_cuda else torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    at = key(device)
    if at not in pools:
        pools[at] = make(device)
    return pools[at]
