"""Loudness on the device: a pool of stateful meter streams (include/mimi_hip.h, mimi_ld_pool_*), and the numbers the finisher needs to
bring a clip to a stated loudness (mimi_fin_segments_ld).

A served TTS is expected to hit a stated loudness (podcast and telephony targets are given in LUFS); dividing a clip by its own peak, as
the reference does (tts_service.py:291), does not give one.  Here the measurement is ITU-R BS.1770-4 / EBU R 128 for one channel in exact
integers -- K-weighting as a 512-tap integer FIR, 100 ms hop energies, 400 ms gating blocks behind the absolute and the relative gate --
for up to 64 clips or streams with two launches per call, with state: a stream's hop energies, concatenated over any chunk schedule, are
bit for bit the one-shot result.  A stream of the same pool can also LEVEL what it is fed (mimi_ld_pool_level_*: ``Level``,
``LoudnessPool.level_reset / level_feed / level_state``, ``level``): a causal gain that follows the gated loudness measured so far, hop by
hop, with as many samples out as in on every call -- what ``generate_many_stream(loudness=)`` puts behind each slot.  All arithmetic is the
library's; this file marshals, and ``lufs`` turns the integers into the number a person reads."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, NamedTuple, Optional, Sequence, Union

import torch

from ._stream_pool import StreamPool, _stream, int16_if_all, one_format, pack, shared_pool, split

MAX_STREAMS = 64                 # MIMI_LD_MAX_STREAMS
HOP = 2400                       # MIMI_LD_HOP: samples per hop at 24 kHz
SAMPLE_RATE = 24000
ROW = 4                          # MIMI_LD_ROW


def lufs(S: int, n: int) -> float:
    """The integrated loudness of {S, n}: -0.691 + 10 log10(S / (n 4 H 32768^2)); -inf where no block passed the gates."""
    return -0.691 + 10.0 * math.log10(S / (n * 4.0 * HOP * 32768.0 ** 2)) if n > 0 and S > 0 else float("-inf")


def target_ms(loudness: float) -> int:
    """P_T of mimi_fin_segments_ld: the K-weighted mean square, in int16 units, of a signal at ``loudness`` LUFS."""
    loudness = float(loudness)
    if not -70.0 <= loudness <= 0.0:
        raise ValueError("loudness: a target in LUFS, -70 .. 0")
    return int(round(2.0 ** 30 * 10.0 ** ((loudness + 0.691) / 10.0)))


def ceiling_i16(ceiling_db: float) -> int:
    """C of mimi_fin_segments_ld: the sample ceiling in int16 units, from dB relative to full scale."""
    ceiling_db = float(ceiling_db)
    if ceiling_db > 0.0:
        raise ValueError("ceiling_db: dB relative to full scale, <= 0")
    return max(1, min(32767, int(math.floor(32767.0 * 10.0 ** (ceiling_db / 20.0)))))


class Loudness(NamedTuple):
    """What the meter says of one clip or stream: S and n, the sum and the count of the gating blocks behind both gates; the sample peak in
    int16 units; the hops measured."""
    S: int
    n: int
    peak: int
    hops: int

    @property
    def lufs(self) -> float:
        return lufs(self.S, self.n)


class LoudnessPool(StreamPool):
    """``n`` independent meter streams.  ``reset(ids)`` starts the listed streams afresh (host arithmetic, no launch); ``feed(ids, chunks,
    final)`` gives every listed stream its new samples at 24 kHz, fp32 or int16, and returns the hop energies each completed: at most two
    launches, no host-to-device copy of a plan, no synchronisation.  ``final`` ends a stream's clip: a partial hop is discarded and the
    stream is fresh.  ``integrate(ids)`` gates what the streams' rings hold: one launch, a (len(ids), 4) int64 tensor {S, n, peak, hops}
    that stays on the device; ``poll()`` reads every stream's (one small copy, the call's only synchronisation).  ring: hop energies a
    stream holds, 4 .. 4096 (0: 4096)."""

    def __init__(self, n: int, device: Union[str, torch.device] = "cuda", ring: int = 0):
        super().__init__("mimi_ld_pool", n, device, int(n), int(ring))

    def hop_count(self, sid: int, n_in: int, final: bool = False) -> int:
        """Hops a feed of ``n_in`` samples would complete for stream ``sid`` now (host arithmetic)."""
        return self._count("hop_count", sid, n_in, final)

    def reset(self, ids: Sequence[int]) -> None:
        ids = [int(i) for i in ids]
        self._check(self._lib.mimi_ld_pool_reset(self._h, (C.c_int32 * max(len(ids), 1))(*ids), len(ids)))

    @torch.inference_mode()
    def feed(self, ids: Sequence[int], chunks: Sequence[torch.Tensor], final: Union[bool, Sequence[bool]] = False,
             packed=None) -> List[torch.Tensor]:
        """ids: n distinct stream ids; chunks[i]: (n_i,) fp32 or int16 at 24 kHz, n_i >= 0, CPU or device (int16 only if every chunk is);
        final: one flag, or one per stream -> per stream the (K_i,) int64 energies of the hops it completed, views of one buffer.
        ``packed``: the call's chunks already packed by ``pack_clips`` (then ids, chunks and final are its own)."""
        p = pack(chunks, self.device, int16_if_all, ids, final) if packed is None else packed
        energy = torch.empty(max(sum(self._counts("hop_count", p)), 1), dtype=torch.int64, device=self.device)
        n_hops = (C.c_long * p.m)()
        self._check(self._lib.mimi_ld_pool_feed(self._h, *p.head, int(p.dtype == torch.int16), energy.data_ptr(), n_hops, _stream()))
        return split(energy, n_hops[:len(p.ids)])

    @torch.inference_mode()
    def integrate(self, ids: Sequence[int]) -> torch.Tensor:
        ids = [int(i) for i in ids]
        out = torch.empty((max(len(ids), 1), ROW), dtype=torch.int64, device=self.device)
        self._check(self._lib.mimi_ld_pool_integrate(self._h, (C.c_int32 * max(len(ids), 1))(*ids), len(ids), out.data_ptr(), _stream()))
        return out[:len(ids)]

    def poll(self) -> List[Loudness]:
        return [Loudness(*r) for r in self.integrate(range(self.n_streams)).cpu().tolist()]

    # -- the streams as live levelers (mimi_ld_pool_level_*): a stream levels from ``level_reset`` until ``reset`` returns it to metering

    def level_reset(self, ids: Sequence[int], levels: Union["Level", Sequence["Level"]]) -> None:
        """The listed streams are fresh, in leveler mode, each with its ``Level`` (one for all, or one per id): host arithmetic, no launch."""
        ids = [int(i) for i in ids]
        levels = [levels] * len(ids) if isinstance(levels, Level) else list(levels)
        assert len(levels) == len(ids), "one Level per id"
        q = [lv.params() for lv in levels]
        m = max(len(ids), 1)
        cols = [(C.c_long * m)(*[v[0] for v in q])] + [(C.c_int32 * m)(*[v[k] for v in q]) for k in range(1, 5)]
        self._check(self._lib.mimi_ld_pool_level_reset(self._h, (C.c_int32 * m)(*ids), *cols, len(ids)))

    @torch.inference_mode()
    def level_feed(self, ids: Sequence[int], chunks: Sequence[torch.Tensor], final: Union[bool, Sequence[bool]] = False,
                   in_place: bool = False) -> List[torch.Tensor]:
        """ids: n distinct leveler streams; chunks[i]: (n_i,) fp32 or int16 at 24 kHz, n_i >= 0 (one format a call: the output keeps it);
        final: one flag, or one per stream -> per stream its n_i levelled samples, views of one buffer: nothing is held back.  At most
        three launches, no host-to-device copy of a plan, no synchronisation.  ``last_energies[i]`` are the hop energies stream i
        completed, ``last_gains[i]`` its n_hops + 2 boundary gains (Q16, int32) from the first hop the call touched to the end of the
        open one: device views.  in_place: the packed input buffer is also the output."""
        p = pack(chunks, self.device, one_format, ids, final)
        counts = self._counts("hop_count", p)
        energy = torch.empty(max(sum(counts), 1), dtype=torch.int64, device=self.device)
        gain = torch.empty(sum(counts) + 2 * p.m, dtype=torch.int32, device=self.device)
        out = p.packed if in_place else torch.empty_like(p.packed)
        n_hops = (C.c_long * p.m)()
        self._check(self._lib.mimi_ld_pool_level_feed(self._h, *p.head, int(p.dtype == torch.int16), out.data_ptr(), energy.data_ptr(),
                                                      gain.data_ptr(), n_hops, _stream()))
        hops = [int(v) for v in n_hops[:len(p.ids)]]
        self.last_energies, self.last_gains = split(energy, hops), split(gain, [h + 2 for h in hops])
        return split(out, p.lens)

    @torch.inference_mode()
    def level_state(self, ids: Sequence[int]) -> torch.Tensor:
        """(len(ids), 4) int64 ON THE DEVICE: {the gain the open hop ends on (Q16), hops, samples clamped since fresh, the running peak of
        the complete hops}, as of each stream's last feed: one launch."""
        ids = [int(i) for i in ids]
        out = torch.empty((max(len(ids), 1), LEVEL_ROW), dtype=torch.int64, device=self.device)
        self._check(self._lib.mimi_ld_pool_level_state(self._h, (C.c_int32 * max(len(ids), 1))(*ids), len(ids), out.data_ptr(), _stream()))
        return out[:len(ids)]

    def poll_level(self, ids: Optional[Sequence[int]] = None) -> List["LevelState"]:
        """``level_state`` read back (one small copy, the call's only synchronisation); ids None: every stream -- all must be levelers."""
        return [LevelState(*r) for r in self.level_state(range(self.n_streams) if ids is None else ids).cpu().tolist()]


LEVEL_ROW = 4                    # MIMI_LD_LEVEL_ROW
GAIN_ONE = 65536                 # a gain of 1 in Q16
GAIN_LIMIT = 1 << 22             # the largest gmax: 64 x


class Level(NamedTuple):
    """How one live stream is levelled (include/mimi_hip.h, mimi_ld_pool_level_reset): ``loudness`` the target in LUFS; ``ceiling_db`` the
    sample ceiling in dB relative to full scale; ``start_gain`` the linear gain the stream starts on, before anything is measured;
    ``max_gain_db`` the largest gain, 6 dB a doubling (24 -> 16 x); ``slew_shift`` = sh: the gain moves by at most 1 / 2^sh of itself per
    100 ms hop (4: about 0.53 dB)."""
    loudness: float
    ceiling_db: float = -1.0
    start_gain: float = 1.0
    max_gain_db: float = 24.0
    slew_shift: int = 4

    def params(self) -> tuple:
        """(P_T, C, g0, gmax, sh): the integers the library takes, checked against its ranges."""
        gmax = int(round(GAIN_ONE * 2.0 ** (float(self.max_gain_db) / 6.0)))
        g0 = int(round(float(self.start_gain) * GAIN_ONE))
        if not 1 <= gmax <= GAIN_LIMIT:
            raise ValueError("max_gain_db: -96 .. 36 dB (a Q16 gain of 1 .. 2^22)")
        if not 1 <= g0 <= gmax:
            raise ValueError("start_gain: above 0 and at most the largest gain")
        if int(self.slew_shift) != self.slew_shift or not 1 <= int(self.slew_shift) <= 16:
            raise ValueError("slew_shift: an integer, 1 .. 16")
        return target_ms(self.loudness), ceiling_i16(self.ceiling_db), g0, gmax, int(self.slew_shift)


class LevelState(NamedTuple):
    """What ``level_state`` says of one stream: ``gain_q16`` the gain its open hop ends on; the hops measured; the samples the ceiling
    clamped; the running sample peak of the complete hops, in int16 units."""
    gain_q16: int
    hops: int
    clipped: int
    peak: int

    @property
    def gain(self) -> float:
        return self.gain_q16 / GAIN_ONE


_POOLS: Dict[str, LoudnessPool] = {}       # measure()'s pools, made on first use and kept


@torch.inference_mode()
def pack_clips(wavs: Sequence[torch.Tensor], device: torch.device):
    """The clips of one ``measure_rows`` call as it packs them -- one device buffer, streams 0 .. n - 1, ``final`` -- for a caller that
    wants the same buffer for something else too (``SegmentFinisher`` hands it to the true-peak meter)."""
    return pack(wavs, device, int16_if_all, list(range(len(wavs))), True)


def measure_rows(wavs: Sequence[torch.Tensor], device: Union[str, torch.device, None] = None, packed=None) -> torch.Tensor:
    """Up to 64 clips of different lengths, each (n_i,) fp32 or int16 at 24 kHz -> (len(wavs), 4) int64 {S, n, peak, hops} ON THE DEVICE,
    on fresh streams with ``final``: three launches, no synchronisation.  What ``SegmentFinisher`` hands to mimi_fin_segments_ld.
    ``packed``: ``pack_clips(wavs, device)``, if the caller has made it already."""
    if not 1 <= len(wavs) <= MAX_STREAMS:
        raise ValueError(f"measure takes 1 .. {MAX_STREAMS} clips a call")
    pool = shared_pool(_POOLS, device, wavs[0], str, lambda dev: LoudnessPool(MAX_STREAMS, device=dev))
    ids = list(range(len(wavs)))
    pool.reset(ids)                    # (host arithmetic: also covers a stream that an earlier call, interrupted, left open)
    if packed is None:
        pool.feed(ids, wavs, final=True)
    else:
        pool.feed(ids, wavs, final=True, packed=packed)
    return pool.integrate(ids)


def measure(wavs: Sequence[torch.Tensor], device: Union[str, torch.device, None] = None) -> List[Loudness]:
    """``measure_rows`` read back: one ``Loudness`` per clip (one small copy, the call's only synchronisation)."""
    return [Loudness(*r) for r in measure_rows(wavs, device).cpu().tolist()]


@torch.inference_mode()
def level(wavs: Sequence[torch.Tensor], loudness: Union[float, "Level", Sequence[Union[float, "Level"]]],
          device: Union[str, torch.device, None] = None) -> List[torch.Tensor]:
    """Up to 64 clips of different lengths, each (n_i,) fp32 or int16 at 24 kHz (one format a call), levelled the way a live stream is:
    on fresh streams with ``final``, in ONE ``level_feed`` -- three launches, no synchronisation.  ``loudness``: a target in LUFS or a
    ``Level``, for all clips or one per clip.  What ``generate_many_stream(loudness=)`` hands out, chunk by chunk, concatenated."""
    if not 1 <= len(wavs) <= MAX_STREAMS:
        raise ValueError(f"level takes 1 .. {MAX_STREAMS} clips a call")
    levels = per_request_levels(loudness, len(wavs))
    if any(v is None for v in levels):
        raise ValueError("level: every clip needs a target")
    pool = shared_pool(_POOLS, device, wavs[0], lambda dev: ("level", str(dev)), lambda dev: LoudnessPool(MAX_STREAMS, device=dev))
    ids = list(range(len(wavs)))
    pool.level_reset(ids, levels)
    return pool.level_feed(ids, wavs, final=True)


def per_request_levels(loudness, n: int) -> List[Optional[Level]]:
    """None, one LUFS value or ``Level`` for all n, or one per request (None among them) -> one ``Level`` or None per request, checked."""
    def one(v):
        lv = None if v is None else v if isinstance(v, Level) else Level(float(v))
        if lv is not None:
            lv.params()
        return lv
    if loudness is None or isinstance(loudness, (int, float, Level)):
        return [one(loudness)] * n
    loudness = [one(v) for v in loudness]
    if len(loudness) != n:
        raise ValueError(f"loudness: one target, or one per request ({n})")
    return loudness


def per_request(loudness, n: int) -> List[Optional[float]]:
    """None, one target for all n, or one per request (None among them) -> one per request."""
    if loudness is None or isinstance(loudness, (int, float)):
        return [None if loudness is None else float(loudness)] * n
    loudness = [None if v is None else float(v) for v in loudness]
    if len(loudness) != n:
        raise ValueError(f"loudness: one target, or one per request ({n})")
    return loudness
