"""A look-ahead peak limiter on the device: a pool of stateful limiter streams (include/mimi_hip.h, mimi_lim_pool_*).

Nothing that leaves may exceed a ceiling, and a hard clamp at the ceiling sends out a clipped waveform.  A limiter stream delays its input
by ``lookahead`` samples and brings its gain down smoothly AHEAD of every peak: the gain is what the peak requires exactly on it and
recovers at a fixed step per sample.  Exact integers (tests/limiter_ref.py states the rule), for up to 64 streams with two launches per
call, with state: a stream's outputs, concatenated over any chunk schedule, are bit for bit the one-shot result.  Behind the live leveler
(``paired``) it lets the leveler overshoot by a known headroom instead of clamping: what ``generate_many_stream(loudness=, limiter=)``
puts behind each slot.  Sample peaks by default; ``Limit(true_peak=True)`` detects the peaks of the 4x oversampled signal
(tests/truepeak_ref.py; ``sesameai.truepeak`` is the meter) at ``TRUE_PEAK_TAPS`` more samples of latency.  All arithmetic is the library's;
this file marshals."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

import torch

from ._stream_pool import StreamPool, _stream, one_format, pack, shared_pool, split

MAX_STREAMS = 64                 # MIMI_LIM_MAX_STREAMS
SAMPLE_RATE = 24000
ROW = 4                          # MIMI_LIM_ROW
GAIN_ONE = 65536                 # a gain of 1 in Q16
LOOKAHEAD_MAX = 480
RHO_MIN, RHO_MAX = 8, 65536
SHIFT_MAX = 4
TRUE_PEAK_TAPS = 8               # TP_T: a true-peak stream's latency is lookahead + 8


def ceiling_i16(ceiling_db: float) -> int:
    """The sample ceiling in int16 units, from dB relative to full scale (as ``sesameai.loudness.ceiling_i16``)."""
    ceiling_db = float(ceiling_db)
    if ceiling_db > 0.0:
        raise ValueError("ceiling_db: dB relative to full scale, <= 0")
    return max(1, min(32767, int(math.floor(32767.0 * 10.0 ** (ceiling_db / 20.0)))))


class Limit(NamedTuple):
    """How one stream is limited (include/mimi_hip.h, mimi_lim_pool_reset): ``ceiling_db`` the sample ceiling in dB relative to full scale;
    ``lookahead`` = L in samples, the stream's latency (120: 5 ms); ``release_ms`` the time from silence of gain back to 1 (the step is
    rho = max(8, rint(65536 / (release_ms * 24))) in Q16 per sample); ``drive_shift`` = hr: the input is multiplied by exactly 2^hr in
    front of the limiter; ``headroom_shift`` = h, read by ``paired`` alone: how many doublings a leveler in front may overshoot;
    ``true_peak``: the stream detects true peaks, 4x oversampled, and its latency is ``lookahead`` + 8 (mimi_lim_pool_reset_tp)."""
    ceiling_db: float = -1.0
    lookahead: int = 120
    release_ms: float = 100.0
    drive_shift: int = 0
    headroom_shift: int = 2
    true_peak: bool = False

    @property
    def latency(self) -> int:
        """Samples the stream holds back until more arrive."""
        return int(self.lookahead) + (TRUE_PEAK_TAPS if self.true_peak else 0)

    def params(self) -> tuple:
        """(C, L, rho, hr): the integers the library takes, checked against its ranges."""
        if int(self.lookahead) != self.lookahead or not 1 <= int(self.lookahead) <= LOOKAHEAD_MAX:
            raise ValueError("lookahead: an integer, 1 .. 480 samples")
        if not float(self.release_ms) > 0.0:
            raise ValueError("release_ms: above 0")
        rho = max(RHO_MIN, int(round(GAIN_ONE / (float(self.release_ms) * 24.0))))
        if rho > RHO_MAX:
            raise ValueError("release_ms: at least one sample (1 / 24 ms)")
        for name, v in (("drive_shift", self.drive_shift), ("headroom_shift", self.headroom_shift)):
            if int(v) != v or not 0 <= int(v) <= SHIFT_MAX:
                raise ValueError(f"{name}: an integer, 0 .. 4")
        return ceiling_i16(self.ceiling_db), int(self.lookahead), rho, int(self.drive_shift)


class LimitState(NamedTuple):
    """What ``state`` says of one stream since it was fresh: ``min_gain_q16`` the smallest gain emitted (65536 while none); the samples
    emitted; the samples whose gain was below 1; the samples the final clamp changed (only an infinite or absurd sample)."""
    min_gain_q16: int
    emitted: int
    limited: int
    clipped: int

    @property
    def min_gain(self) -> float:
        return self.min_gain_q16 / GAIN_ONE


class LimiterPool(StreamPool):
    """``n`` independent limiter streams.  ``reset(ids, limits)`` makes the listed streams fresh, each with its ``Limit`` (host
    arithmetic, no launch; a stream must be reset once before it is fed); ``feed(ids, chunks, final)`` gives every listed stream its new
    samples at 24 kHz, fp32 or int16 (one format a call), and returns what each emits: at most two launches, no host-to-device copy of a
    plan, no synchronisation (a call that lists sample-peak and true-peak streams: two launches for each kind).  A stream holds its last
    ``Limit.latency`` samples back until more arrive or ``final`` ends its clip, which
    leaves it fresh with the same parameters.  ``state(ids)``: one launch, a (len(ids), 4) int64 tensor that stays on the device;
    ``poll()`` reads it (one small copy, the call's only synchronisation)."""

    def __init__(self, n: int, device: Union[str, torch.device] = "cuda"):
        super().__init__("mimi_lim_pool", n, device, int(n))

    def out_count(self, sid: int, n_in: int, final: bool = False) -> int:
        """Samples a feed of ``n_in`` samples would emit for stream ``sid`` now (host arithmetic)."""
        return self._count("out_count", sid, n_in, final)

    def reset(self, ids: Sequence[int], limits: Union[Limit, Sequence[Limit]] = Limit()) -> None:
        ids = [int(i) for i in ids]
        limits = [limits] * len(ids) if isinstance(limits, Limit) else list(limits)
        assert len(limits) == len(ids), "one Limit per id"
        q = [lm.params() for lm in limits]
        m = max(len(ids), 1)
        head = (self._h, (C.c_int32 * m)(*ids), *[(C.c_int32 * m)(*[v[k] for v in q]) for k in range(4)])
        if any(lm.true_peak for lm in limits):
            self._check(self._lib.mimi_lim_pool_reset_tp(*head, (C.c_int32 * m)(*[int(bool(lm.true_peak)) for lm in limits]), len(ids)))
        else:
            self._check(self._lib.mimi_lim_pool_reset(*head, len(ids)))

    @torch.inference_mode()
    def feed(self, ids: Sequence[int], chunks: Sequence[torch.Tensor], final: Union[bool, Sequence[bool]] = False) -> List[torch.Tensor]:
        """ids: n distinct stream ids; chunks[i]: (n_i,) fp32 or int16 at 24 kHz, n_i >= 0, CPU or device (one format a call: the output
        keeps it); final: one flag, or one per stream -> per stream the samples it emits, views of one buffer."""
        p = pack(chunks, self.device, one_format, ids, final)
        out = torch.empty(max(sum(self._counts("out_count", p)), 1), dtype=p.dtype, device=self.device)
        n_out = (C.c_long * p.m)()
        self._check(self._lib.mimi_lim_pool_feed(self._h, *p.head, out.data_ptr(), n_out, int(p.dtype == torch.int16), _stream()))
        return split(out, n_out[:len(p.ids)])

    @torch.inference_mode()
    def state(self, ids: Sequence[int]) -> torch.Tensor:
        """(len(ids), 4) int64 ON THE DEVICE: {min gain emitted (Q16), samples emitted, samples limited, samples clamped} since each
        stream was fresh, as of its last feed: one launch."""
        ids = [int(i) for i in ids]
        out = torch.empty((max(len(ids), 1), ROW), dtype=torch.int64, device=self.device)
        self._check(self._lib.mimi_lim_pool_state(self._h, (C.c_int32 * max(len(ids), 1))(*ids), len(ids), out.data_ptr(), _stream()))
        return out[:len(ids)]

    def poll(self, ids: Optional[Sequence[int]] = None) -> List[LimitState]:
        """``state`` read back; ids None: every stream."""
        return [LimitState(*r) for r in self.state(range(self.n_streams) if ids is None else ids).cpu().tolist()]


_POOLS: Dict[str, LimiterPool] = {}        # limit()'s pools, made on first use and kept


@torch.inference_mode()
def limit(wavs: Sequence[torch.Tensor], limit: Union[Limit, Sequence[Limit]] = Limit(),
          device: Union[str, torch.device, None] = None) -> List[torch.Tensor]:
    """Up to 64 clips of different lengths, each (n_i,) fp32 or int16 at 24 kHz (one format a call), limited the way a live stream is: on
    fresh streams with ``final``, in ONE ``feed`` -- two launches, no synchronisation; every clip comes back whole.  ``limit``: one
    ``Limit`` for all clips or one per clip."""
    if not 1 <= len(wavs) <= MAX_STREAMS:
        raise ValueError(f"limit takes 1 .. {MAX_STREAMS} clips a call")
    pool = shared_pool(_POOLS, device, wavs[0], str, lambda dev: LimiterPool(MAX_STREAMS, device=dev))
    ids = list(range(len(wavs)))
    pool.reset(ids, limit)
    return pool.feed(ids, wavs, final=True)


def paired(level, limit: Limit = Limit()) -> Tuple[object, Limit]:
    """(Level', Limit') for a limiter behind a live leveler (``sesameai.loudness.Level``).  The leveler runs h = ``limit.headroom_shift``
    doublings LOWER -- target loudness - h 20 log10 2, start gain / 2^h, largest gain - 6 h dB -- under a ceiling of 0 dB, and the limiter
    is driven by exactly 2^h (``drive_shift`` = h).  In fp32 that is the same leveler with its cap and clamp 2^h higher, followed by the
    limiter: where the leveler alone would have clamped an onset at the ceiling, the limiter brings it down ahead of the peak."""
    h = int(limit.headroom_shift)
    limit.params()
    lower = level._replace(loudness=float(level.loudness) - h * 20.0 * math.log10(2.0), start_gain=float(level.start_gain) / 2.0 ** h,
                           max_gain_db=float(level.max_gain_db) - 6.0 * h, ceiling_db=0.0)
    lower.params()
    return lower, limit._replace(drive_shift=h)


def per_request_limits(limiter, n: int) -> List[Optional[Limit]]:
    """None, True (the default ``Limit``), one ``Limit`` for all n, or one of these per request (None among them) -> one ``Limit`` or None
    per request, checked."""
    def one(v):
        lm = None if v is None or v is False else Limit() if v is True else v
        if lm is not None:
            if not isinstance(lm, Limit):
                raise ValueError("limiter: None, True or a Limit")
            lm.params()
        return lm
    if limiter is None or isinstance(limiter, (bool, Limit)):
        return [one(limiter)] * n
    limiter = [one(v) for v in limiter]
    if len(limiter) != n:
        raise ValueError(f"limiter: one value, or one per request ({n})")
    return limiter
