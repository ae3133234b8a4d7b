"""Watermark hook with the reference's names (reference: sesameai/watermarking.py:9,20-55), so that
``from sesameai.watermarking import CSM_1B_GH_WATERMARK, watermark`` (reference tts_service.py:23) keeps
working when this package shadows the reference's.

The reference's watermark is a third-party model (``silentcipher``, weights fetched from the hub).  When ``silentcipher`` is importable it
is used exactly where the reference uses it, with SciPy polyphase resampling instead of torchaudio; when it is not, ``load_watermarker``
returns ``None`` and ``watermark`` hands the audio back unchanged (and says so once).

``load_watermarker(device, kind="device")`` returns this project's OWN mark instead (include/mimi_hip.h, mimi_wm_pool_*): a keyed
spread-spectrum mark with host-interference cancellation, one symbol per 1920-sample block, stated in exact integers
(tests/watermark_ref.py) and computed on the device bit for bit -- embedded in any number of live streams by one launch
(``WatermarkPool.feed``), found again in a clip that was cut, padded, scaled or re-quantised (``WatermarkPool.detect``).  It is not
silentcipher's mark and silentcipher's detector does not see it; ``verify`` here does.
"""
import ctypes as C
from math import gcd
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch

from ._stream_pool import StreamPool, _stream, int16_if_all, one_format, pack, shared_pool, split

# Same public (hence not secret) key as the reference; use a private one in another application.
CSM_1B_GH_WATERMARK = [212, 211, 146, 56, 201]

_WM_RATE = 44100
_warned = False

MAX_STREAMS = 64                 # MIMI_WM_MAX_STREAMS
MAX_CLIPS = 64                   # MIMI_WM_MAX_CLIPS
S, K = 1920, 56                  # samples per symbol, symbols per period
P = S * K                        # samples per period
ROW = 64                         # MIMI_WM_ROW
SAMPLE_RATE = 24000
SYNC_MASK = 0xFF
ALL_MASK = (1 << K) - 1


def _resample(x: torch.Tensor, src: int, dst: int) -> torch.Tensor:
    if src == dst:
        return x
    from scipy.signal import resample_poly
    g = gcd(src, dst)
    y = resample_poly(x.detach().to(torch.float32).cpu().numpy(), dst // g, src // g, axis=-1)
    return torch.from_numpy(y.astype("float32")).to(x.device)


def crc8(data: Sequence[int]) -> int:
    c = 0
    for v in data:
        c ^= int(v) & 0xFF
        for _ in range(8):
            c = ((c << 1) ^ 0x07) & 0xFF if c & 0x80 else (c << 1) & 0xFF
    return c


def symbol_bits(payload: Sequence[int]) -> int:
    """The 56 symbols of a five-byte payload as one word: sync 0xB2, the bytes, their CRC-8, MSB first; bit k (LSB = symbol 0) = symbol k."""
    data = _payload(payload)
    word = 0
    for j, byte in enumerate([0xB2] + data + [crc8(data)]):
        for i in range(8):
            word |= ((byte >> (7 - i)) & 1) << (8 * j + i)
    return word


def _payload(payload: Sequence[int]) -> List[int]:
    data = [int(v) for v in payload]
    if len(data) != 5 or any(not 0 <= v <= 255 for v in data):
        raise ValueError("a watermark payload is five bytes")
    return data


def default_secret(payload: Sequence[int] = CSM_1B_GH_WATERMARK) -> int:
    return int.from_bytes(bytes(_payload(payload)), "big")


class DetectRow:
    """One clip's answer from ``WatermarkPool.detect``: the best candidate ``index`` and its ``offset`` (clip sample 0 is stream position
    ``offset``), its ``score`` of ``covered`` symbols, the clip's complete ``blocks``, the decoded ``payload`` (five bytes), whether its
    CRC-8 holds, and ``R`` (56 int64)."""

    def __init__(self, row: Sequence[int]):
        self.index, self.offset, self.score, self.covered, self.blocks = (int(v) for v in row[:5])
        self.payload = list(int(row[5]).to_bytes(5, "big"))
        self.crc_ok = bool(row[6])
        self.R = [int(v) for v in row[8:8 + K]]

    @property
    def found(self) -> bool:
        """``verify``'s decision: at least 16 masked symbols covered and at most an eighth of them wrong."""
        return verify_row(self.score, self.covered)

    def __repr__(self) -> str:
        return f"DetectRow(offset={self.offset}, score={self.score}/{self.covered}, blocks={self.blocks}, payload={self.payload}, crc_ok={self.crc_ok})"


class WatermarkPool(StreamPool):
    """``n`` independent watermark streams under one ``secret`` (None: the default payload's 40-bit value).  ``reset(ids, payloads, t_q4)``
    starts the listed streams afresh (host arithmetic, no launch); ``feed(ids, chunks, final)`` gives every listed stream its new samples at
    24 kHz, fp32 or int16, and returns each stream's finished blocks in that format: ONE launch, no host-to-device copy of a plan, no
    synchronisation.  A stream's output lags its input by fewer than 1920 samples; ``final`` lets the open block through unchanged and
    leaves the stream fresh.  ``embed`` marks whole clips, ``detect`` searches clips for the mark."""

    def __init__(self, n: int, secret: Optional[int] = None, device: Union[str, torch.device] = "cuda"):
        self.secret = default_secret() if secret is None else int(secret) & (2 ** 64 - 1)
        super().__init__("mimi_wm_pool", n, device, int(n), self.secret)           # (resolves the library: importing this module does not)

    def out_count(self, sid: int, n_in: int, final: bool = False) -> int:
        """Samples a feed of ``n_in`` samples would give stream ``sid`` now (host arithmetic)."""
        return self._count("out_count", sid, n_in, final)

    def reset(self, ids: Sequence[int], payloads=CSM_1B_GH_WATERMARK, t_q4: Union[int, Sequence[int]] = 8) -> None:
        """Start the listed streams afresh; ``payloads``: five bytes for all, or one such list per id; ``t_q4``: 1 .. 64, one or one per id."""
        ids = [int(i) for i in ids]
        ps = [_payload(payloads)] * len(ids) if len(payloads) == 5 and not hasattr(payloads[0], "__len__") else [_payload(p) for p in payloads]
        ts = [int(t_q4)] * len(ids) if isinstance(t_q4, int) else [int(t) for t in t_q4]
        assert len(ps) == len(ids) and len(ts) == len(ids), "one payload and one t_q4 per id"
        m = max(len(ids), 1)
        flat = [b for p in ps for b in p] or [0] * 5
        self._check(self._lib.mimi_wm_pool_reset(self._h, (C.c_int32 * m)(*ids), (C.c_uint8 * len(flat))(*flat), (C.c_int32 * m)(*ts), len(ids)))

    @torch.inference_mode()
    def feed(self, ids: Sequence[int], chunks: Sequence[torch.Tensor], final: Union[bool, Sequence[bool]] = False) -> List[torch.Tensor]:
        """ids: n distinct stream ids; chunks[i]: (n_i,) fp32 or int16 at 24 kHz, n_i >= 0, CPU or device, the new samples of stream
        ids[i] (all chunks of a call in one format); final: one flag, or one per stream -> one tensor per stream (views into one buffer)."""
        p = pack(chunks, self.device, one_format, ids, final)
        out = torch.empty(max(sum(self._counts("out_count", p)), 1), dtype=p.dtype, device=self.device)
        n_out = (C.c_long * p.m)()
        self._check(self._lib.mimi_wm_pool_feed(self._h, *p.head, int(p.dtype == torch.int16), out.data_ptr(), n_out, _stream()))
        return split(out, n_out[:len(p.ids)])

    def embed(self, wavs: Sequence[torch.Tensor], payload=CSM_1B_GH_WATERMARK, t_q4: Union[int, Sequence[int]] = 8) -> List[torch.Tensor]:
        """Up to ``n_streams`` whole clips in ONE launch, on fresh streams with ``final``: each clip comes back marked, same length and format."""
        if not 1 <= len(wavs) <= self.n_streams:
            raise ValueError(f"embed takes 1 .. {self.n_streams} clips a call")
        ids = list(range(len(wavs)))
        self.reset(ids, payload, t_q4)         # (host arithmetic: also covers a stream that an earlier call, interrupted, left open)
        return self.feed(ids, wavs, final=True)

    @torch.inference_mode()
    def detect(self, wavs: Sequence[torch.Tensor], payload=None, search: Tuple[int, int] = (0, P), want_rows: bool = False):
        """Up to 64 clips, each (n_i,) fp32 or int16 at 24 kHz, searched over the candidate offsets ``(o0 + i) % P``, ``i < n_off``
        (``search``: one pair for all clips, or one per clip).  ``payload``: five bytes for all, one such list per clip, or None -- then only
        the sync byte is asked for ("find any payload").  -> one ``DetectRow`` per clip (``want_rows``: the raw (n, 64) int64 tensor
        instead, still on the device: no synchronisation)."""
        n = len(wavs)
        if not 1 <= n <= MAX_CLIPS:
            raise ValueError(f"detect takes 1 .. {MAX_CLIPS} clips a call")
        if payload is None:
            expect, mask = [symbol_bits(CSM_1B_GH_WATERMARK)] * n, [SYNC_MASK] * n
        elif len(payload) == 5 and not hasattr(payload[0], "__len__"):
            expect, mask = [symbol_bits(payload)] * n, [ALL_MASK] * n
        else:
            assert len(payload) == n, "one payload per clip"
            expect, mask = [symbol_bits(p) for p in payload], [ALL_MASK] * n
        pairs = [search] * n if isinstance(search[0], int) else list(search)
        assert len(pairs) == n, "one (o0, n_off) per clip"
        p = pack(wavs, self.device, int16_if_all, noun="clip")
        scores = torch.empty(max(sum(max(int(q[1]), 0) for q in pairs), 1), dtype=torch.int32, device=self.device)
        rows = torch.empty(n, ROW, dtype=torch.int64, device=self.device)
        L, U = C.c_long * n, C.c_uint64 * n
        self._check(self._lib.mimi_wm_pool_detect(self._h, p.c_offs, p.c_lens, L(*[int(q[0]) for q in pairs]), L(*[int(q[1]) for q in pairs]),
                                                  U(*expect), U(*mask), n, p.packed.data_ptr(), int(p.dtype == torch.int16), scores.data_ptr(),
                                                  rows.data_ptr(), _stream()))
        if want_rows:
            return rows
        return [DetectRow(r) for r in rows.cpu().tolist()]


def key_of(watermark) -> Optional[List[int]]:
    """``watermark=`` of the paths that make audio as a checked five-byte key: None (no mark), True or "device" (the public CSM key), or
    the key itself."""
    if watermark is None or watermark is False:
        return None
    if watermark is True or watermark == "device":
        return list(CSM_1B_GH_WATERMARK)
    if isinstance(watermark, str):
        raise ValueError("watermark must be None, True, 'device' or a five-byte key")
    return _payload(watermark)


_POOLS: Dict[Tuple[str, int], WatermarkPool] = {}       # embed()'s and detect()'s pools, made on first use and kept


def _shared_pool(key: Sequence[int], device: Union[str, torch.device, None], like: Optional[torch.Tensor] = None) -> WatermarkPool:
    secret = default_secret(key)
    return shared_pool(_POOLS, device, like, lambda dev: (str(dev), secret), lambda dev: WatermarkPool(MAX_STREAMS, secret, device=dev))


def embed(wavs: Sequence[torch.Tensor], key: Sequence[int] = CSM_1B_GH_WATERMARK, device: Union[str, torch.device, None] = None,
          t_q4: int = 8) -> List[torch.Tensor]:
    """Up to 64 clips at 24 kHz, fp32 or int16, marked with ``key`` under its own secret in ONE launch."""
    return _shared_pool(key, device, wavs[0] if len(wavs) else None).embed(wavs, key, t_q4)


def detect(wavs: Sequence[torch.Tensor], key: Sequence[int] = CSM_1B_GH_WATERMARK, search: Tuple[int, int] = (0, P),
           device: Union[str, torch.device, None] = None) -> List[DetectRow]:
    """Up to 64 clips at 24 kHz searched for ``key``'s mark under its own secret."""
    return _shared_pool(key, device, wavs[0] if len(wavs) else None).detect(wavs, key, search=search)


class DeviceWatermarker:
    """What ``load_watermarker(device, kind="device")`` returns: this project's mark under one ``secret`` (None: each key's own 40-bit
    value, the default -- a pool per secret, made on first use and kept)."""

    def __init__(self, device: Union[str, torch.device] = "cuda", secret: Optional[int] = None, t_q4: int = 8):
        self.device, self.secret, self.t_q4 = torch.device(device), secret, int(t_q4)
        self._pools: Dict[int, WatermarkPool] = {}

    def pool(self, key: Sequence[int]) -> WatermarkPool:
        secret = default_secret(key) if self.secret is None else int(self.secret)
        if secret not in self._pools:
            self._pools[secret] = WatermarkPool(MAX_STREAMS, secret, device=self.device)
        return self._pools[secret]

    def _at_24k(self, audio: torch.Tensor, sample_rate: int) -> torch.Tensor:
        if int(sample_rate) == SAMPLE_RATE:
            return audio
        from .resample import resample
        return resample([audio.to(self.device)], int(sample_rate), SAMPLE_RATE, device=self.device)[0]

    def embed(self, audio: torch.Tensor, sample_rate: int, key: Sequence[int]) -> torch.Tensor:
        """The clip marked, at the rate and in the format it came in; on the device.  At 24 kHz no resampler runs."""
        if audio.numel() == 0:
            return audio
        y = self.pool(key).embed([self._at_24k(audio, sample_rate)], key, self.t_q4)[0]
        if int(sample_rate) == SAMPLE_RATE:
            return y
        from .resample import resample
        return resample([y], SAMPLE_RATE, int(sample_rate), device=self.device)[0]

    def detect(self, audio: torch.Tensor, sample_rate: int, key: Sequence[int], search: Optional[Tuple[int, int]] = None) -> DetectRow:
        return self.pool(key).detect([self._at_24k(audio, sample_rate)], key, search=(0, P) if search is None else search)[0]


def load_watermarker(device: str = "cuda", kind: Optional[str] = None):
    """kind None: silentcipher's model if it is importable, else None (the pass-through); "device": this project's own mark."""
    if kind == "device":
        return DeviceWatermarker(device)
    if kind is not None:
        raise ValueError(f"unknown watermarker kind {kind!r}")
    try:
        import silentcipher
    except ImportError:
        return None
    return silentcipher.get_model(model_type="44.1k", device=device)


@torch.inference_mode()
def watermark(watermarker, audio_array: torch.Tensor, sample_rate: int, watermark_key: List[int]) -> Tuple[torch.Tensor, int]:
    """-> (audio, sample rate of the returned audio)."""
    global _warned
    if watermarker is None:
        if not _warned:
            print("sesameai.watermarking: silentcipher is not installed; audio is returned without a watermark")
            _warned = True
        return audio_array, sample_rate
    if isinstance(watermarker, DeviceWatermarker):
        return watermarker.embed(audio_array, sample_rate, watermark_key), sample_rate
    wide = _resample(audio_array, sample_rate, _WM_RATE)
    marked, _ = watermarker.encode_wav(wide, _WM_RATE, watermark_key, calc_sdr=False, message_sdr=36)
    out_rate = min(_WM_RATE, sample_rate)
    return _resample(marked, _WM_RATE, out_rate), out_rate


def verify_row(score: int, covered: int) -> bool:
    """The decision on a detect row: at least 16 symbols covered and at most an eighth of them wrong."""
    return covered >= 16 and covered - score <= covered // 8


@torch.inference_mode()
def verify(watermarker, watermarked_audio: torch.Tensor, sample_rate: int, watermark_key: List[int],
           search: Optional[Tuple[int, int]] = None) -> bool:
    """``search`` = (o0, n_off) (the device mark only; None: one full period)."""
    if watermarker is None:
        return False
    if isinstance(watermarker, DeviceWatermarker):
        row = watermarker.detect(watermarked_audio, sample_rate, watermark_key, search)
        return verify_row(row.score, row.covered)
    res = watermarker.decode_wav(_resample(watermarked_audio, sample_rate, _WM_RATE), _WM_RATE, phase_shift_decoding=True)
    return bool(res["status"]) and res["messages"][0] == watermark_key
