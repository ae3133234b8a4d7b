"""The Whisper encoder on the device (include/mimi_hip.h, mimi_wenc_*): the hot path of every Whisper-family recogniser.

distil-whisper keeps the WHOLE Whisper encoder and a two-layer decoder, and every turn, however short, is padded to 30 s and runs all 1500
encoder positions: the encoder is what stands between the end of a turn and its text.  ``WhisperEncoder`` is the forward of transformers'
``WhisperEncoder`` in fp16 operands and fp32 everything else (tests/whisper_enc_ref.py states the rule in float64): 2 + 7 L + 1 launches
per call whatever the batch, no synchronisation, no allocation in the library.  A clip's output has the same bits alone, at any place in a
batch of any size, and on a repeated call.  All arithmetic is the library's; this file marshals.

Not built: the decoder (the two-layer decoder and the tokenizer stay the user's transformers objects, sesameai/stt.py), long-form windows
past 30 s, cropping the encoder to a turn's live frames (which would change results)."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Mapping, Union

import torch

MAX_LAYERS, MAX_CTX, MAX_BATCH = 32, 1500, 64          # MIMI_WENC_MAX_LAYERS, MIMI_WENC_MAX_CTX, MIMI_WENC_MAX_BATCH
CONFIG_KEYS = ("n_mels", "d_model", "n_layers", "n_heads", "ffn_dim", "n_ctx", "ln_eps")
_FMT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}

# field of the C struct -> name in model.get_encoder().state_dict() (per layer: behind "layers.{i}.").  k_proj has no bias.
TOP_NAMES = {"conv1_w": "conv1.weight", "conv1_b": "conv1.bias", "conv2_w": "conv2.weight", "conv2_b": "conv2.bias",
             "embed_positions": "embed_positions.weight", "layer_norm_w": "layer_norm.weight", "layer_norm_b": "layer_norm.bias"}
LAYER_NAMES = {"self_attn_layer_norm_w": "self_attn_layer_norm.weight", "self_attn_layer_norm_b": "self_attn_layer_norm.bias",
               "q_w": "self_attn.q_proj.weight", "q_b": "self_attn.q_proj.bias", "k_w": "self_attn.k_proj.weight",
               "v_w": "self_attn.v_proj.weight", "v_b": "self_attn.v_proj.bias", "out_w": "self_attn.out_proj.weight",
               "out_b": "self_attn.out_proj.bias", "final_layer_norm_w": "final_layer_norm.weight",
               "final_layer_norm_b": "final_layer_norm.bias", "fc1_w": "fc1.weight", "fc1_b": "fc1.bias", "fc2_w": "fc2.weight",
               "fc2_b": "fc2.bias"}


class WencConfig(C.Structure):
    _fields_ = [(k, C.c_int32) for k in CONFIG_KEYS[:-1]] + [("ln_eps", C.c_float)]


class WencLayerWeights(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in LAYER_NAMES]


class WencWeights(C.Structure):
    _fields_ = [("host", C.c_int32)] + [(k, C.c_void_p) for k in TOP_NAMES] + [("layers", WencLayerWeights * MAX_LAYERS)]


def config_from_model(model) -> Dict[str, Union[int, float]]:
    """The encoder's config out of a transformers Whisper model's ``config`` (the LayerNorm eps is fixed at 1e-5 there)."""
    c = model.config
    return dict(n_mels=int(c.num_mel_bins), d_model=int(c.d_model), n_layers=int(c.encoder_layers), n_heads=int(c.encoder_attention_heads),
                ffn_dim=int(c.encoder_ffn_dim), n_ctx=int(c.max_source_positions), ln_eps=1e-5)


def map_state_dict(config: Mapping, state_dict: Mapping[str, torch.Tensor], device: Union[str, torch.device, None] = None):
    """-> (the C weights struct, the fp32 contiguous tensors it points into: keep them alive until create returns).  ``device`` None: the
    tensors stay where they are, and must all be on the CPU or all on one device."""
    n_layers = int(config["n_layers"])
    if not 1 <= n_layers <= MAX_LAYERS:
        raise ValueError(f"n_layers outside 1 .. {MAX_LAYERS}")
    if any(k.endswith("k_proj.bias") for k in state_dict):
        raise ValueError("a Whisper encoder has no bias on k_proj")
    w, keep = WencWeights(), []

    def put(struct, field, name):
        if name not in state_dict:
            raise KeyError(f"state dict lacks {name}")
        t = state_dict[name].detach()
        t = t.to(device=device if device is not None else t.device, dtype=torch.float32).contiguous()
        keep.append(t)
        setattr(struct, field, t.data_ptr())

    for field, name in TOP_NAMES.items():
        put(w, field, name)
    for i in range(n_layers):
        for field, name in LAYER_NAMES.items():
            put(w.layers[i], field, f"layers.{i}.{name}")
    kinds = {t.device.type for t in keep}
    if len(kinds) != 1:
        raise ValueError("the state dict's tensors lie on the CPU and on a device")
    w.host = int(kinds == {"cpu"})
    return w, keep


class WhisperEncoder:
    """``WhisperEncoder(config, state_dict, max_batch=1)``: config = {n_mels, d_model, n_layers, n_heads, ffn_dim, n_ctx, ln_eps};
    state_dict: a transformers ``model.get_encoder().state_dict()`` (any float dtype, CPU or device; converted to fp16 once).
    ``encode(features) -> (B, n_ctx, d_model)``."""

    def __init__(self, config: Mapping, state_dict: Mapping[str, torch.Tensor], max_batch: int = 1, device: Union[str, torch.device] = "cuda"):
        from . import _abi
        self._abi, self._lib, self._h = _abi, _abi.lib, None
        self.config = {k: (float(config[k]) if k == "ln_eps" else int(config[k])) for k in CONFIG_KEYS}
        self.max_batch, self.device = int(max_batch), torch.device(device)
        self.n_mels, self.d_model, self.n_ctx = self.config["n_mels"], self.config["d_model"], self.config["n_ctx"]
        cfg = WencConfig(**self.config)
        w, keep = map_state_dict(self.config, state_dict)
        h = C.c_void_p(None)
        if self.device.type == "cuda" and torch.cuda.is_available():
            with torch.cuda.device(self.device):
                rc = self._lib.mimi_wenc_create(C.byref(cfg), C.byref(w), self.max_batch, C.byref(h))
        else:
            rc = self._lib.mimi_wenc_create(C.byref(cfg), C.byref(w), self.max_batch, C.byref(h))
        del keep
        if rc != 0:
            raise _abi.CsmError(rc, (self._lib.mimi_wenc_last_error(None) or b"").decode())
        self._h = h

    @classmethod
    def from_model(cls, model, max_batch: int = 1, device: Union[str, torch.device, None] = None) -> "WhisperEncoder":
        """From a transformers Whisper model (``WhisperForConditionalGeneration`` or ``WhisperModel``): its encoder's state dict and config."""
        sd = model.get_encoder().state_dict()
        if device is None:
            device = next(iter(sd.values())).device
            device = device if device.type == "cuda" else "cuda"
        return cls(config_from_model(model), sd, max_batch=max_batch, device=device)

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.mimi_wenc_destroy(self._h)
            self._h = None

    def _check(self, rc: int) -> None:
        if rc < 0:
            raise self._abi.CsmError(rc, (self._lib.mimi_wenc_last_error(self._h) or b"").decode())

    def describe(self, batch: int = 1) -> str:
        """The launch plan of an encode of ``batch`` clips."""
        buf = C.create_string_buffer(4096)
        self._check(self._lib.mimi_wenc_describe(self._h, int(batch), buf, len(buf)))
        return buf.value.decode()

    @torch.inference_mode()
    def encode(self, features: torch.Tensor, dtype: torch.dtype = torch.float32) -> torch.Tensor:
        """features: (B, n_mels, 2 n_ctx) or (n_mels, 2 n_ctx), B <= max_batch -> (B, n_ctx, d_model) in ``dtype`` (fp32, fp16 or bf16)."""
        if dtype not in _FMT:
            raise ValueError("dtype must be float32, float16 or bfloat16")
        x = features[None] if features.dim() == 2 else features
        if x.dim() != 3 or tuple(x.shape[1:]) != (self.n_mels, 2 * self.n_ctx):
            raise ValueError(f"features must be (B, {self.n_mels}, {2 * self.n_ctx})")
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        out = torch.empty((x.shape[0], self.n_ctx, self.d_model), dtype=dtype, device=self.device)
        with torch.cuda.device(self.device):
            from ._stream_pool import _stream
            self._check(self._lib.mimi_wenc_encode(self._h, x.data_ptr(), int(x.shape[0]), out.data_ptr(), _FMT[dtype], _stream()))
        return out
