"""The Whisper encoder's arithmetic rule in float64 torch (include/mimi_hip.h, mimi_wenc_*), as transformers' WhisperEncoder computes it.

features (n_mels, 2 n_ctx) -> conv1 (k = 3, pad 1) + GELU -> conv2 (k = 3, stride 2, pad 1: output t reads inputs 2t-1, 2t, 2t+1) + GELU ->
transpose, + embed_positions -> L pre-LN layers { x += out(attn(LN(x))); x += fc2(gelu(fc1(LN(x)))) } -> LayerNorm.  Self-attention has a bias
on q, v and out and NONE on k; q is scaled by head_dim^-0.5 = 0.125 (head_dim is 64 in every Whisper size); there is no mask.  GELU is the erf
form.  The state dict's names are those of ``model.get_encoder().state_dict()``.

``rounded=True`` rounds to fp16 at exactly the points where the device does and nowhere else: the input features, every weight matrix, conv1's
GELU output, each LayerNorm output (not the final one), q (after bias and x 0.125), k, v, the softmax numerators P (the running sum takes
them unrounded), the attention output, fc1's GELU output.  Everything else -- biases, LayerNorm parameters, positions, accumulators, scores,
the softmax, erf, the statistics, the residual stream -- is exact here and fp32 there.

``fault`` switches ONE ingredient to a plausible wrong one (FAULTS); tests/test_whisper_enc_oracle.py shows that each moves the output far
outside the bound the device is held to."""
import hashlib
import math

import torch

HEAD_DIM = 64
KEY_TILE = 32            # the device walks the keys in tiles of 32: the two key-tail faults are about its last, partial tile
FAULTS = ("q_unscaled", "causal", "pos_shift", "conv2_phase", "heads_interleaved", "no_final_ln", "key_tail_dropped", "key_tail_zero")

CASES = {                # the smallest shapes at which each kernel can still go wrong (tools/whisper_enc_golden.py)
    "A": dict(n_mels=80, d_model=128, n_layers=2, n_heads=2, ffn_dim=512, n_ctx=100, ln_eps=1e-5, gain=2.0, seed=101, live=70),
    "B": dict(n_mels=128, d_model=192, n_layers=3, n_heads=3, ffn_dim=768, n_ctx=100, ln_eps=1e-5, gain=2.0, seed=202, live=130),
    "C": dict(n_mels=80, d_model=384, n_layers=4, n_heads=6, ffn_dim=1536, n_ctx=1500, ln_eps=1e-5, gain=1.0, seed=303, live=900),
}
CONFIG_KEYS = ("n_mels", "d_model", "n_layers", "n_heads", "ffn_dim", "n_ctx", "ln_eps")


def config_of(case):
    return {k: case[k] for k in CONFIG_KEYS}


def stored_rows(n_ctx):
    """The rows of a case that the fixture keeps: all of a short case; of a long one the first and last 40 and every 23rd."""
    if n_ctx <= 200:
        return list(range(n_ctx))
    return sorted(set(range(40)) | set(range(n_ctx - 40, n_ctx)) | set(range(0, n_ctx, 23)))


def sinusoids(length, channels, max_timescale=10000.0):
    inc = math.log(max_timescale) / (channels // 2 - 1)
    inv = torch.exp(-inc * torch.arange(channels // 2, dtype=torch.float64))
    t = torch.arange(length, dtype=torch.float64)[:, None] * inv[None]
    return torch.cat([t.sin(), t.cos()], dim=1)


def weight_names(cfg):
    """(name, shape, kind) of every tensor of the encoder's state dict, in the order make_weights draws them"""
    d, f, m, L = cfg["d_model"], cfg["ffn_dim"], cfg["n_mels"], cfg["n_layers"]
    out = [("conv1.weight", (d, m, 3), "w"), ("conv1.bias", (d,), "b"), ("conv2.weight", (d, d, 3), "w"), ("conv2.bias", (d,), "b"),
           ("embed_positions.weight", (cfg["n_ctx"], d), "pos")]
    for i in range(L):
        p = f"layers.{i}."
        out += [(p + "self_attn_layer_norm.weight", (d,), "g"), (p + "self_attn_layer_norm.bias", (d,), "lb"),
                (p + "self_attn.q_proj.weight", (d, d), "w"), (p + "self_attn.q_proj.bias", (d,), "b"),
                (p + "self_attn.k_proj.weight", (d, d), "w"),
                (p + "self_attn.v_proj.weight", (d, d), "w"), (p + "self_attn.v_proj.bias", (d,), "b"),
                (p + "self_attn.out_proj.weight", (d, d), "w"), (p + "self_attn.out_proj.bias", (d,), "b"),
                (p + "final_layer_norm.weight", (d,), "g"), (p + "final_layer_norm.bias", (d,), "lb"),
                (p + "fc1.weight", (f, d), "w"), (p + "fc1.bias", (f,), "b"), (p + "fc2.weight", (d, f), "w"), (p + "fc2.bias", (d,), "b")]
    out += [("layer_norm.weight", (d,), "g"), ("layer_norm.bias", (d,), "lb")]
    return out


def make_weights(cfg, seed, gain):
    """fp32 state dict: conv and linear weights gain * randn / sqrt(fan_in), biases 0.5 randn, LayerNorm weight 1 + 0.3 randn and bias
    0.3 randn, Whisper's sinusoids as positions; every draw from one seeded CPU generator, in weight_names' order."""
    g = torch.Generator().manual_seed(int(seed))
    sd = {}
    for name, shape, kind in weight_names(cfg):
        if kind == "pos":
            sd[name] = sinusoids(*shape).float()
            continue
        x = torch.randn(shape, generator=g, dtype=torch.float32)
        if kind == "w":
            fan_in = 1
            for s in shape[1:]:
                fan_in *= s
            x = x * (float(gain) / math.sqrt(fan_in))
        elif kind == "b":
            x = x * 0.5
        elif kind == "g":
            x = 1.0 + 0.3 * x
        else:
            x = x * 0.3
        sd[name] = x.float()
    return sd


def make_features(n_mels, T, seed, live, kind="uniform"):
    """(n_mels, T) fp32 like a short turn: values in [-1, 1.5] on the first ``live`` frames and a constant floor after them.
    kind "int": whole numbers in {-1, 0, 1}."""
    g = torch.Generator().manual_seed(int(seed))
    x = torch.rand((n_mels, T), generator=g, dtype=torch.float32) * 2.5 - 1.0
    if kind == "int":
        x = torch.round(x * 0.8)
    x[:, int(live):] = -1.0
    return x


def checksum(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:16]


def checksums(cfg, sd, x):
    out = {name: checksum(sd[name]) for name, _, _ in weight_names(cfg)}
    out["features"] = checksum(x)
    return out


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))


def _ln(x, w, b, eps):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * w + b


def forward(cfg, sd, features, rounded=False, fault=None):
    """features (B, n_mels, 2 n_ctx) or (n_mels, 2 n_ctx) -> (B, n_ctx, d) float64"""
    assert fault is None or fault in FAULTS, fault
    F = torch.nn.functional
    r = (lambda t: t.half().double()) if rounded else (lambda t: t)
    W = lambda name: r(sd[name].double())           # a weight matrix
    V = lambda name: sd[name].double()              # a bias, a LayerNorm parameter, the positions
    d, H, T, eps = cfg["d_model"], cfg["n_heads"], cfg["n_ctx"], float(cfg["ln_eps"])
    assert d == H * HEAD_DIM
    x = features.double()
    if x.dim() == 2:
        x = x[None]
    B = x.shape[0]
    assert x.shape[1:] == (cfg["n_mels"], 2 * T), x.shape
    x = r(x)
    h = r(_gelu(F.conv1d(x, W("conv1.weight"), V("conv1.bias"), padding=1)))
    if fault == "conv2_phase":
        h = _gelu(F.conv1d(F.pad(h, (0, 2)), W("conv2.weight"), V("conv2.bias"), stride=2))
    else:
        h = _gelu(F.conv1d(h, W("conv2.weight"), V("conv2.bias"), stride=2, padding=1))
    pos = V("embed_positions.weight")
    if fault == "pos_shift":
        pos = torch.roll(pos, -1, 0)
    h = h.permute(0, 2, 1) + pos[None]

    def split(t):                                   # (B, T, d) -> (B, H, T, 64)
        if fault == "heads_interleaved":
            return t.view(B, T, HEAD_DIM, H).permute(0, 3, 1, 2)
        return t.view(B, T, H, HEAD_DIM).permute(0, 2, 1, 3)

    def merge(t):
        if fault == "heads_interleaved":
            return t.permute(0, 2, 3, 1).reshape(B, T, d)
        return t.permute(0, 2, 1, 3).reshape(B, T, d)

    for i in range(cfg["n_layers"]):
        p = f"layers.{i}."
        a = r(_ln(h, V(p + "self_attn_layer_norm.weight"), V(p + "self_attn_layer_norm.bias"), eps))
        q = a @ W(p + "self_attn.q_proj.weight").T + V(p + "self_attn.q_proj.bias")
        q = r(q if fault == "q_unscaled" else q * 0.125)
        k = r(a @ W(p + "self_attn.k_proj.weight").T)
        v = r(a @ W(p + "self_attn.v_proj.weight").T + V(p + "self_attn.v_proj.bias"))
        q, k, v = split(q), split(k), split(v)
        n_keys = T
        if fault == "key_tail_dropped":
            n_keys = (T // KEY_TILE) * KEY_TILE
        s = q @ k[:, :, :n_keys].transpose(-1, -2)
        vv = v[:, :, :n_keys]
        if fault == "key_tail_zero":                # the partial tile's missing keys: score 0, value 0
            padn = (-T) % KEY_TILE
            s = torch.cat([s, torch.zeros(B, H, T, padn, dtype=s.dtype)], -1)
            vv = torch.cat([vv, torch.zeros(B, H, padn, HEAD_DIM, dtype=s.dtype)], 2)
        if fault == "causal":
            s = s.masked_fill(torch.ones(T, s.shape[-1], dtype=torch.bool).triu(1), float("-inf"))
        e = torch.exp(s - s.amax(-1, keepdim=True))
        o = r((r(e) @ vv) / e.sum(-1, keepdim=True))
        h = h + merge(o) @ W(p + "self_attn.out_proj.weight").T + V(p + "self_attn.out_proj.bias")
        a = r(_ln(h, V(p + "final_layer_norm.weight"), V(p + "final_layer_norm.bias"), eps))
        m = r(_gelu(a @ W(p + "fc1.weight").T + V(p + "fc1.bias")))
        h = h + m @ W(p + "fc2.weight").T + V(p + "fc2.bias")
    if fault != "no_final_ln":
        h = _ln(h, V("layer_norm.weight"), V("layer_norm.bias"), eps)
    return h


def dist(a, b):
    """(max-abs, RMS) of a - b in float64"""
    e = (a.double() - b.double())
    return float(e.abs().max()), float(torch.sqrt((e * e).mean()))


def hf_config(cfg):
    """keyword arguments of a transformers WhisperConfig whose ENCODER is this config (the decoder is the smallest that constructs)"""
    return dict(num_mel_bins=cfg["n_mels"], d_model=cfg["d_model"], encoder_layers=cfg["n_layers"], encoder_attention_heads=cfg["n_heads"],
                encoder_ffn_dim=cfg["ffn_dim"], max_source_positions=cfg["n_ctx"], decoder_layers=1, decoder_attention_heads=cfg["n_heads"],
                decoder_ffn_dim=64, vocab_size=64, max_target_positions=16, activation_function="gelu", dropout=0.0, attention_dropout=0.0,
                activation_dropout=0.0, pad_token_id=0, bos_token_id=1, eos_token_id=2, decoder_start_token_id=1)
