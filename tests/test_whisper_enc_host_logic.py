"""The Whisper encoder's host side without a GPU: what ``mimi_wenc_create`` refuses before any device call (include/mimi_hip.h), the mapping
of a transformers state dict onto the C weights (sesameai/whisper_enc.py), and ``WhisperSTT(encoder=)`` against recording fakes
(sesameai/stt.py).  A refusal that had touched the device would come back as -2 with HIP's text on a box without one, not as -1 with ours."""
import ctypes as C
import sys
import types

import pytest
import torch

import whisper_enc_ref as R

CFG = R.config_of(R.CASES["A"])
_cache = {}


def _weights():
    if "sd" not in _cache:
        _cache["sd"] = R.make_weights(CFG, 3, 1.0)
    return _cache["sd"]


def _create(cfg, sd, max_batch=1):
    from sesameai import _abi
    from sesameai.whisper_enc import WencConfig, map_state_dict
    w, keep = map_state_dict(cfg, sd)
    c = WencConfig(**{k: (float(cfg[k]) if k == "ln_eps" else int(cfg[k])) for k in R.CONFIG_KEYS})
    h = C.c_void_p(None)
    rc = _abi.lib.mimi_wenc_create(C.byref(c), C.byref(w), max_batch, C.byref(h))
    msg = (_abi.lib.mimi_wenc_last_error(None) or b"").decode()
    if rc == 0:
        _abi.lib.mimi_wenc_destroy(h)
    return rc, msg


@pytest.mark.parametrize("change, max_batch, text", [
    (dict(n_heads=3), 1, "head dim"), (dict(d_model=96, n_heads=2), 1, "head dim"), (dict(n_ctx=1501), 1, "n_ctx"), (dict(n_ctx=0), 1, "n_ctx"),
    (dict(n_mels=64), 1, "n_mels"), (dict(n_mels=127), 1, "n_mels"), ({}, 0, "max_batch"), ({}, 65, "max_batch"),
    (dict(ffn_dim=500), 1, "ffn_dim"), (dict(ln_eps=0.0), 1, "ln_eps")])
def test_create_refuses_bad_dims_without_a_device_call(change, max_batch, text):
    rc, msg = _create({**CFG, **change}, _weights(), max_batch)
    assert rc == -1 and text in msg, (rc, msg)


@pytest.mark.parametrize("name, value, text", [("layers.1.fc1.weight", 1e6, "does not fit fp16"), ("conv2.weight", -7e4, "does not fit fp16"),
                                               ("layers.0.self_attn.q_proj.weight", float("nan"), "does not fit fp16"),
                                               ("layers.0.fc2.bias", float("inf"), "not finite")])
def test_create_refuses_a_weight_fp16_cannot_hold_and_names_it(name, value, text):
    sd = dict(_weights())
    sd[name] = sd[name].clone()
    sd[name].view(-1)[5] = value
    rc, msg = _create(CFG, sd)
    assert rc == -1 and name in msg and text in msg, (rc, msg)


def test_create_refuses_null_pointers():
    from sesameai import _abi
    from sesameai.whisper_enc import WencConfig, WencWeights
    h = C.c_void_p(None)
    assert _abi.lib.mimi_wenc_create(None, None, 1, C.byref(h)) == -1 and b"null" in _abi.lib.mimi_wenc_last_error(None)
    c, w = WencConfig(**{**CFG, "ln_eps": 1e-5}), WencWeights()
    w.host = 1
    assert _abi.lib.mimi_wenc_create(C.byref(c), C.byref(w), 1, C.byref(h)) == -1
    assert b"null pointer: conv1.weight" in _abi.lib.mimi_wenc_last_error(None)
    assert _abi.lib.mimi_wenc_encode(None, None, 1, None, 0, None) == -1 and _abi.lib.mimi_wenc_describe(None, 1, None, 0) == -1


def _tiny_model():
    """a transformers model of case A's encoder where it imports, else an object with the same surface: get_encoder().state_dict(), config"""
    try:
        import transformers
        torch.manual_seed(1)
        return transformers.WhisperForConditionalGeneration(transformers.WhisperConfig(**R.hf_config(CFG))).eval()
    except ImportError:
        sd = _weights()
        enc = types.SimpleNamespace(state_dict=lambda: sd)
        k = R.hf_config(CFG)
        return types.SimpleNamespace(get_encoder=lambda: enc, config=types.SimpleNamespace(**k))


def test_from_model_maps_the_state_dict_and_the_config():
    from sesameai.whisper_enc import LAYER_NAMES, TOP_NAMES, config_from_model, map_state_dict
    model = _tiny_model()
    cfg = config_from_model(model)
    assert cfg == CFG
    sd = model.get_encoder().state_dict()
    assert set(sd) == {n for n, _, _ in R.weight_names(CFG)}, "the rule's names are the state dict's"
    assert not any(k.endswith("k_proj.bias") for k in sd)
    w, keep = map_state_dict(cfg, sd)
    assert w.host == 1 and len(keep) == len(TOP_NAMES) + CFG["n_layers"] * len(LAYER_NAMES) == len(sd)
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in keep)
    assert w.conv1_w == sd["conv1.weight"].data_ptr() and w.embed_positions == sd["embed_positions.weight"].data_ptr()
    assert w.layers[1].k_w == sd["layers.1.self_attn.k_proj.weight"].data_ptr() and w.layers[1].fc2_b == sd["layers.1.fc2.bias"].data_ptr()
    assert w.layers[0].q_b == sd["layers.0.self_attn.q_proj.bias"].data_ptr() and not w.layers[2].q_w          # layers past L stay null
    half = {k: v.half() for k, v in sd.items()}                                 # a checkpoint in fp16: converted copies are kept alive
    w16, keep16 = map_state_dict(cfg, half)
    assert w16.layers[0].v_w == keep16[len(TOP_NAMES) + list(LAYER_NAMES).index("v_w")].data_ptr()
    with pytest.raises(ValueError, match="no bias on k_proj"):
        map_state_dict(cfg, {**sd, "layers.0.self_attn.k_proj.bias": torch.zeros(CFG["d_model"])})
    lacking = dict(sd)
    del lacking["layers.1.fc1.bias"]
    with pytest.raises(KeyError, match="layers.1.fc1.bias"):
        map_state_dict(cfg, lacking)


class _FakeModel:
    dtype = torch.float16

    def __init__(self):
        self.calls = []

    def generate(self, **kw):
        self.calls.append(kw)
        x = kw["input_features"] if "input_features" in kw else kw["encoder_outputs"].last_hidden_state
        return torch.arange(x.shape[0])[:, None]


class _FakeTok:
    def batch_decode(self, ids, skip_special_tokens=True):
        assert skip_special_tokens
        return [f" turn {int(i)} " for i in ids[:, 0]]


class _FakeEncoder:
    max_batch = 2

    def __init__(self):
        self.calls = []

    def encode(self, feats):
        self.calls.append(feats)
        return feats.sum(1, keepdim=True).float() + torch.arange(4.0)[None, :, None]       # (B, 4, T): any tensor of its own


def _base_model_output(monkeypatch):
    try:
        from transformers.modeling_outputs import BaseModelOutput
    except ImportError:                                                         # the adapter imports it lazily: give it the same surface
        class BaseModelOutput:
            def __init__(self, last_hidden_state=None):
                self.last_hidden_state = last_hidden_state
        mod = types.ModuleType("transformers.modeling_outputs")
        mod.BaseModelOutput = BaseModelOutput
        monkeypatch.setitem(sys.modules, "transformers", types.ModuleType("transformers"))
        monkeypatch.setitem(sys.modules, "transformers.modeling_outputs", mod)
    return BaseModelOutput


def test_stt_with_an_encoder_hands_generate_its_output_and_never_the_features(monkeypatch):
    from sesameai.stt import WhisperSTT
    BaseModelOutput = _base_model_output(monkeypatch)
    model, enc = _FakeModel(), _FakeEncoder()
    stt = WhisperSTT(model, _FakeTok(), encoder=enc, max_new_tokens=7)
    f = torch.rand(80, 3000)
    assert stt(f, 120) == "turn 0"
    (kw,) = model.calls
    assert set(kw) == {"encoder_outputs", "max_new_tokens"} and kw["max_new_tokens"] == 7
    assert isinstance(kw["encoder_outputs"], BaseModelOutput)
    h = kw["encoder_outputs"].last_hidden_state
    assert h.dtype == torch.float16 and torch.equal(h, enc.encode(f[None]).to(torch.float16))
    # five turns through an encoder of max_batch 2: three encodes and three generates, texts in order
    model.calls.clear(); enc.calls.clear()
    turns = [(torch.rand(80, 3000), 10 * k) for k in range(5)]
    assert stt.transcribe_many(turns) == ["turn 0", "turn 1", "turn 0", "turn 1", "turn 0"]
    assert [c.shape[0] for c in enc.calls] == [2, 2, 1] and len(model.calls) == 3
    assert torch.equal(enc.calls[1][1], turns[3][0]) and all("input_features" not in c for c in model.calls)
    with pytest.raises(ValueError):
        WhisperSTT(model, _FakeTok(), encoder="host")


def test_stt_without_an_encoder_calls_generate_with_the_features_as_before():
    from sesameai.stt import WhisperSTT
    model = _FakeModel()
    stt = WhisperSTT(model, _FakeTok(), num_beams=1)
    assert stt.encoder is None
    f = torch.rand(80, 3000)
    assert stt(f, 55) == "turn 0"
    (kw,) = model.calls
    assert set(kw) == {"input_features", "num_beams"} and kw["input_features"].dtype == torch.float16
    assert torch.equal(kw["input_features"], f[None].to(torch.float16))
    assert stt.transcribe_many([(f, 1), (f, 2)]) == ["turn 0", "turn 0"] and len(model.calls) == 3
    with pytest.raises(AssertionError):
        stt(torch.rand(80, 2999))
