"""The device's Whisper encoder (include/mimi_hip.h mimi_wenc_*, sesameai/whisper_enc.py) against the rule (tests/whisper_enc_ref.py,
float64) and against what transformers' WhisperEncoder gave the same seeded weights and features (tests/golden/whisper_enc.pt,
tools/whisper_enc_golden.py).  transformers is not needed here but for the last test.

The bound.  G_i is the distance of transformers' OWN fp16 encoder from the float64 rule on case i's weights and input, max-abs and RMS.  The
rounded emulation of the device's rule lies at 0.39 - 0.70 G max-abs (R_i in the fixture), and the device differs from the emulation only by
fp32 accumulation order and ulp-level erff / expf; it is held to 2 G_i on both norms against the rule, and to 2 G_i + 1e-4 against the
stored transformers fp32 output (1e-4: the rule's own distance from it, bounded in tests/test_whisper_enc_oracle.py).  Every gradeable fault
lies at 8 G_i or more on at least one case (same file).  NOT gradeable at this precision: the tanh form of GELU (0.1 - 0.5 G); erff is a
requirement checked by reading.  Company, position and repetition are torch.equal throughout."""
import os

import pytest
import torch

import whisper_enc_ref as R

pytestmark = pytest.mark.gpu
_cache = {}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "whisper_enc.pt")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _fixture():
    if "fix" not in _cache:
        _cache["fix"] = torch.load(GOLDEN)
    return _cache["fix"]


def _case(name):
    """(config, weights, features, the rule's output (n_ctx, d) float64) of a case, each made once"""
    if ("case", name) not in _cache:
        case, stored = R.CASES[name], _fixture()["cases"][name]
        cfg = R.config_of(case)
        assert cfg == stored["config"] and case["seed"] == stored["seed"]
        sd = R.make_weights(cfg, case["seed"], case["gain"])
        x = R.make_features(cfg["n_mels"], 2 * cfg["n_ctx"], case["seed"] + 1, case["live"])
        assert R.checksums(cfg, sd, x) == stored["checksums"], "this torch's generator gives other tensors than the fixture's: regenerate it"
        _cache[("case", name)] = (cfg, sd, x, R.forward(cfg, sd, x)[0])
    return _cache[("case", name)]


def _encoder(name, max_batch=1):
    from sesameai.whisper_enc import WhisperEncoder
    if ("enc", name, max_batch) not in _cache:
        cfg, sd, _, _ = _case(name)
        _cache[("enc", name, max_batch)] = WhisperEncoder(cfg, sd, max_batch=max_batch)
    return _cache[("enc", name, max_batch)]


def _alone(name):
    """the device's B = 1 output of a case's features, fp32 on the CPU, computed once"""
    if ("alone", name) not in _cache:
        _cache[("alone", name)] = _encoder(name).encode(_case(name)[2])[0].cpu()
    return _cache[("alone", name)]


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_device_is_within_2G_of_the_rule_and_of_transformers(name):
    _need_gpu()
    cfg, sd, x, ref = _case(name)
    stored = _fixture()["cases"][name]
    got = _alone(name)
    assert got.shape == (cfg["n_ctx"], cfg["d_model"]) and bool(torch.isfinite(got).all())
    G, rows = stored["G"], stored["rows"]
    e_ref, e_hf = R.dist(got, ref), R.dist(got[rows], stored["hf32"])
    e_rnd = R.dist(got, R.forward(cfg, sd, x, rounded=True)[0])
    print(f"\ncase {name}: G = ({G[0]:.3e}, {G[1]:.3e}); device vs rule ({e_ref[0]:.3e}, {e_ref[1]:.3e}) = ({e_ref[0] / G[0]:.2f}, {e_ref[1] / G[1]:.2f}) G;"
          f" vs transformers fp32 ({e_hf[0]:.3e}, {e_hf[1]:.3e}); vs rounded emulation ({e_rnd[0]:.3e}, {e_rnd[1]:.3e})")
    assert e_ref[0] <= 2 * G[0] and e_ref[1] <= 2 * G[1], (e_ref, G)
    assert e_hf[0] <= 2 * G[0] + 1e-4 and e_hf[1] <= 2 * G[1] + 1e-4, (e_hf, G)


def _company_inputs():
    cfg = _case("A")[0]
    m, T = cfg["n_mels"], 2 * cfg["n_ctx"]
    return [R.make_features(m, T, 11, 0), R.make_features(m, T, 12, T), R.make_features(m, T, 13, 90, kind="int"),
            R.make_features(m, T, 14, 120), R.make_features(m, T, 15, 33)]


def test_a_clip_has_the_same_bits_alone_and_in_any_company():
    _need_gpu()
    xs = _company_inputs()
    one, five = _encoder("A"), _encoder("A", 5)
    alone = [one.encode(x)[0].clone() for x in xs]
    assert not torch.equal(alone[0], alone[1]) and all(bool(torch.isfinite(a).all()) for a in alone)
    both = five.encode(torch.stack(xs)).clone()
    for i in range(5):
        assert torch.equal(both[i], alone[i]), f"clip {i} differs in a batch of 5"
    order = [3, 0, 4, 2, 1]
    shuffled = five.encode(torch.stack([xs[i] for i in order]))
    for at, i in enumerate(order):
        assert torch.equal(shuffled[at], alone[i]), f"clip {i} differs at place {at}"
    assert torch.equal(five.encode(torch.stack(xs)), both), "a second call differs"
    for b in (2, 3):                                                          # a batch smaller than the handle's
        part = five.encode(torch.stack(xs[:b]))
        assert all(torch.equal(part[i], alone[i]) for i in range(b))
    from sesameai.whisper_enc import WhisperEncoder
    cfg, sd, _, _ = _case("A")
    second = WhisperEncoder(cfg, sd, max_batch=5)
    assert torch.equal(second.encode(torch.stack(xs)), both), "a second handle differs"
    for dt in (torch.float16, torch.bfloat16):
        assert torch.equal(five.encode(torch.stack(xs), dtype=dt), both.to(dt)), dt


def test_the_tile_shape_a_launch_picks_does_not_move_a_bit():
    """Case C alone runs every GEMM on 64-row tiles (too few workgroups otherwise); in a batch of three, q|k|v and fc1 go to 128-row tiles
    and the others stay.  Same bits: an element's K chain is the same in both."""
    _need_gpu()
    cfg, _, x, _ = _case("C")
    enc = _encoder("C", 3)
    assert "tile 128x128" not in enc.describe(1) and "tile 128x128" in enc.describe(3) and "tile  64x128" in enc.describe(3)
    x2 = R.make_features(cfg["n_mels"], 2 * cfg["n_ctx"], 77, 2000)
    got = enc.encode(torch.stack([x, x2, x])).cpu()
    assert torch.equal(got[0], _alone("C")) and torch.equal(got[2], _alone("C")) and not torch.equal(got[1], got[0])


def test_a_nan_stays_inside_its_clip():
    _need_gpu()
    xs = _company_inputs()
    five = _encoder("A", 5)
    clean = five.encode(torch.stack(xs)).clone()
    bad = [x.clone() for x in xs]
    bad[2][17, 41] = float("nan")
    got = five.encode(torch.stack(bad)).clone()
    assert bool(torch.isnan(got[2]).all()), "the clip that read a NaN must be NaN"
    for i in (0, 1, 3, 4):
        assert torch.equal(got[i], clean[i]), f"clip {i} was moved by another clip's NaN"
    assert torch.equal(five.encode(torch.stack(xs)), clean), "the handle's next call was moved"


def test_whisper_stt_hands_generate_the_device_encoder_output():
    """A seeded tiny WhisperForConditionalGeneration of case A's shape with transformers' own initialisation (weights of std 0.02, far smaller
    than the fixture's: its fp16 error is no larger), so the bound is case A's 2 G + 1e-4 against ``model.get_encoder()`` in fp32.  Token
    ids of a random-weight model are not asserted: their margins are not controlled."""
    _need_gpu()
    transformers = pytest.importorskip("transformers")
    from sesameai.stt import WhisperSTT
    cfg = _case("A")[0]
    torch.manual_seed(5)
    model = transformers.WhisperForConditionalGeneration(transformers.WhisperConfig(**R.hf_config(cfg))).eval().cuda()
    seen = []
    real = model.generate

    def generate(**kw):
        seen.append(kw)
        return real(**kw)

    model.generate = generate

    class Tok:
        def batch_decode(self, ids, skip_special_tokens=True):
            return [" text "] * int(ids.shape[0])

    stt = WhisperSTT(model, Tok(), encoder="device", max_batch=3, max_new_tokens=2)
    xs = [x.cuda() for x in _company_inputs()[2:5]]
    G = _fixture()["cases"]["A"]["G"]
    singles = []
    for x in xs:
        assert stt(x, 100) == "text"
        kw = seen[-1]
        assert "input_features" not in kw
        h = kw["encoder_outputs"].last_hidden_state
        with torch.inference_mode():
            want = model.get_encoder()(x[None]).last_hidden_state
        e = R.dist(h.cpu(), want.cpu())
        print(f"\nstt: device encoder vs model.get_encoder(): ({e[0]:.3e}, {e[1]:.3e})")
        assert e[0] <= 2 * G[0] + 1e-4 and e[1] <= 2 * G[1] + 1e-4, e
        singles.append(h[0].clone())
    n = len(seen)
    assert stt.transcribe_many([(x, 100) for x in xs]) == ["text"] * 3 and len(seen) == n + 1, "three turns: one generate"
    h3 = seen[-1]["encoder_outputs"].last_hidden_state
    assert all(torch.equal(h3[i], singles[i]) for i in range(3))
