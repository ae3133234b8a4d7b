"""The Whisper encoder's rule (tests/whisper_enc_ref.py, float64) against transformers: the stored fp32 output of its WhisperEncoder on the
fixture's seeded weights and features (tests/golden/whisper_enc.pt, tools/whisper_enc_golden.py) and, where transformers imports, a live
one.  And the grading of the bound the device is held to (tests/test_whisper_enc_gpu.py): with G_i the distance of transformers' own fp16
encoder from the rule, the rounded emulation of the device's arithmetic lies inside G_i on both norms, and every fault of the list moves the
rule by at least 8 G_i max-abs on at least one case: 4 x the device's bound of 2 G_i.

The rule sits 3e-6 .. 6e-6 from transformers' fp32 output (fp32 noise of ITS arithmetic); it is held to 1e-4: more than 10 x that, less than
G / 60.  NOT gradeable at this precision: the tanh form of GELU, which moves the output by 0.1 - 0.5 G."""
import os

import pytest
import torch

import whisper_enc_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "whisper_enc.pt")
_cache = {}


def _fixture():
    if "fix" not in _cache:
        _cache["fix"] = torch.load(GOLDEN)
    return _cache["fix"]


def _case(name):
    if name not in _cache:
        case = R.CASES[name]
        cfg = R.config_of(case)
        sd = R.make_weights(cfg, case["seed"], case["gain"])
        x = R.make_features(cfg["n_mels"], 2 * cfg["n_ctx"], case["seed"] + 1, case["live"])
        _cache[name] = (cfg, sd, x, R.forward(cfg, sd, x)[0])
    return _cache[name]


def test_the_fixture_holds_the_cases_and_is_small():
    fix = _fixture()
    assert sorted(fix["cases"]) == ["A", "B", "C"] and os.path.getsize(GOLDEN) < 1_000_000
    for name, c in fix["cases"].items():
        assert c["config"] == R.config_of(R.CASES[name]) and set(c["faults"]) == set(R.FAULTS)
        assert c["rows"].tolist() == R.stored_rows(c["config"]["n_ctx"]) and c["hf32"].shape == (len(c["rows"]), c["config"]["d_model"])
    assert 130 <= len(fix["cases"]["C"]["rows"]) <= 160


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_generated_tensors_have_the_stored_checksums(name):
    cfg, sd, x, _ = _case(name)
    assert R.checksums(cfg, sd, x) == _fixture()["cases"][name]["checksums"], "this torch's generator gives other tensors than the fixture's"


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_rule_is_within_1e_4_of_transformers_fp32(name):
    c = _fixture()["cases"][name]
    ref = _case(name)[3]
    e = R.dist(ref[c["rows"]], c["hf32"])
    print(f"\ncase {name}: rule vs stored transformers fp32: max-abs {e[0]:.3e}, RMS {e[1]:.3e}")
    assert e[0] <= 1e-4


@pytest.mark.parametrize("name", ["A", "B"])
def test_rule_is_within_1e_4_of_a_live_transformers_encoder(name):
    transformers = pytest.importorskip("transformers")
    cfg, sd, x, ref = _case(name)
    enc = transformers.WhisperForConditionalGeneration(transformers.WhisperConfig(**R.hf_config(cfg))).eval().get_encoder()
    enc.load_state_dict(sd, strict=True)
    with torch.inference_mode():
        got = enc(x[None]).last_hidden_state[0]
    assert R.dist(ref, got)[0] <= 1e-4


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_rounded_emulation_lies_inside_G(name):
    c = _fixture()["cases"][name]
    Rr, G = c["R"], c["G"]
    if name != "C":                                                         # the small cases are recomputed, the long one is the tool's
        cfg, sd, x, ref = _case(name)
        Rr = R.dist(ref, R.forward(cfg, sd, x, rounded=True)[0])
        assert Rr == pytest.approx(c["R"], rel=1e-6)
    print(f"\ncase {name}: R / G = {Rr[0] / G[0]:.2f} max-abs, {Rr[1] / G[1]:.2f} RMS; bf16 G / fp16 G = {c['Gb'][0] / G[0]:.1f}")
    assert Rr[0] <= G[0] and Rr[1] <= G[1]


@pytest.mark.parametrize("fault", R.FAULTS)
def test_every_fault_lies_8_G_out_on_some_case(fault):
    fix = _fixture()["cases"]
    ratios = {}
    for name in ("A", "B", "C"):
        d = fix[name]["faults"][fault]
        if name != "C":
            cfg, sd, x, ref = _case(name)
            d = R.dist(ref, R.forward(cfg, sd, x, fault=fault)[0])
            assert d == pytest.approx(fix[name]["faults"][fault], rel=1e-6)
        ratios[name] = d[0] / fix[name]["G"][0]
    print(f"\n{fault}: " + ", ".join(f"{k} {v:.1f} G" for k, v in ratios.items()))
    assert max(ratios.values()) >= 8.0, ratios


def test_the_key_tail_faults_are_graded_by_the_short_cases():
    """n_ctx = 100 leaves a key tile of 4: dropping it, or counting its 28 missing keys as score 0, is far outside the bound on A or B, while
    1500 = 46 x 32 + 28 hides both in a sum over 1500 keys."""
    fix = _fixture()["cases"]
    for fault in ("key_tail_dropped", "key_tail_zero"):
        assert max(fix[n]["faults"][fault][0] / fix[n]["G"][0] for n in ("A", "B")) >= 8.0


def test_rounded_mode_rounds_and_default_does_not():
    cfg, sd, x, ref = _case("A")
    assert ref.dtype == torch.float64 and not torch.equal(ref, R.forward(cfg, sd, x, rounded=True)[0])
    both = R.forward(cfg, sd, torch.stack([x, x.flip(1)]))
    assert both.shape == (2, cfg["n_ctx"], cfg["d_model"]) and R.dist(both[0], ref)[0] < 1e-12
