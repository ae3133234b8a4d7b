"""Writes tests/golden/whisper_enc.pt: what transformers' WhisperEncoder gives the seeded weights and features of tests/whisper_enc_ref.py's
cases, and how far its own fp16 run, the rounded emulation of the device's rule and every fault lie from the float64 rule.  CPU only.

    python tools/whisper_enc_golden.py            # rewrite the fixture
    python tools/whisper_enc_golden.py --check    # regenerate and compare the checksums and distances with the stored file

Per case: config, seed, gain, live; a checksum of every generated tensor (a different torch's generator is then noticed, not mistaken for a
kernel fault); the stored rows and transformers' fp32 output on them; ref_vs_hf32 (max-abs, RMS); G = transformers' fp16 encoder against
the float64 rule; R = the rounded emulation against it; Gb = the same with a bf16 transformers encoder (why the rule is fp16); the distance
of every fault."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import whisper_enc_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "whisper_enc.pt")


def hf_encoder(cfg, sd, dtype):
    from transformers import WhisperConfig, WhisperForConditionalGeneration
    model = WhisperForConditionalGeneration(WhisperConfig(**R.hf_config(cfg))).eval()
    enc = model.get_encoder()
    missing = enc.load_state_dict(sd, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    return enc.to(dtype)


@torch.inference_mode()
def build():
    cases = {}
    for name, case in R.CASES.items():
        cfg = R.config_of(case)
        sd = R.make_weights(cfg, case["seed"], case["gain"])
        x = R.make_features(cfg["n_mels"], 2 * cfg["n_ctx"], case["seed"] + 1, case["live"])
        rows = R.stored_rows(cfg["n_ctx"])
        ref = R.forward(cfg, sd, x)[0]
        hf32 = hf_encoder(cfg, sd, torch.float32)(x[None]).last_hidden_state[0]
        hf16 = hf_encoder(cfg, sd, torch.float16)(x[None].half()).last_hidden_state[0]
        hfb16 = hf_encoder(cfg, sd, torch.bfloat16)(x[None].bfloat16()).last_hidden_state[0]
        entry = dict(config=cfg, seed=case["seed"], gain=case["gain"], live=case["live"], checksums=R.checksums(cfg, sd, x),
                     rows=torch.tensor(rows), hf32=hf32[rows].float().clone(), ref_vs_hf32=R.dist(ref, hf32), G=R.dist(ref, hf16),
                     Gb=R.dist(ref, hfb16), R=R.dist(ref, R.forward(cfg, sd, x, rounded=True)[0]),
                     faults={f: R.dist(ref, R.forward(cfg, sd, x, fault=f)[0]) for f in R.FAULTS})
        cases[name] = entry
        print(name, {k: entry[k] for k in ("ref_vs_hf32", "G", "Gb", "R")}, flush=True)
        print("   faults / G max-abs:", {f: round(v[0] / entry["G"][0], 1) for f, v in entry["faults"].items()}, flush=True)
    import transformers
    return dict(cases=cases, torch=str(torch.__version__), transformers=str(transformers.__version__))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    fix = build()
    if a.check:
        old = torch.load(OUT)
        for name, c in fix["cases"].items():
            o = old["cases"][name]
            assert o["checksums"] == c["checksums"], f"case {name}: the generated tensors differ from the stored checksums"
            assert torch.equal(o["hf32"], c["hf32"]) and o["G"] == c["G"] and o["R"] == c["R"], f"case {name}: stored results differ"
        print("fixture regenerates to the same checksums and results")
        return
    torch.save(fix, OUT)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
