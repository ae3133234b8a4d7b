"""Writes tests/golden/mel.pt: what transformers' ``WhisperFeatureExtractor`` gives the seeded inputs of tests/mel_ref.py
(``GOLDEN_INPUTS``), so that the GPU tests can hold the device to the extractor on a machine without transformers.  Per input: generator
name, seed, length, format, n_mels; the extractor's features at ``golden_frames`` (every live frame; a subset for the three 30 s clips,
to keep the file small) and the constant that fills the frames behind the clip; E_i = max |extractor - mel_ref| over ALL frames.
Run on the CPU:  python tools/mel_golden.py [--check]   (--check: compare with the stored file instead of writing)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mel_ref  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "mel.pt")


def extractor_features(x, n_mels):
    from transformers import WhisperFeatureExtractor
    fe = WhisperFeatureExtractor(feature_size=n_mels)
    wav = x.astype(np.float32) / 32768.0 if x.dtype == np.int16 else x
    return fe(wav, sampling_rate=16000, return_tensors="np").input_features[0].astype(np.float32)


def build():
    items = []
    for name, seed, length, n_mels in mel_ref.GOLDEN_INPUTS:
        x = mel_ref.signal(name, seed, length)
        got = extractor_features(x, n_mels)
        ref = mel_ref.log_mel(x, n_mels)
        frames = mel_ref.golden_frames(length)
        live = mel_ref.frames_needed(min(length, mel_ref.CAP), True)
        const = got[:, live:]
        assert live == mel_ref.FRAMES or float(np.abs(const - const.flat[0]).max()) == 0.0, "the frames behind the clip are not constant"
        items.append({"name": name, "seed": seed, "length": length, "fmt": "int16" if x.dtype == np.int16 else "fp32", "n_mels": n_mels,
                      "frames": torch.from_numpy(frames.astype(np.int32)), "features": torch.from_numpy(np.ascontiguousarray(got[:, frames])),
                      "constant": float(const.flat[0]) if live < mel_ref.FRAMES else float("nan"), "live": live,
                      "E": float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max())})
        print(f"{name:22s} seed {seed} L {length:6d} n_mels {n_mels:3d} live {live:4d} stored {len(frames):4d}  E_i = {items[-1]['E']:.3e}")
    return {"inputs": items, "E": max(it["E"] for it in items)}


if __name__ == "__main__":
    fix = build()
    print(f"E = {fix['E']:.3e}")
    if "--check" in sys.argv:
        old = torch.load(PATH)
        assert all(torch.equal(a["features"], b["features"]) for a, b in zip(old["inputs"], fix["inputs"])), "the extractor moved"
        print("the stored fixture regenerates")
    else:
        torch.save(fix, PATH)
        print(PATH, os.path.getsize(PATH), "bytes")
