"""The rule (tests/mel_ref.py) against transformers' WhisperFeatureExtractor, and against itself.  The first three checks need
transformers; the others do not.  E is the largest distance of the extractor from the rule over the fixture's inputs
(tests/golden/mel.pt, written by tools/mel_golden.py); the device is held to 2 E from the rule (tests/test_mel_gpu.py), and each of six
plausible faults in the rule moves the features by at least 20 x 2 E."""
import os
import sys

import numpy as np
import pytest
import torch

import mel_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cache = {}


def _fixture():
    if "fix" not in _cache:
        _cache["fix"] = torch.load(os.path.join(ROOT, "tests", "golden", "mel.pt"))
    return _cache["fix"]


def _golden_tool():
    pytest.importorskip("transformers")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import mel_golden
    return mel_golden


def _extractor(i):
    """the extractor's features of fixture input i, computed once"""
    if ("ext", i) not in _cache:
        name, seed, length, n_mels = R.GOLDEN_INPUTS[i]
        x = R.signal(name, seed, length)
        _cache[("ext", i)] = (x, _golden_tool().extractor_features(x, n_mels))
    return _cache[("ext", i)]


@pytest.mark.parametrize("i", range(len(R.GOLDEN_INPUTS)))
def test_the_fixture_regenerates(i):
    _golden_tool()
    it = _fixture()["inputs"][i]
    assert (it["name"], it["seed"], it["length"], it["n_mels"]) == R.GOLDEN_INPUTS[i]
    x, got = _extractor(i)
    assert (it["fmt"] == "int16") == (x.dtype == np.int16)
    assert np.array_equal(got[:, R.golden_frames(it["length"])], it["features"].numpy()), "the extractor no longer gives what is stored"
    assert np.array_equal(it["frames"].numpy(), R.golden_frames(it["length"]))
    if it["live"] < R.FRAMES:
        assert (got[:, it["live"]:] == np.float32(it["constant"])).all()


@pytest.mark.parametrize("i", range(len(R.GOLDEN_INPUTS)))
def test_the_rule_is_within_5e_5_of_the_extractor(i):
    _golden_tool()
    x, got = _extractor(i)
    d = float(np.abs(got.astype(np.float64) - R.log_mel(x, R.GOLDEN_INPUTS[i][3]).astype(np.float64)).max())
    print(f"input {i}: |extractor - mel_ref| = {d:.3e}")
    assert d <= 5e-5
    assert _fixture()["E"] == max(it["E"] for it in _fixture()["inputs"])


@pytest.mark.parametrize("n_mels", [80, 128])
def test_window_and_bank_are_the_extractors(n_mels):
    pytest.importorskip("transformers")
    from transformers.audio_utils import mel_filter_bank, window_function
    assert np.abs(R.window() - window_function(400, "hann")).max() <= 1e-12
    assert np.abs(R.bank(n_mels) - mel_filter_bank(201, n_mels, 0.0, 8000.0, 16000, "slaney", "slaney")).max() <= 1e-12


def _clip(n=6000, seed=61):
    return R.signal("speech", seed, n)


@pytest.mark.parametrize("sizes", [[1], [159], [160], [161], [4000], "random"])
def test_the_chunked_rule_equals_the_one_shot_rule(sizes):
    x = _clip(1200 if sizes == [1] else 6000)
    if sizes == "random":
        sizes = [int(v) for v in np.random.RandomState(3).randint(0, 900, size=64)]
    want = R.raw_rows(x, 80)
    s, rows, at, k = R.MelStream(80), [], 0, 0
    while at < len(x):
        b = min(len(x), at + sizes[k % len(sizes)])
        n = s.frame_count(b - at, b == len(x))
        rows.append(s.feed(x[at:b], final=b == len(x)))
        assert rows[-1].shape == (n, 80)
        at, k = b, k + 1
    got = np.concatenate(rows)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert np.array_equal(R.finish(got, 80), R.log_mel(x, 80)) and s.frames == 0 and len(s.s) == 0


def test_the_cap_and_the_counts_of_the_rule():
    assert [R.frames_needed(n, False) for n in (0, 200, 201, 359, 360, 361, 479999, 480000)] == [0, 0, 1, 1, 2, 2, 2999, 3000]
    assert [R.frames_needed(n, True) for n in (0, 1, 200, 201, 360, 361, 5000, 479801, 480000)] == [2, 2, 3, 3, 4, 4, 33, 3000, 3000]
    s = R.MelStream(80)
    x = _clip(1000)
    s.s = np.zeros(R.CAP - 600)
    s.frames = R.frames_needed(len(s.s), False)
    rows = s.feed(x)
    assert s.dropped == 400 and s.frames == 3000 and rows.shape[0] == 3000 - R.frames_needed(R.CAP - 600, False)
    assert R.log_mel(np.zeros(5), 80).min() == R.log_mel(np.zeros(5), 80).max() == -1.5


FAULTS = ["symmetric", "hop159", "zero_pad_left", "htk", "ln", "frame_max"]


@pytest.mark.parametrize("variant", FAULTS)
def test_each_fault_moves_the_rule_by_20_times_the_bound(variant):
    """The factors found are in docs/experiments/mel.md: each is the distance over 2 E."""
    E = _fixture()["E"]
    x = R.signal("speech", 11, 32000)
    moved = float(np.abs(R.log_mel(x, 80, variant).astype(np.float64) - R.log_mel(x, 80).astype(np.float64)).max())
    print(f"{variant}: moves the features by {moved:.3e} = {moved / (2 * E):.0f} x 2 E")
    assert moved >= 20 * 2 * E
