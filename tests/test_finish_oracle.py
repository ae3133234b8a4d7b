"""The finishing rule's oracle (tests/finish_ref.py) held against what it claims to be: today's ``TTS.generate_audio_segment`` (torch division on
the CPU, a float32 copy, five NumPy passes), bit for bit, on a scripted CPU generator; and its ramp formula against ``np.linspace``.  No GPU."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from finish_ref import finish_ref, finish_ref_ms, ms_to_samples, quantise, ramp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tts(audio: torch.Tensor):
    spec = importlib.util.spec_from_file_location("tts_service_finish_oracle", os.path.join(ROOT, "sesameai-tts_amd", "tts_service.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)

    class Gen:                                   # the scripted generator of tests/test_host_logic.py's say test, with seeded audio
        sample_rate, device = 24_000, torch.device("cpu")
        def _tokenize_text_segment(self, text, speaker): return torch.zeros(3, 33).long(), torch.zeros(3, 33).bool()
        def generate_codes(self, t, m, n, temp, topk): return torch.ones(5, 1, 32, dtype=torch.int32)
        def _decode_frames(self, fr): return audio

    tts = mod.TTS(voice_dir="/nonexistent")
    tts.generator, tts.watermarker = Gen(), None
    return tts


@pytest.mark.parametrize("n", [5 * 1920, 9600])
@pytest.mark.parametrize("scale", [0.2, 1.0, 3.7, 1e-3])
@pytest.mark.parametrize("ms", [(500, 100, 50), (0, 0, 0)])
def test_finish_ref_is_todays_generate_audio_segment(n, scale, ms):
    g = torch.Generator().manual_seed(1000 + n)
    audio = torch.randn(n, generator=g) * scale
    lead, tail, fade = ms
    got = _tts(audio).generate_audio_segment("hello.", fade_duration=fade, start_silence_duration=lead, end_silence_duration=tail)
    want = finish_ref_ms(audio.numpy(), lead, tail, fade, 24_000)
    assert got.dtype == np.int16 and want.dtype == np.int16
    assert np.array_equal(got, want)
    assert len(want) == n + ms_to_samples(lead, 24_000) + ms_to_samples(tail, 24_000)
    assert int(np.abs(want).max()) == 32767                      # the peak sample maps to full scale


def test_finish_ref_floor_and_empty_clip():
    z = finish_ref(np.zeros(10, np.float32), 2, 3, 0)
    assert z.shape == (15,) and not z.any()
    tiny = np.full(4, 1e-7, np.float32)                          # below the floor: divided by 1e-6, not by itself
    assert finish_ref(tiny, 0, 0, 0).tolist() == [int(np.float32(np.float32(1e-7) / np.float32(1e-6)) * np.float32(32767.0))] * 4
    e = finish_ref(np.zeros(0, np.float32), 12000, 2400, 1200)
    assert e.shape == (14400,) and not e.any()
    assert finish_ref(np.zeros(0, np.float32), 0, 0, 5).shape == (0,)


def test_finish_ref_non_finite_samples_give_zero_and_stay_out_of_the_peak():
    x = np.array([0.5, np.nan, -0.25, np.inf, 0.125, -np.inf], np.float32)
    assert finish_ref(x, 0, 0, 0).tolist() == [32767, 0, -16383, 0, 8191, 0]


@pytest.mark.parametrize("n", list(range(1, 70)) + [1199, 1200, 1201, 2400, 4800, 12000])
def test_ramp_formula_is_linspace(n):
    want = np.linspace(0.0, 1.0, n, dtype=np.float32)
    got = ramp(n)
    assert got.dtype == np.float32 and np.array_equal(got, want)


def test_reciprocal_variant_is_a_different_function():
    """The oracle tells x / peak from x * (1 / peak): the bit-exact comparisons of the device kernels are decisive for the division."""
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(300_001, generator=g) * 0.2).numpy()
    a, b = quantise(x), quantise(x, reciprocal=True)
    d = np.abs(a.astype(np.int32) - b.astype(np.int32))
    assert 0 < int((d != 0).sum()) < len(x) // 100 and int(d.max()) == 1
