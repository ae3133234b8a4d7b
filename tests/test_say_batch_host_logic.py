"""``TTS.say`` / ``TTS.export_wav`` with ``batch=`` on a scripted generator whose requests complete in scrambled order: the reorder buffer, the
fallback for a sentence whose prompt cannot be built, the prompts, seeds and finishing parameters handed to ``Generator.generate_segments``,
the voice prefix registered once per loaded voice, and -- with ``batch=None`` -- none of it.  No GPU."""
import importlib.util
import os
import wave

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _module():
    spec = importlib.util.spec_from_file_location("tts_service_say_batch", os.path.join(ROOT, "sesameai-tts_amd", "tts_service.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    return mod


class Gen:
    """Scripted: request k of a generate_segments call completes in the order ``self.order`` says and is (100 * (k + 1) + lead + tail,) int16 of
    value k + 1.  The unbatched entry points are scripted too, and everything is counted."""
    sample_rate, device = 24_000, torch.device("cpu")

    def __init__(self, max_batch=4, order=None):
        self._max_batch, self.order = max_batch, order
        self.segment_calls, self.prefix_calls, self.dropped, self.codes_calls = [], [], [], 0

    def _tokenize_text_segment(self, text, speaker):
        if "boom" in text:
            raise RuntimeError("scripted failure")
        n = len(text.split())
        return torch.full((n, 33), float(n)).long(), torch.ones(n, 33).bool()

    def cache_prefix(self, tokens, mask):
        self.prefix_calls.append((tokens.clone(), mask.clone()))
        return ("handle", len(self.prefix_calls))

    def drop_prefix(self, handle):
        self.dropped.append(handle)

    def generate_segments(self, prompts, max_generation_len, temperature, topk, finish, seed=None, refill_group=1, post=None, on_result=None, slots=None):
        self.segment_calls.append(dict(prompts=prompts, limit=max_generation_len, temperature=temperature, topk=topk, finish=finish, seed=seed,
                                       post=post, slots=slots))
        lead, tail, _ = finish.samples(self.sample_rate)
        out = [torch.full((100 * (k + 1) + lead + tail,), k + 1, dtype=torch.int16) for k in range(len(prompts))]
        for k in (self.order or range(len(prompts))):
            on_result(k, out[k])
        return out

    def generate_codes(self, t, m, n, temp, topk):
        self.codes_calls += 1
        return torch.ones(5, 1, 32, dtype=torch.int32)

    def _decode_frames(self, fr):
        return torch.linspace(-1, 1, fr.shape[0] * 1920)


def _tts(gen):
    tts = _module().TTS(voice_dir="/nonexistent")
    tts.generator, tts.watermarker = gen, None
    tts.cached_context_tokens, tts.cached_context_masks = [torch.full((7, 33), 9).long()], [torch.ones(7, 33).bool()]
    return tts


TEXT = "One. Two words! This one goes boom. Now four words here? Five words are in this."


def test_say_batch_hands_segments_out_in_sentence_order(tmp_path, capsys):
    gen = Gen(order=[3, 1, 0, 2])                      # the four prompts that can be built complete scrambled
    tts = _tts(gen)
    got = []
    out = tmp_path / "say.wav"
    tts.say(TEXT, output_filename=str(out), on_segment=lambda pcm, sr: got.append((len(pcm), int(pcm[0]) if len(pcm) else None, sr)),
            batch=3, seed=40, start_silence_duration=0, end_silence_duration=0, fade_duration=0, fallback_duration=250)
    printed = capsys.readouterr().out
    # request k is sentence owner[k]: sentences 0, 1, 3, 4; sentence 2 got 250 ms of silence
    assert got == [(100, 1, 24_000), (200, 2, 24_000), (6000, 0, 24_000), (300, 3, 24_000), (400, 4, 24_000)]
    lines = [ln for ln in printed.splitlines() if ln.startswith("> ")]
    assert [ln.split(" ... ")[0] for ln in lines] == ["> One.", "> Two words!", "> Now four words here?", "> Five words are in this."]
    assert all("[Audio: " in ln and "RTF: " in ln for ln in lines)
    assert "Error generating audio for sentence: This one goes boom.: scripted failure" in printed
    last = [ln for ln in printed.splitlines() if ln.startswith("Batch of 5 sentences: ")]
    assert len(last) == 1 and "s of audio in " in last[0] and "RTF: " in last[0]
    with wave.open(str(out), "rb") as f:
        assert (f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()) == (1, 2, 24_000, 100 + 200 + 6000 + 300 + 400)
        data = np.frombuffer(f.readframes(f.getnframes()), dtype="<i2")
    assert data[:100].tolist() == [1] * 100 and data[300:6300].tolist() == [0] * 6000 and data[-400:].tolist() == [4] * 400
    # ONE batched call: the four prompts = context + sentence, the 30 s limit, seed + sentence index, the finishing parameters, no post hook
    assert len(gen.segment_calls) == 1 and gen.codes_calls == 0
    call = gen.segment_calls[0]
    assert [t.shape[0] for t, _ in call["prompts"]] == [7 + 1, 7 + 2, 7 + 4, 7 + 5]
    assert all(torch.equal(t[:7], tts.cached_context_tokens[0]) and t.dtype == torch.long and m.dtype == torch.bool for t, m in call["prompts"])
    assert call["limit"] == 375 and call["seed"] == [40, 41, 43, 44] and call["slots"] == 3 and call["post"] is None
    assert (call["temperature"], call["topk"]) == (0.8, 40)
    assert call["finish"] == __import__("sesameai.finish", fromlist=["SegmentFinish"]).SegmentFinish(0, 0, 0)


def test_a_result_is_held_back_until_every_earlier_sentence_is_out():
    events = []

    class Spy(Gen):
        def generate_segments(self, prompts, *a, on_result=None, **kw):
            def spy(k, pcm):
                events.append(("done", k))
                on_result(k, pcm)
            return super().generate_segments(prompts, *a, on_result=spy, **kw)

    tts = _tts(Spy(order=[2, 0, 1]))
    tts.say("A. B b. C c c.", output_filename=None, on_segment=lambda pcm, sr: events.append(("out", int(pcm[-1]))), batch=2,
            start_silence_duration=0, end_silence_duration=0, fade_duration=0)
    assert events == [("done", 2), ("done", 0), ("out", 1), ("done", 1), ("out", 2), ("out", 3)]


def test_the_voice_prefix_is_registered_once_and_dropped_with_the_voice(capsys):
    gen = Gen()
    tts = _tts(gen)
    tts.say("One. Two words.", output_filename=None, batch=2)
    tts.say("Again. And again.", output_filename=None, batch=4)
    assert len(gen.prefix_calls) == 1 and gen.prefix_calls[0][0].shape == (7, 33) and gen.prefix_calls[0][1].dtype == torch.bool
    mod_tts = tts
    mod_tts.voices = {"bob": {}}
    mod_tts._prepare_context = lambda: None
    mod_tts.generate_audio_segment = lambda *a, **k: None          # (load_voice's warm-up sentence)
    mod_tts.load_voice("bob")
    assert gen.dropped == [("handle", 1)] and tts._voice_prefix is None
    capsys.readouterr()


def test_seed_none_and_default_finish(capsys):
    gen = Gen()
    tts = _tts(gen)
    tts.say("One. Two words.", output_filename=None, batch=2)
    call = gen.segment_calls[0]
    assert call["seed"] is None and call["finish"].samples(24_000) == (12000, 2400, 1200)
    capsys.readouterr()


def test_watermarker_becomes_the_post_hook(capsys):
    gen = Gen()
    tts = _tts(gen)
    tts.watermarker = object()
    tts.say("One. Two words.", output_filename=None, batch=2)
    assert callable(gen.segment_calls[0]["post"])
    capsys.readouterr()


def test_export_wav_batch(tmp_path, capsys):
    gen = Gen(order=[1, 0])
    tts = _tts(gen)
    out = tmp_path / "x.wav"
    tts.export_wav("One. This one goes boom. Two words.", str(out), batch=4, seed=5, fallback_duration=100)
    printed = capsys.readouterr().out
    assert "Export complete:" in printed and "Attempt" not in printed          # max_retries is the unbatched path's
    with wave.open(str(out), "rb") as f:
        assert (f.getnchannels(), f.getsampwidth(), f.getframerate()) == (1, 2, 24_000)
        assert f.getnframes() == (100 + 14400) + 2400 + (200 + 14400)
    assert gen.segment_calls[0]["seed"] == [5, 7] and gen.segment_calls[0]["slots"] == 4 and gen.codes_calls == 0


def test_batch_none_calls_nothing_of_the_new_path(tmp_path, capsys):
    gen = Gen()
    tts = _tts(gen)
    tts.say("One. Two words.", output_filename=None)
    tts.export_wav("One. Two words.", str(tmp_path / "y.wav"))
    assert gen.segment_calls == [] and gen.prefix_calls == [] and gen.codes_calls == 4 and tts._voice_prefix is None
    capsys.readouterr()


@pytest.mark.parametrize("batch", [0, 1, 5, -2, 2.0, True])
def test_batch_out_of_range_raises(batch, tmp_path):
    gen = Gen(max_batch=4)
    tts = _tts(gen)
    with pytest.raises(ValueError, match="batch must be None or 2 .. 4"):
        tts.say("One. Two words.", output_filename=None, batch=batch)
    with pytest.raises(ValueError, match="batch must be None or 2 .. 4"):
        tts.export_wav("One. Two words.", str(tmp_path / "z.wav"), batch=batch)
    assert gen.segment_calls == [] and gen.prefix_calls == []


def test_seed_without_batch_raises(tmp_path):
    tts = _tts(Gen())
    with pytest.raises(ValueError, match="seed= needs batch="):
        tts.say("One.", output_filename=None, seed=3)
    with pytest.raises(ValueError, match="seed= needs batch="):
        tts.export_wav("One.", str(tmp_path / "z.wav"), seed=3)


def test_an_error_of_the_batch_run_propagates(tmp_path):
    class Broken(Gen):
        def generate_segments(self, *a, **k):
            raise RuntimeError("the device fell over")

    tts = _tts(Broken())
    with pytest.raises(RuntimeError, match="the device fell over"):
        tts.export_wav("One. Two words.", str(tmp_path / "z.wav"), batch=2, max_retries=5)


def test_max_batch_size_is_passed_on_to_load_csm_1b(monkeypatch, capsys):
    mod = _module()
    calls = []
    monkeypatch.setattr(mod, "load_csm_1b", lambda *a, **k: calls.append((a, k)) or Gen())
    monkeypatch.setattr(mod, "load_watermarker", lambda device: None)
    mod.TTS(voice_dir="/nonexistent").load_model()
    mod.TTS(voice_dir="/nonexistent", max_batch_size=8).load_model()
    assert calls == [(("cuda",), {}), (("cuda",), {"max_batch_size": 8})]
    capsys.readouterr()
