"""Finished segments from the live batch, end to end on the tiny model and the tiny codec: ``Generator.generate_many(finish=)`` /
``generate_segments`` against the oracle's finish (tests/finish_ref.py) of what ``generate_many`` returns without the keyword, and
``TTS.export_wav(batch=)`` against the oracle of every sentence's decoded codes.  Requests carry seeds of their own, so their frames do not
depend on the slot they take or on the block schedule."""
import importlib.util
import os
import wave

import numpy as np
import pytest
import torch

from finish_ref import finish_ref_ms

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMITS = [3, 12, 0, 7, 5, 9]                    # frames; one request is empty before it ever holds a slot
SEEDS = [500 + i for i in range(len(LIMITS))]


@pytest.fixture(scope="module")
def setup():
    from sesameai.finish import SegmentFinish
    from sesameai.generator import Generator, Segment
    from sesameai.mimi import MimiCodec, mimi_tiny_args, synthetic_state_dict
    from sesameai.models import Model, csm_tiny_args
    codec = MimiCodec(mimi_tiny_args(), synthetic_state_dict(mimi_tiny_args(), seed=4321), max_frames=64)
    model = Model(csm_tiny_args(), None, max_frames=64, max_prefill_rows=128)
    gen = Generator(model, audio_tokenizer=codec, max_batch_size=4)
    g = torch.Generator().manual_seed(31)
    texts = [torch.randint(0, 1000, (4 + i % 5,), generator=g).tolist() for i in range(len(LIMITS))]
    ctxs = [[Segment(speaker=1, text=torch.randint(0, 1000, (3,), generator=g).tolist(), audio_codes=torch.randint(0, 2048, (32, 2 + i % 4), generator=g))]
            for i in range(len(LIMITS))]
    how = [SegmentFinish(), SegmentFinish(0, 0, 0), SegmentFinish(20, 10, 30), SegmentFinish(1, 0, 1), SegmentFinish(500, 100, 5000), SegmentFinish(0, 3, 2)]

    def many(order, **kw):
        model.seed(5)
        return gen.generate_many([texts[i] for i in order], [1] * len(order), [ctxs[i] for i in order], max_audio_length_ms=[LIMITS[i] * 80 for i in order],
                                 temperature=0.9, topk=50, seed=[SEEDS[i] for i in order], **kw)

    order = list(range(len(LIMITS)))
    plain = many(order)                                             # today's path: fp32 clips (the reference of the tests below, made once)
    fired = []
    finished = many(order, finish=how, on_result=lambda i, pcm: fired.append((i, pcm.clone())))
    torch.cuda.synchronize()
    return dict(many=many, how=how, plain=plain, finished=finished, fired=fired)


def _want(audio, f):
    return finish_ref_ms(audio.detach().cpu().numpy().reshape(-1).astype(np.float32), f.lead_ms, f.tail_ms, f.fade_ms, 24_000)


def test_generate_many_with_finish_is_the_oracle_of_generate_many(setup):
    for i, n in enumerate(LIMITS):
        assert setup["plain"][i].numel() == n * 1920, "the random tiny model is not expected to sample an all-zero frame"
        got = setup["finished"][i]
        assert got.dtype == torch.int16 and got.is_cuda and got.dim() == 1
        want = _want(setup["plain"][i], setup["how"][i])
        assert got.shape[0] == want.shape[0] and np.array_equal(got.cpu().numpy(), want), i
    empty = setup["finished"][2]                                    # no frames: lead and tail silence all the same
    assert empty.shape[0] == 24 * 20 + 24 * 10 and not bool(empty.any())


def test_on_result_fires_once_per_request(setup):
    fired = setup["fired"]
    assert sorted(i for i, _ in fired) == list(range(len(LIMITS)))
    for i, pcm in fired:
        assert torch.equal(pcm, setup["finished"][i])


def test_a_permuted_list_gives_each_prompt_the_same_segment(setup):
    order = [4, 2, 5, 0, 3, 1]
    got = setup["many"](order, finish=[setup["how"][i] for i in order])
    for k, i in enumerate(order):
        assert torch.equal(got[k], setup["finished"][i]), i


def test_one_finish_for_all_and_a_wrong_count(setup):
    from sesameai.finish import SegmentFinish
    plain = setup["many"]([0, 1])                                   # (a batch of two slots: its own reference, the arithmetic follows the batch's width)
    got = setup["many"]([0, 1], finish=SegmentFinish(10, 10, 10))
    for k in (0, 1):
        assert np.array_equal(got[k].cpu().numpy(), _want(plain[k], SegmentFinish(10, 10, 10)))
    with pytest.raises(ValueError, match="one SegmentFinish"):
        setup["many"]([0, 1], finish=[SegmentFinish()])
    with pytest.raises(ValueError, match="on_result= needs finish="):
        setup["many"]([0, 1], on_result=lambda i, p: None)


def test_post_hook_runs_between_decode_and_finish(setup):
    """``generate_segments(post=)``: the hook sees each non-empty decoded clip; what it returns is what gets finished."""
    from sesameai.finish import SegmentFinish
    from sesameai.generator import Generator
    many, seen = setup["many"], []
    real = Generator.generate_segments

    def with_post(self, *a, **kw):
        return real(self, *a, post=lambda audio: seen.append(int(audio.numel())) or audio.flip(0), **kw)

    plain = many([0, 2, 3])                                         # (a batch of three slots: its own reference)
    Generator.generate_segments = with_post
    try:
        got = many([0, 2, 3], finish=SegmentFinish(0, 0, 0))
    finally:
        Generator.generate_segments = real
    assert sorted(seen) == sorted([LIMITS[0] * 1920, LIMITS[3] * 1920])
    for k, i in enumerate([0, 2, 3]):
        assert np.array_equal(got[k].cpu().numpy(), _want(plain[k].flip(0) if LIMITS[i] else plain[k], SegmentFinish(0, 0, 0)))


def test_export_wav_batch_end_to_end_tiny(tmp_path):
    """``TTS.export_wav(text of 5 sentences, batch=4, seed=1)`` on the set-up of tests/test_mimi_gpu.py's CLI test with ``max_batch_size=4``."""
    from dataclasses import replace
    from tokenizers import Tokenizer
    from tokenizers.models import WordLevel
    from tokenizers.pre_tokenizers import Whitespace
    from sesameai.generator import Generator, load_llama3_tokenizer
    from sesameai.mimi import MimiCodec, mimi_tiny_args
    from sesameai.models import FLAVORS, Model, ModelArgs
    spec = importlib.util.spec_from_file_location("tts_service_segments", os.path.join(ROOT, "sesameai-tts_amd", "tts_service.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    codec = MimiCodec(mimi_tiny_args(), None, max_frames=400)       # a segment may run its full 30 s = 375 frames
    words = "i'm getting all warmed up for our chatting to begin hello there how are you fine thanks and what about the weather".replace("'", " ' ").split()
    vocab = {"[UNK]": 0, "<|begin_of_text|>": 1, "<|end_of_text|>": 2, "[": 3, "]": 4, "1": 5, ".": 6, "?": 7, "'": 8}
    for wd in words:
        vocab.setdefault(wd, len(vocab))
    tok = Tokenizer(WordLevel(vocab, unk_token="[UNK]")); tok.pre_tokenizer = Whitespace()
    tok.save(str(tmp_path / "tokenizer.json"))
    sr = 16000
    t = np.arange(int(0.4 * sr)) / sr
    pcm = (0.3 * np.sin(2 * np.pi * 220 * t) * 32767).astype("<i2")
    with wave.open(str(tmp_path / "prompt.wav"), "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(sr); f.writeframes(pcm.tobytes())
    (tmp_path / "samples.py").write_text(f"alice = {{{str(tmp_path / 'prompt.wav')!r}: 'hello there'}}\n")
    tts = mod.TTS(voice_dir=str(tmp_path), max_batch_size=4)
    FLAVORS["llama-tiny-bb-2k"] = replace(FLAVORS["llama-tiny-bb"], max_seq_len=2048)       # the CLI assumes 2048 positions
    model = Model(ModelArgs("llama-tiny-bb-2k", "llama-tiny-dec", 1000, 2051, 32), None, max_frames=512, max_prefill_rows=128)
    gen = tts.generator = Generator(model, audio_tokenizer=codec, text_tokenizer=load_llama3_tokenizer(str(tmp_path / "tokenizer.json")), max_batch_size=4)
    tts.watermarker = None
    tts.load_voice("alice")
    sentences = ["hello there.", "how are you?", "fine thanks.", "and what about the weather?", "hello."]
    out = str(tmp_path / "out.wav")
    tts.export_wav(" ".join(sentences), out, temperature=0.9, topk=20, batch=4, seed=1)
    assert len(gen.prefixes) == 1                                   # the voice's rows, registered once
    with wave.open(out, "rb") as f:
        assert (f.getnchannels(), f.getsampwidth(), f.getframerate()) == (1, 2, 24000)
        data = np.frombuffer(f.readframes(f.getnframes()), dtype="<i2")
    first = open(out, "rb").read()
    # every sentence's codes from the same prompts and seeds, decoded whole, finished by the oracle
    prompts = []
    for s in sentences:
        gt, gm = gen._tokenize_text_segment(s, 1)
        prompts.append((torch.cat(tts.cached_context_tokens + [gt], 0).long().to(gen.device), torch.cat(tts.cached_context_masks + [gm], 0).bool().to(gen.device)))
    frames = gen.generate_codes_continuous(prompts, 375, 0.9, 20, seed=[1 + i for i in range(len(sentences))])
    want = [finish_ref_ms(gen._decode_frames(fr.unsqueeze(1)).cpu().numpy().reshape(-1), 500, 100, 50, 24_000) if fr.shape[0]
            else finish_ref_ms(np.zeros(0, np.float32), 500, 100, 50, 24_000) for fr in frames]
    assert len(data) == sum(len(w) for w in want)
    at = 0
    for i, w in enumerate(want):
        assert np.array_equal(data[at:at + len(w)], w), i
        at += len(w)
    assert int(np.abs(data).max()) == 32767
    tts.export_wav(" ".join(sentences), out, temperature=0.9, topk=20, batch=4, seed=1)
    assert open(out, "rb").read() == first and len(gen.prefixes) == 1
    with pytest.raises(ValueError, match="batch must be None or 2 .. 4"):
        tts.export_wav("hello.", out, batch=5)
