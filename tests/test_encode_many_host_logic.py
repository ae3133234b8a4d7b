"""Prompt building with context audio (sesameai/generator.py: _encode_contexts, _build_prompts): which clips reach the codec, in which
calls, and that the prompts are those of the per-segment path.  No GPU: a scripted codec whose codes are a function of the clip."""
import copy

import pytest
import torch

from sesameai import generator as G
from sesameai.generator import Generator, Segment


def _codes_of(audio):
    """A clip's scripted codes: (32, ceil(n / 1920)), a function of its samples alone."""
    T = -(-audio.shape[-1] // 1920)
    seed = int(audio.double().abs().sum().item() * 1000) % (2 ** 31)
    return torch.randint(0, 2048, (32, T), generator=torch.Generator().manual_seed(seed))


class _SingleCodec:
    """Today's surface: encode (1, 1, n) -> (1, 32, T)."""

    def __init__(self):
        self.calls = []

    def encode(self, wav):
        assert wav.dim() == 3 and wav.shape[:2] == (1, 1)
        self.calls.append(("encode", [wav[0, 0].clone()]))
        return _codes_of(wav[0, 0]).unsqueeze(0)


class _ManyCodec(_SingleCodec):
    def encode_many(self, wavs):
        assert all(w.dim() == 1 for w in wavs)
        self.calls.append(("encode_many", [w.clone() for w in wavs]))
        return [_codes_of(w) for w in wavs]


def _gen(codec):
    gen = Generator.__new__(Generator)
    gen.device, gen._text_tokenizer, gen._audio_tokenizer = torch.device("cpu"), None, codec
    return gen


def _requests():
    g = torch.Generator().manual_seed(3)
    clip = lambda n: torch.randn(n, generator=g) * 0.3
    voice, a, b, c = clip(1920 * 2 + 5), clip(700), clip(1920), clip(1920 * 3 + 1)
    given = torch.randint(0, 2048, (32, 4), generator=g)
    contexts = [
        [Segment(0, [5, 6], audio=voice), Segment(1, [7], audio=a)],
        [Segment(0, [5, 6], audio=voice), Segment(1, [8, 9], audio_codes=given), Segment(0, [3], audio=b)],
        [Segment(2, [4], audio=c, audio_codes=given)],                        # codes given: its audio is never encoded
        [],
    ]
    texts = [[11, 12], [13], [14, 15, 16], [17]]
    return texts, [0, 1, 2, 0], contexts, [voice, a, b]


def _per_segment_prompts(texts, speakers, contexts):
    gen = _gen(_SingleCodec())
    return [gen._build_prompt(t, sp, ctx) for t, sp, ctx in zip(texts, speakers, contexts)], gen._audio_tokenizer.calls


def test_distinct_clips_reach_one_ragged_call_in_order_and_a_shared_tensor_once():
    texts, speakers, contexts, distinct = _requests()
    before = copy.deepcopy(contexts)
    codec = _ManyCodec()
    prompts = _gen(codec)._build_prompts(texts, speakers, contexts)
    assert len(codec.calls) == 1 and codec.calls[0][0] == "encode_many"
    got = codec.calls[0][1]
    assert len(got) == len(distinct) and all(torch.equal(x, y) for x, y in zip(got, distinct))
    want, single_calls = _per_segment_prompts(texts, speakers, contexts)
    assert [c[0] for c in single_calls] == ["encode"] * 4                    # today's path encodes the shared voice prompt twice
    for (t, m), (wt, wm) in zip(prompts, want):
        assert torch.equal(t, wt) and torch.equal(m, wm) and t.dtype == torch.long and m.dtype == torch.bool
    # the Segments come back as they went in: same objects, nothing filled in
    for ctx, old in zip(contexts, before):
        for seg, o in zip(ctx, old):
            assert seg.speaker == o.speaker and seg.text == o.text
            assert (seg.audio is None) == (o.audio is None) and (seg.audio is None or torch.equal(seg.audio, o.audio))
            assert (seg.audio_codes is None) == (o.audio_codes is None) and (seg.audio_codes is None or torch.equal(seg.audio_codes, o.audio_codes))


def test_a_codec_without_encode_many_sees_exactly_todays_calls():
    texts, speakers, contexts, _ = _requests()
    codec = _SingleCodec()
    prompts = _gen(codec)._build_prompts(texts, speakers, contexts)
    want, single_calls = _per_segment_prompts(texts, speakers, contexts)
    assert len(codec.calls) == len(single_calls) == 4
    for (k, (x,)), (wk, (y,)) in zip(codec.calls, single_calls):
        assert k == wk == "encode" and torch.equal(x, y)
    assert all(torch.equal(t, wt) and torch.equal(m, wm) for (t, m), (wt, wm) in zip(prompts, want))


def test_build_prompt_of_one_request_uses_the_ragged_call_from_two_clips():
    texts, speakers, contexts, _ = _requests()
    codec = _ManyCodec()
    gen = _gen(codec)
    t, m = gen._build_prompt(texts[0], speakers[0], contexts[0])             # two unencoded clips
    assert [c[0] for c in codec.calls] == ["encode_many"] and len(codec.calls[0][1]) == 2
    wt, wm = _per_segment_prompts(texts[:1], speakers[:1], contexts[:1])[0][0]
    assert torch.equal(t, wt) and torch.equal(m, wm)
    codec.calls.clear()
    same = torch.randn(3000, generator=torch.Generator().manual_seed(1))
    gen._build_prompt([1], 0, [Segment(0, [2], audio=same), Segment(0, [3], audio=same)])
    assert [c[0] for c in codec.calls] == ["encode", "encode"]               # ONE distinct clip: nothing to share a chain with
    codec.calls.clear()
    gen._build_prompt(texts[2], speakers[2], contexts[2]); gen._build_prompt(texts[3], speakers[3], contexts[3])
    assert codec.calls == []                                                 # audio_codes everywhere / no context: no encode at all


@pytest.mark.parametrize("threshold", [3, 4])
def test_below_the_threshold_constant_the_helper_makes_todays_calls(monkeypatch, threshold):
    texts, speakers, contexts, distinct = _requests()                        # three distinct clips
    monkeypatch.setattr(G, "ENCODE_MANY_MIN_CLIPS", threshold)
    codec = _ManyCodec()
    prompts = _gen(codec)._build_prompts(texts, speakers, contexts)
    want, single_calls = _per_segment_prompts(texts, speakers, contexts)
    kinds = [c[0] for c in codec.calls]
    assert kinds == (["encode_many"] if len(distinct) >= threshold else ["encode"] * len(single_calls))
    assert all(torch.equal(t, wt) and torch.equal(m, wm) for (t, m), (wt, wm) in zip(prompts, want))


def test_the_threshold_constant_is_a_positive_int():
    assert isinstance(G.ENCODE_MANY_MIN_CLIPS, int) and G.ENCODE_MANY_MIN_CLIPS >= 1
