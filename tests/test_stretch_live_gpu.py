"""The time-stretch pool where audio leaves (tiny codec, tiny model): ``generate_many_stream(speed=)`` chunk by chunk beside the frame loop,
in front of the resampler, and ``generate_many(finish=, speed=)`` / ``generate(speed=)`` on whole clips.  Everything is bit for bit the rule
(tests/stretch_ref.py) applied to what the same call gives without ``speed``: the streamed == one-shot property under the decode pool's own."""
import numpy as np
import pytest
import torch

import stretch_ref as S
from finish_ref import finish_ref_ms

pytestmark = pytest.mark.gpu
LENS = [27, 3, 10, 0, 14, 20, 1]
SPEEDS = [1.2, None, 0.8, 1.2, 2.0, 0.5, 1.2]


@pytest.fixture(scope="module")
def setup():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sesameai.generator import Generator, Segment
    from sesameai.mimi import MimiCodec, mimi_tiny_args, synthetic_state_dict
    from sesameai.models import Model, csm_tiny_args
    codec = MimiCodec(mimi_tiny_args(), synthetic_state_dict(mimi_tiny_args(), seed=4321), max_frames=64)
    model = Model(csm_tiny_args(), None, max_frames=64, max_prefill_rows=128)
    gen = Generator(model, audio_tokenizer=codec, max_batch_size=3)
    gen.refill_row_layers = 10
    g = torch.Generator().manual_seed(21)
    texts = [torch.randint(0, 1000, (4 + i % 5,), generator=g).tolist() for i in range(len(LENS))]
    ctxs = [[Segment(speaker=1, text=torch.randint(0, 1000, (3,), generator=g).tolist(), audio_codes=torch.randint(0, 2048, (32, 2 + i % 4), generator=g))]
            for i in range(len(LENS))]
    ms = [n * 80 for n in LENS]

    def run(**kw):                                          # greedy (top-k 1): every run generates the same frames
        got = {i: [] for i in range(len(LENS))}
        for i, pcm, frames, last in gen.generate_many_stream(texts, [1] * len(LENS), ctxs, max_audio_length_ms=ms, temperature=0.9, topk=1,
                                                             first_chunk_frames=2, **kw):
            got[i].append((pcm.clone(), frames, last))
        return got
    return {"gen": gen, "texts": texts, "ctxs": ctxs, "ms": ms, "run": run, "plain": run()}


def _cat(chunks):
    return torch.cat([c[0] for c in chunks])


def _want(pcm24, speed):
    return S.stretch_ref(pcm24.cpu().numpy(), S.to_pm(speed))[0]


def test_each_requests_chunks_are_the_rule_on_its_plain_chunks(setup):
    plain, fast = setup["plain"], setup["run"](speed=SPEEDS)
    for i, n in enumerate(LENS):
        a, b = plain[i], fast[i]
        assert [c[2] for c in b] == [False] * (len(b) - 1) + [True] and len(a) == len(b)
        assert all(torch.equal(x[1], y[1]) for x, y in zip(a, b)), "the frames of every chunk are those of the plain run"
        if SPEEDS[i] is None:
            assert all(torch.equal(x[0], y[0]) for x, y in zip(a, b)), "a request without a speed is bit-identical, chunk by chunk"
            continue
        got = _cat(b)
        if n == 0:
            assert got.numel() == 0 and len(b) == 1
            continue
        want = _want(_cat(a), SPEEDS[i])
        assert got.dtype == torch.float32 and got.shape[0] == want.shape[0] == S.out_len(1920 * n, S.to_pm(SPEEDS[i]))
        assert np.array_equal(got.cpu().numpy(), want), f"request {i} ({n} frames at {SPEEDS[i]})"
        if b[-1][1].shape[0] == 0:
            assert b[-1][0].numel() > 0, "a closing chunk that is empty at 24 kHz carries the tail"
    again = setup["run"]()
    assert all(torch.equal(_cat(again[i]), _cat(plain[i])) for i in plain), "the plain path is what it was"
    one = setup["run"](speed=1.2)                           # one value for all
    assert all(np.array_equal(_cat(one[i]).cpu().numpy(), _want(_cat(plain[i]), 1.2)) for i in plain if LENS[i])


def test_with_a_foreign_rate_the_stretch_runs_in_front_of_the_resampler(setup):
    from sesameai.resample import resample
    from sesameai.stretch import stretch
    plain, fast = setup["plain"], setup["run"](speed=SPEEDS, out_sample_rate=48000)
    for i, n in enumerate(LENS):
        got = _cat(fast[i])
        if n == 0:
            assert got.numel() == 0
            continue
        pcm24 = _cat(plain[i])
        mid = pcm24 if SPEEDS[i] is None else stretch([pcm24], SPEEDS[i])[0]
        if SPEEDS[i] is not None:
            assert np.array_equal(mid.cpu().numpy(), _want(pcm24, SPEEDS[i]))
        (want,) = resample([mid], 24000, 48000)
        assert got.shape == want.shape and torch.equal(got, want), f"request {i}"


def test_generate_many_with_finish_and_speed_is_finish_of_the_rule(setup):
    from sesameai.finish import SegmentFinish
    gen = setup["gen"]
    kw = dict(max_audio_length_ms=setup["ms"], temperature=0.9, topk=1)
    clips = gen.generate_many(setup["texts"], [1] * len(LENS), setup["ctxs"], **kw)
    how = SegmentFinish(20, 10, 30)
    got = gen.generate_many(setup["texts"], [1] * len(LENS), setup["ctxs"], finish=how, speed=1.2, **kw)
    mixed = gen.generate_many(setup["texts"], [1] * len(LENS), setup["ctxs"], finish=how, speed=SPEEDS, **kw)
    bare = gen.generate_many(setup["texts"], [1] * len(LENS), setup["ctxs"], speed=SPEEDS, **kw)
    for i, n in enumerate(LENS):
        x = clips[i].detach().cpu().numpy().reshape(-1).astype(np.float32)
        assert x.shape[0] == 1920 * n
        assert np.array_equal(got[i].cpu().numpy(), finish_ref_ms(S.stretch_ref(x, 1200)[0], 20, 10, 30, 24_000)), f"request {i}"
        y = x if SPEEDS[i] is None else S.stretch_ref(x, S.to_pm(SPEEDS[i]))[0]
        assert np.array_equal(mixed[i].cpu().numpy(), finish_ref_ms(y, 20, 10, 30, 24_000)), f"request {i} at its own speed"
        assert np.array_equal(bare[i].detach().cpu().numpy().reshape(-1), y), f"request {i} without finish"


def test_generate_with_speed_is_the_rule_on_the_clip(setup):
    gen = setup["gen"]
    args = (setup["texts"][0], 1, setup["ctxs"][0])
    plain = gen.generate(*args, max_audio_length_ms=800, temperature=0.9, topk=1)
    fast = gen.generate(*args, max_audio_length_ms=800, temperature=0.9, topk=1, speed=0.8)
    same = gen.generate(*args, max_audio_length_ms=800, temperature=0.9, topk=1, speed=1.0)
    assert plain.numel() > 0 and plain.numel() % 1920 == 0 and torch.equal(same, plain)
    assert np.array_equal(fast.cpu().numpy(), S.stretch_ref(plain.cpu().numpy(), 800)[0])
    with pytest.raises(ValueError, match="speed"):
        gen.generate(*args, max_audio_length_ms=800, speed=2.5)
