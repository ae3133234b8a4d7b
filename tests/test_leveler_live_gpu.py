"""The leveler where audio leaves (tiny codec, tiny model): ``generate_many_stream(loudness=)`` chunk by chunk beside the frame loop, after
the stretch and in front of the watermark and the resampler.  Everything is bit for bit the rule (tests/leveler_ref.py) applied to what the
same call gives without ``loudness``; the leveler holds nothing back, so chunk lengths, frames and ``last`` flags are the plain run's."""
import numpy as np
import pytest
import torch

import leveler_ref as R
import loudness_ref as L

pytestmark = pytest.mark.gpu
LENS = [27, 3, 10, 0, 14, 20, 1]
SPEEDS = [1.2, None, 0.8, 1.2, 2.0, 0.5, None]
KEY = [212, 211, 146, 56, 201]


def _levels():
    from sesameai.loudness import Level
    return [Level(-19.0), None, Level(-23.0, start_gain=0.5), -19.0, Level(-16.0, ceiling_db=-3.0, slew_shift=2), -30.0, Level(-19.0, start_gain=2.0)]


def _params(v):
    from sesameai.loudness import Level
    return None if v is None else R.Params(*(v if isinstance(v, Level) else Level(float(v))).params())


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
    return {"gen": gen, "run": run, "plain": run()}


def _cat(chunks):
    return torch.cat([c[0] for c in chunks])


def test_each_requests_chunks_are_the_rule_on_its_plain_chunks(setup):
    levels = _levels()
    plain, even = setup["plain"], setup["run"](loudness=levels)
    moved, silent, excused = 0, 0, 0
    for i, n in enumerate(LENS):
        a, b = plain[i], even[i]
        assert [c[2] for c in b] == [c[2] for c in a] == [False] * (len(b) - 1) + [True] and len(a) == len(b)
        assert all(torch.equal(x[1], y[1]) and x[0].shape == y[0].shape for x, y in zip(a, b)), "frames and chunk lengths are the plain run's"
        p = _params(levels[i])
        if p is None:
            assert all(torch.equal(x[0], y[0]) for x, y in zip(a, b)), "a request without a level is bit-identical, chunk by chunk"
            continue
        x = _cat(a).cpu().numpy()
        assert x.shape[0] == 1920 * n
        want = R.level_ref(x, p)
        assert np.array_equal(_cat(b).cpu().numpy(), want.y), f"request {i} ({n} frames, {p})"
        moved += x.shape[0] > 0 and (p.g0 != 65536 or len(set(want.gains.tolist())) > 1)
        silent += x.shape[0] > 0 and L.measure_ref(x)[1] == 0
        excused += x.shape[0] == 0                            # nothing to compare
        print(f"request {i}: {n} frames, {L.lufs(*L.measure_ref(x)[:2]):.2f} LUFS in, gains {want.gains[0]} .. {want.row[0]}, {want.row[2]} clamped")
    print(f"{moved} requests with a gain that leaves 1.0, {silent} under the absolute gate throughout, {excused} without a sample")
    assert moved >= 2, "some request's gain leaves 1.0: no identity passes"
    assert excused <= 1, "only the 0-frame request is excused for silence"
    again = setup["run"]()
    assert all(torch.equal(_cat(again[i]), _cat(plain[i])) for i in plain), "the plain path is what it was"
    one = setup["run"](loudness=-19.0)                      # one value for all
    for i, n in enumerate(LENS):
        assert np.array_equal(_cat(one[i]).cpu().numpy(), R.level_ref(_cat(plain[i]).cpu().numpy(), R.params(-19.0)).y), i


def test_with_speed_watermark_and_a_foreign_rate_the_order_is_stretch_level_mark_resample(setup):
    from sesameai.loudness import level
    from sesameai.resample import resample
    from sesameai.stretch import stretch
    from sesameai.watermarking import embed
    levels = _levels()
    plain = setup["plain"]
    got24 = setup["run"](speed=SPEEDS, watermark=KEY, loudness=levels)
    got48 = setup["run"](speed=SPEEDS, watermark=KEY, loudness=levels, out_sample_rate=48000)
    for i, n in enumerate(LENS):
        if n == 0:
            assert _cat(got24[i]).numel() == 0 and _cat(got48[i]).numel() == 0
            continue
        pcm24 = _cat(plain[i])
        mid = pcm24 if SPEEDS[i] is None else stretch([pcm24], SPEEDS[i])[0]
        p = _params(levels[i])
        if p is not None:
            lev = level([mid], levels[i])[0]
            assert np.array_equal(lev.cpu().numpy(), R.level_ref(mid.cpu().numpy(), p).y), f"request {i}: level() is the rule"
            mid = lev
        (want,) = embed([mid], KEY)
        assert torch.equal(_cat(got24[i]), want), f"request {i}: embed(level(stretch(plain)))"
        (want48,) = resample([want], 24000, 48000)
        assert _cat(got48[i]).shape == want48.shape and torch.equal(_cat(got48[i]), want48), f"request {i}: resample of that"
        assert [c[2] for c in got24[i]] == [c[2] for c in plain[i]] and all(torch.equal(x[1], y[1]) for x, y in zip(plain[i], got24[i]))
