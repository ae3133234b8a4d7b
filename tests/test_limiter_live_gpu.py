"""The limiter where audio leaves (tiny codec, tiny model): ``generate_many_stream(limiter=)`` chunk by chunk beside the frame loop, after
the stretch and the leveler and in front of the watermark and the resampler.  Everything is bit for bit the rule (tests/limiter_ref.py,
tests/leveler_ref.py) applied to what the same call gives without ``limiter``; frames and ``last`` flags are the plain run's, and the
chunk lengths differ only by the look-ahead, which moves from a request's first chunk to its last."""
import numpy as np
import pytest
import torch

import leveler_ref as LR
import limiter_ref as R

pytestmark = pytest.mark.gpu
LENS = [27, 3, 10, 0, 14, 20, 1]
SPEEDS = [1.2, None, 0.8, 1.2, 2.0, 0.5, None]
KEY = [212, 211, 146, 56, 201]


def _limits():
    from sesameai.limiter import Limit
    return [Limit(), None, Limit(-6.0, 480, 250.0), True, Limit(-12.0, 24, 20.0, drive_shift=1), Limit(-3.0, 1, 1.0 / 24), True]


def _levels():
    from sesameai.loudness import Level
    return [Level(-19.0), -23.0, None, -19.0, Level(-16.0, start_gain=2.0), Level(-23.0, slew_shift=2), None]


def _limit_of(v):
    from sesameai.limiter import Limit
    return None if v is None else Limit() if v is True else v


def _level_of(v):
    from sesameai.loudness import Level
    return None if v is None else v if isinstance(v, Level) else Level(float(v))


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


def _same_frames_and_moved_lookahead(a, b, L):
    """frames and last flags are the plain run's; the lengths differ only by the L samples that move from the first chunk(s) to the last"""
    assert [c[2] for c in b] == [c[2] for c in a] == [False] * (len(b) - 1) + [True] and len(a) == len(b)
    assert all(torch.equal(x[1], y[1]) for x, y in zip(a, b))
    la, lb = [x[0].shape[0] for x in a], [y[0].shape[0] for y in b]
    taken = given = 0
    for j in range(len(la)):
        taken += la[j]
        ready = taken if j == len(la) - 1 else max(0, taken - L)
        assert lb[j] == ready - given, (j, la, lb)
        given = ready


def test_each_requests_chunks_are_the_rule_on_its_plain_chunks(setup):
    limits = _limits()
    plain, got = setup["plain"], setup["run"](limiter=limits)
    limited, excused = 0, 0
    for i, n in enumerate(LENS):
        a, b, lm = plain[i], got[i], _limit_of(limits[i])
        if lm is None:
            assert len(a) == len(b) and all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and x[2] == y[2] for x, y in zip(a, b)), \
                "a request without a limit is bit-identical, chunk by chunk"
            continue
        _same_frames_and_moved_lookahead(a, b, lm.lookahead)
        x = _cat(a).cpu().numpy()
        assert x.shape[0] == 1920 * n
        want = R.limit_ref(x, R.Params(*lm.params()))
        assert np.array_equal(_cat(b).cpu().numpy(), want.y), f"request {i} ({n} frames, {lm})"
        limited += want.limited > 0
        excused += x.shape[0] == 0
        print(f"request {i}: {n} frames, peak in {np.abs(x).max(initial=0) * 32768:.0f}, {want.limited} of {x.shape[0]} samples limited, "
              f"min gain {want.row[0] / 65536:.3f}, {want.row[3]} clamped")
    assert limited >= 2, "some requests are limited by the reference: no identity passes"
    assert excused <= 1, "only the 0-frame request is excused"
    again = setup["run"]()
    assert all(torch.equal(_cat(again[i]), _cat(plain[i])) for i in plain), "the plain path is what it was"
    one = setup["run"](limiter=True)                        # one value for all
    for i in range(len(LENS)):
        assert np.array_equal(_cat(one[i]).cpu().numpy(), R.limit_ref(_cat(plain[i]).cpu().numpy(), R.params()).y), i


def test_behind_the_leveler_the_pair_comes_from_paired(setup):
    from sesameai.limiter import paired
    levels, limits = _levels(), _limits()
    plain, got = setup["plain"], setup["run"](loudness=levels, limiter=limits)
    limited = 0
    for i, n in enumerate(LENS):
        lv, lm = _level_of(levels[i]), _limit_of(limits[i])
        if lv is not None and lm is not None:
            lv, lm = paired(lv, lm)
        x = _cat(plain[i]).cpu().numpy()
        if lv is not None:
            x = LR.level_ref(x, LR.Params(*lv.params())).y
        if lm is not None:
            _same_frames_and_moved_lookahead(plain[i], got[i], lm.lookahead)
            w = R.limit_ref(x, R.Params(*lm.params()))
            x = w.y
            limited += w.limited > 0 and lv is not None
            print(f"request {i}: {n} frames, {'levelled, ' if lv is not None else ''}{w.limited} of {x.shape[0]} samples limited, min gain {w.row[0] / 65536:.3f}")
        assert np.array_equal(_cat(got[i]).cpu().numpy(), x), f"request {i}: limit_ref(level_ref(plain, Level'), Limit')"
    assert limited >= 2, "some levelled requests are limited by the reference"


def test_with_speed_watermark_and_a_foreign_rate_the_order_is_stretch_level_limit_mark_resample(setup):
    from sesameai.limiter import limit, paired
    from sesameai.loudness import level
    from sesameai.resample import resample
    from sesameai.stretch import stretch
    from sesameai.watermarking import embed
    levels, limits = _levels(), _limits()
    plain = setup["plain"]
    got24 = setup["run"](speed=SPEEDS, watermark=KEY, loudness=levels, limiter=limits)
    got48 = setup["run"](speed=SPEEDS, watermark=KEY, loudness=levels, limiter=limits, out_sample_rate=48000)
    for i, n in enumerate(LENS):
        if n == 0:
            assert _cat(got24[i]).numel() == 0 and _cat(got48[i]).numel() == 0
            continue
        lv, lm = _level_of(levels[i]), _limit_of(limits[i])
        if lv is not None and lm is not None:
            lv, lm = paired(lv, lm)
        mid = _cat(plain[i])
        mid = mid if SPEEDS[i] is None else stretch([mid], SPEEDS[i])[0]
        if lv is not None:
            mid = level([mid], lv)[0]
        if lm is not None:
            lim = limit([mid], lm)[0]
            assert np.array_equal(lim.cpu().numpy(), R.limit_ref(mid.cpu().numpy(), R.Params(*lm.params())).y), f"request {i}: limit() is the rule"
            mid = lim
        (want,) = embed([mid], KEY)
        assert torch.equal(_cat(got24[i]), want), f"request {i}: embed(limit(level(stretch(plain))))"
        (want48,) = resample([want], 24000, 48000)
        assert _cat(got48[i]).shape == want48.shape and torch.equal(_cat(got48[i]), want48), f"request {i}: resample of that"
        assert [c[2] for c in got24[i]] == [c[2] for c in plain[i]] and all(torch.equal(x[1], y[1]) for x, y in zip(plain[i], got24[i]))
