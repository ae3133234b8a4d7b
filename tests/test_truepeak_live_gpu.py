"""True-peak detection where audio leaves (tiny codec, tiny model): ``generate_many_stream(limiter=Limit(true_peak=True))`` chunk by chunk
beside the frame loop, and ``SegmentFinisher`` with ``SegmentFinish(loudness=, true_peak=True)``.  Everything is bit for bit the rule
(tests/truepeak_ref.py) applied to what the same call gives without the limiter; frames and ``last`` flags are the plain run's, the chunk
lengths differ only by the latency L + T, which moves from a request's first chunk to its last; a request with None, or with
``true_peak=False``, is what it was.  The test prints how many 48 kHz int16 samples sit at +-32767 with and without the flag
(docs/experiments/true_peak.md records them)."""
import numpy as np
import pytest
import torch

import limiter_ref as R
import loudness_ref as LD
import truepeak_ref as P

pytestmark = pytest.mark.gpu
LENS = [27, 3, 10, 0, 14, 20, 1]
SPEEDS = [1.2, None, 0.8, 1.2, 2.0, 0.5, None]
KEY = [212, 211, 146, 56, 201]
T = P.T


def _limits():
    from sesameai.limiter import Limit
    return [Limit(true_peak=True), None, Limit(-6.0, 480, 250.0, true_peak=True), Limit(true_peak=False), Limit(-12.0, 24, 20.0, drive_shift=1, true_peak=True),
            Limit(-3.0, 1, 1.0 / 24, true_peak=True), Limit(true_peak=True)]


def _levels():
    from sesameai.loudness import Level
    return [Level(-19.0), -23.0, None, -19.0, Level(-16.0, start_gain=2.0), Level(-23.0, slew_shift=2), None]


def _level_of(v):
    from sesameai.loudness import Level
    return None if v is None else v if isinstance(v, Level) else Level(float(v))


def _rule(x, lm):
    p = R.Params(*lm.params())
    return P.limit_tp_ref(x, p) if lm.true_peak else R.limit_ref(x, p)


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


def _same_frames_and_moved_latency(a, b, D):
    """frames and last flags are the plain run's; the lengths differ only by the D samples that move from the first chunk(s) to the last"""
    assert [c[2] for c in b] == [c[2] for c in a] == [False] * (len(b) - 1) + [True] and len(a) == len(b)
    assert all(torch.equal(x[1], y[1]) for x, y in zip(a, b))
    la, lb = [x[0].shape[0] for x in a], [y[0].shape[0] for y in b]
    taken = given = 0
    for j in range(len(la)):
        taken += la[j]
        ready = taken if j == len(la) - 1 else max(0, taken - D)
        assert lb[j] == ready - given, (j, la, lb)
        given = ready


def test_each_requests_chunks_are_the_rule_on_its_plain_chunks(setup):
    from sesameai.limiter import Limit
    limits = _limits()
    plain, got = setup["plain"], setup["run"](limiter=limits)
    differs = 0
    for i, n in enumerate(LENS):
        a, b, lm = plain[i], got[i], limits[i]
        if lm is None:
            assert len(a) == len(b) and all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and x[2] == y[2] for x, y in zip(a, b)), \
                "a request without a limit is bit-identical, chunk by chunk"
            continue
        _same_frames_and_moved_latency(a, b, lm.latency)
        assert lm.latency == lm.lookahead + (T if lm.true_peak else 0)
        x = _cat(a).cpu().numpy()
        assert x.shape[0] == 1920 * n
        want = _rule(x, lm)
        assert np.array_equal(_cat(b).cpu().numpy(), want.y), f"request {i} ({n} frames, {lm})"
        if lm.true_peak and n:
            sample_mode = R.limit_ref(x, R.Params(*lm.params()))
            differs += not np.array_equal(want.y, sample_mode.y)
            print(f"request {i}: {n} frames, sample peak in {P.measure_tp(x)[0]}, true peak in {P.measure_tp(x)[1]}; {want.limited} of {x.shape[0]} samples "
                  f"limited (sample-peak rule: {sample_mode.limited}); true peak out {P.measure_tp(want.y)[1]} (sample-peak rule: {P.measure_tp(sample_mode.y)[1]}), C {lm.params()[0]}")
    assert differs >= 3, "the true-peak rule gives other samples than the sample-peak rule: no sample-peak arithmetic passes"
    # true_peak=False and the default are the parent's behaviour: the sample-peak rule, the look-ahead alone as latency
    old = setup["run"](limiter=[Limit(), None, Limit(-6.0, 480, 250.0), True, None, Limit(true_peak=False), True])
    for i, lm in enumerate([Limit(), None, Limit(-6.0, 480, 250.0), Limit(), None, Limit(), Limit()]):
        if lm is None:
            assert all(torch.equal(x[0], y[0]) for x, y in zip(plain[i], old[i])) and len(plain[i]) == len(old[i])
        else:
            _same_frames_and_moved_latency(plain[i], old[i], lm.lookahead)
            assert np.array_equal(_cat(old[i]).cpu().numpy(), R.limit_ref(_cat(plain[i]).cpu().numpy(), R.Params(*lm.params())).y), i
    again = setup["run"]()
    assert all(torch.equal(_cat(again[i]), _cat(plain[i])) for i in plain), "the plain path is what it was"


def test_with_speed_loudness_watermark_and_48_khz_int16_the_order_is_stretch_level_limit_mark_resample(setup):
    from sesameai.limiter import limit, paired
    from sesameai.loudness import level
    from sesameai.resample import resample
    from sesameai.stretch import stretch
    from sesameai.watermarking import embed
    levels, limits = _levels(), _limits()
    plain = setup["plain"]
    kw = dict(speed=SPEEDS, watermark=KEY, loudness=levels, out_sample_rate=48000, out_dtype=torch.int16)
    got48 = setup["run"](limiter=limits, **kw)
    sample48 = setup["run"](limiter=[None if lm is None else lm._replace(true_peak=False) for lm in limits], **kw)
    at_rail = [0, 0]
    for i, n in enumerate(LENS):
        if n == 0:
            assert _cat(got48[i]).numel() == 0
            continue
        lv, lm = _level_of(levels[i]), limits[i]
        if lv is not None and lm is not None:
            lv, lm = paired(lv, lm)
            assert lm.true_peak == limits[i].true_peak
        mid = _cat(plain[i])
        mid = mid if SPEEDS[i] is None else stretch([mid], SPEEDS[i])[0]
        if lv is not None:
            mid = level([mid], lv)[0]
        if lm is not None:
            lim = limit([mid], lm)[0]
            assert np.array_equal(lim.cpu().numpy(), _rule(mid.cpu().numpy(), lm).y), f"request {i}: limit() is the rule"
            mid = lim
        (want,) = embed([mid], KEY)
        (want48,) = resample([want], 24000, 48000, out_dtype=torch.int16)
        assert _cat(got48[i]).dtype == torch.int16 and _cat(got48[i]).shape == want48.shape and torch.equal(_cat(got48[i]), want48), \
            f"request {i}: resample(embed(limit_tp(level(stretch(plain)))))"
        assert [c[2] for c in got48[i]] == [c[2] for c in plain[i]] and all(torch.equal(x[1], y[1]) for x, y in zip(plain[i], got48[i]))
        if lm is not None and lm.true_peak:
            at_rail[0] += int((_cat(got48[i]).abs() >= 32767).sum())
            at_rail[1] += int((_cat(sample48[i]).abs() >= 32767).sum())
            print(f"request {i}: 48 kHz int16 peak {int(_cat(got48[i]).abs().max())} with true_peak, {int(_cat(sample48[i]).abs().max())} without")
    print(f"48 kHz int16 samples at +-32767 over the true-peak requests: {at_rail[0]} with true_peak=True, {at_rail[1]} with true_peak=False")


def test_the_finisher_with_true_peak_is_the_clip_gain_from_the_true_peak(setup):
    from sesameai.finish import SegmentFinish, SegmentFinisher
    from sesameai.truepeak import true_peak
    plain = setup["plain"]
    clips = [_cat(plain[i]) for i in (0, 2, 4, 5)]
    clips = [c * (0.5 / float(c.abs().max())) for c in clips]                               # half of full scale: a loud target makes the ceiling bind
    fin = SegmentFinisher()
    how = [SegmentFinish(20, 10, 5, loudness=-3.0, true_peak=True), SegmentFinish(0, 0, 0, loudness=-3.0, ceiling_db=-2.0, true_peak=True),
           SegmentFinish(20, 10, 5, loudness=-3.0), SegmentFinish(7, 3, 50, loudness=-3.0, true_peak=True)]
    out = fin.finish(clips, how)
    rows = fin.last_meter.cpu().tolist()
    bound = passes = 0
    for k, (c, f) in enumerate(zip(clips, how)):
        x = c.cpu().numpy()
        lead, tail, fade = f.samples(24000)
        P_T, C = f.level()
        S, n, peak, hops = LD.measure_ref(x)
        tp = P.measure_tp(x)
        assert tuple(rows[k]) == (S, n, tp[1] if f.true_peak else peak, hops), (k, rows[k], "the true peak stands in the peak column")
        want = P.finish_tp_ref(x, lead, tail, fade, P_T, C) if f.true_peak else LD.finish_ld_ref(x, lead, tail, fade, P_T, C)
        assert np.array_equal(out[k].cpu().numpy(), want), k
        if f.true_peak and n > 0 and LD.clip_gain(S, n, tp[1], P_T, C)[1]:
            bound += 1
            whole = P.finish_tp_ref(x, 0, 0, 0, P_T, C)                                      # (the clip between its own ends, as it was measured)
            assert np.array_equal(want[lead + fade:len(want) - tail - fade], whole[fade:len(whole) - fade])
            without = P.measure_tp(LD.finish_ld_ref(x, 0, 0, 0, P_T, C))[1]
            print(f"clip {k}: sample peak in {peak}, true peak in {tp[1]}; finished true peak {P.measure_tp(whole)[1]} with the flag, {without} without, C {C}")
            assert P.measure_tp(whole)[1] <= C + 1, (k, "the flag keeps the true peak under C")
            assert (without > C + 1) == (tp[1] * C > (C + 2) * max(tp[0], peak)), (k, "without it the true peak passes C wherever the input's passes its sample peak")
            passes += without > C + 1
            assert true_peak([out[k]])[0].true_peak == P.measure_tp(out[k].cpu().numpy())[1]
    assert bound >= 2 and passes >= 1, "the ceiling binds on some clips and the sample-peak finish passes it: the flag is shown to matter"
