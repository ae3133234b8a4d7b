"""Reply on pause end to end on the device (tiny codec): two microphones per rate -- 48 kHz int16 through the resampler pool, and 24 kHz fp32
-- carry synthetic two-turn signals through ``Generator.open_turn_streams(.., vad=True)``.  The events are where the rule
(tests/vad_ref.py, on the samples the encoder gets) puts them, and every turn's segment is bit for bit ``MimiCodec.encode`` of
``samples[a : a + T * hop]`` with a = max(previous cut, start_frame * 240 - pre_roll), end = end_frame * 240 + post_roll and
T = ceil((end - a) / hop)."""
import numpy as np
import pytest
import torch

import vad_ref as V
from test_vad_oracle import talk

pytestmark = pytest.mark.gpu
PRM = V.Params(min_on=4, hang=20, hold=10)
PRE_MS, POST_MS = 100, 50


@pytest.fixture(scope="module")
def codec():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sesameai.mimi import MimiCodec, mimi_tiny_args, synthetic_state_dict
    return MimiCodec(mimi_tiny_args(), synthetic_state_dict(mimi_tiny_args(), seed=4321), max_frames=64)


def _mic(rate, seed, int16):
    """2.4 s: two voiced stretches with pauses of more than hang between and after them"""
    n = int(2.4 * rate)
    t = np.arange(n) / rate
    x = (np.random.default_rng(seed).standard_normal(n) * 0.002).astype(np.float32)
    for lo, hi, f0 in ((0.3 + 0.05 * seed, 0.8, 150.0), (1.3, 1.8 + 0.05 * seed, 110.0)):
        m = (t >= lo) & (t < hi)
        v = sum(np.sin(2 * np.pi * f0 * h * t[m] + h * h) / h for h in range(1, 12))
        x[m] += (0.3 * v / np.abs(v).max()).astype(np.float32)
    x = torch.from_numpy(x)
    return (x.clamp(-1, 1) * 32767).round().to(torch.int16) if int16 else x


@pytest.mark.parametrize("rate, int16", [(48000, True), (24000, False)])
def test_two_microphones_two_turns_each(codec, rate, int16):
    from sesameai.generator import Generator
    from sesameai.resample import resample
    from sesameai.turns import ReplyOnPause
    from sesameai.vad import VadParams
    gen = Generator.__new__(Generator)
    gen._audio_tokenizer, gen.sample_rate, gen.device = codec, codec.sample_rate, codec.device
    ts = gen.open_turn_streams(3, chunk_frames=4, sample_rate=rate, vad=True, pre_roll_ms=PRE_MS, post_roll_ms=POST_MS)
    assert (ts.resampler is not None) == (rate != 24000) and ts.vad.n_streams == 3
    ts.vad.reset([0, 2], VadParams(*PRM))
    pre, post, hop = PRE_MS * 24, POST_MS * 24, codec.args.hop
    mics = {2: _mic(rate, 1, int16), 0: _mic(rate, 2, int16)}
    replies, starts = {0: [], 2: []}, {0: [], 2: []}
    rop = ReplyOnPause(ts, lambda sid, segment: replies[sid].append(segment(1, [len(replies[sid])])))
    step = {2: int(0.02 * rate) + 7, 0: int(0.033 * rate)}            # uneven feeds, a pump after every one of them
    at = {0: 0, 2: 0}
    events = []
    poll = ts.poll_events
    ts.poll_events = lambda: [events.append(e) or e for e in poll()]      # (a tap: ReplyOnPause consumes them)
    while any(at[s] < mics[s].shape[0] for s in mics):
        for s in (2, 0):
            if at[s] < mics[s].shape[0]:
                chunk = mics[s][at[s]:at[s] + step[s]]
                rop.receive(s, chunk.cuda() if s == 2 or rate == 24000 else chunk)          # (the resampler also takes host memory)
                at[s] += step[s]
    for s, x in mics.items():
        whole = resample([x.cuda()], rate, 24000)[0] if rate != 24000 else x.cuda()
        want = V.vad_ref(whole.cpu().numpy(), PRM).events
        assert [k for k, _ in want] == ["start", "end", "start", "end"], want
        mine = [(k, n) for sid, k, n in events if sid == s]
        cut, ranges = 0, []
        for (_, fs), (_, fe) in zip(want[0::2], want[1::2]):
            a, end = max(cut, fs * V.F - pre), fe * V.F + post
            ranges.append((a, end))
            cut = end
        assert mine == [(k, n) for a, end in ranges for k, n in (("start", a), ("end", end))], (s, mine, ranges)
        assert len(replies[s]) == 2
        for (a, end), seg in zip(ranges, replies[s]):
            T = -(-(end - a) // hop)
            assert a + T * hop <= whole.shape[0]
            ref = codec.encode(whole[a:a + T * hop][None, None])[0]
            assert seg.audio_codes.shape == ref.shape == (32, T) and torch.equal(seg.audio_codes, ref), (s, a, end)
        assert abs(ranges[0][0] / 24000 - (0.3 + 0.05 * (1 if s == 2 else 2) - PRE_MS / 1000)) < 0.03, "the first turn starts where the voice does"
