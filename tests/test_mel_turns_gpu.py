"""The speech-to-text input of a spoken turn, end to end on the device (tiny codec): 48 kHz int16 microphones through
``Generator.open_turn_streams(n=3, sample_rate=48000, vad=True, features=True)`` with uneven feeds.  At every END the features are bit
for bit ``log_mel([resample(samples24k[a:b], 24000, 16000)])`` of exactly the samples the segment's codes encode, within 2 E of the rule
(tests/mel_ref.py; E from tests/golden/mel.pt), and the segment's codes are those of the same run without features.  The same without a
vad, where a turn is what lies between two ``finish`` calls."""
import os

import numpy as np
import pytest
import torch

import mel_ref as R
import vad_ref as V
from test_vad_turns_gpu import POST_MS, PRE_MS, PRM, _mic

pytestmark = pytest.mark.gpu
RATE = 48000


@pytest.fixture(scope="module")
def codec():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sesameai.mimi import MimiCodec, mimi_tiny_args, synthetic_state_dict
    return MimiCodec(mimi_tiny_args(), synthetic_state_dict(mimi_tiny_args(), seed=4321), max_frames=64)


@pytest.fixture(scope="module")
def E():
    return torch.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mel.pt"))["E"]


def _gen(codec):
    from sesameai.generator import Generator
    gen = Generator.__new__(Generator)
    gen._audio_tokenizer, gen.sample_rate, gen.device = codec, codec.sample_rate, codec.device
    return gen


def _run_vad(codec, features):
    from sesameai.turns import ReplyOnPause
    from sesameai.vad import VadParams
    ts = _gen(codec).open_turn_streams(3, chunk_frames=4, sample_rate=RATE, vad=True, pre_roll_ms=PRE_MS, post_roll_ms=POST_MS, features=features)
    ts.vad.reset([0, 2], VadParams(*PRM))
    mics = {2: _mic(RATE, 1, True), 0: _mic(RATE, 2, True)}
    out = {0: [], 2: []}
    events = []
    poll = ts.poll_events
    ts.poll_events = lambda: [events.append(e) or e for e in poll()]

    def respond(sid, segment):
        out[sid].append((segment(1, [0]), ts.take_features(sid) if features else None))

    rop = ReplyOnPause(ts, respond)
    step, at = {2: int(0.02 * RATE) + 7, 0: int(0.033 * RATE)}, {0: 0, 2: 0}
    while any(at[s] < mics[s].shape[0] for s in mics):
        for s in (2, 0):
            if at[s] < mics[s].shape[0]:
                rop.receive(s, mics[s][at[s]:at[s] + step[s]])
                at[s] += step[s]
    return ts, mics, out, events


def test_features_at_every_end_are_those_of_the_samples_the_codes_encode(codec, E):
    from sesameai.mel import TurnFeatures, log_mel
    from sesameai.resample import resample
    ts, mics, out, events = _run_vad(codec, True)
    _, _, plain, events0 = _run_vad(codec, None)
    assert isinstance(ts.features, TurnFeatures) and ts.features.n_mels == 80 and events == events0
    hop = codec.args.hop
    for s, x in mics.items():
        whole = resample([x.cuda()], RATE, 24000)[0]
        ends = [(n) for sid, k, n in events if sid == s and k == "end"]
        starts = [(n) for sid, k, n in events if sid == s and k == "start"]
        assert len(out[s]) == len(plain[s]) == len(ends) == 2
        for a, end, (seg, (feats, n_frames)), (seg0, _) in zip(starts, ends, out[s], plain[s]):
            T = -(-(end - a) // hop)
            b = a + T * hop
            assert seg.audio_codes.shape == (32, T) and torch.equal(seg.audio_codes, seg0.audio_codes), "the codes do not move"
            at16 = resample([whole[a:b]], 24000, 16000)[0]
            want = log_mel([at16], 80)[0]
            assert n_frames == R.frames_needed(at16.shape[0], True) and feats.shape == (80, 3000)
            assert torch.equal(feats, want), (s, a, b)
            d = float(np.abs(feats.cpu().numpy().astype(np.float64) - R.log_mel(at16.cpu().numpy(), 80)).max())
            print(f"stream {s} turn [{a}, {b}): {n_frames} frames, |features - mel_ref| = {d:.3e} = {d / E:.3f} E")
            assert d <= 2 * E


def test_the_same_without_a_vad(codec, E):
    from sesameai.mel import log_mel
    from sesameai.resample import resample
    results = {}
    for features in (128, None):
        ts = _gen(codec).open_turn_streams(3, chunk_frames=4, sample_rate=RATE, features=features)
        mics = {1: _mic(RATE, 1, True)[:50000], 2: _mic(RATE, 2, True)[3000:61234]}
        step, at = {1: 1111, 2: 4097}, {1: 0, 2: 0}
        while any(at[s] < mics[s].shape[0] for s in mics):
            for s in mics:
                if at[s] < mics[s].shape[0]:
                    ts.feed(s, mics[s][at[s]:at[s] + step[s]])
                    at[s] += step[s]
            ts.pump()
        results[features] = {s: (ts.finish(s, 1, [0]), ts.take_features(s) if features else None) for s in mics}
    for s, x in mics.items():
        seg, (feats, n_frames) = results[128][s]
        assert torch.equal(seg.audio_codes, results[None][s][0].audio_codes)
        at16 = resample([resample([x.cuda()], RATE, 24000)[0]], 24000, 16000)[0]
        assert feats.shape == (128, 3000) and n_frames == R.frames_needed(at16.shape[0], True)
        assert torch.equal(feats, log_mel([at16], 128)[0])
        assert float(np.abs(feats.cpu().numpy().astype(np.float64) - R.log_mel(at16.cpu().numpy(), 128)).max()) <= 2 * E
