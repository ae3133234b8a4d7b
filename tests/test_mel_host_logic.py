"""``TurnStreams(features=)``, ``ReplyOnPause(stt=)`` and ``WhisperSTT`` (sesameai/turns.py, sesameai/stt.py) against recording fakes.  No
GPU: the samples are their own indices, so every range a pool received says which samples went where (the fakes of
tests/test_vad_host_logic.py); the fake features object records its feeds and hands out, per ended turn, the ranges that made it."""
import torch

from test_vad_host_logic import F, HOP, _FakeEncPool, _FakeVad, _run


class _FakeResampler:
    """2 : 1, a sample's value is kept: output sample j of a stream is input sample 2 j"""

    def __init__(self, n, log):
        self.n_streams, self.log, self.calls, self._odd = n, log, [], [0] * n

    def reset(self, ids=None):
        for i in (range(self.n_streams) if ids is None else ids):
            self._odd[i] = 0

    def feed(self, ids, chunks, final):
        self.log.append(("rs", [int(i) for i in ids], bool(final)))
        out = []
        for i, c in zip(ids, chunks):
            out.append(c[self._odd[i]::2] / 2)
            self._odd[i] = (self._odd[i] + int(c.shape[0])) % 2
        return out


class _FakeFeatures:
    def __init__(self, n, log):
        self.n_streams, self.log, self.calls = n, log, []
        self._open = {s: [] for s in range(n)}
        self._ready = {s: [] for s in range(n)}

    def reset(self, ids=None):
        for i in (range(self.n_streams) if ids is None else ids):
            self._open[i] = []

    def feed(self, ids, chunks, final):
        ids = [int(i) for i in ids]
        fin = [bool(final)] * len(ids) if isinstance(final, (bool, int)) else [bool(f) for f in final]
        assert len(set(ids)) == len(ids) == len(chunks) == len(fin) >= 1
        self.calls.append([(i, int(c[0]) if c.shape[0] else None, int(c.shape[0]), f) for i, c, f in zip(ids, chunks, fin)])
        self.log.append(("feat", ids))
        for i, c, f in zip(ids, chunks, fin):
            self._open[i] += [int(v) for v in c.tolist()]
            if f:
                self._ready[i].append(self._open[i])
                self._open[i] = []

    def take(self, sid):
        turn = self._ready[sid].pop(0)
        return torch.tensor(turn, dtype=torch.float32), len(turn)


def _scenario(kind, features="absent"):
    """One fixed run of ``kind`` in {"plain", "vad", "vad+rs"}; -> (log, encoder pool, features fake or None, the TurnStreams, segments)"""
    from sesameai.turns import TurnStreams
    log, segs = [], []
    pool = _FakeEncPool(2, 256 if kind != "plain" else 4, log)
    feats = _FakeFeatures(2, log) if features == "fake" else None
    kw = {} if features == "absent" else {"features": feats}
    if kind == "plain":
        ts = TurnStreams(pool, HOP, chunk_frames=4, **kw)
        ts.feed(0, torch.arange(0, 21, dtype=torch.float32)); ts.feed(1, torch.arange(100, 109, dtype=torch.float32))
        ts.pump()
        ts.feed(0, torch.arange(21, 43, dtype=torch.float32))
        ts.pump()
        segs.append(ts.finish(0, 1, [3]))            # 3 samples are left: the last range goes with final
        segs.append(ts.finish(1, 1, [3]))            # 1 sample is left
        ts.feed(0, torch.arange(0, 16, dtype=torch.float32))
        ts.pump()
        segs.append(ts.finish(0, 1, [3]))            # nothing is left: an empty final
        return log, pool, feats, ts, segs
    vad = _FakeVad(2, {0: set(range(5, 10)) | set(range(13, 20)), 1: {2, 3, 4, 5, 6}}, log)
    rs = _FakeResampler(2, log) if kind == "vad+rs" else None
    ts = TurnStreams(pool, HOP, chunk_frames=256, vad=vad, pre_roll=100, post_roll=50, resampler=rs, **kw)
    k = 2 if rs else 1
    for at in range(0, 20 * F * k, 150 * k):
        for s in (0, 1):
            ts.feed(s, torch.arange(at, min(at + 150 * k, 20 * F * k), dtype=torch.float32))
        ts.pump()
    for s, kind_, _ in ts.poll_events():
        if kind_ == "end":
            segs.append((s, ts.finish(s, 1, [7])))
    segs.append((0, ts.finish(0, 1, [7])))           # stream 0's second turn has had no END: the caller ends it
    return log, pool, feats, ts, segs


def test_features_none_makes_todays_calls():
    for kind in ("plain", "vad", "vad+rs"):
        log0, pool0, _, _, segs0 = _scenario(kind)
        log1, pool1, _, ts1, segs1 = _scenario(kind, None)
        log2, pool2, feats, _, segs2 = _scenario(kind, "fake")
        assert ts1.features is None and log0 == log1 and pool0.calls == pool1.calls and pool0.resets == pool1.resets
        assert [c for c in log2 if c[0] != "feat"] == log0 and pool2.calls == pool0.calls, "the other pools' calls do not move"
        assert len(feats.calls) >= 3
        codes = lambda segs: [(s[1] if isinstance(s, tuple) else s).audio_codes for s in segs]
        assert all(torch.equal(a, b) for a, b in zip(codes(segs0), codes(segs2)))


def test_without_a_vad_the_same_ranges_go_to_encode_and_to_feed():
    log, pool, feats, ts, segs = _scenario("plain", "fake")
    enc = [[(i, a, n) for i, a, n in call] for call in pool.calls]
    fed = [[(i, a, n) for i, a, n, f in call] for call in feats.calls if call[0][2]]
    assert enc == fed, "one feed per encode call, over the same ids and ranges"
    finals = [(i, n) for call in feats.calls for i, a, n, f in call if f]
    assert finals == [(0, 3), (1, 1), (0, 0)], "final arrives once per turn, with the turn's last range (an empty one if none is left)"
    for seg, sid, want in zip(segs, (0, 1, 0), (43, 9, 16)):
        turn, n = ts.take_features(sid)
        assert n == want and torch.equal(turn[::HOP].long(), seg.audio_codes[0])


def test_with_a_vad_the_features_are_those_of_the_samples_the_codes_encode():
    for kind in ("vad", "vad+rs"):
        log, pool, feats, ts, segs = _scenario(kind, "fake")
        assert len(segs) == 3 and [s for s, _ in segs].count(0) == 2
        assert sum(f for call in feats.calls for *_, f in call) == 3, "final arrives once per turn"
        for sid, seg in segs:                        # take_features hands out the ended turns of a stream in order
            turn, n = ts.take_features(sid)
            T = seg.audio_codes.shape[1]
            a = int(seg.audio_codes[0, 0])
            assert n > (T - 1) * HOP and n <= T * HOP, "the features end where the segment's audio ends: inside its last frame"
            assert torch.equal(turn, torch.arange(a, a + n, dtype=torch.float32)), "exactly [a, b), in order, nothing twice"
            assert torch.equal(turn[::HOP].long(), seg.audio_codes[0])
        assert sum(n for call in pool.calls for _, _, n in call) > sum(s.audio_codes.shape[1] for _, s in segs) * HOP, \
            "more was encoded than the turns hold: the features were NOT fed that"
        some_early = [call for call in feats.calls if not any(f for *_, f in call)]
        assert some_early, "features are fed while the turn is spoken, not only at its end"


def test_reply_on_pause_passes_the_text():
    from sesameai.turns import ReplyOnPause, TurnStreams
    log = []
    pool, vad, feats = _FakeEncPool(1, 256, log), _FakeVad(1, {0: set(range(5, 10))}, log), _FakeFeatures(1, log)
    ts = TurnStreams(pool, HOP, chunk_frames=256, vad=vad, pre_roll=100, post_roll=50, features=feats)
    got = []

    def respond(sid, segment, text):
        got.append((sid, text, segment(1)))

    heard = []

    def stt(features, n_frames):
        heard.append((features, n_frames))
        return f"heard {n_frames}"

    rop = ReplyOnPause(ts, respond, stt=stt)
    for at in range(0, 14 * F, F):
        rop.receive(0, torch.arange(at, at + F, dtype=torch.float32))
    assert len(got) == 1 and len(heard) == 1
    sid, text, seg = got[0]
    assert sid == 0 and text == f"heard {heard[0][1]}" and seg.text == text and seg.speaker == 1
    assert heard[0][1] == int(heard[0][0].shape[0]) > 0
    # stt=None: today's two-argument respond
    log2 = []
    ts2 = TurnStreams(_FakeEncPool(1, 256, log2), HOP, chunk_frames=256, vad=_FakeVad(1, {0: set(range(5, 10))}, log2), pre_roll=100, post_roll=50)
    got2 = []
    rop2 = ReplyOnPause(ts2, lambda sid, segment: got2.append(segment(1, [9])))
    for at in range(0, 14 * F, F):
        rop2.receive(0, torch.arange(at, at + F, dtype=torch.float32))
    assert len(got2) == 1 and got2[0].text == [9] and torch.equal(got2[0].audio_codes, seg.audio_codes)


def test_whisper_stt_gives_the_model_a_batch_of_one():
    from sesameai.stt import WhisperSTT
    seen = {}

    class Model:
        dtype = torch.float16

        def generate(self, input_features, **kw):
            seen["x"], seen["kw"] = input_features, kw
            return torch.tensor([[50258, 7, 8, 50257]])

    class Tok:
        def batch_decode(self, ids, skip_special_tokens=False):
            assert skip_special_tokens
            return [" hello there "]

    for n_mels, dtype, want in ((80, None, torch.float16), (128, torch.float32, torch.float32)):
        stt = WhisperSTT(Model(), Tok(), dtype=dtype, max_new_tokens=5)
        feats = torch.randn(n_mels, 3000)
        assert stt(feats, 17) == "hello there"
        assert seen["x"].shape == (1, n_mels, 3000) and seen["x"].dtype == want and seen["kw"] == {"max_new_tokens": 5}
        assert torch.equal(seen["x"][0].float(), feats.to(want).float())


def test_open_turn_streams_takes_the_keyword():
    import inspect
    from sesameai.generator import Generator
    assert inspect.signature(Generator.open_turn_streams).parameters["features"].default is None
