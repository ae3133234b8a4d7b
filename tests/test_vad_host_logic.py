"""TurnStreams with a voice-activity detector, and ReplyOnPause (sesameai/turns.py), against recording fakes.  No GPU: the fake encoder's
"codes" of a frame are that frame's first sample in every codebook and the samples are their own indices, so a turn's codes say which
samples went where; the fake detector calls the frames it was told to active and runs the rule's state machine (tests/vad_ref.py)."""
import pytest
import torch

import vad_ref as V

HOP, F = 8, 240
PRM = V.Params(min_on=2, hang=3)


class _FakeEncPool:
    def __init__(self, n, max_chunk_frames, log):
        self.n_streams, self.max_chunk_frames, self.log = n, max_chunk_frames, log
        self.calls, self.resets = [], []
        self._ended = [False] * n

    def encode(self, ids, wavs):
        ids = [int(i) for i in ids]
        assert len(set(ids)) == len(ids) == len(wavs) >= 1
        out = []
        for i, w in zip(ids, wavs):
            n = int(w.shape[0])
            T = -(-n // HOP)
            assert n >= 1 and T <= self.max_chunk_frames and not self._ended[i], "a call the real pool refuses"
            self._ended[i] = n % HOP != 0
            out.append(w[::HOP].long().view(1, T).expand(32, T).clone())
        self.calls.append([(i, int(w[0]), int(w.shape[0])) for i, w in zip(ids, wavs)])
        self.log.append(("enc", ids))
        return out

    def reset(self, ids=None):
        ids = list(range(self.n_streams)) if ids is None else [int(i) for i in ids]
        self.resets.append(ids)
        for i in ids:
            self._ended[i] = False


class _Frames:
    def __init__(self, flags, first):
        self.flags, self.first = torch.tensor(flags, dtype=torch.uint8), first


class _FakeVad:
    """frames listed in ``active[sid]`` are active; steps 7 and 8 of the rule decide the rest"""

    def __init__(self, n, active, log):
        self.n_streams, self.active, self.log = n, active, log
        self.params = {s: PRM for s in range(n)}
        self.calls = []
        self._st = {s: dict(rest=0, k=0, speech=0, run=0, quiet=0) for s in range(n)}

    def feed(self, ids, chunks, final):
        assert final is False and len(ids) == len(chunks) >= 1 and all(int(c.shape[0]) > 0 for c in chunks)
        self.calls.append([(int(i), int(c.shape[0])) for i, c in zip(ids, chunks)])
        self.log.append(("vad", [int(i) for i in ids]))
        out = []
        for i, c in zip(ids, chunks):
            st = self._st[i]
            st["rest"] += int(c.shape[0])
            first, flags = st["k"], []
            while st["rest"] >= F:
                st["rest"] -= F
                act = st["k"] in self.active.get(i, ())
                if not st["speech"]:
                    st["run"] = st["run"] + 1 if act else 0
                    if st["run"] == PRM.min_on:
                        st["speech"], st["run"], st["quiet"] = 1, 0, 0
                else:
                    st["quiet"] = 0 if act else st["quiet"] + 1
                    if st["quiet"] == PRM.hang:
                        st["speech"], st["quiet"] = 0, 0
                flags.append(5 * act | st["speech"] << 3)
                st["k"] += 1
            out.append(_Frames(flags, first))
        return out

    @staticmethod
    def events(frames, params, in_speech):
        return V.events(frames.flags.tolist(), params, frames.first, in_speech)


def _setup(active, n=2, chunk=256, pre=100, post=50):
    from sesameai.turns import TurnStreams
    log = []
    pool, vad = _FakeEncPool(n, chunk, log), _FakeVad(n, active, log)
    return log, pool, vad, TurnStreams(pool, HOP, chunk_frames=chunk, vad=vad, pre_roll=pre, post_roll=post)


def _run(ts, sid, lo, hi, step=F):
    """samples lo .. hi of the stream (each its own index), ``step`` per pump"""
    for at in range(lo, hi, step):
        ts.feed(sid, torch.arange(at, min(at + step, hi), dtype=torch.float32))
        ts.pump()


def test_without_a_vad_the_calls_are_todays():
    from sesameai.turns import TurnStreams
    log = []
    pool = _FakeEncPool(2, 4, log)
    ts = TurnStreams(pool, HOP, chunk_frames=4)
    assert ts.vad is None and not hasattr(ts, "_hist")
    ts.feed(0, torch.arange(0, 21, dtype=torch.float32)); ts.feed(1, torch.arange(100, 105, dtype=torch.float32))
    assert ts.pump() == 2 and pool.calls == [[(0, 0, 16)]] and ts.buffered(0) == 5
    seg = ts.finish(0, 1, [3])
    assert pool.calls[1:] == [[(0, 16, 5)]] and pool.resets == [[0]] and torch.equal(seg.audio_codes[0], torch.tensor([0, 8, 16]))
    assert log == [("enc", [0]), ("enc", [0])]


@pytest.mark.parametrize("pre", [100, 1000])
def test_a_turn_is_gated_by_the_detector(pre):
    # active frames 5 .. 9: START is detected at frame 6 and stamped 5; frames 10 .. 12 are quiet: END is detected at 12 and stamped 10
    log, pool, vad, ts = _setup({0: set(range(5, 10)) | {13, 14, 15}}, pre=pre)
    _run(ts, 0, 0, 6 * F)
    assert pool.calls == [] and ts.poll_events() == [] and ts.frames(0) == 0 and ts.buffered(0) == 0, "nothing is encoded in silence"
    assert len(vad.calls) == 6 and ts._recv[0] - ts._h0[0] <= pre + F, "only the pre-roll and what a START may reach back to is held"
    _run(ts, 0, 6 * F, 7 * F)
    a = max(0, 5 * F - pre)
    assert ts.poll_events() == [(0, "start", a)]
    assert pool.calls == [[(0, a, (7 * F - a) // HOP * HOP)]], "the turn begins at start_frame * 240 - pre_roll, whole frames go at once"
    assert log[-2:] == [("vad", [0]), ("enc", [0])], "the vad call comes first"
    _run(ts, 0, 7 * F, 13 * F)
    end = 10 * F + 50
    assert ts.poll_events() == [(0, "end", end)]
    T = -(-(end - a) // HOP)
    assert sum(c[0][2] for c in pool.calls) // HOP > T, "more was encoded than the turn holds"
    assert pool.resets == [[0]]
    assert [c for c in log if c[0] == "vad"] == [("vad", [0])] * 13, "one vad call per pump"
    seg = ts.finish(0, 1, [4, 5])
    assert seg.speaker == 1 and seg.text == [4, 5] and seg.audio is None
    assert seg.audio_codes.shape == (32, T) and torch.equal(seg.audio_codes[0], a + HOP * torch.arange(T)), "codes past the cut are dropped"
    with pytest.raises(ValueError, match="without samples"):
        ts.finish(0, 1, [1])
    # the second turn on the same stream: frames 13 .. 15 active, START stamped 13; it starts clean, not before the last cut
    n_calls = len(pool.calls)
    _run(ts, 0, 13 * F, 15 * F)
    a2 = max(end, 13 * F - pre)
    assert ts.poll_events() == [(0, "start", a2)] and len(pool.calls) == n_calls + 1
    assert pool.calls[-1] == [(0, a2, (15 * F - a2) // HOP * HOP)]
    _run(ts, 0, 15 * F, 16 * F + 3)
    seg2 = ts.finish(0, 0, "by hand")                                    # no END yet: the turn ends where the samples end
    T2 = -(-(16 * F + 3 - a2) // HOP)
    assert torch.equal(seg2.audio_codes[0], a2 + HOP * torch.arange(T2)) and pool.resets == [[0], [0]]
    assert ts.poll_events() == [(0, "end", 16 * F + 3)]
    _run(ts, 0, 16 * F + 3, 20 * F)                                       # the detector's own END finds no turn and starts none
    assert ts.poll_events() == [] and len(pool.resets) == 2


def test_an_encoder_that_lags_is_caught_up_at_the_end_and_streams_share_the_calls():
    # 4 frames (32 samples) a pump against 240 samples a pump: at END most of the turn is still to be encoded
    log, pool, vad, ts = _setup({0: set(range(5, 10)), 1: set(range(6, 9))}, chunk=4)
    for at in range(0, 13 * F, F):
        ts.feed(0, torch.arange(at, at + F, dtype=torch.float32)); ts.feed(1, torch.arange(at, at + F, dtype=torch.float32) + 100000)
        ts.pump()
    assert vad.calls == [[(0, F), (1, F)]] * 13, "ONE vad call for both streams"
    assert [c for c in log if c[0] == "enc"][1] == ("enc", [0, 1]), "ONE encode call for both"
    ev = ts.poll_events()
    a0, e0, a1, e1 = 5 * F - 100, 10 * F + 50, 6 * F - 100, 9 * F + 50
    assert ev == [(0, "start", a0), (1, "start", a1), (1, "end", e1), (0, "end", e0)]
    s0, s1 = ts.finish(0, 1, [1]), ts.finish(1, 1, [2])
    assert torch.equal(s0.audio_codes[0], a0 + HOP * torch.arange(-(-(e0 - a0) // HOP)))
    assert torch.equal(s1.audio_codes[0], 100000 + a1 + HOP * torch.arange(-(-(e1 - a1) // HOP)))
    assert all(n <= 4 * HOP for call in pool.calls for _, _, n in call)


def test_reply_on_pause_fires_once_per_end_and_interrupts_only_a_reply_in_flight():
    from sesameai.turns import ReplyOnPause
    log, pool, vad, ts = _setup({0: set(range(5, 10)) | set(range(14, 18)) | set(range(25, 29))})
    replies, cuts = [], []

    def respond(sid, segment):
        replies.append((sid, segment(1, [len(replies)])))

    rop = ReplyOnPause(ts, respond, on_interrupt=cuts.append)
    feed = lambda lo, hi: [rop.receive(0, torch.arange(at, at + F, dtype=torch.float32)) for at in range(lo * F, hi * F, F)]
    feed(0, 12)
    assert replies == [] and cuts == []
    feed(12, 13)                                                         # END of turn 1
    assert len(replies) == 1 and replies[0][0] == 0 and replies[0][1].text == [0] and rop.in_flight[0]
    feed(13, 15)
    assert cuts == []
    feed(15, 16)                                                         # START of turn 2 while the reply is in flight: barge-in
    assert cuts == [0] and not rop.in_flight[0]
    feed(16, 21)                                                         # END of turn 2
    assert len(replies) == 2 and cuts == [0]
    assert int(replies[1][1].audio_codes[0, 0]) == max(10 * F + 50, 14 * F - 100)
    rop.reply_done(0)
    feed(21, 32)                                                         # turn 3 starts after the reply has ended: nothing to interrupt
    assert cuts == [0] and len(replies) == 3
    assert [r[1].text for r in replies] == [[0], [1], [2]]
