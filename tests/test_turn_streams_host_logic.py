"""TurnStreams (sesameai/turns.py) against a recording fake pool: what it buffers, which pool calls it makes and what it hands back.  No GPU:
the fake pool's "codes" of a frame are that frame's first sample in every codebook, so a turn's codes say which samples went where."""
import pytest
import torch

HOP = 8


class _FakeEncPool:
    def __init__(self, n, max_chunk_frames):
        self.n_streams, self.max_chunk_frames = n, max_chunk_frames
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
        self.calls.append([(i, int(w.shape[0])) for i, w in zip(ids, wavs)])
        return out

    def reset(self, ids=None):
        ids = list(range(self.n_streams)) if ids is None else [int(i) for i in ids]
        self.resets.append(ids)
        for i in ids:
            self._ended[i] = False


def _turns(n=3, chunk=4):
    from sesameai.turns import TurnStreams
    pool = _FakeEncPool(n, chunk)
    return pool, TurnStreams(pool, HOP, chunk_frames=chunk)


def _ramp(a, b):
    return torch.arange(a, b, dtype=torch.float32)


def test_feed_buffers_across_calls_and_pump_makes_one_call_for_every_stream_with_a_whole_frame():
    pool, ts = _turns()
    assert ts.pump() == 0 and pool.calls == []
    ts.feed(0, _ramp(0, 5)); ts.feed(0, _ramp(5, 7))                    # 7 samples: no whole frame yet
    ts.feed(2, _ramp(100, 100 + 2 * HOP + 3))                           # two frames and three samples
    assert ts.buffered(0) == 7 and ts.buffered(2) == 2 * HOP + 3
    assert ts.pump() == 2 and pool.calls == [[(2, 2 * HOP)]]
    assert ts.buffered(0) == 7 and ts.buffered(2) == 3 and ts.frames(2) == 2
    ts.feed(0, _ramp(7, 9)); ts.feed(1, _ramp(200, 200 + HOP)); ts.feed(2, _ramp(100 + 2 * HOP + 3, 100 + 3 * HOP))
    assert ts.pump() == 3 and pool.calls[1] == [(0, HOP), (1, HOP), (2, HOP)], "ONE call for all three streams"
    assert ts.buffered(0) == 1 and ts.buffered(1) == 0 and ts.buffered(2) == 0
    assert ts.pump() == 0 and len(pool.calls) == 2, "nothing to encode: no call"


def test_pump_gives_a_stream_at_most_chunk_frames_and_keeps_the_rest():
    pool, ts = _turns(chunk=4)
    ts.feed(1, _ramp(0, 9 * HOP + 5))
    assert ts.pump() == 4 and ts.pump() == 4 and ts.pump() == 1 and ts.pump() == 0
    assert pool.calls == [[(1, 4 * HOP)], [(1, 4 * HOP)], [(1, HOP)]] and ts.buffered(1) == 5


@pytest.mark.parametrize("left, calls", [(0, []), (5, [5]), (2 * HOP, [2 * HOP]), (4 * HOP, [4 * HOP]), (4 * HOP + 1, [4 * HOP, 1]),
                                         (9 * HOP + 3, [4 * HOP, 4 * HOP, HOP + 3])])
def test_finish_encodes_what_is_left_in_the_fewest_calls_and_resets(left, calls):
    from sesameai.generator import Segment
    pool, ts = _turns(chunk=4)
    n = 3 * HOP + left
    ts.feed(1, _ramp(0, 3 * HOP))
    assert ts.pump() == 3
    ts.feed(1, _ramp(3 * HOP, n))
    ts.feed(0, _ramp(500, 500 + HOP))                                   # a neighbour's buffer stays out of it
    seg = ts.finish(1, speaker=1, text=[4, 5])
    assert pool.calls[1:] == [[(1, c)] for c in calls]
    assert pool.resets == [[1]], "the finished stream, and only it, is reset"
    assert isinstance(seg, Segment) and seg.speaker == 1 and seg.text == [4, 5] and seg.audio is None
    T = -(-n // HOP)
    assert seg.audio_codes.shape == (32, T) and torch.equal(seg.audio_codes[0], torch.arange(T) * HOP), "every frame once, in order"
    assert ts.buffered(1) == 0 and ts.frames(1) == 0 and ts.buffered(0) == HOP
    # the stream starts its next turn from scratch
    ts.feed(1, _ramp(900, 900 + HOP + 2))
    seg2 = ts.finish(1, 0, "next")
    assert torch.equal(seg2.audio_codes[0], torch.tensor([900, 900 + HOP])) and pool.resets == [[1], [1]]


def test_a_turn_without_samples_is_an_error_and_resets_nothing():
    pool, ts = _turns()
    with pytest.raises(ValueError, match="without samples"):
        ts.finish(0, 0, "x")
    assert pool.calls == [] and pool.resets == []


def test_the_segment_goes_through_the_generators_tokenizer():
    from sesameai.generator import Generator
    pool, ts = _turns()
    ts.feed(0, _ramp(0, 2 * HOP + 1))
    seg = ts.finish(0, 1, [7, 8])
    gen = Generator.__new__(Generator)
    gen.device, gen._text_tokenizer, gen._audio_tokenizer = torch.device("cpu"), None, None
    t, m = gen._tokenize_segment(seg)
    assert t.shape == (2 + 3 + 1, 33) and torch.equal(t[2:5, 0], torch.tensor([0, HOP, 2 * HOP])) and bool(m[2:, :-1].all())
