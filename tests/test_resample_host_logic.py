"""Host logic around the resampler pool (no GPU): TurnStreams (sesameai/turns.py) and SlotStreams (sesameai/live_batch.py, through
Generator.generate_many_stream) against recording fake pools.  The fake resampler is a pure delay -- it holds a stream's last LOOK samples
back until ``final`` -- so a turn's or a request's samples come out once, in order, exactly when the tail is carried; what is checked is the
bookkeeping: ONE resampler call per pump and per decode call, today's call sequence when no rate is given, and a closing chunk with the tail."""
import pytest
import torch

from test_host_logic import _ScriptedSlots, _ScriptedSlotsBeside
from test_first_chunk_host_logic import _Codec
from test_streams_host_logic import _scripts
from test_turn_streams_host_logic import HOP, _FakeEncPool, _ramp

LOOK = 5


class _FakeResampler:
    out_dtype = torch.float32

    def __init__(self, src_rate=48000, dst_rate=24000, n=3, device="cpu", out_dtype=torch.float32):
        self.args = (src_rate, dst_rate, n)
        self.n_streams, self.calls, self.resets = n, [], []
        self._held = [torch.empty(0) for _ in range(n)]

    def reset(self, ids=None):
        ids = list(range(self.n_streams)) if ids is None else [int(i) for i in ids]
        self.resets.append(ids)
        for i in ids:
            self._held[i] = torch.empty(0)

    def feed(self, ids, chunks, final=False):
        ids = [int(i) for i in ids]
        fin = [bool(final)] * len(ids) if isinstance(final, bool) else [bool(f) for f in final]
        assert len(set(ids)) == len(ids) == len(chunks) == len(fin) >= 1 and all(0 <= i < self.n_streams for i in ids)
        self.calls.append([(i, int(c.shape[0]), f) for i, c, f in zip(ids, chunks, fin)])
        out = []
        for i, c, f in zip(ids, chunks, fin):
            assert c.dim() == 1
            x = torch.cat([self._held[i], c.float().cpu()])
            keep = 0 if f else min(LOOK, x.shape[0])
            out.append(x[:x.shape[0] - keep])
            self._held[i] = x[x.shape[0] - keep:]
        return out


def _turns(resampler, n=3, chunk=4):
    from sesameai.turns import TurnStreams
    pool = _FakeEncPool(n, chunk)
    return pool, (TurnStreams(pool, HOP, chunk_frames=chunk) if resampler == "absent" else TurnStreams(pool, HOP, chunk_frames=chunk, resampler=resampler))


def test_feed_launches_nothing_and_pump_makes_one_resampler_call_then_one_encode_call():
    rs = _FakeResampler()
    pool, ts = _turns(rs)
    ts.feed(0, _ramp(0, 3)); ts.feed(0, _ramp(3, 2 * HOP)); ts.feed(2, _ramp(100, 100 + 3 * HOP).to(torch.int16)); ts.feed(1, _ramp(0, 0))
    assert rs.calls == [] and pool.calls == [], "feed only buffers"
    assert ts.pump() == 1 + 2
    assert rs.calls == [[(0, 2 * HOP, False), (2, 3 * HOP, False)]], "ONE call for every stream with new samples, a stream's feeds joined"
    assert pool.calls == [[(0, HOP), (2, 2 * HOP)]], "then ONE encode call: the frames the delayed samples fill"
    assert ts.buffered(0) == HOP - LOOK and ts.buffered(2) == HOP - LOOK
    assert ts.pump() == 0 and len(rs.calls) == 1 and len(pool.calls) == 1, "nothing new: no call of either kind"
    ts.feed(0, _ramp(2 * HOP, 2 * HOP + 2))                              # shorter than the look-ahead's debt: the resampler runs, the encoder not
    assert ts.pump() == 0 and rs.calls[1] == [(0, 2, False)] and len(pool.calls) == 1


def test_finish_ends_the_clip_in_the_resampler_and_the_tail_reaches_the_codes():
    rs = _FakeResampler()
    pool, ts = _turns(rs)
    n = 5 * HOP + 3
    ts.feed(1, _ramp(0, 2 * HOP + 1)); ts.pump()
    ts.feed(1, _ramp(2 * HOP + 1, n))
    seg = ts.finish(1, speaker=1, text=[4, 5])
    assert rs.calls[-1] == [(1, n - 2 * HOP - 1, True)], "what was fed since the last pump goes with final"
    T = -(-n // HOP)
    assert seg.audio_codes.shape == (32, T) and torch.equal(seg.audio_codes[0], torch.arange(T) * HOP), "every sample once, in order, tail included"
    assert pool.resets == [[1]] and ts.buffered(1) == 0
    ts.feed(1, _ramp(900, 900 + HOP + 2).to(torch.int16))               # the next turn starts from scratch
    seg2 = ts.finish(1, 0, "next")
    assert torch.equal(seg2.audio_codes[0], torch.tensor([900, 900 + HOP])) and rs.calls[-1] == [(1, HOP + 2, True)]
    with pytest.raises(ValueError, match="without samples"):
        ts.finish(0, 0, "x")
    assert all(c[0][0] != 0 for c in rs.calls), "a turn without samples makes no resampler call"


def test_without_a_resampler_turn_streams_make_todays_calls():
    seqs = []
    for resampler in ("absent", None):
        pool, ts = _turns(resampler)
        ts.feed(0, _ramp(0, 5)); ts.feed(2, _ramp(100, 100 + 2 * HOP + 3)); ts.pump()
        ts.feed(0, _ramp(5, 9 * HOP)); ts.pump(); ts.pump()
        seg = ts.finish(0, 0, [1]); ts.finish(2, 0, [1])
        seqs.append((pool.calls, pool.resets, seg.audio_codes))
    assert seqs[0][:2] == seqs[1][:2] and torch.equal(seqs[0][2], seqs[1][2])
    assert seqs[0][0] == [[(2, 2 * HOP)], [(0, 4 * HOP)], [(0, 4 * HOP)], [(0, HOP)], [(2, 3)]]


def test_open_turn_streams_without_a_rate_builds_no_resampler():
    from sesameai.generator import Generator

    class _Tok:
        class args:
            hop = HOP
        sample_rate = 24000

        def open_encode_streams(self, n, max_chunk_frames=10):
            return _FakeEncPool(n, max_chunk_frames)
    gen = Generator.__new__(Generator)
    gen._audio_tokenizer, gen.sample_rate, gen.device = _Tok(), 24000, torch.device("cpu")
    assert gen.open_turn_streams(2, chunk_frames=4).resampler is None
    assert gen.open_turn_streams(2, chunk_frames=4, sample_rate=24000).resampler is None


def _run(model_cls, lens, limit, monkeypatch, **kw):
    from sesameai import resample as rs_mod
    from sesameai.generator import Generator
    made = []
    monkeypatch.setattr(rs_mod, "ResamplerPool", lambda *a, **k: made.append(_FakeResampler(*a, **k)) or made[-1])
    scripts = _scripts(lens, 11)
    codec = _Codec([])
    gen = Generator(model_cls(scripts, 3), audio_tokenizer=codec, max_batch_size=3)
    gen.refill_row_layers = 20
    gen._text_ids = lambda text, speaker: [int(text)] * 5
    texts = list(range(len(lens)))
    chunks = list(gen.generate_many_stream(texts, [0] * len(lens), [[]] * len(lens), max_audio_length_ms=limit * 80, **kw))
    return chunks, codec.pools[0], made


@pytest.mark.parametrize("first", [None, 3])
@pytest.mark.parametrize("model_cls", [_ScriptedSlots, _ScriptedSlotsBeside])
def test_slot_streams_resample_every_decode_call_once_and_close_with_the_tail(model_cls, first, monkeypatch):
    lens = [3, 17, 0, 5, 40, 11, 20, 1, 22, 10, 33]
    kw = {} if first is None else {"first_chunk_frames": first}
    plain, pool0, made0 = _run(model_cls, lens, 30, monkeypatch, **kw)
    assert made0 == [], "no rate: no resampler is built"
    got, pool1, made = _run(model_cls, lens, 30, monkeypatch, out_sample_rate=48000, **kw)
    assert len(made) == 1 and made[0].args == (24000, 48000, 3)
    rs = made[0]
    assert pool1.calls == pool0.calls and pool1.resets == pool0.resets, "the decode pool sees the calls it saw"
    assert rs.resets == pool1.resets, "a slot's resampler stream is reset with its decode stream"
    # one resampler call per decode call, over the same slots and the PCM of that call; the others carry only empty closing chunks
    decodes = [e for e in pool1.log if e[0] in ("decode", "decode_ragged")]
    want = [[(i, 1920 * (e[2] if e[0] == "decode" else e[2][j])) for j, i in enumerate(e[1])] for e in decodes]
    with_pcm = [c for c in rs.calls if any(n for _, n, _ in c)]
    assert [[(i, n) for i, n, _ in c] for c in with_pcm] == want and len(decodes) > 10
    assert any(e[0] == "decode_ragged" for e in decodes) == (first is not None)
    bare = [c for c in rs.calls if not any(n for _, n, _ in c)]
    assert all(f for c in bare for _, _, f in c), "an empty feed is only ever a closing one"
    for i in range(len(lens)):
        a = [c for c in plain if c[0] == i]
        b = [c for c in got if c[0] == i]
        assert [c[3] for c in b] == [False] * (len(b) - 1) + [True] and len(a) == len(b)
        assert all(torch.equal(x[2], y[2]) for x, y in zip(a, b)), "the frames of every chunk are those of the plain run"
        assert torch.equal(torch.cat([c[1] for c in b]), torch.cat([c[1] for c in a])), f"request {i}: every sample once, the tail with the last chunk"
        if min(lens[i], 30) > 0:
            assert sum(c[1].numel() for c in b[:-1]) == sum(c[1].numel() for c in a[:-1]) - (LOOK if len(b) > 1 else 0), "the look-ahead is held back until the close"
    ten = [c for c in got if c[0] == 9]                                 # 10 frames: the closing chunk may be empty at 24 kHz -- and still carries the tail
    if ten[-1][2].shape[0] == 0:
        assert ten[-1][1].numel() == LOOK
    assert [c for c in got if c[0] == 2][0][1].numel() == 0, "a request whose first frame is EOS yields zero samples"
    closing = [[c for c in got if c[0] == i][-1] for i in range(len(lens)) if min(lens[i], 30) > 0]
    assert any(c[2].shape[0] == 0 and c[1].numel() == LOOK for c in closing), "some request closes with a chunk that holds the tail alone"


def test_out_dtype_needs_a_foreign_rate(monkeypatch):
    with pytest.raises(ValueError, match="out_dtype"):
        _run(_ScriptedSlots, [3], 30, monkeypatch, out_dtype=torch.int16)
