"""Host logic of ``generate_many_stream(first_chunk_frames=k)`` (no GPU): scripted models stand in for the frame loop and a scripted
stream pool for MimiCodec.open_streams, as in tests/test_streams_host_logic.py.  With None the model calls, pool calls and yields are
those of the call without the keyword; with k = 2 every request's first chunk leaves in the block in which its second frame was queued,
one ragged pool call per block carries everything that is ready, and all the stream invariants hold."""
import pytest
import torch

from test_host_logic import _ScriptedSlots, _ScriptedSlotsBeside
from test_streams_host_logic import _FakePool, _FakeStreamCodec, _scripts

SIZE = 10


class _RaggedPool(_FakePool):
    """_FakePool with decode_ragged(ids, [codes (32,T_i)]) -> [(1, 1920 T_i)]: the same audio rule, per stream; logs into the shared log."""

    def __init__(self, n, max_chunk_frames, log):
        super().__init__(n, max_chunk_frames)
        self.log = log

    def reset(self, ids=None):
        super().reset(ids)
        self.log.append(("reset", tuple(self.resets[-1])))

    def decode(self, ids, codes):
        self.log.append(("decode", tuple(ids), int(codes.shape[2])))
        return super().decode(ids, codes)

    def decode_ragged(self, ids, codes, lengths=None):
        ids = list(ids)
        assert lengths is None and len(codes) == len(ids) == len(set(ids)) and all(0 <= i < self.n for i in ids)
        lens = [int(c.shape[1]) for c in codes]
        assert all(c.shape[0] == 32 and 1 <= t <= self.max_chunk for c, t in zip(codes, lens))
        self.log.append(("decode_ragged", tuple(ids), tuple(lens)))
        out = []
        for j, i in enumerate(ids):
            pos = torch.arange(self.pos[i], self.pos[i] + lens[j])
            out.append((10000.0 * pos + codes[j][0].float()).repeat_interleave(1920)[None])
            self.pos[i] += lens[j]
        return out


class _Codec(_FakeStreamCodec):
    def __init__(self, log):
        super().__init__()
        self.log = log

    def open_streams(self, n, max_chunk_frames=10):
        self.pools.append(_RaggedPool(n, max_chunk_frames, self.log))
        return self.pools[-1]


class _Recording:
    """A scripted model whose every call is written to the shared log (name and its plain-number arguments)."""

    def __init__(self, inner, log):
        self.__dict__["_inner"], self.__dict__["_log"] = inner, log

    def __getattr__(self, name):
        v = getattr(self._inner, name)
        if not callable(v) or name.startswith("_") or isinstance(v, type):
            return v

        def call(*a, **k):
            self._log.append((name,) + tuple(x if isinstance(x, (int, float)) else tuple(x) for x in a if isinstance(x, (int, float, list))))
            return v(*a, **k)
        return call


LENS = [3, 17, 0, 5, 40, 11, 20, 1, 22, 10, 33, 2]
LIMIT = 30


def _run(model_cls, **kw):
    """One run over LENS through 3 slots.  Returns (log of model calls / pool calls / yields in order, chunks per request, scripts, model)."""
    from sesameai.generator import Generator
    scripts = _scripts(LENS, 11)
    log: list = []
    inner = model_cls(scripts, 3)
    codec = _Codec(log)
    gen = Generator(_Recording(inner, log), audio_tokenizer=codec, max_batch_size=3)
    gen.refill_row_layers = 20
    gen._text_ids = lambda text, speaker: [int(text)] * 5
    texts = list(range(len(LENS)))
    got = {i: [] for i in texts}
    for i, pcm, frames, last in gen.generate_many_stream(texts, [0] * len(LENS), [[]] * len(LENS), max_audio_length_ms=LIMIT * 80, **kw):
        assert pcm.dtype == torch.float32 and pcm.shape == (1920 * frames.shape[0],) and frames.dtype == torch.int32
        log.append(("yield", i, tuple(frames[:, 0].tolist()), tuple(pcm[::1920].tolist()), last))
        got[i].append((pcm, frames, last))
    return log, got, scripts, inner


@pytest.mark.parametrize("model_cls", [_ScriptedSlots, _ScriptedSlotsBeside])
def test_none_makes_exactly_the_calls_of_the_path_without_the_keyword(model_cls):
    plain, _, _, _ = _run(model_cls)
    with_none, _, _, _ = _run(model_cls, first_chunk_frames=None)
    assert plain == with_none
    assert any(e[0] == "decode" for e in plain) and not any(e[0] == "decode_ragged" for e in plain), "None keeps the uniform pool calls"
    assert sum(e[0] == "step" for e in plain) > 50 and sum(e[0] == "yield" for e in plain) >= len(LENS)
    # and the keyword is no no-op: k = 2 on the same script makes other calls
    short, _, _, _ = _run(model_cls, first_chunk_frames=2)
    assert short != plain and any(e[0] == "decode_ragged" for e in short) and not any(e[0] == "decode" for e in short)


@pytest.mark.parametrize("model_cls", [_ScriptedSlots, _ScriptedSlotsBeside])
def test_k2_first_chunks_leave_in_the_block_of_their_second_frame(model_cls):
    k = 2
    log, got, scripts, model = _run(model_cls, first_chunk_frames=k)
    texts = list(range(len(LENS)))
    # exactly one last chunk per request, nothing after it; frames in order and complete; stream state from 0 for every request
    for i, n in enumerate(LENS):
        lasts = [last for _, _, last in got[i]]
        assert lasts.count(True) == 1 and lasts[-1], f"request {i}: {lasts}"
        want = scripts[i][: min(n, LIMIT)].to(torch.int32)
        frames = torch.cat([f for _, f, _ in got[i]])
        assert torch.equal(frames, want), f"request {i}"
        pcm = torch.cat([p for p, _, _ in got[i]])
        assert torch.equal(pcm[::1920], 10000.0 * torch.arange(want.shape[0]) + want[:, 0].float()), f"request {i}: stream state"
        # chunk lengths: the first >= k (or the whole request), later ones SIZE, the last whatever remains
        sizes = [f.shape[0] for _, f, _ in got[i]]
        total = want.shape[0]
        assert min(k, total) <= sizes[0] <= SIZE, f"request {i}: first chunk of {sizes[0]} frames"
        assert all(sz == SIZE for sz in sizes[1:-1]) and sizes[-1] <= SIZE, f"request {i}: {sizes}"
    # the block in which a request's second frame was queued: the read that covers the global index of that frame
    reads = [(pos, e[2], e[3]) for pos, e in enumerate(log) if e[0] == "read_frames"]        # (place in the log, first, n)
    assert all(n <= SIZE for _, _, n in reads) and any(n < SIZE for _, _, n in reads), "some blocks must have been cut short"
    for i, n in enumerate(LENS):
        total = min(n, LIMIT)
        if total < k:
            continue
        second = scripts[i][k - 1].to(torch.int32)
        g2 = [g for g, row in enumerate(model.hist) if any(torch.equal(f, second) for f in row.values())]
        assert len(g2) == 1, f"request {i}: its frame {k - 1} should be in the history once"
        block = [b for b, (_, first, cnt) in enumerate(reads) if first <= g2[0] < first + cnt]
        assert len(block) == 1
        b = block[0]
        first_yield = next(pos for pos, e in enumerate(log) if e[0] == "yield" and e[1] == i)
        # (block b's audio is decoded after block b + 1's steps were queued and before block b + 1 is read)
        assert reads[b][0] < first_yield and (b + 1 == len(reads) or first_yield < reads[b + 1][0]), \
            f"request {i}: second frame queued in block {b}, first chunk yielded at log place {first_yield}, reads at {[r[0] for r in reads[b:b + 3]]}"
    # at most one pool call per block, except where a slot held more than SIZE frames (then the slot is in both calls)
    per_block, cur = [], []
    for e in log:
        if e[0] == "read_frames":
            per_block.append(cur); cur = []
        elif e[0] == "decode_ragged":
            cur.append(e)
    per_block.append(cur)
    assert sum(len(c) for c in per_block) >= 10
    for calls in per_block:
        for a, b2 in zip(calls, calls[1:]):
            assert set(a[1]) & set(b2[1]), f"two pool calls in one block without a slot that held more than {SIZE} frames: {calls}"
    assert any(len(set(e[2])) > 1 for c in per_block for e in c), "some call should carry chunks of different lengths"
    # a stream is reset when a new request takes its slot: once per request that held a slot (an empty utterance holds one only where
    # its frame 0 is sampled by the batch, beside the loop)
    resets = [s for e in log if e[0] == "reset" for s in e[1]]
    assert len(texts) - LENS.count(0) <= len(resets) <= len(texts)


@pytest.mark.parametrize("bad", [0, 10, 11, -1])
def test_k_outside_1_to_size_raises(bad):
    from sesameai.generator import Generator
    gen = Generator(_ScriptedSlots(_scripts([3], 1), 1), audio_tokenizer=_Codec([]))
    gen._text_ids = lambda text, speaker: [0] * 5
    with pytest.raises(ValueError, match="first_chunk_frames"):
        next(gen.generate_many_stream([0], [0], [[]], first_chunk_frames=bad))
