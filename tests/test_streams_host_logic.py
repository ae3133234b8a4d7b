"""Host logic of Generator.generate_many_stream (no GPU): scripted models stand in for the frame loop (tests/test_host_logic.py) and a
scripted stream pool for MimiCodec.open_streams.  What is checked is the bookkeeping: which frames go to which pool stream, when a
stream is reset, how slots are grouped into pool calls, and that the collecting iterators still return what they returned."""
import pytest
import torch

from test_host_logic import _FakeCodec, _ScriptedSlots, _ScriptedSlotsBeside


class _FakePool:
    """decode(ids, codes (n,32,T)) -> (n,1,1920 T): every sample of a frame = 10000 * (the frame's position in its stream since the
    last reset) + the frame's first code -- so the audio shows both the frame and the stream state it was decoded with."""

    def __init__(self, n, max_chunk_frames):
        self.n, self.max_chunk, self.pos, self.calls, self.resets = n, max_chunk_frames, [0] * n, [], []

    def reset(self, ids=None):
        ids = list(range(self.n)) if ids is None else list(ids)
        assert len(set(ids)) == len(ids)
        self.resets.append(ids)
        for i in ids:
            self.pos[i] = 0

    def decode(self, ids, codes):
        ids = list(ids)
        n, K, T = codes.shape
        assert n == len(ids) == len(set(ids)) and K == 32 and 1 <= T <= self.max_chunk and all(0 <= i < self.n for i in ids)
        self.calls.append((ids, T))
        out = []
        for j, i in enumerate(ids):
            pos = torch.arange(self.pos[i], self.pos[i] + T)
            out.append((10000.0 * pos + codes[j, 0].float()).repeat_interleave(1920))
            self.pos[i] += T
        return torch.stack(out).unsqueeze(1)


class _FakeStreamCodec(_FakeCodec):
    def __init__(self):
        self.pools = []

    def open_streams(self, n, max_chunk_frames=10):
        self.pools.append(_FakePool(n, max_chunk_frames))
        return self.pools[-1]


def _scripts(lens, seed, lo=8):
    g = torch.Generator().manual_seed(seed)
    out = []
    for n in lens:
        sc = torch.randint(lo, 2048, (n + 1, 32), generator=g); sc[n] = 0
        out.append(sc)
    return out


@pytest.mark.parametrize("model_cls", [_ScriptedSlots, _ScriptedSlotsBeside])
def test_generate_many_stream_hands_out_every_request_in_order_chunk_by_chunk(model_cls):
    from sesameai.generator import Generator
    lens = [3, 17, 0, 5, 40, 11, 20, 1, 22, 10, 33]
    limit = 30
    scripts = _scripts(lens, 11)
    model = model_cls(scripts, 3)
    codec = _FakeStreamCodec()
    gen = Generator(model, audio_tokenizer=codec, max_batch_size=3)
    gen.refill_row_layers = 20
    gen._text_ids = lambda text, speaker: [int(text)] * 5              # the scripted models know a prompt by its first text token
    texts = list(range(len(lens)))
    got = {i: [] for i in texts}
    closed, first_seen_at = [], {}
    for n_yield, (i, pcm, frames, last) in enumerate(gen.generate_many_stream(texts, [0] * len(lens), [[]] * len(lens), max_audio_length_ms=limit * 80)):
        assert i not in closed, "a chunk after the request's last one"
        assert pcm.dtype == torch.float32 and pcm.shape == (1920 * frames.shape[0],) and frames.dtype == torch.int32
        if not last:
            assert frames.shape[0] == 10
        else:
            closed.append(i)
        assert frames.shape[0] <= 10
        first_seen_at.setdefault(i, n_yield)
        got[i].append((pcm, frames))
    assert sorted(closed) == texts, "every request ends with exactly one last chunk"
    for i, n in enumerate(lens):
        want = scripts[i][: min(n, limit)].to(torch.int32)
        frames = torch.cat([f for _, f in got[i]])
        assert torch.equal(frames, want), f"request {i}"
        pcm = torch.cat([p for p, _ in got[i]])
        # position in the stream counts from 0 for every request: its slot's stream was reset when it took the slot
        assert torch.equal(pcm[::1920], 10000.0 * torch.arange(want.shape[0]) + want[:, 0].float()), f"request {i}: stream state"
    assert len(got[2]) == 1 and got[2][0][0].numel() == 0                # the empty utterance: one empty closing chunk
    assert len(got[9]) in (1, 2) and sum(f.shape[0] for _, f in got[9]) == 10
    pool = codec.pools[0]
    assert len(codec.pools) == 1 and pool.n == 3 and pool.max_chunk == 10
    assert any(len(ids) > 1 for ids, _ in pool.calls), "slots that are ready together go into one pool call"
    assert all(T == 10 or T < 10 for _, T in pool.calls)
    assert first_seen_at[4] < max(first_seen_at.values()), "the long request's audio starts before later requests have begun"
    # the collecting iterator is untouched by a stream run in between: same results before and after
    prompts = []
    for i in texts:
        t = torch.zeros(5, 33, dtype=torch.long); t[:, 32] = i
        prompts.append((t, torch.zeros(5, 33, dtype=torch.bool)))
    out = gen.generate_codes_continuous(prompts, limit, 0.9, 50)
    for i, n in enumerate(lens):
        assert torch.equal(out[i], scripts[i][: min(n, limit)].to(torch.int32))
    assert len(codec.pools) == 1, "the pool is kept for the next call"


def test_generate_many_stream_decodes_after_the_next_blocks_steps_are_queued():
    """The pool call for block k is made once block k+1's frame steps have been queued (they run beside it), not before."""
    from sesameai.generator import Generator
    scripts = _scripts([35, 35], 12)
    model = _ScriptedSlots(scripts, 2)
    codec = _FakeStreamCodec()
    gen = Generator(model, audio_tokenizer=codec, max_batch_size=2)
    gen._text_ids = lambda text, speaker: [int(text)] * 5
    steps_at_decode = []
    open_streams = codec.open_streams

    def spying(n, max_chunk_frames=10):
        pool = open_streams(n, max_chunk_frames)
        dec = pool.decode
        pool.decode = lambda ids, codes: (steps_at_decode.append(len(model.hist)), dec(ids, codes))[1]
        return pool
    codec.open_streams = spying
    chunks = list(gen.generate_many_stream([0, 1], [0, 0], [[], []], max_audio_length_ms=40 * 80))
    # frame 0 comes with the prompt, every block adds 10: the first block ends at 11 frames, and its decode is made at 21
    assert steps_at_decode[0] == 21 and steps_at_decode[1] == 31, steps_at_decode
    assert codec.pools[0].calls[0] == ([0, 1], 10)
    assert [c[3] for c in chunks].count(True) == 2


def test_generate_many_stream_needs_a_codec_with_stream_pools():
    from sesameai.generator import Generator
    gen = Generator(_ScriptedSlots(_scripts([3], 1), 1), audio_tokenizer=_FakeCodec())
    gen._text_ids = lambda text, speaker: [0] * 5
    with pytest.raises(RuntimeError, match="open_streams"):
        next(gen.generate_many_stream([0], [0], [[]]))
