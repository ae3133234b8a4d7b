"""Multi-stream Mimi decode: a pool of stateful streams decoded by one launch chain per call (include/mimi_hip.h mimi_pool_*,
sesameai.mimi.MimiStreamPool) against the oracle (oracle/mimi_ref.py), the codec's own whole-clip decode and the single-stream
``decode_stream``.  Tolerances are those of tests/test_mimi_gpu.py: 2e-5 of the clip's peak against the oracle (fp32 summation order
inside a dot product), 1e-5 of the peak between a stateful stream and the whole decode."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
REL_TOL = 2e-5          # vs the oracle
STREAM_TOL = 1e-5       # stateful stream vs whole decode


@pytest.fixture(scope="module")
def tiny():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from oracle import mimi_ref as M
    from sesameai.mimi import MimiCodec, mimi_tiny_args, synthetic_state_dict
    s = M.mimi_tiny()
    w = M.make_weights(s, seed=4321, encoder=True)
    return s, w, MimiCodec(mimi_tiny_args(), synthetic_state_dict(mimi_tiny_args(), seed=4321), max_frames=64)


def _close(got, want, what, tol=REL_TOL):
    got, want = got.detach().cpu().float(), want.detach().cpu().float()
    assert got.shape == want.shape, f"{what}: {tuple(got.shape)} vs {tuple(want.shape)}"
    peak = want.abs().max().item()
    err = (got - want).abs().max().item()
    print(f"{what}: max|d|={err:.3g} peak={peak:.3g} rel={err / peak:.2g}")
    assert err <= tol * peak, f"{what}: max abs err {err} vs peak {peak}"


def _codes(seed, n):
    return torch.randint(0, 2048, (32, n), generator=torch.Generator().manual_seed(seed))


def _drive(pool, jobs):
    """jobs: {stream id: (codes (32,L), [chunk sizes])}.  Every round takes each unfinished stream's next chunk size, groups the
    streams by it and makes ONE pool call per group; returns {stream id: pcm (hop*L,)} and the calls made [(ids, T)]."""
    cur = {sid: [0, 0] for sid in jobs}                 # frames done, index into the schedule
    outs = {sid: [] for sid in jobs}
    calls = []
    while True:
        groups = {}
        for sid, (codes, sched) in jobs.items():
            if cur[sid][0] < codes.shape[1]:
                groups.setdefault(sched[cur[sid][1]], []).append(sid)
        if not groups:
            break
        for T, ids in sorted(groups.items()):
            batch = torch.stack([jobs[sid][0][:, cur[sid][0]:cur[sid][0] + T] for sid in ids])
            pcm = pool.decode(ids, batch)
            assert pcm.shape == (len(ids), 1, pcm.shape[-1]) and pcm.dtype == torch.float32
            for i, sid in enumerate(ids):
                outs[sid].append(pcm[i, 0])
                cur[sid][0] += T; cur[sid][1] += 1
            calls.append((list(ids), T))
    return {sid: torch.cat(o) for sid, o in outs.items()}, calls


def test_pool_of_ragged_streams_vs_oracle_and_whole_decode(tiny):
    """Five streams of 23..40 frames, each on its own ragged chunk schedule, so the calls carry changing subsets of the streams;
    streams 1 and 3 are abandoned mid-way, reset and started on new sequences.  Every sequence's concatenated chunks are the
    oracle's decode of it (2e-5 of peak) and the codec's own whole-clip decode (1e-5 of peak)."""
    from oracle import mimi_ref as M
    s, w, codec = tiny
    pool = codec.open_streams(5, max_chunk_frames=10)
    assert s.hop == 1920
    first = {0: (_codes(20, 23), [1, 2, 10, 3, 1, 6]),
             1: (_codes(21, 12), [2, 10]),                              # the part of a 30-frame sequence decoded before the reset
             2: (_codes(22, 40), [10, 10, 3, 7, 1, 9]),
             3: (_codes(23, 7), [3, 1, 3]),
             4: (_codes(24, 31), [5, 1, 1, 10, 4, 10])}
    assert all(sum(sc) == c.shape[1] for c, sc in first.values())
    got, calls = _drive(pool, first)
    assert len({tuple(ids) for ids, _ in calls}) >= 4 and len({T for _, T in calls}) >= 5, "the schedules should mix subsets and chunk sizes"
    pool.reset([1, 3])
    second = {1: (_codes(31, 29), [10, 9, 10]), 3: (_codes(33, 36), [4, 10, 2, 10, 10])}
    got2, _ = _drive(pool, second)
    for name, res, jobs in (("first", got, first), ("after reset", got2, second)):
        for sid, (codes, _) in jobs.items():
            whole = codec.decode(codes[None])[0, 0]
            _close(res[sid], M.decode(s, w, codes[None])[0, 0], f"{name}: stream {sid} ({codes.shape[1]} frames) vs oracle")
            _close(res[sid], whole, f"{name}: stream {sid} vs the codec's whole-clip decode", STREAM_TOL)


def test_a_streams_pcm_does_not_depend_on_its_company(tiny):
    """The same stream decoded alone, with four others and at another place in the id list: bit-identical -- and identical to the
    single-stream ``decode_stream`` on the same chunk schedule (the summation order depends on the product's shape alone)."""
    s, w, codec = tiny
    codes, sched = _codes(40, 23), [1, 2, 10, 3, 1, 6]
    pool = codec.open_streams(5, max_chunk_frames=10)

    def run(ids, me):
        pool.reset()
        others = {sid: _codes(50 + sid, 23) for sid in ids if sid != me}
        outs, t = [], 0
        for n in sched:
            batch = torch.stack([(codes if sid == me else others[sid])[:, t:t + n] for sid in ids])
            outs.append(pool.decode(ids, batch)[ids.index(me), 0]); t += n
        return torch.cat(outs)

    alone = run([2], 2)
    with_four = run([0, 1, 2, 3, 4], 2)
    elsewhere = run([4, 2, 0], 2)
    other_id = run([3, 1], 1)
    assert torch.equal(alone, with_four), f"alone vs with 4 others: max|d|={(alone - with_four).abs().max().item():.3g}"
    assert torch.equal(alone, elsewhere), f"alone vs another position: max|d|={(alone - elsewhere).abs().max().item():.3g}"
    assert torch.equal(alone, other_id), "the same codes on another stream id"
    codec.reset_stream()
    outs, t = [], 0
    for n in sched:
        outs.append(codec.decode_stream(codes[None, :, t:t + n])[0, 0]); t += n
    single = torch.cat(outs)
    print(f"pool vs decode_stream: max|d|={(alone - single).abs().max().item():.3g}")
    assert torch.equal(alone, single)


def test_streams_far_longer_than_the_ring(tiny):
    """The tiny codec's attention window is 6 tokens; with max_chunk_frames = 3 a stream's K/V ring holds 6 + 2*3 = 12 tokens, so
    a 45-frame stream (90 tokens) goes round it 7 times -- and a single handle of max_frames = 3 could not carry it at all."""
    from oracle import mimi_ref as M
    s, w, codec = tiny
    L, mc = 45, 3
    ring_tokens = s.tr_context + 2 * mc
    assert (2 * L) // ring_tokens >= 2, "the stream must cross the ring's wrap at least twice"
    assert L > 10 * mc
    pool = codec.open_streams(3, max_chunk_frames=mc)
    jobs = {0: (_codes(60, L), [3] * 15), 2: (_codes(62, L), [2, 3, 1] * 7 + [3]), 1: (_codes(61, 9), [3, 3, 3])}
    got, _ = _drive(pool, jobs)
    for sid in (0, 2):
        want = M.decode(s, w, jobs[sid][0][None])[0, 0]
        _close(got[sid], want, f"stream {sid}: {L} frames through a {ring_tokens}-token ring vs oracle")
        _close(got[sid][-10 * 1920:], want[-10 * 1920:], f"stream {sid}: the last 10 frames")


def test_full_size_pool_vs_golden_and_oracle():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from oracle import mimi_ref as M
    from sesameai.mimi import MimiArgs, MimiCodec, synthetic_state_dict
    gold = torch.load(os.path.join(GOLD, "mimi_full.pt"))
    codec = MimiCodec(MimiArgs(), synthetic_state_dict(MimiArgs(), seed=int(gold["weight_seed"])), max_frames=32)
    pool = codec.open_streams(8, max_chunk_frames=10)
    gcodes = gold["codes"][0]
    assert gcodes.shape[1] == 10
    rnd = {sid: _codes(70 + sid, 20) for sid in range(8) if sid != 5}
    ids = [0, 1, 2, 3, 4, 5, 6, 7]
    pcm = pool.decode(ids, torch.stack([gcodes if sid == 5 else rnd[sid][:, :10] for sid in ids]))
    mine = pcm[5:6]
    _close(mine[..., ::16], gold["pcm_stride16"], "golden stream in an 8-stream pool (every 16th sample)")
    _close(mine[..., :4096], gold["pcm_head"], "golden stream head")
    _close(mine[..., -4096:], gold["pcm_tail"], "golden stream tail")
    rest = [sid for sid in ids if sid != 5]
    pcm2 = pool.decode(rest, torch.stack([rnd[sid][:, 10:] for sid in rest]))
    got = torch.cat([pcm[2, 0], pcm2[rest.index(2), 0]])
    s = M.mimi_full()
    w = M.make_weights(s, seed=int(gold["weight_seed"]), encoder=False)
    _close(got, M.decode(s, w, rnd[2][None])[0, 0], "random stream 2 (two 10-frame chunks) vs the full-size oracle")


def test_bad_arguments_are_refused_and_leave_the_pool_usable(tiny):
    from sesameai._abi import CsmError
    s, w, codec = tiny
    pool = codec.open_streams(4, max_chunk_frames=5)
    codes = _codes(80, 8)
    a = pool.decode([1], codes[None, :, :3])
    for ids, T, word in (([1, 1], 2, "duplicate"), ([1, 4], 2, "outside"), ([-1], 2, "outside"), ([1], 6, "max_chunk_frames"),
                         ([0, 1, 2, 3, 0], 2, "n_streams")):
        with pytest.raises(CsmError, match=word):
            pool.decode(ids, torch.stack([codes[:, :T]] * len(ids)))
    with pytest.raises(CsmError, match="duplicate"):
        pool.reset([2, 2])
    with pytest.raises(CsmError, match="n_streams"):
        codec.open_streams(0)
    b = pool.decode([1], codes[None, :, 3:])                            # the refused calls moved nothing: the stream goes on
    _close(torch.cat([a, b], dim=-1), codec.decode(codes[None]), "stream continued after refused calls", STREAM_TOL)


@pytest.mark.parametrize("beside", [True, False], ids=["refill_beside_the_loop", "refill_slot"])
def test_generate_many_stream_end_to_end_tiny(tiny, beside):
    """12 requests through a batch of 4 (tiny model, sampled, seeded; lengths set by each request's own limit, one of them 0):
    audio leaves the batch chunk by chunk while it keeps generating, and what each request got is its whole-clip decode."""
    from oracle import mimi_ref as M
    from sesameai.generator import Generator, Segment
    from sesameai.models import Model, csm_tiny_args
    s, w, codec = tiny
    model = Model(csm_tiny_args(), None, max_frames=64, max_prefill_rows=128)
    gen = Generator(model, audio_tokenizer=codec, max_batch_size=4)
    if beside:
        assert model.supports_refill_beside_the_loop(4), "the tiny model's batch of 4 should take the refill beside the loop"
    gen.refill_beside_the_loop = beside
    gen.refill_row_layers = 10
    g = torch.Generator().manual_seed(21)
    lens = [27, 3, 10, 0, 14, 20, 1, 9, 11, 30, 5, 21]
    texts = [torch.randint(0, 1000, (4 + i % 5,), generator=g).tolist() for i in range(len(lens))]
    ctxs = [[Segment(speaker=1, text=torch.randint(0, 1000, (3,), generator=g).tolist(), audio_codes=torch.randint(0, 2048, (32, 2 + i % 4), generator=g))]
            for i in range(len(lens))]
    ms = [n * 80 for n in lens]
    prompts = [gen._build_prompt(t, 1, c) for t, c in zip(texts, ctxs)]

    model.seed(5)
    before = gen.generate_codes_continuous(prompts, lens, 0.9, 50)
    model.seed(5)
    same_blocks = gen.generate_codes_continuous(prompts, lens, 0.9, 50, poll=gen._stream_buffer_size)
    assert [f.shape[0] for f in before] == lens, "the random tiny model is not expected to sample an all-zero frame"

    model.seed(5)
    got = {i: [] for i in range(len(lens))}
    closed, open_when_first_audio = [], None
    for i, pcm, frames, last in gen.generate_many_stream(texts, [1] * len(lens), ctxs, max_audio_length_ms=ms, temperature=0.9, topk=50):
        assert i not in closed, f"request {i}: a chunk after its last one"
        assert pcm.dim() == 1 and pcm.dtype == torch.float32 and pcm.shape[0] == 1920 * frames.shape[0]
        assert frames.dtype == torch.int32 and frames.device.type == "cpu" and frames.shape[1:] == (32,)
        assert frames.shape[0] == 10 or (last and frames.shape[0] < 10), f"request {i}: a {frames.shape[0]}-frame chunk, last={last}"
        if open_when_first_audio is None and frames.shape[0]:
            open_when_first_audio = len(lens) - len(closed)
        if last:
            closed.append(i)
        got[i].append((pcm, frames))
    assert sorted(closed) == list(range(len(lens))), "exactly one last chunk per request, none dropped"
    assert open_when_first_audio is not None and open_when_first_audio >= len(lens) - 4, "the first audio must leave while most requests are unfinished"
    assert len(got[3]) == 1 and got[3][0][0].numel() == 0 and got[3][0][1].shape == (0, 32), "the empty utterance: one empty last chunk"
    for i, n in enumerate(lens):
        frames = torch.cat([f for _, f in got[i]])
        assert torch.equal(frames, same_blocks[i]), f"request {i}: the streamed frames are not those of the same seeded run collected"
        if n == 0:
            continue
        pcm = torch.cat([p for p, _ in got[i]])
        codes = frames.t().contiguous()[None].long()
        _close(pcm, codec.decode(codes)[0, 0], f"request {i} ({n} frames): chunks vs the codec's whole-clip decode", STREAM_TOL)
        _close(pcm, M.decode(s, w, codes.clamp(max=2047))[0, 0], f"request {i}: chunks vs oracle")
    # generate_many's own path is untouched by the stream run in between
    model.seed(5)
    after = gen.generate_codes_continuous(prompts, lens, 0.9, 50)
    assert all(torch.equal(a, b) for a, b in zip(before, after))
