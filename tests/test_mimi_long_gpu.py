"""Full-size Mimi (MimiArgs(): hidden 512, 8 heads of 64, window 250, hop 1920) at real clip lengths against the oracle
(oracle/mimi_ref.py) and the golden vectors of tests/golden/mimi_long.pt (oracle/make_golden.py --only mimilong).

What the shorter tests of tests/test_mimi_gpu.py and tests/test_mimi_streams_gpu.py cannot see at full size: attention windows that start
above position 0 (clips of 252 .. 2250 transformer tokens against a window of 250), the stream pool's K/V ring past its wrap (600 tokens
through 270 rows), the encoder's transformer with more than 64 keys per query, the K-split products and the last SEANet stage's grids at
240,000 .. 2,160,000 output rows, and the length edges of the C ABI (T = 1, the graph limit 32 / 33, encodes of hop - 1 .. hop + 1 samples).

Tolerances are the suite's own: 2e-5 of the compared samples' peak against the oracle (fp32 both sides; the freedom is the summation
order inside a dot product), 1e-5 of the peak between a stateful stream and the codec's whole-clip decode, bit identity between the pool
and the single stream.  That these tests would notice a window or ring fault is shown without a GPU: the fixture stores how far the
oracle's compared samples move when its window is 249 / 251 / unbounded or its RoPE angle is taken modulo the ring, each >= 10 x the
2e-5 bound (tests/test_mimi_long_oracle.py; measured 23 x .. 920 x).

The oracle's decode of the 1125-frame clip (max_frames' product default, 90 s of audio) took 9.9 s on 8 CPU threads when the fixture
was generated."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
REL_TOL = 2e-5          # vs the oracle / the golden
STREAM_TOL = 1e-5       # stateful stream vs whole decode


@pytest.fixture(scope="module")
def full():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from oracle import mimi_ref as M
    from oracle.make_golden import MIMI_LONG, mimi_long_codes
    from sesameai.mimi import MimiArgs, synthetic_state_dict
    gold = torch.load(os.path.join(GOLD, "mimi_long.pt"))
    assert int(gold["weight_seed"]) == 4321 and gold["bound"] == REL_TOL
    s = M.mimi_full()
    w = M.make_weights(s, seed=4321, encoder=True)
    sd = synthetic_state_dict(MimiArgs(), seed=4321)
    assert set(w) == set(sd) and all(torch.equal(w[k], sd[k]) for k in w), "product and oracle synthetic Mimi weights differ"
    assert MimiArgs().tr_context == s.tr_context == 250 and MimiArgs().hop == s.hop == 1920
    clips = {}
    for g in gold["decode"]:
        codes = mimi_long_codes(int(g["code_seed"]), int(g["frames"]))
        assert int((codes[0] * torch.arange(1, codes.shape[-1] + 1)).sum()) == g["code_checksum"], "the seeded codes are not the fixture's"
        clips[int(g["frames"])] = (codes, g)
    assert sorted(clips) == sorted(f for f, _ in MIMI_LONG["decode"])
    return s, w, sd, gold, clips


def _codec(sd, max_frames):
    from sesameai.mimi import MimiArgs, MimiCodec
    return MimiCodec(MimiArgs(), sd, max_frames=max_frames)


def _close(got, want, what, tol=REL_TOL):
    got, want = got.detach().cpu().float(), want.detach().cpu().float()
    assert got.shape == want.shape, f"{what}: {tuple(got.shape)} vs {tuple(want.shape)}"
    peak = want.abs().max().item()
    err = (got - want).abs().max().item()
    print(f"{what}: max|d|={err:.3g} peak={peak:.3g} rel={err / peak:.2g}")
    assert err <= tol * peak, f"{what}: max abs err {err} vs peak {peak}"


def _vs_golden(pcm, g, what):
    """The stride-16 samples, the head, the tail and the last 10 frames, each against its own peak."""
    from oracle.make_golden import mimi_long_views
    v = mimi_long_views(pcm.reshape(1, 1, -1))
    _close(v["stride16"], g["pcm_stride16"], f"{what}: every 16th sample")
    _close(v["head"], g["pcm_head"], f"{what}: head")
    _close(v["tail"], g["pcm_tail"], f"{what}: tail")
    n = v["last_stride16"].shape[-1]
    _close(v["last_stride16"], g["pcm_stride16"][..., -n:], f"{what}: the last 10 frames")


def _vs_oracle(pcm, want, what):
    """A live oracle clip: all of it, and its last 10 frames (or what there is) against their own peak."""
    pcm, want = pcm.reshape(-1), want.reshape(-1)
    _close(pcm, want, what)
    _close(pcm[-19200:], want[-19200:], f"{what}: the last 10 frames")


def _rand_codes(seed, n, rows=None):
    c = torch.randint(0, 2048, (rows or 1, 32, n), generator=torch.Generator().manual_seed(seed))
    return c if rows else c[0]


@pytest.mark.parametrize("frames", [126, 150, 300])
def test_whole_decode_vs_golden(full, frames):
    """252 / 300 / 600 tokens: the last 2 / 50 / 350 queries have a window that starts above 0, nk reaches 250."""
    s, w, sd, gold, clips = full
    codes, g = clips[frames]
    pcm = _codec(sd, frames).decode(codes)
    assert pcm.shape == (1, 1, 1920 * frames) and pcm.dtype == torch.float32
    _vs_golden(pcm, g, f"whole decode, {frames} frames")


def test_whole_decode_at_the_default_max_frames_vs_golden(full):
    """The product's default buffer size (max_frames = 1125: 90 s, 2250 tokens, 2.16 M rows in the last SEANet stage), filled.
    The oracle took 9.9 s for this clip on 8 CPU threads (stored in the fixture)."""
    s, w, sd, gold, clips = full
    frames = max(clips)
    assert frames == 1125
    codes, g = clips[frames]
    pcm = _codec(sd, frames).decode(codes)
    assert pcm.shape == (1, 1, 1920 * frames)
    _vs_golden(pcm, g, f"whole decode, {frames} frames")


def test_batch_of_three_vs_oracle(full):
    from oracle import mimi_ref as M
    s, w, sd, gold, clips = full
    codes = _rand_codes(301, 150, rows=3)
    codec = _codec(sd, 150)
    pcm = codec.decode(codes)
    assert pcm.shape == (3, 1, 1920 * 150)
    want = M.decode(s, w, codes)
    for b in range(3):
        _vs_oracle(pcm[b], want[b], f"batch of 3, row {b} (150 frames) vs oracle")
    assert torch.equal(pcm[0], codec.decode(codes[:1])[0]), "row 0 of the batch is not the B = 1 decode of its codes"


RAGGED = [1, 2, 10, 3, 32, 7] + [10] * 24 + [4, 1]


def _stream(codec, codes, sched):
    codec.reset_stream()
    outs, t = [], 0
    for n in sched:
        outs.append(codec.decode_stream(codes[..., t:t + n])); t += n
    assert t == codes.shape[-1]
    return torch.cat(outs, dim=-1)


def test_single_stateful_stream_vs_golden_and_whole_decode(full):
    """The 300-frame clip through ``decode_stream``: the linear K/V cache at offsets up to 598, every chunk's queries past token 249
    windowed.  10-frame chunks and a ragged schedule with a 1-frame and a 32-frame chunk."""
    s, w, sd, gold, clips = full
    codes, g = clips[300]
    assert sum(RAGGED) == 300 and 32 in RAGGED and 1 in RAGGED
    codec = _codec(sd, 300)
    whole = codec.decode(codes)
    for name, sched in (("10-frame chunks", [10] * 30), ("ragged chunks", RAGGED)):
        got = _stream(codec, codes, sched)
        _vs_golden(got, g, f"stateful stream, {name}")
        _close(got, whole, f"stateful stream, {name}, vs the whole decode", STREAM_TOL)
        _close(got[..., -19200:], whole[..., -19200:], f"stateful stream, {name}, vs the whole decode: the last 10 frames", STREAM_TOL)


def _drive(pool, jobs):
    """jobs: {stream id: (codes (32,L), [chunk sizes], first round)}.  Every round takes the next chunk size of each stream that has
    started and is unfinished, groups the streams by it and makes ONE pool call per group; returns {stream id: pcm (hop*L,)} and the
    calls made [(ids, T, the streams' token offsets before the call)]."""
    cur = {sid: [0, 0] for sid in jobs}                 # frames done, index into the schedule
    outs = {sid: [] for sid in jobs}
    calls, rnd = [], 0
    while True:
        groups = {}
        for sid, (codes, sched, start) in jobs.items():
            if rnd >= start and cur[sid][0] < codes.shape[1]:
                groups.setdefault(sched[cur[sid][1]], []).append(sid)
        if not groups and all(cur[sid][0] >= jobs[sid][0].shape[1] for sid in jobs):
            break
        for T, ids in sorted(groups.items()):
            batch = torch.stack([jobs[sid][0][:, cur[sid][0]:cur[sid][0] + T] for sid in ids])
            calls.append((list(ids), T, [2 * cur[sid][0] for sid in ids]))
            pcm = pool.decode(ids, batch)
            assert pcm.shape == (len(ids), 1, 1920 * T) and pcm.dtype == torch.float32
            for i, sid in enumerate(ids):
                outs[sid].append(pcm[i, 0])
                cur[sid][0] += T; cur[sid][1] += 1
        rnd += 1
    return {sid: torch.cat(o) for sid, o in outs.items()}, calls


def test_stream_pool_past_the_ring_wrap_vs_golden_oracle_and_single_stream(full):
    """open_streams(4, max_chunk_frames=10): a ring of 250 + 2 * 10 = 270 rows per stream.  Stream 1 carries the 300-frame golden clip
    (600 tokens: two wraps); streams 0 and 3 carry 150-frame random clips (300 tokens: one wrap) that start in other rounds and on other
    chunk schedules, so the streams of a call sit at different ring offsets.  Golden / oracle at 2e-5 of peak, and the bits of the
    single-stream ``decode_stream`` on the same schedule."""
    from oracle import mimi_ref as M
    s, w, sd, gold, clips = full
    gcodes, g = clips[300]
    codec = _codec(sd, 300)
    pool = codec.open_streams(4, max_chunk_frames=10)
    ring = s.tr_context + 2 * pool.max_chunk_frames
    assert ring == gold["pool_ring"] == 270 and 600 // ring == 2
    jobs = {1: (gcodes[0], [10] * 30, 0),
            0: (_rand_codes(310, 150), [3, 10, 7, 10, 10, 1, 9] * 3, 0),
            3: (_rand_codes(313, 150), [10] * 15, 7)}
    assert all(sum(sc) == c.shape[1] for c, sc, _ in jobs.values())
    got, calls = _drive(pool, jobs)
    assert any(len(ids) == 3 for ids, _, _ in calls), "some call should carry all three streams"
    assert any(len(ids) > 1 and len({o % ring for o in offs}) == len(ids) and max(offs) >= ring for ids, _, offs in calls), \
        "some call should carry streams at different ring offsets, one of them past the wrap"
    _vs_golden(got[1], g, "pool stream 1 (300 frames through a 270-row ring)")
    for sid in (0, 3):
        _vs_oracle(got[sid], M.decode(s, w, jobs[sid][0][None]), f"pool stream {sid} (150 frames) vs oracle")
    for sid, (codes, sched, _) in jobs.items():
        single = _stream(codec, codes[None], sched)[0, 0]
        d = (got[sid] - single).abs().max().item()
        print(f"pool stream {sid} vs decode_stream on the same schedule: max|d|={d:.3g}")
        assert torch.equal(got[sid], single), f"pool stream {sid} is not bit-identical to decode_stream (max|d| = {d:.3g})"


def test_length_edges_vs_oracle(full):
    """T = 1, and both sides of the hipGraph replay limit of a stateless decode (32: replayed from the second call on; 33: never)."""
    from oracle import mimi_ref as M
    s, w, sd, gold, clips = full
    codec = _codec(sd, 33)
    for T in (1, 32, 33):
        codes = _rand_codes(320 + T, T, rows=1)
        first = codec.decode(codes)
        assert first.shape == (1, 1, 1920 * T)
        _vs_oracle(first, M.decode(s, w, codes), f"T = {T} vs oracle")
        for again in ("second", "third"):
            assert torch.equal(codec.decode(codes), first), f"T = {T}: the {again} decode of the same codes has other bits than the first"
    other = _rand_codes(400, 32, rows=1)                  # T = 32 is a replay by now: other codes through the replayed graph
    _vs_oracle(codec.decode(other), M.decode(s, w, other), "T = 32, other codes through the replayed graph, vs oracle")


def test_voice_prompts_encode_vs_golden_and_oracle(full):
    """A 5 s and a 10.4 s voice prompt (254 and 522 encoder-transformer tokens: up to 250 keys per query, four passes of the
    lane-strided key loop, windows that start above 0).  tests/test_mimi_long_oracle.py shows that these inputs do not sit on
    quantiser ties: >= 97 % of their frames keep all codes when the oracle's latent is nudged by 1e-6 of its peak."""
    from oracle.make_golden import mimi_long_wav
    from test_mimi_gpu import _check_codes
    s, w, sd, gold, clips = full
    for g in gold["encode"]:
        n = int(g["samples"])
        wav = mimi_long_wav(int(g["wav_seed"]), n)
        assert abs(float(wav.double().abs().sum()) - g["wav_checksum"]) <= 1e-9 * g["wav_checksum"], "the seeded prompt is not the fixture's"
        T = -(-n // 1920)
        codec = _codec(sd, T)
        codes = codec.encode(wav)
        assert codes.shape == (1, 32, T) == tuple(g["codes"].shape)
        _check_codes(codes, s, w, wav, f"full-size encode, {n} samples ({T} frames)", latent=codec.encode_latent(T))
        same = (codes.cpu() == g["codes"].long()).all(dim=1).float().mean().item()
        print(f"full-size encode, {n} samples: frames identical to the golden on all levels {same:.3f}")
        assert same >= 0.9


def test_encode_batch_of_two_and_length_edges_vs_oracle(full):
    """B = 2 at full size, and n_samples around one hop: T = ceil(n / hop) frames, codes by the ``_check_codes`` rule."""
    from oracle.make_golden import MIMI_LONG, mimi_long_wav
    from test_mimi_gpu import _check_codes
    s, w, sd, gold, clips = full
    n, seed = MIMI_LONG["encode_b2"]
    wav = mimi_long_wav(seed, n, rows=2)
    T = -(-n // 1920)
    codec = _codec(sd, T)
    codes = codec.encode(wav)
    assert codes.shape == (2, 32, T)
    _check_codes(codes, s, w, wav, f"full-size encode, B = 2, {n} samples", latent=codec.encode_latent(T))      # (the last clip's latent)
    assert [m for m, _ in MIMI_LONG["encode_edges"]] == [1919, 1920, 1921, 9600]
    for n, seed in MIMI_LONG["encode_edges"]:
        wav = mimi_long_wav(seed, n)
        T = -(-n // 1920)
        codes = codec.encode(wav)
        assert codes.shape == (1, 32, T), f"{n} samples: {tuple(codes.shape)}"
        _check_codes(codes, s, w, wav, f"full-size encode, {n} samples ({T} frame{'s' if T > 1 else ''})", latent=codec.encode_latent(T))
