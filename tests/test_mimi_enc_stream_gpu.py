"""mimi_enc_pool_* (include/mimi_hip.h; MimiCodec.open_encode_streams, Generator.open_turn_streams): a pool of stateful Mimi encode streams
fed by one launch chain per call.

The acceptance criterion is bit identity: a stream's columns, concatenated over its calls, are ``torch.equal`` to ``MimiCodec.encode`` of its
concatenated samples -- for every chunk schedule, every company in the call and every position in the list.  The single encode is graded
against the oracle (oracle/mimi_ref.py) by tests/test_mimi_gpu.py and tests/test_mimi_long_gpu.py; the seam clips are graded against it once
more here by the same rule (``_check_codes``).  That no piece of carried state, no edge mode and no RoPE slip could hide is shown on the oracle
alone by tests/test_enc_stream_oracle.py, on the clip and the cuts of the first test here."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
HOP = 1920
SEAM_SAMPLES = [1, 1919, 1920, 1921, 3 * 1920 + 777, 960 * 31, 960 * 32 + 1]        # one hop +- 1; 31 / 33 tokens: the 32-row tile seam
SEAM_FRAMES = [1, 1, 1, 2, 4, 16, 17]
TAILS = [1, 777, 960, 961]


def _clip(seed, n):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)) * 0.3


def _new_tiny(max_frames=64):
    from sesameai.mimi import MimiCodec, mimi_tiny_args, synthetic_state_dict
    return MimiCodec(mimi_tiny_args(), synthetic_state_dict(mimi_tiny_args(), seed=4321), max_frames=max_frames)


def _single(codec, clip):
    return codec.encode(clip.view(1, 1, -1))[0]


@pytest.fixture(scope="module")
def tiny():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from oracle import mimi_ref as M
    s = M.mimi_tiny()
    w = M.make_weights(s, seed=4321, encoder=True)
    codec = _new_tiny()
    assert codec.args.tr_context == 6 and codec.args.hop == HOP
    clips = [_clip(100 + i, n) for i, n in enumerate(SEAM_SAMPLES)]
    alone = [_single(codec, c) for c in clips]                          # computed once, shared, never changed
    assert [a.shape[1] for a in alone] == SEAM_FRAMES
    return s, w, codec, clips, alone


def _stream(pool, sid, clip, frames):
    """clip through stream ``sid`` alone, cut after ``frames`` [f0, f1, ..] frames (the last chunk takes the rest); the columns joined"""
    out, at = [], 0
    for f in frames[:-1]:
        out += pool.encode([sid], [clip[at:at + f * HOP]]); at += f * HOP
    out += pool.encode([sid], [clip[at:]])
    return torch.cat(out, dim=1)


def test_schedules_through_a_wrapping_ring(tiny):
    s, w, codec, _, _ = tiny
    pool = codec.open_encode_streams(2, max_chunk_frames=3)             # ring: tr_context + 2 * 3 = 12 tokens; the stream runs to 24
    x = _clip(301, 12 * HOP)
    want = _single(codec, x)
    for sid, frames in ((0, [3, 3, 3, 3]), (1, [2, 3, 1, 3, 3]), (0, [1] * 12)):
        pool.reset([sid])
        got = _stream(pool, sid, x, frames)
        assert got.dtype == torch.int64 and got.shape == (32, 12)
        assert torch.equal(got, want), f"chunks of {frames} frames: columns {(got != want).any(dim=0).nonzero().flatten().tolist()} differ"
        assert not pool.ended(sid)


@pytest.mark.parametrize("r", TAILS)
def test_a_partial_last_frame_follows_the_whole_clip_rule(tiny, r):
    s, w, codec, _, _ = tiny
    pool = codec.open_encode_streams(2, max_chunk_frames=3)
    x = _clip(310 + r, 4 * HOP + r)
    want = _single(codec, x)
    assert want.shape == (32, 5)
    got = _stream(pool, 0, x, [2, 3])                                   # the final chunk: two frames and the tail
    assert torch.equal(got, want), f"tail of {r} samples behind two frames of its chunk"
    got = _stream(pool, 1, x, [2, 2, 1])                                # ... and the tail alone
    assert torch.equal(got, want), f"tail of {r} samples as a chunk of its own"
    assert pool.ended(0) and pool.ended(1)


def test_seam_clips_one_call_on_fresh_streams_and_the_oracle(tiny):
    from test_mimi_gpu import _check_codes
    s, w, codec, clips, alone = tiny
    pool = codec.open_encode_streams(len(clips), max_chunk_frames=17)
    got = pool.encode(range(len(clips)), clips)                         # 42 frames: the 32-row tile seam inside a stream and between streams
    lat = pool.encode_latent(sum(SEAM_FRAMES)).split(SEAM_FRAMES)       # the call's latent: stream i owns rows [F_i, F_i + T_i)
    for i, (g, a, c) in enumerate(zip(got, alone, clips)):
        assert g.shape == (32, SEAM_FRAMES[i]) and torch.equal(g, a), f"clip {i} ({c.shape[0]} samples) differs from its single encode"
        _check_codes(g.unsqueeze(0), s, w, c.view(1, 1, -1), f"encode stream, clip {i} ({c.shape[0]} samples)", latent=lat[i])
        assert pool.ended(i) == (c.shape[0] % HOP != 0)
    pool.reset()
    for i, (c, a) in enumerate(zip(clips, alone)):                      # each alone, on a stream that has just been used
        (g,) = pool.encode([i], [c])
        assert torch.equal(g, a), f"clip {i} alone"


def test_company_and_order_do_not_matter(tiny):
    s, w, codec, _, _ = tiny
    pool = codec.open_encode_streams(3, max_chunk_frames=17)
    A, B, Cc = _clip(401, 16 * HOP + 777), _clip(402, 3 * HOP), _clip(403, 18 * HOP)
    wA, wB, wC = _single(codec, A), _single(codec, B), _single(codec, Cc)
    cutA, cutB, cutC = 15 * HOP, 1 * HOP, 17 * HOP
    # T = 15, 1, 17, then the rest of each in the reversed list
    a1, b1, c1 = pool.encode([0, 1, 2], [A[:cutA], B[:cutB], Cc[:cutC]])
    c2, b2, a2 = pool.encode([2, 1, 0], [Cc[cutC:], B[cutB:], A[cutA:]])
    for what, got, want in (("A", torch.cat([a1, a2], 1), wA), ("B", torch.cat([b1, b2], 1), wB), ("C", torch.cat([c1, c2], 1), wC)):
        assert torch.equal(got, want), f"{what} in company: columns {(got != want).any(dim=0).nonzero().flatten().tolist()} differ"
    # the same schedules reversed in both calls, on other streams
    pool.reset()
    c1, b1, a1 = pool.encode([0, 2, 1], [Cc[:cutC], B[:cutB], A[:cutA]])
    a2, b2, c2 = pool.encode([1, 2, 0], [A[cutA:], B[cutB:], Cc[cutC:]])
    assert torch.equal(torch.cat([a1, a2], 1), wA) and torch.equal(torch.cat([b1, b2], 1), wB) and torch.equal(torch.cat([c1, c2], 1), wC)
    # alone
    pool.reset()
    for sid, (x, cut, want) in enumerate(((A, cutA, wA), (B, cutB, wB), (Cc, cutC, wC))):
        got = torch.cat(pool.encode([sid], [x[:cut]]) + pool.encode([sid], [x[cut:]]), 1)
        assert torch.equal(got, want)
    # A beside B and beside another B, in front of it and behind it
    B2 = _clip(404, 3 * HOP)
    for nb in (B, B2):
        for a_first in (True, False):
            pool.reset()
            ids, first, second = ([0, 1], [A[:cutA], nb[:cutB]], [A[cutA:], nb[cutB:]]) if a_first else ([1, 0], [nb[:cutB], A[:cutA]], [nb[cutB:], A[cutA:]])
            o1, o2 = pool.encode(ids, first), pool.encode(ids, second)
            at = 0 if a_first else 1
            assert torch.equal(torch.cat([o1[at], o2[at]], 1), wA), "A's codes depend on its neighbour or its place"
            assert torch.equal(torch.cat([o1[1 - at], o2[1 - at]], 1), _single(codec, nb))


def _raw(pool, ids, offs, lens, n=None, wav=True, codes_ptr=True, null=None):
    """mimi_enc_pool_encode as the C ABI has it; returns (rc, message, codes)."""
    from sesameai._abi import lib
    wavbuf = torch.zeros(8 * HOP, device="cuda")
    codes = torch.full((32, 16), -1, dtype=torch.int32, device="cuda")
    m = max(1, len(ids))
    a_ids, a_off, a_len = (C.c_int32 * m)(*ids), (C.c_long * m)(*offs), (C.c_long * m)(*lens)
    args = [a_ids, a_off, a_len]
    if null is not None:
        args[null] = None
    rc = lib.mimi_enc_pool_encode(pool._h, args[0], args[1], args[2], len(ids) if n is None else n, wavbuf.data_ptr() if wav else None,
                                  codes.data_ptr() if codes_ptr else None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, (lib.mimi_enc_pool_last_error(pool._h) or b"").decode(), codes


def test_state_reset_refusals_and_the_codec_the_pool_shares_weights_with(tiny):
    from sesameai import _abi
    s, w, codec, clips, alone = tiny
    c4 = torch.randint(0, 2048, (1, 32, 4), generator=torch.Generator().manual_seed(21))

    def codec_outputs():
        out = [codec.encode(clips[4].view(1, 1, -1)), *codec.encode_many(clips[3:6]), codec.decode(c4)]
        codec.reset_stream()
        return out + [codec.decode_stream(c4[..., :2]), codec.decode_stream(c4[..., 2:])]

    before = codec_outputs()
    pool = codec.open_encode_streams(2, max_chunk_frames=3)
    x = _clip(501, 5 * HOP + 777)
    want = _single(codec, x)
    (first,) = pool.encode([0], [x[:2 * HOP]])
    assert torch.equal(first, want[:, :2])
    # every refusal: -1, a message, nothing written, and stream 0 goes on as if nothing had been asked
    refusals = [("n = 0", dict(ids=[], offs=[], lens=[])), ("n = 3 > n_streams", dict(ids=[0, 1, 1], offs=[0, 0, 0], lens=[HOP] * 3)),
                ("a duplicate id", dict(ids=[0, 0], offs=[0, 0], lens=[HOP, HOP])), ("id 2 of 2", dict(ids=[0, 2], offs=[0, 0], lens=[HOP, HOP])),
                ("id -1", dict(ids=[-1], offs=[0], lens=[HOP])), ("no samples", dict(ids=[0, 1], offs=[0, 0], lens=[HOP, 0])),
                ("a negative offset", dict(ids=[0], offs=[-1], lens=[HOP])), ("4 frames > max_chunk_frames", dict(ids=[0], offs=[0], lens=[3 * HOP + 1])),
                ("null ids", dict(ids=[0], offs=[0], lens=[HOP], null=0)), ("null offsets", dict(ids=[0], offs=[0], lens=[HOP], null=1)),
                ("null lengths", dict(ids=[0], offs=[0], lens=[HOP], null=2)), ("null wav", dict(ids=[0], offs=[0], lens=[HOP], wav=False)),
                ("null codes", dict(ids=[0], offs=[0], lens=[HOP], codes_ptr=False))]
    for what, kw in refusals:
        rc, msg, codes = _raw(pool, **kw)
        assert rc == -1 and msg.startswith("mimi_enc_pool_encode:") and len(msg) > 30, f"{what}: rc {rc}, '{msg}'"
        assert bool((codes == -1).all()), f"{what}: a refused call wrote codes"
    (second,) = pool.encode([0], [x[2 * HOP:5 * HOP]])
    assert torch.equal(second, want[:, 2:5]), "a refused call moved stream 0's state"
    (last,) = pool.encode([0], [x[5 * HOP:]])
    assert torch.equal(last, want[:, 5:]) and pool.ended(0)
    # ended: refused until reset, through the ABI and through Python, while its neighbour works
    rc, msg, codes = _raw(pool, ids=[0], offs=[0], lens=[HOP])
    assert rc == -1 and "reset" in msg and bool((codes == -1).all())
    with pytest.raises(_abi.CsmError, match="reset"):
        pool.encode([1, 0], [x[:HOP], x[:HOP]])
    assert torch.equal(pool.encode([1], [x[:HOP]])[0], want[:, :1]), "a refused list moved the neighbour's state"
    # a reset stream is a fresh pool's stream
    pool.reset([0])
    assert not pool.ended(0)
    fresh = codec.open_encode_streams(1, max_chunk_frames=3)
    assert torch.equal(_stream(pool, 0, x, [3, 2, 1]), want) and torch.equal(_stream(fresh, 0, x, [3, 2, 1]), want)
    # creation is refused without encoder weights, and for a pool that is too large
    from sesameai.mimi import MimiCodec, mimi_tiny_args, synthetic_state_dict
    bare = MimiCodec(mimi_tiny_args(), synthetic_state_dict(mimi_tiny_args(), seed=4321, encoder=False), max_frames=8)
    with pytest.raises(RuntimeError, match="encoder"):
        bare.open_encode_streams(1)
    with pytest.raises(_abi.CsmError, match="n_streams"):
        codec.open_encode_streams(65)
    # the codec whose weights the pool shares gives what it gave before
    for i, (g, b) in enumerate(zip(codec_outputs(), before)):
        assert torch.equal(g, b), f"the codec's output {i} changed after the pool's calls"


def test_full_size_past_the_attention_window():
    """One stream of 140 frames in 10-frame chunks plus a 777-sample tail (282 tokens: windows that start above 0, a ring of 270 that wraps)
    against the whole-clip encode of the same codec, full-size synthetic weights."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sesameai.mimi import MimiArgs, MimiCodec, synthetic_state_dict
    codec = MimiCodec(MimiArgs(), synthetic_state_dict(MimiArgs(), seed=4321), max_frames=141)
    x = _clip(601, 140 * HOP + 777)
    want = _single(codec, x)
    pool = codec.open_encode_streams(1, max_chunk_frames=10)
    got = _stream(pool, 0, x, [10] * 14 + [1])
    assert got.shape == want.shape == (32, 141)
    assert torch.equal(got, want), f"columns {(got != want).any(dim=0).nonzero().flatten().tolist()} differ from the whole-clip encode"


def test_generator_builds_the_prompt_from_turns_encoded_while_they_were_spoken(tiny):
    from sesameai.generator import Generator, Segment
    s, w, codec, clips, alone = tiny
    gen = Generator.__new__(Generator)
    gen.device, gen._text_tokenizer, gen._audio_tokenizer = torch.device("cuda"), None, codec
    a, b = clips[4], clips[5]                                           # 3 frames + 777 samples; 15.5 frames
    turns = gen.open_turn_streams(2, chunk_frames=3)
    calls = []
    enc = turns.pool.encode
    turns.pool.encode = lambda ids, wavs: (calls.append(list(ids)), enc(ids, wavs))[1]
    # the microphones deliver 0.1 s at a time; a pump after every fourth delivery
    step, n_pumped = 2400, 0
    for k in range(0, max(a.shape[0], b.shape[0]), step):
        if k < a.shape[0]:
            turns.feed(0, a[k:k + step])
        turns.feed(1, b[k:k + step])
        if (k // step) % 4 == 3:
            n_pumped += turns.pump()
    assert n_pumped >= 9 and all(len(c) <= 2 for c in calls) and [0, 1] in calls, "both turns went through shared calls while they were spoken"
    n_before = len(calls)
    seg_a = turns.finish(0, 0, [5, 6])
    seg_b = turns.finish(1, 1, [7])
    assert len(calls) - n_before <= 2 + 2, "finish: what is left of each turn, in the fewest calls"
    assert torch.equal(seg_a.audio_codes, alone[4]) and torch.equal(seg_b.audio_codes, alone[5])
    got = gen._build_prompt([11, 12], 0, [seg_a, seg_b])
    want = gen._build_prompt([11, 12], 0, [Segment(0, [5, 6], audio=a), Segment(1, [7], audio=b)])
    assert got[0].is_cuda and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert got[0].shape[0] == 2 + 5 + 1 + 17 + 2


def test_every_encode_entry_point_interleaved_on_one_codec_equals_fresh_objects():
    """``encode``, a pool call, ``encode_many``, the pool call that ends the stream and a stateless ``decode``, interleaved on ONE codec: all
    of them run the one encoder chain on buffers and state that the calls before them used (the handle's work buffers and their reset after
    an encode, the pool's histories and rings, the latent's row count).  Each result is ``torch.equal`` to the same call on a freshly built
    codec or pool that did nothing else, and the stream's joined codes to ``encode`` of its clip."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    a, b, c = _clip(401, 3 * HOP + 1), _clip(402, 3 * HOP + 777), _clip(403, HOP + 961)
    cut = 2 * HOP                                                       # stream 0: two frames, then hop + 777 samples, which ends it
    codes = torch.randint(0, 2048, (1, 32, 4), generator=torch.Generator().manual_seed(404))
    want_a, want_b = _single(_new_tiny(), a), _single(_new_tiny(), b)
    want_many = _new_tiny().encode_many([a, c])
    fresh_pool = _new_tiny().open_encode_streams(2, max_chunk_frames=3)
    want_b0, want_b1 = fresh_pool.encode([0], [b[:cut]])[0], fresh_pool.encode([0], [b[cut:]])[0]
    want_pcm = _new_tiny().decode(codes)
    assert want_a.shape == (32, 4) and want_b0.shape == (32, 2) and want_b1.shape == (32, 2) and [m.shape[1] for m in want_many] == [4, 2]

    codec = _new_tiny()
    pool = codec.open_encode_streams(2, max_chunk_frames=3)
    got_a = _single(codec, a)
    got_b0 = pool.encode([0], [b[:cut]])[0]
    got_many = codec.encode_many([a, c])
    got_b1 = pool.encode([0], [b[cut:]])[0]
    got_pcm = codec.decode(codes)
    assert torch.equal(got_a, want_a), "encode after nothing"
    assert torch.equal(got_b0, want_b0), "the pool's first call, after an encode on the codec"
    assert len(got_many) == 2 and all(torch.equal(g, w) for g, w in zip(got_many, want_many)), "encode_many between two pool calls"
    assert torch.equal(got_many[0], want_a), "clip A in a list and alone"
    assert torch.equal(got_b1, want_b1) and pool.ended(0), "the pool's second call, which ends the stream"
    assert torch.equal(torch.cat([got_b0, got_b1], dim=1), want_b), "stream 0's joined codes against encode of B alone"
    assert got_pcm.shape == (1, 1, 4 * HOP) and torch.isfinite(got_pcm).all() and torch.equal(got_pcm, want_pcm), "a stateless decode after the encodes"
