"""mimi_encode_many (include/mimi_hip.h; MimiCodec.encode_many): clips of different lengths through one launch chain.

The acceptance criterion is bit identity: a clip's codes are ``torch.equal`` to ``MimiCodec.encode`` of that clip alone, whatever shares
the call and wherever the clip sits in the list.  The single encode is graded against the oracle (oracle/mimi_ref.py) by
tests/test_mimi_gpu.py and tests/test_mimi_long_gpu.py; the seam clips here are graded against it once more by the same rule
(``_check_codes``).  That a leak between neighbours could not hide is shown on the oracle in the isolation test itself."""
import ctypes as C
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
HOP = 1920
SEAM_SAMPLES = [1, 1919, 1920, 1921, 3 * 1920 + 777, 960 * 31, 960 * 32 + 1]        # one hop +- 1; 31 / 33 tokens: the 32-row tile seam
SEAM_FRAMES = [1, 1, 1, 2, 4, 16, 17]                                               # inside a clip and between clips


def _clip(seed, n):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)) * 0.3


def _new_tiny(max_frames=64, encoder=True):
    from sesameai.mimi import MimiCodec, mimi_tiny_args, synthetic_state_dict
    return MimiCodec(mimi_tiny_args(), synthetic_state_dict(mimi_tiny_args(), seed=4321, encoder=encoder), max_frames=max_frames)


@pytest.fixture(scope="module")
def tiny():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from oracle import mimi_ref as M
    from sesameai.mimi import mimi_tiny_args, synthetic_state_dict
    s = M.mimi_tiny()
    w = M.make_weights(s, seed=4321, encoder=True)
    sd = synthetic_state_dict(mimi_tiny_args(), seed=4321)
    assert set(w) == set(sd) and all(torch.equal(w[k], sd[k]) for k in w), "product and oracle synthetic Mimi weights differ"
    codec = _new_tiny()
    clips = [_clip(100 + i, n) for i, n in enumerate(SEAM_SAMPLES)]
    alone = [codec.encode(c.view(1, 1, -1))[0] for c in clips]          # computed once, shared, never changed
    assert [a.shape[1] for a in alone] == SEAM_FRAMES and sum(SEAM_FRAMES) == 42
    return s, w, codec, clips, alone


def _single(codec, clip):
    return codec.encode(clip.view(1, 1, -1))[0]


def test_seams_every_clip_equals_its_single_encode_and_the_oracle(tiny):
    from test_mimi_gpu import _check_codes
    s, w, codec, clips, alone = tiny
    got = codec.encode_many(clips)
    assert len(got) == len(clips)
    lat = codec.encode_latent(sum(SEAM_FRAMES)).split(SEAM_FRAMES)      # one call of 42 frames: clip i owns rows [F_i, F_i + T_i)
    for i, (g, a, c) in enumerate(zip(got, alone, clips)):
        assert g.dtype == torch.int64 and g.shape == (32, SEAM_FRAMES[i])
        assert torch.equal(g, a), f"clip {i} ({c.shape[0]} samples) differs from its single encode"
        _check_codes(g.unsqueeze(0), s, w, c.view(1, 1, -1), f"ragged encode, clip {i} ({c.shape[0]} samples)", latent=lat[i])


def test_company_and_order_do_not_matter(tiny):
    s, w, codec, clips, alone = tiny
    rev = codec.encode_many(clips[::-1])[::-1]
    for i, (g, a) in enumerate(zip(rev, alone)):
        assert torch.equal(g, a), f"clip {i} in the reversed list"
    for i, (c, a) in enumerate(zip(clips, alone)):
        (g,) = codec.encode_many([c])
        assert torch.equal(g, a), f"clip {i} alone through encode_many"


def test_isolation_in_both_directions_with_the_oracle_showing_a_leak_would_move_the_codes(tiny):
    from oracle import mimi_ref as M
    s, w, codec, clips, alone = tiny
    nA = 3 * HOP + 777
    A, A2, B, B2 = _clip(201, nA), _clip(202, nA), _clip(203, 2 * HOP), _clip(204, 2 * HOP)
    enc = lambda x: M.encode(s, w, x.view(1, 1, -1))[0]
    # preconditions on the oracle: were B to see A in front of it, >= 90 % of its frames would change ...
    oB = enc(B)
    # (as one clip A ++ B; and with A's slot filled up to the frame boundary, which is where the ragged call puts B: on the rows behind A's
    #  four frames, so that B's own samples sit on the same frame boundaries as in its single encode)
    for what, joined in (("A ++ B", torch.cat([A, B])), ("A ++ zeros to the frame boundary ++ B", torch.cat([A, torch.zeros((-nA) % HOP), B]))):
        changed = (enc(joined)[:, -2:] != oB).any(dim=0).float().mean().item()
        print(f"oracle: B as the end of the ONE clip {what} changes {changed:.2f} of B's frames")
        assert changed >= 0.9
    # ... and were A to see B behind it, its LAST frame would change
    oA = enc(A)
    assert (enc(torch.cat([A, B]))[:, oA.shape[1] - 1] != oA[:, -1]).any(), "appending B does not move A's last frame on the oracle"
    wantA, wantB = _single(codec, A), _single(codec, B)
    # left: what lies in front of B does not reach it
    for first in (A, A2):
        got = codec.encode_many([first, B])
        assert torch.equal(got[1], wantB) and torch.equal(got[0], _single(codec, first))
    # right: what lies behind (or in front of) A does not reach it
    for lst, at in (([B, A], 1), ([B2, A], 1), ([A, B], 0), ([A, B2], 0)):
        assert torch.equal(codec.encode_many(lst)[at], wantA)


def _raw(codec, n, lens, offs=None, wav_len=None):
    """mimi_encode_many as the C ABI has it; returns (rc, message, codes)."""
    from sesameai._abi import lib
    lens = list(lens)
    offs = list(offs) if offs is not None else [sum(lens[:k]) for k in range(len(lens))]
    wav = torch.zeros(wav_len or max(1, sum(max(x, 0) for x in lens)), device="cuda")
    codes = torch.full((32, 80), -1, dtype=torch.int32, device="cuda")
    arr = lambda v: (C.c_long * max(1, len(v)))(*v)
    rc = lib.mimi_encode_many(codec._h, wav.data_ptr(), arr(offs), arr(lens), n, codes.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, (lib.mimi_last_error(codec._h) or b"").decode(), codes


def test_refusals_leave_the_handle_usable_and_a_ragged_encode_leaves_no_trace_in_later_decodes(tiny):
    s, w, _, clips, alone = tiny
    used, fresh = _new_tiny(), _new_tiny()
    for what, n, lens in (("n = 0", 0, []), ("n = 65", 65, [HOP] * 65), ("sum T = 65", 5, [13 * HOP] * 5), ("a clip of 0 samples", 3, [HOP, 0, HOP])):
        rc, msg, codes = _raw(used, n, lens)
        assert rc == -1 and msg.startswith("mimi_encode_many:") and len(msg) > 20, f"{what}: rc {rc}, '{msg}'"
        assert bool((codes == -1).all()), f"{what}: a refused call wrote codes"
    bare = _new_tiny(encoder=False)
    rc, msg, codes = _raw(bare, 1, [HOP])
    assert rc == -1 and "encoder" in msg and bool((codes == -1).all())
    with pytest.raises(RuntimeError, match="encoder"):
        bare.encode_many([clips[2]])
    with pytest.raises(ValueError, match="max_frames"):
        used.encode_many([torch.zeros(65 * HOP)])
    # a valid call and a plain encode afterwards: a fresh codec's bits
    for g, a in zip(used.encode_many(clips), alone):
        assert torch.equal(g, a)
    assert torch.equal(_single(used, clips[4]), alone[4])
    # encode_many splits a list that does not fit one call (here: 84 frames into 64) and the pieces are still the single encodes
    for g, a in zip(used.encode_many(clips + clips), alone + alone):
        assert torch.equal(g, a)
    # the decoder after a ragged encode: a stateless decode and a two-chunk stateful stream equal a fresh codec's
    c4 = torch.randint(0, 2048, (1, 32, 4), generator=torch.Generator().manual_seed(21))

    def decodes(codec):
        out = [codec.decode(c4)]
        codec.reset_stream()
        return out + [codec.decode_stream(c4[..., :2]), codec.decode_stream(c4[..., 2:])]

    used.encode_many(clips)
    for what, got, want in zip(("stateless T=4", "stream chunk 1", "stream chunk 2"), decodes(used), decodes(fresh)):
        assert torch.isfinite(want).all() and want.abs().max().item() > 0
        assert torch.equal(got, want), f"{what} after a ragged encode differs from a fresh codec's"


def test_full_size_past_the_attention_window():
    """The 10.4 s golden voice prompt (522 tokens: windows that start above 0) and the 5 s one, a clip of one sample less than a hop
    and a 1 s clip in one call.  The yardstick is the single encode, which tests/test_mimi_long_gpu.py grades against the oracle; the two
    long clips must also keep that test's bound against the golden: >= 0.9 of the frames identical on all levels."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from oracle.make_golden import mimi_long_wav
    from sesameai.mimi import MimiArgs, MimiCodec, synthetic_state_dict
    gold = torch.load(os.path.join(GOLD, "mimi_long.pt"))
    assert int(gold["weight_seed"]) == 4321
    enc = sorted(gold["encode"], key=lambda g: -int(g["samples"]))
    assert [int(g["samples"]) for g in enc] == [1920 * 260 + 5, 1920 * 126 + 777]
    clips = []
    for g in enc:
        wav = mimi_long_wav(int(g["wav_seed"]), int(g["samples"]))
        assert abs(float(wav.double().abs().sum()) - g["wav_checksum"]) <= 1e-9 * g["wav_checksum"], "the seeded prompt is not the fixture's"
        clips.append(wav[0, 0])
    clips += [_clip(301, 1919), _clip(302, 24000)]
    frames = [261, 127, 1, 13]
    codec = MimiCodec(MimiArgs(), synthetic_state_dict(MimiArgs(), seed=4321), max_frames=sum(frames))
    got = codec.encode_many(clips)
    assert [g.shape for g in got] == [(32, f) for f in frames]
    for i, (g, c) in enumerate(zip(got, clips)):
        assert torch.equal(g, codec.encode(c.view(1, 1, -1))[0]), f"full size: clip {i} ({c.shape[0]} samples) differs from its single encode"
    for g, e in zip(got, enc):
        same = (g.cpu() == e["codes"][0].long()).all(dim=0).float().mean().item()
        print(f"full-size ragged encode, {int(e['samples'])} samples: frames identical to the golden on all levels {same:.3f}")
        assert same >= 0.9


def test_generator_builds_the_prompts_of_several_requests_from_one_ragged_encode(tiny):
    from sesameai import generator as G
    from sesameai.generator import Generator, Segment
    s, w, codec, clips, alone = tiny
    gen = Generator.__new__(Generator)
    gen.device, gen._text_tokenizer, gen._audio_tokenizer = torch.device("cuda"), None, codec
    voice, a, b = clips[4], clips[3], clips[5]
    given = torch.randint(0, 2048, (32, 5), generator=torch.Generator().manual_seed(5))
    contexts = [[Segment(0, [5, 6], audio=voice), Segment(1, [7], audio=a)],
                [Segment(0, [5, 6], audio=voice), Segment(1, [8, 9], audio_codes=given), Segment(0, [3], audio=b)],
                [Segment(1, [4], audio_codes=given)]]
    texts, speakers = [[11, 12], [13], [14, 15]], [0, 1, 1]
    encoded = []
    many = codec.encode_many
    try:
        codec.encode_many = lambda wavs: (encoded.append(len(wavs)), many(wavs))[1]
        assert 3 >= G.ENCODE_MANY_MIN_CLIPS, "three distinct clips are below the threshold: this test would not reach the ragged call"
        prompts = gen._build_prompts(texts, speakers, contexts)
    finally:
        del codec.encode_many
    assert encoded == [3], "the distinct tensors (a voice prompt shared by two requests, two more clips) go through ONE ragged call"
    G_min = G.ENCODE_MANY_MIN_CLIPS
    try:
        G.ENCODE_MANY_MIN_CLIPS = 1000                                  # today's path: one encode per segment
        want = [gen._build_prompt(t, sp, ctx) for t, sp, ctx in zip(texts, speakers, contexts)]
    finally:
        G.ENCODE_MANY_MIN_CLIPS = G_min
    for (t, m), (wt, wm) in zip(prompts, want):
        assert t.is_cuda and torch.equal(t, wt) and torch.equal(m, wm)
    assert prompts[0][0].shape[0] == 2 + 5 + 1 + 3 + 2 and all(seg.audio_codes is None for seg in contexts[0])
