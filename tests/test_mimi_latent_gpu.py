"""The Mimi ENCODER graded on what it computes, not only on the integer codes that come out of it (include/mimi_hip.h: mimi_encode,
mimi_encode_many, mimi_enc_pool_encode; the latent is read with mimi_debug_encode_latent / mimi_enc_pool_debug_latent).

* the pre-quantisation latent against the oracle on float64 weights and audio, at 2e-5 of peak -- the decode side's bound, for the same
  reason: fp32 on both sides, the only freedom is summation order -- over the whole clip and over the last frame alone, where the
  partial-frame rule and both paddings act; the fp32 CPU oracle is held to the same bound in the same test;
* the "bit for bit" rules of the ragged and the streamed encode on the latents themselves (``torch.equal``), beside the codes;
* the quantiser on its own: exact ties made by duplicating a winning centroid, across the three tie-break sites of ``k_rvq_pick``
  (the teacher-forced walk over every level of every frame lives in tests/test_mimi_gpu.py ``_check_codes(latent=...)``);
* non-finite audio: one NaN / +Inf / -Inf sample gives in-range codes (0 from its frame on), leaves the frames before it, the
  neighbours in the call and everything after a reset bit-identical to a clean run.

tests/test_mimi_latent_oracle.py shows on the CPU why the codes alone do not carry this."""
import pytest
import torch

from test_mimi_latent_oracle import HOP, REL_TOL, TIE_CLIP, float64_walk, latent64, tie_plan, wav_of

pytestmark = pytest.mark.gpu
BAD = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def tiny():
    _need_gpu()
    from oracle import mimi_ref as M
    from sesameai.mimi import MimiCodec, mimi_tiny_args, synthetic_state_dict
    s = M.mimi_tiny()
    w = M.make_weights(s, seed=4321, encoder=True)
    sd = synthetic_state_dict(mimi_tiny_args(), seed=4321)
    assert set(w) == set(sd) and all(torch.equal(w[k], sd[k]) for k in w), "product and oracle synthetic Mimi weights differ"
    new = lambda weights=sd: MimiCodec(mimi_tiny_args(), weights, max_frames=64)
    return s, w, new(), new


@pytest.fixture(scope="module")
def full():
    _need_gpu()
    from oracle import mimi_ref as M
    from sesameai.mimi import MimiArgs, MimiCodec, synthetic_state_dict
    s = M.mimi_full()
    w = M.make_weights(s, seed=4321, encoder=True)
    return s, w, MimiCodec(MimiArgs(), synthetic_state_dict(MimiArgs(), seed=4321), max_frames=16)


def _frames(n):
    return -(-n // HOP)


def _encode(codec, clip):
    """clip (n,) -> (codes (32, T), latent (T, hidden)) of ``encode`` of the clip alone"""
    codes = codec.encode(clip.view(1, 1, -1))[0]
    return codes, codec.encode_latent(codes.shape[1])


def _grade_latent(s, w, codec, wav, what):
    from oracle import mimi_ref as M
    T = _frames(wav.shape[-1])
    z64 = latent64(s, w, wav)[0].t()                                                 # (T, hidden) float64
    z32 = M.encode_latent(s, w, wav)[0].t().double()
    assert codec.encode(wav).shape == (1, 32, T)
    got = codec.encode_latent(T)
    assert got.shape == (T, s.hidden) and got.dtype == torch.float32
    got = got.cpu().double()
    assert torch.isfinite(got).all()
    for part, rows in (("whole clip", slice(None)), ("last frame", slice(T - 1, T))):
        peak = z64[rows].abs().max().item()
        gpu, cpu = ((x[rows] - z64[rows]).abs().max().item() / peak for x in (got, z32))
        print(f"{what}, {part}: GPU latent {gpu:.3g} of the float64 peak ({peak:.3g}), fp32 CPU oracle {cpu:.3g}")
        assert cpu <= REL_TOL, f"{what}, {part}: the fp32 oracle is {cpu:.3g} of peak from its float64 run"
        assert gpu <= REL_TOL, f"{what}, {part}: the GPU latent is {gpu:.3g} of peak from the float64 oracle"


@pytest.mark.parametrize("n", [1, HOP - 1, HOP, HOP + 1, 3 * HOP + 777])
def test_tiny_latent_vs_float64_oracle(tiny, n):
    s, w, codec, _ = tiny
    _grade_latent(s, w, codec, wav_of(40 + n % 7, n), f"tiny latent, {n} samples")


@pytest.mark.parametrize("n", [6 * HOP + 5, 2 * HOP])
def test_full_size_latent_vs_float64_oracle(full, n):
    s, w, codec = full
    _grade_latent(s, w, codec, wav_of(50 + n % 7, n), f"full-size latent, {n} samples")


def test_latent_getter_refuses_a_row_count_that_is_not_the_last_calls(tiny):
    from sesameai._abi import CsmError
    s, w, codec, _ = tiny
    codec.encode(wav_of(3, 2 * HOP + 1))
    assert codec.encode_latent(3).shape == (3, s.hidden)
    for rows in (2, 4, 0):
        with pytest.raises(CsmError, match="rows is not the frame count"):
            codec.encode_latent(rows)
    codec.decode(torch.zeros(1, 32, 3, dtype=torch.long))                            # the code lookup reuses the buffer
    with pytest.raises(CsmError, match="rows is not the frame count"):
        codec.encode_latent(3)
    pool = codec.open_encode_streams(2, max_chunk_frames=2)
    with pytest.raises(CsmError, match="rows is not the frame count"):
        pool.encode_latent(1)
    pool.encode([1, 0], [wav_of(4, HOP)[0, 0], wav_of(5, HOP + 1)[0, 0]])
    assert pool.encode_latent(3).shape == (3, s.hidden)
    with pytest.raises(CsmError, match="rows is not the frame count"):
        pool.encode_latent(2)


# ---- bit-identical latents behind the "bit for bit" rules -------------------------------------------------------------------------------
def _ragged_bit_identity(codec, lengths, seed):
    clips = [wav_of(seed + i, n)[0, 0] for i, n in enumerate(lengths)]
    alone = [_encode(codec, c) for c in clips]
    for order in (list(range(len(clips))), list(range(len(clips)))[::-1]):
        got = codec.encode_many([clips[i] for i in order])
        T = [alone[i][0].shape[1] for i in order]
        lat = codec.encode_latent(sum(T)).split(T)                                   # clip i of the call owns rows [F_i, F_i + T_i)
        for j, i in enumerate(order):
            assert torch.equal(got[j], alone[i][0]), f"order {order}: codes of the clip of {lengths[i]} samples"
            assert torch.equal(lat[j], alone[i][1]), f"order {order}: latent rows of the clip of {lengths[i]} samples differ from its encode alone"


def test_ragged_encode_latents_are_bit_identical_tiny(tiny):
    _ragged_bit_identity(tiny[2], [2 * HOP + 1, 777, 5 * HOP], 60)


def test_ragged_encode_latents_are_bit_identical_full_size(full):
    _ragged_bit_identity(full[2], [HOP + 1, 777], 64)


def _pool_bit_identity(codec, calls, seed):
    """calls: per call {stream id: new samples}; every stream's columns and latent rows, concatenated over its calls, against ``encode`` of
    its concatenated samples"""
    total = {}
    for call in calls:
        for sid, n in call.items():
            total[sid] = total.get(sid, 0) + n
    clips = {sid: wav_of(seed + sid, n)[0, 0] for sid, n in total.items()}
    pool = codec.open_encode_streams(len(total), max_chunk_frames=4)
    at = {sid: 0 for sid in total}
    codes, lat = {sid: [] for sid in total}, {sid: [] for sid in total}
    for call in calls:
        ids = list(call)
        got = pool.encode(ids, [clips[sid][at[sid]:at[sid] + call[sid]] for sid in ids])
        T = [g.shape[1] for g in got]
        rows = pool.encode_latent(sum(T)).split(T)
        for sid, g, z in zip(ids, got, rows):
            codes[sid].append(g); lat[sid].append(z); at[sid] += call[sid]
    for sid in total:
        want_c, want_z = _encode(codec, clips[sid])
        assert pool.ended(sid)
        assert torch.equal(torch.cat(codes[sid], dim=1), want_c), f"stream {sid}: codes"
        assert torch.equal(torch.cat(lat[sid]), want_z), f"stream {sid}: latent rows differ from the encode of its concatenated samples"


def test_encode_stream_latents_are_bit_identical_tiny(tiny):
    # stream 0: 1, 3 and 2 whole frames, then hop + 300 samples that end it; stream 1 shares the first and third call and ends on its own
    _pool_bit_identity(tiny[2], [{0: HOP, 1: 2 * HOP}, {0: 3 * HOP}, {1: 4 * HOP, 0: 2 * HOP}, {1: HOP + 5}, {0: HOP + 300}], 70)


def test_encode_stream_latents_are_bit_identical_full_size(full):
    _pool_bit_identity(full[2], [{0: 2 * HOP, 1: HOP}, {0: HOP + 300}, {1: 2 * HOP + 7}], 74)


# ---- exact ties -----------------------------------------------------------------------------------------------------------------------
def test_exact_ties_take_the_first_index_at_every_tie_break_site(tiny):
    """A winning centroid copied into an unused row of its level is a bit-exact tie on the GPU too: the score product gives identical
    outputs for identical rows and the loader computes |e|^2 per row.  The lower index must win at the ties, and nothing else may move."""
    from oracle import mimi_ref as M
    s, w, codec, new = tiny
    wav = wav_of(*TIE_CLIP)
    base = codec.encode(wav)[0].cpu()
    oracle = M.encode(s, w, wav)[0]
    walk, gaps = float64_walk(s, w, M.encode_latent(s, w, wav))
    plan, w2, _ = tie_plan(s, w, walk, gaps)
    for level, frame, win, dup, site in plan:                                        # preconditions
        assert bool((gaps[:level + 1, frame] >= 1e-3).all()), "a planned frame has a narrow margin before its tie"
        assert torch.equal(base[:level + 1, frame], oracle[:level + 1, frame]) and int(base[level, frame]) == win, \
            f"on the undoctored books the GPU and the oracle part before the tie at level {level}, frame {frame}"
    want_oracle = M.encode(s, w2, wav)[0]
    want = base.clone()
    for level, frame, win, dup, site in plan:
        want[level][base[level] == win] = min(win, dup)
    got = new(w2).encode(wav)[0].cpu()
    for level, frame, win, dup, site in plan:
        assert int(got[level, frame]) == min(win, dup) == int(want_oracle[level, frame]), \
            f"level {level}, frame {frame}: centroids {win} and {dup} tie exactly ({site} site), the GPU took {int(got[level, frame])}"
        assert torch.equal(got[:level + 1, frame], want_oracle[:level + 1, frame]), f"frame {frame}: the stack down to the tie differs from the oracle's"
    assert torch.equal(got, want), "codes other than the tied entries moved"
    assert int((got != base).sum()) >= 3


# ---- non-finite audio -------------------------------------------------------------------------------------------------------------------
def _poisoned(clip, value):
    bad = clip.clone()
    bad[2 * HOP + 100] = value                                                       # one bad sample, in frame 2
    return bad


@pytest.mark.parametrize("kind", list(BAD))
def test_one_bad_sample_encode(tiny, kind):
    from oracle import mimi_ref as M
    s, w, _, new = tiny
    used, fresh = new(), new()
    clean = wav_of(80, 5 * HOP + 300)[0, 0]                                          # 6 frames
    cc, cz = _encode(used, clean)
    bc, bz = _encode(used, _poisoned(clean, BAD[kind]))                              # the call returns
    assert bc.shape == (32, 6) and bool(((bc >= 0) & (bc < s.codebook_size)).all()), "a code outside the codebook"
    assert torch.equal(bc[:, :2], cc[:, :2]) and torch.equal(bz[:2], cz[:2]), "the frames before the bad sample changed"
    assert bool((bc[:, 2:] == 0).all()), f"frames from the bad sample on: {bc[:, 2:].unique().tolist()}"
    assert bool((M.encode(s, w, _poisoned(clean, BAD[kind]).view(1, 1, -1))[0][:, 2:] == 0).all())     # as the oracle
    assert bool(torch.isnan(bz[2:]).all())
    # nothing of it outlives the call: the handle's next decode and its next encode are a fresh codec's
    codes = torch.randint(0, 2048, (1, 32, 4), generator=torch.Generator().manual_seed(81))
    want = fresh.decode(codes)
    assert bool(torch.isfinite(want).all()) and torch.equal(used.decode(codes), want), "a decode after the poisoned encode"
    ac, az = _encode(used, clean)
    fc, fz = _encode(fresh, clean)
    assert torch.equal(ac, fc) and torch.equal(az, fz) and torch.equal(ac, cc), "a clean encode after the poisoned one"


@pytest.mark.parametrize("kind", list(BAD))
def test_one_bad_sample_encode_many_leaves_the_neighbours_alone(tiny, kind):
    s, w, codec, new = tiny
    used = new()
    a, mid, b = wav_of(82, 2 * HOP + 1)[0, 0], _poisoned(wav_of(83, 4 * HOP + 300)[0, 0], BAD[kind]), wav_of(84, 777)[0, 0]
    alone = [_encode(codec, a), _encode(codec, b)]
    got = used.encode_many([a, mid, b])
    lat = used.encode_latent(3 + 5 + 1).split([3, 5, 1])
    assert all(bool(((g >= 0) & (g < s.codebook_size)).all()) for g in got), "a code outside the codebook"
    assert bool((got[1][:, 2:] == 0).all())
    for what, g, z, (wc, wz) in (("before", got[0], lat[0], alone[0]), ("behind", got[2], lat[2], alone[1])):
        assert torch.equal(g, wc) and torch.equal(z, wz), f"the clean clip {what} the poisoned one differs from its encode alone"


@pytest.mark.parametrize("kind", list(BAD))
def test_one_bad_sample_in_a_stream_leaves_the_pool_alone(tiny, kind):
    s, w, codec, _ = tiny
    x0, x1 = _poisoned(wav_of(85, 5 * HOP + 300)[0, 0], BAD[kind]), wav_of(86, 6 * HOP + 5)[0, 0]
    cuts0, cuts1 = [2 * HOP, 3 * HOP, HOP + 300], [2 * HOP, 3 * HOP, HOP + 5]          # the bad sample: first frame of stream 0's second chunk

    def run(pool, streams):
        """streams: {id: (clip, cuts)} fed call by call -> per stream (codes, latent rows) joined over the calls"""
        out = {sid: ([], []) for sid in streams}
        at = {sid: 0 for sid in streams}
        for k in range(3):
            ids = list(streams)
            got = pool.encode(ids, [streams[sid][0][at[sid]:at[sid] + streams[sid][1][k]] for sid in ids])
            T = [g.shape[1] for g in got]
            for sid, g, z in zip(ids, got, pool.encode_latent(sum(T)).split(T)):
                out[sid][0].append(g); out[sid][1].append(z); at[sid] += streams[sid][1][k]
        return {sid: (torch.cat(c, dim=1), torch.cat(z)) for sid, (c, z) in out.items()}

    solo = run(codec.open_encode_streams(2, max_chunk_frames=4), {1: (x1, cuts1)})[1]
    pool = codec.open_encode_streams(2, max_chunk_frames=4)
    both = run(pool, {0: (x0, cuts0), 1: (x1, cuts1)})
    assert torch.equal(both[1][0], solo[0]) and torch.equal(both[1][1], solo[1]), "stream 1 beside the poisoned stream differs from its solo run"
    c0 = both[0][0]
    assert bool(((c0 >= 0) & (c0 < s.codebook_size)).all()) and bool((c0[:, 2:] == 0).all())
    clean = wav_of(85, 5 * HOP + 300)[0, 0]
    assert torch.equal(c0[:, :2], _encode(codec, clean)[0][:, :2]), "the frames before the bad sample changed"
    # after its reset the poisoned stream is a fresh one
    nxt = wav_of(87, 3 * HOP + 11)[0, 0]
    pool.reset([0])
    (got,) = pool.encode([0], [nxt]); got_z = pool.encode_latent(4)
    fresh = codec.open_encode_streams(2, max_chunk_frames=4)
    (want,) = fresh.encode([0], [nxt]); want_z = fresh.encode_latent(4)
    assert bool(torch.isfinite(want_z).all()) and torch.equal(got, want) and torch.equal(got_z, want_z), "a poisoned row survived the stream's reset"
