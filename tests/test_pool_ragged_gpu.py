"""Ragged stream-pool decode: streams with DIFFERENT numbers of new frames in one launch chain (include/mimi_hip.h
mimi_pool_decode_ragged, sesameai.mimi.MimiStreamPool.decode_ragged).  The rule under test is the header's: a stream's PCM from a ragged
call is, bit for bit, what the uniform mimi_pool_decode gives that stream for the same chunk schedule -- whatever shares the call, whatever
the others' lengths are, wherever the stream sits in the list -- and therefore the codec's whole-clip decode.  Against the oracle
(oracle/mimi_ref.py) the bound is the project's Mimi bound, 2e-5 of the clip's peak; tests/test_pool_ragged_oracle.py shows that a stream
given a neighbour's history, or none, would miss it by four orders of magnitude."""
import ctypes as C
import os

import pytest
import torch

from test_pool_ragged_oracle import SEED_A, SEED_B, T0, TA, TB, codes_of

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
REL_TOL = 2e-5          # vs the oracle


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


def _same(got, want, what):
    assert got.shape == want.shape, f"{what}: {tuple(got.shape)} vs {tuple(want.shape)}"
    d = (got - want).abs().max().item() if got.numel() else 0.0
    print(f"{what}: max|d|={d:.3g}")
    assert torch.equal(got, want), f"{what}: not bit-identical, max|d|={d:.3g}"


def _ragged_rounds(pool, jobs, rounds):
    """jobs {sid: codes (32,L)}; rounds [[(sid, T), ...], ...]: one ragged call per round, each stream going on where it stopped.
    Returns {sid: [its chunks (hop*T,)]}."""
    at = {sid: 0 for sid in jobs}
    out = {sid: [] for sid in jobs}
    for rnd in rounds:
        ids = [sid for sid, _ in rnd]
        pcm = pool.decode_ragged(ids, [jobs[sid][:, at[sid]:at[sid] + T] for sid, T in rnd])
        assert len(pcm) == len(rnd)
        for (sid, T), x in zip(rnd, pcm):
            assert x.shape == (1, 1920 * T) and x.dtype == torch.float32
            out[sid].append(x[0]); at[sid] += T
    return out


def _uniform_alone(pool, sid, codes, sched):
    """The same stream through the UNIFORM call, alone, on the schedule: its chunks."""
    out, t = [], 0
    for T in sched:
        out.append(pool.decode([sid], codes[None, :, t:t + T])[0, 0]); t += T
    return out


def test_ragged_equals_uniform_bit_for_bit(tiny):
    from oracle import mimi_ref as M
    s, w, codec = tiny
    Ts = [(1, 10, 3, 2, 9), (10, 1, 1, 10, 4), (2, 2, 10, 7, 1)]
    jobs = {sid: codes_of(100 + sid, sum(r[sid] for r in Ts)) for sid in range(5)}
    pool, twin = codec.open_streams(5, max_chunk_frames=10), codec.open_streams(5, max_chunk_frames=10)
    got = _ragged_rounds(pool, jobs, [[(sid, r[sid]) for sid in range(5)] for r in Ts])
    for sid in range(5):
        want = _uniform_alone(twin, sid, jobs[sid], [r[sid] for r in Ts])
        for k, (a, b) in enumerate(zip(got[sid], want)):
            _same(a, b, f"stream {sid}, round {k} ({Ts[k][sid]} frames): ragged vs uniform")
        whole = torch.cat(got[sid])
        _same(whole, codec.decode(jobs[sid][None])[0, 0], f"stream {sid}: its chunks vs the codec's whole-clip decode")
        _close(whole, M.decode(s, w, jobs[sid][None])[0, 0], f"stream {sid} ({jobs[sid].shape[1]} frames) vs oracle")
    # all T_i equal: ONE uniform call
    pool.reset(); twin.reset()
    ids = [3, 0, 4, 1, 2]
    batch = torch.stack([jobs[sid][:, :4] for sid in ids])
    rag = pool.decode_ragged(ids, batch, [4] * 5)               # (the padded form of the arguments)
    uni = twin.decode(ids, batch)
    for j, sid in enumerate(ids):
        _same(rag[j][0], uni[j, 0], f"all T_i = 4, stream {sid}: ragged vs ONE uniform call")


@pytest.mark.parametrize("Ts", [(15, 1, 16), (1, 17, 1), (16, 16), (17,)], ids=lambda t: "-".join(map(str, t)))
def test_segment_boundaries_inside_a_gemm_tile(tiny, Ts):
    """T_i of 15 / 16 / 17 frames are 30 / 32 / 34 token rows around k_gemm32's 32-row tile: the lists put a segment boundary inside a tile,
    on its edge and one row past it."""
    s, w, codec = tiny
    pool, twin = codec.open_streams(3, max_chunk_frames=17), codec.open_streams(3, max_chunk_frames=17)
    ids = [2, 0, 1][:len(Ts)]
    jobs = {sid: codes_of(200 + sid, T) for sid, T in zip(ids, Ts)}
    got = pool.decode_ragged(ids, [jobs[sid] for sid in ids])
    for j, sid in enumerate(ids):
        _same(got[j][0], twin.decode([sid], jobs[sid][None])[0, 0], f"T = {Ts}: stream {sid} ({Ts[j]} frames) vs the same stream alone")


def _pair(pool, me, other, T_me, T_other, order="MO", other_reset=False, ids=(1, 3)):
    """`me` on stream ids[0] and `other` on ids[1] each decode T0 frames of their own, then ONE ragged call carries my next T_me and the
    other's next T_other frames, listed in `order`.  Returns my chunk's PCM."""
    pool.reset()
    pool.decode_ragged(list(ids), [me[:, :T0], other[:, :T0]])
    if other_reset:
        pool.reset([ids[1]])
    parts = {"M": (ids[0], me[:, T0:T0 + T_me]), "O": (ids[1], other[:, T0:T0 + T_other])}
    out = pool.decode_ragged([parts[x][0] for x in order], [parts[x][1] for x in order])
    return out[order.index("M")][0].clone()


def test_isolation_both_directions(tiny):
    """A and B in one ragged call with different T: nothing about the other -- its codes, its history, its T, its place -- reaches a stream.
    Then the same with A and B exchanged."""
    from oracle import mimi_ref as M
    s, w, codec = tiny
    pool = codec.open_streams(4, max_chunk_frames=10)
    alt = codes_of(SEED_B + 50, T0 + 10)
    for name, me_seed, other_seed, T_me, T_other in (("A", SEED_A, SEED_B, TA, TB), ("B", SEED_B, SEED_A, TB, TA)):
        me, other = codes_of(me_seed, T0 + T_me), codes_of(other_seed, T0 + T_other)
        base = _pair(pool, me, other, T_me, T_other)
        for what, args, kw in (("the other's codes", (me, alt, T_me, T_other), {}),
                               ("a reset of the other", (me, other, T_me, T_other), dict(other_reset=True)),
                               ("the other's T (1)", (me, other, T_me, 1), {}),
                               ("the other's T (max)", (me, alt, T_me, 10), {}),
                               ("the other's place in the list", (me, other, T_me, T_other), dict(order="OM")),
                               ("the stream ids", (me, other, T_me, T_other), dict(ids=(2, 0)))):
            _same(_pair(pool, *args, **kw), base, f"{name}'s PCM after changing {what}")
        _close(base, M.decode(s, w, me[None])[0, 0][1920 * T0:], f"{name}'s {T_me}-frame chunk after {T0} frames vs oracle")


def test_ring_and_offsets_per_stream(tiny):
    """The tiny codec's window is 6 tokens; with max_chunk_frames = 3 a ring holds 12.  Three streams run 60 frames (120 tokens: ten times
    round the ring) on different schedules, so their offsets and ring rows differ at every call."""
    s, w, codec = tiny
    L = 60
    scheds = {0: [1] * 60, 1: [3] * 20, 2: [1, 2, 3] * 10}
    assert all(sum(v) == L for v in scheds.values()) and (2 * L) // (s.tr_context + 6) >= 5
    jobs = {sid: codes_of(300 + sid, L) for sid in scheds}
    pool = codec.open_streams(3, max_chunk_frames=3)
    rounds = [[(sid, sc[k]) for sid, sc in scheds.items() if k < len(sc)] for k in range(60)]
    got = _ragged_rounds(pool, jobs, rounds)
    for sid in scheds:
        _same(torch.cat(got[sid]), codec.decode(jobs[sid][None])[0, 0], f"stream {sid} ({len(scheds[sid])} chunks) vs its whole-clip decode")


def test_refusals_leave_the_pool_as_it_was(tiny):
    from sesameai._abi import CsmError, lib
    s, w, codec = tiny
    pool, clean = codec.open_streams(4, max_chunk_frames=5), codec.open_streams(4, max_chunk_frames=5)
    jobs = {1: codes_of(401, 8), 2: codes_of(402, 8)}
    first = [(1, 3), (2, 1)]
    _ragged_rounds(pool, jobs, [first]); _ragged_rounds(clean, jobs, [first])
    c = codes_of(403, 6)
    for ids, Ts, word in (([1, 1], [2, 2], "duplicate"), ([1, 4], [2, 2], "outside"), ([-1], [2], "outside"), ([1], [6], "max_chunk_frames"),
                          ([1, 2], [2, 0], "max_chunk_frames"), ([0, 1, 2, 3, 0], [1] * 5, "n_streams")):
        with pytest.raises(CsmError, match=word):
            pool.decode_ragged(ids, torch.stack([c] * len(ids)), Ts)
    dev = c[None].to(device=codec.device, dtype=torch.int32)
    pcm = torch.empty(1920 * 2, device=codec.device)
    one, two = (C.c_int32 * 1)(1), (C.c_int32 * 1)(2)
    strides = (dev.stride(0), dev.stride(1), dev.stride(2))
    for ids_, frames_, n, codes_, pcm_, word in ((None, two, 1, dev.data_ptr(), pcm.data_ptr(), b"null"), (one, None, 1, dev.data_ptr(), pcm.data_ptr(), b"null"),
                                                 (one, two, 1, None, pcm.data_ptr(), b"null"), (one, two, 1, dev.data_ptr(), None, b"null"),
                                                 (one, two, 0, dev.data_ptr(), pcm.data_ptr(), b"n_streams"), (one, two, -1, dev.data_ptr(), pcm.data_ptr(), b"n_streams")):
        assert lib.mimi_pool_decode_ragged(pool._h, ids_, frames_, n, codes_, *strides, pcm_, None) == -1
        assert word in lib.mimi_pool_last_error(pool._h)
    # (the 2^31-token refusal needs a stream a billion frames old: tools/pool_segs_check.cpp makes it on the plan this call uses)
    torch.cuda.synchronize()
    nxt = [(2, jobs[2][:, 1:6]), (1, jobs[1][:, 3:5])]
    got = pool.decode_ragged([sid for sid, _ in nxt], [x for _, x in nxt])
    want = clean.decode_ragged([sid for sid, _ in nxt], [x for _, x in nxt])
    for j, (sid, _) in enumerate(nxt):
        _same(got[j][0], want[j][0], f"stream {sid} after the refused calls vs a pool that never saw them")
    _same(got[0][0], _uniform_alone(clean, 0, jobs[2][:, :6], [1, 5])[1], "stream 2's chunk vs the uniform call on the same schedule")


def test_full_size_ragged_vs_uniform_and_golden():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sesameai.mimi import MimiArgs, MimiCodec, synthetic_state_dict
    gold = torch.load(os.path.join(GOLD, "mimi_full.pt"))
    codec = MimiCodec(MimiArgs(), synthetic_state_dict(MimiArgs(), seed=int(gold["weight_seed"])), max_frames=32)
    gcodes = gold["codes"][0]
    assert gcodes.shape[1] == 10
    Ts = [(1, 10, 3, 10), (9, 10, 7, 10)]
    # every stream starts on the golden codes; streams 1 and 3 go on for 10 frames more
    jobs = {sid: torch.cat([gcodes, codes_of(500 + sid, 10)], dim=1)[:, :sum(r[sid] for r in Ts)] for sid in range(4)}
    pool, twin = codec.open_streams(4, max_chunk_frames=10), codec.open_streams(4, max_chunk_frames=10)
    got = _ragged_rounds(pool, jobs, [[(sid, r[sid]) for sid in range(4)] for r in Ts])
    for sid in range(4):
        want = _uniform_alone(twin, sid, jobs[sid], [r[sid] for r in Ts])
        for k in range(2):
            _same(got[sid][k], want[k], f"full size, stream {sid}, round {k} ({Ts[k][sid]} frames): ragged vs uniform")
        mine = torch.cat(got[sid])[None, None, :1920 * 10]          # the frames the golden covers
        _close(mine[..., ::16], gold["pcm_stride16"], f"full size, stream {sid}: golden frames (every 16th sample)")
        _close(mine[..., :4096], gold["pcm_head"], f"full size, stream {sid}: golden head")
        _close(mine[..., -4096:], gold["pcm_tail"], f"full size, stream {sid}: golden tail")
