"""Refilling several slots of the live batch with ONE ragged prefill (include/csm_hip.h csm_refill_group_begin / _advance;
Model.refill_group_begin / refill_group_advance; ``refill_group=`` of the Generator's live-batch entry points).

The numerical rule: a prompt row's bits do not depend on what shares its call, and the ragged launches keep every segment's tile
composition that of a single-slot call.  So a group must leave in every slot the K/V rows, and hand the next frame step the frame-0
input, that the same segments give one after the other through csm_refill_begin.  Every comparison is ``torch.equal``."""
import ctypes
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _generator(model, codec=None, batch=1):
    from sesameai.generator import Generator
    gen = Generator.__new__(Generator)
    gen._model, gen.device, gen._eos_poll, gen._audio_tokenizer, gen._text_tokenizer = model, model.device, 8, codec, None
    gen._max_batch, gen._stream_buffer_size, gen._mimi_stream, gen.sample_rate = batch, 10, None, 24_000
    return gen


def _both_ways(m, B, tok, msk, segs, max_layers):
    """segs: [(slot, P, S, offset)] -- slot runs rows [offset + P, offset + P + S) of the token stream at positions P.., after rows
    [offset, offset + P) were copied in from a snapshot.  Runs them (a) one after the other and (b) as one group; returns per way
    ({slot: K/V rows [0, P + S)}, frame 0 of every slot under greedy)."""
    L = m.bb.num_layers
    layers = L if max_layers is None else max_layers
    snaps = {}
    m.reset_caches()
    for slot, P, S, off in segs:                               # the prefixes: whole-prompt rows of a scratch slot, snapshotted
        if P and (off, P) not in snaps:
            m.refill_slot(B - 1, tok[off:off + P], msk[off:off + P], 1.0, 1)
            snaps[(off, P)] = m.capture_prefix(B - 1, P)
    out = []
    for grouped in (False, True):
        m.reset_caches()
        rows = [(tok[off + P:off + P + S], msk[off + P:off + P + S]) for _, P, S, off in segs]
        if grouped:
            for (off, P), h in snaps.items():
                m.apply_prefix(h, [slot for slot, P_, _, off_ in segs if (off_, P_) == (off, P)])
            m.refill_group_begin([s[0] for s in segs], rows, starts=[s[1] for s in segs])
            calls = 0
            while not m.refill_group_advance(layers):
                calls += 1
            assert calls == (L + layers - 1) // layers - 1
        else:
            for (slot, P, S, off), (t, k) in zip(segs, rows):
                if P:
                    m.apply_prefix(snaps[(off, P)], [slot])
                m.refill_begin(slot, t, k, start=P)
                while not m.refill_advance(layers):
                    pass
        kv = {}
        for slot, P, S, _ in segs:
            h = m.capture_prefix(slot, P + S)
            kv[slot] = h.read()
            h.destroy()
        g0 = m.num_frames()
        m.step(B, 1.0, 1)                                       # samples frame 0 of every refilled slot out of rf_last
        fr, _ = m.read_frames(B, g0, 1)
        out.append((kv, fr[0].clone()))
    for h in snaps.values():
        h.destroy()
    return out


def _assert_same(segs, seq, grp, what):
    for slot, P, S, _ in segs:
        a, b = seq[0][slot], grp[0][slot]
        assert a.shape == b.shape and a.shape[3] == P + S
        assert bool((a[:, :, :, P:].float().abs().sum(dim=(0, 1, 2, 4)) > 0).all()), f"{what}: a row the sequential way wrote is all zero"
        assert torch.equal(a, b), f"{what}: slot {slot} (P={P}, S={S}): K/V rows differ at rows {sorted(set((a != b).nonzero()[:, 3].tolist()))[:8]}"
        assert torch.equal(seq[1][slot], grp[1][slot]), f"{what}: slot {slot}: frame 0 differs (the final-normed last row)"


@pytest.fixture(scope="module")
def tiny():
    _need_gpu()
    from oracle import csm_ref as C
    from oracle.make_golden import toy_prompt
    from sesameai.models import Model, csm_tiny_2k_args, synthetic_state_dict
    tok, msk = toy_prompt(C.csm_tiny(), 12, 20, 298)
    m = Model(csm_tiny_2k_args(), synthetic_state_dict(csm_tiny_2k_args(), seed=1234), max_frames=16, max_prefill_rows=512)
    m.setup_caches(8)
    assert m.supports_refill_beside_the_loop(8)
    return m, tok, msk


# (slot, P, S, offset into the token stream).  Slot lists neither sorted nor contiguous; P in {0, 5, 64} mixed in one group; segment lengths
# at the 32-row tile seams; sum S on both sides of the row counts at which the projections change kernel (64: k_mmt, 256: k_gemm128)
CASES = {
    "tile_seams_1_31_32_33_65": ([(5, 0, 1, 0), (0, 5, 31, 3), (3, 64, 32, 3), (7, 0, 33, 40), (2, 5, 65, 3)], 1),
    "rows_63": ([(5, 0, 31, 0), (0, 5, 32, 7)], 3),
    "rows_64": ([(5, 5, 32, 7), (1, 0, 32, 0)], 3),
    "rows_255": ([(6, 64, 65, 0), (2, 0, 190, 20)], None),
    "rows_256": ([(6, 64, 65, 0), (2, 0, 191, 20)], None),
    "rows_257": ([(6, 64, 65, 0), (2, 0, 192, 20), ], 3),
    "one_segment": ([(4, 5, 40, 11)], 1),
    "one_row_each": ([(1, 0, 1, 0), (0, 64, 1, 9), (6, 5, 1, 2)], None),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_group_leaves_the_bits_of_one_refill_after_the_other(tiny, case):
    m, tok, msk = tiny
    segs, max_layers = CASES[case]
    seq, grp = _both_ways(m, 8, tok, msk, segs, max_layers)
    _assert_same(segs, seq, grp, case)


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_full_size_group_after_a_shared_prefix(dtype):
    """CSM-1B shapes (k_gemm128 and the flash kernel at head_dim 64 exist only there): three suffixes of 40 / 33 / 7 rows after a shared
    320-row prefix and one 300-row prompt from position 0 -- 380 rows, above the 256-row switch."""
    _need_gpu()
    import bench
    from types import SimpleNamespace
    from sesameai.models import Model, csm_1b_args, synthetic_state_dict
    a = SimpleNamespace(ctx_text=40, ctx_frames=125, gen_text=24)
    t, k = bench.synthetic_prompt(a, 1, 128_256, seed0=5000, segments=4, ctx_text=30, ctx_frames=100)
    tok, msk = t[0], k[0]
    assert tok.shape[0] >= 400
    m = Model(csm_1b_args(), synthetic_state_dict(csm_1b_args(), seed=7), max_frames=8, max_prefill_rows=512, weights_dtype=dtype)
    m.setup_caches(8)
    segs = [(6, 320, 40, 0), (1, 320, 33, 0), (4, 320, 7, 0), (2, 0, 300, 30)]
    seq, grp = _both_ways(m, 8, tok, msk, segs, 5)
    _assert_same(segs, seq, grp, f"csm-1b {dtype}")


def _raw_begin(m, slots, rows, n, t, k, p):
    from sesameai._abi import lib
    sl = (ctypes.c_int32 * max(len(slots), 1))(*slots)
    rw = (ctypes.c_int32 * max(len(rows), 1))(*rows)
    return lib.csm_refill_group_begin(m._h, sl, rw, n, t.data_ptr(), k.data_ptr(), p.data_ptr(), None)


def test_refusals_enqueue_nothing():
    """Every CSM_E_INVALID / CSM_E_STATE condition returns its code; afterwards the handle steps exactly like one that never saw the call."""
    _need_gpu()
    from oracle import csm_ref as C
    from oracle.make_golden import toy_prompt
    from sesameai._abi import CsmError, lib
    from sesameai.models import Model, csm_tiny_2k_args, synthetic_state_dict
    tok, msk = toy_prompt(C.csm_tiny(), 12, 20, 298)
    sd = synthetic_state_dict(csm_tiny_2k_args(), seed=1234)
    ms = [Model(csm_tiny_2k_args(), sd, max_frames=16, max_prefill_rows=128) for _ in range(2)]
    frames = []
    for which, m in enumerate(ms):
        m.setup_caches(4)
        m.reset_caches()
        for s in range(4):
            m.refill_slot(s, tok[s:s + 20], msk[s:s + 20], 1.0, 1)
        good = ([3, 1], [(tok[30:50], msk[30:50]), (tok[5:14], msk[5:14])])
        if which == 1:
            m.refill_begin(2, tok[:8], msk[:8])
            while not m.refill_advance(1):
                pass
        if which == 0:
            t = tok[:200].to(m.device, torch.int32).contiguous()
            k = msk[:200].to(m.device, torch.uint8).contiguous()
            p = torch.arange(200, dtype=torch.int32, device=m.device)
            INVALID, STATE = -1, -3
            assert _raw_begin(m, [], [], 0, t, k, p) == INVALID
            assert _raw_begin(m, list(range(33)), [1] * 33, 33, t, k, p) == INVALID
            assert _raw_begin(m, [0, 2, 0], [4, 4, 4], 3, t, k, p) == INVALID and b"twice" in lib.csm_last_error(m._h)
            assert _raw_begin(m, [0, 4], [4, 4], 2, t, k, p) == INVALID
            assert _raw_begin(m, [-1], [4], 1, t, k, p) == INVALID
            assert _raw_begin(m, [0, 1], [4, 0], 2, t, k, p) == INVALID
            assert _raw_begin(m, [0, 1], [100, 29], 2, t, k, p) == INVALID and b"max_rows" in lib.csm_last_error(m._h)
            assert lib.csm_refill_group_advance(m._h, 1, None) == STATE          # nothing began
            assert lib.csm_refill_group_advance(m._h, 0, None) == INVALID
            m.refill_begin(2, tok[:8], msk[:8])                                  # a single refill is pending: no group
            assert _raw_begin(m, [0, 1], [4, 4], 2, t, k, p) == STATE
            assert lib.csm_refill_group_advance(m._h, 1, None) == STATE          # ... and the group's advance does not run it
            while not m.refill_advance(1):
                pass
            pf = m.capture_prefix(0, 4)
        m.refill_group_begin(*good)
        if which == 0:
            assert _raw_begin(m, [0], [4], 1, t, k, p) == STATE                  # a group is pending: no second one, no single refill,
            with pytest.raises(CsmError) as e:
                m.refill_begin(0, tok[:8], msk[:8])
            assert e.value.code == STATE
            for call in (lambda: m.reset_slots([1]), lambda: m.refill_slot(3, tok[:8], msk[:8], 1.0, 1),     # and its slots are not touched
                         lambda: m.capture_prefix(1, 2), lambda: m.apply_prefix(pf, [0, 3])):
                with pytest.raises(CsmError) as e:
                    call()
                assert e.value.code == STATE
            assert lib.csm_refill_advance(m._h, 1, None) == STATE
        while not m.refill_group_advance(1):
            pass
        g0 = m.num_frames()
        for _ in range(3):
            m.step(4, 1.0, 1)
        frames.append(m.read_frames(4, g0, 3)[0].clone())
    assert torch.equal(frames[0], frames[1]), "a refused call changed what the handle computes"


def _copy_model(batch):
    from oracle import csm_ref as C
    from sesameai.models import Model, csm_tiny_args, synthetic_state_dict
    shape = C.csm_tiny()
    m = Model(csm_tiny_args(), synthetic_state_dict(csm_tiny_args(), seed=1234, flavour="decisive_copy"), max_frames=64, max_prefill_rows=256)
    m.setup_caches(batch)
    om = C.OracleModel(shape, C.make_weights(shape, seed=1234, flavour="decisive_copy"))
    om.setup_caches(1)
    return shape, m, om


def test_free_running_codes_of_a_group_and_its_bystanders():
    """The copy checkpoint's codes are read out of cached K/V.  Eight slots under greedy; four utterances end in the same block and their
    slots take four new prompts as ONE group while the other four keep generating: every utterance is the oracle's solo trajectory, and
    the bystanders' frames are those of the same batch without any refill."""
    _need_gpu()
    from oracle import csm_ref as C
    shape, m, om = _copy_model(8)
    g = torch.Generator().manual_seed(77)
    ids = lambda k: torch.randint(0, shape.text_vocab_size, (k,), generator=g).tolist()
    prompts = [C.build_prompt([(ids(6 + i), None)]) for i in range(12)]
    limits = [6] * 4 + [20] * 4 + [8] * 4
    gen = _generator(m, batch=8)
    begins = []
    real = m.refill_group_begin
    m.refill_group_begin = lambda slots, *a, **kw: (begins.append(list(slots)), real(slots, *a, **kw))[1]
    got = gen.generate_codes_continuous(prompts, limits, 1.0, 1, refill_group=4)
    m.refill_group_begin = real
    assert [len(b) for b in begins] == [4, 4, 4], f"initial fill in two groups of four, then the four retired slots as one: {begins}"
    for i, (tok, msk) in enumerate(prompts):
        fr = C.generate_codes(om, tok, msk, limits[i] * 80, 1.0, 1, greedy=True, max_seq_len=shape.backbone.max_seq_len)
        want = torch.cat(fr).to(torch.int32) if fr else torch.empty(0, 32, dtype=torch.int32)
        assert want.shape[0] == limits[i], "the copy checkpoint is not expected to end an utterance early"
        assert torch.equal(got[i], want), f"utterance {i} leaves the oracle's trajectory"
    alone = gen.generate_codes_continuous(prompts[:8], limits[:8], 1.0, 1)
    for i in range(4, 8):
        assert torch.equal(got[i], alone[i]), f"bystander {i} was disturbed by the group refill"


def _mixed_prompts(shape, gen, n):
    from oracle import csm_ref as C
    g = torch.Generator().manual_seed(5)
    ids = lambda k: torch.randint(0, shape.text_vocab_size, (k,), generator=g).tolist()
    voice = (ids(6), torch.randint(0, 2048, (shape.audio_num_codebooks, 40), generator=g))
    vt, vm = C.build_prompt([voice])
    handle = gen.cache_prefix(vt, vm)
    prompts = [C.build_prompt(([voice] if i % 3 != 2 else []) + [(ids(4 + i % 5), None)]) for i in range(n)]
    return handle, prompts


def test_seeded_requests_do_not_depend_on_the_group_size():
    """12 requests on 4 slots, sampled (0.9 / 50), every request with a seed of its own, with and without a registered prefix, mixed
    limits: refill_group=1 and refill_group=4 schedule the refills differently and return the same codes."""
    _need_gpu()
    from oracle import csm_ref as C
    shape = C.csm_tiny()
    from sesameai.models import Model, csm_tiny_args, synthetic_state_dict
    m = Model(csm_tiny_args(), synthetic_state_dict(csm_tiny_args(), seed=1234), max_frames=64, max_prefill_rows=256)
    m.setup_caches(4)
    gen = _generator(m, batch=4)
    handle, prompts = _mixed_prompts(shape, gen, 12)
    limits = [9, 14, 9, 9, 20, 6, 6, 6, 11, 7, 13, 5]
    seeds = [1000 + 17 * i for i in range(12)]
    rows0 = m.prefill_rows_total
    one = gen.generate_codes_continuous(prompts, limits, 0.9, 50, seed=seeds, refill_group=1)
    rows1 = m.prefill_rows_total
    four = gen.generate_codes_continuous(prompts, limits, 0.9, 50, seed=seeds, refill_group=4)
    assert m.prefill_rows_total - rows1 == rows1 - rows0 < sum(t.shape[0] for t, _ in prompts), "both ways run only the rows after the prefix"
    assert [f.shape[0] for f in one] == limits
    for i in range(12):
        assert torch.equal(one[i], four[i]), f"request {i}: codes depend on the refill group size"
    assert len({tuple(f.flatten().tolist()) for f in one}) == 12
    gen.drop_prefix(handle)


def test_streamed_pcm_does_not_depend_on_the_group_size():
    """generate_many_stream of 6 short requests on 3 slots, own seeds: per-request PCM equal for refill_group=1 and 3."""
    _need_gpu()
    from sesameai.generator import Generator, Segment
    from sesameai.mimi import MimiCodec, mimi_tiny_args, synthetic_state_dict as mimi_sd
    from sesameai.models import Model, csm_tiny_args
    codec = MimiCodec(mimi_tiny_args(), mimi_sd(mimi_tiny_args(), seed=4321), max_frames=64)
    model = Model(csm_tiny_args(), None, max_frames=64, max_prefill_rows=128)
    gen = Generator(model, audio_tokenizer=codec, max_batch_size=3)
    assert model.supports_refill_beside_the_loop(3)
    g = torch.Generator().manual_seed(21)
    lens = [12, 5, 12, 7, 10, 3]
    texts = [torch.randint(0, 1000, (4 + i % 3,), generator=g).tolist() for i in range(6)]
    ctxs = [[Segment(speaker=1, text=torch.randint(0, 1000, (3,), generator=g).tolist(), audio_codes=torch.randint(0, 2048, (32, 2 + i % 3), generator=g))]
            for i in range(6)]
    seeds = [31 + i for i in range(6)]
    runs = []
    for group in (1, 3):
        pcm = {i: [] for i in range(6)}
        for i, chunk, _, _ in gen.generate_many_stream(texts, [1] * 6, ctxs, max_audio_length_ms=[n * 80 for n in lens], temperature=0.9, topk=50,
                                                       seed=seeds, refill_group=group):
            pcm[i].append(chunk)
        runs.append([torch.cat(pcm[i]) for i in range(6)])
    for i, n in enumerate(lens):
        assert runs[0][i].shape[0] == 1920 * n
        assert torch.equal(runs[0][i], runs[1][i]), f"request {i}: streamed PCM depends on the refill group size"
