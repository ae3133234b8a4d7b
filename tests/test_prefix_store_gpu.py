"""The prefix store on the GPU (include/csm_hip.h csm_prefix_*; Model.capture_prefix / apply_prefix; Generator.cache_prefix).

The numerical rule: in prompt mode a row's K/V do not depend on how many rows share its call, so a slot seeded from a
snapshot and then prefilled with the rows after it holds the SAME BITS as a slot that ran the whole prompt.  Every comparison here is
``torch.equal``: snapshots against snapshots, free-running greedy codes against the goldens / the live oracle and against the same
run without a prefix, PCM against PCM.  Sampled runs are not comparable across the two ways (a refill that finishes sooner lands its
frame 0 on another global frame index, which is part of the Philox key), so everything runs greedy (top-k 1)."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SPLITS = lambda S: [1, 64, 255, 256, S - 1]          # suffixes of S - P rows: both sides of the switch to k_gemm128 (256 rows)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _generator(model, codec=None, batch=1):
    from sesameai.generator import Generator
    gen = Generator.__new__(Generator)
    gen._model, gen.device, gen._eos_poll, gen._audio_tokenizer, gen._text_tokenizer = model, model.device, 8, codec, None
    gen._max_batch, gen._stream_buffer_size, gen._mimi_stream, gen.sample_rate = batch, 10, None, 24_000
    return gen


def _s1334():
    import bench
    from types import SimpleNamespace
    a = SimpleNamespace(ctx_text=40, ctx_frames=125, gen_text=24)
    t, m = bench.synthetic_prompt(a, 1, 128_256, seed0=5000, segments=10, ctx_text=30, ctx_frames=100)
    return t[0], m[0]


def _snapshot_equality(m, tok, msk, splits):
    """Slot 0 runs the whole prompt; slots 1 (csm_prefill_slot) and 2 (csm_refill_begin / advance) are seeded with P rows and run the rest."""
    S = tok.shape[0]
    L = m.bb.num_layers
    m.reset_caches()
    m.refill_slot(0, tok, msk, 1.0, 1)
    whole = m.capture_prefix(0, S)
    want = whole.read()
    assert want.shape == (L, 2, m.bb.num_kv_heads, S, m.bb.head_dim) and whole.bytes == want.numel() * 2 and whole.rows == S
    assert bool((want.float().abs().sum(dim=(0, 1, 2, 4)) > 0).all()), "a captured row is all zero"
    for P in splits:
        pf = m.capture_prefix(0, P)
        assert torch.equal(pf.read(), want[:, :, :, :P]), f"P={P}: the snapshot is not the slot's first rows"
        m.apply_prefix(pf, [1, 2])                     # one launch, two slots; slot 2's refill begins right after slot 1's prefill
        m.refill_slot(1, tok[P:], msk[P:], 1.0, 1, start=P)
        assert m.last_prefill_rows == S - P
        got = m.capture_prefix(1, S)
        assert torch.equal(got.read(), want), f"P={P}: seeded + suffix-prefilled slot (csm_prefill_slot) differs from the whole prompt's K/V"
        m.refill_begin(2, tok[P:], msk[P:], start=P)
        while not m.refill_advance(max(L // 3, 1)):
            pass
        got2 = m.capture_prefix(2, S)
        assert torch.equal(got2.read(), want), f"P={P}: seeded + suffix-refilled slot (csm_refill_begin) differs from the whole prompt's K/V"
        for h in (pf, got, got2):
            h.destroy()
        assert "prefix_store=1 prefixes" in m.describe()
    again = m.capture_prefix(0, S)
    assert torch.equal(again.read(), want), "a slot never listed in an apply lost its rows"
    again.destroy(); whole.destroy()
    assert "prefix_store=0 prefixes, 0 bytes" in m.describe()


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_tiny_snapshot_of_seeded_slot_equals_whole_prompt(dtype):
    _need_gpu()
    from oracle import csm_ref as C
    from oracle.make_golden import toy_prompt
    from sesameai.models import Model, csm_tiny_2k_args, synthetic_state_dict
    tok, msk = toy_prompt(C.csm_tiny(), 12, 20, 298)
    tok, msk = tok[:320], msk[:320]
    m = Model(csm_tiny_2k_args(), synthetic_state_dict(csm_tiny_2k_args(), seed=1234), max_frames=16, max_prefill_rows=512, weights_dtype=dtype)
    m.setup_caches(3)
    _snapshot_equality(m, tok, msk, SPLITS(320))


_CSM1B = {}


@pytest.fixture(scope="module")
def csm1b():
    """(gold, get(dtype) -> an 8-slot CSM-1B handle on the s1334 copy checkpoint: copy layer 3, lag 700)."""
    _need_gpu()
    from sesameai.models import Model, csm_1b_args, synthetic_state_dict
    gold = torch.load(os.path.join(GOLD, "csm1b_decisive_copy.pt"))
    flavour = gold["flavours"]["s1334"]
    sd = synthetic_state_dict(csm_1b_args(), seed=int(gold["weight_seed"]), flavour=flavour)
    names, sums = gold["weight_checksums"][flavour]
    got = torch.stack([sd[k].view(torch.int16).to(torch.int64).sum() for k in names])
    assert torch.equal(got, sums), "the product's checkpoint is not the one the oracle's codes were generated with"

    def get(dtype):
        if dtype not in _CSM1B:
            _CSM1B.clear()                              # one handle at a time
            m = Model(csm_1b_args(), sd, max_frames=96, max_prefill_rows=2048, weights_dtype=dtype)
            m.setup_caches(8)
            _CSM1B[dtype] = m
        return _CSM1B[dtype]
    yield gold, get
    _CSM1B.clear()


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_csm1b_snapshot_of_seeded_slot_equals_whole_prompt(csm1b, dtype):
    _, get = csm1b
    from sesameai._abi import CsmError
    m = get(dtype)
    tok, msk = _s1334()
    _snapshot_equality(m, tok[:320], msk[:320], SPLITS(320))
    # the whole 1,334-row voice prompt: the flash prefill attends from the suffix rows to 1,294 copied cache rows
    _snapshot_equality(m, tok, msk, [1294])
    # a prefix of another shape is refused
    from sesameai.models import Model, csm_tiny_args, synthetic_state_dict
    t = Model(csm_tiny_args(), synthetic_state_dict(csm_tiny_args(), seed=1), max_frames=8, max_prefill_rows=64)
    t.setup_caches(1)
    t.prefill_prompt(tok[:16].unsqueeze(0) % 1000, msk[:16].unsqueeze(0))
    small = t.capture_prefix(0, 8)
    with pytest.raises(CsmError) as e:
        m.apply_prefix(small, [1])
    assert e.value.code == -1 and "another shape" in str(e.value)


@pytest.mark.parametrize("beside", [True, False])
@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_csm1b_free_running_codes_out_of_copied_rows(csm1b, dtype, beside):
    """c0 of frame t names the last code of the row 700 back, read out of layer 3's cached K / V: with n frames the rows read are
    634 .. 633 + n of the 1,334-row prompt.  Ten requests of that prompt through 8 slots (two slots are refilled inside the live batch), with
    those rows all inside the copied prefix (P = 1200), all in the prefilled suffix (P = 600), and P = S - 1: every utterance is the
    oracle's golden trajectory, and equals the run without a prefix."""
    gold, get = csm1b
    m = get(dtype)
    tok, msk = _s1334()
    S = tok.shape[0]
    want = gold[f"{dtype}_s1334"]["codes"][:, 0].to(torch.int32)
    n = want.shape[0]
    assert S == 1334 == int(gold[f"{dtype}_s1334"]["prompt_rows"]) and 634 + n <= 1200
    gen = _generator(m, batch=8)
    gen.refill_beside_the_loop = beside
    prompts = [(tok, msk)] * 10
    rows0 = m.prefill_rows_total
    plain = gen.generate_codes_continuous(prompts, n, 1.0, 1)
    assert m.prefill_rows_total - rows0 == 10 * S
    for i, g in enumerate(plain):
        assert torch.equal(g, want), f"no prefix: utterance {i} leaves the golden at frame {int((g != want).any(dim=1).nonzero()[0]) if g.shape == want.shape else g.shape}"
    for P in (1200, 600, S - 1):
        h = gen.cache_prefix(tok[:P], msk[:P])
        assert h.rows == P and h.bytes == P * 32768
        rows0 = m.prefill_rows_total
        got = gen.generate_codes_continuous(prompts, n, 1.0, 1)
        assert m.prefill_rows_total - rows0 == 10 * (S - P), "only the suffix rows run"
        for i, g in enumerate(got):
            assert torch.equal(g, want), f"P={P}: utterance {i} differs from the golden"
            assert torch.equal(g, plain[i]), f"P={P}: utterance {i} differs from the run without a prefix"
        gen.drop_prefix(h)
        assert gen.prefixes == [] and not h.alive


def _tiny_copy(batch, dtype="bf16"):
    from oracle import csm_ref as C
    from sesameai.models import Model, csm_tiny_args, synthetic_state_dict
    shape = C.csm_tiny()
    m = Model(csm_tiny_args(), synthetic_state_dict(csm_tiny_args(), seed=1234, flavour="decisive_copy"), max_frames=64, max_prefill_rows=256, weights_dtype=dtype)
    m.setup_caches(batch)
    om = C.OracleModel(shape, C.make_weights(shape, seed=1234, flavour="decisive_copy"))
    om.setup_caches(1)
    return shape, m, om


def _voices(shape):
    """Two voice prompts (text + audio rows) and a text-row generator."""
    from oracle import csm_ref as C
    g = torch.Generator().manual_seed(77)
    ids = lambda k: torch.randint(0, shape.text_vocab_size, (k,), generator=g).tolist()
    codes = lambda k: torch.randint(0, 2048, (shape.audio_num_codebooks, k), generator=g)
    A = (ids(6), codes(50))
    B = (ids(9), codes(30))
    build = lambda voice, k: C.build_prompt(([voice] if voice else []) + [(ids(k), None)])
    return A, B, build, ids


def _oracle_codes(om, shape, tok, msk, n):
    from oracle import csm_ref as C
    fr = C.generate_codes(om, tok, msk, n * 80, 1.0, 1, greedy=True, max_seq_len=shape.backbone.max_seq_len)
    return torch.cat(fr).to(torch.int32) if fr else torch.empty(0, 32, dtype=torch.int32)


@pytest.mark.parametrize("beside", [True, False])
def test_tiny_mixed_traffic_equals_the_oracle_and_runs_only_suffix_rows(beside):
    """Two registered voices, twelve requests through 4 slots with mixed length limits: five per voice with distinct texts, one that matches
    neither voice, one that matches voice A only up to row 30.  Every utterance is the oracle's solo greedy trajectory; the rows
    that ran are exactly the rows after each request's longest match."""
    _need_gpu()
    from oracle import csm_ref as C
    shape, m, om = _tiny_copy(4)
    A, B, build, ids = _voices(shape)
    pa, pam = C.build_prompt([A]); pb, pbm = C.build_prompt([B])
    PA, PB = pa.shape[0], pb.shape[0]
    assert (PA, PB) == (57, 40)
    reqs, matched = [], []
    for k in range(5):
        reqs.append(build(A, 5 + k)); matched.append(PA)
        reqs.append(build(B, 9 - k)); matched.append(PB)
    reqs.append(build(None, 14)); matched.append(0)
    t, mk = build(A, 7)
    cut = C.build_prompt([(ids(12), None)])
    reqs.append((torch.cat([t[:30], cut[0], t[PA:]]), torch.cat([mk[:30], cut[1], mk[PA:]]))); matched.append(30)   # (row 30 of A is an audio row)
    limits = [6 + (5 * i) % 9 for i in range(12)]
    want = [_oracle_codes(om, shape, t, mk, lim) for (t, mk), lim in zip(reqs, limits)]
    assert all(w.shape[0] == lim for w, lim in zip(want, limits)), "an oracle trajectory hit EOS"
    gen = _generator(m, batch=4)
    gen.refill_beside_the_loop = beside
    gen.refill_row_layers = 40
    ha, hb = gen.cache_prefix(pa, pam), gen.cache_prefix(pb, pbm)
    assert gen.prefixes == [ha, hb] and "prefix_store=2 prefixes" in m.describe()
    rows0 = m.prefill_rows_total
    got = gen.generate_codes_continuous(reqs, limits, 1.0, 1)
    ran = m.prefill_rows_total - rows0
    for i, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g, w), f"request {i} (S={reqs[i][0].shape[0]}, match {matched[i]}) differs from the oracle's solo codes"
    assert ran == sum(r[0].shape[0] - p for r, p in zip(reqs, matched)), (ran, [r[0].shape[0] for r in reqs], matched)
    gen.drop_prefix(ha); gen.drop_prefix(hb)
    rows0 = m.prefill_rows_total
    again = gen.generate_codes_continuous(reqs, limits, 1.0, 1)
    assert m.prefill_rows_total - rows0 == sum(r[0].shape[0] for r in reqs)
    assert all(torch.equal(a, g) for a, g in zip(again, got))


def test_b1_prefill_prompt_alternating_two_voices_runs_only_suffix_rows():
    _need_gpu()
    from oracle import csm_ref as C
    shape, m, _ = _tiny_copy(1)
    A, B, build, _ = _voices(shape)
    pa, pam = C.build_prompt([A]); pb, pbm = C.build_prompt([B])
    gen = _generator(m)
    reqs = [build(A if i % 2 == 0 else B, 5 + i) for i in range(6)]

    def frames(tok, msk):
        m.reset_caches()
        rows = m.prefill_prompt(tok.unsqueeze(0), msk.unsqueeze(0))
        m.depth(1, 1.0, 1, commit=True)
        for _ in range(5):
            m.step(1, 1.0, 1)
        return rows, m.read_frames(1)[0][:, 0]

    m.prefix_reuse = False
    cold = [frames(t, mk) for t, mk in reqs]
    assert [r for r, _ in cold] == [t.shape[0] for t, _ in reqs]
    m.prefix_reuse = True
    without = [frames(t, mk)[0] for t, mk in reqs]
    assert without[1:] == [t.shape[0] for t, _ in reqs][1:], "alternating voices: the previous-prompt match alone reuses nothing"
    gen.cache_prefix(pa, pam); gen.cache_prefix(pb, pbm)
    for i, (t, mk) in enumerate(reqs):
        rows, fr = frames(t, mk)
        assert rows == t.shape[0] - (pa if i % 2 == 0 else pb).shape[0], f"request {i}: {rows} rows ran"
        assert torch.equal(fr, cold[i][1]), f"request {i}: frames differ from a cold prefill's"


def test_refusals():
    _need_gpu()
    from oracle import csm_ref as C
    from sesameai._abi import CsmError
    from sesameai.models import Model, csm_tiny_2k_args, synthetic_state_dict
    shape, m, _ = _tiny_copy(3)
    A, B, build, _ = _voices(shape)
    tok, msk = build(A, 6)
    S = tok.shape[0]
    m.reset_caches()
    m.refill_slot(0, tok, msk, 1.0, 1)
    with pytest.raises(CsmError) as e:
        m.capture_prefix(0, S + 1)                     # rows beyond the slot's position
    assert e.value.code == -1
    with pytest.raises(CsmError) as e:
        m.capture_prefix(1, 4)                         # a slot that holds nothing
    assert e.value.code == -1
    pf = m.capture_prefix(0, 40)
    m.refill_begin(1, tok, msk)
    assert not m.refill_advance(1)
    for call in (lambda: m.apply_prefix(pf, [2, 1]), lambda: m.capture_prefix(1, 4)):
        with pytest.raises(CsmError) as e:
            call()                                     # the slot whose refill is running
        assert e.value.code == -3
    assert m.refill_advance(16)
    m.apply_prefix(pf, [1])                            # ... and accepted once it is complete
    with pytest.raises(CsmError) as e:
        m.apply_prefix(pf, [3])                        # outside the batch
    assert e.value.code == -1
    # a prefix from another handle: same layers / heads, but more rows than this handle's max_seq
    big = Model(csm_tiny_2k_args(), synthetic_state_dict(csm_tiny_2k_args(), seed=1234), max_frames=8, max_prefill_rows=512)
    big.setup_caches(1)
    g = torch.Generator().manual_seed(5)
    t300 = torch.zeros(300, 33, dtype=torch.long); t300[:, 32] = torch.randint(0, 1000, (300,), generator=g)
    m300 = torch.zeros(300, 33, dtype=torch.bool); m300[:, 32] = True
    big.prefill_prompt(t300.unsqueeze(0), m300.unsqueeze(0))
    foreign = big.capture_prefix(0, 300)
    with pytest.raises(CsmError) as e:
        m.apply_prefix(foreign, [0])
    assert e.value.code == -1
    pf.destroy()
    assert not pf.alive
    with pytest.raises(ValueError, match="destroyed"):
        m.apply_prefix(pf, [0])
    with pytest.raises(ValueError, match="destroyed"):
        pf.read()
    pf.destroy()                                       # idempotent
    # setup_caches destroys the handle and with it the snapshots captured from it
    keep = big.capture_prefix(0, 10)
    big.setup_caches(1)
    assert not keep.alive and not foreign.alive


def test_generate_many_stream_with_a_prefix_yields_the_same_pcm():
    _need_gpu()
    from sesameai.generator import Segment
    from sesameai.mimi import MimiArgs, MimiCodec, synthetic_state_dict as mimi_sd
    shape, m, _ = _tiny_copy(3)
    codec = MimiCodec(MimiArgs(), mimi_sd(MimiArgs(), seed=4321), max_frames=96)
    gen = _generator(m, codec, batch=3)
    g = torch.Generator().manual_seed(9)
    voice = [Segment(speaker=0, text=torch.randint(0, 1000, (8,), generator=g).tolist(), audio_codes=torch.randint(0, 2048, (32, 45), generator=g))]
    texts = [torch.randint(0, 1000, (4 + i,), generator=g).tolist() for i in range(7)]
    limits = [80 * (12 + (7 * i) % 15) for i in range(7)]

    def run():
        pcm, frames = {}, {}
        for i, chunk, fr, last in gen.generate_many_stream(texts, [0] * 7, [voice] * 7, max_audio_length_ms=limits, temperature=1.0, topk=1):
            pcm.setdefault(i, []).append(chunk.cpu()); frames.setdefault(i, []).append(fr)
        return {i: torch.cat(v) for i, v in pcm.items()}, {i: torch.cat(v) for i, v in frames.items()}

    rows0 = m.prefill_rows_total
    pcm0, fr0 = run()
    plain_rows = m.prefill_rows_total - rows0
    h = gen.cache_prefix(voice)
    assert h.rows == 8 + 45 + 1
    rows0 = m.prefill_rows_total
    pcm1, fr1 = run()
    assert m.prefill_rows_total - rows0 == plain_rows - 7 * h.rows
    assert sorted(pcm0) == sorted(pcm1) == list(range(7))
    for i in range(7):
        assert fr0[i].shape[0] > 0 and torch.equal(fr0[i], fr1[i]), f"request {i}: frames"
        assert torch.equal(pcm0[i], pcm1[i]), f"request {i}: PCM"
