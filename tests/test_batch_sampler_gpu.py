"""The sampler INSIDE the all-CU depth-decoder launches, above all the batched one (csrc/dec_persist_m.cuh, k_dec_persist_m: codebooks
2..31 of every frame of a live batch of 2..32 utterances).  It calls sample_body<2> with plumbing the standalone k_sample does not
share -- logits polled out of the exchange buffer with the 2048..2050 tail on thread 0 only, a quad barrier, scratch that aliases the
half's activation buffer, the noise row at ((cb * M + ob) * V), `ob` as the Philox sequence index, temperature / top-k read from LDS
words -- so what it PICKS is graded here, at top-k > 1:
  1. given Exp(1) noise, every pick is the oracle's sample_topk of the very logits the launch returned, with its own noise row;
  2. without noise, every pick is the standalone sampler's on the same logits and the same Philox {seed, counter}, bit for bit.
Results recorded in docs/experiments/sampler_batch_parity.md.  (The draws themselves against a host Philox, and the (T, k) ranges of
sample_body: tests/test_ops_gpu.py.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu

V, NCB, ROWS = 2051, 32, 16
# (T, k): the product's defaults, a sharper and a flatter pair, k = V (nothing removed, no lower bound: every logit is a candidate), a
# 5-way race, and T >= 2 with k in 129..256 (bisection over the 256 thread maxima, candidate margin 2 ceil(T) + 2 = 8)
CASES = ((0.9, 50), (0.7, 30), (1.0, 2051), (1.3, 5), (2.5, 200))
SEEDS = (4242, 0x1234_5678_9ABC_DEF0)


@pytest.fixture(scope="module")
def csm1b_models():
    """B -> a CSM-1B model (seeded synthetic weights) with B different 16-row prompts prefilled: one model per B, built on first use
    and shared by every test of this module (no test commits a frame without restoring the state it found)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import bench
    from types import SimpleNamespace
    from oracle import csm_ref as C
    from sesameai.models import Model, csm_1b_args, synthetic_state_dict
    sd = synthetic_state_dict(csm_1b_args(), seed=1234)
    shape = SimpleNamespace(ctx_text=8, ctx_frames=4, gen_text=3)         # 8 text rows + 4 audio rows + the EOS row + 3 text rows = 16
    built = {}

    def get(B):
        if B not in built:
            tok, msk = bench.synthetic_prompt(shape, B, C.csm_1b().text_vocab_size, seed0=9100 + 100 * B)
            assert tok.shape == (B, ROWS, 33) and all(not torch.equal(tok[0], tok[b]) for b in range(1, B))
            m = Model(csm_1b_args(), sd, max_frames=8, max_prefill_rows=B * ROWS)
            m.setup_caches(B)
            built[B] = (m, tok, msk)
        return built[B]

    yield get
    built.clear()


def _prefill(m, tok, msk):
    B, S = tok.shape[:2]
    m.reset_caches()
    m.prefill(tok, msk, torch.arange(S).unsqueeze(0).repeat(B, 1))


def _oracle_picks(logits, k, T, noise):
    """sample_topk of logits [32][B][V] with noise [32][B][V] -> picks [B][32]"""
    from oracle.csm_ref import sample_topk
    return sample_topk(logits.reshape(-1, V), k, T, q=noise.reshape(-1, V))[:, 0].view(NCB, -1).t().contiguous()


@pytest.mark.parametrize("B", [2, 5, 17, 32])
def test_batched_launch_samples_like_the_oracle_on_its_own_logits(csm1b_models, B):
    """B = 2, 5 (one half), 17 (a second half with ONE row), 32 (full): for each (T, k) of CASES the launch gets [32][B][V] bf16 Exp(1)
    noise, different in every row, and returns its logits; every pick [b][cb] must be sample_topk(logits[cb, b], k, T, q = noise[cb, b])
    -- so another row's or another codebook's noise, k or T from the wrong word, or scratch that a compute wave still reads, all show.
    A pick may differ only where the oracle's own bf16(p / q) of the two indices are within ONE bf16 ulp and the picked index is kept
    by top-k (fp32 order of the exp-sums: test_ops_gpu._assert_sampler_misses_are_one_ulp_ties); >= 95 % identical per B over all
    (T, k), the project's cap.  The share of rows whose two best bf16(p / q) are within an ulp -- computed from the oracle alone, the
    bound on legitimate misses -- must stay under 5 % (measured: docs/experiments/sampler_batch_parity.md).
    The test first shows, from the oracle alone, that it would SEE the plumbing faults: with k >= 30 a row sampled with its
    neighbour's noise, or codebook cb with cb + 1's, changes 1 - sum p^2 of the picks in expectation (> 0.9 on these logits);
    at least half must change.
    Feedback: a second call teacher-forced on the first call's picks returns bit-identical logits (the token fed to step cb + 1 IS
    the pick), and a second unforced call with the same noise returns the same picks."""
    from philox_ref import oracle_ratio, top2_tie_share
    from test_ops_gpu import _assert_sampler_misses_are_one_ulp_ties
    m, tok, msk = csm1b_models(B)
    assert m.fast_paths() & 2, "the batched persistent depth decoder (k_dec_persist_m) is not in charge"
    _prefill(m, tok, msk)
    g = torch.Generator().manual_seed(7700 + B)
    total = agree = ties = 0
    tie_rows = []
    for T, k in CASES:
        noise = torch.empty(NCB, B, V).exponential_(1, generator=g).to(torch.bfloat16).clamp_min(1e-30)
        out, logits = m.depth(B, T, k, noise=noise, want_logits=True, commit=False)
        got, lg = out.cpu(), logits.cpu()
        assert int(got.min()) >= 0 and int(got.max()) < V and bool(torch.isfinite(lg.float()).all())
        want = _oracle_picks(lg, k, T, noise)
        if k >= 30:
            for what, other in (("its neighbour row's noise", noise.roll(-1, 1)), ("the next codebook's noise", noise.roll(-1, 0))):
                moved = float((_oracle_picks(lg, k, T, other) != want).float().mean())
                print(f"B={B} T={T} k={k}: sampling with {what} changes {100 * moved:.1f} % of the oracle's picks")
                assert moved >= 0.5, f"T={T} k={k}: the test could not see a launch that used {what}"
        # [b][cb] -> the [32 * B] row order of logits / noise
        n_bad = _assert_sampler_misses_are_one_ulp_ties(lg.reshape(-1, V), T, k, noise.reshape(-1, V), got.t().reshape(-1), want.t().reshape(-1),
                                                        f"B={B} T={T} k={k}")
        assert n_bad == int((got != want).sum())
        total += got.numel(); agree += got.numel() - n_bad; ties += n_bad
        tie_rows.append(top2_tie_share(oracle_ratio(lg.reshape(-1, V), k, T, noise.reshape(-1, V))))
        out2, logits2 = m.depth(B, T, k, noise=noise, forced=out, want_logits=True, commit=False)
        assert torch.equal(logits2, logits), f"T={T} k={k}: the token fed to the next step is not the pick"
        assert torch.equal(out2, out), f"T={T} k={k}: teacher forcing changed the picks"
        assert torch.equal(m.depth(B, T, k, noise=noise, commit=False), out), f"T={T} k={k}: the launch is not deterministic"
    share = sum(tie_rows) / len(tie_rows)
    print(f"sampler inside the batched launch, B={B}: {agree}/{total} picks identical to the oracle's on the launch's logits, {ties} excused as "
          f"<= 1-ulp ties of p/q; oracle-only top-2 tie share {100 * share:.2f} % (per (T, k): {', '.join(f'{100 * s:.2f}' for s in tie_rows)})")
    assert share < 0.05, "these rows are too often ties of the oracle itself to grade the sampler: choose another noise seed"
    assert agree / total >= 0.95, f"agreement {agree / total:.3f}"


@pytest.mark.parametrize("B", [1, 2, 17, 32])
def test_in_kernel_philox_equals_the_standalone_samplers(csm1b_models, B):
    """No noise given: the launches draw from Philox.  For seeds 4242 and 0x123456789ABCDEF0 (high word set), at counter 0 (csm_seed
    writes {seed, 0}) and, after one committed frame, at counter 1 (only the end-of-frame advance increments it): the captured logits
    of every codebook go through the standalone k_sample (csm_op_sample) with rng = {seed, counter} and that codebook, and the picks
    must be IDENTICAL -- no excuse list: it is the same sample_body on the same bits, so a difference is plumbing (sequence index,
    codebook, key words, counter).  B = 1: k_dec_persist (and k_dec_first for codebook 1); B >= 2: k_dec_persist_m."""
    from sesameai import _abi
    from gpu_util import stream
    m, tok, msk = csm1b_models(B)
    if B == 1:
        assert m.fast_paths() & 1, "the persistent depth decoder (k_dec_persist) is not in charge"
        assert m.fast_paths() & 32, "the one-launch first decoder step (k_dec_first) is not in charge"
    else:
        assert m.fast_paths() & 2, "the batched persistent depth decoder (k_dec_persist_m) is not in charge"
    T, k, ldl = 0.9, 50, 2560
    total = agree = 0
    firsts = []
    for seed in SEEDS:
        m.seed(seed)
        _prefill(m, tok, msk)
        for counter in (0, 1):
            out, logits = m.depth(B, T, k, want_logits=True, commit=False)
            lg = torch.full((NCB, B, ldl), 99.0, dtype=torch.bfloat16, device=logits.device)      # padding must be ignored
            lg[:, :, :V] = logits
            rng = torch.tensor([seed, counter], dtype=torch.int64, device=logits.device)
            frame = torch.full((B, NCB), -1, dtype=torch.int32, device=logits.device)
            for cb in range(NCB):
                rc = _abi.lib.csm_op_sample(B, V, ldl, lg[cb].data_ptr(), T, k, None, rng.data_ptr(), cb, NCB, frame.data_ptr(), stream())
                assert rc == 0, _abi.lib.csm_last_error(None)
            torch.cuda.synchronize()
            same = out == frame
            total += same.numel(); agree += int(same.sum())
            assert bool(same.all()), (f"B={B} seed {seed:#x} counter {counter}: the launch and the standalone sampler differ at [row, codebook] "
                                      f"{(~same).nonzero().tolist()[:8]}")
            firsts.append(out.cpu())
            if counter == 0:
                m.depth(B, T, k, commit=True)                    # one committed frame: the advance increments the counter
    # the four (seed, counter) frames are different draws (same logits for codebook 0 within a seed: only the noise differs)
    for i in range(len(firsts)):
        for j in range(i + 1, len(firsts)):
            assert float((firsts[i] == firsts[j]).float().mean()) < 0.5, "two (seed, counter) pairs drew the same frame"
    print(f"in-kernel Philox vs the standalone sampler, B={B}: {agree}/{total} picks identical over seeds {[hex(s) for s in SEEDS]} x counters (0, 1)")
