"""Per-request temperature, top-k and seed inside a live batch: the per-slot sampling table (include/csm_hip.h csm_slot_sampling_*,
DESIGN.md 6c) as every sampler of the engine reads it -- k_sample (c0 and codebook 1), k_dec_persist (B = 1), k_dec_persist_m (B = 2..32)
and the batch-1 depth pass of csm_prefill_slot -- on the CSM-1B shapes (the persistent kernels exist only for those), and what it is
for: a request with a seed of its own gets the same frames whatever else the batch was doing when it arrived.
What the tests printed on an MI355X: docs/experiments/slot_sampling.md."""
import ctypes

import pytest
import torch

from test_batch_sampler_gpu import NCB, ROWS, V, _prefill, csm1b_models  # noqa: F401  (the fixture: one CSM-1B model per B, built on first use)

pytestmark = pytest.mark.gpu

# (T, k) of the rows, cycled; adjacent rows differ in k by >= 6 x (the visibility condition of test 1)
PAIRS = ((1.3, 5), (0.9, 50), (1.0, 1), (1.0, 2051), (2.5, 200))
SCALARS = (0.7, 30)           # the call's own pair: what a row WITHOUT an entry is sampled with; no entry holds it
NO_ENTRY_ROW = 1
BIG_SEED = 0x1234_5678_9ABC_DEF0
LDL = 2560


def _assert_kernels_in_charge(m, B):
    if B == 1:
        assert m.fast_paths() & 1, "the persistent depth decoder (k_dec_persist) is not in charge"
        assert m.fast_paths() & 32, "the one-launch first decoder step (k_dec_first) is not in charge"
    else:
        assert m.fast_paths() & 2, "the batched persistent depth decoder (k_dec_persist_m) is not in charge"


def _oracle(lg, k, T, q):
    """sample_topk of rows [n][V] -> picks [n]"""
    from oracle.csm_ref import sample_topk
    return sample_topk(lg, k, T, q=q)[:, 0]


def _lowest_argmax(lg):
    t = lg.float()
    idx = torch.arange(t.shape[-1]).expand_as(t)
    return torch.where(t == t.max(-1, keepdim=True)[0], idx, torch.full_like(idx, t.shape[-1])).min(-1)[0]


def _row_params(B):
    return [SCALARS if b == NO_ENTRY_ROW else PAIRS[b % len(PAIRS)] for b in range(B)]


def _picks_of(lg, noise, params):
    """The oracle's picks [B][32] of logits / noise [32][B][V] with row b sampled at params[b] (k == 1: the greedy rule)."""
    want = torch.empty(len(params), NCB, dtype=torch.int64)
    for b, (T, k) in enumerate(params):
        want[b] = _lowest_argmax(lg[:, b]) if k == 1 else _oracle(lg[:, b], k, T, noise[:, b])
    return want


@pytest.mark.parametrize("B", [5, 17])
def test_each_row_is_sampled_with_its_own_temperature_and_topk(csm1b_models, B):
    """Rows cycle through PAIRS, row 1 has NO entry and is sampled with the call's (0.7, 30); B = 17 puts one row into the second half of
    k_dec_persist_m.  With given Exp(1) noise every pick [b][cb] must be the oracle's sample_topk(logits[cb, b], k_b, T_b, q = noise[cb, b])
    on the launch's own logits; misses are graded per (T, k) group by test_ops_gpu._assert_sampler_misses_are_one_ulp_ties, agreement
    >= 95 % per B and an oracle-only top-2 tie share < 5 % (the project's caps, as in test_batch_sampler_gpu.py).  The greedy rows have no
    excuses: the lowest-index argmax.  Before that the test shows, from the oracle alone, that it would SEE a row sampled with its
    neighbour's (T, k): at least half of the oracle's picks change.  Feedback: a call teacher-forced on the picks returns the same logits."""
    from philox_ref import oracle_ratio, top2_tie_share
    from test_ops_gpu import _assert_sampler_misses_are_one_ulp_ties
    m, tok, msk = csm1b_models(B)
    _assert_kernels_in_charge(m, B)
    _prefill(m, tok, msk)
    params = _row_params(B)
    rows = [b for b in range(B) if b != NO_ENTRY_ROW]
    m.set_slot_sampling(rows, [params[b][0] for b in rows], [params[b][1] for b in rows])
    for b in range(B):
        e = m.slot_sampling(b)
        assert e["has_entry"] == (b != NO_ENTRY_ROW) and not e["own_rng"]
        if b != NO_ENTRY_ROW:
            assert (e["topk"], e["counter"]) == (params[b][1], 0) and abs(e["temperature"] - params[b][0]) < 1e-6
    g = torch.Generator().manual_seed(8800 + B)
    noise = torch.empty(NCB, B, V).exponential_(1, generator=g).to(torch.bfloat16).clamp_min(1e-30)
    out, logits = m.depth(B, *SCALARS, noise=noise, want_logits=True, commit=False)
    got, lg = out.cpu().long(), logits.cpu()
    assert int(got.min()) >= 0 and int(got.max()) < V and bool(torch.isfinite(lg.float()).all())
    want = _picks_of(lg, noise, params)
    moved = float((_picks_of(lg, noise, params[1:] + params[:1]) != want).float().mean())
    print(f"B={B}: sampling every row with its neighbour's (T, k) changes {100 * moved:.1f} % of the oracle's picks")
    assert moved >= 0.5, "the test could not see a launch that sampled a row with another row's entry"
    total = agree = 0
    tie_rows = []
    for T, k in sorted(set(params)):
        idx = [b for b in range(B) if params[b] == (T, k)]
        g_, w_ = got[idx].t().reshape(-1), want[idx].t().reshape(-1)                    # [cb][row] like the logits below
        if k == 1:
            assert torch.equal(g_, w_), f"B={B}: a greedy row (rows {idx}) did not pick the lowest-index argmax"
            n_bad = 0
        else:
            l_, q_ = lg[:, idx].reshape(-1, V), noise[:, idx].reshape(-1, V)
            n_bad = _assert_sampler_misses_are_one_ulp_ties(l_, T, k, q_, g_, w_, f"B={B} rows {idx} T={T} k={k}")
            assert n_bad == int((g_ != w_).sum())
            tie_rows.append(top2_tie_share(oracle_ratio(l_, k, T, q_)))
        print(f"B={B} rows {idx} (T={T}, k={k}{', no entry: the call scalars' if (T, k) == SCALARS else ''}): {g_.numel() - n_bad}/{g_.numel()} picks identical to the oracle's")
        total += g_.numel(); agree += g_.numel() - n_bad
    share = sum(tie_rows) / len(tie_rows)
    print(f"per-row (T, k), B={B}: {agree}/{total} picks identical to the oracle's on the launch's logits; oracle-only top-2 tie share {100 * share:.2f} %")
    assert share < 0.05, "these rows are too often ties of the oracle itself to grade the sampler: choose another noise seed"
    assert agree / total >= 0.95, f"agreement {agree / total:.3f}"
    out2, logits2 = m.depth(B, *SCALARS, noise=noise, forced=out, want_logits=True, commit=False)
    assert torch.equal(logits2, logits), "the token fed to the next step is not the pick"
    assert torch.equal(out2, out), "teacher forcing changed the picks"
    m.clear_slot_sampling()


def _standalone(lg, b, T, k, seed, counter, sequence):
    """Row b of logits [32][B][LDL] (device) through the standalone k_sample at Philox {seed, counter} and sequence index ``sequence`` -> [32]."""
    from sesameai import _abi
    from gpu_util import stream
    n = sequence + 1                                        # csm_op_sample's block index IS the sequence index: row b goes where block `sequence` reads
    rows = torch.zeros(NCB, n, LDL, dtype=torch.bfloat16, device=lg.device)
    rows[:, sequence] = lg[:, b]
    rng = torch.tensor([seed - (1 << 64) if seed >= (1 << 63) else seed, counter], dtype=torch.int64, device=lg.device)
    frame = torch.full((n, NCB), -1, dtype=torch.int32, device=lg.device)
    for cb in range(NCB):
        rc = _abi.lib.csm_op_sample(n, V, LDL, rows[cb].data_ptr(), T, k, None, rng.data_ptr(), cb, NCB, frame.data_ptr(), stream())
        assert rc == 0, _abi.lib.csm_last_error(None)
    torch.cuda.synchronize()
    return frame[sequence].cpu()


@pytest.mark.parametrize("B", [1, 2, 17])
def test_own_seed_draws_at_the_utterances_own_counter(csm1b_models, B):
    """No noise: the launches draw from Philox.  Every row has an entry; all but one have a seed of their own (row 0's has its high word set,
    at B = 17 rows 3 and 9 share seed and (T, k)), one row (the last, B >= 2) has an entry WITHOUT a seed.  For every row and codebook the
    captured logits go through the standalone csm_op_sample with B = 1, rng = {seed_b, counter} and the row's (T, k): IDENTICAL picks, no
    excuse list -- the same sample_body on the same bits at sequence index 0.  At counter 0 and, after one committed frame, at counter 1
    (slot_sampling reads 1).  The seedless row follows today's rule: the handle's {seed, step} at sequence index b.  One row is also
    compared with the host Philox (philox_ref.exp1_draws fed to the oracle's sample_topk, one-ulp rule).  set again: counter 0, and the
    picks of counter 0 come back."""
    from philox_ref import exp1_draws
    from test_ops_gpu import _assert_sampler_misses_are_one_ulp_ties
    m, tok, msk = csm1b_models(B)
    _assert_kernels_in_charge(m, B)
    handle_seed = 4242
    m.seed(handle_seed)
    _prefill(m, tok, msk)
    pairs = ((0.9, 50), (0.8, 40), (1.3, 5), (1.0, 200))
    params = [pairs[b % len(pairs)] for b in range(B)]
    seeds = [BIG_SEED] + [1000 + 7 * b for b in range(1, B)]
    seedless = B - 1 if B >= 2 else None
    if B == 17:
        seeds[9], params[9] = seeds[3], params[3]
    seeded = [b for b in range(B) if b != seedless]

    def set_all():
        m.set_slot_sampling(seeded, [params[b][0] for b in seeded], [params[b][1] for b in seeded], [seeds[b] for b in seeded])
        if seedless is not None:
            m.set_slot_sampling([seedless], *params[seedless])
    set_all()
    assert f"slot_sampling={B} entries ({len(seeded)} with own seed)" in m.describe()
    assert m.slot_sampling(0)["seed"] == BIG_SEED and m.slot_sampling(0)["own_rng"]
    firsts = []
    total = 0
    for counter in (0, 1):
        out, logits = m.depth(B, *SCALARS, want_logits=True, commit=False)
        lg = torch.full((NCB, B, LDL), 99.0, dtype=torch.bfloat16, device=logits.device)          # padding must be ignored
        lg[:, :, :V] = logits
        got = out.cpu()
        for b in range(B):
            assert m.slot_sampling(b)["counter"] == counter
            if b == seedless:
                want = _standalone(lg, b, *params[b], handle_seed, counter, b)
            else:
                want = _standalone(lg, b, *params[b], seeds[b], counter, 0)
            same = got[b] == want
            total += same.numel()
            assert bool(same.all()), (f"B={B} row {b} ({'handle stream' if b == seedless else hex(seeds[b])}) counter {counter}: the launch and the "
                                      f"standalone sampler differ at codebooks {(~same).nonzero().flatten().tolist()[:8]}")
        # the host Philox, for row 0: q of every codebook, then the oracle's sample_topk
        T0, k0 = params[0]
        q = torch.stack([exp1_draws(V, seeds[0], counter, 0, cb) for cb in range(NCB)])
        l0 = logits[:, 0].cpu()
        want0 = _oracle(l0, k0, T0, q)
        n_bad = _assert_sampler_misses_are_one_ulp_ties(l0, T0, k0, q, got[0].long(), want0, f"B={B} row 0 counter {counter} vs the host Philox")
        print(f"B={B} counter {counter}: row 0 vs host Philox + oracle: {NCB - n_bad}/{NCB} picks identical")
        firsts.append(got)
        if counter == 0:
            m.depth(B, *SCALARS, commit=True)                       # one committed frame: k_advance moves every row's own counter on
    assert float((firsts[0] == firsts[1]).float().mean()) < 0.5, "counters 0 and 1 drew the same frame"
    set_all()
    assert all(m.slot_sampling(b)["counter"] == 0 for b in range(B))
    again = m.depth(B, *SCALARS, commit=False).cpu()
    keep = [b for b in range(B) if b != seedless]                   # (the seedless row follows the handle's step, which stays at 1)
    assert torch.equal(again[keep], firsts[0][keep]), "after set the rows did not draw at counter 0 again"
    print(f"own seeds, B={B}: {total}/{total} picks identical to the standalone sampler at counters (0, 1); counter rewound by set")
    m.clear_slot_sampling()


# ---- a request no longer depends on the schedule -------------------------------------------------------------------------------------
R_SEED, R_PAIR = 0xFEED_0000_0001, (0.9, 50)
OTHER = {0: (1.3, 5, 11), 1: (0.8, 40, 12), 2: (1.0, 200, 13), 3: (0.8, 40, None), 4: (2.5, 200, 15)}      # slot -> (T, k, seed); slot 3 is seedless


def _other_prompts(n, seed0):
    import bench
    from types import SimpleNamespace
    from oracle import csm_ref as C
    shape = SimpleNamespace(ctx_text=8, ctx_frames=4, gen_text=3)
    return bench.synthetic_prompt(shape, n, C.csm_1b().text_vocab_size, seed0=seed0)


def _fill(m, tok, msk, skip=()):
    for s, (T, k, seed) in OTHER.items():
        if s not in skip:
            m.set_slot_sampling([s], T, k, None if seed is None else [seed])
            m.refill_slot(s, tok[s], msk[s], *SCALARS)


def _stalling_run(m, tok, msk, rt, rm, slot, steps_before, handle_seed=4242, frames=5):
    """R takes ``slot`` by refill_slot after ``steps_before`` graph-replayed steps of a full batch -> (R's frame 0 .. frame ``frames``, slot 3's rows)."""
    B = 5
    m.seed(handle_seed)
    m.reset_caches()
    if steps_before:
        _fill(m, tok, msk)
        for _ in range(steps_before):
            m.step(B, *SCALARS)
    else:
        _fill(m, tok, msk, skip=(slot,))
    m.set_slot_sampling([slot], *R_PAIR, [R_SEED])
    f0 = m.refill_slot(slot, rt, rm, *SCALARS).cpu()
    g0 = m.num_frames()
    for _ in range(frames):
        m.step(B, *SCALARS)
    fr, _ = m.read_frames(B, g0, frames)
    assert m.slot_sampling(slot)["counter"] == frames + 1
    return torch.cat([f0[None], fr[:, slot]]), fr[:, 3]


def _beside_run(m, tok, msk, rt, rm, slot, layers_per_call, frames=5):
    B = 5
    m.seed(4242)
    m.reset_caches()
    _fill(m, tok, msk)
    m.step(B, *SCALARS)
    m.set_slot_sampling([slot], *R_PAIR, [R_SEED])
    m.refill_begin(slot, rt, rm)
    while not m.refill_advance(layers_per_call):
        m.step(B, *SCALARS)                                     # the slot is parked: its own counter is held at 0
        assert m.slot_sampling(slot)["counter"] == 0
    g0 = m.num_frames()
    for _ in range(frames + 1):                                 # the first of them samples R's frame 0 in the batch
        m.step(B, *SCALARS)
    return m.read_frames(B, g0, frames + 1)[0][:, slot]


@pytest.fixture(scope="module")
def request_r(csm1b_models):
    m, tok, msk = csm1b_models(5)
    assert m.fast_paths() & 2
    rt, rm = _other_prompts(1, 31337)
    return m, tok, msk, rt[0], rm[0]


def test_a_seeded_request_does_not_depend_on_when_it_arrives(request_r):
    """B = 5, slot 2, request R = (prompt, seed, 0.9 / 50); the other slots hold other prompts with other entries.  Run A: R takes the slot
    right after reset_caches.  Run B: the batch first runs 3 graph-replayed steps with another request in slot 2.  R's frame 0 and its
    next 5 frames (graph replay) are bit-identical.  (On an engine that keys the draws on the global frame counter and the refill counter
    they cannot be.)  With another HANDLE seed R's frames still match, and the seedless neighbour's (slot 3) differ."""
    m, tok, msk, rt, rm = request_r
    a, n3a = _stalling_run(m, tok, msk, rt, rm, 2, 0)
    b, _ = _stalling_run(m, tok, msk, rt, rm, 2, 3)
    assert int(a.min()) >= 0 and a.shape == (6, NCB)
    assert torch.equal(a, b), f"R's frames depend on the schedule: first differing frame {int((a != b).any(1).nonzero()[0])}"
    c, n3c = _stalling_run(m, tok, msk, rt, rm, 2, 0, handle_seed=99)
    assert torch.equal(a, c), "R's frames depend on the handle's seed"
    assert not torch.equal(n3a, n3c), "the seedless neighbour did not follow the handle's seed"
    print("stalling refill, B=5 slot 2: R's 6 frames bit-identical after 0 and after 3 earlier steps, and under another handle seed")
    m.clear_slot_sampling()


def test_a_seeded_request_does_not_depend_on_the_slot_it_lands_in(request_r):
    """R in slot 1 of one run and in slot 3 of another (B = 5, the other slots hold what they always hold): the same 6 frames.  The draws
    cannot tell the slots apart (sequence index 0); that the LOGITS of a row do not depend on its row index in the batched kernels
    (mm.cuh, k_dec_persist_m) is what this measures on top."""
    m, tok, msk, rt, rm = request_r
    a, _ = _stalling_run(m, tok, msk, rt, rm, 1, 0)
    b, _ = _stalling_run(m, tok, msk, rt, rm, 3, 2)
    assert int(a.min()) >= 0
    assert torch.equal(a, b), f"R's frames depend on its slot: first differing [frame, codebook] {(a != b).nonzero()[0].tolist()}"
    print("stalling refill, B=5: R's 6 frames bit-identical in slot 1 (no earlier steps) and in slot 3 (after 2 earlier steps)")
    m.clear_slot_sampling()


def test_a_seeded_request_does_not_depend_on_how_its_refill_was_spread(request_r):
    """The same through refill_begin / refill_advance: one advance call that runs all the layers, against 4 layers per call spread over
    frame steps (the slot parked meanwhile, its counter held)."""
    m, tok, msk, rt, rm = request_r
    assert m.supports_refill_beside_the_loop(5)
    one = _beside_run(m, tok, msk, rt, rm, 2, m.bb.num_layers)
    spread = _beside_run(m, tok, msk, rt, rm, 2, 4)
    assert int(one.min()) >= 0 and one.shape == (6, NCB)
    assert torch.equal(one, spread), f"R's frames depend on how the refill was spread: first differing frame {int((one != spread).any(1).nonzero()[0])}"
    print("refill beside the loop, B=5 slot 2: R's 6 frames bit-identical with the layers in one call and spread over 4 frame steps")
    m.clear_slot_sampling()


def test_untouched_rows_and_handles(request_r):
    """Model X never calls set; model Y (same weights, handle seed, prompts, B = 5) holds an entry on row 1 only.  After prefill, a committed
    depth pass and 4 graph steps, rows 0, 2, 3, 4 are bit-identical and row 1 is not; after clear_slot_sampling Y reproduces X in every
    row.  Y captures ONE graph for the batch size however many distinct (T, k) its entries hold."""
    from sesameai.models import Model, csm_1b_args, state_dict_layout
    y, tok, msk, _, _ = request_r
    B, pair = 5, (0.65, 33)                                     # a scalar pair no other test steps with: the capture count below is exact

    def run(m):
        m.seed(777)
        _prefill(m, tok, msk)
        return m

    def frames(m):
        m.depth(B, *pair, commit=True)
        for _ in range(4):
            m.step(B, *pair)
        return m.read_frames(B)[0]
    x = Model(csm_1b_args(), {name: y._w[name] for name, _ in state_dict_layout(csm_1b_args())}, max_frames=8, max_prefill_rows=B * ROWS)      # (Y's device tensors: no copy)
    x.setup_caches(B)
    fx = frames(run(x))
    assert "slot_sampling=0 entries" in x.describe() and "carry the table" not in x.describe()
    del x
    caps = y.graph_captures()
    run(y).set_slot_sampling([1], 1.3, 5, [5])
    fy = frames(y)
    assert fy.shape == fx.shape == (5, B, NCB)
    assert torch.equal(fy[:, [0, 2, 3, 4]], fx[:, [0, 2, 3, 4]]), "an entry on row 1 changed another row"
    assert not torch.equal(fy[:, 1], fx[:, 1])
    assert y.graph_captures() == caps + 1
    run(y).set_slot_sampling([0, 1, 2, 3, 4], [1.3, 0.9, 1.0, 1.0, 2.5], [5, 50, 1, 2051, 200], [1, 2, 3, 4, 5])
    frames(y)
    run(y).set_slot_sampling([0, 2], [0.8, 0.6], [40, 7])
    frames(y)
    assert y.graph_captures() == caps + 1, "captures grew with the table's contents"
    run(y).clear_slot_sampling()
    assert torch.equal(frames(y), fx), "a handle whose table is empty does not reproduce one that never had a table"
    assert y.graph_captures() == caps + 1
    print("untouched rows / handles, B=5: rows 0, 2, 3, 4 bit-identical with an entry on row 1; cleared table == no table; 1 capture for 3 tables")


def test_errors_and_reset(request_r):
    from sesameai import _abi
    from gpu_util import stream
    m = request_r[0]
    lib, h = _abi.lib, m._h

    def call(slot, T, k):
        return lib.csm_slot_sampling_set(h, (ctypes.c_int32 * 1)(slot), 1, (ctypes.c_float * 1)(T), (ctypes.c_int32 * 1)(k), None, stream())
    m.reset_caches()
    for slot, T, k in ((0, 0.0, 50), (0, -1.0, 50), (0, float("nan"), 50), (0, 0.9, 0), (5, 0.9, 50), (-1, 0.9, 50)):
        assert call(slot, T, k) == -1, (slot, T, k)                # CSM_E_INVALID
        assert lib.csm_last_error(h), "no message"
        assert not any(m.slot_sampling(b)["has_entry"] for b in range(5))
    assert lib.csm_slot_sampling_get(h, 5, None, None, None, None, None, None, stream()) == -1
    assert lib.csm_slot_sampling_clear(h, (ctypes.c_int32 * 1)(5), 1, stream()) == -1
    with pytest.raises(ValueError):
        m.set_slot_sampling([0, 1], [0.9], 50)
    assert call(3, 0.9, 50) == 0
    m.set_slot_sampling([4], 0.8, 40, [BIG_SEED])
    assert m.slot_sampling(3) == {"has_entry": True, "temperature": pytest.approx(0.9), "topk": 50, "own_rng": False, "seed": 0, "counter": 0}
    assert m.slot_sampling(4)["seed"] == BIG_SEED and "slot_sampling=2 entries (1 with own seed)" in m.describe()
    m.clear_slot_sampling([3])
    assert not m.slot_sampling(3)["has_entry"] and m.slot_sampling(4)["has_entry"]
    m.reset_caches()                                            # csm_reset empties the table; csm_reset_slots leaves it alone
    assert not m.slot_sampling(4)["has_entry"] and "slot_sampling=0 entries" in m.describe()
    m.set_slot_sampling([4], 0.8, 40)
    m.reset_slots([4])
    assert m.slot_sampling(4)["has_entry"]
    m.clear_slot_sampling()
