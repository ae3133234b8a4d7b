"""The sampler INSIDE the batch-1 persistent depth-decoder launch (csrc/dec_persist.cuh, k_dec_persist: codebooks 2..31 of a frame).
Its front half -- keys, lower bound, candidate list -- runs on the gather wave alone, on the logits that wave's sweep left in its
registers (csrc/sampler.cuh, sample_wave_front); steps that form does not take (top-k 1 or beyond 128, a NaN logit, more than 128
candidates, more than 64 survivors) fall back to the 4-wave sample_body INSIDE the same launch.  Graded here, on a short prompt (8 rows):
  1. given Exp(1) noise, every pick of codebooks 2..31 is the oracle's sample_topk of the very logits the launch returned;
  2. every code equals the one the parent commit's library produced (tests/golden/dec_persist_sampler_pins.pt), no excuse;
  3. without noise, every pick is the stand-alone sampler's on the same logits and the same Philox {seed, counter};
  4. with forced= codes the picks still are the sampler's on each step's logits, and the next step's logits are the forced code's.
Results recorded in docs/experiments/sampler_on_gather.md.

The pins were written by this file's own launches on the parent commit's build of the library:
    CSM_HIP_LIB=<parent libcsm_hip.so> CSM_WRITE_SAMPLER_PINS=<parent commit> pytest tests/test_dec_persist_sampler_gpu.py"""
import os

import pytest
import torch

from test_frame_gpu import csm1b  # noqa: F401  (the shared full-size fixture)

pytestmark = pytest.mark.gpu

V, NCB, ROWS = 2051, 32, 8
PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dec_persist_sampler_pins.pt")
# (T, k).  k around every threshold of the sampler: 1 (greedy), 2, the product's 50, 64 | 65 (survivors per lane: ties at the kth value
# push steps of k = 64 and every step of k = 65 beyond 64 survivors, AFTER the list was published), 128 (more than 128 candidates) | 129
# (the first of the 4-wave form's 256 thread maxima), 256 | 257 (no lower bound beyond), V; a sharp and a flat temperature; and T = 8,
# 40, where bf16(l / T) collapses neighbouring logits (T = 40: more than 128 candidates in every step).  Which form each step takes is
# computed on the host (_form_of_step) and asserted in the first test.
CASES = tuple((0.9, k) for k in (1, 2, 49, 50, 64, 65, 128, 129, 256, 257, 2051)) + ((0.3, 50), (1.3, 50), (8.0, 50), (40.0, 50))
NOISE_SEED = 20262
EXCUSED_CAP = 0.05


@pytest.fixture(scope="module")
def short_model(csm1b):  # noqa: F811
    """A CSM-1B model with the first 8 rows of the golden prompt prefilled; no test commits a frame."""
    from sesameai.models import Model, csm_1b_args
    gold, sd = csm1b
    tok, msk = gold["prompt_tokens"][:ROWS], gold["prompt_mask"][:ROWS]
    m = Model(csm_1b_args(), sd, max_frames=8, max_prefill_rows=64)
    m.setup_caches(1)
    assert m.fast_paths() & 1, "the persistent depth decoder (k_dec_persist) is not in charge"
    m.prefill(tok.unsqueeze(0), msk.unsqueeze(0), torch.arange(ROWS).unsqueeze(0))
    yield m
    del m


@pytest.fixture(scope="module")
def launches(short_model):
    """One pair of identical launches per case, computed once: [(T, k, noise, picks, picks of the second call, logits)], on the host."""
    m = short_model
    g = torch.Generator().manual_seed(NOISE_SEED)
    res = []
    for T, k in CASES:
        noise = torch.empty(NCB, 1, V).exponential_(1, generator=g).to(torch.bfloat16).clamp_min(1e-30)
        out, logits = m.depth(1, T, k, noise=noise, want_logits=True, commit=False)
        out2 = m.depth(1, T, k, noise=noise, commit=False)
        res.append((T, k, noise[:, 0], out[0].cpu(), out2[0].cpu(), logits[:, 0].cpu()))
    return res


def _assert_misses_are_one_ulp_ties(lg, T, k, noise, got, want):
    """Codebooks 2..31 whose pick differs from the oracle's: each must be a tie of the oracle's own bf16(p / q) within one bf16 ulp."""
    import torch.nn.functional as F
    from gpu_util import bf16_ulp_diff
    bad = [cb for cb in (got != want).nonzero().flatten().tolist() if cb >= 2]
    for cb in bad:
        l = lg[cb:cb + 1] / T
        kth = torch.topk(l, k)[0][..., -1, None]
        probs = F.softmax(F.log_softmax(l.masked_fill(l < kth, -float("inf")), dim=-1), dim=-1)
        r = (probs / noise[cb])[0]
        ulp = int(bf16_ulp_diff(r[got[cb].long()], r[want[cb].long()]).max())
        print(f"   T={T} k={k} codebook {cb}: got {int(got[cb])} want {int(want[cb])}, bf16(p/q) {ulp} ulp apart")
        assert ulp <= 1, f"T={T} k={k} codebook {cb}: not a 1-ulp tie"
    return bad


def _form_of_step(row, T, k):
    """Which form of the sampler a step with these logits takes, by sample_wave_front's rule on the host: 'wave' (the one-wave form), or
    the reason for the 4-wave form -- 'k' (top-k 1 or beyond 128: known before the logits), 'nan', 'candidates' (more than 128: decided
    before a list is published) or 'survivors' (more than 64: decided after waves 4..6 drew the list's Exp(1) variates)."""
    import math
    if k <= 1 or min(k, V) > 128:
        return "k"
    raw = row.view(torch.int16).to(torch.int32) & 0xffff
    mag = raw & 0x7fff
    if bool((mag > 0x7f80).any()):
        return "nan"
    key = torch.where((raw & 0x8000) != 0, -mag, mag) + 32768                       # dense in the bf16 values, -0 == +0
    idx = torch.arange(V)
    group = ((idx // 4) % 64) * 2 + (idx & 1)                                       # lane of the sweep, even | odd element
    gm = torch.zeros(128, dtype=torch.int32).scatter_reduce(0, group, key, "amax")
    L = int(gm.sort(descending=True)[0][k - 1])
    margin = 2 * math.ceil(max(T, 1.0)) + 2
    cand = key >= (L - margin if L > margin else 1)
    n = int(cand.sum())
    if n > 128:
        return "candidates"
    t = row[cand] / T
    kept = int((t >= torch.topk(t.float(), k)[0][-1]).sum()) if n > k else n
    return "survivors" if kept > 64 else "wave"


def test_picks_are_the_oracles_on_the_launchs_own_logits(launches):
    """Picks of codebooks 2..31 == oracle.csm_ref.sample_topk(logits, k, T, q=noise); a second identical call reproduces them.  A miss
    is excused only where the oracle's own bf16(p / q) of the two indices are within one bf16 ulp (the rule of
    test_persistent_decoder_samples_like_the_oracle_on_its_own_logits); at most 5 % of all picks of the file may be excused."""
    from oracle.csm_ref import sample_topk
    total = excused = 0
    per_case, taken, mixed = [], {}, False
    for T, k, noise, got, got2, lg in launches:
        assert torch.equal(got, got2), f"T={T} k={k}: the persistent launch is not deterministic"
        assert int(got.min()) >= 0 and int(got.max()) < V and bool(torch.isfinite(lg.float()).all())
        want = sample_topk(lg, k, T, q=noise)[:, 0]
        bad = _assert_misses_are_one_ulp_ties(lg, T, k, noise, got, want)
        print(f"T={T} k={k}: {30 - len(bad)}/30 picks of codebooks 2..31 identical to the oracle's; differing codebooks {bad}")
        total += 30; excused += len(bad)
        per_case.append(len(bad))
        forms = [_form_of_step(lg[cb], T, k) for cb in range(2, NCB)]
        count = {f: forms.count(f) for f in ("wave", "k", "nan", "candidates", "survivors")}
        print(f"T={T} k={k}: paths of the 30 steps {count}")
        for f in count:
            taken[f] = taken.get(f, 0) + count[f]
        mixed = mixed or (count["wave"] > 0 and count["survivors"] > 0)
        assert count["k"] == (30 if k == 1 or k > 128 else 0) and count["nan"] == 0
    # the cases must drive the one-wave form, BOTH in-launch fallbacks, and the hand-over after a published list inside a launch that
    # also takes the one-wave form (measured: k = 64 -> 12 wave + 18 survivors steps, k = 65 -> 30 survivors, k = 128 and T = 40 -> 30
    # candidates each, T = 8 -> 30 wave)
    print(f"steps per path over the file: {taken}")
    assert all(taken[f] > 0 for f in ("wave", "k", "candidates", "survivors")) and mixed, f"paths taken: {taken}, mixed launch: {mixed}"
    print(f"sampler on the gather wave: {total - excused}/{total} picks identical to the oracle's, {excused} excused as 1-ulp ties of p/q "
          f"(per case: {per_case})")
    assert excused <= EXCUSED_CAP * total, f"{excused} of {total} picks excused"


def test_codes_are_the_parent_commits(launches):
    """Every code of every case, codebooks 0..31, equals what the parent commit's library produced for the same call: the one-wave form
    and its fallback change who does the work, not one bit of the result."""
    codes = torch.stack([got for (_, _, _, got, _, _) in launches]).to(torch.int32)
    parent = os.environ.get("CSM_WRITE_SAMPLER_PINS")
    if parent:
        torch.save({"codes": codes, "parent_commit": parent, "cases": [list(c) for c in CASES], "noise_seed": NOISE_SEED, "rows": ROWS}, PINS)
        print(f"wrote {PINS} from the library in charge")
    pins = torch.load(PINS)
    assert [tuple(c) for c in pins["cases"]] == list(CASES) and pins["noise_seed"] == NOISE_SEED and pins["rows"] == ROWS
    same = codes == pins["codes"]
    assert bool(same.all()), f"codes differ from the parent commit's ({pins['parent_commit'][:12]}) at [case, codebook] {(~same).nonzero().tolist()[:8]}"


@pytest.mark.parametrize("T,k", [(0.9, 50), (40.0, 50)])
def test_in_launch_philox_equals_the_standalone_sampler(short_model, T, k):
    """No noise: the launch draws from Philox.  On the model's stream (m.seed) and with a per-slot entry that carries a seed of its own
    (and the case's T, k, while the call's scalars say something else), the captured logits of every codebook go through the
    stand-alone k_sample with the same {seed, counter} and codebook: the picks must be identical, no excuse list."""
    from sesameai import _abi
    from gpu_util import stream
    m = short_model
    ldl = 2560
    runs = []
    seed = 0x1234_5678_9ABC_DEF0
    m.seed(seed)
    runs.append(("the model's stream", m.depth(1, T, k, want_logits=True, commit=False), seed, 0))
    own = 0xFEED_0000_0001
    m.set_slot_sampling([0], T, k, [own])
    try:
        entry = m.slot_sampling(0)
        assert entry["has_entry"] and entry["own_rng"] and entry["seed"] == own
        runs.append(("a slot entry with its own seed", m.depth(1, 1.0, 7, want_logits=True, commit=False), own, int(entry["counter"])))
    finally:
        m.clear_slot_sampling()
    for what, (out, logits), s, counter in runs:
        lg = torch.full((NCB, 1, ldl), 99.0, dtype=torch.bfloat16, device=logits.device)      # padding must be ignored
        lg[:, :, :V] = logits
        rng = torch.tensor([s - (1 << 64) if s >= (1 << 63) else s, counter], dtype=torch.int64, device=logits.device)
        frame = torch.full((1, NCB), -1, dtype=torch.int32, device=logits.device)
        for cb in range(NCB):
            rc = _abi.lib.csm_op_sample(1, V, ldl, lg[cb].data_ptr(), T, k, None, rng.data_ptr(), cb, NCB, frame.data_ptr(), stream())
            assert rc == 0, _abi.lib.csm_last_error(None)
        torch.cuda.synchronize()
        same = out == frame
        assert bool(same.all()), f"T={T} k={k}, {what}: the launch and the stand-alone sampler differ at [row, codebook] {(~same).nonzero().tolist()[:8]}"
    assert float((runs[0][1][0] == runs[1][1][0]).float().mean()) < 0.5, "two seeds drew the same frame"


def test_forced_feed_keeps_the_picks_and_feeds_the_forced_codes(short_model):
    """forced=: frame[] still holds the sampler's picks on each step's logits, while the next step is fed the forced code.  So a call
    forced on its own free-running picks returns the free run's logits and picks bit for bit, and a call forced on OTHER codes returns
    picks that are the oracle's on that call's logits, and logits that differ from the free run's."""
    from oracle.csm_ref import sample_topk
    m = short_model
    T, k = 0.9, 50
    g = torch.Generator().manual_seed(NOISE_SEED + 1)
    noise = torch.empty(NCB, 1, V).exponential_(1, generator=g).to(torch.bfloat16).clamp_min(1e-30)
    out, logits = m.depth(1, T, k, noise=noise, want_logits=True, commit=False)
    out2, logits2 = m.depth(1, T, k, noise=noise, forced=out, want_logits=True, commit=False)
    assert torch.equal(logits2, logits), "the token fed to the next step is not the pick"
    assert torch.equal(out2, out), "teacher forcing changed the picks"
    other = torch.randint(0, 2048, (1, NCB), generator=g).to(torch.int32)
    out3, logits3 = m.depth(1, T, k, noise=noise, forced=other, want_logits=True, commit=False)
    out4, logits4 = m.depth(1, T, k, noise=noise, forced=other, want_logits=True, commit=False)
    assert torch.equal(out3, out4) and torch.equal(logits3, logits4), "the forced launch is not deterministic"
    assert not torch.equal(logits3[3:], logits[3:]), "the forced codes were not fed"
    lg3, got = logits3[:, 0].cpu(), out3[0].cpu()
    want = sample_topk(lg3, k, T, q=noise[:, 0])[:, 0]
    miss = _assert_misses_are_one_ulp_ties(lg3, T, k, noise[:, 0], got, want)
    print(f"forced feed: {30 - len(miss)}/30 picks of codebooks 2..31 identical to the oracle's on the forced launch's logits")
    assert len(miss) <= EXCUSED_CAP * 30, f"picks under forced= are not the sampler's on the step's logits: codebooks {miss}"
