"""Why tests/test_mimi_latent_gpu.py grades the Mimi encoder's LATENT and not only its codes -- measured on the CPU oracle alone
(oracle/mimi_ref.py), no GPU:

* the code-level rule (tests/test_mimi_gpu.py ``_check_codes``) is coarse: with the whole pre-quantisation latent off by 1e-4 of its peak,
  or its last frame -- where the partial-frame rule and both paddings act -- off by 0.1 %, it passes with NO differing code, although
  either error is >= 5 x the 2e-5 of peak that the latent test allows;
* the fp32 oracle itself sits two orders of magnitude inside that bound of its float64 run, so the bound is not the oracle's noise;
* a duplicated winning centroid is a bit-exact tie whose analytic outcome -- the lower index, nothing else changed -- the oracle gives;
  ``tie_plan`` builds the placements the GPU test uses on ``k_rvq_pick``'s three tie-break sites.

The shared helpers (``float64_walk``, ``tie_plan``, ``books``) are imported by the GPU test."""
import torch
import torch.nn.functional as F

HOP = 1920
REL_TOL = 2e-5                    # the project's Mimi bound (tests/test_mimi_gpu.py), of the float64 latent's peak
SPLIT = lambda s: (("rvq_first.input_proj.weight", range(0, s.num_semantic)), ("rvq_rest.input_proj.weight", range(s.num_semantic, s.num_codebooks)))


def wav_of(seed, n, rows=1):
    return torch.randn(rows, 1, n, generator=torch.Generator().manual_seed(seed)) * 0.3


def books(s, w):
    return [w[f"rvq.{k}.embedding_sum"] / w[f"rvq.{k}.cluster_usage"].clamp(min=1e-5)[:, None] for k in range(s.num_codebooks)]


def latent64(s, w, wav):
    """The reference of the latent tests: the oracle on float64 weights and audio, (B, hidden, T)."""
    from oracle import mimi_ref as M
    return M.encode_latent(s, {k: v.double() for k, v in w.items()}, wav.double())


def float64_walk(s, w, z):
    """z (1, hidden, T): the oracle's residual quantiser in float64 -> (codes (K, T), relative gap between the two nearest centroids (K, T))."""
    w64 = {k: v.double() for k, v in w.items()}
    bk = books(s, w64)
    codes, gaps = [], []
    for proj, levels in SPLIT(s):
        res = F.conv1d(z.double(), w64[proj]).transpose(1, 2)[0]                     # (T, D)
        for k in levels:
            two = torch.cdist(res[None], bk[k][None], p=2)[0].topk(2, dim=-1, largest=False)
            codes.append(two.indices[:, 0]); gaps.append((two.values[:, 1] - two.values[:, 0]) / two.values[:, 0])
            res = res - bk[k][two.indices[:, 0]]
    return torch.stack(codes), torch.stack(gaps)


# k_rvq_pick (256 threads, centroid c in thread c % 256) breaks ties at three sites: inside a thread (ascending c), between the lanes of a
# wave (shuffles), between the four waves (shared memory).  One placement above and one below the winner for each, over three levels.
# (Deepest level first: a frame whose 32 decisions all have wide margins is rare, so those are handed out before the shallow levels take them.)
TIE_SITES = ((31, "wave", +1), (31, "lane", -1), (12, "lane", +1), (12, "thread", -1), (0, "thread", +1), (0, "wave", -1))
MIN_MARGIN = 1e-3


def _site(win, dup):
    if (dup - win) % 256 == 0:
        return "thread"
    return "lane" if (dup % 256) // 64 == (win % 256) // 64 else "wave"


def tie_plan(s, w, codes, gaps):
    """codes, gaps (K, T) from ``float64_walk`` on the undoctored books -> (plan, doctored weights, expected codes (K, T)).  Each entry of
    TIE_SITES takes the first unused frame all of whose decisions up to that level have margins >= MIN_MARGIN, and copies its winning
    centroid (embedding_sum and cluster_usage) into the nearest row, on the wanted side and tie-break site, that no frame of the level
    uses.  Expected: min(winner, duplicate) wherever that level chose the winner; nothing else changes."""
    w2 = {k: v.clone() for k, v in w.items()}
    want = codes.clone()
    plan, used_frames, taken = [], set(), {}
    for level, site, side in TIE_SITES:
        frame = next(t for t in range(codes.shape[1]) if t not in used_frames and bool((gaps[:level + 1, t] >= MIN_MARGIN).all()))
        win = int(codes[level, frame])
        busy = set(codes[level].tolist()) | taken.setdefault(level, set())
        dup = next(c for c in (win + side * k for k in range(1, s.codebook_size)) if 0 <= c < s.codebook_size and c not in busy and _site(win, c) == site)
        for name in ("embedding_sum", "cluster_usage"):
            w2[f"rvq.{level}.{name}"][dup] = w[f"rvq.{level}.{name}"][win]
        want[level][codes[level] == win] = min(win, dup)
        used_frames.add(frame); taken[level] |= {win, dup}
        plan.append((level, frame, win, dup, site))
    return plan, w2, want


def _codes_rule_passes_unchanged(s, w, wav, zz, what):
    from oracle import mimi_ref as M
    from test_mimi_gpu import _check_codes
    got = M.quantize(s, w, zz)
    _check_codes(got, s, w, wav, what)                                               # the code-level rule, as the GPU tests apply it
    return int((got != M.encode(s, w, wav)).sum())


def _coarseness(s, wav, name):
    from oracle import mimi_ref as M
    w = M.make_weights(s, seed=4321, encoder=True)
    z = M.encode_latent(s, w, wav)
    z64 = latent64(s, w, wav)
    peak = z64.abs().max().item()
    own = (z.double() - z64).abs().max().item() / peak
    print(f"{name}: fp32 oracle vs float64 oracle {own:.3g} of peak")
    assert own <= REL_TOL / 10, "the fp32 oracle is not far inside the latent bound"
    # (a) the whole latent off by 1e-4 of peak (uniform noise whose largest element is exactly that)
    u = (torch.rand(z.shape, generator=torch.Generator().manual_seed(0)) * 2 - 1).double()
    noise = 1e-4 * peak * u / u.abs().max()
    assert noise.abs().max().item() >= 5 * REL_TOL * peak * (1 - 1e-12)
    zz = (z.double() + noise).float()
    seen = (zz.double() - z64).abs().max().item() / peak                              # what the latent test would measure
    assert _codes_rule_passes_unchanged(s, w, wav, zz, f"{name}, latent + 1e-4 of peak") == 0
    # (b) the last frame alone off by 0.1 %
    zl = z.clone(); zl[..., -1] *= 1.001
    last = (zl[..., -1].double() - z64[..., -1]).abs().max().item() / z64[..., -1].abs().max().item()
    assert _codes_rule_passes_unchanged(s, w, wav, zl, f"{name}, last frame x 1.001") == 0
    print(f"{name}: both pass the code-level rule with no differing code; the latent test would measure {seen:.3g} of peak (whole clip) "
          f"and {last:.3g} of the last frame's peak: {seen / REL_TOL:.1f} x and {last / REL_TOL:.1f} x its bound")
    # (the noise itself is >= 5 x the bound, asserted above; measured against float64 it moves by the fp32 oracle's own 1e-6 of peak)
    assert seen >= 5 * REL_TOL * (1 - 1e-2) and last >= 5 * REL_TOL


def test_code_level_rule_lets_a_wrong_latent_through_tiny():
    from oracle import mimi_ref as M
    _coarseness(M.mimi_tiny(), wav_of(12, HOP * 9 + 777), "tiny, 9 frames + 777")


def test_code_level_rule_lets_a_wrong_latent_through_full_size():
    from oracle import mimi_ref as M
    _coarseness(M.mimi_full(), wav_of(13, HOP * 6 + 5), "full size, 6 frames + 5")


TIE_CLIP = (6, HOP * 19 + 300)                                                       # seed, samples: 20 frames, 6 of them with wide margins throughout


def test_duplicated_centroids_tie_exactly_and_the_first_index_wins():
    from oracle import mimi_ref as M
    s = M.mimi_tiny()
    w = M.make_weights(s, seed=4321, encoder=True)
    wav = wav_of(*TIE_CLIP)
    c0 = M.encode(s, w, wav)[0]
    codes, gaps = float64_walk(s, w, M.encode_latent(s, w, wav))
    plan, w2, want = tie_plan(s, w, codes, gaps)
    assert [(l, k) for l, _, _, _, k in plan] == [(l, k) for l, k, _ in TIE_SITES] and len({f for _, f, _, _, _ in plan}) == len(TIE_SITES)
    for level, frame, win, dup, site in plan:
        assert torch.equal(codes[:level + 1, frame], c0[:level + 1, frame]), "the float64 walk and the fp32 oracle part before a planned tie"
        assert _site(win, dup) == site and dup not in c0[level].tolist()
    assert {(l, k, (d > w_) - (d < w_)) for l, _, w_, d, k in plan} == set(TIE_SITES)     # each site once above and once below the winner
    c2 = M.encode(s, w2, wav)[0]
    expect = c0.clone()
    for level, frame, win, dup, site in plan:
        expect[level][c0[level] == win] = min(win, dup)
    assert torch.equal(c2, expect), "the oracle on the doctored books is not min(winner, duplicate) at the ties and unchanged elsewhere"
    assert int((c2 != c0).sum()) >= 3                                                # the three placements below their winner moved a code
    print("tie plan (level, frame, winner, duplicate, site):", plan)
