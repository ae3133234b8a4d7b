"""The host Philox4x32-10 of tests/philox_ref.py against known answers that do not come from this project's kernel, and the
oracle-only tie share of the draw grid the GPU test uses (how many of its rows an exact implementation may legitimately miss)."""
import numpy as np
import torch

import philox_ref as P

# Random123's known-answer vectors for philox4x32, 10 rounds (its kat_vectors file): counter words, key words, expected output
KAT = [
    ((0x00000000,) * 4, (0x00000000,) * 2, (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),   # digits of pi
]


def test_host_philox_reproduces_the_published_known_answers():
    for ctr, key, want in KAT:
        got = tuple(int(x) for x in P.philox4x32_10(ctr, key))
        assert got == want, f"counter {[hex(c) for c in ctr]} key {[hex(k) for k in key]}: {[hex(g) for g in got]}"
    # vectorised over the first counter word like exp1_draws uses it: element i equals the scalar call
    v = P.philox4x32_10((np.arange(5, dtype=np.uint64), 7, 9, 11), (13, 15))
    for i in range(5):
        assert tuple(int(x[i]) for x in v) == tuple(int(x) for x in P.philox4x32_10((i, 7, 9, 11), (13, 15)))


def test_host_draws_are_exponential_and_every_counter_word_matters():
    q = torch.stack([P.exp1_draws(P.DRAW_V, 4242, 0, b, 3) for b in range(64)]).float()
    assert float(q.min()) > 0 and bool(torch.isfinite(q).all())
    assert abs(float(q.mean()) - 1.0) < 0.02 and abs(float(q.var()) - 1.0) < 0.06           # Exp(1): mean 1, variance 1 (131,264 draws)
    base = P.exp1_draws(P.DRAW_V, 4242, 5, 2, 3)
    for other in (P.exp1_draws(P.DRAW_V, 4243, 5, 2, 3), P.exp1_draws(P.DRAW_V, 4242 + 2 ** 32, 5, 2, 3), P.exp1_draws(P.DRAW_V, 4242, 6, 2, 3),
                  P.exp1_draws(P.DRAW_V, 4242, 5 + 2 ** 32, 2, 3), P.exp1_draws(P.DRAW_V, 4242, 5, 3, 3), P.exp1_draws(P.DRAW_V, 4242, 5, 2, 4)):
        assert float((other == base).float().mean()) < 0.05


def test_draw_grid_rows_are_rarely_ties_of_the_oracle_alone():
    """Equal logits, k = V, T = 1 (the GPU test's rows): the share of rows whose two largest bf16(p / q) lie within one ulp bounds the
    picks an exact kernel may miss (host log vs device logf: one draw a bf16 ulp apart).  Must stay under the 5 % the GPU test allows."""
    logits = torch.zeros(P.DRAW_ROWS, P.DRAW_V, dtype=torch.bfloat16)
    r = torch.cat([P.oracle_ratio(logits, P.DRAW_V, 1.0, noise) for _, _, _, noise in P.draw_grid()])
    share = P.top2_tie_share(r)
    print(f"draw grid: {r.shape[0]} rows, oracle-only top-2 tie share {100 * share:.2f} %")
    assert r.shape[0] == 192 and share < 0.05
