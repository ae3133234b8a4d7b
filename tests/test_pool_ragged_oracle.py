"""What makes the isolation test of tests/test_pool_ragged_gpu.py decisive, checked on the oracle alone (oracle/mimi_ref.py, no GPU): if a
ragged pool call gave stream A a neighbour's history, or no history at all, A's chunk would move by far more than the bound the GPU test
holds it to against the oracle (2e-5 of the peak, the project's Mimi bound).  The margin asked is 4 x that bound, the rule of the decisive
goldens; the measured factors are in docs/experiments/pool_ragged.md."""
import torch

REL_TOL = 2e-5          # the GPU test's bound against the oracle
MARGIN = 4.0
# the isolation case the GPU test runs: A and B each decode T0 frames of their own, then ONE ragged call carries A's next TA and B's next TB
SEED_A, SEED_B, T0, TA, TB = 91, 92, 4, 3, 7


def codes_of(seed, n):
    return torch.randint(0, 2048, (32, n), generator=torch.Generator().manual_seed(seed))


def test_a_leaked_or_lost_history_moves_the_chunk_by_four_times_the_bound():
    from oracle import mimi_ref as M
    s = M.mimi_tiny()
    w = M.make_weights(s, seed=4321, encoder=True)
    hop = s.hop
    for me, other, T_me in ((SEED_A, SEED_B, TA), (SEED_B, SEED_A, TB)):        # both directions
        mine, theirs = codes_of(me, T0 + T_me), codes_of(other, T0 + max(TA, TB))
        whole = M.decode(s, w, mine[None])[0, 0]
        chunk = whole[hop * T0:]
        peak = whole.abs().max().item()
        leaked = M.decode(s, w, torch.cat([theirs[:, :T0], mine[:, T0:]], dim=1)[None])[0, 0][hop * T0:]
        fresh = M.decode(s, w, mine[None, :, T0:])[0, 0]
        for what, wrong in (("the neighbour's history", leaked), ("no history", fresh)):
            moved = (wrong - chunk).abs().max().item()
            factor = moved / (REL_TOL * peak)
            print(f"seed {me}, {T_me}-frame chunk after {T0} frames, decoded with {what}: max|d|={moved:.3g} peak={peak:.3g} = {factor:.0f} x the bound")
            assert factor >= MARGIN, f"with {what} the chunk moves by only {factor:.2f} x the GPU bound: choose another seed"
