"""Host reference of the sampler's on-device Exp(1) draws: a plain numpy Philox4x32-10 written from the published algorithm
(Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11, section 3.3 / Random123's philox.h constants) and
the draw built on it.  tests/test_philox_ref.py checks the generator against Random123's known-answer vectors -- nothing here
is derived from the kernel it grades (csrc/common.cuh philox4x32, csrc/sampler.cuh exp1_draw)."""
import numpy as np
import torch

M0, M1 = 0xD2511F53, 0xCD9E8D57              # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85              # Weyl key increments (golden ratio, sqrt(3) - 1)
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: four uint32 words, key: two uint32 words (scalars or numpy arrays that broadcast) -> four uint32 arrays.
    One round: (hi0, lo0) = M0 * c0, (hi1, lo1) = M1 * c2; c <- (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0); the key is bumped by
    the Weyl increments between rounds (nine times for ten rounds)."""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in ctr]
    k = [np.asarray(x, dtype=np.uint64) & MASK for x in key]
    for rnd in range(10):
        if rnd:
            k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]               # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK, p1 >> np.uint64(32), p1 & MASK
        c = [hi1 ^ c[1] ^ k[0], lo1, hi0 ^ c[3] ^ k[1], lo0]
    return [x.astype(np.uint32) for x in np.broadcast_arrays(*c)]


def exp1_draws(V, seed, step, sequence, codebook):
    """The V draws of one (sequence, codebook) row as the sampler defines them: counter (index, sequence, codebook, step_lo),
    key (seed_lo, seed_hi ^ step_hi); u = (float32(x) + 0.5) * 2**-32 of the first output word, q = bf16(-log(u)) in fp32,
    q <= 0 -> 1e-30.  Returns a bf16 tensor [V]."""
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    x = philox4x32_10((np.arange(V, dtype=np.uint64), sequence, codebook, step & 0xFFFFFFFF),
                      (seed & 0xFFFFFFFF, (seed >> 32) ^ (step >> 32)))[0]
    u = (x.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -32)
    q = torch.from_numpy((-np.log(u)).astype(np.float32)).to(torch.bfloat16)
    return torch.where(q > 0, q, torch.tensor(1e-30, dtype=torch.bfloat16))


# the grid tests/test_ops_gpu.py::test_sampler_philox_draws_equal_the_host_reference drives the kernel over
DRAW_V, DRAW_ROWS = 2051, 8
DRAW_SEEDS = (4242, 0x1234_5678_9ABC_DEF0)
DRAW_COUNTERS = (0, 1, 2 ** 32 + 3)
DRAW_CODEBOOKS = (0, 1, 17, 31)


def draw_grid():
    """(seed, counter, codebook, noise [DRAW_ROWS][DRAW_V] bf16) for every cell of the grid."""
    for seed in DRAW_SEEDS:
        for counter in DRAW_COUNTERS:
            for cb in DRAW_CODEBOOKS:
                yield seed, counter, cb, torch.stack([exp1_draws(DRAW_V, seed, counter, b, cb) for b in range(DRAW_ROWS)])


def top2_tie_share(r):
    """Share of the rows of r = bf16(p / q) [rows][V] whose two largest entries lie within one bf16 ulp: the rows in which an
    implementation that rounds one probability (or one draw) the other way may legitimately pick another index."""
    t = torch.topk(r.float(), 2, dim=-1)[0].to(torch.bfloat16).contiguous().view(torch.int16).to(torch.int32)    # r >= 0: the bit patterns are ordered
    return float(((t[:, 0] - t[:, 1]).abs() <= 1).float().mean())


def oracle_ratio(logits, k, T, q):
    """r = bf16(p / q) exactly as oracle.csm_ref.sample_topk forms it before its argmax."""
    import torch.nn.functional as F
    l = logits / T
    kth = torch.topk(l, k)[0][..., -1, None]
    p = F.softmax(F.log_softmax(l.masked_fill(l < kth, -float("inf")), dim=-1), dim=-1)
    return p / q
