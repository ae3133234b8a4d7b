// The host side of the segment finisher (mimi_fin_*, include/mimi_hip.h): fp32 clips -> peak-normalised int16 with lead and tail silence and
// linear fades, every clip of a call in one launch chain.  This file validates a call, lays the outputs out back to back, builds the
// block -> (segment, tile) maps of both kernels and the struct that travels in the kernel arguments.  Plain C++: no HIP, so it also compiles
// into a stand-alone host program (tools/finish_plan_check.cpp, run under the host sanitizers).
//
// The rule, for one clip x[0 .. N) with lead L, tail T, fade F (samples):
//     peak = max(max |x_i| over the finite x_i, 1e-6f);  q_i = trunc((x_i / peak) * 32767.0f), 0 for a non-finite x_i;
//     y = L zeros ++ q ++ T zeros, M = L + N + T;  n = min(F, M / 2);  ramp r_j = float(j * (1.0 / (n - 1))) in float64, r_(n-1) = 1, and
//     r_0 = 0 for n == 1;  y[j] = trunc(float(y[j]) * r_j) and y[M - n + j] = trunc(float(y[M - n + j]) * r_(n-1-j)) for j < n.
//
// Tiling.  The peak of a segment is reduced in two steps: k_fin_peak writes one partial per PEAK tile, k_fin_write's blocks each reduce their
// segment's partials.  A segment's peak tile is max(FIN_PEAK_TILE, ceil(N / FIN_MAX_PTILES)) samples, so it never has more than
// FIN_MAX_PTILES = 256 partials -- one per thread of a write block -- and the handle's scratch of 64 * 256 floats, made once at create, holds any
// legal call (64 segments of 2^30 samples).  max is exact and order-free: no tiling can change a peak.
// int16 outputs are written as aligned 32-bit PAIRS.  Segment i starts at element O_i of `out`, which may be odd: `par` is the parity of its
// first output's ADDRESS (in int16 units), pair p of the segment holds its outputs 2p - par and 2p + 1 - par, and the one pair in front and
// the one behind that reach into a neighbour (or past the buffer) are written as a single int16.
#pragma once
#include <stdint.h>

#define FIN_MAX_SEGMENTS 64         // = MIMI_FIN_MAX_SEGMENTS
#define FIN_MAX_OUT (1L << 30)      // outputs (lead + samples + tail) of one segment
#define FIN_BLOCK 256               // threads per block, both kernels
#define FIN_PEAK_TILE 4096          // the smallest peak tile, samples
#define FIN_MAX_PTILES 256          // peak tiles (partials) of one segment at most; <= FIN_BLOCK
#define FIN_OUT_TILE 2048           // int16 slots (1024 aligned pairs) one write block covers

// One segment of one call, as the kernels get it.
struct FinSeg {
    const float* in;                // its n_in samples (device); never read when n_in == 0
    long out_off;                   // O_i: its first output, in elements of `out`
    int n_in, lead, m;              // N, L, M = L + N + T
    int nfade;                      // n = min(F, M / 2)
    int ptile, pblk0;               // samples per peak tile; the first of its ceil(N / ptile) blocks of k_fin_peak
    int par, wblk0;                 // parity of its first output's address; the first of its ceil((M + par) / FIN_OUT_TILE) blocks of k_fin_write
};

struct FinPlan {
    int n, pblocks, wblocks;        // segments; blocks of k_fin_peak and of k_fin_write in all
    FinSeg seg[FIN_MAX_SEGMENTS];
};

static inline int fin_ptiles(const FinSeg& g) { return g.n_in == 0 ? 0 : (int)(((long)g.n_in + g.ptile - 1) / g.ptile); }
static inline int fin_wtiles(const FinSeg& g) { return g.m == 0 ? 0 : (int)(((long)g.m + g.par + FIN_OUT_TILE - 1) / FIN_OUT_TILE); }

// lead + n_in + tail, or -1 where mimi_fin_segments would refuse the segment
static inline long fin_out_count(long n_in, long lead, long tail) {
    if (n_in < 0 || lead < 0 || tail < 0) return -1;
    if (n_in > FIN_MAX_OUT || lead > FIN_MAX_OUT || tail > FIN_MAX_OUT) return -1;
    const long m = n_in + lead + tail;
    return m > FIN_MAX_OUT ? -1 : m;
}

// Fills `plan`, out_off[i] and n_out[i] from the caller's host arrays.  Returns nullptr, or what is wrong (plan->n == 0 then: nothing may be
// launched).  `out` is only looked at for its alignment.
static inline const char* fin_plan_build(const float* const* in, const long* n_in, const int32_t* lead, const int32_t* tail, const int32_t* fade,
                                         int n, const void* out, long* out_off, long* n_out, FinPlan* plan) {
    plan->n = 0; plan->pblocks = 0; plan->wblocks = 0;
    if (!in || !n_in || !lead || !tail || !fade || !out || !out_off || !n_out) return "null pointer";
    if (n < 1 || n > FIN_MAX_SEGMENTS) return "segment list: need 1 .. 64 segments";
    if ((uintptr_t)out % sizeof(int16_t) != 0) return "the output buffer is not aligned to int16";
    for (int i = 0; i < n; ++i) {
        if (n_in[i] < 0) return "a clip of negative length";
        if (lead[i] < 0 || tail[i] < 0 || fade[i] < 0) return "a negative lead, tail or fade";
        if (fin_out_count(n_in[i], lead[i], tail[i]) < 0) return "a segment of more than 2^30 samples";
        if (n_in[i] > 0 && !in[i]) return "null pointer for a clip with samples";
        if (n_in[i] > 0 && (uintptr_t)in[i] % sizeof(float) != 0) return "a clip that is not aligned to fp32";
    }
    long O = 0;
    int pblocks = 0, wblocks = 0;
    for (int i = 0; i < n; ++i) {
        FinSeg& g = plan->seg[i];
        const long m = fin_out_count(n_in[i], lead[i], tail[i]);
        g.in = n_in[i] > 0 ? in[i] : nullptr;
        g.out_off = O;
        g.n_in = (int)n_in[i]; g.lead = lead[i]; g.m = (int)m;
        g.nfade = (int)(fade[i] < m / 2 ? fade[i] : m / 2);
        const long per = (n_in[i] + FIN_MAX_PTILES - 1) / FIN_MAX_PTILES;
        g.ptile = (int)(per > FIN_PEAK_TILE ? per : FIN_PEAK_TILE);
        g.pblk0 = pblocks;
        g.par = (int)(((uintptr_t)out / sizeof(int16_t) + (uintptr_t)O) & 1);
        g.wblk0 = wblocks;
        pblocks += fin_ptiles(g);
        wblocks += fin_wtiles(g);
        out_off[i] = O;
        n_out[i] = m;
        O += m;
    }
    for (int i = n; i < FIN_MAX_SEGMENTS; ++i) plan->seg[i] = FinSeg{};
    plan->n = n; plan->pblocks = pblocks; plan->wblocks = wblocks;
    return nullptr;
}
