// The host side of a pool of stateful polyphase resampler streams (mimi_rs_pool_*, include/mimi_hip.h): the filter (scipy.signal.resample_poly's
// default, made in float64), the per-stream running totals and the per-call plan that travels in the kernel arguments.  Plain C++: no HIP, so
// it also compiles into a stand-alone host program (tools/resample_plan_check.cpp, run under the host sanitizers).
//
// Indices.  With up = dst / g, down = src / g, half = 10 * max(up, down), output n of a clip x[0 .. N) is
//     y[n] = sum_k h[n * down + half - k * up] * x[k]      over 0 <= n * down + half - k * up <= 2 * half, 0 <= k < N,
// so only the DIFFERENCE n * down - k * up enters.  A stream keeps two running totals -- samples taken (k_base: the index of the next new
// sample) and outputs emitted (n0: the index of the next output) -- and after every call both are reduced by whole periods (up outputs <->
// down inputs), which leaves every difference as it was: the kernel sees small numbers however long the stream runs.  The clip's first sample
// then sits at a negative index k0 (kept in int64, handed to the kernel clamped): samples in front of it are zero BY INDEX, whatever the
// history memory holds, which is why a reset costs no launch.
#pragma once
#include <stdint.h>

#include <cmath>
#include <vector>

#include "stream_pool.h"

#define RS_MAX_STREAMS 64           // = MIMI_RS_MAX_STREAMS
static_assert(RS_MAX_STREAMS == SP_MAX_STREAMS, "the pools share one spine");
#define RS_MAX_FACTOR 320           // the largest reduced up or down mimi_rs_pool_create takes
#define RS_BLOCK 256                // outputs per block

struct RsRates { int up, down, half, hist; };      // hist = 2 * half / up + 1: the samples in front of a call's first that its outputs can reach

// One listed stream of one call, as the kernel gets it (32-bit but for the two offsets into the caller's buffers).
struct RsSeg {
    long in_off, out_off;           // elements: its new samples in `in`, its outputs in `out`
    int sid, bank;                  // which history bank the call READS (it writes the other one)
    int n_in, n_out;
    int n0, k_base;                 // reduced indices of the call's first output and first new sample
    int k0;                         // reduced index of the clip's first sample, clamped at RS_K0_FLOOR: samples before it are zero
    int blk0;                       // the first of its ceil(n_out / RS_BLOCK) blocks
};
#define RS_K0_FLOOR (-(1 << 30))

struct RsPlan {
    int n, blocks;                  // segments; output blocks in all (the n history blocks follow them)
    RsSeg seg[RS_MAX_STREAMS];
};

struct RsStream { long n_in, n_out, k0; int bank; };   // reduced totals, the clip's first sample (<= 0), the bank that holds the history

static inline long rs_gcd(long a, long b) { while (b) { const long t = a % b; a = b; b = t; } return a; }
static inline long rs_floor_div(long a, long b) { const long q = a / b; return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q; }

// nullptr, or why the pair of rates is refused
static inline const char* rs_rates(int src, int dst, RsRates* r) {
    r->up = r->down = r->half = r->hist = 0;
    if (src <= 0 || dst <= 0) return "a sample rate <= 0";
    if (src == dst) return "source and target rate are equal: nothing to resample";
    const long g = rs_gcd(src, dst);
    const long up = dst / g, down = src / g;
    if (up > RS_MAX_FACTOR || down > RS_MAX_FACTOR) return "reduced up or down factor above 320";
    r->up = (int)up; r->down = (int)down; r->half = 10 * (int)(up > down ? up : down); r->hist = 2 * r->half / r->up + 1;
    return nullptr;
}

// h[0 .. 2 * half] = firwin(2 * half + 1, 1 / max(up, down), window = ('kaiser', 5.0)) * up, in float64
static inline std::vector<double> rs_taps(const RsRates& r) {
    const int nt = 2 * r.half + 1;
    const double pi = 3.14159265358979323846, beta = 5.0, f = 1.0 / (r.up > r.down ? r.up : r.down);
    std::vector<double> h(nt);
    const double i0b = std::cyl_bessel_i(0.0, beta);
    double sum = 0;
    for (int i = 0; i < nt; ++i) {
        const double m = i - r.half, x = f * m;
        const double sinc = x == 0 ? 1.0 : std::sin(pi * x) / (pi * x);
        const double u = m / r.half, w = std::cyl_bessel_i(0.0, beta * std::sqrt(u * u < 1 ? 1 - u * u : 0.0)) / i0b;
        h[i] = f * sinc * w;
        sum += h[i];
    }
    for (int i = 0; i < nt; ++i) h[i] = h[i] / sum * r.up;
    return h;
}

// Outputs a stream with reduced totals (n_in, n_out) has emitted once it holds `more` further samples (final: and its clip has ended).
static inline long rs_emitted(const RsRates& r, long n_in, long n_out, long more, int final) {
    const long N = n_in + more;
    const long e = final ? rs_floor_div(N * r.up + r.down - 1, r.down) : rs_floor_div(N * r.up - 1 - r.half, r.down) + 1;
    return e > n_out ? e : n_out;
}

// nullptr, or why the reset is refused (then no state has moved).  An id may come twice: resetting a stream twice is resetting it.
static inline const char* rs_reset(int n_streams, RsStream* st, const int32_t* streams, int n) {
    if (!st || !streams) return "null pointer";
    if (const char* bad = sp_ids_bad(n_streams, streams, n, true)) return bad;
    for (int i = 0; i < n; ++i) { RsStream& s = st[streams[i]]; s.n_in = s.n_out = s.k0 = 0; }      // (the bank stays: nothing of it is read)
    return nullptr;
}

// Fills `plan` and `next` (the listed streams' states after the call; commit them once the launch is made) from the caller's host arrays.
// Returns nullptr, or what is wrong (plan->n == 0 then: nothing may be launched, no state may move).
static inline const char* rs_plan_build(const RsRates& r, int n_streams, const RsStream* st, const int32_t* streams, const long* in_off, const long* n_in,
                                        const int32_t* final, int n, const void* in, int in_fmt, const void* out, int out_fmt, long* n_out,
                                        RsPlan* plan, RsStream* next) {
    plan->n = 0; plan->blocks = 0;
    if (!st || !streams || !in_off || !n_in || !final || !in || !out || !n_out) return "null pointer";
    if (in_fmt != 0 && in_fmt != 1) return "unknown input format (0 = fp32, 1 = int16)";
    if (out_fmt != 0 && out_fmt != 1) return "unknown output format (0 = fp32, 1 = int16)";
    if (const char* bad = sp_ids_bad(n_streams, streams, n)) return bad;
    for (int i = 0; i < n; ++i) {
        const RsStream& s = st[streams[i]];
        if (const char* bad = sp_chunk_bad(n_in[i], in_off[i], 0)) return bad;        // (the totals are reduced: they never reach 2^48)
        if (rs_emitted(r, s.n_in, s.n_out, n_in[i], final[i] != 0) - s.n_out > SP_MAX_CHUNK) return "a chunk that gives more than 2^30 samples";
    }
    long O = 0;
    int blocks = 0;
    for (int i = 0; i < n; ++i) {
        const RsStream& s = st[streams[i]];
        RsSeg& g = plan->seg[i];
        const long e = rs_emitted(r, s.n_in, s.n_out, n_in[i], final[i] != 0);
        g.in_off = in_off[i]; g.out_off = O;
        g.sid = streams[i]; g.bank = s.bank;
        g.n_in = (int)n_in[i]; g.n_out = (int)(e - s.n_out);
        g.n0 = (int)s.n_out; g.k_base = (int)s.n_in;
        g.k0 = (int)(s.k0 > RS_K0_FLOOR ? s.k0 : RS_K0_FLOOR);
        g.blk0 = blocks;
        blocks += (g.n_out + RS_BLOCK - 1) / RS_BLOCK;
        O += g.n_out;
        n_out[i] = g.n_out;
        RsStream& t = next[i];
        if (final[i]) { t.n_in = 0; t.n_out = 0; t.k0 = 0; }          // the next sample starts a new clip
        else {
            t.n_in = s.n_in + n_in[i]; t.n_out = e; t.k0 = s.k0;
            const long qa = t.n_in / r.down, qb = t.n_out / r.up, q = qa < qb ? qa : qb;       // whole periods both totals hold
            t.n_in -= q * r.down; t.n_out -= q * r.up; t.k0 -= q * r.down;
        }
        t.bank = s.bank ^ 1;                                            // the call wrote the other bank
    }
    sp_zero_tail(plan->seg, n);
    plan->n = n; plan->blocks = blocks;
    return nullptr;
}
