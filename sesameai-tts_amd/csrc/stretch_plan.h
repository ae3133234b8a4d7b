// The host side of a pool of stateful WSOLA time-stretch streams (mimi_ts_pool_*, include/mimi_hip.h states the rule): the per-stream host
// state {pm, R, k, parity}, the emitted block counts, the packed output offsets and the per-call plan that travels in the kernel arguments.
// Plain C++: no HIP, so it also compiles into a stand-alone host program (tools/stretch_plan_check.cpp, run under the host sanitizers).
//
// Positions.  Block k reads x from a_k - D = (k H pm) / 1000 - D on (and from b_k = c_(k-1) + H >= a_(k-1) - D + H on), so a stream whose next
// block is k keeps its samples from base(k) = max(0, a_(k-1) - D) on (base(0) = 0): fewer than TS_CARRY of them, because block k would have
// come out had a_k + D + 2H of them been there.  Everything the kernel sees is RELATIVE to base(k) of the call's first block: the carry is
// positions [0, L), the new chunk [L, L + n_in), a_k - base fits 32 bits however long the stream has run; the 64-bit products stay here.
#pragma once
#include <stdint.h>

#include "stream_pool.h"

#define TS_MAX_STREAMS 64           // = MIMI_TS_MAX_STREAMS
static_assert(TS_MAX_STREAMS == SP_MAX_STREAMS, "the pools share one spine");
#define TS_H 512                    // block and hop
#define TS_D 256                    // search radius
#define TS_LOOK (TS_D + 2 * TS_H)   // block k comes out once a_k + TS_LOOK samples are in
#define TS_CARRY 2560               // floats a stream keeps between calls (the most it needs is 2,559)
#define TS_PM_MIN 500
#define TS_PM_MAX 2000

// One listed stream of one call, as the kernel gets it: 48 bytes.
struct TsSeg {
    long in_off, out_off;           // elements: its new samples in `in`, its outputs in `out`
    int sid;                        // sp_sid_word | fresh << 10 (k0 == 0)
    int L, n_in, n_out;             // carry samples; new samples; outputs (ceil(n_out / H) blocks, only a final's last one cut)
    int a0, rem;                    // a_k0 - base and (k0 H pm) % 1000: a_(k0+i) - base = a0 + (rem + i H pm) / 1000;  rem | pm << 10
    int shift;                      // base of the stream's next call - base of this one: the new carry is positions [shift, L + n_in)
    int blk_off;                    // its blocks' place in d_out
};
#define TS_FRESH(g) (((g).sid >> 10) & 1)
#define TS_REM(g) ((g).rem & 0x3FF)
#define TS_PM(g) ((g).rem >> 10)

struct TsPlan {
    int n, blocks;                  // segments; output blocks in all
    TsSeg seg[TS_MAX_STREAMS];
};

struct TsStream { long R, k; int pm, parity; };     // samples taken and blocks emitted since the reset; speed; the bank that holds the carry

static inline long ts_a(long k, int pm) { return k * TS_H * pm / 1000; }                                  // k <= 2^41 (SP_MAX_TOTAL samples): inside 63 bits
static inline long ts_base(long k, int pm) { const long b = k >= 1 ? ts_a(k - 1, pm) - TS_D : 0; return b > 0 ? b : 0; }
static inline long ts_out_len(long N, int pm) { return (N * 1000 + pm - 1) / pm; }

// Blocks a stream has emitted after R samples in all (final: and its clip has ended).
static inline long ts_emitted(long R, int pm, int final) {
    if (final) return (ts_out_len(R, pm) + TS_H - 1) / TS_H;
    const long T = R - TS_LOOK;
    return T < 0 ? 0 : ((T + 1) * 1000 - 1) / ((long)TS_H * pm) + 1;
}

// Samples a feed of `more` samples gives a stream now.
static inline long ts_out_count(const TsStream& s, long more, int final) {
    const long R = s.R + more;
    return final ? ts_out_len(R, s.pm) - s.k * TS_H : (ts_emitted(R, s.pm, 0) - s.k) * TS_H;
}

// nullptr, or why the reset is refused (then no state has moved)
static inline const char* ts_reset(int n_streams, TsStream* st, const int32_t* streams, const int32_t* speed_pm, int n) {
    if (!st || !streams || !speed_pm) return "null pointer";
    if (const char* bad = sp_ids_bad(n_streams, streams, n)) return bad;
    for (int i = 0; i < n; ++i)
        if (speed_pm[i] < TS_PM_MIN || speed_pm[i] > TS_PM_MAX) return "speed outside 500 .. 2000 permille";
    for (int i = 0; i < n; ++i) { TsStream& s = st[streams[i]]; s.R = 0; s.k = 0; s.pm = speed_pm[i]; }      // (the parity stays: a fresh stream reads no carry)
    return nullptr;
}

// Fills `plan` and `next` (the listed streams' states after the call; commit them once the launch is made) from the caller's host arrays.
// Returns nullptr, or what is wrong (plan->n == 0 then: nothing may be launched, no state may move).
static inline const char* ts_plan_build(int n_streams, const TsStream* st, const int32_t* streams, const long* in_off, const long* n_in,
                                        const int32_t* final, int n, const void* in, const void* out, long* n_out, TsPlan* plan, TsStream* next) {
    plan->n = 0; plan->blocks = 0;
    if (!st || !streams || !in_off || !n_in || !final || !in || !out || !n_out) return "null pointer";
    if (const char* bad = sp_ids_bad(n_streams, streams, n)) return bad;
    for (int i = 0; i < n; ++i) {
        const TsStream& s = st[streams[i]];
        if (s.pm < TS_PM_MIN || s.pm > TS_PM_MAX) return "speed outside 500 .. 2000 permille";
        if (const char* bad = sp_chunk_bad(n_in[i], in_off[i], s.R)) return bad;
        if (ts_out_count(s, n_in[i], final[i] != 0) > SP_MAX_CHUNK) return "a chunk that gives more than 2^30 samples";
    }
    long O = 0;
    int blocks = 0;
    for (int i = 0; i < n; ++i) {
        const TsStream& s = st[streams[i]];
        TsSeg& g = plan->seg[i];
        const int fin = final[i] != 0;
        const long R1 = s.R + n_in[i], k1 = ts_emitted(R1, s.pm, fin), base = ts_base(s.k, s.pm);
        const long cnt = ts_out_count(s, n_in[i], fin);
        g.in_off = in_off[i]; g.out_off = O;
        g.sid = sp_sid_word(streams[i], s.parity, fin) | (s.k == 0) << 10;
        g.L = (int)(s.R - base); g.n_in = (int)n_in[i]; g.n_out = (int)cnt;
        g.a0 = (int)(ts_a(s.k, s.pm) - base);
        g.rem = (int)(s.k * TS_H * s.pm % 1000) | s.pm << 10;
        g.shift = fin ? 0 : (int)(ts_base(k1, s.pm) - base);
        g.blk_off = blocks;
        blocks += (int)((cnt + TS_H - 1) / TS_H);
        O += cnt;
        n_out[i] = cnt;
        TsStream& t = next[i];
        t.pm = s.pm; t.parity = s.parity ^ 1;                         // the call wrote the other bank
        if (fin) { t.R = 0; t.k = 0; }                                // the next sample starts a new clip
        else { t.R = R1; t.k = k1; }
    }
    sp_zero_tail(plan->seg, n);
    plan->n = n; plan->blocks = blocks;
    return nullptr;
}
