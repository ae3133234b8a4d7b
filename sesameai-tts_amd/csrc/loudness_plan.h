// The host side of a pool of loudness-meter streams (mimi_ld_pool_*, include/mimi_hip.h states the rule): the per-stream host state
// {R, k, bank}, the hop counts, the packed hop offsets and the per-call plan that travels in the kernel arguments.
// Plain C++: no HIP, so it also compiles into a stand-alone host program (tools/loudness_plan_check.cpp, run under the host sanitizers).
//
// Positions.  Hop k's K-weighted samples read the stream from k H - (T - 1) on, so a stream whose next unmeasured hop is k keeps its samples
// from base(k) = k H - 511 on: 511 + R % H <= 2910 of them (R: samples taken since the stream was fresh), fewer while base(k) < 0, where the
// positions in front of the clip are zero by rule and are not kept.  Everything the kernels see is RELATIVE to base(k0) of the call's first
// hop: `lead` rule zeros, then the carry, then the new chunk; hop k0 + i reads positions [i H, i H + H + T - 1).  The totals stay here.
#pragma once
#include <stdint.h>

#include "loudness_taps.h"
#include "stream_pool.h"

#define LD_MAX_STREAMS 64            // = MIMI_LD_MAX_STREAMS
static_assert(LD_MAX_STREAMS == SP_MAX_STREAMS, "the pools share one spine");
#define LD_H 2400                    // hop: 100 ms
#define LD_HIST (LD_T - 1)           // samples in front of its next hop that a stream keeps: 511
#define LD_SPAN (LD_H + LD_T - 1)    // samples one hop's energy reads: 2911
#define LD_CARRY 2912                // int16 values per bank (the most a stream keeps is 2910)
#define LD_RING_DEFAULT 4096         // hop energies a stream holds: 409.6 s
#define LD_RING_MAX 4096             // 10 * n_abs * E[j] < 10 * 4096 * 9600 * 2^34 < 2^63: the relative gate compares in 64 bits
#define LD_RING_MIN 4                // one gating block
#define LD_GATE_ABS 1208568L         // floor(4 H 2^30 10^((-70 + 0.691) / 10)): a block passes the absolute gate when E > this
#define LD_ROW 4                     // int64 per stream that integrate writes: S, n, peak, hops
static_assert((long)LD_TAPS_ABS_SUM * 32768 < (1L << 31), "an int32 accumulation could overflow");
static_assert(LD_T == 512 && LD_Q == 14 && LD_SPAN <= LD_CARRY, "loudness.hip is laid out for these");

// One listed stream of one call, as the kernels get it: 40 bytes.
struct LdSeg {
    long in_off;                     // elements: its new samples in `in`
    long k0;                         // hops measured since the stream was fresh
    int sid;                         // sp_sid_word
    int Lc, n_in;                    // carry samples (0: the stream is fresh); new samples
    int nf, f_off;                   // hops measured in this call; their place in the per-hop output
    int pad;
};
#define LD_LEAD(g) ((g).k0 == 0 ? LD_HIST : 0)      // rule zeros in front of the carry (H > T - 1: only hop 0 reaches in front of the clip)

struct LdPlan {
    int n, hops;                     // segments; hops in all
    LdSeg seg[LD_MAX_STREAMS];
};

struct LdStream { long R, k; int parity, touched; };      // samples taken and hops measured since fresh; the bank that holds the carry; fed since its reset

static inline long ld_carry_len(long R) { const long c = LD_HIST + R % LD_H; return R < c ? R : c; }
static inline long ld_hop_count(const LdStream& s, long more) { return (s.R + more) / LD_H - s.k; }

static inline const char* ld_ring_bad(int ring_hops) {
    return ring_hops != 0 && (ring_hops < LD_RING_MIN || ring_hops > LD_RING_MAX) ? "ring outside 4 .. 4096 hops (0: the default)" : nullptr;
}

// nullptr, or why the reset is refused (then no state has moved)
static inline const char* ld_reset(int n_streams, LdStream* st, const int32_t* streams, int n) {
    if (!st || !streams) return "null pointer";
    if (const char* bad = sp_ids_bad(n_streams, streams, n)) return bad;
    for (int i = 0; i < n; ++i) {                                                      // (the parity stays: a fresh stream reads no carry)
        LdStream& s = st[streams[i]];
        s.R = 0; s.k = 0; s.touched = 0;
    }
    return nullptr;
}

// Fills `plan` and `next` (the listed streams' states after the call; commit them once the launches are made) from the caller's host
// arrays.  Returns nullptr, or what is wrong (plan->n == 0 then: nothing may be launched, no state may move).
static inline const char* ld_plan_build(int n_streams, const LdStream* st, const int32_t* streams, const long* in_off, const long* n_in,
                                        const int32_t* final, int n, const void* in, int in_is_i16, const void* energy, long* n_hops,
                                        LdPlan* plan, LdStream* next) {
    plan->n = 0; plan->hops = 0;
    if (!st || !streams || !in_off || !n_in || !final || !in || !energy || !n_hops) return "null pointer";
    if (in_is_i16 != 0 && in_is_i16 != 1) return "unknown input format";
    if ((uintptr_t)in % (in_is_i16 ? 2 : 4) || (uintptr_t)energy % 8) return "a misaligned buffer";
    if (const char* bad = sp_ids_bad(n_streams, streams, n)) return bad;
    long total = 0;
    for (int i = 0; i < n; ++i) {
        const LdStream& s = st[streams[i]];
        if (const char* bad = sp_chunk_bad(n_in[i], in_off[i], s.R)) return bad;
        total += ld_hop_count(s, n_in[i]);
    }
    if (total > (1L << 30)) return "a call of more than 2^30 hops";
    int hops = 0;
    for (int i = 0; i < n; ++i) {
        const LdStream& s = st[streams[i]];
        LdSeg& g = plan->seg[i];
        const int fin = final[i] != 0;
        const long nf = ld_hop_count(s, n_in[i]);
        g.in_off = in_off[i]; g.k0 = s.k;
        g.sid = sp_sid_word(streams[i], s.parity, fin);
        g.Lc = (int)ld_carry_len(s.R); g.n_in = (int)n_in[i];
        g.nf = (int)nf; g.f_off = hops; g.pad = 0;
        hops += (int)nf;
        n_hops[i] = nf;
        LdStream& t = next[i];
        t = s; t.parity = s.parity ^ 1; t.touched = 1;                 // the call wrote the other bank
        if (fin) { t.R = 0; t.k = 0; }                                // the next sample starts a new clip
        else { t.R = s.R + n_in[i]; t.k = s.k + nf; }
    }
    sp_zero_tail(plan->seg, n);
    plan->n = n; plan->hops = hops;
    return nullptr;
}

// nullptr, or why an integrate over the listed streams into `out` is refused
static inline const char* ld_integrate_bad(int n_streams, const int32_t* streams, int n, const void* out) {
    if (!streams || !out) return "null pointer";
    if ((uintptr_t)out % 8) return "a misaligned buffer";
    return sp_ids_bad(n_streams, streams, n);
}

// What mimi_fin_segments_ld takes beside the finisher's own plan: per segment the target mean square P_T (0: the peak rule) and the
// ceiling C, both in int16 units.
#define LD_PT_MAX (1L << 31)         // 0 LUFS is 1.17 * 2^30
struct FinLd { long pt[LD_MAX_STREAMS]; int ceil[LD_MAX_STREAMS]; };

static inline const char* fin_ld_build(const long* pt, const int32_t* ceil, int n, const void* meter, FinLd* ld) {
    if (!pt || !ceil || !meter) return "null pointer";
    if ((uintptr_t)meter % 8) return "a misaligned buffer";
    if (n < 1 || n > LD_MAX_STREAMS) return "segment list: need 1 .. 64 segments";
    for (int i = 0; i < n; ++i) {
        if (pt[i] < 0 || pt[i] > LD_PT_MAX) return "a target mean square outside 0 .. 2^31";
        if (ceil[i] < 1 || ceil[i] > 32767) return "a ceiling outside 1 .. 32767";
    }
    for (int i = 0; i < LD_MAX_STREAMS; ++i) { ld->pt[i] = i < n ? pt[i] : 0; ld->ceil[i] = i < n ? ceil[i] : 0; }
    return nullptr;
}
