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

struct LdStream { long R, k; int parity, touched; int mode, pad; };   // samples taken and hops measured since fresh; the bank that holds the carry; fed since its reset; LD_METER or LD_LEVEL
#define LD_METER 0                   // the stream meters: mimi_ld_pool_feed takes it
#define LD_LEVEL 1                   // the stream levels: mimi_ld_pool_level_feed takes it

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
        s.R = 0; s.k = 0; s.touched = 0; s.mode = LD_METER;
    }
    return nullptr;
}

// Fills `plan` and `next` (the listed streams' states after the call; commit them once the launches are made) from the caller's host
// arrays.  Returns nullptr, or what is wrong (plan->n == 0 then: nothing may be launched, no state may move).
// (ld_plan_in: the body of both feeds' plans -- `mode` is the one the call takes, `extra` what the leveler's feed has against its own buffers)
static inline const char* ld_plan_in(int mode, const char* extra, int n_streams, const LdStream* st, const int32_t* streams,
                                     const long* in_off, const long* n_in, const int32_t* final, int n, const void* in, int in_is_i16,
                                     const void* energy, long* n_hops, LdPlan* plan, LdStream* next) {
    plan->n = 0; plan->hops = 0;
    if (!st || !streams || !in_off || !n_in || !final || !in || !energy || !n_hops) return "null pointer";
    if (in_is_i16 != 0 && in_is_i16 != 1) return "unknown input format";
    if ((uintptr_t)in % (in_is_i16 ? 2 : 4) || (uintptr_t)energy % 8) return "a misaligned buffer";
    if (extra) return extra;
    if (const char* bad = sp_ids_bad(n_streams, streams, n)) return bad;
    long total = 0;
    for (int i = 0; i < n; ++i) {
        const LdStream& s = st[streams[i]];
        if (s.mode != mode) return mode == LD_METER ? "a stream in leveler mode: mimi_ld_pool_level_feed takes it" : "a metering stream: mimi_ld_pool_feed takes it";
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

static inline const char* ld_plan_build(int n_streams, const LdStream* st, const int32_t* streams, const long* in_off, const long* n_in,
                                        const int32_t* final, int n, const void* in, int in_is_i16, const void* energy, long* n_hops,
                                        LdPlan* plan, LdStream* next) {
    return ld_plan_in(LD_METER, nullptr, n_streams, st, streams, in_off, n_in, final, n, in, in_is_i16, energy, n_hops, plan, next);
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

// ---- The leveler (mimi_ld_pool_level_*, include/mimi_hip.h states the rule): a stream in LD_LEVEL mode carries five parameters, set by
// mimi_ld_pool_level_reset on the host; a feed hands them to the scan in the kernel arguments beside the meter's plan, and a second small
// plan tells k_ld_apply which tile of samples belongs to which stream.
#define LD_GAIN_MAX (1 << 22)        // gmax, Q16: 64 x.  s * gi < 2^37, A * H < 2^34: 64-bit arithmetic, float(gi) exact
#define LD_SLEW_MAX 16
#define LD_LEVEL_ROW 4               // = MIMI_LD_LEVEL_ROW: the gain the open hop ends on, hops, clipped, P
#define LD_AP_VEC 16                 // bytes k_ld_apply moves per lane and access where the buffers allow it
#define LD_AP_THREADS 256
#define LD_AP_PER 4                  // 16-byte vectors per thread and tile
#define LD_AP_TILE (LD_AP_THREADS * LD_AP_PER * LD_AP_VEC)      // bytes of one tile: 16 KiB

struct LdLevel { uint32_t pt, g0, gmax; uint16_t ceil; uint8_t sh, pad; };      // P_T (2^31 fits), g0 and gmax in Q16, C, the slew shift: 16 bytes
struct LdLevelPlan { LdLevel lv[LD_MAX_STREAMS]; };                             // seg i's parameters, as the scan gets them

// One listed stream of one call, as k_ld_apply gets it: 32 bytes.
struct LdApSeg {
    long in_off;                     // elements: its samples in `in`, and in `out`
    int n_in;                        // samples
    int t_off;                       // its first tile in the grid
    int i0;                          // R % H: where in its open hop the call's first sample falls
    int g_off;                       // its first boundary gain in `gain`: A[k0]
    int mis;                         // elements between the 16-byte line that holds its first sample and that sample
    uint16_t ceil; uint8_t sid, pad;
};
struct LdApPlan { int n, tiles, vec, pad; LdApSeg seg[LD_MAX_STREAMS]; };         // vec: `in` and `out` agree modulo 16 bytes

// nullptr, or why these five are refused
static inline const char* ld_level_bad(long pt, int ceiling, int g0, int gmax, int sh) {
    if (pt < 1 || pt > LD_PT_MAX) return "a target mean square outside 1 .. 2^31";
    if (ceiling < 1 || ceiling > 32767) return "a ceiling outside 1 .. 32767";
    if (gmax < 1 || gmax > LD_GAIN_MAX) return "a largest gain outside 1 .. 2^22 (Q16)";
    if (g0 < 1 || g0 > gmax) return "a start gain outside 1 .. the largest gain";
    if (sh < 1 || sh > LD_SLEW_MAX) return "a slew shift outside 1 .. 16";
    return nullptr;
}

// nullptr, or why the reset is refused (then no state has moved): the listed streams are fresh, in leveler mode, with these parameters
static inline const char* ld_level_reset(int n_streams, LdStream* st, LdLevel* lv, const int32_t* streams, const long* pt, const int32_t* ceiling,
                                         const int32_t* g0, const int32_t* gmax, const int32_t* sh, int n) {
    if (!st || !lv || !streams || !pt || !ceiling || !g0 || !gmax || !sh) return "null pointer";
    if (const char* bad = sp_ids_bad(n_streams, streams, n)) return bad;
    for (int i = 0; i < n; ++i)
        if (const char* bad = ld_level_bad(pt[i], ceiling[i], g0[i], gmax[i], sh[i])) return bad;
    for (int i = 0; i < n; ++i) {
        LdStream& s = st[streams[i]];
        s.R = 0; s.k = 0; s.touched = 0; s.mode = LD_LEVEL;
        lv[streams[i]] = LdLevel{(uint32_t)pt[i], (uint32_t)g0[i], (uint32_t)gmax[i], (uint16_t)ceiling[i], (uint8_t)sh[i], 0};
    }
    return nullptr;
}

// The leveler's feed: the meter's plan for leveler streams, their parameters, and the tiles of k_ld_apply.  Stream i owns n_hops[i] + 2
// values of `gain` from g_off = (n_hops[0] + 2) + .. + (n_hops[i-1] + 2) on.  nullptr, or what is wrong (plan->n == 0 then).
static inline const char* ld_level_plan_build(int n_streams, const LdStream* st, const LdLevel* lv, const int32_t* streams, const long* in_off,
                                              const long* n_in, const int32_t* final, int n, const void* in, int in_is_i16, const void* out,
                                              const void* energy, const void* gain, long* n_hops, LdPlan* plan, LdLevelPlan* lp, LdApPlan* ap,
                                              LdStream* next) {
    const int esz = in_is_i16 == 1 ? 2 : 4;
    const char* extra = !lv || !out || !gain || !lp || !ap ? "null pointer" : (uintptr_t)out % esz || (uintptr_t)gain % 4 ? "a misaligned buffer" : nullptr;
    if (ap) { ap->n = 0; ap->tiles = 0; }
    if (const char* bad = ld_plan_in(LD_LEVEL, extra, n_streams, st, streams, in_off, n_in, final, n, in, in_is_i16, energy, n_hops, plan, next))
        return bad;
    const int per = LD_AP_VEC / esz, tile = LD_AP_TILE / esz;                          // elements of a vector, of a tile
    ap->vec = ((uintptr_t)in - (uintptr_t)out) % LD_AP_VEC == 0;
    ap->pad = 0;
    long tiles = 0;
    for (int i = 0; i < n; ++i) {
        const LdStream& s = st[streams[i]];
        lp->lv[i] = lv[streams[i]];
        LdApSeg& a = ap->seg[i];
        a.in_off = in_off[i]; a.n_in = (int)n_in[i];
        a.t_off = (int)tiles;
        a.i0 = (int)(s.R % LD_H);
        a.g_off = plan->seg[i].f_off + 2 * i;
        a.mis = (int)(((uintptr_t)in / esz + (uintptr_t)in_off[i]) % per);
        a.ceil = lv[streams[i]].ceil; a.sid = (uint8_t)streams[i]; a.pad = 0;
        tiles += n_in[i] ? (a.mis + n_in[i] + tile - 1) / tile : 0;                    // (<= 64 * (2^30 / 4096 + 1) < 2^25)
    }
    for (int i = n; i < LD_MAX_STREAMS; ++i) lp->lv[i] = LdLevel{};
    sp_zero_tail(ap->seg, n);
    ap->n = n; ap->tiles = (int)tiles;
    return nullptr;
}

// nullptr, or why a state read of the listed streams into `out` is refused
static inline const char* ld_level_state_bad(int n_streams, const LdStream* st, const int32_t* streams, int n, const void* out) {
    if (!st || !streams || !out) return "null pointer";
    if ((uintptr_t)out % 8) return "a misaligned buffer";
    if (const char* bad = sp_ids_bad(n_streams, streams, n)) return bad;
    for (int i = 0; i < n; ++i)
        if (st[streams[i]].mode != LD_LEVEL) return "a metering stream: it has no leveler state";
    return nullptr;
}
