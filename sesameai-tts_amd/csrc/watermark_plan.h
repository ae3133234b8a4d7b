// The host side of a keyed pool of watermark streams (mimi_wm_pool_*, include/mimi_hip.h states the rule): the per-stream host state
// {samples taken, samples given out, t_q4, the 56 symbol bits, the format, the live carry bank}, the refusals, the output counts, and the
// two per-call plans that travel in the kernel arguments -- embed (one segment per listed stream) and detect (one per clip).
// Plain C++: no HIP, so it also compiles into a stand-alone host program (tools/wm_plan_check.cpp, run under the host sanitizers).
//
// Positions.  A block is S samples and a period is K blocks, so a block never straddles a symbol or the period: the stream's block J carries
// symbol J % K with the chips [J % K * S, J % K * S + S).  A stream keeps the R % S samples of its open block (the carry: fewer than S raw
// 32-bit words, fp32 bits or a sign-extended int16) and the kernels see only {carry length, new samples, symbol of the first block}: all
// below 2^31 however long the stream runs.  The totals stay here.
#pragma once
#include <stdint.h>

#include "stream_pool.h"

#define WM_MAX_STREAMS 64            // = MIMI_WM_MAX_STREAMS
static_assert(WM_MAX_STREAMS == SP_MAX_STREAMS, "the pools share one spine");
#define WM_MAX_CLIPS 64              // = MIMI_WM_MAX_CLIPS
#define WM_S 1920                    // samples per symbol: one Mimi frame
#define WM_K 56                      // symbols per period
#define WM_P (WM_S * WM_K)           // 107,520
#define WM_ROW 64                    // int64 per detected clip (= MIMI_WM_ROW)
#define WM_TILE 256                  // candidates per search workgroup
#define WM_SYNC 0xB2
#define WM_MAX_CLIP (1L << 24)       // samples of one detected clip
#define WM_MAX_OFFSETS (1L << 21)    // candidates of one detect call, all clips together
#define WM_ALL ((1ULL << WM_K) - 1)
// |r_i| <= 1920 * 32768 < 2^26: a block's correlation fits a signed 32-bit accumulator in any order; at most 2^24 / 1920 < 2^14 blocks of a
// clip fold into one R_k, |R_k| < 2^40.   E <= 1920 * 2^30 < 2^41, isqrt(E) < 2^21, T <= isqrt(E) * 64 >> 4 < 2^23, |D| <= T + |r| < 2^27,
// |d| <= |D| / 1920 + 1 < 2^17: exact as a float.

constexpr uint8_t wm_crc8(const uint8_t* d, int n) {                                  // (constexpr: host and device both call it)
    uint8_t c = 0;
    for (int i = 0; i < n; ++i) {
        c ^= d[i];
        for (int j = 0; j < 8; ++j) c = (uint8_t)(c & 0x80 ? (c << 1) ^ 0x07 : c << 1);
    }
    return c;
}

// the 56 symbols as one word: bit k (LSB = symbol 0) is 1 where b_k = +1; sync, the five bytes, their CRC-8, each MSB first
static inline uint64_t wm_symbol_bits(const uint8_t* payload) {
    uint8_t bytes[7] = {WM_SYNC, payload[0], payload[1], payload[2], payload[3], payload[4], wm_crc8(payload, 5)};
    uint64_t w = 0;
    for (int j = 0; j < 7; ++j)
        for (int i = 0; i < 8; ++i) w |= (uint64_t)((bytes[j] >> (7 - i)) & 1) << (8 * j + i);
    return w;
}

// One listed stream of one feed, as the kernel gets it: 56 bytes.
struct WmSeg {
    long in_off, out_off;            // elements: its new samples in `in`, its place in the packed `out`
    uint64_t bits;                   // the 56 symbol bits
    int sid;                         // sp_sid_word
    int Lc, n_in;                    // carry samples (< S); new samples
    int nb, g_off;                   // complete blocks; its first workgroup (a stream owns nb + 1: its blocks, then its tail)
    int k0;                          // symbol of its first block
    int t_q4;
    int pad;
};

struct WmPlan {
    int n, groups;                   // segments; workgroups in all
    WmSeg seg[WM_MAX_STREAMS];
};

struct WmStream { long R, given; uint64_t bits; int t_q4, fmt, parity; };       // fmt: -1 not fed since fresh, 0 fp32, 1 int16

static inline long wm_carry_len(long R) { return R % WM_S; }
static inline long wm_out_len(const WmStream& s, long more, int final) {
    const long have = wm_carry_len(s.R) + more;
    return final ? have : have / WM_S * WM_S;
}

static inline void wm_fresh(WmStream& s) { s.R = 0; s.given = 0; s.fmt = -1; }

// nullptr, or why the reset is refused (then no state has moved).  payloads: 5 bytes per listed stream.
static inline const char* wm_reset(int n_streams, WmStream* st, const int32_t* streams, const uint8_t* payloads, const int32_t* t_q4, int n) {
    if (!st || !streams || !payloads || !t_q4) return "null pointer";
    if (const char* bad = sp_ids_bad(n_streams, streams, n)) return bad;
    for (int i = 0; i < n; ++i)
        if (t_q4[i] < 1 || t_q4[i] > 64) return "t_q4 outside 1 .. 64";
    for (int i = 0; i < n; ++i) {                                                      // (the parity stays: a fresh stream reads no carry)
        WmStream& s = st[streams[i]];
        wm_fresh(s);
        s.t_q4 = t_q4[i]; s.bits = wm_symbol_bits(payloads + 5 * i);
    }
    return nullptr;
}

// Fills `plan` and `next` (the listed streams' states after the call; commit them once the launch is made) from the caller's host arrays.
// Returns nullptr, or what is wrong (plan->n == 0 then: nothing may be launched, no state may move).
static inline const char* wm_plan_build(int n_streams, const WmStream* st, const int32_t* streams, const long* in_off, const long* n_in,
                                        const int32_t* final, int n, const void* in, int in_is_i16, const void* out, long* n_out,
                                        WmPlan* plan, WmStream* next) {
    plan->n = 0; plan->groups = 0;
    if (!st || !streams || !in_off || !n_in || !final || !in || !out || !n_out) return "null pointer";
    if (in_is_i16 != 0 && in_is_i16 != 1) return "unknown sample format";
    if ((uintptr_t)in % (in_is_i16 ? 2 : 4) || (uintptr_t)out % (in_is_i16 ? 2 : 4)) return "a misaligned buffer";
    if (const char* bad = sp_ids_bad(n_streams, streams, n)) return bad;
    long groups = 0;
    for (int i = 0; i < n; ++i) {
        const WmStream& s = st[streams[i]];
        if (s.t_q4 < 1 || s.t_q4 > 64) return "t_q4 outside 1 .. 64";
        if (const char* bad = sp_chunk_bad(n_in[i], in_off[i], s.R)) return bad;
        if (s.fmt >= 0 && s.fmt != in_is_i16) return "a stream that changes its sample format between resets";
        groups += (wm_carry_len(s.R) + n_in[i]) / WM_S + 1;
    }
    if (groups > (1L << 30)) return "a call of more than 2^30 blocks";
    int g_off = 0;
    long out_off = 0;
    for (int i = 0; i < n; ++i) {
        const WmStream& s = st[streams[i]];
        WmSeg& g = plan->seg[i];
        const int fin = final[i] != 0;
        const long Lc = wm_carry_len(s.R), nb = (Lc + n_in[i]) / WM_S;
        g.in_off = in_off[i]; g.out_off = out_off; g.bits = s.bits;
        g.sid = sp_sid_word(streams[i], s.parity, fin);
        g.Lc = (int)Lc; g.n_in = (int)n_in[i];
        g.nb = (int)nb; g.g_off = g_off;
        g.k0 = (int)(s.R / WM_S % WM_K);
        g.t_q4 = s.t_q4; g.pad = 0;
        g_off += (int)nb + 1;
        n_out[i] = wm_out_len(s, n_in[i], fin);
        out_off += n_out[i];
        WmStream& t = next[i];
        t = s; t.parity = s.parity ^ 1;                                 // the call wrote the other bank
        if (fin) wm_fresh(t);                                           // the next sample starts a new clip (same payload and t_q4)
        else { t.R = s.R + n_in[i]; t.given = s.given + n_out[i]; t.fmt = in_is_i16; }
    }
    sp_zero_tail(plan->seg, n);
    plan->n = n; plan->groups = g_off;
    return nullptr;
}

// One clip of one detect call, as the kernels get it: 48 bytes.
struct WmClip {
    long in_off;                     // elements
    uint64_t expect, mask;           // K-bit words, bit k = symbol k
    int n_in;                        // samples (<= 2^24)
    int o0, n_off;                   // first candidate (already mod P); candidates
    int s_off, t_off;                // its place in the packed scores; its first search workgroup
    int pad;
};

struct WmDetectPlan {
    int n, tiles;                    // clips; search workgroups in all
    WmClip clip[WM_MAX_CLIPS];
};

static inline const char* wm_detect_plan(const long* in_off, const long* n_in, const long* o0, const long* n_off, const uint64_t* expect,
                                         const uint64_t* mask, int n, const void* in, int in_is_i16, const void* scores, const void* out,
                                         WmDetectPlan* plan) {
    plan->n = 0; plan->tiles = 0;
    if (!in_off || !n_in || !o0 || !n_off || !expect || !mask || !in || !scores || !out) return "null pointer";
    if (in_is_i16 != 0 && in_is_i16 != 1) return "unknown sample format";
    if ((uintptr_t)in % (in_is_i16 ? 2 : 4) || (uintptr_t)scores % 4 || (uintptr_t)out % 8) return "a misaligned buffer";
    if (n < 1 || n > WM_MAX_CLIPS) return "clip list: need 1 .. 64 clips";
    long total = 0;
    for (int i = 0; i < n; ++i) {
        if (n_in[i] < 0) return "a clip of negative length";
        if (in_off[i] < 0) return "a clip at a negative offset";
        if (n_in[i] > WM_MAX_CLIP) return "a clip of more than 2^24 samples";
        if (o0[i] < 0) return "a negative first offset";
        if (n_off[i] < 1 || n_off[i] > WM_MAX_OFFSETS) return "n_off outside 1 .. 2^21";
        if ((expect[i] | mask[i]) & ~WM_ALL) return "expect / mask: bits beyond the 56 symbols";
        total += n_off[i];
    }
    if (total > WM_MAX_OFFSETS) return "more than 2^21 candidate offsets in one call";
    int s_off = 0, t_off = 0;
    for (int i = 0; i < n; ++i) {
        WmClip& c = plan->clip[i];
        c.in_off = in_off[i]; c.expect = expect[i]; c.mask = mask[i];
        c.n_in = (int)n_in[i]; c.o0 = (int)(o0[i] % WM_P); c.n_off = (int)n_off[i];
        c.s_off = s_off; c.t_off = t_off; c.pad = 0;
        s_off += (int)n_off[i];
        t_off += (int)((n_off[i] + WM_TILE - 1) / WM_TILE);
    }
    sp_zero_tail(plan->clip, n);
    plan->n = n; plan->tiles = t_off;
    return nullptr;
}
