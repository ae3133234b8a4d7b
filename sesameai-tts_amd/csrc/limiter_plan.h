// The host side of a pool of look-ahead peak-limiter streams (mimi_lim_pool_*, include/mimi_hip.h states the rule): the per-stream host
// state {R, E, bank, parameters}, the emitted counts, the packed output offsets, the tiles of the grid and the per-call plan that travels in
// the kernel arguments.  Plain C++: no HIP, so it also compiles into a stand-alone host program (tools/limiter_plan_check.cpp, run under
// the host sanitizers); the two small functions that the kernel shares with that program carry LIM_HD.
//
// Positions.  A call's positions are RELATIVE to its first new sample: p = 0 is in[in_off], p < 0 is what the stream had before.  A stream
// that has received R and emitted E samples holds nh = R - E <= L of them (positions -nh .. -1) and the required gains m of its last
// H = K + 2 L positions (-H .. -1; ONE where the clip had not begun).  Output t of the call is position t - nh; its gain reads m from
// K + L behind it to L ahead of it, so the first output reaches back to -nh - K - L >= -H: every halo lies inside the history.
#pragma once
#include <stdint.h>

#include "stream_pool.h"

#ifdef __HIPCC__
#define LIM_HD __host__ __device__
#else
#define LIM_HD
#endif

#define LIM_MAX_STREAMS 64           // = MIMI_LIM_MAX_STREAMS
static_assert(LIM_MAX_STREAMS == SP_MAX_STREAMS, "the pools share one spine");
#define LIM_ONE 65536                // a gain of 1, Q16
#define LIM_L_MAX 480                // look-ahead: 20 ms
#define LIM_RHO_MIN 8                // release step, Q16 per sample: K = ceil(ONE / rho) <= 8192
#define LIM_RHO_MAX 65536
#define LIM_K_MAX 8192
#define LIM_HR_MAX 4                 // drive shift
#define LIM_A_MAX (1 << 30)          // the largest magnitude: (C << 16) / a and a * 1 stay inside 32 bits
#define LIM_HIST_MAX (LIM_K_MAX + 2 * LIM_L_MAX)      // required gains a stream keeps: 9152
#define LIM_BANK (LIM_HIST_MAX + LIM_L_MAX)           // 32-bit words per bank: the gains, then the held samples
#define LIM_TILE 4096                // outputs of one workgroup: 16 KiB of fp32, 8 KiB of int16
#define LIM_THREADS 256
#define LIM_VEC 16                   // bytes moved per lane and access where the buffers allow it
#define LIM_ROW 4                    // = MIMI_LIM_ROW: min gain emitted, samples emitted, samples with g < ONE, samples the clamp changed
#define LIM_LDS_MAX (2 * (LIM_TILE + LIM_HIST_MAX + 1) + LIM_TILE)      // words: two scan buffers and the tile's samples, 122 KiB at most
static_assert((long)LIM_ONE * (LIM_TILE + LIM_HIST_MAX) < (1L << 31), "a tile's sum of gains, and index * rho, must fit 32 bits");
static_assert(LIM_LDS_MAX * 4 <= 160 * 1024, "a workgroup's LDS");

static inline int lim_K(int rho) { return (LIM_ONE + rho - 1) / rho; }

// samples received and emitted since fresh; the bank that holds the carry; fed since its reset; whether reset gave it parameters;
// the format of the held samples (-1: none held since fresh); the parameters
struct LimStream { long R, E; int parity, touched, set, fmt; int C, L, rho, hr; };

// One listed stream of one call, as the kernels get it: 56 bytes.
struct LimSeg {
    long in_off, out_off;            // elements: its new samples in `in`, its outputs in `out`
    int sid;                         // sp_sid_word
    int n_in, n_out;                 // new samples; samples emitted
    int nh;                          // samples held before the call: R - E <= L
    int t_off;                       // its first tile in the grid
    int rho;
    uint16_t C, L, K;
    uint8_t hr, fresh;               // fresh: R == 0, the call reads no carry and starts the state row
    uint8_t mis_in, mis_out;         // elements between the 16-byte line that holds its first sample (output) and that sample (output)
    uint8_t pad[6];
};

struct LimPlan {
    int n, tiles;                    // segments; tiles in all
    int lds_words, pad;              // words of one scan buffer: the call's largest TILE + K + 2 L + 1
    LimSeg seg[LIM_MAX_STREAMS];
};

// nullptr, or why these four are refused
static inline const char* lim_params_bad(int ceiling, int lookahead, int rho, int drive_shift) {
    if (ceiling < 1 || ceiling > 32767) return "a ceiling outside 1 .. 32767";
    if (lookahead < 1 || lookahead > LIM_L_MAX) return "a look-ahead outside 1 .. 480 samples";
    if (rho < LIM_RHO_MIN || rho > LIM_RHO_MAX) return "a release step outside 8 .. 65536 (Q16 per sample)";
    if (drive_shift < 0 || drive_shift > LIM_HR_MAX) return "a drive shift outside 0 .. 4";
    return nullptr;
}

// nullptr, or why the reset is refused (then no state has moved): the listed streams are fresh with these parameters
static inline const char* lim_reset(int n_streams, LimStream* st, const int32_t* streams, const int32_t* ceiling, const int32_t* lookahead,
                                    const int32_t* rho, const int32_t* drive_shift, int n) {
    if (!st || !streams || !ceiling || !lookahead || !rho || !drive_shift) return "null pointer";
    if (const char* bad = sp_ids_bad(n_streams, streams, n)) return bad;
    for (int i = 0; i < n; ++i)
        if (const char* bad = lim_params_bad(ceiling[i], lookahead[i], rho[i], drive_shift[i])) return bad;
    for (int i = 0; i < n; ++i) {                                                      // (the parity stays: a fresh stream reads no carry)
        LimStream& s = st[streams[i]];
        s.R = 0; s.E = 0; s.touched = 0; s.set = 1; s.fmt = -1;
        s.C = ceiling[i]; s.L = lookahead[i]; s.rho = rho[i]; s.hr = drive_shift[i];
    }
    return nullptr;
}

// what a feed of `more` samples would emit for the stream now
static inline long lim_out_count(const LimStream& s, long more, int final) {
    const long R = s.R + more, ready = final ? R : (R > s.L ? R - s.L : 0);
    return ready - s.E;                                                                // (>= 0: E <= max(0, R - L) after every call)
}

static inline long lim_tiles(int mis_out, long n_out) { return n_out ? (mis_out + n_out + LIM_TILE - 1) / LIM_TILE : 0; }

// the outputs [*t_lo, *t_hi) of its segment that tile `tile` of it owns: whole 16-byte lines of `out`, cut at the segment's ends
LIM_HD static inline void lim_tile_range(const LimSeg& g, int tile, int* t_lo, int* t_hi) {
    const int lo = tile * LIM_TILE - g.mis_out, hi = lo + LIM_TILE;
    *t_lo = lo < 0 ? 0 : lo;
    *t_hi = hi < g.n_out ? hi : g.n_out;
}

// the call's positions [*p_lo, *p_hi) whose required gains the tile that owns outputs [t_lo, t_hi) reads
LIM_HD static inline void lim_halo(const LimSeg& g, int t_lo, int t_hi, int* p_lo, int* p_hi) {
    *p_lo = t_lo - g.nh - g.K - g.L;
    *p_hi = t_hi - g.nh + g.L;
}

// Fills `plan`, `n_out` and `next` (the listed streams' states after the call; commit them once the launches are made) from the caller's
// host arrays.  fmt: 0 = fp32, 1 = int16.  Returns nullptr, or what is wrong (plan->n == 0 then: nothing may be launched, no state moved).
static inline const char* lim_plan_build(int n_streams, const LimStream* st, const int32_t* streams, const long* in_off, const long* n_in,
                                         const int32_t* final, int n, const void* in, const void* out, long* n_out, int fmt, LimPlan* plan,
                                         LimStream* next) {
    plan->n = 0; plan->tiles = 0; plan->lds_words = 0; plan->pad = 0;
    if (!st || !streams || !in_off || !n_in || !final || !in || !out || !n_out) return "null pointer";
    if (fmt != 0 && fmt != 1) return "unknown format";
    const int esz = fmt ? 2 : 4, per = LIM_VEC / esz;
    if ((uintptr_t)in % esz || (uintptr_t)out % esz) return "a misaligned buffer";
    if (const char* bad = sp_ids_bad(n_streams, streams, n)) return bad;
    long total = 0, in_lo = -1, in_hi = 0;
    for (int i = 0; i < n; ++i) {
        const LimStream& s = st[streams[i]];
        if (!s.set) return "a stream without parameters: mimi_lim_pool_reset gives them";
        if (const char* bad = sp_chunk_bad(n_in[i], in_off[i], s.R)) return bad;
        if (s.R > s.E && s.fmt != fmt) return "a stream that holds samples of the other format";
        const long give = lim_out_count(s, n_in[i], final[i] != 0);
        if (give > SP_MAX_CHUNK) return "a chunk that gives more than 2^30 samples";
        total += give;
        if (n_in[i]) {
            if (in_lo < 0 || in_off[i] < in_lo) in_lo = in_off[i];
            if (in_off[i] + n_in[i] > in_hi) in_hi = in_off[i] + n_in[i];
        }
    }
    if (total > 0 && in_lo >= 0) {
        const uintptr_t a0 = (uintptr_t)in + (uintptr_t)in_lo * esz, a1 = (uintptr_t)in + (uintptr_t)in_hi * esz;
        const uintptr_t b0 = (uintptr_t)out, b1 = (uintptr_t)out + (uintptr_t)total * esz;
        if (a0 < b1 && b0 < a1) return "in and out overlap";
    }
    long tiles = 0, off = 0;
    int words = 0;
    for (int i = 0; i < n; ++i) {
        const LimStream& s = st[streams[i]];
        LimSeg& g = plan->seg[i];
        const int fin = final[i] != 0;
        const long give = lim_out_count(s, n_in[i], fin);
        g = LimSeg{};
        g.in_off = in_off[i]; g.out_off = off;
        g.sid = sp_sid_word(streams[i], s.parity, fin);
        g.n_in = (int)n_in[i]; g.n_out = (int)give;
        g.nh = (int)(s.R - s.E);
        g.t_off = (int)tiles;
        g.rho = s.rho; g.C = (uint16_t)s.C; g.L = (uint16_t)s.L; g.K = (uint16_t)lim_K(s.rho);
        g.hr = (uint8_t)s.hr; g.fresh = s.R == 0;
        g.mis_in = (uint8_t)(((uintptr_t)in / esz + (uintptr_t)in_off[i]) % per);
        g.mis_out = (uint8_t)(((uintptr_t)out / esz + (uintptr_t)off) % per);
        tiles += lim_tiles(g.mis_out, give);                                           // (<= 64 * (2^30 / 4096 + 1) < 2^25)
        if (give > 0 && LIM_TILE + g.K + 2 * g.L + 1 > words) words = LIM_TILE + g.K + 2 * g.L + 1;
        off += give;
        n_out[i] = give;
        LimStream& t = next[i];
        t = s; t.parity = s.parity ^ 1; t.touched = 1;                 // the call wrote the other bank
        if (fin) { t.R = 0; t.E = 0; t.fmt = -1; }                    // the next sample starts a new clip
        else { t.R = s.R + n_in[i]; t.E = s.E + give; t.fmt = fmt; }
    }
    sp_zero_tail(plan->seg, n);
    plan->n = n; plan->tiles = (int)tiles; plan->lds_words = words;
    return nullptr;
}

// nullptr, or why a state read of the listed streams into `out` is refused
static inline const char* lim_state_bad(int n_streams, const int32_t* streams, int n, const void* out) {
    if (!streams || !out) return "null pointer";
    if ((uintptr_t)out % 8) return "a misaligned buffer";
    return sp_ids_bad(n_streams, streams, n);
}
