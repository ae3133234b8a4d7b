// The host side of a pool of look-ahead peak-limiter streams (mimi_lim_pool_*, include/mimi_hip.h states the rule): the per-stream host
// state {R, E, bank, parameters}, the emitted counts, the packed output offsets, the tiles of the grid and the per-call plan that travels in
// the kernel arguments.  Plain C++: no HIP, so it also compiles into a stand-alone host program (tools/limiter_plan_check.cpp, run under
// the host sanitizers); the two small functions that the kernel shares with that program carry LIM_HD.
//
// Positions.  A call's positions are RELATIVE to its first new sample: p = 0 is in[in_off], p < 0 is what the stream had before.  A stream
// that has received R and emitted E samples holds nh = R - E <= L of them (positions -nh .. -1) and the required gains m of its last
// H = K + 2 L positions (-H .. -1; ONE where the clip had not begun).  Output t of the call is position t - nh; its gain reads m from
// K + L behind it to L ahead of it, so the first output reaches back to -nh - K - L >= -H: every halo lies inside the history.
//
// True-peak streams (mimi_lim_pool_reset_tp; tests/truepeak_ref.py states the rule).  The required gain of a position reads the signed
// samples T = TP_T on either side of it, so it is known T samples late: such a stream holds nh <= L + T samples, its history is the
// required gains of the positions -T - H .. -T, and beside them it keeps the signed samples v of its last 2 T positions, from which the
// next call computes the gains of -T .. on.  The first output still reaches back to -nh - K - L >= -T - H.  True-peak streams have banks
// of their own (LIM_TP_BANK words, behind the sample-peak banks of the same allocation) and plans of their own: a call that lists streams
// of both modes makes one plan, and one pair of launches, per mode, with the outputs of all packed in list order.
#pragma once
#include <stdint.h>

#include "stream_pool.h"
#include "truepeak_taps.h"

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
#define LIM_TP_HELD_MAX (LIM_L_MAX + TP_T)             // samples a true-peak stream holds
#define LIM_TP_BANK (LIM_HIST_MAX + LIM_TP_HELD_MAX + 2 * TP_T)      // the gains, the held samples, the signed samples of the last 2 T positions
#define LIM_TP_LDS_MAX (LIM_LDS_MAX + 4 * TP_T)        // words: each scan buffer 2 T longer, the second one stages the signed samples first
static_assert(LIM_TP_LDS_MAX * 4 <= 160 * 1024, "a workgroup's LDS");
static_assert((long)TP_TAPS_ABS_SUM << 15 < (1L << 30) && (((long)TP_TAPS_ABS_SUM << 30) + (1L << 13)) >> 14 < (1L << 31),
              "the narrow accumulator; a true-peak magnitude fits 31 bits");
static_assert((long)LIM_ONE * (LIM_TILE + LIM_HIST_MAX) < (1L << 31), "a tile's sum of gains, and index * rho, must fit 32 bits");
static_assert(LIM_LDS_MAX * 4 <= 160 * 1024, "a workgroup's LDS");

static inline int lim_K(int rho) { return (LIM_ONE + rho - 1) / rho; }

// samples received and emitted since fresh; the bank that holds the carry; fed since its reset; whether reset gave it parameters;
// the format of the held samples (-1: none held since fresh); the parameters; whether it detects true peaks
struct LimStream { long R, E; int parity, touched, set, fmt; int C, L, rho, hr; int tp; };

// One listed stream of one call, as the kernels get it: 56 bytes.
struct LimSeg {
    long in_off, out_off;            // elements: its new samples in `in`, its outputs in `out`
    int sid;                         // sp_sid_word
    int n_in, n_out;                 // new samples; samples emitted
    int nh;                          // samples held before the call: R - E <= L (a true-peak stream: <= L + T)
    int t_off;                       // its first tile in the grid
    int rho;
    uint16_t C, L, K;
    uint8_t hr, fresh;               // fresh: R == 0, the call reads no carry and starts the state row
    uint8_t mis_in, mis_out;         // elements between the 16-byte line that holds its first sample (output) and that sample (output)
    uint8_t tp;                      // a true-peak stream
    uint8_t pre;                     // true peak: min(R, 2 T), the positions in front of the call that lie inside the clip (0 otherwise)
    uint8_t pad[4];
};

struct LimPlan {
    int n, tiles;                    // segments; tiles in all
    int lds_words, pad;              // words of one scan buffer: the call's largest TILE + K + 2 L + 1 (true peak: + 2 T)
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
// true_peak: nullptr (no stream detects true peaks), or 0 / 1 per listed stream
static inline const char* lim_reset_tp(int n_streams, LimStream* st, const int32_t* streams, const int32_t* ceiling, const int32_t* lookahead,
                                       const int32_t* rho, const int32_t* drive_shift, const int32_t* true_peak, int n) {
    if (!st || !streams || !ceiling || !lookahead || !rho || !drive_shift) return "null pointer";
    if (const char* bad = sp_ids_bad(n_streams, streams, n)) return bad;
    for (int i = 0; i < n; ++i) {
        if (const char* bad = lim_params_bad(ceiling[i], lookahead[i], rho[i], drive_shift[i])) return bad;
        if (true_peak && true_peak[i] != 0 && true_peak[i] != 1) return "a true-peak flag that is neither 0 nor 1";
    }
    for (int i = 0; i < n; ++i) {                                                      // (the parity stays: a fresh stream reads no carry)
        LimStream& s = st[streams[i]];
        s.R = 0; s.E = 0; s.touched = 0; s.set = 1; s.fmt = -1;
        s.C = ceiling[i]; s.L = lookahead[i]; s.rho = rho[i]; s.hr = drive_shift[i];
        s.tp = true_peak ? true_peak[i] : 0;
    }
    return nullptr;
}

static inline const char* lim_reset(int n_streams, LimStream* st, const int32_t* streams, const int32_t* ceiling, const int32_t* lookahead,
                                    const int32_t* rho, const int32_t* drive_shift, int n) {
    return lim_reset_tp(n_streams, st, streams, ceiling, lookahead, rho, drive_shift, nullptr, n);
}

// a stream's latency: the samples it holds back until more arrive
static inline int lim_delay(const LimStream& s) { return s.L + (s.tp ? TP_T : 0); }

// what a feed of `more` samples would emit for the stream now
static inline long lim_out_count(const LimStream& s, long more, int final) {
    const long R = s.R + more, D = lim_delay(s), ready = final ? R : (R > D ? R - D : 0);
    return ready - s.E;                                                                // (>= 0: E <= max(0, R - D) after every call)
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

// True peak.  The required gains of [p_lo, p_hi) come from three places: the history (positions below -T), silence (in front of the clip
// and behind what the stream has received) and, for [*c_lo, *c_hi), the signed samples [*c_lo - T, *c_hi + T) -- the last 2 T of them
// before the call from the bank, zero in front of the clip and behind the call's last sample.
LIM_HD static inline void lim_tp_computed(const LimSeg& g, int p_lo, int p_hi, int* c_lo, int* c_hi) {
    const int first = -(g.pre < TP_T ? (int)g.pre : TP_T);
    *c_lo = p_lo > first ? p_lo : first;
    *c_hi = p_hi < g.n_in ? p_hi : g.n_in;
    if (*c_hi < *c_lo) *c_hi = *c_lo;
}

// True peak, the carry: the positions [*c_lo, *c_hi) among n_in - T - H .. n_in - T whose required gains the call makes final, from the
// signed samples [*c_lo - T, *c_hi + T) = [.., n_in): at most H + 2 T of them.
LIM_HD static inline void lim_tp_carried(const LimSeg& g, int* c_lo, int* c_hi) {
    const int H = g.K + 2 * g.L, first = -(g.pre < TP_T ? (int)g.pre : TP_T), back = g.n_in - TP_T - H;
    *c_lo = back > first ? back : first;
    *c_hi = g.n_in - TP_T;
    if (*c_hi < *c_lo) *c_hi = *c_lo;
}

// Fills `plans` (0: the sample-peak streams of the list, 1: its true-peak streams; each in list order), `n_out` and `next` (the listed
// streams' states after the call; commit them once the launches are made) from the caller's host arrays.  fmt: 0 = fp32, 1 = int16.  Returns nullptr, or what is wrong (both plans have n == 0 then: nothing may be launched, no state moved).
static inline const char* lim_plan_build_tp(int n_streams, const LimStream* st, const int32_t* streams, const long* in_off, const long* n_in,
                                            const int32_t* final, int n, const void* in, const void* out, long* n_out, int fmt,
                                            LimPlan* plans, LimStream* next) {
    for (int m = 0; m < 2; ++m) { plans[m].n = 0; plans[m].tiles = 0; plans[m].lds_words = 0; plans[m].pad = 0; }
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
    long tiles[2] = {0, 0}, off = 0;
    int words[2] = {0, 0}, count[2] = {0, 0};
    for (int i = 0; i < n; ++i) {
        const LimStream& s = st[streams[i]];
        const int tp = s.tp != 0;
        LimSeg& g = plans[tp].seg[count[tp]++];
        const int fin = final[i] != 0;
        const long give = lim_out_count(s, n_in[i], fin);
        g = LimSeg{};
        g.in_off = in_off[i]; g.out_off = off;
        g.sid = sp_sid_word(streams[i], s.parity, fin);
        g.n_in = (int)n_in[i]; g.n_out = (int)give;
        g.nh = (int)(s.R - s.E);
        g.t_off = (int)tiles[tp];
        g.rho = s.rho; g.C = (uint16_t)s.C; g.L = (uint16_t)s.L; g.K = (uint16_t)lim_K(s.rho);
        g.hr = (uint8_t)s.hr; g.fresh = s.R == 0;
        g.mis_in = (uint8_t)(((uintptr_t)in / esz + (uintptr_t)in_off[i]) % per);
        g.mis_out = (uint8_t)(((uintptr_t)out / esz + (uintptr_t)off) % per);
        g.tp = (uint8_t)tp;
        g.pre = (uint8_t)(tp ? (s.R < 2 * TP_T ? s.R : 2 * TP_T) : 0);
        tiles[tp] += lim_tiles(g.mis_out, give);                                       // (<= 64 * (2^30 / 4096 + 1) < 2^25)
        const int w = LIM_TILE + g.K + 2 * g.L + 1 + (tp ? 2 * TP_T : 0);
        if (give > 0 && w > words[tp]) words[tp] = w;
        off += give;
        n_out[i] = give;
        LimStream& t = next[i];
        t = s; t.parity = s.parity ^ 1; t.touched = 1;                 // the call wrote the other bank
        if (fin) { t.R = 0; t.E = 0; t.fmt = -1; }                    // the next sample starts a new clip
        else { t.R = s.R + n_in[i]; t.E = s.E + give; t.fmt = fmt; }
    }
    for (int m = 0; m < 2; ++m) {
        sp_zero_tail(plans[m].seg, count[m]);
        plans[m].n = count[m]; plans[m].tiles = (int)tiles[m]; plans[m].lds_words = words[m];
    }
    return nullptr;
}

// the same for a call whose streams all detect sample peaks: one plan
static inline const char* lim_plan_build(int n_streams, const LimStream* st, const int32_t* streams, const long* in_off, const long* n_in,
                                         const int32_t* final, int n, const void* in, const void* out, long* n_out, int fmt, LimPlan* plan,
                                         LimStream* next) {
    LimPlan both[2];
    const char* bad = lim_plan_build_tp(n_streams, st, streams, in_off, n_in, final, n, in, out, n_out, fmt, both, next);
    if (!bad && both[1].n) { both[0].n = 0; both[0].tiles = 0; both[0].lds_words = 0; bad = "a true-peak stream: lim_plan_build_tp plans it"; }
    *plan = both[0];
    return bad;
}

// nullptr, or why a state read of the listed streams into `out` is refused
static inline const char* lim_state_bad(int n_streams, const int32_t* streams, int n, const void* out) {
    if (!streams || !out) return "null pointer";
    if ((uintptr_t)out % 8) return "a misaligned buffer";
    return sp_ids_bad(n_streams, streams, n);
}

// ---- the stateless true-peak meter (mimi_tp_measure): up to 64 clips, one workgroup per (clip, tile of LIM_TILE positions) ----
#define TP_MAX_CLIPS 64              // = MIMI_TP_MAX_CLIPS
#define TP_ROW 4                     // = MIMI_TP_ROW: sample peak, true peak, the first position that has it, the clip's length

struct TpSeg { long in_off; int n, t_off; };      // elements: the clip in `in`; its length; its first tile in the grid (an empty clip has none)
struct TpPlan { int n, tiles; TpSeg seg[TP_MAX_CLIPS]; };

// Fills `plan` from the caller's host arrays.  fmt: 0 = fp32, 1 = int16.  Returns nullptr, or what is wrong (plan->n == 0 then: nothing
// may be launched, no row written).
static inline const char* tp_plan_build(const void* in, const long* in_off, const long* n_in, int n, int fmt, const void* out, TpPlan* plan) {
    plan->n = 0; plan->tiles = 0;
    if (!in || !in_off || !n_in || !out) return "null pointer";
    if (fmt != 0 && fmt != 1) return "unknown format";
    if ((uintptr_t)in % (fmt ? 2 : 4) || (uintptr_t)out % 8) return "a misaligned buffer";
    if (n < 1 || n > TP_MAX_CLIPS) return "clip list: need 1 .. 64 clips";
    for (int i = 0; i < n; ++i)
        if (const char* bad = sp_chunk_bad(n_in[i], in_off[i], 0)) return bad;
    long tiles = 0;
    for (int i = 0; i < TP_MAX_CLIPS; ++i) {
        TpSeg& g = plan->seg[i];
        g = TpSeg{};
        if (i >= n) continue;
        g.in_off = in_off[i]; g.n = (int)n_in[i]; g.t_off = (int)tiles;
        tiles += (n_in[i] + LIM_TILE - 1) / LIM_TILE;                                  // (<= 64 * 2^18)
    }
    plan->n = n; plan->tiles = (int)tiles;
    return nullptr;
}
