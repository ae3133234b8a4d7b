// The host side of a pool of stateful voice-activity streams (mimi_vad_pool_*, include/mimi_hip.h states the rule): the per-stream host state
// {parameters, R, k, bank}, the frame counts, the packed frame offsets and the per-call plan that travels in the kernel arguments.
// Plain C++: no HIP, so it also compiles into a stand-alone host program (tools/vad_plan_check.cpp, run under the host sanitizers).
//
// Positions.  Frame k reads samples from (k + 1) F - W - TMAX = k F - 640 on, so a stream whose next unjudged frame is k keeps its samples
// from base(k) = k F - 640 on: 640 + R % F <= 879 of them (R: samples taken since the stream was fresh), fewer while base(k) < 0, where the
// positions in front of the clip are zero by rule and are not kept.  Everything the kernels see is RELATIVE to base(k0) of the call's first
// frame: `lead` rule zeros, then the carry, then the new chunk; frame k0 + i reads positions [i F, i F + 880).  The totals stay here; k0 goes
// along as 64 bits only to stamp events.
#pragma once
#include <stdint.h>

#include "stream_pool.h"

#define VAD_MAX_STREAMS 64           // = MIMI_VAD_MAX_STREAMS
static_assert(VAD_MAX_STREAMS == SP_MAX_STREAMS, "the pools share one spine");
#define VAD_F 240                    // frame
#define VAD_W 480                    // analysis window
#define VAD_TMIN 60
#define VAD_TMAX 400
#define VAD_SPAN (VAD_W + VAD_TMAX)  // samples one frame's features read: 880
#define VAD_HIST (VAD_SPAN - VAD_F)  // samples in front of its next frame that a stream keeps: 640
#define VAD_CARRY VAD_SPAN           // int16 values per bank (the most a stream keeps is 879)
#define VAD_SAT (1 << 20)            // since_voiced saturates here
#define VAD_SUMMARY 8                // int64 per stream: in speech, frames, last START, last END, quiet, STARTs, ENDs, 0

struct VadParams { int32_t on_q4, off_q4, min_on, hang, hold, pad; int64_t n_min; };      // = mimi_vad_params
#define VAD_DEFAULT_PARAMS VadParams{128, 48, 8, 70, 30, 0, 3686400}

// One listed stream of one call, as the kernels get it: 56 bytes.
struct VadSeg {
    long in_off;                     // elements: its new samples in `in`
    long n_min;
    long k0;                         // frames judged since the stream was fresh (k0 == 0: the scan starts from the fresh state)
    int sid;                         // sp_sid_word
    int Lc, n_in;                    // carry samples; new samples
    int nf, f_off;                   // frames judged in this call; their place in the per-frame outputs
    int onoff;                       // on_q4 | off_q4 << 12
    int mh;                          // min_on | hang << 10
    int hold;
};
#define VAD_LEAD(g) ((g).k0 < 3 ? VAD_HIST - (int)(g).k0 * VAD_F : 0)      // rule zeros in front of the carry
#define VAD_ON(g) ((g).onoff & 0xFFF)
#define VAD_OFF(g) ((g).onoff >> 12)
#define VAD_MIN_ON(g) ((g).mh & 0x3FF)
#define VAD_HANG(g) ((g).mh >> 10)

struct VadPlan {
    int n, frames;                   // segments; frames in all
    VadSeg seg[VAD_MAX_STREAMS];
};

struct VadStream { long R, k; VadParams prm; int parity, touched; };      // samples taken and frames judged since fresh; the bank that holds the carry; fed since its reset

static inline long vad_carry_len(long R) { const long c = VAD_HIST + R % VAD_F; return R < c ? R : c; }
static inline long vad_frame_count(const VadStream& s, long more) { return (s.R + more) / VAD_F - s.k; }

static inline const char* vad_params_bad(const VadParams& p) {
    if (p.off_q4 < 16 || p.on_q4 < p.off_q4 || p.on_q4 > 4095) return "on_q4 / off_q4 outside 16 <= off_q4 <= on_q4 <= 4095";
    if (p.min_on < 1 || p.min_on > 1000) return "min_on outside 1 .. 1000";
    if (p.hang < 1 || p.hang > 10000) return "hang outside 1 .. 10000";
    if (p.hold < 0 || p.hold > 10000) return "hold outside 0 .. 10000";
    if (p.n_min < 1 || p.n_min > (1L << 40)) return "n_min outside 1 .. 2^40";
    return nullptr;
}

// nullptr, or why the reset is refused (then no state has moved)
static inline const char* vad_reset(int n_streams, VadStream* st, const int32_t* streams, const VadParams* params, int n) {
    if (!st || !streams || !params) return "null pointer";
    if (const char* bad = sp_ids_bad(n_streams, streams, n)) return bad;
    for (int i = 0; i < n; ++i)
        if (const char* bad = vad_params_bad(params[i])) return bad;
    for (int i = 0; i < n; ++i) {                                                      // (the parity stays: a fresh stream reads no carry)
        VadStream& s = st[streams[i]];
        s.R = 0; s.k = 0; s.touched = 0; s.prm = params[i]; s.prm.pad = 0;
    }
    return nullptr;
}

// Fills `plan` and `next` (the listed streams' states after the call; commit them once the launches are made) from the caller's host
// arrays.  Returns nullptr, or what is wrong (plan->n == 0 then: nothing may be launched, no state may move).
static inline const char* vad_plan_build(int n_streams, const VadStream* st, const int32_t* streams, const long* in_off, const long* n_in,
                                         const int32_t* final, int n, const void* in, int in_is_i16, const void* flags, const void* lag,
                                         const void* power, const void* floor, long* n_frames, VadPlan* plan, VadStream* next) {
    plan->n = 0; plan->frames = 0;
    if (!st || !streams || !in_off || !n_in || !final || !in || !flags || !lag || !power || !floor || !n_frames) return "null pointer";
    if (in_is_i16 != 0 && in_is_i16 != 1) return "unknown input format";
    if ((uintptr_t)in % (in_is_i16 ? 2 : 4) || (uintptr_t)lag % 2 || (uintptr_t)power % 8 || (uintptr_t)floor % 8) return "a misaligned buffer";
    if (const char* bad = sp_ids_bad(n_streams, streams, n)) return bad;
    long total = 0;
    for (int i = 0; i < n; ++i) {
        const VadStream& s = st[streams[i]];
        if (const char* bad = vad_params_bad(s.prm)) return bad;
        if (const char* bad = sp_chunk_bad(n_in[i], in_off[i], s.R)) return bad;
        total += vad_frame_count(s, n_in[i]);
    }
    if (total > (1L << 30)) return "a call of more than 2^30 frames";
    int frames = 0;
    for (int i = 0; i < n; ++i) {
        const VadStream& s = st[streams[i]];
        VadSeg& g = plan->seg[i];
        const int fin = final[i] != 0;
        const long nf = vad_frame_count(s, n_in[i]);
        g.in_off = in_off[i]; g.n_min = s.prm.n_min; g.k0 = s.k;
        g.sid = sp_sid_word(streams[i], s.parity, fin);
        g.Lc = (int)vad_carry_len(s.R); g.n_in = (int)n_in[i];
        g.nf = (int)nf; g.f_off = frames;
        g.onoff = s.prm.on_q4 | s.prm.off_q4 << 12;
        g.mh = s.prm.min_on | s.prm.hang << 10;
        g.hold = s.prm.hold;
        frames += (int)nf;
        n_frames[i] = nf;
        VadStream& t = next[i];
        t = s; t.parity = s.parity ^ 1; t.touched = 1;                 // the call wrote the other bank
        if (fin) { t.R = 0; t.k = 0; }                                // the next sample starts a new clip
        else { t.R = s.R + n_in[i]; t.k = s.k + nf; }
    }
    sp_zero_tail(plan->seg, n);
    plan->n = n; plan->frames = frames;
    return nullptr;
}
