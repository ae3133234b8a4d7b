// The host side of a pool of Whisper log-mel streams (mimi_mel_pool_*, include/mimi_hip.h states the rule; tests/mel_ref.py in NumPy): the
// tables -- window, DFT basis, Slaney filter bank -- built in double, the per-stream host state {R, frames, parity, dropped}, the frame
// counts, the packed output rows, the tiles of the grid and the per-call plan that travels in the kernel arguments.  Plain C++: no HIP, so
// it also compiles into a stand-alone host program (tools/mel_plan_check.cpp, run under the host sanitizers); the small functions that the
// kernels share with that program carry MEL_HD.
//
// Positions.  s is the clip: the samples received, zeros behind them, 480,000 in all.  Frame t reads s[160 t - 200 .. 160 t + 199], an
// index below 0 reflected about 0 and one from 480,000 on reflected about 479,999 (only frame 2999 reaches there).  A stream that has
// received R samples (at most the cap: what comes later is counted and dropped) and emitted E frames keeps s[c0 .. R) with
// c0 = max(0, 160 E - 200): what frame E reads of the samples it has.  Frame E waits, so R < 160 E + 200 and the carry is shorter than 400.
#pragma once
#include <math.h>
#include <stdint.h>

#include "stream_pool.h"

#ifdef __HIPCC__
#define MEL_HD __host__ __device__
#else
#define MEL_HD
#endif

#define MEL_MAX_STREAMS 64           // = MIMI_MEL_MAX_STREAMS
static_assert(MEL_MAX_STREAMS == SP_MAX_STREAMS, "the pools share one spine");
#define MEL_RATE 16000
#define MEL_NFFT 400                 // a frame, and the DFT's length
#define MEL_HOP 160
#define MEL_PAD 200                  // reflection at both ends: NFFT / 2
#define MEL_CAP 480000               // = MIMI_MEL_CAP: 30 s
#define MEL_FRAMES 3000              // = MIMI_MEL_FRAMES: CAP / HOP
#define MEL_BINS 201                 // NFFT / 2 + 1
#define MEL_BINS_PAD 224             // bins padded to whole 32-column tiles: 7 of them
#define MEL_BASIS_COLS (2 * MEL_BINS_PAD)      // = MIMI_MEL_BASIS_COLS: cos of bins 0 .. 223, then -sin of them (the padding is zero)
#define MEL_MAX_MELS 128             // = MIMI_MEL_MAX_MELS: the filter bank is [BINS_PAD][MAX_MELS], columns from n_mels on zero
#define MEL_TILE 32                  // frames of one workgroup
#define MEL_WAVES (MEL_BINS_PAD / 32)          // one wave per 32 bins: its cos and its sin accumulator
#define MEL_THREADS (64 * MEL_WAVES)
#define MEL_CARRY 400                // fp32 per bank: the carry is shorter
#define MEL_SPAN ((MEL_TILE - 1) * MEL_HOP + MEL_NFFT)      // samples a tile of 32 frames reads: 5360
#define MEL_FLOOR 1e-10f
#define MEL_LOG_FLOOR (-10.0f)       // log10 of the floor: what a frame of zeros gives, and every frame that a short clip lacks
#define MEL_MAX_CLIPS 64             // = MIMI_MEL_MAX_CLIPS (mimi_mel_finish)

// samples received since fresh (<= CAP); frames emitted; the bank that holds the carry; samples dropped past the cap since fresh
struct MelStream { long R, E; int parity; long dropped; };

// One listed stream of one call, as the kernels get it: 48 bytes.
struct MelSeg {
    long in_off;                     // elements: its new samples in `in`
    int sid;                         // sp_sid_word
    int n_use;                       // new samples taken: n_in less what falls behind the cap
    int R0, R1;                      // samples received before and after the call
    int c0, c1;                      // first sample of the carry it reads, and of the one it writes (c1 == R1: none)
    int t0, nf;                      // its first frame of the call; frames emitted
    int t_off;                       // its first tile in the grid
    int row_off;                     // its first row in `raw`
};

struct MelPlan {
    int n, tiles;                    // segments; tiles in all
    int n_mels, pad;
    MelSeg seg[MEL_MAX_STREAMS];
};

static inline const char* mel_mels_bad(int n_mels) { return n_mels != 80 && n_mels != 128 ? "n_mels must be 80 or 128" : nullptr; }

// frames emitted once R samples (R <= CAP) are in and the clip has ended (final) or not
MEL_HD static inline long mel_frames(long R, int final) {
    if (final) { const long f = (R + MEL_PAD + MEL_HOP - 1) / MEL_HOP; return f < MEL_FRAMES ? f : MEL_FRAMES; }
    if (R >= MEL_CAP) return MEL_FRAMES;
    return R <= MEL_PAD ? 0 : (R - MEL_PAD) / MEL_HOP + 1;          // (frame 0 needs 201 samples, frame t >= 1 needs 160 t + 200; R < CAP: < 3000)
}

// the first sample a stream that has emitted E frames keeps
MEL_HD static inline long mel_carry_from(long E) { return E * MEL_HOP > MEL_PAD ? E * MEL_HOP - MEL_PAD : 0; }

// what a feed of `more` samples would emit for the stream now
static inline long mel_frame_count(const MelStream& s, long more, int final) {
    const long R = s.R + more < MEL_CAP ? s.R + more : MEL_CAP;
    return mel_frames(R, final) - s.E;
}

// Where sample q of the padded clip (q = 160 t - 200 + n of frame t, any integer a frame can read) comes from: -1: it is zero;
// otherwise the index into s, below R1.  Reflection first, then the zeros behind the samples received.
MEL_HD static inline int mel_source(int q, int R1) {
    const int r = q < 0 ? -q : (q >= MEL_CAP ? 2 * (MEL_CAP - 1) - q : q);
    return r < R1 ? r : -1;
}

// nullptr, or why the reset is refused (then no state has moved): the listed streams are fresh
static inline const char* mel_reset(int n_streams, MelStream* st, const int32_t* streams, int n) {
    if (!st || !streams) return "null pointer";
    if (const char* bad = sp_ids_bad(n_streams, streams, n)) return bad;
    for (int i = 0; i < n; ++i) {                                    // (the parity stays: a fresh stream reads no carry)
        MelStream& s = st[streams[i]];
        s.R = 0; s.E = 0; s.dropped = 0;
    }
    return nullptr;
}

// Fills `plan`, `n_frames` and `next` (the listed streams' states after the call; commit them once the launches are made) from the caller's
// host arrays.  fmt: 0 = fp32, 1 = int16.  Returns nullptr, or what is wrong (plan->n == 0 then: nothing may be launched, no state moved).
static inline const char* mel_plan_build(int n_streams, int n_mels, const MelStream* st, const int32_t* streams, const long* in_off,
                                         const long* n_in, const int32_t* final, int n, const void* in, int fmt, const void* raw,
                                         long* n_frames, MelPlan* plan, MelStream* next) {
    plan->n = 0; plan->tiles = 0; plan->n_mels = 0; plan->pad = 0;
    if (!st || !streams || !in_off || !n_in || !final || !in || !raw || !n_frames) return "null pointer";
    if (fmt != 0 && fmt != 1) return "unknown format";
    if ((uintptr_t)in % (fmt ? 2 : 4) || (uintptr_t)raw % 4) return "a misaligned buffer";
    if (const char* bad = mel_mels_bad(n_mels)) return bad;
    if (const char* bad = sp_ids_bad(n_streams, streams, n)) return bad;
    for (int i = 0; i < n; ++i)
        if (const char* bad = sp_chunk_bad(n_in[i], in_off[i], st[streams[i]].R + st[streams[i]].dropped)) return bad;
    long tiles = 0, rows = 0;
    for (int i = 0; i < n; ++i) {
        const MelStream& s = st[streams[i]];
        const int fin = final[i] != 0;
        const long use = s.R + n_in[i] <= MEL_CAP ? n_in[i] : MEL_CAP - s.R, R1 = s.R + use;
        const long E1 = mel_frames(R1, fin), nf = E1 - s.E;
        MelSeg& g = plan->seg[i];
        g = MelSeg{};
        g.in_off = in_off[i];
        g.sid = sp_sid_word(streams[i], s.parity, fin);
        g.n_use = (int)use; g.R0 = (int)s.R; g.R1 = (int)R1;
        g.c0 = (int)mel_carry_from(s.E);
        g.c1 = fin || E1 >= MEL_FRAMES ? (int)R1 : (int)mel_carry_from(E1);      // a clip that has ended or is full keeps nothing
        g.t0 = (int)s.E; g.nf = (int)nf;
        g.t_off = (int)tiles; g.row_off = (int)rows;
        tiles += (nf + MEL_TILE - 1) / MEL_TILE;                                   // (<= 64 * 94)
        rows += nf;
        n_frames[i] = nf;
        MelStream& t = next[i];
        t = s; t.parity = s.parity ^ 1;                                            // the call wrote the other bank
        if (fin) { t.R = 0; t.E = 0; t.dropped = 0; }                              // the next sample starts a new clip
        else { t.R = R1; t.E = E1; t.dropped = s.dropped + (n_in[i] - use); }
    }
    sp_zero_tail(plan->seg, n);
    plan->n = n; plan->tiles = (int)tiles; plan->n_mels = n_mels;
    return nullptr;
}

// ---- the stateless finisher (mimi_mel_finish): up to 64 clips, one workgroup per (clip, tile of 32 frames) ----
struct MelFinSeg { long off; int n_frames, pad; };                   // elements: the clip's first row in `raw`; its rows
struct MelFinPlan { int n, n_mels; MelFinSeg seg[MEL_MAX_CLIPS]; };
#define MEL_FIN_TILES ((MEL_FRAMES + MEL_TILE - 1) / MEL_TILE)       // 94 a clip

static inline const char* mel_fin_plan_build(const void* raw, const long* off, const long* n_frames, int n, int n_mels, const void* out,
                                             MelFinPlan* plan) {
    plan->n = 0; plan->n_mels = 0;
    if (!raw || !off || !n_frames || !out) return "null pointer";
    if ((uintptr_t)raw % 4 || (uintptr_t)out % 4) return "a misaligned buffer";
    if (const char* bad = mel_mels_bad(n_mels)) return bad;
    if (n < 1 || n > MEL_MAX_CLIPS) return "clip list: need 1 .. 64 clips";
    for (int i = 0; i < n; ++i) {
        if (n_frames[i] < 0 || n_frames[i] > MEL_FRAMES) return "a clip of more than 3000 frames, or of fewer than 0";
        if (off[i] < 0) return "a clip at a negative offset";
    }
    for (int i = 0; i < MEL_MAX_CLIPS; ++i) {
        plan->seg[i] = MelFinSeg{};
        if (i < n) { plan->seg[i].off = off[i]; plan->seg[i].n_frames = (int)n_frames[i]; }
    }
    plan->n = n; plan->n_mels = n_mels;
    return nullptr;
}

// ---- the tables, in double ----
static inline double mel_window(int n) { return 0.5 - 0.5 * cos(2.0 * M_PI * n / MEL_NFFT); }      // the PERIODIC Hann window

// basis[n][c], c < BINS_PAD: cos(2 pi n c / 400); c >= BINS_PAD: -sin(2 pi n (c - BINS_PAD) / 400); zero for the padded bins.  The angle
// is reduced in integers first, so the table is exact to double rounding however large n * k is.
static inline double mel_basis(int n, int c) {
    const int k = c < MEL_BINS_PAD ? c : c - MEL_BINS_PAD;
    if (k >= MEL_BINS) return 0.0;
    const double a = 2.0 * M_PI * (double)((long)n * k % MEL_NFFT) / MEL_NFFT;
    return c < MEL_BINS_PAD ? cos(a) : -sin(a);
}

// Slaney's mel scale: linear below 1 kHz (200 / 3 Hz a mel), logarithmic above (27 steps an factor of 6.4)
static inline double mel_hz_to_mel(double hz) {
    const double min_log_hz = 1000.0, min_log_mel = 15.0, logstep = 27.0 / log(6.4);
    return hz >= min_log_hz ? min_log_mel + log(hz / min_log_hz) * logstep : 3.0 * hz / 200.0;
}
static inline double mel_mel_to_hz(double mel) {
    const double min_log_hz = 1000.0, min_log_mel = 15.0, logstep = log(6.4) / 27.0;
    return mel >= min_log_mel ? min_log_hz * exp(logstep * (mel - min_log_mel)) : 200.0 * mel / 3.0;
}

// bank[k][m], k < 201, m < n_mels: the triangular filters between 0 and 8000 Hz, n_mels + 2 edges evenly spaced in mel, each filter scaled
// by 2 / (its upper edge - its lower edge) in Hz (Slaney's area normalisation).  `edges`: n_mels + 2 doubles of scratch.
static inline double mel_bank(const double* edges, int k, int m) {
    const double f = (double)k * (MEL_RATE / 2) / (MEL_BINS - 1);
    const double up = (f - edges[m]) / (edges[m + 1] - edges[m]), down = (edges[m + 2] - f) / (edges[m + 2] - edges[m + 1]);
    const double tri = up < down ? up : down;
    return tri > 0.0 ? tri * 2.0 / (edges[m + 2] - edges[m]) : 0.0;
}
static inline void mel_bank_edges(int n_mels, double* edges) {
    const double lo = mel_hz_to_mel(0.0), hi = mel_hz_to_mel(MEL_RATE / 2.0);
    for (int i = 0; i < n_mels + 2; ++i) edges[i] = mel_mel_to_hz(lo + (hi - lo) * i / (n_mels + 1));
}

// window[400], basis[400][BASIS_COLS], bank[BINS_PAD][MAX_MELS], as fp32
static inline void mel_tables(int n_mels, float* window, float* basis, float* bank) {
    double edges[MEL_MAX_MELS + 2];
    mel_bank_edges(n_mels, edges);
    for (int n = 0; n < MEL_NFFT; ++n) {
        window[n] = (float)mel_window(n);
        for (int c = 0; c < MEL_BASIS_COLS; ++c) basis[(long)n * MEL_BASIS_COLS + c] = (float)mel_basis(n, c);
    }
    for (int k = 0; k < MEL_BINS_PAD; ++k)
        for (int m = 0; m < MEL_MAX_MELS; ++m) bank[k * MEL_MAX_MELS + m] = k < MEL_BINS && m < n_mels ? (float)mel_bank(edges, k, m) : 0.0f;
}
