// The clip plan of a ragged Mimi encode (mimi_encode_many): the host-side argument checks, where every clip's rows lie at every level of
// the encoder, and the per-clip header that travels in the kernel arguments.  Plain C++: no HIP, so the checks also compile into a
// stand-alone host program (tools/enc_segs_check.cpp, run under the host sanitizers).  The engine defines ENC_SEGS_FN as
// `__host__ __device__ static inline` before it includes this file, so that k_enc_plan expands the header with the SAME functions.
#pragma once
#include <stdint.h>

#ifndef ENC_SEGS_FN
#define ENC_SEGS_FN static inline
#endif

#define ENC_MAX_CLIPS 64
#define ENC_MAX_STAGES 8
#define ENC_MAX_LEVELS (ENC_MAX_STAGES + 2)

// Levels of the encoder, S = number of SEANet stages: 0 = the samples, j = 1 .. S the output of the j-th strided convolution (S: the
// 25 Hz tokens the transformer works on), S + 1 = the 12.5 Hz frames.  The j-th strided convolution divides by ratios[S - j] (the decoder's
// ratios, reversed), the token -> frame downsample by 2; every division rounds up, as encode_one does for one clip.
ENC_SEGS_FN long enc_ceil_div(long a, long b) { return (a + b - 1) / b; }
ENC_SEGS_FN int enc_level_div(const int32_t* ratios, int S, int lvl) { return lvl <= S ? ratios[S - lvl] : 2; }     // level lvl - 1 -> lvl
// rows per frame at a level: hop at level 0, 2 at level S, 1 at level S + 1
ENC_SEGS_FN long enc_level_rate(const int32_t* ratios, int S, int lvl) {
    long r = 1;
    for (int l = S + 1; l > lvl; --l) r *= enc_level_div(ratios, S, l);
    return r;
}
// rows of a clip of n samples at a level
ENC_SEGS_FN long enc_level_len(long n, const int32_t* ratios, int S, int lvl) {
    long L = n;
    for (int l = 1; l <= lvl; ++l) L = enc_ceil_div(L, enc_level_div(ratios, S, l));
    return L;
}

// What the first kernel of the chain gets: per clip where its samples start and how many there are.  (~1 KB of kernel arguments: no
// host-to-device copy, no synchronisation.)
struct EncHeader {
    int n, S;
    int32_t ratios[ENC_MAX_STAGES];
    struct { long wav_off, n_samples; } c[ENC_MAX_CLIPS];
};

// Frame-aligned packing: clip i owns frames [F0[i], F0[i] + T[i]) and, at a level with R rows per frame, rows
// [R * F0[i], R * F0[i] + enc_level_len(n_i, level)) of that level's buffer; the rest of its R * T[i] rows is an unused tail.
struct EncSegs {
    int n, S, F;                        // clips, stages, frames in all
    int F0[ENC_MAX_CLIPS], T[ENC_MAX_CLIPS];
};

// Fills `hdr` and `out` from the caller's host arrays.  Returns nullptr, or what is wrong (out->n == 0 then: nothing may be launched):
// a null pointer, no encoder weights, n outside [1, 64], a clip without samples or at a negative offset, more than max_frames frames
// in all (or more rows at the sample level than an int holds).
static inline const char* enc_segs_build(const void* wav, const long* wav_off, const long* n_samples, int n, const void* codes, int has_encoder,
                                         const int32_t* ratios, int S, long max_frames, EncHeader* hdr, EncSegs* out) {
    out->n = 0; out->S = S; out->F = 0;
    hdr->n = 0; hdr->S = S;
    if (!wav || !wav_off || !n_samples || !codes || !ratios) return "null pointer";
    if (!has_encoder) return "this codec was created without encoder weights";
    if (S < 1 || S > ENC_MAX_STAGES) return "stage count outside [1, 8]";
    if (n < 1 || n > ENC_MAX_CLIPS) return "n outside [1, 64]";
    const long hop = enc_level_rate(ratios, S, 0);
    long F = 0;
    for (int i = 0; i < n; ++i) {
        if (n_samples[i] < 1) return "a clip without samples";
        if (wav_off[i] < 0) return "a clip at a negative offset";
        if (n_samples[i] > hop * max_frames) return "more frames than max_frames";         // (before the sum: no overflow)
        const long T = enc_ceil_div(n_samples[i], hop);
        out->F0[i] = (int)F; out->T[i] = (int)T;
        F += T;
        if (F > max_frames) return "more frames than max_frames";
        if (F * hop > 0x7fffffffL) return "more sample rows than an int holds";
    }
    for (int j = 0; j < ENC_MAX_STAGES; ++j) hdr->ratios[j] = j < S ? ratios[j] : 1;
    for (int i = 0; i < ENC_MAX_CLIPS; ++i) {
        hdr->c[i].wav_off = i < n ? wav_off[i] : 0; hdr->c[i].n_samples = i < n ? n_samples[i] : 0;
        if (i >= n) { out->F0[i] = 0; out->T[i] = 0; }
    }
    hdr->n = n; out->n = n; out->F = (int)F;
    return nullptr;
}
