// The segment plan of a pool of stateful Mimi ENCODE streams (mimi_enc_pool_encode): the host-side argument checks, the per-segment header
// that travels in the kernel arguments, and where every listed stream's new rows lie at every level of the encoder.  Plain C++: no HIP, so
// the checks also compile into a stand-alone host program (tools/enc_stream_segs_check.cpp, run under the host sanitizers).  The engine
// defines ENC_SEGS_FN and POOL_SEGS_FN as `__host__ __device__ static inline` before it includes this file, so that k_enc_stream_plan expands
// the header with the SAME functions.
//
// The levels are enc_segs.h's (0 = the samples .. S = the 25 Hz tokens, S + 1 = the frames), the frame-aligned packing and the first four
// blocks of the device table are pool_segs.h's: the products that need nothing else run on the decode pool's ragged instantiations.
#pragma once
#include <stdint.h>

#include "enc_segs.h"
#include "pool_segs.h"

#define ENC_STREAM_MAX_STREAMS POOL_SEG_MAX_STREAMS   // = MIMI_ENC_POOL_MAX_STREAMS
#define ENC_STREAM_MAX_CHUNK POOL_SEG_MAX_CHUNK       // the largest max_chunk_frames mimi_enc_pool_create takes

// The pool's device table, in 32-bit words: pool_segs.h's {stream id, token offset, F0, T} per segment and frame -> segment (sized for the
// largest pool), then per level the segment's NEW rows L (enc_level_len of the chunk's own samples) and whether the chunk is the stream's
// first (token offset 0: the downsample's left edge replicates).  Behind the words, two longs per segment: where its samples start in the
// caller's buffer (ENC_STREAM_LTAB_*).
#define ENC_STREAM_TAB_L(lvl) (POOL_TAB_FRAME + POOL_SEG_MAX_STREAMS * POOL_SEG_MAX_CHUNK + (lvl) * POOL_SEG_MAX_STREAMS)
#define ENC_STREAM_TAB_FIRST ENC_STREAM_TAB_L(ENC_MAX_LEVELS)
#define ENC_STREAM_TAB_WORDS (ENC_STREAM_TAB_FIRST + POOL_SEG_MAX_STREAMS)
#define ENC_STREAM_LTAB_WAV_OFF 0
#define ENC_STREAM_LTAB_LONGS POOL_SEG_MAX_STREAMS

// What the first kernel of the chain gets.  (~1.6 KB of kernel arguments: no host-to-device copy, no synchronisation.)
struct EncStreamHeader {
    int n, S;
    int32_t ratios[ENC_MAX_STAGES];
    int sid[POOL_SEG_MAX_STREAMS], off[POOL_SEG_MAX_STREAMS];
    long wav_off[POOL_SEG_MAX_STREAMS], n_samples[POOL_SEG_MAX_STREAMS];
};

// Segment i owns frames [F0[i], F0[i] + T[i]) of the call, T[i] = ceil(n_i / hop), and columns [F0[i], F0[i] + T[i]) of the codes.
struct EncStreamSegs {
    int n, F;                               // segments, frames in all
    int F0[POOL_SEG_MAX_STREAMS + 1];       // F0[n] = F
    int T[POOL_SEG_MAX_STREAMS];
    unsigned char ends[POOL_SEG_MAX_STREAMS];   // n_i is no multiple of hop: the chunk ends its stream
};

// frames of segment i
ENC_SEGS_FN int enc_stream_T(const EncStreamHeader* hdr, int i) { return (int)enc_ceil_div(hdr->n_samples[i], enc_level_rate(hdr->ratios, hdr->S, 0)); }
// F0[0 .. n] from the header
ENC_SEGS_FN void enc_stream_prefix(const EncStreamHeader* hdr, int* F0) {
    int F = 0;
    for (int i = 0; i < hdr->n; ++i) { F0[i] = F; F += enc_stream_T(hdr, i); }
    F0[hdr->n] = F;
}

// The whole device table from the header, serially (the kernel does the same with one thread per entry).
static inline void enc_stream_expand(const EncStreamHeader* hdr, int* tab, long* ltab) {
    int F0[POOL_SEG_MAX_STREAMS + 1];
    enc_stream_prefix(hdr, F0);
    for (int i = 0; i < hdr->n; ++i) {
        tab[POOL_TAB_SID + i] = hdr->sid[i]; tab[POOL_TAB_OFF + i] = hdr->off[i]; tab[POOL_TAB_F0 + i] = F0[i]; tab[POOL_TAB_T + i] = F0[i + 1] - F0[i];
        for (int l = 0; l < ENC_MAX_LEVELS; ++l) tab[ENC_STREAM_TAB_L(l) + i] = l <= hdr->S + 1 ? (int)enc_level_len(hdr->n_samples[i], hdr->ratios, hdr->S, l) : 0;
        tab[ENC_STREAM_TAB_FIRST + i] = hdr->off[i] == 0;
        ltab[ENC_STREAM_LTAB_WAV_OFF + i] = hdr->wav_off[i];
    }
    for (int f = 0; f < F0[hdr->n]; ++f) tab[POOL_TAB_FRAME + f] = pool_seg_of_frame(F0, f);
}

// Fills `hdr` and `out` from the caller's host arrays; offsets[s] = the tokens stream s has encoded so far, ended[s] != 0: it took a partial
// last frame and waits for its reset.  Returns nullptr, or what is wrong (hdr->n == 0 and out->n == 0 then: nothing may be launched, no offset
// may move): a null pointer, n outside [1, n_streams], an id outside [0, n_streams) or listed twice, an ended stream, a chunk without samples
// or at a negative offset or of more than max_chunk frames, a stream that would pass 2^31 tokens.
static inline const char* enc_stream_segs_build(const int32_t* streams, const long* wav_off, const long* n_samples, int n, const void* wav, const void* codes,
                                                int n_streams, int max_chunk, const long* offsets, const unsigned char* ended, const int32_t* ratios,
                                                int S, EncStreamHeader* hdr, EncStreamSegs* out) {
    hdr->n = 0; hdr->S = S; out->n = 0; out->F = 0;
    if (!streams || !wav_off || !n_samples || !wav || !codes || !offsets || !ended || !ratios) return "null pointer";
    if (S < 1 || S > ENC_MAX_STAGES) return "stage count outside [1, 8]";
    if (n_streams < 1 || n_streams > POOL_SEG_MAX_STREAMS || max_chunk < 1 || max_chunk > POOL_SEG_MAX_CHUNK) return "pool outside 64 streams x 64 frames";
    if (n < 1 || n > n_streams) return "stream list: need 1 .. n_streams ids";
    const long hop = enc_level_rate(ratios, S, 0);
    bool seen[POOL_SEG_MAX_STREAMS] = {};
    for (int i = 0; i < n; ++i) {
        const int s = streams[i];
        if (s < 0 || s >= n_streams) return "stream id outside [0, n_streams)";
        if (seen[s]) return "duplicate stream id in one call";
        seen[s] = true;
        if (ended[s]) return "a stream that took its partial last frame; reset it";
        if (n_samples[i] < 1) return "a chunk without samples";
        if (wav_off[i] < 0) return "a chunk at a negative offset";
        if (n_samples[i] > hop * max_chunk) return "a chunk of more than max_chunk_frames frames";          // (before any product: no overflow)
        if (offsets[s] < 0 || offsets[s] + 2L * enc_ceil_div(n_samples[i], hop) > 0x7fffffffL) return "a stream passed 2^31 tokens; reset it";
    }
    for (int j = 0; j < ENC_MAX_STAGES; ++j) hdr->ratios[j] = j < S ? ratios[j] : 1;
    for (int i = 0; i < POOL_SEG_MAX_STREAMS; ++i) {
        hdr->sid[i] = i < n ? streams[i] : 0; hdr->off[i] = i < n ? (int)offsets[streams[i]] : 0;
        hdr->wav_off[i] = i < n ? wav_off[i] : 0; hdr->n_samples[i] = i < n ? n_samples[i] : 0;
        out->T[i] = 0; out->ends[i] = 0;
    }
    hdr->n = n;
    enc_stream_prefix(hdr, out->F0);
    for (int i = 0; i < n; ++i) { out->T[i] = out->F0[i + 1] - out->F0[i]; out->ends[i] = n_samples[i] % hop != 0; }
    for (int i = n + 1; i <= POOL_SEG_MAX_STREAMS; ++i) out->F0[i] = out->F0[n];
    out->n = n; out->F = out->F0[n];          // (F <= n_streams * max_chunk: every product fits the pool's work buffers)
    return nullptr;
}
