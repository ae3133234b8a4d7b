// The segment plan of a ragged stream-pool decode (mimi_pool_decode_ragged): the host-side argument checks, the per-segment header that
// travels in the kernel arguments, and where every listed stream's rows lie at every level of the decoder.  Plain C++: no HIP, so the checks
// also compile into a stand-alone host program (tools/pool_segs_check.cpp, run under the host sanitizers).  The engine defines POOL_SEGS_FN
// as `__host__ __device__ static inline` before it includes this file, so that k_pool_begin_ragged expands the header with the SAME functions.
#pragma once
#include <stdint.h>

#ifndef POOL_SEGS_FN
#define POOL_SEGS_FN static inline
#endif

#define POOL_SEG_MAX_STREAMS 64         // = MIMI_POOL_MAX_STREAMS
#define POOL_SEG_MAX_CHUNK 64           // the largest max_chunk_frames mimi_pool_create takes

// The pool's device table, in 32-bit words.  The first two blocks are what a uniform call (mimi_pool_decode) writes and reads; a ragged call
// fills all of it: per segment i (the i-th listed stream) its stream id, its token offset, its first frame F0 and its frames T, and behind
// them, per frame of the call, the segment that owns it.
#define POOL_TAB_SID 0
#define POOL_TAB_OFF (1 * POOL_SEG_MAX_STREAMS)
#define POOL_TAB_F0 (2 * POOL_SEG_MAX_STREAMS)
#define POOL_TAB_T (3 * POOL_SEG_MAX_STREAMS)
#define POOL_TAB_FRAME (4 * POOL_SEG_MAX_STREAMS)
POOL_SEGS_FN long pool_tab_words(int n_streams, int max_chunk) { return POOL_TAB_FRAME + (long)n_streams * max_chunk; }

// What the first kernel of the chain gets: {stream id, token offset, frames} per segment.  (772 bytes of kernel arguments: no host-to-device
// copy, no synchronisation.)
struct PoolSegHeader {
    int n;
    int sid[POOL_SEG_MAX_STREAMS], off[POOL_SEG_MAX_STREAMS], T[POOL_SEG_MAX_STREAMS];
};

// Frame-aligned packing: segment i owns frames [F0[i], F0[i] + T[i]) of the call and, at a level with R rows per frame (1 at the frames,
// 2 at the transformer's tokens, each SEANet stage's rate above that, hop at the samples), dense rows [R * F0[i], R * (F0[i] + T[i])).
// Decode only up-samples: no tails, no rounded-up lengths.
struct PoolSegs {
    int n, F;                           // segments, frames in all
    int F0[POOL_SEG_MAX_STREAMS + 1];   // F0[n] = F
};

// F0[0 .. n] from the header's T
POOL_SEGS_FN void pool_segs_prefix(const PoolSegHeader* hdr, int* F0) {
    int F = 0;
    for (int i = 0; i < hdr->n; ++i) { F0[i] = F; F += hdr->T[i]; }
    F0[hdr->n] = F;
}
// the segment of frame f, 0 <= f < F0[n]
POOL_SEGS_FN int pool_seg_of_frame(const int* F0, int f) {
    int i = 0;
    while (f >= F0[i + 1]) ++i;
    return i;
}
// the rows of segment i at a level with R rows per frame: [lo, hi)
POOL_SEGS_FN long pool_seg_row_lo(const int* F0, int i, long R) { return R * F0[i]; }
POOL_SEGS_FN long pool_seg_row_hi(const int* F0, int i, long R) { return R * F0[i + 1]; }

// The whole device table from the header, serially (the kernel does the same with one thread per entry).  tab: pool_tab_words() words.
static inline void pool_segs_expand(const PoolSegHeader* hdr, int* tab) {
    int F0[POOL_SEG_MAX_STREAMS + 1];
    pool_segs_prefix(hdr, F0);
    for (int i = 0; i < hdr->n; ++i) {
        tab[POOL_TAB_SID + i] = hdr->sid[i]; tab[POOL_TAB_OFF + i] = hdr->off[i]; tab[POOL_TAB_F0 + i] = F0[i]; tab[POOL_TAB_T + i] = hdr->T[i];
    }
    for (int f = 0; f < F0[hdr->n]; ++f) tab[POOL_TAB_FRAME + f] = pool_seg_of_frame(F0, f);
}

// Fills `hdr` and `out` from the caller's host arrays; offsets[s] = the tokens stream s has decoded so far.  Returns nullptr, or what is
// wrong (hdr->n == 0 and out->n == 0 then: nothing may be launched and no offset may move): a null pointer, n outside [1, n_streams], an id
// outside [0, n_streams) or listed twice, a frames[i] outside [1, max_chunk], a stream that would pass 2^31 tokens.
static inline const char* pool_segs_build(const int32_t* streams, const int32_t* frames, int n, const void* codes, const void* pcm, int n_streams,
                                          int max_chunk, const long* offsets, PoolSegHeader* hdr, PoolSegs* out) {
    hdr->n = 0; out->n = 0; out->F = 0;
    if (!streams || !frames || !codes || !pcm || !offsets) return "null pointer";
    if (n_streams < 1 || n_streams > POOL_SEG_MAX_STREAMS || max_chunk < 1 || max_chunk > POOL_SEG_MAX_CHUNK) return "pool outside 64 streams x 64 frames";
    if (n < 1 || n > n_streams) return "stream list: need 1 .. n_streams ids";
    bool seen[POOL_SEG_MAX_STREAMS] = {};
    for (int i = 0; i < n; ++i) {
        const int s = streams[i];
        if (s < 0 || s >= n_streams) return "stream id outside [0, n_streams)";
        if (seen[s]) return "duplicate stream id in one call";
        seen[s] = true;
        if (frames[i] < 1 || frames[i] > max_chunk) return "frames[i] must be 1 .. max_chunk_frames given to mimi_pool_create";
        if (offsets[s] < 0 || offsets[s] + 2L * frames[i] > 0x7fffffffL) return "a stream passed 2^31 tokens; reset it";
    }
    for (int i = 0; i < POOL_SEG_MAX_STREAMS; ++i) {
        hdr->sid[i] = i < n ? streams[i] : 0; hdr->off[i] = i < n ? (int)offsets[streams[i]] : 0; hdr->T[i] = i < n ? frames[i] : 0;
    }
    hdr->n = n;
    pool_segs_prefix(hdr, out->F0);
    for (int i = n + 1; i <= POOL_SEG_MAX_STREAMS; ++i) out->F0[i] = out->F0[n];
    out->n = n; out->F = out->F0[n];         // (F <= n_streams * max_chunk: every product fits the workspaces of a full uniform call)
    return nullptr;
}
