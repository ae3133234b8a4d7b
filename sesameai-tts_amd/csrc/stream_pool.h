// What the pools of stateful audio streams share on the host (mimi_rs_pool_*, mimi_ts_pool_*, mimi_vad_pool_*, mimi_wm_pool_*): the refusals
// of a stream list and of a chunk, the `sid` word of a segment, and the two ends of every plan -- the unused segments zeroed, the listed
// streams' next states committed once the launches are made.  Plain C++: no HIP, like the *_plan.h that build on it
// (tools/stream_pool_check.cpp pins every refusal text down through all four pools).
#pragma once
#include <stdint.h>

#define SP_MAX_STREAMS 64           // streams of one pool, and so segments of one plan
#define SP_MAX_CHUNK (1L << 30)     // samples one stream takes, or gives, in one call (grids and index arithmetic stay inside 32 bits)
#define SP_MAX_TOTAL (1L << 48)     // samples one stream takes between two resets

static inline const char* sp_size_bad(int n_streams) { return n_streams < 1 || n_streams > SP_MAX_STREAMS ? "pool outside 1 .. 64 streams" : nullptr; }

// nullptr, or why the list of a call's stream ids is refused.  repeats_ok: an id may come twice (mimi_rs_pool_reset alone takes that).
static inline const char* sp_ids_bad(int n_streams, const int32_t* streams, int n, bool repeats_ok = false) {
    if (const char* bad = sp_size_bad(n_streams)) return bad;
    if (n < 1 || n > n_streams) return "stream list: need 1 .. n_streams ids";
    bool seen[SP_MAX_STREAMS] = {};
    for (int i = 0; i < n; ++i) {
        const int s = streams[i];
        if (s < 0 || s >= n_streams) return "stream id outside [0, n_streams)";
        if (seen[s] && !repeats_ok) return "duplicate stream id in one call";
        seen[s] = true;
    }
    return nullptr;
}

// nullptr, or why a chunk of n_in samples at in_off is refused for a stream that has taken `taken` samples since its reset
static inline const char* sp_chunk_bad(long n_in, long in_off, long taken) {
    if (n_in < 0) return "a chunk of negative length";
    if (in_off < 0) return "a chunk at a negative offset";
    if (n_in > SP_MAX_CHUNK) return "a chunk of more than 2^30 samples";
    if (taken + n_in > SP_MAX_TOTAL) return "a stream of more than 2^48 samples";
    return nullptr;
}

// A segment's `sid` word: the stream, the carry bank the call READS (it writes the other), whether the call ends the stream's clip.
static inline int sp_sid_word(int sid, int parity, int final) { return sid | parity << 8 | final << 9; }
#define SP_SID(g) ((g).sid & 0xFF)
#define SP_PARITY(g) (((g).sid >> 8) & 1)
#define SP_FINAL(g) (((g).sid >> 9) & 1)

// the segments behind a plan's n: zero, so that the kernel arguments hold nothing of an earlier call
template <class Seg, int N> static inline void sp_zero_tail(Seg (&seg)[N], int n) {
    for (int i = n; i < N; ++i) seg[i] = Seg{};
}

// the listed streams take the states their plan foresaw: only once every launch of the call is made
template <class Stream> static inline void sp_commit(Stream* st, const int32_t* streams, const Stream* next, int n) {
    for (int i = 0; i < n; ++i) st[streams[i]] = next[i];
}
