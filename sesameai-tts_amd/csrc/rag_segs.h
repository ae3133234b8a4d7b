// The segment table of a ragged group prefill (csm_refill_group_begin) and the host-side argument checks that build it.  Plain C++: no HIP,
// so the checks also compile into a stand-alone host program (tools/refill_group_args_check.cpp, run under the host sanitizers).
#pragma once
#include <stdint.h>

// A group of prompt segments whose rows lie back to back in one [M][...] buffer: segment i = rows [row0, row0 + rows) of the buffer = the
// prompt rows of batch slot `slot`, each segment with its own length and start position.  The table travels in the kernel arguments like
// the prefix store's slot list: no host-to-device copy, no synchronisation.
#define RAG_MAX_SEGS 32
struct RagSegs { int n; struct { int slot, row0, rows; } s[RAG_MAX_SEGS]; };

// Fills `out` from the caller's host arrays.  Returns nullptr, or what is wrong with them (out->n == 0 then: nothing may be launched):
// n outside [1, 32], a null array, a slot outside [0, max_batch) or listed twice, a segment without rows, more than max_rows rows in all.
// *tiles_out (optional): the group's 32-row query tiles, sum ceil(rows_i / 32).
static inline const char* rag_segs_build(const int32_t* slots, const int32_t* rows, int n, int max_batch, int max_rows, RagSegs* out, int* tiles_out) {
    out->n = 0;
    if (tiles_out) *tiles_out = 0;
    if (!slots || !rows) return "null slot / row array";
    if (n < 1 || n > RAG_MAX_SEGS) return "n outside [1, 32]";
    long total = 0;
    int tiles = 0;
    for (int i = 0; i < n; ++i) {
        if (slots[i] < 0 || slots[i] >= max_batch) return "slot outside the batch";
        for (int j = 0; j < i; ++j)
            if (slots[j] == slots[i]) return "a slot is listed twice";
        if (rows[i] < 1) return "a segment without rows";
        if (rows[i] > max_rows) return "more rows than max_rows";
        out->s[i].slot = slots[i]; out->s[i].row0 = (int)total; out->s[i].rows = rows[i];
        total += rows[i];
        if (total > max_rows) return "more rows than max_rows";
        tiles += (rows[i] - 1) / 32 + 1;
    }
    for (int i = n; i < RAG_MAX_SEGS; ++i) { out->s[i].slot = 0; out->s[i].row0 = 0; out->s[i].rows = 0; }
    out->n = n;
    if (tiles_out) *tiles_out = tiles;
    return nullptr;
}
static inline int rag_segs_rows(const RagSegs& g) { return g.n > 0 ? g.s[g.n - 1].row0 + g.s[g.n - 1].rows : 0; }
static inline bool rag_segs_has_slot(const RagSegs& g, int slot) {
    for (int i = 0; i < g.n; ++i)
        if (g.s[i].slot == slot) return true;
    return false;
}
