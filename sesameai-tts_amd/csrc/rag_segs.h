// The segment table of a ragged group prefill (csm_refill_group_begin), the host-side argument checks that build it, and the record of the
// pending refill beside the frame loop that both begin forms share.  Plain C++: no HIP,
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

// The refill beside the frame loop that a handle has begun and not completed: ONE record for both begin forms.  csm_refill_begin's slot is
// a table of one segment at row 0; sg.n == 0 means nothing is pending.  `ragged` (begun by csm_refill_group_begin, also with one segment)
// only chooses the layer launches of an advance; parking, completion and every predicate read the table alone.
struct RefillRec {
    RagSegs sg;
    bool ragged;
    int tiles;              // the table's 32-row query tiles (read by the ragged launches)
    int layer;              // next backbone layer to run
    const int32_t* pos;     // the caller's position array (device memory, valid until the refill completes)
};
static inline void refill_clear(RefillRec& r) { r.sg.n = 0; r.ragged = false; r.tiles = 0; r.layer = 0; r.pos = nullptr; }
static inline bool refill_pending(const RefillRec& r) { return r.sg.n > 0; }
static inline bool refill_has_slot(const RefillRec& r, int slot) { return rag_segs_has_slot(r.sg, slot); }
// An advance of max_layers >= 1 runs layers [*l0, *l1) of n_layers; true when the refill is complete after them.
static inline bool refill_layers(const RefillRec& r, int max_layers, int n_layers, int* l0, int* l1) {
    *l0 = r.layer;
    *l1 = max_layers < n_layers - r.layer ? r.layer + max_layers : n_layers;
    return *l1 >= n_layers;
}
