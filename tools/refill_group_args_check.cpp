// Stand-alone host check of csm_refill_group_begin's argument validation and segment-table construction, and of the pending-refill record's
// predicates that both refill forms share (sesameai-tts_amd/csrc/rag_segs.h).
// No GPU, no HIP: build it with the host sanitizers and run it,
//   hipcc -Xarch_host -fsanitize=address,undefined -I sesameai-tts_amd/csrc tools/refill_group_args_check.cpp -o /tmp/rgcheck && /tmp/rgcheck
// (or any C++17 compiler with -fsanitize=address,undefined).  Exit status 0 and "ok" when every case behaves.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rag_segs.h"

static int failures = 0;
#define EXPECT(c)                                                               \
    do {                                                                        \
        if (!(c)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); ++failures; } \
    } while (0)

// heap copies of exactly n elements: an over-read of either array is an AddressSanitizer report
static const char* build(std::vector<int32_t> slots, std::vector<int32_t> rows, int n, int max_batch, int max_rows, RagSegs* out, int* tiles) {
    int32_t* s = (int32_t*)std::malloc(slots.size() * 4 + 1);
    int32_t* r = (int32_t*)std::malloc(rows.size() * 4 + 1);
    if (!slots.empty()) std::memcpy(s, slots.data(), slots.size() * 4);
    if (!rows.empty()) std::memcpy(r, rows.data(), rows.size() * 4);
    const char* why = rag_segs_build(s, r, n, max_batch, max_rows, out, tiles);
    std::free(s); std::free(r);
    return why;
}

int main() {
    RagSegs g;
    int tiles = -1;
    // refusals: nothing may be launched with the table they leave (n == 0)
    EXPECT(rag_segs_build(nullptr, nullptr, 1, 8, 64, &g, &tiles) != nullptr && g.n == 0);
    EXPECT(build({}, {}, 0, 8, 64, &g, &tiles) != nullptr && g.n == 0 && tiles == 0);
    EXPECT(build({}, {}, -3, 8, 64, &g, &tiles) != nullptr && g.n == 0);
    EXPECT(build(std::vector<int32_t>(33, 0), std::vector<int32_t>(33, 1), 33, 64, 64, &g, &tiles) != nullptr && g.n == 0);
    EXPECT(build({0, 2, 0}, {4, 4, 4}, 3, 8, 64, &g, &tiles) != nullptr && g.n == 0);          // duplicate
    EXPECT(build({0, 8}, {4, 4}, 2, 8, 64, &g, &tiles) != nullptr && g.n == 0);                // slot == max_batch
    EXPECT(build({-1}, {4}, 1, 8, 64, &g, &tiles) != nullptr && g.n == 0);
    EXPECT(build({0, 1}, {4, 0}, 2, 8, 64, &g, &tiles) != nullptr && g.n == 0);
    EXPECT(build({0, 1}, {4, -7}, 2, 8, 64, &g, &tiles) != nullptr && g.n == 0);
    EXPECT(build({0, 1}, {60, 5}, 2, 8, 64, &g, &tiles) != nullptr && g.n == 0);               // 65 > max_rows
    EXPECT(build({0, 1}, {2147483647, 2147483647}, 2, 8, 2147483647, &g, &tiles) != nullptr && g.n == 0);     // the sum does not wrap
    EXPECT(build({0}, {2147483647}, 1, 8, 64, &g, &tiles) != nullptr && g.n == 0);
    // accepted: the table
    EXPECT(build({5, 0, 3}, {1, 33, 30}, 3, 8, 64, &g, &tiles) == nullptr);
    EXPECT(g.n == 3 && tiles == 1 + 2 + 1 && rag_segs_rows(g) == 64);
    EXPECT(g.s[0].slot == 5 && g.s[0].row0 == 0 && g.s[0].rows == 1);
    EXPECT(g.s[1].slot == 0 && g.s[1].row0 == 1 && g.s[1].rows == 33);
    EXPECT(g.s[2].slot == 3 && g.s[2].row0 == 34 && g.s[2].rows == 30);
    EXPECT(g.s[3].rows == 0 && g.s[31].rows == 0);
    EXPECT(rag_segs_has_slot(g, 3) && rag_segs_has_slot(g, 5) && !rag_segs_has_slot(g, 1) && !rag_segs_has_slot(g, -1));
    std::vector<int32_t> all(32), ones(32, 2);
    for (int i = 0; i < 32; ++i) all[i] = 31 - i;
    EXPECT(build(all, ones, 32, 32, 64, &g, &tiles) == nullptr && g.n == 32 && tiles == 32 && rag_segs_rows(g) == 64 && g.s[31].slot == 0 && g.s[31].row0 == 62);
    EXPECT(build({7}, {64}, 1, 8, 64, &g, &tiles) == nullptr && g.n == 1 && tiles == 2);
    RagSegs none; none.n = 0;
    EXPECT(!rag_segs_has_slot(none, 0) && rag_segs_rows(none) == 0);
    // the pending-refill record: nothing pending
    RefillRec r;
    refill_clear(r);
    EXPECT(!refill_pending(r) && !refill_has_slot(r, 0) && !r.ragged && r.layer == 0 && r.pos == nullptr);
    // a single slot = a table of one segment at row 0
    const int32_t slot = 6, S = 33;
    EXPECT(rag_segs_build(&slot, &S, 1, 8, 64, &r.sg, nullptr) == nullptr);
    EXPECT(refill_pending(r) && r.sg.n == 1 && r.sg.s[0].row0 == 0 && rag_segs_rows(r.sg) == 33);
    EXPECT(refill_has_slot(r, 6) && !refill_has_slot(r, 0) && !refill_has_slot(r, 7) && !refill_has_slot(r, -1));
    const int32_t slot8 = 8, none_rows = 0, too_many = 65;
    EXPECT(rag_segs_build(&slot8, &S, 1, 8, 64, &r.sg, nullptr) != nullptr && !refill_pending(r));         // what csm_refill_begin refuses
    EXPECT(rag_segs_build(&slot, &none_rows, 1, 8, 64, &r.sg, nullptr) != nullptr && !refill_pending(r));
    EXPECT(rag_segs_build(&slot, &too_many, 1, 8, 64, &r.sg, nullptr) != nullptr && !refill_pending(r));
    // a group
    EXPECT(build({5, 0, 3}, {1, 33, 30}, 3, 8, 64, &r.sg, &r.tiles) == nullptr);
    r.ragged = true;
    EXPECT(refill_pending(r) && r.tiles == 4 && refill_has_slot(r, 0) && refill_has_slot(r, 3) && refill_has_slot(r, 5) && !refill_has_slot(r, 4));
    // which layers an advance runs, and whether the refill is complete after them: from layer 0 and from mid-stack
    const int L = 16;
    struct { int layer, max_layers, l0, l1; bool complete; } cases[] = {
        {0, 1, 0, 1, false},  {0, L - 1, 0, L - 1, false},  {0, L, 0, L, true},  {0, L + 1, 0, L, true},  {0, 2147483647, 0, L, true},
        {7, 1, 7, 8, false},  {7, L - 8, 7, L - 1, false},  {7, L - 7, 7, L, true},  {7, L - 1, 7, L, true},  {7, L, 7, L, true},
        {7, L + 1, 7, L, true},  {7, 2147483647, 7, L, true},  {L - 1, 1, L - 1, L, true},
    };
    for (const auto& c : cases) {
        int l0 = -1, l1 = -1;
        r.layer = c.layer;
        EXPECT(refill_layers(r, c.max_layers, L, &l0, &l1) == c.complete && l0 == c.l0 && l1 == c.l1);
    }
    r.layer = 0;
    { int l0 = -1, l1 = -1; EXPECT(refill_layers(r, 1, 1, &l0, &l1) && l0 == 0 && l1 == 1); }             // a one-layer stack
    refill_clear(r);
    EXPECT(!refill_pending(r) && !refill_has_slot(r, 5) && !r.ragged && r.tiles == 0);
    if (failures) return 1;
    std::puts("ok");
    return 0;
}
