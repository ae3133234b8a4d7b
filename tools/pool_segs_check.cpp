// The segment plan of a ragged stream-pool decode (sesameai-tts_amd/csrc/pool_segs.h: no HIP) as a stand-alone host program, built with
// the host sanitizers by tests/test_pool_segs_host.py.  For every list of up to 4 segments with T_i in {1, 2, max - 1, max}, at two chunk
// limits and on shuffled stream ids: the dense slots tile [0, R * F) at every level of the decoder without gap or overlap, the expanded table
// names the right segment at every frame and row, the header carries the caller's arrays and the streams' offsets, and every refusal of
// include/mimi_hip.h's mimi_pool_decode_ragged is made with nothing planned.  Prints "ok".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "pool_segs.h"

static int g_checks = 0;
#define REQUIRE(cond)                                                              \
    do {                                                                           \
        ++g_checks;                                                                \
        if (!(cond)) { printf("FAILED %s (%s:%d)\n", #cond, __FILE__, __LINE__); exit(1); } \
    } while (0)

// rows per frame at every level of the decoder: the frames, the transformer's tokens, then each SEANet stage (the last: samples)
static std::vector<long> level_rates(const int32_t* ratios, int S) {
    std::vector<long> R = {1, 2};
    for (int j = 0; j < S; ++j) R.push_back(R.back() * ratios[j]);
    return R;
}

static void check_plan(const std::vector<int>& Ts, const std::vector<int>& sids, int n_streams, int max_chunk, const std::vector<long>& rates) {
    const int n = (int)Ts.size();
    std::vector<long> offsets(n_streams);
    for (int s = 0; s < n_streams; ++s) offsets[s] = 1000L * s + 6;       // (each stream somewhere else in its life)
    const int32_t codes = 0; const float pcm = 0.f;                       // (only tested against null)
    PoolSegHeader hdr; PoolSegs sg;
    const char* bad = pool_segs_build(sids.data(), Ts.data(), n, &codes, &pcm, n_streams, max_chunk, offsets.data(), &hdr, &sg);
    REQUIRE(bad == nullptr && hdr.n == n && sg.n == n);
    int F = 0;
    for (int i = 0; i < n; ++i) {
        REQUIRE(hdr.sid[i] == sids[i] && hdr.T[i] == Ts[i] && hdr.off[i] == offsets[sids[i]]);
        REQUIRE(sg.F0[i] == F);
        F += Ts[i];
    }
    REQUIRE(sg.F == F && sg.F0[n] == F && F <= n_streams * max_chunk);
    std::vector<int> tab((size_t)pool_tab_words(n_streams, max_chunk), -7);
    pool_segs_expand(&hdr, tab.data());
    for (int i = 0; i < n; ++i)
        REQUIRE(tab[POOL_TAB_SID + i] == sids[i] && tab[POOL_TAB_OFF + i] == offsets[sids[i]] && tab[POOL_TAB_F0 + i] == sg.F0[i] && tab[POOL_TAB_T + i] == Ts[i]);
    for (int f = 0; f < F; ++f) {
        const int si = tab[POOL_TAB_FRAME + f];
        REQUIRE(si >= 0 && si < n && f >= sg.F0[si] && f < sg.F0[si] + Ts[si]);
        REQUIRE(si == pool_seg_of_frame(sg.F0, f));
    }
    for (long w = POOL_TAB_FRAME + F; w < (long)tab.size(); ++w) REQUIRE(tab[w] == -7);       // nothing written behind the call's frames
    for (long R : rates) {
        // the slots tile [0, R * F): each starts where the one before ends, the first at 0, the last at R * F ...
        REQUIRE(pool_seg_row_lo(sg.F0, 0, R) == 0 && pool_seg_row_hi(sg.F0, n - 1, R) == R * F);
        for (int i = 0; i < n; ++i) {
            REQUIRE(pool_seg_row_hi(sg.F0, i, R) - pool_seg_row_lo(sg.F0, i, R) == R * Ts[i]);
            if (i + 1 < n) REQUIRE(pool_seg_row_hi(sg.F0, i, R) == pool_seg_row_lo(sg.F0, i + 1, R));
        }
        // ... and the kernels' map of a dense row g -- si = frame_seg[g / R], tl = g - R * F0_si -- lands inside the slot, every row once
        std::vector<int> hits((size_t)(R * F), 0);
        for (long g = 0; g < R * F; ++g) {
            const int si = tab[POOL_TAB_FRAME + g / R];
            const long tl = g - R * tab[POOL_TAB_F0 + si];
            REQUIRE(tl >= 0 && tl < R * Ts[si] && g >= pool_seg_row_lo(sg.F0, si, R) && g < pool_seg_row_hi(sg.F0, si, R));
            ++hits[(size_t)(pool_seg_row_lo(sg.F0, si, R) + tl)];
        }
        for (int h : hits) REQUIRE(h == 1);
    }
}

static void check_refusals(int n_streams, int max_chunk) {
    const int32_t codes = 0; const float pcm = 0.f;
    std::vector<int32_t> sids(POOL_SEG_MAX_STREAMS + 1), Ts(POOL_SEG_MAX_STREAMS + 1, 1);
    for (int i = 0; i <= POOL_SEG_MAX_STREAMS; ++i) sids[i] = i;
    std::vector<long> offsets(POOL_SEG_MAX_STREAMS + 1, 0);
    PoolSegHeader hdr; PoolSegs sg;
    auto refused = [&](const int32_t* s, const int32_t* t, int n, const void* c, const void* p, const long* o) {
        hdr.n = 7; sg.n = 7; sg.F = 7;
        const char* bad = pool_segs_build(s, t, n, c, p, n_streams, max_chunk, o, &hdr, &sg);
        if (bad == nullptr) return false;
        REQUIRE(bad[0] != 0 && hdr.n == 0 && sg.n == 0 && sg.F == 0);
        return true;
    };
    REQUIRE(!refused(sids.data(), Ts.data(), n_streams, &codes, &pcm, offsets.data()));      // every stream at once: the largest list
    REQUIRE(refused(sids.data(), Ts.data(), 0, &codes, &pcm, offsets.data()));
    REQUIRE(refused(sids.data(), Ts.data(), -1, &codes, &pcm, offsets.data()));
    REQUIRE(refused(sids.data(), Ts.data(), n_streams + 1, &codes, &pcm, offsets.data()));
    if (n_streams >= 2) {
        sids[1] = 0;                                                                             // a duplicate
        REQUIRE(refused(sids.data(), Ts.data(), 2, &codes, &pcm, offsets.data()));
        sids[1] = n_streams;                                                                     // out of range, both sides
        REQUIRE(refused(sids.data(), Ts.data(), 2, &codes, &pcm, offsets.data()));
        sids[1] = -1;
        REQUIRE(refused(sids.data(), Ts.data(), 2, &codes, &pcm, offsets.data()));
        sids[1] = 1;
    }
    for (int bad_T : {0, -3, max_chunk + 1, 0x7fffffff}) {
        Ts[0] = bad_T;
        REQUIRE(refused(sids.data(), Ts.data(), 1, &codes, &pcm, offsets.data()));
    }
    Ts[0] = max_chunk;
    REQUIRE(!refused(sids.data(), Ts.data(), 1, &codes, &pcm, offsets.data()));
    offsets[0] = 0x7fffffffL - 2L * max_chunk;                                                 // exactly 2^31 - 1 tokens after the call: still fine
    REQUIRE(!refused(sids.data(), Ts.data(), 1, &codes, &pcm, offsets.data()) && hdr.off[0] == offsets[0]);
    offsets[0] += 1;                                                                            // one token more: past 2^31
    REQUIRE(refused(sids.data(), Ts.data(), 1, &codes, &pcm, offsets.data()));
    Ts[0] = 1; offsets[0] = 0x7fffffffL - 1;
    REQUIRE(refused(sids.data(), Ts.data(), 1, &codes, &pcm, offsets.data()));
    offsets[0] = 0;
    REQUIRE(refused(nullptr, Ts.data(), 1, &codes, &pcm, offsets.data()));
    REQUIRE(refused(sids.data(), nullptr, 1, &codes, &pcm, offsets.data()));
    REQUIRE(refused(sids.data(), Ts.data(), 1, nullptr, &pcm, offsets.data()));
    REQUIRE(refused(sids.data(), Ts.data(), 1, &codes, nullptr, offsets.data()));
    REQUIRE(refused(sids.data(), Ts.data(), 1, &codes, &pcm, nullptr));
    REQUIRE(!refused(sids.data(), Ts.data(), 1, &codes, &pcm, offsets.data()));
}

int main() {
    const int32_t full[4] = {8, 6, 5, 4};                   // (the tiny codec has the full codec's ratios)
    const int32_t odd[3] = {3, 7, 2};
    struct { const int32_t* ratios; int S; } cfgs[] = {{full, 4}, {odd, 3}};
    for (auto& cf : cfgs) {
        const std::vector<long> rates = level_rates(cf.ratios, cf.S);
        for (int max_chunk : {3, 10, 17}) {
            const int lens[] = {1, 2, max_chunk - 1, max_chunk};
            for (int n = 1; n <= 4; ++n) {
                std::vector<int> idx(n, 0);
                for (;;) {
                    std::vector<int> Ts(n);
                    for (int i = 0; i < n; ++i) Ts[i] = lens[idx[i]];
                    std::vector<int> ids_fwd(n), ids_mix(n);
                    for (int i = 0; i < n; ++i) { ids_fwd[i] = i; ids_mix[i] = (4 - i * 3 % 5 + 5) % 5; }      // 4, 1, 3, 0: distinct, unordered
                    check_plan(Ts, ids_fwd, 4, max_chunk, rates);
                    check_plan(Ts, ids_mix, 5, max_chunk, rates);
                    int k = 0;
                    while (k < n && ++idx[k] == 4) idx[k++] = 0;
                    if (k == n) break;
                }
            }
            check_refusals(4, max_chunk);
            check_refusals(1, max_chunk);
            check_refusals(POOL_SEG_MAX_STREAMS, max_chunk);
        }
    }
    if (g_checks < 100000) { printf("only %d checks ran\n", g_checks); return 1; }
    printf("ok\n");
    return 0;
}
