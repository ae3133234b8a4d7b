// The segment plan of a pool of Mimi encode streams (sesameai-tts_amd/csrc/enc_stream_segs.h: no HIP) as a stand-alone host program, built
// with the host sanitizers by tests/test_enc_stream_segs_host.py.  For lists of up to 4 segments whose chunks are whole frames, whole frames
// plus a tail, or a tail alone, at two chunk limits and on shuffled stream ids: the prefix sums and frame -> segment map of the expanded
// table, every level's rows against enc_level_len of the chunk's own samples (a whole-frame chunk fills its slot, a tail never passes it),
// the header's copy of the caller's arrays and the streams' offsets, which chunks end their stream, the 2^31-token bound and every refusal of
// include/mimi_hip.h's mimi_enc_pool_encode, made with nothing planned.  Prints "ok".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "enc_stream_segs.h"

static int g_checks = 0;
#define REQUIRE(cond)                                                              \
    do {                                                                           \
        ++g_checks;                                                                \
        if (!(cond)) { printf("FAILED %s (%s:%d)\n", #cond, __FILE__, __LINE__); exit(1); } \
    } while (0)

static void check_plan(const std::vector<long>& ns, const std::vector<int>& sids, int n_streams, int max_chunk, const int32_t* ratios, int S) {
    const int n = (int)ns.size();
    const long hop = enc_level_rate(ratios, S, 0);
    std::vector<long> offsets(n_streams), woff(n);
    std::vector<unsigned char> ended(n_streams, 0);
    for (int s = 0; s < n_streams; ++s) offsets[s] = s % 2 ? 1000L * s + 6 : 0;       // (some at their first chunk, some later in their life)
    for (int i = 0; i < n; ++i) woff[i] = 7 + 100000L * i;
    const float wav = 0.f; const int32_t codes = 0;                                   // (only tested against null)
    EncStreamHeader hdr; EncStreamSegs sg;
    const char* bad = enc_stream_segs_build(sids.data(), woff.data(), ns.data(), n, &wav, &codes, n_streams, max_chunk, offsets.data(), ended.data(),
                                            ratios, S, &hdr, &sg);
    REQUIRE(bad == nullptr && hdr.n == n && sg.n == n && hdr.S == S);
    int F = 0;
    for (int i = 0; i < n; ++i) {
        const int T = (int)((ns[i] + hop - 1) / hop);
        REQUIRE(hdr.sid[i] == sids[i] && hdr.off[i] == offsets[sids[i]] && hdr.wav_off[i] == woff[i] && hdr.n_samples[i] == ns[i]);
        REQUIRE(sg.F0[i] == F && sg.T[i] == T && T >= 1 && T <= max_chunk && sg.ends[i] == (ns[i] % hop != 0));
        F += T;
    }
    REQUIRE(sg.F == F && sg.F0[n] == F && F <= n_streams * max_chunk);
    std::vector<int> tab(ENC_STREAM_TAB_WORDS, -7);
    std::vector<long> ltab(ENC_STREAM_LTAB_LONGS, -7);
    enc_stream_expand(&hdr, tab.data(), ltab.data());
    for (int i = 0; i < n; ++i) {
        REQUIRE(tab[POOL_TAB_SID + i] == sids[i] && tab[POOL_TAB_OFF + i] == offsets[sids[i]] && tab[POOL_TAB_F0 + i] == sg.F0[i] && tab[POOL_TAB_T + i] == sg.T[i]);
        REQUIRE(tab[ENC_STREAM_TAB_FIRST + i] == (offsets[sids[i]] == 0) && ltab[ENC_STREAM_LTAB_WAV_OFF + i] == woff[i]);
        long L = ns[i];
        for (int l = 0; l <= S + 1; ++l) {
            // the rounded-up division chain of the chunk's OWN samples, whatever came before it ...
            if (l > 0) L = (L + enc_level_div(ratios, S, l) - 1) / enc_level_div(ratios, S, l);
            const long R = enc_level_rate(ratios, S, l);
            REQUIRE(tab[ENC_STREAM_TAB_L(l) + i] == L && L == enc_level_len(ns[i], ratios, S, l));
            // ... which fills the slot of a whole-frame chunk and stays inside the slot of a tail
            REQUIRE(L >= 1 && L <= R * sg.T[i] && L > R * (sg.T[i] - 1));
            if (!sg.ends[i]) REQUIRE(L == R * sg.T[i]);
        }
        REQUIRE(tab[ENC_STREAM_TAB_L(S + 1) + i] == sg.T[i]);
        for (int l = S + 2; l < ENC_MAX_LEVELS; ++l) REQUIRE(tab[ENC_STREAM_TAB_L(l) + i] == 0);
    }
    for (int i = n; i < POOL_SEG_MAX_STREAMS; ++i) REQUIRE(tab[POOL_TAB_SID + i] == -7 && tab[ENC_STREAM_TAB_L(0) + i] == -7 && ltab[i] == -7);
    for (int f = 0; f < F; ++f) {
        const int si = tab[POOL_TAB_FRAME + f];
        REQUIRE(si >= 0 && si < n && f >= sg.F0[si] && f < sg.F0[si] + sg.T[si]);
    }
    for (int w = POOL_TAB_FRAME + F; w < ENC_STREAM_TAB_L(0); ++w) REQUIRE(tab[w] == -7);        // nothing written behind the call's frames
    // the kernels' map of a dense row g at a level with R rows per frame -- si = frame_seg[g / R], tl = g - R * F0_si -- hits every row of
    // every slot once, and the rows it calls valid (tl < L) are the segment's
    for (int l = 0; l <= S + 1; ++l) {
        const long R = enc_level_rate(ratios, S, l);
        long valid = 0, want = 0;
        for (long g = 0; g < R * F; ++g) {
            const int si = tab[POOL_TAB_FRAME + g / R];
            const long tl = g - R * tab[POOL_TAB_F0 + si];
            REQUIRE(tl >= 0 && tl < R * sg.T[si]);
            valid += tl < tab[ENC_STREAM_TAB_L(l) + si];
        }
        for (int i = 0; i < n; ++i) want += enc_level_len(ns[i], ratios, S, l);
        REQUIRE(valid == want);
    }
}

static void check_refusals(int n_streams, int max_chunk, const int32_t* ratios, int S) {
    const long hop = enc_level_rate(ratios, S, 0);
    const float wav = 0.f; const int32_t codes = 0;
    std::vector<int32_t> sids(POOL_SEG_MAX_STREAMS + 1);
    for (int i = 0; i <= POOL_SEG_MAX_STREAMS; ++i) sids[i] = i;
    std::vector<long> ns(POOL_SEG_MAX_STREAMS + 1, hop), woff(POOL_SEG_MAX_STREAMS + 1, 0), offsets(POOL_SEG_MAX_STREAMS + 1, 0);
    std::vector<unsigned char> ended(POOL_SEG_MAX_STREAMS + 1, 0);
    EncStreamHeader hdr; EncStreamSegs sg;
    auto refused = [&](const int32_t* s, const long* wo, const long* nn, int n, const void* w, const void* c, const long* o, const unsigned char* e,
                       const int32_t* rt) {
        hdr.n = 7; sg.n = 7; sg.F = 7;
        const char* bad = enc_stream_segs_build(s, wo, nn, n, w, c, n_streams, max_chunk, o, e, rt, S, &hdr, &sg);
        if (bad == nullptr) return false;
        REQUIRE(bad[0] != 0 && hdr.n == 0 && sg.n == 0 && sg.F == 0);
        return true;
    };
    auto call = [&](int n) { return refused(sids.data(), woff.data(), ns.data(), n, &wav, &codes, offsets.data(), ended.data(), ratios); };
    REQUIRE(!call(n_streams));                                  // every stream at once: the largest list
    REQUIRE(call(0) && call(-1) && call(n_streams + 1));
    if (n_streams >= 2) {
        sids[1] = 0; REQUIRE(call(2));                          // a duplicate
        sids[1] = n_streams; REQUIRE(call(2));                  // out of range, both sides
        sids[1] = -1; REQUIRE(call(2));
        sids[1] = 1; REQUIRE(!call(2));
    }
    for (long bad_n : {0L, -5L, hop * max_chunk + 1, 0x7fffffffffffffffL}) { ns[0] = bad_n; REQUIRE(call(1)); }
    ns[0] = hop * max_chunk; REQUIRE(!call(1) && sg.T[0] == max_chunk && !sg.ends[0]);
    ns[0] = hop * max_chunk - 1; REQUIRE(!call(1) && sg.T[0] == max_chunk && sg.ends[0]);
    ns[0] = 1; REQUIRE(!call(1) && sg.T[0] == 1 && sg.ends[0]);
    woff[0] = -1; REQUIRE(call(1)); woff[0] = 0;
    ended[0] = 1; REQUIRE(call(1));                             // a stream that took its partial last frame ...
    if (n_streams >= 2) { sids[0] = 1; sids[1] = 0; REQUIRE(call(2)); sids[0] = 0; sids[1] = 1; }       // ... anywhere in the list
    ended[0] = 0; REQUIRE(!call(1));
    ns[0] = hop * max_chunk;
    offsets[0] = 0x7fffffffL - 2L * max_chunk;                  // exactly 2^31 - 1 tokens after the call: still fine
    REQUIRE(!call(1) && hdr.off[0] == offsets[0]);
    offsets[0] += 1; REQUIRE(call(1));                          // one token more: past 2^31
    ns[0] = 1; offsets[0] = 0x7fffffffL - 1; REQUIRE(call(1));
    offsets[0] = 0x7fffffffL - 2; REQUIRE(!call(1));
    offsets[0] = -1; REQUIRE(call(1));
    offsets[0] = 0; ns[0] = hop;
    REQUIRE(refused(nullptr, woff.data(), ns.data(), 1, &wav, &codes, offsets.data(), ended.data(), ratios));
    REQUIRE(refused(sids.data(), nullptr, ns.data(), 1, &wav, &codes, offsets.data(), ended.data(), ratios));
    REQUIRE(refused(sids.data(), woff.data(), nullptr, 1, &wav, &codes, offsets.data(), ended.data(), ratios));
    REQUIRE(refused(sids.data(), woff.data(), ns.data(), 1, nullptr, &codes, offsets.data(), ended.data(), ratios));
    REQUIRE(refused(sids.data(), woff.data(), ns.data(), 1, &wav, nullptr, offsets.data(), ended.data(), ratios));
    REQUIRE(refused(sids.data(), woff.data(), ns.data(), 1, &wav, &codes, nullptr, ended.data(), ratios));
    REQUIRE(refused(sids.data(), woff.data(), ns.data(), 1, &wav, &codes, offsets.data(), nullptr, ratios));
    REQUIRE(refused(sids.data(), woff.data(), ns.data(), 1, &wav, &codes, offsets.data(), ended.data(), nullptr));
    REQUIRE(!call(1));
}

int main() {
    const int32_t full[4] = {8, 6, 5, 4};                   // (the tiny codec has the full codec's ratios)
    const int32_t odd[3] = {3, 7, 2};
    struct { const int32_t* ratios; int S; } cfgs[] = {{full, 4}, {odd, 3}};
    for (auto& cf : cfgs) {
        const long hop = enc_level_rate(cf.ratios, cf.S, 0);
        REQUIRE(hop == (cf.S == 4 ? 1920 : 84));
        for (int max_chunk : {3, 17}) {
            // whole frames, whole frames plus a tail (one sample, half a frame +- 1, one short of a frame), a tail alone
            const long lens[] = {hop, hop * max_chunk, hop * (max_chunk - 1) + 1, hop + hop / 2 + 1, 2 * hop - 1, 1, hop / 2};
            const int n_lens = (int)(sizeof lens / sizeof lens[0]);
            for (int n = 1; n <= 3; ++n) {
                std::vector<int> idx(n, 0);
                for (;;) {
                    std::vector<long> ns(n);
                    for (int i = 0; i < n; ++i) ns[i] = lens[idx[i]];
                    std::vector<int> ids_fwd(n), ids_mix(n);
                    for (int i = 0; i < n; ++i) { ids_fwd[i] = i; ids_mix[i] = (4 - i * 3 % 5 + 5) % 5; }      // 4, 1, 3: distinct, unordered
                    check_plan(ns, ids_fwd, 4, max_chunk, cf.ratios, cf.S);
                    check_plan(ns, ids_mix, 5, max_chunk, cf.ratios, cf.S);
                    int k = 0;
                    while (k < n && ++idx[k] == n_lens) idx[k++] = 0;
                    if (k == n) break;
                }
            }
            check_refusals(4, max_chunk, cf.ratios, cf.S);
            check_refusals(1, max_chunk, cf.ratios, cf.S);
            check_refusals(POOL_SEG_MAX_STREAMS, max_chunk, cf.ratios, cf.S);
        }
    }
    if (g_checks < 100000) { printf("only %d checks ran\n", g_checks); return 1; }
    printf("ok\n");
    return 0;
}
