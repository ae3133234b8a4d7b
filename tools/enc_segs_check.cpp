// The clip plan of a ragged Mimi encode (sesameai-tts_amd/csrc/enc_segs.h: no HIP) as a stand-alone host program, built with the host
// sanitizers by tests/test_enc_segs_host.py.  For every list of up to 4 clips with lengths around 1, hop / 2, hop +- 1 and 2 hop +- 1
// samples, at the tiny and the full ratios: the clips' slots do not overlap at any level, a clip's rows fit its slot, every level's row
// count is the chain of rounded-up divisions that mimi_engine.hip's encode_one computes for the clip alone, the header carries the
// caller's arrays, and every refusal of include/mimi_hip.h's mimi_encode_many is made with nothing planned.  Prints "ok".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "enc_segs.h"

static int g_checks = 0;
#define REQUIRE(cond)                                                              \
    do {                                                                           \
        ++g_checks;                                                                \
        if (!(cond)) { printf("FAILED %s (%s:%d)\n", #cond, __FILE__, __LINE__); exit(1); } \
    } while (0)

// encode_one's own arithmetic for one clip of n samples: L after each strided convolution (r = ratios reversed), then T = ceil(n / hop)
static void encode_one_chain(long n, const int32_t* ratios, int S, long* L /*[S + 2]*/) {
    long hop = 2;
    for (int j = 0; j < S; ++j) hop *= ratios[j];
    L[0] = n;
    for (int j = 0; j < S; ++j) { const int r = ratios[S - 1 - j]; L[j + 1] = (L[j] + r - 1) / r; }
    L[S + 1] = (n + hop - 1) / hop;
}

static void check_plan(const std::vector<long>& ns, const int32_t* ratios, int S, long max_frames) {
    const int n = (int)ns.size();
    std::vector<long> off(n);
    long at = 3;                                             // (the clips need not start at 0 nor lie back to back)
    for (int i = 0; i < n; ++i) { off[i] = at; at += ns[i] + 5; }
    const float wav = 0.f; const int32_t codes = 0;          // (only tested against null)
    EncHeader hdr; EncSegs sg;
    long hop = 2;
    for (int j = 0; j < S; ++j) hop *= ratios[j];
    long F = 0;
    for (long v : ns) F += (v + hop - 1) / hop;
    const char* bad = enc_segs_build(&wav, off.data(), ns.data(), n, &codes, 1, ratios, S, max_frames, &hdr, &sg);
    if (F > max_frames) { REQUIRE(bad != nullptr && sg.n == 0 && hdr.n == 0); return; }
    REQUIRE(bad == nullptr && sg.n == n && hdr.n == n && sg.F == F && sg.S == S && hdr.S == S);
    REQUIRE(enc_level_rate(ratios, S, 0) == hop && enc_level_rate(ratios, S, S) == 2 && enc_level_rate(ratios, S, S + 1) == 1);
    for (int i = 0; i < n; ++i) {
        REQUIRE(hdr.c[i].wav_off == off[i] && hdr.c[i].n_samples == ns[i]);
        REQUIRE(sg.F0[i] == (i ? sg.F0[i - 1] + sg.T[i - 1] : 0));          // slots back to back in frames: no overlap at any level ...
        long L[ENC_MAX_LEVELS];
        encode_one_chain(ns[i], ratios, S, L);
        REQUIRE(sg.T[i] == L[S + 1]);
        for (int l = 0; l <= S + 1; ++l) {
            const long R = enc_level_rate(ratios, S, l), len = enc_level_len(ns[i], ratios, S, l);
            REQUIRE(len == L[l]);                                               // ... the single clip's chain
            REQUIRE(len >= 1 && len <= R * sg.T[i]);                            // ... and the rows fit the slot
            if (i + 1 < n) REQUIRE(R * sg.F0[i] + len <= R * sg.F0[i + 1]);
            REQUIRE(R * sg.F0[i] + len <= R * sg.F);
        }
        REQUIRE(enc_level_len(ns[i], ratios, S, S + 1) == sg.T[i]);          // every frame of a slot is a frame of the clip
    }
}

static void check_refusals(const int32_t* ratios, int S) {
    long hop = 2;
    for (int j = 0; j < S; ++j) hop *= ratios[j];
    const float wav = 0.f; const int32_t codes = 0;
    long off[ENC_MAX_CLIPS + 1], ns[ENC_MAX_CLIPS + 1];
    for (int i = 0; i <= ENC_MAX_CLIPS; ++i) { off[i] = i * hop; ns[i] = hop; }
    EncHeader hdr; EncSegs sg;
    auto refused = [&](const void* w, const long* o, const long* s, int n, const void* c, int enc, long max_frames) {
        sg.n = 7; hdr.n = 7;
        const char* bad = enc_segs_build(w, o, s, n, c, enc, ratios, S, max_frames, &hdr, &sg);
        return bad != nullptr && bad[0] != 0 && sg.n == 0 && hdr.n == 0;
    };
    REQUIRE(!refused(&wav, off, ns, 64, &codes, 1, 64));                     // 64 clips of one frame: the largest call
    REQUIRE(refused(&wav, off, ns, 0, &codes, 1, 64));
    REQUIRE(refused(&wav, off, ns, -1, &codes, 1, 64));
    REQUIRE(refused(&wav, off, ns, 65, &codes, 1, 1000));
    REQUIRE(refused(&wav, off, ns, 64, &codes, 1, 63));                      // sum T = max_frames + 1
    ns[1] = hop + 1;
    REQUIRE(refused(&wav, off, ns, 64, &codes, 1, 64));                      // one sample more: 65 frames
    REQUIRE(!refused(&wav, off, ns, 63, &codes, 1, 64));
    ns[1] = 0;
    REQUIRE(refused(&wav, off, ns, 4, &codes, 1, 64));
    ns[1] = -5;
    REQUIRE(refused(&wav, off, ns, 4, &codes, 1, 64));
    ns[1] = 0x7fffffffffffffffL;                                             // no overflow on the way to the refusal
    REQUIRE(refused(&wav, off, ns, 4, &codes, 1, 64));
    ns[1] = hop; off[2] = -1;
    REQUIRE(refused(&wav, off, ns, 4, &codes, 1, 64));
    off[2] = 2 * hop;
    REQUIRE(refused(&wav, off, ns, 4, &codes, 0, 64));                       // no encoder weights
    REQUIRE(refused(nullptr, off, ns, 4, &codes, 1, 64));
    REQUIRE(refused(&wav, nullptr, ns, 4, &codes, 1, 64));
    REQUIRE(refused(&wav, off, nullptr, 4, &codes, 1, 64));
    REQUIRE(refused(&wav, off, ns, 4, nullptr, 1, 64));
    REQUIRE(!refused(&wav, off, ns, 4, &codes, 1, 64));
}

int main() {
    const int32_t full[4] = {8, 6, 5, 4};
    const int32_t odd[3] = {3, 7, 2};                       // ratios that are not nested multiples: the rounded-up divisions still chain
    struct { const int32_t* ratios; int S; } cfgs[] = {{full, 4}, {odd, 3}};     // (the tiny codec has the full codec's ratios)
    for (auto& cf : cfgs) {
        long hop = 2;
        for (int j = 0; j < cf.S; ++j) hop *= cf.ratios[j];
        const long lens[] = {1, 2, hop / 2, hop / 2 + 1, hop - 1, hop, hop + 1, 2 * hop - 1, 2 * hop, 2 * hop + 1};
        const int nl = (int)(sizeof lens / sizeof lens[0]);
        for (int n = 1; n <= 4; ++n) {
            std::vector<int> idx(n, 0);
            for (;;) {
                std::vector<long> ns(n);
                for (int i = 0; i < n; ++i) ns[i] = lens[idx[i]];
                check_plan(ns, cf.ratios, cf.S, 64);
                check_plan(ns, cf.ratios, cf.S, 5);          // (some lists fit 5 frames, the others are refused)
                int k = 0;
                while (k < n && ++idx[k] == nl) idx[k++] = 0;
                if (k == n) break;
            }
        }
        check_refusals(cf.ratios, cf.S);
    }
    if (g_checks < 100000) { printf("only %d checks ran\n", g_checks); return 1; }
    printf("ok\n");
    return 0;
}
