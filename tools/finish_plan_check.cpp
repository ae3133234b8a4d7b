// The host plan of the segment finisher (sesameai-tts_amd/csrc/finish_plan.h: no HIP) as a stand-alone host program, built with the host
// sanitizers by tests/test_finish_plan_host.py.  Every refusal of include/mimi_hip.h's mimi_fin_segments, made with nothing planned; the packed
// output offsets, odd ones and an odd buffer address included, and the parity each segment's pairs are aligned by; the fade clamp; the tile
// counts of both kernels at lengths around one tile, and the peak tile that grows so that no segment has more than 256 partials, up to 2^30
// samples; 64 segments in one plan; N = 0; and, by walking every block of a plan, that the block -> (segment, tile) maps cover every sample and
// every output exactly once and nothing else.  Prints "ok".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "finish_plan.h"

static int g_checks = 0;
#define REQUIRE(cond)                                                              \
    do {                                                                           \
        ++g_checks;                                                                \
        if (!(cond)) { printf("FAILED %s (%s:%d)\n", #cond, __FILE__, __LINE__); exit(1); } \
    } while (0)

struct Call {
    std::vector<const float*> in;
    std::vector<long> n_in, out_off, n_out;
    std::vector<int32_t> lead, tail, fade;
    void add(const float* p, long n, int l, int t, int f) { in.push_back(p); n_in.push_back(n); lead.push_back(l); tail.push_back(t); fade.push_back(f); }
    const char* build(const void* out, FinPlan* plan) {
        out_off.assign(in.size() + 1, -7); n_out.assign(in.size() + 1, -7);
        return fin_plan_build(in.data(), n_in.data(), lead.data(), tail.data(), fade.data(), (int)in.size(), out, out_off.data(), n_out.data(), plan);
    }
};

static float g_x[4];                       // somewhere aligned to point at; never read
alignas(4) static int16_t g_out[4];

static void refused(Call& c, const void* out, const char* word) {
    FinPlan plan;
    plan.n = 99;
    const char* bad = c.build(out, &plan);
    REQUIRE(bad != nullptr && strstr(bad, word) != nullptr);
    REQUIRE(plan.n == 0 && plan.pblocks == 0 && plan.wblocks == 0);
}

static void check_refusals() {
    FinPlan plan;
    long o[1], m[1];
    const float* in[1] = {g_x};
    const long n_in[1] = {4};
    const int32_t z[1] = {0};
    REQUIRE(fin_plan_build(nullptr, n_in, z, z, z, 1, g_out, o, m, &plan) != nullptr && plan.n == 0);
    REQUIRE(fin_plan_build(in, nullptr, z, z, z, 1, g_out, o, m, &plan) != nullptr);
    REQUIRE(fin_plan_build(in, n_in, nullptr, z, z, 1, g_out, o, m, &plan) != nullptr);
    REQUIRE(fin_plan_build(in, n_in, z, nullptr, z, 1, g_out, o, m, &plan) != nullptr);
    REQUIRE(fin_plan_build(in, n_in, z, z, nullptr, 1, g_out, o, m, &plan) != nullptr);
    REQUIRE(fin_plan_build(in, n_in, z, z, z, 1, nullptr, o, m, &plan) != nullptr);
    REQUIRE(fin_plan_build(in, n_in, z, z, z, 1, g_out, nullptr, m, &plan) != nullptr);
    REQUIRE(fin_plan_build(in, n_in, z, z, z, 1, g_out, o, nullptr, &plan) != nullptr);
    REQUIRE(fin_plan_build(in, n_in, z, z, z, 0, g_out, o, m, &plan) != nullptr && plan.n == 0);
    REQUIRE(fin_plan_build(in, n_in, z, z, z, -1, g_out, o, m, &plan) != nullptr);
    { Call c; for (int i = 0; i < 65; ++i) c.add(g_x, 1, 0, 0, 0); refused(c, g_out, "1 .. 64"); }
    { Call c; c.add(g_x, 3, 0, 0, 0); c.add(g_x, -1, 0, 0, 0); refused(c, g_out, "negative length"); }
    { Call c; c.add(g_x, 3, -1, 0, 0); refused(c, g_out, "negative lead"); }
    { Call c; c.add(g_x, 3, 0, -1, 0); refused(c, g_out, "negative lead"); }
    { Call c; c.add(g_x, 3, 0, 0, -1); refused(c, g_out, "negative lead"); }
    { Call c; c.add(g_x, (1L << 30) + 1, 0, 0, 0); refused(c, g_out, "2^30"); }
    { Call c; c.add(g_x, (1L << 30) - 1, 1, 1, 0); refused(c, g_out, "2^30"); }
    { Call c; c.add(g_x, 1L << 40, 0, 0, 0); refused(c, g_out, "2^30"); }
    { Call c; c.add(g_x, 0, 0x7fffffff, 0x7fffffff, 0); refused(c, g_out, "2^30"); }
    { Call c; c.add(g_x, 2, 0, 0, 0); c.add(nullptr, 1, 0, 0, 0); refused(c, g_out, "null pointer"); }
    { Call c; c.add((const float*)((uintptr_t)g_x + 2), 1, 0, 0, 0); refused(c, g_out, "aligned"); }
    { Call c; c.add(g_x, 1, 0, 0, 0); refused(c, (const char*)g_out + 1, "aligned"); }
    REQUIRE(fin_out_count(-1, 0, 0) == -1 && fin_out_count(0, -1, 0) == -1 && fin_out_count(0, 0, -1) == -1);
    REQUIRE(fin_out_count(1L << 30, 0, 1) == -1 && fin_out_count(1L << 30, 0, 0) == (1L << 30) && fin_out_count(0, 0, 0) == 0);
    REQUIRE(fin_out_count(1L << 62, 1L << 62, 1L << 62) == -1);
    REQUIRE(fin_out_count(5, 12000, 2400) == 14405);
}

// walks every block of both kernels the way the kernels do and counts what each sample and each output is visited
static void walk(const FinPlan& plan, const int16_t* out) {
    long total = 0;
    for (int i = 0; i < plan.n; ++i) total += plan.seg[i].m;
    std::vector<int> seen_out(total, 0);
    for (int i = 0; i < plan.n; ++i) {
        const FinSeg& g = plan.seg[i];
        REQUIRE(fin_ptiles(g) <= FIN_MAX_PTILES && g.ptile >= FIN_PEAK_TILE);
        REQUIRE(g.par == (int)((((uintptr_t)out / 2) + (uintptr_t)g.out_off) & 1));
        REQUIRE(g.nfade >= 0 && g.nfade <= g.m / 2);
    }
    long samples = 0;
    for (int b = 0; b < plan.pblocks; ++b) {
        int i = 0;
        while (i + 1 < plan.n && plan.seg[i + 1].pblk0 <= b) ++i;
        const FinSeg& g = plan.seg[i];
        const int tile = b - g.pblk0;
        REQUIRE(tile >= 0 && tile < fin_ptiles(g));
        const long lo = (long)tile * g.ptile, rest = g.n_in - lo;
        REQUIRE(rest > 0);
        samples += rest < g.ptile ? rest : g.ptile;
    }
    long want = 0;
    for (int i = 0; i < plan.n; ++i) want += plan.seg[i].n_in;
    REQUIRE(samples == want);
    for (int b = 0; b < plan.wblocks; ++b) {
        int i = 0;
        while (i + 1 < plan.n && plan.seg[i + 1].wblk0 <= b) ++i;
        const FinSeg& g = plan.seg[i];
        REQUIRE(b - g.wblk0 >= 0 && b - g.wblk0 < fin_wtiles(g));
        const long p0 = (long)(b - g.wblk0) * (FIN_OUT_TILE / 2);
        for (long p = p0; p < p0 + FIN_OUT_TILE / 2; ++p) {
            const long j0 = 2 * p - g.par;
            if (j0 >= g.m) break;
            REQUIRE((((uintptr_t)out / 2 + (uintptr_t)(g.out_off + j0)) & 1) == 0);      // every pair is 4-byte aligned
            if (j0 >= 0) ++seen_out[g.out_off + j0];
            if (j0 + 1 < g.m) ++seen_out[g.out_off + j0 + 1];
        }
    }
    for (long k = 0; k < total; ++k) REQUIRE(seen_out[k] == 1);
}

static void check_layout() {
    // odd lengths: the second and fourth segments start at odd elements; an empty clip in the middle; a fade clamped by M / 2
    Call c;
    c.add(g_x, 5, 0, 0, 0);              // M = 5
    c.add(g_x, 4096, 3, 4, 1200);        // M = 4103
    c.add(nullptr, 0, 2, 0, 7);          // M = 2, n = 1
    c.add(g_x, 1, 0, 0, 9);              // M = 1, n = 0
    c.add(nullptr, 0, 0, 0, 0);          // M = 0
    c.add(g_x, 4097, 12000, 2400, 1200);
    FinPlan plan;
    REQUIRE(c.build(g_out, &plan) == nullptr && plan.n == 6);
    const long M[6] = {5, 4103, 2, 1, 0, 18497};
    long O = 0;
    for (int i = 0; i < 6; ++i) {
        REQUIRE(c.out_off[i] == O && c.n_out[i] == M[i] && plan.seg[i].out_off == O && plan.seg[i].m == M[i]);
        REQUIRE(plan.seg[i].par == (int)(O & 1));
        O += M[i];
    }
    REQUIRE(c.out_off[6] == -7 && c.n_out[6] == -7);                                   // nothing written past n
    REQUIRE(plan.seg[1].nfade == 1200 && plan.seg[2].nfade == 1 && plan.seg[3].nfade == 0 && plan.seg[4].nfade == 0 && plan.seg[5].nfade == 1200);
    REQUIRE(plan.seg[2].in == nullptr && plan.seg[4].in == nullptr && plan.seg[2].n_in == 0);
    REQUIRE(fin_ptiles(plan.seg[0]) == 1 && fin_ptiles(plan.seg[1]) == 1 && fin_ptiles(plan.seg[2]) == 0 && fin_ptiles(plan.seg[5]) == 2);
    REQUIRE(plan.seg[0].pblk0 == 0 && plan.seg[1].pblk0 == 1 && plan.seg[2].pblk0 == 2 && plan.seg[3].pblk0 == 2 && plan.seg[4].pblk0 == 3 &&
            plan.seg[5].pblk0 == 3 && plan.pblocks == 5);
    REQUIRE(fin_wtiles(plan.seg[4]) == 0 && plan.seg[5].wblk0 == plan.seg[4].wblk0);
    for (int i = 6; i < FIN_MAX_SEGMENTS; ++i) REQUIRE(plan.seg[i].in == nullptr && plan.seg[i].m == 0);
    walk(plan, g_out);
    // the same call into a buffer that itself starts at an odd int16: every parity flips
    FinPlan odd;
    REQUIRE(c.build(g_out + 1, &odd) == nullptr);
    for (int i = 0; i < 6; ++i) REQUIRE(odd.seg[i].par == (plan.seg[i].par ^ 1));
    walk(odd, g_out + 1);
}

static void check_tiles() {
    const long lens[] = {0, 1, 2, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 1048575, 1048576, 1048577, 1048576 + 256, 3000001};
    for (long n : lens)
        for (int par = 0; par < 2; ++par) {
            Call c;
            if (par) c.add(nullptr, 0, 1, 0, 0);                                       // one output in front: the segment under test starts odd
            c.add(g_x, n, 0, 0, 0);
            FinPlan plan;
            REQUIRE(c.build(g_out, &plan) == nullptr);
            const FinSeg& g = plan.seg[par];
            REQUIRE(g.par == par);
            REQUIRE(fin_wtiles(g) == (n == 0 ? 0 : (n + par + FIN_OUT_TILE - 1) / FIN_OUT_TILE));
            const long ptile = n <= (long)FIN_PEAK_TILE * FIN_MAX_PTILES ? FIN_PEAK_TILE : (n + FIN_MAX_PTILES - 1) / FIN_MAX_PTILES;
            REQUIRE(g.ptile == ptile && fin_ptiles(g) == (n + ptile - 1) / ptile);
            if (n <= 1048577) walk(plan, g_out);
        }
    // the largest legal segment: 256 peak tiles of 2^22 samples, 2^19 write blocks, everything inside 32 bits
    Call c;
    c.add(g_x, 1L << 30, 0, 0, 1 << 30);
    c.add(g_x, (1L << 30) - 3, 1, 2, 5);
    FinPlan plan;
    REQUIRE(c.build(g_out, &plan) == nullptr);
    REQUIRE(plan.seg[0].ptile == (1 << 22) && fin_ptiles(plan.seg[0]) == 256 && fin_wtiles(plan.seg[0]) == (1 << 19) && plan.seg[0].nfade == (1 << 29));
    REQUIRE(fin_ptiles(plan.seg[1]) == 256 && plan.seg[1].out_off == (1L << 30) && plan.seg[1].m == (1 << 30));
    REQUIRE(plan.pblocks == 512 && plan.wblocks == (1 << 20) && c.out_off[1] == (1L << 30));
}

static void check_64_segments() {
    Call c;
    long O = 0;
    std::vector<long> want;
    for (int i = 0; i < 64; ++i) { c.add(i % 7 == 3 ? nullptr : g_x, i % 7 == 3 ? 0 : 100 * i + 1, i % 5, i % 3, i * 10); }
    FinPlan plan;
    REQUIRE(c.build(g_out, &plan) == nullptr && plan.n == 64);
    int pb = 0, wb = 0;
    for (int i = 0; i < 64; ++i) {
        const long n = i % 7 == 3 ? 0 : 100 * i + 1, m = n + i % 5 + i % 3;
        REQUIRE(c.out_off[i] == O && c.n_out[i] == m && plan.seg[i].pblk0 == pb && plan.seg[i].wblk0 == wb);
        REQUIRE(plan.seg[i].nfade == (i * 10 < m / 2 ? i * 10 : m / 2));
        pb += fin_ptiles(plan.seg[i]); wb += fin_wtiles(plan.seg[i]);
        O += m;
    }
    REQUIRE(plan.pblocks == pb && plan.wblocks == wb);
    walk(plan, g_out);
    // all clips empty and no silence: a legal call with nothing to launch
    Call e;
    for (int i = 0; i < 64; ++i) e.add(nullptr, 0, 0, 0, 50);
    REQUIRE(e.build(g_out, &plan) == nullptr && plan.n == 64 && plan.pblocks == 0 && plan.wblocks == 0);
}

int main() {
    REQUIRE(sizeof(FinPlan) <= 3200);                                                   // travels in the kernel arguments
    check_refusals();
    check_layout();
    check_tiles();
    check_64_segments();
    REQUIRE(g_checks > 100);
    printf("ok\n");
    return 0;
}
