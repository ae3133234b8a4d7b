// The host plan of a pool of resampler streams (sesameai-tts_amd/csrc/resample_plan.h: no HIP) as a stand-alone host program, built with the
// host sanitizers by tests/test_resample_plan_host.py.  For the ten rate pairs around 24 kHz: the reduced factors and the history length; the
// taps' symmetry and DC gain; every refusal of include/mimi_hip.h's mimi_rs_pool_create / mimi_rs_pool_feed, made with nothing planned; the
// packed output offsets and the block prefix; the emitted counts against the closed formula for chunks of 0, 1, look-ahead - 1, look-ahead and
// 1921 samples, open and final; that no output ever reaches further back than the history holds; and a stream walked past 2^40 samples in
// large steps, whose kernel-visible numbers equal those of its totals reduced by whole periods and stay inside 32 bits.  Prints "ok".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "resample_plan.h"

static int g_checks = 0;
#define REQUIRE(cond)                                                              \
    do {                                                                           \
        ++g_checks;                                                                \
        if (!(cond)) { printf("FAILED %s (%s:%d)\n", #cond, __FILE__, __LINE__); exit(1); } \
    } while (0)

static const int PAIRS[10][2] = {{48000, 24000}, {44100, 24000}, {32000, 24000}, {22050, 24000}, {16000, 24000}, {8000, 24000},
                                 {24000, 48000}, {24000, 44100}, {24000, 16000}, {24000, 8000}};

// the definition's counts, on UNREDUCED totals
static long want_emitted(const RsRates& r, long N, bool final) {
    if (final) return (N * r.up + r.down - 1) / r.down;
    const long a = N * r.up - 1 - r.half;
    return a < 0 ? 0 : a / r.down + 1;
}

struct Walk {                        // one stream, fed through rs_plan_build, beside its unreduced totals
    RsRates r;
    RsStream st[RS_MAX_STREAMS] = {};
    long N = 0, E = 0;               // unreduced: samples taken, outputs emitted
    void feed(int sid, long n, bool final, RsSeg* seg_out = nullptr) {
        const int32_t ids[1] = {sid}, fin[1] = {final ? 1 : 0};
        const long off[1] = {5}, len[1] = {n};
        long n_out[1] = {-1};
        const float x = 0; float y = 0;
        RsPlan plan; RsStream next[RS_MAX_STREAMS];
        const char* bad = rs_plan_build(r, 4, st, ids, off, len, fin, 1, &x, 0, &y, 0, n_out, &plan, next);
        REQUIRE(bad == nullptr && plan.n == 1);
        const RsSeg& g = plan.seg[0];
        const long e = want_emitted(r, N + n, final);
        REQUIRE(n_out[0] == e - E && g.n_out == n_out[0] && g.n_in == n && g.in_off == 5 && g.out_off == 0 && g.sid == sid && g.blk0 == 0);
        REQUIRE(plan.blocks == (g.n_out + RS_BLOCK - 1) / RS_BLOCK);
        // what the kernel sees = the totals reduced by whole periods: the same differences n * down - k * up
        const long Q = N / r.down < E / r.up ? N / r.down : E / r.up;
        REQUIRE(g.k_base == N - Q * r.down && g.n0 == E - Q * r.up);
        REQUIRE(g.k_base >= 0 && g.n0 >= 0 && g.k_base <= r.down + r.hist + 2 && g.n0 <= 2 * r.up + r.down);
        REQUIRE(g.k0 == (-Q * r.down > RS_K0_FLOOR ? -Q * r.down : RS_K0_FLOOR) && g.k0 <= 0);
        REQUIRE(g.bank == st[sid].bank && next[0].bank == (st[sid].bank ^ 1));
        // every 64-bit product the kernel forms from them stays far inside 32 bits' reach of the chunk
        REQUIRE((long)g.k_base + g.n_in < (1L << 31) && (long)g.n0 + g.n_out < (1L << 31));
        if (g.n_out > 0) {
            // the first output's oldest sample lies inside the history, its newest inside the chunk (open clip)
            const long c = (long)g.n0 * r.down + r.half;
            REQUIRE(-rs_floor_div(-(c - 2L * r.half), r.up) >= (long)g.k_base - (r.hist - 1));
            const long cl = (long)(g.n0 + g.n_out - 1) * r.down + r.half;
            if (!final) REQUIRE(rs_floor_div(cl, r.up) <= (long)g.k_base + g.n_in - 1);
        }
        st[sid] = next[0];
        if (final) { REQUIRE(st[sid].n_in == 0 && st[sid].n_out == 0 && st[sid].k0 == 0); N = 0; E = 0; }
        else { N += n; E = e; }
        if (seg_out) *seg_out = g;
    }
};

static void check_pair(int src, int dst) {
    RsRates r;
    REQUIRE(rs_rates(src, dst, &r) == nullptr);
    const long g = rs_gcd(src, dst);
    REQUIRE(r.up == dst / g && r.down == src / g && r.half == 10 * (r.up > r.down ? r.up : r.down) && r.hist == 2 * r.half / r.up + 1);
    REQUIRE(r.half / r.up <= 30 && r.hist <= 61);
    const std::vector<double> h = rs_taps(r);
    REQUIRE((int)h.size() == 2 * r.half + 1);
    double sum = 0;
    for (int i = 0; i <= 2 * r.half; ++i) { sum += h[i]; REQUIRE(fabs(h[i] - h[2 * r.half - i]) < 1e-15 * r.up); }
    REQUIRE(fabs(sum - r.up) < 1e-12 * r.up);
    const int look = r.half / r.up;            // whole samples of look-ahead
    const long chunks[5] = {0, 1, look - 1, look, 1921};
    for (int a = 0; a < 5; ++a)
        for (int b = 0; b < 5; ++b)
            for (int c = 0; c < 5; ++c)
                for (int fin = 0; fin < 2; ++fin) {
                    Walk w; w.r = r;
                    w.feed(1, chunks[a], false); w.feed(1, chunks[b], false); w.feed(1, chunks[c], fin != 0);
                    if (fin) w.feed(1, chunks[a], true);                  // the stream is fresh again
                }
    // an open stream of `look` samples has emitted nothing, one more sample may free the first output
    { Walk w; w.r = r; RsSeg s; w.feed(0, look, false, &s); REQUIRE(s.n_out == 0); }
    // past 2^40 samples in steps of about 2^28: the kernel's numbers never grow
    {
        Walk w; w.r = r;
        long step = (1L << 28) + 12345;
        while (w.N < (1L << 40) + 7) { w.feed(2, step, false); step = (1L << 28) + (step * 7 + 3) % 100003; }
        RsSeg s; w.feed(2, 1921, false, &s);
        REQUIRE(s.k0 == RS_K0_FLOOR);
        w.feed(2, 0, true, &s);
        REQUIRE(s.n_out >= 0 && s.n_out <= r.half / r.down + 2);
    }
}

static void check_offsets_and_refusals() {
    RsRates r;
    REQUIRE(rs_rates(48000, 24000, &r) == nullptr);
    RsStream st[RS_MAX_STREAMS] = {};
    const float x = 0; float y = 0;
    RsPlan plan; RsStream next[RS_MAX_STREAMS];
    // four streams, two of which emit nothing: offsets are packed, zero-output segments own no block
    const int32_t ids[4] = {3, 0, 2, 1}, fin[4] = {0, 1, 0, 1};
    const long off[4] = {0, 100, 5000, 9000}, len[4] = {5, 1000, 0, 300};
    long n_out[4];
    REQUIRE(rs_plan_build(r, 4, st, ids, off, len, fin, 4, &x, 1, &y, 1, n_out, &plan, next) == nullptr && plan.n == 4);
    REQUIRE(n_out[0] == 0 && n_out[1] == 500 && n_out[2] == 0 && n_out[3] == 150);
    REQUIRE(plan.seg[0].out_off == 0 && plan.seg[1].out_off == 0 && plan.seg[2].out_off == 500 && plan.seg[3].out_off == 500);
    REQUIRE(plan.seg[0].blk0 == 0 && plan.seg[1].blk0 == 0 && plan.seg[2].blk0 == 2 && plan.seg[3].blk0 == 2 && plan.blocks == 3);
    for (int b = 0; b < plan.blocks; ++b) {                       // the kernel's search finds the owner of every block
        int i = 0;
        while (i + 1 < plan.n && plan.seg[i + 1].blk0 <= b) ++i;
        REQUIRE(plan.seg[i].n_out > 0 && b >= plan.seg[i].blk0 && (b - plan.seg[i].blk0) * RS_BLOCK < plan.seg[i].n_out);
    }
    for (int i = 0; i < 4; ++i) REQUIRE(plan.seg[i].in_off == off[i] && plan.seg[i].sid == ids[i]);
    REQUIRE(next[0].n_in == 5 && next[0].n_out == 0 && next[1].n_in == 0 && next[2].n_in == 0 && next[3].n_out == 0);

    RsRates q;
    REQUIRE(rs_rates(24000, 24000, &q) != nullptr && rs_rates(0, 24000, &q) != nullptr && rs_rates(24000, -1, &q) != nullptr);
    REQUIRE(rs_rates(24000, 24001, &q) != nullptr && rs_rates(321, 1, &q) != nullptr && rs_rates(1, 321, &q) != nullptr);
    REQUIRE(rs_rates(320, 1, &q) == nullptr && q.down == 320 && q.half == 3200 && q.hist == 6401);
    REQUIRE(rs_rates(1, 320, &q) == nullptr && q.up == 320 && q.hist == 21);

    const int32_t one[1] = {0}, fin0[1] = {0};
    const long o0[1] = {0}, l1[1] = {10};
    long no[4];
#define REFUSED(...)                                                                                   \
    do {                                                                                               \
        plan.n = 7;                                                                                    \
        REQUIRE(rs_plan_build(__VA_ARGS__, no, &plan, next) != nullptr && plan.n == 0 && plan.blocks == 0); \
    } while (0)
    REFUSED(r, 4, st, nullptr, o0, l1, fin0, 1, &x, 0, &y, 0);
    REFUSED(r, 4, st, one, nullptr, l1, fin0, 1, &x, 0, &y, 0);
    REFUSED(r, 4, st, one, o0, nullptr, fin0, 1, &x, 0, &y, 0);
    REFUSED(r, 4, st, one, o0, l1, nullptr, 1, &x, 0, &y, 0);
    REFUSED(r, 4, st, one, o0, l1, fin0, 1, nullptr, 0, &y, 0);
    REFUSED(r, 4, st, one, o0, l1, fin0, 1, &x, 0, nullptr, 0);
    plan.n = 7;
    REQUIRE(rs_plan_build(r, 4, st, one, o0, l1, fin0, 1, &x, 0, &y, 0, nullptr, &plan, next) != nullptr && plan.n == 0);
    REFUSED(r, 4, st, one, o0, l1, fin0, 1, &x, 2, &y, 0);
    REFUSED(r, 4, st, one, o0, l1, fin0, 1, &x, 0, &y, -1);
    REFUSED(r, 4, st, one, o0, l1, fin0, 0, &x, 0, &y, 0);
    REFUSED(r, 4, st, ids, off, len, fin, 5, &x, 0, &y, 0);
    const int32_t dup[2] = {1, 1}, far[1] = {4}, neg[1] = {-1};
    const long o2[2] = {0, 0}, l2[2] = {1, 1};
    const int32_t f2[2] = {0, 0};
    REFUSED(r, 4, st, dup, o2, l2, f2, 2, &x, 0, &y, 0);
    REFUSED(r, 4, st, far, o0, l1, fin0, 1, &x, 0, &y, 0);
    REFUSED(r, 4, st, neg, o0, l1, fin0, 1, &x, 0, &y, 0);
    const long lneg[1] = {-1}, oneg[1] = {-1}, lbig[1] = {SP_MAX_CHUNK + 1};
    REFUSED(r, 4, st, one, o0, lneg, fin0, 1, &x, 0, &y, 0);
    REFUSED(r, 4, st, one, oneg, l1, fin0, 1, &x, 0, &y, 0);
    REFUSED(r, 4, st, one, o0, lbig, fin0, 1, &x, 0, &y, 0);
    RsRates u;
    REQUIRE(rs_rates(24000, 48000, &u) == nullptr);
    const long lmax[1] = {SP_MAX_CHUNK};
    REFUSED(u, 4, st, one, o0, lmax, fin0, 1, &x, 0, &y, 0);          // 2^30 in would give 2^31 out
    REFUSED(r, 0, st, one, o0, l1, fin0, 1, &x, 0, &y, 0);
    REFUSED(r, RS_MAX_STREAMS + 1, st, one, o0, l1, fin0, 1, &x, 0, &y, 0);
    // after all of that an ordinary call still plans
    REQUIRE(rs_plan_build(r, 4, st, one, o0, l1, fin0, 1, &x, 0, &y, 0, no, &plan, next) == nullptr && plan.n == 1 && no[0] == 0);
}

int main() {
    for (int i = 0; i < 10; ++i) check_pair(PAIRS[i][0], PAIRS[i][1]);
    check_offsets_and_refusals();
    REQUIRE(g_checks > 1000);
    printf("ok\n");
    return 0;
}
