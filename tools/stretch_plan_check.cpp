// The host plan of a pool of time-stretch streams (sesameai-tts_amd/csrc/stretch_plan.h: no HIP) as a stand-alone host program, built with the
// host sanitizers by tests/test_stretch_plan_host.py.  For speeds across 500 .. 2000 permille: the emitted block counts against the definition
// (block k is out once a_k + D + 2H samples are in; everything at final), the output lengths, every refusal of include/mimi_hip.h's
// mimi_ts_pool_reset / mimi_ts_pool_feed, made with nothing planned and no state moved; the packed output and block offsets; that the carry
// never exceeds its 2,560 floats and no block reads in front of it or (open clip) behind the chunk; and a stream walked past 2^40 samples in
// large steps, whose kernel-visible numbers are those of its totals relative to the carry's base and stay inside 32 bits.  Prints "ok".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "stretch_plan.h"

static int g_checks = 0;
#define REQUIRE(cond)                                                              \
    do {                                                                           \
        ++g_checks;                                                                \
        if (!(cond)) { printf("FAILED %s (%s:%d)\n", #cond, __FILE__, __LINE__); exit(1); } \
    } while (0)

static const int PMS[9] = {500, 501, 730, 999, 1000, 1200, 1250, 1999, 2000};

// the definition's counts, by walking k (128-bit product: no trust in the header's arithmetic)
static long want_a(long k, int pm) { return (long)((__int128)k * TS_H * pm / 1000); }
static long want_emitted(long R, int pm) {          // the count e with: blocks 0 .. e - 1 are out (a_k + D + 2H <= R), block e is not
    const long T = R - (TS_D + 2 * TS_H);
    if (T < 0) return 0;
    const long e = (long)((((__int128)T + 1) * 1000 - 1) / ((__int128)TS_H * pm)) + 1;
    REQUIRE(want_a(e - 1, pm) + TS_D + 2 * TS_H <= R && want_a(e, pm) + TS_D + 2 * TS_H > R);
    return e;
}

struct Walk {                        // one stream, fed through ts_plan_build, beside its totals
    TsStream st[TS_MAX_STREAMS] = {};
    long R = 0, k = 0;
    int pm = 1000;
    void reset(int sid, int speed) {
        const int32_t ids[1] = {sid}, sp[1] = {speed};
        REQUIRE(ts_reset(4, st, ids, sp, 1) == nullptr);
        REQUIRE(st[sid].R == 0 && st[sid].k == 0 && st[sid].pm == speed);
        R = 0; k = 0; pm = speed;
    }
    void feed(int sid, long n, bool final, TsSeg* seg_out = nullptr) {
        const int32_t ids[1] = {sid}, fin[1] = {final ? 1 : 0};
        const long off[1] = {5}, len[1] = {n};
        long n_out[1] = {-1};
        const float x = 0; float y = 0;
        TsPlan plan; TsStream next[TS_MAX_STREAMS];
        REQUIRE(ts_out_count(st[sid], n, final) >= 0);
        const char* bad = ts_plan_build(4, st, ids, off, len, fin, 1, &x, &y, n_out, &plan, next);
        REQUIRE(bad == nullptr && plan.n == 1);
        const TsSeg& g = plan.seg[0];
        const long R1 = R + n;
        const long M = (long)(((__int128)R1 * 1000 + pm - 1) / pm);
        const long k1 = final ? (M + TS_H - 1) / TS_H : want_emitted(R1, pm);
        const long cnt = final ? M - k * TS_H : (k1 - k) * TS_H;
        REQUIRE(cnt >= 0 && n_out[0] == cnt && g.n_out == cnt && g.n_in == n && g.in_off == 5 && g.out_off == 0 && g.blk_off == 0);
        REQUIRE(plan.blocks == (cnt + TS_H - 1) / TS_H && plan.blocks == k1 - k);
        REQUIRE(SP_SID(g) == sid && SP_PARITY(g) == st[sid].parity && SP_FINAL(g) == (final ? 1 : 0) && TS_FRESH(g) == (k == 0 ? 1 : 0) && TS_PM(g) == pm);
        REQUIRE(next[0].parity == (st[sid].parity ^ 1) && next[0].pm == pm);
        // what the kernel sees: positions relative to the carry's base
        const long base = k >= 1 ? (want_a(k - 1, pm) - TS_D > 0 ? want_a(k - 1, pm) - TS_D : 0) : 0;
        REQUIRE(g.L == R - base && g.L >= 0 && g.L < TS_CARRY);
        REQUIRE(g.a0 == want_a(k, pm) - base && g.a0 >= 0 && TS_REM(g) == (long)((__int128)k * TS_H * pm % 1000));
        const long probe[3] = {0, (k1 - k) / 2, k1 - k - 1};
        for (int q = 0; q < 3; ++q) {
            const long i = probe[q];
            if (i < 0 || i >= k1 - k) continue;                                                    // (a call may emit nothing)
            const long a_rel = g.a0 + (TS_REM(g) + i * (long)(TS_H * TS_PM(g))) / 1000;       // the kernel's formula
            REQUIRE(a_rel == want_a(k + i, pm) - base && a_rel < (1L << 31) - 4 * TS_H);
            if (k + i >= 1) REQUIRE(a_rel - TS_D >= 0);                                            // no block reads in front of the carry
            if (!final) REQUIRE(a_rel + TS_D + 2 * TS_H <= g.L + n);                               // ... nor, open, behind the chunk
        }
        if (final) {
            REQUIRE(next[0].R == 0 && next[0].k == 0 && g.shift == 0);
            R = 0; k = 0;
        } else {
            const long nbase = k1 >= 1 ? (want_a(k1 - 1, pm) - TS_D > 0 ? want_a(k1 - 1, pm) - TS_D : 0) : 0;
            REQUIRE(g.shift == nbase - base && g.shift >= 0 && g.shift <= g.L + n);
            REQUIRE(g.L + n - g.shift == R1 - nbase && g.L + n - g.shift < TS_CARRY);             // the new carry fits
            REQUIRE(next[0].R == R1 && next[0].k == k1);
            R = R1; k = k1;
        }
        st[sid] = next[0];
        if (seg_out) *seg_out = g;
    }
};

static void check_speed(int pm) {
    const long chunks[8] = {0, 1, 7, 255, 512, 1280, 1920, 4000};
    for (int a = 0; a < 8; ++a)
        for (int b = 0; b < 8; ++b)
            for (int c = 0; c < 8; c += 3)
                for (int fin = 0; fin < 2; ++fin) {
                    Walk w; w.reset(1, pm);
                    w.feed(1, chunks[a], false); w.feed(1, chunks[b], false); w.feed(1, chunks[c], fin != 0);
                    if (fin) w.feed(1, chunks[a], true);                  // the stream is fresh again
                }
    // 1,279 samples free nothing, the 1,280th frees block 0
    { Walk w; w.reset(0, pm); TsSeg s; w.feed(0, TS_LOOK - 1, false, &s); REQUIRE(s.n_out == 0); w.feed(0, 1, false, &s); REQUIRE(s.n_out == TS_H); }
    // final alone on a fresh stream gives nothing; one sample gives ceil(1000 / pm) outputs
    { Walk w; w.reset(0, pm); TsSeg s; w.feed(0, 0, true, &s); REQUIRE(s.n_out == 0); w.feed(0, 1, true, &s); REQUIRE(s.n_out == (1000 + pm - 1) / pm); }
    // past 2^40 samples in steps of about 2^28: the kernel's numbers never grow
    {
        Walk w; w.reset(2, pm);
        long step = (1L << 28) + 12345;
        while (w.R < (1L << 40) + 7) { w.feed(2, step, false); step = (1L << 28) + (step * 7 + 3) % 100003; }
        TsSeg s; w.feed(2, 1920, false, &s);
        REQUIRE(s.L < TS_CARRY && s.a0 < TS_CARRY);
        w.feed(2, 0, true, &s);
        REQUIRE(s.n_out >= 0 && s.n_out <= 2 * TS_CARRY);
    }
}

static void check_offsets_and_refusals() {
    TsStream st[TS_MAX_STREAMS] = {};
    const int32_t all[4] = {0, 1, 2, 3}, sp[4] = {1200, 500, 2000, 1000};
    REQUIRE(ts_reset(4, st, all, sp, 4) == nullptr);
    const float x = 0; float y = 0;
    TsPlan plan; TsStream next[TS_MAX_STREAMS];
    // four streams, two of which emit nothing: offsets are packed by samples and by blocks
    const int32_t ids[4] = {3, 0, 2, 1}, fin[4] = {0, 1, 0, 1};
    const long off[4] = {0, 100, 5000, 9000}, len[4] = {5, 1200, 0, 300};
    long n_out[4];
    REQUIRE(ts_plan_build(4, st, ids, off, len, fin, 4, &x, &y, n_out, &plan, next) == nullptr && plan.n == 4);
    REQUIRE(n_out[0] == 0 && n_out[1] == 1000 && n_out[2] == 0 && n_out[3] == 600);
    REQUIRE(plan.seg[0].out_off == 0 && plan.seg[1].out_off == 0 && plan.seg[2].out_off == 1000 && plan.seg[3].out_off == 1000);
    REQUIRE(plan.seg[0].blk_off == 0 && plan.seg[1].blk_off == 0 && plan.seg[2].blk_off == 2 && plan.seg[3].blk_off == 2 && plan.blocks == 4);
    for (int i = 0; i < 4; ++i) REQUIRE(plan.seg[i].in_off == off[i] && SP_SID(plan.seg[i]) == ids[i] && TS_PM(plan.seg[i]) == sp[ids[i]]);
    REQUIRE(next[0].R == 5 && next[0].k == 0 && next[1].R == 0 && next[2].R == 0 && next[3].R == 0);
    for (int i = 4; i < TS_MAX_STREAMS; ++i) REQUIRE(plan.seg[i].n_in == 0 && plan.seg[i].n_out == 0);

    const int32_t one[1] = {0}, fin0[1] = {0};
    const long o0[1] = {0}, l1[1] = {10};
    long no[4];
#define REFUSED(...)                                                                                   \
    do {                                                                                               \
        plan.n = 7;                                                                                    \
        REQUIRE(ts_plan_build(__VA_ARGS__, no, &plan, next) != nullptr && plan.n == 0 && plan.blocks == 0); \
    } while (0)
    REFUSED(4, st, nullptr, o0, l1, fin0, 1, &x, &y);
    REFUSED(4, st, one, nullptr, l1, fin0, 1, &x, &y);
    REFUSED(4, st, one, o0, nullptr, fin0, 1, &x, &y);
    REFUSED(4, st, one, o0, l1, nullptr, 1, &x, &y);
    REFUSED(4, st, one, o0, l1, fin0, 1, nullptr, &y);
    REFUSED(4, st, one, o0, l1, fin0, 1, &x, nullptr);
    REFUSED(4, nullptr, one, o0, l1, fin0, 1, &x, &y);
    plan.n = 7;
    REQUIRE(ts_plan_build(4, st, one, o0, l1, fin0, 1, &x, &y, nullptr, &plan, next) != nullptr && plan.n == 0);
    REFUSED(4, st, one, o0, l1, fin0, 0, &x, &y);
    REFUSED(4, st, ids, off, len, fin, 5, &x, &y);
    const int32_t dup[2] = {1, 1}, far[1] = {4}, neg[1] = {-1};
    const long o2[2] = {0, 0}, l2[2] = {1, 1};
    const int32_t f2[2] = {0, 0};
    REFUSED(4, st, dup, o2, l2, f2, 2, &x, &y);
    REFUSED(4, st, far, o0, l1, fin0, 1, &x, &y);
    REFUSED(4, st, neg, o0, l1, fin0, 1, &x, &y);
    const long lneg[1] = {-1}, oneg[1] = {-1}, lbig[1] = {SP_MAX_CHUNK + 1}, lmax[1] = {SP_MAX_CHUNK};
    REFUSED(4, st, one, o0, lneg, fin0, 1, &x, &y);
    REFUSED(4, st, one, oneg, l1, fin0, 1, &x, &y);
    REFUSED(4, st, one, o0, lbig, fin0, 1, &x, &y);
    const int32_t slow[1] = {1}, fin1[1] = {1};
    REFUSED(4, st, slow, o0, lmax, fin1, 1, &x, &y);                     // 2^30 in at half speed would give 2^31 out
    REQUIRE(ts_plan_build(4, st, one, o0, lmax, fin0, 1, &x, &y, no, &plan, next) == nullptr);       // ... at 1.2 x it is legal
    TsStream big[TS_MAX_STREAMS] = {};
    big[0].pm = 1000; big[0].R = SP_MAX_TOTAL - 5; big[0].k = ts_emitted(big[0].R, 1000, 0);
    REFUSED(4, big, one, o0, l1, fin0, 1, &x, &y);                       // a stream past 2^48 samples
    big[0].pm = 499;  big[0].R = 0; big[0].k = 0;
    REFUSED(4, big, one, o0, l1, fin0, 1, &x, &y);
    REFUSED(0, st, one, o0, l1, fin0, 1, &x, &y);
    REFUSED(TS_MAX_STREAMS + 1, st, one, o0, l1, fin0, 1, &x, &y);
    // resets: refused as a whole, nothing moved
    TsStream keep[TS_MAX_STREAMS];
    st[0].R = 77; st[0].k = 0; st[1].R = 99;
    memcpy(keep, st, sizeof(st));
    const int32_t two[2] = {0, 1}, bad_lo[2] = {1200, 499}, bad_hi[2] = {2001, 1200}, good[2] = {1200, 800};
    REQUIRE(ts_reset(4, st, two, bad_lo, 2) != nullptr && memcmp(keep, st, sizeof(st)) == 0);
    REQUIRE(ts_reset(4, st, two, bad_hi, 2) != nullptr && memcmp(keep, st, sizeof(st)) == 0);
    REQUIRE(ts_reset(4, st, dup, good, 2) != nullptr && memcmp(keep, st, sizeof(st)) == 0);
    REQUIRE(ts_reset(4, st, far, good, 1) != nullptr && ts_reset(4, st, neg, good, 1) != nullptr && memcmp(keep, st, sizeof(st)) == 0);
    REQUIRE(ts_reset(4, st, nullptr, good, 1) != nullptr && ts_reset(4, st, two, nullptr, 2) != nullptr && ts_reset(4, nullptr, two, good, 2) != nullptr);
    REQUIRE(ts_reset(4, st, two, good, 0) != nullptr && ts_reset(4, st, two, good, 5) != nullptr && memcmp(keep, st, sizeof(st)) == 0);
    REQUIRE(ts_reset(4, st, two, good, 2) == nullptr && st[0].R == 0 && st[0].pm == 1200 && st[1].R == 0 && st[1].pm == 800);
    // after all of that an ordinary call still plans
    REQUIRE(ts_plan_build(4, st, one, o0, l1, fin0, 1, &x, &y, no, &plan, next) == nullptr && plan.n == 1 && no[0] == 0);
}

int main() {
    for (int i = 0; i < 9; ++i) check_speed(PMS[i]);
    check_offsets_and_refusals();
    REQUIRE(g_checks > 1000);
    printf("ok\n");
    return 0;
}
