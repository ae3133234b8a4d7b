// The host plan of a pool of voice-activity streams (sesameai-tts_amd/csrc/vad_plan.h: no HIP) as a stand-alone host program, built with the
// host sanitizers by tests/test_vad_plan_host.py.  The frame counts against the definition (frame k is judged once (k + 1) F samples are in;
// a partial frame never, final or not); every refusal of include/mimi_hip.h's mimi_vad_pool_reset / mimi_vad_pool_feed, made with nothing
// planned and no state moved; the packed frame offsets; that the carry never exceeds 879 samples, that no frame reads in front of the
// call's base or behind the chunk; and a stream walked past 2^40 samples in large steps, whose kernel-visible numbers are those of its
// totals relative to the carry's base and stay small.  Prints "ok".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "vad_plan.h"

static int g_checks = 0;
#define REQUIRE(cond)                                                              \
    do {                                                                           \
        ++g_checks;                                                                \
        if (!(cond)) { printf("FAILED %s (%s:%d)\n", #cond, __FILE__, __LINE__); exit(1); } \
    } while (0)

static float g_in[4];
static uint8_t g_flags[4];
static int16_t g_lag[4];
static long g_power[4], g_floor[4];

struct Walk {                        // one stream, fed through vad_plan_build, beside its totals
    VadStream st[VAD_MAX_STREAMS] = {};
    long R = 0, k = 0;
    VadParams prm = VAD_DEFAULT_PARAMS;
    void reset(int sid, VadParams p) {
        const int32_t ids[1] = {sid};
        REQUIRE(vad_reset(4, st, ids, &p, 1) == nullptr);
        REQUIRE(st[sid].R == 0 && st[sid].k == 0 && st[sid].touched == 0 && st[sid].prm.hang == p.hang && st[sid].prm.n_min == p.n_min);
        R = 0; k = 0; prm = p;
    }
    void feed(int sid, long n, bool final, VadSeg* seg_out = nullptr) {
        const int32_t ids[1] = {sid}, fin[1] = {final ? 1 : 0};
        const long off[1] = {5}, len[1] = {n};
        long nfr[1] = {-1};
        VadPlan plan; VadStream next[VAD_MAX_STREAMS];
        const char* bad = vad_plan_build(4, st, ids, off, len, fin, 1, g_in, 0, g_flags, g_lag, g_power, g_floor, nfr, &plan, next);
        REQUIRE(bad == nullptr && plan.n == 1);
        const VadSeg& g = plan.seg[0];
        const long R1 = R + n, k1 = R1 / VAD_F, nf = k1 - k;
        REQUIRE(nf >= 0 && nfr[0] == nf && g.nf == nf && plan.frames == nf && g.f_off == 0 && g.n_in == n && g.in_off == 5);
        REQUIRE(vad_frame_count(st[sid], n) == nf);
        REQUIRE(SP_SID(g) == sid && SP_PARITY(g) == st[sid].parity && SP_FINAL(g) == (final ? 1 : 0) && g.k0 == k);
        REQUIRE(VAD_ON(g) == prm.on_q4 && VAD_OFF(g) == prm.off_q4 && VAD_MIN_ON(g) == prm.min_on && VAD_HANG(g) == prm.hang && g.hold == prm.hold && g.n_min == prm.n_min);
        REQUIRE(next[0].parity == (st[sid].parity ^ 1) && next[0].touched == 1 && next[0].prm.hang == prm.hang);
        // what the kernels see: positions relative to base = k F - 640; `lead` rule zeros, the carry, the chunk
        const long base = k * VAD_F - VAD_HIST;
        const long lead = base < 0 ? -base : 0;
        REQUIRE(VAD_LEAD(g) == lead && g.Lc == R - (base > 0 ? base : 0) && g.Lc >= 0 && g.Lc < VAD_CARRY && g.Lc <= VAD_HIST + VAD_F - 1);
        REQUIRE(lead + g.Lc + n == R1 - base);
        if (nf > 0) REQUIRE((nf - 1) * VAD_F + VAD_SPAN <= lead + g.Lc + n);                       // the last frame's span ends inside the chunk
        REQUIRE(nf * VAD_F + VAD_SPAN > lead + g.Lc + n);                                          // ... and the next frame's does not
        if (final) {
            REQUIRE(next[0].R == 0 && next[0].k == 0);
            R = 0; k = 0;
        } else {
            REQUIRE(next[0].R == R1 && next[0].k == k1);
            const long nbase = k1 * VAD_F - VAD_HIST;
            REQUIRE(vad_carry_len(R1) == R1 - (nbase > 0 ? nbase : 0) && vad_carry_len(R1) <= 879);
            R = R1; k = k1;
        }
        st[sid] = next[0];
        if (seg_out) *seg_out = g;
    }
};

static void check_counts() {
    const long chunks[9] = {0, 1, 7, 239, 240, 241, 880, 1920, 4000};
    for (int a = 0; a < 9; ++a)
        for (int b = 0; b < 9; ++b)
            for (int c = 0; c < 9; c += 2)
                for (int fin = 0; fin < 2; ++fin) {
                    Walk w; w.reset(1, VAD_DEFAULT_PARAMS);
                    w.feed(1, chunks[a], false); w.feed(1, chunks[b], false); w.feed(1, chunks[c], fin != 0);
                    if (fin) w.feed(1, chunks[a], true);                  // the stream is fresh again
                }
    // 239 samples judge nothing, the 240th completes frame 0; the carry peaks at 879
    { Walk w; w.reset(0, VAD_DEFAULT_PARAMS); VadSeg s; w.feed(0, 239, false, &s); REQUIRE(s.nf == 0); w.feed(0, 1, false, &s); REQUIRE(s.nf == 1 && s.Lc == 239);
      w.feed(0, 719, false, &s); REQUIRE(s.nf == 2 && s.Lc == 240); w.feed(0, 0, false, &s); REQUIRE(s.Lc == 879 && VAD_LEAD(s) == 0 && s.k0 == 3); }
    // final alone on a fresh stream judges nothing; a final with a partial frame discards it
    { Walk w; w.reset(0, VAD_DEFAULT_PARAMS); VadSeg s; w.feed(0, 0, true, &s); REQUIRE(s.nf == 0); w.feed(0, 500, true, &s); REQUIRE(s.nf == 2); w.feed(0, 10, false, &s); REQUIRE(s.Lc == 0 && s.k0 == 0); }
    // past 2^40 samples in steps of about 2^28: the kernels' numbers never grow
    {
        Walk w; w.reset(2, VadParams{4095, 16, 1000, 10000, 10000, 0, 1L << 40});
        long step = (1L << 28) + 12345;
        while (w.R < (1L << 40) + 7) { w.feed(2, step, false); step = (1L << 28) + (step * 7 + 3) % 100003; }
        VadSeg s; w.feed(2, 1920, false, &s);
        REQUIRE(s.Lc < VAD_CARRY && s.nf <= 9 && s.k0 > (1L << 32) && VAD_LEAD(s) == 0);
        w.feed(2, 0, true, &s);
        REQUIRE(s.nf == 0);
    }
}

static void check_offsets_and_refusals() {
    VadStream st[VAD_MAX_STREAMS] = {};
    const int32_t all[4] = {0, 1, 2, 3};
    VadParams four[4] = {VAD_DEFAULT_PARAMS, VAD_DEFAULT_PARAMS, VAD_DEFAULT_PARAMS, VAD_DEFAULT_PARAMS};
    four[2].hang = 20; four[3].n_min = 1;
    REQUIRE(vad_reset(4, st, all, four, 4) == nullptr);
    VadPlan plan; VadStream next[VAD_MAX_STREAMS];
    // four streams, two of which judge nothing: offsets are packed by frames
    const int32_t ids[4] = {3, 0, 2, 1}, fin[4] = {0, 1, 0, 1};
    const long off[4] = {0, 100, 5000, 9000}, len[4] = {5, 1200, 0, 490};
    long nfr[4];
    REQUIRE(vad_plan_build(4, st, ids, off, len, fin, 4, g_in, 1, g_flags, g_lag, g_power, g_floor, nfr, &plan, next) == nullptr && plan.n == 4);
    REQUIRE(nfr[0] == 0 && nfr[1] == 5 && nfr[2] == 0 && nfr[3] == 2 && plan.frames == 7);
    REQUIRE(plan.seg[0].f_off == 0 && plan.seg[1].f_off == 0 && plan.seg[2].f_off == 5 && plan.seg[3].f_off == 5);
    for (int i = 0; i < 4; ++i) REQUIRE(plan.seg[i].in_off == off[i] && SP_SID(plan.seg[i]) == ids[i] && VAD_HANG(plan.seg[i]) == four[ids[i]].hang);
    REQUIRE(plan.seg[0].n_min == 1 && next[0].R == 5 && next[0].k == 0 && next[1].R == 0 && next[2].R == 0 && next[3].R == 0);
    for (int i = 4; i < VAD_MAX_STREAMS; ++i) REQUIRE(plan.seg[i].n_in == 0 && plan.seg[i].nf == 0);

    const int32_t one[1] = {0}, fin0[1] = {0};
    const long o0[1] = {0}, l1[1] = {10};
    long no[4];
    VadStream keep[VAD_MAX_STREAMS];
    st[0].R = 77; st[1].R = 99;
    memcpy(keep, st, sizeof(st));
#define REFUSED(...)                                                                                   \
    do {                                                                                               \
        plan.n = 7;                                                                                    \
        REQUIRE(vad_plan_build(__VA_ARGS__, &plan, next) != nullptr && plan.n == 0 && plan.frames == 0 && memcmp(keep, st, sizeof(st)) == 0); \
    } while (0)
    REFUSED(4, st, nullptr, o0, l1, fin0, 1, g_in, 0, g_flags, g_lag, g_power, g_floor, no);
    REFUSED(4, st, one, nullptr, l1, fin0, 1, g_in, 0, g_flags, g_lag, g_power, g_floor, no);
    REFUSED(4, st, one, o0, nullptr, fin0, 1, g_in, 0, g_flags, g_lag, g_power, g_floor, no);
    REFUSED(4, st, one, o0, l1, nullptr, 1, g_in, 0, g_flags, g_lag, g_power, g_floor, no);
    REFUSED(4, st, one, o0, l1, fin0, 1, nullptr, 0, g_flags, g_lag, g_power, g_floor, no);
    REFUSED(4, st, one, o0, l1, fin0, 1, g_in, 0, nullptr, g_lag, g_power, g_floor, no);
    REFUSED(4, st, one, o0, l1, fin0, 1, g_in, 0, g_flags, nullptr, g_power, g_floor, no);
    REFUSED(4, st, one, o0, l1, fin0, 1, g_in, 0, g_flags, g_lag, nullptr, g_floor, no);
    REFUSED(4, st, one, o0, l1, fin0, 1, g_in, 0, g_flags, g_lag, g_power, nullptr, no);
    REFUSED(4, st, one, o0, l1, fin0, 1, g_in, 0, g_flags, g_lag, g_power, g_floor, nullptr);
    REFUSED(4, nullptr, one, o0, l1, fin0, 1, g_in, 0, g_flags, g_lag, g_power, g_floor, no);
    REFUSED(4, st, one, o0, l1, fin0, 1, g_in, 2, g_flags, g_lag, g_power, g_floor, no);                      // an unknown format
    REFUSED(4, st, one, o0, l1, fin0, 1, (const char*)g_in + 2, 0, g_flags, g_lag, g_power, g_floor, no);     // misaligned buffers
    REFUSED(4, st, one, o0, l1, fin0, 1, (const char*)g_in + 1, 1, g_flags, g_lag, g_power, g_floor, no);
    REFUSED(4, st, one, o0, l1, fin0, 1, g_in, 0, g_flags, (const char*)g_lag + 1, g_power, g_floor, no);
    REFUSED(4, st, one, o0, l1, fin0, 1, g_in, 0, g_flags, g_lag, (const char*)g_power + 4, g_floor, no);
    REFUSED(4, st, one, o0, l1, fin0, 1, g_in, 0, g_flags, g_lag, g_power, (const char*)g_floor + 4, no);
    REQUIRE(vad_plan_build(4, st, one, o0, l1, fin0, 1, (const char*)g_in + 2, 1, g_flags + 1, g_lag, g_power, g_floor, no, &plan, next) == nullptr);
    REFUSED(4, st, one, o0, l1, fin0, 0, g_in, 0, g_flags, g_lag, g_power, g_floor, no);
    REFUSED(4, st, ids, off, len, fin, 5, g_in, 0, g_flags, g_lag, g_power, g_floor, no);
    const int32_t dup[2] = {1, 1}, far[1] = {4}, neg[1] = {-1};
    const long o2[2] = {0, 0}, l2[2] = {1, 1};
    const int32_t f2[2] = {0, 0};
    REFUSED(4, st, dup, o2, l2, f2, 2, g_in, 0, g_flags, g_lag, g_power, g_floor, no);
    REFUSED(4, st, far, o0, l1, fin0, 1, g_in, 0, g_flags, g_lag, g_power, g_floor, no);
    REFUSED(4, st, neg, o0, l1, fin0, 1, g_in, 0, g_flags, g_lag, g_power, g_floor, no);
    const long lneg[1] = {-1}, oneg[1] = {-1}, lbig[1] = {SP_MAX_CHUNK + 1}, lmax[1] = {SP_MAX_CHUNK};
    REFUSED(4, st, one, o0, lneg, fin0, 1, g_in, 0, g_flags, g_lag, g_power, g_floor, no);
    REFUSED(4, st, one, oneg, l1, fin0, 1, g_in, 0, g_flags, g_lag, g_power, g_floor, no);
    REFUSED(4, st, one, o0, lbig, fin0, 1, g_in, 0, g_flags, g_lag, g_power, g_floor, no);
    REQUIRE(vad_plan_build(4, st, one, o0, lmax, fin0, 1, g_in, 0, g_flags, g_lag, g_power, g_floor, no, &plan, next) == nullptr && no[0] == (77 + SP_MAX_CHUNK) / VAD_F);
    REFUSED(0, st, one, o0, l1, fin0, 1, g_in, 0, g_flags, g_lag, g_power, g_floor, no);
    REFUSED(VAD_MAX_STREAMS + 1, st, one, o0, l1, fin0, 1, g_in, 0, g_flags, g_lag, g_power, g_floor, no);
    {
        VadStream big[VAD_MAX_STREAMS] = {};
        big[0].prm = VAD_DEFAULT_PARAMS; big[0].R = SP_MAX_TOTAL - 5; big[0].k = big[0].R / VAD_F;
        plan.n = 7;
        REQUIRE(vad_plan_build(4, big, one, o0, l1, fin0, 1, g_in, 0, g_flags, g_lag, g_power, g_floor, no, &plan, next) != nullptr && plan.n == 0);      // past 2^48 samples
        big[0].R = 0; big[0].k = 0; big[0].prm.hang = 0;
        REQUIRE(vad_plan_build(4, big, one, o0, l1, fin0, 1, g_in, 0, g_flags, g_lag, g_power, g_floor, no, &plan, next) != nullptr && plan.n == 0);
    }
    // resets: refused as a whole, nothing moved; every parameter at both ends of its range
    const int32_t two[2] = {0, 1};
    VadParams good[2] = {VadParams{4095, 16, 1000, 10000, 10000, 0, 1L << 40}, VadParams{16, 16, 1, 1, 0, 0, 1}};
    const VadParams bad[11] = {{4096, 48, 8, 70, 30, 0, 1}, {128, 15, 8, 70, 30, 0, 1}, {40, 48, 8, 70, 30, 0, 1}, {128, 48, 0, 70, 30, 0, 1},
                               {128, 48, 1001, 70, 30, 0, 1}, {128, 48, 8, 0, 30, 0, 1}, {128, 48, 8, 10001, 30, 0, 1}, {128, 48, 8, 70, -1, 0, 1},
                               {128, 48, 8, 70, 10001, 0, 1}, {128, 48, 8, 70, 30, 0, 0}, {128, 48, 8, 70, 30, 0, (1L << 40) + 1}};
    for (int i = 0; i < 11; ++i) {
        VadParams mix[2] = {good[0], bad[i]};
        REQUIRE(vad_params_bad(bad[i]) != nullptr);
        REQUIRE(vad_reset(4, st, two, mix, 2) != nullptr && memcmp(keep, st, sizeof(st)) == 0);
    }
    REQUIRE(vad_reset(4, st, dup, good, 2) != nullptr && memcmp(keep, st, sizeof(st)) == 0);
    REQUIRE(vad_reset(4, st, far, good, 1) != nullptr && vad_reset(4, st, neg, good, 1) != nullptr && memcmp(keep, st, sizeof(st)) == 0);
    REQUIRE(vad_reset(4, st, nullptr, good, 1) != nullptr && vad_reset(4, st, two, nullptr, 2) != nullptr && vad_reset(4, nullptr, two, good, 2) != nullptr);
    REQUIRE(vad_reset(4, st, two, good, 0) != nullptr && vad_reset(4, st, two, good, 5) != nullptr && memcmp(keep, st, sizeof(st)) == 0);
    REQUIRE(vad_reset(4, st, two, good, 2) == nullptr && st[0].R == 0 && st[0].prm.hang == 10000 && st[1].R == 0 && st[1].prm.n_min == 1 && st[1].touched == 0);
    // after all of that an ordinary call still plans, with the packed fields whole at the ranges' upper ends
    REQUIRE(vad_plan_build(4, st, one, o0, l1, fin0, 1, g_in, 0, g_flags, g_lag, g_power, g_floor, no, &plan, next) == nullptr && plan.n == 1 && no[0] == 0);
    REQUIRE(VAD_ON(plan.seg[0]) == 4095 && VAD_OFF(plan.seg[0]) == 16 && VAD_MIN_ON(plan.seg[0]) == 1000 && VAD_HANG(plan.seg[0]) == 10000 && plan.seg[0].hold == 10000);
}

int main() {
    check_counts();
    check_offsets_and_refusals();
    REQUIRE(g_checks > 1000);
    printf("ok\n");
    return 0;
}
