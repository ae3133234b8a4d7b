// The host plan of a pool of loudness-meter streams (sesameai-tts_amd/csrc/loudness_plan.h: no HIP) as a stand-alone host program, built with
// the host sanitizers by tests/test_loudness_plan_host.py.  The hop counts against the definition (hop k is measured once (k + 1) H samples
// are in; a partial hop never, final or not); every refusal of include/mimi_hip.h's mimi_ld_pool_create / reset / feed / integrate and of
// mimi_fin_segments_ld's own arguments, made with nothing planned and no state moved, the texts of the shared spine byte for byte; the
// packed hop offsets; that the carry never exceeds 2910 samples, that no hop reads in front of the call's base or behind the chunk, over a
// sweep of R around multiples of H; that `final` leaves the stream fresh; and a stream walked past 2^40 samples in large steps, whose
// kernel-visible numbers stay small.  Prints "ok".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "loudness_plan.h"

static int g_checks = 0;
#define REQUIRE(cond)                                                              \
    do {                                                                           \
        ++g_checks;                                                                \
        if (!(cond)) { printf("FAILED %s (%s:%d)\n", #cond, __FILE__, __LINE__); exit(1); } \
    } while (0)
#define SAYS(call, text)                                                           \
    do {                                                                           \
        const char* said_ = (call);                                                \
        REQUIRE(said_ != nullptr && strcmp(said_, text) == 0);                     \
    } while (0)

static float g_in[4];
static long g_energy[4];

struct Walk {                        // one stream, fed through ld_plan_build, beside its totals
    LdStream st[LD_MAX_STREAMS] = {};
    long R = 0, k = 0;
    void reset(int sid) {
        const int32_t ids[1] = {sid};
        REQUIRE(ld_reset(4, st, ids, 1) == nullptr);
        REQUIRE(st[sid].R == 0 && st[sid].k == 0 && st[sid].touched == 0);
        R = 0; k = 0;
    }
    void feed(int sid, long n, bool final, LdSeg* seg_out = nullptr) {
        const int32_t ids[1] = {sid}, fin[1] = {final ? 1 : 0};
        const long off[1] = {5}, len[1] = {n};
        long nh[1] = {-1};
        LdPlan plan; LdStream next[LD_MAX_STREAMS];
        const char* bad = ld_plan_build(4, st, ids, off, len, fin, 1, g_in, 0, g_energy, nh, &plan, next);
        REQUIRE(bad == nullptr && plan.n == 1);
        const LdSeg& g = plan.seg[0];
        const long R1 = R + n, k1 = R1 / LD_H, nf = k1 - k;
        REQUIRE(nf >= 0 && nh[0] == nf && g.nf == nf && plan.hops == nf && g.f_off == 0 && g.n_in == n && g.in_off == 5 && g.pad == 0);
        REQUIRE(ld_hop_count(st[sid], n) == nf);
        REQUIRE(SP_SID(g) == sid && SP_PARITY(g) == st[sid].parity && SP_FINAL(g) == (final ? 1 : 0) && g.k0 == k);
        REQUIRE(next[0].parity == (st[sid].parity ^ 1) && next[0].touched == 1);
        // what the kernels see: positions relative to base = k H - 511; `lead` rule zeros, the carry, the chunk
        const long base = k * LD_H - LD_HIST;
        const long lead = base < 0 ? -base : 0;
        REQUIRE(LD_LEAD(g) == lead && g.Lc == R - (base > 0 ? base : 0) && g.Lc >= 0 && g.Lc < LD_CARRY && g.Lc <= LD_HIST + LD_H - 1);
        REQUIRE((g.Lc == 0) == (R == 0));                                                           // the kernels read "fresh" off the carry
        REQUIRE(lead + g.Lc + n == R1 - base);
        if (nf > 0) REQUIRE((nf - 1) * LD_H + LD_SPAN <= lead + g.Lc + n);                          // the last hop's span ends inside the chunk
        REQUIRE(nf * LD_H + LD_SPAN > lead + g.Lc + n);                                             // ... and the next hop's does not
        if (final) {
            REQUIRE(next[0].R == 0 && next[0].k == 0);
            R = 0; k = 0;
        } else {
            REQUIRE(next[0].R == R1 && next[0].k == k1);
            const long nbase = k1 * LD_H - LD_HIST;
            REQUIRE(ld_carry_len(R1) == R1 - (nbase > 0 ? nbase : 0) && ld_carry_len(R1) <= 2910);
            R = R1; k = k1;
        }
        st[sid] = next[0];
        if (seg_out) *seg_out = g;
    }
};

static void check_counts() {
    const long chunks[11] = {0, 1, 7, 510, 511, 512, 2399, 2400, 2401, 4800, 19200};
    for (int a = 0; a < 11; ++a)
        for (int b = 0; b < 11; ++b)
            for (int c = 0; c < 11; c += 2)
                for (int fin = 0; fin < 2; ++fin) {
                    Walk w; w.reset(1);
                    w.feed(1, chunks[a], false); w.feed(1, chunks[b], false); w.feed(1, chunks[c], fin != 0);
                    if (fin) w.feed(1, chunks[a], true);                  // the stream is fresh again
                }
    // a sweep of R around the multiples of H: R = m H + d reached in one step, then one more sample, then the rest of a hop
    for (int m = 0; m < 5; ++m)
        for (int d = -3; d <= 3; ++d) {
            const long R = (long)m * LD_H + d;
            if (R < 0) continue;
            Walk w; w.reset(2);
            LdSeg s;
            w.feed(2, R, false, &s); REQUIRE(s.nf == R / LD_H);
            w.feed(2, 1, false, &s); REQUIRE(s.nf == ((R + 1) % LD_H == 0 ? 1 : 0) && s.Lc == (R < LD_HIST + R % LD_H ? R : LD_HIST + R % LD_H));
            w.feed(2, LD_H - 1, false, &s); REQUIRE(s.nf == (R + LD_H) / LD_H - (R + 1) / LD_H);
            REQUIRE(w.k == (R + LD_H) / LD_H && w.R == R + LD_H);
        }
    // 2399 samples measure nothing, the 2400th completes hop 0; the carry peaks at 2910
    { Walk w; w.reset(0); LdSeg s; w.feed(0, 2399, false, &s); REQUIRE(s.nf == 0 && s.Lc == 0 && LD_LEAD(s) == 511);
      w.feed(0, 1, false, &s); REQUIRE(s.nf == 1 && s.Lc == 2399 && LD_LEAD(s) == 511);
      w.feed(0, 2399, false, &s); REQUIRE(s.nf == 0 && s.Lc == 511 && LD_LEAD(s) == 0 && s.k0 == 1);
      w.feed(0, 0, false, &s); REQUIRE(s.Lc == 2910 && s.k0 == 1); }
    // final alone on a fresh stream measures nothing; a final with a partial hop discards it
    { Walk w; w.reset(0); LdSeg s; w.feed(0, 0, true, &s); REQUIRE(s.nf == 0); w.feed(0, 5000, true, &s); REQUIRE(s.nf == 2); w.feed(0, 10, false, &s); REQUIRE(s.Lc == 0 && s.k0 == 0); }
    // past 2^40 samples in steps of about 2^28: the kernels' numbers never grow
    {
        Walk w; w.reset(2);
        long step = (1L << 28) + 12345;
        while (w.R < (1L << 40) + 7) { w.feed(2, step, false); step = (1L << 28) + (step * 7 + 3) % 100003; }
        LdSeg s; w.feed(2, 19200, false, &s);
        REQUIRE(s.Lc < LD_CARRY && s.nf <= 9 && s.k0 > (1L << 28) && LD_LEAD(s) == 0);
        w.feed(2, 0, true, &s);
        REQUIRE(s.nf == 0);
    }
}

static void check_offsets_and_refusals() {
    LdStream st[LD_MAX_STREAMS] = {};
    const int32_t all[4] = {0, 1, 2, 3};
    REQUIRE(ld_reset(4, st, all, 4) == nullptr);
    LdPlan plan; LdStream next[LD_MAX_STREAMS];
    // four streams, two of which measure nothing: offsets are packed by hops
    const int32_t ids[4] = {3, 0, 2, 1}, fin[4] = {0, 1, 0, 1};
    const long off[4] = {0, 100, 50000, 90000}, len[4] = {5, 12000, 0, 4900};
    long nh[4];
    REQUIRE(ld_plan_build(4, st, ids, off, len, fin, 4, g_in, 1, g_energy, nh, &plan, next) == nullptr && plan.n == 4);
    REQUIRE(nh[0] == 0 && nh[1] == 5 && nh[2] == 0 && nh[3] == 2 && plan.hops == 7);
    REQUIRE(plan.seg[0].f_off == 0 && plan.seg[1].f_off == 0 && plan.seg[2].f_off == 5 && plan.seg[3].f_off == 5);
    for (int i = 0; i < 4; ++i) REQUIRE(plan.seg[i].in_off == off[i] && SP_SID(plan.seg[i]) == ids[i]);
    REQUIRE(next[0].R == 5 && next[0].k == 0 && next[1].R == 0 && next[2].R == 0 && next[3].R == 0);
    for (int i = 4; i < LD_MAX_STREAMS; ++i) REQUIRE(plan.seg[i].n_in == 0 && plan.seg[i].nf == 0 && plan.seg[i].sid == 0);

    const int32_t one[1] = {0}, fin0[1] = {0};
    const long o0[1] = {0}, l1[1] = {10};
    long no[4];
    LdStream keep[LD_MAX_STREAMS];
    st[0].R = 77; st[1].R = 99;
    memcpy(keep, st, sizeof(st));
#define REFUSED(text, ...)                                                                             \
    do {                                                                                               \
        plan.n = 7;                                                                                    \
        SAYS(ld_plan_build(__VA_ARGS__, &plan, next), text);                                           \
        REQUIRE(plan.n == 0 && plan.hops == 0 && memcmp(keep, st, sizeof(st)) == 0);                   \
    } while (0)
    REFUSED("null pointer", 4, st, nullptr, o0, l1, fin0, 1, g_in, 0, g_energy, no);
    REFUSED("null pointer", 4, st, one, nullptr, l1, fin0, 1, g_in, 0, g_energy, no);
    REFUSED("null pointer", 4, st, one, o0, nullptr, fin0, 1, g_in, 0, g_energy, no);
    REFUSED("null pointer", 4, st, one, o0, l1, nullptr, 1, g_in, 0, g_energy, no);
    REFUSED("null pointer", 4, st, one, o0, l1, fin0, 1, nullptr, 0, g_energy, no);
    REFUSED("null pointer", 4, st, one, o0, l1, fin0, 1, g_in, 0, nullptr, no);
    REFUSED("null pointer", 4, st, one, o0, l1, fin0, 1, g_in, 0, g_energy, nullptr);
    REFUSED("null pointer", 4, nullptr, one, o0, l1, fin0, 1, g_in, 0, g_energy, no);
    REFUSED("unknown input format", 4, st, one, o0, l1, fin0, 1, g_in, 2, g_energy, no);
    REFUSED("a misaligned buffer", 4, st, one, o0, l1, fin0, 1, (const char*)g_in + 2, 0, g_energy, no);
    REFUSED("a misaligned buffer", 4, st, one, o0, l1, fin0, 1, (const char*)g_in + 1, 1, g_energy, no);
    REFUSED("a misaligned buffer", 4, st, one, o0, l1, fin0, 1, g_in, 0, (const char*)g_energy + 4, no);
    REQUIRE(ld_plan_build(4, st, one, o0, l1, fin0, 1, (const char*)g_in + 2, 1, g_energy, no, &plan, next) == nullptr);
    // the shared spine's texts, byte for byte
    REFUSED("stream list: need 1 .. n_streams ids", 4, st, one, o0, l1, fin0, 0, g_in, 0, g_energy, no);
    REFUSED("stream list: need 1 .. n_streams ids", 4, st, ids, off, len, fin, 5, g_in, 0, g_energy, no);
    const int32_t dup[2] = {1, 1}, far[1] = {4}, neg[1] = {-1};
    const long o2[2] = {0, 0}, l2[2] = {1, 1};
    const int32_t f2[2] = {0, 0};
    REFUSED("duplicate stream id in one call", 4, st, dup, o2, l2, f2, 2, g_in, 0, g_energy, no);
    REFUSED("stream id outside [0, n_streams)", 4, st, far, o0, l1, fin0, 1, g_in, 0, g_energy, no);
    REFUSED("stream id outside [0, n_streams)", 4, st, neg, o0, l1, fin0, 1, g_in, 0, g_energy, no);
    const long lneg[1] = {-1}, oneg[1] = {-1}, lbig[1] = {SP_MAX_CHUNK + 1}, lmax[1] = {SP_MAX_CHUNK};
    REFUSED("a chunk of negative length", 4, st, one, o0, lneg, fin0, 1, g_in, 0, g_energy, no);
    REFUSED("a chunk at a negative offset", 4, st, one, oneg, l1, fin0, 1, g_in, 0, g_energy, no);
    REFUSED("a chunk of more than 2^30 samples", 4, st, one, o0, lbig, fin0, 1, g_in, 0, g_energy, no);
    REQUIRE(ld_plan_build(4, st, one, o0, lmax, fin0, 1, g_in, 0, g_energy, no, &plan, next) == nullptr && no[0] == (77 + SP_MAX_CHUNK) / LD_H);
    REFUSED("pool outside 1 .. 64 streams", 0, st, one, o0, l1, fin0, 1, g_in, 0, g_energy, no);
    REFUSED("pool outside 1 .. 64 streams", LD_MAX_STREAMS + 1, st, one, o0, l1, fin0, 1, g_in, 0, g_energy, no);
    {
        LdStream big[LD_MAX_STREAMS] = {};
        big[0].R = SP_MAX_TOTAL - 5; big[0].k = big[0].R / LD_H;
        plan.n = 7;
        SAYS(ld_plan_build(4, big, one, o0, l1, fin0, 1, g_in, 0, g_energy, no, &plan, next), "a stream of more than 2^48 samples");
        REQUIRE(plan.n == 0);
    }
    // create: the pool's size and the ring
    REQUIRE(sp_size_bad(0) != nullptr && sp_size_bad(65) != nullptr && sp_size_bad(1) == nullptr && sp_size_bad(64) == nullptr);
    REQUIRE(ld_ring_bad(0) == nullptr && ld_ring_bad(4) == nullptr && ld_ring_bad(4096) == nullptr);
    REQUIRE(ld_ring_bad(3) != nullptr && ld_ring_bad(4097) != nullptr && ld_ring_bad(-1) != nullptr);
    // resets: refused as a whole, nothing moved
    const int32_t two[2] = {0, 1};
    SAYS(ld_reset(4, st, dup, 2), "duplicate stream id in one call");
    REQUIRE(memcmp(keep, st, sizeof(st)) == 0);
    REQUIRE(ld_reset(4, st, far, 1) != nullptr && ld_reset(4, st, neg, 1) != nullptr && memcmp(keep, st, sizeof(st)) == 0);
    REQUIRE(ld_reset(4, st, nullptr, 1) != nullptr && ld_reset(4, nullptr, two, 2) != nullptr);
    REQUIRE(ld_reset(4, st, two, 0) != nullptr && ld_reset(4, st, two, 5) != nullptr && ld_reset(0, st, two, 2) != nullptr && memcmp(keep, st, sizeof(st)) == 0);
    REQUIRE(ld_reset(4, st, two, 2) == nullptr && st[0].R == 0 && st[1].R == 0 && st[1].touched == 0);
    // integrate
    REQUIRE(ld_integrate_bad(4, two, 2, g_energy) == nullptr);
    SAYS(ld_integrate_bad(4, nullptr, 2, g_energy), "null pointer");
    SAYS(ld_integrate_bad(4, two, 2, nullptr), "null pointer");
    SAYS(ld_integrate_bad(4, two, 2, (const char*)g_energy + 4), "a misaligned buffer");
    SAYS(ld_integrate_bad(4, dup, 2, g_energy), "duplicate stream id in one call");
    SAYS(ld_integrate_bad(4, two, 0, g_energy), "stream list: need 1 .. n_streams ids");
    SAYS(ld_integrate_bad(65, two, 2, g_energy), "pool outside 1 .. 64 streams");
    // after all of that an ordinary call still plans
    REQUIRE(ld_plan_build(4, st, one, o0, l1, fin0, 1, g_in, 0, g_energy, no, &plan, next) == nullptr && plan.n == 1 && no[0] == 0);
}

static void check_finisher_arguments() {
    FinLd ld;
    long pt[LD_MAX_STREAMS + 1] = {};
    int32_t ce[LD_MAX_STREAMS + 1];
    for (int i = 0; i <= LD_MAX_STREAMS; ++i) { pt[i] = i % 2 ? 13000000 + i : 0; ce[i] = 1 + i * 500; }
    REQUIRE(fin_ld_build(pt, ce, 3, g_energy, &ld) == nullptr);
    REQUIRE(ld.pt[0] == 0 && ld.pt[1] == 13000001 && ld.ceil[2] == 1001 && ld.pt[3] == 0 && ld.ceil[3] == 0 && ld.ceil[63] == 0);
    REQUIRE(fin_ld_build(pt, ce, LD_MAX_STREAMS, g_energy, &ld) == nullptr && ld.pt[63] == 13000063 && ld.ceil[63] == 31501);
    SAYS(fin_ld_build(nullptr, ce, 3, g_energy, &ld), "null pointer");
    SAYS(fin_ld_build(pt, nullptr, 3, g_energy, &ld), "null pointer");
    SAYS(fin_ld_build(pt, ce, 3, nullptr, &ld), "null pointer");
    SAYS(fin_ld_build(pt, ce, 3, (const char*)g_energy + 4, &ld), "a misaligned buffer");
    SAYS(fin_ld_build(pt, ce, 0, g_energy, &ld), "segment list: need 1 .. 64 segments");
    SAYS(fin_ld_build(pt, ce, LD_MAX_STREAMS + 1, g_energy, &ld), "segment list: need 1 .. 64 segments");
    pt[1] = -1; REQUIRE(fin_ld_build(pt, ce, 3, g_energy, &ld) != nullptr);
    pt[1] = LD_PT_MAX + 1; REQUIRE(fin_ld_build(pt, ce, 3, g_energy, &ld) != nullptr);
    pt[1] = LD_PT_MAX; REQUIRE(fin_ld_build(pt, ce, 3, g_energy, &ld) == nullptr);
    REQUIRE((double)(LD_PT_MAX * 4 * LD_H) == (double)LD_PT_MAX * 4 * LD_H && LD_PT_MAX * 4 * LD_H < (1L << 53));      // exact in float64
    ce[2] = 0; REQUIRE(fin_ld_build(pt, ce, 3, g_energy, &ld) != nullptr);
    ce[2] = 32768; REQUIRE(fin_ld_build(pt, ce, 3, g_energy, &ld) != nullptr);
    ce[2] = 32767; REQUIRE(fin_ld_build(pt, ce, 3, g_energy, &ld) == nullptr);
    // the bound behind the relative gate's 64-bit comparison
    const long zmax = ((long)LD_TAPS_ABS_SUM * 32768 + (1L << (LD_Q - 1))) >> LD_Q;
    REQUIRE(zmax < (1L << 17));
    const long emax = 4L * LD_H * zmax * zmax;
    REQUIRE(emax < (1L << 48) && (double)10 * LD_RING_MAX * (double)emax < 9.2e18);
    REQUIRE(LD_GATE_ABS == 1208568L);
}

int main() {
    check_counts();
    check_offsets_and_refusals();
    check_finisher_arguments();
    REQUIRE(g_checks > 1000);
    printf("ok\n");
    return 0;
}
