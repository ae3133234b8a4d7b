// The host plan of the limiter pool's TRUE-PEAK streams and of the stateless true-peak meter (sesameai-tts_amd/csrc/limiter_plan.h: no
// HIP; include/mimi_hip.h, mimi_lim_pool_reset_tp and mimi_tp_measure) as a stand-alone host program, built with the host sanitizers by
// tests/test_truepeak_plan_host.py.  The flag's refusals and that all zeros is mimi_lim_pool_reset; the emitted counts against a walk of
// the definition (sample r leaves once r + L + T + 1 samples are in, or at final); calls that mix both modes, walked the way the
// kernels walk them -- the two plans partition the list in order, the outputs stay packed in list order, every output lies in exactly one
// line of exactly one tile, every halo lies inside the history (now T further back) and inside the call's LDS buffer with the signed
// samples staged T beyond it on either side, every computed gain reads only samples the call or the bank's last 2 T hold, a line moved as a
// vector lies wholly inside the chunk and on a 16-byte address, the carry's indices stay inside a true-peak bank; every refusal of the
// feed and of the meter's plan with nothing planned and no state moved.  Prints "ok".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "limiter_plan.h"

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

alignas(16) static char g_in[64], g_out[64];

struct Pool { LimStream st[LIM_MAX_STREAMS] = {}; };

static const char* reset1(Pool& p, int sid, int c, int l, int rho, int hr, int tp) {
    const int32_t ids[1] = {sid}, cc[1] = {c}, ll[1] = {l}, rr[1] = {rho}, hh[1] = {hr}, tt[1] = {tp};
    return lim_reset_tp(4, p.st, ids, cc, ll, rr, hh, tt, 1);
}

static void check_reset_and_refusals() {
    Pool p, q, keep;
    REQUIRE(TP_T == 8 && TP_Q == 14 && TP_TAPS_ABS_SUM == 31572 && LIM_TP_BANK == LIM_HIST_MAX + LIM_L_MAX + 3 * TP_T);
    // all zeros is mimi_lim_pool_reset
    {
        const int32_t ids[2] = {3, 1}, cc[2] = {100, 29203}, ll[2] = {1, 480}, rr[2] = {8, 65536}, hh[2] = {0, 4}, zz[2] = {0, 0};
        REQUIRE(lim_reset_tp(4, p.st, ids, cc, ll, rr, hh, zz, 2) == nullptr && lim_reset(4, q.st, ids, cc, ll, rr, hh, 2) == nullptr);
        REQUIRE(memcmp(&p, &q, sizeof(p)) == 0 && p.st[1].tp == 0 && lim_delay(p.st[1]) == 480);
        REQUIRE(lim_reset_tp(4, q.st, ids, cc, ll, rr, hh, nullptr, 2) == nullptr && memcmp(&p, &q, sizeof(p)) == 0);
    }
    REQUIRE(reset1(p, 1, 29203, 120, 27, 0, 1) == nullptr && p.st[1].tp == 1 && p.st[1].set == 1 && lim_delay(p.st[1]) == 128);
    REQUIRE(reset1(p, 2, 1, 1, 8, 4, 1) == nullptr && reset1(p, 2, 32767, LIM_L_MAX, LIM_RHO_MAX, 0, 1) == nullptr && lim_delay(p.st[2]) == 488);
    memcpy(&keep, &p, sizeof(p));
    SAYS(reset1(p, 1, 100, 120, 27, 0, 2), "a true-peak flag that is neither 0 nor 1");
    SAYS(reset1(p, 1, 100, 120, 27, 0, -1), "a true-peak flag that is neither 0 nor 1");
    SAYS(reset1(p, 1, 0, 120, 27, 0, 1), "a ceiling outside 1 .. 32767");
    SAYS(reset1(p, 1, 100, 481, 27, 0, 1), "a look-ahead outside 1 .. 480 samples");
    SAYS(reset1(p, 4, 100, 120, 27, 0, 1), "stream id outside [0, n_streams)");
    {   // a list whose LAST flag is bad moves none of the others
        const int32_t ids[2] = {0, 2}, cc[2] = {100, 100}, ll[2] = {120, 120}, rr[2] = {27, 27}, hh[2] = {0, 0}, tt[2] = {1, 7};
        REQUIRE(lim_reset_tp(4, p.st, ids, cc, ll, rr, hh, tt, 2) != nullptr);
        SAYS(lim_reset_tp(4, p.st, ids, cc, nullptr, rr, hh, tt, 2), "null pointer");
    }
    REQUIRE(memcmp(&keep, &p, sizeof(p)) == 0);
    // the feed: stream 1 is a true-peak stream that holds its 128 fp32 samples, stream 0 has no parameters, stream 3 detects sample peaks
    p.st[1].R = 700; p.st[1].E = 572; p.st[1].fmt = 0; p.st[1].touched = 1;
    memcpy(&keep, &p, sizeof(p));
    const int32_t one[1] = {1}, zero[1] = {0}, both[2] = {3, 1}, dup11[2] = {1, 1}, fin0[2] = {0, 0};
    const long o0[2] = {0, 8}, l1[2] = {4, 4};
    long no[2];
    LimPlan plans[2]; LimStream next[LIM_MAX_STREAMS];
#define REFUSED(text, ...)                                                                         \
    do {                                                                                           \
        plans[0].n = plans[1].n = 7; plans[0].tiles = plans[1].tiles = 7;                          \
        SAYS(lim_plan_build_tp(__VA_ARGS__, plans, next), text);                                   \
        REQUIRE(plans[0].n == 0 && plans[0].tiles == 0 && plans[0].lds_words == 0 && plans[1].n == 0 && plans[1].tiles == 0 && \
                plans[1].lds_words == 0 && memcmp(&keep, &p, sizeof(p)) == 0);                     \
    } while (0)
    REFUSED("null pointer", 4, p.st, one, o0, l1, fin0, 1, nullptr, g_out, no, 0);
    REFUSED("null pointer", 4, p.st, one, o0, l1, fin0, 1, g_in, g_out, nullptr, 0);
    REFUSED("unknown format", 4, p.st, one, o0, l1, fin0, 1, g_in, g_out, no, 2);
    REFUSED("a misaligned buffer", 4, p.st, one, o0, l1, fin0, 1, g_in + 2, g_out, no, 0);
    REFUSED("duplicate stream id in one call", 4, p.st, dup11, o0, l1, fin0, 2, g_in, g_out, no, 0);
    REFUSED("stream list: need 1 .. n_streams ids", 4, p.st, one, o0, l1, fin0, 0, g_in, g_out, no, 0);
    REFUSED("a stream without parameters: mimi_lim_pool_reset gives them", 4, p.st, zero, o0, l1, fin0, 1, g_in, g_out, no, 0);
    REFUSED("a stream that holds samples of the other format", 4, p.st, one, o0, l1, fin0, 1, g_in, g_out, no, 1);
    REFUSED("a stream that holds samples of the other format", 4, p.st, both, o0, l1, fin0, 2, g_in, g_out, no, 1);      // in company
    {
        const long neg[1] = {-1}, most[1] = {SP_MAX_CHUNK};
        const int32_t fin1[1] = {1};
        REFUSED("a chunk of negative length", 4, p.st, one, o0, neg, fin0, 1, g_in, g_out, no, 0);
        REFUSED("a chunk at a negative offset", 4, p.st, one, neg, l1, fin0, 1, g_in, g_out, no, 0);
        REFUSED("a chunk that gives more than 2^30 samples", 4, p.st, one, o0, most, fin1, 1, g_in, g_out, no, 0);      // 2^30 and the 128 held
        static float buf[1024];
        const long l200[1] = {200};
        REFUSED("in and out overlap", 4, p.st, one, o0, l200, fin0, 1, buf, buf + 199, no, 0);
    }
    // a good call: 128 held, 4 new, 4 leave, planned as a true-peak segment; the plan for sample-peak streams alone refuses it
    REQUIRE(lim_plan_build_tp(4, p.st, one, o0, l1, fin0, 1, g_in, g_out, no, 0, plans, next) == nullptr && memcmp(&keep, &p, sizeof(p)) == 0);
    REQUIRE(plans[0].n == 0 && plans[0].tiles == 0 && plans[1].n == 1 && plans[1].tiles == 1 && no[0] == 4);
    REQUIRE(plans[1].lds_words == LIM_TILE + 2428 + 240 + 1 + 2 * TP_T && next[0].R == 704 && next[0].E == 576 && next[0].parity == 1 && next[0].tp == 1);
    REQUIRE(plans[1].seg[0].nh == 128 && plans[1].seg[0].tp == 1 && plans[1].seg[0].pre == 2 * TP_T && plans[1].seg[0].fresh == 0 && plans[1].seg[1].n_in == 0);
    {
        LimPlan alone;
        SAYS(lim_plan_build(4, p.st, one, o0, l1, fin0, 1, g_in, g_out, no, 0, &alone, next), "a true-peak stream: lim_plan_build_tp plans it");
        REQUIRE(alone.n == 0 && alone.tiles == 0 && alone.lds_words == 0 && memcmp(&keep, &p, sizeof(p)) == 0);
    }
    // the meter's plan
    {
        TpPlan tp;
        long rows[8];
        const long off[3] = {0, 5, 9000}, len[3] = {5, 0, 4097}, neg[3] = {0, -1, 0}, big[3] = {SP_MAX_CHUNK + 1, 0, 0};
#define TP_REFUSED(text, ...)                                                                      \
    do {                                                                                           \
        tp.n = 7; tp.tiles = 7;                                                                    \
        SAYS(tp_plan_build(__VA_ARGS__, &tp), text);                                               \
        REQUIRE(tp.n == 0 && tp.tiles == 0);                                                       \
    } while (0)
        TP_REFUSED("null pointer", nullptr, off, len, 3, 0, rows);
        TP_REFUSED("null pointer", g_in, nullptr, len, 3, 0, rows);
        TP_REFUSED("null pointer", g_in, off, nullptr, 3, 0, rows);
        TP_REFUSED("null pointer", g_in, off, len, 3, 0, nullptr);
        TP_REFUSED("unknown format", g_in, off, len, 3, 2, rows);
        TP_REFUSED("a misaligned buffer", g_in + 2, off, len, 3, 0, rows);
        TP_REFUSED("a misaligned buffer", g_in + 1, off, len, 3, 1, rows);
        TP_REFUSED("a misaligned buffer", g_in, off, len, 3, 0, (const char*)rows + 4);
        TP_REFUSED("clip list: need 1 .. 64 clips", g_in, off, len, 0, 0, rows);
        TP_REFUSED("clip list: need 1 .. 64 clips", g_in, off, len, 65, 0, rows);
        TP_REFUSED("a chunk of negative length", g_in, off, neg, 3, 0, rows);
        TP_REFUSED("a chunk at a negative offset", g_in, neg, len, 3, 0, rows);
        TP_REFUSED("a chunk of more than 2^30 samples", g_in, off, big, 3, 0, rows);
        REQUIRE(tp_plan_build(g_in + 2, off, len, 3, 1, rows, &tp) == nullptr && tp.n == 3 && tp.tiles == 3);
        REQUIRE(tp.seg[0].t_off == 0 && tp.seg[1].t_off == 1 && tp.seg[2].t_off == 1 && tp.seg[1].n == 0 && tp.seg[2].n == 4097 && tp.seg[2].in_off == 9000);
        REQUIRE(tp.seg[3].n == 0 && tp.seg[3].t_off == 0 && tp.seg[63].in_off == 0);
        // every position of every clip in exactly one tile, the staged window T beyond it on either side inside the kernel's buffer
        for (int i = 0; i < 3; ++i) {
            const int tiles = (int)((len[i] + LIM_TILE - 1) / LIM_TILE);
            long seen = 0;
            for (int t = 0; t < tiles; ++t) {
                const long r0 = (long)t * LIM_TILE, r1 = r0 + LIM_TILE < len[i] ? r0 + LIM_TILE : len[i];
                REQUIRE(r0 < r1 && r1 - r0 + 2 * TP_T <= LIM_TILE + 2 * TP_T);
                seen += r1 - r0;
            }
            REQUIRE(seen == len[i]);
        }
    }
}

// the emitted counts against the definition, over chunk walks; final leaves the stream fresh with its parameters and its mode
static void check_out_count() {
    const int Ls[] = {1, 7, 120, 480};
    const long steps[] = {0, 1, 0, 7, 1, 1, 119, 8, 9, 479, 1, 1, 1, 4096, 5, 0, 13000};
    for (unsigned a = 0; a < 4; ++a)
        for (int fin_at = 0; fin_at < 17; ++fin_at) {
            Pool p;
            REQUIRE(reset1(p, 2, 1000, Ls[a], 27, 1, 1) == nullptr);
            long R = 0, E = 0;
            for (int k = 0; k <= fin_at; ++k) {
                const int fin = k == fin_at;
                long want = 0;                                                      // sample r leaves once r + L + T + 1 are in, or at final
                for (long r = E; r < R + steps[k] && (fin || r + Ls[a] + TP_T + 1 <= R + steps[k]); ++r) ++want;
                const int32_t ids[1] = {2}, ff[1] = {fin};
                const long off[1] = {0}, len[1] = {steps[k]};
                long no[1];
                LimPlan plans[2]; LimStream next[LIM_MAX_STREAMS];
                REQUIRE(lim_out_count(p.st[2], steps[k], fin) == want);
                static float in[20000], out[20000];
                REQUIRE(lim_plan_build_tp(4, p.st, ids, off, len, ff, 1, in, out, no, 0, plans, next) == nullptr && no[0] == want);
                const LimSeg& s = plans[1].seg[0];
                REQUIRE(plans[0].n == 0 && plans[1].n == 1 && s.nh == R - E && s.nh <= Ls[a] + TP_T && s.fresh == (R == 0) && s.n_out == want);
                REQUIRE(s.pre == (R < 2 * TP_T ? R : 2 * TP_T) && s.tp == 1);
                sp_commit(p.st, ids, next, 1);
                R += steps[k]; E += want;
                if (fin) { R = 0; E = 0; }
                REQUIRE(p.st[2].R == R && p.st[2].E == E && p.st[2].L == Ls[a] && p.st[2].set == 1 && p.st[2].tp == 1);
            }
        }
}

// One call of 4 streams, modes mixed; both plans walked the way the kernels walk them.
static void check_tile_plan() {
    static unsigned char seen[4][40000];
    const long lens[] = {0, 1, 3, 7, 8, 9, 15, 16, 17, 119, 128, 129, 4095, 4096, 4097, 8192, 12293, 19200};
    const long offs[] = {0, 1, 2, 3, 5, 7, 8, 4096};
    const int par[4][4] = {{29203, 120, 27, 0}, {1, 1, 65536, 4}, {32767, 480, 8, 2}, {1000, 7, 1000, 1}};
    long runs = 0, vectors = 0, computed = 0;
    for (int i16 = 0; i16 < 2; ++i16)
        for (unsigned a = 0; a < 18; ++a)
            for (unsigned o = 0; o < 8; ++o) {
                Pool p;
                const int esz = i16 ? 2 : 4, per = 16 / esz;
                const int32_t ids[4] = {2, 0, 3, 1};
                int32_t cc[4], ll[4], rr[4], hh[4], tt[4];
                for (int i = 0; i < 4; ++i) {
                    const int* q = par[(a + o + i) % 4];
                    cc[i] = q[0]; ll[i] = q[1]; rr[i] = q[2]; hh[i] = q[3]; tt[i] = i != (int)((a + o) % 4);          // one sample-peak stream
                }
                REQUIRE(lim_reset_tp(4, p.st, ids, cc, ll, rr, hh, tt, 4) == nullptr);
                // stream 2 fresh; stream 0 has a few samples, fewer than 2 T, and holds them all; stream 3 is far into its clip and holds
                // all it may; stream 1 is young and holds all it has
                p.st[0].R = 1 + (a + o) % 13; p.st[0].E = 0; p.st[0].fmt = i16;
                if (p.st[0].R > lim_delay(p.st[0])) p.st[0].R = lim_delay(p.st[0]);
                p.st[3].R = (1L << 40) + 3; p.st[3].E = p.st[3].R - lim_delay(p.st[3]); p.st[3].fmt = i16;
                p.st[1].R = ll[3] / 2 + 4; p.st[1].E = 0; p.st[1].fmt = i16;
                if (p.st[1].R > lim_delay(p.st[1])) p.st[1].R = lim_delay(p.st[1]);
                const long n_in[4] = {lens[a], lens[(a + 5) % 18], lens[(a + 11) % 18], lens[(a + 14) % 18]};
                long in_off[4];
                in_off[0] = offs[o];
                for (int i = 1; i < 4; ++i) in_off[i] = in_off[i - 1] + n_in[i - 1] + offs[(o + 3 * i) % 8];
                const int32_t fin[4] = {(int)(a & 1), (int)(o & 1), (int)((a + o) & 1), (int)((a >> 1) & 1)};
                const char* in = (const char*)((uintptr_t)1 << 32) + esz * (a % 3);    // any element-aligned base (never read); out far behind the inputs
                const char* out = (const char*)((uintptr_t)3 << 32) + esz * (o % 5);
                long no[4];
                LimPlan plans[2]; LimStream next[LIM_MAX_STREAMS];
                REQUIRE(lim_plan_build_tp(4, p.st, ids, in_off, n_in, fin, 4, in, out, no, i16, plans, next) == nullptr);
                REQUIRE(plans[0].n == 1 && plans[1].n == 3 && plans[0].pad == 0 && plans[1].pad == 0);
                int at[2] = {0, 0}, tiles[2] = {0, 0}, words[2] = {0, 0};
                long off = 0;
                for (int i = 0; i < 4; ++i) {
                    const int tp = tt[i];
                    const LimSeg& s = plans[tp].seg[at[tp]++];
                    const LimStream& st = p.st[ids[i]];
                    REQUIRE(s.tp == tp && s.t_off == tiles[tp] && s.out_off == off && s.n_in == n_in[i] && s.n_out == no[i] && s.in_off == in_off[i]);
                    REQUIRE(SP_SID(s) == ids[i] && SP_FINAL(s) == fin[i] && s.C == cc[i] && s.L == ll[i] && s.rho == rr[i] && s.hr == hh[i] && s.K == lim_K(rr[i]));
                    REQUIRE(s.nh == st.R - st.E && s.nh <= lim_delay(st) && s.fresh == (st.R == 0) && no[i] == lim_out_count(st, n_in[i], fin[i]));
                    REQUIRE(s.pre == (tp ? (st.R < 2 * TP_T ? st.R : 2 * TP_T) : 0) && s.mis_in < per && s.mis_out < per);
                    REQUIRE(((uintptr_t)in + (uintptr_t)(in_off[i] - s.mis_in) * esz) % 16 == 0 && ((uintptr_t)out + (uintptr_t)(off - s.mis_out) * esz) % 16 == 0);
                    const int TT = tp ? TP_T : 0, H = s.K + 2 * s.L, nt = (int)lim_tiles(s.mis_out, no[i]);
                    const int w = LIM_TILE + H + 1 + 2 * TT;
                    if (no[i] > 0 && w > words[tp]) words[tp] = w;
                    memset(seen[i], 0, sizeof(seen[i]));
                    for (int t = 0; t < nt; ++t) {
                        int t_lo, t_hi, p_lo, p_hi;
                        lim_tile_range(s, t, &t_lo, &t_hi);
                        lim_halo(s, t_lo, t_hi, &p_lo, &p_hi);
                        REQUIRE(t_lo < t_hi && t_hi - t_lo <= LIM_TILE);
                        REQUIRE(p_lo >= -TT - H && p_hi - p_lo + 1 <= plans[tp].lds_words);   // inside the history; inside a scan buffer
                        REQUIRE(p_hi - p_lo + 2 * TT <= plans[tp].lds_words);                 // and the signed samples, T beyond on either side
                        REQUIRE(p_hi <= n_in[i] - (fin[i] ? -(int)s.L : TT));                  // no gain that needs a sample not yet received
                        REQUIRE(t_lo - s.nh >= -s.nh && t_hi - s.nh <= n_in[i]);               // the outputs' own samples: held, or in the chunk
                        if (tp) {
                            int c_lo, c_hi;
                            lim_tp_computed(s, p_lo, p_hi, &c_lo, &c_hi);
                            REQUIRE(c_lo <= c_hi && c_lo >= p_lo && c_hi <= p_hi && c_hi <= n_in[i]);
                            REQUIRE(c_lo >= -TP_T && c_lo >= -(int)s.pre);                     // below -T the history answers; in front of the clip, silence
                            REQUIRE(c_lo == c_hi || c_lo - TP_T >= -2 * TP_T);                 // the bank's last 2 T samples suffice
                            REQUIRE(c_lo == c_hi || fin[i] || c_hi - 1 + TP_T <= n_in[i] - 1); // and the call's own, but at final (zeros behind)
                            for (int q = p_lo; q < p_hi; ++q) {                                // every gain has exactly one source
                                const int hist = q < -TP_T, front = q >= -TP_T && q < c_lo, calc = q >= c_lo && q < c_hi, behind = q >= n_in[i];
                                if (hist + front + calc + behind != 1) REQUIRE(hist + front + calc + behind == 1);
                                if (hist) REQUIRE(q + TP_T + H >= 0 && q + TP_T + H < H);
                                if (front) REQUIRE(q < -(int)s.pre);
                            }
                            computed += c_hi - c_lo;
                        }
                        // the output lines, as the kernel walks them
                        for (int m = t * (LIM_TILE / per); m < (t + 1) * (LIM_TILE / per); ++m) {
                            const long q0 = (long)m * per - s.mis_out;
                            if (q0 >= no[i] || q0 + per <= 0) continue;
                            if (q0 >= 0 && q0 + per <= no[i]) { REQUIRE(((uintptr_t)out + (uintptr_t)(off + q0) * esz) % 16 == 0); ++vectors; }
                            for (int c = 0; c < per; ++c)
                                if (q0 + c >= 0 && q0 + c < no[i]) { REQUIRE(q0 + c >= t_lo && q0 + c < t_hi); ++seen[i][q0 + c]; }
                        }
                        // the input lines: the halo, and T beyond it for a true-peak stream
                        const long lo = p_lo - TT > 0 ? p_lo - TT : 0, hi = p_hi + TT < n_in[i] ? p_hi + TT : n_in[i];
                        for (long l = (lo + s.mis_in) / per; lo < hi && l < (hi + s.mis_in + per - 1) / per; ++l) {
                            const long q0 = l * per - s.mis_in;
                            REQUIRE(q0 + per > lo && q0 < hi);
                            if (q0 >= 0 && q0 + per <= n_in[i]) REQUIRE(((uintptr_t)in + (uintptr_t)(in_off[i] + q0) * esz) % 16 == 0);
                            for (int c = 0; c < per; ++c)                                      // where the kernel stores it: inside the buffer
                                if (q0 + c >= lo && q0 + c < hi) REQUIRE(q0 + c - (p_lo - TT) >= 0 && q0 + c - (p_lo - TT) < plans[tp].lds_words);
                        }
                    }
                    for (long q = 0; q < no[i]; ++q)
                        if (seen[i][q] != 1) REQUIRE(seen[i][q] == 1);
                    // the carry: the gains of the H positions in front of n_in - T, the samples held after the call, the last 2 T signed ones
                    const long nh2 = s.nh + n_in[i] - no[i];
                    REQUIRE(nh2 >= 0 && nh2 <= (fin[i] ? 0 : lim_delay(st)) && H <= LIM_HIST_MAX);
                    REQUIRE(tp ? LIM_HIST_MAX + nh2 <= LIM_HIST_MAX + LIM_TP_HELD_MAX && LIM_HIST_MAX + LIM_TP_HELD_MAX + 2 * TP_T == LIM_TP_BANK
                               : LIM_HIST_MAX + nh2 <= LIM_BANK);
                    if (n_in[i] < nh2) REQUIRE(n_in[i] - nh2 + s.nh >= no[i]);
                    if (tp && !fin[i]) {                                                       // the gains the carry computes, from samples it stages in LDS
                        int k_lo, k_hi;
                        lim_tp_carried(s, &k_lo, &k_hi);
                        REQUIRE(k_lo <= k_hi && k_hi - k_lo + 2 * TP_T <= LIM_HIST_MAX + 2 * TP_T && k_hi - k_lo <= H);
                        if (k_lo < k_hi) REQUIRE(k_lo - TP_T >= -2 * TP_T && k_hi + TP_T == n_in[i] && k_lo >= n_in[i] - TP_T - H && k_lo >= -(int)s.pre && k_lo >= -TP_T);
                        if (k_lo == k_hi) REQUIRE(n_in[i] - TP_T <= k_lo);                     // nothing new is final yet
                    }
                    REQUIRE(next[i].parity == (st.parity ^ 1) && next[i].touched == 1 && next[i].C == cc[i] && next[i].tp == tp);
                    REQUIRE(fin[i] ? (next[i].R == 0 && next[i].E == 0) : (next[i].R == st.R + n_in[i] && next[i].E == st.E + no[i] && next[i].R - next[i].E == nh2));
                    ++g_checks;
                    tiles[tp] += nt; off += no[i];
                }
                for (int m = 0; m < 2; ++m) {
                    REQUIRE(plans[m].tiles == tiles[m] && plans[m].lds_words == words[m] && 2 * words[m] + LIM_TILE <= (m ? LIM_TP_LDS_MAX : LIM_LDS_MAX));
                    for (int i = plans[m].n; i < LIM_MAX_STREAMS; ++i) REQUIRE(plans[m].seg[i].n_in == 0 && plans[m].seg[i].t_off == 0 && plans[m].seg[i].K == 0);
                }
                ++runs;
            }
    REQUIRE(runs == 2 * 18 * 8 && vectors > 100000 && computed > 100000);
    // the largest call: 64 true-peak streams, one of 2^30 samples
    {
        Pool p;
        int32_t ids[LIM_MAX_STREAMS], cc[LIM_MAX_STREAMS], ll[LIM_MAX_STREAMS], rr[LIM_MAX_STREAMS], hh[LIM_MAX_STREAMS], tt[LIM_MAX_STREAMS], fin[LIM_MAX_STREAMS];
        long n_in[LIM_MAX_STREAMS], in_off[LIM_MAX_STREAMS], no[LIM_MAX_STREAMS];
        for (int i = 0; i < LIM_MAX_STREAMS; ++i) { ids[i] = i; cc[i] = 1000; ll[i] = 480; rr[i] = 8; hh[i] = 4; tt[i] = 1; fin[i] = 0; n_in[i] = i ? 4584 : SP_MAX_CHUNK; in_off[i] = 3; }
        REQUIRE(lim_reset_tp(LIM_MAX_STREAMS, p.st, ids, cc, ll, rr, hh, tt, LIM_MAX_STREAMS) == nullptr);
        LimPlan plans[2]; LimStream next[LIM_MAX_STREAMS];
        REQUIRE(lim_plan_build_tp(LIM_MAX_STREAMS, p.st, ids, in_off, n_in, fin, LIM_MAX_STREAMS, g_in, (char*)((uintptr_t)1 << 40), no, 1, plans, next) == nullptr);
        REQUIRE(no[0] == SP_MAX_CHUNK - 488 && no[1] == 4096 && plans[0].n == 0 && plans[1].n == 64);
        REQUIRE(plans[1].tiles <= (SP_MAX_CHUNK / LIM_TILE) + 2 * 63 + 1 && plans[1].lds_words == LIM_TILE + LIM_HIST_MAX + 1 + 2 * TP_T);
        REQUIRE((2 * plans[1].lds_words + LIM_TILE) * 4 <= 160 * 1024);
    }
}

int main() {
    check_reset_and_refusals();
    check_out_count();
    check_tile_plan();
    REQUIRE(g_checks > 1000);
    printf("ok\n");
    return 0;
}
