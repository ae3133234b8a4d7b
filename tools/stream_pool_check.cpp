// What the four pools of audio streams share on the host (sesameai-tts_amd/csrc/stream_pool.h: no HIP) as a stand-alone host program, built
// with the host sanitizers by tests/test_stream_pool_host.py.  One good call per pool, and then every single fault of a stream list and of
// a chunk, driven through rs_ / ts_ / vad_ / wm_plan_build and rs_ / ts_ / vad_ / wm_reset: the refusal must be the text below byte for
// byte, nothing may be planned (plan.n == 0) and no stream's state may have moved.  The texts are those the four *_plan.h held before
// they shared the checks; the plan check programs of the single pools ask only for "refused".  Prints "ok".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "resample_plan.h"
#include "stretch_plan.h"
#include "vad_plan.h"
#include "watermark_plan.h"

static int g_checks = 0;
#define REQUIRE(cond)                                                              \
    do {                                                                           \
        ++g_checks;                                                                \
        if (!(cond)) { printf("FAILED %s (%s:%d)\n", #cond, __FILE__, __LINE__); exit(1); } \
    } while (0)

// One call: a good one as it stands, and each fault changes one thing about it.
struct Call {
    int n_streams = 4, n = 2;
    int32_t streams[5] = {1, 3, 0, 2, 1};
    const int32_t* ids = streams;        // (nullptr: the null-pointer fault)
    long in_off[5] = {0, 16, 40, 50, 60}, n_in[5] = {10, 20, 0, 1, 2};
    long taken = 0;                      // samples stream ids[0] has taken since its reset
};

struct Fault { const char* what; void (*make)(Call&); const char* text; bool in_reset, in_resample_feed; };
static const Fault FAULTS[] = {
    {"null pointer", [](Call& c) { c.ids = nullptr; }, "null pointer", true, true},
    {"pool size 0", [](Call& c) { c.n_streams = 0; }, "pool outside 1 .. 64 streams", true, true},
    {"pool size 65", [](Call& c) { c.n_streams = 65; }, "pool outside 1 .. 64 streams", true, true},
    {"n = 0", [](Call& c) { c.n = 0; }, "stream list: need 1 .. n_streams ids", true, true},
    {"n > n_streams", [](Call& c) { c.n = 5; }, "stream list: need 1 .. n_streams ids", true, true},
    {"id -1", [](Call& c) { c.streams[1] = -1; }, "stream id outside [0, n_streams)", true, true},
    {"id n_streams", [](Call& c) { c.streams[1] = 4; }, "stream id outside [0, n_streams)", true, true},
    {"duplicate id", [](Call& c) { c.streams[1] = 1; }, "duplicate stream id in one call", true, true},
    {"negative length", [](Call& c) { c.n_in[1] = -1; }, "a chunk of negative length", false, true},
    {"negative offset", [](Call& c) { c.in_off[1] = -1; }, "a chunk at a negative offset", false, true},
    {"length 2^30 + 1", [](Call& c) { c.n_in[1] = (1L << 30) + 1; }, "a chunk of more than 2^30 samples", false, true},
    // (a resampler stream has no such bound: its totals are reduced by whole periods after every call)
    {"a stream at 2^48", [](Call& c) { c.taken = (1L << 48) - 5; }, "a stream of more than 2^48 samples", false, false},
};

static float g_in[4], g_out[4];
static uint8_t g_flags[4];
static int16_t g_lag[4];
static long g_power[4], g_floor[4];
static const int32_t FINAL[5] = {0, 1, 0, 0, 0};

// The pools.  feed / reset: the refusal of the call (nullptr: none), with *planned = plan.n after it.
struct Resample {
    typedef RsStream Stream;
    static constexpr const char* NAME = "resample";
    static constexpr bool REPEATS_RESET = true;
    static void fresh(Stream* st, const Call&) { for (int i = 0; i < SP_MAX_STREAMS; ++i) st[i] = Stream{7 + i, 3, -2, i & 1}; }
    static const char* feed(Stream* st, const Call& c, int* planned) {
        RsRates r; REQUIRE(rs_rates(48000, 24000, &r) == nullptr);
        RsPlan plan; Stream next[SP_MAX_STREAMS]; long n_out[5];
        plan.n = 7;
        const char* bad = rs_plan_build(r, c.n_streams, st, c.ids, c.in_off, c.n_in, FINAL, c.n, g_in, 0, g_out, 0, n_out, &plan, next);
        *planned = plan.n;
        return bad;
    }
    static const char* reset(Stream* st, const Call& c) { return rs_reset(c.n_streams, st, c.ids, c.n); }
};

struct Stretch {
    typedef TsStream Stream;
    static constexpr const char* NAME = "stretch";
    static constexpr bool REPEATS_RESET = false;
    static void fresh(Stream* st, const Call& c) {
        for (int i = 0; i < SP_MAX_STREAMS; ++i) st[i] = Stream{0, 0, 1000, i & 1};
        st[c.streams[0]].R = c.taken; st[c.streams[0]].k = ts_emitted(c.taken, 1000, 0);
    }
    static const char* feed(Stream* st, const Call& c, int* planned) {
        TsPlan plan; Stream next[SP_MAX_STREAMS]; long n_out[5];
        plan.n = 7;
        const char* bad = ts_plan_build(c.n_streams, st, c.ids, c.in_off, c.n_in, FINAL, c.n, g_in, g_out, n_out, &plan, next);
        *planned = plan.n;
        return bad;
    }
    static const char* reset(Stream* st, const Call& c) {
        const int32_t pm[5] = {500, 2000, 1000, 1200, 800};
        return ts_reset(c.n_streams, st, c.ids, pm, c.n);
    }
};

struct Vad {
    typedef VadStream Stream;
    static constexpr const char* NAME = "vad";
    static constexpr bool REPEATS_RESET = false;
    static void fresh(Stream* st, const Call& c) {
        for (int i = 0; i < SP_MAX_STREAMS; ++i) st[i] = Stream{0, 0, VAD_DEFAULT_PARAMS, i & 1, 0};
        st[c.streams[0]].R = c.taken; st[c.streams[0]].k = c.taken / VAD_F;
    }
    static const char* feed(Stream* st, const Call& c, int* planned) {
        VadPlan plan; Stream next[SP_MAX_STREAMS]; long n_frames[5];
        plan.n = 7;
        const char* bad = vad_plan_build(c.n_streams, st, c.ids, c.in_off, c.n_in, FINAL, c.n, g_in, 0, g_flags, g_lag, g_power, g_floor, n_frames, &plan, next);
        *planned = plan.n;
        return bad;
    }
    static const char* reset(Stream* st, const Call& c) {
        const VadParams prm[5] = {VAD_DEFAULT_PARAMS, VAD_DEFAULT_PARAMS, VAD_DEFAULT_PARAMS, VAD_DEFAULT_PARAMS, VAD_DEFAULT_PARAMS};
        return vad_reset(c.n_streams, st, c.ids, prm, c.n);
    }
};

struct Watermark {
    typedef WmStream Stream;
    static constexpr const char* NAME = "watermark";
    static constexpr bool REPEATS_RESET = false;
    static void fresh(Stream* st, const Call& c) {
        for (int i = 0; i < SP_MAX_STREAMS; ++i) st[i] = Stream{0, 0, 0x5AULL, 8, -1, i & 1};
        st[c.streams[0]].R = c.taken; st[c.streams[0]].given = c.taken / WM_S * WM_S;
    }
    static const char* feed(Stream* st, const Call& c, int* planned) {
        WmPlan plan; Stream next[SP_MAX_STREAMS]; long n_out[5];
        plan.n = 7;
        const char* bad = wm_plan_build(c.n_streams, st, c.ids, c.in_off, c.n_in, FINAL, c.n, g_in, 0, g_out, n_out, &plan, next);
        *planned = plan.n;
        return bad;
    }
    static const char* reset(Stream* st, const Call& c) {
        const uint8_t payloads[25] = {1, 2, 3, 4, 5};
        const int32_t t_q4[5] = {1, 64, 8, 8, 8};
        return wm_reset(c.n_streams, st, c.ids, payloads, t_q4, c.n);
    }
};

template <class P> static void check_pool() {
    typename P::Stream st[SP_MAX_STREAMS], keep[SP_MAX_STREAMS];
    int planned = -1;
    // the call without a fault plans its two segments, and resets
    const Call good;
    P::fresh(st, good);
    const char* bad = P::feed(st, good, &planned);
    if (bad) printf("%s: the good feed is refused: %s\n", P::NAME, bad);
    REQUIRE(bad == nullptr && planned == 2);
    bad = P::reset(st, good);
    if (bad) printf("%s: the good reset is refused: %s\n", P::NAME, bad);
    REQUIRE(bad == nullptr);
    for (const Fault& f : FAULTS) {
        Call c;
        f.make(c);
        const bool feeds = f.in_resample_feed || strcmp(P::NAME, "resample") != 0;
        P::fresh(st, c);
        memcpy(keep, st, sizeof(st));
        bad = P::feed(st, c, &planned);
        if (feeds) {
            if (!bad || strcmp(bad, f.text) != 0) printf("%s feed, %s: \"%s\"\n", P::NAME, f.what, bad ? bad : "(taken)");
            REQUIRE(bad != nullptr && strcmp(bad, f.text) == 0 && planned == 0 && memcmp(keep, st, sizeof(st)) == 0);
        } else {
            REQUIRE(bad == nullptr && planned == c.n);
        }
        if (!f.in_reset) continue;
        bad = P::reset(st, c);
        if (P::REPEATS_RESET && strcmp(f.what, "duplicate id") == 0) {          // mimi_rs_pool_reset takes a repeated id
            REQUIRE(bad == nullptr);
            continue;
        }
        if (!bad || strcmp(bad, f.text) != 0) printf("%s reset, %s: \"%s\"\n", P::NAME, f.what, bad ? bad : "(taken)");
        REQUIRE(bad != nullptr && strcmp(bad, f.text) == 0 && memcmp(keep, st, sizeof(st)) == 0);
    }
}

int main() {
    // the shared pieces by themselves
    REQUIRE(sp_sid_word(63, 1, 1) == (63 | 1 << 8 | 1 << 9) && sp_sid_word(5, 0, 1) == (5 | 1 << 9));
    struct { int sid; } g = {sp_sid_word(41, 1, 0) | 1 << 10};                    // (stretch's `fresh` bit rides on top)
    REQUIRE(SP_SID(g) == 41 && SP_PARITY(g) == 1 && SP_FINAL(g) == 0);
    REQUIRE(sp_chunk_bad(SP_MAX_CHUNK, 0, SP_MAX_TOTAL - SP_MAX_CHUNK) == nullptr && sp_chunk_bad(0, 0, SP_MAX_TOTAL) == nullptr);
    int tail[6] = {1, 2, 3, 4, 5, 6};
    sp_zero_tail(tail, 2);
    REQUIRE(tail[0] == 1 && tail[1] == 2 && tail[2] == 0 && tail[5] == 0);
    long st[4] = {10, 11, 12, 13};
    const long next[2] = {30, 20};
    const int32_t ids[2] = {3, 0};
    sp_commit(st, ids, next, 2);
    REQUIRE(st[0] == 20 && st[1] == 11 && st[2] == 12 && st[3] == 30);
    check_pool<Resample>();
    check_pool<Stretch>();
    check_pool<Vad>();
    check_pool<Watermark>();
    REQUIRE(g_checks > 80);
    printf("ok\n");
    return 0;
}
