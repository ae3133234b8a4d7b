// A pool of stateful voice-activity streams on the device (mimi_vad_pool_*, include/mimi_hip.h states the rule): when a speaker starts and
// when they have stopped, for up to 64 microphones at once.  TWO launches per call whatever the number of streams and their chunk lengths:
//   k_vad_features  one workgroup per (stream, frame) of the call: the frame's DC-free power and its first-crossing lag.  Frames do not
//                   depend on each other, so a call's frames -- 80 per stream for a 19,200-sample chunk, 64,000 for 64 clips of 10 s -- fill
//                   the machine instead of queueing behind one workgroup per stream.  It writes `power` and `lag` where the caller reads them.
//   k_vad_scan      one wave per listed stream: reads those two arrays back, runs the serial part (loud against the floor, the hold, the
//                   state machine, the floor's update: a few integer operations per frame), writes `flags`, `floor`, the stream's state and
//                   summary, and moves the stream's last samples into the carry bank that the call did not read.
// The plan (vad_plan.h) travels in the kernel arguments: no host-to-device copy, no allocation, no synchronisation.
//
// Features.  The 880 samples that end with the frame are staged in LDS as block-floating int16 pairs.  Thread t scores lags 400 - 2t and
// 399 - 2t (offsets e = 2t, 2t + 1 into the staged span) with v_dot2 on the pairs: the even offset reads the pairs as staged, the odd one
// the same pairs shifted by one sample, made in registers from two neighbouring words (alignbit by 16; a v_perm_b32 in the ISA), as the stretch's search does.  Lanes
// read consecutive words (no bank conflict), the window's word is a broadcast.  E(tau) comes from the same registers with two more dot2 --
// exact like a prefix sum, and it rides in the shadow of the LDS reads.  Every sum is an exact integer below 2^29 in any order; the
// threshold is compared in 64 bits; "smallest qualifying tau" is a max-reduction over e.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mimi_hip.h"
#include "stream_pool.cuh"
#include "vad_plan.h"

static_assert(MIMI_VAD_MAX_STREAMS == VAD_MAX_STREAMS && MIMI_VAD_SUMMARY == VAD_SUMMARY, "header and plan disagree");
static_assert(sizeof(mimi_vad_params) == sizeof(VadParams) && sizeof(VadParams) == 32, "header and plan disagree");
static_assert(sizeof(VadSeg) == 56 && sizeof(VadPlan) <= 3600, "the plan must fit the kernel arguments");
static_assert(VAD_SPAN == 880 && VAD_F == 240 && VAD_TMAX - VAD_TMIN == 340, "k_vad_features: 256 threads, two lags each");

#define VAD_THREADS 256
#define VAD_WORDS (VAD_SPAN / 2)        // 440 int16 pairs
#define VAD_WIN0 (VAD_TMAX / 2)         // the window's first pair: 200

struct VadState { long N; int run, since; };      // (in speech and quiet live in the summary)

struct MimiVadPool : SpPool<VadStream> {
    int16_t* carry_dev = nullptr;    // [n_streams][2 banks][VAD_CARRY]
    VadState* state_dev = nullptr;   // [n_streams]
    long* summary_dev = nullptr;     // [n_streams][VAD_SUMMARY]
};

// integer sample at position p relative to the call's base: `lead` rule zeros, the carry, the new chunk; zero outside
__device__ __forceinline__ int vad_s(const int16_t* __restrict__ carry, int lead, int Lc, const void* __restrict__ in, long in_off, int n_in,
                                     int i16, int p) {
    p -= lead;
    if (p < 0) return 0;
    if (p < Lc) return carry[p];
    p -= Lc;
    if (p >= n_in) return 0;
    return i16 ? (int)((const int16_t*)in)[in_off + p] : pcm_i16(((const float*)in)[in_off + p]);
}

__global__ void __launch_bounds__(VAD_THREADS) k_vad_features(const VadPlan plan, const int16_t* __restrict__ carry, const void* __restrict__ in,
                                                              int i16, int16_t* __restrict__ lag_out, long* __restrict__ power_out) {
    __shared__ uint32_t q[VAD_WORDS];
    __shared__ int red[4][4];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    // the segment that owns this frame: the last one whose f_off <= blockIdx.x among those with frames
    const VadSeg& g = plan.seg[sp_owner(plan.seg, plan.n, &VadSeg::f_off)];
    const int i = (int)blockIdx.x - g.f_off;
    if (i >= g.nf) return;                                                            // (never: every block below plan.frames lies in a segment)
    const int16_t* old = carry + ((long)SP_SID(g) * 2 + SP_PARITY(g)) * VAD_CARRY;
    const int lead = VAD_LEAD(g), Lc = g.Lc, n_in = g.n_in, p0 = i * VAD_F;
    // the 880 samples that end with the frame: pairs m = t and t + 256 (m < 440)
    int s[4] = {0, 0, 0, 0};
    int m_abs = 0;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int m = t + r * VAD_THREADS;
        if (m < VAD_WORDS) {
            s[2 * r] = vad_s(old, lead, Lc, in, g.in_off, n_in, i16, p0 + 2 * m);
            s[2 * r + 1] = vad_s(old, lead, Lc, in, g.in_off, n_in, i16, p0 + 2 * m + 1);
            m_abs = max(m_abs, max(abs(s[2 * r]), abs(s[2 * r + 1])));
        }
    }
    // the frame is the span's last 240 samples: pairs 320 .. 439, held by threads 64 .. 183 of round 1
    int s1 = 0, sq_lo = 0, sq_hi = 0;
    if (t + VAD_THREADS >= VAD_WORDS - VAD_F / 2 && t + VAD_THREADS < VAD_WORDS) {
        s1 = s[2] + s[3];
        const uint32_t a = (uint32_t)(s[2] * s[2]), b = (uint32_t)(s[3] * s[3]);       // each <= 2^30
        sq_lo = (int)((a & 0x7FFF) + (b & 0x7FFF));
        sq_hi = (int)((a >> 15) + (b >> 15));
    }
    const int wm = wave_max_i(m_abs), ws1 = wave_sum_i(s1), wlo = wave_sum_i(sq_lo), whi = wave_sum_i(sq_hi);
    if (lane == 0) { red[w][0] = wm; red[w][1] = ws1; red[w][2] = wlo; red[w][3] = whi; }
    __syncthreads();
    const int mx = max(max(red[0][0], red[1][0]), max(red[2][0], red[3][0]));
    if (t == 0) {
        const long S1 = (long)red[0][1] + red[1][1] + red[2][1] + red[3][1];
        const long S2 = ((long)red[0][3] + red[1][3] + red[2][3] + red[3][3]) * 32768 + ((long)red[0][2] + red[1][2] + red[2][2] + red[3][2]);
        power_out[g.f_off + i] = VAD_F * S2 - S1 * S1;
    }
    const int sh = max(0, 32 - __builtin_clz((unsigned)mx | 1u) - 10);                 // bitlen(mx) - 10 (mx < 1024 gives 0 either way)
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int m = t + r * VAD_THREADS;
        if (m < VAD_WORDS) q[m] = (uint32_t)((s[2 * r] >> sh) & 0xFFFF) | ((uint32_t)(s[2 * r + 1] >> sh) << 16);
    }
    __syncthreads();
    // E0 over the window's 240 pairs
    const uint32_t wq = t < VAD_W / 2 ? q[VAD_WIN0 + t] : 0u;
    const int we0 = wave_sum_i(dot2_i16(wq, wq, 0));
    if (lane == 0) red[w][0] = we0;                                                   // (the maxima there were read before the last barrier)
    // offsets e = 2t and 2t + 1, e <= 340: R_e = sum_j w[j] B[e + j], E_e = sum_j B[e + j]^2
    const bool mine = t <= (VAD_TMAX - VAD_TMIN) / 2;
    int r0 = 0, r1 = 0, e0 = 0, e1 = 0;
    if (mine) {
        uint32_t cur = q[t];
#pragma unroll 8
        for (int m = 0; m < VAD_W / 2; ++m) {
            const uint32_t nxt = q[t + m + 1];                                        // t + m + 1 <= 170 + 240 < 440
            const uint32_t wv = q[VAD_WIN0 + m];
            const uint32_t odd = __builtin_amdgcn_alignbit(nxt, cur, 16);
            r0 = dot2_i16(cur, wv, r0);
            e0 = dot2_i16(cur, cur, e0);
            r1 = dot2_i16(odd, wv, r1);
            e1 = dot2_i16(odd, odd, e1);
            cur = nxt;
        }
    }
    __syncthreads();
    const long E0 = (long)red[0][0] + red[1][0] + red[2][0] + red[3][0];
    int best = -1;                                                                    // the larger e is the smaller lag
    if (mine && r0 > 0 && 2 * (long)r0 * r0 > E0 * e0) best = 2 * t;
    if (mine && 2 * t + 1 <= VAD_TMAX - VAD_TMIN && r1 > 0 && 2 * (long)r1 * r1 > E0 * e1) best = 2 * t + 1;
    const int wb = wave_max_i(best);
    if (lane == 0) red[w][1] = wb;                                                    // (the sums there were read before the barrier before last)
    __syncthreads();
    if (t == 0) {
        const int b = max(max(red[0][1], red[1][1]), max(red[2][1], red[3][1]));
        lag_out[g.f_off + i] = (int16_t)(b < 0 ? 0 : VAD_TMAX - b);
    }
}

__global__ void __launch_bounds__(64) k_vad_scan(const VadPlan plan, int16_t* __restrict__ carry, VadState* __restrict__ state,
                                                 long* __restrict__ summary, const void* __restrict__ in, int i16,
                                                 const int16_t* __restrict__ lag_in, const long* __restrict__ power_in,
                                                 uint8_t* __restrict__ flags_out, long* __restrict__ floor_out) {
    __shared__ long sp[64];
    __shared__ int sl[64];
    const VadSeg& g = plan.seg[blockIdx.x];
    const int lane = threadIdx.x, sid = SP_SID(g), nf = g.nf;
    const int on = VAD_ON(g), off = VAD_OFF(g), min_on = VAD_MIN_ON(g), hang = VAD_HANG(g), hold = g.hold;
    const long n_min = g.n_min;
    long* sm = summary + (long)sid * VAD_SUMMARY;
    // every lane walks the same scan (uniform: no divergence) and keeps the frame that is its own
    long N = 0, k = g.k0, last_start = -1, last_end = -1, n_start = 0, n_end = 0;
    int speech = 0, run = 0, quiet = 0, since = VAD_SAT;
    if (g.k0 != 0) {
        N = state[sid].N; run = state[sid].run; since = state[sid].since;
        speech = (int)sm[0]; last_start = sm[2]; last_end = sm[3]; quiet = (int)sm[4]; n_start = sm[5]; n_end = sm[6];
    }
    for (int f0 = 0; f0 < nf; f0 += 64) {
        const int cnt = min(64, nf - f0);
        __syncthreads();
        if (lane < cnt) { sp[lane] = power_in[g.f_off + f0 + lane]; sl[lane] = lag_in[g.f_off + f0 + lane]; }
        __syncthreads();
        int my_flags = 0;
        long my_floor = 0;
        for (int j = 0; j < cnt; ++j) {
            const long P = sp[j];
            const int voiced = sl[j] != 0;
            int loud = 0;
            if (k == 0) N = P > n_min ? P : n_min;
            else loud = 16 * P > N * (long)(speech ? off : on);
            since = voiced ? 0 : min(since + 1, VAD_SAT);
            const int active = loud && since <= hold;
            if (!speech) {
                run = active ? run + 1 : 0;
                if (run == min_on) { speech = 1; run = 0; quiet = 0; last_start = k - min_on + 1; ++n_start; }
            } else {
                quiet = active ? 0 : quiet + 1;
                if (quiet == hang) { speech = 0; quiet = 0; last_end = k - hang + 1; ++n_end; }
            }
            if (P < N) N -= (N - P) >> 2; else N += (N >> 9) + 1;
            N = N > n_min ? N : n_min;
            ++k;
            if (j == lane) { my_flags = loud | voiced << 1 | active << 2 | speech << 3; my_floor = N; }
        }
        if (lane < cnt) { flags_out[g.f_off + f0 + lane] = (uint8_t)my_flags; floor_out[g.f_off + f0 + lane] = my_floor; }
    }
    if (lane == 0) {
        sm[0] = speech; sm[1] = k; sm[2] = last_start; sm[3] = last_end; sm[4] = quiet; sm[5] = n_start; sm[6] = n_end; sm[7] = 0;
        state[sid].N = N; state[sid].run = run; state[sid].since = since;
    }
    if (SP_FINAL(g)) return;                                                         // the stream is fresh: it reads no carry
    // the samples from the next call's base on, into the bank this call did not read
    const int16_t* old = carry + ((long)sid * 2 + SP_PARITY(g)) * VAD_CARRY;
    int16_t* nw = carry + ((long)sid * 2 + (SP_PARITY(g) ^ 1)) * VAD_CARRY;
    const int lead = VAD_LEAD(g), Lc = g.Lc, n_in = g.n_in;
    const long k1 = g.k0 + nf;
    const int lead1 = k1 < 3 ? VAD_HIST - (int)k1 * VAD_F : 0;
    const long have = (long)lead + Lc + n_in - (long)nf * VAD_F;                      // positions from the new base on, rule zeros included
    int Ln = (int)(have - lead1);
    Ln = Ln < VAD_CARRY ? Ln : VAD_CARRY;                                             // (Ln <= 879 by the plan's arithmetic)
    for (int p = lane; p < Ln; p += 64) nw[p] = (int16_t)vad_s(old, lead, Lc, in, g.in_off, n_in, i16, nf * VAD_F + lead1 + p);
}

// rows of streams that have not been fed since their reset read as the fresh summary, whatever the memory holds
__global__ void __launch_bounds__(64) k_vad_summary(unsigned long long fresh, int n_streams, const long* __restrict__ summary, long* __restrict__ out) {
    const int s = threadIdx.x;
    if (s >= n_streams) return;
    const bool f = (fresh >> s) & 1;
#pragma unroll
    for (int j = 0; j < VAD_SUMMARY; ++j) out[s * VAD_SUMMARY + j] = f ? (j == 2 || j == 3 ? -1 : 0) : summary[s * VAD_SUMMARY + j];
}

extern "C" int mimi_vad_pool_create(int n_streams, mimi_vad_pool* out) {
    return sp_create("mimi_vad_pool_create", n_streams, out, nullptr, [&](MimiVadPool* p) {
        for (int i = 0; i < n_streams; ++i) p->st[i].prm = VAD_DEFAULT_PARAMS;
        hipError_t e = p->get(&p->carry_dev, sizeof(int16_t) * 2 * VAD_CARRY * (size_t)n_streams, 0);
        if (e == hipSuccess) e = p->get(&p->state_dev, sizeof(VadState) * n_streams, 0);
        if (e == hipSuccess) e = p->get(&p->summary_dev, sizeof(long) * VAD_SUMMARY * n_streams, 0);
        return e;
    });
}

extern "C" void mimi_vad_pool_destroy(mimi_vad_pool p) { delete p; }

extern "C" const char* mimi_vad_pool_last_error(mimi_vad_pool p) { return sp_last_error(p); }

extern "C" int mimi_vad_pool_reset(mimi_vad_pool p, const int32_t* streams, const mimi_vad_params* params, int n) {
    return p ? sp_status(p, vad_reset(p->n_streams, p->st, streams, (const VadParams*)params, n)) : -1;
}

extern "C" long mimi_vad_pool_frame_count(mimi_vad_pool p, int sid, long n_in, int final) {
    (void)final;                                                                      // a partial frame is never judged, final or not
    return sp_count_ok(p, sid, n_in) ? vad_frame_count(p->st[sid], n_in) : -1;
}

extern "C" int mimi_vad_pool_feed(mimi_vad_pool p, const int32_t* streams, const long* in_off, const long* n_in, const int32_t* final, int n,
                                  const void* in, int in_is_i16, uint8_t* flags, int16_t* lag, long* power, long* floor, long* n_frames,
                                  void* stream) {
    if (!p) return -1;
    VadPlan plan;
    VadStream next[SP_MAX_STREAMS];
    if (int rc = sp_status(p, vad_plan_build(p->n_streams, p->st, streams, in_off, n_in, final, n, in, in_is_i16, flags, lag, power, floor,
                                             n_frames, &plan, next)))
        return rc;
    (void)hipGetLastError();
    if (plan.frames > 0) {
        k_vad_features<<<dim3((unsigned)plan.frames), dim3(VAD_THREADS), 0, (hipStream_t)stream>>>(plan, p->carry_dev, in, in_is_i16, lag, power);
        SP_HIP(p, hipGetLastError());
    }
    k_vad_scan<<<dim3((unsigned)plan.n), dim3(64), 0, (hipStream_t)stream>>>(plan, p->carry_dev, p->state_dev, p->summary_dev, in, in_is_i16,
                                                                            lag, power, flags, floor);
    SP_HIP(p, hipGetLastError());
    sp_commit(p->st, streams, next, n);
    return 0;
}

extern "C" int mimi_vad_pool_summary(mimi_vad_pool p, long* out, void* stream) {
    if (!p) return -1;
    if (!out) { p->err = "null pointer"; return -1; }
    if ((uintptr_t)out % 8) { p->err = "a misaligned buffer"; return -1; }
    unsigned long long fresh = 0;
    for (int i = 0; i < p->n_streams; ++i)
        if (!p->st[i].touched) fresh |= 1ull << i;
    (void)hipGetLastError();
    k_vad_summary<<<dim3(1), dim3(64), 0, (hipStream_t)stream>>>(fresh, p->n_streams, p->summary_dev, out);
    SP_HIP(p, hipGetLastError());
    return 0;
}
