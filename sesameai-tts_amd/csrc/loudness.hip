// A pool of stateful loudness-meter streams on the device (mimi_ld_pool_*, include/mimi_hip.h states the rule): ITU-R BS.1770-4 / EBU R 128
// for one channel at 24 kHz in exact integers, for up to 64 streams at once.  TWO launches per feed whatever the number of streams and their
// chunk lengths, ONE per integrate:
//   k_ld_energy     one workgroup per (stream, hop) of the call: the hop's 2400 K-weighted samples and the sum of their squares, one int64.
//                   Hops do not depend on each other, so 64 clips of 10 s are 6,400 workgroups.  It also folds the hop's own sample peak into
//                   the stream's peak word (an integer max: exact in any order).
//   k_ld_scan       one wave per listed stream: appends the call's hop energies to the stream's ring, closes the peak (the open hop's
//                   samples included), writes the stream's state and moves its last samples into the carry bank that the call did not read.
//   k_ld_integrate  one wave per listed stream: the exact two-pass gating over the hops the ring holds, {S, n, peak, hops} to device memory.
// The plan (loudness_plan.h) travels in the kernel arguments: no host-to-device copy, no allocation, no synchronisation.
// A stream may LEVEL instead of metering (mimi_ld_pool_level_*): the same energy kernel, a scan that also walks the gain law, and
// k_ld_apply over the samples -- three launches per feed; they stand behind the meter's, below.
//
// Energy.  The 2911 samples that end with the hop are staged in LDS as int16 pairs W[m] = (w[2m], w[2m + 1]).  With the taps reversed,
// z[i] = sum_m hr[m] w[i + m]: thread t owns the output PAIRS p = t + 256 r (r < 5, p < 1200) and walks k = 0 .. 255 once for all of them --
// the even output 2p takes dot2(W[p + k], HR[k]), the odd one the same pairs shifted by one sample, made in registers from two neighbouring
// words (alignbit by 16), as k_vad_features and the stretch's search make theirs.  Lanes read consecutive words (no bank conflict); HR[k] is
// uniform and comes from constant memory through the scalar cache.  Per hop: 614,400 dot2, 327,680 four-byte LDS reads.
// sum |hq| * 32768 < 2^31, so the int32 accumulation is exact in any order; |z| < 2^17 and z^2 < 2^34 is split at bit 15 so that the wave
// reductions stay inside 32 bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mimi_hip.h"
#include "stream_pool.cuh"
#include "loudness_plan.h"

static_assert(MIMI_LD_MAX_STREAMS == LD_MAX_STREAMS && MIMI_LD_ROW == LD_ROW && MIMI_LD_HOP == LD_H, "header and plan disagree");
static_assert(sizeof(LdSeg) == 40 && sizeof(LdPlan) <= 3600, "the plan must fit the kernel arguments");

#define LD_THREADS 256
#define LD_WORDS (LD_CARRY / 2)         // 1456 int16 pairs staged per hop (sample 2911 is padding)
#define LD_PAIRS (LD_H / 2)             // 1200 output pairs per hop
#define LD_PER 5                        // output pairs per thread: 5 * 256 >= 1200
static_assert(LD_PER * LD_THREADS >= LD_PAIRS && LD_PAIRS - 1 + LD_T / 2 < LD_WORDS, "k_ld_energy: every read stays inside the staged words");

// HR[k] = (hr[2k], hr[2k + 1]) with hr[m] = hq[T - 1 - m]
struct LdHr { uint32_t w[LD_T / 2]; };
static constexpr LdHr ld_make_hr() {
    constexpr int16_t h[LD_T] = {LD_TAPS_LIST};
    LdHr r{};
    for (int k = 0; k < LD_T / 2; ++k)
        r.w[k] = (uint32_t)(uint16_t)h[LD_T - 1 - 2 * k] | (uint32_t)(uint16_t)h[LD_T - 2 - 2 * k] << 16;
    return r;
}
__constant__ LdHr c_ld_hr = ld_make_hr();

struct LdState { long hops; int peak, pad; };      // as of the stream's last call

struct MimiLdPool : SpPool<LdStream> {
    int ring = LD_RING_DEFAULT;
    int16_t* carry_dev = nullptr;    // [n_streams][2 banks][LD_CARRY]
    LdState* state_dev = nullptr;    // [n_streams]
    int* peak_dev = nullptr;         // [n_streams]: the call's hop peaks gather here; 0 between calls
    long* ring_dev = nullptr;        // [n_streams][ring]: hop h at h % ring
    LdLevel lv[LD_MAX_STREAMS] = {}; // (leveler) a stream's parameters, from mimi_ld_pool_level_reset: host only
    struct LdLvState* lstate_dev = nullptr;      // (leveler) [n_streams]
    unsigned long long* clip_dev = nullptr;      // (leveler) [n_streams]: samples clamped since the stream was fresh
};

// integer sample at position p relative to the call's base: `lead` rule zeros, the carry, the new chunk; zero outside
__device__ __forceinline__ int ld_s(const int16_t* __restrict__ carry, int lead, int Lc, const void* __restrict__ in, long in_off, int n_in,
                                    int i16, int p) {
    p -= lead;
    if (p < 0) return 0;
    if (p < Lc) return carry[p];
    p -= Lc;
    if (p >= n_in) return 0;
    return i16 ? (int)((const int16_t*)in)[in_off + p] : pcm_i16(((const float*)in)[in_off + p]);
}

// hop_peak (the leveler's feed; nullptr: the meter's): hop i of segment b also leaves its own sample peak at hop_peak[f_off + 2 b + i + 2],
// the place in the call's boundary gains where the scan reads it before it writes A[k0 + i + 2] there.
__global__ void __launch_bounds__(LD_THREADS) k_ld_energy(const LdPlan plan, const int16_t* __restrict__ carry, const void* __restrict__ in,
                                                          int i16, long* __restrict__ energy_out, int* __restrict__ peak_acc,
                                                          int* __restrict__ hop_peak) {
    __shared__ uint32_t W[LD_WORDS];
    __shared__ int red[4][3];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int seg = sp_owner(plan.seg, plan.n, &LdSeg::f_off);
    const LdSeg& g = plan.seg[seg];
    const int i = (int)blockIdx.x - g.f_off;
    if (i >= g.nf) return;                                                            // (never: every block below plan.hops lies in a segment)
    const int16_t* old = carry + ((long)SP_SID(g) * 2 + SP_PARITY(g)) * LD_CARRY;
    const int lead = LD_LEAD(g), Lc = g.Lc, n_in = g.n_in, p0 = i * LD_H;             // (i H < 2^30 + 2400: a chunk is at most 2^30 samples)
    // the 2911 samples that end with the hop; the hop's own are positions 511 .. 2910 of them
    int m_abs = 0;
    for (int m = t; m < LD_WORDS; m += LD_THREADS) {
        const int a = ld_s(old, lead, Lc, in, g.in_off, n_in, i16, p0 + 2 * m);
        const int b = 2 * m + 1 < LD_SPAN ? ld_s(old, lead, Lc, in, g.in_off, n_in, i16, p0 + 2 * m + 1) : 0;
        if (2 * m >= LD_HIST) m_abs = max(m_abs, abs(a));
        if (2 * m + 1 >= LD_HIST) m_abs = max(m_abs, abs(b));
        W[m] = (uint32_t)(a & 0xFFFF) | ((uint32_t)b << 16);
    }
    __syncthreads();
    int pr[LD_PER], ev[LD_PER], od[LD_PER];
    uint32_t cur[LD_PER];
#pragma unroll
    for (int r = 0; r < LD_PER; ++r) {
        pr[r] = min(t + r * LD_THREADS, LD_PAIRS - 1);                                // (a thread without a fifth pair walks the last one and drops it)
        cur[r] = W[pr[r]];
        ev[r] = 0; od[r] = 0;
    }
#pragma unroll 4
    for (int k = 0; k < LD_T / 2; ++k) {
        const uint32_t hr = c_ld_hr.w[k];
#pragma unroll
        for (int r = 0; r < LD_PER; ++r) {
            const uint32_t nxt = W[pr[r] + k + 1];                                    // <= 1199 + 256 = 1455
            ev[r] = dot2_i16(cur[r], hr, ev[r]);
            od[r] = dot2_i16(__builtin_amdgcn_alignbit(nxt, cur[r], 16), hr, od[r]);
            cur[r] = nxt;
        }
    }
    int sq_lo = 0, sq_hi = 0;
#pragma unroll
    for (int r = 0; r < LD_PER; ++r) {
        if (t + r * LD_THREADS >= LD_PAIRS) continue;
        const long z0 = (ev[r] + (1 << (LD_Q - 1))) >> LD_Q, z1 = (od[r] + (1 << (LD_Q - 1))) >> LD_Q;
        const unsigned long a = (unsigned long)(z0 * z0), b = (unsigned long)(z1 * z1);   // each < 2^34
        sq_lo += (int)(a & 0x7FFF) + (int)(b & 0x7FFF);
        sq_hi += (int)(a >> 15) + (int)(b >> 15);                                     // < 10 * 2^19 per thread, < 2^29 per wave
    }
    const int wm = wave_max_i(m_abs), wlo = wave_sum_i(sq_lo), whi = wave_sum_i(sq_hi);
    if (lane == 0) { red[w][0] = wm; red[w][1] = wlo; red[w][2] = whi; }
    __syncthreads();
    if (t == 0) {
        energy_out[g.f_off + i] = ((long)red[0][2] + red[1][2] + red[2][2] + red[3][2]) * 32768 + ((long)red[0][1] + red[1][1] + red[2][1] + red[3][1]);
        const int mx = max(max(red[0][0], red[1][0]), max(red[2][0], red[3][0]));
        if (mx > 0) atomicMax(peak_acc + SP_SID(g), mx);
        if (hop_peak) hop_peak[g.f_off + 2 * seg + i + 2] = mx;
    }
}

// What both scans end on, one wave per listed stream: the carry, the peak and the stream's state.
__device__ __forceinline__ void ld_scan_tail(const LdSeg& g, int16_t* __restrict__ carry, LdState* __restrict__ state, int* __restrict__ peak_acc,
                                             const void* __restrict__ in, int i16) {
    const int lane = threadIdx.x, sid = SP_SID(g), nf = g.nf;
    // the samples from the next call's base on: into the bank this call did not read, unless the clip ends; those of the open hop enter the peak
    const int16_t* old = carry + ((long)sid * 2 + SP_PARITY(g)) * LD_CARRY;
    int16_t* nw = carry + ((long)sid * 2 + (SP_PARITY(g) ^ 1)) * LD_CARRY;
    const int lead = LD_LEAD(g), Lc = g.Lc, n_in = g.n_in, fin = SP_FINAL(g);
    const int lead1 = g.k0 + nf == 0 ? LD_HIST : 0;
    const long have = (long)lead + Lc + n_in - (long)nf * LD_H;                       // positions from the new base on, rule zeros included
    int Ln = (int)(have - lead1);
    Ln = Ln < LD_CARRY ? Ln : LD_CARRY;                                               // (Ln <= 2910 by the plan's arithmetic)
    int m_abs = 0;
    for (int p = lane; p < Ln; p += 64) {
        const int v = ld_s(old, lead, Lc, in, g.in_off, n_in, i16, nf * LD_H + lead1 + p);
        if (!fin) nw[p] = (int16_t)v;
        if (lead1 + p >= LD_HIST) m_abs = max(m_abs, abs(v));
    }
    m_abs = wave_max_i(m_abs);
    if (lane == 0) {
        const int before = Lc == 0 ? 0 : state[sid].peak;                             // a fresh stream reads no state
        const int mine = peak_acc[sid];
        peak_acc[sid] = 0;
        state[sid].hops = g.k0 + nf;
        state[sid].peak = max(max(before, mine), m_abs);
        state[sid].pad = 0;
    }
}

__global__ void __launch_bounds__(64) k_ld_scan(const LdPlan plan, int ring, int16_t* __restrict__ carry, LdState* __restrict__ state,
                                                int* __restrict__ peak_acc, long* __restrict__ ring_dev, const void* __restrict__ in, int i16,
                                                const long* __restrict__ energy_in) {
    const LdSeg& g = plan.seg[blockIdx.x];
    const int lane = threadIdx.x, sid = SP_SID(g), nf = g.nf;
    // the last min(nf, ring) hops of the call, hop h at h % ring
    long* rg = ring_dev + (long)sid * ring;
    for (int j = max(0, nf - ring) + lane; j < nf; j += 64) rg[(g.k0 + j) % ring] = energy_in[g.f_off + j];
    ld_scan_tail(g, carry, state, peak_acc, in, i16);
}

struct LdIntPlan { int n, ring; unsigned long long fresh; uint8_t sid[LD_MAX_STREAMS]; };

// sum over the wave's 64 lanes of a 64-bit integer 0 <= v < 2^63 (exact in any order); every lane gets it.  Three 21-bit pieces, each
// summed in 32 bits by wave_sum_i (six DPP steps; a chain of 64-bit shuffles through LDS cost the scan a microsecond a hop).
__device__ __forceinline__ long ld_wave_sum_l(long v) {
    const long s0 = wave_sum_i((int)(v & 0x1FFFFF)), s1 = wave_sum_i((int)((v >> 21) & 0x1FFFFF)), s2 = wave_sum_i((int)(v >> 42));
    return s0 + (s1 << 21) + (s2 << 42);
}

// The exact two-pass gating over the hops a ring (in device memory, or its copy in LDS) holds when `hops` are measured, by one wave; every
// lane gets {S, n}.  What other lanes wrote to the ring before the call is seen: it opens on a barrier.
__device__ __forceinline__ void ld_gate(const long* rg, int ring, long hops, long* S_out, long* n_out) {
    const int lane = threadIdx.x;
    const long lo = hops > ring ? hops - ring : 0;                                    // the first held hop
    const int nb = (int)(hops - lo) - 3;                                              // gating blocks of four held hops
    const int lo_at = (int)(lo % ring);                                               // (one 64-bit division a call, none a block)
    auto at = [&](int k) { const int i = lo_at + k; return i >= ring ? i - ring : i; };      // held hop lo + k, k < ring: its place in the ring
    __syncthreads();
    long s_abs = 0, n_abs = 0;
    for (int b = lane; b < nb; b += 64) {
        const long E = rg[at(b)] + rg[at(b + 1)] + rg[at(b + 2)] + rg[at(b + 3)];
        if (E > LD_GATE_ABS) { s_abs += E; ++n_abs; }
    }
    s_abs = ld_wave_sum_l(s_abs);
    n_abs = wave_sum_i((int)n_abs);                                                   // (at most 64 blocks a lane)
    long S = 0, n = 0;
    for (int b = lane; b < nb; b += 64) {
        const long E = rg[at(b)] + rg[at(b + 1)] + rg[at(b + 2)] + rg[at(b + 3)];
        if (E > LD_GATE_ABS && 10 * n_abs * E > s_abs) { S += E; ++n; }               // < 10 * 4096 * 2^47.3 < 2^63
    }
    *S_out = ld_wave_sum_l(S);
    *n_out = wave_sum_i((int)n);
}

__global__ void __launch_bounds__(64) k_ld_integrate(const LdIntPlan plan, const LdState* __restrict__ state, const long* __restrict__ ring_dev,
                                                     long* __restrict__ out) {
    const int lane = threadIdx.x, sid = plan.sid[blockIdx.x], ring = plan.ring;
    long* row = out + (long)blockIdx.x * LD_ROW;
    if ((plan.fresh >> sid) & 1) {                                                    // reset and not fed since: whatever the memory holds
        if (lane < LD_ROW) row[lane] = 0;
        return;
    }
    const long hops = state[sid].hops;
    long S, n;
    ld_gate(ring_dev + (long)sid * ring, ring, hops, &S, &n);
    if (lane == 0) { row[0] = S; row[1] = n; row[2] = state[sid].peak; row[3] = hops; }
}

// ---- The leveler: mimi_ld_pool_level_* (include/mimi_hip.h states the rule, tests/leveler_ref.py in NumPy) ----
// THREE launches per feed: k_ld_energy as above, which also leaves each hop's sample peak where the scan looks for it;
//   k_ld_level_scan  one wave per listed stream walks the call's hops IN ORDER on a copy of the stream's ring in LDS (32 KiB; through
//                    device memory every hop paid a store, a barrier and eight dependent loads from L2: 2.9 us a hop): hop j - 1 enters
//                    the ring and the running peak, the exact two-pass gating over what the ring then holds (a restart per hop: ld_gate,
//                    the integrate's own) gives the target, the slew and the cap give A[j + 1]; then the call's energies go to the ring
//                    in device memory as k_ld_scan writes them, and the meter's tail.  It writes the boundary gains A[k0 .. k0 + nf + 1].
//   k_ld_apply       one workgroup per 16 KiB tile of one stream's samples: the gain of every sample from the two boundaries of its hop,
//                    the product, the clamp.  16-byte loads and stores where `in` and `out` agree modulo 16 bytes, element by element in
//                    the at most two ragged lines of a stream's chunk (and everywhere where they do not); a lane reads what it writes
//                    and nothing else, so in == out is safe.  The clamped samples are counted per workgroup, one atomic each.
struct LdLvState { int a_cur, a_next, P, pad; };      // A[k], A[k + 1], P[k - 1] for k measured hops

static_assert(sizeof(LdLevel) == 16 && sizeof(LdPlan) + sizeof(LdLevelPlan) <= 3700, "the scan's plans must fit the kernel arguments");
static_assert(sizeof(LdApSeg) == 32 && sizeof(LdApPlan) <= 2100, "the apply plan must fit the kernel arguments");
static_assert(LD_LEVEL_ROW == MIMI_LD_LEVEL_ROW, "header and plan disagree");

__global__ void __launch_bounds__(64) k_ld_level_scan(const LdPlan plan, const LdLevelPlan lp, int ring, int16_t* __restrict__ carry,
                                                      LdState* __restrict__ state, int* __restrict__ peak_acc, long* ring_dev,
                                                      LdLvState* __restrict__ lstate, unsigned long long* __restrict__ clip,
                                                      const void* __restrict__ in, int i16, const long* __restrict__ energy_in, int* gain) {
    __shared__ long rl[LD_RING_MAX];                                                  // the stream's ring while the call walks: hop h at h % ring
    const int b = blockIdx.x;
    const LdSeg& g = plan.seg[b];
    const LdLevel& v = lp.lv[b];
    const int lane = threadIdx.x, sid = SP_SID(g), nf = g.nf;
    const bool fresh = g.Lc == 0;                                                     // a fresh stream reads no state
    long* rg = ring_dev + (long)sid * ring;
    int* A = gain + g.f_off + 2 * b;                                                  // A[t] is the boundary of hop k0 + t
    int a_cur = fresh ? (int)v.g0 : lstate[sid].a_cur, a_next = fresh ? (int)v.g0 : lstate[sid].a_next, P = fresh ? 0 : lstate[sid].P;
    if (lane == 0) { A[0] = a_cur; A[1] = a_next; }
    for (long h = (g.k0 > ring ? g.k0 - ring : 0) + lane; h < g.k0; h += 64) rl[h % ring] = rg[h % ring];      // the held hops (none: a fresh stream)
    const double num = (double)((long)v.pt * (4 * LD_H)), gm = (double)v.gmax;
    const int shift = v.sh, gmax = (int)v.gmax;
    const long cnum = (long)v.ceil << 16;
    int w_at = (int)(g.k0 % ring);                                                    // where the next hop enters the ring
    // 64 hops at a time: lane t holds hop m0 + t's peak and energy (one trip to memory per batch, not per hop) and, at the end, its gain --
    // the lane that read a slot's peak is the one that writes its gain
    for (int m0 = 1; m0 <= nf; m0 += 64) {
        const int cnt = min(64, nf - m0 + 1);
        int pk_l = 0, a_l = 0;
        long e_l = 0;
        if (lane < cnt) { pk_l = A[m0 + lane + 1]; e_l = energy_in[g.f_off + m0 + lane - 1]; }
        for (int t = 0; t < cnt; ++t) {                                               // A[j + 1] for j = k0 + m, from the hops <= j - 1
            const int m = m0 + t;
            P = max(P, __shfl(pk_l, t));
            const long e = __shfl(e_l, t);
            if (lane == 0) rl[w_at] = e;
            w_at = w_at + 1 == ring ? 0 : w_at + 1;
            long S, n;
            ld_gate(rl, ring, g.k0 + m, &S, &n);
            int T = a_next;
            if (n > 0) {
                const double q = trunc(sqrt((num * (double)n) / (double)S) * 65536.0);
                T = (int)(q < gm ? q : gm);
            }
            const int d = max(1, a_next >> shift);
            const int B = min(max(T, a_next - d), a_next + d);
            const long cap = cnum / max(P, 1);
            const int a = (int)max(1L, min(min((long)B, cap), (long)gmax));
            a_cur = a_next; a_next = a;
            if (lane == t) a_l = a;
        }
        if (lane < cnt) A[m0 + lane + 1] = a_l;
    }
    for (int j = max(0, nf - ring) + lane; j < nf; j += 64) rg[(g.k0 + j) % ring] = energy_in[g.f_off + j];   // as k_ld_scan leaves the ring
    if (lane == 0) {
        lstate[sid] = LdLvState{a_cur, a_next, P, 0};
        if (fresh) clip[sid] = 0;
    }
    ld_scan_tail(g, carry, state, peak_acc, in, i16);
}

typedef int ld_v4i __attribute__((ext_vector_type(4)));

// the Q16 gain of the call's sample q: between the boundaries of its hop
__device__ __forceinline__ int ld_gi(const int* __restrict__ A, int i0, int q) {
    const int rel = i0 + q, jr = rel / LD_H, i = rel - jr * LD_H;
    return (int)(((unsigned long)A[jr] * (unsigned)(LD_H - i) + (unsigned long)A[jr + 1] * (unsigned)i) / LD_H);
}
__device__ __forceinline__ float ld_level_f(float x, int gi, float Cf, int* clipped) {
    const float y = x * ((float)gi * 0x1p-16f);                                       // gi < 2^24: the factor is exact
    const bool hi = y > Cf, lo = y < -Cf;                                             // (a NaN is neither)
    *clipped += hi | lo;
    return hi ? Cf : lo ? -Cf : y;
}
__device__ __forceinline__ int ld_level_i(int s, int gi, int C, int* clipped) {
    const long w = ((long)s * gi + (1 << 15)) >> 16;
    const long y = w > C ? C : w < -C ? -C : w;
    *clipped += y != w;
    return (int)y;
}

template <bool I16>
__global__ void __launch_bounds__(LD_AP_THREADS) k_ld_apply(const LdApPlan ap, const void* in, void* out, const int* __restrict__ gain,
                                                            unsigned long long* __restrict__ clip) {
    __shared__ int red[LD_AP_THREADS / 64];
    constexpr int ESZ = I16 ? 2 : 4, PER = LD_AP_VEC / ESZ;
    const LdApSeg& a = ap.seg[sp_owner(ap.seg, ap.n, &LdApSeg::t_off)];
    const int t = threadIdx.x, tile = (int)blockIdx.x - a.t_off, n_in = a.n_in, i0 = a.i0, C = a.ceil;
    const int* A = gain + a.g_off;
    const float Cf = (float)C * 0x1p-15f;
    const char* src = (const char*)in + a.in_off * ESZ;
    char* dst = (char*)out + a.in_off * ESZ;
    int clipped = 0;
#pragma unroll
    for (int r = 0; r < LD_AP_PER; ++r) {
        // line m of the stream's chunk holds its samples q0 .. q0 + PER; the first and the last line may reach outside [0, n_in)
        const int m = (tile * LD_AP_PER + r) * LD_AP_THREADS + t;                     // (< 2^30 / PER + 2^12)
        const int q0 = m * PER - a.mis;
        if (q0 >= n_in || q0 + PER <= 0) continue;
        if (ap.vec && q0 >= 0 && q0 + PER <= n_in) {
            ld_v4i w = *(const ld_v4i*)(src + (long)q0 * ESZ);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (I16) {
                    const int lo = ld_level_i((int16_t)(w[c] & 0xFFFF), ld_gi(A, i0, q0 + 2 * c), C, &clipped);
                    const int hi = ld_level_i(w[c] >> 16, ld_gi(A, i0, q0 + 2 * c + 1), C, &clipped);
                    w[c] = (lo & 0xFFFF) | (int)((unsigned)hi << 16);
                } else {
                    w[c] = __float_as_int(ld_level_f(__int_as_float(w[c]), ld_gi(A, i0, q0 + c), Cf, &clipped));
                }
            }
            *(ld_v4i*)(dst + (long)q0 * ESZ) = w;
        } else {
            for (int c = 0; c < PER; ++c) {
                const int q = q0 + c;
                if (q < 0 || q >= n_in) continue;
                if (I16) ((int16_t*)dst)[q] = (int16_t)ld_level_i(((const int16_t*)src)[q], ld_gi(A, i0, q), C, &clipped);
                else ((float*)dst)[q] = ld_level_f(((const float*)src)[q], ld_gi(A, i0, q), Cf, &clipped);
            }
        }
    }
    clipped = wave_sum_i(clipped);
    if ((t & 63) == 0) red[t >> 6] = clipped;
    __syncthreads();
    if (t == 0) {
        int all = 0;
        for (int w = 0; w < LD_AP_THREADS / 64; ++w) all += red[w];
        if (all > 0) atomicAdd(clip + a.sid, (unsigned long long)all);
    }
}

struct LdLsPlan { int n, pad; unsigned long long fresh; uint8_t sid[LD_MAX_STREAMS]; int g0[LD_MAX_STREAMS]; };

__global__ void __launch_bounds__(64) k_ld_level_state(const LdLsPlan plan, const LdState* __restrict__ state, const LdLvState* __restrict__ lstate,
                                                       const unsigned long long* __restrict__ clip, long* __restrict__ out) {
    const int i = threadIdx.x;
    if (i >= plan.n) return;
    const int sid = plan.sid[i];
    long* row = out + (long)i * LD_LEVEL_ROW;
    if ((plan.fresh >> sid) & 1) {                                                    // reset and not fed since: whatever the memory holds
        row[0] = plan.g0[i]; row[1] = 0; row[2] = 0; row[3] = 0;
        return;
    }
    row[0] = lstate[sid].a_next; row[1] = state[sid].hops; row[2] = (long)clip[sid]; row[3] = lstate[sid].P;
}

extern "C" int mimi_ld_pool_create(int n_streams, int ring_hops, mimi_ld_pool* out) {
    return sp_create("mimi_ld_pool_create", n_streams, out, ld_ring_bad(ring_hops), [&](MimiLdPool* p) {
        p->ring = ring_hops ? ring_hops : LD_RING_DEFAULT;
        hipError_t e = p->get(&p->carry_dev, sizeof(int16_t) * 2 * LD_CARRY * (size_t)n_streams, 0);
        if (e == hipSuccess) e = p->get(&p->state_dev, sizeof(LdState) * n_streams, 0);
        if (e == hipSuccess) e = p->get(&p->peak_dev, sizeof(int) * n_streams, 0);
        if (e == hipSuccess) e = p->get(&p->ring_dev, sizeof(long) * (size_t)p->ring * n_streams, 0);
        if (e == hipSuccess) e = p->get(&p->lstate_dev, sizeof(LdLvState) * n_streams, 0);
        if (e == hipSuccess) e = p->get(&p->clip_dev, sizeof(unsigned long long) * n_streams, 0);
        return e;
    });
}

extern "C" void mimi_ld_pool_destroy(mimi_ld_pool p) { delete p; }

extern "C" const char* mimi_ld_pool_last_error(mimi_ld_pool p) { return sp_last_error(p); }

extern "C" int mimi_ld_pool_reset(mimi_ld_pool p, const int32_t* streams, int n) {
    return p ? sp_status(p, ld_reset(p->n_streams, p->st, streams, n)) : -1;
}

extern "C" long mimi_ld_pool_hop_count(mimi_ld_pool p, int sid, long n_in, int final) {
    (void)final;                                                                      // a partial hop is never measured, final or not
    return sp_count_ok(p, sid, n_in) ? ld_hop_count(p->st[sid], n_in) : -1;
}

extern "C" int mimi_ld_pool_feed(mimi_ld_pool p, const int32_t* streams, const long* in_off, const long* n_in, const int32_t* final, int n,
                                 const void* in, int in_is_i16, long* energy, long* n_hops, void* stream) {
    if (!p) return -1;
    LdPlan plan;
    LdStream next[SP_MAX_STREAMS];
    if (int rc = sp_status(p, ld_plan_build(p->n_streams, p->st, streams, in_off, n_in, final, n, in, in_is_i16, energy, n_hops, &plan, next)))
        return rc;
    (void)hipGetLastError();
    if (plan.hops > 0) {
        k_ld_energy<<<dim3((unsigned)plan.hops), dim3(LD_THREADS), 0, (hipStream_t)stream>>>(plan, p->carry_dev, in, in_is_i16, energy, p->peak_dev,
                                                                                             nullptr);
        SP_HIP(p, hipGetLastError());
    }
    k_ld_scan<<<dim3((unsigned)plan.n), dim3(64), 0, (hipStream_t)stream>>>(plan, p->ring, p->carry_dev, p->state_dev, p->peak_dev, p->ring_dev,
                                                                           in, in_is_i16, energy);
    SP_HIP(p, hipGetLastError());
    sp_commit(p->st, streams, next, n);
    return 0;
}

extern "C" int mimi_ld_pool_integrate(mimi_ld_pool p, const int32_t* streams, int n, long* out, void* stream) {
    if (!p) return -1;
    if (int rc = sp_status(p, ld_integrate_bad(p->n_streams, streams, n, out))) return rc;
    LdIntPlan plan = {};
    plan.n = n; plan.ring = p->ring;
    for (int i = 0; i < n; ++i) plan.sid[i] = (uint8_t)streams[i];
    for (int i = 0; i < p->n_streams; ++i)
        if (!p->st[i].touched) plan.fresh |= 1ull << i;
    (void)hipGetLastError();
    k_ld_integrate<<<dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream>>>(plan, p->state_dev, p->ring_dev, out);
    SP_HIP(p, hipGetLastError());
    return 0;
}

extern "C" int mimi_ld_pool_level_reset(mimi_ld_pool p, const int32_t* streams, const long* pt, const int32_t* ceiling, const int32_t* g0_q16,
                                        const int32_t* gmax_q16, const int32_t* slew_shift, int n) {
    return p ? sp_status(p, ld_level_reset(p->n_streams, p->st, p->lv, streams, pt, ceiling, g0_q16, gmax_q16, slew_shift, n)) : -1;
}

extern "C" int mimi_ld_pool_level_feed(mimi_ld_pool p, const int32_t* streams, const long* in_off, const long* n_in, const int32_t* final, int n,
                                       const void* in, int in_is_i16, void* out, long* energy, int32_t* gain, long* n_hops, void* stream) {
    if (!p) return -1;
    LdPlan plan;
    LdLevelPlan lp;
    LdApPlan ap;
    LdStream next[SP_MAX_STREAMS];
    if (int rc = sp_status(p, ld_level_plan_build(p->n_streams, p->st, p->lv, streams, in_off, n_in, final, n, in, in_is_i16, out, energy, gain,
                                                  n_hops, &plan, &lp, &ap, next)))
        return rc;
    (void)hipGetLastError();
    if (plan.hops > 0) {
        k_ld_energy<<<dim3((unsigned)plan.hops), dim3(LD_THREADS), 0, (hipStream_t)stream>>>(plan, p->carry_dev, in, in_is_i16, energy, p->peak_dev,
                                                                                             gain);
        SP_HIP(p, hipGetLastError());
    }
    k_ld_level_scan<<<dim3((unsigned)plan.n), dim3(64), 0, (hipStream_t)stream>>>(plan, lp, p->ring, p->carry_dev, p->state_dev, p->peak_dev,
                                                                                 p->ring_dev, p->lstate_dev, p->clip_dev, in, in_is_i16, energy,
                                                                                 gain);
    SP_HIP(p, hipGetLastError());
    if (ap.tiles > 0) {
        if (in_is_i16) k_ld_apply<true><<<dim3((unsigned)ap.tiles), dim3(LD_AP_THREADS), 0, (hipStream_t)stream>>>(ap, in, out, gain, p->clip_dev);
        else k_ld_apply<false><<<dim3((unsigned)ap.tiles), dim3(LD_AP_THREADS), 0, (hipStream_t)stream>>>(ap, in, out, gain, p->clip_dev);
        SP_HIP(p, hipGetLastError());
    }
    sp_commit(p->st, streams, next, n);
    return 0;
}

extern "C" int mimi_ld_pool_level_state(mimi_ld_pool p, const int32_t* streams, int n, long* out, void* stream) {
    if (!p) return -1;
    if (int rc = sp_status(p, ld_level_state_bad(p->n_streams, p->st, streams, n, out))) return rc;
    LdLsPlan plan = {};
    plan.n = n;
    for (int i = 0; i < n; ++i) { plan.sid[i] = (uint8_t)streams[i]; plan.g0[i] = (int)p->lv[streams[i]].g0; }
    for (int i = 0; i < p->n_streams; ++i)
        if (!p->st[i].touched) plan.fresh |= 1ull << i;
    (void)hipGetLastError();
    k_ld_level_state<<<dim3(1), dim3(64), 0, (hipStream_t)stream>>>(plan, p->state_dev, p->lstate_dev, p->clip_dev, out);
    SP_HIP(p, hipGetLastError());
    return 0;
}
