// A pool of stateful look-ahead peak-limiter streams on the device (mimi_lim_pool_*, include/mimi_hip.h states the rule; tests/limiter_ref.py
// in NumPy): a gain that starts to fall L samples AHEAD of a peak, reaches what the peak requires exactly on it and recovers at rho per
// sample, in exact integers, for up to 64 streams at once.  TWO launches per feed whatever the number of streams and their chunk lengths:
//   k_lim_carry   one workgroup per listed stream: the required gains of the stream's last K + 2 L positions and its held samples go into
//                 the bank that the call did not read; a fresh stream's state row starts here, and the row's count of emitted samples moves.
//   k_lim_apply   one workgroup per (stream, tile of 4096 outputs).  It stages the required gains m of its tile and of the halo -- L ahead,
//                 K + L behind -- in LDS and computes steps 3 to 5 there, every sample independent of every other tile:
//                   3. w = the minimum of m over L + 1: log2(L + 1) doubling passes between two buffers and one pass that joins two windows;
//                   4. e[r] = min over j <= r of (w[j] + (r - j) rho) = r rho + prefix minimum of (w[j] - j rho): ONE workgroup scan from the
//                      halo's first position on, in TILE-RELATIVE indices (below 2^31 whatever the stream's length).  Terms further back than K
//                      cannot win (w <= ONE <= K rho), so the scan's start K behind the first e the tile needs loses nothing;
//                   5. the box sum over L + 1 as a difference of two exclusive prefix sums: a second workgroup scan (a tile's sum of gains is
//                      below 2^31), and one division a sample.
//                 The samples come in as 16-byte lines of `in` and wait in LDS; they leave as 16-byte lines of `out`, whatever the two
//                 buffers' alignment to each other -- a stream's outputs are packed, so its in and out offsets differ by what it holds.
//                 The state row takes one atomicMin and two atomicAdd per workgroup that has something to say: exact in any order.
// The plan (limiter_plan.h) travels in the kernel arguments: no host-to-device copy, no allocation, no synchronisation.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/mimi_hip.h"
#include "stream_pool.cuh"
#include "limiter_plan.h"

static_assert(MIMI_LIM_MAX_STREAMS == LIM_MAX_STREAMS && MIMI_LIM_ROW == LIM_ROW, "header and plan disagree");
static_assert(sizeof(LimSeg) == 56 && sizeof(LimPlan) <= 3600, "the plan must fit the kernel arguments");

typedef unsigned long long lim_u64;
typedef int lim_v4i __attribute__((ext_vector_type(4)));

struct MimiLimPool : SpPool<LimStream> {
    int* bank_dev = nullptr;         // [n_streams][2 banks][LIM_BANK]: required gains of the last K + 2 L positions, then the held samples
    lim_u64* row_dev = nullptr;      // [n_streams][LIM_ROW]
    bool lds_asked[2] = {false, false};      // k_lim_apply<fmt> may take its LDS
};

// step 1: the magnitude of a sample, as the bits the banks and the LDS hold (fp32: the float's; int16: the value)
template <bool I16> __device__ __forceinline__ int lim_mag(int raw, int hr) {
    if (I16) return abs(raw * (1 << hr));
    const float t = fabsf(__int_as_float(raw)) * (float)(1 << (15 + hr));              // exact scaling
    if (!(t == t)) return 0;                                                          // a NaN asks for nothing
    return t >= (float)LIM_A_MAX ? LIM_A_MAX : (int)ceilf(t);
}
// step 2
__device__ __forceinline__ int lim_need(int a, int C) { return a <= C ? LIM_ONE : (int)(((unsigned)C << 16) / (unsigned)a); }

template <bool I16> __device__ __forceinline__ int lim_raw(const void* __restrict__ in, long at) {
    return I16 ? (int)((const int16_t*)in)[at] : ((const int*)in)[at];
}

// exclusive scan over the workgroup's LIM_THREADS values, in thread order; sc: LIM_THREADS / 64 words of LDS, free again on return
template <class Op> __device__ __forceinline__ int lim_wg_scan(int v, int identity, Op op, int* sc) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d);
        if (lane >= d) inc = op(o, inc);
    }
    if (lane == 63) sc[w] = inc;
    __syncthreads();
    int pre = identity;
    for (int j = 0; j < w; ++j) pre = op(pre, sc[j]);
    int exc = __shfl_up(inc, 1);
    if (lane == 0) exc = identity;
    __syncthreads();
    return op(pre, exc);
}

template <bool I16>
__global__ void __launch_bounds__(LIM_THREADS) k_lim_carry(const LimPlan plan, int* __restrict__ bank, const void* __restrict__ in,
                                                           lim_u64* __restrict__ rows) {
    const LimSeg& g = plan.seg[blockIdx.x];
    const int t = threadIdx.x, sid = SP_SID(g), fresh = g.fresh, n_in = g.n_in, nh = g.nh;
    if (t == 0) {
        lim_u64* row = rows + (long)sid * LIM_ROW;
        if (fresh) { row[0] = LIM_ONE; row[1] = (lim_u64)g.n_out; row[2] = 0; row[3] = 0; }          // a fresh stream reads no state
        else row[1] += (lim_u64)g.n_out;
    }
    if (SP_FINAL(g)) return;                                                          // the next call finds the stream fresh
    const int* old = bank + ((long)sid * 2 + SP_PARITY(g)) * LIM_BANK;
    int* nw = bank + ((long)sid * 2 + (SP_PARITY(g) ^ 1)) * LIM_BANK;
    const int H = g.K + 2 * g.L, C = g.C, hr = g.hr;
    for (int i = t; i < H; i += LIM_THREADS) {                                        // the gains of the positions n_in - H .. n_in
        const int p = n_in - H + i;                                                   // (p < 0: the old bank's index p + H = n_in + i < H)
        nw[i] = p >= 0 ? lim_need(lim_mag<I16>(lim_raw<I16>(in, g.in_off + p), hr), C) : fresh ? LIM_ONE : old[p + H];
    }
    const int nh2 = nh + n_in - g.n_out;                                              // held after the call: <= L
    for (int j = t; j < nh2; j += LIM_THREADS) {
        const int p = n_in - nh2 + j;                                                 // (p < 0: the old bank holds it at p + nh >= n_out >= 0)
        nw[LIM_HIST_MAX + j] = p >= 0 ? lim_raw<I16>(in, g.in_off + p) : old[LIM_HIST_MAX + p + nh];
    }
}

// step 6 for one sample: its bits in, its bits out
template <bool I16> __device__ __forceinline__ int lim_out(int raw, int gq, int hr, float Cf, int* clamped) {
    if (I16) return (int)(((long)(raw * (1 << hr)) * gq + (1 << 15)) >> 16);               // (never outside [-C, C]: g <= m)
    const float xs = __fmul_rn(__int_as_float(raw), (float)(1 << hr));
    const float y = __fmul_rn(xs, (float)gq * 0x1p-16f);                              // gq <= 2^16: the factor is exact
    const bool hi = y > Cf, lo = y < -Cf;                                             // (a NaN is neither)
    *clamped += hi | lo;
    return __float_as_int(hi ? Cf : lo ? -Cf : y);
}

template <bool I16>
__global__ void __launch_bounds__(LIM_THREADS) k_lim_apply(const LimPlan plan, const int* __restrict__ bank, const void* __restrict__ in,
                                                           void* __restrict__ out, lim_u64* __restrict__ rows) {
    extern __shared__ int lim_lds[];
    __shared__ int sc[LIM_THREADS / 64];
    __shared__ int red[LIM_THREADS / 64][3];
    constexpr int ESZ = I16 ? 2 : 4, PER = LIM_VEC / ESZ, LINES = LIM_TILE / PER;
    const LimSeg& g = plan.seg[sp_owner(plan.seg, plan.n, &LimSeg::t_off)];
    const int t = threadIdx.x, tile = (int)blockIdx.x - g.t_off;
    int t_lo, t_hi, b, p_end;
    lim_tile_range(g, tile, &t_lo, &t_hi);
    lim_halo(g, t_lo, t_hi, &b, &p_end);                                              // LDS index i is the call's position b + i
    const int T = t_hi - t_lo;
    if (T <= 0) return;                                                               // (never: every tile of the plan owns an output)
    const int L = g.L, K = g.K, rho = g.rho, C = g.C, hr = g.hr, nh = g.nh, n_in = g.n_in, H = K + 2 * L;
    const int n_m = p_end - b, n_w = n_m - L;                                         // T + K + 2 L required gains, T + K + L window minima
    int* A = lim_lds;
    int* B = lim_lds + plan.lds_words;
    int* X = lim_lds + 2 * plan.lds_words;                                            // the tile's samples: X[o] is output t_lo + o
    const int* old = bank + ((long)SP_SID(g) * 2 + SP_PARITY(g)) * LIM_BANK;
    const int p_out = t_lo - nh;                                                      // the position of the tile's first output

    // steps 1 and 2.  In front of the call: the carry (a fresh stream has none: ONE)
    for (int i = t; i < min(n_m, -b); i += LIM_THREADS) A[i] = g.fresh ? LIM_ONE : old[b + i + H];
    for (int o = t; o < min(T, nh - t_lo); o += LIM_THREADS) X[o] = old[LIM_HIST_MAX + t_lo + o];
    // behind what the stream has received (only a final call looks there): silence
    for (int i = max(n_in - b, 0) + t; i < n_m; i += LIM_THREADS) A[i] = LIM_ONE;
    // the call's own samples, by 16-byte lines of `in`
    {
        const int lo = max(b, 0), hi = min(p_end, n_in);
        const char* src = (const char*)in + g.in_off * ESZ;
        const int l0 = (lo + g.mis_in) / PER, l1 = (hi + g.mis_in + PER - 1) / PER;
        for (int l = l0 + t; l < l1 && lo < hi; l += LIM_THREADS) {
            const int q0 = l * PER - g.mis_in;
            int raw[PER];
            if (q0 >= 0 && q0 + PER <= n_in) {
                const lim_v4i v = *(const lim_v4i*)(src + (long)q0 * ESZ);
#pragma unroll
                for (int c = 0; c < PER; ++c) raw[c] = I16 ? (int)(int16_t)(v[c / 2] >> (16 * (c & 1))) : v[c];
            } else {
#pragma unroll
                for (int c = 0; c < PER; ++c) raw[c] = q0 + c >= 0 && q0 + c < n_in ? lim_raw<I16>(src, q0 + c) : 0;
            }
#pragma unroll
            for (int c = 0; c < PER; ++c) {
                const int p = q0 + c;
                if (p < lo || p >= hi) continue;
                A[p - b] = lim_need(lim_mag<I16>(raw[c], hr), C);
                const int o = p - p_out;
                if (o >= 0 && o < T) X[o] = raw[c];
            }
        }
    }
    __syncthreads();

    // step 3: A[i] becomes min m[i .. i + L].  A read past the end is moved to the end: it shortens a window that no output needs whole
    int* src_ = A;
    int* dst_ = B;
    int span = 1;
    while (span < L + 1) {
        const int off = min(span, L + 1 - span);                                      // doubles while it can, then joins two windows to L + 1
        for (int i = t; i < n_m; i += LIM_THREADS) dst_[i] = min(src_[i], src_[min(i + off, n_m - 1)]);
        __syncthreads();
        int* const sw = src_; src_ = dst_; dst_ = sw;
        span += off;
    }

    // step 4: thread t walks its own run of `per` window minima (odd: its neighbours' runs start in other banks)
    const int per = ((n_w + LIM_THREADS - 1) / LIM_THREADS) | 1;
    const int i0 = min(t * per, n_w), i1 = min(i0 + per, n_w);
    int run = INT_MAX;
    for (int i = i0; i < i1; ++i) run = min(run, src_[i] - i * rho);
    run = lim_wg_scan(run, INT_MAX, [](int a, int c) { return min(a, c); }, sc);
    int sum = 0;
    for (int i = i0; i < i1; ++i) {
        run = min(run, src_[i] - i * rho);
        const int e = run + i * rho;                                                  // 0 <= e <= w[i]; the true e[i] from i = K on
        src_[i] = e;
        sum += e;
    }
    // step 5: src_[i] becomes e[0] + .. + e[i - 1], for i up to n_w
    sum = lim_wg_scan(sum, 0, [](int a, int c) { return a + c; }, sc);
    for (int i = i0; i < i1; ++i) {
        const int e = src_[i];
        src_[i] = sum;
        sum += e;
    }
    if (i1 == n_w && i0 < i1) src_[n_w] = sum;
    __syncthreads();

    // steps 5 and 6, by 16-byte lines of `out`: output o of the tile sits at index K + L + o, its box is e[K + o .. K + L + o]
    char* dst = (char*)out + g.out_off * ESZ;
    const float Cf = (float)C * 0x1p-15f;
    const unsigned box = (unsigned)(L + 1);
    int g_min = LIM_ONE, limited = 0, clamped = 0;
#pragma unroll
    for (int r = 0; r < LINES / LIM_THREADS; ++r) {
        const int q0 = (tile * LINES + r * LIM_THREADS + t) * PER - g.mis_out;        // the line's first output, of the stream's n_out
        if (q0 >= g.n_out || q0 + PER <= 0) continue;
        int y[PER];
#pragma unroll
        for (int c = 0; c < PER; ++c) {
            const int o = q0 + c - t_lo;
            if (o < 0 || o >= T) { y[c] = 0; continue; }
            const int gq = (int)((unsigned)(src_[K + L + o + 1] - src_[K + o]) / box);
            g_min = min(g_min, gq);
            limited += gq < LIM_ONE;
            y[c] = lim_out<I16>(X[o], gq, hr, Cf, &clamped);
        }
        if (q0 >= 0 && q0 + PER <= g.n_out) {
            lim_v4i v;
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = I16 ? (y[2 * c] & 0xFFFF) | (int)((unsigned)y[2 * c + 1] << 16) : y[c];
            *(lim_v4i*)(dst + (long)q0 * ESZ) = v;
        } else {
#pragma unroll
            for (int c = 0; c < PER; ++c) {
                if (q0 + c < 0 || q0 + c >= g.n_out) continue;
                if (I16) ((int16_t*)dst)[q0 + c] = (int16_t)y[c];
                else ((int*)dst)[q0 + c] = y[c];
            }
        }
    }
    g_min = wave_min_i(g_min); limited = wave_sum_i(limited); clamped = wave_sum_i(clamped);
    if ((t & 63) == 0) { red[t >> 6][0] = g_min; red[t >> 6][1] = limited; red[t >> 6][2] = clamped; }
    __syncthreads();
    if (t == 0) {
        int mn = LIM_ONE, lim = 0, cl = 0;
        for (int w = 0; w < LIM_THREADS / 64; ++w) { mn = min(mn, red[w][0]); lim += red[w][1]; cl += red[w][2]; }
        lim_u64* row = rows + (long)SP_SID(g) * LIM_ROW;
        if (mn < LIM_ONE) atomicMin(row + 0, (lim_u64)mn);
        if (lim > 0) atomicAdd(row + 2, (lim_u64)lim);
        if (cl > 0) atomicAdd(row + 3, (lim_u64)cl);
    }
}

struct LimStPlan { int n, pad; lim_u64 fresh; uint8_t sid[LIM_MAX_STREAMS]; };

__global__ void __launch_bounds__(64) k_lim_state(const LimStPlan plan, const lim_u64* __restrict__ rows, long* __restrict__ out) {
    const int i = threadIdx.x;
    if (i >= plan.n) return;
    const int sid = plan.sid[i];
    long* row = out + (long)i * LIM_ROW;
    if ((plan.fresh >> sid) & 1) {                                                    // reset and not fed since: whatever the memory holds
        row[0] = LIM_ONE; row[1] = 0; row[2] = 0; row[3] = 0;
        return;
    }
    for (int k = 0; k < LIM_ROW; ++k) row[k] = (long)rows[(long)sid * LIM_ROW + k];
}

extern "C" int mimi_lim_pool_create(int n_streams, mimi_lim_pool* out) {
    return sp_create("mimi_lim_pool_create", n_streams, out, nullptr, [&](MimiLimPool* p) {
        hipError_t e = p->get(&p->bank_dev, sizeof(int) * 2 * LIM_BANK * (size_t)n_streams, 0);
        if (e == hipSuccess) e = p->get(&p->row_dev, sizeof(lim_u64) * LIM_ROW * n_streams, 0);
        return e;
    });
}

extern "C" void mimi_lim_pool_destroy(mimi_lim_pool p) { delete p; }

extern "C" const char* mimi_lim_pool_last_error(mimi_lim_pool p) { return sp_last_error(p); }

extern "C" int mimi_lim_pool_reset(mimi_lim_pool p, const int32_t* streams, const int32_t* ceiling, const int32_t* lookahead, const int32_t* rho,
                                   const int32_t* drive_shift, int n) {
    return p ? sp_status(p, lim_reset(p->n_streams, p->st, streams, ceiling, lookahead, rho, drive_shift, n)) : -1;
}

extern "C" long mimi_lim_pool_out_count(mimi_lim_pool p, int sid, long n_in, int final) {
    if (!sp_count_ok(p, sid, n_in)) return -1;
    if (sp_status(p, p->st[sid].set ? nullptr : "a stream without parameters: mimi_lim_pool_reset gives them") != 0) return -1;
    return lim_out_count(p->st[sid], n_in, final != 0);
}

template <bool I16> static int lim_launch(MimiLimPool* p, const LimPlan& plan, const void* in, void* out, hipStream_t s) {
    const size_t lds = sizeof(int) * (2 * (size_t)plan.lds_words + LIM_TILE);
    if (plan.tiles > 0 && lds > 64 * 1024 && !p->lds_asked[I16]) {                    // (host work, once per pool and format: no device call)
        SP_HIP(p, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_lim_apply<I16>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)(sizeof(int) * LIM_LDS_MAX)));
        p->lds_asked[I16] = true;
    }
    k_lim_carry<I16><<<dim3((unsigned)plan.n), dim3(LIM_THREADS), 0, s>>>(plan, p->bank_dev, in, p->row_dev);
    SP_HIP(p, hipGetLastError());
    if (plan.tiles > 0) {
        k_lim_apply<I16><<<dim3((unsigned)plan.tiles), dim3(LIM_THREADS), lds, s>>>(plan, p->bank_dev, in, out, p->row_dev);
        SP_HIP(p, hipGetLastError());
    }
    return 0;
}

extern "C" int mimi_lim_pool_feed(mimi_lim_pool p, const int32_t* streams, const long* in_off, const long* n_in, const int32_t* final, int n,
                                  const void* in, void* out, long* n_out, int fmt, void* stream) {
    if (!p) return -1;
    LimPlan plan;
    LimStream next[SP_MAX_STREAMS];
    if (int rc = sp_status(p, lim_plan_build(p->n_streams, p->st, streams, in_off, n_in, final, n, in, out, n_out, fmt, &plan, next))) return rc;
    (void)hipGetLastError();
    if (int rc = fmt ? lim_launch<true>(p, plan, in, out, (hipStream_t)stream) : lim_launch<false>(p, plan, in, out, (hipStream_t)stream))
        return rc;
    sp_commit(p->st, streams, next, n);
    return 0;
}

extern "C" int mimi_lim_pool_state(mimi_lim_pool p, const int32_t* streams, int n, long* out, void* stream) {
    if (!p) return -1;
    if (int rc = sp_status(p, lim_state_bad(p->n_streams, streams, n, out))) return rc;
    LimStPlan plan = {};
    plan.n = n;
    for (int i = 0; i < n; ++i) plan.sid[i] = (uint8_t)streams[i];
    for (int i = 0; i < p->n_streams; ++i)
        if (!p->st[i].touched) plan.fresh |= 1ull << i;
    (void)hipGetLastError();
    k_lim_state<<<dim3(1), dim3(64), 0, (hipStream_t)stream>>>(plan, p->row_dev, out);
    SP_HIP(p, hipGetLastError());
    return 0;
}
