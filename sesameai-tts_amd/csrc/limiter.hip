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
// TRUE PEAKS (mimi_lim_pool_reset_tp; tests/truepeak_ref.py): both kernels take the mode as a second template parameter, and the
// sample-peak instantiations are what they were.  A true-peak stream's required gain reads the magnitude of the 4x oversampled signal on
// the sample and in the two intervals beside it, from the signed samples T = 8 on either side: k_lim_apply<.., true> stages those in its
// second buffer first (tp_walk below), the stream's history ends T positions back, and its bank also keeps the signed samples of its last
// 2 T positions.  A call that lists streams of both modes makes the two launches once per mode.  mimi_tp_measure, at the end of this
// file, is the same arithmetic as a stateless meter.
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
    int* bank_dev = nullptr;         // [n_streams][2 banks][LIM_BANK]: required gains of the last K + 2 L positions, then the held samples;
                                     // behind them [n_streams][2 banks][LIM_TP_BANK] for true-peak streams: the gains, the held samples,
                                     // the signed samples of the last 2 T positions
    lim_u64* row_dev = nullptr;      // [n_streams][LIM_ROW]
    bool lds_asked[2][2] = {};       // k_lim_apply<fmt, tp> may take its LDS
};

// The three fractional phases of the true-peak interpolator (truepeak_taps.h): tap j of phase p + 1, and taps 2 j, 2 j + 1 as an int16 pair
__device__ constexpr short TP_H[3 * 2 * TP_T] = {TP_TAPS_LIST};
__device__ __forceinline__ constexpr int tp_h(int p, int j) { return TP_H[p * 2 * TP_T + j]; }
__device__ __forceinline__ constexpr uint32_t tp_h2(int p, int j) {
    return ((uint32_t)tp_h(p, 2 * j) & 0xFFFFu) | ((uint32_t)tp_h(p, 2 * j + 1) << 16);
}

// The inter-sample magnitude of one interval: w[0 .. 2 T) are the signed samples from T in front of the interval to T - 1 behind it;
// the largest of the three phases' (|acc| + 2^13) >> 14.  !WIDE: every |w| < 2^15, int16 pairs and an int32 accumulator (it stays
// below 2^30); WIDE: 64 bits.  Either way the integer is the rule's.
template <bool WIDE> __device__ __forceinline__ int tp_interval(const int* w) {
    int best = 0;
    if (!WIDE) {
        uint32_t pk[TP_T];
#pragma unroll
        for (int j = 0; j < TP_T; ++j) pk[j] = ((uint32_t)w[2 * j] & 0xFFFFu) | ((uint32_t)w[2 * j + 1] << 16);
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            int acc = 0;
#pragma unroll
            for (int j = 0; j < TP_T; ++j) acc = dot2_i16(pk[j], tp_h2(p, j), acc);
            best = max(best, (abs(acc) + (1 << (TP_Q - 1))) >> TP_Q);
        }
    } else {
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            long acc = 0;
#pragma unroll
            for (int j = 0; j < 2 * TP_T; ++j) acc += (long)tp_h(p, j) * (long)w[j];
            best = max(best, (int)(((acc < 0 ? -acc : acc) + (1 << (TP_Q - 1))) >> TP_Q));        // (< 2^31)
        }
    }
    return best;
}

// The true-peak magnitudes of the positions [lo, hi) from signed samples in LDS: V[i] is the sample of position base + i, and
// [lo - T, hi + T) lies inside what V holds.  Every thread of the workgroup walks its own run of positions (an odd length: its
// neighbours' runs start in other banks) and keeps the magnitude of the interval it shares with the next position; done(r, a_tp) takes
// each result.  Wave-uniform: `wide` is the workgroup's.
template <bool WIDE, class Done> __device__ __forceinline__ void tp_walk_as(const int* V, int base, int lo, int hi, Done done) {
    const int n = hi - lo, per = ((n + LIM_THREADS - 1) / LIM_THREADS) | 1;
    const int i0 = min((int)threadIdx.x * per, n), i1 = min(i0 + per, n);
    if (i0 >= i1) return;
    const int* v = V + (lo + i0 - base);                                               // the sample of the run's first position
    int u = tp_interval<WIDE>(v - TP_T);                                               // the interval in front of it
    for (int i = i0; i < i1; ++i, ++v) {
        const int un = tp_interval<WIDE>(v - TP_T + 1);                                // the interval behind position lo + i
        done(lo + i, max(abs(*v), max(u, un)));
        u = un;
    }
}
template <class Done> __device__ __forceinline__ void tp_walk(bool wide, const int* V, int base, int lo, int hi, Done done) {
    if (wide) tp_walk_as<true>(V, base, lo, hi, done);
    else tp_walk_as<false>(V, base, lo, hi, done);
}

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
// true peak, step a: the signed sample, |v| <= 2^30 (a NaN: 0)
template <bool I16> __device__ __forceinline__ int tp_signed(int raw, int hr) {
    if (I16) return raw * (1 << hr);
    const int a = lim_mag<false>(raw, hr);
    return raw < 0 ? -a : a;                                                          // (the float's sign bit)
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

template <bool I16, bool TP>
__global__ void __launch_bounds__(LIM_THREADS) k_lim_carry(const LimPlan plan, int* __restrict__ bank, const void* __restrict__ in,
                                                           lim_u64* __restrict__ rows) {
    constexpr int BANK = TP ? LIM_TP_BANK : LIM_BANK;
    const LimSeg& g = plan.seg[blockIdx.x];
    const int t = threadIdx.x, sid = SP_SID(g), fresh = g.fresh, n_in = g.n_in, nh = g.nh;
    if (t == 0) {
        lim_u64* row = rows + (long)sid * LIM_ROW;
        if (fresh) { row[0] = LIM_ONE; row[1] = (lim_u64)g.n_out; row[2] = 0; row[3] = 0; }          // a fresh stream reads no state
        else row[1] += (lim_u64)g.n_out;
    }
    if (SP_FINAL(g)) return;                                                          // the next call finds the stream fresh
    const int* old = bank + ((long)sid * 2 + SP_PARITY(g)) * BANK;
    int* nw = bank + ((long)sid * 2 + (SP_PARITY(g) ^ 1)) * BANK;
    const int H = g.K + 2 * g.L, C = g.C, hr = g.hr;
    if constexpr (TP) {
        // the signed sample of position q < n_in: the call's, one of the 2 T the old bank keeps, or 0 in front of the clip
        constexpr int PEND = LIM_HIST_MAX + LIM_TP_HELD_MAX;
        const int pre = g.pre;
        auto v_at = [&](int q) {
            return q >= 0 ? tp_signed<I16>(lim_raw<I16>(in, g.in_off + q), hr) : q >= -pre ? old[PEND + q + 2 * TP_T] : 0;
        };
        // The gains of the positions n_in - T - H .. n_in - T.  Those of [c_lo, c_hi) are new: their signed samples, and T more on either
        // side, wait in LDS and are walked as k_lim_apply walks its halo; the others are the old bank's, or silence in front of the clip.
        __shared__ int V[LIM_HIST_MAX + 2 * TP_T];
        __shared__ int wide;
        int c_lo, c_hi;
        lim_tp_carried(g, &c_lo, &c_hi);
        if (t == 0) wide = 0;
        __syncthreads();
        for (int j = t; j < c_hi - c_lo + 2 * TP_T && c_lo < c_hi; j += LIM_THREADS) {
            const int v = v_at(c_lo - TP_T + j);                                      // (c_hi + T = n_in: nothing behind the call)
            V[j] = v;
            if (abs(v) >= (1 << 15)) wide = 1;
        }
        const int first = n_in - TP_T - H;
        for (int i = t; i < H; i += LIM_THREADS) {
            const int p = first + i;                                                  // (p < -T: the old bank's index p + T + H = n_in + i < H)
            if (p < -TP_T) nw[i] = fresh ? LIM_ONE : old[p + TP_T + H];
            else if (p < c_lo) nw[i] = LIM_ONE;                                       // in front of the clip
        }
        __syncthreads();
        tp_walk(wide != 0, V, c_lo - TP_T, c_lo, c_hi, [&](int r, int a_tp) { nw[r - first] = lim_need(a_tp, C); });
        if (t < 2 * TP_T) nw[PEND + t] = v_at(n_in - 2 * TP_T + t);
    } else {
        for (int i = t; i < H; i += LIM_THREADS) {                                    // the gains of the positions n_in - H .. n_in
            const int p = n_in - H + i;                                               // (p < 0: the old bank's index p + H = n_in + i < H)
            nw[i] = p >= 0 ? lim_need(lim_mag<I16>(lim_raw<I16>(in, g.in_off + p), hr), C) : fresh ? LIM_ONE : old[p + H];
        }
    }
    const int nh2 = nh + n_in - g.n_out;                                              // held after the call: <= L (true peak: <= L + T)
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

template <bool I16, bool TP>
__global__ void __launch_bounds__(LIM_THREADS) k_lim_apply(const LimPlan plan, const int* __restrict__ bank, const void* __restrict__ in,
                                                           void* __restrict__ out, lim_u64* __restrict__ rows) {
    extern __shared__ int lim_lds[];
    __shared__ int sc[LIM_THREADS / 64];
    __shared__ int red[LIM_THREADS / 64][3];
    __shared__ int tp_wide;                                                           // true peak: a staged |v| >= 2^15
    constexpr int BANK = TP ? LIM_TP_BANK : LIM_BANK, TPT = TP ? TP_T : 0;
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
    const int* old = bank + ((long)SP_SID(g) * 2 + SP_PARITY(g)) * BANK;
    const int p_out = t_lo - nh;                                                      // the position of the tile's first output
    // True peak: B first holds the signed samples V of the positions b - T .. p_end + T (B[i] is position vb + i); the required gains of
    // [c_lo, c_hi) are computed from them once they are all there, the others are the carry's or silence.
    const int vb = b - TPT;
    int c_lo = 0, c_hi = 0;
    if constexpr (TP) {
        lim_tp_computed(g, b, p_end, &c_lo, &c_hi);
        if (t == 0) tp_wide = 0;
        __syncthreads();
    }

    // steps 1 and 2.  In front of the call: the carry (a fresh stream has none: ONE)
    for (int i = t; i < min(n_m, -TPT - b); i += LIM_THREADS) A[i] = g.fresh ? LIM_ONE : old[b + i + TPT + H];
    for (int o = t; o < min(T, nh - t_lo); o += LIM_THREADS) X[o] = old[LIM_HIST_MAX + t_lo + o];
    // behind what the stream has received (only a final call looks there): silence
    for (int i = max(n_in - b, 0) + t; i < n_m; i += LIM_THREADS) A[i] = LIM_ONE;
    if constexpr (TP) {
        for (int i = max(-TPT - b, 0) + t; i < min(n_m, c_lo - b); i += LIM_THREADS) A[i] = LIM_ONE;          // in front of the clip
        for (int i = t; i < n_m + 2 * TPT; i += LIM_THREADS) {                        // what the lines below do not bring
            const int q = vb + i;
            if (q < 0) {
                const int v = q >= -(int)g.pre ? old[LIM_HIST_MAX + LIM_TP_HELD_MAX + q + 2 * TPT] : 0;
                B[i] = v;
                if (abs(v) >= (1 << 15)) tp_wide = 1;
            } else if (q >= n_in) {
                B[i] = 0;
            }
        }
    }
    // the call's own samples, by 16-byte lines of `in`
    {
        const int lo = max(vb, 0), hi = min(p_end + TPT, n_in);
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
                if constexpr (TP) {
                    const int v = tp_signed<I16>(raw[c], hr);
                    B[p - vb] = v;
                    if (abs(v) >= (1 << 15)) tp_wide = 1;
                } else {
                    A[p - b] = lim_need(lim_mag<I16>(raw[c], hr), C);
                }
                const int o = p - p_out;
                if (o >= 0 && o < T) X[o] = raw[c];
            }
        }
    }
    __syncthreads();
    if constexpr (TP) {
        tp_walk(tp_wide != 0, B, vb, c_lo, c_hi, [&](int r, int a_tp) { A[r - b] = lim_need(a_tp, C); });
        __syncthreads();
    }

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
        hipError_t e = p->get(&p->bank_dev, sizeof(int) * 2 * (LIM_BANK + LIM_TP_BANK) * (size_t)n_streams, 0);
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

extern "C" int mimi_lim_pool_reset_tp(mimi_lim_pool p, const int32_t* streams, const int32_t* ceiling, const int32_t* lookahead,
                                      const int32_t* rho, const int32_t* drive_shift, const int32_t* true_peak, int n) {
    if (!p) return -1;
    if (!true_peak) return sp_status(p, "null pointer");
    return sp_status(p, lim_reset_tp(p->n_streams, p->st, streams, ceiling, lookahead, rho, drive_shift, true_peak, n));
}

extern "C" long mimi_lim_pool_out_count(mimi_lim_pool p, int sid, long n_in, int final) {
    if (!sp_count_ok(p, sid, n_in)) return -1;
    if (sp_status(p, p->st[sid].set ? nullptr : "a stream without parameters: mimi_lim_pool_reset gives them") != 0) return -1;
    return lim_out_count(p->st[sid], n_in, final != 0);
}

template <bool I16, bool TP> static int lim_launch(MimiLimPool* p, const LimPlan& plan, const void* in, void* out, hipStream_t s) {
    if (plan.n == 0) return 0;                                                        // no stream of this mode in the call
    const size_t lds = sizeof(int) * (2 * (size_t)plan.lds_words + LIM_TILE);
    if (plan.tiles > 0 && lds > 64 * 1024 && !p->lds_asked[I16][TP]) {                // (host work, once per pool, format and mode: no device call)
        SP_HIP(p, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_lim_apply<I16, TP>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)(sizeof(int) * (TP ? LIM_TP_LDS_MAX : LIM_LDS_MAX))));
        p->lds_asked[I16][TP] = true;
    }
    int* bank = p->bank_dev + (TP ? 2 * (size_t)LIM_BANK * p->n_streams : 0);         // the true-peak banks lie behind the others
    k_lim_carry<I16, TP><<<dim3((unsigned)plan.n), dim3(LIM_THREADS), 0, s>>>(plan, bank, in, p->row_dev);
    SP_HIP(p, hipGetLastError());
    if (plan.tiles > 0) {
        k_lim_apply<I16, TP><<<dim3((unsigned)plan.tiles), dim3(LIM_THREADS), lds, s>>>(plan, bank, in, out, p->row_dev);
        SP_HIP(p, hipGetLastError());
    }
    return 0;
}

extern "C" int mimi_lim_pool_feed(mimi_lim_pool p, const int32_t* streams, const long* in_off, const long* n_in, const int32_t* final, int n,
                                  const void* in, void* out, long* n_out, int fmt, void* stream) {
    if (!p) return -1;
    LimPlan plans[2];                                                                 // the call's sample-peak streams; its true-peak streams
    LimStream next[SP_MAX_STREAMS];
    if (int rc = sp_status(p, lim_plan_build_tp(p->n_streams, p->st, streams, in_off, n_in, final, n, in, out, n_out, fmt, plans, next))) return rc;
    (void)hipGetLastError();
    hipStream_t s = (hipStream_t)stream;
    if (int rc = fmt ? lim_launch<true, false>(p, plans[0], in, out, s) : lim_launch<false, false>(p, plans[0], in, out, s)) return rc;
    if (int rc = fmt ? lim_launch<true, true>(p, plans[1], in, out, s) : lim_launch<false, true>(p, plans[1], in, out, s)) return rc;
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


// ---- the stateless true-peak meter: mimi_tp_measure ----
// ONE launch over (clip, tile of 4096 positions) workgroups behind the memset that zeroes the rows.  A workgroup stages the signed samples
// of its tile and T more on either side and walks them as k_lim_apply's true-peak pass does.  Its largest true-peak magnitude and the
// first position that has it travel as ONE 64-bit key, (a_tp << 32) | ~position, into an atomicMax on the clip's row, so the row is exact
// in any order; the workgroup that finishes a clip last (a count in the row's last word) unpacks the key and writes n.
static_assert(MIMI_TP_MAX_CLIPS == TP_MAX_CLIPS && MIMI_TP_ROW == TP_ROW, "header and plan disagree");
static_assert(sizeof(TpPlan) <= 3600, "the plan must fit the kernel arguments");

template <bool I16>
__global__ void __launch_bounds__(LIM_THREADS) k_tp_measure(const TpPlan plan, const void* __restrict__ in, lim_u64* __restrict__ out) {
    __shared__ int V[LIM_TILE + 2 * TP_T];
    __shared__ lim_u64 keys[LIM_THREADS / 64];
    __shared__ int peaks[LIM_THREADS / 64];
    __shared__ int tp_wide;
    const int clip = sp_owner(plan.seg, plan.n, &TpSeg::t_off);
    const TpSeg& g = plan.seg[clip];
    const int t = threadIdx.x, tile = (int)blockIdx.x - g.t_off, n = g.n;
    const int r0 = tile * LIM_TILE, r1 = min(r0 + LIM_TILE, n), vb = r0 - TP_T;
    if (t == 0) tp_wide = 0;
    __syncthreads();
    int peak = 0;
    for (int i = t; i < r1 - r0 + 2 * TP_T; i += LIM_THREADS) {
        const int q = vb + i;
        const int v = q >= 0 && q < n ? tp_signed<I16>(lim_raw<I16>(in, g.in_off + q), 0) : 0;
        V[i] = v;
        if (abs(v) >= (1 << 15)) tp_wide = 1;
        if (q >= r0 && q < r1) peak = max(peak, abs(v));
    }
    __syncthreads();
    unsigned best_a = 0, best_r = 0;
    bool any = false;
    tp_walk(tp_wide != 0, V, vb, r0, r1, [&](int r, int a_tp) {
        if (!any || (unsigned)a_tp > best_a) { best_a = (unsigned)a_tp; best_r = (unsigned)r; any = true; }          // (ascending r: the first)
    });
    lim_u64 key = any ? ((lim_u64)best_a << 32) | (lim_u64)(0xFFFFFFFFu - best_r) : 0;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const lim_u64 o = __shfl_xor(key, d);
        key = o > key ? o : key;
    }
    peak = wave_max_i(peak);
    if ((t & 63) == 0) { keys[t >> 6] = key; peaks[t >> 6] = peak; }
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < LIM_THREADS / 64; ++w) { key = keys[w] > key ? keys[w] : key; peak = max(peak, peaks[w]); }
        lim_u64* row = out + (long)clip * MIMI_TP_ROW;
        atomicMax(row + 0, (lim_u64)peak);
        atomicMax(row + 1, key);
        __threadfence();
        const lim_u64 tiles = (lim_u64)((n + LIM_TILE - 1) / LIM_TILE);
        if (atomicAdd(row + 3, 1ull) == tiles - 1) {                                   // every other tile of the clip has put its key in
            __threadfence();
            const lim_u64 top = atomicMax(row + 1, 0ull);
            row[1] = top >> 32;
            row[2] = (lim_u64)(0xFFFFFFFFu - (unsigned)top);
            row[3] = (lim_u64)n;
        }
    }
}

static thread_local std::string g_tp_err;

extern "C" const char* mimi_tp_last_error(void) { return g_tp_err.c_str(); }

extern "C" int mimi_tp_measure(const void* in, const long* in_off, const long* n_in, int n, int fmt, long* out, void* stream) {
    TpPlan plan;
    if (const char* bad = tp_plan_build(in, in_off, n_in, n, fmt, out, &plan)) { g_tp_err = bad; return -1; }
    hipStream_t s = (hipStream_t)stream;
    (void)hipGetLastError();
    hipError_t e = hipMemsetAsync(out, 0, sizeof(long) * MIMI_TP_ROW * (size_t)n, s);
    if (e == hipSuccess && plan.tiles > 0) {
        if (fmt) k_tp_measure<true><<<dim3((unsigned)plan.tiles), dim3(LIM_THREADS), 0, s>>>(plan, in, (lim_u64*)out);
        else k_tp_measure<false><<<dim3((unsigned)plan.tiles), dim3(LIM_THREADS), 0, s>>>(plan, in, (lim_u64*)out);
        e = hipGetLastError();
    }
    if (e != hipSuccess) { g_tp_err = std::string("mimi_tp_measure: ") + hipGetErrorString(e); return -2; }
    return 0;
}
