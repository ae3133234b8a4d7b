// A pool of stateful WSOLA time-stretch streams on the device (mimi_ts_pool_*, include/mimi_hip.h states the rule): speech rate without a
// change of pitch, between the decoder and everything that follows it.  ONE launch per call whatever the number of streams and their chunk
// lengths, one workgroup per listed stream, which walks that stream's blocks of the call one after the other (block k needs c of block k - 1).
// The plan (stretch_plan.h) travels in the kernel arguments: no host-to-device copy, no allocation, no synchronisation.
//
// Per block the workgroup stages the 512 template and 1,024 region samples in LDS, as fp32 (the crossfade's two source runs) and quantised to
// 12 bits as packed int16 pairs.  Thread t scores candidates 2t and 2t + 1 with v_dot2 on the pairs: the even candidate reads the region's
// pairs as staged, the odd one the same pairs shifted by one sample, made in registers from two neighbouring words (v_alignbit) instead of a
// second packing in LDS -- half the LDS reads.  Lanes read consecutive words (no bank conflict), the template word is a broadcast.  The 513th
// candidate is one dot2 per thread and a sum.  A score is an exact integer below 2^31 in any order, so the argmax -- score descending,
// candidate ascending -- is the rule's, bit for bit.  The crossfade is two fp32 multiplies and an fp32 add, never fused.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mimi_hip.h"
#include "stream_pool.cuh"
#include "stretch_plan.h"

#pragma clang fp contract(off)

static_assert(MIMI_TS_MAX_STREAMS == TS_MAX_STREAMS, "header and plan disagree");
static_assert(sizeof(TsSeg) == 48 && sizeof(TsPlan) <= 3200, "the plan must fit the kernel arguments");
static_assert(TS_H == 512 && TS_D == 256, "k_ts_feed: 256 threads, two candidates and two outputs each");

#define TS_THREADS 256

struct MimiStretchPool : SpPool<TsStream> {
    float* carry_dev = nullptr;      // [n_streams][2 banks][TS_CARRY]
    int* c_dev = nullptr;            // [n_streams]: c of the stream's last block, relative to the base of its next call
};

// the 12-bit search samples: q = clamp(rint(x * 2048), -2047, 2047)
__device__ __forceinline__ int ts_quant(float x) { return quant_i16(x, 2048.0f, -2047.0f, 2047.0f); }
__device__ __forceinline__ uint32_t ts_pack(float x0, float x1) {
    return (uint32_t)(ts_quant(x0) & 0xFFFF) | ((uint32_t)ts_quant(x1) << 16);
}

// fl(fl(xc * r) + fl(xb * (1 - r))): the pragma above keeps the compiler from fusing a multiply into the add (the __fmul_rn / __fadd_rn of the
// HIP headers are compiled before it and do get fused)
__device__ __forceinline__ float ts_mix(float xc, float xb, float r) {
    const float u = xc * r, v = xb * (1.0f - r);
    return u + v;
}

// sample at position p relative to the call's base: the carry, then the new chunk, zero outside
__device__ __forceinline__ float ts_x(const float* __restrict__ carry, int L, const float* __restrict__ in, int n_in, int p) {
    if (p < 0) return 0.0f;
    if (p < L) return carry[p];
    p -= L;
    return p < n_in ? in[p] : 0.0f;
}

__global__ void __launch_bounds__(TS_THREADS) k_ts_feed(const TsPlan plan, float* __restrict__ carry, int* __restrict__ cpos,
                                                        const float* __restrict__ in_all, float* __restrict__ out_all, int32_t* __restrict__ d_out) {
    __shared__ float xr[2 * TS_H];               // region: sample a - D + i
    __shared__ float xt[TS_H];                   // template: sample b + j
    __shared__ uint32_t qr[TS_H];                // their 12-bit search samples as int16 pairs (2m, 2m + 1)
    __shared__ uint32_t qt[TS_H / 2];
    __shared__ int red_s[4], red_e[4], red_x[4];
    const TsSeg& g = plan.seg[blockIdx.x];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int sid = SP_SID(g), L = g.L < TS_CARRY ? g.L : TS_CARRY, n_in = g.n_in, n_out = g.n_out, pm = TS_PM(g);
    const float* old = carry + ((long)sid * 2 + SP_PARITY(g)) * TS_CARRY;
    const float* in = in_all + g.in_off;
    float* out = out_all + g.out_off;
    const int nb = (n_out + TS_H - 1) / TS_H;
    int c = TS_FRESH(g) ? 0 : cpos[sid];
    for (int i = 0; i < nb; ++i) {
        const int j0 = t, j1 = t + TS_THREADS, o = i * TS_H;
        if (i == 0 && TS_FRESH(g)) {                                                  // block 0: the clip's first samples as they are
            if (o + j0 < n_out) out[o + j0] = ts_x(old, L, in, n_in, j0);
            if (o + j1 < n_out) out[o + j1] = ts_x(old, L, in, n_in, j1);
            if (t == 0 && d_out) d_out[g.blk_off] = 0;
            c = 0;
            continue;
        }
        const int a = g.a0 + (int)(((long)TS_REM(g) + (long)i * (TS_H * pm)) / 1000);
        const int b = c + TS_H;
        __syncthreads();                                                              // the last block's crossfade has read xr and xt
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int m = t + r * TS_THREADS;
            const float x0 = ts_x(old, L, in, n_in, a - TS_D + 2 * m), x1 = ts_x(old, L, in, n_in, a - TS_D + 2 * m + 1);
            xr[2 * m] = x0; xr[2 * m + 1] = x1;
            qr[m] = ts_pack(x0, x1);
        }
        {
            const float x0 = ts_x(old, L, in, n_in, b + 2 * t), x1 = ts_x(old, L, in, n_in, b + 2 * t + 1);
            xt[2 * t] = x0; xt[2 * t + 1] = x1;
            qt[t] = ts_pack(x0, x1);
        }
        __syncthreads();
        // candidates e = d + D: 2t from the pairs as staged, 2t + 1 from the pairs one sample on
        int s0 = 0, s1 = 0;
        uint32_t cur = qr[t];
#pragma unroll 8
        for (int m = 0; m < TS_H / 2; ++m) {
            const uint32_t nxt = qr[t + m + 1 < TS_H ? t + m + 1 : TS_H - 1];         // (t + m + 1 <= 511 always; the clamp keeps the read provably inside)
            const uint32_t tq = qt[m];
            s0 = dot2_i16(cur, tq, s0);
            s1 = dot2_i16(__builtin_amdgcn_alignbit(nxt, cur, 16), tq, s1);
            cur = nxt;
        }
        int s = s0, e = 2 * t;
        if (s1 > s0) { s = s1; e = 2 * t + 1; }
        const int wm = wave_max_i(s);
        const int we = wave_min_i(s == wm ? e : 0x7FFFFFFF);
        const int px = wave_sum_i(dot2_i16(qr[TS_H / 2 + t], qt[t], 0));            // candidate 512, a 256th of it per thread
        if (lane == 0) { red_s[w] = wm; red_e[w] = we; red_x[w] = px; }
        __syncthreads();
        int best = red_s[0], be = red_e[0];
#pragma unroll
        for (int k = 1; k < 4; ++k)
            if (red_s[k] > best) { best = red_s[k]; be = red_e[k]; }                  // waves hold ascending candidates: > keeps the first
        if (red_x[0] + red_x[1] + red_x[2] + red_x[3] > best) be = 2 * TS_D;
        be = __builtin_amdgcn_readfirstlane(be);
        c = a + be - TS_D;
        if (t == 0 && d_out) d_out[g.blk_off + i] = be - TS_D;
        // y[j] = fl(fl(x[c + j] * r_j) + fl(x[b + j] * (1 - r_j))), r_j = j / 512
        const float r0 = (float)j0 * (1.0f / TS_H), r1 = (float)j1 * (1.0f / TS_H);
        const float y0 = ts_mix(xr[be + j0], xt[j0], r0), y1 = ts_mix(xr[be + j1], xt[j1], r1);
        if (o + j0 < n_out) out[o + j0] = y0;
        if (o + j1 < n_out) out[o + j1] = y1;
    }
    if (SP_FINAL(g)) return;                                                          // the stream is fresh: it reads neither carry nor c
    // the samples from the next call's base on, into the bank this call did not read
    float* nw = carry + ((long)sid * 2 + (SP_PARITY(g) ^ 1)) * TS_CARRY;
    int Ln = L + n_in - g.shift;
    Ln = Ln < TS_CARRY ? Ln : TS_CARRY;
    for (int p = t; p < Ln; p += TS_THREADS) nw[p] = ts_x(old, L, in, n_in, g.shift + p);
    if (t == 0) cpos[sid] = c - g.shift;
}

extern "C" int mimi_ts_pool_create(int n_streams, mimi_ts_pool* out) {
    return sp_create("mimi_ts_pool_create", n_streams, out, nullptr, [&](MimiStretchPool* p) {
        for (int i = 0; i < n_streams; ++i) p->st[i].pm = 1000;
        hipError_t e = p->get(&p->carry_dev, sizeof(float) * 2 * TS_CARRY * (size_t)n_streams, 0);
        if (e == hipSuccess) e = p->get(&p->c_dev, sizeof(int) * n_streams, 0);
        return e;
    });
}

extern "C" void mimi_ts_pool_destroy(mimi_ts_pool p) { delete p; }

extern "C" const char* mimi_ts_pool_last_error(mimi_ts_pool p) { return sp_last_error(p); }

extern "C" int mimi_ts_pool_reset(mimi_ts_pool p, const int32_t* streams, const int32_t* speed_pm, int n) {
    return p ? sp_status(p, ts_reset(p->n_streams, p->st, streams, speed_pm, n)) : -1;
}

extern "C" long mimi_ts_pool_out_count(mimi_ts_pool p, int sid, long n_in, int final) {
    return sp_count_ok(p, sid, n_in) ? ts_out_count(p->st[sid], n_in, final != 0) : -1;
}

extern "C" int mimi_ts_pool_feed(mimi_ts_pool p, const int32_t* streams, const long* in_off, const long* n_in, const int32_t* final, int n,
                                 const float* in, float* out, long* n_out, int32_t* d_out, void* stream) {
    if (!p) return -1;
    TsPlan plan;
    TsStream next[SP_MAX_STREAMS];
    if (int rc = sp_status(p, ts_plan_build(p->n_streams, p->st, streams, in_off, n_in, final, n, in, out, n_out, &plan, next))) return rc;
    (void)hipGetLastError();
    k_ts_feed<<<dim3((unsigned)plan.n), dim3(TS_THREADS), 0, (hipStream_t)stream>>>(plan, p->carry_dev, p->c_dev, in, out, d_out);
    SP_HIP(p, hipGetLastError());
    sp_commit(p->st, streams, next, n);
    return 0;
}
