// The segment finisher on the device (mimi_fin_*, include/mimi_hip.h): fp32 clips -> peak-normalised int16 with lead and tail silence and linear
// fades, the arithmetic of TTS.generate_audio_segment (finish_plan.h states the rule).  One call is TWO launches for all of its segments,
// whatever their number and lengths: k_fin_peak writes one partial max |x| per (segment, peak tile), k_fin_write's blocks each reduce their
// segment's partials and write their int16 outputs -- silence, quantised samples and both fades in one pass, by global index.  The plan travels
// in the kernel arguments: no memset, no atomics, no allocation, no host copy, no synchronisation.
//
// Every output is a function of its own sample, its segment's peak and its index in the segment.  max is exact whatever the order, so nothing
// depends on the tiling, on the company in the call or on list order.  The division is the correctly rounded IEEE one (this file is built
// without fast-math); the ramp is float64 per faded sample, rounded once to fp32.
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include <string>

#include "../../include/mimi_hip.h"
#include "common.cuh"
#include "finish_plan.h"
#include "loudness_plan.h"

static_assert(MIMI_FIN_MAX_SEGMENTS == FIN_MAX_SEGMENTS, "header and plan disagree");
static_assert(sizeof(FinPlan) <= 3200, "the plan must fit the kernel arguments");
static_assert(FIN_MAX_PTILES <= FIN_BLOCK && FIN_OUT_TILE == 8 * FIN_BLOCK, "a write block: one partial and four pairs per thread");

#define FIN_PEAK_FLOOR 1e-6f

struct MimiFinisher {
    float* partials = nullptr;      // [FIN_MAX_SEGMENTS][FIN_MAX_PTILES], made at create: enough for any legal call
    std::string err;
};

static thread_local std::string g_fin_err;

// max over the block's 4 waves; every thread gets it
__device__ __forceinline__ float fin_block_max(float v, float* sh) {
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}

__global__ void __launch_bounds__(FIN_BLOCK) k_fin_peak(const FinPlan plan, float* __restrict__ partials) {
    __shared__ float sh[FIN_BLOCK / 64];
    const int b = blockIdx.x;
    int i = 0;
    while (i + 1 < plan.n && plan.seg[i + 1].pblk0 <= b) ++i;                        // (segment, peak tile) of this block
    const FinSeg& g = plan.seg[i];
    const int tile = b - g.pblk0;
    const long lo = (long)tile * g.ptile;                                            // < n_in <= 2^30
    const long rest = (long)g.n_in - lo;
    const int cnt = (int)(rest < g.ptile ? rest : g.ptile);
    const float* x = g.in + lo;
    float m = 0.0f;
    for (int k = threadIdx.x; k < cnt; k += FIN_BLOCK) {
        const float a = fabsf(x[k]);
        m = a <= FLT_MAX ? fmaxf(m, a) : m;                                          // a NaN or an Inf does not enter the peak
    }
    m = fin_block_max(m, sh);
    if (threadIdx.x == 0) partials[i * FIN_MAX_PTILES + tile] = m;
}

// output j of segment g, 0 <= j < g.m
__device__ __forceinline__ int fin_sample(const FinSeg& g, float peak, int j) {
    int v = 0;
    const int d = j - g.lead;
    if (d >= 0 && d < g.n_in) {
        const float x = g.in[d];
        if (fabsf(x) <= FLT_MAX) v = (int)((x / peak) * 32767.0f);                   // |x| <= peak: inside int16; the cast truncates
    }
    const int n = g.nfade;                                                            // <= m / 2: the two fades never meet
    const int r = j < n ? j : (j >= g.m - n ? g.m - 1 - j : -1);
    if (r >= 0) {
        const float ramp = r == n - 1 ? (n == 1 ? 0.0f : 1.0f) : (float)((double)r * (1.0 / (double)(n - 1)));
        v = (int)((float)v * ramp);
    }
    return v;
}

__global__ void __launch_bounds__(FIN_BLOCK) k_fin_write(const FinPlan plan, const float* __restrict__ partials, int16_t* __restrict__ out) {
    __shared__ float sh[FIN_BLOCK / 64];
    const int b = blockIdx.x;
    int i = 0;
    while (i + 1 < plan.n && plan.seg[i + 1].wblk0 <= b) ++i;                        // (segment, output tile) of this block
    const FinSeg& g = plan.seg[i];
    const int n_pt = g.n_in == 0 ? 0 : (int)(((long)g.n_in + g.ptile - 1) / g.ptile);
    const float part = (int)threadIdx.x < n_pt ? partials[i * FIN_MAX_PTILES + threadIdx.x] : 0.0f;
    const float peak = fmaxf(fin_block_max(part, sh), FIN_PEAK_FLOOR);
    int16_t* o = out + g.out_off;
    const int p0 = (b - g.wblk0) * (FIN_OUT_TILE / 2);
#pragma unroll
    for (int k = 0; k < FIN_OUT_TILE / 2 / FIN_BLOCK; ++k) {
        const int j0 = 2 * (p0 + k * FIN_BLOCK + (int)threadIdx.x) - g.par;          // the aligned pair (j0, j0 + 1); j0 >= -1
        if (j0 >= g.m) continue;
        const bool has0 = j0 >= 0, has1 = j0 + 1 < g.m;
        const int v0 = has0 ? fin_sample(g, peak, j0) : 0;
        const int v1 = has1 ? fin_sample(g, peak, j0 + 1) : 0;
        if (has0 && has1) *(uint32_t*)(o + j0) = (uint32_t)(v0 & 0xFFFF) | ((uint32_t)v1 << 16);
        else if (has0) o[j0] = (int16_t)v0;                                          // the segment's last output, its pair half a neighbour's
        else if (has1) o[j0 + 1] = (int16_t)v1;                                      // its first output at an odd address
    }
}

// ---- mimi_fin_segments_ld: the same chain with a clip gain from the loudness meter's rows in the place of the peak rule ----
// A segment's gain, or 0 where it keeps the peak rule: float64 from integers, rounded once to fp32 (include/mimi_hip.h spells it out).
__device__ __forceinline__ float fin_ld_gain(long pt, int ceiling, const long* __restrict__ row) {
    const long S = row[0], nb = row[1], pk = row[2];
    if (pt <= 0 || nb <= 0 || S <= 0 || pk <= 0) return 0.0f;
    const double g1 = sqrt(((double)(pt * (4 * LD_H)) * (double)nb) / (double)S);
    const double g2 = (double)ceiling / (double)pk;
    return (float)(g1 < g2 ? g1 : g2);
}

// output j of segment g under the gain `gain` (> 0), 0 <= j < g.m
__device__ __forceinline__ int fin_sample_ld(const FinSeg& g, float gain, int j) {
    int v = 0;
    const int d = j - g.lead;
    if (d >= 0 && d < g.n_in) {
        const float x = g.in[d];
        if (fabsf(x) <= FLT_MAX) {
            const float u = fminf(fmaxf((x * gain) * 32767.0f, -32767.0f), 32767.0f);  // the bounds are integers: clamp and trunc commute
            v = (int)u;                                                               // the cast truncates
        }
    }
    const int n = g.nfade;
    const int r = j < n ? j : (j >= g.m - n ? g.m - 1 - j : -1);
    if (r >= 0) {
        const float ramp = r == n - 1 ? (n == 1 ? 0.0f : 1.0f) : (float)((double)r * (1.0 / (double)(n - 1)));
        v = (int)((float)v * ramp);
    }
    return v;
}

__global__ void __launch_bounds__(FIN_BLOCK) k_fin_write_ld(const FinPlan plan, const FinLd ld, const long* __restrict__ meter,
                                                            const float* __restrict__ partials, int16_t* __restrict__ out) {
    __shared__ float sh[FIN_BLOCK / 64];
    const int b = blockIdx.x;
    int i = 0;
    while (i + 1 < plan.n && plan.seg[i + 1].wblk0 <= b) ++i;                        // (segment, output tile) of this block
    const FinSeg& g = plan.seg[i];
    const int n_pt = g.n_in == 0 ? 0 : (int)(((long)g.n_in + g.ptile - 1) / g.ptile);
    const float part = (int)threadIdx.x < n_pt ? partials[i * FIN_MAX_PTILES + threadIdx.x] : 0.0f;
    const float peak = fmaxf(fin_block_max(part, sh), FIN_PEAK_FLOOR);
    const float gain = fin_ld_gain(ld.pt[i], ld.ceil[i], meter + (long)i * LD_ROW);  // uniform over the block
    int16_t* o = out + g.out_off;
    const int p0 = (b - g.wblk0) * (FIN_OUT_TILE / 2);
#pragma unroll
    for (int k = 0; k < FIN_OUT_TILE / 2 / FIN_BLOCK; ++k) {
        const int j0 = 2 * (p0 + k * FIN_BLOCK + (int)threadIdx.x) - g.par;          // the aligned pair (j0, j0 + 1); j0 >= -1
        if (j0 >= g.m) continue;
        const bool has0 = j0 >= 0, has1 = j0 + 1 < g.m;
        int v0 = 0, v1 = 0;
        if (gain > 0.0f) {
            v0 = has0 ? fin_sample_ld(g, gain, j0) : 0;
            v1 = has1 ? fin_sample_ld(g, gain, j0 + 1) : 0;
        } else {
            v0 = has0 ? fin_sample(g, peak, j0) : 0;
            v1 = has1 ? fin_sample(g, peak, j0 + 1) : 0;
        }
        if (has0 && has1) *(uint32_t*)(o + j0) = (uint32_t)(v0 & 0xFFFF) | ((uint32_t)v1 << 16);
        else if (has0) o[j0] = (int16_t)v0;
        else if (has1) o[j0 + 1] = (int16_t)v1;
    }
}

extern "C" int mimi_fin_segments_ld(mimi_finisher p, const float* const* in, const long* n_in, const int32_t* lead, const int32_t* tail,
                                    const int32_t* fade, const long* pt, const int32_t* ceiling, const long* meter, int n, int16_t* out,
                                    long* out_off, long* n_out, void* stream) {
    if (!p) return -1;
    FinPlan plan;
    FinLd ld;
    if (const char* bad = fin_plan_build(in, n_in, lead, tail, fade, n, out, out_off, n_out, &plan)) { p->err = bad; return -1; }
    if (const char* bad = fin_ld_build(pt, ceiling, n, meter, &ld)) { p->err = bad; return -1; }
    hipStream_t s = (hipStream_t)stream;
    (void)hipGetLastError();
    if (plan.pblocks > 0) k_fin_peak<<<dim3((unsigned)plan.pblocks), dim3(FIN_BLOCK), 0, s>>>(plan, p->partials);
    if (plan.wblocks > 0) k_fin_write_ld<<<dim3((unsigned)plan.wblocks), dim3(FIN_BLOCK), 0, s>>>(plan, ld, meter, p->partials, out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { p->err = std::string("mimi_fin_segments_ld: ") + hipGetErrorString(e); return -2; }
    return 0;
}

extern "C" int mimi_fin_create(mimi_finisher* out) {
    if (!out) { g_fin_err = "null pointer"; return -1; }
    *out = nullptr;
    MimiFinisher* p = new MimiFinisher();
    const hipError_t e = hipMalloc((void**)&p->partials, sizeof(float) * FIN_MAX_SEGMENTS * FIN_MAX_PTILES);
    if (e != hipSuccess) {
        g_fin_err = std::string("mimi_fin_create: ") + hipGetErrorString(e);
        mimi_fin_destroy(p);
        return -2;
    }
    *out = p;
    return 0;
}

extern "C" void mimi_fin_destroy(mimi_finisher p) {
    if (!p) return;
    if (p->partials) (void)hipFree(p->partials);
    delete p;
}

extern "C" const char* mimi_fin_last_error(mimi_finisher p) { return p ? p->err.c_str() : g_fin_err.c_str(); }

extern "C" long mimi_fin_out_count(long n_in, long lead, long tail) { return fin_out_count(n_in, lead, tail); }

extern "C" int mimi_fin_segments(mimi_finisher p, const float* const* in, const long* n_in, const int32_t* lead, const int32_t* tail,
                                 const int32_t* fade, int n, int16_t* out, long* out_off, long* n_out, void* stream) {
    if (!p) return -1;
    FinPlan plan;
    if (const char* bad = fin_plan_build(in, n_in, lead, tail, fade, n, out, out_off, n_out, &plan)) { p->err = bad; return -1; }
    hipStream_t s = (hipStream_t)stream;
    (void)hipGetLastError();
    if (plan.pblocks > 0) k_fin_peak<<<dim3((unsigned)plan.pblocks), dim3(FIN_BLOCK), 0, s>>>(plan, p->partials);
    if (plan.wblocks > 0) k_fin_write<<<dim3((unsigned)plan.wblocks), dim3(FIN_BLOCK), 0, s>>>(plan, p->partials, out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { p->err = std::string("mimi_fin_segments: ") + hipGetErrorString(e); return -2; }
    return 0;
}
