// A pool of stateful polyphase resampler streams on the device (mimi_rs_pool_*, include/mimi_hip.h): audio at any sample rate in front of and
// behind the 24 kHz codec.  ONE launch per call whatever the number of streams and their chunk lengths; the plan (resample_plan.h) travels in
// the kernel arguments: no host-to-device copy, no synchronisation.
//
// One output = one thread's sequential fp32 fmaf chain over its in-clip samples in ascending order: nothing about it depends on the tiling, on
// the chunk schedule or on the company in the call, so a stream's outputs are bit for bit the one-shot result of its concatenated samples.
// The samples in front of a call's first come from the stream's history (hist = 2 * half / up + 1 fp32 samples).  Each stream has TWO history
// banks: the call's output blocks read the bank the stream's state names, its history block writes the other one, and the host flips the
// stream's bank once the launch is made -- no block can see a half-written history, and no second launch is needed.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/mimi_hip.h"
#include "resample_plan.h"
#include "stream_pool.cuh"

static_assert(MIMI_RS_MAX_STREAMS == RS_MAX_STREAMS, "header and plan disagree");
static_assert(sizeof(RsPlan) <= 3200, "the plan must fit the kernel arguments");

struct MimiResamplePool : SpPool<RsStream> {
    RsRates r{};
    std::vector<float> taps;         // float32(h), as the device holds them
    float* taps_dev = nullptr;       // [2 * half + 1]
    float* hist_dev = nullptr;       // [n_streams][2 banks][hist]
};

__device__ __forceinline__ long rs_fdiv(long a, int b) { long q = a / b; return (a % b != 0 && a < 0) ? q - 1 : q; }     // b > 0

template <int FMT> __device__ __forceinline__ float rs_load(const void* in, long i) {
    if (FMT == 0) return ((const float*)in)[i];
    return (float)((const int16_t*)in)[i] * (1.0f / 32768.0f);                       // exact
}

template <int FMT> __device__ __forceinline__ void rs_store(void* out, long i, float y) {
    if (FMT == 0) { ((float*)out)[i] = y; return; }
    float c = y != y ? 0.0f : fminf(fmaxf(y, -1.0f), 1.0f);
    ((int16_t*)out)[i] = (int16_t)__float2int_rn(c * 32767.0f);                       // round to nearest even
}

template <int IFMT, int OFMT>
__global__ void __launch_bounds__(RS_BLOCK) k_rs_feed(const RsPlan plan, const float* __restrict__ taps, float* __restrict__ hist,
                                                      const void* __restrict__ in, void* __restrict__ out, int up, int down, int half, int H) {
    const int b = blockIdx.x;
    if (b >= plan.blocks) {
        // history block of segment b - blocks: the H samples in front of the stream's NEXT call, into the bank this call does not read
        const RsSeg& g = plan.seg[b - plan.blocks];
        const float* old = hist + ((long)g.sid * 2 + g.bank) * H;
        float* nw = hist + ((long)g.sid * 2 + (g.bank ^ 1)) * H;
        for (int d = threadIdx.x; d < H; d += RS_BLOCK) {
            const long idx = (long)g.n_in - H + d;                                    // >= -H
            nw[d] = idx >= 0 ? rs_load<IFMT>(in, g.in_off + idx) : old[H + idx];
        }
        return;
    }
    int i = 0;
    while (i + 1 < plan.n && plan.seg[i + 1].blk0 <= b) ++i;                         // (segment, first output) of this block
    const RsSeg& g = plan.seg[i];
    const int j = (b - g.blk0) * RS_BLOCK + threadIdx.x;
    if (j >= g.n_out) return;
    const long c = (long)(g.n0 + j) * down + half;                                    // tap index of sample 0; >= 0
    long klo = -rs_fdiv(-(c - 2L * half), up), khi = rs_fdiv(c, up);                  // the samples its taps cover
    const long kend = (long)g.k_base + g.n_in;
    klo = klo > g.k0 ? klo : g.k0;                                                    // in front of the clip: zero by index, never read
    klo = klo > (long)g.k_base - H ? klo : (long)g.k_base - H;                        // (the plan never asks for more; keeps the read in bounds)
    khi = khi < kend - 1 ? khi : kend - 1;                                            // behind the clip's end (final): zero
    const float* hs = hist + ((long)g.sid * 2 + g.bank) * H + H;
    float acc = 0.0f;
    for (long k = klo; k <= khi; ++k) {
        const long d = k - g.k_base;
        const float x = d >= 0 ? rs_load<IFMT>(in, g.in_off + d) : hs[d];
        acc = fmaf(taps[c - k * up], x, acc);
    }
    rs_store<OFMT>(out, g.out_off + j, acc);
}

extern "C" int mimi_rs_pool_create(int src_rate, int dst_rate, int n_streams, mimi_rs_pool* out) {
    RsRates r;
    const char* bad = rs_rates(src_rate, dst_rate, &r);
    return sp_create("mimi_rs_pool_create", n_streams, out, bad, [&](MimiResamplePool* p) {
        p->r = r;
        const std::vector<double> h = rs_taps(r);
        p->taps.resize(h.size());
        for (size_t i = 0; i < h.size(); ++i) p->taps[i] = (float)h[i];               // rounded once
        const size_t taps_bytes = sizeof(float) * p->taps.size();
        hipError_t e = p->get(&p->taps_dev, taps_bytes);
        if (e == hipSuccess) e = p->get(&p->hist_dev, sizeof(float) * 2 * (size_t)r.hist * n_streams, 0);
        if (e == hipSuccess) e = hipMemcpy(p->taps_dev, p->taps.data(), taps_bytes, hipMemcpyHostToDevice);
        return e;
    });
}

extern "C" void mimi_rs_pool_destroy(mimi_rs_pool p) { delete p; }

extern "C" const char* mimi_rs_pool_last_error(mimi_rs_pool p) { return sp_last_error(p); }

extern "C" int mimi_rs_pool_taps(mimi_rs_pool p, float* host_out, int* up, int* down, int* half) {
    if (!p) return -1;
    if (up) *up = p->r.up;
    if (down) *down = p->r.down;
    if (half) *half = p->r.half;
    if (host_out) for (size_t i = 0; i < p->taps.size(); ++i) host_out[i] = p->taps[i];
    return 0;
}

extern "C" long mimi_rs_pool_out_count(mimi_rs_pool p, int sid, long n_in, int final) {
    return sp_count_ok(p, sid, n_in) ? rs_emitted(p->r, p->st[sid].n_in, p->st[sid].n_out, n_in, final != 0) - p->st[sid].n_out : -1;
}

extern "C" int mimi_rs_pool_reset(mimi_rs_pool p, const int32_t* streams, int n) {
    return p ? sp_status(p, rs_reset(p->n_streams, p->st, streams, n)) : -1;
}

extern "C" int mimi_rs_pool_feed(mimi_rs_pool p, const int32_t* streams, const long* in_off, const long* n_in, const int32_t* final, int n,
                                 const void* in, int in_fmt, void* out, int out_fmt, long* n_out, void* stream) {
    if (!p) return -1;
    RsPlan plan;
    RsStream next[SP_MAX_STREAMS];
    if (int rc = sp_status(p, rs_plan_build(p->r, p->n_streams, p->st, streams, in_off, n_in, final, n, in, in_fmt, out, out_fmt, n_out, &plan, next)))
        return rc;
    const dim3 grid((unsigned)(plan.blocks + plan.n)), block(RS_BLOCK);
    hipStream_t s = (hipStream_t)stream;
    const RsRates& r = p->r;
    (void)hipGetLastError();
    if (in_fmt == 0 && out_fmt == 0) k_rs_feed<0, 0><<<grid, block, 0, s>>>(plan, p->taps_dev, p->hist_dev, in, out, r.up, r.down, r.half, r.hist);
    else if (in_fmt == 0) k_rs_feed<0, 1><<<grid, block, 0, s>>>(plan, p->taps_dev, p->hist_dev, in, out, r.up, r.down, r.half, r.hist);
    else if (out_fmt == 0) k_rs_feed<1, 0><<<grid, block, 0, s>>>(plan, p->taps_dev, p->hist_dev, in, out, r.up, r.down, r.half, r.hist);
    else k_rs_feed<1, 1><<<grid, block, 0, s>>>(plan, p->taps_dev, p->hist_dev, in, out, r.up, r.down, r.half, r.hist);
    SP_HIP(p, hipGetLastError());
    sp_commit(p->st, streams, next, n);
    return 0;
}
