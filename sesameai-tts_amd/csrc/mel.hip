// A pool of stateful Whisper log-mel streams on the device (mimi_mel_pool_*, include/mimi_hip.h states the rule; tests/mel_ref.py in
// NumPy): the input of every Whisper-family recogniser, computed WHILE the turn is spoken, for up to 64 streams at once.  TWO launches per
// feed whatever the number of streams and their chunk lengths:
//   k_mel_carry   one workgroup per listed stream: the samples from the next unemitted frame's first sample on go, as fp32, into the bank
//                 that the call did not read.
//   k_mel_frames  one workgroup of 7 waves per (stream, tile of 32 frames).  It stages the tile's span of 5360 samples in LDS -- rule zeros
//                 and reflection, the carry, the chunk -- and forms the windowed frames as the A operand from there on the fly.
//                   1. the 400-point DFT as a matrix product on v_mfma_f32_32x32x2_f32: wave w owns bins 32 w .. 32 w + 31 and keeps TWO
//                      independent accumulators, the cos and the -sin column tile of its bins, over the 200 k-steps; the basis comes
//                      from global memory (it stays in L2), 128 bytes a half-wave;
//                   2. re^2 + im^2 in registers -- both accumulators have the same lane map -- and into LDS as P[frame][bin];
//                   3. P times the filter bank with the same instruction, one wave per 32 mel bands, the even and the odd k-steps in two
//                      accumulators that are added at the end;
//                   4. floor, log10, and rows of n_mels fp32 out.
//                 Exact fp32 throughout: gfx950 has no reduced-precision form of this instruction and none is wanted here.
// NUMERICAL RULE.  A frame's values depend on its own 400 samples only: an MFMA output row is a k-ordered fp32 fmaf chain over ITS row of
// A, whatever rows share the tile, and every zero the rule asks for is a select, never a product.  So a stream's raw rows, concatenated
// over any chunk schedule, company or list order, are bit for bit its one-shot rows, and a non-finite sample stays inside the frames that
// read it.
// mimi_mel_finish, at the end of this file: the clip's maximum, then clamp, shift, scale and transpose, stateless.
// The plans (mel_plan.h) travel in the kernel arguments: no host-to-device copy, no allocation, no synchronisation.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/mimi_hip.h"
#include "stream_pool.cuh"
#include "mel_plan.h"

static_assert(MIMI_MEL_MAX_STREAMS == MEL_MAX_STREAMS && MIMI_MEL_CAP == MEL_CAP && MIMI_MEL_FRAMES == MEL_FRAMES &&
              MIMI_MEL_BASIS_COLS == MEL_BASIS_COLS && MIMI_MEL_MAX_MELS == MEL_MAX_MELS && MIMI_MEL_MAX_CLIPS == MEL_MAX_CLIPS &&
              MIMI_MEL_BINS_PAD == MEL_BINS_PAD, "header and plan disagree");
static_assert(sizeof(MelSeg) == 48 && sizeof(MelPlan) <= 3600 && sizeof(MelFinPlan) <= 3600, "the plans must fit the kernel arguments");
static_assert(MEL_NFFT % 2 == 0 && MEL_BINS_PAD % 32 == 0 && MEL_HOP % 2 == 0, "whole k-steps, whole column tiles");

typedef float mel_v16 __attribute__((ext_vector_type(16)));

struct MimiMelPool : SpPool<MelStream> {
    int n_mels = 0;
    float* window_dev = nullptr;     // [400]
    float* basis_dev = nullptr;      // [400][BASIS_COLS]
    float* bank_dev = nullptr;       // [BINS_PAD][MAX_MELS]
    float* carry_dev = nullptr;      // [n_streams][2 banks][MEL_CARRY]
};

// sample r of the clip as this call has it: below R0 from the carry, from there on from the chunk
template <bool I16>
__device__ __forceinline__ float mel_sample(const MelSeg& g, int r, const float* __restrict__ carry, const void* __restrict__ in) {
    if (r < g.R0) {
        const int c = r - g.c0;
        return c >= 0 && c < MEL_CARRY ? carry[c] : 0.0f;                              // (always inside: a frame to come reads nothing older)
    }
    const long at = g.in_off + (r - g.R0);                                            // r < R1 = R0 + n_use
    return I16 ? (float)((const short*)in)[at] * (1.0f / 32768.0f) : ((const float*)in)[at];
}

template <bool I16>
__global__ void __launch_bounds__(256) k_mel_carry(const MelPlan plan, float* __restrict__ banks, const void* __restrict__ in) {
    const MelSeg& g = plan.seg[blockIdx.x];
    const int sid = SP_SID(g);
    const float* rd = banks + ((long)sid * 2 + SP_PARITY(g)) * MEL_CARRY;
    float* wr = banks + ((long)sid * 2 + (SP_PARITY(g) ^ 1)) * MEL_CARRY;
    const int keep = g.R1 - g.c1;                                                      // < 400
    for (int i = threadIdx.x; i < keep && i < MEL_CARRY; i += blockDim.x) wr[i] = mel_sample<I16>(g, g.c1 + i, rd, in);
}

// LDS image of the span: sample j of the tile at j + j / 160, so that the 32 frames' samples of one k lie in 32 different banks
#define MEL_SPAN_LDS (MEL_SPAN + MEL_SPAN / MEL_HOP + 1)
#define MEL_P_STRIDE (MEL_BINS_PAD + 1)

template <bool I16>
__global__ void __launch_bounds__(MEL_THREADS) k_mel_frames(const MelPlan plan, const float* __restrict__ window, const float* __restrict__ basis,
                                                           const float* __restrict__ bank, const float* __restrict__ banks,
                                                           const void* __restrict__ in, float* __restrict__ raw) {
    __shared__ float S[MEL_SPAN_LDS];
    __shared__ float W[MEL_NFFT];
    __shared__ float P[MEL_TILE * MEL_P_STRIDE];
    const int owner = sp_owner(plan.seg, plan.n, &MelSeg::t_off);
    const MelSeg& g = plan.seg[owner];
    const int tile = (int)blockIdx.x - g.t_off;
    const int f0 = g.t0 + tile * MEL_TILE;                                             // the tile's first frame of the clip
    const int rows = min(MEL_TILE, g.t0 + g.nf - f0);
    if (rows <= 0) return;                                                             // (uniform; a grid has no such workgroup)
    const float* carry = banks + ((long)SP_SID(g) * 2 + SP_PARITY(g)) * MEL_CARRY;
    const int q0 = f0 * MEL_HOP - MEL_PAD;
    const int span = (rows - 1) * MEL_HOP + MEL_NFFT;
    for (int j = threadIdx.x; j < MEL_SPAN; j += MEL_THREADS) {
        float v = 0.0f;
        if (j < span) {
            const int r = mel_source(q0 + j, g.R1);
            if (r >= 0) v = mel_sample<I16>(g, r, carry, in);
        }
        S[j + j / MEL_HOP] = v;
    }
    for (int j = threadIdx.x; j < MEL_NFFT; j += MEL_THREADS) W[j] = window[j];
    __syncthreads();

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, col = lane & 31, half = lane >> 5;
    {   // 1. and 2.: the DFT of the wave's 32 bins for all 32 frames, then the power
        mel_v16 re = {}, im = {};
        const float* bc = basis + wave * 32 + col;                                     // the cos column; its -sin column is BINS_PAD further
        const int fbase = col * (MEL_HOP + 1);                                         // frame `col` starts at sample 160 col of the span
#pragma unroll 4
        for (int step = 0; step < MEL_NFFT / 2; ++step) {
            const int k = 2 * step + half;
            const float a = S[fbase + k + (k >= MEL_HOP) + (k >= 2 * MEL_HOP)] * W[k];
            const float bcv = bc[(long)k * MEL_BASIS_COLS], bsv = bc[(long)k * MEL_BASIS_COLS + MEL_BINS_PAD];
            re = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bcv, re, 0, 0, 0);
            im = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bsv, im, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * half;                          // the frame; the lane's column is the bin
            P[row * MEL_P_STRIDE + wave * 32 + col] = re[r] * re[r] + im[r] * im[r];
        }
    }
    __syncthreads();
    if (wave * 32 >= plan.n_mels) return;                                              // 3 or 4 waves go on
    {   // 3. and 4.
        mel_v16 e = {}, o = {};
        const float* fb = bank + wave * 32 + col;
#pragma unroll 2
        for (int step = 0; step < MEL_BINS_PAD / 2; step += 2) {
            const int k = 2 * step + half;
            e = __builtin_amdgcn_mfma_f32_32x32x2f32(P[col * MEL_P_STRIDE + k], fb[k * MEL_MAX_MELS], e, 0, 0, 0);
            o = __builtin_amdgcn_mfma_f32_32x32x2f32(P[col * MEL_P_STRIDE + k + 2], fb[(k + 2) * MEL_MAX_MELS], o, 0, 0, 0);
        }
        const int m = wave * 32 + col;
        if (m >= plan.n_mels) return;
        float* out = raw + ((long)g.row_off + tile * MEL_TILE) * plan.n_mels + m;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
            const float v = e[r] + o[r];
            if (row < rows) out[(long)row * plan.n_mels] = v <= MEL_FLOOR ? MEL_LOG_FLOOR : log10f(v);
        }
    }
}

extern "C" int mimi_mel_pool_create(int n_mels, int n_streams, mimi_mel_pool* out) {
    return sp_create("mimi_mel_pool_create", n_streams, out, mel_mels_bad(n_mels), [&](MimiMelPool* p) {
        p->n_mels = n_mels;
        std::vector<float> w(MEL_NFFT), b((size_t)MEL_NFFT * MEL_BASIS_COLS), f((size_t)MEL_BINS_PAD * MEL_MAX_MELS);
        mel_tables(n_mels, w.data(), b.data(), f.data());
        hipError_t e = p->get(&p->window_dev, sizeof(float) * w.size());
        if (e == hipSuccess) e = p->get(&p->basis_dev, sizeof(float) * b.size());
        if (e == hipSuccess) e = p->get(&p->bank_dev, sizeof(float) * f.size());
        if (e == hipSuccess) e = p->get(&p->carry_dev, sizeof(float) * 2 * MEL_CARRY * (size_t)n_streams, 0);
        if (e == hipSuccess) e = hipMemcpy(p->window_dev, w.data(), sizeof(float) * w.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(p->basis_dev, b.data(), sizeof(float) * b.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(p->bank_dev, f.data(), sizeof(float) * f.size(), hipMemcpyHostToDevice);
        return e;
    });
}

extern "C" void mimi_mel_pool_destroy(mimi_mel_pool p) { delete p; }

extern "C" const char* mimi_mel_pool_last_error(mimi_mel_pool p) { return sp_last_error(p); }

extern "C" int mimi_mel_pool_reset(mimi_mel_pool p, const int32_t* streams, int n) {
    return p ? sp_status(p, mel_reset(p->n_streams, p->st, streams, n)) : -1;
}

extern "C" int mimi_mel_pool_tables(mimi_mel_pool p, float* window, float* basis, float* bank) {
    if (!p) return -1;
    if (!window || !basis || !bank) return sp_status(p, "null pointer");
    SP_HIP(p, hipMemcpy(window, p->window_dev, sizeof(float) * MEL_NFFT, hipMemcpyDeviceToHost));
    SP_HIP(p, hipMemcpy(basis, p->basis_dev, sizeof(float) * MEL_NFFT * MEL_BASIS_COLS, hipMemcpyDeviceToHost));
    SP_HIP(p, hipMemcpy(bank, p->bank_dev, sizeof(float) * MEL_BINS_PAD * MEL_MAX_MELS, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" long mimi_mel_pool_frame_count(mimi_mel_pool p, int sid, long n_in, int final) {
    if (!sp_count_ok(p, sid, n_in)) return -1;
    return mel_frame_count(p->st[sid], n_in, final != 0);
}

extern "C" long mimi_mel_pool_dropped(mimi_mel_pool p, int sid) {
    if (!sp_count_ok(p, sid, 0)) return -1;
    return p->st[sid].dropped;
}

template <bool I16> static int mel_launch(MimiMelPool* p, const MelPlan& plan, const void* in, float* raw, hipStream_t s) {
    k_mel_carry<I16><<<dim3((unsigned)plan.n), dim3(256), 0, s>>>(plan, p->carry_dev, in);
    SP_HIP(p, hipGetLastError());
    if (plan.tiles > 0) {
        k_mel_frames<I16><<<dim3((unsigned)plan.tiles), dim3(MEL_THREADS), 0, s>>>(plan, p->window_dev, p->basis_dev, p->bank_dev, p->carry_dev, in, raw);
        SP_HIP(p, hipGetLastError());
    }
    return 0;
}

extern "C" int mimi_mel_pool_feed(mimi_mel_pool p, const int32_t* streams, const long* in_off, const long* n_in, const int32_t* final, int n,
                                  const void* in, int fmt, float* raw, long* n_frames, void* stream) {
    if (!p) return -1;
    MelPlan plan;
    MelStream next[SP_MAX_STREAMS];
    if (int rc = sp_status(p, mel_plan_build(p->n_streams, p->n_mels, p->st, streams, in_off, n_in, final, n, in, fmt, raw, n_frames, &plan, next)))
        return rc;
    (void)hipGetLastError();
    hipStream_t s = (hipStream_t)stream;
    if (int rc = fmt ? mel_launch<true>(p, plan, in, raw, s) : mel_launch<false>(p, plan, in, raw, s)) return rc;
    sp_commit(p->st, streams, next, n);
    return 0;
}


// ---- the stateless finisher: mimi_mel_finish ----
// k_mel_fin_max   one workgroup per clip: the largest raw value of its rows (the floor's -10 if frames are missing) goes into the LAST
//                 element of the clip's output, and a zero into the one before it: a count.
// k_mel_fin       one workgroup per (clip, tile of 32 frames): it reads the maximum, then counts itself in; rows in through LDS, columns out,
//                 (max(raw, maximum - 8) + 4) / 4; the frames the clip lacks get the constant.  The two elements that carried the maximum
//                 and the count are written by the workgroup that counts itself in LAST: every other has read the maximum by then.  No
//                 workgroup waits for another.
__global__ void __launch_bounds__(1024) k_mel_fin_max(const MelFinPlan plan, const float* __restrict__ raw, float* __restrict__ out) {
    __shared__ float part[16];
    const MelFinSeg& g = plan.seg[blockIdx.x];
    const long total = (long)g.n_frames * plan.n_mels;
    const float* rows = raw + g.off;
    float m = g.n_frames < MEL_FRAMES ? MEL_LOG_FLOOR : -INFINITY;
    for (long i = threadIdx.x; i < total; i += 1024) m = fmaxf(m, rows[i]);
    for (int d = 32; d > 0; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 16; ++i) m = fmaxf(m, part[i]);
        float* o = out + ((long)blockIdx.x + 1) * plan.n_mels * MEL_FRAMES;
        o[-1] = m;
        ((unsigned*)o)[-2] = 0u;
    }
}

__device__ __forceinline__ float mel_feature(float v, float lo) { return (fmaxf(v, lo) + 4.0f) * 0.25f; }

__global__ void __launch_bounds__(256) k_mel_fin(const MelFinPlan plan, const float* __restrict__ raw, float* __restrict__ out) {
    __shared__ float T[MEL_TILE * (MEL_MAX_MELS + 1)];
    __shared__ float s_max;
    __shared__ unsigned s_rank;
    const int clip = blockIdx.x / MEL_FIN_TILES, tile = blockIdx.x % MEL_FIN_TILES, n_mels = plan.n_mels;
    const MelFinSeg& g = plan.seg[clip];
    float* o = out + (long)clip * n_mels * MEL_FRAMES;
    float* slot = o + (long)n_mels * MEL_FRAMES - 2;                                  // the count, then the maximum
    if (threadIdx.x == 0) {
        s_max = __hip_atomic_load(slot + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_rank = __hip_atomic_fetch_add((unsigned*)slot, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);      // the read above comes first
    }
    const int f0 = tile * MEL_TILE, rows = min(MEL_TILE, MEL_FRAMES - f0);
    for (int i = threadIdx.x; i < rows * n_mels; i += 256) {
        const int r = i / n_mels, m = i - r * n_mels;
        T[r * (MEL_MAX_MELS + 1) + m] = f0 + r < g.n_frames ? raw[g.off + (long)(f0 + r) * n_mels + m] : MEL_LOG_FLOOR;
    }
    __syncthreads();
    const float lo = s_max - 8.0f;
    const bool last = s_rank == MEL_FIN_TILES - 1;
    for (int i = threadIdx.x; i < MEL_TILE * n_mels; i += 256) {
        const int m = i / MEL_TILE, r = i % MEL_TILE;
        const long at = (long)m * MEL_FRAMES + f0 + r;
        if (r < rows && at < (long)n_mels * MEL_FRAMES - 2) o[at] = mel_feature(T[r * (MEL_MAX_MELS + 1) + m], lo);
    }
    if (last && threadIdx.x < 2) {                                                     // frames 2998 and 2999 of the last band
        const int f = MEL_FRAMES - 2 + threadIdx.x;
        const float v = f < g.n_frames ? raw[g.off + (long)f * n_mels + n_mels - 1] : MEL_LOG_FLOOR;
        slot[threadIdx.x] = mel_feature(v, lo);
    }
}

static thread_local std::string g_mel_err;

extern "C" const char* mimi_mel_last_error(void) { return g_mel_err.c_str(); }

extern "C" int mimi_mel_finish(const float* raw, const long* off, const long* n_frames, int n, int n_mels, float* out, void* stream) {
    MelFinPlan plan;
    if (const char* bad = mel_fin_plan_build(raw, off, n_frames, n, n_mels, out, &plan)) { g_mel_err = bad; return -1; }
    (void)hipGetLastError();
    hipStream_t s = (hipStream_t)stream;
    k_mel_fin_max<<<dim3((unsigned)n), dim3(1024), 0, s>>>(plan, raw, out);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        k_mel_fin<<<dim3((unsigned)(n * MEL_FIN_TILES)), dim3(256), 0, s>>>(plan, raw, out);
        e = hipGetLastError();
    }
    if (e != hipSuccess) { g_mel_err = std::string("mimi_mel_finish: ") + hipGetErrorString(e); return -2; }
    return 0;
}
