// The Whisper encoder on the device (mimi_wenc_*, include/mimi_hip.h states the rule; tests/whisper_enc_ref.py in float64 torch): the
// recogniser's hot path -- every turn, however short, runs all n_ctx positions through all L layers.  fp16 operands on
// v_mfma_f32_32x32x16_f16, fp32 everything else.  2 + 7 L + 1 launches per encode, whatever the batch:
//   k_wenc_gemm<EPI, MI>  one LDS-tiled GEMM, out[M][N] = A[M][K] . W[N][K]^T, a workgroup of 4 waves (2 x 2) per 64 MI x 128 tile, 64-deep K
//                         slices of both operands through a double-buffered, XOR-swizzled LDS image (gemm128.cuh's), the next slice's global
//                         loads in flight while this one feeds the matrix cores.  Its operand A and its epilogue are the template's:
//                           CONV1  A formed while staging from the (n_mels, 2 n_ctx) fp32 features, k = tap n_mels + c (padded to 64s with
//                                  zeros); + bias, GELU -> fp16, time-major
//                           CONV2  A row t, tap j = row 2t - 1 + j of conv1's output, zero outside [0, 2 n_ctx): a 64-deep slice lies inside
//                                  one tap; + bias, GELU, + position row t -> the fp32 residual stream
//                           QKV    N = 3 d: + bias (k has none), q x 0.125 -> fp16, head-major [clip][head][t][64]
//                           RESID  + bias, += into the fp32 residual (out-proj and fc2): each element has ONE owner, no atomics
//                           FC1    + bias, erf-GELU -> fp16
//                         M and N tails: rows and columns past the end are clamped on load and not stored.
//   k_wenc_ln             one wave per row: two-pass mean and variance in fp32 from registers -> fp16, or the caller's format (the last)
//   k_wenc_attn           non-causal flash attention, head dim 64 (attn_flash.cuh's scheme): a workgroup per (clip, head, 128 queries), a
//                         wave per 32 queries; 64 keys of K and V per LDS buffer; S^T = K . Q^T, online softmax in fp32 in a lane pair,
//                         O^T += V^T . P^T with P^T the accumulator registers of S^T rounded to fp16.  A key past n_ctx has the score
//                         -inf: it gives nothing to the maximum and exactly 0 to the sum; its K and V rows are zeros in LDS.  Padding
//                         queries repeat the last one and are not stored.
// NUMERICAL RULE.  Every output element's K chain is one accumulator over k ascending in slices of 64, in either tile shape; a row of any
// kernel reads its own clip only.  So a clip's output has the same bits alone, at any place of any batch, and on every call.  The whole
// unit is compiled without floating-point contraction: what is fused is written as fmaf.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/mimi_hip.h"
#include "hip_backend.h"
#include "whisper_enc_plan.h"

#pragma clang fp contract(off)

static_assert(MIMI_WENC_MAX_LAYERS == WENC_MAX_LAYERS && MIMI_WENC_MAX_CTX == WENC_MAX_CTX && MIMI_WENC_MAX_BATCH == WENC_MAX_BATCH,
              "header and plan disagree");

typedef _Float16 we_h;
typedef _Float16 we_h2 __attribute__((ext_vector_type(2)));
typedef _Float16 we_h8 __attribute__((ext_vector_type(8)));
typedef float we_f16 __attribute__((ext_vector_type(16)));
typedef unsigned we_u4 __attribute__((ext_vector_type(4)));
typedef unsigned we_u2 __attribute__((ext_vector_type(2)));
typedef short we_s4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ we_h8 we_as_h8(const we_u4& v) { return __builtin_bit_cast(we_h8, v); }
__device__ __forceinline__ unsigned we_pack(float a, float b) {                       // two fp32 -> two fp16, round to nearest even
    we_h2 v;
    v[0] = (we_h)a; v[1] = (we_h)b;
    return __builtin_bit_cast(unsigned, v);
}
__device__ __forceinline__ float we_gelu(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f)); }

enum { WE_CONV1 = 0, WE_CONV2 = 1, WE_QKV = 2, WE_RESID = 3, WE_FC1 = 4 };

struct WencGemmArgs {
    const void* a;               // CONV1: the fp32 features; else fp16 rows of lda elements
    const we_h* w;               // [N][K]
    const float* bias;           // [N]
    const float* pos;            // CONV2: [T][N]
    float* resid;                // CONV2, RESID: [M][N]
    we_h* out;                   // CONV1, FC1: [M][N]
    we_h *q, *k, *v;             // QKV: [clip][head][T][64]
    int M, N, K, lda;            // K: a multiple of 64
    int T, d, H, n_mels;
};

#define WE_LD 64                                  // LDS row = one 64-deep K slice (128 B); 16-byte segments XOR-swizzled
#define WE_SMEM(MI) (2 * (64 * (MI) + 128) * WE_LD * 2)

// the 16 bytes (8 k) at k0 + 8 seg of operand A's row: clip b, row t of the clip, row m of the launch
template <int EPI>
__device__ __forceinline__ we_u4 we_a_piece(const WencGemmArgs& g, int b, int t, int m, int k0, int seg) {
    const we_u4 zero = {0u, 0u, 0u, 0u};
    if (EPI == WE_CONV1) {
        const int T2 = 2 * g.T;
        const float* f = (const float*)g.a + (long)b * g.n_mels * T2;
        we_h8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = k0 + seg * 8 + j, tap = k / g.n_mels, c = k - tap * g.n_mels, tt = t - 1 + tap;
            const bool ok = tap < 3 && tt >= 0 && tt < T2;
            const float x = ok ? f[(long)c * T2 + tt] : 0.0f;
            v[j] = (we_h)x;
        }
        return __builtin_bit_cast(we_u4, v);
    } else if (EPI == WE_CONV2) {
        const int tap = k0 / g.d, src = 2 * t - 1 + tap;
        const bool ok = src >= 0 && src < 2 * g.T;
        const we_h* p = (const we_h*)g.a + ((long)b * 2 * g.T + (ok ? src : 0)) * g.d + (k0 - tap * g.d) + seg * 8;
        const we_u4 v = *reinterpret_cast<const we_u4*>(p);
        return ok ? v : zero;
    } else {
        return *reinterpret_cast<const we_u4*>((const we_h*)g.a + (long)m * g.lda + k0 + seg * 8);
    }
}

template <int EPI>
__device__ __forceinline__ void we_finish(const WencGemmArgs& g, int m, int n, float acc, float bias) {
    const float x = acc + bias;
    const long at = (long)m * g.N + n;
    if (EPI == WE_CONV1 || EPI == WE_FC1) g.out[at] = (we_h)we_gelu(x);
    else if (EPI == WE_CONV2) g.resid[at] = we_gelu(x) + g.pos[(long)(m % g.T) * g.N + n];
    else if (EPI == WE_RESID) g.resid[at] = g.resid[at] + x;
    else {
        const int which = n / g.d, c = n - which * g.d, b = m / g.T, t = m - b * g.T;
        const long to = (((long)b * g.H + (c >> 6)) * g.T + t) * WENC_HEAD_DIM + (c & 63);
        if (which == 0) g.q[to] = (we_h)(x * 0.125f);
        else if (which == 1) g.k[to] = (we_h)acc;
        else g.v[to] = (we_h)x;
    }
}

template <int EPI, int MI>
__global__ __launch_bounds__(256, 2) void k_wenc_gemm(const WencGemmArgs g) {
    constexpr int BM = 64 * MI, NA = 2 * MI, LROWS = BM + 128;
    extern __shared__ __align__(16) unsigned char we_smem[];
    we_h* lds = reinterpret_cast<we_h*>(we_smem);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * 128;
    // this thread's 16-byte pieces of each operand slice: rows (tid >> 3) + 32 i, segment tid & 7
    const int seg = tid & 7, row0 = tid >> 3;
    const int per_clip = EPI == WE_CONV1 ? 2 * g.T : g.T;
    int am[NA], ab[NA], at[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        am[i] = min(m0 + row0 + 32 * i, g.M - 1);
        ab[i] = am[i] / per_clip;
        at[i] = am[i] - ab[i] * per_clip;
    }
    const we_h* pb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) pb[i] = g.w + (long)min(n0 + row0 + 32 * i, g.N - 1) * g.K + seg * 8;
    we_u4 ra[NA], rb[4];
#define WE_GLOAD(s_)                                                                                 \
    _Pragma("unroll") for (int i = 0; i < NA; ++i) ra[i] = we_a_piece<EPI>(g, ab[i], at[i], am[i], (s_) * 64, seg); \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) rb[i] = *reinterpret_cast<const we_u4*>(pb[i] + (s_) * 64);
    // rows row0 + 32 i share (row >> 1) & 7, so one swizzled segment serves all pieces
    we_h* const wbase = lds + row0 * WE_LD + (seg ^ ((row0 >> 1) & 7)) * 8;
#define WE_LWRITE(buf)                                                                               \
    _Pragma("unroll") for (int i = 0; i < NA; ++i)                                                   \
        *reinterpret_cast<we_u4*>(wbase + (buf) * (LROWS * WE_LD) + (32 * i) * WE_LD) = ra[i];       \
    _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                    \
        *reinterpret_cast<we_u4*>(wbase + (buf) * (LROWS * WE_LD) + (BM + 32 * i) * WE_LD) = rb[i];
    const int sw = (r >> 1) & 7;

    we_f16 acc[MI][2];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[mi][ni][i] = 0.f;

    const int ns = g.K / 64;
    WE_GLOAD(0)
    WE_LWRITE(0)
    __syncthreads();
    for (int s = 0; s < ns; ++s) {
        const int buf = s & 1;
        if (s + 1 < ns) { WE_GLOAD(s + 1) }                      // in flight while slice s feeds the matrix cores
        const we_h* A = lds + buf * (LROWS * WE_LD) + (wm * 32 * MI + r) * WE_LD;
        const we_h* B = lds + buf * (LROWS * WE_LD) + (BM + wn * 64 + r) * WE_LD;
#pragma unroll
        for (int q = 0; q < 4; ++q) {                            // lane half h, step q <- k = 32 h + 8 q .. + 8 of the slice
            const int so = ((4 * h + q) ^ sw) * 8;
            const we_u4 b0 = *reinterpret_cast<const we_u4*>(B + so);
            const we_u4 b1 = *reinterpret_cast<const we_u4*>(B + 32 * WE_LD + so);
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) {
                const we_u4 a = *reinterpret_cast<const we_u4*>(A + mi * 32 * WE_LD + so);
                acc[mi][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(we_as_h8(a), we_as_h8(b0), acc[mi][0], 0, 0, 0);
                acc[mi][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(we_as_h8(a), we_as_h8(b1), acc[mi][1], 0, 0, 0);
            }
        }
        if (s + 1 < ns) { WE_LWRITE(buf ^ 1) }                   // (its last readers passed the barrier that ended slice s - 1)
        __syncthreads();
    }
#undef WE_GLOAD
#undef WE_LWRITE
    // epilogue: acc register i of lane (r, h) is row 8 (i / 4) + 4 h + (i % 4), column r of its 32 x 32 tile
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
        const int n = n0 + wn * 64 + ni * 32 + r;
        if (n >= g.N) continue;
        const float bias = g.bias[n];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int m = m0 + wm * 32 * MI + mi * 32 + 8 * (i >> 2) + 4 * h + (i & 3);
                if (m < g.M) we_finish<EPI>(g, m, n, acc[mi][ni][i], bias);
            }
    }
}

// ---- LayerNorm: one wave per row, the row in registers ----
__device__ __forceinline__ unsigned short we_bf16(float x) {                           // round to nearest even; NaN stays NaN
    unsigned u = __builtin_bit_cast(unsigned, x);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40u);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}

__device__ __forceinline__ float we_wave_sum(float v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = v + __shfl_xor(v, d);
    return v;
}

// fmt: 0 fp32, 1 fp16, 2 bf16
__global__ __launch_bounds__(256) void k_wenc_ln(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                 void* __restrict__ out, int M, int d, float eps, int fmt) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    const float* xr = x + (long)row * d;
    float v[WENC_MAX_HEADS];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < WENC_MAX_HEADS; ++i) {
        const int c = lane + 64 * i;
        v[i] = c < d ? xr[c] : 0.f;
        s = s + v[i];
    }
    const float mean = we_wave_sum(s) / (float)d;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < WENC_MAX_HEADS; ++i) {
        const float t = lane + 64 * i < d ? v[i] - mean : 0.f;
        ss = fmaf(t, t, ss);
    }
    const float rstd = 1.0f / sqrtf(we_wave_sum(ss) / (float)d + eps);
#pragma unroll
    for (int i = 0; i < WENC_MAX_HEADS; ++i) {
        const int c = lane + 64 * i;
        if (c >= d) continue;
        const float y = fmaf((v[i] - mean) * rstd, w[c], b[c]);
        const long at = (long)row * d + c;
        if (fmt == 0) ((float*)out)[at] = y;
        else if (fmt == 1) ((we_h*)out)[at] = (we_h)y;
        else ((unsigned short*)out)[at] = we_bf16(y);
    }
}

// ---- non-causal flash attention, head dim 64 ----
#define WA_KLD 64            // K tile row = 64 d (128 B), 16-byte segments XOR-swizzled like the GEMM's
#define WA_VLD 96            // V tile row stride 192 B: the 4 rows of a transposed read land on 4 distinct bank quarters
#define WA_LDS_BYTES (2 * 64 * WA_KLD * 2 + 2 * 64 * WA_VLD * 2)      // K + V double buffers: 40 KB

__global__ __launch_bounds__(256) void k_wenc_attn(const we_h* __restrict__ q, const we_h* __restrict__ k, const we_h* __restrict__ v,
                                                  we_h* __restrict__ out, int T, int H, int qtiles) {
    __shared__ __align__(16) char wa_lds[WA_LDS_BYTES];
    we_h (*Ks)[64 * WA_KLD] = reinterpret_cast<we_h (*)[64 * WA_KLD]>(wa_lds);
    we_h (*Vs)[64 * WA_VLD] = reinterpret_cast<we_h (*)[64 * WA_VLD]>(wa_lds + 2 * 64 * WA_KLD * 2);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int qt = blockIdx.x % qtiles, bh = blockIdx.x / qtiles;            // bh = clip * H + head
    const int q0 = qt * WENC_QTILE + wave * 32;                              // this wave's first query
    const int mq = min(q0 + r, T - 1);                                       // this lane's query (padding repeats the last)
    const long base = (long)bh * T * WENC_HEAD_DIM;
    const we_h* kb = k + base;
    const we_h* vb = v + base;
    const int npairs = (T + 63) / 64;                                        // pairs of 32-key tiles

    // staging: thread t moves segment (t & 7) of key rows (t >> 3) and (t >> 3) + 32 of a pair; they share (row >> 1) & 7
    const int skey = tid >> 3, sseg = tid & 7;
    we_u4 kreg[2], vreg[2];
    const we_u4 zero4 = {0u, 0u, 0u, 0u};
#define WA_GLOAD(t)                                                                                     \
    _Pragma("unroll") for (int u = 0; u < 2; ++u) {                                                     \
        const int j = (t) * 64 + 32 * u + skey;                                                         \
        const long off = (long)min(j, T - 1) * WENC_HEAD_DIM + sseg * 8;                                \
        kreg[u] = *reinterpret_cast<const we_u4*>(kb + off);                                            \
        vreg[u] = *reinterpret_cast<const we_u4*>(vb + off);                                            \
        if (j >= T) { kreg[u] = zero4; vreg[u] = zero4; }      /* a missing key: zeros, and the score is masked below */ \
    }
#define WA_LWRITE(buf)                                                                                  \
    _Pragma("unroll") for (int u = 0; u < 2; ++u) {                                                     \
        *reinterpret_cast<we_u4*>(&Ks[buf][(32 * u + skey) * WA_KLD + ((sseg ^ ((skey >> 1) & 7)) * 8)]) = kreg[u]; \
        *reinterpret_cast<we_u4*>(&Vs[buf][(32 * u + skey) * WA_VLD + sseg * 8]) = vreg[u];             \
    }
    // Q fragments (B operand): lane (r = query, h) holds q[32 h + 8 s .. + 8] of its row for k-step s = 0 .. 3
    we_u4 qf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = *reinterpret_cast<const we_u4*>(q + base + (long)mq * WENC_HEAD_DIM + 32 * h + 8 * s);
    we_f16 o0, o1;                                                           // O^T rows d = 0 .. 31 / 32 .. 63, column = query
#pragma unroll
    for (int i = 0; i < 16; ++i) { o0[i] = 0.f; o1[i] = 0.f; }
    float mrun = -INFINITY, lrun = 0.f;

    WA_GLOAD(0)
    WA_LWRITE(0)
    __syncthreads();
    for (int it = 0; it < npairs; ++it) {
        WA_GLOAD(it + 1)                                                     // in flight while this pair is computed (past T: zeros)
#pragma unroll
        for (int u = 0; u < 2; ++u) {                                        // (a tile past T is fully masked: an exact no-op)
            const int t = 2 * it + u;
            const we_h* Kt = Ks[it & 1] + u * 32 * WA_KLD;
            const we_h* Vt = Vs[it & 1] + u * 32 * WA_VLD;
            // ---- S^T = K . Q^T ----
            we_f16 sacc;
#pragma unroll
            for (int i = 0; i < 16; ++i) sacc[i] = 0.f;
            const int sw = (r >> 1) & 7;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const we_u4 kf = *reinterpret_cast<const we_u4*>(Kt + r * WA_KLD + (((4 * h + s) ^ sw) * 8));
                sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(we_as_h8(kf), we_as_h8(qf[s]), sacc, 0, 0, 0);
            }
            // ---- online softmax over this lane pair's 32 keys (q carries the scale) ----
            float p[16];
            float tmax = -INFINITY;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int j = t * 32 + 8 * (i >> 2) + 4 * h + (i & 3);       // key of accumulator register i
                p[i] = j < T ? sacc[i] : -INFINITY;
                tmax = fmaxf(tmax, p[i]);
            }
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
            const float mnew = fmaxf(mrun, tmax);
            const bool none = mnew == -INFINITY;                             // (never: the first tile holds key 0)
            const float corr = none ? 1.0f : __expf(mrun - mnew);            // 0 on the first tile
            float psum = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) { p[i] = none ? 0.f : __expf(p[i] - mnew); psum = psum + p[i]; }
            psum = psum + __shfl_xor(psum, 32);
            lrun = fmaf(lrun, corr, psum);
            mrun = mnew;
#pragma unroll
            for (int i = 0; i < 16; ++i) { o0[i] *= corr; o1[i] *= corr; }
            // ---- O^T += V^T . P^T ----
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                we_u4 pf;                                                    // P^T fragment: registers 8 s .. 8 s + 7 as fp16
                pf[0] = we_pack(p[8 * s + 0], p[8 * s + 1]); pf[1] = we_pack(p[8 * s + 2], p[8 * s + 3]);
                pf[2] = we_pack(p[8 * s + 4], p[8 * s + 5]); pf[3] = we_pack(p[8 * s + 6], p[8 * s + 7]);
                // V^T fragment of lane (r = d, h): element j <- key 16 s + 8 (j >> 2) + 4 h + (j & 3): two transposed reads of
                // 4 keys x 16 d per 16-lane group; lane 4 q + p of a group addresses key row q, columns 4 p .. 4 p + 3
                const int grp_d = 16 * ((lane >> 4) & 1), qq = (lane & 15) >> 2, pp = lane & 3;
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    const we_h* vbase = Vt + (16 * s + 4 * h + qq) * WA_VLD + 32 * dt + grp_d + 4 * pp;
                    const we_s4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((we_s4 __attribute__((address_space(3)))*)(vbase));
                    const we_s4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((we_s4 __attribute__((address_space(3)))*)(vbase + 8 * WA_VLD));
                    we_u4 vf;
                    const we_u2 l2 = __builtin_bit_cast(we_u2, lo), h2 = __builtin_bit_cast(we_u2, hi);
                    vf[0] = l2[0]; vf[1] = l2[1]; vf[2] = h2[0]; vf[3] = h2[1];
                    if (dt == 0) o0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(we_as_h8(vf), we_as_h8(pf), o0, 0, 0, 0);
                    else o1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(we_as_h8(vf), we_as_h8(pf), o1, 0, 0, 0);
                }
            }
        }
        WA_LWRITE((it + 1) & 1)
        __syncthreads();
    }
#undef WA_GLOAD
#undef WA_LWRITE
    // out[clip][query][head 64 + d] = O^T / l: registers 4 g .. 4 g + 3 are 4 consecutive d -> one 8-byte store; padding queries: none
    if (q0 + r < T) {
        const float inv = 1.0f / lrun;
        const int clip = bh / H, head = bh - clip * H;
        we_h* dst = out + ((long)clip * T + q0 + r) * ((long)H * WENC_HEAD_DIM) + head * WENC_HEAD_DIM;
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            we_u2 w0, w1;
            w0[0] = we_pack(o0[4 * g4] * inv, o0[4 * g4 + 1] * inv); w0[1] = we_pack(o0[4 * g4 + 2] * inv, o0[4 * g4 + 3] * inv);
            w1[0] = we_pack(o1[4 * g4] * inv, o1[4 * g4 + 1] * inv); w1[1] = we_pack(o1[4 * g4 + 2] * inv, o1[4 * g4 + 3] * inv);
            *reinterpret_cast<we_u2*>(dst + 8 * g4 + 4 * h) = w0;
            *reinterpret_cast<we_u2*>(dst + 32 + 8 * g4 + 4 * h) = w1;
        }
    }
}

// ---- the handle ----
#pragma GCC visibility push(hidden)

struct WencLayerDev {
    const we_h *wqkv, *wo, *w1, *w2;
    const float *bqkv, *bo, *b1, *b2, *ln1w, *ln1b, *ln2w, *ln2b;
};

struct MimiWenc {
    WencDims c = {};
    int max_batch = 0;
    std::string err;
    DevPool dev{hip_backend()};
    we_h* w16 = nullptr;             // every weight matrix, fp16
    float* w32 = nullptr;            // biases, LayerNorm parameters, positions
    const we_h *conv1_w = nullptr, *conv2_w = nullptr;
    const float *conv1_b = nullptr, *conv2_b = nullptr, *pos = nullptr, *lnf_w = nullptr, *lnf_b = nullptr;
    WencLayerDev layer[WENC_MAX_LAYERS] = {};
    we_h *h1 = nullptr, *ln = nullptr, *q = nullptr, *k = nullptr, *v = nullptr, *att = nullptr, *mlp = nullptr;
    float* resid = nullptr;
};

static thread_local std::string g_wenc_err;

// One tensor of the state dict as create walks it: where it comes from, its shape, where it goes.
struct WencTensor {
    std::string name;
    const float* src;
    long rows, cols;                 // a vector: rows = 1
    int kind;                        // 0: fp32 as it is; 1: matrix -> fp16 [rows][cols]; 2: conv weight (out, in, 3) -> fp16 [out][kpad], k = tap in + c
    long in_ch, kpad;                // kind 2
    long off;                        // elements into w32 (kind 0) or w16
};

static void wenc_tensors(const WencDims& c, const MimiWencWeights& w, std::vector<WencTensor>& ts, long* n16, long* n32) {
    long o16 = 0, o32 = 0;
    auto f32 = [&](const std::string& name, const float* p, long n) { ts.push_back({name, p, 1, n, 0, 0, 0, o32}); o32 += (n + 3) / 4 * 4; };
    auto mat = [&](const std::string& name, const float* p, long rows, long cols) { ts.push_back({name, p, rows, cols, 1, 0, 0, o16}); o16 += rows * cols; };
    auto conv = [&](const std::string& name, const float* p, long out, long in) {
        const long kpad = wenc_pad64((int)(3 * in));
        ts.push_back({name, p, out, 3 * in, 2, in, kpad, o16});
        o16 += out * kpad;
    };
    const long d = c.d, f = c.ffn;
    conv("conv1.weight", w.conv1_w, d, c.n_mels); f32("conv1.bias", w.conv1_b, d);
    conv("conv2.weight", w.conv2_w, d, d); f32("conv2.bias", w.conv2_b, d);
    f32("embed_positions.weight", w.embed_positions, (long)c.T * d);
    for (int l = 0; l < c.L; ++l) {
        const MimiWencLayerWeights& y = w.layers[l];
        const std::string p = "layers." + std::to_string(l) + ".";
        f32(p + "self_attn_layer_norm.weight", y.self_attn_layer_norm_w, d); f32(p + "self_attn_layer_norm.bias", y.self_attn_layer_norm_b, d);
        mat(p + "self_attn.q_proj.weight", y.q_w, d, d);                   // q | k | v back to back: one [3 d][d] matrix
        mat(p + "self_attn.k_proj.weight", y.k_w, d, d);
        mat(p + "self_attn.v_proj.weight", y.v_w, d, d);
        f32(p + "self_attn.q_proj.bias", y.q_b, d);                        // and one [3 d] bias, zero for k
        f32(p + "self_attn.k_proj.bias (none)", nullptr, d);
        f32(p + "self_attn.v_proj.bias", y.v_b, d);
        mat(p + "self_attn.out_proj.weight", y.out_w, d, d); f32(p + "self_attn.out_proj.bias", y.out_b, d);
        f32(p + "final_layer_norm.weight", y.final_layer_norm_w, d); f32(p + "final_layer_norm.bias", y.final_layer_norm_b, d);
        mat(p + "fc1.weight", y.fc1_w, f, d); f32(p + "fc1.bias", y.fc1_b, f);
        mat(p + "fc2.weight", y.fc2_w, d, f); f32(p + "fc2.bias", y.fc2_b, d);
    }
    f32("layer_norm.weight", w.layer_norm_w, d); f32("layer_norm.bias", w.layer_norm_b, d);
    *n16 = o16; *n32 = o32;
}
// whether a host tensor holds a value that fp16 cannot hold (matrices), or that is not finite
static bool wenc_values_bad(const WencTensor& t, const float* host) {
    const long n = t.rows * t.cols;
    for (long i = 0; i < n; ++i)
        if (!(fabsf(host[i]) <= (t.kind ? WENC_F16_MAX : 3.0e38f))) return true;
    return false;
}

static void wenc_convert(const WencTensor& t, const float* host, std::vector<we_h>& out) {
    if (t.kind == 1) {
        out.resize((size_t)(t.rows * t.cols));
        for (long i = 0; i < t.rows * t.cols; ++i) out[i] = (we_h)host[i];
        return;
    }
    out.assign((size_t)(t.rows * t.kpad), (we_h)0.0f);
    for (long n = 0; n < t.rows; ++n)
        for (long c = 0; c < t.in_ch; ++c)
            for (int tap = 0; tap < 3; ++tap) out[n * t.kpad + tap * t.in_ch + c] = (we_h)host[(n * t.in_ch + c) * 3 + tap];
}

static hipError_t wenc_take(MimiWenc* p, char** out, size_t bytes) { return (hipError_t)p->dev.get(out, bytes); }

#pragma GCC visibility pop

extern "C" int mimi_wenc_create(const MimiWencConfig* cfg, const MimiWencWeights* w, int max_batch, mimi_wenc* out) {
    std::string& err = g_wenc_err;
    if (!out) { err = "null pointer"; return -1; }
    *out = nullptr;
    if (!cfg || !w) { err = "null pointer"; return -1; }
    const WencDims c = {cfg->n_mels, cfg->d_model, cfg->n_layers, cfg->n_heads, cfg->ffn_dim, cfg->n_ctx, cfg->ln_eps};
    if (const char* bad = wenc_dims_bad(c, max_batch)) { err = bad; return -1; }
    std::vector<WencTensor> ts;
    long n16 = 0, n32 = 0;
    wenc_tensors(c, *w, ts, &n16, &n32);
    for (const WencTensor& t : ts)
        if (!t.src && t.name.find("(none)") == std::string::npos) { err = "null pointer: " + t.name; return -1; }
    if (w->host)                                                             // host weights are judged before the device is touched
        for (const WencTensor& t : ts)
            if (t.src && wenc_values_bad(t, t.src)) {
                err = t.name + (t.kind ? ": a value does not fit fp16" : ": a value is not finite");
                return -1;
            }

    MimiWenc* p = new MimiWenc();
    p->c = c;
    p->max_batch = max_batch;
    const size_t rows = (size_t)max_batch * c.T, rd = rows * c.d;
    char *m16 = nullptr, *m32 = nullptr, *h1 = nullptr, *ln = nullptr, *q = nullptr, *k = nullptr, *v = nullptr, *att = nullptr, *mlp = nullptr, *res = nullptr;
    hipError_t e = wenc_take(p, &m16, sizeof(we_h) * (size_t)n16);
    if (e == hipSuccess) e = wenc_take(p, &m32, sizeof(float) * (size_t)n32);
    if (e == hipSuccess) e = wenc_take(p, &h1, sizeof(we_h) * 2 * rd);
    if (e == hipSuccess) e = wenc_take(p, &ln, sizeof(we_h) * rd);
    if (e == hipSuccess) e = wenc_take(p, &q, sizeof(we_h) * rd);
    if (e == hipSuccess) e = wenc_take(p, &k, sizeof(we_h) * rd);
    if (e == hipSuccess) e = wenc_take(p, &v, sizeof(we_h) * rd);
    if (e == hipSuccess) e = wenc_take(p, &att, sizeof(we_h) * rd);
    if (e == hipSuccess) e = wenc_take(p, &mlp, sizeof(we_h) * rows * c.ffn);
    if (e == hipSuccess) e = wenc_take(p, &res, sizeof(float) * rd);
    p->w16 = (we_h*)m16; p->w32 = (float*)m32;
    p->h1 = (we_h*)h1; p->ln = (we_h*)ln; p->q = (we_h*)q; p->k = (we_h*)k; p->v = (we_h*)v; p->att = (we_h*)att; p->mlp = (we_h*)mlp;
    p->resid = (float*)res;
    std::string refused;
    if (e == hipSuccess) {
        std::vector<float> host;
        std::vector<we_h> half;
        for (const WencTensor& t : ts) {
            const long n = t.rows * t.cols;
            const float* src = t.src;
            if (!src) { host.assign((size_t)n, 0.0f); src = host.data(); }   // k has no bias: zeros
            else if (!w->host) {
                host.resize((size_t)n);
                if ((e = hipMemcpy(host.data(), t.src, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost)) != hipSuccess) break;
                src = host.data();
                if (wenc_values_bad(t, src)) { refused = t.name + (t.kind ? ": a value does not fit fp16" : ": a value is not finite"); break; }
            }
            if (t.kind == 0) e = hipMemcpy(p->w32 + t.off, src, sizeof(float) * (size_t)n, hipMemcpyHostToDevice);
            else {
                wenc_convert(t, src, half);
                e = hipMemcpy(p->w16 + t.off, half.data(), sizeof(we_h) * half.size(), hipMemcpyHostToDevice);
            }
            if (e != hipSuccess) break;
        }
    }
    if (e != hipSuccess || !refused.empty()) {
        err = refused.empty() ? std::string("mimi_wenc_create: ") + hipGetErrorString(e) : refused;
        delete p;                                                            // frees every allocation made so far
        return refused.empty() ? -2 : -1;
    }
    // the tensors' places, in wenc_tensors' order
    size_t i = 0;
    auto h16 = [&]() { return (const we_h*)(p->w16 + ts[i++].off); };
    auto f32 = [&]() { return (const float*)(p->w32 + ts[i++].off); };
    p->conv1_w = h16(); p->conv1_b = f32(); p->conv2_w = h16(); p->conv2_b = f32(); p->pos = f32();
    for (int l = 0; l < c.L; ++l) {
        WencLayerDev& y = p->layer[l];
        y.ln1w = f32(); y.ln1b = f32();
        y.wqkv = h16(); i += 2;
        y.bqkv = f32(); i += 2;
        y.wo = h16(); y.bo = f32();
        y.ln2w = f32(); y.ln2b = f32();
        y.w1 = h16(); y.b1 = f32(); y.w2 = h16(); y.b2 = f32();
    }
    p->lnf_w = f32(); p->lnf_b = f32();
    *out = p;
    return 0;
}

extern "C" void mimi_wenc_destroy(mimi_wenc h) { delete h; }

extern "C" const char* mimi_wenc_last_error(mimi_wenc h) { return h ? h->err.c_str() : g_wenc_err.c_str(); }

extern "C" int mimi_wenc_describe(mimi_wenc h, int batch, char* text, int cap) {
    if (!h) return -1;
    if (batch < 1 || batch > h->max_batch || cap < 0 || (cap > 0 && !text)) { h->err = "describe: batch outside 1 .. max_batch, or no room"; return -1; }
    const std::string s = wenc_describe(h->c, batch);
    if (cap > 0) { const size_t n = s.size() < (size_t)cap - 1 ? s.size() : (size_t)cap - 1; memcpy(text, s.data(), n); text[n] = 0; }
    return (int)s.size() + 1;                                                // the room the whole text takes
}

#pragma GCC visibility push(hidden)
template <int EPI> static hipError_t wenc_gemm(const WencGemmArgs& g, hipStream_t s) {
    const int tr = wenc_tile_rows(g.M, g.N);
    const dim3 grid((unsigned)((g.N + 127) / 128), (unsigned)((g.M + tr - 1) / tr));
    if (tr == 128) k_wenc_gemm<EPI, 2><<<grid, dim3(256), WE_SMEM(2), s>>>(g);
    else k_wenc_gemm<EPI, 1><<<grid, dim3(256), WE_SMEM(1), s>>>(g);
    return hipGetLastError();
}
#pragma GCC visibility pop

#define WENC_HIP(call)                                                                               \
    do {                                                                                             \
        hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess) { h->err = std::string(#call) + ": " + hipGetErrorString(e_); return -2; } \
    } while (0)

extern "C" int mimi_wenc_encode(mimi_wenc h, const float* features, int batch, void* out, int out_fmt, void* stream) {
    if (!h) return -1;
    if (!features || !out) { h->err = "null pointer"; return -1; }
    if (batch < 1 || batch > h->max_batch) { h->err = "batch outside 1 .. max_batch"; return -1; }
    if (out_fmt < 0 || out_fmt > 2) { h->err = "unknown output format"; return -1; }
    if (((uintptr_t)features & 3) || ((uintptr_t)out & 3)) { h->err = "misaligned buffer"; return -1; }
    (void)hipGetLastError();
    hipStream_t s = (hipStream_t)stream;
    const WencDims& c = h->c;
    const int M = batch * c.T, d = c.d;
    WencGemmArgs g = {};
    g.T = c.T; g.d = d; g.H = c.H; g.n_mels = c.n_mels;
    g.resid = h->resid; g.pos = h->pos; g.q = h->q; g.k = h->k; g.v = h->v;
    // conv1: (n_mels, 2 T) fp32 -> h1 (2 T, d) fp16
    g.a = features; g.w = h->conv1_w; g.bias = h->conv1_b; g.out = h->h1; g.M = 2 * M; g.N = d; g.K = wenc_pad64(3 * c.n_mels); g.lda = 0;
    WENC_HIP(wenc_gemm<WE_CONV1>(g, s));
    g.a = h->h1; g.w = h->conv2_w; g.bias = h->conv2_b; g.M = M; g.K = 3 * d;
    WENC_HIP(wenc_gemm<WE_CONV2>(g, s));
    const dim3 ln_grid((unsigned)((M + 3) / 4));
    const int qtiles = (c.T + WENC_QTILE - 1) / WENC_QTILE;
    for (int l = 0; l < c.L; ++l) {
        const WencLayerDev& y = h->layer[l];
        k_wenc_ln<<<ln_grid, dim3(256), 0, s>>>(h->resid, y.ln1w, y.ln1b, h->ln, M, d, c.eps, 1);
        WENC_HIP(hipGetLastError());
        g.a = h->ln; g.lda = d; g.w = y.wqkv; g.bias = y.bqkv; g.M = M; g.N = 3 * d; g.K = d;
        WENC_HIP(wenc_gemm<WE_QKV>(g, s));
        k_wenc_attn<<<dim3((unsigned)(batch * c.H * qtiles)), dim3(256), 0, s>>>(h->q, h->k, h->v, h->att, c.T, c.H, qtiles);
        WENC_HIP(hipGetLastError());
        g.a = h->att; g.lda = d; g.w = y.wo; g.bias = y.bo; g.N = d; g.K = d;
        WENC_HIP(wenc_gemm<WE_RESID>(g, s));
        k_wenc_ln<<<ln_grid, dim3(256), 0, s>>>(h->resid, y.ln2w, y.ln2b, h->ln, M, d, c.eps, 1);
        WENC_HIP(hipGetLastError());
        g.a = h->ln; g.lda = d; g.w = y.w1; g.bias = y.b1; g.out = h->mlp; g.N = c.ffn; g.K = d;
        WENC_HIP(wenc_gemm<WE_FC1>(g, s));
        g.a = h->mlp; g.lda = c.ffn; g.w = y.w2; g.bias = y.b2; g.N = d; g.K = c.ffn;
        WENC_HIP(wenc_gemm<WE_RESID>(g, s));
    }
    k_wenc_ln<<<ln_grid, dim3(256), 0, s>>>(h->resid, h->lnf_w, h->lnf_b, out, M, d, c.eps, out_fmt);
    WENC_HIP(hipGetLastError());
    return 0;
}
