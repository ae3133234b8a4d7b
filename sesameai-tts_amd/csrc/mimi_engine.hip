// Mimi codec decode on gfx950 (fp32): RVQ gather-sum + output projections, depthwise
// upsample, 8-layer causal transformer (window 250, interleaved RoPE, LayerScale) and the
// SEANet conv decoder.  C ABI in include/mimi_hip.h.
//
// Replaces moshi 0.2.2 MimiModel.decode as called at sesameai/generator.py:116,299 and
// tts_service.py:245 (structure: SURVEY.md App. A.3; checked against oracle/mimi_ref.py).
//
// Layout: every activation is token-major [time][channels] fp32, so the channel (reduction)
// axis is contiguous for loads and the output-channel axis is contiguous for stores.  Every
// linear layer, causal Conv1d and ConvTranspose1d is ONE kernel: a multi-tap GEMM
//     out[t*phases + p][co] = bias[co] + sum_tap sum_ci act(x[t + shift_tap][ci]) * w[p][tap][co][ci]
// on the exact-fp32 matrix cores (v_mfma_f32_32x32x2_f32, bit-identical to an fmaf chain), one
// wave per 32(time) x 32(channel) tile, operands straight from L2 in 64-byte contiguous pieces
// (the K order inside a 32-wide chunk is permuted so each lane reads 16 consecutive floats).
// A transposed conv with k = 2*stride is `stride` phase-GEMMs with 2 taps each.  Buffers that
// feed a causal op carry `hist` rows of left context in front of row 0: zero for a stateless
// decode, the previous call's tail for a stateful stream.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../include/mimi_hip.h"
#include "switches.h"
#define ENC_SEGS_FN __host__ __device__ static inline
#include "enc_segs.h"
static_assert(ENC_MAX_CLIPS == MIMI_ENCODE_MAX_CLIPS && ENC_MAX_STAGES == MIMI_MAX_STAGES, "enc_segs.h and mimi_hip.h disagree");
#define POOL_SEGS_FN __host__ __device__ static inline
#include "pool_segs.h"
static_assert(POOL_SEG_MAX_STREAMS == MIMI_POOL_MAX_STREAMS, "pool_segs.h and mimi_hip.h disagree");
#include "enc_stream_segs.h"
static_assert(ENC_STREAM_MAX_STREAMS == MIMI_ENC_POOL_MAX_STREAMS, "enc_stream_segs.h and mimi_hip.h disagree");

typedef float f32x16 __attribute__((ext_vector_type(16)));
static thread_local std::string g_mimi_err;

#define MAX_TAPS 16

// K-split workspace of a handle (mimi_create): partial tiles [MIMI_KSPLIT][cap_rows][cap_cols] fp32 + one ticket per output tile
#define MIMI_KSPLIT 8                   // default number of K slices (MIMI_KSPLIT=n in the environment: 0 = off, 2 / 4 / 8; measured: profiles/r05/mimi_ksplit_ab.txt)
#define MIMI_KSPLIT_MAX 8
#define MIMI_KSPLIT_MIN_ITERS 64        // deep products only: (taps * C_in / 32) iterations, e.g. the K = 2048 linear (64), the 7-tap 512 -> 1024 conv (112)
struct KSplitWs { float* part; int* ticket; long cap_rows; int cap_cols, n_tickets, ksplit; };

// Device table of a ragged encode (mimi_encode_many; written by k_enc_plan, the first kernel of the chain): per clip where its samples
// start, its first frame and its rows at every level (enc_segs.h); behind the clips, frame -> clip for the call's F frames.
struct EncClipTab { long wav_off; int F0; int L[ENC_MAX_LEVELS]; };
struct RagArgs { const EncClipTab* clips; const int* frame_clip; int lvl_in, lvl_out, rate_in, rate_out; };

struct GemmArgs {
    const float* x; long ldx;       // A row for output time t, tap j: x + (t * in_stride + shift0 + j * dshift) * ldx
    int in_stride;                  // 1, or the stride of a down-sampling conv
    int edge, row_lo, row_hi;       // edge 0: rows are always in range (left context stored in front of row 0);
                                    // 1: rows outside [row_lo,row_hi) read as zero; 2: clamped (replicate padding)
    int T_in, C_in, C_out;
    const float* w;                 // [phases][taps][C_out][C_in]
    const float* bias;
    int taps, phases;
    int shift0, dshift;             // tap j reads row t * in_stride + shift0 + j * dshift
    int act_out;                    // 1 = exact GELU
    const float* col_scale;         // optional per-output-channel scale (LayerScale)
    const float* resid; long ldr;   // optional residual, indexed like out
    float* out; long ldo;
    // q|k|v projection of the transformer (round 4: was a k_rope_split launch behind every in_proj): C_out = 3 d; channels
    // [0,d) -> rope_q[t] with RoPE, [d,2d) -> rope_k[rope_offset + t] with RoPE, [2d,3d) -> rope_v[rope_offset + t]; head_dim 64,
    // interleaved pairs (the partner channel sits in the neighbouring lane)
    float *rope_q, *rope_k, *rope_v; const float* rope_freqs; int rope_offset, rope_d;
    // K split over blockIdx.z (round 5; phases == 1 only): block (tile, ks) runs iterations [ks, ks + 1) * iters / ksplit, parks its fp32
    // partial tile in kpart[ks][T_in][C_out] with write-through stores, and the LAST of a tile's ksplit blocks to arrive adds the
    // partials in ks order and runs the epilogue.  ksplit is a function of (taps, C_in) alone: streaming == whole decode, bit for bit.
    int ksplit; float* kpart; int* kticket;
    // Stream pool (the SEG instantiation only; MimiStreamPool below): the T_in rows of the launch are the rows of several streams stacked,
    // seg_T per stream.  Global row g = si * seg_T + tl belongs to the si-th listed stream; its A rows start at segment * seg_x + tl * in_stride,
    // its output (residual) row is segment * seg_o (seg_r) + tl * phases + p, where segment = the stream's id (seg_tab[si]) for a buffer that
    // keeps every stream's history in place (bit 0 / 1 / 2 of seg_by_id: x / out / resid) and si for a dense work buffer.  A tap therefore
    // reaches back into its OWN stream's history rows, never into its neighbour's.  RoPE position and K/V ring slot come from the stream's
    // token offset seg_tab[MIMI_POOL_MAX_STREAMS + si].
    // Ragged pool call (the PRG instantiation, with SEG; mimi_pool_decode_ragged): the streams' rows are stacked frame-aligned and seg_T is the
    // launch's rows per FRAME, R.  Global row g belongs to segment si = frame_seg[g / R] (seg_tab + POOL_TAB_FRAME) at tl = g - R * F0_si; a dense
    // buffer's segment starts at row R * F0_si (times `phases` on the output side) where the uniform call has si * seg_x.  Everything else is SEG.
    int seg_T, seg_x, seg_o, seg_r, seg_by_id, rope_ring;
    const int* seg_tab;
    // Ragged encode (the RAG instantiation only; mimi_encode_many below): the rows of the launch are those of several clips, frame-aligned:
    // at a level with R rows per frame clip c owns rows [R * F0_c, R * F0_c + L_c(level)).  Output row g belongs to the clip of frame
    // g / rate_out; with edge != 0 its A rows start at rate_in * F0_c + (g - rate_out * F0_c) * in_stride and the edge bounds are the CLIP's
    // [rate_in * F0_c, + L_c(lvl_in)): a tap reads neither a neighbour's rows nor the unused tail of its own slot.  (edge 0: a dense product,
    // A row = output row.)  The q|k|v epilogue takes the RoPE position from the token's index inside its clip; the K/V row is the global row.
    RagArgs rag;
    // Encode stream pool (the ENS instantiation, with SEG and PRG; mimi_enc_pool_encode): a product whose taps reach past the rows its segment
    // got in this call.  x keeps every stream in place (seg_by_id bit 0) and the edge bounds are the SEGMENT's: below, row_lo rows relative to
    // the stream's row 0 (-hist: its saved history, or -- edge 2 at token offset 0, the downsample's replicate padding -- row 0 itself); above,
    // the rows the segment has at the input level, seg_tab[ens_L + si] (enc_stream_segs.h).
    int ens_L;
};

__device__ __forceinline__ float elu1(float v) { return v > 0.f ? v : expf(v) - 1.0f; }

// One block = one 32 (time) x 32 (channel) output tile; its G32_NW waves split the (tap, 32-wide k chunk) iteration space
// round-robin and add their partial tiles through LDS in a fixed order.  (One wave per tile walked all taps x C_in/32
// chunks serially: at 20 transformer tokens a K = 2048 linear was 64 dependent load->MFMA round trips on 16 blocks.)
// The split depends only on (taps, C_in), never on T, so streaming decode stays bit-identical to whole decode.
#ifndef G32_NW
#define G32_NW 8
#endif
// ELU = the input activation as a compile-time choice.
// Round 4 (tools/dbg/mimi_chunk_timeline.py, profiles/r04/mimi_chunk10_timeline.txt): at 20 transformer tokens every iteration was
// TWO dependent memory round trips -- the tap's row shift came from an indexed array in the argument block (a vector load the
// operand addresses waited for), then the operands -- and every MFMA sat behind a run-time "ELU?" branch.  Now the shift is
// arithmetic (shift0 + j * dshift: every convolution here is an arithmetic progression of taps) and the iteration index is scalar.
// Measured and NOT kept: four iterations' operands requested at once (slower: these launches are bound by the misses 16..64 CUs
// keep in flight and by ~4.7 us of dependent-launch latency each, not by the depth of one wave's queue); the LayerNorm folded
// into the following product (every block normalising its 32 rows itself: 12.7 us against 4.7 + 8.0 for the two launches -- equal);
// the weights re-tiled into MFMA operand order so that every wave load is one contiguous 1 KB (the K = 2048 linear 24 us against
// 19.5 row-major: with one 32-row tile these launches sit on 16..64 CUs and are bound by the fp32 matrix pipe -- 128 dependent
// 64-cycle v_mfma_f32_32x32x2_f32 per wave, two waves per SIMD = 6.8 us -- plus the ~4.7 us of a dependent launch, not by loads).
template <bool ELU, bool SEG = false, bool RAG = false, bool PRG = false, bool ENS = false>
__global__ __launch_bounds__(64 * G32_NW) void k_gemm32(const GemmArgs a) {
    __shared__ float red[G32_NW][16][64];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int ks = a.ksplit > 1 ? (int)blockIdx.z : 0;
    const int t0 = blockIdx.x * 32, n0 = blockIdx.y * 32, p = a.ksplit > 1 ? 0 : (int)blockIdx.z;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    const bool trow_ok = (t0 + r) < a.T_in;
    const bool nrow_ok = (n0 + r) < a.C_out;
    const int trow = trow_ok ? (t0 + r) : (a.T_in - 1);
    const int nrow = nrow_ok ? (n0 + r) : (a.C_out - 1);
    const int kchunks = a.C_in / 32, iters = a.taps * kchunks;
    int arow0 = trow * a.in_stride + a.shift0;
    int row_lo = a.row_lo, row_hi = a.row_hi;
    if (SEG) {
        if (PRG) {
            const int si = a.seg_tab[POOL_TAB_FRAME + trow / a.seg_T], r0 = a.seg_T * a.seg_tab[POOL_TAB_F0 + si];
            arow0 = ((a.seg_by_id & 1) ? a.seg_tab[si] * a.seg_x : r0) + (trow - r0) * a.in_stride + a.shift0;
            if (ENS) {
                const int base = a.seg_tab[si] * a.seg_x;
                row_lo = base + ((a.edge == 2 && a.seg_tab[ENC_STREAM_TAB_FIRST + si]) ? 0 : a.row_lo);
                row_hi = base + a.seg_tab[a.ens_L + si];
            }
        } else {
            const int si = trow / a.seg_T, tl = trow - si * a.seg_T;
            arow0 = ((a.seg_by_id & 1) ? a.seg_tab[si] : si) * a.seg_x + tl * a.in_stride + a.shift0;
        }
    }
    if (RAG && a.edge != 0) {
        const EncClipTab& c = a.rag.clips[a.rag.frame_clip[trow / a.rag.rate_out]];
        row_lo = a.rag.rate_in * c.F0; row_hi = row_lo + c.L[a.rag.lvl_in];
        arow0 = row_lo + (trow - a.rag.rate_out * c.F0) * a.in_stride + a.shift0;
    }
    const float* const wrow = a.w + ((long)p * a.taps * a.C_out + nrow) * a.C_in + h * 16;
    const int it_lo = a.ksplit > 1 ? ks * (iters / a.ksplit) : 0, it_hi = a.ksplit > 1 ? it_lo + iters / a.ksplit : iters;
    for (int it = it_lo + wave; it < it_hi; it += G32_NW) {
        const int j = it / kchunks, kc = (it - j * kchunks) * 32;
        int arow = arow0 + j * a.dshift;
        bool use = trow_ok;
        if (a.edge == 1) { use = trow_ok && arow >= row_lo && arow < row_hi; arow = min(max(arow, row_lo), row_hi - 1); }
        else if (a.edge == 2) arow = min(max(arow, row_lo), row_hi - 1);
        const float* xa = a.x + (long)arow * a.ldx + h * 16 + kc;
        const float* wb = wrow + (long)j * a.C_out * a.C_in + kc;
        float4 av[4], bv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            av[q] = *reinterpret_cast<const float4*>(xa + q * 4);
            bv[q] = *reinterpret_cast<const float4*>(wb + q * 4);
        }
        float af[16], bf[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            af[q * 4 + 0] = av[q].x; af[q * 4 + 1] = av[q].y; af[q * 4 + 2] = av[q].z; af[q * 4 + 3] = av[q].w;
            bf[q * 4 + 0] = bv[q].x; bf[q * 4 + 1] = bv[q].y; bf[q * 4 + 2] = bv[q].z; bf[q * 4 + 3] = bv[q].w;
        }
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            float va = af[s];
            if (ELU) va = elu1(va);
            va = use ? va : 0.f;
            const float vb = nrow_ok ? bf[s] : 0.f;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(va, vb, acc, 0, 0, 0);
        }
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) red[wave][i][lane] = acc[i];
    __syncthreads();
    // C/D map of the 32x32 tile: col = lane & 31 (channel), row = (reg&3) + 8*(reg>>2) + 4*(lane>>5) (time);
    // wave g finishes registers 4g .. 4g+3
    const int ch = n0 + r;
    float part4[4] = {0.f, 0.f, 0.f, 0.f};
    if (a.ksplit > 1) {
        // park this K slice's partial tile (waves 0..3: registers 4w..4w+3, as in the epilogue), then take a ticket: the tile's last
        // block reduces.  Write-through (sc1) stores + vmcnt(0) before the ticket, sc1 loads after it: the guide's counter hand-off.
        if (wave < 4 && ch < a.C_out) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int reg = wave * 4 + i;
                const int t = t0 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
                float sum = 0.f;
#pragma unroll
                for (int w = 0; w < G32_NW; ++w) sum += red[w][reg][lane];      // fixed order
                if (t < a.T_in) {
                    float* dst = a.kpart + ((long)ks * a.T_in + t) * a.C_out + ch;
                    asm volatile("global_store_dword %0, %1, off sc1" ::"v"(dst), "v"(sum) : "memory");
                }
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        __shared__ int s_last;
        if (threadIdx.x == 0) {
            int* tk = a.kticket + blockIdx.y * gridDim.x + blockIdx.x;
            const int got = __hip_atomic_fetch_add(tk, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_last = got == a.ksplit - 1;
            if (s_last) __hip_atomic_store(tk, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // ready for the next launch
        }
        __syncthreads();
        if (!s_last) return;
        if (wave < 4 && ch < a.C_out) {
            float pv[4][MIMI_KSPLIT_MAX];                                            // every load in flight, ONE wait
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int reg = wave * 4 + i;
                const int t = min(t0 + (reg & 3) + 8 * (reg >> 2) + 4 * h, a.T_in - 1);
#pragma unroll
                for (int q = 0; q < MIMI_KSPLIT_MAX; ++q) {
                    pv[i][q] = 0.f;
                    if (q < a.ksplit) {
                        const float* src = a.kpart + ((long)q * a.T_in + t) * a.C_out + ch;
                        asm volatile("global_load_dword %0, %1, off sc1" : "=v"(pv[i][q]) : "v"(src) : "memory");
                    }
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float acc4 = 0.f;
#pragma unroll
                for (int q = 0; q < MIMI_KSPLIT_MAX; ++q) { asm volatile("" : "+v"(pv[i][q])); if (q < a.ksplit) acc4 += pv[i][q]; }     // slice order: deterministic whoever arrived last
                part4[i] = acc4;
            }
        }
    }
    if (ch >= a.C_out || wave >= 4) return;
    const float bias = a.bias ? a.bias[ch] : 0.f;
    const float cs = a.col_scale ? a.col_scale[ch] : 1.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int reg = wave * 4 + i;
        const int t = t0 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
        if (t >= a.T_in) continue;
        float sum = 0.f;
        if (a.ksplit > 1) sum = part4[i];
        else {
#pragma unroll
            for (int w = 0; w < G32_NW; ++w) sum += red[w][reg][lane];          // fixed order
        }
        long orow = (long)t * a.phases + p, rrow = orow;
        int pos = a.rope_offset + t;                                    // token position (RoPE angle)
        long kvrow = pos;                                               // its row in the K / V cache
        if (SEG && !PRG) {
            const int si = t / a.seg_T, tl = t - si * a.seg_T, sid = a.seg_tab[si];
            orow = (long)((a.seg_by_id & 2) ? sid : si) * a.seg_o + (long)tl * a.phases + p;
            rrow = (long)((a.seg_by_id & 4) ? sid : si) * a.seg_r + (long)tl * a.phases + p;
            if (a.rope_q) { pos = a.seg_tab[MIMI_POOL_MAX_STREAMS + si] + tl; kvrow = (long)sid * a.rope_ring + pos % a.rope_ring; }
        }
        if (SEG && PRG) {
            const int si = a.seg_tab[POOL_TAB_FRAME + t / a.seg_T], r0 = a.seg_T * a.seg_tab[POOL_TAB_F0 + si], tl = t - r0, sid = a.seg_tab[si];
            const long dense0 = (long)r0 * a.phases;                    // the segment's first row of a dense output at this launch's rate
            orow = ((a.seg_by_id & 2) ? (long)sid * a.seg_o : dense0) + (long)tl * a.phases + p;
            rrow = ((a.seg_by_id & 4) ? (long)sid * a.seg_r : dense0) + (long)tl * a.phases + p;
            if (a.rope_q) { pos = a.seg_tab[POOL_TAB_OFF + si] + tl; kvrow = (long)sid * a.rope_ring + pos % a.rope_ring; }
        }
        if (RAG && a.rope_q) pos = t - a.rag.rate_out * a.rag.clips[a.rag.frame_clip[t / a.rag.rate_out]].F0;       // (kvrow stays t)
        float v = sum + bias;
        if (a.rope_q) {                                                 // (whole 32-channel tiles: every lane of the half-wave is here)
            const float partner = __shfl_xor(v, 1, 64);
            const int sec = ch / a.rope_d, cc = ch - sec * a.rope_d;
            if (sec == 2) { a.rope_v[kvrow * a.rope_d + cc] = v; continue; }
            const float ang = (float)pos * a.rope_freqs[(cc & 63) >> 1];
            const float c = cosf(ang), s = sinf(ang);
            const float o = (cc & 1) ? partner * s + v * c : v * c - partner * s;
            if (sec == 0) a.rope_q[(long)t * a.rope_d + cc] = o;
            else a.rope_k[kvrow * a.rope_d + cc] = o;
            continue;
        }
        if (a.act_out == 1) v = 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));
        if (a.col_scale) v = cs * v;
        if (a.resid) v = a.resid[rrow * a.ldr + ch] + v;
        a.out[orow * a.ldo + ch] = v;
    }
}

// RVQ decode: q_first = emb_0[c0]; q_rest = sum_{k>=1} emb_k[c_k]; out = Wf q_first + Wr q_rest
// (one frame: `codes` points at the frame's codebook 0, `out` at the frame's row; shared by k_rvq and the stream pool's k_pool_rvq)
__device__ __forceinline__ void rvq_frame(float* q, const int* codes, long stride_k, int ncb, int nsem, int cbsize, int cbdim, int hidden,
                                          const float* books, const float* pf, const float* pr, float* out) {
    int* cidx = reinterpret_cast<int*>(q + 2 * cbdim);
    for (int k = threadIdx.x; k < ncb; k += blockDim.x)                  // the frame's codes once, not once per thread
        cidx[k] = min(max(codes[k * stride_k], 0), cbsize - 1);
    __syncthreads();
    for (int d = threadIdx.x; d < cbdim; d += blockDim.x) {
        float s1 = 0.f, s2 = 0.f;
#pragma unroll 8
        for (int k = 0; k < ncb; ++k) {                                   // independent row loads, summed in codebook order
            const float v = books[((long)k * cbsize + cidx[k]) * cbdim + d];
            if (k < nsem) s1 += v; else s2 += v;
        }
        q[d] = s1; q[cbdim + d] = s2;
    }
    __syncthreads();
    // blockIdx.y = group of 64 output channels (round 4: with one block per frame a 10-frame chunk was 10 blocks pulling 1 MB of
    // projection weights each, 30 us); the lookup-sum above is repeated per group (32 KB of codebook rows from L2)
    const int c_lo = blockIdx.y * 64, c_hi = min(c_lo + 64, hidden);
    for (int c = c_lo + threadIdx.x; c < c_hi; c += blockDim.x) {
        float a1 = 0.f, a2 = 0.f;
#pragma unroll 8
        for (int d = 0; d < cbdim; ++d) {                                 // (unroll 32 -- 64 loads in flight -- was measured: 4x SLOWER)
            a1 = fmaf(pf[(long)d * hidden + c], q[d], a1);
            a2 = fmaf(pr[(long)d * hidden + c], q[cbdim + d], a2);
        }
        out[c] = a1 + a2;
    }
}

__global__ __launch_bounds__(256) void k_rvq(const int* codes, long stride_k, long stride_t, int T, int ncb, int nsem,
                                             int cbsize, int cbdim, int hidden, const float* books, const float* pf,
                                             const float* pr, float* out, long ldo) {
    extern __shared__ float q[];                 // [2][cbdim] sums, then [ncb] clamped codes
    const int t = blockIdx.x;
    rvq_frame(q, codes + t * stride_t, stride_k, ncb, nsem, cbsize, cbdim, hidden, books, pf, pr, out + (long)t * ldo);
}

// depthwise ConvTranspose1d k4 s2, causal: out[2t+p][c] = x[t][c] w[p][0][c] + x[t-1][c] w[p][1][c]
// (+ the K-split tiles' arrival tickets back to zero: they reset themselves, but only in a launch that completes -- the first kernel of every
//  pass puts them at zero so that an aborted launch cannot leave a tile one arrival ahead; no launch of its own)
__device__ __forceinline__ float upsample_tap2(const float* xr, long ldx, const float* w, int p, int C, int c) {
    return xr[c] * w[(p * 2 + 0) * C + c] + xr[c - ldx] * w[(p * 2 + 1) * C + c];
}

__global__ void k_upsample(const float* x, long ldx, int T, int C, const float* w, float* out, long ldo, int* tickets, int n_tickets) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (tickets != nullptr)
        for (long j = i; j < n_tickets; j += (long)gridDim.x * blockDim.x) tickets[j] = 0;
    if (i >= (long)T * 2 * C) return;
    const int c = (int)(i % C);
    const long n = i / C;
    const long t = n >> 1;
    const int p = (int)(n & 1);
    out[n * ldo + c] = upsample_tap2(x + t * ldx, ldx, w, p, C, c);
}

// One wave per row; the row is read ONCE into registers (up to 16 values per lane, d <= 1024) with w and b loads in
// flight beside it -- the three-pass version paid three dependent global round trips per call (6.7 us x 16 per decode).
__global__ __launch_bounds__(64) void k_layernorm(const float* x, int d, const float* w, const float* b, float eps, float* out) {
    const long row = blockIdx.x;
    const float* xr = x + row * d;
    const int lane = threadIdx.x;
    float v[16], wv[16], bv[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int i = lane + 64 * j;
        const bool in = i < d;
        v[j] = in ? xr[i] : 0.f; wv[j] = in ? w[i] : 0.f; bv[j] = in ? b[i] : 0.f;
    }
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) s += v[j];                     // same per-lane order as before: i = lane, lane + 64, ...
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const float mean = s / d;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) { const float dlt = v[j] - mean; if (lane + 64 * j < d) q += dlt * dlt; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
    const float rstd = 1.0f / sqrtf(q / d + eps);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int i = lane + 64 * j;
        if (i < d) out[row * d + i] = (v[j] - mean) * rstd * wv[j] + bv[j];
    }
}

// causal windowed attention, one wave per (query, head); head_dim 64.  qr / outr: the query's and the output's 64 floats of this head;
// pi: the query's token position; kc / vc: the stream's cache at this head.  RING: position p sits in row p % ring (stream pool), and the
// keys are still walked in chronological order from the window start, so the sums are those of the linear cache.
template <bool RING>
__device__ __forceinline__ void attn_row(float* pbuf, const float* qr, const float* kc, const float* vc, int d, int pi, int context, int ring,
                                         float* outr) {
    const int lane = threadIdx.x;
    const int lo = max(0, pi - context + 1);
    const int nk = pi - lo + 1;
    float qv[64];
#pragma unroll
    for (int e = 0; e < 64; e += 4) {
        const float4 v = *reinterpret_cast<const float4*>(qr + e);
        qv[e] = v.x; qv[e + 1] = v.y; qv[e + 2] = v.z; qv[e + 3] = v.w;
    }
    float mx = -INFINITY;
    for (int j = lane; j < nk; j += 64) {
        const float* kr = kc + (long)(RING ? (lo + j) % ring : lo + j) * d;
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < 64; e += 4) {
            const float4 v = *reinterpret_cast<const float4*>(kr + e);
            s = fmaf(qv[e], v.x, s); s = fmaf(qv[e + 1], v.y, s); s = fmaf(qv[e + 2], v.z, s); s = fmaf(qv[e + 3], v.w, s);
        }
        s *= 0.125f;
        pbuf[j] = s;
        mx = fmaxf(mx, s);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    float sum = 0.f;
    for (int j = lane; j < nk; j += 64) { const float pw = expf(pbuf[j] - mx); pbuf[j] = pw; sum += pw; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    __syncthreads();
    float o = 0.f;
    if (RING) {
        int row = lo % ring;
        for (int j = 0; j < nk; ++j) { o = fmaf(pbuf[j], vc[(long)row * d + lane], o); if (++row == ring) row = 0; }
    } else {
        for (int j = 0; j < nk; ++j) o = fmaf(pbuf[j], vc[(long)(lo + j) * d + lane], o);
    }
    outr[lane] = o / sum;
}

__global__ __launch_bounds__(64) void k_mimi_attn(const float* q, const float* kc, const float* vc, int d, int offset,
                                                  int context, float* out) {
    __shared__ float pbuf[1024];
    const int i = blockIdx.x, hh = blockIdx.y;
    attn_row<false>(pbuf, q + (long)i * d + hh * 64, kc + hh * 64, vc + hh * 64, d, offset + i, context, 0, out + (long)i * d + hh * 64);
}

// final Conv1d (taps x C_in -> 1 channel) with ELU on the input; one thread per output sample
// (xt: the input row of the output sample's own time step; the earlier taps sit in the rows before it)
__device__ __forceinline__ float conv_out_sample(const float* xt, long ldx, int C_in, int taps, const float* w, const float* bias) {
    float acc = bias ? bias[0] : 0.f;
    for (int j = 0; j < taps; ++j) {
        const float* xr = xt + (j - (taps - 1)) * ldx;
        const float* wr = w + (long)j * C_in;
        for (int c = 0; c < C_in; c += 4) {
            const float4 v = *reinterpret_cast<const float4*>(xr + c);
            const float4 u = *reinterpret_cast<const float4*>(wr + c);
            acc = fmaf(elu1(v.x), u.x, acc); acc = fmaf(elu1(v.y), u.y, acc);
            acc = fmaf(elu1(v.z), u.z, acc); acc = fmaf(elu1(v.w), u.w, acc);
        }
    }
    return acc;
}

__global__ void k_conv_out(const float* x, long ldx, long T, int C_in, int taps, const float* w /*[taps][1][C_in]*/,
                           const float* bias, float* pcm) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    pcm[t] = conv_out_sample(x + t * ldx, ldx, C_in, taps, w, bias);
}

// slide the left-context window of a [hist + T][C] buffer: new hist rows = last hist rows of (old hist ++ new T rows)
__global__ void k_slide_hist(float* base /*row -hist*/, int hist, long T, int C) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    for (int r = 0; r < hist; ++r) base[(long)r * C + c] = base[((long)r + T) * C + c];   // ascending r: source is always ahead
}

// ---- encode-side kernels ---------------------------------------------------------------
// first encoder conv (1 channel in): out[t][co] = b[co] + sum_k w[k][co] * wav[t - (taps-1) + k]
__global__ void k_enc_conv_in(const float* wav, long n, int taps, int C, const float* w, const float* b, float* out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * C) return;
    const long t = i / C;
    const int co = (int)(i % C);
    float acc = b[co];
    for (int k = 0; k < taps; ++k) {
        const long ti = t - (taps - 1) + k;
        if (ti >= 0) acc = fmaf(wav[ti], w[k * C + co], acc);
    }
    out[i] = acc;
}

// nearest centroid of one RVQ level + residual update: score[t][c] = r_t . e_c (from the GEMM),
// code = argmin_c (|e_c|^2 - 2 score) (first index on ties), r_t -= e_code.   grid = T, block = 256
// A row without a finite minimum (non-finite audio: every score NaN, no comparison below is ever true) takes code 0, the argmin a
// reference gives for an all-NaN row; the residual then stays NaN.  The index written and read through is always inside [0, ncodes).
__global__ __launch_bounds__(256) void k_rvq_pick(const float* score, int ncodes, const float* sqnorm, const float* book, int dim,
                                                  float* resid, int32_t* codes, long code_stride_t) {
    __shared__ float bv[4];
    __shared__ int bi[4];
    __shared__ int pick;
    const int t = blockIdx.x, tid = threadIdx.x;
    float best = INFINITY; int idx = 0;                      // (a thread that takes no candidate ties at +inf and loses to any lower index)
    for (int c = tid; c < ncodes; c += 256) {
        const float dsc = sqnorm[c] - 2.0f * score[(long)t * ncodes + c];
        if (dsc < best) { best = dsc; idx = c; }             // ascending c per thread: keeps the first minimum
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64); const int oi = __shfl_xor(idx, o, 64);
        if (ob < best || (ob == best && oi < idx)) { best = ob; idx = oi; }
    }
    if ((tid & 63) == 0) { bv[tid >> 6] = best; bi[tid >> 6] = idx; }
    __syncthreads();
    if (tid == 0) {
        for (int x = 1; x < 4; ++x) if (bv[x] < best || (bv[x] == best && bi[x] < idx)) { best = bv[x]; idx = bi[x]; }
        if ((unsigned)idx >= (unsigned)ncodes) idx = 0;      // never write, or read the codebook through, an index outside it
        pick = idx; codes[(long)t * code_stride_t] = idx;
    }
    __syncthreads();
    const int e = pick;
    for (int d = tid; d < dim; d += 256) resid[(long)t * dim + d] -= book[(long)e * dim + d];
}

// ---- ragged encode: several clips in one chain (mimi_encode_many; layout: enc_segs.h) ---------------------------------------------------
// first kernel of a call: the per-clip header of the kernel arguments -> the device table every later kernel reads.  One block.
__global__ __launch_bounds__(256) void k_enc_plan(const EncHeader hdr, EncClipTab* clips, int* frame_clip) {
    __shared__ int f0[ENC_MAX_CLIPS + 1];
    const long hop = enc_level_rate(hdr.ratios, hdr.S, 0);
    if (threadIdx.x == 0) {
        int F = 0;
        for (int i = 0; i < hdr.n; ++i) { f0[i] = F; F += (int)enc_ceil_div(hdr.c[i].n_samples, hop); }
        f0[hdr.n] = F;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < hdr.n; i += blockDim.x) {
        clips[i].wav_off = hdr.c[i].wav_off; clips[i].F0 = f0[i];
        for (int l = 0; l < ENC_MAX_LEVELS; ++l) clips[i].L[l] = l <= hdr.S + 1 ? (int)enc_level_len(hdr.c[i].n_samples, hdr.ratios, hdr.S, l) : 0;
    }
    for (int f = threadIdx.x; f < f0[hdr.n]; f += blockDim.x) {
        int c = 0;
        while (f >= f0[c + 1]) ++c;
        frame_clip[f] = c;
    }
}

// k_enc_conv_in over the clips' sample slots: a sample's clip comes from its frame, the taps read the clip's own samples, and the rows of
// a slot's unused tail (no sample behind them) are left alone
__global__ void k_enc_conv_in_many(const float* wav, long rows, int hop, int taps, int C, const float* w, const float* b, const EncClipTab* clips,
                                   const int* frame_clip, float* out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * C) return;
    const long g = i / C;
    const int co = (int)(i % C);
    const EncClipTab& c = clips[frame_clip[g / hop]];
    const long t = g - (long)hop * c.F0;                    // the sample's index inside its clip
    if (t >= c.L[0]) return;
    const float* x = wav + c.wav_off;
    float acc = b[co];
    for (int k = 0; k < taps; ++k) {
        const long ti = t - (taps - 1) + k;
        if (ti >= 0) acc = fmaf(x[ti], w[k * C + co], acc);
    }
    out[i] = acc;
}

// k_mimi_attn over the clips' token slots: position = the token's index inside its clip, keys from the clip's row 0
__global__ __launch_bounds__(64) void k_enc_attn(const float* q, const float* kc, const float* vc, int d, int context, const EncClipTab* clips,
                                                 const int* frame_clip, float* out) {
    __shared__ float pbuf[1024];
    const int g = blockIdx.x, hh = blockIdx.y;
    const long row0 = 2L * clips[frame_clip[g >> 1]].F0;
    attn_row<false>(pbuf, q + (long)g * d + hh * 64, kc + row0 * d + hh * 64, vc + row0 * d + hh * 64, d, (int)(g - row0), context, 0,
                    out + (long)g * d + hh * 64);
}

// the left-context rows of every activation buffer, zeroed by ONE launch (was 11 hipMemsetAsync per stateless decode)
struct ZeroRegions { float* p[3 + 2 * MIMI_MAX_STAGES]; int n[3 + 2 * MIMI_MAX_STAGES]; int count; };
__global__ void k_zero_regions(const ZeroRegions z) {
    const int reg = blockIdx.y;
    if (reg >= z.count) return;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < z.n[reg]; i += gridDim.x * blockDim.x) z.p[reg][i] = 0.f;
}

// ---- stream-pool kernels: N stateful streams decoded by one launch chain (include/mimi_hip.h; the segment layout: struct Ladder) -------
struct PoolIds { int n; int sid[MIMI_POOL_MAX_STREAMS]; int off[MIMI_POOL_MAX_STREAMS]; };
#define POOL_MAX_REGIONS (3 + 2 * MIMI_MAX_STAGES)
struct PoolRegions { float* base[POOL_MAX_REGIONS]; int hist[POOL_MAX_REGIONS], C[POOL_MAX_REGIONS], seg[POOL_MAX_REGIONS]; long T[POOL_MAX_REGIONS]; int count; };

// first kernel of a call: the call's streams and offsets into the device table every later kernel reads, the K-split tickets to zero
__global__ void k_pool_begin(const PoolIds ids, int* tab, int* tickets, int n_tickets) {
    for (int i = threadIdx.x; i < ids.n; i += blockDim.x) { tab[i] = ids.sid[i]; tab[MIMI_POOL_MAX_STREAMS + i] = ids.off[i]; }
    for (int j = threadIdx.x; j < n_tickets; j += blockDim.x) tickets[j] = 0;
}

// its ragged twin (mimi_pool_decode_ragged; layout: pool_segs.h): per segment {stream id, token offset, first frame, frames}, then frame ->
// segment for the call's F frames.  One block.
__global__ __launch_bounds__(256) void k_pool_begin_ragged(const PoolSegHeader hdr, int* tab, int* tickets, int n_tickets) {
    __shared__ int f0[POOL_SEG_MAX_STREAMS + 1];
    if (threadIdx.x == 0) pool_segs_prefix(&hdr, f0);
    __syncthreads();
    for (int i = threadIdx.x; i < hdr.n; i += blockDim.x) {
        tab[POOL_TAB_SID + i] = hdr.sid[i]; tab[POOL_TAB_OFF + i] = hdr.off[i]; tab[POOL_TAB_F0 + i] = f0[i]; tab[POOL_TAB_T + i] = hdr.T[i];
    }
    for (int f = threadIdx.x; f < f0[hdr.n]; f += blockDim.x) tab[POOL_TAB_FRAME + f] = pool_seg_of_frame(f0, f);
    for (int j = threadIdx.x; j < n_tickets; j += blockDim.x) tickets[j] = 0;
}

// The kernels below map a dense row g to (si, tl): the si-th listed stream and the row inside its chunk.  Uniform call: `rows` rows per
// stream, si = g / rows.  PRG (a ragged call): `rows` is the level's rows per FRAME and si = frame_seg[g / rows], tl = g - rows * F0_si.
// (I: int or long, the index type the uniform kernel has always divided in)
template <bool PRG, class I>
__device__ __forceinline__ void pool_row(const int* tab, I g, I rows, int& si, I& tl) {
    if (PRG) { si = tab[POOL_TAB_FRAME + g / rows]; tl = g - rows * tab[POOL_TAB_F0 + si]; }
    else { si = (int)(g / rows); tl = g - si * rows; }
}

template <bool PRG = false>
__global__ __launch_bounds__(256) void k_pool_rvq(const int* codes, long stride_s, long stride_k, long stride_t, int T, int ncb, int nsem,
                                                  int cbsize, int cbdim, int hidden, const float* books, const float* pf, const float* pr,
                                                  float* out /*row 0 of stream 0*/, int seg, const int* tab) {
    extern __shared__ float q[];
    int si, t;
    pool_row<PRG, int>(tab, blockIdx.x, T, si, t);
    rvq_frame(q, codes + si * stride_s + t * stride_t, stride_k, ncb, nsem, cbsize, cbdim, hidden, books, pf, pr,
              out + ((long)tab[si] * seg + t) * hidden);
}

template <bool PRG = false>
__global__ void k_pool_upsample(const float* x /*row 0 of stream 0*/, int seg, const int* tab, int T, int n, int C, const float* w, float* out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)n * T * 2 * C) return;
    const int c = (int)(i % C);
    const long g = i / C;                           // dense output row
    int si; long nl;
    pool_row<PRG, long>(tab, g, 2 * T, si, nl);
    out[g * C + c] = upsample_tap2(x + ((long)tab[si] * seg + (nl >> 1)) * C, (long)C, w, nl & 1, C, c);
}

template <bool PRG = false>
__global__ __launch_bounds__(64) void k_pool_attn(const float* q, const float* kc, const float* vc, int d, int T2, int ring, int context,
                                                  const int* tab, float* out) {
    __shared__ float pbuf[1024];
    const int g = blockIdx.x, hh = blockIdx.y;
    int si, tl;
    pool_row<PRG, int>(tab, g, T2, si, tl);
    const long cache = (long)tab[si] * ring * d + hh * 64;
    attn_row<true>(pbuf, q + (long)g * d + hh * 64, kc + cache, vc + cache, d, tab[MIMI_POOL_MAX_STREAMS + si] + tl, context, ring,
                   out + (long)g * d + hh * 64);
}

template <bool PRG = false>
__global__ void k_pool_conv_out(const float* x /*row 0 of stream 0*/, int seg, const int* tab, long Tj, int n, int C_in, int taps, const float* w,
                                const float* bias, float* pcm) {
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= Tj * n) return;
    int si; long tl;
    pool_row<PRG, long>(tab, g, Tj, si, tl);
    pcm[g] = conv_out_sample(x + ((long)tab[si] * seg + tl) * C_in, (long)C_in, C_in, taps, w, bias);
}

// k_slide_hist for every segmented buffer (blockIdx.z) of every listed stream (blockIdx.y) in one launch.  PRG: z.T is the buffer's rows per
// FRAME and each stream's history moves by ITS chunk, z.T * T_si rows.
template <bool PRG = false>
__global__ void k_pool_slide(const PoolRegions z, const int* tab) {
    const int reg = blockIdx.z, c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= z.C[reg]) return;
    float* base = z.base[reg] + (long)tab[blockIdx.y] * z.seg[reg] * z.C[reg];
    const long T = PRG ? z.T[reg] * tab[POOL_TAB_T + blockIdx.y] : z.T[reg];
    for (int r = 0; r < z.hist[reg]; ++r) base[(long)r * z.C[reg] + c] = base[((long)r + T) * z.C[reg] + c];    // ascending r: source is always ahead
}

__global__ void k_pool_zero_hist(const PoolRegions z, const PoolIds ids) {
    const int reg = blockIdx.z;
    float* base = z.base[reg] + (long)ids.sid[blockIdx.y] * z.seg[reg] * z.C[reg];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < z.hist[reg] * z.C[reg]; i += gridDim.x * blockDim.x) base[i] = 0.f;
}

// ---- encode stream pool: N stateful ENCODE streams fed by one launch chain (mimi_enc_pool_encode; layout: enc_stream_segs.h) ---------------
// first kernel of a call: the header of the kernel arguments -> the device table every later kernel reads.  One block.
__global__ __launch_bounds__(256) void k_enc_stream_plan(const EncStreamHeader hdr, int* tab, long* ltab) {
    __shared__ int f0[POOL_SEG_MAX_STREAMS + 1];
    if (threadIdx.x == 0) enc_stream_prefix(&hdr, f0);
    __syncthreads();
    for (int i = threadIdx.x; i < hdr.n; i += blockDim.x) {
        tab[POOL_TAB_SID + i] = hdr.sid[i]; tab[POOL_TAB_OFF + i] = hdr.off[i]; tab[POOL_TAB_F0 + i] = f0[i]; tab[POOL_TAB_T + i] = f0[i + 1] - f0[i];
        for (int l = 0; l < ENC_MAX_LEVELS; ++l) tab[ENC_STREAM_TAB_L(l) + i] = l <= hdr.S + 1 ? (int)enc_level_len(hdr.n_samples[i], hdr.ratios, hdr.S, l) : 0;
        tab[ENC_STREAM_TAB_FIRST + i] = hdr.off[i] == 0;
        ltab[ENC_STREAM_LTAB_WAV_OFF + i] = hdr.wav_off[i];
    }
    for (int f = threadIdx.x; f < f0[hdr.n]; f += blockDim.x) tab[POOL_TAB_FRAME + f] = pool_seg_of_frame(f0, f);
}

// k_enc_conv_in over the streams' new samples: a sample's segment comes from its frame, the taps in front of the chunk read the stream's
// saved tail (its last taps - 1 samples; zeros after a reset), the output goes to the stream's own segment, and the rows of a last partial
// frame that have no sample behind them are left alone
__global__ void k_enc_stream_conv_in(const float* wav, long rows, int hop, int taps, int C, const float* w, const float* b, const int* tab,
                                     const long* ltab, const float* tail /*[stream][taps - 1]*/, float* out /*row 0 of stream 0*/, int seg) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * C) return;
    const long g = i / C;
    const int co = (int)(i % C);
    const int si = tab[POOL_TAB_FRAME + g / hop];
    const int t = (int)(g - (long)hop * tab[POOL_TAB_F0 + si]);         // the sample's index inside its chunk
    if (t >= tab[ENC_STREAM_TAB_L(0) + si]) return;
    const int sid = tab[POOL_TAB_SID + si];
    const float* x = wav + ltab[ENC_STREAM_LTAB_WAV_OFF + si];
    const float* th = tail + (long)sid * (taps - 1);
    float acc = b[co];
    for (int k = 0; k < taps; ++k) {
        const int ti = t - (taps - 1) + k;
        acc = fmaf(ti >= 0 ? x[ti] : th[taps - 1 + ti], w[k * C + co], acc);
    }
    out[((long)sid * seg + t) * C + co] = acc;
}

// after it: every listed stream's tail = the last `hist` samples of (old tail ++ the chunk).  One block; all reads before any write.
__global__ __launch_bounds__(256) void k_enc_stream_tail(const float* wav, int n, int hist, const int* tab, const long* ltab, float* tail) {
    __shared__ float v[POOL_SEG_MAX_STREAMS * (MAX_TAPS - 1)];
    for (int i = threadIdx.x; i < n * hist; i += blockDim.x) {
        const int si = i / hist, j = tab[ENC_STREAM_TAB_L(0) + si] + (i - si * hist);      // index into (old tail ++ the chunk)
        v[i] = j < hist ? tail[(long)tab[POOL_TAB_SID + si] * hist + j] : wav[ltab[ENC_STREAM_LTAB_WAV_OFF + si] + j - hist];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n * hist; i += blockDim.x) {
        const int si = i / hist;
        tail[(long)tab[POOL_TAB_SID + si] * hist + (i - si * hist)] = v[i];
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
// Activation buffer of N streams that keeps EVERY stream's segment in place: stream s owns rows [s * seg, (s + 1) * seg) with seg = hist +
// the rows of the longest chunk, its `hist` rows of left context in front of its row 0.  A handle is the N = 1 case.
struct SegBuf {
    float* base = nullptr;
    int hist = 0, C = 0, rate = 0;                  // rate: rows per frame at this level
    long cap = 0;                                   // rows of one stream's longest chunk at this level
    int seg() const { return (int)(hist + cap); }   // rows between two streams' segments
    float* row0() const { return base + (long)hist * C; }       // row 0 of stream 0
};

// The buffer ladder that a handle (MimiDecoder, N = 1) and a stream pool embed.  Buffers that feed a causal op are segmented (SegBuf) -- so a
// pool call needs no gather and the slide is what it is for one stream.  Work buffers between two such buffers (tok, ln, q, att, ffn, r1) are
// dense: the listed streams' rows one after the other.  Products between dense buffers are the plain k_gemm32 over n * rows rows; those of a
// pool that touch a segmented buffer, and its q|k|v projection, are the SEG instantiation.
struct Ladder {
    SegBuf sb[3 + 2 * MIMI_MAX_STAGES];             // every buffer with history, in slide order: rvq, a0, s0, then u[j], xj[j] per stage
    int n_sb = 0;
    SegBuf &rvq = sb[0], &a0 = sb[1], &s0 = sb[2];  // rvq out (hist 1), transformer out (hist kernel-1), conv_in out (hist 1)
    SegBuf& u(int j) { return sb[3 + 2 * j]; }
    SegBuf& xj(int j) { return sb[4 + 2 * j]; }
    float* r1[MIMI_MAX_STAGES] = {};
    float *tok = nullptr, *ln = nullptr, *q = nullptr, *att = nullptr, *ffn = nullptr;
    float *kc = nullptr, *vc = nullptr;             // handle: [layer][cap_tokens][d]; pool: [layer][stream][ring][d]
    long kv_layer = 0;                              // floats of one layer in kc / vc
    KSplitWs ksw = {nullptr, nullptr, 0, 0, 0, 0};
};

struct MimiDecoder {
    MimiConfig cfg;
    MimiWeights w;
    int max_frames;
    long cap_tokens;                    // transformer KV capacity (tokens)
    int offset;                         // tokens already in the KV caches (stateful stream)
    Ladder b;
    hipStream_t cap_stream = nullptr;   // graph capture of decode_middle
    hipGraphExec_t mid_exec[65] = {};   // by T (stateless decodes of up to MIMI_GRAPH_MAX_T frames)
    int mid_uses[65] = {};
    EncClipTab* enc_clips = nullptr;    // device table of a ragged encode: [MIMI_ENCODE_MAX_CLIPS] clips, then frame -> clip [max_frames]
    int* enc_frame_clip = nullptr;      // (inside the enc_clips allocation)
    long enc_rows = 0;                  // frames of the last encode call whose latent still lies in b.rvq (0: none; a decode reuses the buffer)
    std::string err;
};

// What a decode pool and an encode pool are alike in: N streams on one ladder, each with its token offset and its K/V ring.
struct PoolBase {
    MimiConfig cfg;
    MimiWeights w;
    int n_streams = 0, max_chunk = 0, ring = 0;
    std::vector<long> offset;                       // tokens each stream has decoded / encoded so far
    Ladder b;
    int* tab = nullptr;                             // device table of the running call: [i] stream id, [MIMI_POOL_MAX_STREAMS + i] token offset;
                                                    // a ragged call also fills the rest (pool_segs.h; an encode pool's: enc_stream_segs.h)
    std::string err;
    ~PoolBase();                                    // frees the ladder and the table (safe on a half-built pool: every pointer starts null)
};

struct MimiStreamPool : PoolBase {};

// The encoder on the pool's ladder: stage j lives in the stage buffers of index S-1-j, as in a handle's encode, but every buffer that feeds
// a convolution with taps keeps each stream's rows IN PLACE behind its history, so the left padding of the whole-clip encode (zeros; row 0
// replicated for the downsample) becomes the rows the stream's previous call left there.
struct MimiEncStreamPool : PoolBase {
    std::vector<unsigned char> ended;               // the stream took a partial last frame: refused until reset
    long* ltab = nullptr;                           // ENC_STREAM_LTAB_LONGS longs behind the table's words (same allocation)
    float* wav_tail = nullptr;                      // [stream][kernel - 1]: the samples in front of the next chunk's first
    long enc_rows = 0;                              // frames of the last encode call: its latent lies dense in b.rvq
    ~MimiEncStreamPool() { (void)hipFree(wav_tail); }
};
static_assert(MIMI_ENC_POOL_MAX_STREAMS == MIMI_POOL_MAX_STREAMS, "PoolIds and pool_ids() serve both kinds of pool");

// h: a handle or a pool (anything with .err), or a null pointer of either type: the thread's error
#define MCHK(h, x)                                                                                     \
    do {                                                                                               \
        hipError_t e_ = (x);                                                                           \
        if (e_ != hipSuccess) {                                                                        \
            char b_[256];                                                                              \
            snprintf(b_, sizeof b_, "%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
            if (h) (h)->err = b_; else g_mimi_err = b_;                                                \
            return -2;                                                                                 \
        }                                                                                              \
    } while (0)

template <class H>
static int fail(H* h, const char* msg) {
    if (h) h->err = msg; else g_mimi_err = msg;
    return -1;
}
static int fail(decltype(nullptr), const char* msg) { return fail((MimiDecoder*)nullptr, msg); }
// "<the entry point's name>: <what a plan or a check found wrong>"
template <class H>
static int fail(H* h, const char* who, const char* bad) { return fail(h, (std::string(who) + ": " + bad).c_str()); }

extern "C" void csm_warn_unknown_switches(void);     // csm_engine.hip: names under CSM_ / MIMI_ that no switch reads, once per process

// what the kernels assume of a configuration (mimi_create and mimi_pool_create)
static const char* config_error(const MimiConfig* cfg) {
    if (cfg->hidden % 32 || cfg->hidden > 1024 || cfg->codebook_dim % 4 || cfg->tr_ffn % 32 || cfg->hidden / cfg->tr_heads != 64)
        return "mimi_create: hidden%32, hidden<=1024, tr_ffn%32 and head_dim==64 required";
    if (cfg->n_stages < 1 || cfg->n_stages > MIMI_MAX_STAGES || cfg->tr_layers > MIMI_MAX_TR_LAYERS || cfg->tr_context > 1024)
        return "mimi_create: too many stages/layers or context > 1024";
    if (cfg->kernel > MAX_TAPS || cfg->res_kernel > MAX_TAPS) return "mimi_create: kernel too wide";
    int c = cfg->n_filters << cfg->n_stages;
    for (int j = 0; j < cfg->n_stages; ++j) { c /= 2; if ((c / 2) % 32) return "mimi_create: SEANet channels must stay multiples of 32"; }
    return nullptr;
}

// columns of ffn where an encoder runs on the ladder (a handle, an encode pool): ffn is also the RVQ score buffer of quantize()
static int enc_ffn_cols(const MimiConfig& c) { return c.tr_ffn > c.codebook_size ? c.tr_ffn : c.codebook_size; }
// samples per frame: rows per frame at level 0 of the encoder (enc_segs.h), the decoder's 2 * prod(ratios)
static long samples_per_frame(const MimiConfig& c) { return enc_level_rate(c.ratios, c.n_stages, 0); }

// The ladder of N streams of up to `frames` frames a call, kv_rows K/V rows per stream and layer, ffn_cols columns of ffn.
// enc: the histories the ENCODER's taps need (an encode stream pool): two rows of a0 in front of the 4-tap downsample, last_kernel - 1 rows
// of s0 in front of the output convolution, ratios[j] rows of xj[j] in front of the strided convolution (taps at -r .. r - 1), none of rvq
// (the downsample's dense output); no K-split workspace, since no encode product takes a K split.
template <class H>
static int ladder_alloc(H* h, Ladder& b, const MimiConfig& c, int N, long frames, long kv_rows, int ffn_cols, bool enc = false) {
    const int d = c.hidden;
    const long M2 = 2L * N * frames;                 // rows of a full call at the transformer's rate
    auto seg = [&](SegBuf& s, int hist, int rate, int C) {
        s.hist = hist; s.C = C; s.rate = rate; s.cap = frames * rate;
        const size_t bytes = (size_t)N * (hist + s.cap) * C * 4;
        hipError_t e = hipMalloc((void**)&s.base, bytes);
        return e != hipSuccess ? e : hipMemset(s.base, 0, bytes);
    };
#define A4(ptr, n) MCHK(h, hipMalloc((void**)&(ptr), (size_t)(n) * 4))
    int C = c.n_filters << c.n_stages, rate = 2;
    const int ccap = C > d ? C : d;                  // widest output of a split product (conv_in); >= hidden
    b.n_sb = 3 + 2 * c.n_stages;
    MCHK(h, seg(b.rvq, enc ? 0 : 1, 1, d));
    MCHK(h, seg(b.a0, enc ? 2 : c.kernel - 1, 2, d));
    MCHK(h, seg(b.s0, enc ? c.last_kernel - 1 : 1, 2, C));
    for (int j = 0; j < c.n_stages; ++j) {
        rate *= c.ratios[j]; C /= 2;
        MCHK(h, seg(b.u(j), c.res_kernel - 1, rate, C));
        A4(b.r1[j], N * frames * rate * (C / 2));
        MCHK(h, seg(b.xj(j), enc ? c.ratios[j] : (j + 1 < c.n_stages) ? 1 : c.last_kernel - 1, rate, C));
    }
    A4(b.tok, M2 * d); A4(b.ln, M2 * d); A4(b.q, M2 * d); A4(b.att, M2 * d); A4(b.ffn, M2 * ffn_cols);
    b.kv_layer = N * kv_rows * d;
    A4(b.kc, c.tr_layers * b.kv_layer); A4(b.vc, c.tr_layers * b.kv_layer);
    // K-split workspace (k_gemm32): the deep products' partial tiles and tile tickets, sized for a full call.  MIMI_KSPLIT=0 in the
    // environment: no split.  (A pool splits the same shapes as a handle: its sums are those of a single handle.)
    const int want = sw_int(SW_MIMI_KSPLIT, MIMI_KSPLIT);
    if (!enc && (want == 2 || want == 4 || want == 8)) {
        b.ksw.ksplit = want; b.ksw.cap_rows = M2; b.ksw.cap_cols = ccap;
        b.ksw.n_tickets = (int)((M2 + 31) / 32) * ((ccap + 31) / 32);
        A4(b.ksw.part, (long)want * M2 * ccap);
        A4(b.ksw.ticket, b.ksw.n_tickets);
        MCHK(h, hipMemset(b.ksw.ticket, 0, (size_t)b.ksw.n_tickets * 4));
    }
#undef A4
    MCHK(h, hipDeviceSynchronize());
    return 0;
}

static void ladder_free(Ladder& b) {                 // (safe on a half-built ladder: every pointer starts null)
    for (SegBuf& s : b.sb) (void)hipFree(s.base);
    for (float* p : b.r1) (void)hipFree(p);
    void* ps[] = {b.tok, b.ln, b.q, b.att, b.ffn, b.kc, b.vc, b.ksw.part, b.ksw.ticket};
    for (void* p : ps) (void)hipFree(p);
}
PoolBase::~PoolBase() { ladder_free(b); (void)hipFree(tab); }

// the buffers with history, with the rows a chunk of T frames adds to each (reset: T = 0)
static PoolRegions hist_regions(const Ladder& b, int T) {
    PoolRegions z;
    z.count = 0;
    for (int i = 0; i < b.n_sb; ++i) {
        const SegBuf& s = b.sb[i];
        if (!s.hist) continue;
        z.base[z.count] = s.base; z.hist[z.count] = s.hist; z.C[z.count] = s.C; z.seg[z.count] = s.seg(); z.T[z.count] = (long)T * s.rate; ++z.count;
    }
    return z;
}

extern "C" int mimi_create(const MimiConfig* cfg, const MimiWeights* w, int max_frames, int reserved, mimi_handle* out) {
    csm_warn_unknown_switches();
    (void)reserved;
    if (!cfg || !w || !out || max_frames < 1) return fail(nullptr, "mimi_create: null/invalid argument");
    if (const char* bad = config_error(cfg)) return fail(nullptr, bad);
    MimiDecoder* m = new MimiDecoder();
    m->cfg = *cfg; m->w = *w; m->max_frames = max_frames; m->offset = 0;
    m->cap_tokens = 2L * max_frames;
    const int rc = ladder_alloc(m, m->b, *cfg, 1, max_frames, m->cap_tokens, enc_ffn_cols(*cfg));
    if (rc) { g_mimi_err = m->err; mimi_destroy(m); return rc; }
    if (w->has_encoder) {
        const size_t clips_bytes = sizeof(EncClipTab) * MIMI_ENCODE_MAX_CLIPS;
        if (hipMalloc((void**)&m->enc_clips, clips_bytes + (size_t)max_frames * 4) != hipSuccess) {
            g_mimi_err = "mimi_create: hipMalloc of the ragged encode's table failed"; mimi_destroy(m); return -2;
        }
        m->enc_frame_clip = reinterpret_cast<int*>(reinterpret_cast<char*>(m->enc_clips) + clips_bytes);
    }
    *out = m;
    return 0;
}

extern "C" void mimi_destroy(mimi_handle m) {
    if (!m) return;
    ladder_free(m->b);
    (void)hipFree(m->enc_clips);
    for (hipGraphExec_t g : m->mid_exec) if (g) (void)hipGraphExecDestroy(g);
    if (m->cap_stream) (void)hipStreamDestroy(m->cap_stream);
    delete m;
}

extern "C" const char* mimi_last_error(mimi_handle m) { return m ? m->err.c_str() : g_mimi_err.c_str(); }

extern "C" int mimi_reset_stream(mimi_handle m, void* stream) {
    if (!m) return -1;
    const PoolRegions r = hist_regions(m->b, 0);
    ZeroRegions z;
    z.count = r.count;
    for (int i = 0; i < r.count; ++i) { z.p[i] = r.base[i]; z.n[i] = r.hist[i] * r.C[i]; }
    if (z.count) {
        hipLaunchKernelGGL(k_zero_regions, dim3(8, z.count), dim3(256), 0, (hipStream_t)stream, z);
        MCHK(m, hipGetLastError());
    }
    m->offset = 0;
    return 0;
}

// ---- one product ---------------------------------------------------------------------------------------------------------------------
struct RopeOut { float *q, *k, *v; const float* freqs; int offset, d; };
// GemmArgs.seg_*: a product over the stacked rows of a stream pool; ragged: T = the launch's rows per frame (the PRG instantiation)
struct SegArgs { int T, x, o, r, by_id, ring; const int* tab; bool ragged; };

// One k_gemm32 launch as its call site states it.  The operands every product has come first (linear() / conv() below fill them); everything
// else is named by a setter and otherwise keeps the default written here.
struct Product {
    const float* x; long ldx, rows;
    const float *w, *bias; int c_in, c_out, taps, phases;
    float* out; long ldo;
    int shift0 = 0, dshift = 0;                     // tap j reads row t * in_stride + shift0 + j * dshift
    bool elu_in = false, gelu_out = false;
    const float *col_scale = nullptr, *resid = nullptr; long ldr = 0;
    int in_stride = 1, edge = 0, row_lo = 0, row_hi = 0;
    RopeOut ro = {};                                // ro.q != nullptr: the q|k|v projection
    const KSplitWs* ksw = nullptr;
    SegArgs sg = {};                                // sg.tab != nullptr: the SEG instantiation
    RagArgs rg = {};                                // rg.clips != nullptr: the RAG instantiation (a ragged encode)
    int ens_L = -1;                                 // >= 0: the ENS instantiation (an encode stream pool), with seg()
    Product& taps_at(int s0, int ds) { shift0 = s0; dshift = taps > 1 ? ds : 0; return *this; }
    Product& elu() { elu_in = true; return *this; }
    Product& gelu() { gelu_out = true; return *this; }
    Product& residual(const float* r, long ld) { resid = r; ldr = ld; return *this; }
    Product& scale_residual(const float* cs, const float* r, long ld) { col_scale = cs; return residual(r, ld); }      // LayerScale, then + r
    Product& rope(const RopeOut& r) { ro = r; return *this; }
    Product& ksplit(const KSplitWs& k) { ksw = &k; return *this; }
    Product& seg(const SegArgs& s) { if (s.tab) sg = s; return *this; }        // (no table: a handle's one stream, the plain instantiation)
    // a product of a ragged encode from level lvl_in to lvl_out (enc_segs.h); no table: one clip, the plain instantiation
    Product& rag(const RagArgs* r, int lvl_in, int lvl_out, const MimiConfig& c) {
        if (r) { rg = *r; rg.lvl_in = lvl_in; rg.lvl_out = lvl_out; rg.rate_in = (int)enc_level_rate(c.ratios, c.n_stages, lvl_in); rg.rate_out = (int)enc_level_rate(c.ratios, c.n_stages, lvl_out); }
        return *this;
    }
    Product& stride(int s) { in_stride = s; return *this; }                       // a down-sampling conv
    Product& zero_padded(long lo, long hi) { edge = 1; row_lo = (int)lo; row_hi = (int)hi; return *this; }       // input rows outside [lo, hi) read as zero
    Product& replicate_padded(long lo, long hi) { edge = 2; row_lo = (int)lo; row_hi = (int)hi; return *this; }  // ... are clamped into [lo, hi)
    // a product of an encode stream pool whose taps pass its segment's rows: `hist` rows of the stream's history below (a replicate edge at
    // token offset 0: row 0), the segment's rows at level lvl_in above, padded as `edge_mode` says (1 zero, 2 replicate)
    Product& seg_edges(int edge_mode, int hist, int lvl_in) { edge = edge_mode; row_lo = -hist; row_hi = 0; ens_L = ENC_STREAM_TAB_L(lvl_in); return *this; }
};
static Product linear(const float* x, long ldx, long rows, const float* w, int c_in, int c_out, float* out, long ldo) {
    return Product{x, ldx, rows, w, nullptr, c_in, c_out, 1, 1, out, ldo};
}
// a MimiConv brings its own w, bias, c_in, c_out, taps, phases; causal (tap j reads row t + j - (taps - 1)) unless taps_at() says otherwise
static Product conv(const float* x, long ldx, long rows, const MimiConv& cv, float* out, long ldo) {
    return Product{x, ldx, rows, cv.w, cv.bias, cv.c_in, cv.c_out, cv.taps, cv.phases, out, ldo}.taps_at(-(cv.taps - 1), 1);
}

// the ten k_gemm32 instantiations there are, [variant][ELU]: <ELU, SEG, RAG, PRG, ENS>
enum { G32_PLAIN, G32_SEG, G32_SEG_PRG, G32_SEG_PRG_ENS, G32_RAG };
static void (*const k_gemm32_of[5][2])(const GemmArgs) = {
    {k_gemm32<false>, k_gemm32<true>},
    {k_gemm32<false, true>, k_gemm32<true, true>},
    {k_gemm32<false, true, false, true>, k_gemm32<true, true, false, true>},
    {k_gemm32<false, true, false, true, true>, k_gemm32<true, true, false, true, true>},
    {k_gemm32<false, false, true>, k_gemm32<true, false, true>},
};

static hipError_t gemm(hipStream_t st, const Product& g) {
    GemmArgs a;
    memset(&a, 0, sizeof a);
    const bool rope = g.ro.q != nullptr, seg = g.sg.tab != nullptr;
    if (rope) { a.rope_q = g.ro.q; a.rope_k = g.ro.k; a.rope_v = g.ro.v; a.rope_freqs = g.ro.freqs; a.rope_offset = g.ro.offset; a.rope_d = g.ro.d; }
    a.in_stride = g.in_stride; a.edge = g.edge; a.row_lo = g.row_lo; a.row_hi = g.row_hi;
    a.x = g.x; a.ldx = g.ldx; a.T_in = (int)g.rows; a.C_in = g.c_in; a.C_out = g.c_out; a.w = g.w; a.bias = g.bias; a.taps = g.taps;
    a.phases = g.phases;
    a.shift0 = g.shift0; a.dshift = g.dshift;           // (every convolution here is an arithmetic progression of taps)
    a.act_out = g.gelu_out ? 1 : 0; a.col_scale = g.col_scale; a.resid = g.resid; a.ldr = g.ldr; a.out = g.out; a.ldo = g.ldo;
    dim3 grid((unsigned)((g.rows + 31) / 32), (unsigned)((g.c_out + 31) / 32), (unsigned)g.phases);
    // (the choice depends on the product's shape alone, never on T_in: a streamed chunk and the whole clip sum in the same order)
    const int iters = g.taps * (g.c_in / 32);
    const KSplitWs* ksw = g.ksw;
    if (ksw != nullptr && ksw->part != nullptr && g.phases == 1 && !rope && iters >= MIMI_KSPLIT_MIN_ITERS && iters % ksw->ksplit == 0) {
        // (the workspace is sized for the handle's max_frames at mimi_create, so a product the decoder accepts always fits; if one ever
        //  does not, it runs unsplit -- same value to fp32 rounding -- instead of failing the decode: ADVICE r5.  A ragged pool call has
        //  F <= n_streams * max_chunk_frames frames, so its split products -- lin2 and conv_in, 2 F token rows -- fit the workspace of the
        //  uniform call at T = max_chunk_frames that mimi_pool_create sized it for: the unsplit branch stays unreachable, and a stream's
        //  sums stay those of the uniform call.)
        if (g.rows <= ksw->cap_rows && g.c_out <= ksw->cap_cols && (long)grid.x * grid.y <= ksw->n_tickets) {
            a.ksplit = ksw->ksplit; a.kpart = ksw->part; a.kticket = ksw->ticket;
            grid.z = (unsigned)ksw->ksplit;
        }
    }
    // the instantiation: a variant (a table wins over a clip list, as it always has; ens_L counts in a ragged pool call only) and ELU
    int v = G32_PLAIN;
    if (seg) {
        const SegArgs& s = g.sg;
        a.seg_T = s.T; a.seg_x = s.x; a.seg_o = s.o; a.seg_r = s.r; a.seg_by_id = s.by_id; a.rope_ring = s.ring; a.seg_tab = s.tab;
        v = !s.ragged ? G32_SEG : g.ens_L < 0 ? G32_SEG_PRG : G32_SEG_PRG_ENS;
        if (v == G32_SEG_PRG_ENS) a.ens_L = g.ens_L;
    } else if (g.rg.clips != nullptr) {
        a.rag = g.rg;
        v = G32_RAG;
    }
    hipLaunchKernelGGL(k_gemm32_of[v][g.elu_in], grid, dim3(64 * G32_NW), 0, st, a);
    return hipGetLastError();
}

// ---- the chains every user shares: transformer, SEANet decoder, encoder ------------------------------------------------------------------
// What differs between the transformer's users: the handle's decode, the decode pool, and the encoder's three (EncPass below).
struct TrPass {
    const MimiTrLayer* layers;
    long rows;                      // 2T (decode), L (encode), n * 2T (pool: the listed streams' rows stacked)
    int offset = 0;                 // tokens already in the handle's linear K/V cache: RoPE position and cache row of row 0 (encode: 0)
    bool lin2_ksplit = true;        // false for the encoder alone: unsplit, its lin2 sums in another order, and the encode goldens were recorded so
    const int* tab = nullptr;       // pool only: the call's table (position and K/V ring row per stream come from it), rows per stream, ring
    int T2 = 0, ring = 0;
    bool ragged = false;            // pool only: a ragged call -- rows = 2 F, T2 = 2 (the tokens of one frame), the streams frame-aligned
    const RagArgs* rag = nullptr;   // ragged encode only: the clips' table (RoPE position and attention window inside the token's clip)
};

// What differs between the encoder's three users: one clip (mimi_encode), a clip list (mimi_encode_many) and an encode stream pool.  The
// last two are frame-aligned: a clip or a chunk owns whole frames, R rows each at a level with R rows per frame.
struct EncPass {
    long rows0, frames;             // rows at level 0 (the one clip's samples, or frames * samples per frame); frames: the latent's rows
    const RagArgs* rag = nullptr;   // clip list only: the clips' table (the RAG instantiation)
    const int* tab = nullptr;       // pool only: the call's table (SEG + PRG; ENS where a product reaches forward) and the K/V ring
    int ring = 0;
    // the encoder transformer's pass over `rows` tokens: stateless, or on the pool's rings.  No K split (TrPass::lin2_ksplit says why).
    TrPass tr(const MimiWeights& w, long rows) const {
        TrPass tp{w.enc_tr, rows};
        tp.lin2_ksplit = false; tp.rag = rag; tp.tab = tab; tp.T2 = 2; tp.ring = ring; tp.ragged = tab != nullptr;
        return tp;
    }
    // The ONE place that says how a product learns where its input ends.  reach: the rows its taps read -- its OWN, BACK from it, also
    // FORWARD; kind: 1 zero, 2 replicate padding; L: the launch's rows at the input level; hist: the input buffer's history rows.
    //  * Clips: [0, L), and from the clip list's table the row's own clip inside it.  The one-tap res2 never leaves its row, so it takes no
    //    table: in a clip list too it stays the plain instantiation, its padding an edge that is never reached.
    //  * Pool: every stream's history lies in place, so res2, res1 and the output convolution read rows that are always there -- a decode
    //    pool's ragged product, no edge.  The strided products (down-convolutions, downsample) also reach forward, to where a stream's
    //    last partial frame has the whole-clip encode's right padding: seg_edges.
    enum Reach { OWN, BACK, FORWARD };
    Product& edges(Product& g, const MimiConfig& c, Reach reach, int lvl_in, int lvl_out, int kind, long L, int hist) const {
        if (tab) return reach == FORWARD ? g.seg_edges(kind, hist, lvl_in) : g;
        if (kind == 1) g.zero_padded(0, L); else g.replicate_padded(0, L);
        return reach == OWN ? g : g.rag(rag, lvl_in, lvl_out, c);
    }
};

static long ceil_div(long a, long b) { return (a + b - 1) / b; }

// layernorm, q|k|v + RoPE, attention, out-proj + LayerScale + residual, layernorm, lin1 + GELU, lin2 + LayerScale + residual: tok -> a0
template <class H>
static int transformer(H* h, const MimiConfig& c, const MimiWeights& w, Ladder& b, const TrPass& p, hipStream_t st) {
    const int d = c.hidden;
    for (int l = 0; l < c.tr_layers; ++l) {
        const MimiTrLayer& L = p.layers[l];
        const bool last = l + 1 == c.tr_layers;
        float *kc = b.kc + l * b.kv_layer, *vc = b.vc + l * b.kv_layer;
        hipLaunchKernelGGL(k_layernorm, dim3((unsigned)p.rows), dim3(64), 0, st, b.tok, d, L.ln1_w, L.ln1_b, c.norm_eps, b.ln);
        MCHK(h, gemm(st, linear(b.ln, d, p.rows, L.in_proj, d, 3 * d, nullptr, 0).rope({b.q, kc, vc, w.rope_freqs, p.offset, d})
                             .seg({p.T2, p.T2, p.T2, p.T2, 0, p.ring, p.tab, p.ragged}).rag(p.rag, c.n_stages, c.n_stages, c)));
        if (p.rag) hipLaunchKernelGGL(k_enc_attn, dim3((unsigned)p.rows, c.tr_heads), dim3(64), 0, st, b.q, kc, vc, d, c.tr_context, p.rag->clips, p.rag->frame_clip, b.att);
        else if (p.tab && p.ragged) hipLaunchKernelGGL(k_pool_attn<true>, dim3((unsigned)p.rows, c.tr_heads), dim3(64), 0, st, b.q, kc, vc, d, p.T2, p.ring, c.tr_context, p.tab, b.att);
        else if (p.tab) hipLaunchKernelGGL(k_pool_attn<false>, dim3((unsigned)p.rows, c.tr_heads), dim3(64), 0, st, b.q, kc, vc, d, p.T2, p.ring, c.tr_context, p.tab, b.att);
        else hipLaunchKernelGGL(k_mimi_attn, dim3((unsigned)p.rows, c.tr_heads), dim3(64), 0, st, b.q, kc, vc, d, p.offset, c.tr_context, b.att);
        MCHK(h, gemm(st, linear(b.att, d, p.rows, L.out_proj, d, d, b.tok, d).scale_residual(L.ls1, b.tok, d)));
        hipLaunchKernelGGL(k_layernorm, dim3((unsigned)p.rows), dim3(64), 0, st, b.tok, d, L.ln2_w, L.ln2_b, c.norm_eps, b.ln);
        MCHK(h, gemm(st, linear(b.ln, d, p.rows, L.lin1, d, c.tr_ffn, b.ffn, c.tr_ffn).gelu()));
        Product g = linear(b.ffn, c.tr_ffn, p.rows, L.lin2, c.tr_ffn, d, last ? b.a0.row0() : b.tok, d).scale_residual(L.ls2, b.tok, d);
        if (p.lin2_ksplit) g.ksplit(b.ksw);
        if (last) g.seg({p.T2, p.T2, b.a0.seg(), p.T2, 2, 0, p.tab, p.ragged});            // the last layer writes the streams' a0 segments
        MCHK(h, gemm(st, g));
        MCHK(h, hipGetLastError());
    }
    return 0;
}

// SEANet decoder: a0 -> conv_in -> per stage up / res1 / res2 -> xj[last], for n streams of T2 rows each (a handle: n = 1, no table).
// A ragged pool call: n = the call's frames, T2 = 2 -- every level's rows per FRAME where the uniform call has rows per stream.
template <class H>
static int seanet_decoder(H* h, const MimiWeights& w, int n_stages, Ladder& b, int n, int T2, const int* tab, hipStream_t st, bool rg = false) {
    MCHK(h, gemm(st, conv(b.a0.row0(), b.a0.C, (long)n * T2, w.conv_in, b.s0.row0(), w.conv_in.c_out).ksplit(b.ksw)
                         .seg({T2, b.a0.seg(), b.s0.seg(), 0, 1 | 2, 0, tab, rg})));
    const SegBuf* xin = &b.s0;
    int Tj = T2;                                                        // rows per stream at the current level
    for (int j = 0; j < n_stages; ++j) {
        const MimiConv &up = w.up[j], &r1 = w.res1[j], &r2 = w.res2[j];
        const SegBuf &u = b.u(j), &xj = b.xj(j);
        // ELU -> ConvTranspose1d (stride phases, 2 taps each: rows t and t - 1)
        MCHK(h, gemm(st, conv(xin->row0(), xin->C, (long)n * Tj, up, u.row0(), up.c_out).taps_at(0, -1).elu()
                             .seg({Tj, xin->seg(), u.seg(), 0, 1 | 2, 0, tab, rg})));
        Tj *= up.phases;
        // residual block: u + conv_k1(ELU(conv_k3(ELU(u))))
        MCHK(h, gemm(st, conv(u.row0(), up.c_out, (long)n * Tj, r1, b.r1[j], r1.c_out).elu().seg({Tj, u.seg(), Tj, 0, 1, 0, tab, rg})));
        MCHK(h, gemm(st, conv(b.r1[j], r1.c_out, (long)n * Tj, r2, xj.row0(), r2.c_out).elu().residual(u.row0(), up.c_out)
                             .seg({Tj, Tj, xj.seg(), u.seg(), 2 | 4, 0, tab, rg})));
        xin = &xj;
    }
    return 0;
}

// SEANet encoder, from the first convolution's output (in u[S-1]; the front kernels write it) to tok: per stage res1 / res2 / strided
// down-conv, then the output convolution.  Stage j lives in the decoder's stage buffers of index S-1-j (same time scale and width).
// *tok_rows: the rows at the tokens' level.  (.seg() without a table -- the clips -- is a no-op, as in seanet_decoder.)
template <class H>
static int seanet_encoder(H* h, const MimiConfig& c, const MimiWeights& w, Ladder& b, const EncPass& p, hipStream_t st, long* tok_rows) {
    const int S = c.n_stages;
    long L = p.rows0;                                                   // rows of a launch at the current level
    int R = (int)samples_per_frame(c), C = c.n_filters;                 // its rows per frame, its channels
    for (int j = 0; j < S; ++j) {
        const int bi = S - 1 - j;
        const MimiConv &r1 = w.enc_res1[j], &r2 = w.enc_res2[j], &dn = w.enc_down[j];
        const SegBuf &u = b.u(bi), &xj = b.xj(bi), &nxt = (j + 1 < S) ? b.u(bi - 1) : b.s0;
        // residual block: u + conv_k1(ELU(conv_k3(ELU(u))))
        MCHK(h, gemm(st, p.edges(conv(u.row0(), C, L, r1, b.r1[bi], r1.c_out).elu().seg({R, u.seg(), R, 0, 1, 0, p.tab, true}),
                                 c, EncPass::BACK, j, j, 1, L, u.hist)));
        MCHK(h, gemm(st, p.edges(conv(b.r1[bi], r1.c_out, L, r2, xj.row0(), C).elu().residual(u.row0(), C).seg({R, R, xj.seg(), u.seg(), 2 | 4, 0, p.tab, true}),
                                 c, EncPass::OWN, j, j, 1, L, 0)));
        // ELU -> strided conv k = 2r: out[t] = sum_k W_k x[t*r + k - r]; zero padding on both sides.  Frame-aligned rows divide exactly
        // (frames * R, r divides R); one clip's last row rounds up, the partial window the right padding completes.
        const int r = dn.taps / 2;
        const long Lo = (p.rag || p.tab) ? L / r : ceil_div(L, r);
        MCHK(h, gemm(st, p.edges(conv(xj.row0(), C, Lo, dn, nxt.row0(), dn.c_out).taps_at(-r, 1).stride(r).elu().seg({R / r, xj.seg(), nxt.seg(), 0, 1 | 2, 0, p.tab, true}),
                                 c, EncPass::FORWARD, j, j + 1, 1, L, xj.hist)));
        L = Lo; R /= r; C = dn.c_out;
    }
    MCHK(h, gemm(st, p.edges(conv(b.s0.row0(), C, L, w.enc_conv_out, b.tok, c.hidden).elu().seg({R, b.s0.seg(), R, 0, 1, 0, p.tab, true}),
                             c, EncPass::BACK, S, S, 1, L, b.s0.hist)));
    *tok_rows = L;
    return 0;
}

// stride-2 downsample, taps at rows 2t - 2 .. 2t + 1, replicate padding, no bias: a0 -> the latent, dense in the rvq buffer [frames][d]
template <class H>
static int encode_downsample(H* h, const MimiConfig& c, const MimiWeights& w, Ladder& b, const EncPass& p, long tok_rows, hipStream_t st) {
    const int d = c.hidden, S = c.n_stages;
    const MimiConv down = {w.downsample, nullptr, d, d, 4, 1};
    MCHK(h, gemm(st, p.edges(conv(b.a0.row0(), d, p.frames, down, b.rvq.row0(), d).taps_at(-2, 1).stride(2).seg({1, b.a0.seg(), 1, 0, 1, 0, p.tab, true}),
                             c, EncPass::FORWARD, S, S + 1, 2, tok_rows, b.a0.hist)));
    return 0;
}

// split RVQ of the latent's `rows` rows: semantic level on in_proj_first(z), acoustic levels on in_proj_rest(z); per codebook the scores
// against the residual (into ffn), then nearest centroid and residual update -> codes [codebook][rows]
template <class H>
static int quantize(H* h, const MimiConfig& c, const MimiWeights& w, Ladder& b, long rows, int32_t* codes, hipStream_t st) {
    const int d = c.hidden, cd = c.codebook_dim;
    float *res_first = b.ln, *res_rest = b.q;       // [rows][cd]
    MCHK(h, gemm(st, linear(b.rvq.row0(), d, rows, w.in_proj_first, d, cd, res_first, cd)));
    MCHK(h, gemm(st, linear(b.rvq.row0(), d, rows, w.in_proj_rest, d, cd, res_rest, cd)));
    for (int k = 0; k < c.n_codebooks; ++k) {
        float* res = k < c.n_semantic ? res_first : res_rest;
        const float* book = w.codebooks + (long)k * c.codebook_size * cd;
        MCHK(h, gemm(st, linear(res, cd, rows, book, cd, c.codebook_size, b.ffn, c.codebook_size)));
        hipLaunchKernelGGL(k_rvq_pick, dim3((unsigned)rows), dim3(256), 0, st, b.ffn, c.codebook_size,
                           w.codebook_sqnorm + (long)k * c.codebook_size, book, cd, res, codes + (long)k * rows, 1L);
        MCHK(h, hipGetLastError());
    }
    return 0;
}

// every buffer with history slides by its stream's chunk, for the call's n listed streams in one launch: `per` frames each, or -- PRG, a
// ragged call -- per = 1 and each stream's own frame count from the table
template <bool PRG, class H>
static int pool_slide(H* h, const Ladder& b, int per, int n, const int* tab, hipStream_t st) {
    const PoolRegions z = hist_regions(b, per);
    int maxC = 0;
    for (int r = 0; r < z.count; ++r) maxC = z.C[r] > maxC ? z.C[r] : maxC;
    hipLaunchKernelGGL(k_pool_slide<PRG>, dim3((maxC + 255) / 256, n, z.count), dim3(256), 0, st, z, tab);
    MCHK(h, hipGetLastError());
    return 0;
}

// ---- single handle ---------------------------------------------------------------------------------------------------------------------
// A decode is three pieces: front (the only kernel that reads the caller's codes), middle (everything between buffers the handle
// owns: up-sampling, transformer, SEANet stages -- ~70 launches whose arguments depend on T and the stream offset only) and back (the
// only kernel that writes the caller's PCM).  The middle of a STATELESS decode (offset 0) is replayed from a hipGraph per T.
static int decode_front(MimiDecoder* m, const int32_t* codes, long stride_k, long stride_t, int T, hipStream_t st) {
    const MimiConfig& c = m->cfg;
    const int d = c.hidden;
    // RVQ lookup-sum + output projections -> rvq [T][d]
    hipLaunchKernelGGL(k_rvq, dim3(T, (d + 63) / 64), dim3(256), (size_t)(2 * c.codebook_dim + c.n_codebooks) * 4, st, codes, stride_k, stride_t, T, c.n_codebooks,
                       c.n_semantic, c.codebook_size, c.codebook_dim, d, m->w.codebooks, m->w.proj_first, m->w.proj_rest,
                       m->b.rvq.row0(), (long)d);
    MCHK(m, hipGetLastError());
    return 0;
}

static int decode_middle(MimiDecoder* m, int T, hipStream_t st) {
    Ladder& b = m->b;
    const int d = m->cfg.hidden;
    // (ONE stream per handle: the K-split partial tiles and their tickets are per handle, include/mimi_hip.h)
    // depthwise transposed conv x2 -> tok [2T][d]
    hipLaunchKernelGGL(k_upsample, dim3((unsigned)((2L * T * d + 255) / 256)), dim3(256), 0, st, b.rvq.row0(), (long)d, T, d,
                       m->w.upsample, b.tok, (long)d, b.ksw.ticket, b.ksw.ticket ? b.ksw.n_tickets : 0);
    MCHK(m, hipGetLastError());
    TrPass tp{m->w.tr, 2L * T};
    tp.offset = m->offset;
    if (int rc = transformer(m, m->cfg, m->w, b, tp, st)) return rc;
    return seanet_decoder(m, m->w, m->cfg.n_stages, b, 1, 2 * T, nullptr, st);
}

static int decode_back(MimiDecoder* m, int T, float* pcm, hipStream_t st) {
    const SegBuf& last = m->b.xj(m->cfg.n_stages - 1);
    const long Tj = (long)T * last.rate;
    const MimiConv& co = m->w.conv_out;
    hipLaunchKernelGGL(k_conv_out, dim3((unsigned)((Tj + 255) / 256)), dim3(256), 0, st, last.row0(), (long)last.C, Tj, co.c_in, co.taps, co.w,
                       co.bias, pcm);
    MCHK(m, hipGetLastError());
    return 0;
}

// chunk sizes whose middle is worth a graph (a streaming chunk is 10 frames, the last one of an utterance 1..9): captured at the
// SECOND stateless decode of a T, replayed from then on.  Longer decodes (whole utterances, a different T every time) stay eager.
static const int MIMI_GRAPH_MAX_T = sw_int(SW_MIMI_GRAPH_MAX_T, 32);

static int decode_one(MimiDecoder* m, const int32_t* codes, long stride_k, long stride_t, int T, float* pcm, hipStream_t st, bool stateless) {
    int rc = decode_front(m, codes, stride_k, stride_t, T, st);
    if (rc) return rc;
    if (stateless && T <= MIMI_GRAPH_MAX_T && T < (int)(sizeof m->mid_uses / sizeof m->mid_uses[0]) && m->offset == 0) {
        if (!m->mid_exec[T] && ++m->mid_uses[T] >= 2) {
            if (!m->cap_stream) MCHK(m, hipStreamCreateWithFlags(&m->cap_stream, hipStreamNonBlocking));
            hipGraph_t g = nullptr;
            MCHK(m, hipStreamBeginCapture(m->cap_stream, hipStreamCaptureModeThreadLocal));
            const int rc_mid = decode_middle(m, T, m->cap_stream);
            const hipError_t e2 = hipStreamEndCapture(m->cap_stream, &g);
            if (rc_mid) { if (g) (void)hipGraphDestroy(g); return rc_mid; }
            MCHK(m, e2);
            const hipError_t e3 = hipGraphInstantiate(&m->mid_exec[T], g, nullptr, nullptr, 0);
            (void)hipGraphDestroy(g);
            MCHK(m, e3);
        }
        if (m->mid_exec[T]) {
            MCHK(m, hipGraphLaunch(m->mid_exec[T], st));
            return decode_back(m, T, pcm, st);
        }
    }
    rc = decode_middle(m, T, st);
    if (rc) return rc;
    return decode_back(m, T, pcm, st);
}

// slide the left-context window of every buffer with history by a chunk of T frames
static int slide_all(MimiDecoder* m, int T, hipStream_t st) {
    const PoolRegions z = hist_regions(m->b, T);
    for (int r = 0; r < z.count; ++r) {
        hipLaunchKernelGGL(k_slide_hist, dim3((z.C[r] + 255) / 256), dim3(256), 0, st, z.base[r], z.hist[r], z.T[r], z.C[r]);
        MCHK(m, hipGetLastError());
    }
    return 0;
}

// One clip of n samples (T frames), or -- rag: the table of a ragged encode -- the clips of the table in their frame-aligned slots: T = the
// call's frames in all, every level runs over all of its rate * T rows, and the products that reach beyond their own row take the edge
// bounds of the row's clip from the table (the RAG instantiation) in place of [0, L).  No left context here: the input is zero-padded.
static int encode_one(MimiDecoder* m, const float* wav, long n, int32_t* codes, long T, hipStream_t st, const RagArgs* rag = nullptr) {
    const MimiConfig& c = m->cfg;
    const MimiWeights& w = m->w;
    Ladder& b = m->b;
    const long hop = samples_per_frame(c);
    EncPass p{rag ? hop * T : n, T}; p.rag = rag;
    // front: the first convolution (1 channel in) -> u[S-1]
    const int C = c.n_filters; const long tot = p.rows0 * C;
    if (rag) hipLaunchKernelGGL(k_enc_conv_in_many, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, wav, p.rows0, (int)hop, c.kernel, C,
                                w.enc_conv_in_w, w.enc_conv_in_b, rag->clips, rag->frame_clip, b.u(c.n_stages - 1).row0());
    else hipLaunchKernelGGL(k_enc_conv_in, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, wav, p.rows0, c.kernel, C,
                            w.enc_conv_in_w, w.enc_conv_in_b, b.u(c.n_stages - 1).row0());
    long L;
    if (int rc = seanet_encoder(m, c, w, b, p, st, &L)) return rc;
    if (int rc = transformer(m, c, w, b, p.tr(w, L), st)) return rc;
    if (int rc = encode_downsample(m, c, w, b, p, L, st)) return rc;
    return quantize(m, c, w, b, T, codes, st);
}

extern "C" int mimi_encode(mimi_handle m, const float* wav, long n_samples, long stride_b, int B, int32_t* codes, void* stream) {
    if (!m || !wav || !codes || B < 1 || n_samples < 1) return fail(m, "mimi_encode: bad argument");
    if (!m->w.has_encoder) return fail(m, "mimi_encode: this codec was created without encoder weights");
    const long T = ceil_div(n_samples, samples_per_frame(m->cfg));
    if (T > m->max_frames) return fail(m, "mimi_encode: audio longer than hop * max_frames");
    hipStream_t st = (hipStream_t)stream;
    for (int b = 0; b < B; ++b) {
        if (int rc = encode_one(m, wav + (long)b * stride_b, n_samples, codes + (long)b * m->cfg.n_codebooks * T, T, st)) return rc;
    }
    m->enc_rows = T;
    return mimi_reset_stream(m, stream);      // the work buffers were reused: start any later stream from scratch
}

extern "C" int mimi_encode_many(mimi_handle m, const float* wav, const long* wav_off, const long* n_samples, int n, int32_t* codes, void* stream) {
    if (!m) return fail(m, "mimi_encode_many: null handle");
    EncHeader hdr;
    EncSegs sg;
    if (const char* bad = enc_segs_build(wav, wav_off, n_samples, n, codes, m->w.has_encoder, m->cfg.ratios, m->cfg.n_stages, m->max_frames, &hdr, &sg))
        return fail(m, "mimi_encode_many", bad);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_enc_plan, dim3(1), dim3(256), 0, st, hdr, m->enc_clips, m->enc_frame_clip);
    MCHK(m, hipGetLastError());
    const RagArgs rag = {m->enc_clips, m->enc_frame_clip, 0, 0, 0, 0};
    if (int rc = encode_one(m, wav, 0, codes, sg.F, st, &rag)) return rc;
    m->enc_rows = sg.F;
    return mimi_reset_stream(m, stream);      // as mimi_encode
}

// The pre-quantisation latent of the last encode call, which the chain leaves dense in the rvq buffer ([rows][hidden]; mimi_reset_stream
// zeroes history rows only): a device-to-device copy on the caller's stream, nothing else.
template <class H>
static int copy_encode_latent(H* h, const char* who, const float* src, long have, int hidden, float* out, long rows, void* stream) {
    if (rows < 1 || rows != have) {
        h->err = std::string(who) + ": rows is not the frame count of the last encode call (" + std::to_string(have) +
                 "; 0: no encode yet, or a decode has reused the buffer)";
        return -1;
    }
    if (!out) { h->err = std::string(who) + ": null pointer"; return -1; }
    MCHK(h, hipMemcpyAsync(out, src, (size_t)rows * hidden * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

extern "C" int mimi_debug_encode_latent(mimi_handle m, float* out, long rows, void* stream) {
    if (!m) return fail(m, "mimi_debug_encode_latent: null handle");
    return copy_encode_latent(m, "mimi_debug_encode_latent", m->b.rvq.row0(), m->enc_rows, m->cfg.hidden, out, rows, stream);
}

extern "C" int mimi_decode_strided(mimi_handle m, const int32_t* codes, int B, int T, long stride_b, long stride_k, long stride_t,
                                   void* pcm, int stateful, void* stream) {
    if (!m || !codes || !pcm || B < 1 || T < 1) return fail(m, "mimi_decode: bad argument");
    if (T > m->max_frames) return fail(m, "mimi_decode: T exceeds max_frames given to mimi_create");
    if (stateful && B != 1) return fail(m, "mimi_decode: stateful streaming needs B == 1");
    m->enc_rows = 0;                           // the code lookup writes the rvq buffer: the last encode's latent is gone
    hipStream_t st = (hipStream_t)stream;
    const long hop = samples_per_frame(m->cfg);
    for (int b = 0; b < B; ++b) {
        if (!stateful) { int rc = mimi_reset_stream(m, stream); if (rc) return rc; }
        if (m->offset + 2L * T > m->cap_tokens) return fail(m, "mimi_decode: stream longer than max_frames; call mimi_reset_stream");
        int rc = decode_one(m, codes + (long)b * stride_b, stride_k, stride_t, T, (float*)pcm + (long)b * hop * T, st, !stateful);
        if (rc) return rc;
        if (stateful) { rc = slide_all(m, T, st); if (rc) return rc; m->offset += 2 * T; }
    }
    return 0;
}

extern "C" int mimi_decode(mimi_handle m, const int32_t* codes, int B, int T, long stride_b, long stride_k, void* pcm,
                           int stateful, void* stream) {
    return mimi_decode_strided(m, codes, B, T, stride_b, stride_k, 1, pcm, stateful, stream);
}

// ---- the skeleton of both kinds of pool ---------------------------------------------------------------------------------------------------
// What both create functions check and fill before they allocate anything: 0 and the new pool in *pp, or -1 and the thread's error under
// the caller's name `who` (max_name: its n_streams limit, as the header spells it)
template <class P>
static int pool_new(const char* who, const char* max_name, bool need_encoder, const MimiConfig* cfg, const MimiWeights* w, const void* out,
                    int n_streams, int max_chunk_frames, P** pp) {
    csm_warn_unknown_switches();
    const std::string f = std::string(who) + ": ";
    if (!cfg || !w || !out) return fail(nullptr, (f + "null argument").c_str());
    if (need_encoder && !w->has_encoder) return fail(nullptr, (f + "these weights have no encoder").c_str());
    if (n_streams < 1 || n_streams > POOL_SEG_MAX_STREAMS) return fail(nullptr, (f + "n_streams must be 1 .. " + max_name + " (64)").c_str());
    if (max_chunk_frames < 1 || max_chunk_frames > POOL_SEG_MAX_CHUNK) return fail(nullptr, (f + "max_chunk_frames must be 1 .. 64").c_str());
    if (const char* bad = config_error(cfg)) return fail(nullptr, bad);
    P* p = *pp = new P();
    p->cfg = *cfg; p->w = *w; p->n_streams = n_streams; p->max_chunk = max_chunk_frames;
    p->ring = cfg->tr_context + 2 * max_chunk_frames;        // a call's oldest key (offset - context + 1) and newest (offset + 2T - 1) never share a row
    p->offset.assign(n_streams, 0);
    return 0;
}

// distinct ids in range -> PoolIds (offsets filled by the caller): 0, or -1 and the pool's error under the caller's name
static int pool_ids(PoolBase* p, const char* who, const int32_t* streams, int n, PoolIds* ids) {
    if (!streams || n < 1 || n > p->n_streams) return fail(p, who, "stream list: need 1 .. n_streams ids");
    bool seen[MIMI_POOL_MAX_STREAMS] = {};
    for (int i = 0; i < n; ++i) {
        if (streams[i] < 0 || streams[i] >= p->n_streams) return fail(p, who, "stream id outside [0, n_streams)");
        if (seen[streams[i]]) return fail(p, who, "duplicate stream id in one call");
        seen[streams[i]] = true;
        ids->sid[i] = streams[i]; ids->off[i] = 0;
    }
    ids->n = n;
    return 0;
}

// The listed streams start afresh: their history rows -- and `tail`, an encode pool's [stream][tail_n] samples -- to zero in one launch, their
// token offsets to 0.  (The rings need no clearing: a window never starts before position 0, and every position is written before it is read.)
static int pool_reset(PoolBase* p, const char* who, const int32_t* streams, int n, float* tail, int tail_n, void* stream) {
    PoolIds ids;
    if (int rc = pool_ids(p, who, streams, n, &ids)) return rc;
    PoolRegions z = hist_regions(p->b, 0);
    if (tail) { z.base[z.count] = tail; z.hist[z.count] = tail_n; z.C[z.count] = 1; z.seg[z.count] = tail_n; z.T[z.count] = 0; ++z.count; }
    hipLaunchKernelGGL(k_pool_zero_hist, dim3(8, n, z.count), dim3(256), 0, (hipStream_t)stream, z, ids);
    MCHK(p, hipGetLastError());
    for (int i = 0; i < n; ++i) p->offset[streams[i]] = 0;
    return 0;
}

// ---- stream pool -----------------------------------------------------------------------------------------------------------------------
extern "C" int mimi_pool_create(const MimiConfig* cfg, const MimiWeights* w, int n_streams, int max_chunk_frames, mimi_pool* out) {
    MimiStreamPool* p = nullptr;
    if (int rc = pool_new("mimi_pool_create", "MIMI_POOL_MAX_STREAMS", false, cfg, w, out, n_streams, max_chunk_frames, &p)) return rc;
    auto alloc = [&]() {
        MCHK(p, hipMalloc((void**)&p->tab, (size_t)pool_tab_words(n_streams, max_chunk_frames) * 4));
        return ladder_alloc(p, p->b, *cfg, n_streams, max_chunk_frames, p->ring, cfg->tr_ffn);
    };
    if (const int rc = alloc()) { g_mimi_err = p->err; delete p; return rc; }
    *out = p;
    return 0;
}

extern "C" void mimi_pool_destroy(mimi_pool p) { delete p; }

extern "C" const char* mimi_pool_last_error(mimi_pool p) { return p ? p->err.c_str() : g_mimi_err.c_str(); }

extern "C" int mimi_pool_reset(mimi_pool p, const int32_t* streams, int n, void* stream) {
    if (!p) return fail(p, "mimi_pool_reset: null pool");
    return pool_reset(p, "mimi_pool_reset", streams, n, nullptr, 0, stream);
}

// The launch chain behind the call's first kernel, for both kinds of call.  The kernels take a UNIT and rows per unit: in a uniform call
// the unit is a listed stream (`units` = n streams of `per` = T frames each), in a ragged call (PRG) it is a FRAME of the call (`units` = F,
// `per` = 1) and the table says whose frame it is.  `n` streams slide.  Same launches, same grids per row, in the same order.
template <bool PRG>
static int pool_chain(MimiStreamPool* p, const int32_t* codes, long stride_s, long stride_k, long stride_t, float* pcm, int n, int units, int per,
                      hipStream_t st) {
    const MimiConfig& c = p->cfg;
    Ladder& b = p->b;
    const int d = c.hidden;
    const int T2 = 2 * per;
    const long M2 = (long)units * T2;
    const int* tab = p->tab;
    // RVQ lookup-sum + output projections -> rvq segments
    hipLaunchKernelGGL(k_pool_rvq<PRG>, dim3(units * per, (d + 63) / 64), dim3(256), (size_t)(2 * c.codebook_dim + c.n_codebooks) * 4, st, codes, stride_s,
                       stride_k, stride_t, per, c.n_codebooks, c.n_semantic, c.codebook_size, c.codebook_dim, d, p->w.codebooks, p->w.proj_first,
                       p->w.proj_rest, b.rvq.row0(), b.rvq.seg(), tab);
    // depthwise transposed conv x2 -> tok (dense)
    hipLaunchKernelGGL(k_pool_upsample<PRG>, dim3((unsigned)((M2 * d + 255) / 256)), dim3(256), 0, st, b.rvq.row0(), b.rvq.seg(), tab, per, units, d,
                       p->w.upsample, b.tok);
    MCHK(p, hipGetLastError());
    // transformer and SEANet decoder: every product as in a handle's decode_middle, over all the call's token rows
    TrPass tp{p->w.tr, M2};
    tp.tab = tab; tp.T2 = T2; tp.ring = p->ring; tp.ragged = PRG;
    if (int rc = transformer(p, c, p->w, b, tp, st)) return rc;
    if (int rc = seanet_decoder(p, p->w, c.n_stages, b, units, T2, tab, st, PRG)) return rc;
    // output convolution -> pcm, stream after stream, then every segmented buffer's history slides by its stream's chunk
    const SegBuf& last = b.xj(c.n_stages - 1);
    const long Tj = (long)per * last.rate;
    const MimiConv& co = p->w.conv_out;
    hipLaunchKernelGGL(k_pool_conv_out<PRG>, dim3((unsigned)((units * Tj + 255) / 256)), dim3(256), 0, st, last.row0(), last.seg(), tab, Tj, units, co.c_in,
                       co.taps, co.w, co.bias, pcm);
    return pool_slide<PRG>(p, b, per, n, tab, st);
}

extern "C" int mimi_pool_decode(mimi_pool p, const int32_t* streams, int n, const int32_t* codes, int T, long stride_s, long stride_k,
                                long stride_t, void* pcm_out, void* stream) {
    if (!p) return fail(p, "mimi_pool_decode: null pool");
    if (!codes || !pcm_out) return fail(p, "mimi_pool_decode: null codes or pcm");
    if (T < 1 || T > p->max_chunk) return fail(p, "mimi_pool_decode: T must be 1 .. max_chunk_frames given to mimi_pool_create");
    PoolIds ids;
    if (int rc = pool_ids(p, "mimi_pool_decode", streams, n, &ids)) return rc;
    for (int i = 0; i < n; ++i) {
        if (p->offset[ids.sid[i]] + 2L * T > 0x7fffffffL) return fail(p, "mimi_pool_decode: a stream passed 2^31 tokens; reset it");
        ids.off[i] = (int)p->offset[ids.sid[i]];
    }
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_pool_begin, dim3(1), dim3(256), 0, st, ids, p->tab, p->b.ksw.ticket, p->b.ksw.ticket ? p->b.ksw.n_tickets : 0);
    if (int rc = pool_chain<false>(p, codes, stride_s, stride_k, stride_t, (float*)pcm_out, n, n, T, st)) return rc;
    for (int i = 0; i < n; ++i) p->offset[ids.sid[i]] += 2 * T;
    return 0;
}

extern "C" int mimi_pool_decode_ragged(mimi_pool p, const int32_t* streams, const int32_t* frames, int n, const int32_t* codes, long stride_s,
                                       long stride_k, long stride_t, void* pcm_out, void* stream) {
    if (!p) return fail(p, "mimi_pool_decode_ragged: null pool");
    PoolSegHeader hdr;
    PoolSegs sg;
    if (const char* bad = pool_segs_build(streams, frames, n, codes, pcm_out, p->n_streams, p->max_chunk, p->offset.data(), &hdr, &sg))
        return fail(p, "mimi_pool_decode_ragged", bad);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_pool_begin_ragged, dim3(1), dim3(256), 0, st, hdr, p->tab, p->b.ksw.ticket, p->b.ksw.ticket ? p->b.ksw.n_tickets : 0);
    if (int rc = pool_chain<true>(p, codes, stride_s, stride_k, stride_t, (float*)pcm_out, n, sg.F, 1, st)) return rc;
    for (int i = 0; i < n; ++i) p->offset[hdr.sid[i]] += 2 * hdr.T[i];
    return 0;
}

// ---- encode stream pool (struct MimiEncStreamPool above) -----------------------------------------------------------------------------------
extern "C" int mimi_enc_pool_create(const MimiConfig* cfg, const MimiWeights* w, int n_streams, int max_chunk_frames, mimi_enc_pool* out) {
    MimiEncStreamPool* p = nullptr;
    if (int rc = pool_new("mimi_enc_pool_create", "MIMI_ENC_POOL_MAX_STREAMS", true, cfg, w, out, n_streams, max_chunk_frames, &p)) return rc;
    // the histories below are sized from the configuration: the weights must have its taps
    bool taps_ok = cfg->kernel >= 2 && cfg->codebook_dim % 32 == 0 && cfg->codebook_dim <= 2 * cfg->hidden && w->enc_conv_out.taps == cfg->last_kernel;
    for (int j = 0; j < cfg->n_stages; ++j)
        taps_ok = taps_ok && w->enc_res1[j].taps == cfg->res_kernel && w->enc_res2[j].taps == 1 && w->enc_down[j].taps == 2 * cfg->ratios[cfg->n_stages - 1 - j];
    if (!taps_ok) { delete p; return fail(nullptr, "mimi_enc_pool_create: encoder weights whose taps are not the configuration's (or codebook_dim % 32)"); }
    p->ended.assign(n_streams, 0);
    auto alloc = [&]() {
        MCHK(p, hipMalloc((void**)&p->tab, (size_t)ENC_STREAM_TAB_WORDS * 4 + (size_t)ENC_STREAM_LTAB_LONGS * 8));
        static_assert(ENC_STREAM_TAB_WORDS % 2 == 0, "the longs behind the table must be 8-byte aligned");
        p->ltab = reinterpret_cast<long*>(p->tab + ENC_STREAM_TAB_WORDS);
        const size_t tail_bytes = (size_t)n_streams * (cfg->kernel - 1) * 4;
        MCHK(p, hipMalloc((void**)&p->wav_tail, tail_bytes));
        MCHK(p, hipMemset(p->wav_tail, 0, tail_bytes));
        return ladder_alloc(p, p->b, *cfg, n_streams, max_chunk_frames, p->ring, enc_ffn_cols(*cfg), true);
    };
    if (const int rc = alloc()) { g_mimi_err = p->err; delete p; return rc; }
    *out = p;
    return 0;
}

extern "C" void mimi_enc_pool_destroy(mimi_enc_pool p) { delete p; }

extern "C" const char* mimi_enc_pool_last_error(mimi_enc_pool p) { return p ? p->err.c_str() : g_mimi_err.c_str(); }

extern "C" int mimi_enc_pool_reset(mimi_enc_pool p, const int32_t* streams, int n, void* stream) {
    if (!p) return fail(p, "mimi_enc_pool_reset: null pool");
    // every history row and the sample tail to zero: the whole-clip encode's left padding
    if (int rc = pool_reset(p, "mimi_enc_pool_reset", streams, n, p->wav_tail, p->cfg.kernel - 1, stream)) return rc;
    for (int i = 0; i < n; ++i) p->ended[streams[i]] = 0;
    return 0;
}

extern "C" int mimi_enc_pool_encode(mimi_enc_pool p, const int32_t* streams, const long* wav_off, const long* n_samples, int n, const float* wav,
                                    int32_t* codes, void* stream) {
    if (!p) return fail(p, "mimi_enc_pool_encode: null pool");
    const MimiConfig& c = p->cfg;
    const MimiWeights& w = p->w;
    EncStreamHeader hdr;
    EncStreamSegs sg;
    if (const char* bad = enc_stream_segs_build(streams, wav_off, n_samples, n, wav, codes, p->n_streams, p->max_chunk, p->offset.data(), p->ended.data(),
                                                c.ratios, c.n_stages, &hdr, &sg))
        return fail(p, "mimi_enc_pool_encode", bad);
    hipStream_t st = (hipStream_t)stream;
    Ladder& b = p->b;
    const int hop = (int)samples_per_frame(c), C = c.n_filters;
    EncPass ep{(long)sg.F * hop, sg.F}; ep.tab = p->tab; ep.ring = p->ring;
    hipLaunchKernelGGL(k_enc_stream_plan, dim3(1), dim3(256), 0, st, hdr, p->tab, p->ltab);
    // front: the first convolution into the streams' level-0 segments, then the sample tails move on
    const SegBuf& x0 = b.u(c.n_stages - 1);
    hipLaunchKernelGGL(k_enc_stream_conv_in, dim3((unsigned)((ep.rows0 * C + 255) / 256)), dim3(256), 0, st, wav, ep.rows0, hop, c.kernel, C, w.enc_conv_in_w,
                       w.enc_conv_in_b, p->tab, p->ltab, p->wav_tail, x0.row0(), x0.seg());
    hipLaunchKernelGGL(k_enc_stream_tail, dim3(1), dim3(256), 0, st, wav, n, c.kernel - 1, p->tab, p->ltab, p->wav_tail);
    MCHK(p, hipGetLastError());
    // every product runs over ALL the call's rows at its level, frame-aligned; the transformer on the streams' K/V rings -> a0 segments
    long L;
    if (int rc = seanet_encoder(p, c, w, b, ep, st, &L)) return rc;
    if (int rc = transformer(p, c, w, b, ep.tr(w, L), st)) return rc;
    if (int rc = encode_downsample(p, c, w, b, ep, L, st)) return rc;
    if (int rc = quantize(p, c, w, b, sg.F, codes, st)) return rc;
    // every buffer's history slides by its stream's chunk.  (A stream that ended slides rows nobody reads: its reset zeroes them.)
    if (int rc = pool_slide<true>(p, b, 1, n, p->tab, st)) return rc;
    for (int i = 0; i < n; ++i) { p->offset[hdr.sid[i]] += 2 * sg.T[i]; p->ended[hdr.sid[i]] = sg.ends[i]; }
    p->enc_rows = sg.F;
    return 0;
}

extern "C" int mimi_enc_pool_debug_latent(mimi_enc_pool p, float* out, long rows, void* stream) {
    if (!p) return fail(p, "mimi_enc_pool_debug_latent: null pool");
    return copy_encode_latent(p, "mimi_enc_pool_debug_latent", p->b.rvq.row0(), p->enc_rows, p->cfg.hidden, out, rows, stream);
}
