// Which kernels one Llama stack call launches (csm_engine.hip run_stack): named ops, kernel families, weight streams, and the selection
// policy as pure functions of the stack's shape, the call's rows and the knobs -- computed ONCE per call.  Plain C++: no HIP and no getenv
// (switches.h reads the knobs where it always did; the engine passes them in), so the policy also compiles into a stand-alone host program
// (tools/stack_plan_check.cpp, run under the host sanitizers).  The wide-M families are bit-identical to one another by design, so no parity
// test can see a changed selection: that program is the policy's test.
#pragma once

#define BB_NSPLIT_MAX 8
#define PART_ROWS 32
#define WIDE_MIN_ROWS 3       // M >= this: MFMA path (mm.cuh) instead of the weight-stationary GEMV (measured: B=3 6.0 vs 6.5 ms, B=2 narrow wins)

// what a projection launch does around its GEMM: STORE = plain store, RESID = + residual, NORM_STORE = RMSNorm + store (heads), QKV = q|k|v +
// RoPE + KV append, SWIGLU = gate/up + SiLU*up, ATTN_RESID = fused depth-decoder attention + residual (hd 128, <= 32 keys), COMBINE_RESID =
// fused split-K attention merge + residual (hd 64), SLAB = fp32 K-split partials for a finisher, QKV_RAG = QKV of a ragged group (a.row_slot
// names each row's cache slot).  The narrow forms of QKV / SWIGLU apply the RMSNorm themselves; the wide ones read normalised rows.
enum class Op { STORE, RESID, NORM_STORE, QKV, SWIGLU, ATTN_RESID, COMBINE_RESID, SLAB, QKV_RAG };
// GEMV = k_gemv (weight-stationary rows), MM32 = k_mm32 (32-row tiles), MMT / MMQ = k_mmt / k_mmq (several tiles per wave, 64..256 prompt rows),
// G128 = k_gemm128 (LDS-tiled, long prompts)
enum class Fam { GEMV, MM32, MMT, MMQ, G128 };
// the four copies of a layer's matrices: row-major [N][K] or matrix-core operand order (k_pack_w / k_pack_w8), bf16 or OCP-e4m3 + per-row scales
enum class Stream { ROW_BF16, ROW_E4M3, PACK_BF16, PACK_E4M3 };
static inline bool stream_e4m3(Stream s) { return s == Stream::ROW_E4M3 || s == Stream::PACK_E4M3; }

// The public `kind` of csm_op_gemv (include/csm_hip_ops.h) -> family and op; false for every number that is not one of the sixteen
// {0..4, 10, 11, 13, 14, 20, 21, 23, 24, 31, 33, 34}.  31 = k_mmq's slabs (the hook runs the finisher after them).
static inline bool public_kind(int kind, Fam* fam, Op* op) {
    static const Op base[5] = {Op::STORE, Op::RESID, Op::NORM_STORE, Op::QKV, Op::SWIGLU};
    const int f = kind / 10, k = kind % 10;
    if (kind < 0 || f > 3 || k > 4 || (f > 0 && k == 2) || (f == 3 && k == 0)) return false;
    *fam = f == 0 ? Fam::GEMV : f == 1 ? Fam::MM32 : f == 2 ? Fam::G128 : k == 1 ? Fam::MMQ : Fam::MMT;
    *op = kind == 31 ? Op::SLAB : base[k];
    return true;
}

struct StackDims { int d, nq, nkv, ffn, hd, n_heads, n_kv_heads, cache_len; bool backbone; };
// every number and flag the selection reads, as the engine read them: at library load (g128_min_rows, mmt_min_rows, mmt_ops), at first use
// (slab_k), per handle in csm_create (the rest) or per call (the all-CU launches may have given up)
struct PlanKnobs {
    int wide_path, wide_min, g128_min_rows, mmt_min_rows, mmt_ops, slab_k, part_rows;
    bool xpack, xpack_prompt, fp8_wide, attn_merge;       // attn_merge: the arrival counters of the attention's in-kernel merge exist
    bool bb_block, bb_layer, bb_layer8, fuse_dec_attn;    // narrow path: all-CU backbone launches usable / + MLP / e4m3 form; attention fused into the decoder's o-proj
};
static inline bool stack_is_wide(const PlanKnobs& k, int M, bool force_wide) { return (M >= k.wide_min || force_wide) && k.wide_path; }

// prompts of 64..256 rows may take k_mmt / k_mmq: K/4 quarters in rings of up to 8 half-chunks
static inline bool mmt_ok(int min_rows, int M, int K, int N) { return M >= min_rows && M <= 256 && K % 1024 == 0 && N % 64 == 0; }
// residual projections of the wide path: fp32 partial tiles into the slab buffer, K split over `kg` blocks
static inline int slab_groups(int K, bool prompt, int slab_k) {
    // Prompt rows must not depend on how many rows share the call (prefix-KV reuse is bit-identical to a cold
    // prefill): no split there -- the four K quarters of a block's waves are the canonical summation order that
    // k_gemm128 reproduces for long prompts.
    if (prompt) return 1;
    // Decode steps (M <= a few row tiles): one block pulls its bytes through ONE CU at ~70 GB/s, so spread K over
    // up to 8 blocks of >= 256 k each (measured at M = 32: K 1024 -> kg 1/2/4 = 5.1/3.9/3.3 us, K 2048 N 2048 ->
    // kg 2/4/8 = 5.4/4.3/4.4 us; K 8192 -> 8 x 1024: blocks of 2048 or 4096 k are 3 % / 12 % slower end to end)
    const int kg = K / slab_k;
    return kg < 1 ? 1 : (kg > 8 ? 8 : kg);
}
static inline Op qkv_op(bool ragged) { return ragged ? Op::QKV_RAG : Op::QKV; }       // a ragged group changes this op and the last layer's tail, nothing of the plan
static inline int attn_splits(int budget, int M, int kv_heads) { const int ns = budget / (M * kv_heads); return ns < 1 ? 1 : (ns > BB_NSPLIT_MAX ? BB_NSPLIT_MAX : ns); }

// a residual projection (o-proj, down): kg >= 1 = fp32 slabs of K / kg each, then the finisher (h += sum of the slabs, next norm);
// kg == 0 = the kernel's own residual epilogue, then a norm launch
struct Proj { Fam fam; int kg; };
struct WidePlan {
    bool big, quarter_slabs, f8, xp, xp0, mid;
    Stream stream;
    Fam qkv, gate_up;
    Proj o_proj, down;
    int nsplit;                 // key ranges per (row, KV head) of the attention
    bool merge_in_kernel;       // ... merged by the last block to arrive (no k_attn_combine launch)
};
// The matrix-core path of M rows.  mmt_ops: which projections take k_mmt / k_mmq when `mid` (bit 0 q|k|v, 1 gate/up, 2 o-proj, 3 down).
// Measured per backbone layer at 190 rows, operand-order x, us: q|k|v 21.3 vs k_mm32 14.9 (96 fat blocks leave 160 CUs idle and a CU pulls
// only ~30 GB/s from HBM whatever the prefetch depth), gate/up 28.4 vs 41.6, o-proj 11.5 vs 13.0, down 37.4 vs 31.0 -> default 6: gate/up and o-proj
static inline WidePlan plan_wide(const StackDims& s, const PlanKnobs& k, int M, int rows_per_seq, bool prompt, bool x_normed, bool has_pk8) {
    WidePlan p = {};
    const bool prefill = prompt || rows_per_seq > 2;      // prompt mode or a plain multi-row prefill; never decode steps
    p.nsplit = 1;
    // 128 x 128 LDS-tiled kernels (same bits as the 32-row-tile kernels) for prefill from g128_min_rows rows (its measurement: where the engine reads
    // it); decode steps (<= 2 rows per sequence) stay on the 32-row-tile kernels with operand-order activations whatever the batch (B = 256: 13.7 vs 21 ms)
    p.big = M >= k.g128_min_rows && prefill;
    if (p.big) {
        // residual projections: d/128 column tiles only -- below ~2 tiles per CU split K into its four quarters over
        // blocks (fp32 slabs) and let the small path's finisher add them, the residual and the next norm
        p.quarter_slabs = (long)((M + 127) / 128) * ((s.d + 127) / 128) < 512 && s.d <= 2048;
        p.stream = Stream::ROW_BF16;
        p.qkv = p.gate_up = Fam::G128;
        p.o_proj = p.down = Proj{Fam::G128, p.quarter_slabs ? 4 : 0};
        return p;
    }
    // decode steps in fp8 mode stream the e4m3 copies (same values as the bf16 weights, which are their
    // dequantisation: identical bits, half the bytes); prompts keep the bf16 stream they share with k_gemm128
    p.f8 = has_pk8 && !prompt && k.fp8_wide;
    p.stream = p.f8 ? Stream::PACK_E4M3 : Stream::PACK_BF16;
    // decode steps keep their activations (xn, attention output, SiLU*up) in matrix-core operand order between
    // the kernels of a layer (common.cuh xp_off): producers write it, consumers read 1 KB pieces
    // (from 24 rows: a 1 KB piece always carries 32 rows, so for a few rows the row-major gather touches fewer lines:
    //  B=8 5.39 vs 5.52 ms packed, B=32 6.15 vs 6.01, B=64 7.42 vs 6.93, B=128 10.29 vs 9.07)
    const bool xp_decode = k.xpack && !prompt && rows_per_seq <= 2 && M >= 24 && (s.d == 512 || s.d == 1024 || s.d == 2048);
    // prompts below the LDS-tiled kernels' row count do the same (round 2): their projections were bound by exactly those
    // gathers (TA address cycles, 64 lines per fragment), not by bytes
    const bool xp_prompt = k.xpack_prompt && prefill && !p.f8 && M >= 24 && s.d % 64 == 0 && s.nq % 64 == 0 && s.ffn % 64 == 0 && s.d <= 2048;
    p.xp = xp_decode || xp_prompt;
    p.xp0 = xp_prompt && !x_normed;             // layer 0's normalised input is written by this call: operand order too (decode steps: it comes row-major)
    // prompts of 64..256 rows: the several-tiles-per-wave forms of k_mm32 (prompt mode: same bits; half the L2 traffic)
    p.mid = prefill && !p.f8 && mmt_ok(k.mmt_min_rows, M, s.d, s.nq + 2 * s.nkv) && mmt_ok(k.mmt_min_rows, M, s.nq, s.d) &&
            mmt_ok(k.mmt_min_rows, M, s.d, s.ffn) && mmt_ok(k.mmt_min_rows, M, s.ffn, s.d);
    p.qkv = p.mid && (k.mmt_ops & 1) ? Fam::MMT : Fam::MM32;
    p.gate_up = p.mid && (k.mmt_ops & 2) ? Fam::MMT : Fam::MM32;
    p.o_proj = p.mid && (k.mmt_ops & 4) ? Proj{Fam::MMQ, 4} : Proj{Fam::MM32, slab_groups(s.nq, prompt, k.slab_k)};
    p.down = p.mid && (k.mmt_ops & 8) ? Proj{Fam::MMQ, 4} : Proj{Fam::MM32, slab_groups(s.ffn, prompt, k.slab_k)};
    // batched backbone decode step (one row per sequence, long key ranges): a (row, KV head) block alone walks
    // its ~200+ keys in ~8 dependent round trips -- split the keys over up to 8 blocks like the B = 1 path
    if (!prompt && rows_per_seq == 1 && s.backbone && M <= k.part_rows) p.nsplit = attn_splits(1024, M, s.n_kv_heads);
    p.merge_in_kernel = p.nsplit > 1 && k.attn_merge;
    return p;
}

// The weight-stationary GEMV path (M below wide_min).  A backbone row alone may run a layer as ONE all-CU launch (bb_block.cuh k_bb_layer), or
// its attention block as one (k_bb_attn_block) in front of the gate/up and down GEMVs; everything else is the five-launch chain.
enum class NarrowLayer { ONE_LAUNCH, ATTN_BLOCK, CHAIN };
struct NarrowPlan {
    Stream stream;
    NarrowLayer layer;
    int nsplit;                 // chain: key ranges of the attention launch
    bool fuse_attn;             // chain: no attention launch, the o-proj computes it in its prologue (Op::ATTN_RESID)
    bool fuse_comb;             // chain: no k_attn_combine launch, the o-proj merges the key ranges (Op::COMBINE_RESID)
};
static inline NarrowPlan plan_narrow(const StackDims& s, const PlanKnobs& k, int M, bool e4m3_rows, bool per_row_pos) {
    NarrowPlan p = {};
    p.stream = e4m3_rows ? Stream::ROW_E4M3 : Stream::ROW_BF16;
    p.layer = NarrowLayer::CHAIN;
    if (s.backbone && M == 1 && k.bb_block && (!e4m3_rows || k.bb_layer8) && per_row_pos)
        p.layer = k.bb_layer || e4m3_rows ? NarrowLayer::ONE_LAUNCH : NarrowLayer::ATTN_BLOCK;
    p.nsplit = s.backbone && M <= PART_ROWS ? attn_splits(256, M, s.n_kv_heads) : 1;
    p.fuse_attn = s.hd == 128 && s.cache_len <= 32 && k.fuse_dec_attn && (s.n_heads / s.n_kv_heads) % 2 == 0;
    p.fuse_comb = !p.fuse_attn && p.nsplit > 1 && s.hd == 64;
    return p;
}

// the heads (c0 / audio): matrix-core rows take the packed copies, e4m3 when they exist and fp8_wide allows; the GEMV takes the model's rows
static inline Stream plan_head(const PlanKnobs& k, bool wide, bool pk8_heads, bool e4m3_rows) {
    if (wide) return pk8_heads && k.fp8_wide ? Stream::PACK_E4M3 : Stream::PACK_BF16;
    return e4m3_rows ? Stream::ROW_E4M3 : Stream::ROW_BF16;
}
