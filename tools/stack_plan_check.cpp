// Stand-alone host check of the launch plan of a transformer layer (sesameai-tts_amd/csrc/stack_plan.h): the public `kind` numbers of
// csm_op_gemv, and which kernel family / split / activation order the matrix-core and the GEMV path choose for a table of calls read off the
// code the header replaced.  The wide-M kernel families are bit-identical, so no parity test can see a changed selection: this can.
// No GPU, no HIP: build it with the host sanitizers and run it,
//   hipcc -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all -I sesameai-tts_amd/csrc tools/stack_plan_check.cpp -o /tmp/spcheck && /tmp/spcheck
// (or any C++17 compiler with -fsanitize=address,undefined -fno-sanitize-recover=all).  Exit status 0 and "ok" when every case behaves.
#include <cstdio>

#include "stack_plan.h"

static int failures = 0;
#define EXPECT(c)                                                               \
    do {                                                                        \
        if (!(c)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); ++failures; } \
    } while (0)

//                        d     nq    nkv  ffn   hd   H   KV cache  backbone
static const StackDims BB = {2048, 2048, 512, 8192, 64, 32, 8, 2048, true};
static const StackDims DEC = {1024, 1024, 256, 8192, 128, 8, 2, 32, false};
static const StackDims TINY = {512, 512, 128, 1024, 64, 8, 2, 64, true};

static PlanKnobs defaults() {
    PlanKnobs k = {};
    k.wide_path = 1; k.wide_min = 3; k.g128_min_rows = 256; k.mmt_min_rows = 64; k.mmt_ops = 6; k.slab_k = 256; k.part_rows = 32;
    k.xpack = k.xpack_prompt = k.fp8_wide = k.attn_merge = true;
    k.bb_block = k.bb_layer = true; k.bb_layer8 = true; k.fuse_dec_attn = true;
    return k;
}
static bool is(const Proj& p, Fam fam, int kg) { return p.fam == fam && p.kg == kg; }
// the six flags of a plan in the order of the table: big, quarter_slabs, f8, xp, xp0, mid
static bool flags(const WidePlan& p, bool big, bool quarter, bool f8, bool xp, bool xp0, bool mid) {
    return p.big == big && p.quarter_slabs == quarter && p.f8 == f8 && p.xp == xp && p.xp0 == xp0 && p.mid == mid;
}
// the four projections all on k_mm32, slabs of kg_o / kg_d
static bool all_mm32(const WidePlan& p, int kg_o, int kg_d) {
    return p.qkv == Fam::MM32 && p.gate_up == Fam::MM32 && is(p.o_proj, Fam::MM32, kg_o) && is(p.down, Fam::MM32, kg_d);
}
static bool all_g128(const WidePlan& p, int kg) { return p.qkv == Fam::G128 && p.gate_up == Fam::G128 && is(p.o_proj, Fam::G128, kg) && is(p.down, Fam::G128, kg) && p.stream == Stream::ROW_BF16; }

static void public_kinds() {
    static const struct { int kind; Fam fam; Op op; } want[16] = {
        {0, Fam::GEMV, Op::STORE}, {1, Fam::GEMV, Op::RESID}, {2, Fam::GEMV, Op::NORM_STORE}, {3, Fam::GEMV, Op::QKV}, {4, Fam::GEMV, Op::SWIGLU},
        {10, Fam::MM32, Op::STORE}, {11, Fam::MM32, Op::RESID}, {13, Fam::MM32, Op::QKV}, {14, Fam::MM32, Op::SWIGLU},
        {20, Fam::G128, Op::STORE}, {21, Fam::G128, Op::RESID}, {23, Fam::G128, Op::QKV}, {24, Fam::G128, Op::SWIGLU},
        {31, Fam::MMQ, Op::SLAB}, {33, Fam::MMT, Op::QKV}, {34, Fam::MMT, Op::SWIGLU}};
    int mapped = 0;
    for (int kind = -8; kind <= 64; ++kind) {
        const Fam f0 = Fam::G128; const Op o0 = Op::QKV_RAG;
        Fam fam = f0; Op op = o0;
        const bool ok = public_kind(kind, &fam, &op);
        bool listed = false;
        for (const auto& w : want)
            if (w.kind == kind) { listed = true; EXPECT(ok && fam == w.fam && op == w.op); }
        EXPECT(ok == listed);
        if (!ok) EXPECT(fam == f0 && op == o0);          // a refusal writes nothing
        mapped += ok;
    }
    EXPECT(mapped == 16);
}

static void wide_plans() {
    const PlanKnobs K = defaults();
    PlanKnobs k;
    WidePlan p;
    // batched backbone decode steps
    p = plan_wide(BB, K, 32, 1, false, false, false);
    EXPECT(flags(p, false, false, false, true, false, false) && all_mm32(p, 8, 8) && p.nsplit == 4 && p.merge_in_kernel && p.stream == Stream::PACK_BF16);
    k = K; k.attn_merge = false;
    p = plan_wide(BB, k, 32, 1, false, false, false);
    EXPECT(p.nsplit == 4 && !p.merge_in_kernel);
    p = plan_wide(BB, K, 8, 1, false, false, false);
    EXPECT(flags(p, false, false, false, false, false, false) && all_mm32(p, 8, 8) && p.nsplit == 8 && p.merge_in_kernel);
    p = plan_wide(BB, K, 23, 1, false, false, false);
    EXPECT(!p.xp && p.nsplit == 5);
    p = plan_wide(BB, K, 24, 1, false, false, false);
    EXPECT(p.xp && !p.xp0 && p.nsplit == 5);
    p = plan_wide(BB, K, 64, 1, false, false, false);
    EXPECT(flags(p, false, false, false, true, false, false) && all_mm32(p, 8, 8) && p.nsplit == 1 && !p.merge_in_kernel);
    k = K; k.part_rows = 64;
    p = plan_wide(BB, k, 64, 1, false, false, false);
    EXPECT(flags(p, false, false, false, true, false, false) && all_mm32(p, 8, 8) && p.nsplit == 2 && p.merge_in_kernel);
    k = K; k.slab_k = 1024;
    p = plan_wide(BB, k, 32, 1, false, false, false);
    EXPECT(all_mm32(p, 2, 8));
    // prompts below the k_mmt row count
    p = plan_wide(BB, K, 16, 16, true, false, false);
    EXPECT(flags(p, false, false, false, false, false, false) && all_mm32(p, 1, 1) && p.nsplit == 1);
    p = plan_wide(BB, K, 40, 40, true, false, false);
    EXPECT(flags(p, false, false, false, true, true, false) && all_mm32(p, 1, 1) && p.nsplit == 1);
    p = plan_wide(BB, K, 40, 40, true, true, false);
    EXPECT(p.xp && !p.xp0);                              // layer 0's input came normalised (row-major) from the caller
    k = K; k.xpack_prompt = false;
    p = plan_wide(BB, k, 40, 40, true, false, false);
    EXPECT(!p.xp && !p.xp0);
    p = plan_wide(BB, K, 63, 63, true, false, false);
    EXPECT(flags(p, false, false, false, true, true, false) && all_mm32(p, 1, 1));
    p = plan_wide(BB, K, 64, 64, true, false, false);
    EXPECT(flags(p, false, false, false, true, true, true));
    // 190 prompt rows: the measured default (gate/up and o-proj on the several-tiles-per-wave kernels)
    p = plan_wide(BB, K, 190, 190, true, false, false);
    EXPECT(flags(p, false, false, false, true, true, true) && p.qkv == Fam::MM32 && is(p.o_proj, Fam::MMQ, 4) && p.gate_up == Fam::MMT && is(p.down, Fam::MM32, 1) &&
           p.nsplit == 1 && p.stream == Stream::PACK_BF16);
    const WidePlan p190 = p;
    p = plan_wide(BB, K, 190, 190, true, false, true);   // e4m3 copies present: prompts keep the bf16 stream
    EXPECT(flags(p, false, false, false, true, true, true) && p.qkv == p190.qkv && p.gate_up == p190.gate_up && is(p.o_proj, p190.o_proj.fam, p190.o_proj.kg) &&
           is(p.down, p190.down.fam, p190.down.kg) && p.stream == Stream::PACK_BF16);
    k = K; k.mmt_ops = 15;
    p = plan_wide(BB, k, 190, 190, true, false, false);
    EXPECT(p.mid && p.qkv == Fam::MMT && is(p.o_proj, Fam::MMQ, 4) && p.gate_up == Fam::MMT && is(p.down, Fam::MMQ, 4));
    k = K; k.mmt_ops = 0;
    p = plan_wide(BB, k, 190, 190, true, false, false);
    EXPECT(p.mid && all_mm32(p, 1, 1));
    k = K; k.mmt_min_rows = 191;
    p = plan_wide(BB, k, 190, 190, true, false, false);
    EXPECT(!p.mid && all_mm32(p, 1, 1));
    p = plan_wide(BB, K, 380, 190, false, false, false);  // two sequences of 190 rows, not prompt mode: > 2 rows per sequence and >= 256 rows is long
    EXPECT(flags(p, true, true, false, false, false, false) && all_g128(p, 4));
    p = plan_wide(BB, K, 190, 190, false, false, false);  // not prompt mode, but > 2 rows per sequence: the prefill forms, split-K slabs as decode steps
    EXPECT(flags(p, false, false, false, true, true, true) && p.qkv == Fam::MM32 && is(p.o_proj, Fam::MMQ, 4) && p.gate_up == Fam::MMT && is(p.down, Fam::MM32, 8));
    k = K; k.g128_min_rows = 128;
    p = plan_wide(BB, k, 190, 190, true, false, false);
    EXPECT(flags(p, true, true, false, false, false, false) && all_g128(p, 4) && p.nsplit == 1);
    p = plan_wide(BB, K, 255, 255, true, false, false);
    EXPECT(flags(p, false, false, false, true, true, true));
    p = plan_wide(BB, K, 256, 256, true, false, false);
    EXPECT(flags(p, true, true, false, false, false, false) && all_g128(p, 4));
    // long prompts and batched prefill
    p = plan_wide(BB, K, 1334, 1334, true, false, false);
    EXPECT(flags(p, true, true, false, false, false, false) && all_g128(p, 4) && p.nsplit == 1 && !p.merge_in_kernel);
    p = plan_wide(BB, K, 3968, 3968, true, false, false);
    EXPECT(flags(p, true, true, false, false, false, false) && all_g128(p, 4));
    p = plan_wide(BB, K, 3969, 3969, true, false, false);
    EXPECT(flags(p, true, false, false, false, false, false) && all_g128(p, 0));    // residual epilogue + a norm launch
    p = plan_wide(BB, K, 6080, 190, false, false, false);
    EXPECT(flags(p, true, false, false, false, false, false) && all_g128(p, 0) && p.nsplit == 1);
    p = plan_wide(BB, K, 256, 1, false, false, false);    // decode steps never take them, whatever the batch
    EXPECT(flags(p, false, false, false, true, false, false) && all_mm32(p, 8, 8) && p.nsplit == 1);
    // fp8 mode
    p = plan_wide(BB, K, 32, 1, false, false, true);
    EXPECT(flags(p, false, false, true, true, false, false) && all_mm32(p, 8, 8) && p.nsplit == 4 && p.stream == Stream::PACK_E4M3);
    k = K; k.fp8_wide = false;
    p = plan_wide(BB, k, 32, 1, false, false, true);
    EXPECT(flags(p, false, false, false, true, false, false) && p.stream == Stream::PACK_BF16);
    k = K; k.xpack = false;
    p = plan_wide(BB, k, 32, 1, false, false, true);
    EXPECT(flags(p, false, false, true, false, false, false) && p.stream == Stream::PACK_E4M3);
    // depth decoder
    p = plan_wide(DEC, K, 32, 1, false, false, false);
    EXPECT(flags(p, false, false, false, true, false, false) && all_mm32(p, 4, 8) && p.nsplit == 1);
    p = plan_wide(DEC, K, 64, 2, false, false, false);
    EXPECT(flags(p, false, false, false, true, false, false) && all_mm32(p, 4, 8) && p.nsplit == 1);
    p = plan_wide(DEC, K, 32, 1, false, true, false);
    EXPECT(flags(p, false, false, false, true, false, false));
    // the tiny test model
    p = plan_wide(TINY, K, 190, 190, true, false, false);
    EXPECT(flags(p, false, false, false, true, true, false) && all_mm32(p, 1, 1) && p.nsplit == 1);      // K = 512 is no multiple of 1024: never mid
    p = plan_wide(TINY, K, 32, 1, false, false, false);
    // (8 key ranges, not the 4 of the issue's table: 1024 / (32 rows x 2 KV heads) = 16, clamped to BB_NSPLIT_MAX -- read off the replaced code)
    EXPECT(flags(p, false, false, false, true, false, false) && all_mm32(p, 2, 4) && p.nsplit == 8 && p.merge_in_kernel);
    EXPECT(qkv_op(false) == Op::QKV && qkv_op(true) == Op::QKV_RAG);      // a ragged group: the same plan, this op (and every row normed + take-last)
    // the path itself
    EXPECT(!stack_is_wide(K, 2, false) && stack_is_wide(K, 3, false) && stack_is_wide(K, 1, true));
    k = K; k.wide_path = 0;
    EXPECT(!stack_is_wide(k, 64, false) && !stack_is_wide(k, 64, true));
    k = K; k.wide_min = 5;
    EXPECT(!stack_is_wide(k, 4, false) && stack_is_wide(k, 5, false));
    EXPECT(slab_groups(100, false, 256) == 1 && slab_groups(8192, false, 256) == 8 && slab_groups(8192, true, 256) == 1);
    EXPECT(mmt_ok(64, 64, 1024, 64) && !mmt_ok(64, 257, 1024, 64) && !mmt_ok(64, 64, 512, 64) && !mmt_ok(64, 64, 1024, 96));
}

static void narrow_plans() {
    const PlanKnobs K = defaults();
    PlanKnobs k;
    NarrowPlan p;
    p = plan_narrow(BB, K, 1, false, true);
    EXPECT(p.layer == NarrowLayer::ONE_LAUNCH && p.stream == Stream::ROW_BF16);
    p = plan_narrow(BB, K, 1, false, false);                 // positions by constant: the all-CU launches read them per row
    EXPECT(p.layer == NarrowLayer::CHAIN);
    k = K; k.bb_layer = false;
    p = plan_narrow(BB, k, 1, false, true);
    EXPECT(p.layer == NarrowLayer::ATTN_BLOCK && p.stream == Stream::ROW_BF16);
    k = K; k.bb_block = false;                               // one-launch layer off: QKV, attention in 8 key ranges without a combine launch, COMBINE_RESID, SWIGLU, RESID
    p = plan_narrow(BB, k, 1, false, true);
    EXPECT(p.layer == NarrowLayer::CHAIN && p.nsplit == 8 && !p.fuse_attn && p.fuse_comb && p.stream == Stream::ROW_BF16);
    p = plan_narrow(BB, K, 2, false, true);
    EXPECT(p.layer == NarrowLayer::CHAIN && p.nsplit == 8 && !p.fuse_attn && p.fuse_comb);
    p = plan_narrow(DEC, K, 1, false, false);
    EXPECT(p.layer == NarrowLayer::CHAIN && p.nsplit == 1 && p.fuse_attn && !p.fuse_comb);
    p = plan_narrow(DEC, K, 2, false, false);
    EXPECT(p.layer == NarrowLayer::CHAIN && p.nsplit == 1 && p.fuse_attn && !p.fuse_comb);
    k = K; k.fuse_dec_attn = false;
    p = plan_narrow(DEC, k, 2, false, false);
    EXPECT(p.nsplit == 1 && !p.fuse_attn && !p.fuse_comb);   // an attention launch, then RESID
    StackDims long_dec = DEC; long_dec.cache_len = 33;
    EXPECT(!plan_narrow(long_dec, K, 1, false, false).fuse_attn);
    // e4m3 rows present: the e4m3 table throughout; the one-launch layer only in its e4m3 form
    p = plan_narrow(BB, K, 1, true, true);
    EXPECT(p.layer == NarrowLayer::ONE_LAUNCH && p.stream == Stream::ROW_E4M3);
    k = K; k.bb_layer = false;
    EXPECT(plan_narrow(BB, k, 1, true, true).layer == NarrowLayer::ONE_LAUNCH);
    k = K; k.bb_layer8 = false;
    p = plan_narrow(BB, k, 1, true, true);
    EXPECT(p.layer == NarrowLayer::CHAIN && p.stream == Stream::ROW_E4M3 && p.nsplit == 8 && p.fuse_comb);
    p = plan_narrow(DEC, K, 2, true, false);
    EXPECT(p.stream == Stream::ROW_E4M3 && p.fuse_attn);
    // heads
    EXPECT(plan_head(K, false, false, false) == Stream::ROW_BF16 && plan_head(K, false, true, true) == Stream::ROW_E4M3);
    EXPECT(plan_head(K, true, false, true) == Stream::PACK_BF16 && plan_head(K, true, true, true) == Stream::PACK_E4M3);
    k = K; k.fp8_wide = false;
    EXPECT(plan_head(k, true, true, true) == Stream::PACK_BF16 && plan_head(k, false, true, true) == Stream::ROW_E4M3);
    EXPECT(stream_e4m3(Stream::ROW_E4M3) && stream_e4m3(Stream::PACK_E4M3) && !stream_e4m3(Stream::ROW_BF16) && !stream_e4m3(Stream::PACK_BF16));
}

int main() {
    public_kinds();
    wide_plans();
    narrow_plans();
    if (failures) { std::fprintf(stderr, "%d failure(s)\n", failures); return 1; }
    std::puts("ok");
    return 0;
}
