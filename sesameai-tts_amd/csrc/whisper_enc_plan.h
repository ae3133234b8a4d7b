// The host side of the Whisper encoder (mimi_wenc_*, include/mimi_hip.h states the rule; tests/whisper_enc_ref.py in float64 torch): what a
// config may be, the tile shape of every GEMM launch, the launches of an encode in order and that plan as text.  Plain C++: no
// HIP, so the refusals cost no device call.
//
// Tiles.  A GEMM workgroup owns 128 columns and 128 or 64 rows.  The choice is a matter of filling 256 CUs and of nothing else: an output
// element's K chain is ONE accumulator walked over k ascending in both shapes, so its bits do not depend on the choice.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <string>

#define WENC_HEAD_DIM 64
#define WENC_MAX_LAYERS 32           // = MIMI_WENC_MAX_LAYERS
#define WENC_MAX_CTX 1500            // = MIMI_WENC_MAX_CTX
#define WENC_MAX_BATCH 64            // = MIMI_WENC_MAX_BATCH
#define WENC_MAX_HEADS 20            // d_model <= 1280: a LayerNorm row lives in one wave's registers, 20 values a lane
#define WENC_MAX_FFN 8192
#define WENC_CUS 256
#define WENC_QTILE 128               // queries of one attention workgroup: 4 waves of 32
#define WENC_F16_MAX 65504.0f

struct WencDims { int n_mels, d, L, H, ffn, T; float eps; };

static inline int wenc_pad64(int k) { return (k + 63) / 64 * 64; }

// nullptr, or why create refuses the config
static inline const char* wenc_dims_bad(const WencDims& c, int max_batch) {
    if (c.n_mels != 80 && c.n_mels != 128) return "dims: n_mels must be 80 or 128";
    if (c.H < 1 || c.H > WENC_MAX_HEADS) return "dims: n_heads outside 1 .. 20";
    if (c.d != c.H * WENC_HEAD_DIM) return "dims: head dim (d_model / n_heads) must be 64";
    if (c.L < 1 || c.L > WENC_MAX_LAYERS) return "dims: n_layers outside 1 .. 32";
    if (c.T < 1 || c.T > WENC_MAX_CTX) return "dims: n_ctx outside 1 .. 1500";
    if (c.ffn < 64 || c.ffn > WENC_MAX_FFN || c.ffn % 64 != 0) return "dims: ffn_dim must be a multiple of 64 in 64 .. 8192";
    if (!(c.eps > 0.0f) || !(c.eps < 1.0f)) return "dims: ln_eps outside (0, 1)";
    if (max_batch < 1 || max_batch > WENC_MAX_BATCH) return "max_batch outside 1 .. 64";
    return nullptr;
}

// rows of a GEMM workgroup's tile for an M x N launch: 128 where that still gives every CU a workgroup, else 64
static inline int wenc_tile_rows(long M, int N) {
    const long nt = (N + 127) / 128;
    return ((M + 127) / 128) * nt >= WENC_CUS ? 128 : 64;
}

struct WencLaunch { const char* name; int kind; long M; int N, K, tile_rows; long groups; };      // kind: 0 GEMM, 1 attention, 2 rows

// the launches of one encode of `batch` clips, in order; returns their number (n <= 3 + 7 L <= 227)
static inline int wenc_plan(const WencDims& c, int batch, WencLaunch* out) {
    int n = 0;
    const long M1 = (long)batch * 2 * c.T, M = (long)batch * c.T;
    auto gemm = [&](const char* name, long m, int N, int K) {
        const int tr = wenc_tile_rows(m, N);
        out[n++] = {name, 0, m, N, K, tr, ((m + tr - 1) / tr) * ((N + 127) / 128)};
    };
    auto rows = [&](const char* name) { out[n++] = {name, 2, M, c.d, 0, 0, (M + 3) / 4}; };
    gemm("conv1+gelu", M1, c.d, wenc_pad64(3 * c.n_mels));
    gemm("conv2+gelu+pos", M, c.d, 3 * c.d);
    for (int l = 0; l < c.L; ++l) {
        rows("ln1");
        gemm("q|k|v", M, 3 * c.d, c.d);
        out[n++] = {"attention", 1, M, c.d, c.T, WENC_QTILE, (long)batch * c.H * ((c.T + WENC_QTILE - 1) / WENC_QTILE)};
        gemm("out+resid", M, c.d, c.d);
        rows("ln2");
        gemm("fc1+gelu", M, c.ffn, c.d);
        gemm("fc2+resid", M, c.d, c.ffn);
    }
    rows("final ln");
    return n;
}

static inline std::string wenc_describe(const WencDims& c, int batch) {
    WencLaunch ls[3 + 7 * WENC_MAX_LAYERS];
    const int n = wenc_plan(c, batch, ls);
    char line[200];
    snprintf(line, sizeof line, "whisper encoder: n_mels %d, d %d, layers %d, heads %d, ffn %d, n_ctx %d, batch %d: %d launches\n", c.n_mels, c.d, c.L,
             c.H, c.ffn, c.T, batch, n);
    std::string s = line;
    for (int i = 0; i < n && i < 2 + 7; ++i) {           // the two convolutions and layer 0: every layer has the same plan
        const WencLaunch& l = ls[i];
        if (l.kind == 0)
            snprintf(line, sizeof line, "  %-15s gemm  M %6ld N %5d K %5d  tile %3dx128  %5ld workgroups\n", l.name, l.M, l.N, l.K, l.tile_rows, l.groups);
        else if (l.kind == 1)
            snprintf(line, sizeof line, "  %-15s flash rows %5ld keys %5d  %d queries a workgroup  %5ld workgroups\n", l.name, l.M, l.K, l.tile_rows, l.groups);
        else
            snprintf(line, sizeof line, "  %-15s rows  M %6ld d %5d  one wave a row  %5ld workgroups\n", l.name, l.M, l.N, l.groups);
        s += line;
    }
    snprintf(line, sizeof line, "  (layers 1 .. %d as layer 0)\n  %-15s rows  M %6ld d %5d\n", c.L - 1, ls[n - 1].name, ls[n - 1].M, ls[n - 1].N);
    s += line;
    return s;
}
