// The Whisper encoder's host plan (sesameai-tts_amd/csrc/whisper_enc_plan.h: no HIP) as a stand-alone host program, built under the host
// sanitizers by tests/test_whisper_enc_plan_host.py: every refusal of a config, the tile choice around the 256-workgroup threshold, the
// launch list of an encode (2 + 7 L + 1 launches, workgroup counts that cover M and N with their tails, K in whole 64-deep slices) for every
// Whisper size at batches 1 .. 64, and the plan's text.  Prints "ok".
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "whisper_enc_plan.h"

#define CHECK(c)                                                           \
    do {                                                                   \
        if (!(c)) { printf("line %d: %s\n", __LINE__, #c); exit(1); }      \
    } while (0)

static bool refused(WencDims c, int max_batch, const char* word) {
    const char* bad = wenc_dims_bad(c, max_batch);
    return bad && strstr(bad, word);
}

int main() {
    const WencDims tiny = {80, 384, 4, 6, 1536, 1500, 1e-5f};
    CHECK(!wenc_dims_bad(tiny, 1) && !wenc_dims_bad(tiny, 64));
    { WencDims c = tiny; c.n_mels = 64; CHECK(refused(c, 1, "n_mels")); c.n_mels = 128; CHECK(!wenc_dims_bad(c, 1)); }
    { WencDims c = tiny; c.H = 5; CHECK(refused(c, 1, "head dim")); c.H = 0; CHECK(refused(c, 1, "n_heads")); c.H = 21; c.d = 21 * 64; CHECK(refused(c, 1, "n_heads")); }
    { WencDims c = tiny; c.T = 1501; CHECK(refused(c, 1, "n_ctx")); c.T = 0; CHECK(refused(c, 1, "n_ctx")); c.T = 1; CHECK(!wenc_dims_bad(c, 1)); }
    { WencDims c = tiny; c.L = 0; CHECK(refused(c, 1, "n_layers")); c.L = 33; CHECK(refused(c, 1, "n_layers")); c.L = 32; CHECK(!wenc_dims_bad(c, 1)); }
    { WencDims c = tiny; c.ffn = 1500; CHECK(refused(c, 1, "ffn_dim")); c.ffn = 0; CHECK(refused(c, 1, "ffn_dim")); c.ffn = 8256; CHECK(refused(c, 1, "ffn_dim")); }
    { WencDims c = tiny; c.eps = 0.f; CHECK(refused(c, 1, "ln_eps")); c.eps = 1.f; CHECK(refused(c, 1, "ln_eps")); c.eps = nanf(""); CHECK(refused(c, 1, "ln_eps")); }
    CHECK(refused(tiny, 0, "max_batch") && refused(tiny, 65, "max_batch") && refused(tiny, -1, "max_batch"));

    CHECK(wenc_pad64(240) == 256 && wenc_pad64(384) == 384 && wenc_pad64(1) == 64);
    // 128-row tiles exactly where they still give each of the 256 CUs a workgroup
    CHECK(wenc_tile_rows(1500, 1024) == 64 && wenc_tile_rows(1500, 3072) == 128 && wenc_tile_rows(1500, 4096) == 128);
    CHECK(wenc_tile_rows(128 * 256, 128) == 128 && wenc_tile_rows(128 * 255, 128) == 64 && wenc_tile_rows(128 * 255 + 1, 128) == 128);
    CHECK(wenc_tile_rows(100, 128) == 64 && wenc_tile_rows(1, 1) == 64);

    const WencDims sizes[] = {tiny, {80, 128, 2, 2, 512, 100, 1e-5f}, {128, 192, 3, 3, 768, 100, 1e-5f}, {80, 768, 12, 12, 3072, 1500, 1e-5f},
                              {80, 1024, 24, 16, 4096, 1500, 1e-5f}, {128, 1280, 32, 20, 5120, 1500, 1e-5f}};
    static WencLaunch ls[3 + 7 * WENC_MAX_LAYERS];
    for (const WencDims& c : sizes) {
        CHECK(!wenc_dims_bad(c, WENC_MAX_BATCH));
        for (int b = 1; b <= WENC_MAX_BATCH; ++b) {
            const int n = wenc_plan(c, b, ls);
            CHECK(n == 3 + 7 * c.L && n <= (int)(sizeof ls / sizeof ls[0]));
            const long M = (long)b * c.T;
            CHECK(ls[0].kind == 0 && ls[0].M == 2 * M && ls[0].K == wenc_pad64(3 * c.n_mels) && ls[0].K >= 3 * c.n_mels);
            CHECK(ls[1].kind == 0 && ls[1].M == M && ls[1].K == 3 * c.d && c.d % 64 == 0);      // a 64-deep slice lies inside one tap
            CHECK(ls[n - 1].kind == 2 && ls[n - 1].M == M);
            int gemms = 0, rows = 0, attn = 0;
            for (int i = 0; i < n; ++i) {
                const WencLaunch& l = ls[i];
                CHECK(l.groups >= 1 && l.M >= 1);
                if (l.kind == 0) {
                    ++gemms;
                    CHECK(l.K % 64 == 0 && l.K >= 64 && (l.tile_rows == 64 || l.tile_rows == 128) && l.tile_rows == wenc_tile_rows(l.M, l.N));
                    const long mt = (l.M + l.tile_rows - 1) / l.tile_rows, nt = (l.N + 127) / 128;
                    CHECK(l.groups == mt * nt && mt * l.tile_rows >= l.M && (mt - 1) * l.tile_rows < l.M && nt * 128 >= l.N && mt <= 65535);
                } else if (l.kind == 1) {
                    ++attn;
                    const long qt = (c.T + WENC_QTILE - 1) / WENC_QTILE;
                    CHECK(l.groups == (long)b * c.H * qt && qt * WENC_QTILE >= c.T && l.K == c.T);
                } else {
                    ++rows;
                    CHECK(l.groups * 4 >= l.M && (l.groups - 1) * 4 < l.M && l.N == c.d && c.d <= 64 * WENC_MAX_HEADS);
                }
            }
            CHECK(gemms == 2 + 4 * c.L && attn == c.L && rows == 2 * c.L + 1);
            const std::string text = wenc_describe(c, b);
            CHECK(text.size() < 4096 && text.find("launches") != std::string::npos && text.find("q|k|v") != std::string::npos);
        }
    }
    printf("ok\n");
    return 0;
}
