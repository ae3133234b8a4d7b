// A keyed pool of watermark streams on the device (mimi_wm_pool_*, include/mimi_hip.h states the rule): every clip this build makes can carry
// a spread-spectrum mark, embedded per 1920-sample block in any number of live streams by ONE launch, and found again in a clip that was cut,
// padded, scaled or re-quantised by a search over the period's offsets.  Every decision is exact integer arithmetic (tests/watermark_ref.py
// states it in NumPy), so summation order is free and the device is held to the rule bit for bit.
//   k_wm_chips   once per pool: the key's P chips from Philox4x32-10 as +-1 int16 (210 KiB).
//   k_wm_embed   one workgroup per (stream, complete block) plus one per stream for its tail: E = sum q^2 and r = sum q c over the block, the
//                push D, and the block written out; the tail workgroup moves the open block's samples into the carry bank that the call did
//                not read, or, on `final`, writes them through unchanged.
//   k_wm_search  one workgroup per (clip, tile of 256 consecutive candidate offsets): the hot path, see below.
//   k_wm_pick    one workgroup per clip: first-index argmax over the clip's scores, then the winner's 56 R_k again, its payload and CRC.
// The plans (watermark_plan.h) travel in the kernel arguments: no host-to-device copy, no allocation, no synchronisation.
//
// Search.  Candidate i of a tile says "clip sample 0 is stream position o_0 + i", so its blocks start at first_0 - i + b S in the clip
// (first_0 = -o_0 mod S): consecutive candidates read windows that slide by ONE sample against the SAME chips, and all candidates of a tile
// agree on which symbol block b carries, ((o_0 + first_0) / S + b) mod K -- also those whose start has wrapped below 0 (their block 0 is
// not complete and is masked out, their block b is the real block b - 1 of the next symbol: the same one).  Per block the S + 255 samples
// [first_0 - 255 + b S, first_0 + (b + 1) S) are staged in LDS as int16 pairs, zero outside the clip.  Thread t scores the candidates that
// read at window offsets 2t and 2t + 1 with v_dot2 on the pairs: the even one reads the pairs as staged, the odd one the same pairs shifted
// by one sample, made in registers from two neighbouring words (alignbit by 16), as the stretch's and the VAD's searches do.  Lanes read
// consecutive words (no bank conflict); the chips' word is the same for all lanes (a scalar load).  The loop runs over the symbols k and
// inside over the blocks that carry k, so ONE 64-bit accumulator per candidate holds R_k and the score is counted as each k closes.
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include "../../include/mimi_hip.h"
#include "stream_pool.cuh"
#include "watermark_plan.h"

static_assert(MIMI_WM_MAX_STREAMS == WM_MAX_STREAMS && MIMI_WM_MAX_CLIPS == WM_MAX_CLIPS && MIMI_WM_ROW == WM_ROW, "header and plan disagree");
static_assert(MIMI_WM_S == WM_S && MIMI_WM_K == WM_K, "header and plan disagree");
static_assert(sizeof(WmSeg) == 56 && sizeof(WmPlan) <= 3600, "the plan must fit the kernel arguments");
static_assert(sizeof(WmClip) == 48 && sizeof(WmDetectPlan) <= 3600, "the plan must fit the kernel arguments");
static_assert(WM_P % 128 == 0 && WM_S % 2 == 0 && WM_TILE == 256, "k_wm_chips: 128 chips a thread; k_wm_search: 128 threads, two candidates each");

#define WM_THREADS 256                   // k_wm_embed, k_wm_pick
#define WM_ST (WM_TILE / 2)              // k_wm_search
#define WM_WIN (WM_S + WM_TILE)          // samples staged per block: 2176 (the last one is read by nobody)
#define WM_WORDS (WM_WIN / 2)            // 1088 int16 pairs

struct MimiWmPool : SpPool<WmStream> {
    uint64_t secret = 0;
    int16_t* chips_dev = nullptr;    // [WM_P] +-1
    uint32_t* carry_dev = nullptr;   // [n_streams][2 banks][WM_S] raw words: fp32 bits, or a sign-extended int16
};

// the clip's integer sample at position p, zero outside [0, N)
__device__ __forceinline__ int wm_q_at(const void* __restrict__ in, long in_off, int N, int i16, int p) {
    if (p < 0 || p >= N) return 0;
    return i16 ? (int)((const int16_t*)in)[in_off + p] : pcm_i16(((const float*)in)[in_off + p]);
}

__global__ void __launch_bounds__(64) k_wm_chips(uint2 key, int16_t* __restrict__ chips) {
    const int g = blockIdx.x * 64 + threadIdx.x;
    if (g >= WM_P / 128) return;
    const uint4 r = philox4x32(make_uint4((uint32_t)g, 0u, 0u, 0x574Du), key);
    const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int j = 0; j < 4; ++j)
        for (int b = 0; b < 32; ++b) chips[g * 128 + j * 32 + b] = (int16_t)(1 - 2 * (int)((w[j] >> b) & 1u));
}

__global__ void __launch_bounds__(WM_THREADS) k_wm_embed(const WmPlan plan, const int16_t* __restrict__ chips, uint32_t* __restrict__ carry,
                                                         const void* __restrict__ in, int i16, void* __restrict__ out) {
    __shared__ int red[4][3];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    // the segment that owns this workgroup: the last one whose g_off <= blockIdx.x (every segment owns at least its tail group)
    const WmSeg& g = plan.seg[sp_owner(plan.seg, plan.n, &WmSeg::g_off)];
    const int j = (int)blockIdx.x - g.g_off, sid = SP_SID(g), Lc = g.Lc, n_in = g.n_in, nb = g.nb;
    if (j > nb) return;                                                               // (never: every group below plan.groups lies in a segment)
    const uint32_t* old = carry + ((long)sid * 2 + SP_PARITY(g)) * WM_S;
    // raw word at position p of carry + chunk (p < Lc + n_in by construction of every use below)
    auto raw = [&](int p) -> uint32_t {
        if (p < Lc) return old[p];
        const long at = g.in_off + (p - Lc);
        return i16 ? (uint32_t)(int)((const int16_t*)in)[at] : ((const uint32_t*)in)[at];
    };
    if (j == nb) {                                                                    // the open block: fewer than S samples
        const int base = nb * WM_S, tl = Lc + n_in - base;
        uint32_t* nw = carry + ((long)sid * 2 + (SP_PARITY(g) ^ 1)) * WM_S;
        for (int p = t; p < tl; p += WM_THREADS) {
            const uint32_t v = raw(base + p);
            if (!SP_FINAL(g)) nw[p] = v;
            else if (i16) ((int16_t*)out)[g.out_off + base + p] = (int16_t)(int)v;
            else ((uint32_t*)out)[g.out_off + base + p] = v;
        }
        return;
    }
    const int base = j * WM_S, k = (g.k0 + j) % WM_K;
    const int bk = (g.bits >> k) & 1 ? 1 : -1;
    const int16_t* cp = chips + k * WM_S;
    uint32_t x[8];
    int q[8], c[8];
    unsigned long e = 0;
    int r = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int m = t + i * WM_THREADS;
        x[i] = 0; q[i] = 0; c[i] = 0;
        if (m < WM_S) {
            x[i] = raw(base + m);
            q[i] = i16 ? (int)x[i] : pcm_i16(__uint_as_float(x[i]));
            c[i] = cp[m];
            e += (unsigned long)(q[i] * q[i]);                                        // q^2 <= 2^30
            r += q[i] * c[i];
        }
    }
    // e <= 2^33 per thread: its low 15 bits and the rest are summed apart, each sum below 2^31 over the 256 threads
    const int wr = wave_sum_i(r), wlo = wave_sum_i((int)(e & 0x7FFF)), whi = wave_sum_i((int)(e >> 15));
    if (lane == 0) { red[w][0] = wr; red[w][1] = wlo; red[w][2] = whi; }
    __syncthreads();
    const long R = (long)red[0][0] + red[1][0] + red[2][0] + red[3][0];
    const unsigned long E = (((unsigned long)red[0][2] + red[1][2] + red[2][2] + red[3][2]) << 15) + ((unsigned long)red[0][1] + red[1][1] + red[2][1] + red[3][1]);
    unsigned long s = (unsigned long)sqrt((double)E);                                 // E < 2^41 is exact as a double: off by one at the most
    while (s * s > E) --s;
    while ((s + 1) * (s + 1) <= E) ++s;
    const long T = (long)(s * (unsigned long)g.t_q4) >> 4, u = bk * R;
    const long D = u >= T ? 0 : bk * (T - u);
    const long aD = D < 0 ? -D : D;
    const int a = (int)(aD / WM_S), rem = (int)(aD % WM_S), sg = D > 0 ? 1 : D < 0 ? -1 : 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int m = t + i * WM_THREADS;
        if (m < WM_S) {
            const int d = sg * c[i] * (a + (m < rem ? 1 : 0));
            if (i16) {
                ((int16_t*)out)[g.out_off + base + m] = (int16_t)min(max(q[i] + d, -32768), 32767);
            } else {
                const float xf = __uint_as_float(x[i]);
                // d * 2^-15 is exact (|d| < 2^17), so the sum is rounded once; an untouched or non-finite sample keeps its bits
                const bool touch = d != 0 && fabsf(xf) <= FLT_MAX;
                ((uint32_t*)out)[g.out_off + base + m] = touch ? __float_as_uint(xf + (float)d * 0x1p-15f) : x[i];
            }
        }
    }
}

__global__ void __launch_bounds__(WM_ST) k_wm_search(const WmDetectPlan plan, const uint32_t* __restrict__ chips2, const void* __restrict__ in,
                                                     int i16, int32_t* __restrict__ scores) {
    __shared__ uint32_t L[WM_WORDS];
    const int t = threadIdx.x;
    int lo = 0, hi = plan.n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (plan.clip[mid].t_off <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const WmClip& c = plan.clip[lo];
    const int i0 = ((int)blockIdx.x - c.t_off) * WM_TILE, N = c.n_in;
    if (i0 >= c.n_off) return;                                                        // (never)
    const int o_0 = (c.o0 + i0) % WM_P;
    const int first_0 = (WM_S - o_0 % WM_S) % WM_S;
    const int kbase = (o_0 + first_0) / WM_S % WM_K;
    const int nvb = N - first_0 + (WM_TILE - 1) >= 0 ? (N - first_0 + (WM_TILE - 1)) / WM_S : 0;      // blocks some candidate of the tile may own
    // this thread's candidates: window offset 2t is candidate 255 - 2t, offset 2t + 1 is candidate 254 - 2t; v = where its block 0 starts
    const int ca = WM_TILE - 1 - 2 * t, cb = ca - 1;
    const int va = first_0 - ca, vb = first_0 - cb;
    int score_a = 0, score_b = 0;
    for (int k = 0; k < WM_K; ++k) {
        long Ra = 0, Rb = 0;
        int cov_a = 0, cov_b = 0;
        for (int b = (k - kbase + WM_K) % WM_K; b < nvb; b += WM_K) {
            const int ws = first_0 - (WM_TILE - 1) + b * WM_S;                        // the window's first sample in the clip
            __syncthreads();                                                          // the block before has been read
            for (int wd = t; wd < WM_WORDS; wd += WM_ST) {
                const int s0 = wm_q_at(in, c.in_off, N, i16, ws + 2 * wd), s1 = wm_q_at(in, c.in_off, N, i16, ws + 2 * wd + 1);
                L[wd] = (uint32_t)(s0 & 0xFFFF) | ((uint32_t)s1 << 16);
            }
            __syncthreads();
            const uint32_t* __restrict__ cp = chips2 + k * (WM_S / 2);
            int ra = 0, rb = 0;
            uint32_t cur = L[t];
#pragma unroll 8
            for (int m = 0; m < WM_S / 2; ++m) {
                const uint32_t nxt = L[t + m + 1];                                    // t + m + 1 <= 127 + 960 < 1088
                const uint32_t cw = cp[m];
                const uint32_t odd = __builtin_amdgcn_alignbit(nxt, cur, 16);
                ra = dot2_i16(cur, cw, ra);
                rb = dot2_i16(odd, cw, rb);
                cur = nxt;
            }
            // a candidate owns the block if it lies in the clip whole
            if (va + b * WM_S >= 0 && va + (b + 1) * WM_S <= N) { Ra += ra; ++cov_a; }
            if (vb + b * WM_S >= 0 && vb + (b + 1) * WM_S <= N) { Rb += rb; ++cov_b; }
        }
        if ((c.mask >> k) & 1) {
            const bool one = (c.expect >> k) & 1;
            score_a += cov_a > 0 && (one ? Ra > 0 : Ra < 0);
            score_b += cov_b > 0 && (one ? Rb > 0 : Rb < 0);
        }
    }
    if (i0 + ca < c.n_off) scores[c.s_off + i0 + ca] = score_a;
    if (i0 + cb < c.n_off) scores[c.s_off + i0 + cb] = score_b;
}

__global__ void __launch_bounds__(WM_THREADS) k_wm_pick(const WmDetectPlan plan, const int16_t* __restrict__ chips, const void* __restrict__ in,
                                                        int i16, const int32_t* __restrict__ scores, long* __restrict__ out) {
    __shared__ int red[4];
    __shared__ unsigned long long R[WM_K];
    __shared__ int cov[WM_K];
    const WmClip& c = plan.clip[blockIdx.x];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, N = c.n_in;
    // the highest score, and among equals the smallest i: i < 2^21 rides in the key's low bits, inverted
    int key = -1;
    for (int i = t; i < c.n_off; i += WM_THREADS) key = max(key, scores[c.s_off + i] << 21 | (0x1FFFFF - i));
    const int wk = wave_max_i(key);
    if (lane == 0) red[w] = wk;
    if (t < WM_K) { R[t] = 0; cov[t] = 0; }
    __syncthreads();
    const int best = max(max(red[0], red[1]), max(red[2], red[3]));
    const int bi = 0x1FFFFF - (best & 0x1FFFFF);
    const int o = (c.o0 + bi) % WM_P, first = (WM_S - o % WM_S) % WM_S;
    const int nb = N >= first ? (N - first) / WM_S : 0, kb = (o + first) / WM_S % WM_K;
    for (int b = w; b < nb; b += 4) {
        const int k = (kb + b) % WM_K;
        int r = 0;
        for (int m = lane; m < WM_S; m += 64) r += wm_q_at(in, c.in_off, N, i16, first + b * WM_S + m) * chips[k * WM_S + m];
        r = wave_sum_i(r);
        if (lane == 0) { atomicAdd(&R[k], (unsigned long long)(long)r); atomicAdd(&cov[k], 1); }
    }
    __syncthreads();
    long* row = out + (long)blockIdx.x * WM_ROW;
    if (t < WM_K) row[8 + t] = (long)R[t];
    if (t == 0) {
        int score = 0, covered = 0;
        uint64_t bits = 0;
        bool decided = true;
        for (int k = 0; k < WM_K; ++k) {
            const long r = (long)R[k];
            if (r > 0) bits |= 1ULL << k;
            if (k >= 8 && (cov[k] == 0 || r == 0)) decided = false;
            if ((c.mask >> k) & 1 && cov[k] > 0) {
                ++covered;
                score += (c.expect >> k) & 1 ? r > 0 : r < 0;
            }
        }
        uint8_t byte[6];
        for (int j = 0; j < 6; ++j) {
            int v = 0;
            for (int i = 0; i < 8; ++i) v |= (int)((bits >> (8 * (j + 1) + i)) & 1) << (7 - i);
            byte[j] = (uint8_t)v;
        }
        long payload = 0;
        for (int j = 0; j < 5; ++j) payload = payload << 8 | byte[j];
        row[0] = bi; row[1] = o; row[2] = score; row[3] = covered; row[4] = nb; row[5] = payload;
        row[6] = decided && wm_crc8(byte, 5) == byte[5];
        row[7] = 0;
    }
}

extern "C" int mimi_wm_pool_create(int n_streams, uint64_t secret, mimi_wm_pool* out) {
    return sp_create("mimi_wm_pool_create", n_streams, out, nullptr, [&](MimiWmPool* p) {
        p->secret = secret;
        const uint8_t dflt[5] = {212, 211, 146, 56, 201};
        for (int i = 0; i < n_streams; ++i) { wm_fresh(p->st[i]); p->st[i].t_q4 = 8; p->st[i].bits = wm_symbol_bits(dflt); }
        hipError_t e = p->get(&p->chips_dev, sizeof(int16_t) * WM_P);
        if (e == hipSuccess) e = p->get(&p->carry_dev, sizeof(uint32_t) * 2 * WM_S * (size_t)n_streams, 0);
        if (e == hipSuccess) {
            k_wm_chips<<<dim3((WM_P / 128 + 63) / 64), dim3(64), 0, 0>>>(make_uint2((uint32_t)secret, (uint32_t)(secret >> 32)), p->chips_dev);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(0);                              // the table is there before any stream uses it
        return e;
    });
}

extern "C" void mimi_wm_pool_destroy(mimi_wm_pool p) { delete p; }

extern "C" const char* mimi_wm_pool_last_error(mimi_wm_pool p) { return sp_last_error(p); }

extern "C" int mimi_wm_pool_reset(mimi_wm_pool p, const int32_t* streams, const uint8_t* payloads, const int32_t* t_q4, int n) {
    return p ? sp_status(p, wm_reset(p->n_streams, p->st, streams, payloads, t_q4, n)) : -1;
}

extern "C" long mimi_wm_pool_out_count(mimi_wm_pool p, int sid, long n_in, int final) {
    return sp_count_ok(p, sid, n_in) ? wm_out_len(p->st[sid], n_in, final != 0) : -1;
}

extern "C" int mimi_wm_pool_feed(mimi_wm_pool p, const int32_t* streams, const long* in_off, const long* n_in, const int32_t* final, int n,
                                 const void* in, int in_is_i16, void* out, long* n_out, void* stream) {
    if (!p) return -1;
    WmPlan plan;
    WmStream next[SP_MAX_STREAMS];
    if (int rc = sp_status(p, wm_plan_build(p->n_streams, p->st, streams, in_off, n_in, final, n, in, in_is_i16, out, n_out, &plan, next))) return rc;
    (void)hipGetLastError();
    k_wm_embed<<<dim3((unsigned)plan.groups), dim3(WM_THREADS), 0, (hipStream_t)stream>>>(plan, p->chips_dev, p->carry_dev, in, in_is_i16, out);
    SP_HIP(p, hipGetLastError());
    sp_commit(p->st, streams, next, n);
    return 0;
}

extern "C" int mimi_wm_pool_detect(mimi_wm_pool p, const long* in_off, const long* n_in, const long* o0, const long* n_off,
                                   const uint64_t* expect, const uint64_t* mask, int n, const void* in, int in_is_i16, int32_t* scores,
                                   long* out, void* stream) {
    if (!p) return -1;
    WmDetectPlan plan;
    if (int rc = sp_status(p, wm_detect_plan(in_off, n_in, o0, n_off, expect, mask, n, in, in_is_i16, scores, out, &plan))) return rc;
    (void)hipGetLastError();
    k_wm_search<<<dim3((unsigned)plan.tiles), dim3(WM_ST), 0, (hipStream_t)stream>>>(plan, (const uint32_t*)p->chips_dev, in, in_is_i16, scores);
    SP_HIP(p, hipGetLastError());
    k_wm_pick<<<dim3((unsigned)plan.n), dim3(WM_THREADS), 0, (hipStream_t)stream>>>(plan, p->chips_dev, in, in_is_i16, scores, out);
    SP_HIP(p, hipGetLastError());
    return 0;
}
