/*
 * libcsm_hip.so -- Mimi codec DECODE path (RVQ lookup + upsample + 8-layer transformer +
 * SEANet conv decoder), fp32, gfx950; below it the ENCODE path, and both as pools of stateful
 * streams (mimi_pool_*: decode, mimi_enc_pool_*: encode).
 *
 * Replaces `self._audio_tokenizer.decode(codes)` of the reference, i.e. moshi 0.2.2
 * `MimiModel.decode` as called at sesameai/generator.py:116 (stateless 10-frame stream
 * chunks), sesameai/generator.py:299 and tts_service.py:245 (whole utterance).
 * All pointers are device pointers unless stated; conv/linear weights are fp32 and already
 * re-laid-out by the loader (sesameai-tts_amd/sesameai/mimi.py) into the tap-major form the
 * kernels stream:  w[phase][tap][c_out][c_in].
 */
#ifndef MIMI_HIP_H
#define MIMI_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MIMI_MAX_TR_LAYERS 16
#define MIMI_MAX_STAGES     8

typedef struct MimiConfig {
    int32_t hidden;          /* 512  */
    int32_t codebook_size;   /* 2048 */
    int32_t codebook_dim;    /* 256  */
    int32_t n_codebooks;     /* 32   */
    int32_t n_semantic;      /* 1    */
    int32_t tr_layers, tr_heads, tr_ffn, tr_context;   /* 8, 8, 2048, 250 */
    float   rope_theta;      /* 10000 */
    float   norm_eps;        /* 1e-5  */
    int32_t n_stages;        /* 4 SEANet upsampling stages */
    int32_t ratios[MIMI_MAX_STAGES];   /* 8,6,5,4 */
    int32_t n_filters;       /* 64 */
    int32_t kernel, last_kernel, res_kernel;   /* 7, 3, 3 */
} MimiConfig;

/* one (possibly transposed) causal convolution in tap-major layout */
typedef struct MimiConv {
    const float* w;          /* [phases][taps][c_out][c_in]                            */
    const float* bias;       /* [c_out] or NULL                                        */
    int32_t c_in, c_out, taps, phases;
} MimiConv;

typedef struct MimiTrLayer {
    const float *ln1_w, *ln1_b, *in_proj /*[3d][d]*/, *out_proj /*[d][d]*/, *ls1 /*[d]*/;
    const float *ln2_w, *ln2_b, *lin1 /*[ffn][d]*/, *lin2 /*[d][ffn]*/, *ls2 /*[d]*/;
} MimiTrLayer;

typedef struct MimiWeights {
    const float* codebooks;  /* [n_codebooks][codebook_size][codebook_dim] = embedding_sum / clamp(usage,1e-5) */
    const float* proj_first; /* [codebook_dim][hidden]  rvq_first.output_proj, K-major    */
    const float* proj_rest;  /* [codebook_dim][hidden]  rvq_rest.output_proj,  K-major    */
    const float* rope_freqs; /* [head_dim/2] fp32: theta^(-2i/hd), built on the host       */
    const float* upsample;   /* [2 phases][2 taps][hidden] depthwise ConvTranspose1d k4 s2 */
    MimiTrLayer tr[MIMI_MAX_TR_LAYERS];
    MimiConv conv_in;
    MimiConv up[MIMI_MAX_STAGES];     /* ConvTranspose1d k=2r s=r: phases=r, taps=2     */
    MimiConv res1[MIMI_MAX_STAGES];   /* Conv1d k3  C -> C/2                             */
    MimiConv res2[MIMI_MAX_STAGES];   /* Conv1d k1  C/2 -> C                             */
    MimiConv conv_out;                /* Conv1d k3  n_filters -> 1                       */
    /* ---- ENCODE side (voice prompts, sesameai/generator.py:86); has_encoder == 0: absent ---- */
    int32_t has_encoder;
    const float* enc_conv_in_w;       /* [taps][n_filters]  (c_in = 1)                   */
    const float* enc_conv_in_b;       /* [n_filters]                                     */
    MimiConv enc_res1[MIMI_MAX_STAGES];   /* Conv1d k3  C -> C/2   (stage j works at C = n_filters << j) */
    MimiConv enc_res2[MIMI_MAX_STAGES];   /* Conv1d k1  C/2 -> C                         */
    MimiConv enc_down[MIMI_MAX_STAGES];   /* Conv1d k=2r stride r, C -> 2C, r = ratios reversed; taps = 2r */
    MimiConv enc_conv_out;            /* Conv1d k3  (n_filters << n_stages) -> hidden    */
    MimiTrLayer enc_tr[MIMI_MAX_TR_LAYERS];
    const float* downsample;          /* [4 taps][hidden][hidden] Conv1d k4 s2, replicate padding, no bias */
    const float* in_proj_first;       /* [codebook_dim][hidden]  rvq_first.input_proj    */
    const float* in_proj_rest;        /* [codebook_dim][hidden]  rvq_rest.input_proj     */
    const float* codebook_sqnorm;     /* [n_codebooks][codebook_size]  |e|^2             */
} MimiWeights;

typedef struct MimiDecoder* mimi_handle;

/* max_frames = longest code sequence one call (or one stream) will carry.
 * A handle's workspaces (activations, K-split partial tiles and their arrival tickets, the stream's history) are shared by all of its
 * calls: drive ONE HIP stream per handle at a time (a side-stream chunk decode and a whole-clip decode need two handles).            */
int  mimi_create(const MimiConfig* cfg, const MimiWeights* w, int max_frames, int reserved, mimi_handle* out);
void mimi_destroy(mimi_handle h);
const char* mimi_last_error(mimi_handle h);

/* codes: int32, element (b,k,t) at codes[b*stride_b + k*stride_k + t*stride_t] -- lets the
 * caller pass either a (B,32,T) tensor or the frame history [T][B][32] of csm_frames_dev()
 * without a transpose.  pcm: [B][hop*T] fp32.  stateful == 0: stateless decode of exactly
 * these T frames (what the reference does, whole utterance or per 10-frame chunk);
 * stateful != 0: continue the stream of the previous stateful call (B must be 1): conv left
 * contexts and the transformer KV window carry over, so chunked output == whole decode.
 * Codes >= codebook_size (CSM's vocab is 2051 > 2048) are clamped to codebook_size-1.
 * A stateless decode of T <= 32 frames (a streaming chunk) replays everything between the code
 * lookup and the output convolution from a hipGraph the handle captures at the second decode
 * of that T (kernel nodes only; MIMI_GRAPH_MAX_T=0 turns it off): same kernels, a quarter of
 * the host time per chunk.  One handle serves one thread at a time.                          */
int mimi_decode(mimi_handle h, const int32_t* codes, int B, int T, long stride_b, long stride_k,
                void* pcm, int stateful, void* stream);
/* stride_t is 1 for a (B,32,T) tensor; use mimi_decode_strided for other layouts. */
int mimi_decode_strided(mimi_handle h, const int32_t* codes, int B, int T, long stride_b, long stride_k,
                        long stride_t, void* pcm, int stateful, void* stream);
int mimi_reset_stream(mimi_handle h, void* stream);

/* MimiModel.encode (sesameai/generator.py:86): wav [B] rows of n_samples fp32 @ 24 kHz (row b at
 * wav + b*stride_b) -> codes [B][n_codebooks][T] int32, T = ceil(n_samples / hop).  Residual
 * vector quantisation = nearest centroid per level (first index on ties).  Uses the decoder's
 * work buffers: it ends any stateful decode stream.  n_samples <= hop * max_frames.
 * NON-FINITE AUDIO (a NaN or +-Inf sample) is not checked on the host -- that would synchronise -- and flows through as NaN: every op of
 * the chain is causal, so the frames that end before the bad sample keep their codes and their latent rows bit for bit; from the bad
 * sample's frame on the latent is NaN, no centroid is nearest, and every level's code is 0 (what an argmin over an all-NaN row gives);
 * the residual update subtracts centroid 0 and stays NaN.  A code written by any encode entry point is always inside
 * [0, codebook_size).  Nothing of it outlives the call: the handle's, and after mimi_enc_pool_reset the stream's, next results are those
 * of a fresh one, and the other clips of a mimi_encode_many call and the other streams of a pool call are untouched.                      */
int mimi_encode(mimi_handle h, const float* wav, long n_samples, long stride_b, int B, int32_t* codes, void* stream);

/* For tests: the pre-quantisation latent of the handle's LAST encode call ([rows][hidden] fp32, the stride-2 downsample's output that both
 * RVQ input projections read), copied device to device on `stream`; `rows` = that call's frames -- T of mimi_encode, where for B > 1 only the
 * LAST clip's latent is still there, or F of mimi_encode_many (clip i owns rows [F_i, F_i + T_i)).  Read only: no encode kernel changes for it.
 * Returns -1 with a message in mimi_last_error when `rows` is not the last encode call's frame count, when there was none, or when a decode
 * has since reused the buffer.                                                                                                            */
int mimi_debug_encode_latent(mimi_handle h, float* out, long rows, void* stream);

/* Several clips of DIFFERENT lengths through ONE launch chain (a request's context segments, a batch of voice prompts).
 * Clip i = n_samples[i] fp32 samples at wav + wav_off[i] (wav: device memory; wav_off, n_samples: host arrays, read before the call
 * returns).  With T_i = ceil(n_samples[i] / hop), F_i = T_0 + .. + T_(i-1) and F = sum T_i the output is codes[n_codebooks][F] int32
 * (device): clip i owns columns [F_i, F_i + T_i) of every level.  The clips' rows are stacked along the row axis of every product in
 * frame-aligned slots -- at a level with R rows per frame clip i owns rows [R * F_i, R * F_i + L_i), L_i <= R * T_i -- in the handle's
 * existing work buffers; the kernels that reach beyond their own row (the convolutions with taps or a stride, the q|k|v epilogue's RoPE
 * position, the attention window, the first convolution) find the row's clip in a small device table the chain's first kernel writes from
 * the kernel arguments: no host-to-device copy, no synchronisation.  No encode product takes a K split and every element's summation
 * order depends on the product's shape alone, so a clip's codes are, bit for bit, those of mimi_encode of that clip alone, whatever
 * shares the call and wherever the clip sits in the list.  Like mimi_encode it ends any stateful decode stream of the handle.
 * Returns -1 with a message in mimi_last_error, nothing enqueued and the handle still usable, for: n outside [1, MIMI_ENCODE_MAX_CLIPS],
 * an n_samples[i] < 1 (or a negative wav_off[i]), F > max_frames, a handle without encoder weights, a null pointer.                     */
#define MIMI_ENCODE_MAX_CLIPS 64
int mimi_encode_many(mimi_handle h, const float* wav, const long* wav_off, const long* n_samples, int n, int32_t* codes, void* stream);

/* ---- A pool of stateful decode streams decoded TOGETHER (many callers served from one batch of the frame loop) ----
 * A pool holds n_streams independent streams: per stream the left-context rows of every causal buffer, a per-layer K/V ring of
 * tr_context + 2 * max_chunk_frames tokens and its own token offset (RoPE position, window start).  A stream runs for any number of
 * frames: nothing in it grows with its length.  mimi_pool_decode takes a list of DISTINCT stream ids and the same T new frames for each
 * (1 <= T <= max_chunk_frames) and runs ONE launch chain for all of them: the streams' rows are stacked along the row axis of every
 * product, and each kernel maps a global row to (stream, local row) from a small device table, so that no tap and no attention window
 * reaches into a neighbour.  The K-split choice and every element's summation order depend on the product's shape alone -- a stream's PCM
 * does not depend on which other streams share the call or on its place in the list, and equals, bit for bit, what a single handle's
 * stateful mimi_decode gives for the same chunk schedule.
 * codes: element (i,k,t) at codes[i*stride_s + k*stride_k + t*stride_t], i = index in `streams` (a host array); codes >= codebook_size clamp
 * as in mimi_decode.  pcm: [n][hop*T] fp32 (device).  Each listed stream continues where its last call ended; mimi_pool_reset starts the
 * listed streams afresh.  Returns 0, or -1 (bad argument: a duplicate id, an id outside [0, n_streams), T > max_chunk_frames, ...) / -2 (HIP
 * error) with a message in mimi_pool_last_error; a refused call changes nothing.  Drive ONE HIP stream per pool at a time.
 * The weights are those of the MimiWeights given (device memory the caller keeps alive); a pool can share them with a mimi_handle.       */
#define MIMI_POOL_MAX_STREAMS 64
typedef struct MimiStreamPool* mimi_pool;
int  mimi_pool_create(const MimiConfig* cfg, const MimiWeights* w, int n_streams, int max_chunk_frames, mimi_pool* out);
void mimi_pool_destroy(mimi_pool p);
const char* mimi_pool_last_error(mimi_pool p);      /* p == NULL: why mimi_pool_create failed (this thread) */
int  mimi_pool_reset(mimi_pool p, const int32_t* streams, int n, void* stream);
int  mimi_pool_decode(mimi_pool p, const int32_t* streams, int n, const int32_t* codes, int T,
                      long stride_s, long stride_k, long stride_t, void* pcm, void* stream);

/* The same for streams with DIFFERENT numbers of new frames: stream streams[i] gets T_i = frames[i] frames (streams, frames: host arrays,
 * read before the call returns; 1 <= T_i <= max_chunk_frames), element (i,k,t) of codes at codes[i*stride_s + k*stride_k + t*stride_t] for
 * t < T_i.  With F_i = T_0 + .. + T_(i-1) and F = sum T_i the output is pcm[hop * F] fp32 (device): stream i owns samples
 * [hop * F_i, hop * (F_i + T_i)).  ONE launch chain of the length of mimi_pool_decode's, whatever the T_i are: the streams' rows are stacked
 * frame-aligned, as in mimi_encode_many -- at a level with R rows per frame (1 at the frames, 2 at the transformer's tokens, each SEANet
 * stage's rate above that) segment i owns dense rows [R * F_i, R * (F_i + T_i)); decode only up-samples, so there are no tails -- while the
 * buffers with history keep every stream in place, as for the uniform call.  The chain's first kernel expands a header of at most
 * MIMI_POOL_MAX_STREAMS entries {id, token offset, T_i} from the kernel arguments into the pool's device table ({id, offset, F_i, T_i} per
 * segment and the segment of every frame): no host-to-device copy, no synchronisation.  Each stream's history slides by ITS chunk and its
 * token offset advances by its own 2 * T_i.
 * NUMERICAL RULE: a stream's PCM from a ragged call is, bit for bit, what mimi_pool_decode gives that stream for the same chunk schedule --
 * and so, by the rule above, what a single handle's stateful mimi_decode and the whole-clip decode's stream give -- whatever shares the
 * call, whatever the others' T_j are and wherever the stream sits in the list: an MFMA output element depends on its own A rows, the wave
 * split and the K split depend on the product's shape (taps, C_in) alone, and everything else is per row or per sample.  (F <= n_streams *
 * max_chunk_frames, so every split product fits the workspace of the uniform call at T = max_chunk_frames.)
 * Returns -1 with a message in mimi_pool_last_error, nothing enqueued, no offset advanced and the pool still usable, for: n outside
 * [1, n_streams], a duplicate or out-of-range id, a frames[i] outside [1, max_chunk_frames], a null pointer, a stream that would pass
 * 2^31 tokens.                                                                                                                         */
int  mimi_pool_decode_ragged(mimi_pool p, const int32_t* streams, const int32_t* frames, int n, const int32_t* codes,
                             long stride_s, long stride_k, long stride_t, void* pcm, void* stream);

/* ---- A pool of stateful ENCODE streams fed TOGETHER (every microphone's new frames as they arrive, all conversations in one chain) ----
 * A pool holds n_streams independent encode streams: per stream the rows of left context in front of every convolution of the encoder (the
 * last kernel - 1 samples, res_kernel - 1 rows in front of each stage's residual convolution, r_j rows in front of its strided one, 2 in
 * front of the output convolution and of the downsample), a per-layer K/V ring of tr_context + 2 * max_chunk_frames tokens and its token
 * offset.  Nothing in a stream grows with its length.
 * mimi_enc_pool_encode: stream streams[i] gets n_samples[i] >= 1 new samples at wav + wav_off[i] (wav: device memory; streams, wav_off,
 * n_samples: host arrays, read before the call returns).  With T_i = ceil(n_samples[i] / hop) <= max_chunk_frames, F_i = T_0 + .. + T_(i-1)
 * and F = sum T_i the output is codes[n_codebooks][F] int32 (device): stream i owns columns [F_i, F_i + T_i).  ONE launch chain per call,
 * whatever n and the T_i are; the plan travels in the kernel arguments and the chain's first kernel expands it into the pool's device table
 * ({id, token offset, F_i, T_i, rows per level, first} per segment and the segment of every frame): no host-to-device copy, no
 * synchronisation.
 * A chunk whose n_samples[i] is NOT a multiple of hop ends its stream: its last frame follows the whole-clip rule (every level's length is the
 * rounded-up division chain of the chunk's own samples; zero padding behind the strided convolutions, replicate behind the downsample), and
 * the stream is refused until mimi_enc_pool_reset.  A stream that ends on a frame boundary is simply reset.
 * NUMERICAL RULE: a stream's columns, concatenated over its calls, are BIT FOR BIT mimi_encode of its concatenated samples -- for every chunk
 * schedule, every company in the call and every position in the list.  Every encode op is causal, its left padding is the history rows (zero
 * after a reset; the downsample replicates the first token at offset 0 and reads history afterwards), hop divides into every level's
 * stride, no product takes a K split, the wave split depends on (taps, C_in) alone and the attention walks its keys in chronological order.
 * Returns -1 with a message in mimi_enc_pool_last_error, nothing enqueued, no offset moved and the pool still usable, for: n outside
 * [1, n_streams], a duplicate or out-of-range id, an n_samples[i] < 1, a negative wav_off[i], T_i > max_chunk_frames, an ended stream, a null
 * pointer, a stream that would pass 2^31 tokens.  -2: a HIP error.  Drive ONE HIP stream per pool at a time.
 * The pool shares the caller's MimiWeights (device memory the caller keeps alive); creation is refused when has_encoder == 0.            */
#define MIMI_ENC_POOL_MAX_STREAMS 64
typedef struct MimiEncStreamPool* mimi_enc_pool;
int  mimi_enc_pool_create(const MimiConfig* cfg, const MimiWeights* w, int n_streams, int max_chunk_frames, mimi_enc_pool* out);
void mimi_enc_pool_destroy(mimi_enc_pool p);
const char* mimi_enc_pool_last_error(mimi_enc_pool p);   /* p == NULL: why mimi_enc_pool_create failed (this thread) */
int  mimi_enc_pool_reset(mimi_enc_pool p, const int32_t* streams, int n, void* stream);
int  mimi_enc_pool_encode(mimi_enc_pool p, const int32_t* streams, const long* wav_off, const long* n_samples, int n,
                          const float* wav, int32_t* codes, void* stream);
/* As mimi_debug_encode_latent, for the pool's last mimi_enc_pool_encode call: rows = its F, stream i of the call owns rows [F_i, F_i + T_i). */
int  mimi_enc_pool_debug_latent(mimi_enc_pool p, float* out, long rows, void* stream);

/* ---- A pool of stateful RESAMPLER streams (audio at any sample rate in front of the encoder and behind the decoder) ----
 * The filter is scipy.signal.resample_poly's default: g = gcd(src, dst), up = dst / g, down = src / g, half = 10 * max(up, down),
 * h = firwin(2 * half + 1, 1 / max(up, down), window = ('kaiser', 5.0)) * up, made once at create in float64 on the host, rounded once to fp32
 * and kept on the device.  A clip x[0 .. N) gives M = ceil(N * up / down) outputs
 *     y[n] = sum_k h[n * down + half - k * up] * x[k]     over the k with 0 <= n * down + half - k * up <= 2 * half and 0 <= k < N;
 * samples outside the clip are zero.  A pool holds n_streams independent streams.  After N samples in all a stream has emitted
 * floor((N * up - 1 - half) / down) + 1 outputs (0 while N * up - 1 - half < 0) while its clip is open, and ceil(N * up / down) once the clip is
 * ended (`final`); per stream the pool keeps the last 2 * half / up + 1 samples (two banks, flipped per call: a call's outputs read one, its
 * history update writes the other) and two running totals, reduced by whole periods (up outputs <-> down inputs) after every call -- a stream
 * runs for ever, and the kernel sees small numbers for ever.
 * mimi_rs_pool_feed: stream streams[i] gets n_in[i] >= 0 samples at in + in_off[i] ELEMENTS; final[i] != 0 ends its clip (the tail comes out
 * and the stream is left fresh; n_in[i] == 0 with final emits the tail alone).  in_fmt / out_fmt: 0 = fp32, 1 = int16 (in: x = s * 2^-15,
 * exact; out: clamp(y, -1, 1) * 32767 rounded to nearest even, NaN gives 0).  in, out: device memory; streams, in_off, n_in, final: host
 * arrays read before the call returns; n_out: a host array WRITTEN before the call returns.  Outputs are packed back to back: with
 * O_i = n_out[0] + .. + n_out[i - 1], stream i owns out[O_i .. O_i + n_out[i]); mimi_rs_pool_out_count says beforehand (host arithmetic only)
 * what a feed of n_in samples would give stream sid now.  A feed that emits nothing for a stream is legal.  ONE launch per call whatever n
 * and the lengths are; the plan (at most MIMI_RS_MAX_STREAMS entries) travels in the kernel arguments: no host-to-device copy, no
 * synchronisation.
 * NUMERICAL RULE: one output is one thread's sequential fp32 fmaf chain over its in-clip k in ascending order; nothing about it depends on
 * tiling, on the chunk schedule, on which other streams share the call or on list order -- a stream's outputs, concatenated over its calls,
 * are BIT FOR BIT the one-shot (single final feed) result of its concatenated samples.  In front of the clip's first sample the kernel
 * reads 0.0f by index rule, whatever the history memory holds: mimi_rs_pool_reset is host arithmetic, no launch.  A non-finite sample
 * reaches exactly the outputs whose tap range covers it: nothing in other streams, nothing after a reset or a `final`.
 * Returns -1 with a message in mimi_rs_pool_last_error, nothing enqueued and no state moved, for: src == dst, a rate <= 0, a reduced up or
 * down above 320 (create); n outside [1, n_streams], a duplicate or out-of-range id, a negative n_in or in_off, a null pointer, an unknown
 * format, a chunk that takes or gives more than 2^30 samples (feed).  -2: a HIP error.  Drive ONE HIP stream per pool at a time.          */
#define MIMI_RS_MAX_STREAMS 64
typedef struct MimiResamplePool* mimi_rs_pool;
int  mimi_rs_pool_create(int src_rate, int dst_rate, int n_streams, mimi_rs_pool* out);
void mimi_rs_pool_destroy(mimi_rs_pool p);
const char* mimi_rs_pool_last_error(mimi_rs_pool p);           /* p == NULL: why mimi_rs_pool_create failed (this thread) */
/* For tests: the fp32 taps the device holds (host_out: 2 * half + 1 floats, host memory, may be NULL) and the reduced factors. */
int  mimi_rs_pool_taps(mimi_rs_pool p, float* host_out, int* up, int* down, int* half);
long mimi_rs_pool_out_count(mimi_rs_pool p, int sid, long n_in, int final);
int  mimi_rs_pool_reset(mimi_rs_pool p, const int32_t* streams, int n);
int  mimi_rs_pool_feed(mimi_rs_pool p, const int32_t* streams, const long* in_off, const long* n_in, const int32_t* final, int n,
                       const void* in, int in_fmt, void* out, int out_fmt, long* n_out, void* stream);

/* ---- The segment finisher: decoded fp32 clips -> the int16 segments a WAV holds, every clip that is ready in ONE launch chain ----
 * What tts_service.TTS.generate_audio_segment does on the host per clip (peak-normalise, int16, lead and tail silence, fade in and out), as
 * the rule below.  One clip x[0 .. N), N >= 0, with lead L, tail T and fade F (samples, >= 0):
 *   1. peak = max(max |x_i| over the FINITE x_i, 1e-6f); an empty clip has the floor as its peak.
 *   2. q_i = trunc_toward_zero((x_i / peak) * 32767.0f), every operation rounded to fp32, `/` the correctly rounded IEEE division (not a
 *      multiply by a reciprocal).  A non-finite x_i (NaN, +-Inf) gives q_i = 0 and does not enter the peak.
 *   3. y = L zeros ++ q ++ T zeros; M = L + N + T.
 *   4. n = min(F, M / 2).  For n > 0 the ramp is made in float64: r_j = float(j * (1.0 / (n - 1))), r_(n-1) = 1, and r_0 = 0 when n == 1
 *      (numpy.linspace(0, 1, n, dtype=float32) bit for bit); y[j] = trunc(float(y[j]) * r_j) and y[M-n+j] = trunc(float(y[M-n+j]) * r_(n-1-j)).
 * mimi_fin_segments: segment i = n_in[i] fp32 samples at in[i] (in: a HOST array of DEVICE pointers, one per segment, so clips of separate
 * decode calls need no concatenation; in[i] may be NULL where n_in[i] == 0) with lead[i], tail[i], fade[i].  in, n_in, lead, tail, fade: host
 * arrays read before the call returns; out_off, n_out: host arrays WRITTEN before the call returns.  Outputs are packed back to back in `out`
 * (device, int16): with O_i = n_out[0] + .. + n_out[i-1] = out_off[i], segment i owns out[O_i .. O_i + n_out[i]), n_out[i] = M_i;
 * mimi_fin_out_count says beforehand (host arithmetic only) what a segment gives, or -1 for one the call would refuse.  A call is TWO launches
 * on `stream` whatever n and the lengths are (a partial peak per tile; then every output tile reduces its segment's partials and writes);
 * the plan (at most MIMI_FIN_MAX_SEGMENTS entries) travels in the kernel arguments: no memset, no atomics, no allocation, no host copy, no
 * synchronisation.  The handle's scratch for the partials (64 segments x 256 tiles, 64 KiB) is made ONCE at create and holds any legal call:
 * a segment's peak tile grows with its length so that it never has more than 256.
 * NUMERICAL RULE: an output depends on its own sample, its segment's peak and its index in the segment -- not on the tiling, not on which
 * segments share the call, not on list order: bit for bit the rule above.  A non-finite sample reaches nothing but its own output.
 * Returns -1 with a message in mimi_fin_last_error and nothing enqueued for: n outside [1, MIMI_FIN_MAX_SEGMENTS], a negative length, lead,
 * tail or fade, an M_i above 2^30, a null pointer (in[i] where n_in[i] > 0 included), a misaligned buffer.  -2: a HIP error.  Drive ONE HIP
 * stream per handle at a time.                                                                                                           */
#define MIMI_FIN_MAX_SEGMENTS 64
typedef struct MimiFinisher* mimi_finisher;
int  mimi_fin_create(mimi_finisher* out);
void mimi_fin_destroy(mimi_finisher p);
const char* mimi_fin_last_error(mimi_finisher p);              /* p == NULL: why mimi_fin_create failed (this thread) */
long mimi_fin_out_count(long n_in, long lead, long tail);
int  mimi_fin_segments(mimi_finisher p, const float* const* in, const long* n_in, const int32_t* lead, const int32_t* tail,
                       const int32_t* fade, int n, int16_t* out, long* out_off, long* n_out, void* stream);

/* ---- A pool of stateful TIME-STRETCH streams (speech rate without a change of pitch, behind the decoder) ----
 * WSOLA: overlap-add of 512-sample blocks, each joint placed where the waveforms agree.  Every decision is exact integer arithmetic, so the
 * device computes THE RULE below bit for bit.  Constants in samples: H = 512 (block and hop, 21.3 ms at 24 kHz), D = 256 (search radius).
 * Speed is an integer in permille, pm in [500, 2000] (1200 = 1.2 x faster).  For a clip x[0 .. N) of fp32:
 *   - x^[i] = x[i] for 0 <= i < N, else 0.0f (zero extension); q^ likewise.
 *   - search samples q[i] = clamp(rint(x[i] * 2048.0f), -2047, 2047), rint to nearest even, a non-finite x[i] gives 0.  12 bits on purpose:
 *     512 * 2047^2 = 2,145,387,008 < 2^31, so a whole score fits a signed 32-bit accumulator in any summation order.
 *   - M = (N * 1000 + pm - 1) / pm outputs y[0 .. M) in K = ceil(M / H) blocks, the last one cut at M.
 *   - block 0: c_0 = 0, y[j] = x^[j].
 *   - block k >= 1: a_k = (k * H * pm) / 1000 (64-bit integers), b_k = c_(k-1) + H (the natural continuation of what was last played),
 *     S_k(d) = sum over j < H of q^[a_k + d + j] * q^[b_k + j] for d = -D .. D, d_k = the SMALLEST d with the largest S_k, c_k = a_k + d_k,
 *     y[k H + j] = fl(fl(x^[c_k + j] * r_j) + fl(x^[b_k + j] * (1 - r_j))) with r_j = j / 512: two fp32 multiplies and one fp32 add, NOT fused.
 *   - a non-finite sample enters no decision (its q is 0) and appears in exactly the outputs mixed from it.
 * STREAMING: block k comes out once the stream has received R >= a_k + D + 2 H samples in all, or at `final`, when all remaining blocks up
 * to K come out and the stream is left fresh -- a function of k alone, so mimi_ts_pool_out_count is host arithmetic (latency: 1,280 samples).
 * A stream's outputs, concatenated over ANY chunk schedule, are bit for bit the one-shot result; they do not depend on which streams share
 * the call, on list order or on the stream id.  Per stream the device keeps the samples from a_(k'-1) - D on (k' the next block; fewer than
 * 2,560 floats, two banks flipped per call: a call reads one and writes the other) and c of the last block; the host keeps {pm, R, k, bank}.
 * A fresh stream reads neither, so mimi_ts_pool_reset (which also sets each listed stream's speed) is host arithmetic, no launch.  Streams of
 * a new pool are fresh at pm = 1000.
 * mimi_ts_pool_feed: stream streams[i] gets n_in[i] >= 0 fp32 samples at in + in_off[i] ELEMENTS; final[i] != 0 ends its clip.  in, out, d_out:
 * device memory; streams, in_off, n_in, final: host arrays read before the call returns; n_out: a host array WRITTEN before the call returns.
 * Outputs are packed back to back: stream i owns out[O_i .. O_i + n_out[i]), O_i = n_out[0] + .. + n_out[i-1].  d_out (may be NULL): d_k of
 * every emitted block (0 for block 0), packed the same way by blocks: stream i owns ceil(n_out[i] / H) entries after those of the streams
 * listed before it.  ONE launch per call, one workgroup per listed stream; the plan travels in the kernel arguments: no host-to-device copy,
 * no allocation, no synchronisation.
 * Returns -1 with a message in mimi_ts_pool_last_error, nothing enqueued and no state moved, for: n_streams outside [1, 64] (create); n
 * outside [1, n_streams], a duplicate or out-of-range id, a speed outside [500, 2000] (reset); a negative n_in or in_off, a null pointer, a
 * chunk that takes or gives more than 2^30 samples, a stream of more than 2^48 samples since its reset (feed).  -2: a HIP error.  Drive ONE
 * HIP stream per pool at a time.                                                                                                          */
#define MIMI_TS_MAX_STREAMS 64
typedef struct MimiStretchPool* mimi_ts_pool;
int  mimi_ts_pool_create(int n_streams, mimi_ts_pool* out);
void mimi_ts_pool_destroy(mimi_ts_pool p);
const char* mimi_ts_pool_last_error(mimi_ts_pool p);           /* p == NULL: why mimi_ts_pool_create failed (this thread) */
int  mimi_ts_pool_reset(mimi_ts_pool p, const int32_t* streams, const int32_t* speed_pm, int n);
long mimi_ts_pool_out_count(mimi_ts_pool p, int sid, long n_in, int final);
int  mimi_ts_pool_feed(mimi_ts_pool p, const int32_t* streams, const long* in_off, const long* n_in, const int32_t* final, int n,
                       const float* in, float* out, long* n_out, int32_t* d_out, void* stream);

/* ---- A pool of stateful VOICE-ACTIVITY streams (when a speaker starts and when they have stopped: reply on pause, barge-in) ----
 * Every decision is exact integer arithmetic, so the device computes THE RULE below bit for bit (tests/vad_ref.py states it in NumPy).
 * 24 kHz.  Constants in samples: F = 240 (frame, 10 ms), W = 480 (analysis window), lags TMIN = 60 .. TMAX = 400 (400 Hz .. 60 Hz).
 *   - samples: fp32 input s[i] = clamp(rint(x[i] * 32768.0f), -32768, 32767), rint to nearest even, a non-finite x[i] gives 0; int16 input
 *     s[i] = x[i]; s[i] = 0 for i < 0.  A clip of N samples has K = N / F frames; a trailing partial frame is never judged.
 * Frame k covers samples [k F, (k + 1) F).  Steps 1 to 5 depend on no other frame's result:
 *   1. power, DC-free: P_k = F * sum(s^2) - (sum s)^2 over the frame; 0 <= P_k < 2^46.
 *   2. search samples: m = max |s[i]| over the 880 samples [(k + 1) F - W - TMAX, (k + 1) F), sh = max(0, bitlen(m) - 10), q[i] = s[i] >> sh
 *      (arithmetic): |q| <= 1024, so a 480-term dot product fits a signed 32-bit accumulator in any order.
 *   3. for tau in TMIN .. TMAX, over i in [(k + 1) F - W, (k + 1) F): R(tau) = sum q[i] q[i - tau], E(tau) = sum q[i - tau]^2, E0 = sum q[i]^2.
 *   4. lag_k = the SMALLEST tau with R(tau) > 0 and 2 R(tau)^2 > E0 E(tau) (a normalised correlation above 0.707; both sides below 2^59),
 *      0 if none.  It is the FIRST lag that crosses the threshold: not the best lag, not a pitch estimate (a 220 Hz voice gives 103 .. 107
 *      where the best lag is 109).
 *   5. voiced_k = lag_k != 0 (silence is unvoiced: the inequality is strict).
 * The scan, per stream with parameters {on_q4, off_q4, min_on, hang, hold, n_min}, all in 64-bit integers:
 *   6. frame 0 first sets N = max(P_0, n_min) and has loud_0 = false; for k >= 1 loud_k = (16 P_k > N r), N the floor BEFORE this frame's
 *      update, r = off_q4 while in speech and on_q4 otherwise.
 *   7. since_voiced = 0 if voiced, else since_voiced + 1 (saturating at 2^20; a fresh stream starts saturated);
 *      active_k = loud_k and since_voiced <= hold.
 *   8. in silence: run = active ? run + 1 : 0; at run == min_on the state becomes speech, START is stamped at frame k - min_on + 1,
 *      run = quiet = 0.  In speech: quiet = active ? 0 : quiet + 1; at quiet == hang the state becomes silence, END is stamped at frame
 *      k - hang + 1, quiet = 0.
 *   9. after the test: if P_k < N then N -= (N - P_k) >> 2, else N += (N >> 9) + 1; then N = max(N, n_min).
 * Per frame the call writes flags (bit 0 loud, bit 1 voiced, bit 2 active, bit 3 in speech AFTER the frame), lag, power and floor (N after
 * the update).  Per stream the pool holds a summary of MIMI_VAD_SUMMARY int64, rewritten at the end of every call: in speech, frames
 * judged, frame of the last START (-1: none), frame of the last END (-1), the current quiet run, the numbers of STARTs and of ENDs, 0 --
 * counted since the stream was last fresh.  mimi_vad_pool_summary enqueues the copy of all n_streams rows to `out` (device memory, or
 * pinned host memory that the device can write); a stream that was reset and not fed since reads as the fresh summary.
 * STREAMING: a stream's per-frame outputs, concatenated over ANY chunk schedule, are bit for bit the one-shot result; they do not depend
 * on which streams share the call, on list order or on the stream id.  Per stream the device keeps the samples from k F - 640 on (k the
 * next unjudged frame; at most 879 int16, two banks flipped per call: a call reads one and writes the other) and {N, state, run, quiet,
 * since_voiced}; the host keeps the parameters, the counts {R, k} and the bank.  final[i] != 0 ends the stream's clip: a partial frame is
 * discarded and the stream is left fresh with the same parameters (its summary still describes the clip that ended, until the next call).
 * A fresh stream reads neither carry nor state, so mimi_vad_pool_reset (which also sets each listed stream's parameters) is host
 * arithmetic, no launch.  Streams of a new pool are fresh with the defaults {128, 48, 8, 70, 30, 3686400}.
 * mimi_vad_pool_feed: stream streams[i] gets n_in[i] >= 0 samples at in + in_off[i] ELEMENTS (in_is_i16: 0 = fp32, 1 = int16).  in, flags,
 * lag, power, floor: device memory; streams, in_off, n_in, final: host arrays read before the call returns; n_frames: a host array
 * WRITTEN before the call returns.  Per-frame outputs are packed back to back by frames: stream i owns entries [O_i, O_i + n_frames[i]),
 * O_i = n_frames[0] + .. + n_frames[i-1]; mimi_vad_pool_frame_count says beforehand (host arithmetic only) what a feed of n_in samples
 * would give stream sid now.  A feed that judges nothing for a stream is legal.  At most TWO launches per call whatever n and the lengths
 * are: one workgroup per (stream, frame) for steps 1 to 5, which writes power and lag, then one wave per stream for steps 6 to 9 and the
 * carry.  The plan travels in the kernel arguments: no host-to-device copy, no allocation, no synchronisation.
 * Returns -1 with a message in mimi_vad_pool_last_error, nothing enqueued and no state moved, for: n_streams outside [1, 64] (create); n
 * outside [1, n_streams], a duplicate or out-of-range id, a parameter outside 16 <= off_q4 <= on_q4 <= 4095, min_on 1 .. 1000, hang
 * 1 .. 10000, hold 0 .. 10000, n_min 1 .. 2^40 (reset); a negative n_in or in_off, a null pointer, a misaligned buffer, an unknown format,
 * a chunk of more than 2^30 samples, a stream of more than 2^48 samples since it was fresh (feed).  -2: a HIP error.  Drive ONE HIP stream
 * per pool at a time.                                                                                                                    */
#define MIMI_VAD_MAX_STREAMS 64
#define MIMI_VAD_SUMMARY 8
typedef struct MimiVadPool* mimi_vad_pool;
typedef struct { int32_t on_q4, off_q4, min_on, hang, hold, reserved; int64_t n_min; } mimi_vad_params;
int  mimi_vad_pool_create(int n_streams, mimi_vad_pool* out);
void mimi_vad_pool_destroy(mimi_vad_pool p);
const char* mimi_vad_pool_last_error(mimi_vad_pool p);         /* p == NULL: why mimi_vad_pool_create failed (this thread) */
int  mimi_vad_pool_reset(mimi_vad_pool p, const int32_t* streams, const mimi_vad_params* params, int n);
long mimi_vad_pool_frame_count(mimi_vad_pool p, int sid, long n_in, int final);
int  mimi_vad_pool_feed(mimi_vad_pool p, const int32_t* streams, const long* in_off, const long* n_in, const int32_t* final, int n,
                        const void* in, int in_is_i16, uint8_t* flags, int16_t* lag, long* power, long* floor, long* n_frames, void* stream);
int  mimi_vad_pool_summary(mimi_vad_pool p, long* out, void* stream);

/* ---- A keyed pool of WATERMARK streams (every clip marked on the device; the mark found again in a cut, padded, scaled clip) ----
 * This project's own keyed spread-spectrum mark with host-interference cancellation -- not silentcipher's, and not compatible with it.
 * Every decision is exact integer arithmetic, so the device computes THE RULE below bit for bit (tests/watermark_ref.py states it in NumPy).
 * 24 kHz.  Constants: S = 1920 samples per symbol (one Mimi frame, 80 ms), K = 56 symbols per period, P = S K = 107,520 samples (4.48 s).
 *   - samples: fp32 input q = clamp(rint(x * 32768.0f), -32768, 32767), rint to nearest even, a non-finite x gives q = 0; int16 input q = x.
 *   - symbols: a one bit is b = +1, a zero bit b = -1.  k = 0 .. 7: the sync byte 0xB2; k = 8 .. 47: the five payload bytes; k = 48 .. 55: the
 *     CRC-8 of the five bytes (polynomial 0x07, initial value 0); every byte MSB first.  As a word, bit k (LSB = symbol 0) holds symbol k.
 *   - chips from the pool's 64-bit secret: w = philox4x32_10(counter (p >> 7, 0, 0, 0x574D), key (secret_lo, secret_hi))[(p >> 5) & 3],
 *     c[p] = 1 - 2 * ((w >> (p & 31)) & 1) for p in [0, P).
 * EMBED, per stream: sample n (counted from the reset) lies in block J = n / S, which carries symbol k = J % K; its chip is c[n % P].  For
 * each COMPLETE block, sums over its S samples:
 *   1. E = sum q^2, r = sum q c, T = (isqrt(E) * t_q4) >> 4, u = b_k r.            (|r| <= 1920 * 32768 < 2^26; E <= 1920 * 2^30 < 2^41)
 *   2. u >= T: D = 0, the block already says its bit with margin and is untouched; otherwise D = b_k (T - u).
 *   3. a = |D| / S, rem = |D| % S; d[m] = sgn(D) c[m] (a + (m < rem)) for the block's sample m, so that sum d c == D exactly.
 *   4. fp32: y = x + float(d) * 2^-15 (one rounding) where d != 0 and x is finite, else y = x bit for bit; int16: y = clamp(q + d).
 * t_q4 in 1 .. 64 per stream (default 8: the block says its bit at no less than half a standard deviation of the host's own correlation; at
 * 0 a cancelled block would sum to exactly 0 and say nothing).  Digital silence stays digital silence; a NaN or Inf stays what it was.
 * STREAMING: a block comes out once it is complete, so a stream's output lags its input by fewer than S samples; final[i] != 0 writes the
 * open block through unchanged and leaves the stream fresh (same payload and t_q4).  A stream's outputs, concatenated over ANY chunk
 * schedule, are bit for bit the one-shot result; they do not depend on which streams share the call, on list order or on the stream id.
 * Per stream the device keeps the open block's samples (fewer than 1920 raw words, two banks flipped per call: a call reads one and writes
 * the other); the host keeps {samples taken, samples given, t_q4, the symbol bits, the format, the bank}.  mimi_wm_pool_reset (payloads: 5
 * bytes per listed stream) is host arithmetic, no launch.  Streams of a new pool are fresh with the payload {212, 211, 146, 56, 201}, t_q4 8.
 * mimi_wm_pool_feed: stream streams[i] gets n_in[i] >= 0 samples at in + in_off[i] ELEMENTS (in_is_i16: 0 = fp32, 1 = int16; out has the
 * format of in; a stream keeps one format between resets).  in, out: device memory; streams, in_off, n_in, final: host arrays read before
 * the call returns; n_out: a host array WRITTEN before the call returns.  Outputs are packed back to back: stream i owns
 * out[O_i .. O_i + n_out[i]), O_i = n_out[0] + .. + n_out[i-1]; mimi_wm_pool_out_count says beforehand what a feed would give.  ONE launch.
 * DETECT, per clip: candidate offset o in [0, P) says "clip sample 0 is stream position o".  With first = (-o) mod S the clip's complete
 * blocks start at first + i S; block i carries symbol k_i = ((o + first) / S + i) % K; r_i = sum_m q[first + i S + m] c[(o + first + i S + m) % P];
 * R_k = sum of the r_i with k_i = k (int64), cov_k their number.  With the caller's K-bit words expect and mask (bit k = symbol k):
 * score(o) = the number of k with the mask bit set, cov_k > 0 and sign(R_k) == b_k (R_k == 0 matches nothing); covered(o) = the number of k
 * with the mask bit set and cov_k > 0.  The candidates are (o0 + i) % P for i < n_off; the best is the highest score, on ties the smallest i.
 * All K mask bits: "verify this payload"; the 8 sync bits alone: "find any payload".  Per clip the call writes MIMI_WM_ROW int64: the best i,
 * its offset, its score, its covered count, the number of complete blocks, the decoded payload (bit = R_k > 0) as one 40-bit integer,
 * whether its CRC-8 holds (every symbol 8 .. 55 has cov_k > 0 and R_k != 0, and the decoded sixth byte is the CRC-8 of the five), 0,
 * R_0 .. R_55 of the best offset.  scores: device scratch of sum n_off int32 (every candidate's score, clip after clip).  TWO launches: one
 * workgroup per (clip, 256 consecutive candidates), then one per clip.
 * feed and detect allocate nothing, copy nothing from the host beyond the kernel arguments and never synchronise.
 * Returns -1 with a message in mimi_wm_pool_last_error, nothing enqueued and no state moved, for: n_streams outside [1, 64] (create); n
 * outside [1, n_streams], a duplicate or out-of-range id, t_q4 outside 1 .. 64 (reset); a negative n_in or in_off, a null pointer, a
 * misaligned buffer, an unknown format, a chunk of more than 2^30 samples, a stream of more than 2^48 samples since it was fresh, a stream
 * that changes format between resets (feed); more than 64 clips, a clip of more than 2^24 samples, a negative o0, n_off < 1, more than 2^21
 * candidates in a call, expect or mask bits beyond the 56 symbols (detect).  -2: a HIP error.  Drive ONE HIP stream per pool at a time.     */
#define MIMI_WM_MAX_STREAMS 64
#define MIMI_WM_MAX_CLIPS 64
#define MIMI_WM_S 1920
#define MIMI_WM_K 56
#define MIMI_WM_ROW 64
typedef struct MimiWmPool* mimi_wm_pool;
int  mimi_wm_pool_create(int n_streams, uint64_t secret, mimi_wm_pool* out);
void mimi_wm_pool_destroy(mimi_wm_pool p);
const char* mimi_wm_pool_last_error(mimi_wm_pool p);           /* p == NULL: why mimi_wm_pool_create failed (this thread) */
int  mimi_wm_pool_reset(mimi_wm_pool p, const int32_t* streams, const uint8_t* payloads, const int32_t* t_q4, int n);
long mimi_wm_pool_out_count(mimi_wm_pool p, int sid, long n_in, int final);
int  mimi_wm_pool_feed(mimi_wm_pool p, const int32_t* streams, const long* in_off, const long* n_in, const int32_t* final, int n,
                       const void* in, int in_is_i16, void* out, long* n_out, void* stream);
int  mimi_wm_pool_detect(mimi_wm_pool p, const long* in_off, const long* n_in, const long* o0, const long* n_off, const uint64_t* expect,
                         const uint64_t* mask, int n, const void* in, int in_is_i16, int32_t* scores, long* out, void* stream);

/* ---- A pool of LOUDNESS-METER streams, and the finisher that brings a clip to a stated loudness ----
 * ITU-R BS.1770-4 / EBU R 128 for one channel, made integer, so the device computes THE RULE below bit for bit (tests/loudness_ref.py
 * states it in NumPy).  24 kHz.  Constants in samples: T = 512 (taps), Q = 14, H = 2400 (hop, 100 ms).
 *   - samples: fp32 input s[i] = clamp(rint(x[i] * 32768.0f), -32768, 32767), rint to nearest even, a non-finite x[i] gives 0; int16 input
 *     s[i] = x[i]; s[i] = 0 for i < 0.
 *   1. K-weighting as an integer FIR: the two BS.1770 biquads (high shelf, RLB high-pass) re-derived for 24 kHz, their cascaded impulse
 *      response h cut at T taps, hq[j] = rint(h[j] * 2^Q) as int16 (tools/loudness_taps.py makes the table the library holds);
 *      z[i] = (sum over j < T of hq[j] s[i - j] + 2^(Q-1)) >> Q, an arithmetic shift.  sum |hq| * 32768 = 0.806 * 2^31: the sum fits a signed
 *      32-bit accumulator in any order, and |z| < 2^17.
 *   2. hop h covers samples [h H, (h + 1) H): e[h] = sum z^2 < 2^45.3, an exact integer.  A clip of N samples has N / H hops; a trailing
 *      partial hop has no energy, at `final` or ever.
 *   3. gating blocks of 400 ms with 75 % overlap: E[j] = e[j] + e[j+1] + e[j+2] + e[j+3] for every j whose four hops are HELD.  A stream
 *      holds its last `ring` hops (4096 unless create says otherwise: 409.6 s); the integrated value is the exact two-pass gating over what
 *      the ring holds, not an approximation of a longer programme.  Absolute gate: E[j] > 1208568 = floor(4 H 2^30 10^((-70 + 0.691) / 10)),
 *      which is -70 LUFS; S_abs, n_abs = sum and count of those blocks.  Relative gate, 10 LU under their mean, compared as integers:
 *      10 n_abs E[j] > S_abs (below 10 * 4096 * 2^47.3 < 2^63: this is why a ring holds at most 4096 hops).  S, n = sum and count of the
 *      blocks behind BOTH gates.  peak = max |s[i]| over every sample taken, a partial hop's included (0 .. 32768).
 *      The integrated loudness, for display, is -0.691 + 10 log10(S / (n * 4 H * 32768^2)) LUFS; n == 0 has none.
 * mimi_ld_pool_integrate writes MIMI_LD_ROW int64 per LISTED stream to `out` (device memory, row i for streams[i]): S, n, peak, hops, as of
 * the stream's last feed (a `final` feed included: the row still describes the clip that ended, until the stream is fed again); a stream
 * that was reset and not fed since gives zeros.  ONE launch, one wave per listed stream, no synchronisation: whatever reads `out` on the
 * same HIP stream -- mimi_fin_segments_ld -- sees it.
 * STREAMING: a stream's hop energies, concatenated over ANY chunk schedule, are bit for bit the one-shot result, and so is what integrate
 * gives; they do not depend on which streams share the call, on list order or on the stream id.  Per stream the device keeps the samples
 * from k H - 511 on (k the next unmeasured hop; at most 2910 int16, two banks flipped per call: a call reads one and writes the other),
 * the ring and {hops, peak}; the host keeps the counts {R, k} and the bank.  final[i] != 0 ends the stream's clip: a partial hop is
 * discarded and the stream is left fresh.  A fresh stream reads neither carry nor state, so mimi_ld_pool_reset is host arithmetic, no launch.
 * mimi_ld_pool_feed: stream streams[i] gets n_in[i] >= 0 samples at in + in_off[i] ELEMENTS (in_is_i16: 0 = fp32, 1 = int16).  in, energy:
 * device memory; streams, in_off, n_in, final: host arrays read before the call returns; n_hops: a host array WRITTEN before the call
 * returns.  The hop energies are packed back to back: stream i owns energy[O_i .. O_i + n_hops[i]), O_i = n_hops[0] + .. + n_hops[i-1];
 * mimi_ld_pool_hop_count says beforehand (host arithmetic only) what a feed of n_in samples would give stream sid now.  A feed that
 * completes no hop is legal.  At most TWO launches per call whatever n and the lengths are: one workgroup per (stream, hop) for steps 1 and
 * 2, then one wave per stream for the ring, the peak and the carry.  The plan travels in the kernel arguments: no host-to-device copy, no
 * allocation, no synchronisation.  (This feed meters and does not change a stream's samples; the leveler's feed is stated further down.)
 *
 * mimi_fin_segments_ld is mimi_fin_segments with a per-segment target: pt[i] (host) is P_T, the K-weighted mean square of the target in
 * int16 units, rint(2^30 10^((L + 0.691) / 10)) for L LUFS, or 0 for a segment that keeps the peak rule; ceiling[i] (host) is the sample
 * ceiling C in 1 .. 32767; meter: DEVICE memory, MIMI_LD_ROW int64 per segment, row i = what mimi_ld_pool_integrate gave for clip i.  For
 * a segment with pt[i] > 0 whose row has n > 0, steps 1 and 2 of the finishing rule become
 *     g = float(min(sqrt((double(P_T * 4 H) * double(n)) / double(S)), double(C) / double(peak))), every conversion and operation IEEE
 *     round-to-nearest in float64, then ONE rounding to fp32;  q_i = clamp(trunc(fl(fl(x_i * g) * 32767.0f)), -32767, 32767), 0 for a
 *     non-finite x_i;
 * lead, tail and fades as in mimi_fin_segments.  A segment with pt[i] == 0, or whose row has n == 0 (shorter than 400 ms, or nothing above
 * -70 LUFS), is bit for bit what mimi_fin_segments gives.  Same two launches, same refusals, and -1 also for: a null pt, ceiling or meter, a
 * misaligned meter, pt outside 0 .. 2^31, a ceiling outside 1 .. 32767.
 * Returns -1 with a message in mimi_ld_pool_last_error, nothing enqueued and no state moved, for: n_streams outside [1, 64], a ring
 * outside 4 .. 4096 and not 0 (create); n outside [1, n_streams], a duplicate or out-of-range id (reset, feed, integrate); a negative n_in
 * or in_off, a null pointer, a misaligned buffer, an unknown format, a chunk of more than 2^30 samples, a stream of more than 2^48 samples
 * since it was fresh (feed).  -2: a HIP error.  Drive ONE HIP stream per pool at a time.                                                  */
#define MIMI_LD_MAX_STREAMS 64
#define MIMI_LD_ROW 4
#define MIMI_LD_HOP 2400
typedef struct MimiLdPool* mimi_ld_pool;
int  mimi_ld_pool_create(int n_streams, int ring_hops, mimi_ld_pool* out);       /* ring_hops == 0: 4096 */
void mimi_ld_pool_destroy(mimi_ld_pool p);
const char* mimi_ld_pool_last_error(mimi_ld_pool p);           /* p == NULL: why mimi_ld_pool_create failed (this thread) */
int  mimi_ld_pool_reset(mimi_ld_pool p, const int32_t* streams, int n);
long mimi_ld_pool_hop_count(mimi_ld_pool p, int sid, long n_in, int final);
int  mimi_ld_pool_feed(mimi_ld_pool p, const int32_t* streams, const long* in_off, const long* n_in, const int32_t* final, int n,
                       const void* in, int in_is_i16, long* energy, long* n_hops, void* stream);
int  mimi_ld_pool_integrate(mimi_ld_pool p, const int32_t* streams, int n, long* out, void* stream);
int  mimi_fin_segments_ld(mimi_finisher p, const float* const* in, const long* n_in, const int32_t* lead, const int32_t* tail,
                          const int32_t* fade, const long* pt, const int32_t* ceiling, const long* meter, int n, int16_t* out, long* out_off,
                          long* n_out, void* stream);

/* ---- The pool's streams as LIVE LEVELERS: a causal gain that follows the gated loudness measured so far ----
 * n_out == n_in on every call and no sample is held back; exact integers plus a few spelled-out IEEE operations, so the device computes THE
 * RULE below bit for bit (tests/leveler_ref.py states it in NumPy).  Samples s, hop energies e[h] (H = 2400) and the gating are the meter's.
 * Per stream, set when the stream is made fresh: P_T, the target mean square (1 .. 2^31, as pt above); C, the ceiling (1 .. 32767);
 * g0, the start gain, Q16 (1 .. gmax); gmax, the largest gain, Q16 (1 .. 2^22); sh, the slew shift (1 .. 16: at most 1 / 2^sh per hop).
 *   1. pk[h] = max |s| over hop h; P[h] = max(pk[0 .. h]) since the stream was fresh (the ring does not limit it).
 *   2. boundary gains A[j], the gain at the start of hop j, Q16: A[0] = A[1] = g0, and for j >= 1, from hops <= j - 1 only -- so A[j + 1] is
 *      known before hop j's first sample arrives:  (S, n) = the two-pass gating over e[max(0, j - ring) .. j - 1];
 *      T = A[j] if n == 0, else int(min(double(gmax), trunc(sqrt((double(P_T * 4 H) * double(n)) / double(S)) * 65536.0))), every operation
 *      IEEE round-to-nearest in float64;  d = max(1, A[j] >> sh);  B = min(max(T, A[j] - d), A[j] + d);
 *      cap = (C << 16) / max(P[j - 1], 1), an integer division;  A[j + 1] = max(1, min(B, cap, gmax)).
 *   3. the sample at stream position r, j = r / H, i = r % H: gi = (A[j] (H - i) + A[j + 1] i) / H, an integer division in 64 bits.
 *   4. the output has the input's format.  int16: v = (s gi + 2^15) >> 16, y = clamp(v, -C, C).  fp32: y = fl(x * gf) with
 *      gf = float(gi) * 2^-16 (exact), then y > Cf -> Cf and y < -Cf -> -Cf with Cf = float(C) * 2^-15: a NaN stays a NaN, an infinite
 *      sample becomes +-Cf.  `clipped` counts the samples the clamp changed.
 *   5. final[i] != 0 ends the clip: a trailing partial hop is levelled like any other sample (its gains were known); the stream is then
 *      fresh with the same parameters.
 * A stream's outputs, gains and counters, concatenated over ANY chunk schedule, are the one-shot result, whatever the company in the call,
 * the list order and the stream id.  Known limits: there is no look-ahead (a sudden onset is clamped at C, not anticipated), and the cap
 * follows the all-time peak (one plosive holds the gain down for the rest of the clip).
 * mimi_ld_pool_level_reset: host arithmetic, no launch.  The listed streams are fresh, in LEVELER mode, with pt[i], ceiling[i], g0_q16[i],
 * gmax_q16[i], slew_shift[i] (host arrays).  A stream keeps one mode between resets: mimi_ld_pool_feed refuses a stream in leveler mode,
 * mimi_ld_pool_level_feed a metering one; mimi_ld_pool_reset returns a stream to metering.  mimi_ld_pool_hop_count and
 * mimi_ld_pool_integrate work on a leveler stream as on any other (they see its INPUT).
 * mimi_ld_pool_level_feed: arguments as mimi_ld_pool_feed, and: out, DEVICE memory in the format of `in` -- stream i's samples go to
 * out + in_off[i]; out == in is allowed, any other overlap is not; gain, int32 DEVICE memory: stream i owns n_hops[i] + 2 values, packed
 * back to back, A[k0] .. A[k0 + n_hops[i] + 1] for k0 hops measured before the call: the boundaries of every hop the call touches, the open
 * hop included.  At most THREE launches per call whatever n and the lengths are: the energies (and hop peaks), one wave per stream for
 * steps 1 and 2 with the meter's ring, state and carry, then the samples in 16 KiB tiles spread over the chip.  The plan travels in the
 * kernel arguments: no host-to-device copy, no allocation, no synchronisation.
 * mimi_ld_pool_level_state writes MIMI_LD_LEVEL_ROW int64 per LISTED stream to `out` (device memory): the gain the open hop ends on
 * (A[k + 1] for k measured hops), k, `clipped` since the stream was fresh, P[k - 1] (0 while k == 0).  ONE launch.  After `final` the row
 * still describes the clip that ended, until the stream is fed again; a stream reset and not fed since gives {g0, 0, 0, 0}.
 * Returns -1 with a message in mimi_ld_pool_last_error, nothing enqueued and no state moved, for everything mimi_ld_pool_reset / feed /
 * integrate refuse, and for: pt outside 1 .. 2^31, a ceiling outside 1 .. 32767, gmax outside 1 .. 2^22, g0 outside 1 .. gmax, a slew
 * shift outside 1 .. 16 (level_reset); a null or misaligned out or gain (level_feed); a stream in the wrong mode (feed, level_feed,
 * level_state).  -2: a HIP error.                                                                                                        */
#define MIMI_LD_LEVEL_ROW 4
int  mimi_ld_pool_level_reset(mimi_ld_pool p, const int32_t* streams, const long* pt, const int32_t* ceiling, const int32_t* g0_q16,
                              const int32_t* gmax_q16, const int32_t* slew_shift, int n);
int  mimi_ld_pool_level_feed(mimi_ld_pool p, const int32_t* streams, const long* in_off, const long* n_in, const int32_t* final, int n,
                             const void* in, int in_is_i16, void* out, long* energy, int32_t* gain, long* n_hops, void* stream);
int  mimi_ld_pool_level_state(mimi_ld_pool p, const int32_t* streams, int n, long* out, void* stream);

/* ---- A pool of LOOK-AHEAD PEAK-LIMITER streams (nothing above a ceiling, and no clipped waveform: behind the leveler, or alone) ----
 * A gain that starts to fall L samples AHEAD of a peak, is what the peak requires exactly on it, and recovers at a fixed step per sample.
 * Exact integers plus a few spelled-out IEEE operations, so the device computes THE RULE below bit for bit (tests/limiter_ref.py states it
 * in NumPy).  Sample peaks by default; a stream made fresh by mimi_lim_pool_reset_tp with its flag set detects TRUE PEAKS, 4x oversampled
 * (below).  One channel, one band.  ONE = 65536 is a gain of 1 in Q16.
 * Per stream, set when the stream is made fresh: C, the ceiling (1 .. 32767); L, the look-ahead in samples (1 .. 480); rho, the release
 * step in Q16 per sample (8 .. 65536; K = ceil(ONE / rho) <= 8192 samples from silence of gain back to 1); hr, the drive shift (0 .. 4):
 * the input is multiplied by exactly 2^hr in front of the limiter.  A stream is preceded and followed by silence: m[r] = ONE for r < 0 and
 * for r >= the clip's length.
 *   1. magnitude, an integer.  int16: a = |s 2^hr|.  fp32: t = fl(|x| * 2^(15 + hr)), an exact scaling; a = 0 for a NaN, a = 2^30 if
 *      t >= 2^30 (an infinite sample too), else a = int(ceil(t)).
 *   2. required gain, Q16: m[r] = ONE if a[r] <= C, else (C << 16) / a[r], an integer division.
 *   3. look-ahead minimum: w[r] = min(m[r .. r + L]), for r >= -L.
 *   4. release: e[r] = min(w[r], e[r - 1] + rho), e = ONE before r = -L; equivalently, and exactly,
 *      e[r] = min over j in [r - K, r] of (w[j] + (r - j) rho): terms further back cannot win because w <= ONE.
 *   5. attack smoothing: g[r] = (e[r - L] + .. + e[r]) / (L + 1), an integer division.  Every e[r - k] <= w[r - k] <= m[r], so g[r] <= m[r].
 *   6. the output has the input's format.  int16: y = (s 2^hr g + 2^15) >> 16, which cannot leave [-C, C].  fp32: y = fl(fl(x * 2^hr) * gf)
 *      with gf = float(g) * 2^-16 (exact), two multiplies, NOT fused; then y > Cf -> Cf and y < -Cf -> -Cf with Cf = float(C) * 2^-15.
 *      The clamp fires only where a = 2^30, an infinite or absurd sample; a NaN stays a NaN and moves no other sample.  (Where such a
 *      sample's own g is 0 -- only possible with C < 16384 -- inf * 0 is a NaN, by IEEE.)
 *   7. STREAMING: sample r comes out once the stream has received r + L + 1 samples, or at `final`: the latency is L samples.  With R
 *      received and E emitted after the call's n_in are counted, a call emits max(0, R - L) - E, or R - E at `final`, which then leaves the
 *      stream fresh with the same parameters; mimi_lim_pool_out_count is host arithmetic.  A stream's outputs, concatenated over ANY chunk
 *      schedule, are bit for bit the one-shot result; they do not depend on which streams share the call, on list order or on the stream id.
 *   8. the state row, MIMI_LIM_ROW int64 since the stream was fresh: the smallest g emitted (ONE while none), samples emitted, samples
 *      with g < ONE, samples the clamp changed.
 * Per stream the device keeps the required gains of its last K + 2 L positions and the at most L samples it holds (two banks flipped per
 * call: a call reads one and writes the other) and the row; the host keeps {R, E, bank, parameters}.  A fresh stream reads neither, so
 * mimi_lim_pool_reset is host arithmetic, no launch.  A stream must be reset once before it is fed: a new pool's streams have no parameters.
 * mimi_lim_pool_feed: stream streams[i] gets n_in[i] >= 0 samples at in + in_off[i] ELEMENTS; fmt: 0 = fp32, 1 = int16, one per call; a
 * stream that HOLDS samples takes only their format.  in, out: device memory in that format, which must not overlap; streams, in_off, n_in,
 * final: host arrays read before the call returns; n_out: a host array WRITTEN before the call returns.  Outputs are packed back to back:
 * stream i owns out[O_i .. O_i + n_out[i]), O_i = n_out[0] + .. + n_out[i-1].  At most TWO launches per call whatever n and the lengths
 * are: one workgroup per stream for the carry, then one per (stream, tile of 4096 outputs), which stages the tile's required gains with
 * their halo (L ahead, K + L behind) in LDS and runs steps 3 to 5 there as a doubling minimum and two workgroup scans -- no walk over a
 * clip; samples move as 16-byte vectors wherever a line lies wholly inside the chunk.  The plan travels in the kernel arguments: no
 * host-to-device copy, no allocation, no synchronisation.
 * mimi_lim_pool_state writes the row of every LISTED stream to `out` (device memory), as of the stream's last feed (a `final` feed
 * included: the row still describes the clip that ended, until the stream is fed again); a stream reset and not fed since gives
 * {ONE, 0, 0, 0}.  ONE launch.
 * Returns -1 with a message in mimi_lim_pool_last_error, nothing enqueued and no state moved, for: n_streams outside [1, 64] (create); n
 * outside [1, n_streams], a duplicate or out-of-range id (reset, feed, state); a ceiling outside 1 .. 32767, a look-ahead outside 1 .. 480,
 * a release step outside 8 .. 65536, a drive shift outside 0 .. 4 (reset); a negative n_in or in_off, a null pointer, a misaligned buffer,
 * an unknown format, a chunk that takes or gives more than 2^30 samples, a stream of more than 2^48 samples since it was fresh, a stream
 * without parameters, a stream that holds samples of the other format, in and out that overlap (feed).  -2: a HIP error.  Drive ONE HIP
 * stream per pool at a time.                                                                                                              */
#define MIMI_LIM_MAX_STREAMS 64
#define MIMI_LIM_ROW 4
typedef struct MimiLimPool* mimi_lim_pool;
int  mimi_lim_pool_create(int n_streams, mimi_lim_pool* out);
void mimi_lim_pool_destroy(mimi_lim_pool p);
const char* mimi_lim_pool_last_error(mimi_lim_pool p);         /* p == NULL: why mimi_lim_pool_create failed (this thread) */
int  mimi_lim_pool_reset(mimi_lim_pool p, const int32_t* streams, const int32_t* ceiling, const int32_t* lookahead, const int32_t* rho,
                         const int32_t* drive_shift, int n);
long mimi_lim_pool_out_count(mimi_lim_pool p, int sid, long n_in, int final);
int  mimi_lim_pool_feed(mimi_lim_pool p, const int32_t* streams, const long* in_off, const long* n_in, const int32_t* final, int n,
                        const void* in, void* out, long* n_out, int fmt, void* stream);
int  mimi_lim_pool_state(mimi_lim_pool p, const int32_t* streams, int n, long* out, void* stream);

/* ---- TRUE PEAKS: 4x oversampled detection for the limiter, and a stateless meter (tests/truepeak_ref.py states the rule in NumPy) ----
 * A 24 kHz waveform whose samples all lie under a ceiling can pass it between them, and a resampler behind the limiter makes those
 * inter-sample peaks real samples.  T = 8.  Three fractional phases p = 1, 2, 3 of 16 taps in Q14, H[p][k + 7] for k = -7 .. 8
 * (csrc/truepeak_taps.h; tools/truepeak_taps.py makes them: a 63-tap Kaiser windowed sinc); phase 0 is the sample itself.  Exact integers:
 *   a. signed sample v[r].  int16: s 2^hr.  fp32: sign(x) a[r] with a of step 1 above (a NaN: 0; |v| <= 2^30).  v = 0 outside the clip.
 *   b. interval i lies between samples i - 1 and i (i = 0 .. N): acc = sum over k of H[p][k + 7] v[i - 1 + k], in 64 bits
 *      (|acc| < 2^45); U[i][p] = (|acc| + 2^13) >> 14.
 *   c. a_tp[r] = max(a[r], U[r][1 .. 3], U[r + 1][1 .. 3]) < 2^31, for the samples of the clip.
 *   d. step 2 above reads a_tp in the place of a.  a_tp >= a, so the gain is never above the sample-peak gain and |y| <= C still holds
 *      exactly; the OUTPUT's own true peak can pass C by a little, because the gain moves between samples (docs/experiments/true_peak.md
 *      has the measured worst).  Steps 3 to 6 and the state row are unchanged.
 *   e. m[r] needs v up to r + T, so the latency is L + T: a call emits max(0, R - L - T) - E, or R - E at `final`.
 * mimi_lim_pool_reset_tp is mimi_lim_pool_reset with true_peak[i] = 0 or 1 per listed stream (all 0: the same call); every other entry
 * point keeps its signature.  A true-peak stream keeps, beside the required gains (of the K + 2 L positions in front of its last T), the
 * signed samples of its last 2 T positions and the at most L + T samples it holds.  A call may list streams of both modes: each mode
 * present takes its own two launches, outputs packed in list order as before.  Where every |v| a workgroup stages is below 2^15 the taps
 * run as int16 pairs into an int32 accumulator (it stays below 2^30), else in 64 bits: the integer is the rule's either way.
 * Additionally refused (-1): a flag that is neither 0 nor 1, a null true_peak.
 * mimi_tp_measure: a stateless meter with hr = 0.  Clip i is n_in[i] >= 0 samples at in + in_off[i] ELEMENTS (device memory; fmt as
 * above); in_off, n_in: host arrays of n <= MIMI_TP_MAX_CLIPS entries, read before the call returns.  out: device memory, MIMI_TP_ROW
 * int64 per clip: {sample peak max a, true peak max a_tp, the first r with a_tp[r] == true peak, n_in[i]}; an empty clip gives four
 * zeros.  One memset of the rows and ONE launch over (clip, tile of 4096 positions) workgroups; the maximum and its first position go
 * through one packed 64-bit atomicMax, so the row is exact in any order.  No host-to-device copy, no allocation, no synchronisation.
 * Returns -1 with a message in mimi_tp_last_error (this thread), nothing enqueued, for: a null pointer, an unknown format, a misaligned
 * buffer (out: 8 bytes), n outside [1, 64], a negative n_in or in_off, a clip of more than 2^30 samples.  -2: a HIP error.              */
#define MIMI_TP_MAX_CLIPS 64
#define MIMI_TP_ROW 4
int  mimi_lim_pool_reset_tp(mimi_lim_pool p, const int32_t* streams, const int32_t* ceiling, const int32_t* lookahead, const int32_t* rho,
                            const int32_t* drive_shift, const int32_t* true_peak, int n);
int  mimi_tp_measure(const void* in, const long* in_off, const long* n_in, int n, int fmt, long* out, void* stream);
const char* mimi_tp_last_error(void);

/* ---- WHISPER LOG-MEL STREAMS: the speech-to-text front end (tests/mel_ref.py states the rule in NumPy, float64) ----
 * Every Whisper-family recogniser takes a log-mel spectrogram of 30 s at 16 kHz, n_mels = 80 or 128 bands by 3000 frames.  It is a pure
 * function of the samples and causal but for a final clamp, so a stream computes it WHILE the turn is spoken.
 *   1. s: 480,000 samples, the clip's first min(L, 480000) and zeros behind them; int16 is x 2^-15, exact.  Samples past the cap are
 *      counted (the dropped count) and dropped, not refused.
 *   2. p: s reflected by 200 samples at both ends, p[j] = s[|j - 200|] on the left, mirrored about s[479999] on the right.
 *   3. frame t = 0 .. 2999 reads p[160 t .. 160 t + 399], times the PERIODIC Hann window w[n] = 0.5 - 0.5 cos(2 pi n / 400);
 *      P[k] = |DFT_400|^2, k = 0 .. 200; mel[m] = sum over k of F[k][m] P[k], F the Slaney-scale, Slaney-normalised triangular bank over
 *      0 .. 8000 Hz; raw[t][m] = log10(max(mel, 1e-10)).  A frame that reads only zeros is exactly -10.
 *   4. features[m][t] = (max(raw[t][m], M - 8) + 4) / 4 with M the largest raw value of all 3000 frames: the finisher's part.
 *   5. streaming: a frame is emitted once every sample it reads has been received or is known to be zero or reflected: with R samples in,
 *      frame 0 needs 201 and frame t >= 1 needs 160 t + 200; `final` or the cap settle the rest.  At `final` a clip of L samples has
 *      emitted min(3000, ceil((L + 200) / 160)) frames in all; the frames behind them are the constant -10 and are not written.
 * NUMERICAL RULE.  The DFT and the bank are fp32 matrix products on v_mfma_f32_32x32x2_f32 (exact fp32; no reduced-precision form exists
 * on gfx950 and bf16 would lose the bins 80 dB under a frame's strongest): every output is a k-ordered fp32 fmaf chain over the frame's own
 * 400 windowed samples, whichever frames share its tile.  So a stream's raw rows, concatenated over ANY chunk schedule, company, stream
 * id or list order, are bit for bit its one-shot rows.  A non-finite sample may make its own clip's features anything; it gives nothing
 * to other streams, to other clips of the call, or to the stream's next clip after `final` or a reset.
 * The pool builds its tables on the host in double and keeps them as fp32: window[400]; basis[400][MIMI_MEL_BASIS_COLS], the cos of bins
 * 0 .. 223 and then their -sin, zero from bin 201 on; bank[MIMI_MEL_BINS_PAD][MIMI_MEL_MAX_MELS], zero outside [201][n_mels].  The
 * call named ..._tables reads them back into host memory (it synchronises; for tests).
 * The feed: stream streams[i] gets n_in[i] >= 0 samples at 16 kHz at in + in_off[i] ELEMENTS; fmt: 0 = fp32, 1 = int16, one per
 * call (the carry is fp32: a stream may change format between calls).  The frames it completes come out as rows of n_mels fp32 in `raw`
 * (device memory, room for the sum of the frame counts), packed back to back in list order; n_frames[i] is written before the call
 * returns.  The host arrays are read before the call returns.  Per stream the device keeps the samples from the next unemitted frame's
 * first sample on, fewer than 400 fp32, in two banks flipped per call; the host keeps {R, frames, bank, dropped}.  `final` ends the clip
 * and leaves the stream fresh; the reset is host arithmetic with no launch, and a fresh stream reads no carry.  TWO launches per
 * call whatever n and the lengths are; no host-to-device copy, no allocation, no synchronisation.  The frame count and the dropped count
 * (samples past the cap since the stream was fresh) are host arithmetic; -1: ask the last error.
 * The finisher is stateless: clip i has n_frames[i] <= 3000 raw rows at raw + off[i] ELEMENTS (off, n_frames: host arrays of
 * n <= MIMI_MEL_MAX_CLIPS entries); out[i] is (n_mels, 3000) fp32, device memory.  M is taken over the clip's rows, and -10 if frames are
 * missing; the missing frames get the constant.  Two launches: a clip's M travels in the last two elements of its own output, which the
 * workgroup that finishes the clip last overwrites with their values; no workgroup waits for another.
 * Returns -1 with a message in the pool's last error (the finisher: mimi_mel_last_error, this thread), nothing enqueued and no state
 * moved, for: n_mels not 80 or 128, n_streams outside [1, 64] (create); n outside [1, n_streams], a stream id outside [0, n_streams) or
 * listed twice, a null pointer, an unknown format, a misaligned buffer, a negative n_in or in_off, a chunk of more than 2^30 samples;
 * the finisher: n outside [1, 64], n_frames outside [0, 3000], a negative off.  -2: a HIP error.                                       */
#define MIMI_MEL_MAX_STREAMS 64
#define MIMI_MEL_MAX_CLIPS 64
#define MIMI_MEL_CAP 480000
#define MIMI_MEL_FRAMES 3000
#define MIMI_MEL_BINS_PAD 224
#define MIMI_MEL_BASIS_COLS 448
#define MIMI_MEL_MAX_MELS 128
typedef struct MimiMelPool* mimi_mel_pool;
int  mimi_mel_pool_create(int n_mels, int n_streams, mimi_mel_pool* out);
void mimi_mel_pool_destroy(mimi_mel_pool p);
const char* mimi_mel_pool_last_error(mimi_mel_pool p);         /* p == NULL: why mimi_mel_pool_create failed (this thread) */
int  mimi_mel_pool_reset(mimi_mel_pool p, const int32_t* streams, int n);
int  mimi_mel_pool_tables(mimi_mel_pool p, float* window, float* basis, float* bank);
long mimi_mel_pool_frame_count(mimi_mel_pool p, int sid, long n_in, int final);
long mimi_mel_pool_dropped(mimi_mel_pool p, int sid);
int  mimi_mel_pool_feed(mimi_mel_pool p, const int32_t* streams, const long* in_off, const long* n_in, const int32_t* final, int n,
                        const void* in, int fmt, float* raw, long* n_frames, void* stream);
int  mimi_mel_finish(const float* raw, const long* off, const long* n_frames, int n, int n_mels, float* out, void* stream);
const char* mimi_mel_last_error(void);

/* ---- THE WHISPER ENCODER: the recogniser's hot path (tests/whisper_enc_ref.py states the rule in float64 torch) ----
 * What stands between the log-mel features above and the text is a Whisper-family model; its encoder runs all n_ctx positions of every
 * turn, however short, and distil-whisper keeps the whole of it.  This is that encoder, the forward of transformers' WhisperEncoder:
 *   1. conv1 (k = 3, pad 1) + GELU over the (n_mels, 2 n_ctx) features; conv2 (k = 3, stride 2, pad 1: output t reads inputs 2t - 1, 2t,
 *      2t + 1, zero outside) + GELU; transposed to (n_ctx, d); + embed_positions.
 *   2. L pre-LN layers: x += out_proj(attention(LN(x))); x += fc2(GELU(fc1(LN(x)))).  Self-attention has a bias on q, v and out and NONE
 *      on k; q is scaled by head_dim^-0.5 = 0.125; there is NO mask.  GELU is the erf form.
 *   3. a final LayerNorm.
 * Head dim is 64, as in every Whisper size: create refuses d_model != 64 n_heads.
 * NUMERICAL RULE.  fp16 operands on v_mfma_f32_32x32x16_f16, fp32 everything else (Whisper checkpoints are published in fp16: the weights
 * stay exact).  The residual stream is fp32 in device memory from conv2 + positions to the final LayerNorm.  Rounded to fp16 exactly
 * here and nowhere else: the input features; every weight matrix, once at create; conv1's GELU output; each LayerNorm output but the
 * last; q (after bias and the exact x 0.125), k and v; the softmax numerators P (the running sum takes them unrounded); the attention
 * output; fc1's GELU output.  Kept in fp32: biases, LayerNorm parameters, positions, accumulators, scores, the softmax with its running
 * maximum and sum, erff, the LayerNorm statistics (two passes).  Every output element's K chain has ONE fixed order (k ascending, one
 * accumulator), whatever the batch size, the clip's place in the batch or the tile shape a launch picked; no split-K, no atomics.  So a
 * clip's output has the same bits alone, at any position in a batch of any size, and on a repeated call; a non-finite feature stays
 * inside its own clip.  A key tile's missing keys (n_ctx is no multiple of 32) give nothing to the maximum and exactly 0 to the sum.
 * Weights: fp32 pointers named after model.get_encoder().state_dict(), all in host memory (host = 1) or all in device memory (host = 0);
 * matrices are (out, in) row-major, the convolutions (out, in, 3).  They are converted once at create, which synchronises; a matrix value
 * that does not fit fp16, or any value that is not finite, fails create with the tensor's name (host weights: before any device call).
 * encode: features (batch, n_mels, 2 n_ctx) fp32 as mimi_mel_finish writes them, out (batch, n_ctx, d_model) in out_fmt (0 = fp32,
 * 1 = fp16, 2 = bf16: the fp32 value rounded to nearest even), both device memory; 2 + 7 n_layers + 1 launches on `stream`, no host
 * synchronisation, no allocation, no host-to-device copy.  One encode at a time per handle: the handle owns the activations.
 * describe: the launch plan of an encode of `batch` clips as text; returns the bytes the whole text takes, writes at most cap.
 * Returns -1 with a message (mimi_wenc_last_error; h == NULL: this thread's create error) and NO device call for: a null pointer, n_mels
 * not 80 or 128, n_heads outside [1, 20], d_model != 64 n_heads, n_layers outside [1, 32], n_ctx outside [1, 1500], ffn_dim no multiple
 * of 64 in [64, 8192], ln_eps outside (0, 1), max_batch outside [1, 64]; encode: batch outside [1, max_batch], an unknown format, a
 * misaligned buffer.  -2: a HIP error; a create that fails frees everything it took.                                                    */
#define MIMI_WENC_MAX_LAYERS 32
#define MIMI_WENC_MAX_CTX 1500
#define MIMI_WENC_MAX_BATCH 64
typedef struct MimiWenc* mimi_wenc;
typedef struct { int32_t n_mels, d_model, n_layers, n_heads, ffn_dim, n_ctx; float ln_eps; } MimiWencConfig;
typedef struct {
    const float *self_attn_layer_norm_w, *self_attn_layer_norm_b, *q_w, *q_b, *k_w, *v_w, *v_b, *out_w, *out_b;
    const float *final_layer_norm_w, *final_layer_norm_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;
} MimiWencLayerWeights;
typedef struct {
    int32_t host;                                                  /* 1: every pointer is host memory; 0: device memory */
    const float *conv1_w, *conv1_b, *conv2_w, *conv2_b, *embed_positions, *layer_norm_w, *layer_norm_b;
    MimiWencLayerWeights layers[MIMI_WENC_MAX_LAYERS];
} MimiWencWeights;
int  mimi_wenc_create(const MimiWencConfig* cfg, const MimiWencWeights* w, int max_batch, mimi_wenc* out);
void mimi_wenc_destroy(mimi_wenc h);
const char* mimi_wenc_last_error(mimi_wenc h);                 /* h == NULL: why mimi_wenc_create failed (this thread) */
int  mimi_wenc_encode(mimi_wenc h, const float* features, int batch, void* out, int out_fmt, void* stream);
int  mimi_wenc_describe(mimi_wenc h, int batch, char* text, int cap);

#ifdef __cplusplus
}
#endif
#endif
