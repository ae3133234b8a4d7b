/*
 * libcsm_hip.so -- C ABI of the MI355X-native CSM speech-generation hot path.
 *
 * The reference (zenoran/sesameai-tts) has no FFI: its boundary for this path is the Python
 * surface `Model.generate_frame` / `Model.setup_caches` / `Model.reset_caches`
 * (sesameai/models.py:120-188) and `mimi.decode` (sesameai/generator.py:299).  This header is
 * the C ABI the build puts UNDER that surface; each entry point cites the reference
 * interface it replaces.  The Python shim (sesameai-tts_amd/sesameai/_abi.py) binds exactly
 * these symbols with ctypes; tests/test_abi.py checks that every one is exported.
 *
 * Conventions: plain pointers and sizes only (no torch types).  Every pointer marked
 * `dev` is a device pointer owned by the caller and must stay valid for the lifetime of the
 * handle (weights) or of the call (inputs/outputs).  `stream` is a hipStream_t passed as
 * void*.  All functions return 0 on success or a negative CSM_E_* code; the message is
 * available from csm_last_error().  A handle is not thread-safe: one handle per GPU
 * (the reference model is single-threaded too: one KV-cache set, tts_service.py:191).
 */
#ifndef CSM_HIP_H
#define CSM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CSM_OK            0
#define CSM_E_INVALID    -1   /* bad argument / unsupported shape                       */
#define CSM_E_HIP        -2   /* a HIP runtime call failed                              */
#define CSM_E_STATE      -3   /* call order violated (e.g. frame step before prefill)   */
#define CSM_E_TOO_LONG   -4   /* position would exceed max_seq (generator.py:276-281)   */
#define CSM_E_NO_PAGES   -5   /* the session store's pool is too short for this save    */

#define CSM_MAX_LAYERS   32

/* One Llama stack = torchtune llama3_2(...) with tok_embeddings/output stripped
 * (sesameai/models.py:10-52). */
typedef struct CsmLlamaDims {
    int32_t n_layers, n_heads, n_kv_heads, dim, ffn, max_seq;
    float   norm_eps;
} CsmLlamaDims;

/* ModelArgs (sesameai/models.py:90-96) + the two flavours. */
typedef struct CsmConfig {
    CsmLlamaDims backbone;      /* llama-1B   : 16L 32H/8KV d2048 ffn8192 */
    CsmLlamaDims decoder;       /* llama-100M :  4L  8H/2KV d1024 ffn8192 */
    int32_t text_vocab;         /* 128256 */
    int32_t audio_vocab;        /* 2051   */
    int32_t n_codebooks;        /* 32     */
} CsmConfig;

/* bf16 tensors, row-major, nn.Linear layout [out][in]. */
typedef struct CsmLayerWeights {
    const void *wq, *wk, *wv, *wo;      /* [H*hd][d] [KV*hd][d] [KV*hd][d] [d][H*hd] */
    const void *w1, *w2, *w3;           /* gate [ffn][d], down [d][ffn], up [ffn][d] */
    const void *sa_norm, *mlp_norm;     /* [d] */
} CsmLayerWeights;

typedef struct CsmWeights {
    const void *text_emb;               /* [text_vocab][d_bb]                         */
    const void *audio_emb;              /* [n_codebooks*audio_vocab][d_bb]            */
    CsmLayerWeights bb[CSM_MAX_LAYERS];
    const void *bb_norm;                /* [d_bb]                                     */
    CsmLayerWeights dec[CSM_MAX_LAYERS];
    const void *dec_norm;               /* [d_dec]                                    */
    const void *projection;             /* [d_dec][d_bb]                              */
    const void *c0_head;                /* [audio_vocab][d_bb]                        */
    const void *audio_head_t;           /* [n_codebooks-1][audio_vocab][d_dec]: the reference's
                                           K-major audio_head (models.py:118,176) transposed once
                                           at load time so each logit is a contiguous row      */
    const void *bb_rope;                /* [max_seq][hd/2][2] bf16 (cos,sin), Llama3ScaledRoPE
                                           cache after model.to(bf16) (generator.py:343)       */
    const void *dec_rope;               /* same for the decoder's head_dim                     */
    /* ---- optional OCP-e4m3 weight stream for the decode step (BASELINE config 5) -------------
     * fp8 != 0: bb8/dec8 hold wq..w3 as e4m3 bytes [out][in] and bb8s/dec8s the per-output-row
     * fp32 scales (powers of two, so e4m3*scale is exactly the bf16 value in bb/dec above, which
     * the prefill / batched path keeps using).  Heads likewise.                                */
    int32_t fp8;
    CsmLayerWeights bb8[CSM_MAX_LAYERS], bb8s[CSM_MAX_LAYERS];
    CsmLayerWeights dec8[CSM_MAX_LAYERS], dec8s[CSM_MAX_LAYERS];
    const void *c0_head8, *c0_head8s;   /* [audio_vocab][d_bb] e4m3, [audio_vocab] f32          */
    const void *audio_head8, *audio_head8s;   /* [n_codebooks-1][audio_vocab][d_dec] e4m3, [..][audio_vocab] f32 */
} CsmWeights;

typedef struct CsmModel* csm_handle;
typedef struct CsmPrefix* csm_prefix;   /* a K/V snapshot of a prompt prefix (csm_prefix_capture) */
typedef struct CsmSession* csm_session; /* a conversation's K/V in pages of the handle's session store (csm_session_open) */

/* Model(config) + setup_caches(max_batch) (models.py:107-130): allocates KV caches
 * [L][B][KV][max_seq][hd] (backbone) / [L][B][KV][n_codebooks][hd] (decoder) and workspaces.
 * max_rows = largest B*S one csm_prefill call will carry.                                   */
int  csm_create(const CsmConfig* cfg, const CsmWeights* w /*dev ptrs*/, int max_batch, int max_rows,
                int max_frames, csm_handle* out);
void csm_destroy(csm_handle h);
const char* csm_last_error(csm_handle h);   /* h may be NULL: last create() error */

/* Model.reset_caches() (models.py:186-188): rewinds positions and the frame history.  The
 * caches need no zeroing: attention is bounded by position, never by a 2048-wide mask.     */
int csm_reset(csm_handle h, void* stream);

/* Seeds the on-device Philox sampler (the reference uses the global torch RNG, models.py:73).  Frame steps draw at
 * (seed, frame counter, sequence, codebook); the frame 0 of a slot refill (csm_prefill_slot) draws from a second key domain
 * (seed ^ salt, refill counter), so neither two refills nor a refill and a frame step ever share a noise stream.            */
int csm_seed(csm_handle h, uint64_t seed, void* stream);

/* Per-slot sampling table: temperature, top-k and Philox seed of ONE request inside a live batch.  The reference samples every frame with the
 * caller's scalars (tts_service.py:175 uses 0.9/50, :266 0.8/40) and is batch-1, so two such requests never meet; here they share a batch.
 * The handle keeps one entry per batch slot in device memory: {temperature, topk, seed, counter, own_rng}.  A slot WITH an entry is sampled
 * with its own temperature and top-k by every sampler that serves its row (csm_depth, csm_frame_step, csm_generate_frame_s1 at any batch
 * size, and the batch-1 depth pass of csm_prefill_slot, which reads the entry of `slot`); a slot without one uses the call's scalars.
 * topk == 1 in an entry is the greedy rule for that row only.  With a seed of its own the row draws Philox at (its seed, its own frame
 * counter, sequence 0, codebook) instead of (handle seed, global frame counter, slot, codebook): the counter is the utterance's frame index --
 * 0 for the frame 0 that csm_depth, csm_prefill_slot or the step after csm_refill_* samples, + 1 per committed frame, held while the slot is
 * parked, and rewound by csm_slot_sampling_set, csm_prefill (rows 0..B-1), csm_prefill_slot and csm_refill_begin -- so a request's codes
 * depend neither on the slot it landed in nor on what the batch did before it arrived.
 *   csm_slot_sampling_set:   slots is a host array of n slots; temperature / topk hold one value per listed slot (temperature > 0,
 *                            topk >= 1, slot in [0, max_batch), else CSM_E_INVALID and nothing is written); seed holds one per listed slot,
 *                            or is NULL = the slots keep drawing from the handle's stream (csm_seed).  Stream-ordered, no host
 *                            synchronisation (the values travel as kernel arguments): in force for everything enqueued after it; legal
 *                            between frame steps and for a slot whose refill is parked.  The first call makes the handle's later frame steps
 *                            capture a graph that carries the table (ONE graph per (B, topk, temperature) whatever the entries hold); a
 *                            handle that never calls it runs exactly the launches it ran before this interface existed.
 *   csm_slot_sampling_clear: removes the listed slots' entries (slots == NULL: all of them).  Stream-ordered.  csm_reset clears the whole
 *                            table, csm_reset_slots leaves it alone.
 *   csm_slot_sampling_get:   one slot's entry (any out pointer may be NULL); synchronises the stream.  For tests and diagnostics.          */
int csm_slot_sampling_set(csm_handle h, const int32_t* slots /*host*/, int n, const float* temperature, const int32_t* topk,
                          const uint64_t* seed, void* stream);
int csm_slot_sampling_clear(csm_handle h, const int32_t* slots /*host; NULL = all*/, int n, void* stream);
int csm_slot_sampling_get(csm_handle h, int slot, int32_t* has_entry, float* temperature, int32_t* topk, int32_t* own_rng,
                          uint64_t* seed, uint64_t* counter, void* stream);

/* The backbone half of Model.generate_frame (models.py:153-160) on B sequences x S rows:
 * masked embedding sum -> 16 layers with KV append at pos -> final norm of each sequence's
 * last row (kept in the handle as last_h).  tokens [B][S][33] i32, mask [B][S][33] u8,
 * pos [B][S] i32, all dev.  After it the internal position of sequence b is pos[b][S-1]+1.
 * prompt_mode != 0: always take the matrix-core (wide-M) kernels, so that a prompt row's result
 * does not depend on how many rows share the call (needed for bit-identical prefix-KV reuse);
 * 0: fewer than 16 rows run on the weight-stationary GEMV kernels of the decode step.       */
int csm_prefill(csm_handle h, const int32_t* tokens, const uint8_t* mask, const int32_t* pos,
                int B, int S, int prompt_mode, void* stream);

/* The depth half of Model.generate_frame (models.py:160-184): c0 head + sample, then 31
 * decoder steps.  Consumes last_h; writes the frame into out_frame [B][32] i32 (dev, may be
 * NULL) and into the handle's history.  topk==1 selects the deterministic lowest-index argmax.
 * forced [B][32] i32 (dev, may be NULL): teacher forcing -- fed back instead of the samples.
 * logits_out (dev, may be NULL): [32][B][audio_vocab] bf16 capture for tests.
 * noise (dev, may be NULL): [32][B][audio_vocab] bf16 Exp(1) draws replacing the Philox RNG.
 * commit != 0: append the frame to the history and stage it (or `forced`, if given) as the
 * input of the next csm_frame_step -- the first generated frame after a prefill.             */
int csm_depth(csm_handle h, int B, float temperature, int topk, const int32_t* forced,
              int32_t* out_frame, void* logits_out, const void* noise, int commit, void* stream);

/* One whole generated frame for the continuing loop (generator.py:283-294): the previous
 * frame (kept on device) is embedded with mask [1 x32, 0] at the internal position, one
 * backbone step, csm_depth, position += 1, frame appended to the history, EOS flag
 * (all 32 codes == 0, generator.py:285) accumulated per sequence.  No host sync; the whole
 * step is captured once into a hipGraph and replayed.  Up to 4 captured steps are kept per handle, keyed on
 * (B, topk, temperature, carries the per-slot sampling table) and replaced least-recently-used first: callers that alternate sampling parameters or batch
 * sizes (tts_service.py:175 uses 0.9/50, :266 0.8/40) replay, they do not capture again.
 * Batch 1 on the CSM-1B shapes: codebooks 1..31 and every backbone layer run as launches of 256 workgroups
 * that must all be resident at once (csrc/dec_first.cuh, csrc/dec_persist.cuh, csrc/bb_block.cuh).  Drive ONE frame loop per GPU (batch, or
 * one process per GPU); two loops sharing a GPU can starve each other, which ends -- after a bounded 50 ms spin, never a
 * hang -- in CSM_E_HIP from csm_read_frames; csm_reset makes the handle usable again.  CSM_PERSIST=0 / CSM_DEC_FIRST=0 / CSM_BB_BLOCK=0
 * select the plain launch chain.                                                              */
int csm_frame_step(csm_handle h, int B, float temperature, int topk, int use_graph, void* stream);
/* Copies the most recent frame [B][32] i32 to out_frame (dev) on the stream.                 */
int csm_copy_frame(csm_handle h, int B, int32_t* out_frame, void* stream);

/* Replace the "previous frame" inputs of the next csm_frame_step with caller data
 * (Model.generate_frame called directly with S==1, tts_service.py:225):
 * tokens [B][33] i32, mask [B][33] u8, pos [B] i32, dev.                                     */
int csm_set_step_inputs(csm_handle h, const int32_t* tokens, const uint8_t* mask, const int32_t* pos,
                        int B, void* stream);

/* Model.generate_frame for every frame AFTER the prompt, with the reference's own tensors (models.py:132-139 as called from
 * tts_service.py:224-241 and generator.py:283-294): tokens [B][1][33] int64, mask [B][1][33] bool (one byte each), pos [B][1]
 * int64, all dev and contiguous -> out_frame [B][32] int32 (dev).  = csm_set_step_inputs + csm_frame_step (hipGraph replay) +
 * csm_copy_frame in ONE call: the staging kernel reads the reference's dtypes (no conversion kernels on the host side), the
 * frame carries -1 if an all-CU launch gave up, and the handle's device is made current inside the call.  No host sync.       */
int csm_generate_frame_s1(csm_handle h, const int64_t* tokens, const uint8_t* mask, const int64_t* pos, int B,
                          float temperature, int topk, int32_t* out_frame, void* stream);

/* Per-slot reset and refill of a live batch (SURVEY.md 8b `csm_reset(handle, batch_slots, n)`; the reference is batch-1 and resets
 * its one cache set per utterance, generator.py:255).  Utterances of a batch end at different frames (generator.py:285): a finished
 * one is retired and its slot given to the next prompt while the other slots keep generating.
 * csm_reset_slots: position 0 and "no EOS yet" for the listed slots (host array); their K/V need no clearing.
 * csm_prefill_slot: the prompt rows tokens [S][33] / mask [S][33] / pos [S] (dev) run through the backbone into slot `slot`'s
 * caches, the depth pass produces the new utterance's frame 0 (written to out_frame [32] dev if given, and into the history at the
 * NEWEST global frame index, replacing that slot's entry there), and the frame is staged as the slot's input of the next
 * csm_frame_step.  The other slots' state is untouched: their frames are bit-identical to an undisturbed run, and
 * csm_copy_frame keeps returning every slot's own newest frame (the refilled slot's: its frame 0).  Call between
 * frame steps, on the stream that runs them.  A batch may also be FILLED slot by slot this way after csm_reset (prompts of
 * different lengths): the first call opens global frame 0.                                                                       */
int csm_reset_slots(csm_handle h, const int32_t* slots /*host*/, int n, void* stream);
int csm_prefill_slot(csm_handle h, int slot, const int32_t* tokens, const uint8_t* mask, const int32_t* pos, int S,
                     int prompt_mode, float temperature, int topk, int32_t* out_frame, void* stream);

/* Refill BESIDE the frame loop (round 4): csm_prefill_slot makes the other slots wait for the new prompt's whole prefill and a
 * batch-1 depth pass (4 ms at 190 rows, > 8 ms at 1,334).  Here the prompt runs a few backbone layers per call between frame
 * steps, in buffers of its own, and the new utterance's frame 0 is sampled BY THE NEXT FRAME STEP, in the batch, from the prompt's
 * last row (an inject node in the frame-step graph; the slot's position stays for that one step and its EOS word restarts).
 * ONE mechanism with two begin forms: a handle holds at most one pending refill, begun for one slot (csm_refill_begin) or for a group of
 * slots in one ragged prefill (csm_refill_group_begin, below).  Parking, the frame steps' treatment of parked slots, completion and the
 * refusals are the same for both; each form is advanced by its own call, and the other form's advance is refused (CSM_E_STATE).
 *   csm_refill_begin:   embeds the prompt rows (tokens [S][33] / mask [S][33] / pos [S], dev; pos must stay valid until the refill
 *                       completes) and parks the slot: until completion its rows of the frame steps are placeholders whose frames
 *                       the caller ignores and its position is HELD at S (however many steps the prompt takes, it never nears
 *                       max_seq).  CSM_E_STATE while a refill of either form is pending.  Needs csm_refill_supported(h, max_batch).
 *   csm_refill_advance: runs up to max_layers more backbone layers of the pending prompt.  Returns 1 when the prompt is complete --
 *                       the NEXT csm_frame_step then yields the utterance's frame 0 in that slot's row, at that step's global frame
 *                       index -- 0 while layers remain, < 0 on error.  Call both on the stream that runs the frame steps.
 *   csm_refill_supported: 1 when frame steps of B rows carry the inject node (the matrix-core decode path: B >= 3 by default,
 *                       CSM_WIDE / CSM_WIDE_MIN move it), else 0 -- the ONE predicate begin, the frame step and the host share.
 *                       While a refill is parked or waits to be sampled, csm_frame_step with a B for which this is 0 is refused
 *                       (CSM_E_STATE) instead of stepping the slot like a generating one; csm_reset_slots / csm_prefill_slot on
 *                       the slot whose prompt is still running are refused too, and drop a completed-but-unsampled refill.
 * The other slots' frames are bit-identical to an undisturbed run (their rows never see the refill).                          */
int csm_refill_supported(csm_handle h, int B);
int csm_refill_begin(csm_handle h, int slot, const int32_t* tokens, const uint8_t* mask, const int32_t* pos, int S, void* stream);
int csm_refill_advance(csm_handle h, int max_layers, void* stream);

/* The other begin form: SEVERAL slots at once -- one ragged prefill.  Slots that retire in the same block would otherwise queue behind each other,
 * each taking the backbone's whole launch chain for a handful of rows (after a prefix copy a refill is ~40 rows: launch-bound).
 *   csm_refill_group_begin:   n <= 32 segments; segment i is the prompt rows of batch slot slots[i], rows[i] >= 1 of them, and the rows of all
 *                       segments lie back to back in tokens [M][33] / mask [M][33] / pos [M] (dev; M = sum rows[i] <= max_rows; pos gives every
 *                       row its true position -- a segment that follows a copied prefix starts at the prefix length -- and must stay valid
 *                       until the group completes).  `slots` and `rows` are host arrays, read before the call returns; the segment table
 *                       travels in the kernel arguments, so the call neither copies to the device nor synchronises.  What csm_refill_begin
 *                       does for one slot happens for every listed slot: embedded, parked at its own pos[last row] + 1, sampling-table
 *                       counter rewound.  CSM_E_INVALID (nothing is enqueued) for n outside [1, 32], a slot outside [0, max_batch) or listed
 *                       twice, rows[i] < 1, M > max_rows.  CSM_E_STATE while a refill of either form is pending.  Needs
 *                       csm_refill_supported(h, max_batch).
 *   csm_refill_group_advance: up to max_layers more backbone layers over all M rows.  1 when the group is complete -- the NEXT csm_frame_step
 *                       yields frame 0 of all n utterances --, 0 while layers remain, < 0 on error.
 * csm_reset_slots / csm_prefill_slot / csm_prefix_capture / csm_prefix_apply on a slot of the pending refill are refused, whichever form
 * began it.  The forms differ in the layer launches alone: one slot runs as a batch of one sequence, a group (also of one) through the
 * ragged kernels.  Every row's K/V and every slot's frame 0 input are the bits the same segments give one after the other through
 * csm_refill_begin / csm_refill_advance (a group of n = 1 included).                                                            */
int csm_refill_group_begin(csm_handle h, const int32_t* slots /*host*/, const int32_t* rows /*host*/, int n,
                           const int32_t* tokens /*dev [M][33]*/, const uint8_t* mask /*dev [M][33]*/, const int32_t* pos /*dev [M]*/, void* stream);
int csm_refill_group_advance(csm_handle h, int max_layers, void* stream);

/* Prefix store: shared voice-prompt K/V for the live batch.  A request is a 900-1,550-row voice prompt followed by a few dozen rows of new
 * text, and the reference re-runs the whole prompt for every sentence (tts_service.py:191-207).  In prompt mode a row's K/V do not depend on
 * how many rows share the call, so the backbone K/V rows of a prompt prefix are the same bits in every slot and for every request that starts
 * with it: they are snapshotted once and copied instead of recomputed; only the rows after the prefix are prefilled, at their true positions
 * (the `pos` arrays of csm_prefill / csm_prefill_slot / csm_refill_begin start at the prefix length P; a parked slot is held at P + S).
 *   csm_prefix_capture: snapshots rows [0, rows) of `slot`'s backbone K/V, all layers, into a dense allocation
 *                       [layer][K|V][kv head][rows][hd] bf16 that the prefix owns.  rows must not exceed the slot's position (the rows must
 *                       have been written: synchronises the stream to learn it) and must be < max_seq; CSM_E_STATE for the slot whose refill
 *                       beside the loop is running.
 *   csm_prefix_apply:   writes the snapshot into rows [0, rows) of each listed slot's caches (host array, n <= max_batch) -- ONE launch for
 *                       all layers, K and V, all kv heads and all n slots, no host synchronisation.  Positions and every other state of the
 *                       slots are untouched.  Enqueue it IMMEDIATELY before the csm_refill_begin / csm_prefill_slot / csm_prefill call that
 *                       runs the suffix, on the same stream: a retired slot keeps stepping from position 0 as a placeholder and a frame step
 *                       in between would overwrite the first copied rows.  CSM_E_STATE for a slot whose refill is in flight; CSM_E_INVALID
 *                       for a prefix of another shape (layers / kv heads / head_dim), of another GPU, or with rows >= this handle's max_seq.
 *   csm_prefix_rows / csm_prefix_bytes: the snapshot's row count / size of its allocation (0 for NULL).
 *   csm_prefix_read:    downloads the snapshot to host memory (bytes must equal csm_prefix_bytes; synchronises).  For tests.
 *   csm_prefix_destroy: frees the snapshot.  csm_destroy of the handle it was captured from releases the device memory of the prefixes still
 *                       alive (they can then only be destroyed); csm_describe reports their number and total bytes.                         */
int    csm_prefix_capture(csm_handle h, int slot, int rows, csm_prefix* out, void* stream);
int    csm_prefix_apply(csm_handle h, csm_prefix prefix, const int32_t* slots /*host*/, int n, void* stream);
int    csm_prefix_rows(csm_prefix prefix);
size_t csm_prefix_bytes(csm_prefix prefix);
int    csm_prefix_read(csm_prefix prefix, void* host_buf, size_t bytes, void* stream);
void   csm_prefix_destroy(csm_prefix prefix);

/* Session store: a conversation's backbone K/V carried from turn to turn.  A spoken dialogue's prompt is its whole history -- the voice
 * prompt, every earlier turn, the audio generated a second ago -- and all of its rows but the few dozen of the new turn were in the slot's
 * cache when the last reply ended.  A prefix snapshot (above) could keep them, but every capture allocates a dense block, synchronises and
 * copies all rows again: right once per voice, wrong once per turn between two frame steps.  A SESSION keeps the rows in fixed-size pages
 * of one pool that the handle allocates once: a page holds page_rows rows of every layer's K and V of every kv head
 * ([layer][K|V][kv head][page_rows][hd] bf16; 2 MB at CSM-1B with 64 rows).  At the end of a turn only the new rows are appended; at the
 * start of the next the pages are gathered into whichever slot the request gets and only the rows after them are prefilled.
 * ORDERING: csm_session_save, csm_session_load, csm_session_forget and csm_session_truncate allocate nothing, copy nothing from the host and never
 * synchronise (the page numbers travel in kernel arguments into a device table that the load reads).  They are meant for the frame
 * loop's stream, between frame steps, and that ONE stream is what makes page reuse safe: a page that a truncate or close gives back may
 * be handed to the next save at once, because every load that still reads it was enqueued earlier on the same stream.  Calls on a second
 * stream need the caller's own events between them.
 *   csm_session_store_create: the pool of n_pages pages of page_rows rows (1 <= page_rows <= max_seq), once per handle (CSM_E_STATE the
 *                       second time; CSM_E_HIP, and no store, when the allocation fails).  Up to n_pages + 32 sessions can be open.
 *   csm_session_open:   a new, empty session.
 *   csm_session_save:   appends rows [csm_session_rows(s), rows) of `slot`'s caches, all layers; the session then holds `rows` rows.  The
 *                       rows must have been written (rows <= the slot's position: the CALLER's knowledge -- reading the position would
 *                       synchronise).  CSM_E_NO_PAGES when the pool has too few free pages: a code of its own, so that the host can
 *                       truncate or close another session and call again.
 *   csm_session_load:   writes the rows [0, rows_i) of n <= 32 sessions into the slots slots[i] (host arrays) in ONE launch -- sessions of
 *                       different lengths resume together in one refill group.  Rows at and beyond rows_i of a slot are not written;
 *                       positions and every other state of the slots are untouched: the caller runs the suffix at its true positions
 *                       (pos starts at rows_i), exactly as after csm_prefix_apply, and enqueues the load IMMEDIATELY before that call.
 *   csm_session_truncate: the session keeps its first `rows` rows (barge-in: the listener heard only part of the last reply); whole
 *                       pages beyond the new end return to the pool.  Host bookkeeping only.
 *   csm_session_forget: the session drops its rows [from, to) IN PLACE (an endless conversation forgets its oldest turns and keeps the
 *                       voice prompt).  Rows below `from` stay where they are (attention is causal: they never saw what
 *                       is dropped); rows from `to` on move down by d = to - from, V as it is and K -- stored rotated -- rotated BACK by d
 *                       positions: a pair (x0, x1) becomes (x0 c + x1 s, x1 c - x0 s) with rot[j] = (c, s) = (cos, sin)(d * theta_j), a
 *                       HOST array [head_dim / 2][2] of floats that the caller computes from the frequencies of its rope table (the
 *                       library does not know theta).  fp32 on the bf16 values, multiplies and adds kept apart, ONE rounding to bf16 per
 *                       forget.  Logical pages below from / page_rows keep their page numbers; the rows from there on are rewritten into
 *                       FRESH pages (pages_for(rows - d) - from / page_rows of them) by one copy launch, and the old pages return to the
 *                       pool in the same call.  Like save and load it allocates nothing, copies nothing from the host and never
 *                       synchronises: rot and the new page numbers travel in kernel arguments.  to == rows is a truncate to `from`;
 *                       from == to returns CSM_OK and enqueues nothing.  head_dim 64 and 128.  Refused with nothing enqueued and the
 *                       session unchanged: a range outside [0, rows] or to < from, a NULL rot, a closed session or one of another handle
 *                       (CSM_E_INVALID); too few free pages (CSM_E_NO_PAGES).
 *   csm_session_rows / csm_session_pages: rows held / pages owned (0 for NULL or after csm_destroy of the handle).
 *   csm_session_read:   the session's rows, dense in csm_prefix_read's layout [layer][K|V][kv head][rows][hd] (bytes must match;
 *                       synchronises).  For tests.
 *   csm_session_close:  returns the pages and frees the object.
 * Refused with nothing enqueued and the session unchanged: rows below the session's row count or >= max_seq (CSM_E_INVALID); a slot
 * outside the batch or listed twice in one load (CSM_E_INVALID); a slot whose refill beside the loop is running (CSM_E_STATE, the
 * predicate of the prefix calls); a session of another handle or a closed one (CSM_E_INVALID); a pool too short (CSM_E_NO_PAGES).
 * csm_destroy releases the pool; session objects still alive can then only be closed.  csm_describe reports
 * `session_store=<n> sessions, <used>/<total> pages; session_forgets=<n> (<rows> rows moved)`. */
int  csm_session_store_create(csm_handle h, int n_pages, int page_rows);
int  csm_session_open(csm_handle h, csm_session* out);
int  csm_session_save(csm_handle h, csm_session s, int slot, int rows, void* stream);
int  csm_session_load(csm_handle h, const csm_session* ss, const int32_t* slots /*host*/, int n, void* stream);
int  csm_session_forget(csm_handle h, csm_session s, int from, int to, const float* rot /*host, [head_dim/2][2]*/, void* stream);
int  csm_session_truncate(csm_session s, int rows);
int  csm_session_rows(csm_session s);
int  csm_session_pages(csm_session s);
int  csm_session_read(csm_session s, void* host_buf, size_t bytes, void* stream);
void csm_session_close(csm_session s);

/* Start-up weight broadcast (SURVEY.md 8b's csm_broadcast_weights; 8e: "one RCCL ncclBroadcast of the packed weight blob at start-up
 * over xGMI ... no per-step collective").  The reference has no counterpart (it is single-GPU: every process downloads its own
 * checkpoint, sesameai/generator.py:330-346); in the replica layout rank `root` holds the weights and every other
 * rank's blob -- `bytes` bytes of device memory at the same layout -- is filled by ONE in-place ncclBroadcast on `stream`.
 * The communicator is the CALLER's (an ncclComm_t made with ncclCommInitRank / ncclCommInitAll, passed as void*): this library does
 * not link RCCL and never creates a communicator -- it resolves ncclBroadcast from the RCCL instance already loaded in the process
 * (global scope, else the loaded librccl.so.1 by soname), i.e. the one the communicator belongs to, so a process never holds two
 * RCCL instances / bootstraps / sets of xGMI rings.  CSM_E_STATE when no RCCL is loaded, CSM_E_HIP when the collective fails
 * (csm_last_error(NULL) has the text).  Python hosts that use torch.distributed keep using dist.broadcast on the same blob
 * (sesameai/parallel.py: torch owns that communicator and does not hand out the ncclComm_t); plain-C hosts call this
 * (examples/c_host/csm_c_host.c).  The CsmWeights pointers handed to csm_create then point into the blob.      */
int csm_broadcast_weights(void* dev_blob, size_t bytes, void* rccl_comm, int root, void* stream);

/* What this handle runs, as one line of text: weight stream, the kernels of a batch-1 / batched backbone step, of the depth decoder and of
 * prompts, the frame-graph cache, the live prefixes of the prefix store (number, total bytes), the session store (open sessions, pages used / total), and every CSM_* / MIMI_* switch set in the environment.  Writes at most n - 1 characters + NUL into buf (may
 * be NULL) and returns the length the whole text needs.  The reference has no counterpart (it has one eager path); bench.py records it with
 * every number it prints (config.paths).                                                                                              */
int csm_describe(csm_handle h, char* buf, int n);
/* Lists on stderr, once per process, the environment names under CSM_ / MIMI_ that no switch reads (csm_create calls it).           */
void csm_warn_unknown_switches(void);

/* History readback: frames [first, first + n) as [n][B][32] i32 into host memory (synchronises the stream);
 * eos_at[b] = global index of the first all-zero frame of sequence b, or -1.  The history is a RING of max_frames frames
 * (global frame g lives in row g % max_frames), so a frame loop may run for any number of frames as long as every frame is
 * read before max_frames newer ones exist; a range that has been overwritten is CSM_E_INVALID.                                */
int csm_num_frames(csm_handle h);
int csm_read_frames(csm_handle h, int B, int first, int n, int32_t* host_frames, int32_t* host_eos_at,
                    void* stream);
/* Device pointer to the history ring [max_frames][B_stride=max_batch][32] i32 (row = global frame % max_frames).           */
const int32_t* csm_frames_dev(csm_handle h);
/* Device pointer to last_h [max_batch][d_bb] bf16 (tests). */
const void* csm_last_h_dev(csm_handle h);

/* Bytes the dominant kernels stream per generated frame (unique weights + KV at mean
 * position p_mean); used by bench.py's roofline.                              */
double csm_bytes_per_frame(csm_handle h, int B, double p_mean);

#ifdef __cplusplus
}
#endif
#endif /* CSM_HIP_H */
