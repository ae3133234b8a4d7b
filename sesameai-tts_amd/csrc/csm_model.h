// The handle behind csm_handle and what every translation unit of the host side shares: the structs, the error plumbing (fail, HIPCHK) and
// the handle's allocator.  Private to csrc/ (the C ABI is include/csm_hip.h).  The only kernel header it may include is common.cuh: whoever
// includes this one does not instantiate a launcher.  csm_engine.hip holds what instantiates or sequences the kernels; host-only parts of
// the ABI (csm_kv_store.hip) live beside it and see the handle through this header.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string>
#include <vector>

#include "../../include/csm_hip.h"
#include "common.cuh"
#include "hip_backend.h"            /* dev_pool.h and its binding to HIP */

#define CSM_LOCAL __attribute__((visibility("hidden")))       /* crosses translation units, stays out of the library's dynamic symbol table */

#define CSM_FRAME_GRAPHS 4    // captured frame steps kept per handle
#define CSM_REFILL_SALT 0x9E3779B97F4A7C15ull      /* Philox key domain of slot refills (csm_seed) */

struct Stack {
    CsmLlamaDims d;
    const CsmLayerWeights* lw;
    const bf16_t* final_norm;
    const bf16_t* rope;
    int hd, nq, nkv, cache_len;
    bf16_t *kc, *vc;            // [L][B][KV][cache_len][hd]
    long layer_stride;          // elements per layer
    long slot_off = 0;          // elements: batch slot the rows of the current call belong to (csm_prefill_slot), else 0
    int nt_attn, nt_mlp;        // cache policy of the q/k/v/o and of the gate/up/down weight streams
    const CsmLayerWeights *w8 = nullptr, *w8s = nullptr;      // fp8 weight stream + scales (nullptr = bf16)
    CsmLayerWeights pk[CSM_MAX_LAYERS];   // matrix-core operand-order copies of wq..w3 (k_pack_w) for the wide-M path
    CsmLayerWeights pk8[CSM_MAX_LAYERS];  // the same for the e4m3 weight stream (k_pack_w8); valid when has_pk8
    bool has_pk8 = false;
};

// The two K/V stores' state in the handle (csm_kv_store.hip owns it: nothing else reads inside)
class SessionPages;
struct PrefixStore {
    std::vector<struct CsmPrefix*> live;         // live K/V snapshots captured from this handle (csm_prefix_capture); orphaned by csm_destroy
};
// session store (csm_session_store_create): conversations' backbone K/V in fixed-size pages of ONE pool allocation
struct SessionStore {
    SessionPages* pages = nullptr;      // the bookkeeping (session_pages.h); nullptr: no store
    bf16_t* pool = nullptr;             // [n_pages][layer][K|V][kv head][page_rows][hd]
    int* tab = nullptr;                 // [max sessions][tab_stride] device page table: row = session id, entry k = the session's logical page k
    int tab_stride = 0;                 //   (written by k_session_save from its kernel arguments, read by k_session_load: no host-to-device copy);
                                        //   one row more than sessions can be open: csm_session_forget's staging row (the new page list while the kernel reads the old)
    int forgets = 0;                    // csm_session_forget calls that dropped rows, and the rows they moved down (csm_describe)
    long forget_moved = 0;
    std::vector<struct CsmSession*> open;        // open session objects of this handle; orphaned by csm_destroy
};

// Initial values are stated HERE, once (members without an initialiser start as zero: new CsmModel() value-initialises); csm_create assigns
// only what it computes from its arguments or reads from a switch.
struct CsmModel {
    DevPool pool{hip_backend()};       // owns every device allocation of the handle: csm_destroy and a failed csm_create release it, nothing else frees
    CsmConfig cfg;
    CsmWeights w;
    int max_batch, max_rows, max_frames, ldl;
    Stack bb, dec;
    // workspaces (bf16 unless noted)
    bf16_t *h, *q, *att, *act;          // backbone rows [max_rows][..]
    float* part;                        // [max(PART_ROWS, max_batch)][H][NSPLIT][ATTN_PS(hd)] split-K attention partials
    int part_rows;
    int* attn_ctr = nullptr;            // [part_rows][KV heads] arrival counters of the split-K attention's in-kernel merge (attn.cuh); nullptr: CSM_ATTN_MERGE=0
    bf16_t *dec_in;                     // [B][2][d_bb]   row0 = last_h, row1 = c0 embedding
    float* slab;                        // [8][max_rows][max(d_bb, d_dec)] fp32 split-K partials of the wide path
    bf16_t *pk_projection, *pk_c0_head, *pk_audio_head;   // packed copies for the wide-M path
    uint8_t *pk8_c0_head = nullptr, *pk8_audio_head = nullptr;    // e4m3 heads in operand order (fp8 mode)
    long pk_head_stride;                // elements between packed audio heads
    bf16_t *qkv0_tab = nullptr;         // [(n_codebooks-2)*audio_vocab][nq + 2 nkv]: layer-0 q | k | v of the depth decoder for every
                                        // (codebook c in 1..ncb-2, token) at its fixed position c+1 (env CSM_QKV0_TABLE=0 disables)
    bf16_t *proj_emb;                   // [n_codebooks*audio_vocab][d_dec] = projection(audio_embeddings), built once at create:
                                        // the decoder input of steps >= 2 is a 2 KB row gather instead of a 4.2 MB GEMV
    bf16_t *hdec, *qd, *attd, *actd;    // decoder rows [2B][..]
    bf16_t* logits;                     // [B][ldl]
    int *frame, *cur_tokens, *cur_pos, *history, *n_frames, *eos_at, *dec_pos, *slot_scratch;
    uint8_t* cur_mask;
    uint64_t* rng;                      // [0..1] {seed, frame-step counter}; [2..3] the refill domain {seed ^ REFILL_SALT, refill counter} (rng_slot)
    uint64_t* rng_slot;
    // per-slot sampling table (csm_slot_sampling_set): one entry per batch slot, read by every sampler of the slot's row.  The
    // launches get the pointer only once the handle has set an entry (slot_tab_used); until then they get nullptr and every captured
    // frame step is node for node what it is without the table -- the rule of the inject node
    SlotSampling* slot_tab;             // [max_batch]
    bool slot_tab_used = false;
    std::vector<unsigned char> slot_tab_host;   // [max_batch] host mirror for csm_describe: bit 0 = has an entry, bit 1 = own seed
    int* frame_save;                    // [ncb] slot 0's newest frame while a slot refill's depth pass uses scratch row 0
    // refill beside the frame loop (csm_refill_begin / csm_refill_advance): a prompt runs a few backbone layers per call between frame
    // steps; its residual stream and the next layer's normalised input live in buffers of their own, everything else is transient
    int* fresh;                         // [max_batch] device flags: the slot's next frame step yields its frame 0 from rf_last
    bf16_t *rf_h = nullptr, *rf_xn = nullptr, *rf_last = nullptr;     // [max_rows][d_bb] x 2, [max_batch][2 d_bb] final-normed last prompt row per slot (dec_in
                                        // layout).  Made together by the handle's first begin call (refill_buffers): all three or none
    std::vector<char> rf_fresh_host;    // [max_batch] host mirror of `fresh` == 1: slots whose completed refill waits for a frame step to sample its
    int rf_fresh_count = 0;             // frame 0 -- several can wait at once (a generator fills B slots before the first step: ADVICE r5)
    RefillRec rf = {};                  // (nothing pending) the pending refill, one slot (csm_refill_begin) or a group in one ragged prefill (csm_refill_group_begin): rag_segs.h
    int* rg_row_slot = nullptr;         // [max_rows] batch slot of each of the group's rows        } written by k_rag_plan at begin; made together
    int4* rg_tiles = nullptr;           // [max_rows / 32 + 32] {slot, first row, rows, -} by walk  } by the handle's first group begin: both or none
    int device = 0;                     // the GPU this handle lives on (csm_generate_frame_s1 makes it current itself)
    int host_frames = 0;                // frames launched since reset (host mirror); the history is a ring of max_frames rows
    int wide_path;                      // MFMA path for M >= wide_min (env CSM_WIDE=0 disables)
    int wide_min;                       // WIDE_MIN_ROWS unless env CSM_WIDE_MIN overrides (tuning knob)
    int xpack;                          // batched decode steps keep activations in operand order (env CSM_XPACK=0 disables)
    int xpack_prompt;                   // prompts below the LDS-tiled kernels' row count too (env CSM_XPACK_PROMPT=0 disables)
    int fp8_wide;                       // fp8 mode: batched decode steps stream e4m3 on the matrix-core path too (env CSM_FP8_WIDE=0 disables)
    int fuse_dec_attn;                  // depth-decoder attention fused into the O-projection (env CSM_FUSE_DEC_ATTN=0 disables)
    // persistent depth decoder (dec_persist.cuh): steps 2..ncb-1 of a batch-1 frame as one launch (env CSM_PERSIST=0 disables)
    bool persist = false;
    dp_u64 *pg_q, *pg_h1, *pg_h2, *pg_l, *pg_p;
    uint32_t* p_state;                  // [0] tag epoch, [1] give-up code of the last launch (0 = ok), [2] tag epoch of the first-step launch
    // the first decoder step (codebook 1: positions 0, 1) of a batch-1 frame as one launch (dec_first.cuh; env CSM_DEC_FIRST=0 disables)
    bool dec_first = false;
    dp_u64 *fg_q, *fg_h1, *fg_h2, *fg_p;
    // backbone attention block of a batch-1 decode step as one launch per layer (bb_block.cuh)
    bool bb_block = false;
    dp_u64 *bg_q, *bg_a, *bg_s;
    bool bb_layer = false;              // ... and the MLP in the same launch (k_bb_layer)
    dp_u64 *bg_h, *bg_p;
    uint4* b_w2t;                       // [layers] W2 re-tiled, 256 * 4 * 2048 pieces each
    uint4* b_w2t8 = nullptr;            // fp8 mode: [layers] e4m3 W2 re-tiled, 256 * 2 * 2048 pieces each
    bool bb_layer8 = false;             // fp8 mode: the one-launch layer streams the e4m3 bytes (k_bb_layer<true>)
    uint32_t* b_state;                  // [0] tag epoch, [1] give-up code
    uint4 *p_w2s, *p_w13p;              // [4 layers] re-tiled W2 / packed W1|W3, constant layer stride
    bf16_t *p_wsm, *p_norms;            // [4][2560][1024] q|k|v|o rows, [4][2][1024] norm scales
    int p_trickle, p_poll;
    // the same for 2..32 batched utterances (dec_persist_m.cuh; env CSM_PERSIST_M=0 disables)
    bool persist_m = false;
    uint4 *pm_w13, *pm_w2;              // [4 layers] A-operand packed W1 | W3 / W2
    char* pm_xchg;                      // exchange buffers (DM_XCHG_BYTES), 0xFF-filled in front of every launch
    int pm_max_rows;                    // rows up to which the launch is used (env CSM_PERSIST_M_MAX, default 32)
    int pm_trickle;                     // its weight-trickle nap (env CSM_PERSIST_M_TRICKLE; swept 2..16 x poll 0..4 at B = 4 and 32: 4)
    dp_u64* p_stamps = nullptr;         // debug timeline (csm_debug_persist_stamps), else nullptr
    char* xslab = nullptr; size_t xslab_used = 0, xslab_align = 4096;     // the small exchange buffers of the B = 1 all-CU launches live in one 2 MB-aligned slab (placement under our control)
    bool persist_disabled = false, bb_disabled = false;     // a launch gave up once: the chain runs from then on (the buffers stay: error words are still read)
    bool have_last = false;             // prefill or a frame step has produced h for csm_depth
    int last_S = 1;                     // rows per sequence of the h buffer feeding csm_depth
    // captured frame steps: a small LRU keyed on (batch, top-k, temperature, carries the per-slot sampling table) -- a service whose requests alternate sampling parameters or
    // batch sizes (the reference's callers use 0.7/30, 0.8/40 and 0.9/50: tts_service.py:175,266) replays, it does not re-capture
    struct FrameGraph { hipGraphExec_t exec = nullptr; hipGraph_t graph = nullptr; int B = -1, topk = 0; float temp = 0.f; bool tab = false; uint64_t used = 0; };     // tab: carries the per-slot sampling table
    FrameGraph graphs[CSM_FRAME_GRAPHS];
    uint64_t graph_clock = 0;
    int graph_captures = 0;             // hipGraphInstantiate calls since csm_create (csm_debug_graph_captures)
    hipStream_t cap_stream = nullptr;   // capture happens on an internal stream: the caller's may be the legacy NULL stream
    PrefixStore prefixes;
    SessionStore sess;
    std::string err;
};

// One conversation's place in the handle's session store: all state is in m->sess.pages under `id`.
struct CsmSession {
    CsmModel* owner;                    // nullptr once the handle is destroyed: the pages are gone with it
    int id;
};

// A voice prompt's backbone K/V rows [0, rows) of every layer, dense: [layer][K|V][kv head][rows][hd] bf16 (csm_prefix_capture).
struct CsmPrefix {
    CsmModel* owner;                    // the handle it was captured from (nullptr once that handle is destroyed: the snapshot is gone with it)
    int n_layers, kv_heads, hd, rows, device;
    bf16_t* data;
    size_t bytes;
};

// records `msg` as the handle's last error -- without a handle as the calling thread's create error (csm_last_error(nullptr)) -- and returns
// `code`.  Defined once, in csm_engine.hip, beside the one per-thread create-error text of the library.
CSM_LOCAL int fail(CsmModel* h, int code, const char* msg);

#define HIPCHK(h, x)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (x);                                                                 \
        if (e_ != hipSuccess) {                                                              \
            char buf_[256];                                                                  \
            snprintf(buf_, sizeof buf_, "%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
            return fail(h, CSM_E_HIP, buf_);                                                 \
        }                                                                                    \
    } while (0)

// a device allocation the handle owns, optionally with every byte set to `fill`; *p stays null on failure (and the last-error word is clean)
template <class T> static hipError_t dev_get(CsmModel* m, T** p, size_t bytes, int fill = DevPool::NO_FILL) {
    const hipError_t e = (hipError_t)m->pool.get(p, bytes, fill);
    if (e != hipSuccess) (void)hipGetLastError();
    return e;
}

// a refill beside the loop, or a group of them, has begun and not completed / `slot` is (one of) its slot(s)
static inline bool refill_pending(const CsmModel* m) { return refill_pending(m->rf); }
static inline bool slot_refilling(const CsmModel* m, int slot) { return refill_has_slot(m->rf, slot); }

// The stores' two calls from the rest of the handle's life (csm_kv_store.hip).  kv_stores_release (csm_destroy): frees the live prefixes'
// snapshots and orphans their objects, orphans the open sessions, deletes the page bookkeeping; the pool's pages go with the handle's
// allocations.  kv_stores_describe (csm_describe): appends "; prefix_store=...; session_store=...; session_forgets=..." to *t.
CSM_LOCAL void kv_stores_release(CsmModel* m);
CSM_LOCAL void kv_stores_describe(const CsmModel* m, std::string* t);
