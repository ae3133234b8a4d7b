// The two K/V stores of a CSM handle -- the prefix store (csm_prefix_*) and the session store (csm_session_*) of include/csm_hip.h -- with
// their copy kernels.  A translation unit of its own: it needs the handle (csm_model.h) and the page bookkeeping, and none of the GEMV,
// matrix, attention, sampler or persistent kernels that csm_engine.hip instantiates, so an edit here compiles in seconds.
#include <algorithm>

#include "csm_model.h"
#include "session_pages.h"

// ---------------------------------------------------------------------------------------
// prefix store: K/V snapshots of prompt prefixes (the reference re-runs the whole 900-1,550-row voice prompt for every sentence,
// tts_service.py:191-207).  The backbone cache is [L][B][KV][cache_len][hd], so rows [0, rows) of one slot are L * 2 * KV runs of
// rows * hd contiguous elements; a snapshot keeps the runs back to back.  One launch moves every run of every listed slot: grid =
// (pieces of a run, run, slot), 16 B per lane, four independent loads in flight per lane before the first store.  The slot list
// travels in the kernel arguments (max_batch <= 256), so an apply needs neither a host-to-device copy nor a synchronisation.
// ---------------------------------------------------------------------------------------
#define PREFIX_VECS_PER_BLOCK (256 * 4)
struct PrefixSlots { unsigned short s[256]; };

template <bool APPLY>
__global__ __launch_bounds__(256) void k_prefix_copy(bf16_t* kc, bf16_t* vc, bf16_t* snap, long run_vecs, int kv_heads, long layer_stride,
                                                     long slot_stride, long head_stride, PrefixSlots sl) {
    const int run = blockIdx.y, kvh = run % kv_heads, which = (run / kv_heads) & 1, l = run / (2 * kv_heads);
    const long slot = sl.s[blockIdx.z];
    uint4* c = (uint4*)((which ? vc : kc) + (long)l * layer_stride + slot * slot_stride + (long)kvh * head_stride);
    uint4* s = (uint4*)snap + (long)run * run_vecs;
    const long i0 = (long)blockIdx.x * PREFIX_VECS_PER_BLOCK + threadIdx.x;
    uint4 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long i = i0 + j * 256;
        if (i < run_vecs) v[j] = APPLY ? s[i] : c[i];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long i = i0 + j * 256;
        if (i < run_vecs) { if (APPLY) c[i] = v[j]; else s[i] = v[j]; }
    }
}

static hipError_t launch_prefix_copy(CsmModel* m, const CsmPrefix* p, const PrefixSlots& sl, int n, bool apply, hipStream_t st) {
    const Stack& S = m->bb;
    const long run_vecs = (long)p->rows * p->hd / 8;
    const long head_stride = (long)S.cache_len * S.hd, slot_stride = (long)S.d.n_kv_heads * head_stride;
    const dim3 grid((unsigned)((run_vecs + PREFIX_VECS_PER_BLOCK - 1) / PREFIX_VECS_PER_BLOCK), (unsigned)(p->n_layers * 2 * p->kv_heads), (unsigned)n);
    if (apply) hipLaunchKernelGGL(k_prefix_copy<true>, grid, dim3(256), 0, st, S.kc, S.vc, p->data, run_vecs, p->kv_heads, S.layer_stride, slot_stride, head_stride, sl);
    else hipLaunchKernelGGL(k_prefix_copy<false>, grid, dim3(256), 0, st, S.kc, S.vc, p->data, run_vecs, p->kv_heads, S.layer_stride, slot_stride, head_stride, sl);
    return hipGetLastError();
}

extern "C" int csm_prefix_capture(csm_handle m, int slot, int rows, csm_prefix* out, void* stream) {
    if (!m || !out) return fail(m, CSM_E_INVALID, "csm_prefix_capture: null argument");
    if (slot < 0 || slot >= m->max_batch || rows < 1 || rows >= m->cfg.backbone.max_seq) return fail(m, CSM_E_INVALID, "csm_prefix_capture: slot outside the batch or rows outside [1, max_seq)");
    if (slot_refilling(m, slot)) return fail(m, CSM_E_STATE, "csm_prefix_capture: the slot's refill beside the frame loop is still running (csm_refill_advance)");
    hipStream_t st = (hipStream_t)stream;
    int pos = 0;
    HIPCHK(m, hipMemcpyAsync(&pos, m->cur_pos + slot, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(m, hipStreamSynchronize(st));
    if (rows > pos) return fail(m, CSM_E_INVALID, "csm_prefix_capture: rows beyond the slot's position (those rows have not been written)");
    CsmPrefix* p = new CsmPrefix();
    p->owner = m; p->n_layers = m->cfg.backbone.n_layers; p->kv_heads = m->cfg.backbone.n_kv_heads; p->hd = m->bb.hd; p->rows = rows; p->device = m->device;
    p->bytes = (size_t)p->n_layers * 2 * p->kv_heads * rows * p->hd * 2;
    hipError_t e = hipMalloc((void**)&p->data, p->bytes);
    if (e == hipSuccess) {
        PrefixSlots sl; sl.s[0] = (unsigned short)slot;
        e = launch_prefix_copy(m, p, sl, 1, false, st);
        if (e != hipSuccess) (void)hipFree(p->data);
    }
    if (e != hipSuccess) { delete p; HIPCHK(m, e); }
    m->prefixes.live.push_back(p);
    *out = p;
    return CSM_OK;
}

extern "C" int csm_prefix_apply(csm_handle m, csm_prefix p, const int32_t* slots, int n, void* stream) {
    if (!m || !p || !slots || n < 0 || n > m->max_batch) return fail(m, CSM_E_INVALID, "csm_prefix_apply: bad argument");
    if (!p->data) return fail(m, CSM_E_INVALID, "csm_prefix_apply: the handle this prefix was captured from has been destroyed");
    if (p->n_layers != m->cfg.backbone.n_layers || p->kv_heads != m->cfg.backbone.n_kv_heads || p->hd != m->bb.hd || p->device != m->device)
        return fail(m, CSM_E_INVALID, "csm_prefix_apply: the prefix comes from a handle of another shape (layers / kv heads / head_dim) or another GPU");
    if (p->rows >= m->cfg.backbone.max_seq) return fail(m, CSM_E_INVALID, "csm_prefix_apply: the prefix has max_seq rows or more");
    PrefixSlots sl;
    for (int i = 0; i < n; ++i) {
        if (slots[i] < 0 || slots[i] >= m->max_batch) return fail(m, CSM_E_INVALID, "csm_prefix_apply: slot outside the batch");
        if (slot_refilling(m, slots[i])) return fail(m, CSM_E_STATE, "csm_prefix_apply: the slot's refill beside the frame loop is still running (csm_refill_advance)");
        sl.s[i] = (unsigned short)slots[i];
    }
    if (n == 0) return CSM_OK;
    HIPCHK(m, launch_prefix_copy(m, p, sl, n, true, (hipStream_t)stream));
    return CSM_OK;
}

extern "C" int csm_prefix_rows(csm_prefix p) { return p ? p->rows : 0; }
extern "C" size_t csm_prefix_bytes(csm_prefix p) { return p ? p->bytes : 0; }

extern "C" int csm_prefix_read(csm_prefix p, void* host_buf, size_t bytes, void* stream) {
    if (!p || !host_buf || bytes != p->bytes) return fail(p ? p->owner : nullptr, CSM_E_INVALID, "csm_prefix_read: null argument or bytes != csm_prefix_bytes");
    if (!p->data) return fail(nullptr, CSM_E_INVALID, "csm_prefix_read: the handle this prefix was captured from has been destroyed");
    HIPCHK(p->owner, hipMemcpyAsync(host_buf, p->data, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(p->owner, hipStreamSynchronize((hipStream_t)stream));
    return CSM_OK;
}

extern "C" void csm_prefix_destroy(csm_prefix p) {
    if (!p) return;
    if (p->owner) {
        auto& v = p->owner->prefixes.live;
        v.erase(std::remove(v.begin(), v.end(), p), v.end());
    }
    if (p->data) (void)hipFree(p->data);
    delete p;
}

// ---------------------------------------------------------------------------------------
// session store: a conversation's backbone K/V carried from turn to turn.  The prefix store snapshots a slot into a dense
// allocation of its own -- right once per voice, wrong once per turn between two frame steps (an allocation, a synchronisation, every row
// copied again).  Here the rows live in fixed-size pages of ONE pool allocated at csm_session_store_create: a page holds page_rows rows
// of each of the L * 2 * KV runs of a slot's cache, [run][page_rows][hd] -- at CSM-1B with 64 rows 8 KB per run, 2 MB per page.  A save
// appends only the rows the session does not hold; a load gathers the pages of up to 32 sessions into as many slots in one launch.
// The page lists reach the kernels through a device table [session id][logical page] that the SAVE writes from its kernel arguments
// (k_session_tab, <= 256 entries per launch) ahead of the copy; the load passes (session id, slot, rows) per pair in its arguments and
// reads the table.  So save, load and truncate allocate nothing, copy nothing from the host and never synchronise, and a page that a
// truncate or close gives back may go to the next save at once: everything that still reads it was enqueued earlier on the one stream.
// Both copies are k_prefix_copy's: 16 B per lane, four independent loads in flight per lane before the first store, indexed by the
// position in the slot's run (each lane finds its own page: neighbouring lanes share it, the table entry comes from the cache).
// ---------------------------------------------------------------------------------------
#define SESS_VECS_PER_BLOCK (256 * 4)
#define SESS_TAB_PER_LAUNCH 256
#define SESS_MAX_LOAD 32
struct SessTabEntries { int page[SESS_TAB_PER_LAUNCH]; };
struct SessLoadPairs { int id[SESS_MAX_LOAD], slot[SESS_MAX_LOAD], rows[SESS_MAX_LOAD]; };
struct SessGeom { long layer_stride, slot_stride, head_stride; int kv_heads, n_runs, page_rows, hv; };     // hv: 16-byte pieces per row (hd / 8)

__global__ __launch_bounds__(SESS_TAB_PER_LAUNCH) void k_session_tab(int* tab_row, int first, int n, SessTabEntries e) {
    if ((int)threadIdx.x < n) tab_row[first + threadIdx.x] = e.page[threadIdx.x];
}

// pieces [i0 + j * 256 (j < 4)) below `end` of run `run` of one slot <-> the session's pages; i counts 16-byte pieces from the run's row 0
template <bool LOAD>
__device__ __forceinline__ void session_copy(uint4* c, uint4* pool, const int* tab_row, const SessGeom& g, int run, long i0, long end) {
    const long page_vecs = (long)g.page_rows * g.hv;
    uint4* pp[4];
    uint4 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long i = i0 + j * 256;
        if (i < end) {
            const long lp = i / page_vecs;
            pp[j] = pool + ((long)tab_row[lp] * g.n_runs + run) * page_vecs + (i - lp * page_vecs);
            v[j] = LOAD ? *pp[j] : c[i];
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long i = i0 + j * 256;
        if (i < end) { if (LOAD) c[i] = v[j]; else *pp[j] = v[j]; }
    }
}

__device__ __forceinline__ uint4* session_run(bf16_t* kc, bf16_t* vc, const SessGeom& g, int run, long slot) {
    const int kvh = run % g.kv_heads, which = (run / g.kv_heads) & 1, l = run / (2 * g.kv_heads);
    return (uint4*)((which ? vc : kc) + (long)l * g.layer_stride + slot * g.slot_stride + (long)kvh * g.head_stride);
}

// slot rows [from, to) -> the session's pages.  grid = (pieces of the range, run)
__global__ __launch_bounds__(256) void k_session_save(bf16_t* kc, bf16_t* vc, bf16_t* pool, const int* tab_row, SessGeom g, int slot, int from, int to) {
    const int run = blockIdx.y;
    session_copy<false>(session_run(kc, vc, g, run, slot), (uint4*)pool, tab_row, g, run,
                        (long)from * g.hv + (long)blockIdx.x * SESS_VECS_PER_BLOCK + threadIdx.x, (long)to * g.hv);
}

// the pages of pair z's session -> rows [0, rows[z]) of slot[z], all pairs in one launch.  grid = (pieces of the longest, run, pair)
__global__ __launch_bounds__(256) void k_session_load(bf16_t* kc, bf16_t* vc, bf16_t* pool, const int* tab, int tab_stride, SessGeom g, SessLoadPairs a) {
    const int run = blockIdx.y, z = blockIdx.z;
    const long end = (long)a.rows[z] * g.hv, b0 = (long)blockIdx.x * SESS_VECS_PER_BLOCK;
    if (b0 >= end) return;                                      // (a shorter session of the group)
    session_copy<true>(session_run(kc, vc, g, run, a.slot[z]), (uint4*)pool, tab + (long)a.id[z] * tab_stride, g, run, b0 + threadIdx.x, end);
}

// csm_session_forget: the session's rows [first, rows) rewritten into fresh pages without its old rows [from, from + d).  New row r < from is
// old row r; new row r >= from is old row r + d, verbatim in V runs and with its keys rotated BACK by d positions in K runs (K is stored
// rotated; rot[j] = (cos, sin)(d * theta_j), so a pair (x0, x1) becomes (x0 c + x1 s, x1 c - x0 s)): fp32 on the bf16 values, multiplies and
// adds kept apart as in dp_rope_pair so that they equal torch's bit for bit, one rounding to bf16.  old_row: the session's table row (still
// the old page list: it is rewritten after this launch), new_row: the staging row.  k_session_load's shape: 16 B per lane, four
// independent loads in flight per lane before the first store; grid = (pieces of the rewritten range, run).  rot is staged into LDS
// while the loads fly (a lane-varying index into kernel arguments would go to scratch).
#define SESS_ROT_MAX 64                 // head_dim / 2 at head_dim 128
struct SessRot { float cs[SESS_ROT_MAX][2]; };
__device__ __forceinline__ uint32_t session_unrope_pair(uint32_t w, float2 cs) {
#pragma clang fp contract(off)
    const float x0 = lo2f(w), x1 = hi2f(w);
    const float o0 = x0 * cs.x + x1 * cs.y;
    const float o1 = x1 * cs.x - x0 * cs.y;
    return pack_bf(o0, o1);
}
__global__ __launch_bounds__(256) void k_session_forget(bf16_t* pool_, const int* old_row, const int* new_row, SessGeom g, int first, int from, int d, int rows, int n_rot, SessRot rot) {
    __shared__ float2 lrot[SESS_ROT_MAX];
    uint4* pool = (uint4*)pool_;
    const int run = blockIdx.y;
    const bool is_k = ((run / g.kv_heads) & 1) == 0;
    const long page_vecs = (long)g.page_rows * g.hv, end = (long)rows * g.hv, moved_from = (long)from * g.hv;
    const long i0 = (long)first * g.hv + (long)blockIdx.x * SESS_VECS_PER_BLOCK + threadIdx.x;
    uint4* pp[4];
    uint4 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long i = i0 + j * 256;
        if (i < end) {
            const long si = i >= moved_from ? i + (long)d * g.hv : i, sp = si / page_vecs, lp = i / page_vecs;
            v[j] = pool[((long)old_row[sp] * g.n_runs + run) * page_vecs + (si - sp * page_vecs)];
            pp[j] = pool + ((long)new_row[lp] * g.n_runs + run) * page_vecs + (i - lp * page_vecs);
        }
    }
    if (is_k) {                                                 // (uniform over the block)
        if (threadIdx.x == 0) {
#pragma unroll
            for (int j = 0; j < SESS_ROT_MAX; ++j)
                if (j < n_rot) lrot[j] = make_float2(rot.cs[j][0], rot.cs[j][1]);
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long i = i0 + j * 256;
            if (i < end && i >= moved_from) {
                const int p = (int)(i % g.hv) * 4;              // the row's pair index of this piece's first pair
                v[j].x = session_unrope_pair(v[j].x, lrot[p]);     v[j].y = session_unrope_pair(v[j].y, lrot[p + 1]);
                v[j].z = session_unrope_pair(v[j].z, lrot[p + 2]); v[j].w = session_unrope_pair(v[j].w, lrot[p + 3]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (i0 + j * 256 < end) *pp[j] = v[j];
}

static SessGeom session_geom(const CsmModel* m) {
    const Stack& S = m->bb;
    SessGeom g;
    g.head_stride = (long)S.cache_len * S.hd; g.slot_stride = (long)S.d.n_kv_heads * g.head_stride; g.layer_stride = S.layer_stride;
    g.kv_heads = S.d.n_kv_heads; g.n_runs = S.d.n_layers * 2 * S.d.n_kv_heads; g.page_rows = m->sess.pages->page_rows(); g.hv = S.hd / 8;
    return g;
}

static bool session_live(const CsmModel* m, const CsmSession* s) {     // by address: a closed session's object is gone and is never read
    return s && std::find(m->sess.open.begin(), m->sess.open.end(), s) != m->sess.open.end();
}

extern "C" int csm_session_store_create(csm_handle m, int n_pages, int page_rows) {
    if (!m) return fail(m, CSM_E_INVALID, "csm_session_store_create: null handle");
    if (m->sess.pages) return fail(m, CSM_E_STATE, "csm_session_store_create: this handle has a session store already");
    const Stack& S = m->bb;
    if (n_pages < 1 || page_rows < 1 || page_rows > S.cache_len || S.hd % 8 != 0) return fail(m, CSM_E_INVALID, "csm_session_store_create: n_pages >= 1, 1 <= page_rows <= max_seq, head_dim % 8 == 0 required");
    const size_t page_bytes = (size_t)S.d.n_layers * 2 * S.d.n_kv_heads * page_rows * S.hd * 2;
    const int stride = (S.cache_len + page_rows - 1) / page_rows, max_sessions = n_pages + 32;
    const size_t mark = m->pool.mark();
    hipError_t e = dev_get(m, &m->sess.pool, page_bytes * (size_t)n_pages);
    if (e == hipSuccess) e = dev_get(m, &m->sess.tab, (size_t)(max_sessions + 1) * stride * sizeof(int), 0);     // (+ 1: csm_session_forget's staging row)
    if (e != hipSuccess) { m->pool.release_to(mark); m->sess.pool = nullptr; m->sess.tab = nullptr; HIPCHK(m, e); }
    m->sess.tab_stride = stride;
    m->sess.pages = new SessionPages(n_pages, page_rows, max_sessions);
    return CSM_OK;
}

extern "C" int csm_session_open(csm_handle m, csm_session* out) {
    if (!m || !out) return fail(m, CSM_E_INVALID, "csm_session_open: null argument");
    if (!m->sess.pages) return fail(m, CSM_E_STATE, "csm_session_open: no session store (csm_session_store_create)");
    const int id = m->sess.pages->open();
    if (id < 0) return fail(m, CSM_E_STATE, "csm_session_open: too many open sessions (pages + 32)");
    CsmSession* s = new CsmSession{m, id};
    m->sess.open.push_back(s);
    *out = s;
    return CSM_OK;
}

// entries [first, end) of a table row from the session's page list, <= 256 per launch
static hipError_t session_tab_write(CsmModel* m, int id, int* tab_row, int first, int end, hipStream_t st) {
    hipError_t e = hipSuccess;
    for (; first < end && e == hipSuccess; first += SESS_TAB_PER_LAUNCH) {
        SessTabEntries te;
        const int n = std::min(end - first, SESS_TAB_PER_LAUNCH);
        for (int k = 0; k < n; ++k) te.page[k] = m->sess.pages->page_at(id, first + k);
        hipLaunchKernelGGL(k_session_tab, dim3(1), dim3(SESS_TAB_PER_LAUNCH), 0, st, tab_row, first, n, te);
        e = hipGetLastError();
    }
    return e;
}

extern "C" int csm_session_save(csm_handle m, csm_session s, int slot, int rows, void* stream) {
    if (!m || !m->sess.pages) return fail(m, m ? CSM_E_STATE : CSM_E_INVALID, "csm_session_save: null handle or no session store");
    if (!session_live(m, s)) return fail(m, CSM_E_INVALID, "csm_session_save: not an open session of this handle");
    const int from = m->sess.pages->rows(s->id);
    if (slot < 0 || slot >= m->max_batch || rows < from || rows >= m->cfg.backbone.max_seq)
        return fail(m, CSM_E_INVALID, "csm_session_save: slot outside the batch, rows below the session's row count, or rows >= max_seq");
    if (slot_refilling(m, slot)) return fail(m, CSM_E_STATE, "csm_session_save: the slot's refill beside the frame loop is still running (csm_refill_advance)");
    if (rows == from) return CSM_OK;
    const int had_pages = m->sess.pages->pages(s->id);
    if (!m->sess.pages->grow_to(s->id, rows)) return fail(m, CSM_E_NO_PAGES, "csm_session_save: the pool has too few free pages (truncate or close a session and call again)");
    hipStream_t st = (hipStream_t)stream;
    int* tab_row = m->sess.tab + (long)s->id * m->sess.tab_stride;
    hipError_t e = session_tab_write(m, s->id, tab_row, had_pages, m->sess.pages->pages(s->id), st);     // the new pages' table entries, ahead of the copy
    if (e == hipSuccess) {
        const SessGeom g = session_geom(m);
        const long vecs = (long)(rows - from) * g.hv;
        hipLaunchKernelGGL(k_session_save, dim3((unsigned)((vecs + SESS_VECS_PER_BLOCK - 1) / SESS_VECS_PER_BLOCK), (unsigned)g.n_runs), dim3(256), 0, st,
                           m->bb.kc, m->bb.vc, m->sess.pool, (const int*)tab_row, g, slot, from, rows);
        e = hipGetLastError();
    }
    if (e != hipSuccess) { (void)m->sess.pages->truncate(s->id, from); HIPCHK(m, e); }
    return CSM_OK;
}

extern "C" int csm_session_load(csm_handle m, const csm_session* ss, const int32_t* slots, int n, void* stream) {
    if (!m || !m->sess.pages) return fail(m, m ? CSM_E_STATE : CSM_E_INVALID, "csm_session_load: null handle or no session store");
    if (!ss || !slots || n < 0 || n > SESS_MAX_LOAD) return fail(m, CSM_E_INVALID, "csm_session_load: null argument or n outside [0, 32]");
    SessLoadPairs a;
    int longest = 0;
    for (int i = 0; i < n; ++i) {
        if (!session_live(m, ss[i])) return fail(m, CSM_E_INVALID, "csm_session_load: not an open session of this handle");
        if (slots[i] < 0 || slots[i] >= m->max_batch) return fail(m, CSM_E_INVALID, "csm_session_load: slot outside the batch");
        for (int j = 0; j < i; ++j)
            if (slots[j] == slots[i]) return fail(m, CSM_E_INVALID, "csm_session_load: a slot is listed twice");
        if (slot_refilling(m, slots[i])) return fail(m, CSM_E_STATE, "csm_session_load: the slot's refill beside the frame loop is still running (csm_refill_advance)");
        a.id[i] = ss[i]->id; a.slot[i] = slots[i]; a.rows[i] = m->sess.pages->rows(ss[i]->id);
        longest = std::max(longest, a.rows[i]);
    }
    if (longest == 0) return CSM_OK;
    const SessGeom g = session_geom(m);
    const long vecs = (long)longest * g.hv;
    hipLaunchKernelGGL(k_session_load, dim3((unsigned)((vecs + SESS_VECS_PER_BLOCK - 1) / SESS_VECS_PER_BLOCK), (unsigned)g.n_runs, (unsigned)n), dim3(256), 0,
                       (hipStream_t)stream, m->bb.kc, m->bb.vc, m->sess.pool, (const int*)m->sess.tab, m->sess.tab_stride, g, a);
    HIPCHK(m, hipGetLastError());
    return CSM_OK;
}

extern "C" int csm_session_forget(csm_handle m, csm_session s, int from, int to, const float* rot, void* stream) {
    if (!m || !m->sess.pages) return fail(m, m ? CSM_E_STATE : CSM_E_INVALID, "csm_session_forget: null handle or no session store");
    if (!session_live(m, s)) return fail(m, CSM_E_INVALID, "csm_session_forget: not an open session of this handle");
    const int had = m->sess.pages->rows(s->id), hd = m->bb.hd;
    if (from < 0 || to < from || to > had) return fail(m, CSM_E_INVALID, "csm_session_forget: 0 <= from <= to <= the session's row count required");
    if (from == to) return CSM_OK;
    if (!rot || (hd != 64 && hd != 128)) return fail(m, CSM_E_INVALID, "csm_session_forget: null rotation table, or a head_dim other than 64 or 128");
    SessRot r;
    for (int j = 0; j < hd / 2; ++j) { r.cs[j][0] = rot[2 * j]; r.cs[j][1] = rot[2 * j + 1]; }
    for (int j = hd / 2; j < SESS_ROT_MAX; ++j) { r.cs[j][0] = 1.f; r.cs[j][1] = 0.f; }
    const int rc = m->sess.pages->forget(s->id, from, to);
    if (rc == SessionPages::FORGET_NO_PAGES) return fail(m, CSM_E_NO_PAGES, "csm_session_forget: the pool has too few free pages for the rewritten rows (truncate or close a session and call again)");
    if (rc != SessionPages::FORGET_OK) return fail(m, CSM_E_INVALID, "csm_session_forget: refused by the page bookkeeping");
    const SessGeom g = session_geom(m);
    const int k0 = from / g.page_rows, first = k0 * g.page_rows, rows = m->sess.pages->rows(s->id), pages = m->sess.pages->pages(s->id);
    hipStream_t st = (hipStream_t)stream;
    int* tab_row = m->sess.tab + (long)s->id * m->sess.tab_stride;
    int* stage_row = m->sess.tab + (long)m->sess.pages->max_sessions() * m->sess.tab_stride;
    hipError_t e = hipSuccess;
    if (rows > first) {                                         // the new page list into the staging row, the copy (it reads the old list in the session's row), then the session's row
        e = session_tab_write(m, s->id, stage_row, k0, pages, st);
        if (e == hipSuccess) {
            const long vecs = (long)(rows - first) * g.hv;
            hipLaunchKernelGGL(k_session_forget, dim3((unsigned)((vecs + SESS_VECS_PER_BLOCK - 1) / SESS_VECS_PER_BLOCK), (unsigned)g.n_runs), dim3(256), 0, st,
                               m->sess.pool, (const int*)tab_row, (const int*)stage_row, g, first, from, to - from, rows, hd / 2, r);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = session_tab_write(m, s->id, tab_row, k0, pages, st);
    }
    if (e != hipSuccess) { (void)m->sess.pages->truncate(s->id, first); HIPCHK(m, e); }       // (the kept pages below `first` are whole and untouched)
    m->sess.forgets += 1; m->sess.forget_moved += rows - from;
    return CSM_OK;
}

extern "C" int csm_session_truncate(csm_session s, int rows) {
    if (!s || !s->owner) return fail(nullptr, CSM_E_INVALID, "csm_session_truncate: null session, or its handle has been destroyed");
    if (!s->owner->sess.pages->truncate(s->id, rows)) return fail(s->owner, CSM_E_INVALID, "csm_session_truncate: rows outside [0, the session's row count]");
    return CSM_OK;
}

extern "C" int csm_session_rows(csm_session s) { return s && s->owner ? s->owner->sess.pages->rows(s->id) : 0; }
extern "C" int csm_session_pages(csm_session s) { return s && s->owner ? s->owner->sess.pages->pages(s->id) : 0; }

extern "C" int csm_session_read(csm_session s, void* host_buf, size_t bytes, void* stream) {
    if (!s || !s->owner) return fail(nullptr, CSM_E_INVALID, "csm_session_read: null session, or its handle has been destroyed");
    CsmModel* m = s->owner;
    const SessGeom g = session_geom(m);
    const int rows = m->sess.pages->rows(s->id);
    const size_t row_bytes = (size_t)g.hv * 16, page_run_bytes = row_bytes * g.page_rows;
    if (bytes != row_bytes * rows * g.n_runs || (!host_buf && bytes)) return fail(m, CSM_E_INVALID, "csm_session_read: bytes != layers * 2 * kv heads * rows * head_dim * 2, or a null buffer");
    std::vector<SessionCopy> plan;
    (void)m->sess.pages->plan(s->id, 0, rows, &plan);
    for (const SessionCopy& c : plan)                       // one strided copy per page: the page's piece of every run
        HIPCHK(m, hipMemcpy2DAsync((char*)host_buf + c.slot_row * row_bytes, row_bytes * rows,
                                   (const char*)m->sess.pool + (size_t)c.page * g.n_runs * page_run_bytes + c.page_row * row_bytes, page_run_bytes,
                                   c.rows * row_bytes, (size_t)g.n_runs, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(m, hipStreamSynchronize((hipStream_t)stream));
    return CSM_OK;
}

extern "C" void csm_session_close(csm_session s) {
    if (!s) return;
    if (s->owner) {
        s->owner->sess.pages->close(s->id);
        auto& v = s->owner->sess.open;
        v.erase(std::remove(v.begin(), v.end(), s), v.end());
    }
    delete s;
}

// ---------------------------------------------------------------------------------------
// the stores' part of csm_destroy and csm_describe
// ---------------------------------------------------------------------------------------
void kv_stores_release(CsmModel* m) {
    for (CsmPrefix* p : m->prefixes.live) { (void)hipFree(p->data); p->data = nullptr; p->owner = nullptr; }      // (the caller still destroys the objects)
    for (CsmSession* s : m->sess.open) s->owner = nullptr;                                                    // (likewise: they can only be closed now)
    delete m->sess.pages;
}

void kv_stores_describe(const CsmModel* m, std::string* t) {
    char tmp[160];
    const SessionPages* sp = m->sess.pages;
    { size_t pb = 0; for (const CsmPrefix* p : m->prefixes.live) pb += p->bytes;
      snprintf(tmp, sizeof tmp, "; prefix_store=%d prefixes, %zu bytes", (int)m->prefixes.live.size(), pb); *t += tmp; }
    snprintf(tmp, sizeof tmp, "; session_store=%d sessions, %d/%d pages", sp ? sp->sessions() : 0, sp ? sp->pages_used() : 0, sp ? sp->pages_total() : 0);
    *t += tmp;
    snprintf(tmp, sizeof tmp, "; session_forgets=%d (%ld rows moved)", m->sess.forgets, m->sess.forget_moved);
    *t += tmp;
}
