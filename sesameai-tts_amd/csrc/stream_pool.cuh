// What the pools of stateful audio streams share in their .hip files (resample, stretch, vad, watermark): the handle's base -- the streams'
// host states, the error text, the owner of its device memory -- with the create ladder, the refusals of the small entry points and the launch
// check; and the one device helper that is theirs alone, the search for the segment that owns a workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "common.cuh"
#include "hip_backend.h"
#include "stream_pool.h"

// The segment that owns this workgroup: the last of seg[0 .. n) (n >= 1, ascending in `first`) whose first workgroup is <= blockIdx.x, in a
// grid whose every workgroup lies in a segment.  Two selects a step, no branch in the loop.
template <class Seg>
__device__ __forceinline__ int sp_owner(const Seg* seg, int n, int Seg::*first) {
    int hi = n - 1, lo = 0;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        const bool up = seg[mid].*first <= (int)blockIdx.x;      // the owner is mid or lies behind it
        hi = up ? hi : mid - 1;
        lo = up ? mid : lo;
    }
    return lo;
}

#pragma GCC visibility push(hidden)      // the rest is host code private to the library: nothing of it enters the dynamic symbol table

// A pool's handle starts with this.  `dev` owns every device allocation of the pool: deleting the pool frees them, nothing else does.
template <class Stream> struct SpPool {
    int n_streams = 0;
    Stream st[SP_MAX_STREAMS] = {};
    std::string err;
    DevPool dev{hip_backend()};
    template <class T> hipError_t get(T** p, size_t bytes, int fill = DevPool::NO_FILL) {
        char* v = nullptr;                                     // (one instantiation of DevPool::get whatever the element type)
        const hipError_t e = (hipError_t)dev.get(&v, bytes, fill);
        *p = (T*)v;
        return e;
    }
};

// why the calling thread's last create of a P failed: one text per pool type
template <class P> std::string& sp_create_err() {
    static thread_local std::string err;
    return err;
}

// The create ladder.  `refused`: what the caller has against its own arguments, reported in its place (after a null `out`, before the pool's
// size).  `init(p)` sets the streams' first states and takes the device memory through p->get: whatever it took is freed if it fails.
template <class P, class Init> int sp_create(const char* api, int n_streams, P** out, const char* refused, Init init) {
    std::string& err = sp_create_err<P>();
    if (!out) { err = "null pointer"; return -1; }
    *out = nullptr;
    if (!refused) refused = sp_size_bad(n_streams);
    if (refused) { err = refused; return -1; }
    P* p = new P();
    p->n_streams = n_streams;
    const hipError_t e = init(p);
    if (e != hipSuccess) {
        err = std::string(api) + ": " + hipGetErrorString(e);
        delete p;
        return -2;
    }
    *out = p;
    return 0;
}

template <class P> const char* sp_last_error(P* p) { return p ? p->err.c_str() : sp_create_err<P>().c_str(); }

// 0, or -1 with the refusal kept for last_error
template <class P> int sp_status(P* p, const char* bad) {
    if (!bad) return 0;
    p->err = bad;
    return -1;
}

// whether *_out_count / *_frame_count may answer for stream sid and a chunk of n_in samples
template <class P> bool sp_count_ok(P* p, int sid, long n_in) {
    if (!p) return false;
    const int32_t id = sid;
    if (sp_status(p, sp_ids_bad(p->n_streams, &id, 1)) != 0) return false;
    return sp_status(p, n_in < 0 || n_in > SP_MAX_CHUNK ? "a chunk of negative length or of more than 2^30 samples" : nullptr) == 0;
}

#define SP_HIP(p, call)                                                                              \
    do {                                                                                             \
        hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess) { (p)->err = std::string(#call) + ": " + hipGetErrorString(e_); return -2; } \
    } while (0)

#pragma GCC visibility pop
