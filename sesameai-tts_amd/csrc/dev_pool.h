// The device allocations of ONE owner, each freed exactly once.  No HIP here: the allocate / free / fill functions are the user's
// (hip_backend.h binds them to hipMalloc / hipFree / hipMemset in one place; tools/dev_pool_check.cpp drives the pool on the CPU with a
// counting fake).  Status 0 = success.  An optional block is abandoned as a unit: mark(), then release_to(mark).
#pragma once
#include <stddef.h>
#include <vector>

struct DevBackend { int (*alloc)(void** p, size_t bytes); int (*free)(void* p); int (*fill)(void* p, int byte, size_t bytes); };

class DevPool {
    const DevBackend* be_;
    std::vector<void*> live_;           // in allocation order; freed newest first
public:
    enum { NO_FILL = -1 };
    explicit DevPool(const DevBackend* be) : be_(be) {}
    DevPool(const DevPool&) = delete;
    DevPool& operator=(const DevPool&) = delete;
    ~DevPool() { release_all(); }

    // allocate, optionally set every byte to `fill`, register; the backend's status, and *p null unless it is 0
    template <class T> int get(T** p, size_t bytes, int fill = NO_FILL) {
        *p = nullptr;
        void* v = nullptr;
        int rc = be_->alloc(&v, bytes);
        if (rc != 0) return rc;
        if (v == nullptr) return 0;                             // a request of 0 bytes: nothing was handed out, nothing to fill or free
        if (fill != NO_FILL && (rc = be_->fill(v, fill, bytes)) != 0) { (void)be_->free(v); return rc; }
        live_.push_back(v);
        *p = (T*)v;
        return 0;
    }
    size_t mark() const { return live_.size(); }
    void release_to(size_t mark) {                          // frees exactly what was allocated after the mark
        while (live_.size() > mark) { (void)be_->free(live_.back()); live_.pop_back(); }
    }
    void release_all() { release_to(0); }                   // idempotent
};
