// THE binding of a device-memory owner (dev_pool.h) to HIP: hipMalloc / hipFree / hipMemset.  The CSM handle (csm_model.h) and the pools of
// audio streams (stream_pool.cuh) both allocate through it.  Hidden: one object in the library, none in its dynamic symbol table.
#pragma once
#include <hip/hip_runtime.h>

#include "dev_pool.h"

__attribute__((visibility("hidden"))) inline const DevBackend* hip_backend() {
    static const DevBackend be = {[](void** p, size_t bytes) { return (int)hipMalloc(p, bytes); }, [](void* p) { return (int)hipFree(p); },
                                  [](void* p, int byte, size_t bytes) { return (int)hipMemset(p, byte, bytes); }};
    return &be;
}
