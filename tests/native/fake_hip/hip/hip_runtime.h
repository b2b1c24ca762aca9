// A malloc-backed stand-in for the part of the HIP runtime that gw_devmem.h uses, so that the
// header's ownership rules run on the CPU (tests/native/devmem.cpp).  Counters in fake_hip::.
#pragma once
#include <cstddef>
#include <cstdlib>
#include <cstring>

typedef int hipError_t;
typedef void* hipStream_t;
enum : hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 };
enum hipMemcpyKind { hipMemcpyDeviceToDevice = 3 };
enum : unsigned { hipHostMallocDefault = 0x0, hipHostMallocCoherent = 0x40000000 };

namespace fake_hip {
inline int fail_in = 0;  // > 0: the fail_in-th allocation from now fails (once)
inline int live = 0;     // blocks allocated and not freed
inline int syncs = 0;    // hipStreamSynchronize calls
inline int allocs = 0;   // successful allocations
inline unsigned last_host_flags = ~0u;

inline hipError_t alloc(void** p, size_t bytes) {
    if (fail_in > 0 && --fail_in == 0) { *p = nullptr; return hipErrorOutOfMemory; }
    *p = malloc(bytes ? bytes : 1);
    ++live;
    ++allocs;
    return hipSuccess;
}
inline hipError_t release(void* p) {
    if (p) --live;
    free(p);
    return hipSuccess;
}
}  // namespace fake_hip

inline hipError_t hipMalloc(void** p, size_t bytes) { return fake_hip::alloc(p, bytes); }
inline hipError_t hipFree(void* p) { return fake_hip::release(p); }
inline hipError_t hipHostMalloc(void** p, size_t bytes, unsigned flags) {
    fake_hip::last_host_flags = flags;
    return fake_hip::alloc(p, bytes);
}
inline hipError_t hipHostFree(void* p) { return fake_hip::release(p); }
inline hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind, hipStream_t) {
    memcpy(dst, src, bytes);
    return hipSuccess;
}
inline hipError_t hipStreamSynchronize(hipStream_t) {
    ++fake_hip::syncs;
    return hipSuccess;
}
