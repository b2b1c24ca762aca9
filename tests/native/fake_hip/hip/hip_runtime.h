// A malloc-backed stand-in for the part of the HIP runtime that the host-only headers use
// (gw_devmem.h, gw_joinop.h), so that their ownership and ordering rules run on the CPU
// (tests/native/devmem.cpp, joinop.cpp).  Counters and a log of stream operations in fake_hip::.
#pragma once
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <vector>

typedef int hipError_t;
typedef void* hipStream_t;
typedef void* hipEvent_t;
enum : hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorInvalidDevice = 101 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2, hipMemcpyDeviceToDevice = 3 };
enum : unsigned { hipHostMallocDefault = 0x0, hipHostMallocCoherent = 0x40000000 };
enum : unsigned { hipStreamNonBlocking = 0x1, hipEventDisableTiming = 0x2 };

namespace fake_hip {
inline int fail_in = 0;  // > 0: the fail_in-th allocation or stream / event creation from now fails (once)
inline int live = 0;     // blocks, streams and events made and not freed or destroyed
inline int syncs = 0;    // hipStreamSynchronize calls
inline int allocs = 0;   // successful allocations and creations
inline unsigned last_host_flags = ~0u;
inline int device = -1;          // the last hipSetDevice
inline int bad_device = -1;      // hipSetDevice of this one fails
inline int copies[4] = {};       // hipMemcpyAsync calls by hipMemcpyKind
inline hipError_t last_error = hipSuccess;  // what hipGetLastError returns and clears

// Stream operations in the order they were issued: 'R' record event `ev` on `stream`, 'W'
// `stream` waits for `ev`, 'S' the host waits for `stream`.
struct Op {
    char kind;
    hipStream_t stream;
    hipEvent_t ev;
};
inline std::vector<Op> log;

inline hipError_t alloc(void** p, size_t bytes) {
    if (fail_in > 0 && --fail_in == 0) { *p = nullptr; return last_error = hipErrorOutOfMemory; }
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
inline hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t) {
    ++fake_hip::copies[kind];
    memcpy(dst, src, bytes);
    return hipSuccess;
}
inline hipError_t hipStreamSynchronize(hipStream_t s) {
    ++fake_hip::syncs;
    fake_hip::log.push_back({'S', s, nullptr});
    return hipSuccess;
}

inline hipError_t hipSetDevice(int d) {
    if (d == fake_hip::bad_device) return fake_hip::last_error = hipErrorInvalidDevice;
    fake_hip::device = d;
    return hipSuccess;
}
inline hipError_t hipGetLastError() {
    const hipError_t e = fake_hip::last_error;
    fake_hip::last_error = hipSuccess;
    return e;
}
inline const char* hipGetErrorString(hipError_t e) {
    return e == hipSuccess ? "no error" : e == hipErrorOutOfMemory ? "out of memory" : "invalid device ordinal";
}
// Streams and events are one-byte blocks: they count in `live`, and fail_in fails their creation.
inline hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { return fake_hip::alloc(s, 1); }
inline hipError_t hipStreamDestroy(hipStream_t s) { return fake_hip::release(s); }
inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return fake_hip::alloc(e, 1); }
inline hipError_t hipEventCreate(hipEvent_t* e) { return fake_hip::alloc(e, 1); }
inline hipError_t hipEventDestroy(hipEvent_t e) { return fake_hip::release(e); }
inline hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
    fake_hip::log.push_back({'R', s, e});
    return hipSuccess;
}
inline hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) {
    fake_hip::log.push_back({'W', s, e});
    return hipSuccess;
}
inline hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) {
    *ms = 0;
    return hipSuccess;
}
