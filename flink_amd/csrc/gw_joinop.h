// gw_joinop.h — the host side of a two-stream operator, shared by the window join (gw_join.hip)
// and the interval join (gw_ijoin.hip): the handle's sticky error, its stream with the hand-off
// from and to a producer's stream, the pending output rows, and the staged ingest of host
// columns.  Small types, no policy beyond what both operators share.  Header-only, HIP runtime +
// standard library, no kernels (tests/native/joinop.cpp runs it on the CPU over tests/native/fake_hip).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <utility>

#include "../../include/gpuwin.h"
#include "gw_devmem.h"

namespace gw {

// The handle's error state.  A bad argument (GW_E_INVALID) and rows left to drain
// (GW_E_OUTPUT_FULL) leave the handle usable; every other error fails it for good.
struct OpError {
    const char* name;  // "window join", "interval join": the prefix of the shared messages
    bool failed = false;
    std::string err;

    __attribute__((format(printf, 3, 4))) int fail(int rc, const char* fmt, ...) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        err = buf;
        if (rc != GW_E_OUTPUT_FULL && rc != GW_E_INVALID) failed = true;
        return rc;
    }
    int dev_fail(hipError_t e) { return fail(GW_E_DEVICE, "%s: %s", name, hipGetErrorString(e)); }
};

// The operator's own stream and the two events of the hand-off.
struct OpStream {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    // *what: the call that failed ("hipSetDevice", "hipStreamCreate", "hipEventCreate").
    hipError_t create(int dev, const char** what) {
        device = dev;
        hipError_t e;
        *what = "hipSetDevice";
        if ((e = hipSetDevice(dev)) != hipSuccess) return e;
        *what = "hipStreamCreate";
        if ((e = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking)) != hipSuccess) return e;
        *what = "hipEventCreate";
        if ((e = hipEventCreateWithFlags(&ev_in, hipEventDisableTiming)) != hipSuccess) return e;
        return hipEventCreateWithFlags(&ev_out, hipEventDisableTiming);
    }
    // Waits for the stream and destroys what create() made, however far it came.
    void destroy() {
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
        if (ev_in) (void)hipEventDestroy(ev_in);
        if (ev_out) (void)hipEventDestroy(ev_out);
        if (stream) (void)hipStreamDestroy(stream);
        stream = nullptr;
        ev_in = ev_out = nullptr;
    }

    // While it lives the operator reads a producer's columns: the operator's stream waits for
    // the producer's work so far, and on every way out the producer's stream waits for the
    // operator's reads.  With the operator's own stream, or with no records (work = false: the
    // operator launches nothing, so neither stream has anything to wait for), it does nothing.
    struct Handoff {
        OpStream& o;
        hipStream_t producer;
        bool active;
        Handoff(OpStream& op, hipStream_t ps, bool work) : o(op), producer(ps), active(work && ps != op.stream) {
            if (!active) return;
            (void)hipEventRecord(o.ev_in, producer);
            (void)hipStreamWaitEvent(o.stream, o.ev_in, 0);
        }
        ~Handoff() {
            if (!active) return;
            (void)hipEventRecord(o.ev_out, o.stream);
            (void)hipStreamWaitEvent(producer, o.ev_out, 0);
        }
        Handoff(const Handoff&) = delete;
    };
};

// In front of every entry point of a handle with members `er` (OpError) and `os` (OpStream).
#define GW_OP_ENTER(h)                       \
    if (!(h)) return GW_E_INVALID;           \
    if ((h)->er.failed) return GW_E_STATE;   \
    (void)hipSetDevice((h)->os.device)

// The output rows that wait for a drain: five int64 columns and, for an operator that has one,
// a byte per row (the window join's `present`).  The pending rows are [from, from + pending);
// new rows go behind them, and a drain in parts moves `from` up.
struct RowBuf {
    bool with_bytes;  // set at construction: RowBuf rows{true}
    DevCols<5> col;
    DevBuf<uint8_t> bytes;
    int64_t from = 0, pending = 0;

    // Where the next rows go (after reserve()): the columns to out, the bytes (or null) returned.
    uint8_t* tail(int64_t* out[5]) const {
        for (int c = 0; c < 5; ++c) out[c] = col[c] + from + pending;
        return bytes.p ? bytes.p + from + pending : nullptr;
    }
    // Room for `more` rows behind the pending ones; growth moves the pending rows to row 0.
    // All or nothing: the new bytes are allocated and filled first and published only after the
    // columns have grown (whose growth synchronises s, so the byte copy is done by then).
    hipError_t reserve(int64_t more, hipStream_t s) {
        if (from + pending + more <= col.cap) return hipSuccess;
        const int64_t cap = std::max<int64_t>(pending + more, 2 * col.cap);
        DevBuf<uint8_t> nb;
        hipError_t e = hipSuccess;
        if (with_bytes) {
            e = nb.reserve_discard(cap);
            if (e == hipSuccess && bytes.p && pending > 0)
                e = hipMemcpyAsync(nb.p, bytes.p + from, (size_t)pending, hipMemcpyDeviceToDevice, s);
        }
        if (e == hipSuccess) e = col.reserve_keep(cap, from, pending, s);
        if (e != hipSuccess) return e;
        if (with_bytes) bytes = std::move(nb);
        from = 0;
        return hipSuccess;
    }
    // Copies min(cap, pending) rows to the host columns (and their bytes, where `present` is not
    // null) and removes them; GW_E_OUTPUT_FULL while rows remain.
    int drain(int64_t* const dst[5], uint8_t* present, int64_t cap, int64_t* n, hipStream_t s, OpError& er) {
        const int64_t m = std::min(cap, pending);
        *n = m;
        hipError_t e = hipSuccess;
        for (int c = 0; c < 5 && m > 0 && e == hipSuccess; ++c)
            e = hipMemcpyAsync(dst[c], col[c] + from, (size_t)m * 8, hipMemcpyDeviceToHost, s);
        if (present && bytes.p && m > 0 && e == hipSuccess)
            e = hipMemcpyAsync(present, bytes.p + from, (size_t)m, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return er.dev_fail(e);
        from += m;
        pending -= m;
        if (pending == 0) from = 0;
        return pending > 0 ? GW_E_OUTPUT_FULL : GW_OK;
    }
    // The pending rows in place; null pointers when there are none.  `present` may be null.
    void view(const int64_t** const ptrs[5], const uint8_t** present, int64_t* n) const {
        for (int c = 0; c < 5; ++c) *ptrs[c] = pending ? col[c] + from : nullptr;
        if (present) *present = pending && bytes.p ? bytes.p + from : nullptr;
        *n = pending;
    }
    void clear() { from = pending = 0; }
};

// n records of three host columns through the operator's device path, max_batch at a time:
// each chunk is copied to `stage` on s and handed to body(m, stage columns) -> GW_* code, which
// waits for s before it returns, so the host columns and `stage` are free for the next chunk.
template <typename Body>
int staged_ingest(DevCols<3>& stage, int64_t max_batch, int64_t n, const int64_t* const src[3], hipStream_t s, OpError& er, Body body) {
    for (int64_t at = 0; at < n; at += max_batch) {
        const int64_t m = std::min(max_batch, n - at);
        if (stage.cap < m && stage.reserve_keep(m, 0, 0, s) != hipSuccess) {
            (void)hipGetLastError();
            return er.fail(GW_E_OOM, "%s: out of device memory staging a batch", er.name);
        }
        for (int c = 0; c < 3; ++c) {
            const hipError_t e = hipMemcpyAsync(stage[c], src[c] + at, (size_t)m * 8, hipMemcpyHostToDevice, s);
            if (e != hipSuccess) return er.dev_fail(e);
        }
        const int rc = body(m, stage.col);
        if (rc) return rc;
    }
    return GW_OK;
}

}  // namespace gw
