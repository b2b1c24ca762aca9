// gw_devmem.h — owners of device and pinned host memory.
//
// Three move-only types and no policy: every caller computes its own new capacity and maps
// the hipError_t to its own error code.  Growth that keeps contents is all-or-nothing: the
// new blocks are allocated and filled before the old ones are freed, so a failure leaves the
// owner exactly as it was and leaks nothing.  Header-only, HIP runtime + standard library
// only (tests/native/devmem.cpp runs it on the CPU against a malloc-backed hip_runtime.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace gw {

// One device allocation of `cap` elements.
template <typename T>
struct DevBuf {
    T* p = nullptr;
    int64_t cap = 0;

    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            reset();
            p = o.p; cap = o.cap;
            o.p = nullptr; o.cap = 0;
        }
        return *this;
    }
    ~DevBuf() { reset(); }

    T* get() const { return p; }
    operator T*() const { return p; }

    void reset() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    // At least n elements, contents not kept: the old block is freed first (the caller
    // synchronises before, where the device may still use it).  Empty after a failure.
    hipError_t reserve_discard(int64_t n) {
        if (n <= cap) return hipSuccess;
        reset();
        hipError_t e = hipMalloc((void**)&p, (size_t)n * sizeof(T));
        if (e != hipSuccess) { p = nullptr; return e; }
        cap = n;
        return hipSuccess;
    }
    // A new block of n elements with [live_from, live_from + live_n) of the old one at its
    // front (live_n <= n), copied on s; s is synchronised before the old block is freed.
    hipError_t reserve_keep(int64_t n, int64_t live_from, int64_t live_n, hipStream_t s) {
        T* nb = nullptr;
        hipError_t e = hipMalloc((void**)&nb, (size_t)n * sizeof(T));
        if (e != hipSuccess) return e;
        if (p && live_n > 0)
            e = hipMemcpyAsync(nb, p + live_from, (size_t)live_n * sizeof(T), hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) { (void)hipFree(nb); return e; }
        if (p) (void)hipFree(p);
        p = nb;
        cap = n;
        return hipSuccess;
    }
};

// N int64 columns of one capacity that grow together.
template <int N>
struct DevCols {
    int64_t* col[N] = {};
    int64_t cap = 0;

    DevCols() = default;
    DevCols(const DevCols&) = delete;
    DevCols& operator=(const DevCols&) = delete;
    DevCols(DevCols&& o) noexcept { take(o); }
    DevCols& operator=(DevCols&& o) noexcept {
        if (this != &o) { reset(); take(o); }
        return *this;
    }
    ~DevCols() { reset(); }

    int64_t* operator[](int i) const { return col[i]; }

    void reset() {
        for (auto& c : col) {
            if (c) (void)hipFree(c);
            c = nullptr;
        }
        cap = 0;
    }
    // DevBuf::reserve_keep over the columns in `mask` (the others stay null): allocate all,
    // copy all, one synchronise, free all old, then publish.
    hipError_t reserve_keep(int64_t n, int64_t live_from, int64_t live_n, hipStream_t s, unsigned mask = ~0u) {
        int64_t* nb[N] = {};
        hipError_t e = hipSuccess;
        for (int i = 0; i < N && e == hipSuccess; ++i)
            if (mask >> i & 1) e = hipMalloc((void**)&nb[i], (size_t)n * 8);
        for (int i = 0; i < N && e == hipSuccess; ++i)
            if (nb[i] && col[i] && live_n > 0)
                e = hipMemcpyAsync(nb[i], col[i] + live_from, (size_t)live_n * 8, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            for (auto* b : nb)
                if (b) (void)hipFree(b);
            return e;
        }
        for (int i = 0; i < N; ++i) {
            if (!(mask >> i & 1)) continue;
            if (col[i]) (void)hipFree(col[i]);
            col[i] = nb[i];
        }
        cap = n;
        return hipSuccess;
    }

private:
    void take(DevCols& o) {
        for (int i = 0; i < N; ++i) { col[i] = o.col[i]; o.col[i] = nullptr; }
        cap = o.cap;
        o.cap = 0;
    }
};

// One hipHostMalloc block of `cap` elements.
template <typename T>
struct PinnedBuf {
    T* p = nullptr;
    int64_t cap = 0;

    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    PinnedBuf(PinnedBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    PinnedBuf& operator=(PinnedBuf&& o) noexcept {
        if (this != &o) {
            reset();
            p = o.p; cap = o.cap;
            o.p = nullptr; o.cap = 0;
        }
        return *this;
    }
    ~PinnedBuf() { reset(); }

    T* get() const { return p; }
    operator T*() const { return p; }
    T* operator->() const { return p; }

    void reset() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
    // A fresh block of n elements (hipHostMallocDefault, hipHostMallocCoherent, ...); the old
    // one is freed first.  Empty after a failure.
    hipError_t alloc(int64_t n, unsigned flags) {
        reset();
        hipError_t e = hipHostMalloc((void**)&p, (size_t)n * sizeof(T), flags);
        if (e != hipSuccess) { p = nullptr; return e; }
        cap = n;
        return hipSuccess;
    }
};

}  // namespace gw
