// gw_joinutil.h — what the two-stream joins share (gw_join.hip: the window join and coGroup;
// gw_ijoin.hip: the interval join): the two-pass exclusive scan, the wave-wide reductions and
// search of their kernels, the stable compaction of a log, small host helpers (header read-back,
// the expand kernels' alignment test, the timed event pair) and the carved scratch; the operators'
// host side is gw_joinop.h.  Each including file gets its own copy of the kernels (static, or
// template instances), so nothing here is a link-time symbol.
#pragma once
#include <algorithm>
#include <string>

#include "gw_devmem.h"
#include "gw_joinop.h"
#include "gw_kernels.h"

namespace gw {

constexpr int kJoinThreads = 256;
constexpr int kJoinMaxBlocks = 2048;  // grid-stride kernels that end in a few atomics per block

GW_HD uint64_t join_key_word(int64_t key) { return (uint64_t)key ^ 0x8000000000000000ull; }

// ---- scans --------------------------------------------------------------------------------
constexpr int kScanTile = kJoinThreads * 4;

__device__ __forceinline__ int64_t block_scan256(int64_t v, int64_t& total) {
    __shared__ int64_t s_w[4];
    const int lane = __lane_id(), wave = threadIdx.x >> 6;
    int64_t incl = v;
    for (int o = 1; o < 64; o <<= 1) {
        const int64_t up = (int64_t)__shfl_up((long long)incl, o);
        if (lane >= o) incl += up;
    }
    __syncthreads();  // an earlier call's readers are done with s_w
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    int64_t base = 0;
    total = 0;
    for (int w = 0; w < 4; ++w) {
        if (w < wave) base += s_w[w];
        total += s_w[w];
    }
    return base + incl - v;
}

template <typename TIn>
__global__ void __launch_bounds__(kJoinThreads) k_scan_reduce(const TIn* __restrict__ in, int64_t n, int64_t* blk) {
    const int64_t i0 = (int64_t)blockIdx.x * kScanTile + threadIdx.x * 4;
    int64_t v = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (i0 + j < n) v += (int64_t)in[i0 + j];
    int64_t total;
    block_scan256(v, total);
    if (threadIdx.x == 0) blk[blockIdx.x] = total;
}
static __global__ void __launch_bounds__(kJoinThreads) k_scan_blocks(int64_t* blk, int64_t nb, int64_t* total_out) {
    const int64_t per = (nb + kJoinThreads - 1) / kJoinThreads;
    const int64_t lo = std::min<int64_t>(nb, threadIdx.x * per), hi = std::min<int64_t>(nb, lo + per);
    int64_t v = 0;
    for (int64_t i = lo; i < hi; ++i) v += blk[i];
    int64_t total;
    int64_t run = block_scan256(v, total);
    for (int64_t i = lo; i < hi; ++i) {
        const int64_t x = blk[i];
        blk[i] = run;
        run += x;
    }
    if (threadIdx.x == 0) *total_out = total;
}
template <typename TIn, typename TOut>
__global__ void __launch_bounds__(kJoinThreads) k_scan_down(const TIn* __restrict__ in, int64_t n,
                                                             const int64_t* __restrict__ blk, TOut* out) {
    const int64_t i0 = (int64_t)blockIdx.x * kScanTile + threadIdx.x * 4;
    int64_t x[4], v = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        x[j] = i0 + j < n ? (int64_t)in[i0 + j] : 0;
        v += x[j];
    }
    int64_t total;
    int64_t run = blk[blockIdx.x] + block_scan256(v, total);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (i0 + j < n) out[i0 + j] = (TOut)run;
        run += x[j];
    }
}
static int64_t scan_blocks(int64_t n) { return (n + kScanTile - 1) / kScanTile; }
// out[i] = in[0] + ... + in[i - 1]; *total = the sum; blk: scan_blocks(n) words.
template <typename TIn, typename TOut>
static hipError_t scan_excl(const TIn* in, TOut* out, int64_t n, int64_t* blk, int64_t* total, hipStream_t s) {
    const int64_t nb = scan_blocks(n);
    if (nb > 0) hipLaunchKernelGGL(k_scan_reduce<TIn>, dim3((unsigned)nb), dim3(kJoinThreads), 0, s, in, n, blk);
    hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(kJoinThreads), 0, s, blk, nb, total);
    if (nb > 0)
        hipLaunchKernelGGL((k_scan_down<TIn, TOut>), dim3((unsigned)nb), dim3(kJoinThreads), 0, s, in, n, blk, out);
    return hipGetLastError();
}

// ---- wave-wide reductions and search --------------------------------------------------------
__device__ __forceinline__ int64_t wave_min_i64(int64_t v) {
    for (int o = 32; o > 0; o >>= 1) {
        const int64_t x = (int64_t)__shfl_xor((long long)v, o);
        v = x < v ? x : v;
    }
    return v;
}
__device__ __forceinline__ int64_t wave_max_i64(int64_t v) {
    for (int o = 32; o > 0; o >>= 1) {
        const int64_t x = (int64_t)__shfl_xor((long long)v, o);
        v = x > v ? x : v;
    }
    return v;
}
__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t x = (uint64_t)__shfl_xor((unsigned long long)v, o);
        v = x < v ? x : v;
    }
    return v;
}
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t x = (uint64_t)__shfl_xor((unsigned long long)v, o);
        v = x > v ? x : v;
    }
    return v;
}

struct alignas(16) I64x2 {
    int64_t a, b;
};

// One wave: the largest c in [0, nc) with coff[c] <= p (coff[0] = 0 <= p), 64 probes a round.
__device__ __forceinline__ int64_t wave_search(const int64_t* __restrict__ coff, int64_t nc, int64_t p) {
    const int lane = __lane_id();
    int64_t lo = 0, hi = nc;
    while (hi - lo > 1) {
        const int64_t step = (hi - lo + 63) / 64;
        const int64_t idx = lo + lane * step;
        const bool ok = idx < hi && coff[idx] <= p;
        const int k = (int)__popcll(__ballot(ok)) - 1;  // the probes that hold are a prefix of the lanes
        lo += k * step;
        hi = std::min<int64_t>(hi, lo + step);
    }
    return lo;
}

// ---- stable compaction of three columns -----------------------------------------------------
struct Cols3 {
    const int64_t* in[3];
    int64_t* out[3];
};
// Record i with keep[i] goes to row off[i] (off: the exclusive scan of keep).
static __global__ void __launch_bounds__(kJoinThreads) k_compact3(int64_t n, const uint32_t* __restrict__ keep,
                                                                  const uint32_t* __restrict__ off, Cols3 c) {
    for (int64_t i = (int64_t)blockIdx.x * kJoinThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kJoinThreads) {
        if (!keep[i]) continue;
        const uint32_t d = off[i];
        c.out[0][d] = c.in[0][i];
        c.out[1][d] = c.in[1][i];
        c.out[2][d] = c.in[2][i];
    }
}

// ---- host helpers ---------------------------------------------------------------------------
static int dev_fail(const char* prefix, hipError_t e, std::string& why) {
    why = std::string(prefix) + ": " + hipGetErrorString(e);
    return GW_E_DEVICE;
}
// `words` header words to the host, and the stream idle behind them.
static hipError_t read_hdr(int64_t* h, const int64_t* d_hdr, int words, hipStream_t s) {
    const hipError_t e = hipMemcpyAsync(h, d_hdr, (size_t)words * 8, hipMemcpyDeviceToHost, s);
    return e != hipSuccess ? e : hipStreamSynchronize(s);
}
// An expand kernel writes two rows per 16-byte store where the five columns share one alignment;
// with shift = 1 they start 8 bytes past a 16-byte boundary and row 0 is written alone: {vec, shift}.
static std::pair<bool, int> expand_alignment(int64_t* const col[5]) {
    int par[5];
    for (int c = 0; c < 5; ++c) par[c] = (int)(((uintptr_t)col[c] >> 3) & 1);
    const bool vec = par[0] == par[1] && par[0] == par[2] && par[0] == par[3] && par[0] == par[4] &&
                     !((uintptr_t)col[0] & 7);
    return {vec, vec ? par[0] : 0};
}
// The event pair around a timed kernel: empty (and begin / end do nothing) unless create() ran.
// Move-only: the declared move leaves no implicit copy.
struct TimedPair {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    TimedPair() = default;
    TimedPair(TimedPair&& o) noexcept : e0(o.e0), e1(o.e1) { o.e0 = o.e1 = nullptr; }
    ~TimedPair() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    hipError_t create() { const hipError_t e = hipEventCreate(&e0); return e != hipSuccess ? e : hipEventCreate(&e1); }
    void begin(hipStream_t s) const { if (e0) (void)hipEventRecord(e0, s); }
    void end(hipStream_t s) const { if (e1) (void)hipEventRecord(e1, s); }
    hipError_t elapsed(float* ms) const { return hipEventElapsedTime(ms, e0, e1); }
};

// ---- scratch ------------------------------------------------------------------------------
// Carves 256-byte aligned arrays out of one block; with base = nullptr it only adds up.
struct Carve {
    char* base;
    size_t at = 0;
    template <typename T>
    T* take(int64_t n) {
        T* r = base ? reinterpret_cast<T*>(base + at) : nullptr;
        at += ((size_t)std::max<int64_t>(n, 1) * sizeof(T) + 255) / 256 * 256;
        return r;
    }
};
// The two kinds of block a call carves its arrays from.  A stateless call's per-device Scratch:
// every call ends synchronised, so the block is free when the next one grows it.
struct Scratch {
    char* p = nullptr;
    size_t cap = 0;
};
static int scratch_ensure(Scratch& s, size_t need, char*& base, const char* prefix, std::string& why) {
    if (need > s.cap) {
        if (s.p) hipFree(s.p);
        s.p = nullptr;
        s.cap = 0;
        if (hipMalloc((void**)&s.p, need) != hipSuccess) {
            (void)hipGetLastError();
            why = std::string(prefix) + ": scratch allocation failed";
            return GW_E_OOM;
        }
        s.cap = need;
    }
    base = s.p;
    return GW_OK;
}
// A handle's own block.  idle: the handle's stream where its work may still use the block (it is
// synchronised before the block is freed), null where every use ends synchronised.
static int scratch_ensure(DevBuf<char>& b, size_t need, char*& base, OpError& er, hipStream_t idle) {
    if ((int64_t)need > b.cap) {
        const hipError_t e = idle ? hipStreamSynchronize(idle) : hipSuccess;
        if (e != hipSuccess) return er.dev_fail(e);
        if (b.reserve_discard((int64_t)need) != hipSuccess) {
            (void)hipGetLastError();
            return er.fail(GW_E_OOM, "%s: out of device memory", er.name);
        }
    }
    base = b.p;
    return GW_OK;
}
// Size, ensure, carve: carve(Carve&) runs over a null base for the size, then over the block
// that scratch_ensure(mem, size, base, how...) gives.
template <typename F, typename Mem, typename... How>
static int carve_from(F carve, Mem& mem, How&&... how) {
    Carve size{nullptr};
    carve(size);
    char* base = nullptr;
    const int rc = scratch_ensure(mem, size.at, base, how...);
    if (rc) return rc;
    Carve c{base};
    carve(c);
    return GW_OK;
}
static int grid_for(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + kJoinThreads - 1) / kJoinThreads, kJoinMaxBlocks)); }
static int bit_length(uint64_t v) { return v ? 64 - __builtin_clzll(v) : 0; }

}  // namespace gw
