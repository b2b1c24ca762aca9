// gw_joinutil.h — what the two-stream joins share (gw_join.hip: the window join and coGroup;
// gw_ijoin.hip: the interval join): the two-pass exclusive scan, the wave-wide reductions and
// search of their kernels, and the carved per-device scratch.  Each including file gets its own
// copy of the kernels (static, or template instances), so nothing here is a link-time symbol.
#pragma once
#include <algorithm>
#include <string>

#include "gw_devmem.h"
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

// ---- scratch ------------------------------------------------------------------------------
struct Scratch {
    char* p = nullptr;
    size_t cap = 0;
};
static int scratch_ensure(Scratch& s, size_t need, std::string& why) {
    if (need <= s.cap) return GW_OK;
    if (s.p) hipFree(s.p);
    s.p = nullptr;
    s.cap = 0;
    if (hipMalloc((void**)&s.p, need) != hipSuccess) {
        (void)hipGetLastError();
        why = "window join: scratch allocation failed";
        return GW_E_OOM;
    }
    s.cap = need;
    return GW_OK;
}
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
static int grid_for(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + kJoinThreads - 1) / kJoinThreads, kJoinMaxBlocks)); }
static int bit_length(uint64_t v) { return v ? 64 - __builtin_clzll(v) : 0; }

}  // namespace gw
