// gw_topn.hip — per-window top-N over fired rows (include/gpuwin.h gw_top_n_device, gw_top_n_rows).
//
// The non-keyed second stage of Nexmark Q5 ("hot items": per window, the auctions with the
// highest count) and Q7 (per-window maximum): in Flink a windowAll(...).maxBy(...) or a top-N
// process function behind the keyed window aggregate.  The keyed stage's fire leaves one row
// per live key in device memory; this stage reduces them there to `top` rows per window, so
// only the winners cross PCIe.
//
// Rows are (key, start, end, result) columns in any order, windows interleaved.  Three steps:
//
//   discover  one pass over (end, start): every wave finds the few distinct ends among its 64
//             rows (ballot against the first active lane's value), checks that the rows of one
//             end agree on start, and adds (end, start min, start max, rows) to a block table
//             in LDS; the block's table goes to a global directory, an open-addressing table
//             on `end` whose slots are claimed with a 64-bit atomicCAS and whose other words
//             are only ever touched by atomics (no word is read plainly in the launch that
//             writes it).  The host reads the directory (the call is synchronous), rejects
//             disagreeing starts and too many windows, sorts the ends and sizes the output.
//   select    one pass over (end, result, key), 24 B per row: a persistent grid, each block
//             keeping for up to kTopnPassWindows windows a sorted list of the `top` best
//             (order word, key) pairs in LDS and its worst entry as a threshold.  A row is
//             compared with its window's threshold (two LDS reads); the few that pass are
//             appended to a candidate buffer (ballot + one LDS atomic per wave), which one wave
//             merges into the lists when it fills and at the end.  The window ends of the
//             pass are kernel arguments (scalar registers), so finding a row's window is a
//             handful of scalar compares.  More than kTopnPassWindows windows: one such pass
//             per chunk of windows, each ignoring the other chunks' rows (the end-of-input
//             case: correct, not fast).
//   merge     a second launch (the kernel boundary publishes the blocks' lists), one workgroup
//             per window: the blocks' lists into one, written out with the window's start,
//             end and row count.
//
// Order: `better` is (order word descending, key ascending).  The order word is the result as
// a signed int64, f64_order_key of it for doubles, and its complement when the smallest are
// wanted, so one comparison serves every mode and the result bits come back from the word.
#include "gw_kernels.h"

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

namespace gw {

constexpr int kTopnThreads = 256, kTopnItems = 4, kTopnTile = kTopnThreads * kTopnItems;
constexpr int kTopnCand = 512;       // candidate buffer entries; merged once fewer than one
                                     // step's worth (kTopnThreads) are free
constexpr int kTopnMaxBlocks = 512;  // persistent grid: 2 blocks per CU
constexpr int kDirSlots = 2048;      // global directory slots (power of two, 2 * GW_TOPN_MAX_WINDOWS)
constexpr int kDirProbe = kDirSlots; // slot kDirSlots holds the end INT64_MIN (the empty mark)
constexpr int kBlkDir = 32;          // block-local directory slots
constexpr int64_t kNoEnd = INT64_MIN;

struct Entry {
    int64_t ord;
    int64_t key;
};
__device__ __forceinline__ bool better(int64_t ao, int64_t ak, int64_t bo, int64_t bk) {
    return ao > bo || (ao == bo && ak < bk);
}
__device__ __forceinline__ int64_t order_word(int64_t bits, int mode) {
    int64_t o = (mode & GW_TOPN_F64) ? f64_order_key(bits) : bits;
    return (mode & GW_TOPN_SMALLEST) ? ~o : o;
}
__device__ __forceinline__ int64_t result_bits(int64_t ord, int mode) {
    const int64_t o = (mode & GW_TOPN_SMALLEST) ? ~ord : ord;
    return (mode & GW_TOPN_F64) ? f64_from_order_key(o) : o;
}
__device__ __forceinline__ int64_t shfl64(int64_t v, int lane) {
    return (int64_t)__shfl((long long)v, lane);
}
__device__ __forceinline__ int64_t shfl_up64(int64_t v) {
    return (int64_t)__shfl_up((long long)v, 1);
}

// ---- discovery ---------------------------------------------------------------------------
// Directory words (int64): head[4] = (distinct ends, directory full, start mismatch, -),
// then end / start min / start max / rows, kDirSlots + 1 each.
constexpr int kDirHead = 4;
constexpr int64_t kDirWords = kDirHead + 4ll * (kDirSlots + 1);

__global__ void __launch_bounds__(256) k_topn_dir_init(int64_t* dir) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < kDirHead) dir[i] = 0;
    if (i > kDirSlots) return;
    int64_t* d = dir + kDirHead;
    d[i] = kNoEnd;
    d[(kDirSlots + 1) + i] = INT64_MAX;
    d[2 * (kDirSlots + 1) + i] = INT64_MIN;
    d[3 * (kDirSlots + 1) + i] = 0;
}

static __device__ void dir_insert(int64_t* dir, int64_t end, int64_t smin, int64_t smax, int64_t rows) {
    using ull = unsigned long long;
    int64_t* d_end = dir + kDirHead;
    int slot = -1;
    if (end == kNoEnd) {
        slot = kDirSlots;
        // its end word doubles as the claim: kNoEnd -> kNoEnd + 1 by the first arrival
        if (atomicCAS((ull*)&d_end[slot], (ull)kNoEnd, (ull)(kNoEnd + 1)) == (ull)kNoEnd) atomicAdd((ull*)&dir[0], 1ull);
    } else {
        int s = (int)(slot_hash(end) & (kDirSlots - 1));
        for (int p = 0; p < kDirProbe; ++p) {
            const int64_t old = (int64_t)atomicCAS((ull*)&d_end[s], (ull)kNoEnd, (ull)end);
            if (old == kNoEnd) atomicAdd((ull*)&dir[0], 1ull);
            if (old == kNoEnd || old == end) { slot = s; break; }
            s = (s + 1) & (kDirSlots - 1);
        }
    }
    if (slot < 0) {
        atomicOr((ull*)&dir[1], 1ull);
        return;
    }
    atomicMin((long long*)&d_end[(kDirSlots + 1) + slot], (long long)smin);
    atomicMax((long long*)&d_end[2 * (kDirSlots + 1) + slot], (long long)smax);
    atomicAdd((ull*)&d_end[3 * (kDirSlots + 1) + slot], (ull)rows);
}

__global__ void __launch_bounds__(kTopnThreads) k_topn_discover(int64_t n, const int64_t* __restrict__ end,
                                                                const int64_t* __restrict__ start, int64_t ntiles,
                                                                int64_t* dir) {
    using ull = unsigned long long;
    __shared__ int64_t s_end[kBlkDir], s_min[kBlkDir], s_max[kBlkDir], s_rows[kBlkDir];
    const int lane = __lane_id();
    if (threadIdx.x < kBlkDir) {
        s_end[threadIdx.x] = kNoEnd;
        s_min[threadIdx.x] = INT64_MAX;
        s_max[threadIdx.x] = INT64_MIN;
        s_rows[threadIdx.x] = 0;
    }
    __syncthreads();
    bool mismatch = false;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        int64_t e[kTopnItems], st[kTopnItems];
        bool ok[kTopnItems];
#pragma unroll
        for (int j = 0; j < kTopnItems; ++j) {
            const int64_t i = t * kTopnTile + j * kTopnThreads + threadIdx.x;
            ok[j] = i < n;
            e[j] = ok[j] ? end[i] : 0;
            st[j] = ok[j] ? start[i] : 0;
        }
#pragma unroll
        for (int j = 0; j < kTopnItems; ++j) {
            bool active = ok[j];
            unsigned long long left;
            while ((left = __ballot(active)) != 0ull) {  // one round per distinct end of the wave
                const int lead = __ffsll((long long)left) - 1;
                const int64_t v = shfl64(e[j], lead), sv = shfl64(st[j], lead);
                const bool mine = active && e[j] == v;
                mismatch |= mine && st[j] != sv;
                const int64_t rows = (int64_t)__popcll(__ballot(mine));
                if (lane == lead) {
                    int q = 0;
                    if (v != kNoEnd) {
                        for (; q < kBlkDir; ++q) {
                            const int64_t old = (int64_t)atomicCAS((ull*)&s_end[q], (ull)kNoEnd, (ull)v);
                            if (old == kNoEnd || old == v) break;
                        }
                    } else {
                        q = kBlkDir;
                    }
                    if (q < kBlkDir) {
                        atomicMin((long long*)&s_min[q], (long long)sv);
                        atomicMax((long long*)&s_max[q], (long long)sv);
                        atomicAdd((ull*)&s_rows[q], (ull)rows);
                    } else {  // block table full (or the end that is its empty mark)
                        dir_insert(dir, v, sv, sv, rows);
                    }
                }
                active = active && !mine;
            }
        }
    }
    if (__any(mismatch) && lane == 0) atomicOr((ull*)&dir[2], 1ull);
    __syncthreads();
    if (threadIdx.x < kBlkDir && s_end[threadIdx.x] != kNoEnd)
        dir_insert(dir, s_end[threadIdx.x], s_min[threadIdx.x], s_max[threadIdx.x], s_rows[threadIdx.x]);
}

// ---- selection ---------------------------------------------------------------------------
struct PassWindows {
    int64_t end[kTopnPassWindows];
    int32_t nw;
};

// One wave holds a sorted list, entry l in lane l (cnt <= top of them): add the lanes' entries
// (have) to it.  Entries that cannot make a full list are dropped by one ballot.
__device__ __forceinline__ bool wave_list_add(bool have, int64_t co, int64_t ck, int top, int& cnt, int64_t& mo,
                                              int64_t& mk) {
    const int lane = __lane_id();
    const int64_t to = shfl64(mo, top - 1), tk = shfl64(mk, top - 1);  // the worst entry once full
    unsigned long long todo = __ballot(have && (cnt < top || better(co, ck, to, tk)));
    bool changed = false;
    while (todo) {
        const int b = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int64_t xo = shfl64(co, b), xk = shfl64(ck, b);
        // entries x does not beat stay ahead of it
        const int pos = (int)__popcll(__ballot(lane < cnt && !better(xo, xk, mo, mk)));
        if (pos >= top) continue;
        const int64_t uo = shfl_up64(mo), uk = shfl_up64(mk);
        if (lane > pos) { mo = uo; mk = uk; }
        if (lane == pos) { mo = xo; mk = xk; }
        cnt = min(cnt + 1, top);
        changed = true;
    }
    return changed;
}

// One wave: the candidates of window w (cand[0..ncand)) into its sorted list in LDS.
static __device__ void wave_merge_window(int w, int top, int ncand, const Entry* cand, const int32_t* cand_w, Entry* list,
                                  int32_t* list_n, Entry* thr) {
    const int lane = __lane_id();
    int cnt = list_n[w];
    int64_t mo = lane < cnt ? list[w * GW_TOPN_MAX_N + lane].ord : 0;
    int64_t mk = lane < cnt ? list[w * GW_TOPN_MAX_N + lane].key : 0;
    bool changed = false;
    for (int c0 = 0; c0 < ncand; c0 += 64) {
        const int c = c0 + lane;
        const bool have = c < ncand && cand_w[c] == w;
        changed |= wave_list_add(have, have ? cand[c].ord : 0, have ? cand[c].key : 0, top, cnt, mo, mk);
    }
    if (!changed) return;
    if (lane < cnt) {
        list[w * GW_TOPN_MAX_N + lane].ord = mo;
        list[w * GW_TOPN_MAX_N + lane].key = mk;
    }
    if (lane == 0) list_n[w] = cnt;
    if (cnt == top && lane == top - 1) {
        thr[w].ord = mo;
        thr[w].key = mk;
    }
}

// part: [window of the pass][block][top] entries; part_n: [window][block] list lengths.
__global__ void __launch_bounds__(kTopnThreads) k_topn_select(int64_t n, const int64_t* __restrict__ end,
                                                              const int64_t* __restrict__ res,
                                                              const int64_t* __restrict__ key, int64_t ntiles,
                                                              PassWindows pw, int top, int mode, Entry* part,
                                                              int32_t* part_n) {
    __shared__ Entry s_list[kTopnPassWindows * GW_TOPN_MAX_N];
    __shared__ Entry s_thr[kTopnPassWindows];
    __shared__ int32_t s_list_n[kTopnPassWindows];
    __shared__ Entry s_cand[kTopnCand];
    __shared__ int32_t s_cand_w[kTopnCand];
    __shared__ int32_t s_ncand;
    const int lane = __lane_id(), wave = threadIdx.x >> 6;
    const int nw = pw.nw;
    if (threadIdx.x < kTopnPassWindows) {
        s_thr[threadIdx.x].ord = INT64_MIN;  // nothing is worse: every row passes until the list is full
        s_thr[threadIdx.x].key = INT64_MAX;
        s_list_n[threadIdx.x] = 0;
    }
    if (threadIdx.x == 0) s_ncand = 0;
    __syncthreads();
    int fill = 0;  // candidates waiting (the same in every thread)
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        int64_t e[kTopnItems], r[kTopnItems], k[kTopnItems];
        bool ok[kTopnItems];
#pragma unroll
        for (int j = 0; j < kTopnItems; ++j) {
            const int64_t i = t * kTopnTile + j * kTopnThreads + threadIdx.x;
            ok[j] = i < n;
            e[j] = ok[j] ? end[i] : 0;
            r[j] = ok[j] ? res[i] : 0;
            k[j] = ok[j] ? key[i] : 0;
        }
#pragma unroll
        for (int j = 0; j < kTopnItems; ++j) {
            int w = -1;
#pragma unroll
            for (int q = 0; q < kTopnPassWindows; ++q) {
                if (q >= nw) break;  // uniform: a pass of one window costs one compare per row
                if (e[j] == pw.end[q]) w = q;
            }
            const int64_t o = order_word(r[j], mode);
            bool pass = false;
            if (ok[j] && w >= 0) {
                const int64_t to = s_thr[w].ord, tk = s_thr[w].key;
                pass = o > to || (o == to && k[j] <= tk);
            }
            const unsigned long long m = __ballot(pass);
            if (m) {
                int base = 0;
                const int lead = __ffsll((long long)m) - 1;
                if (lane == lead) base = atomicAdd(&s_ncand, (int)__popcll(m));
                base = __shfl(base, lead);
                const int slot = base + (int)__popcll(m & ((1ull << lane) - 1ull));
                if (pass && slot < kTopnCand) {
                    s_cand[slot].ord = o;
                    s_cand[slot].key = k[j];
                    s_cand_w[slot] = w;
                }
            }
            fill += __syncthreads_count(pass);
            if (fill > kTopnCand - kTopnThreads) {  // the next step might not fit
                if (wave == 0) {
                    for (int q = 0; q < nw; ++q) wave_merge_window(q, top, fill, s_cand, s_cand_w, s_list, s_list_n, s_thr);
                    if (lane == 0) s_ncand = 0;
                }
                fill = 0;
                __syncthreads();
            }
        }
    }
    if (wave == 0 && fill > 0)
        for (int q = 0; q < nw; ++q) wave_merge_window(q, top, fill, s_cand, s_cand_w, s_list, s_list_n, s_thr);
    __syncthreads();
    for (int x = threadIdx.x; x < nw * top; x += kTopnThreads) {
        const int q = x / top, l = x - q * top;
        if (l < s_list_n[q]) part[((int64_t)q * gridDim.x + blockIdx.x) * top + l] = s_list[q * GW_TOPN_MAX_N + l];
    }
    if (threadIdx.x < nw) part_n[threadIdx.x * gridDim.x + blockIdx.x] = s_list_n[threadIdx.x];
}

// One workgroup per window of the pass: the nblocks lists into the final one, then the output
// rows.  Each wave merges every kTopnMergeWaves-th list (a list is one dependent load, so the
// waves' loads overlap), wave 0 then merges the waves' lists through LDS.
// wdir: sorted window directory (end, start, rows, first output row), wcap each.
constexpr int kTopnMergeWaves = 16;
__global__ void __launch_bounds__(kTopnMergeWaves * 64)
k_topn_merge(const Entry* __restrict__ part, const int32_t* __restrict__ part_n, int nblocks, int top, int mode,
             const int64_t* __restrict__ wdir, int64_t wcap, int w0, int64_t* key_out, int64_t* start_out,
             int64_t* end_out, int64_t* res_out, int64_t* rows_out) {
    __shared__ Entry s_l[kTopnMergeWaves][GW_TOPN_MAX_N];
    __shared__ int32_t s_n[kTopnMergeWaves];
    const int lane = __lane_id(), wave = threadIdx.x >> 6;
    const int q = blockIdx.x;
    int cnt = 0;
    int64_t mo = 0, mk = 0;
    for (int b = wave; b < nblocks; b += kTopnMergeWaves) {
        const int len = part_n[q * nblocks + b];
        const Entry* src = part + ((int64_t)q * nblocks + b) * top;
        // loaded without waiting for len (slots past it are allocated, unwritten and unused)
        const int64_t co = lane < top ? src[lane].ord : 0, ck = lane < top ? src[lane].key : 0;
        wave_list_add(lane < len, co, ck, top, cnt, mo, mk);
    }
    if (lane < cnt) {
        s_l[wave][lane].ord = mo;
        s_l[wave][lane].key = mk;
    }
    if (lane == 0) s_n[wave] = cnt;
    __syncthreads();
    if (wave != 0) return;
    for (int v = 1; v < kTopnMergeWaves; ++v) {
        const bool have = lane < s_n[v];
        wave_list_add(have, have ? s_l[v][lane].ord : 0, have ? s_l[v][lane].key : 0, top, cnt, mo, mk);
    }
    const int w = w0 + q;
    const int64_t off = wdir[3 * wcap + w];
    if (lane < cnt) {
        key_out[off + lane] = mk;
        start_out[off + lane] = wdir[wcap + w];
        end_out[off + lane] = wdir[w];
        res_out[off + lane] = result_bits(mo, mode);
        if (rows_out) rows_out[off + lane] = wdir[2 * wcap + w];
    }
}

struct Scratch {
    char* p = nullptr;
    size_t cap = 0;
};

constexpr size_t kDirBytes = ((size_t)kDirWords * 8 + 255) / 256 * 256;
constexpr size_t kWdirBytes = 4ull * GW_TOPN_MAX_WINDOWS * 8;

static int scratch_ensure(Scratch& s, size_t need, std::string& why) {
    if (need <= s.cap) return GW_OK;
    if (s.p) hipFree(s.p);
    s.p = nullptr;
    s.cap = 0;
    if (hipMalloc((void**)&s.p, need) != hipSuccess) {
        (void)hipGetLastError();
        why = "top-N: scratch allocation failed";
        return GW_E_OOM;
    }
    s.cap = need;
    return GW_OK;
}

// The device top-N (gpuwin.h gw_top_n_device).  host_out: the output columns are host arrays
// (gw_top_n_rows), filled from a device staging area in the scratch.  Synchronous on s.
int top_n_run(int64_t n, const int64_t* d_key, const int64_t* d_start, const int64_t* d_end, const int64_t* d_res,
              int top, int mode, int64_t* key_out, int64_t* start_out, int64_t* end_out, int64_t* res_out,
              int64_t* rows_out, int64_t cap, int64_t* n_out, bool host_out, hipStream_t s, std::string& why) {
    static std::mutex mu;
    static Scratch scr[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { why = "top-N: no device"; return GW_E_DEVICE; }
    std::lock_guard<std::mutex> lock(mu);  // every call waits for its launches before it returns
    Scratch& S = scr[dev];
    int rc = scratch_ensure(S, kDirBytes + kWdirBytes, why);
    if (rc) return rc;
    auto dev_fail = [&](hipError_t e) {
        why = std::string("top-N: ") + hipGetErrorString(e);
        return GW_E_DEVICE;
    };
    const int64_t ntiles = (n + kTopnTile - 1) / kTopnTile;
    const int grid = (int)std::min<int64_t>(ntiles, kTopnMaxBlocks);
    int64_t* dir = reinterpret_cast<int64_t*>(S.p);
    hipLaunchKernelGGL(k_topn_dir_init, dim3((kDirSlots + 1 + 255) / 256), dim3(256), 0, s, dir);
    hipLaunchKernelGGL(k_topn_discover, dim3(grid), dim3(kTopnThreads), 0, s, n, d_end, d_start, ntiles, dir);
    hipError_t e = hipGetLastError();
    std::vector<int64_t> hdir((size_t)kDirWords);
    if (e == hipSuccess) e = hipMemcpyAsync(hdir.data(), dir, (size_t)kDirWords * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return dev_fail(e);
    if (hdir[2]) { why = "top-N: rows of one window end carry different starts"; return GW_E_INVALID; }
    if (hdir[1] || hdir[0] > GW_TOPN_MAX_WINDOWS) {
        why = "top-N: more than GW_TOPN_MAX_WINDOWS distinct window ends in one call";
        return GW_E_UNSUPPORTED;
    }
    struct Win {
        int64_t end, start, rows;
    };
    std::vector<Win> wins;
    const int64_t* h = hdir.data() + kDirHead;
    constexpr int kS = kDirSlots + 1;
    for (int i = 0; i < kS; ++i) {
        if (h[3 * kS + i] == 0) continue;  // a claimed slot always has rows
        if (h[kS + i] != h[2 * kS + i]) { why = "top-N: rows of one window end carry different starts"; return GW_E_INVALID; }
        wins.push_back({i == kDirSlots ? kNoEnd : h[i], h[kS + i], h[3 * kS + i]});
    }
    std::sort(wins.begin(), wins.end(), [](const Win& a, const Win& b) { return a.end < b.end; });
    const int64_t W = (int64_t)wins.size();
    std::vector<int64_t> wdir(4 * (size_t)W);
    int64_t total = 0;
    for (int64_t i = 0; i < W; ++i) {
        wdir[i] = wins[i].end;
        wdir[W + i] = wins[i].start;
        wdir[2 * W + i] = wins[i].rows;
        wdir[3 * W + i] = total;
        total += std::min<int64_t>(top, wins[i].rows);
    }
    *n_out = total;
    if (total > cap) { why = "top-N: output arrays too small"; return GW_E_OUTPUT_FULL; }
    const int64_t passw = std::min<int64_t>(W, kTopnPassWindows);
    const size_t part_bytes = ((size_t)passw * grid * top * sizeof(Entry) + 255) / 256 * 256;
    const size_t partn_bytes = ((size_t)passw * grid * 4 + 255) / 256 * 256;
    const size_t out_bytes = host_out ? (size_t)total * 8 * 5 : 0;
    if ((rc = scratch_ensure(S, kDirBytes + kWdirBytes + part_bytes + partn_bytes + out_bytes, why))) return rc;
    int64_t* d_wdir = reinterpret_cast<int64_t*>(S.p + kDirBytes);
    Entry* part = reinterpret_cast<Entry*>(S.p + kDirBytes + kWdirBytes);
    int32_t* part_n = reinterpret_cast<int32_t*>(S.p + kDirBytes + kWdirBytes + part_bytes);
    int64_t* stage = reinterpret_cast<int64_t*>(S.p + kDirBytes + kWdirBytes + part_bytes + partn_bytes);
    int64_t* ko = host_out ? stage : key_out;
    int64_t* so = host_out ? stage + total : start_out;
    int64_t* eo = host_out ? stage + 2 * total : end_out;
    int64_t* ro = host_out ? stage + 3 * total : res_out;
    int64_t* wo = host_out ? (rows_out ? stage + 4 * total : nullptr) : rows_out;
    e = hipMemcpyAsync(d_wdir, wdir.data(), wdir.size() * 8, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return dev_fail(e);
    for (int64_t w0 = 0; w0 < W; w0 += kTopnPassWindows) {
        PassWindows pw{};
        pw.nw = (int32_t)std::min<int64_t>(kTopnPassWindows, W - w0);
        for (int q = 0; q < pw.nw; ++q) pw.end[q] = wins[w0 + q].end;
        hipLaunchKernelGGL(k_topn_select, dim3(grid), dim3(kTopnThreads), 0, s, n, d_end, d_res, d_key, ntiles, pw, top,
                           mode, part, part_n);
        hipLaunchKernelGGL(k_topn_merge, dim3(pw.nw), dim3(kTopnMergeWaves * 64), 0, s, part, part_n, grid, top, mode, d_wdir, W, (int)w0,
                           ko, so, eo, ro, wo);
    }
    e = hipGetLastError();
    if (e == hipSuccess && host_out && total > 0) {
        int64_t* dst[5] = {key_out, start_out, end_out, res_out, rows_out};
        for (int c = 0; c < 5 && e == hipSuccess; ++c)
            if (dst[c]) e = hipMemcpyAsync(dst[c], stage + c * total, (size_t)total * 8, hipMemcpyDeviceToHost, s);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);  // also keeps wdir / wins alive for the copies
    if (e != hipSuccess) return dev_fail(e);
    return GW_OK;
}

}  // namespace gw
