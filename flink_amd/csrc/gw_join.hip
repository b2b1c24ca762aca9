// gw_join.hip — event-time window join of two keyed streams (include/gpuwin.h gw_window_join_*,
// gw_join_*): stream.join(other).where(k1).equalTo(k2).window(assigner).apply(JoinFunction),
// Nexmark Q8.
//
// Flink runs a window join as union -> keyBy -> WindowOperator with ListState, and at the fire
// JoinCoGroupFunction emits the per-(key, window) cross product of the two sides
// (RS/api/datastream/JoinedStreams.java, CoGroupedStreams.java).  Here a fire over the records
// of both sides and the watermark interval (w0, w1] is six stages over device columns:
//
//   count    per record the number of its windows with w0 < end - 1 <= w1, an exclusive scan of
//            those counts, and the device-wide minimum / maximum of the fired window starts and
//            of the fired records' key words (so the sort sees only the bits that vary);
//   emit     one tuple per (record, fired window): the key word (sign bit flipped, minus the
//            minimum), the window ordinal (start - min start) / slide and a source word (side in
//            the top bit, record index below); left tuples before right tuples, arrival order;
//   sort     two stable passes of gw::sort_pairs_u64 -- by key word, then by ordinal -- so a
//            (window, key) group is contiguous, windows ascending, keys ascending, and inside a
//            group the left records precede the right ones, each side in arrival order;
//   groups   heads where (ordinal, key) changes; per group its first tuple, L and R; an int64
//            exclusive scan of L * R.  This table is a stage of its own (a coGroup or an outer
//            join reads the same table).  Groups with L * R > 0 are compacted into descriptors;
//   expand   the hot kernel: a workgroup owns kExpTile consecutive output pairs, finds the
//            descriptors its tile touches with one search per end of the tile, keeps them in LDS,
//            and every lane writes two consecutive pairs of each of the five columns with one
//            16-byte store.  Work is split by output pairs, never by groups, so one group of
//            4096 x 64 and a million groups of 1 x 1 are the same work per workgroup.
//
// stream.coGroup(other)... (CoGroupedStreams, the primitive under the join) shares count .. groups
// and differs in what leaves (gw_window_join_outer_*, gw_window_cogroup_*, gw_join_set_mode):
//
//   outer    the left / right / full outer joins as modes of the expansion: a one-sided group
//            the mode keeps becomes a descriptor of its own (L x 1 or 1 x R, the lacking side
//            flagged), its rows carry the caller's null payload, and a `present` byte per row
//            tells the kinds apart.  The expand kernel is instantiated per mode; the inner one
//            knows nothing of this;
//   cogroup  the group table itself as a CSR: two scans of the groups' L and R, one writer of
//            the group rows, one pass that sends every sorted tuple's payload to its place.
//
// No atomics in the expand kernel; the scans are two-pass (block sums, one block over the sums,
// a down-sweep); the only look-back is gw_sort.hip's own.  The host reads the device twice per
// call: the tuple count (it sizes the sort) and the pair count (it sizes the output).
#include <algorithm>
#include <cstring>
#include <functional>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "gw_joinop.h"    // the host side of the operator: OpError, OpStream, RowBuf, staged_ingest (and gw_devmem.h)
#include "gw_joinutil.h"  // scan_excl, the wave reductions and search, k_compact3, Scratch, Carve
#include "gw_kernels.h"
#include "gw_sort.h"

namespace gw {

struct JoinGeom {
    int64_t size, slide, offset;
};

constexpr const char* kJoinName = "window join";  // the prefix of the shared helpers' messages
constexpr uint32_t kJoinRight = 0x80000000u;
// header words (int64) shared by the stages of one call
enum { JH_NT = 0, JH_MINS, JH_MAXS, JH_MINK, JH_MAXK, JH_FLAGS, JH_NG, JH_TOTAL, JH_NC, JH_KEPT, JH_LATE, kJoinHdr = 16 };

// SlidingEventTimeWindows.assignWindows (RS/api/windowing/assigners/SlidingEventTimeWindows.java:
// 75-90) with TimeWindow.getWindowStartWithOffset (TimeWindow.java:264-272): the record's last
// window start and the number of its windows (starts ls - k * slide, k < nw).  A step that leaves
// int64 is GW_DF_RANGE instead of Java's wrap-around.
GW_HD unsigned join_windows(const JoinGeom& g, int64_t ts, int64_t& ls, int& nw) {
    ls = 0;
    nw = 0;
    if (ts == INT64_MIN) return (unsigned)GW_DF_NO_TS;
    int64_t rel, end;
    if (__builtin_sub_overflow(ts, g.offset, &rel)) return (unsigned)GW_DF_RANGE;
    int64_t rem = rel % g.slide;
    if (rem < 0) rem += g.slide;
    if (__builtin_sub_overflow(ts, rem, &ls) || __builtin_add_overflow(ls, g.size, &end)) return (unsigned)GW_DF_RANGE;
    if (g.size <= rem) return 0;  // size < slide: between two windows
    nw = g.size == g.slide ? 1 : (int)(((uint64_t)(g.size - rem) + (uint64_t)(g.slide - 1)) / (uint64_t)g.slide);
    int64_t back, first;
    if (__builtin_mul_overflow((int64_t)(nw - 1), g.slide, &back) || __builtin_sub_overflow(ls, back, &first))
        return (unsigned)GW_DF_RANGE;
    return 0;
}
// Windows k of the record firing in (w0, w1] (EventTimeTrigger: at maxTimestamp = end - 1).
GW_HD uint64_t join_fired(const JoinGeom& g, int64_t ls, int nw, int64_t w0, int64_t w1) {
    uint64_t m = 0;
    for (int k = 0; k < nw; ++k) {
        const int64_t mt = ls - (int64_t)k * g.slide + (g.size - 1);
        if (mt > w0 && mt <= w1) m |= 1ull << k;
    }
    return m;
}

// ---- count / emit ---------------------------------------------------------------------------
struct JoinIn {
    const int64_t *key[2], *ts[2], *pay[2];
    int64_t n_l, n;  // left records, all records (left first)
    JoinGeom g;
    int64_t w0, w1;
};

__global__ void __launch_bounds__(kJoinThreads) k_join_hdr_init(int64_t* hdr) {
    if (threadIdx.x >= kJoinHdr) return;
    int64_t v = 0;
    if (threadIdx.x == JH_MINS) v = INT64_MAX;
    if (threadIdx.x == JH_MAXS) v = INT64_MIN;
    if (threadIdx.x == JH_MINK) v = -1;  // all ones
    hdr[threadIdx.x] = v;
}

__global__ void __launch_bounds__(kJoinThreads) k_join_count(JoinIn a, uint32_t* cnt, int64_t* hdr) {
    using ull = unsigned long long;
    __shared__ int64_t s_min[4], s_max[4];
    __shared__ uint64_t s_kmin[4], s_kmax[4], s_flags[4];
    int64_t mins = INT64_MAX, maxs = INT64_MIN;
    uint64_t mink = ~0ull, maxk = 0, flags = 0;
    for (int64_t i = (int64_t)blockIdx.x * kJoinThreads + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kJoinThreads) {
        const int side = i >= a.n_l;
        const int64_t j = side ? i - a.n_l : i;
        int64_t ls;
        int nw;
        const unsigned f = join_windows(a.g, a.ts[side][j], ls, nw);
        flags |= f;
        uint32_t c = 0;
        if (!f) {
            const uint64_t m = join_fired(a.g, ls, nw, a.w0, a.w1);
            if (m) {
                c = (uint32_t)__popcll(m);
                const int klo = __ffsll((long long)m) - 1, khi = 63 - __clzll((long long)m);
                const int64_t hi_s = ls - (int64_t)klo * a.g.slide, lo_s = ls - (int64_t)khi * a.g.slide;
                mins = lo_s < mins ? lo_s : mins;
                maxs = hi_s > maxs ? hi_s : maxs;
                const uint64_t kw = join_key_word(a.key[side][j]);
                mink = kw < mink ? kw : mink;
                maxk = kw > maxk ? kw : maxk;
            }
        }
        cnt[i] = c;
    }
    mins = wave_min_i64(mins);
    maxs = wave_max_i64(maxs);
    mink = wave_min_u64(mink);
    maxk = wave_max_u64(maxk);
    flags = wave_ior(flags);
    const int wave = threadIdx.x >> 6;
    if (__lane_id() == 0) {
        s_min[wave] = mins; s_max[wave] = maxs; s_kmin[wave] = mink; s_kmax[wave] = maxk; s_flags[wave] = flags;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < 4; ++w) {
        mins = s_min[w] < mins ? s_min[w] : mins;
        maxs = s_max[w] > maxs ? s_max[w] : maxs;
        mink = s_kmin[w] < mink ? s_kmin[w] : mink;
        maxk = s_kmax[w] > maxk ? s_kmax[w] : maxk;
        flags |= s_flags[w];
    }
    if (flags) atomicOr((ull*)&hdr[JH_FLAGS], (ull)flags);
    if (mins <= maxs) {  // the block saw a fired window
        atomicMin((long long*)&hdr[JH_MINS], (long long)mins);
        atomicMax((long long*)&hdr[JH_MAXS], (long long)maxs);
        atomicMin((ull*)&hdr[JH_MINK], (ull)mink);
        atomicMax((ull*)&hdr[JH_MAXK], (ull)maxk);
    }
}

__global__ void __launch_bounds__(kJoinThreads) k_join_emit(JoinIn a, const uint32_t* __restrict__ toff, int64_t min_start,
                                                            uint64_t min_kw, uint64_t* kw, uint64_t* ord, uint32_t* src) {
    for (int64_t i = (int64_t)blockIdx.x * kJoinThreads + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kJoinThreads) {
        const int side = i >= a.n_l;
        const int64_t j = side ? i - a.n_l : i;
        int64_t ls;
        int nw;
        if (join_windows(a.g, a.ts[side][j], ls, nw)) continue;
        uint64_t m = join_fired(a.g, ls, nw, a.w0, a.w1);
        if (!m) continue;
        const uint64_t k = join_key_word(a.key[side][j]) - min_kw;
        const uint32_t sw = (uint32_t)j | (side ? kJoinRight : 0u);
        uint32_t t = toff[i];
        while (m) {
            const int q = __ffsll((long long)m) - 1;
            m &= m - 1;
            const int64_t start = ls - (int64_t)q * a.g.slide;
            kw[t] = k;
            ord[t] = ((uint64_t)start - (uint64_t)min_start) / (uint64_t)a.g.slide;
            src[t] = sw;
            ++t;
        }
    }
}

__global__ void __launch_bounds__(kJoinThreads) k_join_gather_ord(int64_t nt, const uint32_t* __restrict__ perm,
                                                                  const uint64_t* __restrict__ ord, uint64_t* out) {
    for (int64_t i = (int64_t)blockIdx.x * kJoinThreads + threadIdx.x; i < nt; i += (int64_t)gridDim.x * kJoinThreads)
        out[i] = ord[perm[i]];
}

// Sorted tuple i: its key, ordinal, source word and payload, and whether a group starts at it.
__global__ void __launch_bounds__(kJoinThreads) k_join_gather(JoinIn a, int64_t nt, const uint32_t* __restrict__ perm,
                                                              const uint64_t* __restrict__ ord,
                                                              const uint32_t* __restrict__ src, int64_t* gkey, uint64_t* gord,
                                                              uint32_t* gsrc, int64_t* gpay) {
    for (int64_t i = (int64_t)blockIdx.x * kJoinThreads + threadIdx.x; i < nt; i += (int64_t)gridDim.x * kJoinThreads) {
        const uint32_t t = perm[i];
        const uint32_t sw = src[t];
        const int side = sw >> 31;
        const uint32_t j = sw & ~kJoinRight;
        gkey[i] = a.key[side][j];
        gord[i] = ord[t];
        gsrc[i] = sw;
        gpay[i] = a.pay[side][j];
    }
}

// ---- group table ----------------------------------------------------------------------------
__global__ void __launch_bounds__(kJoinThreads) k_join_heads(int64_t nt, const int64_t* __restrict__ gkey,
                                                             const uint64_t* __restrict__ gord, uint32_t* head) {
    for (int64_t i = (int64_t)blockIdx.x * kJoinThreads + threadIdx.x; i < nt; i += (int64_t)gridDim.x * kJoinThreads)
        head[i] = i == 0 || gkey[i] != gkey[i - 1] || gord[i] != gord[i - 1];
}
// gfirst[g]: the group's first tuple; gmid[g]: its first right tuple (stays ~0 without one).
__global__ void __launch_bounds__(kJoinThreads) k_join_group_fill(int64_t nt, const uint32_t* __restrict__ head,
                                                                  const uint32_t* __restrict__ hex,
                                                                  const uint32_t* __restrict__ gsrc, uint32_t* gfirst,
                                                                  uint32_t* gmid) {
    for (int64_t i = (int64_t)blockIdx.x * kJoinThreads + threadIdx.x; i < nt; i += (int64_t)gridDim.x * kJoinThreads) {
        const uint32_t h = head[i];
        const uint32_t g = hex[i] + h - 1;
        if (h) gfirst[g] = (uint32_t)i;
        if ((gsrc[i] >> 31) && (h || !(gsrc[i - 1] >> 31))) gmid[g] = (uint32_t)i;
    }
}
// A descriptor's R word: R below, and above it which side the group lacks (an outer join's
// unmatched rows).  R < 2^30, so the inner join's words are plain R.
constexpr uint32_t kDescNoLeft = 1u << 30, kDescNoRight = 1u << 31, kDescRMask = kDescNoLeft - 1;

// Over nt entries (the groups are the first hdr[JH_NG] of them): the group's rows in `mode` (L * R,
// or with one side empty L or R where the mode keeps that side) and whether it has any.
__global__ void __launch_bounds__(kJoinThreads) k_join_group_prod(int64_t nt, const int64_t* __restrict__ hdr,
                                                                  const uint32_t* __restrict__ gfirst,
                                                                  const uint32_t* __restrict__ gmid, int mode, int64_t* prod,
                                                                  uint32_t* ne) {
    const int64_t ng = hdr[JH_NG];
    for (int64_t g = (int64_t)blockIdx.x * kJoinThreads + threadIdx.x; g < nt; g += (int64_t)gridDim.x * kJoinThreads) {
        int64_t p = 0;
        if (g < ng) {
            const int64_t first = gfirst[g], end = g + 1 < ng ? (int64_t)gfirst[g + 1] : nt;
            const int64_t mid = gmid[g] == ~0u ? end : (int64_t)gmid[g];
            const int64_t L = mid - first, R = end - mid;  // both below 2^30
            p = L * R;
            if (R == 0 && (mode & GW_JOIN_MODE_LEFT_OUTER)) p = L;
            if (L == 0 && (mode & GW_JOIN_MODE_RIGHT_OUTER)) p = R;
        }
        prod[g] = p;
        ne[g] = p > 0;
    }
}
// Descriptors of the groups with rows: row offset, first left tuple, first right tuple, R, key
// and window start; coff[nc] = the total.  A left-only group is L x 1 and a right-only group
// 1 x R with the lacking side flagged in the R word; its tuple index is the group's first, so it
// stays inside gpay whether or not a lane reads through it.
__global__ void __launch_bounds__(kJoinThreads) k_join_compact(int64_t nt, const int64_t* __restrict__ hdr,
                                                               const uint32_t* __restrict__ gfirst,
                                                               const uint32_t* __restrict__ gmid,
                                                               const int64_t* __restrict__ prod,
                                                               const int64_t* __restrict__ poff,
                                                               const uint32_t* __restrict__ cidx,
                                                               const int64_t* __restrict__ gkey,
                                                               const uint64_t* __restrict__ gord, int64_t min_start,
                                                               int64_t slide, int64_t* coff, uint32_t* cfirst, uint32_t* crb,
                                                               uint32_t* cR, int64_t* ckey, int64_t* cws) {
    const int64_t ng = hdr[JH_NG];
    for (int64_t g = (int64_t)blockIdx.x * kJoinThreads + threadIdx.x; g < ng; g += (int64_t)gridDim.x * kJoinThreads) {
        if (g == 0) coff[hdr[JH_NC]] = hdr[JH_TOTAL];
        if (prod[g] <= 0) continue;
        const uint32_t c = cidx[g];
        const int64_t first = gfirst[g], end = g + 1 < ng ? (int64_t)gfirst[g + 1] : nt;
        coff[c] = poff[g];
        cfirst[c] = (uint32_t)first;
        if (gmid[g] == ~0u) {  // left only: kept by the mode, or prod[g] were 0
            crb[c] = (uint32_t)first;
            cR[c] = 1u | kDescNoRight;
        } else {
            crb[c] = gmid[g];
            cR[c] = (uint32_t)(end - (int64_t)gmid[g]) | ((int64_t)gmid[g] == first ? kDescNoLeft : 0u);
        }
        ckey[c] = gkey[first];
        cws[c] = (int64_t)((uint64_t)min_start + gord[first] * (uint64_t)slide);
    }
}

// ---- expand ---------------------------------------------------------------------------------
constexpr int kExpTile = 1024;  // output slots per workgroup: 2 steps of 256 lanes x 2 pairs
struct JoinOut {
    int64_t* col[5];      // key, start, end, left payload, right payload
    uint8_t* present;     // outer modes: 1 left only, 2 right only, 3 both (may be null)
    int64_t null_payload; // outer modes: the lacking side's payload
};

struct Pair {
    int64_t key, ws, lp, rp;
};

// Output slot q holds row q - shift: with shift = 1 the columns start 8 bytes past a 16-byte
// boundary and row 0 is written alone, so every two-row store is aligned.
// MODE: the GW_JOIN_MODE_* of the call.  The inner join (0) knows no flagged descriptor and is
// the kernel it was; an outer mode tests only the flags its descriptors can carry.  A lacking
// side's tuples are never read: its payload is o.null_payload.  `present` takes the two rows of
// a lane as one 2-byte store where that is aligned (always so for the operator, whose columns
// and present bytes advance together) and as two bytes elsewhere.
template <bool VEC, int MODE>
__global__ void __launch_bounds__(kJoinThreads) k_join_expand(int64_t P, int shift, int64_t nc,
                                                              const int64_t* __restrict__ coff,
                                                              const uint32_t* __restrict__ cfirst,
                                                              const uint32_t* __restrict__ crb,
                                                              const uint32_t* __restrict__ cR,
                                                              const int64_t* __restrict__ ckey,
                                                              const int64_t* __restrict__ cws,
                                                              const int64_t* __restrict__ gpay, int64_t size, JoinOut o) {
    constexpr bool kNoRight = (MODE & GW_JOIN_MODE_LEFT_OUTER) != 0;  // left-only descriptors occur
    constexpr bool kNoLeft = (MODE & GW_JOIN_MODE_RIGHT_OUTER) != 0;  // right-only descriptors occur
    __shared__ int64_t s_off[kExpTile + 1];
    __shared__ uint32_t s_first[kExpTile], s_rb[kExpTile], s_R[kExpTile];
    __shared__ int64_t s_c[2];
    const int64_t slot0 = (int64_t)blockIdx.x * kExpTile;
    const int64_t p_first = std::max<int64_t>(slot0 - shift, 0);
    const int64_t p_last = std::min<int64_t>(slot0 + kExpTile - 1 - shift, P - 1);
    const int wave = threadIdx.x >> 6;
    if (wave < 2) {
        const int64_t c = wave_search(coff, nc, wave == 0 ? p_first : p_last);
        if (__lane_id() == 0) s_c[wave] = c;
    }
    __syncthreads();
    const int64_t c0 = s_c[0];
    const int ngt = (int)(s_c[1] - c0) + 1;  // <= kExpTile: every descriptor has a row in the tile
    for (int i = threadIdx.x; i <= ngt; i += kJoinThreads) {
        s_off[i] = coff[c0 + i];
        if (i < ngt) {
            s_first[i] = cfirst[c0 + i];
            s_rb[i] = crb[c0 + i];
            s_R[i] = cR[c0 + i];
        }
    }
    __syncthreads();
#pragma unroll
    for (int step = 0; step < kExpTile / (2 * kJoinThreads); ++step) {
        const int64_t q = slot0 + step * 2 * kJoinThreads + 2 * threadIdx.x;
        const int64_t pa = q - shift, pb = pa + 1;
        const bool va = pa >= 0 && pa < P, vb = pb < P;
        if (!va && !vb) continue;
        const int64_t p = va ? pa : pb;
        int lo = 0, hi = ngt;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (s_off[mid] <= p) lo = mid; else hi = mid;
        }
        const uint64_t r = (uint64_t)(p - s_off[lo]);
        uint32_t R = s_R[lo];
        uint32_t fx = 0;  // the sides x's descriptor lacks: 1 left, 2 right
        if constexpr (MODE != 0) {
            fx = R >> 30;
            R &= kDescRMask;  // >= 1: a left-only descriptor is L x 1
        }
        uint64_t li, rj;
        if (r >> 32) {
            li = r / R;
            rj = r - li * R;
        } else {
            li = (uint32_t)r / R;
            rj = (uint32_t)r - (uint32_t)li * R;
        }
        const bool xl = !(kNoLeft && (fx & 1)), xr = !(kNoRight && (fx & 2));
        Pair x, y;
        x.key = ckey[c0 + lo];
        x.ws = cws[c0 + lo];
        x.lp = xl ? gpay[s_first[lo] + li] : o.null_payload;
        x.rp = xr ? gpay[s_rb[lo] + rj] : o.null_payload;
        y = x;
        uint32_t fy = fx;
        if (va && vb) {
            if (pb >= s_off[lo + 1]) {  // the next descriptor: its row 0
                ++lo;
                if constexpr (MODE != 0) fy = s_R[lo] >> 30;
                y.key = ckey[c0 + lo];
                y.ws = cws[c0 + lo];
                y.lp = !(kNoLeft && (fy & 1)) ? gpay[s_first[lo]] : o.null_payload;
                y.rp = !(kNoRight && (fy & 2)) ? gpay[s_rb[lo]] : o.null_payload;
            } else if (rj + 1 < R) {  // (R > 1: the descriptor has right tuples)
                y.rp = gpay[s_rb[lo] + rj + 1];
            } else {  // (li + 1 < L: the descriptor has left tuples)
                y.lp = gpay[s_first[lo] + li + 1];
                if (xr) y.rp = gpay[s_rb[lo]];
            }
        }
        if (VEC && va && vb) {
            *reinterpret_cast<I64x2*>(o.col[0] + pa) = I64x2{x.key, y.key};
            *reinterpret_cast<I64x2*>(o.col[1] + pa) = I64x2{x.ws, y.ws};
            *reinterpret_cast<I64x2*>(o.col[2] + pa) = I64x2{x.ws + size, y.ws + size};
            *reinterpret_cast<I64x2*>(o.col[3] + pa) = I64x2{x.lp, y.lp};
            *reinterpret_cast<I64x2*>(o.col[4] + pa) = I64x2{x.rp, y.rp};
        } else {
            if (va) {
                o.col[0][pa] = x.key; o.col[1][pa] = x.ws; o.col[2][pa] = x.ws + size;
                o.col[3][pa] = x.lp; o.col[4][pa] = x.rp;
            }
            if (vb) {
                o.col[0][pb] = y.key; o.col[1][pb] = y.ws; o.col[2][pb] = y.ws + size;
                o.col[3][pb] = y.lp; o.col[4][pb] = y.rp;
            }
        }
        if constexpr (MODE != 0) {
            if (o.present) {
                const uint32_t bx = 3u ^ fx, by = 3u ^ fy;
                if (va && vb && !((uintptr_t)(o.present + pa) & 1)) {
                    *reinterpret_cast<uint16_t*>(o.present + pa) = (uint16_t)(bx | by << 8);
                } else {
                    if (va) o.present[pa] = (uint8_t)bx;
                    if (vb) o.present[pb] = (uint8_t)by;
                }
            }
        }
    }
}

// ---- the stateless core ---------------------------------------------------------------------
struct RecArrays {  // by records
    int64_t* hdr;
    uint32_t *cnt, *toff;
    int64_t* blk;
    void carve(Carve& c, int64_t n) {
        hdr = c.take<int64_t>(kJoinHdr);
        cnt = c.take<uint32_t>(n);
        toff = c.take<uint32_t>(n);
        blk = c.take<int64_t>(scan_blocks(n) + 1);
    }
};
struct TupArrays {  // by tuples
    uint64_t *kw0, *kw1, *ord, *ord0, *ord1, *gord;
    uint32_t *v0, *v1, *src, *gsrc, *head, *hex, *gfirst, *gmid, *ne, *cidx, *cfirst, *crb, *cR;
    int64_t *gkey, *gpay, *prod, *poff, *coff, *ckey, *cws, *blk;
    void* sort;
    void carve(Carve& c, int64_t nt) {
        kw0 = c.take<uint64_t>(nt); kw1 = c.take<uint64_t>(nt); ord = c.take<uint64_t>(nt);
        ord0 = c.take<uint64_t>(nt); ord1 = c.take<uint64_t>(nt); gord = c.take<uint64_t>(nt);
        v0 = c.take<uint32_t>(nt); v1 = c.take<uint32_t>(nt); src = c.take<uint32_t>(nt); gsrc = c.take<uint32_t>(nt);
        head = c.take<uint32_t>(nt); hex = c.take<uint32_t>(nt); gfirst = c.take<uint32_t>(nt);
        // (nt + 1: a coGroup keeps its per-group L and R in ne and cidx and their scans, with the
        // totals as entry ng, in poff and coff)
        gmid = c.take<uint32_t>(nt); ne = c.take<uint32_t>(nt + 1); cidx = c.take<uint32_t>(nt + 1);
        cfirst = c.take<uint32_t>(nt); crb = c.take<uint32_t>(nt); cR = c.take<uint32_t>(nt);
        gkey = c.take<int64_t>(nt); gpay = c.take<int64_t>(nt); prod = c.take<int64_t>(nt); poff = c.take<int64_t>(nt + 1);
        coff = c.take<int64_t>(nt + 1); ckey = c.take<int64_t>(nt); cws = c.take<int64_t>(nt);
        blk = c.take<int64_t>(scan_blocks(nt + 1) + 1);
        sort = c.take<char>(sort_scratch_bytes(nt));
    }
};

// ---- coGroup: the group table itself, as a CSR over two element columns ----------------------
// Over nt + 1 entries: the group's L and R, 0 past the groups, so that entry ng of their
// exclusive scans is the total.
__global__ void __launch_bounds__(kJoinThreads) k_cogroup_sizes(int64_t nt, const int64_t* __restrict__ hdr,
                                                                const uint32_t* __restrict__ gfirst,
                                                                const uint32_t* __restrict__ gmid, uint32_t* gl,
                                                                uint32_t* gr) {
    const int64_t ng = hdr[JH_NG];
    for (int64_t g = (int64_t)blockIdx.x * kJoinThreads + threadIdx.x; g <= nt; g += (int64_t)gridDim.x * kJoinThreads) {
        uint32_t L = 0, R = 0;
        if (g < ng) {
            const int64_t first = gfirst[g], end = g + 1 < ng ? (int64_t)gfirst[g + 1] : nt;
            const int64_t mid = gmid[g] == ~0u ? end : (int64_t)gmid[g];
            L = (uint32_t)(mid - first);
            R = (uint32_t)(end - mid);
        }
        gl[g] = L;
        gr[g] = R;
    }
}
struct CoGroupOut {
    int64_t *key, *start, *end, *loff, *roff;  // rows of this fire's groups (loff, roff: one more)
    int64_t *lelem, *relem;                    // the element columns from their row 0
    int64_t lbase, rbase;                      // elements ahead of this fire's: the offsets' base
};
// Group g's key, window and offsets; entry ng closes the offsets with the totals.
__global__ void __launch_bounds__(kJoinThreads) k_cogroup_groups(const int64_t* __restrict__ hdr,
                                                                 const uint32_t* __restrict__ gfirst,
                                                                 const int64_t* __restrict__ gkey,
                                                                 const uint64_t* __restrict__ gord, int64_t min_start,
                                                                 int64_t slide, int64_t size,
                                                                 const int64_t* __restrict__ loff,
                                                                 const int64_t* __restrict__ roff, CoGroupOut o) {
    const int64_t ng = hdr[JH_NG];
    for (int64_t g = (int64_t)blockIdx.x * kJoinThreads + threadIdx.x; g <= ng; g += (int64_t)gridDim.x * kJoinThreads) {
        o.loff[g] = o.lbase + loff[g];
        o.roff[g] = o.rbase + roff[g];
        if (g == ng) continue;
        const uint32_t first = gfirst[g];
        const int64_t ws = (int64_t)((uint64_t)min_start + gord[first] * (uint64_t)slide);
        o.key[g] = gkey[first];
        o.start[g] = ws;
        o.end[g] = ws + size;
    }
}
// Sorted tuple i of group g goes to its side's column at the group's offset plus its rank in
// the group's side (the sort kept each side in arrival order).
__global__ void __launch_bounds__(kJoinThreads) k_cogroup_elems(int64_t nt, const uint32_t* __restrict__ head,
                                                                const uint32_t* __restrict__ hex,
                                                                const uint32_t* __restrict__ gsrc,
                                                                const uint32_t* __restrict__ gfirst,
                                                                const uint32_t* __restrict__ gmid,
                                                                const int64_t* __restrict__ gpay,
                                                                const int64_t* __restrict__ loff,
                                                                const int64_t* __restrict__ roff, CoGroupOut o) {
    for (int64_t i = (int64_t)blockIdx.x * kJoinThreads + threadIdx.x; i < nt; i += (int64_t)gridDim.x * kJoinThreads) {
        const uint32_t g = hex[i] + head[i] - 1;
        if (gsrc[i] >> 31)
            o.relem[o.rbase + roff[g] + (i - (int64_t)gmid[g])] = gpay[i];
        else
            o.lelem[o.lbase + loff[g] + (i - (int64_t)gfirst[g])] = gpay[i];
    }
}

// provide(total, out): the caller's output columns for `total` rows (or an error).
typedef std::function<int(int64_t, JoinOut&, std::string&)> JoinProvide;
// provide(groups, left elements, right elements, out): the caller's CSR columns (or an error).
typedef std::function<int(int64_t, int64_t, int64_t, CoGroupOut&, std::string&)> CoGroupProvide;

// One call at a time per process: every call waits for its launches before it returns, so the
// per-device scratch is free for the next.
static std::mutex g_join_mu;
static Scratch g_scr_rec[64], g_scr_tup[64];

struct JoinStage {  // what stages count .. groups leave behind (g_join_mu held)
    RecArrays R;
    TupArrays T;
    int64_t nt = 0, min_start = 0;
    int64_t h[kJoinHdr];
};

// Stages count, emit, sort and groups: the sorted tuples (gkey, gord, gsrc, gpay) and the group
// table (head, hex, gfirst, gmid; hdr[JH_NG] groups, on the device).  st.nt = 0: nothing fired.
static int join_groups(const JoinIn& a, JoinStage& st, int64_t* n_tuples, hipStream_t s, std::string& why) {
    if (n_tuples) *n_tuples = 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { why = "window join: no device"; return GW_E_DEVICE; }
    RecArrays& R = st.R;
    TupArrays& T = st.T;
    int64_t* h = st.h;
    int rc = carve_from([&](Carve& c) { R.carve(c, a.n); }, g_scr_rec[dev], kJoinName, why);
    if (rc) return rc;
    hipLaunchKernelGGL(k_join_hdr_init, dim3(1), dim3(kJoinThreads), 0, s, R.hdr);
    hipLaunchKernelGGL(k_join_count, dim3(grid_for(a.n)), dim3(kJoinThreads), 0, s, a, R.cnt, R.hdr);
    hipError_t e = scan_excl<uint32_t, uint32_t>(R.cnt, R.toff, a.n, R.blk, R.hdr + JH_NT, s);
    if (e == hipSuccess) e = read_hdr(h, R.hdr, kJoinHdr, s);
    if (e != hipSuccess) return dev_fail(kJoinName, e, why);
    if (h[JH_FLAGS] & GW_DF_NO_TS) {
        why = "Record has Long.MIN_VALUE timestamp (= no timestamp marker)";
        return GW_E_NO_TIMESTAMP;
    }
    if (h[JH_FLAGS] & GW_DF_RANGE) { why = "window join: window bounds overflow int64"; return GW_E_RANGE; }
    const int64_t nt = h[JH_NT];
    if (n_tuples) *n_tuples = nt;
    if (nt > kSortMaxRecords) {
        why = "window join: more than 2^30 - 1 (record, fired window) tuples in one fire";
        return GW_E_UNSUPPORTED;
    }
    st.nt = nt;
    if (nt == 0) return GW_OK;
    const int64_t min_start = st.min_start = h[JH_MINS];
    const uint64_t min_kw = (uint64_t)h[JH_MINK];
    const int kbits = bit_length((uint64_t)h[JH_MAXK] - min_kw);
    const int obits = bit_length(((uint64_t)h[JH_MAXS] - (uint64_t)min_start) / (uint64_t)a.g.slide);
    if ((rc = carve_from([&](Carve& c) { T.carve(c, nt); }, g_scr_tup[dev], kJoinName, why))) return rc;
    const int gt = grid_for(nt);
    hipLaunchKernelGGL(k_join_emit, dim3(grid_for(a.n)), dim3(kJoinThreads), 0, s, a, R.toff, min_start, min_kw, T.kw0, T.ord,
                       T.src);
    if ((e = hipGetLastError()) != hipSuccess) return dev_fail(kJoinName, e, why);
    // by key word, then by window ordinal: both stable, so a group keeps left before right and
    // each side its arrival order
    int alt = 0;
    if ((e = sort_pairs_u64(T.kw0, T.v0, T.kw1, T.v1, nt, 0, kbits, T.sort, s, &alt, true)) != hipSuccess)
        return dev_fail(kJoinName, e, why);
    uint32_t* perm = alt ? T.v1 : T.v0;
    if (obits > 0) {
        uint32_t* other = alt ? T.v0 : T.v1;
        hipLaunchKernelGGL(k_join_gather_ord, dim3(gt), dim3(kJoinThreads), 0, s, nt, perm, T.ord, T.ord0);
        if ((e = sort_pairs_u64(T.ord0, perm, T.ord1, other, nt, 0, obits, T.sort, s, &alt, false)) != hipSuccess)
            return dev_fail(kJoinName, e, why);
        if (alt) perm = other;
    }
    hipLaunchKernelGGL(k_join_gather, dim3(gt), dim3(kJoinThreads), 0, s, a, nt, perm, T.ord, T.src, T.gkey, T.gord, T.gsrc,
                       T.gpay);
    hipLaunchKernelGGL(k_join_heads, dim3(gt), dim3(kJoinThreads), 0, s, nt, T.gkey, T.gord, T.head);
    if ((e = scan_excl<uint32_t, uint32_t>(T.head, T.hex, nt, T.blk, R.hdr + JH_NG, s)) != hipSuccess) return dev_fail(kJoinName, e, why);
    if ((e = hipMemsetAsync(T.gmid, 0xFF, (size_t)nt * 4, s)) != hipSuccess) return dev_fail(kJoinName, e, why);
    hipLaunchKernelGGL(k_join_group_fill, dim3(gt), dim3(kJoinThreads), 0, s, nt, T.head, T.hex, T.gsrc, T.gfirst, T.gmid);
    if ((e = hipGetLastError()) != hipSuccess) return dev_fail(kJoinName, e, why);
    return GW_OK;
}

template <int MODE>
static void launch_expand(bool vec, int64_t nblk, hipStream_t s, int64_t total, int shift, int64_t nc, const TupArrays& T,
                          int64_t size, const JoinOut& out) {
    if (vec)
        hipLaunchKernelGGL((k_join_expand<true, MODE>), dim3((unsigned)nblk), dim3(kJoinThreads), 0, s, total, shift, nc,
                           T.coff, T.cfirst, T.crb, T.cR, T.ckey, T.cws, T.gpay, size, out);
    else
        hipLaunchKernelGGL((k_join_expand<false, MODE>), dim3((unsigned)nblk), dim3(kJoinThreads), 0, s, total, shift, nc,
                           T.coff, T.cfirst, T.crb, T.cR, T.ckey, T.cws, T.gpay, size, out);
}

// mode: GW_JOIN_MODE_INNER .. FULL_OUTER; the rows carry null_payload for a lacking side, and
// out.present (when provide leaves one) says which sides a row has.  max_rows: the byte bound.
int join_run(const JoinIn& a, int mode, int64_t null_payload, int64_t max_rows, const JoinProvide& provide,
             int64_t* n_pairs, int64_t* n_tuples, hipStream_t s, std::string& why, const TimedPair& times = TimedPair()) {
    *n_pairs = 0;
    std::lock_guard<std::mutex> lock(g_join_mu);
    JoinStage st;
    int rc = join_groups(a, st, n_tuples, s, why);
    if (rc) return rc;
    const int64_t nt = st.nt;
    if (nt == 0) {
        JoinOut none{};
        return provide(0, none, why);
    }
    RecArrays& R = st.R;
    TupArrays& T = st.T;
    int64_t* h = st.h;
    const int gt = grid_for(nt);
    hipError_t e;
    hipLaunchKernelGGL(k_join_group_prod, dim3(gt), dim3(kJoinThreads), 0, s, nt, R.hdr, T.gfirst, T.gmid, mode, T.prod, T.ne);
    if ((e = scan_excl<int64_t, int64_t>(T.prod, T.poff, nt, T.blk, R.hdr + JH_TOTAL, s)) != hipSuccess) return dev_fail(kJoinName, e, why);
    if ((e = scan_excl<uint32_t, uint32_t>(T.ne, T.cidx, nt, T.blk, R.hdr + JH_NC, s)) != hipSuccess) return dev_fail(kJoinName, e, why);
    hipLaunchKernelGGL(k_join_compact, dim3(gt), dim3(kJoinThreads), 0, s, nt, R.hdr, T.gfirst, T.gmid, T.prod, T.poff, T.cidx,
                       T.gkey, T.gord, st.min_start, a.g.slide, T.coff, T.cfirst, T.crb, T.cR, T.ckey, T.cws);
    e = hipGetLastError();
    if (e == hipSuccess) e = read_hdr(h, R.hdr, kJoinHdr, s);
    if (e != hipSuccess) return dev_fail(kJoinName, e, why);
    const int64_t total = h[JH_TOTAL], nc = h[JH_NC];
    if (total > max_rows) { why = "window join: the pairs of one fire exceed int64 bytes"; return GW_E_RANGE; }
    *n_pairs = total;
    JoinOut out{};
    if ((rc = provide(total, out, why))) return rc;
    if (total == 0) return GW_OK;
    out.null_payload = null_payload;
    const auto [vec, shift] = expand_alignment(out.col);
    const int64_t nblk = (total + shift + kExpTile - 1) / kExpTile;
    times.begin(s);
    switch (mode) {
        case GW_JOIN_MODE_INNER:  // every row has both sides
            if (out.present && (e = hipMemsetAsync(out.present, 3, (size_t)total, s)) != hipSuccess) return dev_fail(kJoinName, e, why);
            launch_expand<GW_JOIN_MODE_INNER>(vec, nblk, s, total, shift, nc, T, a.g.size, out);
            break;
        case GW_JOIN_MODE_LEFT_OUTER: launch_expand<GW_JOIN_MODE_LEFT_OUTER>(vec, nblk, s, total, shift, nc, T, a.g.size, out); break;
        case GW_JOIN_MODE_RIGHT_OUTER: launch_expand<GW_JOIN_MODE_RIGHT_OUTER>(vec, nblk, s, total, shift, nc, T, a.g.size, out); break;
        default: launch_expand<GW_JOIN_MODE_FULL_OUTER>(vec, nblk, s, total, shift, nc, T, a.g.size, out); break;
    }
    e = hipGetLastError();
    times.end(s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);  // the scratch is free for the next call
    if (e != hipSuccess) return dev_fail(kJoinName, e, why);
    return GW_OK;
}

// The fired groups as a CSR: n[0] groups, n[1] left and n[2] right elements.
int cogroup_run(const JoinIn& a, const CoGroupProvide& provide, int64_t* n, int64_t* n_tuples, hipStream_t s,
                std::string& why, const TimedPair& times = TimedPair()) {
    n[0] = n[1] = n[2] = 0;
    std::lock_guard<std::mutex> lock(g_join_mu);
    JoinStage st;
    int rc = join_groups(a, st, n_tuples, s, why);
    if (rc) return rc;
    const int64_t nt = st.nt;
    CoGroupOut out{};
    if (nt == 0) return provide(0, 0, 0, out, why);
    RecArrays& R = st.R;
    TupArrays& T = st.T;
    int64_t* h = st.h;
    uint32_t *gl = T.ne, *gr = T.cidx;  // per group L and R, nt + 1 entries
    int64_t *loff = T.poff, *roff = T.coff;
    hipError_t e;
    hipLaunchKernelGGL(k_cogroup_sizes, dim3(grid_for(nt + 1)), dim3(kJoinThreads), 0, s, nt, R.hdr, T.gfirst, T.gmid, gl, gr);
    if ((e = scan_excl<uint32_t, int64_t>(gl, loff, nt + 1, T.blk, R.hdr + JH_TOTAL, s)) != hipSuccess) return dev_fail(kJoinName, e, why);
    if ((e = scan_excl<uint32_t, int64_t>(gr, roff, nt + 1, T.blk, R.hdr + JH_NC, s)) != hipSuccess) return dev_fail(kJoinName, e, why);
    if ((e = read_hdr(h, R.hdr, kJoinHdr, s)) != hipSuccess) return dev_fail(kJoinName, e, why);
    const int64_t ng = h[JH_NG];
    n[0] = ng;
    n[1] = h[JH_TOTAL];
    n[2] = h[JH_NC];
    if ((rc = provide(n[0], n[1], n[2], out, why))) return rc;
    times.begin(s);
    hipLaunchKernelGGL(k_cogroup_groups, dim3(grid_for(ng + 1)), dim3(kJoinThreads), 0, s, R.hdr, T.gfirst, T.gkey, T.gord,
                       st.min_start, a.g.slide, a.g.size, loff, roff, out);
    hipLaunchKernelGGL(k_cogroup_elems, dim3(grid_for(nt)), dim3(kJoinThreads), 0, s, nt, T.head, T.hex, T.gsrc, T.gfirst,
                       T.gmid, T.gpay, loff, roff, out);
    e = hipGetLastError();
    times.end(s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);  // the scratch is free for the next call
    if (e != hipSuccess) return dev_fail(kJoinName, e, why);
    return GW_OK;
}

// ---- operator state: the late filter (the stable compaction behind it is k_compact3) ---------
// keep[i] = 1 for the records that stay: at ingest those with a window still open at wm (the
// others are late, counted in hdr[JH_LATE]); after a fire the same test at the new watermark.
__global__ void __launch_bounds__(kJoinThreads) k_join_filter(int64_t n, const int64_t* __restrict__ ts, JoinGeom g,
                                                              int64_t wm, uint32_t* keep, int64_t* hdr) {
    using ull = unsigned long long;
    __shared__ uint64_t s_late[4], s_flags[4];
    uint64_t late = 0, flags = 0;
    for (int64_t i = (int64_t)blockIdx.x * kJoinThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kJoinThreads) {
        int64_t ls;
        int nw;
        const unsigned f = join_windows(g, ts[i], ls, nw);
        flags |= f;
        const bool k = !f && ls + (g.size - 1) > wm;
        late += !f && !k;
        keep[i] = k;
    }
    late = wave_sum(late);
    flags = wave_ior(flags);
    if (__lane_id() == 0) {
        s_late[threadIdx.x >> 6] = late;
        s_flags[threadIdx.x >> 6] = flags;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < 4; ++w) {
        late += s_late[w];
        flags |= s_flags[w];
    }
    if (late) atomicAdd((ull*)&hdr[JH_LATE], (ull)late);
    if (flags) atomicOr((ull*)&hdr[JH_FLAGS], (ull)flags);
}

}  // namespace gw

using namespace gw;

// ---- the operator ---------------------------------------------------------------------------
struct gw_join {
    gw_join_config cfg{};
    JoinGeom g{};
    OpError er{kJoinName};
    OpStream os;
    DevCols<3> log[2], alt, stage;
    int64_t n_log[2] = {0, 0};
    RowBuf rows{true};  // the pending pairs; the byte column is the rows' `present`
    // gw_join_set_mode; `touched` once an ingest or a watermark has come
    int32_t mode = GW_JOIN_MODE_INNER;
    int64_t null_payload = 0;
    bool touched = false;
    // coGroup mode: pending groups (key, start, end, loff, roff; the offsets one row more) and
    // the two element columns, all from row 0
    DevCols<5> cg;
    DevCols<1> cg_elem[2];
    int64_t cg_n[3] = {0, 0, 0};  // groups, left elements, right elements
    DevBuf<char> scr;
    int64_t wm = INT64_MIN, late = 0, max_batch = 0;
    gw_join_stats st{};

    // The records of (key, ts, pay)[0..n) with a window open at `w`, in order, to dst columns
    // from row `at`; *kept and *dropped their numbers.  One synchronisation, at its end, so the
    // scratch (hdr, keep, off, the scan's block sums) is never in use when the next call grows it.
    int filter_into(int64_t n, const int64_t* key, const int64_t* ts, const int64_t* pay, int64_t w, int64_t* const* dst,
                    int64_t at, int64_t* kept, int64_t* dropped) {
        hipStream_t stream = os.stream;
        RecArrays R;
        int rc = carve_from([&](Carve& c) { R.carve(c, n); }, scr, er, nullptr);
        if (rc) return rc;
        hipLaunchKernelGGL(k_join_hdr_init, dim3(1), dim3(kJoinThreads), 0, stream, R.hdr);
        hipLaunchKernelGGL(k_join_filter, dim3(grid_for(n)), dim3(kJoinThreads), 0, stream, n, ts, g, w, R.cnt, R.hdr);
        hipError_t e = scan_excl<uint32_t, uint32_t>(R.cnt, R.toff, n, R.blk, R.hdr + JH_KEPT, stream);
        if (e != hipSuccess) return er.dev_fail(e);
        Cols3 c{{key, ts, pay}, {dst[0] + at, dst[1] + at, dst[2] + at}};
        hipLaunchKernelGGL(k_compact3, dim3(grid_for(n)), dim3(kJoinThreads), 0, stream, n, R.cnt, R.toff, c);
        int64_t h[kJoinHdr];
        e = hipGetLastError();
        if (e == hipSuccess) e = read_hdr(h, R.hdr, kJoinHdr, stream);
        if (e != hipSuccess) return er.dev_fail(e);
        if (h[JH_FLAGS] & GW_DF_NO_TS)
            return er.fail(GW_E_NO_TIMESTAMP, "Record has Long.MIN_VALUE timestamp (= no timestamp marker)");
        if (h[JH_FLAGS] & GW_DF_RANGE) return er.fail(GW_E_RANGE, "window join: window bounds overflow int64");
        *kept = h[JH_KEPT];
        *dropped = h[JH_LATE];
        return GW_OK;
    }
    int reserve_log(int side, int64_t need) {
        if (need <= log[side].cap) return GW_OK;
        const int64_t cap = std::max<int64_t>(need, 2 * log[side].cap);
        if (log[side].reserve_keep(cap, 0, n_log[side], os.stream) != hipSuccess) {
            (void)hipGetLastError();
            return er.fail(GW_E_OOM, "window join: out of device memory growing the %s log", side ? "right" : "left");
        }
        ++st.log_growths;
        return GW_OK;
    }
    // device columns, already ordered behind their producer
    int ingest_cols(int side, int64_t n, const int64_t* key, const int64_t* ts, const int64_t* pay) {
        for (int64_t at = 0; at < n; at += max_batch) {
            const int64_t m = std::min(max_batch, n - at);
            int rc = reserve_log(side, n_log[side] + m);
            if (rc) return rc;
            int64_t kept = 0, dropped = 0;
            if ((rc = filter_into(m, key + at, ts + at, pay + at, wm, log[side].col, n_log[side], &kept, &dropped))) return rc;
            n_log[side] += kept;
            late += dropped;
        }
        return GW_OK;
    }
    // room for `more` groups and elements behind the pending CSR (the offsets: one row more)
    int reserve_cogroup(const int64_t more[3]) {
        hipError_t e = hipSuccess;
        const int64_t need_g = cg_n[0] + more[0] + 1;
        if (need_g > cg.cap) e = cg.reserve_keep(std::max<int64_t>(need_g, 2 * cg.cap), 0, cg.cap ? cg_n[0] + 1 : 0, os.stream);
        for (int sd = 0; sd < 2 && e == hipSuccess; ++sd) {
            const int64_t need = cg_n[1 + sd] + more[1 + sd];
            if (need > cg_elem[sd].cap)
                e = cg_elem[sd].reserve_keep(std::max<int64_t>(need, 2 * cg_elem[sd].cap), 0, cg_n[1 + sd], os.stream);
        }
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return er.fail(GW_E_OOM, "window join: out of device memory for %lld pending groups", (long long)(cg_n[0] + more[0]));
        }
        return GW_OK;
    }
    int advance(int64_t w, int64_t* pairs_fired) {
        if (pairs_fired) *pairs_fired = 0;
        touched = true;
        if (w <= wm) return GW_OK;  // a watermark that does not advance is ignored
        int64_t fired = 0, tuples = 0;
        // a side without records still fires where the mode keeps the other side's
        const bool keep_l = mode == GW_JOIN_MODE_COGROUP || (mode & GW_JOIN_MODE_LEFT_OUTER);
        const bool keep_r = mode == GW_JOIN_MODE_COGROUP || (mode & GW_JOIN_MODE_RIGHT_OUTER);
        if ((n_log[0] > 0 || keep_r) && (n_log[1] > 0 || keep_l) && n_log[0] + n_log[1] > 0) {
            JoinIn a{};
            for (int sd = 0; sd < 2; ++sd) {
                a.key[sd] = log[sd][0];
                a.ts[sd] = log[sd][1];
                a.pay[sd] = log[sd][2];
            }
            a.n_l = n_log[0];
            a.n = n_log[0] + n_log[1];
            a.g = g;
            a.w0 = wm;
            a.w1 = w;
            std::string why;
            int rc;
            if (mode == GW_JOIN_MODE_COGROUP) {
                int64_t n3[3];
                rc = cogroup_run(a, [&](int64_t ng, int64_t nl, int64_t nr, CoGroupOut& o, std::string&) {
                    if (ng == 0) return (int)GW_OK;
                    const int64_t more[3] = {ng, nl, nr};
                    int r = reserve_cogroup(more);
                    if (r) return r;
                    o = CoGroupOut{cg[0] + cg_n[0], cg[1] + cg_n[0], cg[2] + cg_n[0], cg[3] + cg_n[0], cg[4] + cg_n[0],
                                   cg_elem[0][0], cg_elem[1][0], cg_n[1], cg_n[2]};
                    return (int)GW_OK;
                }, n3, &tuples, os.stream, why);
                if (rc) return er.failed ? rc : er.fail(rc, "%s", why.c_str());
                fired = n3[0];
                for (int c = 0; c < 3; ++c) cg_n[c] += n3[c];
            } else {
                rc = join_run(a, mode, null_payload, INT64_MAX / (mode ? 41 : 40), [&](int64_t total, JoinOut& o, std::string&) {
                    if (rows.reserve(total, os.stream) != hipSuccess) {
                        (void)hipGetLastError();
                        return er.fail(GW_E_OOM, "window join: out of device memory for %lld pending pairs",
                                       (long long)(rows.pending + total));
                    }
                    o.present = rows.tail(o.col);
                    return (int)GW_OK;
                }, &fired, &tuples, os.stream, why);
                if (rc) return er.failed ? rc : er.fail(rc, "%s", why.c_str());
                rows.pending += fired;
            }
        }
        // the records whose last window has fired leave the logs
        for (int sd = 0; sd < 2; ++sd) {
            if (n_log[sd] == 0) continue;
            if (alt.cap < n_log[sd] && alt.reserve_keep(std::max(n_log[sd], log[sd].cap), 0, 0, os.stream) != hipSuccess) {
                (void)hipGetLastError();
                return er.fail(GW_E_OOM, "window join: out of device memory compacting a log");
            }
            int64_t kept = 0, dropped = 0;
            const int rc = filter_into(n_log[sd], log[sd][0], log[sd][1], log[sd][2], w, alt.col, 0, &kept, &dropped);
            if (rc) return rc;
            std::swap(log[sd], alt);
            n_log[sd] = kept;
        }
        wm = w;
        ++st.fires;
        st.pairs_fired += fired;
        st.last_fire_tuples = tuples;
        if (pairs_fired) *pairs_fired = fired;
        return GW_OK;
    }
};

namespace {

int join_geom(int64_t size, int64_t slide, int64_t offset, JoinGeom& g, std::string& why) {
    auto ab = [](int64_t v) { return v < 0 ? -v : v; };
    if (size <= 0 || slide <= 0 || offset == INT64_MIN || ab(offset) >= slide) {
        why = "window join: parameters must satisfy size > 0, slide > 0 and abs(offset) < slide";
        return GW_E_INVALID;
    }
    if ((size - 1) / slide + 1 > GW_JOIN_MAX_WINDOWS) {
        why = "window join: more than GW_JOIN_MAX_WINDOWS (64) windows per record";
        return GW_E_UNSUPPORTED;
    }
    g = JoinGeom{size, slide, offset};
    return GW_OK;
}

int join_args(int64_t n_l, int64_t n_r, int64_t size, int64_t slide, int64_t offset, int64_t cap, const int64_t* n_out,
              JoinGeom& g, std::string& why) {
    if (!n_out || n_l < 0 || n_r < 0 || cap < 0) { why = "window join: bad argument"; return GW_E_INVALID; }
    return join_geom(size, slide, offset, g, why);
}

}  // namespace

extern "C" {

// gw_window_join_device / _outer_device, with the expand kernel's time in *expand_ms when that
// is not null.  max_rows: INT64_MAX / bytes per row.
static int join_device(int64_t n_l, const int64_t* d_lkey, const int64_t* d_lts, const int64_t* d_lpay, int64_t n_r,
                       const int64_t* d_rkey, const int64_t* d_rts, const int64_t* d_rpay, int64_t size, int64_t slide,
                       int64_t offset, int64_t w0, int64_t w1, int32_t mode, int64_t null_payload, int64_t max_rows,
                       int64_t* d_key_out, int64_t* d_start_out, int64_t* d_end_out, int64_t* d_lpay_out,
                       int64_t* d_rpay_out, uint8_t* d_present_out, int64_t cap, int64_t* n_out, void* stream,
                       double* expand_ms) {
    JoinGeom g;
    std::string why;
    int rc = join_args(n_l, n_r, size, slide, offset, cap, n_out, g, why);
    if (rc) { set_last_error(why); return rc; }
    *n_out = 0;
    if (expand_ms) *expand_ms = 0;
    if (mode < GW_JOIN_MODE_INNER || mode > GW_JOIN_MODE_FULL_OUTER) {
        set_last_error("window join: unknown mode");
        return GW_E_INVALID;
    }
    // a side without records leaves rows only where the mode keeps the other side's
    if ((n_l == 0 && !(mode & GW_JOIN_MODE_RIGHT_OUTER)) || (n_r == 0 && !(mode & GW_JOIN_MODE_LEFT_OUTER)) ||
        n_l + n_r == 0 || w1 <= w0)
        return GW_OK;
    if ((n_l > 0 && (!d_lkey || !d_lts || !d_lpay)) || (n_r > 0 && (!d_rkey || !d_rts || !d_rpay)) ||
        (cap > 0 && (!d_key_out || !d_start_out || !d_end_out || !d_lpay_out || !d_rpay_out))) {
        set_last_error("window join: null column");
        return GW_E_INVALID;
    }
    if (n_l > INT32_MAX || n_r > INT32_MAX) {
        set_last_error("window join: more than 2^31 - 1 records on one side");
        return GW_E_UNSUPPORTED;
    }
    TimedPair t;
    if (expand_ms && t.create() != hipSuccess) { set_last_error("window join: hipEventCreate"); return GW_E_DEVICE; }
    JoinIn a{{d_lkey, d_rkey}, {d_lts, d_rts}, {d_lpay, d_rpay}, n_l, n_l + n_r, g, w0, w1};
    int64_t pairs = 0;
    rc = join_run(a, mode, null_payload, max_rows, [&](int64_t total, JoinOut& o, std::string& w) {
        *n_out = total;
        if (total > cap) { w = "window join: output arrays too small"; return (int)GW_E_OUTPUT_FULL; }
        o = JoinOut{{d_key_out, d_start_out, d_end_out, d_lpay_out, d_rpay_out}, d_present_out, 0};
        return (int)GW_OK;
    }, &pairs, nullptr, (hipStream_t)stream, why, t);
    float ms = 0;
    if (expand_ms && rc == GW_OK && pairs > 0 && t.elapsed(&ms) == hipSuccess) *expand_ms = ms;
    if (rc) set_last_error(why);
    return rc;
}

int gw_window_join_device(int64_t n_l, const int64_t* d_lkey, const int64_t* d_lts, const int64_t* d_lpay, int64_t n_r,
                          const int64_t* d_rkey, const int64_t* d_rts, const int64_t* d_rpay, int64_t size, int64_t slide,
                          int64_t offset, int64_t w0, int64_t w1, int64_t* d_key_out, int64_t* d_start_out,
                          int64_t* d_end_out, int64_t* d_lpay_out, int64_t* d_rpay_out, int64_t cap, int64_t* n_out,
                          void* stream) {
    return join_device(n_l, d_lkey, d_lts, d_lpay, n_r, d_rkey, d_rts, d_rpay, size, slide, offset, w0, w1,
                       GW_JOIN_MODE_INNER, 0, INT64_MAX / 40, d_key_out, d_start_out, d_end_out, d_lpay_out, d_rpay_out,
                       nullptr, cap, n_out, stream, nullptr);
}

int gw_window_join_outer_device(int64_t n_l, const int64_t* d_lkey, const int64_t* d_lts, const int64_t* d_lpay,
                                int64_t n_r, const int64_t* d_rkey, const int64_t* d_rts, const int64_t* d_rpay,
                                int64_t size, int64_t slide, int64_t offset, int64_t w0, int64_t w1, int32_t mode,
                                int64_t null_payload, int64_t* d_key_out, int64_t* d_start_out, int64_t* d_end_out,
                                int64_t* d_lpay_out, int64_t* d_rpay_out, uint8_t* d_present_out, int64_t cap,
                                int64_t* n_out, void* stream) {
    return join_device(n_l, d_lkey, d_lts, d_lpay, n_r, d_rkey, d_rts, d_rpay, size, slide, offset, w0, w1, mode,
                       null_payload, INT64_MAX / 41, d_key_out, d_start_out, d_end_out, d_lpay_out, d_rpay_out,
                       d_present_out, cap, n_out, stream, nullptr);
}

int gw_window_join_outer_device_timed(int64_t n_l, const int64_t* d_lkey, const int64_t* d_lts, const int64_t* d_lpay,
                                      int64_t n_r, const int64_t* d_rkey, const int64_t* d_rts, const int64_t* d_rpay,
                                      int64_t size, int64_t slide, int64_t offset, int64_t w0, int64_t w1, int32_t mode,
                                      int64_t null_payload, int64_t* d_key_out, int64_t* d_start_out,
                                      int64_t* d_end_out, int64_t* d_lpay_out, int64_t* d_rpay_out,
                                      uint8_t* d_present_out, int64_t cap, int64_t* n_out, void* stream,
                                      double* expand_ms) {
    if (!expand_ms) { set_last_error("window join: null expand_ms"); return GW_E_INVALID; }
    return join_device(n_l, d_lkey, d_lts, d_lpay, n_r, d_rkey, d_rts, d_rpay, size, slide, offset, w0, w1, mode,
                       null_payload, INT64_MAX / 41, d_key_out, d_start_out, d_end_out, d_lpay_out, d_rpay_out,
                       d_present_out, cap, n_out, stream, expand_ms);
}

// gw_window_cogroup_device, with the time of its two writer kernels in *write_ms when not null.
static int cogroup_device(int64_t n_l, const int64_t* d_lkey, const int64_t* d_lts, const int64_t* d_lpay, int64_t n_r,
                          const int64_t* d_rkey, const int64_t* d_rts, const int64_t* d_rpay, int64_t size,
                          int64_t slide, int64_t offset, int64_t w0, int64_t w1, int64_t* d_key_out,
                          int64_t* d_start_out, int64_t* d_end_out, int64_t* d_loff_out, int64_t* d_roff_out,
                          int64_t* d_lelem_out, int64_t cap_left, int64_t* d_relem_out, int64_t cap_right,
                          int64_t cap_groups, int64_t* n_out, void* stream, double* write_ms) {
    JoinGeom g;
    std::string why;
    int rc = join_args(n_l, n_r, size, slide, offset, std::min(cap_groups, std::min(cap_left, cap_right)), n_out, g, why);
    if (rc) { set_last_error(why); return rc; }
    n_out[0] = n_out[1] = n_out[2] = 0;
    if (write_ms) *write_ms = 0;
    if ((n_l > 0 && (!d_lkey || !d_lts || !d_lpay)) || (n_r > 0 && (!d_rkey || !d_rts || !d_rpay)) || !d_loff_out ||
        !d_roff_out || (cap_groups > 0 && (!d_key_out || !d_start_out || !d_end_out)) || (cap_left > 0 && !d_lelem_out) ||
        (cap_right > 0 && !d_relem_out)) {
        set_last_error("window coGroup: null column");
        return GW_E_INVALID;
    }
    if (n_l > INT32_MAX || n_r > INT32_MAX) {
        set_last_error("window join: more than 2^31 - 1 records on one side");
        return GW_E_UNSUPPORTED;
    }
    hipStream_t s = (hipStream_t)stream;
    auto no_groups = [&]() {  // a CSR of no groups: loff[0] = roff[0] = 0
        hipError_t e = hipMemsetAsync(d_loff_out, 0, 8, s);
        if (e == hipSuccess) e = hipMemsetAsync(d_roff_out, 0, 8, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) { set_last_error(std::string("window coGroup: ") + hipGetErrorString(e)); return (int)GW_E_DEVICE; }
        return (int)GW_OK;
    };
    if (n_l + n_r == 0 || w1 <= w0) return no_groups();
    TimedPair t;
    if (write_ms && t.create() != hipSuccess) { set_last_error("window coGroup: hipEventCreate"); return GW_E_DEVICE; }
    JoinIn a{{d_lkey, d_rkey}, {d_lts, d_rts}, {d_lpay, d_rpay}, n_l, n_l + n_r, g, w0, w1};
    bool wrote = false;
    rc = cogroup_run(a, [&](int64_t ng, int64_t nl, int64_t nr, CoGroupOut& o, std::string& w) {
        n_out[0] = ng; n_out[1] = nl; n_out[2] = nr;
        if (ng > cap_groups || nl > cap_left || nr > cap_right) {
            w = "window coGroup: output arrays too small";
            return (int)GW_E_OUTPUT_FULL;
        }
        if (ng == 0) return no_groups();
        o = CoGroupOut{d_key_out, d_start_out, d_end_out, d_loff_out, d_roff_out, d_lelem_out, d_relem_out, 0, 0};
        wrote = true;
        return (int)GW_OK;
    }, n_out, nullptr, s, why, t);
    float ms = 0;
    if (write_ms && rc == GW_OK && wrote && t.elapsed(&ms) == hipSuccess) *write_ms = ms;
    if (rc) set_last_error(why);
    return rc;
}

int gw_window_cogroup_device(int64_t n_l, const int64_t* d_lkey, const int64_t* d_lts, const int64_t* d_lpay, int64_t n_r,
                             const int64_t* d_rkey, const int64_t* d_rts, const int64_t* d_rpay, int64_t size,
                             int64_t slide, int64_t offset, int64_t w0, int64_t w1, int64_t* d_key_out,
                             int64_t* d_start_out, int64_t* d_end_out, int64_t* d_loff_out, int64_t* d_roff_out,
                             int64_t* d_lelem_out, int64_t cap_left, int64_t* d_relem_out, int64_t cap_right,
                             int64_t cap_groups, int64_t* n_out, void* stream) {
    return cogroup_device(n_l, d_lkey, d_lts, d_lpay, n_r, d_rkey, d_rts, d_rpay, size, slide, offset, w0, w1, d_key_out,
                          d_start_out, d_end_out, d_loff_out, d_roff_out, d_lelem_out, cap_left, d_relem_out, cap_right,
                          cap_groups, n_out, stream, nullptr);
}

int gw_window_cogroup_device_timed(int64_t n_l, const int64_t* d_lkey, const int64_t* d_lts, const int64_t* d_lpay,
                                   int64_t n_r, const int64_t* d_rkey, const int64_t* d_rts, const int64_t* d_rpay,
                                   int64_t size, int64_t slide, int64_t offset, int64_t w0, int64_t w1,
                                   int64_t* d_key_out, int64_t* d_start_out, int64_t* d_end_out, int64_t* d_loff_out,
                                   int64_t* d_roff_out, int64_t* d_lelem_out, int64_t cap_left, int64_t* d_relem_out,
                                   int64_t cap_right, int64_t cap_groups, int64_t* n_out, void* stream,
                                   double* write_ms) {
    if (!write_ms) { set_last_error("window coGroup: null write_ms"); return GW_E_INVALID; }
    return cogroup_device(n_l, d_lkey, d_lts, d_lpay, n_r, d_rkey, d_rts, d_rpay, size, slide, offset, w0, w1, d_key_out,
                          d_start_out, d_end_out, d_loff_out, d_roff_out, d_lelem_out, cap_left, d_relem_out, cap_right,
                          cap_groups, n_out, stream, write_ms);
}

int gw_window_join_device_timed(int64_t n_l, const int64_t* d_lkey, const int64_t* d_lts, const int64_t* d_lpay,
                                int64_t n_r, const int64_t* d_rkey, const int64_t* d_rts, const int64_t* d_rpay,
                                int64_t size, int64_t slide, int64_t offset, int64_t w0, int64_t w1, int64_t* d_key_out,
                                int64_t* d_start_out, int64_t* d_end_out, int64_t* d_lpay_out, int64_t* d_rpay_out,
                                int64_t cap, int64_t* n_out, void* stream, double* expand_ms) {
    if (!expand_ms) { set_last_error("window join: null expand_ms"); return GW_E_INVALID; }
    return join_device(n_l, d_lkey, d_lts, d_lpay, n_r, d_rkey, d_rts, d_rpay, size, slide, offset, w0, w1,
                       GW_JOIN_MODE_INNER, 0, INT64_MAX / 40, d_key_out, d_start_out, d_end_out, d_lpay_out, d_rpay_out,
                       nullptr, cap, n_out, stream, expand_ms);
}

}  // extern "C"

// ---- the host entry points ------------------------------------------------------------------
namespace {

struct HostTup {
    int64_t start, key, pay;
    int side;
};
// The (record, fired window) tuples of both sides sorted into groups: windows ascending, keys
// ascending, left before right, each side in arrival order.
int host_tuples(const JoinGeom& g, int64_t n_l, const int64_t* lkey, const int64_t* lts, const int64_t* lpay, int64_t n_r,
                const int64_t* rkey, const int64_t* rts, const int64_t* rpay, int64_t w0, int64_t w1,
                std::vector<HostTup>& t) {
    const int64_t* keys[2] = {lkey, rkey};
    const int64_t* tss[2] = {lts, rts};
    const int64_t* pays[2] = {lpay, rpay};
    const int64_t ns[2] = {n_l, n_r};
    for (int side = 0; side < 2; ++side)
        for (int64_t i = 0; i < ns[side]; ++i) {
            int64_t ls;
            int nw;
            const unsigned f = join_windows(g, tss[side][i], ls, nw);
            if (f & GW_DF_NO_TS) {
                set_last_error("Record has Long.MIN_VALUE timestamp (= no timestamp marker)");
                return GW_E_NO_TIMESTAMP;
            }
            if (f) { set_last_error("window join: window bounds overflow int64"); return GW_E_RANGE; }
            uint64_t m = join_fired(g, ls, nw, w0, w1);
            for (int k = 0; m; ++k, m >>= 1)
                if (m & 1) t.push_back({ls - (int64_t)k * g.slide, keys[side][i], pays[side][i], side});
        }
    if ((int64_t)t.size() > kSortMaxRecords) {
        set_last_error("window join: more than 2^30 - 1 (record, fired window) tuples in one fire");
        return GW_E_UNSUPPORTED;
    }
    // left tuples were made first, each side in arrival order: stability keeps both
    std::stable_sort(t.begin(), t.end(), [](const HostTup& x, const HostTup& y) {
        return x.start != y.start ? x.start < y.start : x.key < y.key;
    });
    return GW_OK;
}
// The group starting at tuple i: its end and its number of left tuples.
size_t host_group(const std::vector<HostTup>& t, size_t i, size_t& l) {
    size_t j = i;
    l = 0;
    for (; j < t.size() && t[j].start == t[i].start && t[j].key == t[i].key; ++j) l += t[j].side == 0;
    return j;
}

int join_host(int64_t n_l, const int64_t* lkey, const int64_t* lts, const int64_t* lpay, int64_t n_r, const int64_t* rkey,
              const int64_t* rts, const int64_t* rpay, int64_t size, int64_t slide, int64_t offset, int64_t w0, int64_t w1,
              int32_t mode, int64_t null_payload, int64_t max_rows, int64_t* key_out, int64_t* start_out, int64_t* end_out,
              int64_t* lpay_out, int64_t* rpay_out, uint8_t* present_out, int64_t cap, int64_t* n_out) {
    JoinGeom g;
    std::string why;
    int rc = join_args(n_l, n_r, size, slide, offset, cap, n_out, g, why);
    if (rc) { set_last_error(why); return rc; }
    *n_out = 0;
    if (mode < GW_JOIN_MODE_INNER || mode > GW_JOIN_MODE_FULL_OUTER) {
        set_last_error("window join: unknown mode");
        return GW_E_INVALID;
    }
    const bool keep_l = mode & GW_JOIN_MODE_LEFT_OUTER, keep_r = mode & GW_JOIN_MODE_RIGHT_OUTER;
    if ((n_l == 0 && !keep_r) || (n_r == 0 && !keep_l) || n_l + n_r == 0 || w1 <= w0) return GW_OK;
    if ((n_l > 0 && (!lkey || !lts || !lpay)) || (n_r > 0 && (!rkey || !rts || !rpay)) ||
        (cap > 0 && (!key_out || !start_out || !end_out || !lpay_out || !rpay_out))) {
        set_last_error("window join: null column");
        return GW_E_INVALID;
    }
    try {
        std::vector<HostTup> t;
        if ((rc = host_tuples(g, n_l, lkey, lts, lpay, n_r, rkey, rts, rpay, w0, w1, t))) return rc;
        const size_t n = t.size();
        auto rows = [&](size_t l, size_t r) -> __int128 {
            if (l && r) return (__int128)l * (__int128)r;
            return l ? (keep_l ? l : 0) : (keep_r ? r : 0);
        };
        __int128 total = 0;
        for (size_t i = 0, l; i < n;) {
            const size_t j = host_group(t, i, l);
            total += rows(l, j - i - l);
            i = j;
        }
        if (total > (__int128)max_rows) {
            set_last_error("window join: the pairs of one fire exceed int64 bytes");
            return GW_E_RANGE;
        }
        *n_out = (int64_t)total;
        if ((int64_t)total > cap) { set_last_error("window join: output arrays too small"); return GW_E_OUTPUT_FULL; }
        int64_t o = 0;
        auto row = [&](const HostTup& h, const HostTup* x, const HostTup* y) {
            key_out[o] = h.key;
            start_out[o] = h.start;
            end_out[o] = h.start + g.size;
            lpay_out[o] = x ? x->pay : null_payload;
            rpay_out[o] = y ? y->pay : null_payload;
            if (present_out) present_out[o] = (uint8_t)((x ? 1 : 0) | (y ? 2 : 0));
            ++o;
        };
        for (size_t i = 0, l; i < n;) {
            const size_t j = host_group(t, i, l);
            if (rows(l, j - i - l) > 0) {
                if (l == 0)
                    for (size_t y = i; y < j; ++y) row(t[i], nullptr, &t[y]);
                else if (l == j - i)
                    for (size_t x = i; x < j; ++x) row(t[i], &t[x], nullptr);
                else
                    for (size_t x = i; x < i + l; ++x)
                        for (size_t y = i + l; y < j; ++y) row(t[i], &t[x], &t[y]);
            }
            i = j;
        }
    } catch (const std::bad_alloc&) {
        set_last_error("window join: out of host memory");
        return GW_E_OOM;
    }
    return GW_OK;
}

}  // namespace

extern "C" {

int gw_window_join_host(int64_t n_l, const int64_t* lkey, const int64_t* lts, const int64_t* lpay, int64_t n_r,
                        const int64_t* rkey, const int64_t* rts, const int64_t* rpay, int64_t size, int64_t slide,
                        int64_t offset, int64_t w0, int64_t w1, int64_t* key_out, int64_t* start_out, int64_t* end_out,
                        int64_t* lpay_out, int64_t* rpay_out, int64_t cap, int64_t* n_out) {
    return join_host(n_l, lkey, lts, lpay, n_r, rkey, rts, rpay, size, slide, offset, w0, w1, GW_JOIN_MODE_INNER, 0,
                     INT64_MAX / 40, key_out, start_out, end_out, lpay_out, rpay_out, nullptr, cap, n_out);
}

int gw_window_join_outer_host(int64_t n_l, const int64_t* lkey, const int64_t* lts, const int64_t* lpay, int64_t n_r,
                              const int64_t* rkey, const int64_t* rts, const int64_t* rpay, int64_t size, int64_t slide,
                              int64_t offset, int64_t w0, int64_t w1, int32_t mode, int64_t null_payload,
                              int64_t* key_out, int64_t* start_out, int64_t* end_out, int64_t* lpay_out,
                              int64_t* rpay_out, uint8_t* present_out, int64_t cap, int64_t* n_out) {
    return join_host(n_l, lkey, lts, lpay, n_r, rkey, rts, rpay, size, slide, offset, w0, w1, mode, null_payload,
                     INT64_MAX / 41, key_out, start_out, end_out, lpay_out, rpay_out, present_out, cap, n_out);
}

int gw_window_cogroup_host(int64_t n_l, const int64_t* lkey, const int64_t* lts, const int64_t* lpay, int64_t n_r,
                           const int64_t* rkey, const int64_t* rts, const int64_t* rpay, int64_t size, int64_t slide,
                           int64_t offset, int64_t w0, int64_t w1, int64_t* key_out, int64_t* start_out,
                           int64_t* end_out, int64_t* loff_out, int64_t* roff_out, int64_t* lelem_out, int64_t cap_left,
                           int64_t* relem_out, int64_t cap_right, int64_t cap_groups, int64_t* n_out) {
    JoinGeom g;
    std::string why;
    int rc = join_args(n_l, n_r, size, slide, offset, std::min(cap_groups, std::min(cap_left, cap_right)), n_out, g, why);
    if (rc) { set_last_error(why); return rc; }
    n_out[0] = n_out[1] = n_out[2] = 0;
    if ((n_l > 0 && (!lkey || !lts || !lpay)) || (n_r > 0 && (!rkey || !rts || !rpay)) || !loff_out || !roff_out ||
        (cap_groups > 0 && (!key_out || !start_out || !end_out)) || (cap_left > 0 && !lelem_out) ||
        (cap_right > 0 && !relem_out)) {
        set_last_error("window coGroup: null column");
        return GW_E_INVALID;
    }
    try {
        std::vector<HostTup> t;
        if (w1 > w0 && (rc = host_tuples(g, n_l, lkey, lts, lpay, n_r, rkey, rts, rpay, w0, w1, t))) return rc;
        const size_t n = t.size();
        int64_t ng = 0, nl = 0;
        for (size_t i = 0, l; i < n; ++ng) {
            i = host_group(t, i, l);
            nl += (int64_t)l;
        }
        n_out[0] = ng;
        n_out[1] = nl;
        n_out[2] = (int64_t)n - nl;
        if (ng > cap_groups || n_out[1] > cap_left || n_out[2] > cap_right) {
            set_last_error("window coGroup: output arrays too small");
            return GW_E_OUTPUT_FULL;
        }
        int64_t gi = 0, lo = 0, ro = 0;
        loff_out[0] = roff_out[0] = 0;
        for (size_t i = 0, l; i < n; ++gi) {
            const size_t j = host_group(t, i, l);
            key_out[gi] = t[i].key;
            start_out[gi] = t[i].start;
            end_out[gi] = t[i].start + g.size;
            for (size_t x = i; x < i + l; ++x) lelem_out[lo++] = t[x].pay;
            for (size_t y = i + l; y < j; ++y) relem_out[ro++] = t[y].pay;
            loff_out[gi + 1] = lo;
            roff_out[gi + 1] = ro;
            i = j;
        }
    } catch (const std::bad_alloc&) {
        set_last_error("window join: out of host memory");
        return GW_E_OOM;
    }
    return GW_OK;
}

int gw_join_create(const gw_join_config* cfg, gw_join** out) {
    if (!cfg || !out) { set_last_error("gw_join_create: null argument"); return GW_E_INVALID; }
    *out = nullptr;
    if (cfg->assigner != GW_TUMBLING && cfg->assigner != GW_SLIDING) {
        set_last_error("window join: only tumbling and sliding event-time windows (no session or count windows)");
        return GW_E_UNSUPPORTED;
    }
    JoinGeom g;
    std::string why;
    int rc = join_geom(cfg->size, cfg->assigner == GW_TUMBLING ? cfg->size : cfg->slide, cfg->offset, g, why);
    if (rc) { set_last_error(why); return rc; }
    if (cfg->capacity_hint < 0 || cfg->max_batch < 0) { set_last_error("gw_join_create: negative capacity"); return GW_E_INVALID; }
    gw_join* h = new (std::nothrow) gw_join();
    if (!h) { set_last_error("gw_join_create: out of host memory"); return GW_E_OOM; }
    auto bail = [&](int code, const std::string& msg) {
        set_last_error(msg);
        gw_join_destroy(h);
        return code;
    };
    h->cfg = *cfg;
    h->g = g;
    h->max_batch = cfg->max_batch > 0 ? std::min<int64_t>(cfg->max_batch, (int64_t)1 << 30) : (int64_t)1 << 22;
    const char* what;
    const hipError_t e = h->os.create(cfg->device, &what);
    if (e != hipSuccess) return bail(GW_E_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
    const int64_t cap0 = std::max<int64_t>(cfg->capacity_hint, 16);
    for (int sd = 0; sd < 2; ++sd)
        if (h->log[sd].reserve_keep(cap0, 0, 0, h->os.stream) != hipSuccess) return bail(GW_E_OOM, "window join: out of device memory");
    *out = h;
    return GW_OK;
}

int gw_join_destroy(gw_join* h) {
    if (!h) return GW_OK;
    h->os.destroy();
    delete h;
    return GW_OK;
}

const char* gw_join_last_error(const gw_join* h) { return h ? h->er.err.c_str() : gw_last_error(nullptr); }

int gw_join_ingest_device(gw_join* h, int32_t side, int64_t n, const int64_t* d_key, const int64_t* d_ts,
                          const int64_t* d_payload, void* stream) {
    GW_OP_ENTER(h);
    if ((side != 0 && side != 1) || n < 0 || (n > 0 && (!d_key || !d_ts || !d_payload)))
        return h->er.fail(GW_E_INVALID, "gw_join_ingest_device: bad side or null column");
    h->touched = true;
    if (n + h->n_log[side] > INT32_MAX) return h->er.fail(GW_E_UNSUPPORTED, "window join: more than 2^31 - 1 live records on one side");
    OpStream::Handoff handoff(h->os, (hipStream_t)stream, n > 0);
    return h->ingest_cols(side, n, d_key, d_ts, d_payload);
}

int gw_join_ingest(gw_join* h, int32_t side, int64_t n, const int64_t* key, const int64_t* ts, const int64_t* payload) {
    GW_OP_ENTER(h);
    if ((side != 0 && side != 1) || n < 0 || (n > 0 && (!key || !ts || !payload)))
        return h->er.fail(GW_E_INVALID, "gw_join_ingest: bad side or null column");
    h->touched = true;
    if (n + h->n_log[side] > INT32_MAX) return h->er.fail(GW_E_UNSUPPORTED, "window join: more than 2^31 - 1 live records on one side");
    const int64_t* src[3] = {key, ts, payload};
    // (ingest_cols waits for the stream, so the host columns are free when this returns)
    return staged_ingest(h->stage, h->max_batch, n, src, h->os.stream, h->er,
                         [&](int64_t m, int64_t* const* d) { return h->ingest_cols(side, m, d[0], d[1], d[2]); });
}

int gw_join_advance_watermark(gw_join* h, int64_t watermark, int64_t* pairs_fired) {
    GW_OP_ENTER(h);
    return h->advance(watermark, pairs_fired);
}

int gw_join_end_input(gw_join* h, int64_t* pairs_fired) {
    GW_OP_ENTER(h);
    return h->advance(INT64_MAX, pairs_fired);
}

int gw_join_set_mode(gw_join* h, int32_t mode, int64_t null_payload) {
    GW_OP_ENTER(h);
    if (mode < GW_JOIN_MODE_INNER || mode > GW_JOIN_MODE_COGROUP) return h->er.fail(GW_E_INVALID, "gw_join_set_mode: unknown mode");
    if (h->touched) {  // (not a failure of the handle: it goes on in the mode it has)
        h->er.err = "gw_join_set_mode: only before the first ingest or watermark";
        return GW_E_STATE;
    }
    h->mode = mode;
    h->null_payload = null_payload;
    return GW_OK;
}

#define JOIN_PAIRS(h, what)                                                                          \
    if ((h)->mode == GW_JOIN_MODE_COGROUP) return (h)->er.fail(GW_E_INVALID, what ": the handle is in coGroup mode")
#define JOIN_COGROUP(h, what)                                                                        \
    if ((h)->mode != GW_JOIN_MODE_COGROUP) return (h)->er.fail(GW_E_INVALID, what ": the handle is not in coGroup mode")

int gw_join_pending(gw_join* h, int64_t* n) {
    GW_OP_ENTER(h);
    JOIN_PAIRS(h, "gw_join_pending");
    if (!n) return h->er.fail(GW_E_INVALID, "gw_join_pending: null argument");
    *n = h->rows.pending;
    return GW_OK;
}

int gw_join_drain_outer(gw_join* h, int64_t* key, int64_t* start, int64_t* end, int64_t* lpay, int64_t* rpay,
                        uint8_t* present, int64_t cap, int64_t* n) {
    GW_OP_ENTER(h);
    JOIN_PAIRS(h, "gw_join_drain");
    if (!n || cap < 0 || (cap > 0 && (!key || !start || !end || !lpay || !rpay)))
        return h->er.fail(GW_E_INVALID, "gw_join_drain: bad argument");
    int64_t* const dst[5] = {key, start, end, lpay, rpay};
    return h->rows.drain(dst, present, cap, n, h->os.stream, h->er);
}

int gw_join_drain(gw_join* h, int64_t* key, int64_t* start, int64_t* end, int64_t* lpay, int64_t* rpay, int64_t cap,
                  int64_t* n) {
    return gw_join_drain_outer(h, key, start, end, lpay, rpay, nullptr, cap, n);
}

int gw_join_rows_device_outer(gw_join* h, const int64_t** d_key, const int64_t** d_start, const int64_t** d_end,
                              const int64_t** d_lpay, const int64_t** d_rpay, const uint8_t** d_present, int64_t* n) {
    GW_OP_ENTER(h);
    JOIN_PAIRS(h, "gw_join_rows_device");
    if (!d_key || !d_start || !d_end || !d_lpay || !d_rpay || !n) return h->er.fail(GW_E_INVALID, "gw_join_rows_device: null argument");
    const int64_t** const dst[5] = {d_key, d_start, d_end, d_lpay, d_rpay};
    h->rows.view(dst, d_present, n);
    return GW_OK;
}

int gw_join_rows_device(gw_join* h, const int64_t** d_key, const int64_t** d_start, const int64_t** d_end,
                        const int64_t** d_lpay, const int64_t** d_rpay, int64_t* n) {
    return gw_join_rows_device_outer(h, d_key, d_start, d_end, d_lpay, d_rpay, nullptr, n);
}

int gw_join_cogroup_pending(gw_join* h, int64_t* n) {
    GW_OP_ENTER(h);
    JOIN_COGROUP(h, "gw_join_cogroup_pending");
    if (!n) return h->er.fail(GW_E_INVALID, "gw_join_cogroup_pending: null argument");
    for (int c = 0; c < 3; ++c) n[c] = h->cg_n[c];
    return GW_OK;
}

int gw_join_cogroup_drain(gw_join* h, int64_t* key, int64_t* start, int64_t* end, int64_t* loff, int64_t* roff,
                          int64_t* lelem, int64_t cap_left, int64_t* relem, int64_t cap_right, int64_t cap_groups,
                          int64_t* n) {
    GW_OP_ENTER(h);
    JOIN_COGROUP(h, "gw_join_cogroup_drain");
    const int64_t* m = h->cg_n;
    if (!n || cap_groups < 0 || cap_left < 0 || cap_right < 0 || !loff || !roff ||
        (cap_groups > 0 && (!key || !start || !end)) || (cap_left > 0 && !lelem) || (cap_right > 0 && !relem))
        return h->er.fail(GW_E_INVALID, "gw_join_cogroup_drain: bad argument");
    for (int c = 0; c < 3; ++c) n[c] = m[c];
    if (m[0] > cap_groups || m[1] > cap_left || m[2] > cap_right)
        return h->er.fail(GW_E_OUTPUT_FULL, "gw_join_cogroup_drain: output arrays too small");
    loff[0] = roff[0] = 0;
    if (m[0] == 0) return GW_OK;
    int64_t* dst[5] = {key, start, end, loff, roff};
    hipError_t e = hipSuccess;
    for (int c = 0; c < 5 && e == hipSuccess; ++c)
        e = hipMemcpyAsync(dst[c], h->cg[c], (size_t)(m[0] + (c >= 3)) * 8, hipMemcpyDeviceToHost, h->os.stream);
    if (m[1] > 0 && e == hipSuccess) e = hipMemcpyAsync(lelem, h->cg_elem[0][0], (size_t)m[1] * 8, hipMemcpyDeviceToHost, h->os.stream);
    if (m[2] > 0 && e == hipSuccess) e = hipMemcpyAsync(relem, h->cg_elem[1][0], (size_t)m[2] * 8, hipMemcpyDeviceToHost, h->os.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->os.stream);
    if (e != hipSuccess) return h->er.dev_fail(e);
    h->cg_n[0] = h->cg_n[1] = h->cg_n[2] = 0;
    return GW_OK;
}

int gw_join_cogroup_rows_device(gw_join* h, const int64_t** d_key, const int64_t** d_start, const int64_t** d_end,
                                const int64_t** d_loff, const int64_t** d_roff, const int64_t** d_lelem,
                                const int64_t** d_relem, int64_t* n) {
    GW_OP_ENTER(h);
    JOIN_COGROUP(h, "gw_join_cogroup_rows_device");
    if (!d_key || !d_start || !d_end || !d_loff || !d_roff || !d_lelem || !d_relem || !n)
        return h->er.fail(GW_E_INVALID, "gw_join_cogroup_rows_device: null argument");
    const int64_t** dst[5] = {d_key, d_start, d_end, d_loff, d_roff};
    for (int c = 0; c < 5; ++c) *dst[c] = h->cg_n[0] ? h->cg[c] : nullptr;
    *d_lelem = h->cg_n[1] ? h->cg_elem[0][0] : nullptr;
    *d_relem = h->cg_n[2] ? h->cg_elem[1][0] : nullptr;
    for (int c = 0; c < 3; ++c) n[c] = h->cg_n[c];
    return GW_OK;
}

int gw_join_clear_rows(gw_join* h) {
    GW_OP_ENTER(h);
    h->rows.clear();
    h->cg_n[0] = h->cg_n[1] = h->cg_n[2] = 0;
    return GW_OK;
}

int64_t gw_join_late_dropped(const gw_join* h) { return h ? h->late : 0; }

int gw_join_get_stats(const gw_join* h, gw_join_stats* out) {
    if (!h || !out) return GW_E_INVALID;
    *out = h->st;
    out->live_left = h->n_log[0];
    out->live_right = h->n_log[1];
    out->log_capacity_left = h->log[0].cap;
    out->log_capacity_right = h->log[1].cap;
    return GW_OK;
}

void* gw_join_stream(gw_join* h) { return h ? (void*)h->os.stream : nullptr; }

}  // extern "C"
