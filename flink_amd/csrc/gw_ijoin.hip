// gw_ijoin.hip — event-time interval join of two keyed streams (include/gpuwin.h
// gw_interval_join_*, gw_ijoin_*): keyedA.intervalJoin(keyedB).between(lower, upper).process(...),
// Flink's IntervalJoinOperator (RS/api/operators/co/IntervalJoinOperator.java).
//
// Flink keeps a MapState ts -> list per key and side; processElement scans the other side's map
// for the timestamps inside the bounds and registers a cleanup timer.  Here each side's buffer is
// a device log of three columns kept sorted by (key, ts) as signed values -- the order of the
// sign-flipped words the sort uses -- with equal (key, ts) in arrival order, so the partners of a
// record are one contiguous range of the other side's log, already in the output's order.  One
// ingest pass of a batch is seven stages:
//
//   filter   the late test, the Long.MIN_VALUE and the range check in one kernel, which also
//            reduces the extremes of the kept records' key and ts words (so the sort sees only
//            the bits that vary); a stable compaction through the scan;
//   sort     two stable passes of gw::sort_pairs_u64 carrying the arrival index: by ts word, then
//            by key word;
//   probe    per sorted batch record two binary searches in the other side's log: the lower
//            bound of (key, ts + rel_lower) and the upper bound of (key, ts + rel_upper); `first`
//            and `count` go to the record's arrival slot;
//   scan     the counts in arrival order: every record's first output row, and the total;
//   compact  the probes that found something become descriptors (row offset, first partner, the
//            probe's key, ts and payload): a tile of the expansion then touches at most as many
//            descriptors as it has rows, however many probes found nothing in between;
//   expand   the hot kernel: a workgroup owns kIjTile consecutive output rows, finds its
//            descriptors with one search per end of the tile, stages them in LDS, and every lane
//            writes two consecutive rows of each of the five columns with one 16-byte store.  The
//            probe's fields come from LDS, the partner's ts and payload from consecutive log
//            rows.  Split by rows, never by probes: one probe with a million partners and a
//            million probes with one partner each are the same work per workgroup;
//   merge    the sorted batch into its own side's log by mutual ranking: a log record moves up by
//            its lower bound in the batch, a batch record lands at its index plus its upper bound
//            in the log (old before new on equal (key, ts)); one scatter pass into the log's
//            other buffer.
//
// A watermark evicts by a stable compaction per side, which keeps the order.  No atomics in the
// probe, expand and merge kernels; the filter ends in a few per block.  The host reads the device
// twice per pass: the kept count with the extremes (it sizes the sort) and the row count with the
// descriptor count (it sizes the output).
#include <algorithm>
#include <cstring>
#include <mutex>
#include <new>
#include <numeric>
#include <string>
#include <vector>

#include "gw_joinop.h"    // the host side of the operator: OpError, OpStream, RowBuf, staged_ingest (and gw_devmem.h)
#include "gw_joinutil.h"  // scan_excl, the wave reductions and search, k_compact3, Scratch, Carve
#include "gw_kernels.h"
#include "gw_sort.h"

namespace gw {

constexpr const char* kIjName = "interval join";  // the prefix of the shared helpers' messages
struct IjBounds {
    int64_t lower, upper;  // inclusive, relative to the left record
};
// header words (int64) shared by the stages of one pass
enum { IH_FLAGS = 0, IH_LATE, IH_KEPT, IH_MINK, IH_MAXK, IH_MINT, IH_MAXT, IH_P, IH_NC, kIjHdr = 16 };
constexpr int64_t kIjMaxRows = INT64_MAX / 40;

// IntervalJoinOperator.processElement computes ts + lowerBound and ts + upperBound of the other
// side (for a right record the bounds are -upper and -lower); leaving int64 is GW_DF_RANGE.
GW_HD bool ij_fits(int side, int64_t ts, IjBounds b) {
    int64_t x;
    if (side == GW_JOIN_LEFT) return !__builtin_add_overflow(ts, b.lower, &x) && !__builtin_add_overflow(ts, b.upper, &x);
    return !__builtin_sub_overflow(ts, b.upper, &x) && !__builtin_sub_overflow(ts, b.lower, &x);
}
// The record's cleanup timer (processElement1 / 2: registerCleanupTimer); fits by ij_fits.
GW_HD int64_t ij_cleanup(int side, int64_t ts, IjBounds b) {
    if (side == GW_JOIN_LEFT) return b.upper > 0 ? ts + b.upper : ts;
    return b.lower < 0 ? ts - b.lower : ts;
}
// Probe (key, ts) of `side` meets the other side's ts in [ts + rel.lower, ts + rel.upper].
GW_HD IjBounds ij_relative(int side, IjBounds b) { return side == GW_JOIN_LEFT ? b : IjBounds{-b.upper, -b.lower}; }

// First index of the (key, ts)-sorted columns whose record is not below (UPPER: is above) (k, t).
template <bool UPPER>
GW_HD int64_t ij_bound(const int64_t* __restrict__ key, const int64_t* __restrict__ ts, int64_t lo, int64_t hi, int64_t k,
                       int64_t t) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const int64_t mk = key[mid];
        const bool before = mk < k || (mk == k && (UPPER ? ts[mid] <= t : ts[mid] < t));
        if (before) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ---- filter ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(kJoinThreads) k_ij_hdr_init(int64_t* hdr) {
    if (threadIdx.x >= kIjHdr) return;
    hdr[threadIdx.x] = threadIdx.x == IH_MINK || threadIdx.x == IH_MINT ? -1 : 0;  // minima: all ones
}

// keep[i] = 1 for the records that stay (keep may be null: the checks alone).  Flags: any
// Long.MIN_VALUE timestamp, and a bound that leaves int64 on a record that is not late.
__global__ void __launch_bounds__(kJoinThreads) k_ij_filter(int64_t n, const int64_t* __restrict__ key,
                                                            const int64_t* __restrict__ ts, int side, IjBounds b, int64_t wm,
                                                            uint32_t* keep, int64_t* hdr) {
    using ull = unsigned long long;
    __shared__ uint64_t s_late[4], s_flags[4], s_kmin[4], s_kmax[4], s_tmin[4], s_tmax[4];
    uint64_t late = 0, flags = 0, mink = ~0ull, maxk = 0, mint = ~0ull, maxt = 0;
    for (int64_t i = (int64_t)blockIdx.x * kJoinThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kJoinThreads) {
        const int64_t t = ts[i];
        uint64_t f = t == INT64_MIN ? GW_DF_NO_TS : 0;
        const bool is_late = !f && wm != INT64_MIN && t < wm;
        if (!f && !is_late && !ij_fits(side, t, b)) f = GW_DF_RANGE;
        const bool k = !f && !is_late;
        flags |= f;
        late += is_late;
        if (k) {
            const uint64_t kw = join_key_word(key[i]), tw = join_key_word(t);
            mink = kw < mink ? kw : mink;
            maxk = kw > maxk ? kw : maxk;
            mint = tw < mint ? tw : mint;
            maxt = tw > maxt ? tw : maxt;
        }
        if (keep) keep[i] = k;
    }
    late = wave_sum(late);
    flags = wave_ior(flags);
    mink = wave_min_u64(mink);
    maxk = wave_max_u64(maxk);
    mint = wave_min_u64(mint);
    maxt = wave_max_u64(maxt);
    const int wave = threadIdx.x >> 6;
    if (__lane_id() == 0) {
        s_late[wave] = late; s_flags[wave] = flags; s_kmin[wave] = mink; s_kmax[wave] = maxk; s_tmin[wave] = mint;
        s_tmax[wave] = maxt;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < 4; ++w) {
        late += s_late[w];
        flags |= s_flags[w];
        mink = s_kmin[w] < mink ? s_kmin[w] : mink;
        maxk = s_kmax[w] > maxk ? s_kmax[w] : maxk;
        mint = s_tmin[w] < mint ? s_tmin[w] : mint;
        maxt = s_tmax[w] > maxt ? s_tmax[w] : maxt;
    }
    if (late) atomicAdd((ull*)&hdr[IH_LATE], (ull)late);
    if (flags) atomicOr((ull*)&hdr[IH_FLAGS], (ull)flags);
    if (mink <= maxk) {  // the block kept a record
        atomicMin((ull*)&hdr[IH_MINK], (ull)mink);
        atomicMax((ull*)&hdr[IH_MAXK], (ull)maxk);
        atomicMin((ull*)&hdr[IH_MINT], (ull)mint);
        atomicMax((ull*)&hdr[IH_MAXT], (ull)maxt);
    }
}
// The eviction's test: the records whose cleanup timer has not fired at watermark w.
__global__ void __launch_bounds__(kJoinThreads) k_ij_evict_flags(int64_t n, const int64_t* __restrict__ ts, int side,
                                                                 IjBounds b, int64_t w, uint32_t* keep) {
    for (int64_t i = (int64_t)blockIdx.x * kJoinThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kJoinThreads)
        keep[i] = ij_cleanup(side, ts[i], b) > w;
}

// ---- sort -----------------------------------------------------------------------------------
__global__ void __launch_bounds__(kJoinThreads) k_ij_ts_words(int64_t n, const int64_t* __restrict__ ts, uint64_t min_tw,
                                                              uint64_t* w) {
    for (int64_t i = (int64_t)blockIdx.x * kJoinThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kJoinThreads)
        w[i] = join_key_word(ts[i]) - min_tw;
}
__global__ void __launch_bounds__(kJoinThreads) k_ij_key_words(int64_t n, const uint32_t* __restrict__ perm,
                                                               const int64_t* __restrict__ key, uint64_t min_kw, uint64_t* w) {
    for (int64_t i = (int64_t)blockIdx.x * kJoinThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kJoinThreads)
        w[i] = join_key_word(key[perm[i]]) - min_kw;
}
__global__ void __launch_bounds__(kJoinThreads) k_ij_gather3(int64_t n, const uint32_t* __restrict__ perm, Cols3 c) {
    for (int64_t i = (int64_t)blockIdx.x * kJoinThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kJoinThreads) {
        const uint32_t j = perm[i];
        c.out[0][i] = c.in[0][j];
        c.out[1][i] = c.in[1][j];
        c.out[2][i] = c.in[2][j];
    }
}

// ---- probe ----------------------------------------------------------------------------------
struct IjLog {  // a side's records sorted by (key, ts), equal ones in arrival order
    const int64_t *key, *ts, *pay;
    int64_t n;
};
// Sorted batch record i (arrival slot perm[i]): its partners are log rows [first, first + cnt).
__global__ void __launch_bounds__(kJoinThreads) k_ij_probe(int64_t n, const int64_t* __restrict__ skey,
                                                           const int64_t* __restrict__ sts,
                                                           const uint32_t* __restrict__ perm, IjBounds rel, IjLog o,
                                                           uint32_t* first, uint32_t* cnt, uint32_t* ne) {
    for (int64_t i = (int64_t)blockIdx.x * kJoinThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kJoinThreads) {
        const int64_t k = skey[i], t = sts[i];
        const int64_t a = ij_bound<false>(o.key, o.ts, 0, o.n, k, t + rel.lower);
        const int64_t e = ij_bound<true>(o.key, o.ts, a, o.n, k, t + rel.upper);
        const uint32_t slot = perm[i];
        first[slot] = (uint32_t)a;
        cnt[slot] = (uint32_t)(e - a);
        ne[slot] = e > a;
    }
}
// Descriptors of the probes with partners, in arrival order; doff[nc] = the total.
__global__ void __launch_bounds__(kJoinThreads) k_ij_desc(int64_t n, const int64_t* __restrict__ hdr,
                                                          const uint32_t* __restrict__ cnt,
                                                          const int64_t* __restrict__ roff,
                                                          const uint32_t* __restrict__ cidx,
                                                          const uint32_t* __restrict__ first,
                                                          const int64_t* __restrict__ key, const int64_t* __restrict__ ts,
                                                          const int64_t* __restrict__ pay, int64_t* doff, uint32_t* dfirst,
                                                          int64_t* dkey, int64_t* dts, int64_t* dpay) {
    for (int64_t i = (int64_t)blockIdx.x * kJoinThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kJoinThreads) {
        if (i == 0) doff[hdr[IH_NC]] = hdr[IH_P];
        if (cnt[i] == 0) continue;
        const uint32_t c = cidx[i];
        doff[c] = roff[i];
        dfirst[c] = first[i];
        dkey[c] = key[i];
        dts[c] = ts[i];
        dpay[c] = pay[i];
    }
}

// ---- expand ---------------------------------------------------------------------------------
constexpr int kIjTile = 1024;  // output slots per workgroup: 2 steps of 256 lanes x 2 rows
struct IjOut {
    int64_t* col[5];  // key, left ts, right ts, left payload, right payload
};
struct IjRow {
    int64_t key, pts, ppay, ots, opay;  // the probe's fields and the partner's
};

// Output slot q holds row q - shift: with shift = 1 the columns start 8 bytes past a 16-byte
// boundary and row 0 is written alone, so every two-row store is aligned.  Row p belongs to the
// descriptor c with doff[c] <= p < doff[c + 1] and pairs the probe with log row
// dfirst[c] + (p - doff[c]).  PROBE_LEFT: the probe's fields are the left columns.
template <bool VEC, bool PROBE_LEFT>
__global__ void __launch_bounds__(kJoinThreads) k_ij_expand(int64_t P, int shift, int64_t nc,
                                                            const int64_t* __restrict__ doff,
                                                            const uint32_t* __restrict__ dfirst,
                                                            const int64_t* __restrict__ dkey,
                                                            const int64_t* __restrict__ dts,
                                                            const int64_t* __restrict__ dpay,
                                                            const int64_t* __restrict__ ots,
                                                            const int64_t* __restrict__ opay, IjOut o) {
    __shared__ int64_t s_off[kIjTile + 1], s_key[kIjTile], s_ts[kIjTile], s_pay[kIjTile];
    __shared__ uint32_t s_first[kIjTile];
    __shared__ int64_t s_c[2];
    const int64_t slot0 = (int64_t)blockIdx.x * kIjTile;
    const int64_t p_first = std::max<int64_t>(slot0 - shift, 0);
    const int64_t p_last = std::min<int64_t>(slot0 + kIjTile - 1 - shift, P - 1);
    const int wave = threadIdx.x >> 6;
    if (wave < 2) {
        const int64_t c = wave_search(doff, nc, wave == 0 ? p_first : p_last);
        if (__lane_id() == 0) s_c[wave] = c;
    }
    __syncthreads();
    const int64_t c0 = s_c[0];
    const int ngt = (int)(s_c[1] - c0) + 1;  // <= kIjTile: every descriptor has a row in the tile
    for (int i = threadIdx.x; i <= ngt; i += kJoinThreads) {
        s_off[i] = doff[c0 + i];
        if (i < ngt) {
            s_first[i] = dfirst[c0 + i];
            s_key[i] = dkey[c0 + i];
            s_ts[i] = dts[c0 + i];
            s_pay[i] = dpay[c0 + i];
        }
    }
    __syncthreads();
#pragma unroll
    for (int step = 0; step < kIjTile / (2 * kJoinThreads); ++step) {
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
        int64_t j = (int64_t)s_first[lo] + (p - s_off[lo]);
        IjRow x{s_key[lo], s_ts[lo], s_pay[lo], ots[j], opay[j]}, y = x;
        if (va && vb) {
            if (pb >= s_off[lo + 1]) {  // the next descriptor: its row 0
                ++lo;
                y.key = s_key[lo];
                y.pts = s_ts[lo];
                y.ppay = s_pay[lo];
                j = s_first[lo];
            } else {
                ++j;
            }
            y.ots = ots[j];
            y.opay = opay[j];
        }
        const int64_t xl = PROBE_LEFT ? x.pts : x.ots, xr = PROBE_LEFT ? x.ots : x.pts;
        const int64_t yl = PROBE_LEFT ? y.pts : y.ots, yr = PROBE_LEFT ? y.ots : y.pts;
        const int64_t xlp = PROBE_LEFT ? x.ppay : x.opay, xrp = PROBE_LEFT ? x.opay : x.ppay;
        const int64_t ylp = PROBE_LEFT ? y.ppay : y.opay, yrp = PROBE_LEFT ? y.opay : y.ppay;
        if (VEC && va && vb) {
            *reinterpret_cast<I64x2*>(o.col[0] + pa) = I64x2{x.key, y.key};
            *reinterpret_cast<I64x2*>(o.col[1] + pa) = I64x2{xl, yl};
            *reinterpret_cast<I64x2*>(o.col[2] + pa) = I64x2{xr, yr};
            *reinterpret_cast<I64x2*>(o.col[3] + pa) = I64x2{xlp, ylp};
            *reinterpret_cast<I64x2*>(o.col[4] + pa) = I64x2{xrp, yrp};
        } else {
            if (va) {
                o.col[0][pa] = x.key; o.col[1][pa] = xl; o.col[2][pa] = xr; o.col[3][pa] = xlp; o.col[4][pa] = xrp;
            }
            if (vb) {
                o.col[0][pb] = y.key; o.col[1][pb] = yl; o.col[2][pb] = yr; o.col[3][pb] = ylp; o.col[4][pb] = yrp;
            }
        }
    }
}

// ---- merge ----------------------------------------------------------------------------------
// Items [0, m) are the log's records, [m, m + n) the sorted batch's: each goes to its own index
// plus its rank in the other sequence, the log's by lower bound and the batch's by upper bound,
// so on equal (key, ts) the old records come first.  The ranks are monotone along each sequence,
// so neighbouring lanes search the same few cache lines and write neighbouring rows.
__global__ void __launch_bounds__(kJoinThreads) k_ij_merge(IjLog batch, IjLog log, int64_t* okey, int64_t* ots,
                                                           int64_t* opay) {
    const int64_t m = log.n, total = log.n + batch.n;
    for (int64_t x = (int64_t)blockIdx.x * kJoinThreads + threadIdx.x; x < total; x += (int64_t)gridDim.x * kJoinThreads) {
        int64_t k, t, pay, pos;
        if (x < m) {
            k = log.key[x]; t = log.ts[x]; pay = log.pay[x];
            pos = x + ij_bound<false>(batch.key, batch.ts, 0, batch.n, k, t);
        } else {
            const int64_t i = x - m;
            k = batch.key[i]; t = batch.ts[i]; pay = batch.pay[i];
            pos = i + ij_bound<true>(log.key, log.ts, 0, m, k, t);
        }
        okey[pos] = k;
        ots[pos] = t;
        opay[pos] = pay;
    }
}

// ---- host side of the stages ------------------------------------------------------------------
struct IjFilterArrays {  // by records: the filter and its compaction
    int64_t* hdr;
    uint32_t *keep, *koff;
    int64_t* blk;
    void carve(Carve& c, int64_t n) {
        hdr = c.take<int64_t>(kIjHdr);
        keep = c.take<uint32_t>(n);
        koff = c.take<uint32_t>(n);
        blk = c.take<int64_t>(scan_blocks(n) + 1);
    }
};
struct IjArrays : IjFilterArrays {  // one batch through the pass
    int64_t *c[3], *s[3];  // the kept records in arrival order, and sorted
    uint64_t *w0, *w1;
    uint32_t *v0, *v1, *perm;
    void* sort;
    uint32_t *first, *cnt, *ne, *cidx, *dfirst;  // probe == true only
    int64_t *roff, *doff, *dkey, *dts, *dpay;
    void carve(Carve& cv, int64_t n, bool probe) {
        IjFilterArrays::carve(cv, n);
        for (auto& x : c) x = cv.take<int64_t>(n);
        for (auto& x : s) x = cv.take<int64_t>(n);
        w0 = cv.take<uint64_t>(n); w1 = cv.take<uint64_t>(n);
        v0 = cv.take<uint32_t>(n); v1 = cv.take<uint32_t>(n);
        sort = cv.take<char>(sort_scratch_bytes(n));
        perm = nullptr;
        if (!probe) return;
        first = cv.take<uint32_t>(n); cnt = cv.take<uint32_t>(n); ne = cv.take<uint32_t>(n); cidx = cv.take<uint32_t>(n);
        dfirst = cv.take<uint32_t>(n);
        roff = cv.take<int64_t>(n); doff = cv.take<int64_t>(n + 1); dkey = cv.take<int64_t>(n); dts = cv.take<int64_t>(n);
        dpay = cv.take<int64_t>(n);
    }
    IjLog sorted(int64_t n) const { return IjLog{s[0], s[1], s[2], n}; }
};

// Filter: the checks, keep flags, their scan (the kept count to hdr[IH_KEPT]) and the compaction
// of (key, ts, pay)[0..n) into dst; the caller reads hdr behind it.
static hipError_t ij_launch_filter(int64_t n, const int64_t* key, const int64_t* ts, const int64_t* pay, int side, IjBounds b,
                                   int64_t wm, IjFilterArrays& A, int64_t* const* dst, hipStream_t s) {
    hipLaunchKernelGGL(k_ij_hdr_init, dim3(1), dim3(kJoinThreads), 0, s, A.hdr);
    hipLaunchKernelGGL(k_ij_filter, dim3(grid_for(n)), dim3(kJoinThreads), 0, s, n, key, ts, side, b, wm, A.keep, A.hdr);
    hipError_t e = scan_excl<uint32_t, uint32_t>(A.keep, A.koff, n, A.blk, A.hdr + IH_KEPT, s);
    if (e != hipSuccess) return e;
    Cols3 c{{key, ts, pay}, {dst[0], dst[1], dst[2]}};
    hipLaunchKernelGGL(k_compact3, dim3(grid_for(n)), dim3(kJoinThreads), 0, s, n, A.keep, A.koff, c);
    return hipGetLastError();
}
static int ij_flag_error(uint64_t flags, std::string& why) {
    if (flags & GW_DF_NO_TS) {
        why = "Record has Long.MIN_VALUE timestamp (= no timestamp marker)";
        return GW_E_NO_TIMESTAMP;
    }
    if (flags & GW_DF_RANGE) { why = "interval join: a record's timestamp plus a bound overflows int64"; return GW_E_RANGE; }
    return GW_OK;
}
// The n kept records A.c sorted by (key, ts), stable, into A.s, with A.perm[i] the arrival slot
// of sorted record i; h: the filter's header on the host (the extremes).
static hipError_t ij_sort(IjArrays& A, int64_t n, const int64_t* h, hipStream_t s) {
    const uint64_t min_kw = (uint64_t)h[IH_MINK], min_tw = (uint64_t)h[IH_MINT];
    const int kbits = bit_length((uint64_t)h[IH_MAXK] - min_kw), tbits = bit_length((uint64_t)h[IH_MAXT] - min_tw);
    const int g = grid_for(n);
    hipError_t e;
    int alt = 0;
    hipLaunchKernelGGL(k_ij_ts_words, dim3(g), dim3(kJoinThreads), 0, s, n, A.c[1], min_tw, A.w0);
    if ((e = sort_pairs_u64(A.w0, A.v0, A.w1, A.v1, n, 0, tbits, A.sort, s, &alt, true)) != hipSuccess) return e;
    uint32_t* perm = alt ? A.v1 : A.v0;
    if (kbits > 0) {
        uint32_t* other = alt ? A.v0 : A.v1;
        hipLaunchKernelGGL(k_ij_key_words, dim3(g), dim3(kJoinThreads), 0, s, n, perm, A.c[0], min_kw, A.w0);
        if ((e = sort_pairs_u64(A.w0, perm, A.w1, other, n, 0, kbits, A.sort, s, &alt, false)) != hipSuccess) return e;
        if (alt) perm = other;
    }
    A.perm = perm;
    Cols3 c{{A.c[0], A.c[1], A.c[2]}, {A.s[0], A.s[1], A.s[2]}};
    hipLaunchKernelGGL(k_ij_gather3, dim3(g), dim3(kJoinThreads), 0, s, n, perm, c);
    return hipGetLastError();
}
// Probe, the two scans and the descriptors of the n sorted records of `side` against `other`;
// the totals go to hdr[IH_P] and hdr[IH_NC].
static hipError_t ij_launch_probe(IjArrays& A, int64_t n, int side, IjBounds b, const IjLog& other, hipStream_t s) {
    const int g = grid_for(n);
    hipLaunchKernelGGL(k_ij_probe, dim3(g), dim3(kJoinThreads), 0, s, n, A.s[0], A.s[1], A.perm, ij_relative(side, b), other,
                       A.first, A.cnt, A.ne);
    hipError_t e;
    if ((e = scan_excl<uint32_t, int64_t>(A.cnt, A.roff, n, A.blk, A.hdr + IH_P, s)) != hipSuccess) return e;
    if ((e = scan_excl<uint32_t, uint32_t>(A.ne, A.cidx, n, A.blk, A.hdr + IH_NC, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_ij_desc, dim3(g), dim3(kJoinThreads), 0, s, n, A.hdr, A.cnt, A.roff, A.cidx, A.first, A.c[0], A.c[1],
                       A.c[2], A.doff, A.dfirst, A.dkey, A.dts, A.dpay);
    return hipGetLastError();
}
static hipError_t ij_launch_expand(const IjArrays& A, int64_t P, int64_t nc, int side, const IjLog& other, const IjOut& out,
                                   hipStream_t s) {
    const auto [vec, shift] = expand_alignment(out.col);
    const unsigned nblk = (unsigned)((P + shift + kIjTile - 1) / kIjTile);
    const bool left = side == GW_JOIN_LEFT;
#define IJ_EXPAND(V, L)                                                                                             \
    hipLaunchKernelGGL((k_ij_expand<V, L>), dim3(nblk), dim3(kJoinThreads), 0, s, P, shift, nc, A.doff, A.dfirst, A.dkey, \
                       A.dts, A.dpay, other.ts, other.pay, out)
    if (vec && left) IJ_EXPAND(true, true);
    else if (vec) IJ_EXPAND(true, false);
    else if (left) IJ_EXPAND(false, true);
    else IJ_EXPAND(false, false);
#undef IJ_EXPAND
    return hipGetLastError();
}

// One stateless call at a time per process: every call waits for its launches before it returns,
// so the per-device scratch is free for the next.
static std::mutex g_ij_mu;
static Scratch g_ij_scr[64];

}  // namespace gw

using namespace gw;

namespace {

int ij_args(int32_t probe_side, int64_t n_p, int64_t n_b, int64_t lower, int64_t upper, int64_t cap, const int64_t* n_out,
            std::string& why) {
    if (!n_out || (probe_side != GW_JOIN_LEFT && probe_side != GW_JOIN_RIGHT) || n_p < 0 || n_b < 0 || cap < 0) {
        why = "interval join: bad argument";
        return GW_E_INVALID;
    }
    if (lower > upper || lower < -GW_IJOIN_MAX_BOUND || upper > GW_IJOIN_MAX_BOUND) {
        why = "interval join: the bounds must satisfy -2^62 <= lower <= upper <= 2^62";
        return GW_E_INVALID;
    }
    if (n_p > kSortMaxRecords || n_b > kSortMaxRecords) {
        why = "interval join: more than 2^30 - 1 records on one side";
        return GW_E_UNSUPPORTED;
    }
    return GW_OK;
}

int ij_device(int32_t probe_side, int64_t n_p, const int64_t* d_pkey, const int64_t* d_pts, const int64_t* d_ppay, int64_t n_b,
              const int64_t* d_bkey, const int64_t* d_bts, const int64_t* d_bpay, int64_t lower, int64_t upper,
              int64_t* const* d_out, int64_t cap, int64_t* n_out, hipStream_t s, double* expand_ms, std::string& why) {
    int rc = ij_args(probe_side, n_p, n_b, lower, upper, cap, n_out, why);
    if (rc) return rc;
    *n_out = 0;
    if (expand_ms) *expand_ms = 0;
    if (n_p == 0 || n_b == 0) return GW_OK;
    if (!d_pkey || !d_pts || !d_ppay || !d_bkey || !d_bts || !d_bpay ||
        (cap > 0 && (!d_out[0] || !d_out[1] || !d_out[2] || !d_out[3] || !d_out[4]))) {
        why = "interval join: null column";
        return GW_E_INVALID;
    }
    const IjBounds b{lower, upper};
    std::lock_guard<std::mutex> lock(g_ij_mu);
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { why = "interval join: no device"; return GW_E_DEVICE; }
    IjArrays B, A;  // the build side and the probe side
    auto carve = [&](Carve& c) {
        B.carve(c, n_b, false);
        A.carve(c, n_p, true);
    };
    if ((rc = carve_from(carve, g_ij_scr[dev], kIjName, why))) return rc;
    // no late test (the watermark is Long.MIN_VALUE): the filter is the two checks
    int64_t hb[kIjHdr], hp[kIjHdr];
    hipError_t e = ij_launch_filter(n_b, d_bkey, d_bts, d_bpay, 1 - probe_side, b, INT64_MIN, B, B.c, s);
    if (e == hipSuccess) e = ij_launch_filter(n_p, d_pkey, d_pts, d_ppay, probe_side, b, INT64_MIN, A, A.c, s);
    if (e == hipSuccess) e = hipMemcpyAsync(hb, B.hdr, sizeof hb, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = read_hdr(hp, A.hdr, kIjHdr, s);
    if (e != hipSuccess) return dev_fail(kIjName, e, why);
    if ((rc = ij_flag_error((uint64_t)(hb[IH_FLAGS] | hp[IH_FLAGS]), why))) return rc;
    if ((e = ij_sort(B, n_b, hb, s)) != hipSuccess || (e = ij_sort(A, n_p, hp, s)) != hipSuccess) return dev_fail(kIjName, e, why);
    const IjLog build = B.sorted(n_b);
    e = ij_launch_probe(A, n_p, probe_side, b, build, s);
    if (e == hipSuccess) e = read_hdr(hp, A.hdr, kIjHdr, s);
    if (e != hipSuccess) return dev_fail(kIjName, e, why);
    const int64_t P = hp[IH_P], nc = hp[IH_NC];
    if (P > kIjMaxRows) { why = "interval join: the rows of one call exceed int64 bytes"; return GW_E_RANGE; }
    *n_out = P;
    if (P > cap) { why = "interval join: output arrays too small"; return GW_E_OUTPUT_FULL; }
    if (P == 0) return GW_OK;
    TimedPair t;
    if (expand_ms && t.create() != hipSuccess) { why = "interval join: hipEventCreate"; return GW_E_DEVICE; }
    const IjOut out{{d_out[0], d_out[1], d_out[2], d_out[3], d_out[4]}};
    t.begin(s);
    e = ij_launch_expand(A, P, nc, probe_side, build, out, s);
    t.end(s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);  // the scratch is free for the next call
    if (e != hipSuccess) return dev_fail(kIjName, e, why);
    float ms = 0;
    if (expand_ms && t.elapsed(&ms) == hipSuccess) *expand_ms = ms;
    return GW_OK;
}

}  // namespace

// ---- the operator ---------------------------------------------------------------------------
struct gw_ijoin {
    gw_ijoin_config cfg{};
    IjBounds b{};
    OpError er{kIjName};
    OpStream os;
    TimedPair probe_t, merge_t;  // the last pass: around its probe stage and around its merge
    bool timed = false;
    DevCols<3> log[2], alt[2], stage;  // alt: the buffer the next merge or eviction writes
    int64_t n_log[2] = {0, 0};
    RowBuf rows{false};  // the pending rows
    // the passes' scratch; the stream is idle before a block it may still use is freed
    DevBuf<char> scr;
    int64_t wm = INT64_MIN, late = 0, max_batch = 0;
    gw_ijoin_stats st{};

    // alt[side] with room for `need` rows; grow: a log that outgrows its capacity doubles
    int reserve_alt(int side, int64_t need, bool grow) {
        if (need <= alt[side].cap) return GW_OK;
        const int64_t cap = grow ? std::max<int64_t>(need, 2 * std::max(log[side].cap, alt[side].cap)) : std::max(need, log[side].cap);
        if (alt[side].reserve_keep(cap, 0, 0, os.stream) != hipSuccess) {
            (void)hipGetLastError();
            return er.fail(GW_E_OOM, "interval join: out of device memory for the %s log", side ? "right" : "left");
        }
        if (grow) ++st.log_growths;
        return GW_OK;
    }
    IjLog side_log(int side) const { return IjLog{log[side][0], log[side][1], log[side][2], n_log[side]}; }

    // The checks over a whole call that runs in several passes, so that an error leaves nothing
    // of the call behind (device columns, ordered behind their producer).
    int check_call(int side, int64_t n, const int64_t* key, const int64_t* ts) {
        IjFilterArrays F;
        int rc = carve_from([&](Carve& c) { F.carve(c, 1); }, scr, er, os.stream);
        if (rc) return rc;
        hipLaunchKernelGGL(k_ij_hdr_init, dim3(1), dim3(kJoinThreads), 0, os.stream, F.hdr);
        hipLaunchKernelGGL(k_ij_filter, dim3(grid_for(n)), dim3(kJoinThreads), 0, os.stream, n, key, ts, side, b, wm,
                           (uint32_t*)nullptr, F.hdr);
        int64_t h[kIjHdr];
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = read_hdr(h, F.hdr, kIjHdr, os.stream);
        if (e != hipSuccess) return er.dev_fail(e);
        std::string why;
        if ((rc = ij_flag_error((uint64_t)h[IH_FLAGS], why))) return er.fail(rc, "%s", why.c_str());
        return GW_OK;
    }

    // One pass: m records of `side` in device columns, already ordered behind their producer.
    // The columns are free once this returns.
    int pass(int side, int64_t m, const int64_t* key, const int64_t* ts, const int64_t* pay, int64_t* made) {
        hipStream_t stream = os.stream;
        IjArrays A;
        int rc = carve_from([&](Carve& c) { A.carve(c, m, true); }, scr, er, os.stream);
        if (rc) return rc;
        int64_t h[kIjHdr];
        hipError_t e = ij_launch_filter(m, key, ts, pay, side, b, wm, A, A.c, stream);
        if (e == hipSuccess) e = read_hdr(h, A.hdr, kIjHdr, stream);
        if (e != hipSuccess) return er.dev_fail(e);
        std::string why;
        if ((rc = ij_flag_error((uint64_t)h[IH_FLAGS], why))) return er.fail(rc, "%s", why.c_str());
        const int64_t kept = h[IH_KEPT];
        late += h[IH_LATE];
        if (kept == 0) return GW_OK;
        if (n_log[side] + kept > kSortMaxRecords)
            return er.fail(GW_E_UNSUPPORTED, "interval join: more than 2^30 - 1 live records on one side");
        if ((e = ij_sort(A, kept, h, stream)) != hipSuccess) return er.dev_fail(e);
        timed = true;
        probe_t.begin(stream);
        const IjLog other = side_log(1 - side);
        if (other.n > 0) {
            e = ij_launch_probe(A, kept, side, b, other, stream);
            if (e == hipSuccess) e = hipMemcpyAsync(h, A.hdr, sizeof h, hipMemcpyDeviceToHost, stream);
            probe_t.end(stream);
            if (e == hipSuccess) e = hipStreamSynchronize(stream);
            if (e != hipSuccess) return er.dev_fail(e);
            const int64_t P = h[IH_P], nc = h[IH_NC];
            if (P > kIjMaxRows - rows.pending) return er.fail(GW_E_RANGE, "interval join: the pending rows exceed int64 bytes");
            if (P > 0) {
                if (rows.reserve(P, stream) != hipSuccess) {
                    (void)hipGetLastError();
                    return er.fail(GW_E_OOM, "interval join: out of device memory for %lld pending rows",
                                   (long long)(rows.pending + P));
                }
                IjOut o;
                rows.tail(o.col);
                if ((e = ij_launch_expand(A, P, nc, side, other, o, stream)) != hipSuccess) return er.dev_fail(e);
                rows.pending += P;
                *made += P;
            }
        } else {
            probe_t.end(stream);
        }
        // the batch joins its own side's log, in the log's other buffer
        const int64_t need = n_log[side] + kept;
        if ((rc = reserve_alt(side, need, true))) return rc;
        merge_t.begin(stream);
        hipLaunchKernelGGL(k_ij_merge, dim3(grid_for(need)), dim3(kJoinThreads), 0, stream, A.sorted(kept), side_log(side),
                           alt[side][0], alt[side][1], alt[side][2]);
        merge_t.end(stream);
        if ((e = hipGetLastError()) != hipSuccess) return er.dev_fail(e);
        std::swap(log[side], alt[side]);
        n_log[side] = need;
        ++st.merges;
        return GW_OK;
    }

    int advance(int64_t w) {
        if (w <= wm) return GW_OK;  // a watermark that does not advance is ignored
        hipStream_t stream = os.stream;
        for (int sd = 0; sd < 2; ++sd) {
            const int64_t n = n_log[sd];
            if (n == 0) continue;
            IjFilterArrays F;
            int rc = carve_from([&](Carve& c) { F.carve(c, n); }, scr, er, os.stream);
            if (rc) return rc;
            if ((rc = reserve_alt(sd, n, false))) return rc;
            hipLaunchKernelGGL(k_ij_evict_flags, dim3(grid_for(n)), dim3(kJoinThreads), 0, stream, n, log[sd][1], sd, b, w, F.keep);
            hipError_t e = scan_excl<uint32_t, uint32_t>(F.keep, F.koff, n, F.blk, F.hdr + IH_KEPT, stream);
            if (e != hipSuccess) return er.dev_fail(e);
            Cols3 c{{log[sd][0], log[sd][1], log[sd][2]}, {alt[sd][0], alt[sd][1], alt[sd][2]}};
            hipLaunchKernelGGL(k_compact3, dim3(grid_for(n)), dim3(kJoinThreads), 0, stream, n, F.keep, F.koff, c);
            int64_t kept = 0;
            e = hipGetLastError();
            if (e == hipSuccess) e = read_hdr(&kept, F.hdr + IH_KEPT, 1, stream);
            if (e != hipSuccess) return er.dev_fail(e);
            std::swap(log[sd], alt[sd]);
            n_log[sd] = kept;
        }
        wm = w;
        return GW_OK;
    }
};

extern "C" {

int gw_interval_join_device(int32_t probe_side, int64_t n_p, const int64_t* d_pkey, const int64_t* d_pts,
                            const int64_t* d_ppay, int64_t n_b, const int64_t* d_bkey, const int64_t* d_bts,
                            const int64_t* d_bpay, int64_t lower, int64_t upper, int64_t* d_key_out, int64_t* d_lts_out,
                            int64_t* d_rts_out, int64_t* d_lpay_out, int64_t* d_rpay_out, int64_t cap, int64_t* n_out,
                            void* stream) {
    std::string why;
    int64_t* const out[5] = {d_key_out, d_lts_out, d_rts_out, d_lpay_out, d_rpay_out};
    const int rc = ij_device(probe_side, n_p, d_pkey, d_pts, d_ppay, n_b, d_bkey, d_bts, d_bpay, lower, upper, out, cap, n_out,
                             (hipStream_t)stream, nullptr, why);
    if (rc) set_last_error(why);
    return rc;
}

int gw_interval_join_device_timed(int32_t probe_side, int64_t n_p, const int64_t* d_pkey, const int64_t* d_pts,
                                  const int64_t* d_ppay, int64_t n_b, const int64_t* d_bkey, const int64_t* d_bts,
                                  const int64_t* d_bpay, int64_t lower, int64_t upper, int64_t* d_key_out,
                                  int64_t* d_lts_out, int64_t* d_rts_out, int64_t* d_lpay_out, int64_t* d_rpay_out,
                                  int64_t cap, int64_t* n_out, void* stream, double* expand_ms) {
    if (!expand_ms) { set_last_error("interval join: null expand_ms"); return GW_E_INVALID; }
    std::string why;
    int64_t* const out[5] = {d_key_out, d_lts_out, d_rts_out, d_lpay_out, d_rpay_out};
    const int rc = ij_device(probe_side, n_p, d_pkey, d_pts, d_ppay, n_b, d_bkey, d_bts, d_bpay, lower, upper, out, cap, n_out,
                             (hipStream_t)stream, expand_ms, why);
    if (rc) set_last_error(why);
    return rc;
}

int gw_interval_join_host(int32_t probe_side, int64_t n_p, const int64_t* pkey, const int64_t* pts, const int64_t* ppay,
                          int64_t n_b, const int64_t* bkey, const int64_t* bts, const int64_t* bpay, int64_t lower,
                          int64_t upper, int64_t* key_out, int64_t* lts_out, int64_t* rts_out, int64_t* lpay_out,
                          int64_t* rpay_out, int64_t cap, int64_t* n_out) {
    std::string why;
    int rc = ij_args(probe_side, n_p, n_b, lower, upper, cap, n_out, why);
    if (rc) { set_last_error(why); return rc; }
    *n_out = 0;
    if (n_p == 0 || n_b == 0) return GW_OK;
    if (!pkey || !pts || !ppay || !bkey || !bts || !bpay || (cap > 0 && (!key_out || !lts_out || !rts_out || !lpay_out || !rpay_out))) {
        set_last_error("interval join: null column");
        return GW_E_INVALID;
    }
    const IjBounds b{lower, upper};
    uint64_t flags = 0;
    for (int64_t i = 0; i < n_b; ++i) flags |= bts[i] == INT64_MIN ? GW_DF_NO_TS : ij_fits(1 - probe_side, bts[i], b) ? 0 : GW_DF_RANGE;
    for (int64_t i = 0; i < n_p; ++i) flags |= pts[i] == INT64_MIN ? GW_DF_NO_TS : ij_fits(probe_side, pts[i], b) ? 0 : GW_DF_RANGE;
    if ((rc = ij_flag_error(flags, why))) { set_last_error(why); return rc; }
    try {
        // the buffer as the operator keeps it: by (key, ts), equal ones in arrival order
        std::vector<int64_t> idx((size_t)n_b), sk((size_t)n_b), st((size_t)n_b);
        std::iota(idx.begin(), idx.end(), (int64_t)0);
        std::stable_sort(idx.begin(), idx.end(), [&](int64_t x, int64_t y) {
            return bkey[x] != bkey[y] ? bkey[x] < bkey[y] : bts[x] < bts[y];
        });
        for (int64_t i = 0; i < n_b; ++i) {
            sk[(size_t)i] = bkey[idx[(size_t)i]];
            st[(size_t)i] = bts[idx[(size_t)i]];
        }
        const IjBounds rel = ij_relative(probe_side, b);
        std::vector<int64_t> first((size_t)n_p), end((size_t)n_p);
        int64_t total = 0;  // below 2^60
        for (int64_t i = 0; i < n_p; ++i) {
            first[(size_t)i] = ij_bound<false>(sk.data(), st.data(), 0, n_b, pkey[i], pts[i] + rel.lower);
            end[(size_t)i] = ij_bound<true>(sk.data(), st.data(), first[(size_t)i], n_b, pkey[i], pts[i] + rel.upper);
            total += end[(size_t)i] - first[(size_t)i];
        }
        if (total > kIjMaxRows) { set_last_error("interval join: the rows of one call exceed int64 bytes"); return GW_E_RANGE; }
        *n_out = total;
        if (total > cap) { set_last_error("interval join: output arrays too small"); return GW_E_OUTPUT_FULL; }
        const bool left = probe_side == GW_JOIN_LEFT;
        int64_t o = 0;
        for (int64_t i = 0; i < n_p; ++i)
            for (int64_t j = first[(size_t)i]; j < end[(size_t)i]; ++j, ++o) {
                const int64_t x = idx[(size_t)j];
                key_out[o] = pkey[i];
                lts_out[o] = left ? pts[i] : bts[x];
                rts_out[o] = left ? bts[x] : pts[i];
                lpay_out[o] = left ? ppay[i] : bpay[x];
                rpay_out[o] = left ? bpay[x] : ppay[i];
            }
    } catch (const std::bad_alloc&) {
        set_last_error("interval join: out of host memory");
        return GW_E_OOM;
    }
    return GW_OK;
}

int gw_ijoin_create(const gw_ijoin_config* cfg, gw_ijoin** out) {
    if (!cfg || !out) { set_last_error("gw_ijoin_create: null argument"); return GW_E_INVALID; }
    *out = nullptr;
    if (cfg->lower > cfg->upper || cfg->lower < -GW_IJOIN_MAX_BOUND || cfg->upper > GW_IJOIN_MAX_BOUND) {
        set_last_error("interval join: the bounds must satisfy -2^62 <= lower <= upper <= 2^62");
        return GW_E_INVALID;
    }
    if (cfg->capacity_hint < 0 || cfg->max_batch < 0) { set_last_error("gw_ijoin_create: negative capacity"); return GW_E_INVALID; }
    gw_ijoin* h = new (std::nothrow) gw_ijoin();
    if (!h) { set_last_error("gw_ijoin_create: out of host memory"); return GW_E_OOM; }
    auto bail = [&](int code, const std::string& msg) {
        set_last_error(msg);
        gw_ijoin_destroy(h);
        return code;
    };
    h->cfg = *cfg;
    h->b = IjBounds{cfg->lower, cfg->upper};
    h->max_batch = cfg->max_batch > 0 ? std::min<int64_t>(cfg->max_batch, kSortMaxRecords) : (int64_t)1 << 22;
    const char* what;
    hipError_t e = h->os.create(cfg->device, &what);
    if (e != hipSuccess) return bail(GW_E_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
    if ((e = h->probe_t.create()) != hipSuccess || (e = h->merge_t.create()) != hipSuccess)
        return bail(GW_E_DEVICE, std::string("hipEventCreate: ") + hipGetErrorString(e));
    const int64_t cap0 = std::max<int64_t>(cfg->capacity_hint, 16);
    for (int sd = 0; sd < 2; ++sd)
        if (h->log[sd].reserve_keep(cap0, 0, 0, h->os.stream) != hipSuccess || h->alt[sd].reserve_keep(cap0, 0, 0, h->os.stream) != hipSuccess)
            return bail(GW_E_OOM, "interval join: out of device memory");
    *out = h;
    return GW_OK;
}

int gw_ijoin_destroy(gw_ijoin* h) {
    if (!h) return GW_OK;
    h->os.destroy();
    delete h;  // (the timing events go with it: the stream they were recorded on has been waited for)
    return GW_OK;
}

const char* gw_ijoin_last_error(const gw_ijoin* h) { return h ? h->er.err.c_str() : gw_last_error(nullptr); }

static int ij_ingested(gw_ijoin* h, int rc, int64_t made, int64_t* rows) {
    if (rc) return rc;
    h->st.rows_emitted += made;
    h->st.last_call_rows = made;
    if (rows) *rows = made;
    return GW_OK;
}

int gw_ijoin_ingest_device(gw_ijoin* h, int32_t side, int64_t n, const int64_t* d_key, const int64_t* d_ts,
                           const int64_t* d_payload, void* stream, int64_t* rows) {
    GW_OP_ENTER(h);
    if (rows) *rows = 0;
    if ((side != GW_JOIN_LEFT && side != GW_JOIN_RIGHT) || n < 0 || (n > 0 && (!d_key || !d_ts || !d_payload)))
        return h->er.fail(GW_E_INVALID, "gw_ijoin_ingest_device: bad side or null column");
    OpStream::Handoff handoff(h->os, (hipStream_t)stream, n > 0);
    int64_t made = 0;
    int rc = n > h->max_batch ? h->check_call(side, n, d_key, d_ts) : GW_OK;
    for (int64_t at = 0; at < n && rc == GW_OK; at += h->max_batch)
        rc = h->pass(side, std::min(h->max_batch, n - at), d_key + at, d_ts + at, d_payload + at, &made);
    return ij_ingested(h, rc, made, rows);
}

int gw_ijoin_ingest(gw_ijoin* h, int32_t side, int64_t n, const int64_t* key, const int64_t* ts, const int64_t* payload,
                    int64_t* rows) {
    GW_OP_ENTER(h);
    if (rows) *rows = 0;
    if ((side != GW_JOIN_LEFT && side != GW_JOIN_RIGHT) || n < 0 || (n > 0 && (!key || !ts || !payload)))
        return h->er.fail(GW_E_INVALID, "gw_ijoin_ingest: bad side or null column");
    if (n > h->max_batch) {  // several passes: the checks over the whole call first
        uint64_t flags = 0;
        for (int64_t i = 0; i < n; ++i) {
            if (ts[i] == INT64_MIN) flags |= GW_DF_NO_TS;
            else if (!(h->wm != INT64_MIN && ts[i] < h->wm) && !ij_fits(side, ts[i], h->b)) flags |= GW_DF_RANGE;
        }
        std::string why;
        const int rc = ij_flag_error(flags, why);
        if (rc) return h->er.fail(rc, "%s", why.c_str());
    }
    int64_t made = 0;
    const int64_t* src[3] = {key, ts, payload};
    // (the pass waits for the stream behind its filter, so the host columns and the staging
    // columns are free when it returns)
    const int rc = staged_ingest(h->stage, h->max_batch, n, src, h->os.stream, h->er,
                                 [&](int64_t m, int64_t* const* d) { return h->pass(side, m, d[0], d[1], d[2], &made); });
    return ij_ingested(h, rc, made, rows);
}

int gw_ijoin_advance_watermark(gw_ijoin* h, int64_t watermark) {
    GW_OP_ENTER(h);
    return h->advance(watermark);
}

int gw_ijoin_end_input(gw_ijoin* h) {
    GW_OP_ENTER(h);
    return h->advance(INT64_MAX);
}

int gw_ijoin_pending(gw_ijoin* h, int64_t* n) {
    GW_OP_ENTER(h);
    if (!n) return h->er.fail(GW_E_INVALID, "gw_ijoin_pending: null argument");
    *n = h->rows.pending;
    return GW_OK;
}

int gw_ijoin_drain(gw_ijoin* h, int64_t* key, int64_t* lts, int64_t* rts, int64_t* lpay, int64_t* rpay, int64_t cap,
                   int64_t* n) {
    GW_OP_ENTER(h);
    if (!n || cap < 0 || (cap > 0 && (!key || !lts || !rts || !lpay || !rpay)))
        return h->er.fail(GW_E_INVALID, "gw_ijoin_drain: bad argument");
    int64_t* const dst[5] = {key, lts, rts, lpay, rpay};
    return h->rows.drain(dst, nullptr, cap, n, h->os.stream, h->er);
}

int gw_ijoin_rows_device(gw_ijoin* h, const int64_t** d_key, const int64_t** d_lts, const int64_t** d_rts,
                         const int64_t** d_lpay, const int64_t** d_rpay, int64_t* n) {
    GW_OP_ENTER(h);
    if (!d_key || !d_lts || !d_rts || !d_lpay || !d_rpay || !n) return h->er.fail(GW_E_INVALID, "gw_ijoin_rows_device: null argument");
    // (an ingest returns with its expand kernel in flight: the view is of finished rows)
    const hipError_t e = hipStreamSynchronize(h->os.stream);
    if (e != hipSuccess) return h->er.dev_fail(e);
    const int64_t** const dst[5] = {d_key, d_lts, d_rts, d_lpay, d_rpay};
    h->rows.view(dst, nullptr, n);
    return GW_OK;
}

int gw_ijoin_clear_rows(gw_ijoin* h) {
    GW_OP_ENTER(h);
    h->rows.clear();
    return GW_OK;
}

int64_t gw_ijoin_late_dropped(const gw_ijoin* h) { return h ? h->late : 0; }

int gw_ijoin_get_stats(const gw_ijoin* h, gw_ijoin_stats* out) {
    if (!h || !out) return GW_E_INVALID;
    *out = h->st;
    out->live_left = h->n_log[0];
    out->live_right = h->n_log[1];
    out->log_capacity_left = h->log[0].cap;
    out->log_capacity_right = h->log[1].cap;
    return GW_OK;
}

int gw_ijoin_last_times(gw_ijoin* h, double* probe_ms, double* merge_ms) {
    GW_OP_ENTER(h);
    if (!probe_ms || !merge_ms) return h->er.fail(GW_E_INVALID, "gw_ijoin_last_times: null argument");
    *probe_ms = *merge_ms = 0;
    if (!h->timed) return GW_OK;
    hipError_t e = hipStreamSynchronize(h->os.stream);
    if (e != hipSuccess) return h->er.dev_fail(e);
    float p = 0, m = 0;
    if ((e = h->probe_t.elapsed(&p)) != hipSuccess) return h->er.dev_fail(e);
    // (a pass that kept nothing, or failed before its merge, leaves the merge's events of an earlier pass)
    if (h->merge_t.elapsed(&m) != hipSuccess) {
        (void)hipGetLastError();
        m = 0;
    }
    *probe_ms = p;
    *merge_ms = m;
    return GW_OK;
}

void* gw_ijoin_stream(gw_ijoin* h) { return h ? (void*)h->os.stream : nullptr; }

}  // extern "C"
