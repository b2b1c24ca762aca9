// gw_rowenc.hip — fired rows to network-buffer bytes on the device (include/gpuwin.h
// gw_encode_rows_device, gw_encode_rows_host; the format: gw_rowenc.h).
//
// The output side's counterpart of gw_netbuf.hip: the (key, start, end, result[, payload])
// columns a fire leaves in device memory become the bytes RecordWriter.serializeRecord would
// have produced for every row, one contiguous range per downstream channel, so a JVM task
// hands slices to its partition writer instead of building and serializing an object per row,
// and a second operator on the same GPU takes them through gw_ingest_serialized_device.
//
// Rows are fixed-width but odd-sized (13 + 8a + 4b bytes), so a row starts at any byte
// alignment.  Four consecutive rows, though, are a whole number of dwords.  One workgroup takes
// a tile of kEncTile consecutive rows of one channel:
//   load    the columns the layout reads, coalesced (thread t: rows t, t + 128, ...), into LDS;
//   encode  thread t turns rows 4t .. 4t + 3 into row_bytes dwords of its own in the LDS image
//           of the tile's bytes: a little shift register fed big-endian words, flushed a dword
//           at a time.  The byte positions depend on the layout alone, so the control flow is
//           the same in every lane; a thread's dwords are row_bytes (odd) apart from its
//           neighbour's, so the LDS writes meet no bank conflicts;
//   store   the image goes out as 16-byte vectors, lane after lane (tile starts are 16-byte
//           aligned: kEncTile * row_bytes is a multiple of 16 and channels start aligned).
// Only the last tile of a channel has a tail of fewer than 16 bytes, stored bytewise; the
// channel's watermark element is appended to that tile's image.
//
// channels > 1: the columns are first partitioned by channel with the keyBy partition of
// gw_keygroups.hip (launch_partition: stable, the same owner computation as the exchange), into
// scratch; the row counts come to the host, which lays out the ranges, and the same kernel runs
// over the partitioned columns with a small table telling each workgroup its channel.
#include "gw_rowenc.h"

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "gw_devmem.h"
#include "gw_kernels.h"

namespace gw {

constexpr int kEncThreads = 128, kEncTile = 4 * kEncThreads;

// Rows [row0, row0 + rows) of the (partitioned) columns are one channel's, encoded from byte
// byte0 of the output by tiles tile0 ...
struct EncChan {
    int64_t tile0, row0, rows, byte0;
};
struct EncCols {
    const int64_t* p[kRowSources];
};

int row_plan(const gw_row_layout* l, int32_t mode, bool have_payload, RowPlan& p, std::string& why) {
    if (!l) { why = "row layout: null"; return GW_E_INVALID; }
    if (mode & ~GW_ENCODE_GLOBAL_WINDOW) { why = "row layout: unknown mode bits"; return GW_E_INVALID; }
    if (l->nfields < 1 || l->nfields > GW_MAX_FIELDS) { why = "row layout: 1..GW_MAX_FIELDS fields"; return GW_E_INVALID; }
    p = RowPlan{};
    p.nfields = l->nfields;
    p.row_bytes = 4 + 1 + 8;
    p.global_window = (mode & GW_ENCODE_GLOBAL_WINDOW) ? 1 : 0;
    if (!p.global_window) p.used |= 1u << GW_ROW_END;
    for (int f = 0; f < l->nfields; ++f) {
        const int32_t s = l->source[f];
        const char t = l->types[f];
        if (s < 0 || s >= kRowSources) { why = "row layout: unknown field source"; return GW_E_INVALID; }
        if (t != 'J' && t != 'D' && t != 'I') { why = "row layout: field types are 'J', 'D' or 'I'"; return GW_E_INVALID; }
        if (t == 'D' && s != GW_ROW_RESULT) { why = "row layout: 'D' only from GW_ROW_RESULT"; return GW_E_INVALID; }
        if (s == GW_ROW_PAYLOAD && !have_payload) { why = "row layout: GW_ROW_PAYLOAD without a payload column"; return GW_E_INVALID; }
        p.src[f] = s;
        p.width[f] = t == 'I' ? 4 : 8;
        p.row_bytes += p.width[f];
        p.used |= 1u << s;
    }
    return GW_OK;
}

int64_t row_ranges(const RowPlan& p, int32_t channels, const int64_t* rows, bool has_wm, int64_t* chan_off,
                   int64_t* chan_bytes) {
    int64_t off = 0, end = 0;
    for (int32_t c = 0; c < channels; ++c) {
        chan_off[c] = off;
        chan_bytes[c] = rows[c] * p.row_bytes + (has_wm ? kWatermarkBytes : 0);
        end = off + chan_bytes[c];
        off = (end + 15) & ~(int64_t)15;
    }
    return end;
}

// ---- host --------------------------------------------------------------------------------
static inline uint8_t* put_be(uint8_t* o, uint64_t v, int nbytes) {
    for (int b = nbytes - 1; b >= 0; --b) *o++ = (uint8_t)(v >> (8 * b));
    return o;
}
static inline uint8_t* put_watermark(uint8_t* o, int64_t wm) {
    o = put_be(o, kWatermarkBytes - 4, 4);
    *o++ = 2;  // StreamElementSerializer TAG_WATERMARK
    return put_be(o, (uint64_t)wm, 8);
}

int row_encode_host(int64_t n, const int64_t* const col[kRowSources], const RowPlan& p, int32_t channels,
                    int32_t max_p, int64_t watermark, uint8_t* bytes, int64_t cap, int64_t* chan_off,
                    int64_t* chan_bytes, std::string& why) {
    const bool has_wm = watermark != INT64_MIN;
    std::vector<int64_t> rows((size_t)channels, 0);
    if (channels == 1) rows[0] = n;
    else
        for (int64_t i = 0; i < n; ++i) ++rows[(size_t)row_channel(col[GW_ROW_KEY][i], max_p, channels)];
    const int64_t need = row_ranges(p, channels, rows.data(), has_wm, chan_off, chan_bytes);
    if (need > cap) {
        chan_off[0] = need;
        why = "row encode: output buffer too small";
        return GW_E_OUTPUT_FULL;
    }
    std::vector<int64_t> at(chan_off, chan_off + channels);  // next byte of every channel
    for (int64_t i = 0; i < n; ++i) {
        const int32_t c = channels == 1 ? 0 : row_channel(col[GW_ROW_KEY][i], max_p, channels);
        uint8_t* o = bytes + at[(size_t)c];
        o = put_be(o, (uint64_t)(p.row_bytes - 4), 4);
        *o++ = 0;  // TAG_REC_WITH_TIMESTAMP
        o = put_be(o, p.global_window ? (uint64_t)INT64_MAX : (uint64_t)col[GW_ROW_END][i] - 1ull, 8);
        for (int f = 0; f < p.nfields; ++f) {
            const int64_t v = col[p.src[f]][i];
            if (p.width[f] == 4 && v != (int64_t)(int32_t)v) {
                why = "row encode: a value of an 'I' field does not fit a Java int";
                return GW_E_RANGE;
            }
            o = put_be(o, (uint64_t)v, p.width[f]);
        }
        at[(size_t)c] += p.row_bytes;
    }
    if (has_wm)
        for (int32_t c = 0; c < channels; ++c) put_watermark(bytes + at[(size_t)c], watermark);
    return GW_OK;
}

// ---- device ------------------------------------------------------------------------------
// The encode step's shift register: bytes wait in the low end of acc (npend of them, the same
// in every lane) until a dword is full.
struct DwordStream {
    uint32_t* w;
    uint64_t acc = 0;
    int npend = 0;
    __device__ __forceinline__ void word(uint32_t be) {  // 4 bytes, most significant first
        acc |= (uint64_t)__builtin_bswap32(be) << (8 * npend);
        *w++ = (uint32_t)acc;
        acc >>= 32;
    }
    __device__ __forceinline__ void dword(uint64_t be) {
        word((uint32_t)(be >> 32));
        word((uint32_t)be);
    }
    __device__ __forceinline__ void byte(uint32_t b) {
        acc |= (uint64_t)b << (8 * npend);
        if (++npend == 4) {
            *w++ = (uint32_t)acc;
            acc = 0;
            npend = 0;
        }
    }
};

// Dynamic LDS: [columns read][kEncTile] int64, then the tile's bytes (kEncTile * row_bytes +
// a watermark, rounded up to 16).
__global__ void __launch_bounds__(kEncThreads)
k_rowenc(RowPlan p, EncCols cols, const EncChan* __restrict__ table, int nchan, EncChan one, int64_t wm, int has_wm,
         uint8_t* __restrict__ out, unsigned* flag) {
    extern __shared__ uint4 enc_lds[];
    const int t = threadIdx.x;
    EncChan ch = one;
    if (nchan > 1) {  // the last channel whose first tile is not past this one
        int lo = 0, hi = nchan - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (table[mid].tile0 <= (int64_t)blockIdx.x) lo = mid;
            else hi = mid - 1;
        }
        ch = table[lo];
    }
    const int64_t r0 = ((int64_t)blockIdx.x - ch.tile0) * kEncTile;  // first row of the tile in its channel
    const int rows = (int)min((int64_t)kEncTile, ch.rows - r0);     // 0: an empty channel's watermark
    const bool last = r0 + kEncTile >= ch.rows;
    const int rb = p.row_bytes;
    int64_t* stage = reinterpret_cast<int64_t*>(enc_lds);
    const int ncols = __popc(p.used);
    uint32_t* image = reinterpret_cast<uint32_t*>(stage + ncols * kEncTile);

#pragma unroll
    for (int s = 0; s < kRowSources; ++s) {
        if (!(p.used >> s & 1)) continue;
        const int64_t* __restrict__ src = cols.p[s] + ch.row0 + r0;
        int64_t* dst = stage + __popc(p.used & ((1u << s) - 1u)) * kEncTile;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = j * kEncThreads + t;
            if (r < rows) dst[r] = src[r];
        }
    }
    __syncthreads();

    bool bad = false;
    if (4 * t < rows) {
        DwordStream o;
        o.w = image + t * rb;  // 4 rows = rb dwords
        const int64_t* s_end = stage + __popc(p.used & ((1u << GW_ROW_END) - 1u)) * kEncTile;
#pragma unroll 1
        for (int q = 0; q < 4; ++q) {
            const int r = 4 * t + q;
            const bool valid = r < rows;  // rows past the tile: dwords the store never reads
            o.word((uint32_t)(rb - 4));
            o.byte(0);  // TAG_REC_WITH_TIMESTAMP
            o.dword(p.global_window ? (uint64_t)INT64_MAX : (uint64_t)s_end[r] - 1ull);
#pragma unroll
            for (int f = 0; f < GW_MAX_FIELDS; ++f) {
                if (f >= p.nfields) break;
                const int64_t v = stage[__popc(p.used & ((1u << p.src[f]) - 1u)) * kEncTile + r];
                if (p.width[f] == 8) {
                    o.dword((uint64_t)v);
                } else {
                    bad |= valid && v != (int64_t)(int32_t)v;
                    o.word((uint32_t)v);
                }
            }
        }
    }
    if (bad) atomicOr(flag, 1u);
    __syncthreads();

    uint8_t* image_b = reinterpret_cast<uint8_t*>(image);
    int len = rows * rb;
    if (last && has_wm) {  // the same in every thread of the workgroup
        if (t < kWatermarkBytes)
            image_b[len + t] = t < 4 ? (t == 3 ? kWatermarkBytes - 4 : 0) : t == 4 ? 2 : (uint8_t)((uint64_t)wm >> (8 * (12 - t)));
        len += kWatermarkBytes;
        __syncthreads();
    }
    uint8_t* dst = out + ch.byte0 + ((int64_t)blockIdx.x - ch.tile0) * ((int64_t)kEncTile * rb);
    uint4* dst_v = reinterpret_cast<uint4*>(dst);
    const uint4* src_v = reinterpret_cast<const uint4*>(image);
    const int nvec = len >> 4;
    for (int v = t; v < nvec; v += kEncThreads) dst_v[v] = src_v[v];
    const int tail = nvec << 4;
    if (tail + t < len) dst[tail + t] = image_b[tail + t];  // kEncThreads >= 16
}

static constexpr size_t up256(size_t b) { return (b + 255) / 256 * 256; }
static int64_t enc_tiles(int64_t rows, bool has_wm) {
    const int64_t tiles = (rows + kEncTile - 1) / kEncTile;
    return has_wm ? std::max<int64_t>(tiles, 1) : tiles;
}

int row_encode_run(int64_t n, const int64_t* const col[kRowSources], const RowPlan& p, int32_t channels,
                   int32_t max_p, int64_t watermark, uint8_t* d_bytes, int64_t cap, int64_t* chan_off,
                   int64_t* chan_bytes, hipStream_t s, std::string& why) {
    static std::mutex mu;
    static DevBuf<char>* const scr = new DevBuf<char>[64];  // per device; never freed (process exit)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { why = "row encode: no device"; return GW_E_DEVICE; }
    std::lock_guard<std::mutex> lock(mu);  // every call waits for its launches before it returns
    auto dev_fail = [&](hipError_t e) {
        why = std::string("row encode: ") + hipGetErrorString(e);
        return GW_E_DEVICE;
    };
    const bool has_wm = watermark != INT64_MIN;
    // scratch: flag | counts | table | partition scratch | partitioned columns
    constexpr size_t kFlagBytes = 256, kCountBytes = up256(kEncMaxChannels * 8),
                     kTableBytes = up256(kEncMaxChannels * sizeof(EncChan));
    const bool part = channels > 1 && n > 0;
    const bool second = part && (p.used & (1u << GW_ROW_START | 1u << GW_ROW_PAYLOAD));
    const size_t part_bytes = part ? up256((size_t)partition_scratch_bytes(n, channels)) : 0;
    const size_t col_bytes = part ? up256((size_t)n * 8) : 0;
    const size_t need_scr = kFlagBytes + kCountBytes + kTableBytes + part_bytes + col_bytes * (second ? 5 : 3);
    DevBuf<char>& S = scr[dev];
    if (S.cap < (int64_t)need_scr) {
        hipError_t e = hipStreamSynchronize(s);
        if (e != hipSuccess) return dev_fail(e);
        if (S.reserve_discard((int64_t)need_scr) != hipSuccess) {
            (void)hipGetLastError();
            why = "row encode: scratch allocation failed";
            return GW_E_OOM;
        }
    }
    unsigned* flag = reinterpret_cast<unsigned*>(S.p);
    int64_t* d_counts = reinterpret_cast<int64_t*>(S.p + kFlagBytes);
    EncChan* d_table = reinterpret_cast<EncChan*>(S.p + kFlagBytes + kCountBytes);
    char* d_part = S.p + kFlagBytes + kCountBytes + kTableBytes;
    int64_t* pc = reinterpret_cast<int64_t*>(d_part + part_bytes);  // partitioned: key | end | result | start | payload
    const size_t cw = col_bytes / 8;

    std::vector<int64_t> rows((size_t)channels, 0);
    EncCols cols{};
    for (int q = 0; q < kRowSources; ++q) cols.p[q] = col[q];
    hipError_t e = hipSuccess;
    if (part) {
        // (key, end, result), then (key, start, payload) when the layout reads those: the same
        // stable partition twice, so the columns stay row-aligned
        e = launch_partition(n, col[GW_ROW_KEY], nullptr, col[GW_ROW_END], col[GW_ROW_RESULT], max_p, channels, pc, pc + cw,
                             pc + 2 * cw, d_counts, d_part, s);
        if (e == hipSuccess && second)
            e = launch_partition(n, col[GW_ROW_KEY], nullptr, col[GW_ROW_START], col[GW_ROW_PAYLOAD], max_p, channels, pc,
                                 pc + 3 * cw, pc + 4 * cw, d_counts, d_part, s);
        if (e == hipSuccess) e = hipMemcpyAsync(rows.data(), d_counts, (size_t)channels * 8, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return dev_fail(e);
        cols.p[GW_ROW_KEY] = pc;
        cols.p[GW_ROW_END] = pc + cw;
        cols.p[GW_ROW_RESULT] = pc + 2 * cw;
        cols.p[GW_ROW_START] = pc + 3 * cw;
        cols.p[GW_ROW_PAYLOAD] = pc + 4 * cw;
    } else {
        rows[0] = n;  // (channels > 1 and no rows: every channel empty)
    }
    const int64_t need = row_ranges(p, channels, rows.data(), has_wm, chan_off, chan_bytes);
    if (need > cap) {
        chan_off[0] = need;
        why = "row encode: output buffer too small";
        return GW_E_OUTPUT_FULL;
    }
    std::vector<EncChan> table((size_t)channels);
    int64_t tiles = 0, row0 = 0;
    for (int32_t c = 0; c < channels; ++c) {
        table[(size_t)c] = EncChan{tiles, row0, rows[(size_t)c], chan_off[c]};
        tiles += enc_tiles(rows[(size_t)c], has_wm);
        row0 += rows[(size_t)c];
    }
    if (tiles == 0) return GW_OK;
    if (tiles > INT32_MAX) { why = "row encode: too many rows for one call"; return GW_E_UNSUPPORTED; }
    e = hipMemsetAsync(flag, 0, 4, s);
    if (e == hipSuccess && channels > 1)
        e = hipMemcpyAsync(d_table, table.data(), table.size() * sizeof(EncChan), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return dev_fail(e);
    const size_t image = ((size_t)kEncTile * p.row_bytes + kWatermarkBytes + 15) / 16 * 16;
    const size_t lds = (size_t)__builtin_popcount(p.used) * kEncTile * 8 + image;
    hipLaunchKernelGGL(k_rowenc, dim3((unsigned)tiles), dim3(kEncThreads), lds, s, p, cols, d_table, (int)channels, table[0],
                       watermark, has_wm ? 1 : 0, d_bytes, flag);
    e = hipGetLastError();
    unsigned h_flag = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&h_flag, flag, 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);  // also keeps table alive for its copy
    if (e != hipSuccess) return dev_fail(e);
    if (h_flag) {
        why = "row encode: a value of an 'I' field does not fit a Java int";
        return GW_E_RANGE;
    }
    return GW_OK;
}

}  // namespace gw
