// gw_netbuf.h — network-buffer decode (gw_netbuf.hip): layout, status, launcher.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gpuwin.h"

namespace gw {

#ifndef GW_NB_CHUNK
#define GW_NB_CHUNK 1024
#endif
constexpr int kNbChunk = GW_NB_CHUNK;  // bytes per wave in the chain walk

// The record value layout reduced to what the decoder needs (validated on the host).
struct NbLayout {
    int32_t vbytes;    // serialized value bytes (sum of the field widths)
    int32_t key_off;   // byte offset of the Long key field in the value
    int32_t val_off;   // byte offset of the aggregated field
    int32_t val_type;  // its type code ('J', 'D', ...), 0 = none (COUNT)
};

// corrupt / unsupported: 0 = none, otherwise nb_error_rank of the earliest byte position that
// raised it (larger = earlier).  The sequential reader fails on the stream's first bad element;
// the chunks behind it may still decode (from a later chunk with a unique exit) and raise errors
// of their own, so of the two the one with the larger rank is the stream's (nb_corrupt_first).
struct NbStatus {
    unsigned long long corrupt;      // unknown tag / length that does not match the element
    unsigned long long unsupported;  // an element longer than GW_MAX_ELEMENT
    unsigned long long full;         // rec_cap / wm_cap exceeded
    unsigned long long skipped;      // latency markers, stream status, record attributes
    long long consumed;              // bytes up to the end of the last complete element
    long long records, watermarks;
    unsigned long long walkback;     // chunk steps k_nb_resolve walked back over non-converged chunks
    unsigned long long fallback;     // chunks whose candidates disagreed after the sync window
};

__host__ __device__ inline unsigned long long nb_error_rank(int64_t pos) {
    return (1ull << 62) - (unsigned long long)pos;
}
// corrupt is the stream's first error (a chunk-granular corrupt rank ties towards corrupt)
inline bool nb_corrupt_first(const NbStatus& st) { return st.corrupt && st.corrupt >= st.unsupported; }

inline int nb_field_width(char t) {
    switch (t) {
    case 'J': case 'D': return 8;
    case 'I': case 'F': return 4;
    case 'S': return 2;
    case 'B': case 'Z': return 1;
    default: return -1;
    }
}

int64_t nb_scratch_bytes(int64_t nbytes);
hipError_t launch_nb_decode(const uint8_t* buf, int64_t nbytes, const NbLayout& L, int64_t* key, int64_t* ts,
                            int64_t* val, int64_t rec_cap, int64_t* wm_pos, int64_t* wm_val, int64_t wm_cap,
                            void* scratch, NbStatus* d_st, hipStream_t s);

// ---- segmented decode: many byte ranges (input channels) in one pipeline run ----
// Every range starts on a chunk of its own, so the chunks of all ranges form one virtual
// stream: range r's byte b stands at virtual position first[r] * kNbChunk + b, where first[r]
// is the number of chunks of the ranges before it.  Positions, error ranks and the scans work
// on virtual positions; only where a chunk's bytes lie and where they end comes from a
// per-chunk descriptor (k_nb_desc builds them on the device from the range table).
struct NbRange {
    const uint8_t* ptr;  // device pointer, 4-byte aligned
    int64_t len;         // bytes (0 allowed)
    int64_t first;       // index of the range's first chunk (nb_seg_plan fills it)
};
struct NbChunkDesc {
    const uint8_t* ptr;  // the chunk's first byte
    int64_t left;        // bytes from there to the end of its range
    int32_t range;       // the range it belongs to
    int32_t first;       // the range's first chunk (== this chunk: chains enter at byte 0)
};
// Sets ranges[r].first; returns the total chunk count, or -1 where it exceeds what a descriptor holds.
int64_t nb_seg_plan(NbRange* ranges, int32_t nranges);
int64_t nb_seg_scratch_bytes(int64_t nchunks, int32_t nranges);
// ranges: host memory that stays valid until the stream has run (pinned for an asynchronous
// copy), `first` set by nb_seg_plan.  d_rng: 3 * nranges words, written as consumed[r] |
// first record of range r | first event of range r (the latter two only for ranges with bytes).
// Events: ev_pos (records of the whole call before it), ev_kind (0 watermark, 1 watermark
// status), ev_val; d_st->watermarks counts them all.
hipError_t launch_nb_decode_seg(const NbRange* ranges, int32_t nranges, int64_t nchunks, const NbLayout& L,
                                int64_t* key, int64_t* ts, int64_t* val, int64_t rec_cap, int64_t* ev_pos,
                                int32_t* ev_kind, int64_t* ev_val, int64_t ev_cap, void* scratch, NbStatus* d_st,
                                int64_t* d_rng, hipStream_t s);

}  // namespace gw
