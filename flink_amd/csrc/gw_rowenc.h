// gw_rowenc.h — fired rows as serialized stream elements (gw_rowenc.hip; include/gpuwin.h
// gw_encode_rows_device / gw_encode_rows_host and the handle calls built on them).
//
// A row becomes what RecordWriter.serializeRecord + StreamElementSerializer.serialize write
// for a StreamRecord<TupleN> with a timestamp (flink_amd/netbuf.py record()):
//   be32 length | tag 0 | be64 timestamp | the fields, big-endian
// so a row is 13 + 8 * (longs and doubles) + 4 * ints bytes: always odd, the same for every
// row of a call.
#pragma once
#include <string>

#include "gw_common.h"

namespace gw {

constexpr int kRowSources = 5;       // GW_ROW_KEY .. GW_ROW_PAYLOAD
constexpr int kWatermarkBytes = 13;  // be32 9 | tag 2 | be64 timestamp (netbuf.watermark)
constexpr int kEncMaxChannels = 128;

// A checked gw_row_layout in the form the encoders read (a kernel argument: its arrays are
// only ever indexed by constants).
struct RowPlan {
    int32_t nfields;
    int32_t row_bytes;             // 4 + 1 + 8 + the fields
    int32_t src[GW_MAX_FIELDS];    // GW_ROW_*
    int32_t width[GW_MAX_FIELDS];  // 8 or 4
    uint32_t used;                 // bit s: source column s is read (GW_ROW_END for the timestamp)
    int32_t global_window;         // timestamp Long.MAX_VALUE instead of end - 1
};

// GW_OK, or GW_E_INVALID with the reason in why.  have_payload: a payload column is given.
int row_plan(const gw_row_layout* l, int32_t mode, bool have_payload, RowPlan& p, std::string& why);

// Channel of a row key (KeyGroupStreamPartitioner.selectChannel for a Long key).
GW_HD int32_t row_channel(int64_t key, int32_t max_p, int32_t channels) {
    return operator_for_key_group(max_p, channels, key_group_for_hash(java_long_hash(key), max_p));
}

// Byte ranges of the channels from their row counts: chan_off (16-byte aligned starts) and
// chan_bytes; returns the needed total (the end of the last range).
int64_t row_ranges(const RowPlan& p, int32_t channels, const int64_t* rows, bool has_wm, int64_t* chan_off,
                   int64_t* chan_bytes);

// The contract of gw_encode_rows_host / gw_encode_rows_device with the arguments checked
// (channels in [1, kEncMaxChannels], n >= 0, cap >= 0, columns present).  col[s]: source s.
int row_encode_host(int64_t n, const int64_t* const col[kRowSources], const RowPlan& p, int32_t channels,
                    int32_t max_p, int64_t watermark, uint8_t* bytes, int64_t cap, int64_t* chan_off,
                    int64_t* chan_bytes, std::string& why);
// Device columns and bytes (16-byte aligned); waits on s.  Scratch is owned per device.
int row_encode_run(int64_t n, const int64_t* const col[kRowSources], const RowPlan& p, int32_t channels,
                   int32_t max_p, int64_t watermark, uint8_t* d_bytes, int64_t cap, int64_t* chan_off,
                   int64_t* chan_bytes, hipStream_t s, std::string& why);

}  // namespace gw
