/*
 * gpuwin.h — C ABI of libgpuwin.so, the MI355X-native keyed event-time window
 * aggregation operator (a drop-in for Flink's WindowOperator on the
 * keyBy().window(...).aggregate/reduce path).
 *
 * Plain C types only: pointers, sizes, int64 timestamps. No torch, no C++.
 * Every entry point returns an int status (0 = GW_OK, negative = error) and
 * never lets a C++ exception cross the boundary; gw_last_error() explains a
 * failure.  The JVM shim turns a negative status into an
 * Exception, which is exactly how the reference operator fails its task
 * ("Any exception from processElement or onEventTime fails the
 * task").
 *
 * Reference slot replaced (paths relative to the Flink tree,
 * RS/ = flink-runtime/src/main/java/org/apache/flink/streaming/):
 *   gw_create            WindowOperatorFactory.createStreamOperator
 *                          (RS/runtime/operators/windowing/WindowOperatorFactory.java:96-99)
 *                        + WindowOperator.open (WindowOperator.java:226-281)
 *   gw_ingest            WindowOperator.processElement, batched over all records
 *                        between two watermarks (WindowOperator.java:293-447;
 *                        per-record dispatch OneInputStreamTask.java:249-252)
 *   gw_advance_watermark AbstractStreamOperator.processWatermark ->
 *                        InternalTimerServiceImpl.tryAdvanceWatermark ->
 *                        WindowOperator.onEventTime
 *                        (AbstractStreamOperator.java:690-703,
 *                         InternalTimerServiceImpl.java:328-347,
 *                         WindowOperator.java:450-494)
 *   gw_drain             TimestampedCollector / Output.collect of the fired rows
 *                        (WindowOperator.emitWindowContents :575-580)
 *   gw_late_dropped      WindowOperator.numLateRecordsDropped (:144,229)
 *   gw_destroy           WindowOperator.close / dispose
 *   gw_java_long_hash,
 *   gw_murmur_hash,
 *   gw_key_group_*       KeyGroupRangeAssignment (flink-runtime/.../runtime/state/
 *                        KeyGroupRangeAssignment.java:50-147), MathUtils.murmurHash
 *                        (flink-core/.../util/MathUtils.java:137-201)
 *   gw_partition_device  KeyGroupStreamPartitioner.selectChannel
 *                        (RS/runtime/partitioner/KeyGroupStreamPartitioner.java:55-64)
 *                        feeding the RCCL all-to-all that replaces the Netty keyBy shuffle
 */
#ifndef GPUWIN_H
#define GPUWIN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GW_ABI_VERSION 3

/* ---- status codes -------------------------------------------------------- */
#define GW_OK              0
#define GW_E_INVALID      -1  /* bad argument / config (Flink: IllegalArgumentException)      */
#define GW_E_UNSUPPORTED  -2  /* valid in Flink, not (yet) on the GPU path                   */
#define GW_E_DEVICE       -3  /* HIP runtime error                                            */
#define GW_E_OOM          -4  /* device or host allocation failed                             */
#define GW_E_OUTPUT_FULL  -5  /* more fired rows pending: call gw_drain again                 */
#define GW_E_NO_TIMESTAMP -6  /* record carries Long.MIN_VALUE (assigners throw RuntimeException) */
#define GW_E_RANGE        -7  /* window bounds overflow int64                                 */
#define GW_E_STATE        -8  /* illegal call sequence / merge into the past                  */

/* ---- configuration ------------------------------------------------------- */
typedef enum gw_assigner {
    GW_TUMBLING = 0, /* TumblingEventTimeWindows.of(size, offset)  (stagger ALIGNED)   */
    GW_SLIDING  = 1, /* SlidingEventTimeWindows.of(size, slide, offset)                */
    GW_SESSION  = 2, /* EventTimeSessionWindows.withGap(gap)                           */
    /* Count windows over GlobalWindows, per key in arrival order;
     * timestamps, watermarks and allowed lateness play no part (GlobalWindows is not an
     * event-time assigner).  A row is (key, first element ordinal, end ordinal, result):
     * the window holds the key's elements [start, end) in arrival order, counted from 0.
     * Rows are produced by gw_ingest* itself (CountTrigger fires on the element). */
    GW_COUNT_TUMBLING = 3, /* KeyedStream.countWindow(size): PurgingTrigger(CountTrigger(size))
                              (RS/api/datastream/KeyedStream.java:676-678)                  */
    GW_COUNT_SLIDING  = 4, /* KeyedStream.countWindow(size, slide): CountEvictor(size) +
                              CountTrigger(slide) (KeyedStream.java:686-690)                */
    /* DynamicEventTimeSessionWindows.withDynamicGap(extractor): element i gets the window
     * [ts[i], ts[i] + gap[i]) from a gap column the caller evaluates the extractor into
     * (gw_ingest_gap*).  gw_config.gap, size and slide are ignored.  Everything else is
     * GW_SESSION: merging, lateness, triggers, the late side output, snapshots (a blob's
     * header carries this assigner and gap 0; its body is the session body). */
    GW_SESSION_DYNAMIC = 5
} gw_assigner;

typedef enum gw_trigger {
    GW_EVENT_TIME_TRIGGER         = 0, /* EventTimeTrigger.create()                   */
    GW_PURGING_EVENT_TIME_TRIGGER = 1  /* PurgingTrigger.of(EventTimeTrigger.create()) */
} gw_trigger;

/* The closed set of aggregate functions of the path.
 * Result column type: int64 for COUNT/SUM_I64/MIN_I64/MAX_I64/SUM_I32 (sign-extended
 * Java int), IEEE double for SUM_F64/MIN_F64/MAX_F64/AVG_I64/AVG_F64. */
typedef enum gw_agg {
    GW_COUNT   = 0, /* AggregateFunction<T, Long, Long> counting records           */
    GW_SUM_I64 = 1, /* WindowedStream.sum on a Long field (Java wrap-around)        */
    GW_SUM_F64 = 2, /* WindowedStream.sum on a Double field                         */
    GW_MIN_I64 = 3, /* WindowedStream.min on a Long field                           */
    GW_MAX_I64 = 4, /* WindowedStream.max on a Long field                           */
    GW_MIN_F64 = 5, /* WindowedStream.min on a Double field (Double.compareTo order) */
    GW_MAX_F64 = 6, /* WindowedStream.max on a Double field                         */
    GW_AVG_I64 = 7, /* AverageAggregate: acc (long sum, long count) -> (double)sum/count */
    GW_AVG_F64 = 8, /* acc (double sum, long count) -> sum/count                    */
    GW_SUM_I32 = 9  /* WindowedStream.sum on an Integer field (int32 wrap-around)   */
} gw_agg;

typedef struct gw_config {
    int32_t assigner;         /* gw_assigner                                          */
    int32_t trigger;          /* gw_trigger                                           */
    int64_t size;             /* tumbling/sliding window size, ms                     */
    int64_t slide;            /* sliding slide, ms (ignored for tumbling)             */
    int64_t offset;           /* window offset, ms                                    */
    int64_t gap;              /* session gap, ms                                      */
    int64_t allowed_lateness; /* WindowedStream.allowedLateness, ms (>= 0)            */
    int32_t agg;              /* gw_agg                                               */
    int32_t max_parallelism;  /* number of key groups (0 -> 128)                      */
    int32_t parallelism;      /* operator parallelism (0 -> 1)                        */
    int32_t operator_index;   /* this subtask                                         */
    int32_t device;           /* HIP device ordinal                                   */
    int32_t flags;            /* GW_FLAG_*                                            */
    int64_t capacity_hint;    /* expected live keys (sizes the HBM state table)       */
    int64_t max_batch;        /* records per ingest call (sizes staging), 0 -> 1<<20  */
} gw_config;

#define GW_FLAG_FORCE_LDS_PREAGG   1 /* always pre-aggregate in LDS before the HBM RMW  */
#define GW_FLAG_NO_LDS_PREAGG      2 /* never pre-aggregate in LDS                       */
#define GW_FLAG_CHECK_KEY_GROUPS   4 /* reject keys outside this subtask's key groups    */
#define GW_FLAG_FORCE_REGION       8 /* always use the region-bucketed ingest path      */
#define GW_FLAG_NO_REGION         16 /* never use the region-bucketed ingest path       */
#define GW_FLAG_NO_BUFFER         32 /* region path: apply every batch at once instead of
                                        buffering pass-1 segments until the next fire    */
#define GW_FLAG_LATE_SIDE_OUTPUT  64 /* WindowedStream.sideOutputLateData: late records go to
                                        gw_drain_late instead of numLateRecordsDropped    */
#define GW_FLAG_NO_NARROW        256 /* region path: never narrow records (compact or wide only) */
#define GW_FLAG_FIRST_ELEMENT    128 /* positional sum/min/max (WindowedStream.sum(i) etc.):
                                        records carry a 64-bit payload (the tuple's other
                                        fields, packed by the caller) and every row carries the
                                        payload of its window's first element in arrival
                                        order (gw_ingest_payload*, gw_drain_payload);
                                        tumbling / sliding windows with EventTimeTrigger    */
#define GW_FLAG_BY_FIELD       512 /* minBy / maxBy (WindowedStream.minBy(i, first) etc.,
                                        WindowedStream.java:725-771; ComparableAggregator
                                        byAggregate, ComparableAggregator.java:88-95): with
                                        GW_MIN_* / GW_MAX_*, every row carries the payload of
                                        the window's element whose field is the minimum /
                                        maximum, the first of equal ones in arrival order
                                        (implies GW_FLAG_FIRST_ELEMENT's payload ingest/drain) */
#define GW_FLAG_BY_LAST       1024 /* with GW_FLAG_BY_FIELD: the last of equal ones
                                        (minBy(i, false)); needs allowed lateness 0         */

typedef struct gw_handle gw_handle;

/* Per-operator counters (Flink: numRecordsIn, numLateRecordsDropped, numFiredTimers). */
typedef struct gw_stats {
    int64_t events_in;        /* records handed to gw_ingest*                      */
    int64_t late_dropped;     /* numLateRecordsDropped                             */
    int64_t rows_fired;       /* fired (key, window) rows so far                   */
    int64_t live_keys;        /* occupied state-table slots                        */
    int64_t table_capacity;   /* state-table slots                                 */
    int64_t table_bytes;      /* HBM bytes of the state table                      */
    int64_t deferred;         /* partial aggregates parked outside the pane ring   */
    int64_t batches;          /* ingest calls                                      */
    int64_t fires;            /* fire passes launched                              */
    int64_t rehashes;         /* table growths                                     */
    int64_t preagg_batches;   /* batches that used the LDS pre-aggregation kernel  */
    int64_t session_merges;   /* sessions merged away (M_b)                        */
    int64_t applies;          /* region pass-2 + apply launches (buffer flushes)   */
    int64_t region_format;    /* record format of the last region flush window: 0 wide,
                                 1 compact (hash word + 32-bit value), 2 narrow (32-bit
                                 key + 28-bit value; 4 B for COUNT); -1 none yet       */
    int64_t session_punted;   /* session records whose key found no free slot in the main
                                 table: replayed after the table grew                    */
    int64_t session_slow;     /* reserved (0): the removed bucketed session ingest's
                                 general-path count                                      */
} gw_stats;

/* ---- lifecycle ------------------------------------------------------------ */
int  gw_create(const gw_config* cfg, gw_handle** out);
int  gw_destroy(gw_handle* h);
/* Last error text of h (or of the last failed gw_create when h == NULL). */
const char* gw_last_error(const gw_handle* h);
int  gw_abi_version(void);

/* ---- data path ------------------------------------------------------------ */
/* Host columns: key[n], ts[n], value[n] (8 bytes each: int64 or IEEE double per agg;
 * value may be NULL for GW_COUNT).  key_hash[n] (Java key.hashCode()) may be NULL:
 * the key group is then computed from Long.hashCode(key).  Buffers are reusable as
 * soon as the call returns.  All records of one call see the same current
 * watermark (the one last passed to gw_advance_watermark), which is exactly what a
 * Flink operator sees for the records between two watermarks. */
int  gw_ingest(gw_handle* h, int64_t n, const int64_t* key, const int32_t* key_hash,
               const int64_t* ts, const void* value);
/* Library-owned pinned column slots for callers that build a batch in place (the JVM operator
 * writes each record's fields straight into them as direct ByteBuffers, so no copy precedes the
 * PCIe transfer).  gw_stage_alloc: `slots` slots of `cap` records.  gw_stage_columns: slot's
 * key / key_hash / ts / value columns (any pointer may be NULL), once the slot's previous
 * transfer has read it.  gw_ingest_stage: the slot's first n records, as gw_ingest would take
 * them (cols: GW_STAGE_VALUE and / or GW_STAGE_KEY_HASH); the transfer runs on a copy stream
 * into one of three device buffers used in turn, so it overlaps the previous batches' kernels.  The
 * slot may be refilled after the next gw_stage_columns on it returns.  Not for composite or
 * first-element handles (GW_E_UNSUPPORTED). */
#define GW_STAGE_VALUE    1
#define GW_STAGE_KEY_HASH 2
int  gw_stage_alloc(gw_handle* h, int32_t slots, int64_t cap);
int  gw_stage_columns(gw_handle* h, int32_t slot, int64_t** key, int32_t** key_hash, int64_t** ts,
                      int64_t** value);
int  gw_ingest_stage(gw_handle* h, int32_t slot, int64_t n, int32_t cols);
/* Send a filled slot's first n records over PCIe ahead of its gw_ingest_stage (into the next of
 * the three device buffers, once the ingest that last read it is done), e.g. batches b+1 and b+2
 * while batch b is fired and its rows drained.  At most two batches ahead; the gw_ingest_stage
 * calls must name the sent slots, n and cols in the order they were sent (GW_E_STATE otherwise). */
int  gw_stage_send(gw_handle* h, int32_t slot, int64_t n, int32_t cols);
/* Same, with the columns already resident in device memory (d_* are device
 * pointers).  `stream` is the hipStream_t the inputs were produced on (NULL = the
 * default stream).  The handle's stream (gw_stream) reads them after that stream's
 * pending work, and the producer stream is made to wait for those reads, so the caller
 * may reuse or free the columns in stream order on the producer stream (e.g. a PyTorch
 * caching allocator) without further synchronisation. */
int  gw_ingest_device(gw_handle* h, int64_t n, const int64_t* d_key, const int32_t* d_key_hash,
                      const int64_t* d_ts, const void* d_value, void* stream);
/* GW_SESSION_DYNAMIC handles: gw_ingest / gw_ingest_device plus the gap column, gap[i] > 0 the
 * session gap of element i in ms (SessionWindowTimeGapExtractor.extract, evaluated by the
 * caller).  A gap <= 0 fails the operator with GW_E_INVALID ("Dynamic session time gap must
 * satisfy 0 < gap", DynamicEventTimeSessionWindows.assignWindows), ts + gap beyond int64 with
 * GW_E_RANGE; like a Long.MIN_VALUE timestamp, either may surface at the next call on the
 * handle, and every later call returns GW_E_STATE.  GW_E_INVALID: these calls on any other
 * handle, gw_ingest / gw_ingest_device on a dynamic handle, a NULL gap column with n > 0.
 * Not on a dynamic handle (GW_E_UNSUPPORTED): gw_stage_alloc (callers keep their own buffers
 * and use these calls), gw_ingest_serialized*, gw_ingest_packed_device, gw_top_n_rows. */
int  gw_ingest_gap(gw_handle* h, int64_t n, const int64_t* key, const int32_t* key_hash,
                   const int64_t* ts, const void* value, const int64_t* gap);
int  gw_ingest_gap_device(gw_handle* h, int64_t n, const int64_t* d_key, const int32_t* d_key_hash,
                          const int64_t* d_ts, const void* d_value, const int64_t* d_gap, void* stream);
/* Advance event time to wm: fire every window whose maxTimestamp (end-1) <= wm,
 * purge its state, and append the fired rows to the output.  *rows_fired (may be
 * NULL) receives the number of rows this call produced.  Watermarks that do not
 * advance are ignored, as in InternalTimerServiceImpl.tryAdvanceWatermark. */
int  gw_advance_watermark(gw_handle* h, int64_t wm, int64_t* rows_fired);
/* Apply every buffered record to the window state now.  The region path buffers
 * pass-1 segments of several watermark batches and applies them before the next fire
 * by itself; gw_flush makes the state exact at any point, as a snapshot needs
 * (StreamOperator.prepareSnapshotPreBarrier, RS/api/operators/StreamOperator.java:122). */
int  gw_flush(gw_handle* h);
/* ---- checkpoint / restore ------------------------------------------------ */
/* Snapshot of the window state of key groups [kg_lo, kg_hi] (buffered records are
 * applied first).  Replaces the keyed-state part of StreamOperator.snapshotState
 * (RS/api/operators/StreamOperator.java:131) in the heap backend's per-key-group layout
 * (HeapSnapshotStrategy.java:97-154).  The blob is a 96-byte header (magic "GWS1",
 * version, window, aggregate, max parallelism, key-group range, flags), int64
 * kg_offsets[kg_hi - kg_lo + 2], then per key group:
 *   version 4 (tumbling / sliding windows, also under allowed lateness and PurgingTrigger;
 *   big-endian like DataOutputView): be32 n + n "window-contents" entries
 *   (window.start, window.end, key, [be32 key hash,] state) as
 *   CopyOnWriteStateMapSnapshot.writeState writes them (:127-149; one entry per (key,
 *   window) holding state: not fired, or fired and kept until its cleanup time), be32 0
 *   (no merging window set), be32 t + t event-time timers (flipSignBit(ts), key, start,
 *   end) as TimerSerializer.serialize writes them (:147-152; the window's maxTimestamp
 *   and, under lateness, its cleanup time);
 *   version 4 (session windows): the same three sections -- be32 n + n "window-contents"
 *   entries (state window, key, [be32 key hash,] state) of the sessions holding state (a
 *   session fired under PurgingTrigger holds none), be32 m + m "merging-window-set" records
 *   (key, [be32 key hash,] be32 c, c x (window, state window)) as MergingWindowSet.persist
 *   writes its ListState (:99-106), be32 t + t timers (maxTimestamp while a session has not
 *   fired; its cleanup time under allowed lateness).  libgpuwin names each session as its own
 *   state window; a restore takes any state window the set names (the reference keeps a
 *   merged session's state under one of its original windows, MergingWindowSet.java:188-201);
 *   version 3 (count windows): per key (key, element count, ring of count-pane
 *   accumulators): the CountTrigger count and the evicting operator's window contents.
 * Keys fed with a key_hash column (String, Integer, ... keys as caller ids) are filed
 * under the key group of that hash (KeyGroupRangeAssignment.java:63-66), and the blob
 * carries each entry's key hash (header flags bit 0: a be32 after the key of every
 * version-4 entry and merging-window-set record, one more int64 word per entry in version 3).  A window-class composite writes
 * its classes' entries merged per key group.  Two calls: buf == NULL returns the size in
 * *len; then a buffer of cap >= *len. */
int  gw_snapshot(gw_handle* h, int32_t kg_lo, int32_t kg_hi, void* buf, int64_t cap, int64_t* len);
/* Restore one snapshot blob (call once per key-group range, e.g. after rescaling) into a
 * handle with the same assigner, aggregate and max parallelism
 * (StreamOperator.initializeState, StreamOperator.java:139).  The watermark is not part
 * of the state: like Flink after a restore it starts at Long.MIN_VALUE. */
int  gw_restore(gw_handle* h, const void* buf, int64_t len);

/* The part of a gw_snapshot blob that belongs to key group kg, as a blob of its own (what
 * GpuWindowOperator writes per key group into the raw keyed state stream, like the heap
 * backend's per-key-group write, HeapSnapshotStrategy.java:97-154).  Pure host code; any
 * blob version.  Two calls as gw_snapshot: out == NULL returns the size in *out_len.
 * GW_E_INVALID for a corrupt blob or kg outside its key-group range (gw_last_error(NULL)). */
int  gw_snapshot_slice(const void* blob, int64_t len, int32_t kg, void* out, int64_t cap, int64_t* out_len);

/* The distinct keys a blob's entries and timers name, ascending, into keys[cap]; *n gets
 * their number (keys == NULL: only the count).  With gw_snapshot_remap_keys this is what a
 * caller that maps its keys to int64 ids (GpuWindowOperator<IN, K> for non-Long K) needs
 * to write the real keys beside the blob (through the key serializer) and to restore them
 * under the ids of another process.  Pure host code; GW_E_INVALID for a corrupt blob. */
int  gw_snapshot_keys(const void* blob, int64_t len, int64_t* keys, int64_t cap, int64_t* n);
/* Rewrite in place every key of the blob found in from[0..n) (ascending) to the matching
 * to[i]; key hashes stay.  GW_E_INVALID for a corrupt blob or unsorted from[]. */
int  gw_snapshot_remap_keys(void* blob, int64_t len, const int64_t* from, const int64_t* to, int64_t n);
/* First-element handles (GW_FLAG_FIRST_ELEMENT): their blob's version-4 entries end with the
 * be64 payload of the window's first element (header flags bit 1).  gw_snapshot_payloads
 * lists the distinct payloads ascending (payloads == NULL: only the count) and the latest
 * window end among the entries -- what the caller needs to write the elements beside the
 * blob and to keep them after a restore until those windows are cleaned;
 * gw_snapshot_remap_payloads rewrites them to a restoring process's own ids. */
int  gw_snapshot_payloads(const void* blob, int64_t len, int64_t* payloads, int64_t cap, int64_t* n,
                          int64_t* max_window_end);
int  gw_snapshot_remap_payloads(void* blob, int64_t len, const int64_t* from, const int64_t* to, int64_t n);

/* ---- network-buffer ingest ----------------------------- */
/* Layout of the record value: a Flink Tuple of fixed-width fields as TupleSerializer
 * writes them (fields in order, no null markers; flink-core/.../api/java/typeutils/
 * runtime/TupleSerializer.java:139-145), each field big-endian as DataOutputView
 * writes it (LongSerializer.serialize = writeLong, DoubleSerializer = writeDouble,
 * IntSerializer = writeInt, ...).  Type codes are JVM descriptors:
 *   'J' long, 'D' double, 'I' int, 'F' float, 'S' short, 'B' byte, 'Z' boolean. */
#define GW_MAX_FIELDS 8
typedef struct gw_record_layout {
    int32_t nfields;               /* fields of the Tuple (1..GW_MAX_FIELDS)             */
    int32_t key_field;             /* index of the Long key field (keyBy(t -> t.fN))     */
    int32_t value_field;           /* index of the aggregated field; -1 for GW_COUNT     */
    char    types[GW_MAX_FIELDS];  /* type code per field                                */
} gw_record_layout;

/* Result of decoding one input channel's bytes. */
typedef struct gw_decode_result {
    int64_t records;    /* StreamRecords decoded (columns written)                         */
    int64_t watermarks; /* Watermark elements (wm_pos/wm_val written)                      */
    int64_t consumed;   /* bytes up to the end of the last complete element; the caller
                           keeps the rest and prepends it to the next call (a record
                           spanning network buffers, SpanningWrapper)                      */
    int64_t skipped;    /* latency markers, stream status and record attributes            */
} gw_decode_result;

/* Decode the serialized stream elements of one input channel on the device.  The bytes
 * are the concatenated payloads of the channel's network buffers: per element a 4-byte
 * big-endian length, then StreamElementSerializer's tag and body
 * (RecordWriter.serializeRecord, flink-runtime/.../io/network/api/writer/
 * RecordWriter.java:144-156; StreamElementSerializer.serialize/deserialize,
 * RS/runtime/streamrecord/StreamElementSerializer.java:163-225).  Records go to the
 * columns (key, timestamp, value as 8-byte int64 / IEEE double bits; a record without
 * timestamp gets Long.MIN_VALUE), watermarks to (wm_pos = number of records before it,
 * wm_val).  Elements are at most GW_MAX_ELEMENT bytes long including the length word.
 * Synchronous; allocates its own scratch.  GW_E_INVALID on a corrupt stream ("Corrupt
 * stream, found tag"), GW_E_OUTPUT_FULL if rec_cap / wm_cap are too small. */
#define GW_MAX_ELEMENT 128
int  gw_decode_serialized(const void* d_bytes, int64_t nbytes, const gw_record_layout* layout,
                          int64_t* d_key, int64_t* d_ts, int64_t* d_value, int64_t rec_cap,
                          int64_t* d_wm_pos, int64_t* d_wm_val, int64_t wm_cap,
                          gw_decode_result* out, void* stream);
/* Decode and process one input channel's bytes on the operator: the records between
 * two watermarks go through gw_ingest, each watermark through gw_advance_watermark —
 * what StreamTaskNetworkInput.processElement does per element (RS/runtime/io/
 * AbstractStreamTaskNetworkInput.java:152-175, processElement :205-230) with a single
 * input channel's StatusWatermarkValve.  *consumed (may be NULL) as in
 * gw_decode_result; *rows_fired (may be NULL) counts the rows the watermarks fired.
 * One host synchronisation per call (the watermark positions): pass many buffers at
 * once. */
int  gw_ingest_serialized(gw_handle* h, const void* bytes, int64_t nbytes, const gw_record_layout* layout,
                          int64_t* consumed, int64_t* rows_fired);
/* Same, with the bytes in device memory, produced on `stream` (NULL = default stream). */
int  gw_ingest_serialized_device(gw_handle* h, const void* d_bytes, int64_t nbytes,
                                 const gw_record_layout* layout, void* stream, int64_t* consumed,
                                 int64_t* rows_fired);

/* ---- several input channels ---------------------------------------------------
 * An operator behind a keyBy reads one input channel per upstream subtask and acts on the
 * output of StatusWatermarkValve: the minimum watermark over the channels that are active
 * and aligned.  gw_valve is that valve by itself (host code, no device); a handle with
 * gw_set_input_channels owns one and gw_ingest_channels* feeds it. */
#define GW_EVENT_WATERMARK 0   /* value: the watermark's timestamp                        */
#define GW_EVENT_STATUS    1   /* value: GW_STATUS_ACTIVE / GW_STATUS_IDLE (WatermarkStatus) */
#define GW_STATUS_ACTIVE   0
#define GW_STATUS_IDLE   (-1)
#define GW_MAX_INPUT_CHANNELS 1024
typedef struct gw_valve gw_valve;
typedef struct gw_valve_output {
    int32_t has_watermark;  /* the input emitted a watermark (before the status, if both)  */
    int32_t has_status;     /* the input emitted a status                                  */
    int64_t watermark;
    int32_t status;         /* GW_STATUS_ACTIVE / GW_STATUS_IDLE                           */
    int32_t reserved;
} gw_valve_output;
/* 1 <= nchannels <= GW_MAX_INPUT_CHANNELS.  Every channel starts active and aligned at
 * Long.MIN_VALUE, the valve's output at Long.MIN_VALUE and ACTIVE. */
int  gw_valve_create(int32_t nchannels, gw_valve** out);
int  gw_valve_destroy(gw_valve* v);
/* One watermark or status of `channel`; *out what it emitted (at most one watermark and one
 * status).  A watermark is ignored unless the valve's output and the channel are active and
 * it advances the channel; an idle channel leaves the minimum, and comes back aligned only
 * once its watermark has caught up with the output; when the last active channel goes idle
 * the valve flushes the maximum over all channels (if that channel was holding it back) and
 * emits IDLE.  GW_E_INVALID: channel outside [0, n), unknown kind, a status other than
 * GW_STATUS_ACTIVE / GW_STATUS_IDLE. */
int  gw_valve_input(gw_valve* v, int32_t channel, int32_t kind, int64_t value, gw_valve_output* out);

/* Result of gw_decode_channels_device. */
typedef struct gw_decode_channels_result {
    int64_t records;      /* over all ranges                                               */
    int64_t events;       /* watermarks and watermark statuses over all ranges             */
    int64_t skipped;      /* latency markers and record attributes                         */
    int32_t error_range;  /* the range of the reported error, -1 if none                   */
    int32_t reserved;
    int64_t error_pos;    /* its byte position in that range (chunk-granular for a bad tag) */
} gw_decode_channels_result;
/* gw_decode_serialized for nranges byte ranges at once (one per input channel, for example):
 * one pipeline run whose kernel launches and single host synchronisation do not depend on
 * nranges.  d_ptr[r] (host array of device pointers, 4-byte aligned, separate allocations
 * allowed) and len[r] >= 0 give range r.  Every range is a stream of its own: its chain
 * starts at its first byte, nothing past its end is read, and it may end inside an element
 * (consumed[r] = end of its last complete element).  Records go to the columns in range
 * order and stream order within a range, rec_count[r] of them; watermarks (kind
 * GW_EVENT_WATERMARK) and WatermarkStatus elements (GW_EVENT_STATUS, value as written) to
 * (ev_pos = records of the whole call before the event, ev_kind, ev_val), ev_count[r] of
 * them.  consumed, rec_count, ev_count: host arrays of nranges (each may be NULL).  Errors
 * as gw_decode_serialized; the earliest in (range, byte position) is reported and
 * gw_last_error(NULL) names the range. */
int  gw_decode_channels_device(int32_t nranges, const void* const* d_ptr, const int64_t* len,
                               const gw_record_layout* layout, int64_t* d_key, int64_t* d_ts,
                               int64_t* d_value, int64_t rec_cap, int64_t* d_ev_pos, int32_t* d_ev_kind,
                               int64_t* d_ev_val, int64_t ev_cap, int64_t* consumed, int64_t* rec_count,
                               int64_t* ev_count, gw_decode_channels_result* out, void* stream);

/* The handle reads n input channels (1..GW_MAX_INPUT_CHANNELS) through a valve of its own;
 * calling it again resets the valve.  From then on gw_ingest_serialized* returns
 * GW_E_INVALID on this handle: its single-channel valve would bypass this one. */
int  gw_set_input_channels(gw_handle* h, int32_t n);
/* Decode and process the bytes of several input channels: range r holds bytes of channel
 * channel[r] (each channel at most once per call, in [0, n)).  The elements are processed as
 * if the ranges had arrived in array order: one segmented decode, the watermarks and statuses
 * go through the handle's valve on the host, the records between two watermarks the valve
 * emits go through gw_ingest_device's path as one batch, each emitted watermark through
 * gw_advance_watermark's.  Records are never filtered by status.  consumed[r] (may be NULL)
 * as in gw_decode_result: the caller keeps each channel's tail.  One host synchronisation
 * per call.  A window-class composite decodes once for all its children.  First-element and
 * GW_SESSION_DYNAMIC handles: GW_E_UNSUPPORTED.  A corrupt stream fails the operator. */
int  gw_ingest_channels_device(gw_handle* h, int32_t nranges, const int32_t* channel, const void* const* d_ptr,
                               const int64_t* len, const gw_record_layout* layout, void* stream,
                               int64_t* consumed, int64_t* rows_fired);
/* Same with the bytes in host memory: the ranges are staged into one pinned buffer at
 * aligned offsets and copied to the device at once. */
int  gw_ingest_channels(gw_handle* h, int32_t nranges, const int32_t* channel, const void* const* ptr,
                        const int64_t* len, const gw_record_layout* layout, int64_t* consumed,
                        int64_t* rows_fired);
/* The valve's last output: the watermark it emitted last (Long.MIN_VALUE before the first)
 * and whether its status is idle -- what the operator forwards downstream.  gw_restore
 * resets the valve: like the watermark it is not part of the state. */
int  gw_input_status(gw_handle* h, int64_t* watermark, int32_t* idle);

/* Bounded input ended (BoundedOneInput.endInput) — equivalent to MAX_WATERMARK. */
int  gw_end_input(gw_handle* h, int64_t* rows_fired);

/* ---- output ---------------------------------------------------------------- */
int  gw_pending_rows(gw_handle* h, int64_t* n);
/* Copy up to cap pending rows (key, window start, window end, result) to host
 * arrays and remove them.  Returns GW_E_OUTPUT_FULL if rows remain. */
/* GW_FLAG_FIRST_ELEMENT handles: the batch with each record's payload (SumAggregator /
 * ComparableAggregator keep the first element's other fields, RS/api/functions/aggregation/
 * SumAggregator.java:66-76, ComparableAggregator.java:83-104), and rows with the payload of
 * their window's first element.  gw_ingest / gw_ingest_device return GW_E_INVALID on such
 * handles; gw_drain drains the rows without the payload. */
int  gw_ingest_payload(gw_handle* h, int64_t n, const int64_t* key, const int32_t* key_hash, const int64_t* ts,
                       const void* value, const int64_t* payload);
int  gw_ingest_payload_device(gw_handle* h, int64_t n, const int64_t* d_key, const int32_t* d_key_hash,
                              const int64_t* d_ts, const void* d_value, const int64_t* d_payload, void* stream);
int  gw_drain_payload(gw_handle* h, int64_t* key, int64_t* start, int64_t* end, void* result, int64_t* payload,
                      int64_t cap, int64_t* n);
int  gw_drain(gw_handle* h, int64_t* key, int64_t* start, int64_t* end, void* result,
              int64_t cap, int64_t* n);
/* Zero-copy device view of the pending rows (for a device-side consumer). */
int  gw_rows_device(gw_handle* h, const int64_t** d_key, const int64_t** d_start,
                    const int64_t** d_end, const void** d_result, int64_t* n);
/* Drop all pending rows (after a device consumer read them). */
int  gw_clear_rows(gw_handle* h);

/* ---- per-window top-N over fired rows ----------------------------------------
 * The non-keyed stage that follows the keyed window aggregate in Nexmark Q5 ("hot items": per
 * window, the auctions with the highest count) and Q7 (per-window maximum): in Flink a
 * windowAll(...).maxBy(...) or a top-N process function over the keyed stage's output.  Run on
 * the device it leaves `top` rows per window to bring to the host instead of one per live key.
 *
 * Input: n rows in the columns key, start, end (int64) and result (8 bytes), in any order, rows
 * of different windows interleaved.  A window is identified by its end; every row with the same
 * end must carry the same start (GW_E_INVALID otherwise), which holds for the rows of any
 * tumbling or sliding handle, window classes included (the size is fixed).
 * Order of result: signed int64; with GW_TOPN_F64 that of Double.compare (-0.0 < 0.0, every NaN
 * equal to every other and greater than +inf).  The best rows are the largest, with
 * GW_TOPN_SMALLEST the smallest.  Among equal results the smaller key (signed) wins: Flink's
 * maxBy keeps the first of equal elements in arrival order, but behind a parallel upstream that
 * order is undefined, so the key decides and the answer is reproducible.
 * Output: windows in ascending end, within a window up to `top` rows, best first, as key, start,
 * end, result and (win_rows, may be NULL) the number of input rows of the row's window;
 * *n_out = the sum over windows of min(top, rows of the window).  result bits come back as
 * they went in, except that a NaN may come back as the canonical NaN.
 * Limits: 1 <= top <= GW_TOPN_MAX_N (GW_E_INVALID); at most GW_TOPN_MAX_WINDOWS distinct ends
 * per call (GW_E_UNSUPPORTED); outputs of cap < *n_out rows: GW_E_OUTPUT_FULL with the needed
 * number in *n_out.  n = 0: GW_OK and no rows.
 *
 * gw_top_n_device: stateless, device columns in and out; waits on `stream` (the result size is
 * known only then), using scratch of its own per device.  Errors: gw_last_error of NULL.
 * gw_top_n_rows: over the handle's pending rows (the view gw_rows_device gives: plain,
 * window-class, first-element and minBy handles) on the handle's stream, into host arrays.
 * GW_TOPN_F64 follows from the handle's aggregate; mode carries GW_TOPN_SMALLEST only.  The rows
 * stay pending: follow it with gw_clear_rows or gw_drain.  It ranks whatever is pending: under
 * allowed lateness that may include the re-fired rows of a window next to its earlier ones
 * (drain or clear at every watermark to rank one firing at a time).  Session and count-window
 * handles: GW_E_UNSUPPORTED (their windows are per key).
 * gw_top_n_host: the same contract as pure host code (no device, no handle): how a job at
 * parallelism > 1 combines its subtasks' lists.  Key groups partition the keys over the
 * subtasks, so the top-N of the concatenated per-subtask top-Ns is the global top-N, and
 * top x windows rows per subtask need no collective of their own. */
#define GW_TOPN_MAX_N       64
#define GW_TOPN_MAX_WINDOWS 1024
#define GW_TOPN_SMALLEST    1
#define GW_TOPN_F64         2
int  gw_top_n_device(int64_t n, const int64_t* d_key, const int64_t* d_start, const int64_t* d_end,
                     const void* d_result, int32_t top, int32_t mode, int64_t* d_key_out, int64_t* d_start_out,
                     int64_t* d_end_out, void* d_result_out, int64_t* d_win_rows_out, int64_t cap, int64_t* n_out,
                     void* stream);
int  gw_top_n_rows(gw_handle* h, int32_t top, int32_t mode, int64_t* key, int64_t* start, int64_t* end,
                   void* result, int64_t* win_rows, int64_t cap, int64_t* n);
int  gw_top_n_host(int64_t n, const int64_t* key, const int64_t* start, const int64_t* end, const void* result,
                   int32_t top, int32_t mode, int64_t* key_out, int64_t* start_out, int64_t* end_out,
                   void* result_out, int64_t* win_rows_out, int64_t cap, int64_t* n_out);

/* ---- event-time window join of two keyed streams ---------------------------------
 * stream.join(other).where(k1).equalTo(k2).window(assigner).apply(JoinFunction): JoinedStreams /
 * CoGroupedStreams (RS/api/datastream/JoinedStreams.java, CoGroupedStreams.java), Nexmark Q8.
 * Flink tags and unions both inputs, keys the union and runs the same WindowOperator with
 * ListState; at the fire JoinCoGroupFunction.coGroup emits the cross product of the two sides'
 * elements per (key, window) (JoinedStreams.java, JoinCoGroupFunction).
 *
 * Records: side L (0) or R (1), (key, ts, payload) int64 columns; payload is the element as the
 * caller packs or numbers it.  Assigners: tumbling (slide = size) and sliding, size > 0,
 * slide > 0, |offset| < slide (GW_E_INVALID otherwise).  A record's windows are those of
 * SlidingEventTimeWindows.assignWindows (:75-90): lastStart = TimeWindow.getWindowStartWithOffset
 * (ts, offset, slide) (TimeWindow.java:264-272), starts lastStart - k * slide for k >= 0 while
 * start > ts - size.  ts = Long.MIN_VALUE: GW_E_NO_TIMESTAMP; a window bound (or a step of the
 * arithmetic) beyond int64: GW_E_RANGE; more than GW_JOIN_MAX_WINDOWS windows per record
 * (ceil(size / slide)): GW_E_UNSUPPORTED.
 * Firing: EventTimeTrigger, allowed lateness 0.  The watermark going from w0 to w1 > w0 fires the
 * windows with w0 < end - 1 <= w1, each with the records ingested so far whose window set contains
 * it.  A record ingested at watermark w is late when lastStart + size - 1 <= w (all its windows
 * have passed): dropped and counted (numLateRecordsDropped, WindowOperator.java:440-446; with
 * size < slide a record between two windows falls under the same test, where Flink tests its
 * timestamp).  A record that is not late but has windows that passed never shows up in those.  A
 * watermark that does not advance is ignored; end of input is Long.MAX_VALUE.
 * Output of a fire: for every fired (window, key) with L >= 1 left and R >= 1 right records the
 * L * R pairs (key, start, end, left payload, right payload); an inner join.  Order: windows by
 * ascending end, within a window keys ascending (signed), within a (window, key) left-major, each
 * side in arrival order (ingest call, then index): JoinCoGroupFunction.coGroup's nested loop.
 * The emitted element's timestamp is end - 1, which gw_encode_rows_* writes: the five columns
 * are the (key, start, end, 8 bytes, payload) columns it takes.
 * Not offered: allowed lateness > 0, PurgingTrigger and evictors, session and count windows
 * (GW_E_UNSUPPORTED at create), snapshots, key_hash columns, the RCCL exchange (partition the
 * inputs with gw_partition_device), network-buffer ingest, null fields in gw_encode_rows_*.
 *
 * coGroup and outer joins.  CoGroupedStreams is the primitive under the join: at the fire
 * CoGroupFunction.coGroup sees every (key, window) with a record on either side, one Iterable
 * possibly empty, and every outer window join is written as one.  Two forms:
 * - the outer modes, the closed set of CoGroupFunctions that run wholly on the device.  A fired
 *   (window, key) group with L left and R right records gives L * R rows when both are positive,
 *   L rows when R = 0 and the mode has bit 0 (GW_JOIN_MODE_LEFT_OUTER), R rows when L = 0 and the
 *   mode has bit 1 (GW_JOIN_MODE_RIGHT_OUTER), otherwise none.  An unmatched row carries its own
 *   side's payload and the caller's null_payload in the lacking side's column, so the five columns
 *   feed gw_encode_rows_* as they are and the caller chooses its id for null.  The optional sixth
 *   column `present` (one byte per row; may be NULL) is 1 = left only, 2 = right only, 3 = both,
 *   whatever the payloads are.  Order as above; a group's unmatched rows in arrival order.
 *   GW_JOIN_MODE_INNER gives exactly the rows of the inner join, `present` all 3.
 * - the groups themselves as a CSR: per fired group (key, start, end) and offsets loff, roff (one
 *   entry more than groups, loff[0] = roff[0] = 0) into two element columns: group g's left
 *   payloads are lelem[loff[g] .. loff[g + 1]) in arrival order, likewise right.  Groups in the
 *   order above.
 *
 * gw_window_join_outer_device / _host: gw_window_join_device / _host with a mode, null_payload
 * and d_present_out (cap bytes, or NULL).  A call with one empty side is not empty: with n_l = 0,
 * right and full outer emit every fired right record, and the other way round; both empty: GW_OK,
 * no rows.  cap too small: GW_E_OUTPUT_FULL, the needed number in *n_out, nothing written.  More
 * than INT64_MAX / 41 rows: GW_E_RANGE.  An unknown mode: GW_E_INVALID.  _device_timed: as
 * gw_window_join_device_timed.
 * gw_window_cogroup_device / _host: the CSR of the interval's groups.  d_key_out, d_start_out,
 * d_end_out: cap_groups rows; d_loff_out, d_roff_out: cap_groups + 1 rows (never NULL); the
 * element columns cap_left and cap_right rows.  n_out: int64[3] = groups, left elements, right
 * elements.  Any of the three caps too small: GW_E_OUTPUT_FULL, all three needed numbers in n_out,
 * nothing written.  Limits and errors as the join's.  _device_timed also reports the time of the
 * two kernels that write the CSR (*write_ms), for measurements.
 *
 * gw_window_join_device: stateless; n_l left and n_r right records in arrival order in device
 * columns, the geometry and the interval (w0, w1]; the pairs of the windows firing in it, in the
 * order above, to five device columns of cap rows.  cap < the number of pairs: GW_E_OUTPUT_FULL,
 * the needed number in *n_out, nothing written.  n_l = 0 or n_r = 0: GW_OK, no pairs.  At most
 * 2^30 - 1 (record, fired window) tuples per call (GW_E_UNSUPPORTED); more than INT64_MAX / 40
 * pairs: GW_E_RANGE.  Waits on `stream` (the host reads the tuple count and the pair count), using
 * scratch of its own per device.  Errors: gw_last_error of NULL.
 * gw_window_join_host: the same contract as plain host code over host arrays, no device: for a
 * fire of a few records, or a process without a GPU.
 * gw_window_join_device_timed: gw_window_join_device that also reports the time of its expand
 * kernel between two HIP events (*expand_ms; 0 when no pair fired), for measurements.
 *
 * gw_join: the operator.  One append-only device log per side; gw_join_ingest* drops and counts
 * the late records on the device and appends the rest (the log grows as needed).  gw_join_ingest_device
 * orders itself with `stream` as gw_ingest_device does.  gw_join_advance_watermark fires
 * (previous watermark, watermark] over the two logs, appends the pairs to the pending output
 * (*pairs_fired, may be NULL: their number) and drops the records whose last window has fired.
 * Pairs of several watermarks accumulate until drained or cleared: gw_join_drain copies up to cap
 * and removes them (GW_E_OUTPUT_FULL while pairs remain), gw_join_rows_device is the zero-copy
 * view, gw_join_clear_rows drops them.  After GW_E_NO_TIMESTAMP, GW_E_RANGE or a device error
 * every call returns GW_E_STATE.  max_batch: records per device pass of an ingest (0: 2^22);
 * capacity_hint: initial log rows per side.
 * gw_join_set_mode: an outer mode (with its null_payload) or GW_JOIN_MODE_COGROUP for the handle;
 * only before the first ingest or watermark (GW_E_STATE afterwards, the handle goes on as it was);
 * the default is inner.  Late filtering, log growth and log compaction do not depend on the mode.
 * Outer modes: gw_join_advance_watermark appends the mode's rows and *pairs_fired counts them;
 * gw_join_drain and gw_join_rows_device give the five columns, gw_join_drain_outer and
 * gw_join_rows_device_outer add `present` (may be NULL).  coGroup mode: a fire appends its groups
 * and elements to the pending CSR, the offsets rebased by the pending totals, so several
 * watermarks accumulate into one valid CSR; *pairs_fired is the number of groups.
 * gw_join_cogroup_pending: n[3] = pending groups, left and right elements.  gw_join_cogroup_drain
 * copies everything and removes it, all or nothing: GW_E_OUTPUT_FULL with the needed numbers in
 * n[3] otherwise (loff, roff: cap_groups + 1 rows).  gw_join_cogroup_rows_device: the zero-copy
 * view (NULL for an empty column).  gw_join_clear_rows clears either form.  The pair accessors
 * (gw_join_pending, _drain*, _rows_device*) return GW_E_INVALID on a coGroup handle and the
 * coGroup accessors on any other. */
#define GW_JOIN_MAX_WINDOWS 64
#define GW_JOIN_LEFT  0
#define GW_JOIN_RIGHT 1
#define GW_JOIN_MODE_INNER       0
#define GW_JOIN_MODE_LEFT_OUTER  1   /* bit 0: keep left records without a partner  */
#define GW_JOIN_MODE_RIGHT_OUTER 2   /* bit 1: keep right records without a partner */
#define GW_JOIN_MODE_FULL_OUTER  3
#define GW_JOIN_MODE_COGROUP     4   /* gw_join_set_mode only: the groups as a CSR   */
int  gw_window_join_device(int64_t n_l, const int64_t* d_lkey, const int64_t* d_lts, const int64_t* d_lpay,
                           int64_t n_r, const int64_t* d_rkey, const int64_t* d_rts, const int64_t* d_rpay,
                           int64_t size, int64_t slide, int64_t offset, int64_t w0, int64_t w1,
                           int64_t* d_key_out, int64_t* d_start_out, int64_t* d_end_out, int64_t* d_lpay_out,
                           int64_t* d_rpay_out, int64_t cap, int64_t* n_out, void* stream);
int  gw_window_join_device_timed(int64_t n_l, const int64_t* d_lkey, const int64_t* d_lts, const int64_t* d_lpay,
                                 int64_t n_r, const int64_t* d_rkey, const int64_t* d_rts, const int64_t* d_rpay,
                                 int64_t size, int64_t slide, int64_t offset, int64_t w0, int64_t w1,
                                 int64_t* d_key_out, int64_t* d_start_out, int64_t* d_end_out, int64_t* d_lpay_out,
                                 int64_t* d_rpay_out, int64_t cap, int64_t* n_out, void* stream, double* expand_ms);
int  gw_window_join_host(int64_t n_l, const int64_t* lkey, const int64_t* lts, const int64_t* lpay, int64_t n_r,
                         const int64_t* rkey, const int64_t* rts, const int64_t* rpay, int64_t size, int64_t slide,
                         int64_t offset, int64_t w0, int64_t w1, int64_t* key_out, int64_t* start_out,
                         int64_t* end_out, int64_t* lpay_out, int64_t* rpay_out, int64_t cap, int64_t* n_out);
int  gw_window_join_outer_device(int64_t n_l, const int64_t* d_lkey, const int64_t* d_lts, const int64_t* d_lpay,
                                 int64_t n_r, const int64_t* d_rkey, const int64_t* d_rts, const int64_t* d_rpay,
                                 int64_t size, int64_t slide, int64_t offset, int64_t w0, int64_t w1, int32_t mode,
                                 int64_t null_payload, int64_t* d_key_out, int64_t* d_start_out, int64_t* d_end_out,
                                 int64_t* d_lpay_out, int64_t* d_rpay_out, uint8_t* d_present_out, int64_t cap,
                                 int64_t* n_out, void* stream);
int  gw_window_join_outer_device_timed(int64_t n_l, const int64_t* d_lkey, const int64_t* d_lts, const int64_t* d_lpay,
                                       int64_t n_r, const int64_t* d_rkey, const int64_t* d_rts, const int64_t* d_rpay,
                                       int64_t size, int64_t slide, int64_t offset, int64_t w0, int64_t w1,
                                       int32_t mode, int64_t null_payload, int64_t* d_key_out, int64_t* d_start_out,
                                       int64_t* d_end_out, int64_t* d_lpay_out, int64_t* d_rpay_out,
                                       uint8_t* d_present_out, int64_t cap, int64_t* n_out, void* stream,
                                       double* expand_ms);
int  gw_window_join_outer_host(int64_t n_l, const int64_t* lkey, const int64_t* lts, const int64_t* lpay, int64_t n_r,
                               const int64_t* rkey, const int64_t* rts, const int64_t* rpay, int64_t size,
                               int64_t slide, int64_t offset, int64_t w0, int64_t w1, int32_t mode,
                               int64_t null_payload, int64_t* key_out, int64_t* start_out, int64_t* end_out,
                               int64_t* lpay_out, int64_t* rpay_out, uint8_t* present_out, int64_t cap,
                               int64_t* n_out);
int  gw_window_cogroup_device(int64_t n_l, const int64_t* d_lkey, const int64_t* d_lts, const int64_t* d_lpay,
                              int64_t n_r, const int64_t* d_rkey, const int64_t* d_rts, const int64_t* d_rpay,
                              int64_t size, int64_t slide, int64_t offset, int64_t w0, int64_t w1,
                              int64_t* d_key_out, int64_t* d_start_out, int64_t* d_end_out, int64_t* d_loff_out,
                              int64_t* d_roff_out, int64_t* d_lelem_out, int64_t cap_left, int64_t* d_relem_out,
                              int64_t cap_right, int64_t cap_groups, int64_t* n_out, void* stream);
int  gw_window_cogroup_device_timed(int64_t n_l, const int64_t* d_lkey, const int64_t* d_lts, const int64_t* d_lpay,
                                    int64_t n_r, const int64_t* d_rkey, const int64_t* d_rts, const int64_t* d_rpay,
                                    int64_t size, int64_t slide, int64_t offset, int64_t w0, int64_t w1,
                                    int64_t* d_key_out, int64_t* d_start_out, int64_t* d_end_out, int64_t* d_loff_out,
                                    int64_t* d_roff_out, int64_t* d_lelem_out, int64_t cap_left, int64_t* d_relem_out,
                                    int64_t cap_right, int64_t cap_groups, int64_t* n_out, void* stream,
                                    double* write_ms);
int  gw_window_cogroup_host(int64_t n_l, const int64_t* lkey, const int64_t* lts, const int64_t* lpay, int64_t n_r,
                            const int64_t* rkey, const int64_t* rts, const int64_t* rpay, int64_t size, int64_t slide,
                            int64_t offset, int64_t w0, int64_t w1, int64_t* key_out, int64_t* start_out,
                            int64_t* end_out, int64_t* loff_out, int64_t* roff_out, int64_t* lelem_out,
                            int64_t cap_left, int64_t* relem_out, int64_t cap_right, int64_t cap_groups,
                            int64_t* n_out);

typedef struct gw_join gw_join;
typedef struct gw_join_config {
    int32_t assigner;        /* GW_TUMBLING or GW_SLIDING                         */
    int64_t size;
    int64_t slide;           /* GW_SLIDING only                                   */
    int64_t offset;
    int32_t device;
    int64_t capacity_hint;   /* initial rows of each side's log (0: 16)           */
    int64_t max_batch;       /* records per device pass of an ingest (0: 2^22)    */
} gw_join_config;
typedef struct gw_join_stats {
    int64_t live_left, live_right;                  /* records in the logs        */
    int64_t log_capacity_left, log_capacity_right;  /* rows allocated             */
    int64_t fires;                                  /* watermarks that advanced   */
    int64_t pairs_fired;
    int64_t log_growths;
    int64_t last_fire_tuples;                       /* (record, window) tuples    */
} gw_join_stats;
int  gw_join_create(const gw_join_config* cfg, gw_join** out);
int  gw_join_destroy(gw_join* h);
const char* gw_join_last_error(const gw_join* h);
int  gw_join_ingest(gw_join* h, int32_t side, int64_t n, const int64_t* key, const int64_t* ts,
                    const int64_t* payload);
int  gw_join_ingest_device(gw_join* h, int32_t side, int64_t n, const int64_t* d_key, const int64_t* d_ts,
                           const int64_t* d_payload, void* stream);
int  gw_join_advance_watermark(gw_join* h, int64_t watermark, int64_t* pairs_fired);
int  gw_join_end_input(gw_join* h, int64_t* pairs_fired);
int  gw_join_pending(gw_join* h, int64_t* n);
int  gw_join_drain(gw_join* h, int64_t* key, int64_t* start, int64_t* end, int64_t* lpay, int64_t* rpay,
                   int64_t cap, int64_t* n);
int  gw_join_rows_device(gw_join* h, const int64_t** d_key, const int64_t** d_start, const int64_t** d_end,
                         const int64_t** d_lpay, const int64_t** d_rpay, int64_t* n);
int  gw_join_clear_rows(gw_join* h);
int  gw_join_set_mode(gw_join* h, int32_t mode, int64_t null_payload);
int  gw_join_drain_outer(gw_join* h, int64_t* key, int64_t* start, int64_t* end, int64_t* lpay, int64_t* rpay,
                         uint8_t* present, int64_t cap, int64_t* n);
int  gw_join_rows_device_outer(gw_join* h, const int64_t** d_key, const int64_t** d_start, const int64_t** d_end,
                               const int64_t** d_lpay, const int64_t** d_rpay, const uint8_t** d_present,
                               int64_t* n);
int  gw_join_cogroup_pending(gw_join* h, int64_t* n);
int  gw_join_cogroup_drain(gw_join* h, int64_t* key, int64_t* start, int64_t* end, int64_t* loff, int64_t* roff,
                           int64_t* lelem, int64_t cap_left, int64_t* relem, int64_t cap_right, int64_t cap_groups,
                           int64_t* n);
int  gw_join_cogroup_rows_device(gw_join* h, const int64_t** d_key, const int64_t** d_start, const int64_t** d_end,
                                 const int64_t** d_loff, const int64_t** d_roff, const int64_t** d_lelem,
                                 const int64_t** d_relem, int64_t* n);
int64_t gw_join_late_dropped(const gw_join* h);
int  gw_join_get_stats(const gw_join* h, gw_join_stats* out);
void* gw_join_stream(gw_join* h);

/* ---- event-time interval join of two keyed streams -------------------------------
 * keyedA.intervalJoin(keyedB).between(lower, upper).process(ProcessJoinFunction): KeyedStream
 * .IntervalJoined on IntervalJoinOperator (RS/api/operators/co/IntervalJoinOperator.java), not
 * WindowOperator.  Records are (key, ts, payload) int64 columns per side (GW_JOIN_LEFT /
 * GW_JOIN_RIGHT).  A left l and a right r match when
 *     l.key == r.key  and  l.ts + lower <= r.ts <= l.ts + upper,
 * lower <= upper both inclusive and always relative to the left record (lowerBoundExclusive /
 * upperBoundExclusive are lower + 1 / upper - 1, the caller's arithmetic).  A row is
 * (key, left ts, right ts, left payload, right payload); the element's timestamp is
 * max(left ts, right ts), which the caller derives.
 *
 * One ingest call of side S with n records at the handle's watermark w is n processElementS
 * calls in order: any ts == Long.MIN_VALUE in the call is GW_E_NO_TIMESTAMP (checked over the
 * whole call, before the late test); record i is late when w != Long.MIN_VALUE and ts[i] < w,
 * and is dropped and counted; for every other record ts + lower and ts + upper (left) or
 * ts - upper and ts - lower (right) must fit int64, else GW_E_RANGE (Java wraps silently; this
 * fails instead, as the window join does).  On either error nothing of the call is appended or
 * emitted and every later call on the handle returns GW_E_STATE.  Each record that is not late is
 * appended to its side's buffer and joined against the other side's buffer as it stands: records
 * of one call never pair with each other.  Order of a call's rows: its records in arrival order;
 * within one record its partners by ascending (partner ts, partner arrival), arrival being
 * (ingest call, index).  Flink's inner order is a HashMap's; this is one of its valid orders.  A
 * call longer than max_batch runs in passes and gives the same rows in the same order.
 *
 * A watermark greater than the current one emits nothing and removes the buffered records whose
 * cleanup time is <= it: left ts + upper if upper > 0 else ts; right ts - lower if lower < 0 else
 * ts (onEventTime's two namespaces).  A watermark that does not advance is ignored; the end of
 * input is Long.MAX_VALUE.  So a pair inside the bounds is not emitted when the earlier record
 * was cleaned at exactly the watermark the later one arrives on (ts == w is not late).
 *
 * gw_interval_join_device: stateless; the rows of one ingest call of probe_side (n_p records
 * in device columns) against a buffer of n_b records of the other side given in arrival order.
 * No late filtering; the Long.MIN_VALUE and range checks cover both sides.  cap too small:
 * GW_E_OUTPUT_FULL with the needed number in *n_out and nothing written.  Either side empty:
 * GW_OK and no rows (the other side is not read).  lower > upper or a bound beyond +-2^62:
 * GW_E_INVALID; more than 2^30 - 1 records on a side: GW_E_UNSUPPORTED; more than INT64_MAX / 40
 * rows: GW_E_RANGE.  Waits on `stream`; its scratch is per device and grows as needed.
 * gw_interval_join_device_timed also reports the time of its expand kernel between two HIP
 * events.  gw_interval_join_host: the same contract as plain host code over host arrays.
 *
 * gw_ijoin: the operator.  Each side's records live in a device log kept sorted by (key, ts),
 * equal (key, ts) in arrival order; an ingest sorts its batch, probes the other side's log,
 * expands the rows and merges the batch into its own log (*rows: the rows of this call, may be
 * NULL).  gw_ijoin_ingest_device orders itself with `stream` as gw_join_ingest_device does.  Rows
 * of several calls accumulate until drained or cleared: gw_ijoin_drain copies up to cap and
 * removes them (GW_E_OUTPUT_FULL while rows remain), gw_ijoin_rows_device is the zero-copy view
 * (it waits for the handle's stream, so the rows it shows are written), gw_ijoin_clear_rows
 * drops them.  gw_ijoin_last_times: the device time of the last ingest
 * pass's probe stage (probe, scans, descriptors) and of its merge, in milliseconds; it waits for
 * the handle's stream.
 *
 * Not offered: the late side outputs (sideOutputLeftLateData / Right), snapshots, key_hash
 * columns, the RCCL exchange, network-buffer ingest, and gw_encode_rows_* of these rows (the
 * encoder stamps end - 1, not max(left ts, right ts)). */
#define GW_IJOIN_MAX_BOUND ((int64_t)1 << 62)
int  gw_interval_join_device(int32_t probe_side, int64_t n_p, const int64_t* d_pkey, const int64_t* d_pts,
                             const int64_t* d_ppay, int64_t n_b, const int64_t* d_bkey, const int64_t* d_bts,
                             const int64_t* d_bpay, int64_t lower, int64_t upper, int64_t* d_key_out,
                             int64_t* d_lts_out, int64_t* d_rts_out, int64_t* d_lpay_out, int64_t* d_rpay_out,
                             int64_t cap, int64_t* n_out, void* stream);
int  gw_interval_join_device_timed(int32_t probe_side, int64_t n_p, const int64_t* d_pkey, const int64_t* d_pts,
                                   const int64_t* d_ppay, int64_t n_b, const int64_t* d_bkey, const int64_t* d_bts,
                                   const int64_t* d_bpay, int64_t lower, int64_t upper, int64_t* d_key_out,
                                   int64_t* d_lts_out, int64_t* d_rts_out, int64_t* d_lpay_out,
                                   int64_t* d_rpay_out, int64_t cap, int64_t* n_out, void* stream,
                                   double* expand_ms);
int  gw_interval_join_host(int32_t probe_side, int64_t n_p, const int64_t* pkey, const int64_t* pts,
                           const int64_t* ppay, int64_t n_b, const int64_t* bkey, const int64_t* bts,
                           const int64_t* bpay, int64_t lower, int64_t upper, int64_t* key_out, int64_t* lts_out,
                           int64_t* rts_out, int64_t* lpay_out, int64_t* rpay_out, int64_t cap, int64_t* n_out);

typedef struct gw_ijoin gw_ijoin;
typedef struct gw_ijoin_config {
    int64_t lower;           /* inclusive, relative to the left record            */
    int64_t upper;
    int32_t device;
    int64_t capacity_hint;   /* initial rows of each side's log (0: 16)           */
    int64_t max_batch;       /* records per device pass of an ingest (0: 2^22)    */
} gw_ijoin_config;
typedef struct gw_ijoin_stats {
    int64_t live_left, live_right;                  /* records in the logs        */
    int64_t log_capacity_left, log_capacity_right;  /* rows allocated             */
    int64_t rows_emitted;
    int64_t log_growths;
    int64_t merges;                                 /* ingest passes that merged  */
    int64_t last_call_rows;                         /* rows of the last ingest    */
} gw_ijoin_stats;
int  gw_ijoin_create(const gw_ijoin_config* cfg, gw_ijoin** out);
int  gw_ijoin_destroy(gw_ijoin* h);
const char* gw_ijoin_last_error(const gw_ijoin* h);
int  gw_ijoin_ingest(gw_ijoin* h, int32_t side, int64_t n, const int64_t* key, const int64_t* ts,
                     const int64_t* payload, int64_t* rows);
int  gw_ijoin_ingest_device(gw_ijoin* h, int32_t side, int64_t n, const int64_t* d_key, const int64_t* d_ts,
                            const int64_t* d_payload, void* stream, int64_t* rows);
int  gw_ijoin_advance_watermark(gw_ijoin* h, int64_t watermark);
int  gw_ijoin_end_input(gw_ijoin* h);
int  gw_ijoin_pending(gw_ijoin* h, int64_t* n);
int  gw_ijoin_drain(gw_ijoin* h, int64_t* key, int64_t* lts, int64_t* rts, int64_t* lpay, int64_t* rpay,
                    int64_t cap, int64_t* n);
int  gw_ijoin_rows_device(gw_ijoin* h, const int64_t** d_key, const int64_t** d_lts, const int64_t** d_rts,
                          const int64_t** d_lpay, const int64_t** d_rpay, int64_t* n);
int  gw_ijoin_clear_rows(gw_ijoin* h);
int64_t gw_ijoin_late_dropped(const gw_ijoin* h);
int  gw_ijoin_get_stats(const gw_ijoin* h, gw_ijoin_stats* out);
int  gw_ijoin_last_times(gw_ijoin* h, double* probe_ms, double* merge_ms);
void* gw_ijoin_stream(gw_ijoin* h);

/* ---- network-buffer output: fired rows as serialized stream elements -------------
 * The output side's counterpart of gw_ingest_serialized*: instead of columns that the JVM turns
 * into one object per row and pushes through TimestampedCollector.collect and
 * RecordWriter.serializeRecord, the rows leave as the bytes that path would have written, one
 * contiguous range per downstream channel, ready for ResultPartitionWriter.emitRecord or for a
 * second operator's gw_ingest_serialized_device on the same GPU.
 *
 * gw_row_layout: the emitted Tuple, field by field: where a field's 8 source bytes come from
 * (GW_ROW_*) and its type.  'J': the source as a long.  'D': the source's IEEE bits unchanged
 * (NaN payloads and -0.0 included), from GW_ROW_RESULT only.  'I': the low 32 bits of a source
 * value that fits a Java int; one that does not fails the whole call with GW_E_RANGE (nothing is
 * truncated; the output contents are then unspecified).  Every row becomes
 *   be32 length | tag 0 (a record with timestamp) | be64 timestamp | the fields, big-endian
 * (RecordWriter.java:144-156, StreamElementSerializer.java:163-197, TupleSerializer.java:135-144),
 * gw_row_encoded_bytes(l) = 4 + 1 + 8 + the field widths bytes (< 0: an invalid layout).  The
 * timestamp is end - 1 (emitWindowContents: setAbsoluteTimestamp(window.maxTimestamp()),
 * WindowOperator.java:575-580); with GW_ENCODE_GLOBAL_WINDOW it is Long.MAX_VALUE
 * (GlobalWindow.maxTimestamp()), for count-window rows whose start and end are ordinals.
 * GW_E_INVALID: a field count outside 1..GW_MAX_FIELDS, an unknown source or type, 'D' from
 * another source than the result, GW_ROW_PAYLOAD without a payload column.
 *
 * gw_encode_rows_device: stateless; n rows in device columns (d_payload may be NULL) to
 * d_bytes[cap] in device memory (16-byte aligned).  channels == 1: the rows in input order.
 * channels > 1 (a downstream keyBy on the row key, KeyGroupStreamPartitioner.selectChannel):
 * row i goes to channel gw_operator_for_key_group(max_parallelism, channels,
 * gw_key_group_for_hash(gw_java_long_hash(key[i]), max_parallelism)), a channel's rows keep
 * their input order, and channel c's bytes are [chan_off[c], chan_off[c] + chan_bytes[c]) of
 * d_bytes (host arrays of `channels` entries; starts are 16-byte aligned, the bytes between two
 * ranges unspecified).  More than 128 channels: GW_E_UNSUPPORTED.  watermark != INT64_MIN: every
 * channel's range ends with the serialized Watermark(watermark) (13 bytes), as the operator
 * forwards the watermark to every channel behind the rows it fired; an empty channel then holds
 * just the watermark.  cap too small: GW_E_OUTPUT_FULL with the needed size in chan_off[0] and
 * nothing written.  No byte is ever written outside the reported ranges and their alignment
 * padding.  n = 0: GW_OK, empty ranges (or watermarks only).  Waits on `stream` (the offsets go
 * to the host), using scratch of its own per device.  Errors: gw_last_error of NULL.
 * gw_encode_rows_host: the same contract as plain host code over host columns and bytes (any
 * alignment): for a firing of a few rows, or a process without a device.
 *
 * gw_rows_serialized_device / gw_drain_serialized: the handle's pending rows (the view
 * gw_rows_device gives: plain, window-class, session, count-window, first-element and minBy
 * handles) encoded on the handle's stream; count-window handles get GW_ENCODE_GLOBAL_WINDOW,
 * GW_ROW_PAYLOAD is valid on first-element / minBy handles only.  *n_rows (may be NULL): the
 * rows encoded.  gw_rows_serialized_device writes d_bytes in device memory (16-byte aligned)
 * behind the pending work of `stream` (the consumer's, which may still be using the buffer; NULL =
 * the default stream), returns with the bytes complete, and leaves the rows pending: follow it
 * with gw_clear_rows.  gw_drain_serialized copies the bytes to the host array and removes the
 * rows on GW_OK; on any error they stay pending.  A handle fed a key_hash column carries keys
 * whose hashCode the rows do not hold: channels > 1 is GW_E_UNSUPPORTED there (channels == 1
 * works on every handle). */
#define GW_ROW_KEY 0      /* row key                        */
#define GW_ROW_START 1    /* window start                   */
#define GW_ROW_END 2      /* window end                     */
#define GW_ROW_RESULT 3   /* aggregate result (8 bytes)     */
#define GW_ROW_PAYLOAD 4  /* first-element / minBy payload  */
typedef struct gw_row_layout {
    int32_t nfields;                 /* 1..GW_MAX_FIELDS fields of the emitted Tuple    */
    int32_t source[GW_MAX_FIELDS];   /* GW_ROW_* per field                              */
    char    types[GW_MAX_FIELDS];    /* 'J', 'D' or 'I'                                 */
} gw_row_layout;
#define GW_ENCODE_GLOBAL_WINDOW 1
int64_t gw_row_encoded_bytes(const gw_row_layout* l);
int  gw_encode_rows_device(int64_t n, const int64_t* d_key, const int64_t* d_start, const int64_t* d_end,
                           const void* d_result, const int64_t* d_payload, const gw_row_layout* l, int32_t mode,
                           int32_t channels, int32_t max_parallelism, int64_t watermark, void* d_bytes, int64_t cap,
                           int64_t* chan_off, int64_t* chan_bytes, void* stream);
int  gw_encode_rows_host(int64_t n, const int64_t* key, const int64_t* start, const int64_t* end, const void* result,
                         const int64_t* payload, const gw_row_layout* l, int32_t mode, int32_t channels,
                         int32_t max_parallelism, int64_t watermark, void* bytes, int64_t cap, int64_t* chan_off,
                         int64_t* chan_bytes);
int  gw_drain_serialized(gw_handle* h, const gw_row_layout* l, int32_t channels, int32_t max_parallelism,
                         int64_t watermark, void* bytes, int64_t cap, int64_t* chan_off, int64_t* chan_bytes,
                         int64_t* n_rows);
int  gw_rows_serialized_device(gw_handle* h, const gw_row_layout* l, int32_t channels, int32_t max_parallelism,
                               int64_t watermark, void* d_bytes, int64_t cap, int64_t* chan_off, int64_t* chan_bytes,
                               int64_t* n_rows, void* stream);

int64_t gw_late_dropped(const gw_handle* h);
/* Late-data side output (GW_FLAG_LATE_SIDE_OUTPUT; WindowedStream.sideOutputLateData, RS/api/
 * datastream/WindowedStream.java): the records WindowOperator.processElement skips as late
 * (isSkippedElement && isElementLate, WindowOperator.java:440-446) are kept, as the element
 * itself (key, timestamp, value bits), instead of being counted in numLateRecordsDropped, and
 * handed out here (sideOutput :587-588).  A record is pending from the ingest call that saw
 * it; gw_drain_late copies up to cap records and removes them (GW_E_OUTPUT_FULL if more
 * remain).  Without the flag both report 0 records. */
int  gw_pending_late(gw_handle* h, int64_t* n);
int  gw_drain_late(gw_handle* h, int64_t* key, int64_t* ts, void* value, int64_t cap, int64_t* n);
int  gw_get_stats(const gw_handle* h, gw_stats* out);
int  gw_synchronize(gw_handle* h);
/* hipStream_t the handle launches on (for ordering / event timing by callers). */
void* gw_stream(gw_handle* h);
/* Average device duration (ms) per launch of each kernel family since the last call,
 * measured with HIP events on the handle's stream.  which: 0 = ingest (per batch;
 * region path: pass 1), 1 = fire, 2 = region pass 2 + apply (per buffer flush).
 * which = 3: *launches = the fires enqueued right behind their flush, without a host
 * round trip between them (gw_advance_watermark's common case), *ms = 0.
 * which = 4: *launches = those of them whose rows the flush's apply kernel emitted itself (the
 * fused fire: its time is part of which = 2, and which = 1 counts no launch for it), *ms = 0.
 * which = 5: *launches = the fused fires that were revoked (their rows dropped, the windows
 * fired the exact way instead), *ms = 0.
 * which = 6, 7, 8 (session handles, timing enabled with 2): the ingest's slot lookup (prep),
 * grouping sort and per-key replay (segment), per launch; parts of which = 0.
 * which = 9, 10 (pane handles): *launches = the region pass-1 launches so far that took the lean
 * kernel (9) and the general one (10), *ms = 0; not reset by the call. */
int  gw_kernel_time_ms(gw_handle* h, int which, double* ms, int64_t* launches);
/* enable: 0 off, 1 every launch, k > 1: the region path's pass 1 (one launch per batch, all
 * alike) is timed on every k-th batch only (two event records per timed launch cost host
 * time between batches); `launches` then counts the timed ones.  Session handles: 2 also times
 * the ingest's three stages by themselves (which = 6, 7, 8; six more event records per batch). */
int  gw_enable_kernel_timing(gw_handle* h, int enable);

/* ---- window stagger (stateless) ------------------------------------------ */
/* WindowStagger (RS/api/windowing/assigners/WindowStagger.java:27-60) applied to a tumbling
 * assigner's global offset as TumblingEventTimeWindows.assignWindows does at the first
 * element (TumblingEventTimeWindows.java:72-79): *offset_out = (global_offset + stagger) % size
 * (Java remainder), the offset to create the operator with.  stagger = 0 (ALIGNED),
 * (long)(random01 * size) (RANDOM: random01 is the caller's ThreadLocalRandom.nextDouble()),
 * or max(0, processing_time - TimeWindow.getWindowStartWithOffset(processing_time, 0, size))
 * (NATURAL).  GW_E_INVALID for size <= 0, |global_offset| >= size or random01 outside [0, 1). */
#define GW_STAGGER_ALIGNED 0
#define GW_STAGGER_RANDOM  1
#define GW_STAGGER_NATURAL 2
int  gw_window_stagger_offset(int32_t stagger, int64_t processing_time, double random01, int64_t size,
                              int64_t global_offset, int64_t* offset_out);

/* ---- key groups (stateless) ---------------------------------------------- */
int32_t gw_java_long_hash(int64_t key);             /* Long.hashCode                     */
int32_t gw_murmur_hash(int32_t code);               /* MathUtils.murmurHash              */
int32_t gw_key_group_for_hash(int32_t key_hash, int32_t max_parallelism);
int32_t gw_operator_for_key_group(int32_t max_parallelism, int32_t parallelism, int32_t kg);
int32_t gw_default_max_parallelism(int32_t parallelism);
/* Device kernel: kg[i] / owner[i] (either may be NULL) for n keys. */
int  gw_key_groups_device(int64_t n, const int64_t* d_key, const int32_t* d_key_hash,
                          int32_t max_parallelism, int32_t parallelism,
                          int32_t* d_kg, int32_t* d_owner, void* stream);
/* Device kernel: stable partition of (key, ts, value) by owner subtask
 * (KeyGroupStreamPartitioner).  Output columns are grouped by destination; counts[p]
 * (device int64[parallelism]) receives the number of records for subtask p.
 * d_scratch must hold gw_partition_scratch_bytes(n, parallelism) bytes. */
int64_t gw_partition_scratch_bytes(int64_t n, int32_t parallelism);
int  gw_partition_device(int64_t n, const int64_t* d_key, const int32_t* d_key_hash,
                         const int64_t* d_ts, const void* d_value,
                         int32_t max_parallelism, int32_t parallelism,
                         int64_t* d_key_out, int64_t* d_ts_out, void* d_value_out,
                         int64_t* d_counts, void* d_scratch, void* stream);

/* Packed exchange records -- this path's serialized form of the records RecordWriter.emit
 * ships to the key group's owner (flink-runtime/.../io/network/api/writer/RecordWriter.java:
 * 104-110, KeyGroupStreamPartitioner.java:55-64), chosen for xGMI: one 8-byte word per record
 * instead of 24 B of key, ts and value
 *   lo32 = key, hi32 = value << 4 | d        (d = pane - base_pane, 0 <= d < 16)
 * for records whose key is in [0, 2^32), whose value (if the batch has values) is in
 * [-2^27, 2^27), and whose pane floor((ts - offset) / pane) lies in [base_pane, base_pane + 16);
 * the others travel as (key, ts, value).  Unpacked, a record's timestamp is its pane's start,
 * which changes no window decision of a tumbling / sliding assigner with size >= slide and
 * pane = gcd(size, slide) (assignWindows, isWindowLate and the cleanup time depend on the pane
 * alone).  Not for sessions, size < slide, the late side output, first-element / minBy
 * handles or floating values: those need the record's own timestamp or value.
 * gw_pack_geom_init: pane = gcd(size, slide) and base_pane = the pane of `watermark` (the
 * operator's watermark before the batch: records of earlier panes travel unpacked);
 * GW_E_UNSUPPORTED when size < slide or watermark = Long.MIN_VALUE.
 * gw_pack_records / gw_unpack_records: the same packing on the host (fits[i] = 0: record i
 * does not pack). */
typedef struct gw_pack_geom {
    int64_t pane;
    int64_t offset;
    int64_t base_pane;
    int32_t enabled;
    int32_t pad;
} gw_pack_geom;
int  gw_pack_geom_init(gw_pack_geom* g, int64_t size, int64_t slide, int64_t offset, int64_t watermark);
int  gw_pack_records(int64_t n, const int64_t* key, const int64_t* ts, const int64_t* value, const gw_pack_geom* g,
                     uint64_t* words, uint8_t* fits);
int  gw_unpack_records(int64_t n, const uint64_t* words, const gw_pack_geom* g, int64_t* key, int64_t* ts,
                       int64_t* value);
/* Device: stable partition by owner with packing (g->enabled): counts[2q] packed words of
 * subtask q (in d_packed_out), counts[2q + 1] its other records (in the columns), buckets laid
 * out q-major (q's packed words, then its other records, then q + 1's ...) at positions of one
 * numbering into both outputs.  parallelism <= 128.  d_scratch: gw_partition_scratch_bytes(n,
 * 2 * parallelism).  gw_unpack_device: n words back to columns. */
int  gw_partition_packed_device(int64_t n, const int64_t* d_key, const int64_t* d_ts, const int64_t* d_value,
                                int32_t max_parallelism, int32_t parallelism, const gw_pack_geom* g,
                                uint64_t* d_packed_out, int64_t* d_key_out, int64_t* d_ts_out, int64_t* d_value_out,
                                int64_t* d_counts, void* d_scratch, void* stream);
/* The exchange's single-pass partition (ranks <= 16): owner q's records go to region q of
 * capacity cap >= n -- its packed words (g enabled, else none) at d_packed_out + q * cap, its
 * other records at d_key_out / d_ts_out / d_value_out + q * cap, both in arrival order; d_counts
 * as gw_partition_packed_device's ([2p] with g enabled, else [p]).  No histogram pass: a
 * region per owner lets each tile's positions follow from earlier tiles' counts alone.  g may
 * be NULL (no packing); scratch: gw_partition_scratch_bytes(n, 2p). */
int  gw_partition_regions_device(int64_t n, const int64_t* d_key, const int64_t* d_ts, const int64_t* d_value,
                                 int32_t max_parallelism, int32_t parallelism, const gw_pack_geom* g, int64_t cap,
                                 uint64_t* d_packed_out, int64_t* d_key_out, int64_t* d_ts_out,
                                 int64_t* d_value_out, int64_t* d_counts, void* d_scratch, void* stream);
int  gw_unpack_device(int64_t n, const uint64_t* d_words, const gw_pack_geom* g, int64_t* d_key, int64_t* d_ts,
                      int64_t* d_value, void* stream);
/* The stages a job chains ahead of keyBy on simple records, fused on the device (no Flink-core
 * interface: the Yahoo Streaming Benchmark's FilterFunction(event_type == view) + projection +
 * join against a static ad -> campaign table, AdvertisingTopologyNative): of the n records
 * whose d_sel[i] == sel_value, in arrival order, d_key_out[j] = d_dict[d_idx[i]] and
 * d_ts_out[j] = d_ts[i]; *n_out = their number (the call waits for it on `stream`).  An index
 * outside [0, dict_n) is GW_E_RANGE.  Outputs hold n records at most. */
int  gw_select_lookup_device(int64_t n, const int64_t* d_sel, int64_t sel_value, const int64_t* d_idx,
                             const int64_t* d_dict, int64_t dict_n, const int64_t* d_ts, int64_t* d_key_out,
                             int64_t* d_ts_out, int64_t* n_out, void* stream);
/* gw_ingest_device for a batch of n_other column records followed by n_words packed words
 * (the receive side of the packed exchange: what StreamTaskNetworkInput deserializes before
 * WindowOperator.processElement, WindowOperator.java:293-447, sees record by record)
 * (gw_exchange_last_words): the words' timestamps are their panes' starts (gw_pack_geom).  A
 * plain pane operator's region pass 1 decodes the words itself; the direct / pre-aggregation
 * paths and window-class handles get them unpacked first.  GW_E_UNSUPPORTED when n_words > 0
 * and the handle needs a record's own timestamp or value (sessions, count windows,
 * first-element / minBy handles, the late side output, floating aggregates) or when g's pane
 * does not divide the handle's size, slide and offset difference.  Column pointers may be NULL
 * when n_other = 0. */
int  gw_ingest_packed_device(gw_handle* h, int64_t n_other, const int64_t* d_key, const int64_t* d_ts,
                             const int64_t* d_value, int64_t n_words, const uint64_t* d_words,
                             const gw_pack_geom* g, void* stream);

/* ---- keyBy exchange over RCCL (one process per GPU) ------------------------
 * Replaces the network shuffle behind KeyGroupStreamPartitioner.selectChannel
 * (flink-runtime/.../streaming/runtime/partitioner/KeyGroupStreamPartitioner.java:55-64)
 * and RecordWriter.emit (flink-runtime/.../io/network/api/writer/RecordWriter.java:
 * 104-110): per watermark batch, the device partition above, an RCCL all-to-all of the
 * per-destination counts, then one grouped ncclSend/ncclRecv per column and peer over
 * xGMI.  The watermark combine of StatusWatermarkValve.inputWatermark (minimum over the
 * input channels, flink-streaming-java/.../watermarkstatus/StatusWatermarkValve.java:
 * 153-185) is an RCCL all-reduce(MIN).
 *
 * gw_exchange_unique_id: rank 0 creates the 128-byte communicator id; the caller hands it
 * to every rank out of band (the JobManager / a TCP rendezvous), each rank calls
 * gw_exchange_create with it.
 *
 * gw_exchange_batch: d_key/d_ts (d_value, d_key_hash may be NULL) hold this rank's n records
 * of one watermark batch and wm the watermark its source emitted after them.  One RCCL
 * all-to-all carries, per peer, (record count, watermark, column presence); the host waits
 * for it once (one device->host copy: the only host synchronisation of the batch), checks
 * that every rank sends the same columns (GW_E_INVALID otherwise, on every rank), then
 * enqueues one grouped ncclSend/ncclRecv per column and peer on `stream`.  Out: the *n_out
 * records this rank owns in receive columns owned by the exchange (*d_*_out; NULL for an
 * absent column), valid until GW_EXCHANGE_RECV_SETS batches later (receive sets used in turn);
 * *wm_out = the minimum of the ranks' watermarks (StatusWatermarkValve); *ingest_stream = a
 * hand-off stream of this receive set, ordered after the receives: pass it as the producer
 * stream of gw_ingest_device, whose "producer waits for my reads" ordering then lands on
 * the hand-off stream, so the exchange of the next batch never waits for this batch's
 * ingest, only the reuse of this receive set GW_EXCHANGE_RECV_SETS batches later does; that
 * ordering is taken when the later batch is finished, so a driver that finishes batches ahead of
 * the ingest (e.g. from a thread of its own) finishes batch b only once the ingest of batch
 * b - GW_EXCHANGE_RECV_SETS has been issued.  All ranks call it
 * for every batch (n may be 0).  gw_exchange_counts: the last batch's per-peer send and
 * receive record counts (nranks each; either may be NULL).
 *
 * Failure: no host wait of the exchange is unbounded (a failed channel fails the task in the
 * reference; here a dead or diverging peer would otherwise leave every rank spinning in RCCL).
 * Each wait polls the stream, ncclCommGetAsyncError and a deadline (gw_exchange_set_timeout,
 * default 60000 ms; 0: none); on a stream error, an asynchronous RCCL error or expiry the
 * communicator is aborted (ncclCommAbort) and the call returns GW_E_STATE with the reason in
 * gw_exchange_last_error.  Every later call on that exchange returns GW_E_STATE; destroy it
 * and fail the task (the JVM side throws, GpuKeyByExchange.java). */
#define GW_EXCHANGE_ID_BYTES 128
#define GW_EXCHANGE_RECV_SETS 3
typedef struct gw_exchange gw_exchange;
int  gw_exchange_unique_id(void* id);
int  gw_exchange_create(gw_exchange** out, int32_t nranks, int32_t rank, const void* id, int32_t device,
                        int32_t max_parallelism);
void gw_exchange_destroy(gw_exchange* ex);
int  gw_exchange_set_timeout(gw_exchange* ex, int64_t timeout_ms);
/* gw_exchange_batch in two halves, so no host wait sits between batches: gw_exchange_begin
 * partitions a batch and queues its count all-to-all (no wait); gw_exchange_finish takes the
 * oldest begun batch, waits for its counts (the batch's one host wait, bounded as above),
 * queues the sends / receives and returns what gw_exchange_batch returns.  Up to two batches
 * may be begun and not finished (GW_E_STATE beyond); issue begin(b + 1) before finish(b) and
 * the partition of b + 1 runs while the host waits for b's counts.  Both halves of a batch
 * on the same stream.  Each call selects the exchange's device for the calling thread, so the
 * exchange may run on a host thread of its own (one thread per exchange at a time).  Packing takes its base pane from the combined watermark of the last
 * batch finished before the begin (the same on every rank, which begin and finish in the
 * same order). */
int  gw_exchange_begin(gw_exchange* ex, int64_t n, const int64_t* d_key, const int32_t* d_key_hash,
                       const int64_t* d_ts, const int64_t* d_value, int64_t wm, void* stream);
int  gw_exchange_finish(gw_exchange* ex, int64_t* n_out, const int64_t** d_key_out, const int32_t** d_key_hash_out,
                        const int64_t** d_ts_out, const int64_t** d_value_out, int64_t* wm_out, void** ingest_stream,
                        void* stream);
int  gw_exchange_batch(gw_exchange* ex, int64_t n, const int64_t* d_key, const int32_t* d_key_hash,
                       const int64_t* d_ts, const int64_t* d_value, int64_t wm, int64_t* n_out,
                       const int64_t** d_key_out, const int32_t** d_key_hash_out, const int64_t** d_ts_out,
                       const int64_t** d_value_out, int64_t* wm_out, void** ingest_stream, void* stream);
int  gw_exchange_counts(const gw_exchange* ex, int64_t* send, int64_t* recv);
/* Packing (gw_pack_geom above) for the following batches of a tumbling / sliding operator
 * (size >= slide) without the late side output: from the second batch on, the records that
 * fit travel as 8-byte words (base pane: the previous batch's combined watermark) and arrive
 * unpacked, behind the records that did not fit; per key the arrival order then differs, so
 * only for integer aggregates (with_values: the value column is an integer sum / min / max /
 * count operand).  Every rank must enable it alike (else GW_E_INVALID on every rank at the
 * next batch).  gw_exchange_last_packed: records this rank received packed in the last batch. */
int  gw_exchange_enable_packing(gw_exchange* ex, int64_t size, int64_t slide, int64_t offset, int32_t with_values);
int64_t gw_exchange_last_packed(const gw_exchange* ex);
/* gw_exchange_set_unpack(ex, 0): the received words stay packed -- gw_exchange_batch's
 * *n_out and columns then hold only the records that travelled unpacked, and
 * gw_exchange_last_words gives the words (device, valid like the columns) and their geometry
 * for gw_ingest_packed_device, whose region pass 1 decodes them (8 B read per record instead
 * of an unpack pass writing 24 B that pass 1 reads again). */
int  gw_exchange_set_unpack(gw_exchange* ex, int32_t unpack);
int  gw_exchange_last_words(const gw_exchange* ex, int64_t* n_words, const uint64_t** d_words, gw_pack_geom* g);
int  gw_exchange_min_watermark(gw_exchange* ex, int64_t wm, int64_t* out, void* stream);
const char* gw_exchange_last_error(const gw_exchange* ex);
/* The per-peer plan gw_exchange_batch runs after its count all-to-all, as a host function
 * (no device, no communicator): from the messages this rank sent and received --
 * msg[4q .. 4q+3] = (records, watermark, column mask, packed records) for peer q -- the
 * offsets and counts of every send and receive (send_off[q]: the first record for q in the
 * rank's owner-partitioned numbering; recv_off[q]: where q's records land when nothing is
 * packed: the receive columns hold the peers' records in rank order, as all_to_all_single
 * lays them out), the total received and the minimum watermark over the ranks
 * (StatusWatermarkValve).  GW_E_INVALID when a peer's column mask (value column, key hashes,
 * packing) differs from this rank's.
 * gw_exchange_plan_packed: the packed split -- send_packed[q] of q's records are words (at
 * send_off[q]), the rest follow them; q's unpacked-in-transit records land at
 * recv_other_off[q] of the receive columns, its words at recv_packed_off[q] of the word
 * buffer (recv_packed[q] of them), and are unpacked to positions total_other + recv_packed_off[q]. */
int  gw_exchange_plan(int32_t nranks, const int64_t* sent_msg, const int64_t* recv_msg, int64_t cols_mask,
                      int64_t wm, int64_t* send_off, int64_t* send_cnt, int64_t* recv_off, int64_t* recv_cnt,
                      int64_t* total, int64_t* wm_min);
int  gw_exchange_plan_packed(int32_t nranks, const int64_t* sent_msg, const int64_t* recv_msg, int64_t* send_packed,
                             int64_t* recv_other_off, int64_t* recv_packed_off, int64_t* recv_packed,
                             int64_t* total_other, int64_t* total_packed);

#ifdef __cplusplus
}
#endif
#endif /* GPUWIN_H */
