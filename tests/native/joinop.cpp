// The host side of a two-stream operator (flink_amd/csrc/gw_joinop.h) on the CPU: the real
// header over the malloc-backed hip_runtime.h of tests/native/fake_hip, whose log shows which
// stream recorded and waited for what (tests/test_joinop_host.py builds this with ASan + UBSan,
// so a double free, a leak or a read past a block ends the program).
#include "gw_joinop.h"

#include <cstdio>
#include <vector>

using namespace gw;

#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            fprintf(stderr, "joinop.cpp:%d: %s\n", __LINE__, #c);    \
            exit(1);                                                 \
        }                                                            \
    } while (0)

static int64_t value(int col, int64_t row) { return 1000 * (col + 1) + row; }
static uint8_t byte_value(int64_t row) { return (uint8_t)(1 + row % 3); }

// Writes rows [first, first + n) (numbered from the buffer's first row ever) behind the pending ones.
static void append(RowBuf& rb, int64_t first, int64_t n) {
    CHECK(rb.reserve(n, nullptr) == hipSuccess);
    int64_t* col[5];
    uint8_t* const bytes = rb.tail(col);
    for (int64_t j = 0; j < n; ++j) {
        for (int c = 0; c < 5; ++c) col[c][j] = value(c, first + j);
        if (bytes) bytes[j] = byte_value(first + j);
    }
    rb.pending += n;
}
// The pending rows are rows [first, first + rb.pending), in place.
static void check_live(const RowBuf& rb, int64_t first) {
    const int64_t* p[5];
    const int64_t** const pp[5] = {&p[0], &p[1], &p[2], &p[3], &p[4]};
    const uint8_t* b;
    int64_t n;
    rb.view(pp, &b, &n);
    CHECK(n == rb.pending);
    for (int64_t j = 0; j < n; ++j) {
        for (int c = 0; c < 5; ++c) CHECK(p[c][j] == value(c, first + j));
        if (rb.with_bytes) CHECK(b[j] == byte_value(first + j));
    }
}
struct HostRows {
    std::vector<int64_t> col[5];
    std::vector<uint8_t> bytes;
    int64_t* dst[5];
    explicit HostRows(int64_t n) : bytes((size_t)n, 0) {
        for (int c = 0; c < 5; ++c) {
            col[c].assign((size_t)n, -1);
            dst[c] = col[c].data();
        }
    }
};
// capacity 8, rows 0..7 appended, 3 drained: 5 pending from row 3, no free tail
static void drained3_pending5(RowBuf& rb, OpError& er) {
    append(rb, 0, 8);
    CHECK(rb.col.cap == 8 && rb.from == 0 && rb.pending == 8);
    HostRows h(3);
    int64_t n = -1;
    CHECK(rb.drain(h.dst, rb.with_bytes ? h.bytes.data() : nullptr, 3, &n, nullptr, er) == GW_E_OUTPUT_FULL);
    CHECK(n == 3 && rb.from == 3 && rb.pending == 5 && !er.failed);
    for (int64_t j = 0; j < 3; ++j) {
        for (int c = 0; c < 5; ++c) CHECK(h.col[c][(size_t)j] == value(c, j));
        if (rb.with_bytes) CHECK(h.bytes[(size_t)j] == byte_value(j));
    }
    check_live(rb, 3);
}

static void check_rowbuf_growth(bool with_bytes) {
    const int live0 = fake_hip::live;
    const int blocks = with_bytes ? 6 : 5;
    OpError er{"test join"};
    {
        // growth moves exactly the live rows (and their bytes) to row 0
        RowBuf rb{with_bytes};
        drained3_pending5(rb, er);
        CHECK(fake_hip::live == live0 + blocks);
        const int d2d = fake_hip::copies[hipMemcpyDeviceToDevice];
        CHECK(rb.reserve(4, nullptr) == hipSuccess);  // free tail: 0 rows
        CHECK(rb.from == 0 && rb.pending == 5 && rb.col.cap == 16);
        CHECK(rb.bytes.cap == (with_bytes ? 16 : 0));
        CHECK(fake_hip::copies[hipMemcpyDeviceToDevice] == d2d + blocks && fake_hip::live == live0 + blocks);
        check_live(rb, 3);
        int64_t* t[5];
        CHECK(rb.tail(t) == (with_bytes ? rb.bytes.p + 5 : nullptr) && t[0] == rb.col[0] + 5 && t[4] == rb.col[4] + 5);
        append(rb, 8, 4);  // the room that was asked for is there
        CHECK(rb.col.cap == 16 && rb.pending == 9);
        check_live(rb, 3);
    }
    CHECK(fake_hip::live == live0);
    // each allocation of that growth failing in turn: nothing changes, nothing leaks
    for (int k = 1; k <= blocks; ++k) {
        RowBuf rb{with_bytes};
        drained3_pending5(rb, er);
        int64_t* before[5];
        for (int c = 0; c < 5; ++c) before[c] = rb.col[c];
        uint8_t* const bytes_before = rb.bytes.p;
        fake_hip::fail_in = k;
        CHECK(rb.reserve(4, nullptr) == hipErrorOutOfMemory);
        CHECK(fake_hip::fail_in == 0);
        CHECK(rb.from == 3 && rb.pending == 5 && rb.col.cap == 8 && rb.bytes.p == bytes_before);
        CHECK(rb.bytes.cap == (with_bytes ? 8 : 0));
        for (int c = 0; c < 5; ++c) CHECK(rb.col[c] == before[c]);
        check_live(rb, 3);
        CHECK(fake_hip::live == live0 + blocks);
        CHECK(rb.reserve(4, nullptr) == hipSuccess && rb.from == 0);  // and with memory it grows
        check_live(rb, 3);
    }
    CHECK(fake_hip::live == live0);
    (void)hipGetLastError();
    printf("RowBuf: growth ok (%d blocks)\n", blocks);
}

static void check_rowbuf_drain() {
    OpError er{"test join"};
    RowBuf rb{true};
    const int64_t* p[5];
    const int64_t** const pp[5] = {&p[0], &p[1], &p[2], &p[3], &p[4]};
    const uint8_t* b = (const uint8_t*)1;
    int64_t n = -1;
    rb.view(pp, &b, &n);  // never used: empty
    CHECK(n == 0 && b == nullptr);
    for (int c = 0; c < 5; ++c) CHECK(p[c] == nullptr);

    append(rb, 0, 12);
    rb.view(pp, &b, &n);
    const int64_t* p0[5] = {p[0], p[1], p[2], p[3], p[4]};
    const uint8_t* const b0 = b;
    CHECK(n == 12 && p[0] == rb.col[0]);
    // in parts: cap rows each, the view moves up by 8 * cap bytes and the byte pointer by cap
    HostRows h(12);
    int64_t at = 0;
    for (int part = 0; part < 2; ++part) {
        int64_t* dst[5];
        for (int c = 0; c < 5; ++c) dst[c] = h.dst[c] + at;
        CHECK(rb.drain(dst, h.bytes.data() + at, 5, &n, nullptr, er) == GW_E_OUTPUT_FULL);
        CHECK(n == 5 && !er.failed);
        at += n;
        rb.view(pp, &b, &n);
        CHECK(n == 12 - at && b == b0 + at);
        for (int c = 0; c < 5; ++c) CHECK((const char*)p[c] == (const char*)p0[c] + 8 * at);
    }
    // the last part without the bytes: five copies, not six
    const int d2h = fake_hip::copies[hipMemcpyDeviceToHost];
    int64_t* dst[5];
    for (int c = 0; c < 5; ++c) dst[c] = h.dst[c] + at;
    CHECK(rb.drain(dst, nullptr, 5, &n, nullptr, er) == GW_OK);
    CHECK(n == 2 && rb.pending == 0 && rb.from == 0);
    CHECK(fake_hip::copies[hipMemcpyDeviceToHost] == d2h + 5);
    for (int64_t j = 0; j < 12; ++j) {
        for (int c = 0; c < 5; ++c) CHECK(h.col[c][(size_t)j] == value(c, j));
        CHECK(h.bytes[(size_t)j] == (j < 10 ? byte_value(j) : 0));
    }
    rb.view(pp, &b, &n);  // drained: empty again
    CHECK(n == 0 && b == nullptr && p[0] == nullptr && p[4] == nullptr);
    CHECK(rb.drain(dst, nullptr, 5, &n, nullptr, er) == GW_OK && n == 0);  // nothing to drain

    // clear() drops the rows; the next ones start at row 0 of the same blocks
    append(rb, 0, 8);
    HostRows h3(3);
    CHECK(rb.drain(h3.dst, nullptr, 3, &n, nullptr, er) == GW_E_OUTPUT_FULL && rb.from == 3);
    rb.clear();
    CHECK(rb.from == 0 && rb.pending == 0);
    const int allocs = fake_hip::allocs;
    CHECK(rb.reserve(2, nullptr) == hipSuccess && fake_hip::allocs == allocs);
    int64_t* t[5];
    CHECK(rb.tail(t) == rb.bytes.p && t[0] == rb.col[0] && t[4] == rb.col[4]);
    CHECK(!er.failed && er.err.empty());
    printf("RowBuf: drain ok\n");
}

static void check_operror() {
    for (int rc : {GW_E_INVALID, GW_E_OUTPUT_FULL}) {
        OpError er{"test join"};
        CHECK(er.fail(rc, "bad %s %d", "argument", 7) == rc);
        CHECK(!er.failed && er.err == "bad argument 7");
    }
    for (int rc : {GW_E_OOM, GW_E_DEVICE, GW_E_RANGE, GW_E_NO_TIMESTAMP, GW_E_UNSUPPORTED}) {
        OpError er{"test join"};
        CHECK(er.fail(rc, "broken") == rc);
        CHECK(er.failed && er.err == "broken");
        CHECK(er.fail(GW_E_INVALID, "later") == GW_E_INVALID && er.failed);  // failed stays
    }
    OpError er{"interval join"};
    CHECK(er.dev_fail(hipErrorOutOfMemory) == GW_E_DEVICE);
    CHECK(er.failed && er.err == "interval join: out of memory");
    printf("OpError: ok\n");
}

static int marked_body(OpStream& os, hipStream_t producer, bool work, int rc) {
    OpStream::Handoff handoff(os, producer, work);
    fake_hip::log.push_back({'B', nullptr, nullptr});  // the operator's work
    return rc;
}
static void check_opstream() {
    const int live0 = fake_hip::live;
    OpStream os;
    const char* what = nullptr;
    CHECK(os.create(3, &what) == hipSuccess && fake_hip::device == 3 && os.device == 3);
    CHECK(os.stream && os.ev_in && os.ev_out && fake_hip::live == live0 + 3);
    int other;
    hipStream_t producer = &other;
    for (int rc : {GW_OK, GW_E_DEVICE}) {  // the way back is taken on an error too
        fake_hip::log.clear();
        CHECK(marked_body(os, producer, true, rc) == rc);
        const auto& log = fake_hip::log;
        CHECK(log.size() == 5);
        CHECK(log[0].kind == 'R' && log[0].ev == os.ev_in && log[0].stream == producer);
        CHECK(log[1].kind == 'W' && log[1].ev == os.ev_in && log[1].stream == os.stream);
        CHECK(log[2].kind == 'B');
        CHECK(log[3].kind == 'R' && log[3].ev == os.ev_out && log[3].stream == os.stream);
        CHECK(log[4].kind == 'W' && log[4].ev == os.ev_out && log[4].stream == producer);
    }
    // the operator's own stream, or no records: only the body
    fake_hip::log.clear();
    CHECK(marked_body(os, os.stream, true, GW_OK) == GW_OK);
    CHECK(marked_body(os, producer, false, GW_OK) == GW_OK);
    CHECK(fake_hip::log.size() == 2 && fake_hip::log[0].kind == 'B' && fake_hip::log[1].kind == 'B');
    fake_hip::log.clear();
    hipStream_t own = os.stream;
    os.destroy();  // waits for the stream first
    CHECK(fake_hip::log.size() == 1 && fake_hip::log[0].kind == 'S' && fake_hip::log[0].stream == own);
    CHECK(fake_hip::live == live0 && !os.stream && !os.ev_in && !os.ev_out);
    os.destroy();  // and again: nothing left to do

    const char* calls[3] = {"hipStreamCreate", "hipEventCreate", "hipEventCreate"};
    for (int k = 1; k <= 3; ++k) {
        OpStream half;
        fake_hip::fail_in = k;
        CHECK(half.create(0, &what) == hipErrorOutOfMemory && std::string(what) == calls[k - 1]);
        CHECK(fake_hip::live == live0 + k - 1);
        half.destroy();
        CHECK(fake_hip::live == live0);
    }
    OpStream none;
    fake_hip::bad_device = 9;
    CHECK(none.create(9, &what) == hipErrorInvalidDevice && std::string(what) == "hipSetDevice");
    fake_hip::bad_device = -1;
    none.destroy();
    CHECK(fake_hip::live == live0);
    (void)hipGetLastError();
    printf("OpStream: ok\n");
}

static void check_staged_ingest() {
    const int live0 = fake_hip::live;
    OpError er{"test join"};
    std::vector<int64_t> host[3];
    for (int c = 0; c < 3; ++c)
        for (int64_t j = 0; j < 10; ++j) host[c].push_back(value(c, j));
    const int64_t* src[3] = {host[0].data(), host[1].data(), host[2].data()};
    {
        DevCols<3> stage;
        std::vector<int64_t> sizes;
        int64_t at = 0;
        const int allocs = fake_hip::allocs, h2d = fake_hip::copies[hipMemcpyHostToDevice];
        auto body = [&](int64_t m, int64_t* const* d) {
            for (int c = 0; c < 3; ++c) {
                CHECK(d[c] == stage[c]);
                for (int64_t j = 0; j < m; ++j) CHECK(d[c][j] == value(c, at + j));
            }
            sizes.push_back(m);
            at += m;
            return (int)GW_OK;
        };
        CHECK(staged_ingest(stage, 4, 0, src, nullptr, er, body) == GW_OK);  // no records: no stage, no call
        CHECK(sizes.empty() && stage.cap == 0 && fake_hip::allocs == allocs);
        CHECK(staged_ingest(stage, 4, 10, src, nullptr, er, body) == GW_OK);
        CHECK((sizes == std::vector<int64_t>{4, 4, 2}));
        CHECK(stage.cap == 4 && fake_hip::allocs == allocs + 3);  // allocated once
        CHECK(fake_hip::copies[hipMemcpyHostToDevice] == h2d + 9);
        // an error of the body ends the call and comes back as it is
        int calls = 0;
        CHECK(staged_ingest(stage, 4, 10, src, nullptr, er, [&](int64_t, int64_t* const*) {
                  return ++calls == 2 ? (int)GW_E_RANGE : (int)GW_OK;
              }) == GW_E_RANGE);
        CHECK(calls == 2 && fake_hip::allocs == allocs + 3 && !er.failed);
        // a chunk larger than the stage grows it
        CHECK(staged_ingest(stage, 8, 10, src, nullptr, er, [&](int64_t, int64_t* const*) { return (int)GW_OK; }) == GW_OK);
        CHECK(stage.cap == 8 && fake_hip::live == live0 + 3);
    }
    {
        DevCols<3> stage;  // no memory for the stage: the operator fails, the body never runs
        fake_hip::fail_in = 2;
        CHECK(staged_ingest(stage, 4, 10, src, nullptr, er, [&](int64_t, int64_t* const*) { CHECK(false); return 0; }) == GW_E_OOM);
        CHECK(er.failed && er.err == "test join: out of device memory staging a batch" && fake_hip::live == live0);
    }
    printf("staged_ingest: ok\n");
}

int main() {
    check_rowbuf_growth(true);
    check_rowbuf_growth(false);
    check_rowbuf_drain();
    check_operror();
    check_opstream();
    check_staged_ingest();
    CHECK(fake_hip::live == 0 && fake_hip::fail_in == 0);
    printf("ok\n");
    return 0;
}
