// The memory owners of flink_amd/csrc/gw_devmem.h on the CPU: the real header over the
// malloc-backed hip_runtime.h of tests/native/fake_hip (tests/test_devmem.py builds this with
// ASan + UBSan, so a double free, a leak or a read past a block ends the program).
#include "gw_devmem.h"

#include <cstdio>
#include <utility>

using namespace gw;

#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            fprintf(stderr, "devmem.cpp:%d: %s\n", __LINE__, #c);    \
            exit(1);                                                 \
        }                                                            \
    } while (0)

// One interface over DevBuf<int64_t> (a single column) and DevCols<K> with a column mask.
struct OneBuf {
    static constexpr int N = 1;
    DevBuf<int64_t> b;
    unsigned mask = 1;
    int64_t* col(int) const { return b.p; }
    int64_t cap() const { return b.cap; }
    hipError_t grow(int64_t n, int64_t from, int64_t live) { return b.reserve_keep(n, from, live, nullptr); }
    void reset() { b.reset(); }
};
template <int K>
struct Cols {
    static constexpr int N = K;
    DevCols<K> c;
    unsigned mask;
    explicit Cols(unsigned m) : mask(m) {}
    int64_t* col(int i) const { return c.col[i]; }
    int64_t cap() const { return c.cap; }
    hipError_t grow(int64_t n, int64_t from, int64_t live) { return c.reserve_keep(n, from, live, nullptr, mask); }
    void reset() { c.reset(); }
};

static int64_t value(int col, int64_t j) { return 1000 * (col + 1) + j; }

template <class O>
static void fill(O& o) {
    for (int i = 0; i < O::N; ++i)
        for (int64_t j = 0; o.col(i) && j < o.cap(); ++j) o.col(i)[j] = value(i, j);
}
// The front of every column holds what fill() put at [from, from + live).
template <class O>
static void check_front(const O& o, int64_t from, int64_t live) {
    for (int i = 0; i < O::N; ++i) {
        CHECK((o.col(i) != nullptr) == ((o.mask >> i & 1) != 0));
        for (int64_t j = 0; o.col(i) && j < live; ++j) CHECK(o.col(i)[j] == value(i, from + j));
    }
}

template <class O>
static void check_keep(O o, const char* name) {
    int ncol = 0;
    for (int i = 0; i < O::N; ++i) ncol += o.mask >> i & 1;
    const int live0 = fake_hip::live;
    // a successful growth: cap as asked, the live range in front, one synchronise, the old blocks freed
    auto grow_ok = [&](int64_t n, int64_t from, int64_t live) {
        const int syncs = fake_hip::syncs, allocs = fake_hip::allocs;
        CHECK(o.grow(n, from, live) == hipSuccess);
        CHECK(o.cap() == n);
        CHECK(fake_hip::syncs == syncs + 1);
        CHECK(fake_hip::allocs == allocs + ncol);
        CHECK(fake_hip::live == live0 + ncol);
        check_front(o, from, live);
    };
    grow_ok(8, 0, 0);  // from empty
    fill(o);
    grow_ok(20, 3, 4);  // live_from > 0
    fill(o);
    // the k-th allocation of a growth fails: nothing changes, nothing leaks
    for (int k = 1; k <= ncol; ++k) {
        int64_t* before[O::N];
        for (int i = 0; i < O::N; ++i) before[i] = o.col(i);
        const int syncs = fake_hip::syncs;
        fake_hip::fail_in = k;
        CHECK(o.grow(40, 5, 6) == hipErrorOutOfMemory);
        CHECK(fake_hip::fail_in == 0);
        for (int i = 0; i < O::N; ++i) CHECK(o.col(i) == before[i]);
        CHECK(o.cap() == 20);
        check_front(o, 0, 20);
        CHECK(fake_hip::live == live0 + ncol);
        CHECK(fake_hip::syncs == syncs);
    }
    grow_ok(40, 5, 6);  // the growth that failed, now with memory
    fill(o);
    grow_ok(64, 7, 0);  // nothing live
    o.reset();
    CHECK(o.cap() == 0 && fake_hip::live == live0);
    for (int i = 0; i < O::N; ++i) CHECK(o.col(i) == nullptr);
    grow_ok(4, 0, 0);  // usable after reset(); freed by the destructor
    printf("%s: keep ok (%d columns)\n", name, ncol);
}

static void check_discard() {
    DevBuf<int32_t> b;
    CHECK(b.reserve_discard(10) == hipSuccess && b.cap == 10 && b.get() && fake_hip::live == 1);
    int32_t* p = b;
    const int allocs = fake_hip::allocs;
    CHECK(b.reserve_discard(10) == hipSuccess && b.reserve_discard(3) == hipSuccess);  // enough: nothing happens
    CHECK(b.p == p && b.cap == 10 && fake_hip::allocs == allocs);
    b[9] = 7;
    fake_hip::fail_in = 1;
    CHECK(b.reserve_discard(100) == hipErrorOutOfMemory);
    CHECK(b.p == nullptr && b.cap == 0 && fake_hip::live == 0);
    CHECK(b.reserve_discard(100) == hipSuccess && b.cap == 100 && fake_hip::live == 1);
    b[99] = 1;
    printf("DevBuf: discard ok\n");
}

template <class T, class Alloc>
static void check_moves(Alloc alloc, const char* name) {
    const int live0 = fake_hip::live;
    {
        T a;
        alloc(a);
        const auto cap = a.cap;
        CHECK(fake_hip::live > live0);
        const int blocks = fake_hip::live - live0;
        T b(std::move(a));  // move construction: the source is empty
        CHECK(a.cap == 0 && b.cap == cap && fake_hip::live == live0 + blocks);
        T c;
        alloc(c);
        CHECK(fake_hip::live == live0 + 2 * blocks);
        c = std::move(b);  // move assignment: c's own blocks are freed, the source is empty
        CHECK(b.cap == 0 && c.cap == cap && fake_hip::live == live0 + blocks);
        a.reset();  // empty owners: nothing to free
        b.reset();
        CHECK(fake_hip::live == live0 + blocks);
    }
    CHECK(fake_hip::live == live0);  // freed once (a second free would end the program under ASan)
    printf("%s: moves ok\n", name);
}

static void check_pinned() {
    PinnedBuf<int64_t> h;
    CHECK(h.alloc(4, hipHostMallocCoherent) == hipSuccess && fake_hip::last_host_flags == hipHostMallocCoherent);
    CHECK(h.cap == 4 && h.get() && fake_hip::live == 1);
    h[3] = 5;
    CHECK(h.alloc(16, hipHostMallocDefault) == hipSuccess && fake_hip::last_host_flags == hipHostMallocDefault);
    CHECK(h.cap == 16 && fake_hip::live == 1);  // the old block went first
    h[15] = 5;
    fake_hip::fail_in = 1;
    CHECK(h.alloc(32, hipHostMallocDefault) == hipErrorOutOfMemory && h.p == nullptr && h.cap == 0 && fake_hip::live == 0);
    CHECK(h.alloc(2, hipHostMallocDefault) == hipSuccess);
    h.reset();
    CHECK(h.p == nullptr && h.cap == 0 && fake_hip::live == 0);
    printf("PinnedBuf: ok\n");
}

int main() {
    check_keep(OneBuf{}, "DevBuf");
    check_keep(Cols<3>(0x7), "DevCols<3>");
    check_keep(Cols<5>(0x17), "DevCols<5> mask 0x17");  // column 3 never allocated
    check_discard();
    check_moves<DevBuf<int64_t>>([](DevBuf<int64_t>& b) { CHECK(b.reserve_discard(6) == hipSuccess); }, "DevBuf");
    check_moves<DevCols<3>>([](DevCols<3>& c) { CHECK(c.reserve_keep(6, 0, 0, nullptr) == hipSuccess); }, "DevCols<3>");
    check_moves<PinnedBuf<char>>([](PinnedBuf<char>& h) { CHECK(h.alloc(6, hipHostMallocDefault) == hipSuccess); }, "PinnedBuf");
    check_pinned();
    CHECK(fake_hip::live == 0 && fake_hip::fail_in == 0);
    printf("ok\n");
    return 0;
}
