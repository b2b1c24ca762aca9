// udiv32 / make_udiv32 and the lean pass-1 classification p1_lean (flink_amd/csrc/gw_common.h) on
// the CPU, on their own (tests/test_udiv32_host.py builds this with -fsanitize=undefined over
// tests/native/fake_hip, with __host__ / __device__ / __forceinline__ defined away).
//   * udiv32 against `/`: every n < 2^32 for divisors 2, 3 and 2000; 0, 1, the neighbours of
//     sampled multiples of d up to 2^32 - 1, and 2^32 - 1 for the other divisors, among them 1
//     and divisors >= 2^32;
//   * p1_lean against a restatement in 128-bit arithmetic with `/` and `%`, over random
//     geometries and records near every boundary (t_late, t_late + 2^32, the ring's ends, the
//     re-fire bound, the record formats' key and value limits, Long.MIN_VALUE).
// The full classify (gw_pane.hip) takes the whole IngestArgs of gw_kernels.h, which needs the
// device intrinsics of gw_device.h: it is not compared here but on the GPU
// (tests/test_gpu_p1_paths.py).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "gw_common.h"

using namespace gw;

static int fails = 0;
static void fail(const char* what, uint64_t n, uint64_t d, uint64_t got, uint64_t want) {
    if (fails++ < 20) printf("FAIL %s: n=%llu d=%llu got=%llu want=%llu\n", what, (unsigned long long)n,
                             (unsigned long long)d, (unsigned long long)got, (unsigned long long)want);
}

static void check(uint64_t n, uint64_t d, const UDiv32& m) {
    const uint32_t got = udiv32((uint32_t)n, m);
    const uint64_t want = n / d;
    if (got != want) fail("udiv32", n, d, got, want);
}

static void exhaustive(uint32_t d) {
    const UDiv32 m = make_udiv32(d);
    constexpr int kThreads = 8;
    std::vector<std::thread> th;
    std::vector<uint64_t> bad(kThreads, 0), first(kThreads, 0);
    for (int t = 0; t < kThreads; ++t)
        th.emplace_back([&, t] {
            const uint64_t lo = ((uint64_t)1 << 32) / kThreads * t, hi = ((uint64_t)1 << 32) / kThreads * (t + 1);
            for (uint64_t n = lo; n < hi; ++n)
                if (udiv32((uint32_t)n, m) != (uint32_t)n / d && bad[t]++ == 0) first[t] = n;
        });
    for (auto& x : th) x.join();
    for (int t = 0; t < kThreads; ++t)
        if (bad[t]) fail("udiv32 exhaustive", first[t], d, udiv32((uint32_t)first[t], m), first[t] / d);
    printf("udiv32 d=%u: every n < 2^32 ok\n", d);
}

static void sampled(uint64_t d) {
    const UDiv32 m = make_udiv32(d);
    const uint64_t top = 0xffffffffull;
    check(0, d, m); check(1, d, m); check(top, d, m); check(top - 1, d, m);
    if (d <= top) {
        const uint64_t nmul = top / d;                     // multiples of d up to 2^32 - 1
        const uint64_t step = nmul / 2000000 + 1;          // about two million of them, the last included
        for (uint64_t k = 1; k <= nmul; k += step) {
            check(k * d - 1, d, m); check(k * d, d, m);
            if (k * d + 1 <= top) check(k * d + 1, d, m);
        }
        check(nmul * d - 1, d, m); check(nmul * d, d, m);
        if (nmul * d + 1 <= top) check(nmul * d + 1, d, m);
    } else {
        for (uint64_t n = 0; n <= top; n += 65521) check(n, d, m);
    }
    printf("udiv32 d=%llu: sampled ok\n", (unsigned long long)d);
}

// ---- p1_lean against a restatement ----
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}
static int64_t clamp_add(int64_t a, __int128 b) {
    __int128 r = (__int128)a + b;
    if (r < INT64_MIN) r = INT64_MIN;
    if (r > INT64_MAX) r = INT64_MAX;
    return (int64_t)r;
}

template <bool NR, bool N4, bool V32>
static int lean_ref(const P1Hot& h, uint64_t g, int64_t key, int64_t ts, int64_t v) {
    if (ts == INT64_MIN) return P1_SPECIAL;
    if (ts < h.t_late) return h.late_plain ? P1_LATE : P1_SPECIAL;
    const unsigned __int128 d = (unsigned __int128)((__int128)ts - (__int128)h.t_late);
    if (d >> 32) return P1_SPECIAL;
    const uint64_t q = (uint64_t)(d / g);
    if (q < h.q_refire || q < h.delta || q - h.delta >= h.ring) return P1_SPECIAL;
    if (NR) {
        if (key < 0 || key >= (N4 ? kNarCountKeyLimit : kNarKeyLimit)) return P1_SPECIAL;
        if (!N4 && (v < -kNarValLimit || v >= kNarValLimit)) return P1_SPECIAL;
    } else {
        if (key == INT64_MIN) return P1_SPECIAL;
        if (V32 && (v < INT32_MIN || v > INT32_MAX)) return P1_SPECIAL;
    }
    return (int)((h.b_pos + (q - h.delta)) % h.ring);
}

template <bool NR, bool N4, bool V32>
static void fuzz(const char* name, int rounds) {
    static const uint64_t widths[] = {1, 2, 3, 7, 500, 1000, 2000, 1u << 20, 86400000, 0x7fffffffull, 0x80000000ull,
                                      0xffffffffull, 1ull << 32, (1ull << 32) + 5, 1ull << 40};
    static const int64_t origins[] = {0, 1700000000000ll, -5000000000ll, INT64_MIN, INT64_MIN + 1, INT64_MAX - 10,
                                      INT64_MAX - (1ll << 32)};
    long n = 0;
    for (int r = 0; r < rounds; ++r) {
        const uint64_t g = widths[rnd() % (sizeof widths / sizeof *widths)];
        P1Hot h{};
        h.t_late = r % 3 ? origins[rnd() % (sizeof origins / sizeof *origins)] : (int64_t)rnd();
        h.div = make_udiv32(g);
        h.ring = 1 + rnd() % 64;
        h.b_pos = rnd() % h.ring;
        h.delta = r % 4 == 0 ? (uint32_t)(rnd() % (1u << 31)) : (uint32_t)(rnd() % 8);
        h.q_refire = r % 5 == 0 ? (uint32_t)rnd() : (uint32_t)(rnd() % (h.delta + 3));
        h.late_plain = rnd() & 1;
        const __int128 edges[] = {0, (__int128)1 << 32, (__int128)g * h.delta, (__int128)g * ((uint64_t)h.delta + h.ring),
                                  (__int128)g * h.q_refire};
        for (int e = 0; e < 5; ++e)
            for (int o = -2; o <= 2; ++o)
                for (int kk = 0; kk < 6; ++kk) {
                    const int64_t ts = kk == 5 ? INT64_MIN : clamp_add(h.t_late, edges[e] + o + (kk == 4 ? (int64_t)(rnd() % (4 * g + 1)) : 0));
                    static const int64_t keys[] = {0, 1, -1, INT64_MIN, INT64_MAX, kNarKeyLimit - 1, kNarKeyLimit,
                                                   kNarCountKeyLimit - 1, kNarCountKeyLimit, 1ll << 32};
                    static const int64_t vals[] = {0, -1, kNarValLimit - 1, kNarValLimit, -kNarValLimit, -kNarValLimit - 1,
                                                   INT32_MAX, (int64_t)INT32_MAX + 1, INT32_MIN, (int64_t)INT32_MIN - 1,
                                                   INT64_MIN, INT64_MAX};
                    const int64_t key = kk < 3 ? keys[rnd() % 10] : (int64_t)(rnd() % 1000);
                    const int64_t v = kk < 3 ? vals[rnd() % 12] : (int64_t)(rnd() % 1000);
                    const int got = p1_lean<NR, N4, V32>(h, key, ts, v), want = lean_ref<NR, N4, V32>(h, g, key, ts, v);
                    ++n;
                    if (got != want && fails++ < 20)
                        printf("FAIL p1_lean %s: g=%llu t_late=%lld delta=%u q_refire=%u ring=%u b_pos=%u plain=%u key=%lld ts=%lld "
                               "v=%lld got=%d want=%d\n", name, (unsigned long long)g, (long long)h.t_late, h.delta, h.q_refire,
                               h.ring, h.b_pos, h.late_plain, (long long)key, (long long)ts, (long long)v, got, want);
                }
    }
    printf("p1_lean %s: %ld records ok\n", name, n);
}

int main() {
    exhaustive(2); exhaustive(3); exhaustive(2000);
    const uint64_t ds[] = {1, 7, 500, 1000, 1u << 20, 86400000, 0x7fffffffull, 0x80000000ull, 0xffffffffull,
                           1ull << 32, (1ull << 32) + 1, 1ull << 40, 1ull << 63, UINT64_MAX};
    for (uint64_t d : ds) sampled(d);
    fuzz<false, false, false>("wide", 20000);
    fuzz<false, false, true>("compact", 20000);
    fuzz<true, false, false>("narrow", 20000);
    fuzz<true, true, false>("narrow count", 20000);
    if (fails) { printf("%d failures\n", fails); return 1; }
    printf("ok\n");
    return 0;
}
