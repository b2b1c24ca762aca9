// The checkpoint blob format ("GWS1", versions 1-4): one bounds-checked host codec.
// Header-only and host-only (standard headers + include/gpuwin.h): every reader and writer
// of the runtime goes through it, and tests/native/snapshot_codec.cpp runs it under the
// sanitizers without a GPU.
//
// Blob (little-endian): Header, int64 kg_offsets[kg_hi - kg_lo + 2], then the entries of
// each key group.  Versions: 1 pane entries (32 bytes), 2 session and 3 count windows
// (fixed-size entries of `reserved` int64 words, key first, offsets in entries), 4 the heap
// backend's per-key-group byte layout (big-endian, offsets in bytes; walk_windows,
// walk_count_windows).
// flags: kKeyHashes -- the keys came with a key_hash column (String, Integer, ... keys as
// caller ids): each state entry carries the key's Java hashCode after the key (version 4:
// be32 after the be64 key; versions 2 / 3: one more int64 word at the end).
// kFirstElement -- version-4 entries end with the first element's payload (be64).
#pragma once

#include <cstdint>
#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/gpuwin.h"

namespace gw {
namespace snap {

struct Header {
    char magic[4];
    uint32_t version;
    int32_t agg, assigner;
    int64_t size, slide, offset, gap, flags;
    int32_t max_parallelism, kg_lo, kg_hi, reserved;
    int64_t fired_lo, fired_hi;
    int64_t entries;  // entries (versions 1-3) / payload bytes (version 4)
};
static_assert(sizeof(Header) == 96, "snapshot header layout");

constexpr uint32_t kMaxVersion = 4;
constexpr int64_t kKeyHashes = 1;
constexpr int64_t kFirstElement = 2;

// code GW_OK: no error
struct Err {
    int code = GW_OK;
    const char* reason = "";
    explicit operator bool() const { return code != GW_OK; }
};
inline Err invalid(const char* why) { return Err{GW_E_INVALID, why}; }
constexpr const char* kTruncated = "truncated snapshot blob";

// ---- bytes ------------------------------------------------------------------------------
inline void put64(std::vector<uint8_t>& o, int64_t v) {
    for (int i = 0; i < 8; ++i) o.push_back((uint8_t)((uint64_t)v >> (56 - 8 * i)));
}
inline void put32(std::vector<uint8_t>& o, int32_t v) {
    for (int i = 0; i < 4; ++i) o.push_back((uint8_t)((uint32_t)v >> (24 - 8 * i)));
}
inline int64_t get64(const uint8_t* p) {
    uint64_t v = 0;
    for (int i = 0; i < 8; ++i) v = (v << 8) | p[i];
    return (int64_t)v;
}
inline int32_t get32(const uint8_t* p) {
    uint32_t v = 0;
    for (int i = 0; i < 4; ++i) v = (v << 8) | p[i];
    return (int32_t)v;
}
// Timers sort by their bytes: the timestamp is stored with its sign bit flipped
// (TimerSerializer.serialize, TimerSerializer.java:147-152).  Its own inverse.
inline int64_t flip_sign(int64_t ts) { return (int64_t)((uint64_t)ts ^ 0x8000000000000000ull); }

// ---- widths and fields --------------------------------------------------------------------
inline int64_t acc_bytes(int32_t agg) {
    return agg == GW_SUM_I32 ? 4 : (agg == GW_AVG_I64 || agg == GW_AVG_F64) ? 16 : 8;
}
inline int64_t num_key_groups(const Header& hd) { return (int64_t)hd.kg_hi - hd.kg_lo + 1; }
inline int64_t hash_bytes(const Header& hd) { return (hd.flags & kKeyHashes) ? 4 : 0; }
// Bytes that `entries` and the offset table count in: version 4 counts bytes.
inline int64_t entry_unit(const Header& hd) {
    return hd.version == 1 ? 32 : hd.version >= 4 ? 1 : (int64_t)hd.reserved * 8;
}
// Window layout.  State entry: (start, end, key, [be32 hash,] accumulator, [be64 payload]).
inline int64_t state_acc_at(const Header& hd) { return 24 + hash_bytes(hd); }
inline int64_t state_payload_at(const Header& hd) { return state_acc_at(hd) + acc_bytes(hd.agg); }
inline int64_t state_entry_bytes(const Header& hd) {
    return state_payload_at(hd) + ((hd.flags & kFirstElement) ? 8 : 0);
}
inline int64_t state_start(const uint8_t* p) { return get64(p); }
inline int64_t state_end(const uint8_t* p) { return get64(p + 8); }
constexpr int64_t kStateKeyAt = 16, kStateHashAt = 24;
inline int64_t state_key(const uint8_t* p) { return get64(p + kStateKeyAt); }
inline int32_t state_hash(const uint8_t* p) { return get32(p + kStateHashAt); }
// Merging-window-set head: (key, [be32 hash,] be32 c); then c x (window, state window).
inline int64_t set_head_bytes(const Header& hd) { return 12 + hash_bytes(hd); }
constexpr int64_t kSetHashAt = 8, kSetWindowBytes = 32;
// Timer: (flip_sign(timestamp), key, window start, window end).
constexpr int64_t kTimerBytes = 32, kTimerKeyAt = 8;
inline int64_t timer_time(const uint8_t* p) { return flip_sign(get64(p)); }
inline int64_t timer_key(const uint8_t* p) { return get64(p + kTimerKeyAt); }
inline int64_t timer_start(const uint8_t* p) { return get64(p + 16); }
inline int64_t timer_end(const uint8_t* p) { return get64(p + 24); }
inline void put_timer(std::vector<uint8_t>& o, int64_t ts, int64_t key, int64_t start, int64_t end) {
    put64(o, flip_sign(ts)); put64(o, key); put64(o, start); put64(o, end);
}
// Count-window layout.  Contents: (GlobalWindow = byte 0, key, [be32 hash,] accumulator);
// count: (byte 0, key, [be32 hash,] be64 count).
constexpr int64_t kCountKeyAt = 1, kCountHashAt = 9;
inline int64_t count_value_at(const Header& hd) { return 9 + hash_bytes(hd); }
inline int64_t count_state_bytes(const Header& hd) { return count_value_at(hd) + acc_bytes(hd.agg); }
inline int64_t count_entry_bytes(const Header& hd) { return count_value_at(hd) + 8; }

// ---- reading ------------------------------------------------------------------------------
// Every step over blob bytes is taken and bounds-checked here (Entries indexes a range that
// take() has handed out).
struct Cursor {
    const uint8_t* p = nullptr;
    const uint8_t* end = nullptr;
    bool at_end() const { return p == end; }
    int64_t left() const { return end - p; }
    // The next n bytes, or null when n is negative or more than what is left.
    const uint8_t* take(int64_t n) {
        if (n < 0 || n > end - p) return nullptr;
        const uint8_t* q = p;
        p += n;
        return q;
    }
    // A be32 count of entries at least `width` bytes each: not negative, and the entries fit.
    Err count(int64_t width, const char* negative, int32_t& n) {
        const uint8_t* q = take(4);
        if (!q) return invalid(kTruncated);
        n = get32(q);
        if (n < 0) return invalid(negative);
        if (width > 0 && n > (end - p) / width) return invalid(kTruncated);
        return Err{};
    }
};

// Magic and version range.
inline Err header(const void* buf, int64_t len, uint32_t vmin, uint32_t vmax, Header& hd) {
    if (!buf || len < (int64_t)sizeof hd) return invalid("snapshot blob too short");
    memcpy(&hd, buf, sizeof hd);
    if (memcmp(hd.magic, "GWS1", 4) != 0 || hd.version < vmin || hd.version > vmax) return invalid("not a gpuwin snapshot");
    return Err{};
}
// The key-group range, the offset table and the payload lie inside the blob.
inline Err payload(const void* buf, int64_t len, const Header& hd, Cursor& pay) {
    const int64_t nk = num_key_groups(hd), unit = entry_unit(hd), pay0 = (int64_t)sizeof hd + (nk + 1) * 8;
    if (unit <= 0 || nk <= 0 || hd.entries < 0 || len < pay0 || hd.entries > (len - pay0) / unit) return invalid(kTruncated);
    pay.p = (const uint8_t*)buf + pay0;
    pay.end = pay.p + hd.entries * unit;
    return Err{};
}
inline Err open(const void* buf, int64_t len, uint32_t vmin, uint32_t vmax, Header& hd, Cursor& pay) {
    const Err e = header(buf, len, vmin, vmax, hd);
    return e ? e : payload(buf, len, hd, pay);
}
// Key group g's part of an opened blob's payload, by the offset table.
inline Err group(const void* buf, const Header& hd, int64_t g, Cursor& part) {
    int64_t o[2];
    memcpy(o, (const uint8_t*)buf + sizeof hd + g * 8, 16);
    if (o[0] < 0 || o[1] < o[0] || o[1] > hd.entries) return invalid("corrupt snapshot offsets");
    const int64_t unit = entry_unit(hd);
    part.p = (const uint8_t*)buf + sizeof hd + (num_key_groups(hd) + 1) * 8 + o[0] * unit;
    part.end = part.p + (o[1] - o[0]) * unit;
    return Err{};
}

// A callback may return Err or nothing.
template <class F, class... A>
inline Err call(F& f, A&&... a) {
    if constexpr (std::is_void<decltype(f(std::forward<A>(a)...))>::value) {
        f(std::forward<A>(a)...);
        return Err{};
    } else {
        return f(std::forward<A>(a)...);
    }
}

// The heap backend's layout (HeapSnapshotStrategy.java:97-154) of the window operator's keyed
// state, per key group and big-endian:
//   "window-contents": be32 n; n x state entry (CopyOnWriteStateMapSnapshot.writeState :127-149);
//   "merging-window-set": be32 m; m x (set head, c x (window, state window)): a key's
//       MergingWindowSet mapping (MergingWindowSet.persist :99-106); session windows only;
//   timers: be32 t; t x timer (TimerSerializer.serialize :147-152).
// Calls state(entry), set(head, c, windows), timer(timer) and group() at each key group's
// end.  A set varies in size, so each head is bounds-checked as it is read.
// NoSets in place of a set callback, for layouts that hold no merging window sets: a count
// other than 0 fails with `reason`; without a reason the count is not looked at.
struct NoSets {
    const char* reason;
};
template <class M>
inline Err walk_sets(const Header& hd, Cursor& c, M& set) {
    if constexpr (std::is_same<M, const NoSets>::value || std::is_same<M, NoSets>::value) {
        const uint8_t* m = c.take(4);
        if (!m) return invalid(kTruncated);
        return set.reason && get32(m) != 0 ? invalid(set.reason) : Err{};
    } else {
        const int64_t mh = set_head_bytes(hd);
        int32_t m = 0;
        Err e = c.count(0, "negative merging window set count in snapshot key group", m);
        for (int32_t i = 0; !e && i < m; ++i) {
            const uint8_t* head = c.take(mh);
            if (!head) return invalid(kTruncated);
            const int32_t n = get32(head + mh - 4);
            if (n < 0) return invalid("negative merging window set size");
            const uint8_t* windows = c.take((int64_t)n * kSetWindowBytes);
            if (!windows) return invalid(kTruncated);
            e = call(set, head, n, windows);
        }
        return e;
    }
}
template <class S, class M, class T, class G>
inline Err walk_windows(const Header& hd, Cursor c, S&& state, M&& set, T&& timer, G&& group) {
    const int64_t eb = state_entry_bytes(hd);
    for (int64_t g = 0, nk = num_key_groups(hd); g < nk; ++g) {
        int32_t n = 0;
        Err e = c.count(eb, "negative entry count in snapshot key group", n);
        for (int32_t i = 0; !e && i < n; ++i) e = call(state, c.take(eb));
        if (!e) e = walk_sets(hd, c, set);
        if (!e) e = c.count(kTimerBytes, "negative timer count in snapshot key group", n);
        for (int32_t i = 0; !e && i < n; ++i) e = call(timer, c.take(kTimerBytes));
        if (!e) e = call(group);
        if (e) return e;
    }
    return c.at_end() ? Err{} : invalid("snapshot blob has trailing bytes");
}

// countWindow(size) = GlobalWindows + PurgingTrigger(CountTrigger(size)) (KeyedStream.java:
// 676-678) in the heap layout (as oracle/flink_oracle.c count_snapshot), per key group:
//   "window-contents": be32 n; n x (GlobalWindow = one byte 0, key, [be32 hash,] state) -- the
//       fold of the key's elements since its last FIRE_AND_PURGE;
//   "count": be32 m; m x (byte 0, key, [be32 hash,] be64 c mod size) -- CountTrigger's
//       ReducingState<Long> (CountTrigger.java:39-40);
//   be32 0 timers (GlobalWindow ends at Long.MAX_VALUE: no cleanup timer; CountTrigger
//       registers none).
// Calls contents(Entries) and counts(Entries) once per key group.
struct Entries {
    const uint8_t* p;
    int64_t width;
    int32_t n;
    const uint8_t* operator[](int32_t i) const { return p + i * width; }
};
template <class S, class C>
inline Err walk_count_windows(const Header& hd, Cursor c, S&& contents, C&& counts) {
    const int64_t sb = count_state_bytes(hd), cb = count_entry_bytes(hd);
    for (int64_t g = 0, nk = num_key_groups(hd); g < nk; ++g) {
        int32_t n = 0;
        Err e = c.count(sb, "corrupt snapshot blob", n);
        if (!e) e = call(contents, Entries{c.take(n * sb), sb, n});
        if (!e) e = c.count(cb, "corrupt snapshot blob", n);
        if (!e) e = call(counts, Entries{c.take(n * cb), cb, n});
        if (e) return e;
        const uint8_t* t = c.take(4);
        if (!t) return invalid(kTruncated);
        if (get32(t) != 0) return invalid("count windows hold no timers");
    }
    return c.at_end() ? Err{} : invalid("snapshot blob has trailing bytes");
}

// ---- writing ------------------------------------------------------------------------------
struct Writer {
    std::vector<uint8_t> pay;
    std::vector<int64_t> offs;
    void begin_group() { offs.push_back((int64_t)pay.size()); }
    void bytes(const uint8_t* p, int64_t n) { pay.insert(pay.end(), p, p + n); }
    // A counted section: be32 n, then the n entries' bytes.
    void count(int32_t n) { put32(pay, n); }
    void section(int32_t n, const std::vector<uint8_t>& entries) {
        count(n);
        pay.insert(pay.end(), entries.begin(), entries.end());
    }
    // The blob of hd (magic and entries filled in here) over the groups written.  Always
    // sets *len to the blob's size; without a buffer that is all (the length query);
    // GW_E_OUTPUT_FULL when cap is less.
    Err finish(Header hd, void* buf, int64_t cap, int64_t* len) {
        begin_group();  // the end offset
        const int64_t unit = entry_unit(hd), table = (int64_t)offs.size() * 8;
        *len = (int64_t)sizeof hd + table + (int64_t)pay.size();
        if (!buf) return Err{};
        if (cap < *len) return Err{GW_E_OUTPUT_FULL, "snapshot buffer too small"};
        for (int64_t& o : offs) o /= unit;
        memcpy(hd.magic, "GWS1", 4);
        hd.entries = (int64_t)pay.size() / unit;
        uint8_t* out = (uint8_t*)buf;
        memcpy(out, &hd, sizeof hd);
        memcpy(out + sizeof hd, offs.data(), (size_t)table);
        if (!pay.empty()) memcpy(out + sizeof hd + table, pay.data(), pay.size());
        return Err{};
    }
    std::vector<uint8_t> finish(const Header& hd) {
        std::vector<uint8_t> blob(sizeof hd + (offs.size() + 1) * 8 + pay.size());
        int64_t len;
        finish(hd, blob.data(), (int64_t)blob.size(), &len);
        return blob;
    }
};

}  // namespace snap
}  // namespace gw
