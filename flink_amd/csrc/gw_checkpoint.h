// What a checkpoint blob's entries mean for an operator (gw::ckpt), above the byte format of
// gw_snapshot.h (gw::snap): which (key, window) entries and timers a state has, for a window,
// session or count-window operator, a window-class composite and a first-element pair.  Header-
// and host-only: plain vectors in, a snap::Writer or plain vectors out, no device call.
#pragma once

#include <algorithm>
#include <array>
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "gw_common.h"
#include "gw_snapshot.h"

namespace gw {
namespace ckpt {

typedef __int128 i128;
inline i128 floor_div(i128 a, i128 b) {  // b > 0
    i128 q = a / b;
    if ((a % b) != 0 && a < 0) --q;
    return q;
}
inline bool fits64(i128 v) { return v >= (i128)INT64_MIN && v <= (i128)INT64_MAX; }

// Accumulator <-> cell words (the serializer's value, gw_common.h cells).
inline void acc_to_be(int agg, std::vector<uint8_t>& o, int64_t a0, int64_t a1) {
    switch (agg) {
    case GW_SUM_I32: snap::put32(o, (int32_t)(uint32_t)(uint64_t)a0); break;
    case GW_MIN_F64: case GW_MAX_F64: snap::put64(o, f64_from_order_key(a0)); break;
    case GW_AVG_I64: case GW_AVG_F64: snap::put64(o, a0); snap::put64(o, a1); break;
    default: snap::put64(o, a0); break;
    }
}
inline void acc_from_be(int agg, const uint8_t* p, int64_t& a0, int64_t& a1) {
    a1 = 0;
    switch (agg) {
    case GW_SUM_I32: a0 = (int64_t)snap::get32(p); break;
    case GW_MIN_F64: case GW_MAX_F64: a0 = f64_order_key(snap::get64(p)); break;
    case GW_AVG_I64: case GW_AVG_F64: a0 = snap::get64(p); a1 = snap::get64(p + 8); break;
    default: a0 = snap::get64(p); break;
    }
}

constexpr const char* kOtherOperator = "snapshot of a different window / aggregate / max parallelism";
constexpr const char* kTwoHashes = "snapshot: a key with two different key hashes";

// What the blobs depend on of an operator's configuration and geometry.
struct Spec {
    int32_t agg, assigner, trigger, max_parallelism;
    int64_t size, slide, cfg_slide;  // slide: the effective one (tumbling: size); cfg_slide: as configured
    int64_t offset, gap, allowed_lateness;
    int64_t n, m;  // a window is n panes, a slide m
    int64_t ew;    // session / count windows: int64 words of a slot entry (gw_session.h)
    bool session() const { return assigner == GW_SESSION || assigner == GW_SESSION_DYNAMIC; }
    bool purging() const { return trigger == GW_PURGING_EVENT_TIME_TRIGGER; }
    i128 win_start(i128 k) const { return (i128)offset + k * (i128)slide; }
    i128 win_k(int64_t s0) const { return floor_div((i128)s0 - offset, (i128)slide); }
    // Session and tumbling count windows: the heap layout (4); sliding count windows: fixed entries (3).
    uint32_t slot_version() const { return assigner == GW_COUNT_SLIDING ? 3u : 4u; }
    snap::Header header(uint32_t version, int32_t kg_lo, int32_t kg_hi, bool hashed) const {
        snap::Header hd{};
        hd.version = version; hd.agg = agg; hd.assigner = assigner;
        hd.size = size; hd.slide = cfg_slide; hd.offset = offset; hd.gap = gap;
        hd.flags = hashed ? snap::kKeyHashes : 0;
        hd.max_parallelism = max_parallelism; hd.kg_lo = kg_lo; hd.kg_hi = kg_hi;
        return hd;
    }
    // A blob of this assigner, aggregate and max parallelism (ew == 0: tumbling / sliding windows)?
    bool matches(const snap::Header& hd) const {
        const bool same = hd.agg == agg && hd.assigner == assigner && hd.max_parallelism == max_parallelism;
        if (ew == 0) return same && hd.version == 4 && hd.size == size && hd.slide == slide && hd.offset == offset;
        if (hd.version != slot_version() || !same) return false;
        if (session()) return hd.gap == gap && !(hd.flags & ~snap::kKeyHashes);
        if (assigner == GW_COUNT_TUMBLING) return hd.size == size && !(hd.flags & ~snap::kKeyHashes);
        return hd.gap == gap && hd.size == size && hd.slide == cfg_slide &&
               hd.reserved == (int32_t)(ew + snap::hash_bytes(hd) / 4);
    }
};

// The Java hashCodes of the keys fed with a key_hash, sorted by key: a key's key group at
// snapshot time.  Long.MIN_VALUE (the slot sentinel) has its own place.
struct KeyHashes {
    std::vector<std::pair<int64_t, int32_t>> kv;
    bool has_min = false;
    int32_t min_hash = 0;
    bool on() const { return has_min || !kv.empty(); }
    bool known(int64_t key, int32_t& h) const {
        if (key == kEmptyKey) { h = min_hash; return has_min; }
        auto it = std::lower_bound(kv.begin(), kv.end(), std::make_pair(key, INT32_MIN));
        if (it == kv.end() || it->first != key) return false;
        h = it->second;
        return true;
    }
    int32_t hash(int64_t key) const {
        int32_t h;
        return known(key, h) ? h : java_long_hash(key);
    }
    int32_t key_group(int64_t key, int32_t max_p) const { return key_group_for_hash(hash(key), max_p); }
};

// A restored blob's (key, hash) pairs, checked before anything changes: one hash per key
// within the blob (check()), and the hash the operator already holds for that key.
struct HashPairs {
    std::vector<int64_t> keys;
    std::vector<int32_t> hashes;
    void add(int64_t key, int32_t hash) { keys.push_back(key); hashes.push_back(hash); }
    snap::Err check() const {
        std::map<int64_t, int32_t> seen;
        for (size_t i = 0; i < keys.size(); ++i)
            if (seen.emplace(keys[i], hashes[i]).first->second != hashes[i]) return snap::invalid(kTwoHashes);
        return snap::Err{};
    }
    snap::Err check(const KeyHashes& kh) const {
        int32_t h0;
        for (size_t i = 0; i < keys.size(); ++i)
            if (kh.known(keys[i], h0) && h0 != hashes[i]) return snap::invalid(kTwoHashes);
        return snap::Err{};
    }
};

// A restored window's state: window index, accumulator, flags (gw_kernels.h kOv*).
struct WindowEntry {
    int64_t key, k, a0, a1;
    uint32_t flags;
};
constexpr uint32_t kTimer = 1;  // its event-time timer (maxTimestamp) is pending
inline bool by_key_k(const WindowEntry& x, const WindowEntry& y) { return x.key != y.key ? x.key < y.key : x.k < y.k; }

// Indices 0 .. n-1 by key group: kg_of(i) is i's; those outside [kg_lo, kg_hi] are left out.
template <class K>
inline std::vector<std::vector<int64_t>> by_key_group(size_t n, int32_t kg_lo, int32_t kg_hi, K kg_of) {
    std::vector<std::vector<int64_t>> by_kg((size_t)(kg_hi - kg_lo + 1));
    for (size_t i = 0; i < n; ++i) {
        const int32_t g = kg_of(i);
        if (g >= kg_lo && g <= kg_hi) by_kg[g - kg_lo].push_back((int64_t)i);
    }
    return by_kg;
}

// One key group of the window layout as it is written: state entries, merging window sets, timers.
struct Group {
    std::vector<uint8_t> st, ms, tm;
    int32_t nst = 0, nms = 0, ntm = 0;
    void state(const uint8_t* p, int64_t bytes) { st.insert(st.end(), p, p + bytes); nst++; }
    void state(const Spec& s, const KeyHashes& kh, int64_t s0, int64_t e0, int64_t key, int64_t a0, int64_t a1) {
        snap::put64(st, s0); snap::put64(st, e0); snap::put64(st, key);
        if (kh.on()) snap::put32(st, kh.hash(key));
        acc_to_be(s.agg, st, a0, a1);
        nst++;
    }
    void timer(int64_t ts, int64_t key, int64_t s0, int64_t e0) { snap::put_timer(tm, ts, key, s0, e0); ntm++; }
    void timer(const uint8_t* t) { tm.insert(tm.end(), t, t + snap::kTimerBytes); ntm++; }
    // A window's trigger timer (while it has not fired) and, under allowed lateness, its
    // cleanup timer (registerCleanupTimer :631-643; with lateness 0 the two coincide).
    void window_timers(const Spec& s, bool trigger, int64_t key, int64_t s0, int64_t e0) {
        const i128 mx = (i128)e0 - 1, ct = mx + (i128)s.allowed_lateness;
        if (trigger) timer((int64_t)mx, key, s0, e0);
        if (s.allowed_lateness > 0 && ct < (i128)INT64_MAX) timer((int64_t)ct, key, s0, e0);
    }
    void end(snap::Writer& w) {
        w.begin_group();
        w.section(nst, st); w.section(nms, ms); w.section(ntm, tm);
        *this = Group{};
    }
};

// ---- tumbling / sliding windows -----------------------------------------------------------
// Heap-layout blob (version 4, snap::walk_windows) of the tumbling / sliding window state: per
// key group every (key, window) whose panes hold data, folded, plus the restored windows; no
// merging window sets; the event-time timers:
//   state:   windows not fired yet; under allowed lateness with EventTimeTrigger also the
//            fired windows that are not cleaned yet (WindowOperator.cleanupTime :670-677);
//   timers:  maxTimestamp for the windows not fired yet (EventTimeTrigger.onElement),
//            maxTimestamp + lateness for every window with state when lateness > 0.
// col: (key, pane, a0, a1) of the non-null pane cells, kgs their key groups (keys with a key
// hash: by that hash); ov: the live restored windows; what lies outside [kg_lo, kg_hi] is left
// out.  fired_k: the first window not fired; state_lo: the first that holds state.
inline snap::Err encode_windows(const Spec& s, const KeyHashes& kh, int32_t kg_lo, int32_t kg_hi,
                                const std::vector<int64_t> (&col)[4], const std::vector<int32_t>& kgs,
                                const std::vector<WindowEntry>& ov, i128 fired_k, i128 state_lo, snap::Writer& w,
                                snap::Header& hd) {
    auto kg_of = [&](int64_t key) { return kh.key_group(key, s.max_parallelism); };
    auto by_kg = by_key_group(kgs.size(), kg_lo, kg_hi, [&](size_t i) { return kh.on() ? kg_of(col[0][i]) : kgs[i]; });
    auto ov_kg = by_key_group(ov.size(), kg_lo, kg_hi, [&](size_t i) { return kg_of(ov[i].key); });
    const int64_t id0 = identity0(s.agg);
    struct Win { int64_t a0, a1; bool timer; };
    Group grp;
    for (size_t g = 0; g < by_kg.size(); ++g) {
        // the windows holding state, by (key, k): those covering a pane with data, its cells
        // folded in pane order, then the restored ones
        std::map<std::pair<int64_t, i128>, Win> wins;
        auto add = [&](int64_t key, i128 k, int64_t a0, int64_t a1, bool timer) {
            if (k < state_lo) return;
            Win& x = wins.emplace(std::make_pair(key, k), Win{id0, 0, false}).first->second;
            fold_cell(s.agg, x.a0, x.a1, a0, a1);
            if (timer && k >= fired_k) x.timer = true;
        };
        auto& ix = by_kg[g];
        std::sort(ix.begin(), ix.end(), [&](int64_t x, int64_t y) {
            return col[0][x] != col[0][y] ? col[0][x] < col[0][y] : col[1][x] < col[1][y];
        });
        for (size_t a = 0; a < ix.size();) {
            const int64_t key = col[0][ix[a]], p = col[1][ix[a]];
            int64_t c0 = col[2][ix[a]], c1 = col[3][ix[a]];  // the pane's cells (the table's and parked ones), folded
            for (++a; a < ix.size() && col[0][ix[a]] == key && col[1][ix[a]] == p; ++a)
                fold_cell(s.agg, c0, c1, col[2][ix[a]], col[3][ix[a]]);
            for (i128 k = floor_div((i128)p - s.n, s.m) + 1; k <= floor_div(p, s.m); ++k) add(key, k, c0, c1, true);
        }
        for (int64_t i : ov_kg[g]) add(ov[i].key, ov[i].k, ov[i].a0, ov[i].a1, (ov[i].flags & kTimer) != 0);
        for (const auto& kx : wins) {
            const int64_t key = kx.first.first;
            const i128 s0 = s.win_start(kx.first.second), e0 = s0 + (i128)s.size;
            if (!fits64(s0) || !fits64(e0)) return snap::Err{GW_E_RANGE, "window bounds overflow int64"};
            grp.state(s, kh, (int64_t)s0, (int64_t)e0, key, kx.second.a0, kx.second.a1);
            grp.window_timers(s, kx.second.timer, key, (int64_t)s0, (int64_t)e0);
        }
        grp.end(w);  // merging window sets: none for tumbling / sliding windows
    }
    hd = s.header(4, kg_lo, kg_hi, kh.on());
    hd.slide = s.slide;
    return snap::Err{};
}

// The entries of a window blob (any key-group range), parsed and checked whole: windows of
// this assigner; an event-time timer at a window's maxTimestamp means that the window has not
// fired (kTimer).  why: holds the text of a formatted error.
inline snap::Err decode_windows(const Spec& s, snap::Header hd, snap::Cursor c, std::vector<WindowEntry>& out, HashPairs& hp,
                                std::string& why) {
    hd.flags &= snap::kKeyHashes;  // entries of this operator's width, whatever else the blob claims
    const bool hashed = hd.flags != 0;
    const int64_t acc_at = snap::state_acc_at(hd);
    std::set<std::pair<int64_t, int64_t>> armed;  // (key, k) of the current key group's timers at maxTimestamp
    size_t base = out.size();                     // its first entry in out
    return snap::walk_windows(
        hd, c,
        [&](const uint8_t* p) {
            const int64_t s0 = snap::state_start(p), e0 = snap::state_end(p), key = snap::state_key(p);
            const i128 k = s.win_k(s0);
            if (s.win_start(k) != (i128)s0 || (i128)s0 + s.size != (i128)e0) {
                char buf[128];
                snprintf(buf, sizeof buf, "snapshot window [%lld, %lld) is not a window of this assigner", (long long)s0,
                         (long long)e0);
                why = buf;
                return snap::invalid(why.c_str());
            }
            WindowEntry o{key, (int64_t)k, 0, 0, 0};
            if (hashed) hp.add(key, snap::state_hash(p));
            acc_from_be(s.agg, p + acc_at, o.a0, o.a1);
            out.push_back(o);
            return snap::Err{};
        },
        snap::NoSets{"merging window set in a tumbling / sliding snapshot"},
        [&](const uint8_t* t) {  // any other timer is a cleanup timer: implied by the state
            if (snap::timer_time(t) == (int64_t)((uint64_t)snap::timer_end(t) - 1))
                armed.insert({snap::timer_key(t), (int64_t)s.win_k(snap::timer_start(t))});
        },
        [&] {
            std::sort(out.begin() + base, out.end(), by_key_k);
            for (; base < out.size(); ++base)
                if (armed.count({out[base].key, out[base].k})) out[base].flags |= kTimer;
            armed.clear();
        });
}

// ---- session and count windows: ent holds the slot table's entries, kgs their key groups -------
// Session windows (snap::walk_windows), ent: (key, start, end, a0, a1, fired) per session.  A
// session's state is kept under the session itself, so its state window is the window; a
// fired session under PurgingTrigger holds no state (WindowOperator.java:482-484) and has no
// entry.  Timers: the trigger's at maxTimestamp while the session has not fired and, under
// allowed lateness, its cleanup timer.  Keys ascending, a key's sessions by start.
inline snap::Header encode_sessions(const Spec& s, const KeyHashes& kh, int32_t kg_lo, int32_t kg_hi,
                                    const std::vector<int64_t>& ent, const std::vector<int32_t>& kgs, snap::Writer& w) {
    Group grp;
    for (auto& ix : by_key_group(kgs.size(), kg_lo, kg_hi, [&](size_t i) { return kgs[i]; })) {
        std::sort(ix.begin(), ix.end(), [&](int64_t x, int64_t y) {
            const int64_t *a = &ent[6 * x], *b = &ent[6 * y];
            return a[0] != b[0] ? a[0] < b[0] : a[1] < b[1];
        });
        for (size_t a = 0, b = 0; a < ix.size(); a = b) {
            const int64_t key = ent[6 * ix[a]];
            while (b < ix.size() && ent[6 * ix[b]] == key) ++b;
            snap::put64(grp.ms, key);
            if (kh.on()) snap::put32(grp.ms, kh.hash(key));
            snap::put32(grp.ms, (int32_t)(b - a));
            grp.nms++;
            for (size_t q = a; q < b; ++q) {
                const int64_t* x = &ent[6 * ix[q]];
                const int64_t s0 = x[1], e0 = x[2];
                const bool fired = x[5] != 0;
                for (int64_t v : {s0, e0, s0, e0}) snap::put64(grp.ms, v);
                if (!(s.purging() && fired)) grp.state(s, kh, s0, e0, key, x[3], x[4]);
                grp.window_timers(s, !fired, key, s0, e0);
            }
        }
        grp.end(w);
    }
    return s.header(4, kg_lo, kg_hi, kh.on());
}

// ... and back into (key, start, end, a0, a1, fired) sessions: each merging-window-set mapping
// (window -> state window) takes the state of its state window (any original window, as
// MergingWindowSet.addWindow keeps it, :188-201), or none; a session has fired when its trigger
// timer at maxTimestamp is gone.  A session without state that has not fired is a trigger
// outside EventTimeTrigger / PurgingTrigger (GW_E_UNSUPPORTED); state no mapping names, or
// overlapping sessions of one key, are a corrupt blob.
inline snap::Err decode_sessions(const Spec& s, const snap::Header& hd, snap::Cursor c, std::vector<int64_t>& out,
                                 HashPairs& hp) {
    const bool hashed = snap::hash_bytes(hd) != 0;
    const int64_t acc_at = snap::state_acc_at(hd);
    const int64_t id0 = s.agg == GW_AVG_F64 ? INT64_MIN : identity0(s.agg);  // a purged session
    typedef std::tuple<int64_t, int64_t, int64_t> KW;  // (key, start, end)
    std::map<KW, std::pair<std::pair<int64_t, int64_t>, bool>> state;  // of the current key group -> (acc, used)
    std::vector<std::array<int64_t, 5>> ses;  // (key, start, end, state start, state end)
    std::set<KW> armed;  // sessions whose trigger timer (at maxTimestamp) is still set
    return snap::walk_windows(
        hd, c,
        [&](const uint8_t* p) {
            const int64_t key = snap::state_key(p);
            int64_t a0, a1;
            acc_from_be(s.agg, p + acc_at, a0, a1);
            if (hashed) hp.add(key, snap::state_hash(p));
            const KW kw{key, snap::state_start(p), snap::state_end(p)};
            if (!state.emplace(kw, std::make_pair(std::make_pair(a0, a1), false)).second)
                return snap::invalid("two state entries of one (key, window) in a snapshot key group");
            return snap::Err{};
        },
        [&](const uint8_t* head, int32_t n, const uint8_t* win) {
            const int64_t key = snap::get64(head);
            if (hashed) hp.add(key, snap::get32(head + snap::kSetHashAt));
            for (int32_t j = 0; j < n; ++j, win += snap::kSetWindowBytes)
                ses.push_back({key, snap::get64(win), snap::get64(win + 8), snap::get64(win + 16), snap::get64(win + 24)});
        },
        [&](const uint8_t* t) {
            const int64_t e0 = snap::timer_end(t);
            if (snap::timer_time(t) == (int64_t)((uint64_t)e0 - 1))
                armed.insert(KW{snap::timer_key(t), snap::timer_start(t), e0});
        },
        [&] {
            std::sort(ses.begin(), ses.end());
            for (size_t i = 0; i < ses.size(); ++i) {
                const auto& x = ses[i];
                if (x[2] <= x[1]) return snap::invalid("empty session window in a snapshot");
                if (i && ses[i - 1][0] == x[0] && ses[i - 1][2] >= x[1])  // TimeWindow.intersects is inclusive
                    return snap::invalid("overlapping sessions of one key in a snapshot");
                const bool fired = armed.count(KW{x[0], x[1], x[2]}) == 0;
                auto it = state.find(KW{x[0], x[3], x[4]});
                int64_t a0 = id0, a1 = 0;
                if (it != state.end()) {
                    if (it->second.second) return snap::invalid("two sessions share one state window");
                    it->second.second = true;
                    a0 = it->second.first.first, a1 = it->second.first.second;
                } else if (!fired) {
                    return snap::Err{GW_E_UNSUPPORTED, "a session without state whose timer has not fired "
                                                       "(a trigger other than EventTimeTrigger / PurgingTrigger)"};
                }
                out.insert(out.end(), {x[0], x[1], x[2], a0, a1, (int64_t)fired});
            }
            for (auto& kv : state)
                if (!kv.second.second) return snap::invalid("a state entry outside every merging window set");
            state.clear(); ses.clear(); armed.clear();
            return snap::Err{};
        });
}

// A tumbling count window (version 4, snap::walk_count_windows), ent: (key, element count, ring
// of count-pane accumulators) per key.  The contents are the current count pane; a key whose
// element count is a multiple of size was just purged and holds no state.
inline snap::Header encode_count(const Spec& s, const KeyHashes& kh, int32_t kg_lo, int32_t kg_hi,
                                 const std::vector<int64_t>& ent, const std::vector<int32_t>& kgs, snap::Writer& w) {
    const int64_t ew = s.ew, W = cell_words(s.agg), ring = (ew - 2) / W;
    auto live = [&](size_t i) { return ent[ew * i + 1] % s.size ? kgs[i] : -1; };
    for (auto& ix : by_key_group(kgs.size(), kg_lo, kg_hi, live)) {
        w.begin_group();
        std::sort(ix.begin(), ix.end(), [&](int64_t x, int64_t y) { return ent[ew * x] < ent[ew * y]; });
        std::vector<uint8_t> st, cnt;
        for (int64_t i : ix) {
            const int64_t* e = &ent[ew * i];
            const int64_t key = e[0], c = e[1];
            const int64_t* cell = e + 2 + (((c - 1) / s.size) % ring) * W;  // the current count pane
            for (std::vector<uint8_t>* v : {&st, &cnt}) {  // (GlobalWindow, key, [hash,] ...
                v->push_back(0);
                snap::put64(*v, key);
                if (kh.on()) snap::put32(*v, kh.hash(key));
            }
            acc_to_be(s.agg, st, cell[0], W == 2 ? cell[1] : 0);
            snap::put64(cnt, c % s.size);
        }
        w.section((int32_t)ix.size(), st);
        w.section((int32_t)ix.size(), cnt);
        w.section(0, {});  // no timers
    }
    return s.header(4, kg_lo, kg_hi, kh.on());
}
// ... and back: (key, element count = the trigger's count, the contents in count pane 0, identities elsewhere)
inline snap::Err decode_count(const Spec& s, const snap::Header& hd, snap::Cursor c, std::vector<int64_t>& ent,
                              HashPairs& hp) {
    const int64_t at = snap::count_value_at(hd), W = cell_words(s.agg);
    const bool hashed = snap::hash_bytes(hd) != 0;
    snap::Entries st{};
    return snap::walk_count_windows(
        hd, c, [&](snap::Entries contents) { st = contents; },
        [&](snap::Entries counts) {
            if (counts.n != st.n) return snap::invalid("count-window contents without their CountTrigger count");
            for (int32_t i = 0; i < st.n; ++i) {
                const uint8_t *x = st[i], *q = counts[i];
                const int64_t key = snap::get64(x + snap::kCountKeyAt), cnt = snap::get64(q + at);
                if (x[0] != 0 || q[0] != 0 || snap::get64(q + snap::kCountKeyAt) != key || cnt <= 0 || cnt >= s.size)
                    return snap::invalid("corrupt count-window snapshot entry");
                if (hashed) hp.add(key, snap::get32(x + snap::kCountHashAt));
                const size_t o = ent.size();
                ent.resize(o + (size_t)s.ew, 0);
                ent[o] = key, ent[o + 1] = cnt;
                // identities, then the contents in pane 0
                for (int64_t r = 2; r < s.ew; r += W) ent[o + r] = identity0(s.agg);
                int64_t a1;
                acc_from_be(s.agg, x + at, ent[o + 2], a1);
                if (W == 2) ent[o + 3] = a1;
            }
            return snap::Err{};
        });
}

// Sliding count windows (version 3): per key the CountTrigger count and the ring of count-pane
// accumulators, the contents the evicting operator keeps (EvictingWindowOperator.java:92-135).
// Key-group order, collection order within one; with key hashes, the key's hash as one more word.
inline snap::Header encode_slots(const Spec& s, const KeyHashes& kh, int32_t kg_lo, int32_t kg_hi,
                                 const std::vector<int64_t>& ent, const std::vector<int32_t>& kgs, snap::Writer& w) {
    for (auto& ix : by_key_group(kgs.size(), kg_lo, kg_hi, [&](size_t i) { return kgs[i]; })) {
        w.begin_group();
        for (int64_t i : ix) {
            w.bytes((const uint8_t*)&ent[s.ew * i], s.ew * 8);
            if (kh.on()) {
                const int64_t hw = (int64_t)kh.hash(ent[s.ew * i]);
                w.bytes((const uint8_t*)&hw, 8);
            }
        }
    }
    snap::Header hd = s.header(s.slot_version(), kg_lo, kg_hi, kh.on());
    hd.offset = 0; hd.reserved = (int32_t)(s.ew + (kh.on() ? 1 : 0));
    return hd;
}
// ... and back: an aligned copy of the entry words without the hash words.
inline snap::Err decode_slots(const Spec& s, const snap::Header& hd, snap::Cursor c, std::vector<int64_t>& ent,
                              HashPairs& hp) {
    const int64_t ew = s.ew + snap::hash_bytes(hd) / 4;
    if (hd.entries > c.left() / (ew * 8)) return snap::invalid(snap::kTruncated);  // not this operator's entries
    ent.resize((size_t)(hd.entries * s.ew));
    for (int64_t i = 0; i < hd.entries; ++i) {
        const uint8_t* x = c.take(ew * 8);
        memcpy(&ent[i * s.ew], x, (size_t)s.ew * 8);
        if (ew > s.ew) {
            int64_t hw;
            memcpy(&hw, x + s.ew * 8, 8);
            hp.add(ent[i * s.ew], (int32_t)hw);
        }
    }
    return snap::Err{};
}

// ---- window-class composites --------------------------------------------------------------
// The classes' heap-layout blobs merged per key group (their (window, key, state) entries and
// timers are disjoint by window), under the composite's own assigner header; the cut splits
// each key group's entries and timers by the class of their window.  No merging window sets.
struct WindowBlob {  // an operator's own blob (it outlives this): entries and timers per key group
    snap::Header hd;
    snap::Cursor c;
    std::vector<std::vector<const uint8_t*>> st, tm;
    size_t entries = 0;
    snap::Err open(const std::vector<uint8_t>& blob) { return snap::open(blob.data(), (int64_t)blob.size(), 4, 4, hd, c); }
    snap::Err walk() {
        st.assign(1, {}); tm.assign(1, {});
        return snap::walk_windows(
            hd, c, [&](const uint8_t* p) { st.back().push_back(p); entries++; }, snap::NoSets{},
            [&](const uint8_t* t) { tm.back().push_back(t); }, [&] { st.emplace_back(); tm.emplace_back(); });
    }
    size_t groups() const { return st.size() - 1; }
};
inline snap::Err merge_classes(const Spec& s, const std::vector<std::vector<uint8_t>>& blobs, int32_t kg_lo, int32_t kg_hi,
                               snap::Writer& w, snap::Header& hd) {
    std::vector<WindowBlob> cls(blobs.size());
    for (size_t j = 0; j < blobs.size(); ++j) {
        snap::Err e = cls[j].open(blobs[j]);
        if (e) return e;
        // every class sees every batch, so all or none carry key hashes
        if (cls[j].hd.flags != cls[0].hd.flags) return snap::Err{GW_E_STATE, "window classes disagree on key hashes"};
        if (cls[j].hd.kg_lo != kg_lo || cls[j].hd.kg_hi != kg_hi)
            return snap::Err{GW_E_STATE, "window classes disagree on key groups"};
        if ((e = cls[j].walk())) return e;
    }
    hd = blobs.empty() ? s.header(4, kg_lo, kg_hi, false) : cls[0].hd;
    const int64_t eb = snap::state_entry_bytes(hd);
    for (int64_t g = 0; g <= (int64_t)kg_hi - kg_lo; ++g) {  // encode_windows' order
        std::vector<const uint8_t*> st, tm;
        for (const WindowBlob& b : cls) {
            st.insert(st.end(), b.st[g].begin(), b.st[g].end());
            tm.insert(tm.end(), b.tm[g].begin(), b.tm[g].end());
        }
        std::sort(st.begin(), st.end(), [](const uint8_t* x, const uint8_t* y) {  // by (key, window)
            return std::make_pair(snap::state_key(x), snap::state_start(x)) <
                   std::make_pair(snap::state_key(y), snap::state_start(y));
        });
        std::sort(tm.begin(), tm.end(), [](const uint8_t* x, const uint8_t* y) {  // by (key, window, time bytes)
            return std::make_tuple(snap::timer_key(x), snap::timer_start(x), (uint64_t)snap::get64(x)) <
                   std::make_tuple(snap::timer_key(y), snap::timer_start(y), (uint64_t)snap::get64(y));
        });
        w.begin_group();
        w.count((int32_t)st.size());
        for (const uint8_t* p : st) w.bytes(p, eb);
        w.count(0);
        w.count((int32_t)tm.size());
        for (const uint8_t* t : tm) w.bytes(t, snap::kTimerBytes);
    }
    hd.assigner = s.assigner; hd.slide = s.slide; hd.offset = s.offset;
    return snap::Err{};
}
// One blob per class (kids: the classes' operators) of a composite's opened blob.
inline snap::Err cut_classes(const Spec& s, const std::vector<Spec>& kids, const snap::Header& hd, snap::Cursor c,
                             std::vector<std::vector<uint8_t>>& blobs) {
    const int64_t J = (int64_t)kids.size();
    snap::Header lay = hd;  // entries of the classes' width (decode_windows)
    lay.flags &= snap::kKeyHashes;
    const int64_t eb = snap::state_entry_bytes(lay);
    auto cls = [&](int64_t s0) {  // window class of a window start
        const int64_t k = (int64_t)s.win_k(s0);
        return (size_t)(((k % J) + J) % J);
    };
    std::vector<snap::Writer> w(J);
    std::vector<Group> grp(J);  // of the current key group
    const snap::Err e = snap::walk_windows(
        lay, c, [&](const uint8_t* p) { grp[cls(snap::state_start(p))].state(p, eb); },
        snap::NoSets{"merging window set in a sliding snapshot"},
        [&](const uint8_t* t) { grp[cls(snap::timer_start(t))].timer(t); },
        [&] { for (int64_t j = 0; j < J; ++j) grp[j].end(w[j]); });
    if (e) return e;
    blobs.resize(J);
    for (int64_t j = 0; j < J; ++j) {
        snap::Header kh = hd;
        kh.assigner = kids[j].assigner; kh.slide = kids[j].cfg_slide; kh.offset = kids[j].offset;
        blobs[j] = w[j].finish(kh);
    }
    return snap::Err{};
}

// ---- first-element pairs: one heap-layout blob for both operators ---------------------------
// The reference keeps one reduced Tuple per (key, window): the window's first element with the
// aggregated field replaced (HeapReducingState.java:90-97).  The blob holds that per entry:
// (window, key, [hash], aggregate, the first element's payload), flags |= snap::kFirstElement,
// and the aggregating operator's timers.  The second operator folds MIN of each record's arrival
// sequence; a minBy / maxBy pair has none and finds the element by (key, window, MIN / MAX).
struct FirstElementJoin {
    WindowBlob a;                                   // the aggregating operator's
    std::vector<int64_t> seqs;                      // the sequence of every entry's first element, in entry order
    std::vector<int64_t> by_key, by_start, by_res;  // minBy / maxBy: every entry's key, window start, MIN / MAX
    // Pass 1 over the operators' blobs (bb: null for minBy / maxBy).
    snap::Err open(const std::vector<uint8_t>& ba, const std::vector<uint8_t>* bb) {
        WindowBlob b;
        if (a.open(ba) || (bb && (b.open(*bb) || a.hd.flags != b.hd.flags)) ||
            snap::acc_bytes(bb ? b.hd.agg : a.hd.agg) != 8)
            return snap::Err{GW_E_STATE, "first-element snapshot: the operators' blobs differ"};
        snap::Err bad = a.walk();
        if (!bad && bb) bad = b.walk();
        if (bad) return bad;
        const snap::Err differ{GW_E_STATE, "first-element snapshot: entries differ"};
        const int64_t acc_at = snap::state_acc_at(a.hd);
        if (bb && b.groups() != a.groups()) return differ;
        for (size_t g = 0; g < a.groups(); ++g) {
            if (bb && b.st[g].size() != a.st[g].size()) return differ;
            for (size_t i = 0; i < a.st[g].size(); ++i) {
                const uint8_t* p = a.st[g][i];
                if (!bb) {  // (start, end, key, [hash], MIN / MAX)
                    by_start.push_back(snap::state_start(p));
                    by_key.push_back(snap::state_key(p));
                    by_res.push_back(snap::get64(p + acc_at));
                } else {  // the second operator: MIN_I64 of the sequence
                    if (memcmp(p, b.st[g][i], (size_t)acc_at) != 0) return differ;
                    seqs.push_back(snap::get64(b.st[g][i] + acc_at));
                }
            }
        }
        return snap::Err{};
    }
    // Pass 2: the blob of aggregate agg, pays[i] the payload of entry i's element.
    snap::Header write(int32_t agg, const std::vector<int64_t>& pays, snap::Writer& w) const {
        const int64_t ea = snap::state_entry_bytes(a.hd);
        size_t i = 0;
        for (size_t g = 0; g < a.groups(); ++g) {
            w.begin_group();
            w.count((int32_t)a.st[g].size());
            for (const uint8_t* p : a.st[g]) { w.bytes(p, ea); snap::put64(w.pay, pays[i++]); }
            w.count(0);
            w.count((int32_t)a.tm[g].size());
            for (const uint8_t* t : a.tm[g]) w.bytes(t, snap::kTimerBytes);
        }
        snap::Header hd = a.hd;
        hd.agg = agg; hd.flags |= snap::kFirstElement;
        return hd;
    }
};

// An opened first-element blob of aggregate agg split into the operators' blobs: the first
// gets the entries without their payloads, the second (window, key, new sequence) with the
// restored first elements numbered from seq0; both get the timers.
struct FirstElementSplit {
    std::vector<uint8_t> blobs[2];
    std::vector<int64_t> pays, by_cols[3];  // per entry: its payload; its key, window start, aggregate
    int64_t max_end = INT64_MIN;            // the latest window end
    snap::Err split(int32_t agg, int64_t seq0, const snap::Header& hd, snap::Cursor c) {
        const int64_t acc_at = snap::state_acc_at(hd), ea = snap::state_payload_at(hd);
        snap::Writer w[2];
        Group grp[2];  // of the current key group
        const snap::Err bad = snap::walk_windows(
            hd, c,
            [&](const uint8_t* p) {
                grp[0].state(p, ea), grp[1].state(p, acc_at);
                snap::put64(grp[1].st, seq0 + (int64_t)pays.size());  // the restored first element's new sequence
                pays.push_back(snap::get64(p + ea));
                max_end = std::max(max_end, snap::state_end(p));
                by_cols[0].push_back(snap::state_key(p));
                by_cols[1].push_back(snap::state_start(p));
                by_cols[2].push_back(snap::get64(p + acc_at));
            },
            snap::NoSets{"merging window set in a first-element snapshot"},
            [&](const uint8_t* t) { grp[0].timer(t), grp[1].timer(t); },
            [&] { grp[0].end(w[0]), grp[1].end(w[1]); });
        if (bad) return bad;
        for (int o = 0; o < 2; ++o) {
            snap::Header kh = hd;
            kh.flags &= ~snap::kFirstElement; kh.agg = o ? GW_MIN_I64 : agg;
            blobs[o] = w[o].finish(kh);
        }
        return snap::Err{};
    }
};

// ---- blob tools (the layout: gw_snapshot.h) ---------------------------------------------------
inline snap::Err slice(const void* blob, int64_t len, int32_t kg, void* out, int64_t cap, int64_t* out_len) {
    snap::Header hd;
    snap::Cursor c, part;
    snap::Err e = out_len ? snap::open(blob, len, 1, snap::kMaxVersion, hd, c) : snap::invalid("snapshot blob too short");
    if (!e && (kg < hd.kg_lo || kg > hd.kg_hi)) e = snap::invalid("key group outside the blob's key-group range");
    if (!e) e = snap::group(blob, hd, kg - hd.kg_lo, part);
    if (e) return e;
    snap::Writer w;
    w.begin_group();
    const int64_t n = part.left();
    w.bytes(part.take(n), n);
    hd.kg_lo = hd.kg_hi = kg;
    if (w.finish(hd, out, cap, out_len)) return snap::Err{GW_E_OUTPUT_FULL, "slice buffer too small"};
    return snap::Err{};
}

// Calls f(p, big_endian) for the key field of every entry, merging-set key and timer of a
// version 2-4 blob; false for a corrupt blob.
template <class F>
inline bool each_key(const uint8_t* b, int64_t len, F&& f) {
    snap::Header hd;
    snap::Cursor c;
    if (snap::open(b, len, 2, snap::kMaxVersion, hd, c)) return false;
    if (hd.version < 4) {  // fixed entries, key first
        while (const uint8_t* p = c.take(snap::entry_unit(hd))) f(p, false);
        return true;
    }
    if (hd.assigner == GW_COUNT_TUMBLING) {
        auto keys = [&](snap::Entries s) {
            for (int32_t i = 0; i < s.n; ++i) f(s[i] + snap::kCountKeyAt, true);
        };
        return !snap::walk_count_windows(hd, c, keys, keys);
    }
    return !snap::walk_windows(
        hd, c, [&](const uint8_t* p) { f(p + snap::kStateKeyAt, true); },
        [&](const uint8_t* head, int32_t, const uint8_t*) { f(head, true); },
        [&](const uint8_t* t) { f(t + snap::kTimerKeyAt, true); }, [] {});
}
// Calls f(payload field, big_endian = true, window end) for every entry of a first-element
// blob; false for a corrupt blob or one without payloads.
template <class F>
inline bool each_payload(const uint8_t* b, int64_t len, F&& f) {
    snap::Header hd;
    snap::Cursor c;
    if (snap::open(b, len, 4, 4, hd, c) || !(hd.flags & snap::kFirstElement)) return false;
    const int64_t at = snap::state_payload_at(hd);
    return !snap::walk_windows(
        hd, c, [&](const uint8_t* p) { f(p + at, true, snap::state_end(p)); }, snap::NoSets{}, [](const uint8_t*) {}, [] {});
}

inline int64_t word_at(const uint8_t* p, bool be) {
    int64_t k;
    memcpy(&k, p, 8);
    return be ? snap::get64(p) : k;
}
// The sorted distinct values into out[cap] (null: only their number *n).
inline snap::Err distinct(std::vector<int64_t>& v, int64_t* out, int64_t cap, int64_t* n, const char* too_small) {
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    *n = (int64_t)v.size();
    if (!out) return snap::Err{};
    if (cap < *n) return snap::Err{GW_E_OUTPUT_FULL, too_small};
    if (!v.empty()) memcpy(out, v.data(), v.size() * 8);
    return snap::Err{};
}
// Checks the table from[] -> to[] (present, ascending); -> f(p, be, ...) that maps the word at p.
inline auto remapper(const int64_t* from, const int64_t* to, int64_t n, const char* null_map, const char* unsorted,
                     snap::Err& e) {
    if (n < 0 || (n > 0 && (!from || !to))) e = snap::invalid(null_map);
    for (int64_t i = 1; !e && i < n; ++i)
        if (from[i] <= from[i - 1]) e = snap::invalid(unsorted);
    return [=](const uint8_t* cp, bool be, int64_t = 0) {
        uint8_t* p = const_cast<uint8_t*>(cp);
        const int64_t* it = std::lower_bound(from, from + n, word_at(p, be));
        if (it == from + n || *it != word_at(p, be)) return;
        const int64_t v = to[it - from];
        if (!be) memcpy(p, &v, 8);
        for (int i = 0; be && i < 8; ++i) p[i] = (uint8_t)((uint64_t)v >> (56 - 8 * i));
    };
}

inline snap::Err keys(const void* blob, int64_t len, int64_t* out, int64_t cap, int64_t* n) {
    std::vector<int64_t> ks;
    if (!each_key((const uint8_t*)blob, len, [&](const uint8_t* p, bool be) { ks.push_back(word_at(p, be)); }))
        return snap::invalid("corrupt snapshot blob");
    return distinct(ks, out, cap, n, "key buffer too small");
}
inline snap::Err remap_keys(void* blob, int64_t len, const int64_t* from, const int64_t* to, int64_t n) {
    snap::Err e;
    auto map = remapper(from, to, n, "null key map", "remap keys: from[] not ascending", e);
    if (!e && !each_key((const uint8_t*)blob, len, map)) e = snap::invalid("corrupt snapshot blob");
    return e;
}
inline snap::Err payloads(const void* blob, int64_t len, int64_t* out, int64_t cap, int64_t* n, int64_t* max_window_end) {
    std::vector<int64_t> ps;
    int64_t mx = INT64_MIN;
    if (!each_payload((const uint8_t*)blob, len, [&](const uint8_t* p, bool, int64_t e) {
            ps.push_back(snap::get64(p));
            mx = std::max(mx, e);
        }))
        return snap::invalid("not a first-element snapshot blob");
    if (max_window_end) *max_window_end = mx;
    return distinct(ps, out, cap, n, "payload buffer too small");
}
inline snap::Err remap_payloads(void* blob, int64_t len, const int64_t* from, const int64_t* to, int64_t n) {
    snap::Err e;
    auto map = remapper(from, to, n, "null payload map", "remap payloads: from[] not ascending", e);
    if (!e && !each_payload((const uint8_t*)blob, len, map)) e = snap::invalid("not a first-element snapshot blob");
    return e;
}

}  // namespace ckpt
}  // namespace gw
