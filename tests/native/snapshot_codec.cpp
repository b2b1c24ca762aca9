// The checkpoint blob codec (flink_amd/csrc/gw_snapshot.h) on its own: reads a file of
// (int64 length, bytes) blobs and prints one line per blob -- "invalid", or
//   v<version> rt=<1: rebuilt through snap::Writer byte for byte> counts=<per key group
//   a:b:c, ...> keys=<sorted unique keys, ...>
// with a:b:c = state entries : merging window sets : timers (window layout), contents :
// counts : 0 (count-window layout), entries : 0 : 0 (fixed entries, by the offset table;
// "-" when that table is corrupt).  Every blob sits in a heap block of exactly its length,
// so the sanitizers see any read outside it.  tests/test_snapshot_codec.py.
#include <algorithm>
#include <cstdio>
#include <memory>
#include <string>

#include "gw_snapshot.h"

namespace snap = gw::snap;

static void line(const uint8_t* b, int64_t len) {
    snap::Header hd;
    snap::Cursor c;
    if (snap::open(b, len, 2, snap::kMaxVersion, hd, c)) {
        puts("invalid");
        return;
    }
    std::vector<int64_t> keys;
    std::string counts;
    auto group_counts = [&](int64_t x, int64_t y, int64_t z) {
        counts += (counts.empty() ? "" : ",") + std::to_string(x) + ":" + std::to_string(y) + ":" + std::to_string(z);
    };
    snap::Writer w;
    snap::Err e;
    bool rebuilt = true;
    if (hd.version < 4) {
        const int64_t unit = snap::entry_unit(hd);
        while (const uint8_t* p = c.take(unit)) {
            int64_t k;
            memcpy(&k, p, 8);
            keys.push_back(k);
        }
        for (int64_t g = 0; g < snap::num_key_groups(hd) && rebuilt; ++g) {
            snap::Cursor part;
            rebuilt = !snap::group(b, hd, g, part);
            if (!rebuilt) break;
            const int64_t n = part.left();
            w.begin_group();
            w.bytes(part.take(n), n);
            group_counts(n / unit, 0, 0);
        }
        if (!rebuilt) counts = "-";
    } else if (hd.assigner == GW_COUNT_TUMBLING) {
        int32_t contents = 0;
        e = snap::walk_count_windows(
            hd, c,
            [&](snap::Entries s) {
                for (int32_t i = 0; i < s.n; ++i) keys.push_back(snap::get64(s[i] + snap::kCountKeyAt));
                contents = s.n;
                w.begin_group();
                w.count(s.n);
                w.bytes(s[0], s.n * s.width);
            },
            [&](snap::Entries s) {
                for (int32_t i = 0; i < s.n; ++i) keys.push_back(snap::get64(s[i] + snap::kCountKeyAt));
                group_counts(contents, s.n, 0);
                w.count(s.n);
                w.bytes(s[0], s.n * s.width);
                w.count(0);
            });
    } else {
        const int64_t eb = snap::state_entry_bytes(hd), mh = snap::set_head_bytes(hd);
        std::vector<uint8_t> st, ms, tm;
        int32_t nms = 0;
        e = snap::walk_windows(
            hd, c,
            [&](const uint8_t* p) {
                keys.push_back(snap::state_key(p));
                st.insert(st.end(), p, p + eb);
            },
            [&](const uint8_t* head, int32_t n, const uint8_t* windows) {
                keys.push_back(snap::get64(head));
                ms.insert(ms.end(), head, head + mh);
                ms.insert(ms.end(), windows, windows + n * snap::kSetWindowBytes);
                nms++;
            },
            [&](const uint8_t* t) {
                keys.push_back(snap::timer_key(t));
                snap::put_timer(tm, snap::timer_time(t), snap::timer_key(t), snap::timer_start(t), snap::timer_end(t));
            },
            [&] {
                const int32_t nst = (int32_t)(st.size() / eb), ntm = (int32_t)(tm.size() / snap::kTimerBytes);
                group_counts(nst, nms, ntm);
                w.begin_group();
                w.section(nst, st);
                w.section(nms, ms);
                w.section(ntm, tm);
                st.clear();
                ms.clear();
                tm.clear();
                nms = 0;
            });
    }
    if (e) {
        puts("invalid");
        return;
    }
    if (rebuilt) {
        const std::vector<uint8_t> again = w.finish(hd);
        rebuilt = (int64_t)again.size() == len && memcmp(again.data(), b, (size_t)len) == 0;
    }
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    printf("v%u rt=%d counts=%s keys=", hd.version, (int)rebuilt, counts.c_str());
    for (size_t i = 0; i < keys.size(); ++i) printf(i ? ",%lld" : "%lld", (long long)keys[i]);
    puts("");
}

int main(int argc, char** argv) {
    FILE* f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
    if (!f) return 2;
    int64_t len;
    while (fread(&len, 8, 1, f) == 1) {
        std::unique_ptr<uint8_t[]> blob(new uint8_t[(size_t)len]);
        if (len && fread(blob.get(), (size_t)len, 1, f) != 1) return 2;
        line(blob.get(), len);
    }
    fclose(f);
    return 0;
}
