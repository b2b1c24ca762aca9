// gw_valve.h — the watermark valve of an operator with several input channels: what Flink's
// StatusWatermarkValve does with the watermarks and watermark statuses of its channels (the
// minimum watermark over the active, aligned channels; idle channels do not hold it back).
// Plain host code; gw_runtime.cpp wraps it as the C ABI's gw_valve and keeps one per handle.
#pragma once
#include <stdint.h>

#include <vector>

namespace gw {

struct Valve {
    struct Channel {
        int64_t wm = INT64_MIN;
        bool active = true;
        bool aligned = true;  // its watermark counts towards the minimum
    };
    struct Out {
        bool has_wm = false, has_status = false;
        int64_t wm = 0;
        int32_t status = 0;  // 0 active, -1 idle
    };
    std::vector<Channel> ch;
    int64_t last_wm = INT64_MIN;
    bool idle = false;  // the last status emitted

    explicit Valve(int n) : ch((size_t)n) {}
    void reset() {
        for (Channel& c : ch) c = Channel();
        last_wm = INT64_MIN;
        idle = false;
    }

    void new_min(Out& o) {
        bool any = false;
        int64_t m = INT64_MAX;
        for (const Channel& c : ch)
            if (c.aligned) { any = true; if (c.wm < m) m = c.wm; }
        if (any && m > last_wm) {
            last_wm = m;
            o.has_wm = true;
            o.wm = m;
        }
    }

    Out watermark(int c, int64_t t) {
        Out o;
        Channel& x = ch[(size_t)c];
        if (idle || !x.active || t <= x.wm) return o;
        x.wm = t;
        if (!x.aligned && t >= last_wm) x.aligned = true;
        new_min(o);
        return o;
    }

    // st: 0 active, -1 idle (the caller has checked the value)
    Out status(int c, int32_t st) {
        Out o;
        Channel& x = ch[(size_t)c];
        if (st != 0 && x.active) {
            x.active = false;
            x.aligned = false;
            bool any_active = false;
            for (const Channel& k : ch) any_active = any_active || k.active;
            if (!any_active) {
                // the last channel to go idle held the watermark back: flush what the others reached
                if (x.wm == last_wm) {
                    int64_t m = INT64_MIN;
                    for (const Channel& k : ch) if (k.wm > m) m = k.wm;
                    if (m > last_wm) {
                        last_wm = m;
                        o.has_wm = true;
                        o.wm = m;
                    }
                }
                idle = true;
                o.has_status = true;
                o.status = -1;
            } else if (x.wm == last_wm) {
                new_min(o);
            }
        } else if (st == 0 && !x.active) {
            x.active = true;
            if (x.wm >= last_wm) x.aligned = true;
            if (idle) {
                idle = false;
                o.has_status = true;
                o.status = 0;
            }
        }
        return o;
    }
};

}  // namespace gw
