// queue_slots.h -- the host's bookkeeping of the slot loop (engine_queue.cc): what a slot holds and the three decisions a burst
// boundary takes from it. Host-only, no HIP include: tests/native/queue_slots_driver.cc drives it without a GPU.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace q3 {

struct QSlot {
    int req = -1;      // request in this slot, -1: empty
    int since = 0;     // frame steps since its admission
    int reported = 0;  // TOKEN events delivered
    int np = 0;
    double t0 = 0;     // admission (host clock)
    int cap = 0;       // its max_frames
    // an open-text request: its text may still grow (open), its row waits for text on the device (starved)
    bool open = false, starved = false;
    int n_content = 0;  // content tokens so far
};

inline int starved_count(const std::vector<QSlot>& sl) {
    int n = 0;
    for (const QSlot& x : sl) n += x.req >= 0 && x.starved ? 1 : 0;
    return n;
}

// The next burst: no longer than the first running row's remaining frames (its cap ends it on time; an open-text row: the open
// cap, max_tokens, until its close). A starved row takes no frame step whatever is launched, and bounds nothing.
struct BurstPlan {
    int running = 0, runnable = 0, burst = 0;
};
inline BurstPlan burst_length(const std::vector<QSlot>& sl, int burst_frames) {
    BurstPlan p{0, 0, burst_frames};
    for (const QSlot& x : sl) {
        if (x.req < 0) continue;
        ++p.running;
        if (x.starved) continue;
        ++p.runnable;
        p.burst = std::min(p.burst, x.cap - x.since);
    }
    if (p.runnable > 0) p.burst = std::max(p.burst, 1);
    return p;
}

// What a burst left behind, read back per slot. A starved row carries the finished flag of a parked row (row_jobs.h
// frame_end_job) without having ended: neither the retirement nor the stream's last chunks may take it for a finished one, so
// its h_fin is cleared; it is an event if it ran before. A closed queue (!open_text) does not read h_starved. An open or
// starved row may have taken fewer steps than were launched: its `since` is its frame count.
struct StarveCount {
    int starved_now = 0, starve_events = 0;
};
inline StarveCount after_burst(std::vector<QSlot>& sl, int burst, const int32_t* h_nframes, uint8_t* h_fin, const uint8_t* h_starved,
                               bool open_text) {
    StarveCount c;
    for (size_t s = 0; s < sl.size(); ++s) {
        QSlot& x = sl[s];
        if (open_text) {
            const bool st = x.req >= 0 && h_starved[s] != 0;
            if (st) {
                h_fin[s] = 0;
                ++c.starved_now;
                if (!x.starved) ++c.starve_events;
            }
            x.starved = st;
        }
        if (x.req >= 0) x.since = x.open || x.starved ? h_nframes[s] : x.since + burst;
    }
    return c;
}

}  // namespace q3
