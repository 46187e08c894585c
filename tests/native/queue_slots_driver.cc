// queue_slots_driver.cc -- drives the slot loop's host-only bookkeeping (csrc/queue_slots.h) for tests/test_queue_slots.py.
// Reads from stdin, any number of cases:
//   burst_frames open_text n_slots
//   req since cap open starved  nframes fin starved_byte      (one line per slot: the slot, then what the burst's read-back holds)
// and writes per case
//   plan <running> <runnable> <burst>                          burst_length
//   after <starved_now> <starve_events> <starved_count>        after_burst with that burst, then starved_count
//   slot <since> <starved> <fin>                               every slot behind it (fin: the masked finished flag)
#include <cstdio>
#include <vector>

#include "queue_slots.h"

int main() {
    int burst_frames, open_text, S;
    while (std::scanf("%d %d %d", &burst_frames, &open_text, &S) == 3) {
        std::vector<q3::QSlot> sl((size_t)S);
        std::vector<int32_t> nframes((size_t)S);
        std::vector<uint8_t> fin((size_t)S), starved((size_t)S);
        for (int s = 0; s < S; ++s) {
            int open, st, f, sb;
            q3::QSlot& x = sl[(size_t)s];
            if (std::scanf("%d %d %d %d %d %d %d %d", &x.req, &x.since, &x.cap, &open, &st, &nframes[(size_t)s], &f, &sb) != 8) return 2;
            x.open = open != 0;
            x.starved = st != 0;
            fin[(size_t)s] = uint8_t(f);
            starved[(size_t)s] = uint8_t(sb);
        }
        const q3::BurstPlan p = q3::burst_length(sl, burst_frames);
        std::printf("plan %d %d %d\n", p.running, p.runnable, p.burst);
        const q3::StarveCount c = q3::after_burst(sl, p.burst, nframes.data(), fin.data(), starved.data(), open_text != 0);
        std::printf("after %d %d %d\n", c.starved_now, c.starve_events, q3::starved_count(sl));
        for (int s = 0; s < S; ++s) std::printf("slot %d %d %d\n", sl[(size_t)s].since, int(sl[(size_t)s].starved), int(fin[(size_t)s]));
    }
    return 0;
}
