// stream_plan_driver.cc -- replays the slotted codec stream's host-only planner (csrc/stream_plan.h) over a queue schedule and
// prints what it decides, for tests/test_stream_plan.py. Reads from stdin, any number of cases:
//   chunk window lookahead max_frames slots burst n_reqs  count_0 .. count_{n-1}
// and writes per case
//   case
//   admit <slot> <request>                              a request takes a slot (the row is reset)
//   push <avail_0> <final_0> .. per slot                 a step of the schedule: frames and final flag of every slot
//   pass                                                one pass of the stream ...
//   row <slot> <request> <k> <f0> <w0> <wlen> <take>    ... and every row taking part in it
//   end
#include <cstdio>
#include <vector>

#include "stream_plan.h"

int main() {
    int C, W, L, F, slots, burst, n;
    while (std::scanf("%d %d %d %d %d %d %d", &C, &W, &L, &F, &slots, &burst, &n) == 7) {
        std::vector<int32_t> counts((size_t)n);
        for (auto& c : counts)
            if (std::scanf("%d", &c) != 1) return 2;
        q3::SlotPlanCfg cfg;
        cfg.rows = slots; cfg.chunk = C; cfg.window = W; cfg.lookahead = L; cfg.max_frames = F;
        q3::SlotPlanner pl;
        pl.open(cfg);
        std::vector<q3::RowPlan> rows;
        std::printf("case\n");
        q3::replay_queue_schedule(
            counts.data(), n, slots, burst,
            [&](int s, int r) {
                pl.reset_row(s);
                std::printf("admit %d %d\n", s, r);
            },
            [&](const int* avail, const uint8_t* fin, const int* req) {
                std::printf("push");
                for (int s = 0; s < slots; ++s) std::printf(" %d %d", avail[s], int(fin[s]));
                std::printf("\n");
                while (pl.plan_pass(avail, fin, rows) > 0) {
                    std::printf("pass\n");
                    for (int s = 0; s < slots; ++s) {
                        const q3::RowPlan& p = rows[(size_t)s];
                        if (p.part) std::printf("row %d %d %d %d %d %d %d\n", s, req[s], p.k, p.f0, p.w0, p.wlen, p.take);
                    }
                }
            });
        std::printf("end\n");
    }
    return 0;
}
