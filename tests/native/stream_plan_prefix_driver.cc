// stream_plan_prefix_driver.cc -- the slotted codec stream's host-only planner (csrc/stream_plan.h) with rows that carry a
// reference prefix (streamed voice-clone rows), for tests/test_clone_stream_plan.py. Reads from stdin, any number of cases:
//   chunk window lookahead max_frames slots burst n_reqs  prefix_0 count_0 .. prefix_{n-1} count_{n-1}
// and writes per case
//   case
//   probe <k> <f0> <w0> <wlen> <take> <emit>                   what request 0 alone is given while it has NO generated frame
//   admit <slot> <request>                                     a request takes a slot (the row is reset with its prefix)
//   push <avail_0> <final_0> .. per slot                        a step of the schedule: generated frames and final flag per slot
//   pass                                                       one pass of the stream ...
//   row <slot> <request> <k> <f0> <w0> <wlen> <take> <emit>    ... and every row taking part in it
//   end
#include <cstdio>
#include <vector>

#include "stream_plan.h"

int main() {
    int C, W, L, F, slots, burst, n;
    while (std::scanf("%d %d %d %d %d %d %d", &C, &W, &L, &F, &slots, &burst, &n) == 7) {
        std::vector<int32_t> prefix((size_t)n), counts((size_t)n);
        for (int i = 0; i < n; ++i)
            if (std::scanf("%d %d", &prefix[(size_t)i], &counts[(size_t)i]) != 2) return 2;
        q3::SlotPlanCfg cfg;
        cfg.rows = slots; cfg.chunk = C; cfg.window = W; cfg.lookahead = L; cfg.max_frames = F;
        std::vector<q3::RowPlan> rows;
        std::printf("case\n");
        {
            q3::SlotPlanCfg one = cfg;
            one.rows = 1;
            q3::SlotPlanner pl;
            pl.open(one);
            pl.reset_row(0, prefix[0]);
            const int avail = 0;
            const uint8_t fin = 0;
            for (int guard = 0; guard < 1 << 20 && pl.plan_pass(&avail, &fin, rows) > 0; ++guard)
                std::printf("probe %d %d %d %d %d %d\n", rows[0].k, rows[0].f0, rows[0].w0, rows[0].wlen, rows[0].take, rows[0].emit);
        }
        q3::SlotPlanner pl;
        pl.open(cfg);
        q3::replay_queue_schedule(
            counts.data(), n, slots, burst,
            [&](int s, int r) {
                pl.reset_row(s, prefix[(size_t)r]);
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
                        if (p.part) std::printf("row %d %d %d %d %d %d %d %d\n", s, req[s], p.k, p.f0, p.w0, p.wlen, p.take, p.emit);
                    }
                }
            });
        std::printf("end\n");
    }
    return 0;
}
