// request_speed_driver.cc -- csrc/request_speed_plan.h behind a command line, for tests/test_request_speed_host.py. No HIP
// include and no library: the header's arithmetic must stay host-only.
//   info  <speed> <hops> <L> <M> <handle_hs>   ->  "hs spf mid_spf max_spf max_mid_spf"   (hs 0: refused)
//   place <L> <M> <frames_per_row> <hs...>     ->  per row "first one_past_last" of its samples: the rows lie packed at the
//                                                   start of their parts and no two overlap (checked here, exit 3 otherwise)
//   fade  <hs>                                  ->  "offset" and the table's words as the all-hops table holds them, in hex
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "request_speed_plan.h"

using namespace q3;

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string cmd = argv[1];
    if (cmd == "info" && argc == 7) {
        RequestSpeedPlan p;
        p.hops_per_frame = std::atoi(argv[3]);
        p.L = std::atoi(argv[4]);
        p.M = std::atoi(argv[5]);
        p.handle_hs = std::atoi(argv[6]);
        const int hs = p.hs_of(float(std::strtod(argv[2], nullptr)));
        std::printf("%d %d %d %d %d\n", hs, hs ? p.spf(hs) : 0, hs ? p.mid_spf(hs) : 0, p.max_spf(), p.max_mid_spf());
        return 0;
    }
    if (cmd == "place" && argc >= 6) {
        RequestSpeedPlan p;
        p.L = std::atoi(argv[2]);
        p.M = std::atoi(argv[3]);
        const int F = std::atoi(argv[4]);
        std::vector<int> hs;
        for (int i = 5; i < argc; ++i) hs.push_back(std::atoi(argv[i]));
        // every sample of every row written once into one buffer of the advertised size
        std::vector<int> owner(size_t(hs.size()) * size_t(F) * size_t(p.max_spf()), -1);
        for (size_t b = 0; b < hs.size(); ++b) {
            const int64_t first = p.sample_at(int(b), F, hs[b], 0), end = p.sample_at(int(b), F, hs[b], F);
            for (int64_t i = first; i < end; ++i) {
                if (owner.at(size_t(i)) != -1) return 3;
                owner[size_t(i)] = int(b);
            }
            std::printf("%lld %lld\n", (long long)first, (long long)end);
        }
        return 0;
    }
    if (cmd == "fade" && argc == 3) {
        const int hs = std::atoi(argv[2]);
        const std::vector<float> all = make_fade_all();
        if (all.size() != kFadeAllFloats) return 3;
        std::printf("%zu\n", fade_all_offset(hs));
        for (int n = 0; n < kStretchHsMax; ++n) {
            uint32_t w;
            std::memcpy(&w, &all.at(fade_all_offset(hs) + size_t(n)), 4);
            std::printf("%08x ", w);
        }
        std::printf("\n");
        return 0;
    }
    return 2;
}
