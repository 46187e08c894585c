// Driver of tests/test_stretch_plan.py: csrc/stretch_plan.h as a stand-alone program (no HIP include path).
//   choose SPEED HOPS L M               -> the synthesis hop stretch_choose_hs picks (0: refused); SPEED as strtod reads it
//   plan HS                             -> "D lookback" and one line with the Hs fade values as fp32 bit patterns
//   run HS CAUSAL HIST STATE N X Y      -> file X holds HIST + N float32 samples (the first HIST in front of the row);
//                                          stretch_reference's outputs go to file Y; prints their number, the state word
//                                          behind the row and d of every hop
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "stretch_plan.h"

static int fail(const char* what) {
    std::fprintf(stderr, "stretch_plan_driver: %s\n", what);
    return 2;
}

int main(int argc, char** argv) {
    if (argc < 2) return fail("no mode");
    const std::string mode = argv[1];
    if (mode == "choose") {
        if (argc != 6) return fail("choose takes SPEED HOPS L M");
        const int hops = std::atoi(argv[3]), L = std::atoi(argv[4]), M = std::atoi(argv[5]);
        if (hops < 1 || L < 1 || M < 1) return fail("HOPS, L and M must be positive");
        std::printf("%d\n", q3::stretch_choose_hs(std::strtod(argv[2], nullptr), hops, L, M));
        return 0;
    }
    if (argc < 3) return fail("missing HS");
    const int hs = std::atoi(argv[2]);
    if (hs < q3::kStretchHsMin || hs > q3::kStretchHsMax) return fail("HS out of range");
    const q3::StretchPlan p = q3::make_stretch_plan(hs);
    if (mode == "plan") {
        std::printf("%d %d\n", p.delay, q3::stretch_lookback(hs));
        for (int n = 0; n < hs; ++n) {
            uint32_t bits;
            std::memcpy(&bits, &p.fade[size_t(n)], 4);
            std::printf("%08x%c", bits, n + 1 == hs ? '\n' : ' ');
        }
        return 0;
    }
    if (mode == "run") {
        if (argc != 9) return fail("run takes HS CAUSAL HIST STATE N X Y");
        const bool causal = std::atoi(argv[3]) != 0;
        const long hist = std::atol(argv[4]), n = std::atol(argv[6]);
        int32_t state = int32_t(std::atoi(argv[5]));
        if (hist < 0 || n < 0 || n > (1L << 24) || hist > (1L << 24)) return fail("lengths out of range");
        if (state < 0 || state > q3::kStretchCandidates) return fail("state word out of range");
        std::vector<float> x(size_t(hist + n));
        FILE* f = std::fopen(argv[7], "rb");
        if (!f) return fail("cannot open the input");
        const size_t got = x.empty() ? 0 : std::fread(x.data(), 4, x.size(), f);
        std::fclose(f);
        if (got != x.size()) return fail("short input");
        std::vector<float> y(size_t(p.out_len(n, causal)));
        std::vector<int> d;
        q3::stretch_reference(p, x.data() + hist, n, hist, causal, &state, y.data(), &d);
        f = std::fopen(argv[8], "wb");
        if (!f) return fail("cannot open the output");
        const size_t put = y.empty() ? 0 : std::fwrite(y.data(), 4, y.size(), f);
        if (std::fclose(f) != 0 || put != y.size()) return fail("short output");
        std::printf("%zu %d", y.size(), int(state));
        for (int v : d) std::printf(" %d", v);
        std::printf("\n");
        return 0;
    }
    return fail("unknown mode");
}
