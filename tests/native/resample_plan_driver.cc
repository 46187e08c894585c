// Driver of tests/test_resample_plan.py: csrc/resample_plan.h as a stand-alone program (no HIP include path).
//   table IN OUT                          -> "L M K" and one line of 2K taps per phase, as the bit patterns of the fp32 values
//   run IN OUT CENTRED HIST CLAMP N X Y   -> file X holds HIST + N float32 samples (the first HIST in front of the row);
//                                            resample_reference's ceil(N L / M) outputs go to file Y; prints their number
//   pairs                                 -> which of a grid of rate pairs resample_pair_supported accepts
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "resample_plan.h"

static int fail(const char* what) {
    std::fprintf(stderr, "resample_plan_driver: %s\n", what);
    return 2;
}

int main(int argc, char** argv) {
    if (argc < 2) return fail("no mode");
    const std::string mode = argv[1];
    if (mode == "pairs") {
        const int rates[] = {8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 96000};
        for (int a : rates)
            for (int b : rates)
                if (q3::resample_pair_supported(a, b)) std::printf("%d %d\n", a, b);
        return 0;
    }
    if (argc < 4) return fail("missing rates");
    const int in_rate = std::atoi(argv[2]), out_rate = std::atoi(argv[3]);
    if (in_rate <= 0 || out_rate <= 0) return fail("rates must be positive");
    const q3::ResamplePlan p = q3::make_resample_plan(in_rate, out_rate);
    if (mode == "table") {
        std::printf("%d %d %d\n", p.L, p.M, p.K);
        for (int r = 0; r < p.L; ++r) {
            for (int i = 0; i < p.taps(); ++i) {
                uint32_t bits;
                std::memcpy(&bits, &p.tab[size_t(r) * p.taps() + i], 4);
                std::printf("%08x%c", bits, i + 1 == p.taps() ? '\n' : ' ');
            }
        }
        return 0;
    }
    if (mode == "run") {
        if (argc != 10) return fail("run takes IN OUT CENTRED HIST CLAMP N X Y");
        const bool centred = std::atoi(argv[4]) != 0, clamp = std::atoi(argv[6]) != 0;
        const long hist = std::atol(argv[5]), n = std::atol(argv[7]);
        if (hist < 0 || n < 0 || n > (1L << 24) || hist > (1L << 24)) return fail("lengths out of range");
        std::vector<float> x(size_t(hist + n));
        FILE* f = std::fopen(argv[8], "rb");
        if (!f) return fail("cannot open the input");
        const size_t got = x.empty() ? 0 : std::fread(x.data(), 4, x.size(), f);
        std::fclose(f);
        if (got != x.size()) return fail("short input");
        std::vector<float> y(size_t(p.out_len(n)));
        q3::resample_reference(p, x.data() + hist, n, hist, centred, clamp, y.data());
        f = std::fopen(argv[9], "wb");
        if (!f) return fail("cannot open the output");
        const size_t put = y.empty() ? 0 : std::fwrite(y.data(), 4, y.size(), f);
        if (std::fclose(f) != 0 || put != y.size()) return fail("short output");
        std::printf("%zu\n", y.size());
        return 0;
    }
    return fail("unknown mode");
}
