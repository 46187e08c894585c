// Driver of tests/test_formant_plan.py: csrc/formant_plan.h as a stand-alone program (no HIP include path).
//   levinson R A              -> file R holds P + 1 float32 (lag-windowed autocorrelation); a[0..P] go to file A; prints 1, or 0
//                                when a fallback branch was taken
//   analyse HP N HIST X C E   -> file X holds HIST + N float32 mid samples (HIST of them in front of the row);
//                                formant_analyse_whiten; coef [hops][P] goes to file C, e [N] to file E; prints hops and, per hop,
//                                1 or 0 (0: a fallback)
//   synth HO N PIECE EP C Z [S_IN] [S_OUT]
//                             -> file EP holds N float32, file C the coefficients [ceil(N / HO)][P]; formant_synthesise in pieces
//                                of PIECE samples (a multiple of HO, or 0: one piece) with the state handed on; z (unclipped)
//                                goes to file Z. S_IN ("-": zeros) / S_OUT: the state in front / behind. Prints N
//   shift HP N X Y            -> file X holds N float32 at 24 kHz; formant_shift_reference; the result goes to file Y; prints its
//                                length
//   causal HP HO N X Y        -> the decoder's tail at 24 kHz on file X (N float32, whole 480-sample hops): the causal stretch at
//                                HP (none when HP == 480), analyse + whiten, the causal FIR HP -> HO unclipped, synthesise at HO
//                                samples per hop, clipped to [-1, 1]; the result goes to file Y; prints its length
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "formant_plan.h"

static int fail(const char* what) {
    std::fprintf(stderr, "formant_plan_driver: %s\n", what);
    return 2;
}

static bool read_floats(const char* path, std::vector<float>& v) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    const size_t got = v.empty() ? 0 : std::fread(v.data(), 4, v.size(), f);
    std::fclose(f);
    return got == v.size();
}

static bool write_floats(const char* path, const std::vector<float>& v) {
    FILE* f = std::fopen(path, "wb");
    if (!f) return false;
    const size_t put = v.empty() ? 0 : std::fwrite(v.data(), 4, v.size(), f);
    return std::fclose(f) == 0 && put == v.size();
}

int main(int argc, char** argv) {
    if (argc < 2) return fail("no mode");
    const std::string mode = argv[1];
    constexpr int P = q3::kFormantOrder;
    if (mode == "levinson") {
        if (argc != 4) return fail("levinson takes R A");
        std::vector<float> r(size_t(P + 1)), a(size_t(P + 1));
        if (!read_floats(argv[2], r)) return fail("short input");
        const bool ok = q3::formant_levinson(r.data(), a.data());
        if (!write_floats(argv[3], a)) return fail("short output");
        std::printf("%d\n", ok ? 1 : 0);
        return 0;
    }
    if (mode == "analyse") {
        if (argc != 8) return fail("analyse takes HP N HIST X C E");
        const int hp = std::atoi(argv[2]);
        const long n = std::atol(argv[3]), hist = std::atol(argv[4]);
        if (hp < q3::kStretchHsMin || hp > q3::kStretchHsMax || n < 0 || n > (1L << 24) || hist < 0 || hist > (1L << 20)) return fail("arguments out of range");
        std::vector<float> x(size_t(hist + n));
        if (!read_floats(argv[5], x)) return fail("short input");
        const q3::FormantPlan fp = q3::make_formant_plan(hp);
        const long hops = (n + hp - 1) / hp;
        std::vector<float> coef(size_t(hops) * P), e((size_t)(n));
        q3::formant_analyse_whiten(fp, x.data() + hist, n, hist, coef.data(), e.data());
        if (!write_floats(argv[6], coef) || !write_floats(argv[7], e)) return fail("short output");
        std::printf("%ld", hops);
        float a[P + 1];
        for (long h = 0; h < hops; ++h) std::printf(" %d", q3::formant_analyse(fp, x.data() + hist, n, hist, h, a) ? 1 : 0);
        std::printf("\n");
        return 0;
    }
    if (mode == "synth") {
        if (argc < 8 || argc > 10) return fail("synth takes HO N PIECE EP C Z [S_IN] [S_OUT]");
        const int ho = std::atoi(argv[2]);
        const long n = std::atol(argv[3]), piece = std::atol(argv[4]);
        if (ho < 1 || n < 0 || n > (1L << 24) || piece < 0 || piece % ho != 0) return fail("arguments out of range");
        const long hops = (n + ho - 1) / ho;
        std::vector<float> ep((size_t)(n)), coef(size_t(hops) * P), z((size_t)(n)), state(size_t(P), 0.0f);
        if (!read_floats(argv[5], ep) || !read_floats(argv[6], coef)) return fail("short input");
        if (argc >= 9 && std::strcmp(argv[8], "-") != 0 && !read_floats(argv[8], state)) return fail("short state");
        const long step = piece ? piece : (n ? n : 1);
        for (long s = 0; s < n; s += step) {
            const long m = s + step < n ? step : n - s;
            q3::formant_synthesise(ep.data() + s, m, ho, coef.data() + (s / ho) * P, state.data(), z.data() + s);
        }
        if (!write_floats(argv[7], z)) return fail("short output");
        if (argc == 10 && !write_floats(argv[9], state)) return fail("short output");
        std::printf("%ld\n", n);
        return 0;
    }
    if (mode == "shift") {
        if (argc != 6) return fail("shift takes HP N X Y");
        const int hp = std::atoi(argv[2]);
        const long n = std::atol(argv[3]);
        if (hp < q3::kStretchHsMin || hp > q3::kStretchHsMax || n < 1 || n > (1L << 24)) return fail("arguments out of range");
        std::vector<float> x((size_t)(n));
        if (!read_floats(argv[4], x)) return fail("short input");
        const std::vector<float> y = q3::formant_shift_reference(hp, x.data(), n);
        if (!write_floats(argv[5], y)) return fail("short output");
        std::printf("%zu\n", y.size());
        return 0;
    }
    if (mode == "causal") {
        if (argc != 7) return fail("causal takes HP HO N X Y");
        const int hp = std::atoi(argv[2]), ho = std::atoi(argv[3]);
        const long n = std::atol(argv[4]);
        if (hp < q3::kStretchHsMin || hp > q3::kStretchHsMax || ho < q3::kStretchHsMin || ho > q3::kStretchHsMax || hp == ho || n < 1 ||
            n > (1L << 24) || n % q3::kStretchHa != 0)
            return fail("arguments out of range");
        std::vector<float> x((size_t)(n));
        if (!read_floats(argv[5], x)) return fail("short input");
        std::vector<float> mid = x;
        if (hp != q3::kStretchHa) {
            const q3::StretchPlan sp = q3::make_stretch_plan(hp);
            mid.assign(size_t(sp.out_len(n, true)), 0.0f);
            q3::stretch_reference(sp, x.data(), n, 0, true, nullptr, mid.data());
        }
        const long nm = long(mid.size()), hops = nm / hp;
        const q3::FormantPlan fp = q3::make_formant_plan(hp);
        std::vector<float> coef(size_t(hops) * P), e((size_t)(nm));
        q3::formant_analyse_whiten(fp, mid.data(), nm, 0, coef.data(), e.data());
        const q3::ResamplePlan rp = q3::make_resample_plan(hp, ho);
        std::vector<float> ep(size_t(rp.out_len(nm))), z(ep.size());
        if (long(ep.size()) != hops * ho) return fail("a hop in is not a hop out");
        q3::resample_reference(rp, e.data(), nm, 0, false, false, ep.data());
        q3::formant_synthesise(ep.data(), long(ep.size()), ho, coef.data(), nullptr, z.data());
        for (float& v : z) v = v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);
        if (!write_floats(argv[6], z)) return fail("short output");
        std::printf("%zu\n", z.size());
        return 0;
    }
    return fail("unknown mode");
}
