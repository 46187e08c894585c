// Driver of tests/test_pitch_plan.py: csrc/pitch_plan.h as a stand-alone program (no HIP include path).
//   choose SEMITONES SPEED HOPS L M    -> "status ho hp L' M' K' table_bytes delay_out effective_semitones"
//   hp HO SEMITONES                    -> pitch_choose_hp
//   plan IN OUT                        -> pitch_ratio against make_resample_plan and the output-order table against the plan's:
//                                         "L M K ok"
//   sweep HIST_FRAMES STRIDE SEED      -> every admissible (rate, Ho, Hp), Hp != Ho (STRIDE > 1: a seeded 1 / STRIDE of them):
//                                         "triples checked violations max_table_bytes max_K max_span_bytes" and, on the next
//                                         lines, the triples holding the maxima
//   shift HP IN OUT CAUSAL CLAMP N X Y -> file X holds N float32 samples at 24 kHz; stretch_reference at HP (skipped when
//                                         HP == 480) and resample_reference IN -> OUT behind it, both causal or both
//                                         whole / centred; the outputs go to file Y; prints their number
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pitch_plan.h"

static int fail(const char* what) {
    std::fprintf(stderr, "pitch_plan_driver: %s\n", what);
    return 2;
}

int main(int argc, char** argv) {
    if (argc < 2) return fail("no mode");
    const std::string mode = argv[1];
    if (mode == "choose") {
        if (argc != 7) return fail("choose takes SEMITONES SPEED HOPS L M");
        const float semi = std::strtof(argv[2], nullptr), speed = std::strtof(argv[3], nullptr);
        const int hops = std::atoi(argv[4]), L = std::atoi(argv[5]), M = std::atoi(argv[6]);
        if (hops < 1 || L < 1 || M < 1) return fail("geometry must be positive");
        const q3::PitchChoice c = q3::pitch_choose(semi, speed, hops, L, M);
        const q3::PitchRatio r = q3::pitch_ratio(c.hp, c.ho, L, M);
        std::printf("%d %d %d %d %d %d %lld %d %.17g\n", c.status, c.ho, c.hp, r.L, r.M, r.K, (long long)r.table_bytes(),
                    c.on() ? q3::pitch_delay_out_samples(c.hp, r) : 0, c.on() ? q3::pitch_effective_semitones(c.hp, c.ho) : 0.0);
        return 0;
    }
    if (mode == "hp") {
        if (argc != 4) return fail("hp takes HO SEMITONES");
        std::printf("%d\n", q3::pitch_choose_hp(std::atoi(argv[2]), std::strtof(argv[3], nullptr)));
        return 0;
    }
    if (mode == "plan") {
        if (argc != 4) return fail("plan takes IN OUT");
        const int in = std::atoi(argv[2]), out = std::atoi(argv[3]);
        if (in <= 0 || out <= 0) return fail("units must be positive");
        const q3::PitchRatio r = q3::pitch_ratio(in, out, 1, 1);
        const q3::ResamplePlan p = q3::make_resample_plan(in, out);
        const std::vector<float> t = q3::resample_table_output_order(p);
        bool ok = r.L == p.L && r.M == p.M && r.K == p.K && t.size() == p.tab.size();
        for (int64_t n = 0; ok && n < 3 * int64_t(p.L) + 5; ++n)  // as the kernel indexes it: column n mod L, phase n M mod L
            for (int i = 0; ok && i < p.taps(); ++i)
                ok = std::memcmp(&t[size_t(i) * p.L + size_t(n % p.L)], &p.tab[size_t(n * p.M % p.L) * p.taps() + i], 4) == 0;
        std::printf("%d %d %d %s\n", r.L, r.M, r.K, ok ? "ok" : "MISMATCH");
        return 0;
    }
    if (mode == "sweep") {
        if (argc != 5) return fail("sweep takes HIST_FRAMES STRIDE SEED");
        const int hist = std::atoi(argv[2]), stride = std::atoi(argv[3]);
        uint64_t rng = std::strtoull(argv[4], nullptr, 10) * 2862933555777941757ull + 3037000493ull;
        if (hist < 1 || stride < 1) return fail("sweep geometry");
        const int rates[] = {24000, 8000, 12000, 16000, 22050, 32000, 44100, 48000};
        const int hops = 4;
        long long triples = 0, checked = 0, bad = 0, max_tab = 0, max_span = 0;
        int max_k = 0, at_tab[3] = {0, 0, 0}, at_k[3] = {0, 0, 0}, at_span[3] = {0, 0, 0};
        for (int rate : rates) {
            const int g = q3::resample_detail::gcd(q3::kResampleNative, rate);
            const int L = rate / g, M = q3::kResampleNative / g;
            for (int ho = q3::kStretchHsMin; ho <= q3::kStretchHsMax; ++ho) {
                if ((int64_t(hops) * ho * L) % M != 0) continue;  // what stretch_choose_hs admits
                for (int hp = q3::kStretchHsMin; hp <= q3::kStretchHsMax; ++hp) {
                    if (hp == ho) continue;
                    ++triples;
                    rng = rng * 6364136223846793005ull + 1442695040888963407ull;
                    if (stride > 1 && (rng >> 33) % uint64_t(stride) != 0) continue;
                    ++checked;
                    const q3::PitchRatio r = q3::pitch_ratio(hp, ho, L, M);
                    const int64_t out_frame = int64_t(hops) * ho * L / M, in_frame = int64_t(hops) * hp;
                    const int64_t span = (int64_t(255) * r.M / r.L + 2 * int64_t(r.K) + 8 + 3) / 4 * 4 * 4;  // resample_ratio_lds_bytes
                    bool ok = out_frame % r.L == 0;                                     // phase 0 recurs at every frame
                    ok = ok && out_frame * r.M == in_frame * r.L;                       // a frame in is a frame out
                    ok = ok && (out_frame - 1) * r.M / r.L < in_frame;                  // q stays inside the frame
                    ok = ok && q3::stretch_lookback(hp) <= hist * hops * q3::kStretchHa;  // the margins
                    ok = ok && 2 * r.K - 1 <= hist * in_frame && 2 * r.K - 1 <= in_frame && 2 * r.K - 1 <= 407;
                    ok = ok && r.table_bytes() <= 939624 && r.K <= 204 && span <= 64 * 1024;
                    if (!ok) ++bad;
                    if (r.table_bytes() > max_tab) { max_tab = r.table_bytes(); at_tab[0] = rate; at_tab[1] = ho; at_tab[2] = hp; }
                    if (r.K > max_k) { max_k = r.K; at_k[0] = rate; at_k[1] = ho; at_k[2] = hp; }
                    if (span > max_span) { max_span = span; at_span[0] = rate; at_span[1] = ho; at_span[2] = hp; }
                }
            }
        }
        std::printf("%lld %lld %lld %lld %d %lld\n", triples, checked, bad, max_tab, max_k, max_span);
        std::printf("%d %d %d\n%d %d %d\n%d %d %d\n", at_tab[0], at_tab[1], at_tab[2], at_k[0], at_k[1], at_k[2], at_span[0], at_span[1], at_span[2]);
        return 0;
    }
    if (mode == "shift") {
        if (argc != 10) return fail("shift takes HP IN OUT CAUSAL CLAMP N X Y");
        const int hp = std::atoi(argv[2]), in = std::atoi(argv[3]), out = std::atoi(argv[4]);
        const bool causal = std::atoi(argv[5]) != 0, clamp = std::atoi(argv[6]) != 0;
        const long n = std::atol(argv[7]);
        if (hp < q3::kStretchHsMin || hp > q3::kStretchHsMax || in <= 0 || out <= 0 || n < 0 || n > (1L << 24)) return fail("arguments out of range");
        std::vector<float> x((size_t)(n));
        FILE* f = std::fopen(argv[8], "rb");
        if (!f) return fail("cannot open the input");
        const size_t got = x.empty() ? 0 : std::fread(x.data(), 4, x.size(), f);
        std::fclose(f);
        if (got != x.size()) return fail("short input");
        std::vector<float> mid = x;
        if (hp != q3::kStretchHa) {
            const q3::StretchPlan sp = q3::make_stretch_plan(hp);
            mid.assign(size_t(sp.out_len(n, causal)), 0.0f);
            q3::stretch_reference(sp, x.data(), n, 0, causal, nullptr, mid.data());
        }
        const q3::ResamplePlan p = q3::make_resample_plan(in, out);
        std::vector<float> y(size_t(p.out_len(int64_t(mid.size()))));
        q3::resample_reference(p, mid.data(), int64_t(mid.size()), 0, !causal, clamp, y.data());
        f = std::fopen(argv[9], "wb");
        if (!f) return fail("cannot open the output");
        const size_t put = y.empty() ? 0 : std::fwrite(y.data(), 4, y.size(), f);
        if (std::fclose(f) != 0 || put != y.size()) return fail("short output");
        std::printf("%zu\n", y.size());
        return 0;
    }
    return fail("unknown mode");
}
