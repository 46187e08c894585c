// stretch_plan.h -- the pitch-preserving time stretch of the codec tail (speaking rate): its constants, the choice of the
// synthesis hop from a requested speed, and the arithmetic of one hop (kernels/stretch.hip evaluates exactly this, bit for
// bit). Host arithmetic alone: no HIP include, so tests/native/stretch_plan_driver.cc compiles it with a plain C++ compiler.
//
// WSOLA in crossfade form at the codec's 24 kHz. Analysis hop Ha = 480 (4 hops per 1920-sample frame), search radius
// Delta = 240, synthesis hop Hs an integer in [240, 960]: speed = Ha / Hs, 4 Hs samples leave per frame.
// Fade f[n] = 0.5 - 0.5 cos(pi (n + 0.5) / Hs), n = 0 .. Hs-1, in double, rounded to fp32.
// Delay D = max(0, Delta + Hs - Ha, Delta + 2 Hs - 2 Ha) in the causal form, 0 in the whole form.
// Hop m = 0, 1, ...:   cont[n] = x[p_{m-1} + Hs + n],   p_{-1} = -D - Hs,   d_0 = 0;
//   for m > 0 and every d in [-Delta, Delta]:  c(d) = sum_n cont[n] * x[m Ha + d - D + n]   (fp32, one accumulator, fmaf, n
//   ascending);  d_m: the candidates are visited in the order 0, -1, +1, -2, +2, ... and one replaces the best only when its c
//   is strictly greater (a NaN c counts as -infinity): ties go to the smallest |d|, then to the negative one;
//   p_m = m Ha + d_m - D;   y[m Hs + n] = fmaf(f[n], x[p_m + n] - cont[n], cont[n]).
// With this D hop m reads nothing beyond x[m Ha + Ha - 1]: output frame f depends on input up to the end of frame f alone.
// Causal form: x[j] for -hist <= j < 0 are the samples in front of the row (a stream's margin), everything else outside
// [0, n_in) is zero; floor(n_in / Ha) hops. Whole form: D = 0, reads outside [0, n_in) are zero, ceil(n_in / Ha) hops, the
// output is cut to ceil(n_in Hs / Ha) samples.
// A row's state between two calls is one int32: 0 -- nothing has been written yet (the next hop is hop 0), otherwise
// d_{m-1} + Delta + 1 of the last hop written. A row continued with that word and its samples in front equals the row in one
// piece.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

namespace q3 {

constexpr int kStretchHa = 480;      // analysis hop
constexpr int kStretchDelta = 240;   // search radius
constexpr int kStretchHsMin = 240;   // 2x
constexpr int kStretchHsMax = 960;   // 0.5x
constexpr int kStretchCandidates = 2 * kStretchDelta + 1;

inline int stretch_delay(int hs) {
    const int a = kStretchDelta + hs - kStretchHa, b = kStretchDelta + 2 * hs - 2 * kStretchHa;
    return a > b ? (a > 0 ? a : 0) : (b > 0 ? b : 0);
}
// the furthest a hop of the causal form reads in front of its own first input sample m Ha
inline int stretch_lookback(int hs) { return stretch_delay(hs) + kStretchDelta + (hs < kStretchHa ? kStretchHa - hs : 0); }

// The synthesis hop for a requested speed: the admissible integer in [240, 960] nearest to 480 / speed, ties toward 480.
// Admissible: a frame of `hops_per_frame` hops holds a whole number of samples behind an L / M resampler
// (hops_per_frame * Hs * L % M == 0; L == M == 1: every integer). 0: refused (speed outside [0.5, 2], NaN or infinite).
inline int stretch_choose_hs(double speed, int hops_per_frame = 4, int L = 1, int M = 1) {
    if (!(speed >= 0.5 && speed <= 2.0)) return 0;  // (a NaN fails both comparisons)
    const double want = double(kStretchHa) / speed;
    int best = 0;
    double best_dist = 0.0;
    for (int hs = kStretchHsMin; hs <= kStretchHsMax; ++hs) {
        if ((int64_t(hops_per_frame) * hs * L) % M != 0) continue;
        const double dist = std::fabs(double(hs) - want);
        const bool closer = best == 0 || dist < best_dist ||
                            (dist == best_dist && std::abs(hs - kStretchHa) < std::abs(best - kStretchHa));
        if (closer) {
            best = hs;
            best_dist = dist;
        }
    }
    return best;
}

struct StretchPlan {
    int hs = kStretchHa;
    int delay = 0;            // D of the causal form
    std::vector<float> fade;  // [hs]
    double speed() const { return double(kStretchHa) / double(hs); }
    // samples out for n_in samples in
    int64_t out_len(int64_t n_in, bool causal) const {
        return causal ? (n_in / kStretchHa) * hs : (n_in * hs + kStretchHa - 1) / kStretchHa;
    }
};

inline StretchPlan make_stretch_plan(int hs) {
    const double kPi = 3.14159265358979323846;
    StretchPlan p;
    p.hs = hs;
    p.delay = stretch_delay(hs);
    p.fade.resize(size_t(hs));
    for (int n = 0; n < hs; ++n) p.fade[size_t(n)] = float(0.5 - 0.5 * std::cos(kPi * (double(n) + 0.5) / double(hs)));
    return p;
}

// place of candidate d in the visiting order 0, -1, +1, -2, +2, ...
inline int stretch_order_key(int d) { return d < 0 ? -2 * d - 1 : 2 * d; }

// The definition, on the host: what kernels/stretch.hip computes, in the same order. y holds out_len(n_in, causal) samples.
// state (optional, causal form): the row's word, read on entry and written on exit. d_out (optional): d_m of every hop.
inline void stretch_reference(const StretchPlan& p, const float* x, int64_t n_in, int64_t hist, bool causal, int32_t* state, float* y,
                              std::vector<int>* d_out = nullptr) {
    const int Ha = kStretchHa, Hs = p.hs, Dl = kStretchDelta;
    const int64_t D = causal ? p.delay : 0;
    const int64_t lo = causal ? -hist : 0;
    const int64_t hops = causal ? n_in / Ha : (n_in + Ha - 1) / Ha;
    const int64_t n_out = p.out_len(n_in, causal);
    auto at = [&](int64_t j) { return (j >= lo && j < n_in) ? x[j] : 0.0f; };
    int32_t word = (causal && state) ? *state : 0;
    std::vector<float> cont((size_t)(Hs));
    for (int64_t m = 0; m < hops; ++m) {
        const bool first = word == 0;
        const int64_t c0 = first ? -D : (m - 1) * Ha + (word - Dl - 1) - D + Hs;  // p_{m-1} + Hs
        for (int n = 0; n < Hs; ++n) cont[size_t(n)] = at(c0 + n);
        int best_d = 0;
        if (!first) {
            float best_c = -INFINITY;
            for (int k = 0; k < kStretchCandidates; ++k) {
                const int d = (k & 1) ? -((k + 1) / 2) : k / 2;
                const int64_t s0 = m * Ha + d - D;
                float c = 0.0f;
                for (int n = 0; n < Hs; ++n) c = std::fmaf(cont[size_t(n)], at(s0 + n), c);
                if (c != c) c = -INFINITY;  // a NaN never wins
                if (k == 0 || c > best_c) {
                    best_c = c;
                    best_d = d;
                }
            }
        }
        const int64_t pm = m * Ha + best_d - D;
        for (int n = 0; n < Hs; ++n) {
            const int64_t o = m * Hs + n;
            if (o < n_out) y[o] = std::fmaf(p.fade[size_t(n)], at(pm + n) - cont[size_t(n)], cont[size_t(n)]);
        }
        word = best_d + Dl + 1;
        if (d_out) d_out->push_back(best_d);
    }
    if (causal && state) *state = word;
}

}  // namespace q3
