// resample_plan.h -- the polyphase FIR between 24 kHz and the other supported rates: which pairs exist, the filter's taps and
// the index arithmetic of one output sample (kernels/resample.hip evaluates exactly this). Host arithmetic alone: no HIP
// include, so tests/native/resample_plan_driver.cc compiles it with a plain C++ compiler.
//
// For in -> out Hz: g = gcd(in, out), L = out / g, M = in / g, s = 0.945 * min(1, L / M), half width K = ceil(16 / s) input
// samples, 2K taps per phase. Tap i (0 .. 2K-1) of phase r (0 .. L-1) belongs to k = i - K + 1 and sits at t = k - r / L:
//     g(t) = s * sinc(s t) * I0(8.6 * sqrt(1 - (t / K)^2)) / I0(8.6)   for |t| < K, otherwise 0,   sinc(x) = sin(pi x) / (pi x)
// evaluated in double, every phase normalised to sum 1 in double, then rounded to fp32.
// Output sample n has q = floor(n M / L) and r = (n M) mod L:
//     centred: y[n] = sum_i tab[r][i] * x[q - K + 1 + i]        causal: y[n] = sum_i tab[r][i] * x[q - 2K + 1 + i]
// The causal form is the centred one delayed by K input samples and reads nothing beyond x[q]. Samples outside the signal are
// zero, the output has ceil(n_in * L / M) samples, and the sum runs in fp32 with fmaf, one accumulator, i ascending.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

namespace q3 {

constexpr int kResampleNative = 24000;       // the codec's own rate: one side of every supported pair
constexpr double kResampleRolloff = 0.945;   // cutoff as a fraction of the lower rate's Nyquist frequency
constexpr double kResampleZeroCrossings = 16.0;
constexpr double kResampleBeta = 8.6;        // Kaiser window

inline bool resample_rate_supported(int rate) {
    switch (rate) {
        case 8000: case 12000: case 16000: case 22050: case 32000: case 44100: case 48000: return true;
        default: return false;
    }
}
// one side is 24000, the other one of the seven rates above (24000 -> 24000 is no resampling and is not a pair)
inline bool resample_pair_supported(int in_rate, int out_rate) {
    return (in_rate == kResampleNative && resample_rate_supported(out_rate)) ||
           (out_rate == kResampleNative && resample_rate_supported(in_rate));
}

struct ResamplePlan {
    int in_rate = 0, out_rate = 0;
    int L = 1, M = 1, K = 0;     // up factor, down factor, half width in input samples
    std::vector<float> tab;      // [L][2K]
    int taps() const { return 2 * K; }
    int64_t out_len(int64_t n_in) const { return (n_in * L + M - 1) / M; }
};

namespace resample_detail {
inline int gcd(int a, int b) {
    while (b) {
        const int t = a % b;
        a = b;
        b = t;
    }
    return a;
}
inline double bessel_i0(double x) {  // power series: every term positive, converged to double well before 64 terms at x <= 8.6
    const double q = x * x / 4.0;
    double sum = 1.0, term = 1.0;
    for (int k = 1; k < 64; ++k) {
        term *= q / (double(k) * double(k));
        sum += term;
    }
    return sum;
}
}  // namespace resample_detail

// in_rate, out_rate > 0; whether the pair is one the engine offers is resample_pair_supported's business
inline ResamplePlan make_resample_plan(int in_rate, int out_rate) {
    using namespace resample_detail;
    const double kPi = 3.14159265358979323846;
    ResamplePlan p;
    p.in_rate = in_rate;
    p.out_rate = out_rate;
    const int g = gcd(in_rate, out_rate);
    p.L = out_rate / g;
    p.M = in_rate / g;
    const double s = kResampleRolloff * (p.L < p.M ? double(p.L) / double(p.M) : 1.0);
    p.K = int(std::ceil(kResampleZeroCrossings / s));
    const int n = 2 * p.K;
    const double i0b = bessel_i0(kResampleBeta);
    p.tab.resize(size_t(p.L) * n);
    std::vector<double> row((size_t)(n));
    for (int r = 0; r < p.L; ++r) {
        double sum = 0.0;
        for (int i = 0; i < n; ++i) {
            const double t = double(i - p.K + 1) - double(r) / double(p.L);
            double v = 0.0;
            if (std::fabs(t) < double(p.K)) {
                const double x = s * t, u = t / double(p.K);
                const double sinc = x == 0.0 ? 1.0 : std::sin(kPi * x) / (kPi * x);
                v = s * sinc * bessel_i0(kResampleBeta * std::sqrt(1.0 - u * u)) / i0b;
            }
            row[size_t(i)] = v;
            sum += v;
        }
        for (int i = 0; i < n; ++i) p.tab[size_t(r) * n + i] = float(row[size_t(i)] / sum);
    }
    return p;
}

// The definition, on the host: what kernels/resample.hip computes, in the same order. x[j] for -hist <= j < 0 are the samples
// in front of the row (causal streams); everything else outside [0, n_in) is zero. y holds out_len(n_in) samples.
inline void resample_reference(const ResamplePlan& p, const float* x, int64_t n_in, int64_t hist, bool centred, bool clamp, float* y) {
    const int n = p.taps();
    const int64_t n_out = p.out_len(n_in);
    for (int64_t o = 0; o < n_out; ++o) {
        const int64_t q = o * p.M / p.L;
        const int r = int(o * p.M % p.L);
        const int64_t j0 = q - (centred ? p.K : 2 * p.K) + 1;
        float acc = 0.0f;
        for (int i = 0; i < n; ++i) {
            const int64_t j = j0 + i;
            const float v = (j >= -hist && j < n_in) ? x[j] : 0.0f;
            acc = std::fmaf(p.tab[size_t(r) * n + i], v, acc);
        }
        if (clamp) acc = acc < -1.0f ? -1.0f : (acc > 1.0f ? 1.0f : acc);  // (a NaN stays a NaN)
        y[o] = acc;
    }
}

}  // namespace q3
