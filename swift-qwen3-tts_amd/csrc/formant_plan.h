// formant_plan.h -- the formant-preserving stage of a pitched handle (q3tts_load_opts_ex2.keep_formants): a spectral envelope
// per hop by linear prediction, taken off the signal in front of the pitch resampler and put back behind it, so the excitation
// is resampled (the pitch moves) while the envelope is applied at 24 kHz spacing on both sides (the formants stay). This header
// is the definition: its constants and three reference functions that kernels/formant.hip equals bit for bit. Host arithmetic
// alone: no HIP include, so tests/native/formant_plan_driver.cc compiles it with a plain C++ compiler (-ffp-contract=off: where a
// multiply and an add are written apart they round apart; every fused step is an explicit fmaf).
//
// Terms. The mid signal y is the resampler's input, Hp samples per hop (the stretch's output, or out_conv's signal when
// Hp == 480); the output signal has Ho samples per hop. Hop h covers mid samples [h Hp, (h+1) Hp) and output samples
// [h Ho, (h+1) Ho). y[j] for -hist <= j < 0 are the samples in front of the row (a stream's margin), everything else outside
// [0, n) is zero. A row of n mid samples has ceil(n / Hp) hops, the last one possibly short.
//
// formant_analyse, per (row, hop h), order P = 24:
//   w[i] = win[i] * y[(h-1) Hp + i], i = 0 .. 2 Hp - 1; win: the periodic Hann of 2 Hp samples, 0.5 - 0.5 cos(2 pi i / (2 Hp)),
//   in double, rounded to fp32.
//   Autocorrelation r[k], k = 0 .. P, in fp32, in the order of a workgroup of 256 = four waves of 64: lane t sums its own
//   products in one fmaf chain, v[t] = sum over i = t, t + 256, ... with i >= k, i ascending, of w[i] * w[i-k]; the 64 values of
//   a wave fold as a butterfly, v[l] += v[l + off] for off = 32, 16, 8, 4, 2, 1 (l < off); r[k] = (s0 + s1) + (s2 + s3) of the
//   four waves' sums.
//   r[k] *= lag[k]: the Gaussian lag window of 60 Hz, exp(-0.5 (2 pi 60 k / 24000)^2) in double, rounded to fp32 (lag[0] = 1);
//   r[0] *= 1 + 1e-4 (the fp32 constant 1.0001f).
//   Levinson-Durbin in fp32, a[0] = 1, err = r[0]; for i = 1 .. P:
//       p[j] = a[j] * r[i-j] for 1 <= j < i, 0 for every other j of 0 .. 31; p[l] += p[l + off] for off = 16, 8, 4, 2, 1
//       (l < off): the butterfly of half a wave;  acc = r[i] + p[0];  k = (-acc) / err;
//       a'[j] = fmaf(k, a[i-j], a[j]) for 1 <= j < i, a'[i] = k;  err = err * (1 - k * k)  (multiply, subtract, multiply).
//   Fallback, a[1..P] = 0 and the hop passes through unchanged: r[0] (windowed) not in [1e-9, FLT_MAX]; some |k| not below 1
//   (a NaN included); some err not above 0 (a NaN included). No bandwidth expansion. Hop h depends on y up to the end of hop h
//   alone.
// formant_whiten: e[n] = y[n] + sum_{k=1..P} a_h[k] y[n-k] for n in mid hop h: acc = y[n], then acc = fmaf(a[k], y[n-k], acc)
//   with k ascending.
// formant_synthesise: z[n] = e'[n] - sum_{k=1..P} a_h[k] z[n-k] for n in output hop h, e' the resampler's unclipped output:
//   acc = 0, then acc = fmaf(-a[k], z[n-k], acc) with k DESCENDING from P to 1, z[n] = e'[n] + acc; pcm[n] = clip(z[n], -1, 1)
//   and the recursion runs on the unclipped z. (The order is that of the transposed direct form, which a wave evaluates with
//   one lane shift per sample: s_k = fmaf(-a[k], z[n], s_{k+1}) in lane k, z[n+1] = e'[n+1] + s_1.) The row's state between
//   two calls is its last P values of z, oldest first; zeros in front of a row's start.
// Alignment: output hop h uses the coefficients of mid hop h. The causal FIR's K' mid samples of lag are left as they are.
// formant_shift_reference: the whole form -- the whole stretch at Hp, analyse + whiten, the centred FIR Hp -> 480, synthesise,
//   not clipped.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <vector>

#include "pitch_plan.h"
#include "resample_plan.h"
#include "stretch_plan.h"

namespace q3 {

constexpr int kFormantOrder = 24;             // P
constexpr int kFormantLanes = 256;            // the autocorrelation's partial sums: four waves of 64
constexpr double kFormantLagHz = 60.0;        // the Gaussian lag window
constexpr float kFormantR0Scale = 1.0001f;    // r[0] *= 1 + 1e-4
constexpr float kFormantR0Floor = 1.0e-9f;    // below it (or not finite): the hop passes through

struct FormantPlan {
    int hp = kStretchHa;
    std::vector<float> win;  // [2 hp]
    float lag[kFormantOrder + 1];
};

inline FormantPlan make_formant_plan(int hp) {
    const double kPi = 3.14159265358979323846;
    FormantPlan p;
    p.hp = hp;
    p.win.resize(size_t(2 * hp));
    for (int i = 0; i < 2 * hp; ++i) p.win[size_t(i)] = float(0.5 - 0.5 * std::cos(2.0 * kPi * double(i) / double(2 * hp)));
    for (int k = 0; k <= kFormantOrder; ++k) {
        const double t = 2.0 * kPi * kFormantLagHz * double(k) / double(kResampleNative);
        p.lag[k] = float(std::exp(-0.5 * t * t));
    }
    return p;
}

// r[0..P] of a windowed block w[0..n), in the order stated above
inline void formant_autocorr(const float* w, int n, float* r) {
    float v[kFormantLanes];
    for (int k = 0; k <= kFormantOrder; ++k) {
        for (int t = 0; t < kFormantLanes; ++t) {
            float acc = 0.0f;
            for (int i = t; i < n; i += kFormantLanes)
                if (i >= k) acc = std::fmaf(w[i], w[i - k], acc);
            v[t] = acc;
        }
        for (int off = 32; off >= 1; off >>= 1)
            for (int g = 0; g < kFormantLanes; g += 64)
                for (int l = 0; l < off; ++l) v[g + l] = v[g + l] + v[g + l + off];
        r[k] = (v[0] + v[64]) + (v[128] + v[192]);
    }
}

// Levinson-Durbin on r[0..P] (already lag-windowed): a[0..P], a[0] = 1. false: a fallback branch was taken, a[1..P] = 0.
inline bool formant_levinson(const float* r, float* a) {
    constexpr int P = kFormantOrder;
    a[0] = 1.0f;
    for (int j = 1; j <= P; ++j) a[j] = 0.0f;
    if (!(r[0] >= kFormantR0Floor && r[0] <= FLT_MAX)) return false;
    float err = r[0];
    float cur[32], p[32];
    for (int j = 0; j < 32; ++j) cur[j] = 0.0f;
    bool ok = true;
    for (int i = 1; i <= P && ok; ++i) {
        for (int j = 0; j < 32; ++j) p[j] = (j >= 1 && j < i) ? cur[j] * r[i - j] : 0.0f;
        for (int off = 16; off >= 1; off >>= 1)
            for (int l = 0; l < off; ++l) p[l] = p[l] + p[l + off];
        const float acc = r[i] + p[0];
        const float k = (-acc) / err;
        if (!(std::fabs(k) < 1.0f)) ok = false;
        float nxt[32];
        for (int j = 0; j < 32; ++j) nxt[j] = (j >= 1 && j < i) ? std::fmaf(k, cur[i - j], cur[j]) : (j == i ? k : 0.0f);
        for (int j = 0; j < 32; ++j) cur[j] = nxt[j];
        const float kk = k * k;
        const float u = 1.0f - kk;
        err = err * u;
        if (!(err > 0.0f)) ok = false;
    }
    if (!ok) return false;
    for (int j = 1; j <= P; ++j) a[j] = cur[j];
    return true;
}

// a[0..P] of mid hop h of the row y (n samples, `hist` in front). false: the hop passes through (a[1..P] = 0).
inline bool formant_analyse(const FormantPlan& p, const float* y, int64_t n, int64_t hist, int64_t h, float* a) {
    const int N = 2 * p.hp;
    std::vector<float> w((size_t)(N));
    const int64_t j0 = (h - 1) * p.hp;
    for (int i = 0; i < N; ++i) {
        const int64_t j = j0 + i;
        w[size_t(i)] = p.win[size_t(i)] * ((j >= -hist && j < n) ? y[j] : 0.0f);
    }
    float r[kFormantOrder + 1];
    formant_autocorr(w.data(), N, r);
    for (int k = 0; k <= kFormantOrder; ++k) r[k] = r[k] * p.lag[k];
    r[0] = r[0] * kFormantR0Scale;
    return formant_levinson(r, a);
}

// e[n] for n in [n0, n1) with the coefficients a[0..P]
inline void formant_whiten(const float* y, int64_t n, int64_t hist, const float* a, int64_t n0, int64_t n1, float* e) {
    for (int64_t i = n0; i < n1; ++i) {
        float acc = y[i];
        for (int k = 1; k <= kFormantOrder; ++k) {
            const int64_t j = i - k;
            acc = std::fmaf(a[k], (j >= -hist && j < n) ? y[j] : 0.0f, acc);
        }
        e[i] = acc;
    }
}

// analyse + whiten of a whole row: coef [hops][P] (a[1..P] of every hop), e [n]
inline void formant_analyse_whiten(const FormantPlan& p, const float* y, int64_t n, int64_t hist, float* coef, float* e) {
    const int64_t hops = (n + p.hp - 1) / p.hp;
    float a[kFormantOrder + 1];
    for (int64_t h = 0; h < hops; ++h) {
        formant_analyse(p, y, n, hist, h, a);
        for (int k = 1; k <= kFormantOrder; ++k) coef[h * kFormantOrder + (k - 1)] = a[k];
        const int64_t n1 = (h + 1) * p.hp < n ? (h + 1) * p.hp : n;
        formant_whiten(y, n, hist, a, h * p.hp, n1, e);
    }
}

// z[0..n) from e'[0..n) at `ho` samples per hop with coef [hops][P]; state (optional): the row's last P values of z, oldest
// first, read on entry and written on exit. z is NOT clipped (the caller clips what it hands out).
inline void formant_synthesise(const float* ep, int64_t n, int ho, const float* coef, float* state, float* z) {
    constexpr int P = kFormantOrder;
    float past[P];  // past[P - k] = z[-k]
    for (int k = 0; k < P; ++k) past[k] = state ? state[k] : 0.0f;
    auto zat = [&](int64_t j) { return j >= 0 ? z[j] : past[P + j]; };
    for (int64_t i = 0; i < n; ++i) {
        const float* a = coef + (i / ho) * P;
        float acc = 0.0f;
        for (int k = P; k >= 1; --k) acc = std::fmaf(-a[k - 1], zat(i - k), acc);
        z[i] = ep[i] + acc;
    }
    if (state) {
        float nxt[P];
        for (int k = 0; k < P; ++k) nxt[k] = zat(n - P + k);
        for (int k = 0; k < P; ++k) state[k] = nxt[k];
    }
}

// The whole form on a 24 kHz buffer: the whole stretch at hp (none when hp == 480), analyse + whiten, the centred FIR
// hp -> 480, synthesise; not clipped. Returns ceil(ceil(n_in hp / 480) * L' / M') samples.
inline std::vector<float> formant_shift_reference(int hp, const float* x, int64_t n_in) {
    std::vector<float> mid(x, x + n_in);
    if (hp != kStretchHa) {
        const StretchPlan sp = make_stretch_plan(hp);
        mid.assign(size_t(sp.out_len(n_in, false)), 0.0f);
        stretch_reference(sp, x, n_in, 0, false, nullptr, mid.data());
    } else {
        return mid;
    }
    const int64_t n = int64_t(mid.size());
    const FormantPlan fp = make_formant_plan(hp);
    const int64_t hops = (n + hp - 1) / hp;
    std::vector<float> coef(size_t(hops) * kFormantOrder), e((size_t)(n));
    formant_analyse_whiten(fp, mid.data(), n, 0, coef.data(), e.data());
    const ResamplePlan rp = make_resample_plan(hp, kStretchHa);
    std::vector<float> ep(size_t(rp.out_len(n))), z(ep.size());
    resample_reference(rp, e.data(), n, 0, true, false, ep.data());
    formant_synthesise(ep.data(), int64_t(ep.size()), kStretchHa, coef.data(), nullptr, z.data());
    return z;
}

}  // namespace q3
