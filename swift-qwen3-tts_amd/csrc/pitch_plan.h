// pitch_plan.h -- a pitch shift per handle at an unchanged duration (q3tts_load_opts_ex.pitch): which numbers the codec tail runs
// with. The definitions are stretch_plan.h (the time stretch) and resample_plan.h (the polyphase FIR); this header only chooses
// their parameters. Host arithmetic alone: no HIP include, so tests/native/pitch_plan_driver.cc compiles it with a plain C++
// compiler.
//
// semitones s in [-12, 12], rho = 2^(s / 12). Ho is the hop the handle would have had without a pitch: 480 without a speed,
// otherwise stretch_choose_hs(speed, hops, L, M) for the output rate L / M. Hp is the integer nearest to Ho * rho, ties toward
// Ho; outside [240, 960] the combination is refused, never clamped. Hp == Ho is off. Otherwise the time stretch runs with
// Hs = Hp (every 480-sample hop becomes Hp samples, pitch preserved; Hp == 480: no stretch stage at all) and ONE resampler
// takes Hp * M input samples to Ho * L output samples -- pitch and output rate together, make_resample_plan(Hp * M, Ho * L),
// which reduces by the gcd to L' / M' and puts the cutoff at 0.945 * min(1, L' / M') of the input Nyquist. Every frequency moves
// by Hp / Ho, the effective shift is 12 log2(Hp / Ho) semitones, and a frame of hops * Hp samples in front of the resampler
// yields hops * Ho * L / M samples: what the same handle without a pitch hands out.
// Phase 0 recurs at every frame: (hops Ho L / M) * M' = hops * Hp * L', so q = floor(n M' / L') stays inside the frame.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "resample_plan.h"
#include "stretch_plan.h"

namespace q3 {

constexpr float kPitchMaxSemitones = 12.0f;

// 0 is off; a NaN fails both comparisons
inline bool pitch_semitones_valid(float s) { return s >= -kPitchMaxSemitones && s <= kPitchMaxSemitones; }

// The hop in front of the resampler for the handle's hop `ho`: the integer nearest to ho * 2^(s / 12), ties toward ho.
// 0: refused (the pitch is not valid, or the integer lies outside [240, 960]).
inline int pitch_choose_hp(int ho, float semitones) {
    if (!pitch_semitones_valid(semitones) || ho < kStretchHsMin || ho > kStretchHsMax) return 0;
    const double want = double(ho) * std::pow(2.0, double(semitones) / 12.0);
    const double lo = std::floor(want), hi = std::ceil(want);
    const double dl = want - lo, dh = hi - want;
    double pick = dl < dh ? lo : hi;
    if (dl == dh) pick = std::fabs(lo - double(ho)) <= std::fabs(hi - double(ho)) ? lo : hi;
    const int hp = int(pick);
    return (hp >= kStretchHsMin && hp <= kStretchHsMax) ? hp : 0;
}

inline double pitch_effective_semitones(int hp, int ho) { return 12.0 * std::log2(double(hp) / double(ho)); }

// The one resampler behind the stretch: Hp * M in, Ho * L out, reduced. K as make_resample_plan computes it (the driver checks
// the two against each other); the table has L * 2K floats.
struct PitchRatio {
    int64_t in_units = 1, out_units = 1;  // what make_resample_plan is called with
    int L = 1, M = 1, K = 0;              // reduced up factor, down factor, half width
    int64_t table_bytes() const { return int64_t(L) * 2 * K * 4; }
};

inline PitchRatio pitch_ratio(int hp, int ho, int L, int M) {
    PitchRatio r;
    r.in_units = int64_t(hp) * M;
    r.out_units = int64_t(ho) * L;
    int64_t a = r.in_units, b = r.out_units;
    while (b) {
        const int64_t t = a % b;
        a = b;
        b = t;
    }
    r.L = int(r.out_units / a);
    r.M = int(r.in_units / a);
    const double s = kResampleRolloff * (r.L < r.M ? double(r.L) / double(r.M) : 1.0);
    r.K = int(std::ceil(kResampleZeroCrossings / s));
    return r;
}

// The plan's table as kernels/resample_ratio.hip reads it: output order, [2K][L], column c = n mod L holding the taps of phase
// (c * M) mod L (L and M are coprime: every phase has one column).
inline std::vector<float> resample_table_output_order(const ResamplePlan& p) {
    const int n = p.taps();
    std::vector<float> t(size_t(p.L) * size_t(n));
    for (int c = 0; c < p.L; ++c) {
        const int r = int(int64_t(c) * p.M % p.L);
        for (int i = 0; i < n; ++i) t[size_t(i) * size_t(p.L) + size_t(c)] = p.tab[size_t(r) * size_t(n) + size_t(i)];
    }
    return t;
}

struct PitchChoice {
    int status = 0;  // 0: fine; 1: pitch outside [-12, 12], NaN or infinite; 2: no synthesis hop for the speed; 3: no Hp in [240, 960]
    int ho = kStretchHa, hp = kStretchHa;
    bool on() const { return status == 0 && hp != ho; }
};

// speed 0 or 1: no speaking rate (Ho = 480); L / M: the handle's output rate over 24000, reduced
inline PitchChoice pitch_choose(float semitones, float speed, int hops_per_frame, int L, int M) {
    PitchChoice c;
    if (!pitch_semitones_valid(semitones)) {
        c.status = 1;
        return c;
    }
    if (speed != 0.0f && speed != 1.0f) {
        c.ho = stretch_choose_hs(double(speed), hops_per_frame, L, M);
        if (c.ho == 0) {
            c.status = 2;
            c.ho = c.hp = kStretchHa;
            return c;
        }
    }
    c.hp = c.ho;
    if (semitones == 0.0f) return c;
    c.hp = pitch_choose_hp(c.ho, semitones);
    if (c.hp == 0) {
        c.status = 3;
        c.hp = c.ho;
    }
    return c;
}

// The delay of a pitched handle in output samples: the stretch's D(Hp) 24 kHz samples are D * Hp / 480 samples in front of the
// resampler (0 when Hp == 480: no stretch stage), the causal FIR adds K; both go through L' / M':
//     ceil((D(Hp) * Hp / 480 + K) * L' / M')
inline int pitch_delay_out_samples(int hp, const PitchRatio& r) {
    const int64_t d = hp == kStretchHa ? 0 : stretch_delay(hp);
    const int64_t num = (d * hp + int64_t(kStretchHa) * r.K) * r.L, den = int64_t(kStretchHa) * r.M;
    return int((num + den - 1) / den);
}

}  // namespace q3
