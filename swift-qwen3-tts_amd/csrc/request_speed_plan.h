// request_speed_plan.h -- a speaking rate per request (q3tts_request.speed on a handle loaded with request_speeds): what a
// request's speed becomes on a handle with output ratio L / M, how a row's samples lie in buffers sized for the slowest row,
// and the fade tables of every hop as the device holds them. Host arithmetic alone: no HIP include, so
// tests/native/request_speed_driver.cc compiles it with a plain C++ compiler.
//
// A request at speed s gets the synthesis hop stretch_choose_hs(s, hops_per_frame, L, M) -- the rule of the handle's own
// speed, so a request at s equals a handle loaded with speed = s. Hs = 480 is "off" for that row (a copy of the 24 kHz
// signal), whatever the handle's own speed. A row at hop Hs has hops_per_frame * Hs * L / M samples per frame; every buffer
// behind the tail is sized by the slowest case, Hs = 960, and a row's samples lie packed at the start of its part of it:
// frame f of row b starts at  b * frames_per_row * max_spf + f * spf_b.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "stretch_plan.h"

namespace q3 {

struct RequestSpeedPlan {
    int hops_per_frame = 4;  // 480-sample hops per codec frame
    int L = 1, M = 1;        // output rate / 24000, reduced
    int handle_hs = kStretchHa;  // the handle's own hop (480: its time stretch is off)

    // samples per frame at the output rate of a row at hop hs (exact: stretch_choose_hs admits no other hop)
    int spf(int hs) const { return int(int64_t(hops_per_frame) * hs * L / M); }
    int mid_spf(int hs) const { return hops_per_frame * hs; }  // behind the stretch, in front of the resampler
    int max_spf() const { return spf(kStretchHsMax); }
    int max_mid_spf() const { return mid_spf(kStretchHsMax); }
    // The hop of a request: speed 0 -- the handle's. 0: refused (outside [0.5, 2], NaN, infinite).
    int hs_of(float speed) const {
        if (speed == 0.0f) return handle_hs;
        return stretch_choose_hs(double(speed), hops_per_frame, L, M);
    }
    // first sample of frame f of row b in a buffer of frames_per_row frames per row
    int64_t sample_at(int b, int frames_per_row, int hs, int64_t f) const {
        return int64_t(b) * frames_per_row * max_spf() + f * spf(hs);
    }
};

// the fade tables of every hop in [240, 960], table Hs at (Hs - 240) * 960 (the tail of a shorter table is zero)
constexpr size_t kFadeAllFloats = size_t(kStretchHsMax - kStretchHsMin + 1) * kStretchHsMax;
inline size_t fade_all_offset(int hs) { return size_t(hs - kStretchHsMin) * kStretchHsMax; }
inline std::vector<float> make_fade_all() {
    std::vector<float> t(kFadeAllFloats, 0.0f);
    for (int hs = kStretchHsMin; hs <= kStretchHsMax; ++hs) {
        const StretchPlan p = make_stretch_plan(hs);
        for (int n = 0; n < hs; ++n) t[fade_all_offset(hs) + size_t(n)] = p.fade[size_t(n)];
    }
    return t;
}

}  // namespace q3
