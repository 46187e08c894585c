// stretch.hip -- the time stretch of stretch_plan.h on the device: the codec tail's speaking-rate stage (24 kHz in, 4 Hs samples
// per frame out) and, in whole form, q3tts_time_stretch.
// The chain d_{m-1} -> d_m is sequential per row, so one workgroup of 512 owns a row and walks its hops. Per hop it stages the
// search window (Hs + 2 Delta samples) and `cont` in LDS; thread t < 481 owns candidate d = t - Delta and sums its correlation
// in the defined order (one accumulator, fmaf, n ascending: neighbouring lanes read neighbouring LDS words, cont[n] is a
// broadcast); the pair (c, place in the visiting order) is reduced with wave shuffles and one LDS round. The order is total, so
// the reduction tree does not matter. Every output is one fmaf: nothing here depends on the launch geometry.
#include "../common.h"
#include "../codec_kernels.h"
#include "../stretch_plan.h"

namespace q3 {
namespace {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kWinMax = kStretchHsMax + 2 * kStretchDelta;  // 1440

// (c, key) of the better of two candidates: greater c, then the earlier place in the visiting order
__device__ __forceinline__ void take_better(float& c, int& key, float oc, int okey) {
    if (oc > c || (oc == c && okey < key)) {
        c = oc;
        key = okey;
    }
}

__global__ __launch_bounds__(kThreads) void stretch_kernel(StretchArgs a) {
    __shared__ float win[kWinMax];
    __shared__ float cont[kStretchHsMax];
    __shared__ float fade[kStretchHsMax];
    __shared__ float red_c[kWaves];
    __shared__ int red_k[kWaves];
    const int b = blockIdx.x, t = threadIdx.x;
    const int64_t n_in = int64_t(a.len[b]) * a.len_mul;
    if (n_in <= 0) return;  // a row of length 0 touches nothing, its state included
    constexpr int Ha = kStretchHa, Dl = kStretchDelta;
    // The hop is the row's own when the launch carries a table (uniform over the workgroup: one workgroup owns a row, so
    // its hop count, window length and loop bounds are scalars as before). Entry 0: the row speaks at speed 1 -- a copy.
    int Hs = a.hs, delay = a.delay;
    const float* fd = a.fade;
    if (a.hs_rows) {
        Hs = __builtin_amdgcn_readfirstlane(a.hs_rows[b]);
        if (Hs == 0) {
            const float* xc = a.x + int64_t(b) * a.x_bstride;
            float* yc = a.y + int64_t(b) * a.y_bstride;
            for (int64_t n = t; n < n_in; n += kThreads) yc[n] = xc[n];
            return;
        }
        if (Hs < kStretchHsMin || Hs > kStretchHsMax) return;  // (never: the host chose it; the LDS arrays end at 960)
        const int d1 = Dl + Hs - Ha, d2 = Dl + 2 * Hs - 2 * Ha;  // stretch_delay(Hs)
        delay = d1 > d2 ? (d1 > 0 ? d1 : 0) : (d2 > 0 ? d2 : 0);
        fd = a.fade_all + size_t(Hs - kStretchHsMin) * kStretchHsMax;
    }
    const int64_t D = a.causal ? delay : 0;
    const int64_t lo = a.causal ? -int64_t(a.hist) : 0;
    const int64_t hops = a.causal ? n_in / Ha : (n_in + Ha - 1) / Ha;
    const int64_t n_out = a.causal ? hops * Hs : (n_in * Hs + Ha - 1) / Ha;
    const float* x = a.x + int64_t(b) * a.x_bstride;
    float* y = a.y + int64_t(b) * a.y_bstride;
    for (int n = t; n < Hs; n += kThreads) fade[n] = fd[n];
    int word = a.state_in ? a.state_in[int64_t(b) * a.state_in_bstride] : 0;
    const int wlen = Hs + 2 * Dl;
    for (int64_t m = 0; m < hops; ++m) {
        const bool first = word == 0;
        const int64_t c0 = first ? -D : (m - 1) * Ha + (word - Dl - 1) - D + Hs;  // p_{m-1} + Hs
        const int64_t w0 = m * Ha - Dl - D;                                         // candidate d reads win[d + Delta + n]
        for (int n = t; n < Hs; n += kThreads) {
            const int64_t j = c0 + n;
            cont[n] = (j >= lo && j < n_in) ? x[j] : 0.f;
        }
        for (int i = t; i < wlen; i += kThreads) {
            const int64_t j = w0 + i;
            win[i] = (j >= lo && j < n_in) ? x[j] : 0.f;
        }
        __syncthreads();
        int best_d = 0;
        if (!first) {  // (uniform over the workgroup)
            float c = -INFINITY;
            int key = 0x7fffffff;
            if (t < kStretchCandidates) {
                const float* w = win + t;
                float acc = 0.f;
#pragma unroll 8
                for (int n = 0; n < Hs; ++n) acc = fmaf(cont[n], w[n], acc);
                c = acc != acc ? -INFINITY : acc;  // a NaN never wins
                const int d = t - Dl;
                key = d < 0 ? -2 * d - 1 : 2 * d;  // stretch_order_key: the place in 0, -1, +1, -2, +2, ...
            }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                const float oc = __shfl_xor(c, o, 64);
                const int ok = __shfl_xor(key, o, 64);
                take_better(c, key, oc, ok);
            }
            if ((t & 63) == 0) {
                red_c[t >> 6] = c;
                red_k[t >> 6] = key;
            }
            __syncthreads();
            c = red_c[0];
            key = red_k[0];
#pragma unroll
            for (int i = 1; i < kWaves; ++i) take_better(c, key, red_c[i], red_k[i]);
            best_d = (key & 1) ? -((key + 1) >> 1) : (key >> 1);
        }
        const float* px = win + best_d + Dl;  // x[p_m + n]
        const int64_t o0 = m * Hs;
        for (int n = t; n < Hs; n += kThreads)
            if (o0 + n < n_out) y[o0 + n] = fmaf(fade[n], px[n] - cont[n], cont[n]);
        word = best_d + Dl + 1;
        if (a.state_frames && t == 0 && (m + 1) % a.frame_hops == 0)
            a.state_frames[int64_t(b) * a.state_frames_bstride + (m / a.frame_hops) * a.state_frame_words] = word;
        __syncthreads();  // the next hop restages win / cont / red
    }
    if (a.state_out && t == 0) a.state_out[int64_t(b) * a.state_out_bstride] = word;
}

}  // namespace

void launch_stretch(const StretchArgs& a, hipStream_t st) {
    if (a.B <= 0) return;
    if (a.hs_rows) {
        Q3_CHECK(a.fade_all && a.causal && a.len_mul >= 1 && a.hist >= 0, 7, "internal error: time stretch geometry (per-row hops)");
    } else {
        Q3_CHECK(a.hs >= kStretchHsMin && a.hs <= kStretchHsMax && a.len_mul >= 1 && a.hist >= 0 && a.delay >= 0, 7,
                 "internal error: time stretch geometry");
        Q3_CHECK(!a.causal || a.delay == stretch_delay(a.hs), 7, "internal error: time stretch delay");
    }
    Q3_CHECK(!a.state_frames || (a.frame_hops >= 1 && a.state_frame_words >= 1), 7, "internal error: time stretch state layout");
    Q3_CHECK(a.B <= 0x7fffffff, 3, "Invalid input: too many rows in one time stretch");
    (void)hipGetLastError();  // the runtime's last-error slot is sticky: an earlier, handled failure must not be read as this launch's
    hipLaunchKernelGGL(stretch_kernel, dim3(unsigned(a.B)), dim3(kThreads), 0, st, a);
    Q3_HIP(hipGetLastError());
}

}  // namespace q3
