// formant.hip -- the formant-preserving stage of a pitched handle (formant_plan.h is the definition; both kernels equal it bit
// for bit): formant_analyse_kernel in front of the pitch resampler, formant_synth_kernel behind it.
// Analyse: one workgroup of 256 per (row, hop). The 2 Hp + P samples of the hop's window are staged in LDS, every thread sums
// its own products of all P + 1 lags in registers (one fmaf chain per lag, i ascending), the waves fold them with xor
// butterflies, wave 0 runs Levinson-Durbin with the coefficients spread over its lanes (the inner product is the 32-lane
// butterfly of the definition), and every thread whitens its samples of the hop with one fmaf chain.
// Synthesise: the recursion is sequential per row, so one wave owns a row and walks its hops and samples in order. It runs the
// transposed direct form: lane k-1 holds s_k, per sample z = e' + s_1, then s_k = fmaf(-a[k], z, s_{k+1}) with s_{k+1} taken
// from the next lane by one DPP wave shift -- the fmaf chain of the definition, k descending, at one shift, one broadcast and
// one fmaf per sample instead of a P-term reduction. At a hop's start the s_k are rebuilt from the row's last P values of z
// with the new coefficients, which is exactly what the direct form of the definition does across the boundary.
#include "../common.h"
#include "../codec_kernels.h"
#include "../formant_plan.h"

#pragma clang fp contract(off)  // a multiply and an add written apart round apart, as in the definition; every fused step is an fmaf

namespace q3 {
namespace {

constexpr int P = kFormantOrder;
constexpr int kThreads = kFormantLanes;  // 256
constexpr int kWaves = kThreads / 64;
constexpr int kHopMax = kStretchHsMax;   // 960

__global__ __launch_bounds__(kThreads) void formant_analyse_kernel(FormantAnalyseArgs a) {
    __shared__ float ys[2 * kHopMax + P];  // y[(h-1) Hp - P ...]
    __shared__ float ws[2 * kHopMax];      // the windowed block
    __shared__ float red[kWaves][P + 1];
    __shared__ float r_s[P + 1];
    __shared__ float a_s[P + 1];
    const int b = blockIdx.y, t = threadIdx.x;
    const int64_t h = blockIdx.x;
    const int64_t n = int64_t(a.len[b]) * a.len_mul;
    const int hp = a.hp;
    if (n <= 0 || h * hp >= n) return;  // a row of length 0 touches nothing
    const float* y = a.y + int64_t(b) * a.y_bstride;
    const int64_t lo = -int64_t(a.hist), j0 = (h - 1) * hp - P;
    const int N = 2 * hp;
    for (int i = t; i < N + P; i += kThreads) {
        const int64_t j = j0 + i;
        ys[i] = (j >= lo && j < n) ? y[j] : 0.f;
    }
    __syncthreads();
    for (int i = t; i < N; i += kThreads) ws[i] = a.win[i] * ys[P + i];
    __syncthreads();
    // the autocorrelation: lane t's own chain per lag, then the butterfly of each wave, then the four waves
    float acc[P + 1];
#pragma unroll
    for (int k = 0; k <= P; ++k) acc[k] = 0.f;
    for (int i = t; i < N; i += kThreads) {
        const float wi = ws[i];
#pragma unroll
        for (int k = 0; k <= P; ++k) {
            const float wk = ws[i >= k ? i - k : 0];
            acc[k] = i >= k ? fmaf(wi, wk, acc[k]) : acc[k];
        }
    }
#pragma unroll
    for (int k = 0; k <= P; ++k) {
        float v = acc[k];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
        if ((t & 63) == 0) red[t >> 6][k] = v;
    }
    __syncthreads();
    if (t <= P) {
        float r = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
        r = r * a.lag[t];
        if (t == 0) r = r * kFormantR0Scale;
        r_s[t] = r;
    }
    __syncthreads();
    if (t < 64) {  // Levinson-Durbin on wave 0: lane j holds a[j]
        const float r0 = r_s[0];
        bool ok = r0 >= kFormantR0Floor && r0 <= FLT_MAX;
        float err = r0, cur = 0.f;
        for (int i = 1; i <= P && ok; ++i) {
            const bool mine = t >= 1 && t < i;
            const float rj = r_s[mine ? i - t : 0];
            float p = mine ? cur * rj : 0.f;
#pragma unroll
            for (int off = 16; off >= 1; off >>= 1) p = p + __shfl_xor(p, off, 64);
            const float sum = r_s[i] + p;
            const float k = (-sum) / err;
            if (!(fabsf(k) < 1.0f)) ok = false;
            const float other = __shfl(cur, (i - t) & 63, 64);
            cur = mine ? fmaf(k, other, cur) : (t == i ? k : 0.f);
            const float kk = k * k;
            const float u = 1.0f - kk;
            err = err * u;
            if (!(err > 0.0f)) ok = false;
        }
        if (t >= 1 && t <= P) {
            const float v = ok ? cur : 0.f;
            a_s[t] = v;
            a.coef[int64_t(b) * a.coef_bstride + h * P + (t - 1)] = v;
        }
    }
    __syncthreads();
    const int64_t left = n - h * hp;
    const int cnt = left < hp ? int(left) : hp;
    float* e = a.e + int64_t(b) * a.e_bstride + h * hp;
    for (int s = t; s < cnt; s += kThreads) {
        const float* yv = ys + P + hp + s;
        float v = yv[0];
#pragma unroll
        for (int k = 1; k <= P; ++k) v = fmaf(a_s[k], yv[-k], v);
        e[s] = v;
    }
}

// lane l <- lane l + 1 (lane 63 <- 0): DPP wave_shl:1
__device__ __forceinline__ float lane_from_next(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x130, 0xf, 0xf, true));
}

__global__ __launch_bounds__(64) void formant_synth_kernel(FormantSynthArgs a) {
    __shared__ float zl[P + kHopMax];       // [P values in front of the hop][the hop's z]
    __shared__ float as[P];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int64_t n = int64_t(a.len[b]) * a.len_mul;
    if (n <= 0) return;  // a row of length 0 touches nothing, its state included
    const int ho = a.ho;
    const int64_t hops = (n + ho - 1) / ho;
    const float* ep = a.ep + int64_t(b) * a.ep_bstride;
    float* out = a.out + int64_t(b) * a.out_bstride;
    const float* coef = a.coef + int64_t(b) * a.coef_bstride;
    if (lane < P) zl[lane] = a.state_in ? a.state_in[int64_t(b) * a.state_in_bstride + lane] : 0.f;
    for (int64_t h = 0; h < hops; ++h) {
        const int64_t left = n - h * ho;
        const int cnt = left < ho ? int(left) : ho;
        if (lane < P) as[lane] = coef[h * P + lane];  // a[lane + 1]
        __syncthreads();
        // s_k at the hop's start from the last P values of z and this hop's coefficients, k = lane + 1:
        // the tail j = P .. k of the chain that z[n0 + k - 1] will finish
        const float na = lane < P ? -as[lane] : 0.f;
        float s = 0.f;
        if (lane < P) {
            for (int j = P; j > lane; --j) s = fmaf(-as[j - 1], zl[P + lane - j], s);
        }
        for (int base = 0; base < cnt; base += 64) {
            const int m = cnt - base < 64 ? cnt - base : 64;
            const float eb = lane < m ? ep[h * ho + base + lane] : 0.f;
            float zb = 0.f;
            for (int i = 0; i < m; ++i) {
                const float en = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(eb), i));
                const float z = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(en + s)));
                const float next = lane_from_next(s);
                s = lane < P ? fmaf(na, z, next) : 0.f;
                zb = lane == i ? z : zb;
            }
            if (lane < m) {
                zl[P + base + lane] = zb;
                out[h * ho + base + lane] = a.clamp ? (zb < -1.f ? -1.f : (zb > 1.f ? 1.f : zb)) : zb;  // (a NaN stays a NaN)
            }
        }
        __syncthreads();
        const float keep = lane < P ? zl[cnt + lane] : 0.f;  // the last P values behind this hop
        __syncthreads();
        if (lane < P) {
            zl[lane] = keep;
            if (a.state_frames && (h + 1) % a.frame_hops == 0)
                a.state_frames[int64_t(b) * a.state_frames_bstride + (h / a.frame_hops) * a.state_frame_words + lane] = keep;
        }
        __syncthreads();
    }
    if (a.state_out && lane < P) a.state_out[int64_t(b) * a.state_out_bstride + lane] = zl[lane];
}

}  // namespace

void launch_formant_analyse(const FormantAnalyseArgs& a, hipStream_t st) {
    if (a.B <= 0 || a.max_len <= 0) return;
    Q3_CHECK(a.hp >= 1 && a.hp <= kHopMax && a.len_mul >= 1 && a.hist >= 0, 7, "internal error: formant analysis geometry");
    Q3_CHECK(a.y && a.len && a.win && a.lag && a.coef && a.e, 7, "internal error: formant analysis without its tensors");
    const int64_t hops = (a.max_len + a.hp - 1) / a.hp;
    Q3_CHECK(a.B == 1 || (a.coef_bstride >= hops * P && a.e_bstride >= a.max_len && a.y_bstride >= a.max_len), 7,
             "internal error: formant analysis rows overlap");
    Q3_CHECK(hops <= 0x7fffffff && a.B <= 65535, 3, "Invalid input: too many samples or rows in one formant analysis");
    (void)hipGetLastError();  // the runtime's last-error slot is sticky: an earlier, handled failure must not be read as this launch's
    hipLaunchKernelGGL(formant_analyse_kernel, dim3(unsigned(hops), unsigned(a.B)), dim3(kThreads), 0, st, a);
    Q3_HIP(hipGetLastError());
}

void launch_formant_synth(const FormantSynthArgs& a, hipStream_t st) {
    if (a.B <= 0 || a.max_len <= 0) return;
    Q3_CHECK(a.ho >= 1 && a.ho <= kHopMax && a.len_mul >= 1, 7, "internal error: formant synthesis geometry");
    Q3_CHECK(a.ep && a.out && a.len && a.coef, 7, "internal error: formant synthesis without its tensors");
    const int64_t hops = (a.max_len + a.ho - 1) / a.ho;
    Q3_CHECK(a.B == 1 || (a.coef_bstride >= hops * P && a.ep_bstride >= a.max_len && a.out_bstride >= a.max_len), 7,
             "internal error: formant synthesis rows overlap");
    Q3_CHECK(!a.state_frames || (a.frame_hops >= 1 && a.state_frame_words >= P), 7, "internal error: formant synthesis state layout");
    (void)hipGetLastError();
    hipLaunchKernelGGL(formant_synth_kernel, dim3(unsigned(a.B)), dim3(64), 0, st, a);
    Q3_HIP(hipGetLastError());
}

}  // namespace q3
