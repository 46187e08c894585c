// resample_ratio.hip -- the polyphase FIR of resample_plan.h for ANY reduced ratio L / M: the one stage behind the time stretch
// of a pitched handle (pitch_plan.h: Hp * M -> Ho * L, pitch and output rate together), q3tts_pitch_shift and
// q3tts_debug_resample_ratio. The seven fixed rates stay on resample.hip, whose whole [L][2K] table fits LDS; here L runs to
// 6909 and the table to 0.94 MB, so it stays in global memory (L2 holds it) in OUTPUT ORDER, [2K][L] with column c = n mod L
// holding phase (c M) mod L: the 64 lanes of a wave are consecutive outputs and read consecutive words per tap. The input span
// of a workgroup's 256 outputs is staged in LDS as in resample.hip (at most 13.6 KiB for every pitched handle, K up to 204).
// One thread per output, one fmaf chain over its 2K taps in ascending order: the result does not depend on the launch geometry
// and equals resample_reference bit for bit.
#include "../common.h"
#include "../codec_kernels.h"

namespace q3 {
namespace {

constexpr int kTile = 256;  // outputs per workgroup == threads

// LDS: xs [span]. Rows, lengths and zero-fill as resample_kernel's; the `hist` samples in front of a row are read in either
// form, as resample_reference reads them (the centred callers have none).
__global__ __launch_bounds__(256) void resample_ratio_kernel(ResampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) float xs[];
    const int b = blockIdx.y;
    const int64_t n_in = int64_t(a.len[b]) * (a.len_mul_rows ? a.len_mul_rows[b] : a.len_mul);
    if (n_in <= 0) return;  // a row of length 0 touches nothing
    const int64_t n_out = (n_in * a.L + a.M - 1) / a.M;
    const int64_t n0 = int64_t(blockIdx.x) * kTile;
    if (n0 >= n_out) return;
    const int taps = 2 * a.K;
    const int64_t n_last = (n0 + kTile - 1 < n_out ? n0 + kTile - 1 : n_out - 1);
    const int back = a.centred ? a.K - 1 : taps - 1, fwd = a.centred ? a.K : 0;
    const int64_t s0 = n0 * a.M / a.L - back, s1 = n_last * a.M / a.L + fwd;  // the span, inclusive
    const int64_t a0 = s0 & ~int64_t(3);  // floor to a float4 of the row (rows start 16-byte aligned)
    const int n4 = int((s1 - a0 + 4) >> 2);
    const int64_t lo = -int64_t(a.hist), hi = n_in;
    const float* xb = a.x + int64_t(b) * a.x_bstride;
    for (int v = threadIdx.x; v < n4; v += kTile) {
        const int64_t j = a0 + 4 * int64_t(v);
        float4 w;
        if (j >= lo && j + 3 < hi) {
            w = *reinterpret_cast<const float4*>(xb + j);
        } else {
            w.x = (j + 0 >= lo && j + 0 < hi) ? xb[j + 0] : 0.f;
            w.y = (j + 1 >= lo && j + 1 < hi) ? xb[j + 1] : 0.f;
            w.z = (j + 2 >= lo && j + 2 < hi) ? xb[j + 2] : 0.f;
            w.w = (j + 3 >= lo && j + 3 < hi) ? xb[j + 3] : 0.f;
        }
        reinterpret_cast<float4*>(xs)[v] = w;
    }
    __syncthreads();
    const int64_t n = n0 + threadIdx.x;
    if (n >= n_out) return;
    const int64_t q = n * a.M / a.L;
    const float* __restrict__ t = a.tab + int(n % a.L);  // tap i of this output: t[i * L]
    const float* xv = xs + (q - back - a0);
    const int L = a.L;
    float acc = 0.f;
    int i = 0;
    // four taps' loads in flight ahead of their fmafs; the chain itself stays one accumulator, i ascending
    for (; i + 4 <= taps; i += 4) {
        const float t0 = t[0], t1 = t[L], t2 = t[2 * L], t3 = t[3 * L];
        const float x0 = xv[i], x1 = xv[i + 1], x2 = xv[i + 2], x3 = xv[i + 3];
        t += 4 * int64_t(L);
        acc = fmaf(t0, x0, acc);
        acc = fmaf(t1, x1, acc);
        acc = fmaf(t2, x2, acc);
        acc = fmaf(t3, x3, acc);
    }
    for (; i < taps; ++i) {
        acc = fmaf(t[0], xv[i], acc);
        t += L;
    }
    if (a.clamp) acc = acc < -1.f ? -1.f : (acc > 1.f ? 1.f : acc);  // (a NaN stays a NaN)
    a.y[int64_t(b) * a.y_bstride + n] = acc;
}

}  // namespace

size_t resample_ratio_lds_bytes(int L, int M, int K) {
    const int64_t span = (int64_t(kTile - 1) * M) / L + 2 * int64_t(K) + 8;  // q1 - q0 <= 255 M / L + 1, 2K taps, 3 of alignment
    return size_t((span + 3) / 4 * 4) * sizeof(float);
}

void launch_resample_ratio(const ResampleArgs& a, hipStream_t st) {
    if (a.B <= 0 || a.max_in <= 0) return;
    Q3_CHECK(a.L >= 1 && a.M >= 1 && a.K >= 1 && a.len_mul >= 1 && a.hist >= 0, 7, "internal error: resampler geometry");
    Q3_CHECK((reinterpret_cast<uintptr_t>(a.x) & 15) == 0 && (a.x_bstride & 3) == 0, 7,
             "internal error: resampler rows must start at 16-byte boundaries");
    Q3_CHECK(int64_t(a.L) * 2 * a.K <= (int64_t(1) << 24), 3, "Invalid input: the ratio's phase table is larger than 64 MiB");
    Q3_CHECK(resample_ratio_lds_bytes(a.L, a.M, a.K) <= 64 * 1024, 3, "Invalid input: the ratio's input span is larger than its LDS budget");
    Q3_CHECK(a.max_in <= (int64_t(1) << 40) / a.L, 3, "Invalid input: too many samples in one resampling call");
    const int64_t max_out = (a.max_in * a.L + a.M - 1) / a.M;
    const int64_t gx = (max_out + kTile - 1) / kTile;
    Q3_CHECK(gx <= 0x7fffffff && a.B <= 65535, 3, "Invalid input: too many samples or rows in one resampling call");
    (void)hipGetLastError();  // the runtime's last-error slot is sticky: an earlier, handled failure must not be read as this launch's
    hipLaunchKernelGGL(resample_ratio_kernel, dim3(unsigned(gx), unsigned(a.B)), dim3(kTile), resample_ratio_lds_bytes(a.L, a.M, a.K), st, a);
    Q3_HIP(hipGetLastError());
}

}  // namespace q3
