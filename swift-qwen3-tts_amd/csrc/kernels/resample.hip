// resample.hip -- the polyphase FIR of resample_plan.h on the device: the codec tail's last causal stage (24 kHz -> the
// handle's output rate) and, in centred form, the resampling of reference clips and of q3tts_resample.
// One thread per output sample; a workgroup of 256 stages the phase table and the input span of its 256 outputs in LDS, so
// neighbouring outputs take their taps from LDS. Every output is one fmaf chain over its 2K taps in ascending order: the
// result does not depend on the launch geometry, which is what keeps a streamed decode bit-identical to the one-shot one.
#include "../common.h"
#include "../codec_kernels.h"

namespace q3 {
namespace {

constexpr int kTile = 256;  // outputs per workgroup == threads

// LDS: tab [align4(L * 2K)] | xs [span]. Row b's sample j sits at x + b * x_bstride + j; valid j: [lo, n_in) with lo = -hist
// in causal mode (the stream's margin) and 0 otherwise; everything else reads as zero and is never loaded.
__global__ __launch_bounds__(256) void resample_kernel(ResampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int b = blockIdx.y;
    const int64_t n_in = int64_t(a.len[b]) * (a.len_mul_rows ? a.len_mul_rows[b] : a.len_mul);  // (a row's own frame size behind per-row hops)
    if (n_in <= 0) return;  // a row of length 0 touches nothing
    const int64_t n_out = (n_in * a.L + a.M - 1) / a.M;
    const int64_t n0 = int64_t(blockIdx.x) * kTile;
    if (n0 >= n_out) return;
    const int taps = 2 * a.K;
    const int tab4 = (a.L * taps + 3) >> 2;  // the device table is padded to whole float4s
    float* tabs = sm;
    float* xs = sm + 4 * tab4;
    for (int i = threadIdx.x; i < tab4; i += kTile) reinterpret_cast<float4*>(tabs)[i] = reinterpret_cast<const float4*>(a.tab)[i];
    const int64_t n_last = (n0 + kTile - 1 < n_out ? n0 + kTile - 1 : n_out - 1);
    const int back = a.centred ? a.K - 1 : taps - 1, fwd = a.centred ? a.K : 0;
    const int64_t s0 = n0 * a.M / a.L - back, s1 = n_last * a.M / a.L + fwd;  // the span, inclusive
    const int64_t a0 = s0 & ~int64_t(3);  // floor to a float4 of the row (rows start 16-byte aligned)
    const int n4 = int((s1 - a0 + 4) >> 2);
    const int64_t lo = a.centred ? 0 : -int64_t(a.hist), hi = n_in;
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
    const int64_t nm = n * a.M;
    const int64_t q = nm / a.L;
    const int r = int(nm - q * a.L);
    const float* t = tabs + r * taps;
    const float* xv = xs + (q - back - a0);
    float acc = 0.f;
    for (int i = 0; i < taps; ++i) acc = fmaf(t[i], xv[i], acc);
    if (a.clamp) acc = acc < -1.f ? -1.f : (acc > 1.f ? 1.f : acc);  // (a NaN stays a NaN)
    a.y[int64_t(b) * a.y_bstride + n] = acc;
}

}  // namespace

size_t resample_lds_bytes(int L, int M, int K) {
    const size_t tab = size_t((L * 2 * K + 3) / 4) * 4;
    const size_t span = size_t((int64_t(kTile - 1) * M) / L + 2 * K + 8);  // q1 - q0 <= 255 M / L + 1, 2K taps, 3 of alignment
    return (tab + (span + 3) / 4 * 4) * sizeof(float);
}

void launch_resample(const ResampleArgs& a, hipStream_t st) {
    if (a.B <= 0 || a.max_in <= 0) return;
    Q3_CHECK(a.L >= 1 && a.M >= 1 && a.K >= 1 && a.len_mul >= 1 && a.hist >= 0, 7, "internal error: resampler geometry");
    Q3_CHECK((reinterpret_cast<uintptr_t>(a.x) & 15) == 0 && (a.x_bstride & 3) == 0 && (reinterpret_cast<uintptr_t>(a.tab) & 15) == 0, 7,
             "internal error: resampler rows must start at 16-byte boundaries");
    const size_t lds = resample_lds_bytes(a.L, a.M, a.K);
    Q3_CHECK(lds <= 64 * 1024, 7, "internal error: resampler table larger than its LDS budget");
    const int64_t max_out = (a.max_in * a.L + a.M - 1) / a.M;
    const int64_t gx = (max_out + kTile - 1) / kTile;
    Q3_CHECK(gx <= 0x7fffffff && a.B <= 65535, 3, "Invalid input: too many samples or rows in one resampling call");
    (void)hipGetLastError();  // the runtime's last-error slot is sticky: an earlier, handled failure must not be read as this launch's
    hipLaunchKernelGGL(resample_kernel, dim3(unsigned(gx), unsigned(a.B)), dim3(kTile), lds, st, a);
    Q3_HIP(hipGetLastError());
}

}  // namespace q3
