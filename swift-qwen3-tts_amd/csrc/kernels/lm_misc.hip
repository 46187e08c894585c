// lm_misc.hip -- small row kernels of the AR loop: residual+RMSNorm, embedding gathers, the
// next-input embedding sum and the per-row loop bookkeeping. All are HBM/L2 trivial (<= 64 rows of
// <= 2048 bf16); they exist to keep the frame step free of host round trips (the reference pays
// >= 17 eval()/.item() syncs per frame: SURVEY.md section 3.2).
#include <algorithm>

#include "../common.h"
#include "../kernels.h"
#include "row_jobs.h"

namespace q3 {
namespace {

__device__ __forceinline__ float block_sum_256(float v, float* sh) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// RMSNorm of whole rows, fragment-major in and out. One workgroup per row (the arithmetic lives in row_jobs.h: the frame
// step carries the same job inside the codec_head launch).
__global__ __launch_bounds__(256) void norm_rows_kernel(NormRowsArgs a) {
    __shared__ float sh[4];
    __shared__ float parts[8];
    norm_row_job(a, blockIdx.x, threadIdx.x, sh, parts);
}

__global__ void gather_rows_kernel(const uint16_t* table, int ld, const int32_t* ids, const int32_t* token_map,
                                   int dim, uint16_t* out, int ldo, int out_MB) {
    const int r = blockIdx.x;
    int id = ids[r];
    if (token_map) id = token_map[id];  // embedText, Talker.swift:627-633
    const uint4* src = reinterpret_cast<const uint4*>(table + (size_t)id * ld);
    for (int i = threadIdx.x; i < dim / 8; i += blockDim.x) {
        if (out_MB > 0) *reinterpret_cast<uint4*>(out + act_tiled_offset(r, 8 * i, out_MB)) = src[i];
        else reinterpret_cast<uint4*>(out + (size_t)r * ldo)[i] = src[i];
    }
}

__global__ void tile_rows_kernel(const uint16_t* src, int lds, uint16_t* dst, int dstMB, int dim) {
    const int r = blockIdx.x;
    const uint4* s = reinterpret_cast<const uint4*>(src + (size_t)r * lds);
    for (int i = threadIdx.x; i < dim / 8; i += blockDim.x)
        *reinterpret_cast<uint4*>(dst + act_tiled_offset(r, 8 * i, dstMB)) = s[i];
}
__global__ void untile_rows_kernel(const uint16_t* src, int srcMB, uint16_t* dst, int ldd, int dim) {
    const int r = blockIdx.x;
    uint4* d = reinterpret_cast<uint4*>(dst + (size_t)r * ldd);
    for (int i = threadIdx.x; i < dim / 8; i += blockDim.x)
        d[i] = *reinterpret_cast<const uint4*>(src + act_tiled_offset(r, 8 * i, srcMB));
}

__global__ void add_rows_kernel(const uint16_t* a, int lda, const uint16_t* b, int ldb, int dim, uint16_t* out,
                                int ldo) {
    const int r = blockIdx.x;
    const uint16_t* ar = a + (size_t)r * lda;
    const uint16_t* br = b + (size_t)r * ldb;
    uint16_t* orow = out + (size_t)r * ldo;
    for (int i = threadIdx.x; i < dim; i += blockDim.x) orow[i] = f2bf(bf2f(ar[i]) + bf2f(br[i]));
}

__global__ void compose_rows_kernel(const uint16_t* proj, int ldp, const uint16_t* table, int ldt, const uint16_t* extra,
                                    int lde, const int32_t* a, const int32_t* b, const int32_t* dst_row, uint16_t* dst,
                                    int ldd, int dim) {
    const int r = blockIdx.x;
    const uint16_t* pa = proj + (size_t)a[r] * ldp;
    const int bi = b[r];
    uint16_t* o = dst + (size_t)dst_row[r] * ldd;
    if (bi == -1) {
        for (int i = threadIdx.x; i < dim; i += blockDim.x) o[i] = pa[i];
    } else {
        const uint16_t* pb = bi >= 0 ? table + (size_t)bi * ldt : extra + (size_t)(-2 - bi) * lde;
        for (int i = threadIdx.x; i < dim; i += blockDim.x) o[i] = f2bf(bf2f(pa[i]) + bf2f(pb[i]));
    }
}

// Voice-clone prompt rows (Qwen3.swift:485-491): out[t] = codec_emb[c0[t]] + cp_emb[0][c1[t]] + ... left to right,
// each add rounded to bf16. codes [groups][T].
__global__ void ref_embed_rows_kernel(const int32_t* codes, int T, int groups, const uint16_t* codec_emb,
                                      const uint16_t* const* cp_emb, int H, uint16_t* out, int ldo) {
    const int t = blockIdx.x;
    for (int i = threadIdx.x; i < H; i += blockDim.x) {
        float v = bf2f(codec_emb[(size_t)codes[t] * H + i]);
        for (int g = 1; g < groups; ++g) v = rbf(v + bf2f(cp_emb[g - 1][(size_t)codes[(size_t)g * T + t] * H + i]));
        out[(size_t)t * ldo + i] = f2bf(v);
    }
}

// Decoder input of the rows of a decode batch (Qwen3.swift:1176-1180; kernels.h DecodeRowDesc): per row the reference frames
// ([16][Tref], none for a row without a reference) then the generated ones ([F][16]). blockIdx.y = row, one thread per quarter
// frame (4 codes, 16 bytes). A pure copy: the reference part transposes [16][Tref] into frames, the generated part moves as is.
template <bool VEC>
__global__ __launch_bounds__(256) void build_decode_codes_rows_kernel(const DecodeRowDesc* rows, int32_t* out, int Fdec) {
    const DecodeRowDesc d = rows[blockIdx.y];
    if (d.F <= 0) return;
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (d.Tref + d.F) * 4) return;
    const int f = q >> 2, g = (q & 3) * 4;
    int32_t v[4];
    if (f < d.Tref) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = d.ref[(size_t)(g + j) * d.Tref + f];
    } else {
        const int32_t* src = d.gen + (size_t)(f - d.Tref) * 16 + g;
        if constexpr (VEC) {
            const int4 w = *reinterpret_cast<const int4*>(src);
            v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = src[j];
        }
    }
    int32_t* dst = out + ((size_t)d.dst_row * Fdec + f) * 16 + g;
    if constexpr (VEC) {
        *reinterpret_cast<int4*>(dst) = make_int4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) dst[j] = v[j];
    }
}

__global__ void f32_to_bf16_kernel(const float* x, uint16_t* out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = f2bf(x[i]);
}

__global__ void ss_to_table_kernel(const float* ss, int ss_ld, float* dst, int nss, int rows) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < rows * nss) dst[i] = ss[(size_t)(i % nss) * ss_ld + i / nss];
}

__global__ void copy_rows_kernel(const uint16_t* src, int lds, uint16_t* dst, int ldd, int dim) {
    const int r = blockIdx.x;
    const uint4* s = reinterpret_cast<const uint4*>(src + (size_t)r * lds);
    uint4* d = reinterpret_cast<uint4*>(dst + (size_t)r * ldd);
    for (int i = threadIdx.x; i < dim / 8; i += blockDim.x) d[i] = s[i];
}

// Right-aligned position-by-position prefill: row b starts at step Pmax - n_prompt[b], so every
// row finishes its prompt at the same step and enters the frame loop together.
__global__ __launch_bounds__(256) void prefill_load_kernel(PrefillLoadArgs a) {
    __shared__ float sh[4];
    const int b = blockIdx.x;
    const int idx = a.step - (a.Pmax - a.n_prompt[b]);
    const bool on = idx >= 0;
    if (threadIdx.x == 0) a.active[b] = on ? 1 : 0;
    const uint4* src = reinterpret_cast<const uint4*>(a.prompt + ((size_t)b * a.Pmax + (on ? idx : 0)) * a.H);
    float ss = 0.f;
    for (int i = threadIdx.x; i < a.H / 8; i += 256) {
        const uint4 v = src[i];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) ss += lo_bf(w[j]) * lo_bf(w[j]) + hi_bf(w[j]) * hi_bf(w[j]);
        *reinterpret_cast<uint4*>(a.h + act_tiled_offset(b, 8 * i, a.hMB)) = v;
    }
    const float tot = block_sum_256(ss, sh);
    if (threadIdx.x == 0) a.ss_out[b] = tot;
}

// Chunked prefill: element p of row b is prompt position r = r_base + n_prompt[b] + p (right-aligned so that the last
// chunk ends at the row's second-to-last prompt position); r < 0 is padding. Row m = p * B + b of the residual stream.
__global__ __launch_bounds__(256) void prefill_chunk_load_kernel(PrefillLoadArgs a) {
    __shared__ float sh[4];
    const int b = blockIdx.x, p = blockIdx.y;
    const int r = a.step + a.n_prompt[b] + p;  // `step` carries r_base
    const bool on = r >= 0;
    const int m = p * a.B + b;
    const uint4* src = reinterpret_cast<const uint4*>(a.prompt + ((size_t)b * a.Pmax + (on ? r : 0)) * a.H);
    float ss = 0.f;
    for (int i = threadIdx.x; i < a.H / 8; i += 256) {
        const uint4 v = on ? src[i] : make_uint4(0, 0, 0, 0);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) ss += lo_bf(w[j]) * lo_bf(w[j]) + hi_bf(w[j]) * hi_bf(w[j]);
        *reinterpret_cast<uint4*>(a.h + act_tiled_offset(m, 8 * i, a.hMB)) = v;
    }
    const float tot = block_sum_256(ss, sh);
    if (threadIdx.x == 0) a.ss_out[m] = tot;
}
__global__ void advance_len_chunk_kernel(int32_t* kv_len, const int32_t* n_prompt, int r_base, int C, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int r0 = r_base + n_prompt[b];
    const int p0 = r0 < 0 ? (-r0 < C ? -r0 : C) : 0;
    kv_len[b] += C - p0;
}

// Continuous batching: row j of the prefilled sub-batch takes slot desc[j].slot of the frame step (kernels.h AdmitArgs).
// Only that slot's row of every array is written: the rows in flight around it carry their state across this launch.
__global__ __launch_bounds__(256) void admit_rows_kernel(AdmitArgs a) {
    const int j = blockIdx.x, tid = threadIdx.x;
    const AdmitDesc d = a.desc[j];
    const int s = d.slot;
    if (s < 0 || s >= a.slots) return;
    for (int i = tid; i < a.H / 8; i += 256)
        *reinterpret_cast<uint4*>(a.h + act_tiled_offset(s, 8 * i, a.hMB)) =
            *reinterpret_cast<const uint4*>(a.src_h + act_tiled_offset(j, 8 * i, a.srcMB));
    uint8_t* seen = a.seen + (size_t)s * a.V;
    for (int i = tid; i < a.V; i += 256) seen[i] = 0;
    int32_t* codes = a.codes + (size_t)s * a.Fmax * 16;
    for (int i = tid; i < a.Fmax * 16; i += 256) codes[i] = 0;
    if (tid < 16) a.cur_codes[(size_t)s * 16 + tid] = 0;
    if (tid == 0) {
        a.ss[s] = a.src_ss[j];
        a.kv_len[s] = a.src_kv_len[j];
        a.n_prompt[s] = a.src_n_prompt[j];
        a.n_trailing[s] = d.n_trailing;
        a.max_frames[s] = d.max_frames;
        a.row_key[s] = d.row_key;
        a.sp[s] = d.sp;
        a.n_frames[s] = 0;
        a.cp_len[s] = 0;
        a.trailing_idx[s] = 0;
        a.finished[s] = 0;
        a.active[s] = 1;
        if (a.text_open) a.text_open[s] = d.text_open ? 1 : 0;
        if (a.starved) a.starved[s] = 0;
    }
}

// Open-text requests of a session: new trailing text for the slots listed in desc, and the resume of the ones that starved
// (kernels.h TextAppendArgs). Only the listed slots' rows are written; the rows in flight around them carry on.
__global__ __launch_bounds__(256) void text_append_rows_kernel(TextAppendArgs a) {
    __shared__ float sh[4];
    const TextAppendDesc d = a.desc[blockIdx.x];
    const int s = d.slot, tid = threadIdx.x;
    const FrameEndArgs& fe = a.fe;
    if (s < 0 || s >= a.slots || d.n_new < 0) return;
    const int nt = a.n_trailing[s];
    const int add = d.n_new + (d.close ? 1 : 0);
    if (nt < 0 || nt + add > fe.Tmax) return;  // (the host has checked it: nothing is ever written past the slot's rows)
    uint16_t* dst = a.trailing + ((size_t)s * fe.Tmax + nt) * fe.H;
    for (int r = 0; r < add; ++r) {
        const uint4* from = reinterpret_cast<const uint4*>(r < d.n_new ? a.src + (size_t)(d.src_row + r) * fe.H : a.eos_row);
        uint4* to = reinterpret_cast<uint4*>(dst + (size_t)r * fe.H);
        for (int i = tid; i < fe.H / 8; i += 256) to[i] = from[i];
    }
    // A starved row stopped exactly at the end of what had arrived (trailing_idx == n_trailing): its next text row is the first
    // new one, read from the source rather than from the copy just stored.
    const int ti = fe.trailing_idx[s];
    const bool resume = fe.starved[s] != 0 && add > 0 && ti == nt;  // block-uniform
    float ss = 0.f;
    if (resume) {
        const uint16_t* text = d.n_new > 0 ? a.src + (size_t)d.src_row * fe.H : a.eos_row;
        ss = next_input_row(fe, s, tid, fe.cur_codes + (size_t)s * 16, -1, text);
    }
    const float tot = block_sum_first256(ss, sh, tid);
    if (tid == 0) {
        a.n_trailing[s] = nt + add;
        if (d.close) {
            a.text_open[s] = 0;
            a.max_frames[s] = d.max_frames;
        }
        if (resume) {
            fe.ss_out[s] = tot;
            fe.trailing_idx[s] = ti + 1;
            fe.cp_len[s] = 0;
            fe.starved[s] = 0;
            fe.finished[s] = 0;
            fe.active[s] = 1;
        }
    }
}

// Continuous batching: the slots listed in `mask` (bit s: slot s) leave the frame step at once -- finished up, active down, the
// state of an empty slot -- whatever their rows were doing. The slots around them are not touched. One launch, one wave.
__global__ __launch_bounds__(64) void cancel_rows_kernel(unsigned long long mask, uint8_t* finished, uint8_t* active, int slots) {
    const int s = threadIdx.x;
    if (s >= slots || !((mask >> s) & 1ull)) return;
    finished[s] = 1;
    active[s] = 0;
}

// Diagnostics (Q3TTS_FRAME_STAMPS=1): slot[k] accumulates the time between this stamp and the previous one of the same
// frame step, so that the phases of a REPLAYED graph can be timed (a tracing profiler perturbs a chain of 5 us launches).
__global__ void stamp_kernel(unsigned long long* acc, unsigned long long* last, int k) {
    const unsigned long long t = wall_clock64();  // 100 MHz constant clock
    if (k > 0) acc[k] += t - *last;
    else acc[0] += 1;  // frame steps seen
    *last = t;
}

__global__ void advance_len_kernel(int32_t* kv_len, const uint8_t* active, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B && (!active || active[b])) kv_len[b] += 1;
}

// End of a frame as a launch of its own (row_jobs.h frame_end_job; the frame step runs it in the last sampler's launch)
__global__ __launch_bounds__(256) void frame_end_kernel(FrameEndArgs a) {
    __shared__ float sh[4];
    const int b = blockIdx.x;
    if (a.finished[b]) {
        if (threadIdx.x == 0) a.cp_len[b] = 0;
        return;
    }
    frame_end_job(a, b, threadIdx.x, -1, sh);
}

}  // namespace

void launch_norm_rows(const NormRowsArgs& a, hipStream_t st) {
    Q3_CHECK(a.H % 128 == 0 && a.H <= 4096, 3, "norm_rows: H must be a multiple of 128, at most 4096");
    // norm_row_job folds 32 partials per thread on 8 threads; the GEMM prologue's tail loop would take more, and the two
    // must add up the same partials
    Q3_CHECK(!a.ss_in || (a.ss_count >= 1 && a.ss_count <= 256), 3, "norm_rows: at most 256 partial sums of squares per row");
    hipLaunchKernelGGL(norm_rows_kernel, dim3(a.M), dim3(256), 0, st, a);
}
void launch_gather_rows(const uint16_t* table, int ld, const int32_t* ids, const int32_t* token_map, int n,
                        int dim, uint16_t* out, int ldo, int out_MB, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(gather_rows_kernel, dim3(n), dim3(256), 0, st, table, ld, ids, token_map, dim, out, ldo, out_MB);
}
void launch_tile_rows(const uint16_t* src, int lds, uint16_t* dst, int dstMB, int rows, int dim, hipStream_t st) {
    if (rows <= 0) return;
    hipLaunchKernelGGL(tile_rows_kernel, dim3(rows), dim3(256), 0, st, src, lds, dst, dstMB, dim);
}
void launch_untile_rows(const uint16_t* src, int srcMB, uint16_t* dst, int ldd, int rows, int dim, hipStream_t st) {
    if (rows <= 0) return;
    hipLaunchKernelGGL(untile_rows_kernel, dim3(rows), dim3(256), 0, st, src, srcMB, dst, ldd, dim);
}
void launch_add_rows(const uint16_t* a, int lda, const uint16_t* b, int ldb, int rows, int dim, uint16_t* out,
                     int ldo, hipStream_t st) {
    if (rows <= 0) return;
    hipLaunchKernelGGL(add_rows_kernel, dim3(rows), dim3(256), 0, st, a, lda, b, ldb, dim, out, ldo);
}
void launch_compose_rows(const uint16_t* proj, int ldp, const uint16_t* table, int ldt, const uint16_t* extra, int lde,
                         const int32_t* a, const int32_t* b, const int32_t* dst_row, uint16_t* dst, int ldd, int n, int dim,
                         hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(compose_rows_kernel, dim3(n), dim3(256), 0, st, proj, ldp, table, ldt, extra, lde, a, b, dst_row, dst,
                       ldd, dim);
}
void launch_ref_embed_rows(const int32_t* codes, int T, int groups, const uint16_t* codec_emb, const uint16_t* const* cp_emb,
                           int H, uint16_t* out, int ldo, hipStream_t st) {
    if (T <= 0) return;
    hipLaunchKernelGGL(ref_embed_rows_kernel, dim3(T), dim3(256), 0, st, codes, T, groups, codec_emb, cp_emb, H, out, ldo);
}
void launch_build_decode_codes_rows(const DecodeRowDesc* host, const DecodeRowDesc* rows, int R, int32_t* out, int out_rows,
                                    int Fdec, hipStream_t st) {
    int frames = 0;
    bool vec = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    for (int r = 0; r < R; ++r) {
        const DecodeRowDesc& d = host[r];
        if (d.F <= 0) continue;
        Q3_CHECK(d.Tref >= 0 && (d.Tref == 0 || d.ref) && d.gen && d.dst_row >= 0 && d.dst_row < out_rows && d.Tref + d.F <= Fdec, 7,
                 "internal error: decode row outside the decoder's code buffer");
        frames = std::max(frames, d.Tref + d.F);
        vec = vec && (reinterpret_cast<uintptr_t>(d.gen) & 15) == 0;
    }
    if (frames == 0) return;
    const dim3 grid((frames * 4 + 255) / 256, R);
    if (vec) hipLaunchKernelGGL(build_decode_codes_rows_kernel<true>, grid, dim3(256), 0, st, rows, out, Fdec);
    else hipLaunchKernelGGL(build_decode_codes_rows_kernel<false>, grid, dim3(256), 0, st, rows, out, Fdec);
}
void launch_f32_to_bf16(const float* x, uint16_t* out, int n, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(f32_to_bf16_kernel, dim3((n + 255) / 256), dim3(256), 0, st, x, out, n);
}
void launch_ss_to_table(const float* ss, int ss_ld, float* dst, int nss, int rows, hipStream_t st) {
    hipLaunchKernelGGL(ss_to_table_kernel, dim3((rows * nss + 255) / 256), dim3(256), 0, st, ss, ss_ld, dst, nss, rows);
}
void launch_copy_rows(const uint16_t* src, int lds, uint16_t* dst, int ldd, int rows, int dim, hipStream_t st) {
    if (rows <= 0) return;
    hipLaunchKernelGGL(copy_rows_kernel, dim3(rows), dim3(256), 0, st, src, lds, dst, ldd, dim);
}
void launch_prefill_load(const PrefillLoadArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(prefill_load_kernel, dim3(a.B), dim3(256), 0, st, a);
}
void launch_prefill_chunk_load(const PrefillLoadArgs& a, int C, hipStream_t st) {
    hipLaunchKernelGGL(prefill_chunk_load_kernel, dim3(a.B, C), dim3(256), 0, st, a);
}
void launch_advance_len_chunk(int32_t* kv_len, const int32_t* n_prompt, int r_base, int C, int B, hipStream_t st) {
    hipLaunchKernelGGL(advance_len_chunk_kernel, dim3(1), dim3(64), 0, st, kv_len, n_prompt, r_base, C, B);
}
void launch_stamp(unsigned long long* acc, unsigned long long* last, int k, hipStream_t st) {
    hipLaunchKernelGGL(stamp_kernel, dim3(1), dim3(1), 0, st, acc, last, k);
}
void launch_advance_len(int32_t* kv_len, const uint8_t* active, int B, hipStream_t st) {
    hipLaunchKernelGGL(advance_len_kernel, dim3(1), dim3(64), 0, st, kv_len, active, B);
}
void launch_admit_rows(const AdmitArgs& a, int k, hipStream_t st) {
    if (k <= 0) return;
    hipLaunchKernelGGL(admit_rows_kernel, dim3(k), dim3(256), 0, st, a);
}
void launch_text_append_rows(const TextAppendArgs& a, const TextAppendDesc* host, int k, hipStream_t st) {
    if (k <= 0) return;
    Q3_CHECK(a.fe.starved && a.text_open && a.fe.H % 8 == 0, 7, "internal error: text_append_rows without the open-text arrays");
    for (int j = 0; j < k; ++j)
        Q3_CHECK(host[j].slot >= 0 && host[j].slot < a.slots && host[j].n_new >= 0 && host[j].src_row >= 0 &&
                     host[j].n_new + (host[j].close ? 1 : 0) <= a.fe.Tmax,
                 7, "internal error: text_append_rows descriptor outside the slot's trailing text");
    hipLaunchKernelGGL(text_append_rows_kernel, dim3(k), dim3(256), 0, st, a);
}
void launch_cancel_rows(uint64_t mask, uint8_t* finished, uint8_t* active, int slots, hipStream_t st) {
    Q3_CHECK(slots >= 1 && slots <= 64, 7, "internal error: cancel_rows covers at most 64 slots");
    if (slots < 64) mask &= (uint64_t(1) << slots) - 1;
    if (mask == 0) return;
    hipLaunchKernelGGL(cancel_rows_kernel, dim3(1), dim3(64), 0, st, (unsigned long long)mask, finished, active, slots);
}
void launch_frame_end(const FrameEndArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(frame_end_kernel, dim3(a.B), dim3(256), 0, st, a);
}

}  // namespace q3
