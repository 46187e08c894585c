// rowop_debug.cc -- q3tts_debug_rowop (q3tts.h): one launch of a non-GEMM row kernel (kernels/codec_misc.hip,
// kernels/voice_frontend.hip) on host buffers, through its own launcher. The host checks need neither an engine nor a GPU.
#include <algorithm>
#include <utility>
#include <vector>

#include "codec_kernels.h"
#include "common.h"
#include "engine.h"

namespace q3 {

namespace {

constexpr int kIn = 8, kIo = 4;
constexpr int64_t kPool = -1;             // a slot of any whole number of floats
constexpr int64_t kMaxElems = int64_t(1) << 27;

// What an op's shape states: bytes per slot (0: the slot must be NULL), and which slots may be left out.
struct Plan {
    int64_t in[kIn] = {}, io[kIo] = {};
    bool in_opt[kIn] = {}, io_opt[kIo] = {};
};

#define ROW_CHECK(cond, msg) Q3_CHECK(cond, 3, "debug_rowop: " msg)

void check_slots(const q3tts_rowop_debug& d, const Plan& pl) {
    auto one = [](const void* p, int64_t bytes, int64_t need, bool opt) {
        if (need == 0) {
            ROW_CHECK(p == nullptr && bytes == 0, "a slot the op does not name must be NULL");
            return;
        }
        if (!p) {
            ROW_CHECK(opt && bytes == 0, "null argument");
            return;
        }
        if (need == kPool) ROW_CHECK(bytes >= 4 && bytes % 4 == 0 && bytes / 4 <= kMaxElems, "a pool holds whole floats");
        else ROW_CHECK(bytes == need, "a buffer's size disagrees with the strides and counts given");
    };
    for (int i = 0; i < kIn; ++i) one(d.in[i], d.in_bytes[i], pl.in[i], pl.in_opt[i]);
    for (int i = 0; i < kIo; ++i) one(d.io[i], d.io_bytes[i], pl.io[i], pl.io_opt[i]);
}

const int32_t* i32(const void* p) { return static_cast<const int32_t*>(p); }
const int64_t* i64(const void* p) { return static_cast<const int64_t*>(p); }

// [lo, hi) ranges must not meet
void check_disjoint(std::vector<std::pair<int64_t, int64_t>> r, const char* msg) {
    std::sort(r.begin(), r.end());
    for (size_t i = 1; i < r.size(); ++i) Q3_CHECK(r[i].first >= r[i - 1].second, 3, msg);
}

// ops 1-4: frames[b] * ppf rows inside the allocation behind `margin`
void check_frames(const q3tts_rowop_debug& d, int slot, int B, int64_t ppf, int64_t margin, int64_t Tmax) {
    const int32_t* fr = i32(d.in[slot]);
    for (int b = 0; b < B; ++b) ROW_CHECK(fr[b] >= 0 && margin + int64_t(fr[b]) * ppf <= Tmax, "margin + frames[b] * ppf must not exceed Tmax");
}

// ops 6 and 7: the tensors of a RollDesc table inside the pool, apart from one another, float4-aligned where the kernels say so
void check_desc(const q3tts_rowop_debug& d, int n_desc, int B, int Tal) {
    const int64_t* t = i64(d.in[0]);
    const int64_t pool = d.io_bytes[0] / 4;
    std::vector<std::pair<int64_t, int64_t>> r;
    for (int i = 0; i < n_desc; ++i) {
        const int64_t off = t[3 * i], ff = t[3 * i + 1];
        ROW_CHECK(ff >= 1 && ff <= (1 << 20) && off >= 0 && off <= pool, "RollDesc: frame_floats / offset out of range");
        ROW_CHECK(off + int64_t(B) * Tal * ff <= pool, "RollDesc: a tensor ends outside the pool");
        ROW_CHECK(ff % 4 != 0 || off % 4 == 0, "RollDesc: a tensor of whole float4 frames must be 16-byte aligned");
        r.emplace_back(off, off + int64_t(B) * Tal * ff);
    }
    check_disjoint(r, "debug_rowop: RollDesc tensors overlap");
}

}  // namespace

void Engine::debug_rowop_check(const q3tts_rowop_debug& d) {
    ROW_CHECK(d.op >= 0 && d.op <= 20, "unknown op");
    const int32_t* p = d.p;
    for (int i = 0; i < 16; ++i) ROW_CHECK(p[i] >= -1 && p[i] <= (1 << 24), "parameter out of range");
    Plan pl;
    auto elems = [](int64_t a, int64_t b = 1, int64_t c = 1, int64_t e = 1) {  // bytes of an fp32 tensor of a * b * c * e elements
        int64_t n = 1;
        for (const int64_t v : {a, b, c, e}) {  // every factor is below 2^31 and the running product at most 2^27: no overflow
            ROW_CHECK(v >= 1 && v <= kMaxElems, "tensor beyond 2^27 elements");
            n *= v;
            ROW_CHECK(n <= kMaxElems, "tensor beyond 2^27 elements");
        }
        return n * 4;
    };
    auto batch = [](int B) { ROW_CHECK(B >= 1 && B <= 64, "batch out of range"); };
    switch (d.op) {
        case 0: {  // rvq_gather
            const int B = p[0], Fmax = p[1], csf = p[2], n_rest = p[3], inner = p[4], rf = p[5], rr = p[6];
            batch(B);
            ROW_CHECK(Fmax >= 1 && csf >= 1 && n_rest >= 1 && n_rest <= 15 && inner >= 1 && rf >= 1 && rr >= 1, "rvq_gather: sizes out of range");
            pl.in[0] = elems(B, csf, 16); pl.in[1] = elems(rf, inner); pl.in[2] = kPool; pl.in[3] = B * 4;
            pl.in[4] = B * 4; pl.in_opt[4] = true; pl.in[5] = n_rest * 8;
            pl.io[0] = elems(B, Fmax, 2, inner);
            check_slots(d, pl);
            const int32_t *fr = i32(d.in[3]), *ff = i32(d.in[4]);
            for (int b = 0; b < B; ++b) {
                const int64_t f0 = ff ? ff[b] : 0;
                ROW_CHECK(fr[b] >= 0 && fr[b] <= Fmax && f0 >= 0 && f0 + fr[b] <= csf, "rvq_gather: frames / first_frame outside the code rows");
            }
            for (int j = 0; j < n_rest; ++j) {
                const int64_t off = i64(d.in[5])[j];
                ROW_CHECK(off >= 0 && off <= d.in_bytes[2] / 4 && off + int64_t(rr) * inner <= d.in_bytes[2] / 4, "rvq_gather: a codebook ends outside the pool");
            }
            break;
        }
        case 1: case 3: {  // rmsnorm_f32, silu_mul_f32
            const int B = p[0], Tmax = p[1], ppf = p[2], C = p[3];
            batch(B);
            ROW_CHECK(Tmax >= 1 && ppf >= 1 && C >= 1, "sizes out of range");
            if (d.op == 1) { pl.in[0] = elems(B, Tmax, C); pl.in[1] = C * 4; pl.in[2] = B * 4; }
            else { pl.in[0] = elems(B, Tmax, 2, C); pl.in[1] = B * 4; }
            pl.io[0] = elems(B, Tmax, C);
            check_slots(d, pl);
            check_frames(d, d.op == 1 ? 2 : 1, B, ppf, 0, Tmax);
            break;
        }
        case 2: {  // dwconv_ln
            const int B = p[0], Tmax = p[1], ppf = p[2], C = p[3], hist = p[4], margin = p[5];
            batch(B);
            ROW_CHECK(Tmax >= 1 && ppf >= 1 && C >= 1 && C <= 4096, "dwconv_ln: 1 <= C <= 4096");
            ROW_CHECK(hist >= 0 && hist <= margin && margin <= Tmax, "dwconv_ln: 0 <= hist <= margin <= Tmax");
            pl.in[0] = elems(B, Tmax, C); pl.in[1] = int64_t(C) * 7 * 4; pl.in[2] = pl.in[3] = pl.in[4] = C * 4; pl.in[5] = B * 4;
            pl.io[0] = pl.in[0];
            check_slots(d, pl);
            check_frames(d, 5, B, ppf, margin, Tmax);
            break;
        }
        case 4: {  // attn_full_f32
            const int B = p[0], Tmax = p[1], heads = p[2];
            batch(B);
            ROW_CHECK(Tmax >= 1 && heads >= 1 && heads <= 64, "attn_full_f32: sizes out of range");
            pl.in[0] = elems(B, Tmax, 3 * heads * 64); pl.in[1] = B * 4;
            pl.io[0] = elems(B, Tmax, heads * 64);
            check_slots(d, pl);
            check_frames(d, 1, B, 1, 0, Tmax);
            break;
        }
        case 5: {  // roll_history
            const int B = p[0];
            const int64_t bstride = p[1], keep = p[2], chunk = p[3];
            batch(B);
            ROW_CHECK(keep >= 0 && keep % 4 == 0 && chunk >= keep && chunk >= 1, "roll_history: keep % 4 == 0, chunk >= keep");
            ROW_CHECK(chunk % 4 == 0 && bstride % 4 == 0 && bstride >= keep + chunk, "roll_history: chunk and bstride in whole float4s, bstride >= keep + chunk");
            pl.io[0] = elems((B - 1) * bstride + keep + chunk);
            check_slots(d, pl);
            break;
        }
        case 6: {  // roll_history_rows
            const int B = p[0], Tal = p[1], hist = p[2], chunk = p[3], n_desc = p[4], only_row = p[5];
            batch(B);
            ROW_CHECK(hist >= 0 && chunk >= 1 && chunk >= hist && Tal == hist + chunk, "roll_history_rows: chunk >= hist && Tal == hist + chunk");
            ROW_CHECK(n_desc >= 1 && n_desc <= 16, "roll_history_rows: 1..16 tensors");
            pl.in[0] = n_desc * 24; pl.in[1] = pl.in[2] = B * 4; pl.in_opt[1] = pl.in_opt[2] = true;
            pl.io[0] = kPool; pl.io[1] = B * 4; pl.io_opt[1] = true;
            check_slots(d, pl);
            ROW_CHECK(d.in[1] != nullptr || (only_row >= 0 && only_row < B), "roll_history_rows: only_row outside the stream");
            if (d.in[1])
                for (int b = 0; b < B; ++b) ROW_CHECK(i32(d.in[1])[b] >= 0 && i32(d.in[1])[b] <= 2, "roll_history_rows: mode in 0..2");
            check_desc(d, n_desc, B, Tal);
            break;
        }
        case 7: {  // history_state_rows
            const int B = p[0], Tal = p[1], hist = p[2], n_desc = p[3], row = p[4];
            batch(B);
            ROW_CHECK(hist >= 0 && Tal >= 1 && hist <= Tal && n_desc >= 1 && n_desc <= 16 && row >= 0 && row < B, "history_state_rows: sizes / row out of range");
            pl.in[0] = n_desc * 24;
            pl.io[0] = kPool; pl.io[1] = kPool; pl.io[2] = B * 4; pl.io_opt[2] = true;
            check_slots(d, pl);
            check_desc(d, n_desc, B, Tal);
            std::vector<std::pair<int64_t, int64_t>> r;
            for (int i = 0; i < n_desc; ++i) {
                const int64_t so = i64(d.in[0])[3 * i + 2], bytes = int64_t(hist) * i64(d.in[0])[3 * i + 1] * 4;
                ROW_CHECK(so >= 0 && so % 16 == 0 && so <= d.io_bytes[1] && so + bytes <= d.io_bytes[1], "history_state_rows: state_off 16-byte aligned and inside the blob");
                r.emplace_back(so, so + bytes);
            }
            check_disjoint(r, "debug_rowop: history_state_rows: blob ranges overlap");
            break;
        }
        case 8: {  // stream_take_chunk
            const int B = p[0];
            const int64_t fbs = p[1], lbs = p[2], latent = p[3], max_take = p[4], lat_off = p[5];
            batch(B);
            ROW_CHECK(latent >= 4 && latent % 4 == 0 && fbs >= 4 && fbs % 4 == 0 && lbs >= 4 && lbs % 4 == 0 && lat_off >= 0 && lat_off % 4 == 0 && lat_off < lbs && max_take >= 0,
                      "stream_take_chunk: latent, strides and lat_off in whole float4s");
            pl.in[0] = elems(B, fbs); pl.in[1] = pl.in[2] = B * 4;
            pl.io[0] = elems(B, lbs);
            check_slots(d, pl);
            for (int b = 0; b < B; ++b) {
                const int64_t off = i32(d.in[1])[b], take = i32(d.in[2])[b];
                ROW_CHECK(take <= max_take, "stream_take_chunk: take[b] > max_take");
                if (take > 0) {
                    ROW_CHECK(off >= 0 && (off + take) * latent <= fbs, "stream_take_chunk: off + take outside the front buffer");
                    ROW_CHECK(lat_off + take * latent <= lbs, "stream_take_chunk: take outside the latent row");
                }
            }
            break;
        }
        case 9: {  // enc_init_conv
            const int B = p[0];
            const int64_t S = p[1], C = p[2], K = p[3], obs = p[4];
            batch(B);
            ROW_CHECK(K >= 1 && K <= 17, "enc_init_conv: 1 <= K <= 17");
            ROW_CHECK(S >= 1 && C >= 1 && C <= 4096 && S * C <= kMaxElems && obs >= S * C, "enc_init_conv: sizes out of range, out_bstride >= S * C");
            pl.in[0] = elems(B, S); pl.in[1] = C * K * 4; pl.in[2] = C * 4;
            pl.io[0] = elems(B, obs);
            check_slots(d, pl);
            break;
        }
        case 10: {  // layernorm_f32
            const int B = p[0];
            const int64_t T = p[1], C = p[2], xbs = p[3], obs = p[4];
            batch(B);
            ROW_CHECK(T >= 1 && C >= 1 && T * C <= kMaxElems && xbs >= T * C && obs >= T * C, "layernorm_f32: strides >= T * C");
            pl.in[0] = elems(B, xbs); pl.in[1] = pl.in[2] = C * 4;
            pl.io[0] = elems(B, obs);
            check_slots(d, pl);
            break;
        }
        case 11: case 12: {  // rope_qk_f32, attn_causal_f32
            const int B = p[0], T = p[1], heads = p[2];
            batch(B);
            ROW_CHECK(T >= 1 && heads >= 1 && heads <= 64, "sizes out of range");
            if (d.op == 11) {
                pl.in[0] = pl.in[1] = elems(T, 32);
                pl.io[0] = elems(B, T, 3 * heads * 64);
            } else {
                pl.in[0] = elems(B, T, 3 * heads * 64);
                pl.io[0] = elems(B, T, heads * 64);
            }
            check_slots(d, pl);
            break;
        }
        case 13: {  // rvq_encode
            const int B = p[0], Tmax = p[1], n_layers = p[6], layer0 = p[7];
            const int64_t ldx = p[2], xbs = p[3], dim = p[4], bins = p[5], xcol = p[8];
            batch(B);
            ROW_CHECK(dim >= 1 && dim <= 4096, "rvq_encode: 1 <= dim <= 4096 (the residual in LDS)");
            ROW_CHECK(Tmax >= 1 && bins >= 1 && bins <= 65536 && n_layers >= 1 && n_layers <= 16 && layer0 >= 0 && layer0 <= 16, "rvq_encode: sizes out of range");
            ROW_CHECK(xcol >= 0 && ldx >= 1 && xcol + dim <= ldx && xbs >= 1, "rvq_encode: columns xcol .. xcol + dim outside a row of x");
            pl.in[0] = elems(B, xbs); pl.in[1] = B * 4; pl.in[2] = B * 8; pl.in[3] = kPool; pl.in[4] = kPool; pl.in[5] = pl.in[6] = n_layers * 8;
            pl.io[0] = kPool;
            check_slots(d, pl);
            std::vector<std::pair<int64_t, int64_t>> r;
            const int64_t ncodes = d.io_bytes[0] / 4;
            for (int b = 0; b < B; ++b) {
                const int64_t T = i32(d.in[1])[b], off = i64(d.in[2])[b];
                ROW_CHECK(T >= 0 && T <= Tmax && T * ldx <= xbs, "rvq_encode: valid[b] outside the batch row");
                ROW_CHECK(off >= 0 && off <= ncodes && off + (layer0 + n_layers) * T <= ncodes, "rvq_encode: a code range ends outside codes");
                if (T > 0) r.emplace_back(off, off + (layer0 + n_layers) * T);
            }
            check_disjoint(r, "debug_rowop: rvq_encode: code ranges overlap");
            for (int j = 0; j < n_layers; ++j) {
                const int64_t co = i64(d.in[5])[j], c2o = i64(d.in[6])[j];
                ROW_CHECK(co >= 0 && co <= d.in_bytes[3] / 4 && co + bins * dim <= d.in_bytes[3] / 4, "rvq_encode: a codebook ends outside the pool");
                ROW_CHECK(c2o >= 0 && c2o <= d.in_bytes[4] / 4 && c2o + bins <= d.in_bytes[4] / 4, "rvq_encode: a c2 table ends outside the pool");
            }
            break;
        }
        case 14: {  // log_mel
            const int64_t T = p[0], ld = p[1], nfreq = p[2], n_mels = p[3];
            ROW_CHECK(T >= 1 && n_mels >= 1 && nfreq >= 1 && nfreq * 4 <= 64 * 1024, "log_mel: nfreq floats of LDS <= 64 KiB");
            ROW_CHECK(ld >= 2 * nfreq, "log_mel: ld >= 2 nfreq");
            pl.in[0] = elems(T, ld); pl.in[1] = elems(nfreq, n_mels);
            pl.io[0] = elems(T, n_mels);
            check_slots(d, pl);
            break;
        }
        case 15: {  // time_stats
            const int64_t T = p[0], C = p[1], ld = p[2];
            ROW_CHECK(T >= 1 && C >= 1 && ld >= C, "time_stats: T >= 1, ld >= C");
            pl.in[0] = elems(T, ld);
            pl.io[0] = pl.io[1] = C * 4; pl.io_opt[1] = true;
            check_slots(d, pl);
            break;
        }
        case 16: {  // scale_res
            const int64_t T = p[0], C = p[1];
            ROW_CHECK(T >= 1 && C >= 1 && p[2] >= C && p[3] >= C && p[4] >= C && T * C <= kMaxElems, "scale_res: ld >= C");
            pl.in[0] = elems(T, p[2]); pl.in[1] = C * 4; pl.in[2] = elems(T, p[3]);
            pl.io[0] = elems(T, p[4]);
            check_slots(d, pl);
            break;
        }
        case 17: case 18: {  // asp_concat, asp_pool
            const int64_t T = p[0], C = p[1];
            ROW_CHECK(T >= 1 && C >= 1, "sizes out of range");
            pl.in[0] = elems(T, C);
            if (d.op == 17) { pl.in[1] = pl.in[2] = C * 4; pl.io[0] = elems(T, 3, C); }
            else { pl.in[1] = pl.in[0]; pl.io[0] = 2 * C * 4; }
            check_slots(d, pl);
            break;
        }
        case 19: {  // mask_tail
            const int B = p[0];
            const int64_t Tpad = p[1], C = p[2], bs = p[3];
            batch(B);
            ROW_CHECK(Tpad >= 1 && C >= 1 && Tpad * C <= kMaxElems && bs >= Tpad * C, "mask_tail: bstride >= Tpad * C");
            pl.in[0] = B * 4;
            pl.io[0] = elems(B, bs);
            check_slots(d, pl);
            for (int b = 0; b < B; ++b) ROW_CHECK(i32(d.in[0])[b] >= 0 && i32(d.in[0])[b] <= Tpad, "mask_tail: valid[b] outside 0..Tpad");
            break;
        }
        default: {  // copy2d_f32
            const int64_t T = p[0], C = p[1];
            ROW_CHECK(T >= 1 && C >= 1 && p[2] >= C && p[3] >= C && T * C <= kMaxElems, "copy2d_f32: ld >= C");
            pl.in[0] = elems(T, p[2]);
            pl.io[0] = elems(T, p[3]);
            check_slots(d, pl);
            break;
        }
    }
}

void Engine::debug_rowop(q3tts_rowop_debug& d) {
    debug_rowop_check(d);
    DevBuf<uint8_t> din[kIn], dio[kIo], dtab[3];
    const uint8_t* in[kIn] = {};
    uint8_t* io[kIo] = {};
    for (int i = 0; i < kIn; ++i)
        if (d.in[i]) {
            in[i] = din[i].grow(size_t(d.in_bytes[i]));
            Q3_HIP(hipMemcpy(din[i], d.in[i], size_t(d.in_bytes[i]), hipMemcpyHostToDevice));
        }
    for (int i = 0; i < kIo; ++i)
        if (d.io[i]) {
            io[i] = dio[i].grow(size_t(d.io_bytes[i]));
            Q3_HIP(hipMemcpy(dio[i], d.io[i], size_t(d.io_bytes[i]), hipMemcpyHostToDevice));
        }
    auto F = [&](int i) { return reinterpret_cast<const float*>(in[i]); };
    auto I = [&](int i) { return reinterpret_cast<const int32_t*>(in[i]); };
    auto O = [&](int i) { return reinterpret_cast<float*>(io[i]); };
    auto OI = [&](int i) { return reinterpret_cast<int32_t*>(io[i]); };
    // a device table (pointers, RollDesc, the transposed codebooks) built on the host
    auto table = [&](DevBuf<uint8_t>& b, const void* host, size_t bytes) -> const void* {
        b.grow(bytes);
        Q3_HIP(hipMemcpy(b, host, bytes, hipMemcpyHostToDevice));
        return b;
    };
    auto roll_table = [&](int n_desc, int64_t& max_ff) {
        std::vector<RollDesc> t(static_cast<size_t>(n_desc));
        max_ff = 0;
        for (int i = 0; i < n_desc; ++i) {
            const int64_t* h = i64(d.in[0]) + 3 * i;
            t[size_t(i)] = RollDesc{O(0) + h[0], h[1], h[2]};
            max_ff = std::max(max_ff, h[1]);
        }
        return static_cast<const RollDesc*>(table(dtab[0], t.data(), t.size() * sizeof(RollDesc)));
    };
    const int32_t* p = d.p;
    switch (d.op) {
        case 0: {
            std::vector<const float*> t(static_cast<size_t>(p[3]));
            for (int j = 0; j < p[3]; ++j) t[size_t(j)] = F(2) + i64(d.in[5])[j];
            const auto* tab = static_cast<const float* const*>(table(dtab[0], t.data(), t.size() * sizeof(float*)));
            launch_rvq_gather(I(0), p[2], F(1), tab, p[3], p[4], I(3), p[1], p[0], O(0), p[5], p[6], st_, I(4));
            break;
        }
        case 1: launch_rmsnorm_f32(F(0), F(1), d.f[0], p[3], I(2), p[2], p[1], p[0], O(0), st_); break;
        case 2:
            launch_dwconv_ln(F(0) + int64_t(p[5]) * p[3], F(1), F(2), F(3), F(4), d.f[0], p[3], I(5), p[2], p[1], p[0], O(0) + int64_t(p[5]) * p[3], st_, p[4]);
            break;
        case 3: launch_silu_mul_f32(F(0), p[3], I(1), p[2], p[1], p[0], O(0), st_); break;
        case 4: launch_attn_full_f32(F(0), p[2], I(1), p[1], p[0], O(0), st_); break;
        case 5: launch_roll_history(O(0) + p[2], p[1], p[2], p[3], p[0], st_); break;
        case 6: {
            int64_t max_ff = 0;
            const RollDesc* tab = roll_table(p[4], max_ff);
            launch_roll_history_rows(tab, p[4], max_ff, p[1], p[2], p[3], I(1), p[5], p[0], OI(1), st_, I(2));
            break;
        }
        case 7: {
            int64_t max_ff = 0;
            const RollDesc* tab = roll_table(p[3], max_ff);
            launch_history_state_rows(tab, p[3], max_ff, p[1], p[2], p[4], p[0], io[1], p[5] != 0, OI(2), st_);
            break;
        }
        case 8: launch_stream_take_chunk(F(0), p[1], O(0) + p[5], p[2], p[3], p[4], I(1), I(2), p[0], st_); break;
        case 9: launch_enc_init_conv(F(0), p[1], p[0], F(1), F(2), p[2], p[3], O(0), p[4], st_); break;
        case 10: launch_layernorm_f32(F(0), p[3], F(1), F(2), d.f[0], p[2], p[1], p[0], O(0), p[4], st_); break;
        case 11: launch_rope_qk_f32(O(0), p[2], p[1], p[0], F(0), F(1), st_); break;
        case 12: launch_attn_causal_f32(F(0), p[2], p[1], p[0], O(0), st_); break;
        case 13: {
            const int dim = p[4], bins = p[5], n_layers = p[6];
            const size_t per = size_t(dim) * bins;
            std::vector<float> all(per * n_layers), embt;
            for (int j = 0; j < n_layers; ++j) {  // [bins][dim] as a checkpoint holds it -> the loader's [dim][bins]
                transpose_codebook(static_cast<const float*>(d.in[3]) + i64(d.in[5])[j], bins, dim, embt);
                std::copy(embt.begin(), embt.end(), all.begin() + per * j);
            }
            const float* cbt = static_cast<const float*>(table(dtab[0], all.data(), all.size() * 4));
            std::vector<const float*> tc(static_cast<size_t>(n_layers)), t2(static_cast<size_t>(n_layers));
            for (int j = 0; j < n_layers; ++j) {
                tc[size_t(j)] = cbt + per * j;
                t2[size_t(j)] = F(4) + i64(d.in[6])[j];
            }
            const auto* cb = static_cast<const float* const*>(table(dtab[1], tc.data(), tc.size() * sizeof(float*)));
            const auto* c2 = static_cast<const float* const*>(table(dtab[2], t2.data(), t2.size() * sizeof(float*)));
            launch_rvq_encode(F(0) + p[8], p[2], p[3], p[1], p[0], I(1), reinterpret_cast<const int64_t*>(in[2]), dim, bins, cb, c2, n_layers, p[7], OI(0), st_);
            break;
        }
        case 14: launch_log_mel(F(0), p[1], p[0], p[2], F(1), p[3], O(0), st_); break;
        case 15: launch_time_stats(F(0), p[2], p[0], p[1], O(0), O(1), d.f[0], st_); break;
        case 16: launch_scale_res(F(0), p[2], F(1), F(2), p[3], O(0), p[4], p[0], p[1], st_); break;
        case 17: launch_asp_concat(F(0), F(1), F(2), p[0], p[1], O(0), st_); break;
        case 18: launch_asp_pool(F(0), F(1), p[0], p[1], d.f[0], O(0), st_); break;
        case 19: launch_mask_tail(O(0), p[3], I(0), p[1], p[2], p[0], st_); break;
        default: launch_copy2d_f32(F(0), p[2], O(0), p[3], p[0], p[1], st_); break;
    }
    Q3_HIP(hipGetLastError());
    Q3_HIP(hipStreamSynchronize(st_));
    for (int i = 0; i < kIo; ++i)
        if (d.io[i]) Q3_HIP(hipMemcpy(d.io[i], dio[i], size_t(d.io_bytes[i]), hipMemcpyDeviceToHost));
}

}  // namespace q3
