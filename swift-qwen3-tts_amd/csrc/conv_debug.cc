// conv_debug.cc -- q3tts_debug_conv (q3tts.h): one launch of a codec conv launcher on host buffers. The host checks and the
// geometry need neither an engine nor a GPU; weights and SnakeBeta parameters are packed by the loader's own functions (model.h).
#include <cstring>
#include <vector>

#include "codec_kernels.h"
#include "common.h"
#include "engine.h"

namespace q3 {

namespace {

// Device addresses of one launch. For the geometry any non-null address stands for "this operand takes part".
struct ConvPtrs {
    const void* x = nullptr;
    const float* x2 = nullptr;
    const float* w = nullptr;        // fp32 [N][K][Cin] (kind 0; the out-convs' taps)
    const uint16_t* wh = nullptr;    // pack_conv_h2 (kind 0 split, kind 1 conv1)
    const float* wsc = nullptr;
    const uint16_t* w2ph = nullptr;  // pack_conv_h2_perm (kind 1 conv2)
    const float* wsc2 = nullptr;
    const uint16_t* w1 = nullptr;    // pack_conv_h1 (kinds 2, 3)
    const uint16_t* w2p = nullptr;   // pack_conv_h1_perm (kind 3 conv2)
    const float* bias = nullptr;
    const float* bias2 = nullptr;
    const float* scale = nullptr;
    const float* ea = nullptr;       // snake_* as the kernels take it
    const float* ib = nullptr;
    const float* ea2 = nullptr;
    const float* ib2 = nullptr;
    const float* pea = nullptr;
    const float* pib = nullptr;
    const void* res = nullptr;
    void* out = nullptr;
    void* out2 = nullptr;
    const int32_t* frames = nullptr;
    float* pcm = nullptr;
    int32_t* nonfinite = nullptr;
};

template <class T>
T* rows_in(const void* p, int64_t elems) {  // row 0 of the sequences sits behind the history margin
    return p ? const_cast<T*>(static_cast<const T*>(p)) + elems : nullptr;
}

ConvGemmArgs conv_args(const q3tts_conv_debug& d, const ConvPtrs& p) {
    ConvGemmArgs a{};
    a.x = rows_in<float>(p.x, int64_t(d.margin) * d.ldx); a.ldx = d.ldx; a.x_bstride = int64_t(d.Tmax) * d.ldx;
    a.w = p.w; a.wh = p.wh; a.wsc = p.wsc; a.bias = p.bias; a.scale = p.scale;
    a.res = rows_in<float>(p.res, int64_t(d.margin) * d.ldr); a.ldr = d.ldr; a.res_bstride = int64_t(d.Tmax) * d.ldr;
    a.out = rows_in<float>(p.out, int64_t(d.margin) * d.ldo); a.ldo = d.ldo; a.out_bstride = int64_t(d.Tmax) * d.ldo;
    a.out2 = rows_in<float>(p.out2, int64_t(d.margin) * d.ldo);
    a.post_ea = p.pea; a.post_ib = p.pib; a.post_C = d.post_C;
    a.snake_ea = p.ea; a.snake_ib = p.ib;
    a.frames = p.frames; a.ppf = d.ppf; a.Tmax = d.Tmax; a.B = d.B; a.Cin = d.Cin; a.N = d.N; a.K = d.K; a.dil = d.dil;
    a.act = d.act; a.pre_act = d.pre_act;
    a.x2 = rows_in<float>(p.x2, int64_t(d.margin) * d.ldx2); a.ldx2 = d.ldx2;
    a.shift = d.shift; a.reflect = d.reflect; a.hist = d.hist;
    return a;
}

ResUnitArgs unit_args(const q3tts_conv_debug& d, const ConvPtrs& p) {
    ResUnitArgs r{};
    const int64_t m = int64_t(d.margin) * d.N;
    r.y = rows_in<float>(p.x, m); r.out = rows_in<float>(p.out, m); r.out2 = rows_in<float>(p.out2, m);
    r.post_ea = p.pea; r.post_ib = p.pib; r.b1 = p.bias; r.b2 = p.bias2;
    r.w1h = p.wh; r.w2ph = p.w2ph; r.wsc1 = p.wsc; r.wsc2 = p.wsc2;
    r.ea1 = p.ea; r.ib1 = p.ib; r.ea2 = p.ea2; r.ib2 = p.ib2;
    r.frames = p.frames; r.ppf = d.ppf; r.Tmax = d.Tmax; r.B = d.B; r.C = d.N; r.K = d.K; r.dil = d.dil; r.hist = d.hist;
    return r;
}

ConvH1Args conv_h1_args(const q3tts_conv_debug& d, const ConvPtrs& p) {
    ConvH1Args a{};
    a.x = d.x_f32 ? static_cast<const void*>(rows_in<float>(p.x, int64_t(d.margin) * d.ldx))
                  : static_cast<const void*>(rows_in<uint16_t>(p.x, int64_t(d.margin) * d.ldx));
    a.x_f32 = d.x_f32 ? 1 : 0; a.ldx = d.ldx; a.x_bstride = int64_t(d.Tmax) * d.ldx;
    a.w1 = p.w1; a.bias = p.bias;
    a.res = rows_in<uint16_t>(p.res, int64_t(d.margin) * d.ldr); a.ldr = d.ldr; a.res_bstride = int64_t(d.Tmax) * d.ldr;
    a.out = rows_in<uint16_t>(p.out, int64_t(d.margin) * d.ldo); a.ldo = d.ldo; a.out_bstride = int64_t(d.Tmax) * d.ldo;
    a.out2 = rows_in<uint16_t>(p.out2, int64_t(d.margin) * d.ldo);
    a.post_ea = p.pea; a.post_ib = p.pib; a.post_C = d.post_C;
    a.frames = p.frames; a.ppf = d.ppf; a.Tmax = d.Tmax; a.B = d.B; a.Cin = d.Cin; a.N = d.N; a.K = d.K; a.dil = d.dil; a.hist = d.hist;
    return a;
}

ResUnitH1Args unit_h1_args(const q3tts_conv_debug& d, const ConvPtrs& p) {
    ResUnitH1Args r{};
    const int64_t m = int64_t(d.margin) * d.N;
    r.y = rows_in<uint16_t>(p.x, m); r.out = rows_in<uint16_t>(p.out, m); r.out2 = rows_in<uint16_t>(p.out2, m);
    r.post_ea = p.pea; r.post_ib = p.pib; r.b1 = p.bias; r.b2 = p.bias2;
    r.w1 = p.w1; r.w2p = p.w2p;
    r.ea1 = p.ea; r.ib1 = p.ib; r.ea2 = p.ea2; r.ib2 = p.ib2;
    r.frames = p.frames; r.ppf = d.ppf; r.Tmax = d.Tmax; r.B = d.B; r.C = d.N; r.dil = d.dil; r.hist = d.hist;
    return r;
}

ConvDispatch dispatch_of(const q3tts_conv_debug& d, const ConvPtrs& p) {
    switch (d.kind) {
        case 0: return conv_gemm_dispatch(conv_args(d, p));
        case 1: return resunit_dispatch(unit_args(d, p));
        case 2: return conv_gemm_h1_dispatch(conv_h1_args(d, p));
        case 3: return resunit_h1_dispatch(unit_h1_args(d, p));
        default: return out_conv_dispatch(d.Cin, d.Tmax, d.B, d.kind == 5);
    }
}

}  // namespace

// Everything the kernels turn into an address is checked here against the sizes the caller states.
void Engine::debug_conv_check(q3tts_conv_debug& d) {
    static const float dummy = 0.f;  // the geometry: "this operand takes part" without a buffer
    d.family = d.BN = d.pro = d.pw_depth = d.KT = d.X32 = d.CT2 = d.PT = d.wdb = d.grid_x = d.grid_y = d.grid_z = 0;
    d.lds_bytes = 0;
    Q3_CHECK(d.kind >= 0 && d.kind <= 5, 3, "debug_conv: unknown kind");
    const bool unit = d.kind == 1 || d.kind == 3, outc = d.kind >= 4;
    Q3_CHECK(d.B >= 1 && d.B <= 64 && d.Tmax >= 1 && d.Tmax <= (1 << 20) && d.ppf >= 1 && d.ppf <= 4096 && d.hist >= 0 && d.hist <= d.margin && d.margin <= d.Tmax, 3,
             "debug_conv: batch / length out of range");
    Q3_CHECK(d.Cin >= 4 && d.Cin <= 4096 && d.K >= 1 && d.K <= 64 && d.dil >= 1 && d.dil <= 64, 3, "debug_conv: Cin / K / dil out of range");
    Q3_CHECK((d.K - 1) * d.dil <= 56, 3, "debug_conv: receptive field too large ((K - 1) * dil <= 56)");
    const int cm = (d.kind == 2 || d.kind == 3) ? 8 : 4;  // sixteen-byte pieces of the staged input
    Q3_CHECK(d.Cin % cm == 0 && d.ldx >= d.Cin && d.ldx <= d.Cin + 1024 && d.ldx % cm == 0, 3,
             "debug_conv: Cin and ldx must be multiples of 4 (kinds 2 and 3: of 8), ldx >= Cin");
    if (outc) {
        Q3_CHECK(d.K == 7 && d.dil == 1 && d.ldx == d.Cin, 3, "debug_conv: the out-convs have seven taps, dilation 1 and dense rows");
        Q3_CHECK(!d.res && !d.res_is_out && !d.out && !d.out2 && !d.scale && !d.bias2 && !d.w2 && !d.act2_alpha && !d.act2_beta && !d.post_alpha && !d.post_beta, 3,
                 "debug_conv: an out-conv takes x, w, bias, snake_*, pcm and nonfinite only");
        Q3_CHECK(d.snake_alpha && d.snake_beta && d.w && d.pcm && (d.kind == 5 || d.bias), 3, "debug_conv: null out-conv argument");
    } else {
        Q3_CHECK(d.N >= 4 && d.N <= 4096 && d.N % 4 == 0 && d.ldo >= d.N && d.ldo <= d.N + 1024 && d.ldo % 4 == 0, 3,
                 "debug_conv: N and ldo must be multiples of 4, ldo >= N");
        Q3_CHECK(!d.pcm && !d.nonfinite, 3, "debug_conv: pcm / nonfinite belong to the out-convs");
        Q3_CHECK(d.w && (d.out || d.out2), 3, "debug_conv: null argument (w; out or out2)");
        Q3_CHECK(!d.res_is_out || d.out, 3, "debug_conv: res_is_out without out");
        if (d.res || d.res_is_out) {
            Q3_CHECK(!unit, 3, "debug_conv: a fused unit's residual is its input");
            Q3_CHECK(d.ldr >= d.N && d.ldr <= d.N + 1024 && d.ldr % 4 == 0 && (!d.res_is_out || d.ldr == d.ldo), 3, "debug_conv: ldr");
        }
        Q3_CHECK((d.post_alpha != nullptr) == (d.out2 != nullptr) && (d.post_beta != nullptr) == (d.out2 != nullptr), 3,
                 "debug_conv: post_alpha / post_beta go with out2");
        if (d.out2 && !unit) Q3_CHECK(d.post_C >= 4 && d.post_C % 4 == 0 && d.N % d.post_C == 0, 3, "debug_conv: post_C must be a multiple of 4 dividing N");
        Q3_CHECK((d.snake_alpha != nullptr) == (d.snake_beta != nullptr) && (d.act2_alpha != nullptr) == (d.act2_beta != nullptr), 3,
                 "debug_conv: alpha and beta go together");
    }
    Q3_CHECK(d.act >= 0 && d.act <= 5 && d.pre_act >= 0 && d.pre_act <= 1 && (d.reflect == 0 || d.reflect == 1) && d.shift >= 0 &&
                 d.shift <= (d.K - 1) * d.dil, 3, "debug_conv: act / pre_act / shift / reflect out of range");
    if (d.kind != 0) {
        Q3_CHECK(!d.split && !d.act && !d.pre_act && !d.shift && !d.reflect && !d.x2 && !d.scale, 3,
                 "debug_conv: split, act, pre_act, shift, reflect, x2 and scale belong to kind 0");
        Q3_CHECK(d.kind == 2 || !d.x_f32, 3, "debug_conv: x_f32 belongs to kind 2");
        Q3_CHECK(d.kind != 2 || !d.snake_alpha, 3, "debug_conv: the float16 conv has no prologue");
    } else {
        Q3_CHECK(!d.x_f32 && !d.w2 && !d.bias2 && !d.act2_alpha, 3, "debug_conv: x_f32, w2, bias2 and act2 belong to other kinds");
        if (d.x2) Q3_CHECK(d.B == 1 && d.ldx2 >= d.Cin && d.ldx2 <= d.Cin + 1024 && d.ldx2 % 4 == 0, 3, "debug_conv: x2 is single-row (B == 1), ldx2 >= Cin, a multiple of 4");
    }
    if (unit) {
        Q3_CHECK(d.Cin == d.N && d.ldx == d.N && d.ldo == d.N, 3, "debug_conv: a fused unit has Cin == N == ldx == ldo");
        Q3_CHECK(d.kind == 1 ? resunit_supported(d.N, d.K, d.dil) : (d.K == 7 && resunit_h1_supported(d.N, d.K, d.dil)), 3,
                 "debug_conv: the fused unit does not support this (C, K, dil)");
        Q3_CHECK(d.out && d.w2 && d.snake_alpha && d.act2_alpha, 3, "debug_conv: a fused unit needs out, w2, snake_* (act1) and act2_*");
    }
    Q3_CHECK(d.geometry_only || (d.frames && d.x), 3, "debug_conv: null argument (frames, x)");
    if (d.frames)
        for (int b = 0; b < d.B; ++b) {
            const int64_t T = int64_t(d.frames[b]) * d.ppf;
            Q3_CHECK(d.frames[b] >= 0 && d.margin + T <= d.Tmax, 3, "debug_conv: margin + frames[b] * ppf must not exceed Tmax");
            // reflect: rows -( halo - shift ) .. T - 1 + shift are read; their mirror images must be rows of the sequence
            if (d.reflect && T > 0) Q3_CHECK((d.K - 1) * d.dil - d.shift <= T - 1 && d.shift <= T - 1, 3, "debug_conv: reflect padding wider than the sequence");
        }
    else Q3_CHECK(!d.reflect || d.geometry_only, 3, "debug_conv: reflect needs frames");
    const int64_t ldmax = std::max(std::max(d.ldx, d.ldo), std::max(d.ldr, d.ldx2));
    Q3_CHECK(int64_t(d.B) * d.Tmax * ldmax <= (int64_t(1) << 27), 3, "debug_conv: tensors beyond 2^27 elements");

    ConvPtrs p;
    const void* any = &dummy;
    auto on = [&](const void* v) { return v ? any : nullptr; };
    p.x = any; p.frames = static_cast<const int32_t*>(any);
    p.x2 = static_cast<const float*>(on(d.x2));
    p.bias = static_cast<const float*>(on(d.bias)); p.bias2 = static_cast<const float*>(on(d.bias2)); p.scale = static_cast<const float*>(on(d.scale));
    p.ea = p.ib = static_cast<const float*>(on(d.snake_alpha));
    p.ea2 = p.ib2 = static_cast<const float*>(on(d.act2_alpha));
    p.pea = p.pib = static_cast<const float*>(on(d.post_alpha));
    p.res = (d.res || d.res_is_out) ? any : nullptr;
    p.out = const_cast<void*>(on(d.out)); p.out2 = const_cast<void*>(on(d.out2));
    if (unit && p.out) p.out = const_cast<float*>(&dummy) + 1;  // (the launchers refuse out == y)
    if (d.kind == 0) {
        p.w = &dummy;
        if (d.split) { p.wh = static_cast<const uint16_t*>(any); p.wsc = &dummy; }
    } else if (d.kind == 1) {
        p.wh = p.w2ph = static_cast<const uint16_t*>(any); p.wsc = p.wsc2 = &dummy;
    } else if (d.kind == 2 || d.kind == 3) {
        p.w1 = p.w2p = static_cast<const uint16_t*>(any);
    }
    const ConvDispatch g = dispatch_of(d, p);
    d.family = g.family; d.BN = g.BN; d.pro = g.pro; d.pw_depth = g.pw_depth; d.KT = g.KT; d.X32 = g.X32; d.CT2 = g.CT2; d.PT = g.PT; d.wdb = g.wdb;
    d.grid_x = int32_t(g.gx); d.grid_y = int32_t(g.gy); d.grid_z = int32_t(g.gz);
    d.lds_bytes = int64_t(g.lds);
}

void Engine::debug_conv(q3tts_conv_debug& d) {
    debug_conv_check(d);
    const bool unit = d.kind == 1 || d.kind == 3, h1 = d.kind == 2 || d.kind == 3 || d.kind == 5, outc = d.kind >= 4;
    const int N = outc ? 1 : d.N;
    const size_t rows = size_t(d.B) * d.Tmax, esz = h1 ? 2 : 4;
    DevBuf<uint8_t> dx, dres, dout, dout2;
    DevBuf<float> dx2, dw, dwsc, dwsc2, dbias, dbias2, dscale, dpar[6], dpcm;
    DevBuf<uint16_t> dwh, dw2h;
    DevBuf<int32_t> dfr, dnf;
    auto upf = [&](DevBuf<float>& b, const float* src, size_t n) -> const float* {
        if (!src) return nullptr;
        b.grow(n);
        Q3_HIP(hipMemcpy(b, src, n * 4, hipMemcpyHostToDevice));
        return b;
    };
    auto up16 = [&](DevBuf<uint16_t>& b, const std::vector<uint16_t>& v) -> const uint16_t* {
        b.grow(v.size());
        Q3_HIP(hipMemcpy(b, v.data(), v.size() * 2, hipMemcpyHostToDevice));
        return b;
    };
    auto upb = [&](DevBuf<uint8_t>& b, const void* src, size_t bytes) -> uint8_t* {
        if (!src) return nullptr;
        b.grow(bytes);
        Q3_HIP(hipMemcpy(b, src, bytes, hipMemcpyHostToDevice));
        return b;
    };
    ConvPtrs p;
    dfr.grow(size_t(d.B));
    Q3_HIP(hipMemcpy(dfr, d.frames, size_t(d.B) * 4, hipMemcpyHostToDevice));
    p.frames = dfr;
    p.x = upb(dx, d.x, rows * d.ldx * ((h1 && !d.x_f32) ? 2 : 4));
    p.x2 = upf(dx2, d.x2, size_t(d.Tmax) * d.ldx2);
    p.bias = upf(dbias, d.bias, size_t(N));
    p.bias2 = upf(dbias2, d.bias2, size_t(N));
    p.scale = upf(dscale, d.scale, size_t(N));
    // SnakeBeta: raw alpha / beta through the loader's conversion (put_snake)
    auto snake = [&](const float* al, const float* be, int C, DevBuf<float>& bea, DevBuf<float>& bib, const float*& ea, const float*& ib) {
        if (!al) return;
        const std::vector<float> a(al, al + C), b(be, be + C);
        std::vector<float> e, i;
        if (h1) snake_params_f16(a, b, e, i);
        else snake_params(a, b, e, i);
        ea = upf(bea, e.data(), e.size());
        ib = upf(bib, i.data(), i.size());
    };
    snake(d.snake_alpha, d.snake_beta, d.Cin, dpar[0], dpar[1], p.ea, p.ib);
    snake(d.act2_alpha, d.act2_beta, d.N, dpar[2], dpar[3], p.ea2, p.ib2);
    snake(d.post_alpha, d.post_beta, unit ? d.N : d.post_C, dpar[4], dpar[5], p.pea, p.pib);
    // weights as the loader packs them (model.cc attach_*)
    ConvW cw;
    cw.N = N; cw.K = d.K; cw.Cin = d.Cin; cw.dil = d.dil;
    const std::vector<float> w(d.w, d.w + size_t(N) * d.K * d.Cin);
    std::vector<uint16_t> pk;
    std::vector<float> sc;
    if (d.kind == 0 || outc) p.w = upf(dw, w.data(), w.size());
    if ((d.kind == 0 && d.split) || d.kind == 1) {
        pack_conv_h2(cw, w, pk, sc);
        p.wh = up16(dwh, pk);
        p.wsc = upf(dwsc, sc.data(), sc.size());
    }
    if (d.kind == 2 || d.kind == 3) {
        pack_conv_h1(cw, w, pk);
        p.w1 = up16(dwh, pk);
    }
    if (unit) {
        ConvW c2;
        c2.N = d.N; c2.K = 1; c2.Cin = d.N;
        const std::vector<float> w2(d.w2, d.w2 + size_t(d.N) * d.N);
        if (d.kind == 1) {
            std::vector<uint16_t> plain;
            pack_conv_h2(c2, w2, plain, sc);  // (attach_h2's row scales, which attach_h2_perm's copy shares)
            pack_conv_h2_perm(c2, w2, pk);
            p.w2ph = up16(dw2h, pk);
            p.wsc2 = upf(dwsc2, sc.data(), sc.size());
        } else {
            pack_conv_h1_perm(c2, w2, pk);
            p.w2p = up16(dw2h, pk);
        }
    }
    p.out = upb(dout, d.out, rows * d.ldo * esz);
    p.out2 = upb(dout2, d.out2, rows * d.ldo * esz);
    p.res = d.res_is_out ? static_cast<const void*>(p.out) : upb(dres, d.res, rows * d.ldr * esz);
    if (outc) {
        dpcm.grow(rows);
        Q3_HIP(hipMemcpy(dpcm, d.pcm, rows * 4, hipMemcpyHostToDevice));
        p.pcm = dpcm;
        if (d.nonfinite) {
            dnf.grow(size_t(d.B));
            Q3_HIP(hipMemcpy(dnf, d.nonfinite, size_t(d.B) * 4, hipMemcpyHostToDevice));
            p.nonfinite = dnf;
        }
    }
    const ConvDispatch g = dispatch_of(d, p);  // with the real operands: must be what the check reported
    Q3_CHECK(g.family == d.family && g.BN == d.BN && g.pro == d.pro && int64_t(g.lds) == d.lds_bytes && int32_t(g.gx) == d.grid_x, 7,
             "debug_conv: the launch disagrees with the reported geometry");
    switch (d.kind) {
        case 0: launch_conv_gemm(conv_args(d, p), st_); break;
        case 1: launch_resunit(unit_args(d, p), st_); break;
        case 2: launch_conv_gemm_h1(conv_h1_args(d, p), st_); break;
        case 3: launch_resunit_h1(unit_h1_args(d, p), st_); break;
        case 4:
            launch_out_conv(rows_in<float>(p.x, int64_t(d.margin) * d.Cin), d.Cin, p.ea, p.ib, p.w, p.bias, p.frames, d.ppf, d.Tmax, d.B,
                            p.pcm + d.margin, st_, d.hist, p.nonfinite);
            break;
        default:
            launch_out_conv_h1(rows_in<uint16_t>(p.x, int64_t(d.margin) * d.Cin), d.Cin, p.ea, p.ib, p.w, p.bias, p.frames, d.ppf, d.Tmax, d.B,
                               p.pcm + d.margin, st_, p.nonfinite, d.hist);
            break;
    }
    Q3_HIP(hipGetLastError());  // an instantiation the device cannot launch must not pass as "nothing written"
    Q3_HIP(hipStreamSynchronize(st_));
    if (d.out) Q3_HIP(hipMemcpy(d.out, dout, rows * d.ldo * esz, hipMemcpyDeviceToHost));
    if (d.out2) Q3_HIP(hipMemcpy(d.out2, dout2, rows * d.ldo * esz, hipMemcpyDeviceToHost));
    if (outc) {
        Q3_HIP(hipMemcpy(d.pcm, dpcm, rows * 4, hipMemcpyDeviceToHost));
        if (d.nonfinite) Q3_HIP(hipMemcpy(d.nonfinite, dnf, size_t(d.B) * 4, hipMemcpyDeviceToHost));
    }
}

}  // namespace q3
