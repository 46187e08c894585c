// codec.cc -- codec decoder pipeline (codes -> PCM). See codec.h.
#include "codec.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <utility>

#include "codec_kernels.h"

namespace q3 {

namespace {
size_t kScratchBudget = size_t(24) << 30;  // activation scratch per group of rows (of 288 GB HBM); tests lower it
}
void CodecRunner::set_scratch_budget(size_t bytes) { kScratchBudget = bytes ? bytes : (size_t(24) << 30); }

CodecRunner::CodecRunner(const Model& m, hipStream_t st, bool fp32_convs, int output_rate, float speed, bool request_speeds,
                         float pitch, bool keep_formants)
    : m_(m), st_(st) {
    native_ = mid_ = up_ = m.cfg.codec.total_upsample();
    const bool other_rate = output_rate != 0 && output_rate != kResampleNative;
    int hL = 1, hM = 1;  // the handle's output rate over 24000, reduced
    if (other_rate && resample_rate_supported(output_rate)) {
        const int g = resample_detail::gcd(kResampleNative, output_rate);
        hL = output_rate / g;
        hM = kResampleNative / g;
    }
    if (pitch != 0.0f && (!other_rate || resample_rate_supported(output_rate))) {  // (an unsupported rate is refused below)
        Q3_CHECK(!request_speeds, 3, "Invalid input: pitch and request_speeds cannot be combined (a table per pair of hops)");
        Q3_CHECK(native_ % kStretchHa == 0, 3, "Invalid input: the codec's frame is not a whole number of 480-sample hops: no pitch other than 0");
        const int hops = native_ / kStretchHa;
        const PitchChoice pc = pitch_choose(pitch, speed, hops, hL, hM);
        Q3_CHECK(pc.status != 1, 3, "Invalid input: pitch must be 0 (off) or between -12 and 12 semitones");
        Q3_CHECK(pc.status != 2, 3, "Invalid input: speed must be 0 (off) or between 0.5 and 2.0");
        Q3_CHECK(pc.status == 0, 3, "Invalid input: no hop in [240, 960] for this pitch and speed");
        if (pc.on()) {
            pitched_ = true;
            ho_ = pc.ho;
            pitch_hp_ = pc.hp;
            out_rate_ = other_rate ? output_rate : kResampleNative;
            mid_ = hops * pc.hp;
            if (pc.hp != kStretchHa) {  // (Hp == 480: the resampler reads out_conv's signal, no stretch stage and no delay of one)
                st_plan_ = make_stretch_plan(pc.hp);
                Q3_CHECK(stretch_lookback(pc.hp) <= hist_frames() * native_, 7, "internal error: time stretch history beyond the stream's margin");
                stretch_ = true;
                Q3_HIP(hipMemcpy(st_fade_.grow(size_t(pc.hp)), st_plan_.fade.data(), size_t(pc.hp) * 4, hipMemcpyHostToDevice));
            }
            const PitchRatio pr = pitch_ratio(pc.hp, pc.ho, hL, hM);
            out_plan_ = make_resample_plan(int(pr.in_units), int(pr.out_units));
            Q3_CHECK(out_plan_.L == pr.L && out_plan_.M == pr.M && out_plan_.K == pr.K, 7, "internal error: pitch ratio and resampling plan disagree");
            up_ = int(int64_t(hops) * pc.ho * hL / hM);
            // phase 0 recurs at every frame and q stays inside it; the FIR's look-back lies inside the margins the streams and
            // decode_chunked (one frame of the stretched signal) carry
            Q3_CHECK(int64_t(up_) * out_plan_.M == int64_t(mid_) * out_plan_.L, 7, "internal error: a pitched frame is not whole samples");
            Q3_CHECK(out_plan_.taps() - 1 <= hist_frames() * mid_ && out_plan_.taps() - 1 <= mid_, 7,
                     "internal error: resampler history beyond the stream's margin");
            Q3_CHECK(resample_ratio_lds_bytes(out_plan_.L, out_plan_.M, out_plan_.K) <= 64 * 1024, 7, "internal error: resampler span beyond its LDS budget");
            resample_ = true;
            pitch_delay_ = q3::pitch_delay_out_samples(pc.hp, pr);
            const std::vector<float> tab = resample_table_output_order(out_plan_);
            Q3_HIP(hipMemcpy(out_tab_.grow(tab.size()), tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
            if (keep_formants) {
                Q3_CHECK(!other_rate, 3, "Invalid input: keep_formants needs output_sample_rate 0 or 24000 (the synthesis filter runs at 24 kHz spacing)");
                // the analysis reads Hp + P samples in front of a frame's first one: inside the mid tensor's margin
                Q3_CHECK(pc.hp + kFormantOrder <= hist_frames() * mid_ && up_ % hops == 0, 7, "internal error: formant history beyond the stream's margin");
                const FormantPlan fp = make_formant_plan(pc.hp);
                std::vector<float> t(fp.win);
                t.insert(t.end(), fp.lag, fp.lag + kFormantOrder + 1);
                Q3_HIP(hipMemcpy(fm_win_.grow(t.size()), t.data(), t.size() * 4, hipMemcpyHostToDevice));
                formant_ = true;
            }
        }
    }
    if (!pitched_ && speed != 0.0f && speed != 1.0f) {
        Q3_CHECK(speed >= 0.5f && speed <= 2.0f, 3, "Invalid input: speed must be 0 (off) or between 0.5 and 2.0");
        Q3_CHECK(native_ % kStretchHa == 0, 3, "Invalid input: the codec's frame is not a whole number of 480-sample hops: no speed other than 1");
        const int hops = native_ / kStretchHa;
        int L = 1, M = 1;
        if (output_rate != 0 && output_rate != kResampleNative && resample_rate_supported(output_rate)) {
            const int g = resample_detail::gcd(kResampleNative, output_rate);
            L = output_rate / g;
            M = kResampleNative / g;
        }
        const int hs = stretch_choose_hs(double(speed), hops, L, M);
        Q3_CHECK(hs != 0, 3, "Invalid input: no synthesis hop for this speed and output_sample_rate");
        if (hs != kStretchHa) {
            st_plan_ = make_stretch_plan(hs);
            // the stage reads this far in front of a frame's first sample: inside the margin every streamed tail tensor carries
            Q3_CHECK(stretch_lookback(hs) <= hist_frames() * native_, 7, "internal error: time stretch history beyond the stream's margin");
            mid_ = up_ = hops * hs;
            stretch_ = true;
            ho_ = hs;
            Q3_HIP(hipMemcpy(st_fade_.grow(size_t(hs)), st_plan_.fade.data(), size_t(hs) * 4, hipMemcpyHostToDevice));
        }
    }
    if (!pitched_ && other_rate) {
        Q3_CHECK(resample_rate_supported(output_rate), 3,
                 "Invalid input: output_sample_rate must be 0, 8000, 12000, 16000, 22050, 24000, 32000, 44100 or 48000");
        out_plan_ = make_resample_plan(kResampleNative, output_rate);
        // (with a time stretch in front, mid_ is its frame: stretch_choose_hs took only hops that pass this)
        Q3_CHECK((int64_t(mid_) * out_plan_.L) % out_plan_.M == 0, 3,
                 "Invalid input: the codec's frame does not hold a whole number of samples at output_sample_rate");
        // the stage reads 2K - 1 samples back: they must lie inside the margin every streamed tail tensor carries
        Q3_CHECK(out_plan_.taps() - 1 <= hist_frames() * mid_, 7, "internal error: resampler history beyond the stream's margin");
        up_ = int(int64_t(mid_) * out_plan_.L / out_plan_.M);
        resample_ = true;
        out_rate_ = output_rate;
        const size_t n = align_up(out_plan_.tab.size(), 4);
        std::vector<float> padded(n, 0.0f);
        std::copy(out_plan_.tab.begin(), out_plan_.tab.end(), padded.begin());
        Q3_HIP(hipMemcpy(out_tab_.grow(n), padded.data(), n * 4, hipMemcpyHostToDevice));
    }
    if (native_ % kStretchHa == 0) rs_plan_.hops_per_frame = native_ / kStretchHa;
    rs_plan_.L = hL;
    rs_plan_.M = hM;
    rs_plan_.handle_hs = stretch_hs();
    if (request_speeds) {
        Q3_CHECK(native_ % kStretchHa == 0, 3, "Invalid input: the codec's frame is not a whole number of 480-sample hops: no request speeds");
        const std::vector<float> all = make_fade_all();
        Q3_HIP(hipMemcpy(fade_all_.grow(all.size()), all.data(), all.size() * 4, hipMemcpyHostToDevice));
        rs_ = true;
    }
    Q3_CHECK(m.cfg.codec.head_dim == 64, 6, "codec transformer head_dim must be 64");
    const char* e = std::getenv("Q3TTS_CODEC_FP32");  // tests switch per model load without touching the load options
    fp32_mfma_ = fp32_convs || (e && e[0] == '1');
    Q3_HIP(hipMemset(nf_dev_.grow(kMaxRows), 0, size_t(kMaxRows) * 4));
    const char* nf = std::getenv("Q3TTS_CODEC_NO_FUSE");
    no_fuse_ = nf && nf[0] == '1';
    const char* nh = std::getenv("Q3TTS_CODEC_NO_F16");  // float16 checkpoints through the up-cast two-plane path (comparisons)
    no_h1_ = nh && nh[0] == '1';
}

// floats per frame of the widest tensor in front of the tail (RVQ, pre_conv, pre-transformer and its latent result)
size_t CodecRunner::front_floats_per_frame() const {
    const CodecDecoderConfig& dc = m_.cfg.codec;
    size_t pf = std::max<size_t>(size_t(2) * m_.codec.inner, size_t(dc.codebook_dim));
    pf = std::max(pf, size_t(3) * dc.num_attention_heads * 64);
    pf = std::max(pf, size_t(2) * dc.intermediate_size);
    return std::max(pf, size_t(dc.latent_dim));
}

// floats per frame of the largest intermediate tensor
size_t CodecRunner::floats_per_frame() const {
    const CodecDecoderConfig& dc = m_.cfg.codec;
    size_t per_frame = front_floats_per_frame();
    int ppf = 1;
    for (int r : dc.upsampling_ratios) {
        ppf *= r;
        per_frame = std::max(per_frame, size_t(ppf) * 4 * dc.latent_dim);
    }
    per_frame = std::max(per_frame, size_t(ppf) * dc.decoder_dim);
    int C = dc.decoder_dim;
    for (int r : dc.upsample_rates) {
        ppf *= r;
        C /= 2;
        per_frame = std::max(per_frame, size_t(ppf) * C);
    }
    if (stretch_) per_frame = std::max(per_frame, size_t(mid_));  // the stretched signal in front of the resampler
    if (rs_) per_frame = std::max(per_frame, size_t(rs_plan_.max_mid_spf()));  // ... of the slowest row
    return per_frame;
}

// Frames of left context after which the causal tail of the decoder (everything behind the pre-transformer:
// SpeechTokenizer.swift:767-781) no longer sees where its input began: every CausalConv1d looks (K - 1) * dilation
// positions back at its own rate (:298-301), a CausalTransposeConv1d with K = 2 * stride one input position (:346-351).
int CodecRunner::tail_context_frames() const {
    const CodecDecoderConfig& dc = m_.cfg.codec;
    double ctx = 0.0, rate = 1.0;
    for (int r : dc.upsampling_ratios) {
        rate *= r;          // K == stride: no overlap between input positions
        ctx += 6.0 / rate;  // ConvNeXt depthwise k7 (:372-377)
    }
    ctx += 6.0 / rate;      // initConv k7
    for (int r : dc.upsample_rates) {
        ctx += 1.0 / rate;  // transposed conv k = 2r, stride r: one earlier input position
        rate *= r;
        ctx += 6.0 * (1 + 3 + 9) / rate;  // three residual units, k7 with dilation 1, 3, 9
    }
    ctx += 6.0 / rate;      // outConv k7
    // the time stretch reads its look-back from the recomputed context (its state word and the resampler's input behind it
    // are carried instead, decode_chunked)
    if (stretch_) ctx += double(stretch_lookback(st_plan_.hs)) / rate;
    if (resample_) ctx += double(out_plan_.taps() - 1) / rate;  // the causal polyphase FIR behind it: 2K - 1 samples back
    return int(ctx) + 2;
}

void CodecRunner::upload_lens(const int32_t* lens, int n) {
    if (size_t(n) > lens_dev_.capacity()) Q3_HIP(hipStreamSynchronize(st_));  // the pair about to be freed may still be read
    lens_dev_.grow(size_t(n));
    lens_host_.grow(size_t(n));
    // the pinned staging copy may still feed the previous call's transfer
    Q3_HIP(hipStreamSynchronize(st_));
    std::memcpy(lens_host_, lens, size_t(n) * 4);
    Q3_HIP(hipMemcpyAsync(lens_dev_, lens_host_, size_t(n) * 4, hipMemcpyHostToDevice, st_));
}

// `post`: also (or, with out == nullptr, only) write SnakeBeta_post(result) to out2 for the next conv
void CodecRunner::conv(const Pass& ps, const ConvW& cw, const float* x, int Tmax, int ppf, float* out, const SnakeW* sn,
                       const float* res, int act, const SnakeW* post, float* out2) {
    launch([&] {
        ConvGemmArgs a{};
        // streamed decode: Tmax counts the allocation's rows (history margin + chunk); row 0 of the chunk sits behind the margin
        const int64_t m_in = int64_t(ps.hist_frames) * ppf * cw.Cin, m_out = int64_t(ps.hist_frames) * ppf * cw.N;
        a.hist = ps.hist_frames * ppf;
        a.x = x + m_in; a.ldx = cw.Cin; a.x_bstride = int64_t(Tmax) * cw.Cin;
        a.w = cw.w; a.bias = cw.bias; a.scale = cw.scale;
        if (!fp32_mfma_) { a.wh = cw.wh; a.wsc = cw.wsc; }
        a.res = res ? res + m_out : nullptr; a.ldr = cw.N; a.res_bstride = int64_t(Tmax) * cw.N;
        a.out = out ? out + m_out : nullptr; a.ldo = cw.N; a.out_bstride = int64_t(Tmax) * cw.N;
        a.snake_ea = sn ? sn->ea : nullptr; a.snake_ib = sn ? sn->ib : nullptr;
        if (post) { a.out2 = out2 + m_out; a.post_ea = post->ea; a.post_ib = post->ib; a.post_C = post->C; }
        a.frames = ps.fr; a.ppf = ppf; a.Tmax = Tmax; a.B = ps.nb;
        a.Cin = cw.Cin; a.N = cw.N; a.K = cw.K; a.dil = cw.dil; a.act = act;
        launch_conv_gemm(a, st_);
    });
}

void CodecRunner::capture(const Pass& ps, const char* name, const float* t, int T, int C) {
    if (!ps.stage_out || *ps.stage != name) return;
    Q3_HIP(hipStreamSynchronize(st_));
    ps.stage_out->resize(size_t(ps.nb) * T * C);
    Q3_HIP(hipMemcpy(ps.stage_out->data(), t, ps.stage_out->size() * 4, hipMemcpyDeviceToHost));
    if (ps.stage_T) *ps.stage_T = T;
    if (ps.stage_C) *ps.stage_C = C;
}

// Steps 1-4 (SpeechTokenizer.swift:757-765): split-RVQ dequantisation, pre_conv, pre_transformer over ALL frames of a row
// (its attention has neither mask nor positions, :512-528). Result: bufs[0] = [nb][Fmax][latent].
void CodecRunner::run_front(const Pass& ps, const int32_t* codes, int code_stride_frames, int Fmax, float* const* bufs,
                            const int32_t* first_frame) {
    const CodecDecoderConfig& dc = m_.cfg.codec;
    const CodecW& w = m_.codec;
    const int nb = ps.nb;
    const int32_t* fr = ps.fr;
    int T = Fmax, ppf = 1;
    // 1-2. Split-RVQ dequantisation (SpeechTokenizer.swift:214-226)
    launch_rvq_gather(codes, code_stride_frames, w.cb_first, w.cb_rest_dev, int(w.cb_rest.size()), w.inner, fr, Fmax, nb,
                      bufs[0], w.cb_first_rows, w.cb_rest_rows, st_, first_frame);
    conv(ps, w.rvq_out, bufs[0], T, ppf, bufs[1], nullptr, nullptr, 0);
    capture(ps, "quantizer", bufs[1], T, w.rvq_out.N);
    // 3. pre_conv (:759)
    conv(ps, w.pre_conv, bufs[1], T, ppf, bufs[0], nullptr, nullptr, 0);
    capture(ps, "pre_conv", bufs[0], T, w.pre_conv.N);
    // 4. pre_transformer (:629-643)
    {
        const int hid = dc.hidden_size, heads = dc.num_attention_heads, I = dc.intermediate_size;
        float *x = bufs[1], *t1 = bufs[2], *t2 = bufs[3];
        conv(ps, w.t_in, bufs[0], T, ppf, x, nullptr, nullptr, 0);
        for (auto& L : w.tlayers) {
            launch_rmsnorm_f32(x, L.ln1, dc.rms_norm_eps, hid, fr, ppf, T, nb, t1, st_);
            conv(ps, L.qkv, t1, T, ppf, t2, nullptr, nullptr, 0);
            launch_attn_full_f32(t2, heads, fr, T, nb, t1, st_);
            conv(ps, L.o, t1, T, ppf, x, nullptr, x, 0);  // x = x + layer_scale * o_proj(attn)  (:589-592)
            launch_rmsnorm_f32(x, L.ln2, dc.rms_norm_eps, hid, fr, ppf, T, nb, t1, st_);
            conv(ps, L.gateup, t1, T, ppf, t2, nullptr, nullptr, 0);
            launch_silu_mul_f32(t2, I, fr, ppf, T, nb, t1, st_);
            conv(ps, L.down, t1, T, ppf, x, nullptr, x, 0);  // (:594-598)
        }
        launch_rmsnorm_f32(x, w.t_norm, dc.rms_norm_eps, hid, fr, ppf, T, nb, t1, st_);
        conv(ps, w.t_out, t1, T, ppf, bufs[0], nullptr, nullptr, 0);
    }
    capture(ps, "pre_transformer", bufs[0], T, w.t_out.N);
}

// ---- float16 speech tokenizers ("lite" checkpoints, docs/paper.tex:207): the MainDecoder as the reference computes it ----
void CodecRunner::conv_h1(const Pass& ps, const ConvW& cw, const void* x, bool x_f32, int Tmax, int ppf, uint16_t* out, const uint16_t* res,
                          const SnakeW* post, uint16_t* out2) {
    launch([&] {
        Q3_CHECK(cw.w1 != nullptr, 7, "internal error: float16 decoder without its one-plane weights");
        ConvH1Args a{};
        // streamed decode (as conv()): Tmax counts the allocation's rows, row 0 of the chunk sits behind the history margin
        const int64_t m_in = int64_t(ps.hist_frames) * ppf * cw.Cin, m_out = int64_t(ps.hist_frames) * ppf * cw.N;
        a.hist = ps.hist_frames * ppf;
        a.x = x_f32 ? static_cast<const void*>(static_cast<const float*>(x) + m_in) : static_cast<const void*>(static_cast<const uint16_t*>(x) + m_in);
        a.x_f32 = x_f32 ? 1 : 0; a.ldx = cw.Cin; a.x_bstride = int64_t(Tmax) * cw.Cin;
        a.w1 = cw.w1; a.bias = cw.bias;
        a.res = res ? res + m_out : nullptr; a.ldr = cw.N; a.res_bstride = int64_t(Tmax) * cw.N;
        a.out = out ? out + m_out : nullptr; a.ldo = cw.N; a.out_bstride = int64_t(Tmax) * cw.N;
        if (post) { a.out2 = out2 + m_out; a.post_ea = post->ea16; a.post_ib = post->ib16; a.post_C = post->C; }
        a.frames = ps.fr; a.ppf = ppf; a.Tmax = Tmax; a.B = ps.nb;
        a.Cin = cw.Cin; a.N = cw.N; a.K = cw.K; a.dil = cw.dil;
        launch_conv_gemm_h1(a, st_);
    });
}

void CodecRunner::capture(const Pass& ps, const char* name, const uint16_t* t, int T, int C) {
    if (!ps.stage_out || *ps.stage != name) return;
    Q3_HIP(hipStreamSynchronize(st_));
    std::vector<uint16_t> h(size_t(ps.nb) * T * C);
    Q3_HIP(hipMemcpy(h.data(), t, h.size() * 2, hipMemcpyDeviceToHost));
    ps.stage_out->resize(h.size());
    for (size_t i = 0; i < h.size(); ++i) {
        _Float16 v;
        std::memcpy(&v, &h[i], 2);
        (*ps.stage_out)[i] = float(v);
    }
    if (ps.stage_T) *ps.stage_T = T;
    if (ps.stage_C) *ps.stage_C = C;
}

// Narrow blocks: each DecoderResidualUnit is one launch (codec_conv.hip resunit_h2_kernel, codec_conv_h1.hip resunit_h1_kernel).
bool CodecRunner::fused_block(const CodecW::Block& Bk, float) const {
    bool fused = !fp32_mfma_ && !no_fuse_ && resunit_supported(Bk.Cout, Bk.res[0].conv1.K, 9);
    for (const auto& R : Bk.res)
        fused = fused && R.conv1.wh && R.conv2.whp && R.conv1.N == Bk.Cout && R.conv2.K == 1 && resunit_supported(Bk.Cout, R.conv1.K, R.conv1.dil);
    return fused;
}
bool CodecRunner::fused_block(const CodecW::Block& Bk, uint16_t) const {
    bool fused = !no_fuse_ && resunit_h1_supported(Bk.Cout, Bk.res[0].conv1.K, 9);
    for (const auto& R : Bk.res)
        fused = fused && R.conv1.w1 && R.conv2.w1p && R.conv1.N == Bk.Cout && R.conv2.K == 1 && resunit_h1_supported(Bk.Cout, R.conv1.K, R.conv1.dil);
    return fused;
}

void CodecRunner::resunit(const Pass& ps, const CodecW::Res& R, int C, int Tmax, int ppf, const float* y, float* out, float* out2,
                          const SnakeW* after) {
    launch([&] {
        const size_t m = size_t(ps.hist_frames) * ppf * C;
        ResUnitArgs r{};
        r.y = y + m; r.out = out + m;
        if (out2) { r.out2 = out2 + m; r.post_ea = after->ea; r.post_ib = after->ib; }
        r.b1 = R.conv1.bias; r.b2 = R.conv2.bias;
        r.w1h = R.conv1.wh; r.w2ph = R.conv2.whp; r.wsc1 = R.conv1.wsc; r.wsc2 = R.conv2.wsc;
        r.ea1 = R.act1.ea; r.ib1 = R.act1.ib; r.ea2 = R.act2.ea; r.ib2 = R.act2.ib;
        r.frames = ps.fr; r.ppf = ppf; r.Tmax = Tmax; r.B = ps.nb; r.C = C; r.K = R.conv1.K; r.dil = R.conv1.dil;
        r.hist = ps.hist_frames * ppf;
        launch_resunit(r, st_);
    });
}
void CodecRunner::resunit(const Pass& ps, const CodecW::Res& R, int C, int Tmax, int ppf, const uint16_t* y, uint16_t* out, uint16_t* out2,
                          const SnakeW* after) {
    launch([&] {
        const size_t m = size_t(ps.hist_frames) * ppf * C;
        ResUnitH1Args r{};
        r.y = y + m; r.out = out + m;
        if (out2) { r.out2 = out2 + m; r.post_ea = after->ea16; r.post_ib = after->ib16; }
        r.b1 = R.conv1.bias; r.b2 = R.conv2.bias;
        r.w1 = R.conv1.w1; r.w2p = R.conv2.w1p;
        r.ea1 = R.act1.ea16; r.ib1 = R.act1.ib16; r.ea2 = R.act2.ea16; r.ib2 = R.act2.ib16;
        r.frames = ps.fr; r.ppf = ppf; r.Tmax = Tmax; r.B = ps.nb; r.C = C; r.dil = R.conv1.dil;
        r.hist = ps.hist_frames * ppf;
        launch_resunit_h1(r, st_);
    });
}

// ---- where the tail's tensors live: get(bytes per frame, does a later causal conv read back into it?) and put() when done ----
// One-shot and chunked decode: the four scratch buffers, a released one is handed out again. The tail never holds more than
// four tensors at once (decode's and decode_chunked's scratch arithmetic counts on four); its input sits in slot[0].
struct CodecRunner::Ring {
    void* slot[4];
    size_t slot_bytes, frames;  // bytes per slot; rows x frames of one pass
    bool taken[4] = {true, false, false, false};
    Ring(float* const* bufs, size_t bytes, size_t rows_x_frames) : slot{bufs[0], bufs[1], bufs[2], bufs[3]}, slot_bytes(bytes), frames(rows_x_frames) {}
    void* get(size_t frame_bytes, bool) {
        Q3_CHECK(frames * frame_bytes <= slot_bytes, 7, "internal error: codec tail tensor wider than its scratch buffer");
        const int i = int(std::find(taken, taken + 4, false) - taken);
        Q3_CHECK(i < 4, 7, "internal error: codec tail holds more than four tensors");
        taken[i] = true;
        return slot[i];
    }
    void put(const void* p) {
        const int i = int(std::find(slot, slot + 4, p) - slot);
        Q3_CHECK(i < 4 && taken[i], 7, "internal error: codec tail released a tensor it does not hold");
        taken[i] = false;
    }
};

// Streamed decode: every tensor in its own persistent piece of the arena, Tal = hist + chunk frames per row, whose first `hist`
// frames are the previous chunk's last ones (rolled in by stream_push), so a conv's causal halo comes from memory instead of
// being zero (first chunk: the margins are zero, i.e. exactly the reference's left padding). Nothing is handed out twice.
uint8_t* CodecRunner::Stream::take(size_t bytes) {
    off = align_up(off, 256);
    uint8_t* p = dry ? nullptr : arena + off;
    off += bytes;
    return p;
}
void* CodecRunner::Stream::get(size_t frame_bytes, bool reads_back) {
    Q3_CHECK(frame_bytes % 4 == 0, 7, "internal error: a streamed tensor's frame is not whole floats");  // roll_history moves floats
    const size_t bytes = size_t(cfg.rows) * Tal * frame_bytes;
    uint8_t* p = take(bytes);
    if (reads_back && !dry) rolls.emplace_back(reinterpret_cast<float*>(p), frame_bytes / 4);
    if (reads_back && dry) roll_offs.emplace_back(off - bytes, frame_bytes / 4);  // the table of a slotted stream
    return p;
}

// Steps 5-7 (SpeechTokenizer.swift:767-781): the causal tail. In: [nb][Trows][latent] with fr[b] valid frames per row behind
// ps.hist_frames frames of history; out: pcm [nb][Trows * upsample] (row stride Trows * upsample). Every tensor is addressed as
// base + hist_frames * elements per frame; the one-shot decode has no margin. With an output rate other than the decoder's
// own, out_conv's 24 kHz signal goes to one more tail tensor and the causal polyphase FIR (resample_plan.h) writes pcm.
// With a speed, the time stretch (stretch_plan.h) sits between the two: 24 kHz in, 4 Hs samples per frame out.
template <class Mem>
void CodecRunner::run_tail(const Pass& ps, Mem& mem, float* in, int Trows, float* pcm) {
    const CodecW& w = m_.codec;
    const int nb = ps.nb, H = ps.hist_frames;
    const int32_t* fr = ps.fr;
    int T = Trows, ppf = 1;  // T: rows of a tensor at the current rate
    auto f32 = [&](size_t per_frame, bool reads_back) { return static_cast<float*>(mem.get(per_frame * sizeof(float), reads_back)); };
    // 5. upsample stages: transposed conv (k = stride) + ConvNeXt (:767-775)
    float* h = in;
    for (size_t i = 0; i < w.ups.size(); ++i) {
        const auto& U = w.ups[i];
        const int C = U.tconv.N / U.stride;
        const size_t ff = size_t(ppf) * U.stride * C;  // floats per frame behind the transposed conv
        float* y = f32(ff, true);                      // dwconv reads six rows back
        float* t1 = f32(ff, false);
        float* t2 = f32(size_t(ppf) * U.stride * U.pw1.N, false);
        conv(ps, U.tconv, h, T, ppf, y, nullptr, nullptr, 0);  // [T][s*C] == [T*s][C]
        mem.put(h);
        T *= U.stride;
        ppf *= U.stride;
        launch([&] {
            launch_dwconv_ln(y + size_t(H) * ff, U.dw_w, U.dw_b, U.ln_w, U.ln_b, 1e-6f, C, fr, ppf, T, nb, t1 + size_t(H) * ff, st_, H * ppf);
        });
        conv(ps, U.pw1, t1, T, ppf, t2, nullptr, nullptr, 1);
        float* yo = f32(ff, i + 1 == w.ups.size());      // the last stage feeds initConv (k7)
        conv(ps, U.pw2, t2, T, ppf, yo, nullptr, y, 0);  // yo = y + gamma * (pwconv2(...) + b)  (:396-400); y stays dwconv's history
        mem.put(y);
        mem.put(t1);
        mem.put(t2);
        h = yo;
        capture(ps, ("upsample" + std::to_string(i)).c_str(), h, T, C);
    }
    // 6. MainDecoder (:681-690), on E = fp32 tensors or, for a float16 speech tokenizer, float16 ones as the reference computes
    // it. Every SnakeBeta sits in front of a conv; it is evaluated in the epilogue of the conv that PRODUCES the tensor (one
    // sinf per element) and the activated copy is what the next conv stages.
    auto main_decoder = [&](auto elem) {
        using E = decltype(elem);
        constexpr bool f16 = std::is_same<E, uint16_t>::value;
        auto ten = [&](size_t per_frame, bool reads_back) { return static_cast<E*>(mem.get(per_frame * sizeof(E), reads_back)); };
        auto cv = [&](const ConvW& cw, const void* x, bool x_f32, E* out, const E* res, const SnakeW* post, E* out2) {
            if constexpr (f16) conv_h1(ps, cw, x, x_f32, T, ppf, out, res, post, out2);
            else conv(ps, cw, static_cast<const float*>(x), T, ppf, out, nullptr, res, 0, post, out2);
        };
        const size_t nblk = w.blocks.size();
        size_t ef = size_t(ppf) * w.init_conv.N;  // elements per frame of the current tensor
        E* y = ten(ef, nblk == 0);                // the residual stream; without blocks it feeds outConv (k7)
        E* ys = nblk ? ten(ef, true) : nullptr;   // SnakeBeta of it = the next transposed conv's input (one row back)
        cv(w.init_conv, h, true, y, nullptr, nblk ? &w.blocks[0].snake : nullptr, ys);
        mem.put(h);
        capture(ps, "init_conv", y, T, w.init_conv.N);
        for (size_t i = 0; i < nblk; ++i) {
            const auto& Bk = w.blocks[i];
            const SnakeW* after = i + 1 < nblk ? &w.blocks[i + 1].snake : nullptr;
            const bool lastb = i + 1 == nblk;  // the last block feeds outConv (k7)
            ef = size_t(ppf) * Bk.stride * Bk.Cout;
            mem.put(y);  // the block reads the activated copy alone
            E* ys_next = nullptr;
            if (fused_block(Bk, E{})) {
                y = ten(ef, true);  // the units' inputs: k7, dilated
                cv(Bk.tconv, ys, false, y, nullptr, nullptr, nullptr);  // snake (already applied by the producer) -> transposed conv
                mem.put(ys);
                T *= Bk.stride;
                ppf *= Bk.stride;
                for (int j = 0; j < 3; ++j) {
                    E* yout = ten(ef, j < 2 || lastb);
                    if (j == 2 && after) ys_next = ten(ef, true);
                    resunit(ps, Bk.res[j], Bk.Cout, T, ppf, y, yout, ys_next, after);
                    mem.put(y);
                    y = yout;
                }
            } else {
                y = ten(ef, lastb);
                E* ya = ten(ef, true);  // act1(y): conv1's input (k7, dilated)
                cv(Bk.tconv, ys, false, y, nullptr, &Bk.res[0].act1, ya);  // snake -> transposed conv (:474-475)
                mem.put(ys);
                T *= Bk.stride;
                ppf *= Bk.stride;
                E* t1 = ten(ef, false);
                for (int j = 0; j < 3; ++j) {  // DecoderResidualUnit (:430-437): y += conv2(act2(conv1(act1(y))))
                    cv(Bk.res[j].conv1, ya, false, nullptr, nullptr, &Bk.res[j].act2, t1);
                    const SnakeW* next = j < 2 ? &Bk.res[j + 1].act1 : after;
                    E* yn = next ? ten(ef, true) : nullptr;  // the next unit's input, or the next block's
                    cv(Bk.res[j].conv2, t1, false, y, y, next, yn);
                    mem.put(ya);
                    ya = yn;
                }
                mem.put(t1);
                ys_next = ya;
            }
            ys = ys_next;
            capture(ps, ("block" + std::to_string(i)).c_str(), y, T, Bk.Cout);
        }
        // 7. outSnake -> outConv -> clip (:687-688, :781)
        // (a resampled decode: out_conv's own clip stays, the flags of a non-finite waveform come from it as before)
        // rows with hops of their own (a one-shot decode with row_hs): the stretch runs from the rows' table and everything
        // behind it has frames of the slowest row's size, a row's samples packed at the start of its part
        const bool own_hops = ps.own_hops;
        const bool stretch = stretch_ || own_hops;
        const int up = own_hops ? rs_plan_.max_spf() : up_, midf = own_hops ? rs_plan_.max_mid_spf() : mid_;
        const bool post = resample_ || stretch;  // stages behind out_conv: its signal goes to one more tail tensor
        float* p24 = post ? static_cast<float*>(mem.get(size_t(ppf) * sizeof(float), true)) : nullptr;
        launch([&] {
            const E* x = y + size_t(H) * ppf * w.out_C;
            float* out = (post ? p24 : pcm) + size_t(H) * ppf;
            if constexpr (f16)
                launch_out_conv_h1(x, w.out_C, w.out_snake.ea16, w.out_snake.ib16, w.out_w, w.out_b, fr, ppf, T, nb, out, st_, nf_dev_ + ps.row0, H * ppf);
            else
                launch_out_conv(x, w.out_C, w.out_snake.ea, w.out_snake.ib, w.out_w, w.out_b, fr, ppf, T, nb, out, st_, H * ppf, nf_dev_ + ps.row0);
        });
        mem.put(y);
        // X: decode_chunked with a time stretch -- recomputed context frames in front of the new ones; the stages below run on
        // the new frames (frn) and find their input's history in the context (0 everywhere else)
        const int X = stretch ? ps.ctx_frames : 0;
        const int32_t* frn = (stretch && ps.fr_new) ? ps.fr_new : fr;
        // the resampler's input: its first new sample, row stride, samples in memory in front of it, samples per frame
        float* rin = p24 ? p24 + size_t(H) * ppf : nullptr;
        int64_t rin_stride = int64_t(T);
        int rin_hist = H * ppf, rin_frame = ppf;
        float* mid = nullptr;
        if (stretch) {
            // 8. the time stretch (stretch_plan.h): output frame f depends on input up to the end of frame f alone, and on one
            // word of state per row. A stream keeps the word in a tensor of its own, one entry per frame: the stage reads the
            // entry of the frame in front of the chunk (the margin's last: zero behind a reset, i.e. hop 0 comes next) and
            // writes one behind every frame, so the margin machinery carries it like samples.
            int32_t* words = H > 0 ? static_cast<int32_t*>(mem.get(size_t(kStateWords) * sizeof(int32_t), true)) : nullptr;
            float* sy = nullptr;
            int64_t sy_stride = 0;
            if (!resample_) {
                sy = pcm ? pcm + size_t(H + X) * up : nullptr;  // (no memory behind the tensors in stream_open's counting pass)
                sy_stride = int64_t(Trows) * up;
            } else if (ps.mid_carry) {
                sy = ps.mid_carry + mid_;
                sy_stride = ps.mid_stride;
                rin_hist = mid_;
            } else {
                mid = static_cast<float*>(mem.get(size_t(midf) * sizeof(float), true));
                sy = mid ? mid + size_t(H) * midf : nullptr;
                sy_stride = int64_t(Trows) * midf;
                rin_hist = H * midf;
            }
            launch([&] {
                StretchArgs a{};
                a.x = p24 + size_t(H + X) * ppf; a.x_bstride = int64_t(T);
                a.y = sy; a.y_bstride = sy_stride;
                a.len = frn; a.len_mul = ppf;
                a.fade = st_fade_; a.hs = st_plan_.hs; a.delay = st_plan_.delay;
                a.hs_rows = ps.hs_rows; a.fade_all = own_hops ? static_cast<const float*>(fade_all_) : nullptr;
                a.hist = (H + X) * ppf; a.causal = 1; a.B = nb;
                if (words) {
                    a.state_in = words + size_t(H - 1) * kStateWords; a.state_in_bstride = int64_t(Trows) * kStateWords;
                    a.state_frames = words + size_t(H) * kStateWords; a.state_frames_bstride = int64_t(Trows) * kStateWords;
                    a.frame_hops = ppf / kStretchHa; a.state_frame_words = kStateWords;
                } else if (ps.carry) {
                    a.state_in = ps.carry; a.state_in_bstride = 1;
                    a.state_out = ps.carry; a.state_out_bstride = 1;
                }
                launch_stretch(a, st_);
            });
            if (words) mem.put(words);
            rin = sy;
            rin_stride = sy_stride;
            rin_frame = midf;
        }
        // 8b. keep_formants (formant_plan.h): analyse + whiten the resampler's input hop by hop; the resampler then reads the
        // whitened signal e (one more tail tensor with a margin: the FIR reads 2K' - 1 samples back) and writes the unclipped
        // e' to a tail tensor instead of the PCM; the synthesis filter behind it writes the PCM. Hop h depends on the mid
        // signal up to the end of hop h alone, and the filter's state, P floats per row, lives in a tensor of its own, one
        // entry per frame, exactly as the stretch's word does.
        const int fhops = ppf / kStretchHa;  // hops per frame
        float *fe = nullptr, *fcoef = nullptr, *fep = nullptr, *fstate = nullptr;
        bool tail_in_held = post;  // p24 (and mid) are still held
        if (formant_) {
            Q3_CHECK(resample_ && !own_hops && !ps.mid_carry && X == 0, 7, "internal error: formant stage on a path that cannot carry it");
            fe = static_cast<float*>(mem.get(size_t(midf) * sizeof(float), true));
            fcoef = static_cast<float*>(mem.get(size_t(fhops) * kFormantOrder * sizeof(float), false));
            launch([&] {
                FormantAnalyseArgs a{};
                a.y = rin; a.y_bstride = rin_stride;
                a.len = frn; a.len_mul = rin_frame; a.hist = rin_hist; a.hp = pitch_hp_;
                a.win = fm_win_; a.lag = fm_win_ + 2 * size_t(pitch_hp_);
                a.coef = fcoef + size_t(H) * fhops * kFormantOrder; a.coef_bstride = int64_t(Trows) * fhops * kFormantOrder;
                a.e = fe + size_t(H) * midf; a.e_bstride = int64_t(Trows) * midf;
                a.B = nb; a.max_len = int64_t(Trows - H) * rin_frame;
                launch_formant_analyse(a, st_);
            });
            // (the Ring holds four tensors at most: the stage's input is done with)
            if (mid) mem.put(mid);
            mid = nullptr;
            mem.put(p24);
            tail_in_held = false;
            fep = static_cast<float*>(mem.get(size_t(up) * sizeof(float), false));
        }
        if (resample_) {
            // Output frame f depends on input up to the end of frame f alone (q = floor(n M / L) stays inside the frame), and
            // the phase of a chunk's first sample is 0: the rows are addressed frame by frame like every other tensor.
            launch([&] {
                ResampleArgs a{};
                a.x = rin; a.x_bstride = rin_stride;
                if (formant_) {
                    a.x = fe + size_t(H) * midf; a.x_bstride = int64_t(Trows) * midf;
                }
                a.y = (formant_ ? fep : pcm) + size_t(H + X) * up; a.y_bstride = int64_t(Trows) * up;
                a.len = frn; a.len_mul = rin_frame; a.max_in = int64_t(Trows - H - X) * rin_frame;
                a.len_mul_rows = ps.mid_rows;
                a.tab = out_tab_; a.L = out_plan_.L; a.M = out_plan_.M; a.K = out_plan_.K;
                a.hist = formant_ ? H * midf : rin_hist; a.centred = 0; a.clamp = formant_ ? 0 : 1; a.B = nb;
                if (pitched_) launch_resample_ratio(a, st_);
                else launch_resample(a, st_);
            });
        }
        if (formant_) {
            mem.put(fe);
            fstate = H > 0 ? static_cast<float*>(mem.get(size_t(kFormantOrder) * sizeof(float), true)) : nullptr;
            launch([&] {
                FormantSynthArgs a{};
                a.ep = fep + size_t(H) * up; a.ep_bstride = int64_t(Trows) * up;
                a.out = pcm + size_t(H) * up; a.out_bstride = int64_t(Trows) * up;
                a.len = frn; a.len_mul = up; a.ho = up / fhops;
                a.coef = fcoef + size_t(H) * fhops * kFormantOrder; a.coef_bstride = int64_t(Trows) * fhops * kFormantOrder;
                a.clamp = 1; a.B = nb; a.max_len = int64_t(Trows - H) * up;
                if (fstate) {
                    a.state_in = fstate + size_t(H - 1) * kFormantOrder; a.state_in_bstride = int64_t(Trows) * kFormantOrder;
                    a.state_frames = fstate + size_t(H) * kFormantOrder; a.state_frames_bstride = int64_t(Trows) * kFormantOrder;
                    a.frame_hops = fhops; a.state_frame_words = kFormantOrder;
                }
                launch_formant_synth(a, st_);
            });
            if (fstate) mem.put(fstate);
            mem.put(fep);
            mem.put(fcoef);
        }
        if (mid) mem.put(mid);
        if (tail_in_held) mem.put(p24);
    };
    if (w.f16_main && !fp32_mfma_ && !no_h1_) main_decoder(uint16_t{});
    else main_decoder(float{});
    Q3_CHECK(ppf == native_, 7, "internal error: codec upsampling mismatch");
}

int CodecRunner::decode(const int32_t* codes_dev, int code_stride_frames, const std::vector<int>& frames, float** pcm_dev,
                        const std::string& stage, std::vector<float>* stage_out, int* stage_T, int* stage_C, int32_t* nonfinite_host,
                        bool force_fp32, const int* row_hs) {
    Q3_CHECK(!row_hs || rs_, 7, "internal error: per-row hops on a handle without request speeds");
    const int up = row_hs ? rs_plan_.max_spf() : up_;  // samples per frame of the PCM's layout
    struct Fp32Scope {  // the override ends with the call, however it ends
        bool& flag;
        bool old;
        ~Fp32Scope() { flag = old; }
    } fp32_scope{fp32_mfma_, fp32_mfma_};
    if (force_fp32) fp32_mfma_ = true;
    const int B = int(frames.size());
    Q3_CHECK(B <= kMaxRows, 3, "Invalid input: too many rows in one codec decode");
    Q3_HIP(hipMemsetAsync(nf_dev_, 0, size_t(B) * 4, st_));
    int Fmax = 0;
    for (int f : frames) Fmax = std::max(Fmax, f);
    Q3_CHECK(Fmax > 0, 3, "Invalid input: no frames to decode");
    const size_t per_frame = floats_per_frame();
    const size_t pcm_floats = size_t(B) * Fmax * up;
    int rows_per_chunk = int(std::max<size_t>(1, kScratchBudget / (4 * per_frame * Fmax * sizeof(float))));
    rows_per_chunk = std::min(rows_per_chunk, B);
    const size_t big = align_up(size_t(rows_per_chunk) * Fmax * per_frame * sizeof(float), 256);
    float* pcm = reinterpret_cast<float*>(buf_.grow(align_up(pcm_floats * sizeof(float), 256) + 4 * big));
    float* bufs[4];
    for (int i = 0; i < 4; ++i) bufs[i] = reinterpret_cast<float*>(buf_ + align_up(pcm_floats * sizeof(float), 256) + size_t(i) * big);
    upload_lens(frames.data(), B);
    if (row_hs) {  // (behind upload_lens' synchronisation: the staging pair is free)
        if (size_t(2 * B) > rowhs_dev_.capacity()) Q3_HIP(hipStreamSynchronize(st_));
        rowhs_dev_.grow(size_t(2 * B));
        rowhs_host_.grow(size_t(2 * B));
        for (int b = 0; b < B; ++b) {
            const int hs = row_hs[b];
            Q3_CHECK(hs >= kStretchHsMin && hs <= kStretchHsMax && rs_plan_.spf(hs) * int64_t(rs_plan_.M) == int64_t(rs_plan_.mid_spf(hs)) * rs_plan_.L,
                     7, "internal error: a row's synthesis hop is not admissible");
            rowhs_host_[b] = hs == kStretchHa ? 0 : hs;
            rowhs_host_[B + b] = rs_plan_.mid_spf(hs);
        }
        Q3_HIP(hipMemcpyAsync(rowhs_dev_, rowhs_host_, size_t(2 * B) * 4, hipMemcpyHostToDevice, st_));
    }
    for (int r0 = 0; r0 < B; r0 += rows_per_chunk) {
        Pass ps{};
        ps.nb = std::min(rows_per_chunk, B - r0);
        ps.row0 = r0;
        ps.fr = lens_dev_ + r0;
        if (row_hs) {
            ps.own_hops = true;
            ps.hs_rows = rowhs_dev_ + r0;
            ps.mid_rows = rowhs_dev_ + B + r0;
        }
        ps.stage = &stage; ps.stage_out = stage_out; ps.stage_T = stage_T; ps.stage_C = stage_C;
        run_front(ps, codes_dev + size_t(r0) * code_stride_frames * 16, code_stride_frames, Fmax, bufs);
        Ring ring(bufs, big, size_t(ps.nb) * Fmax);
        run_tail(ps, ring, bufs[0], Fmax, pcm + size_t(r0) * Fmax * up);
    }
    if (nonfinite_host) Q3_HIP(hipMemcpyAsync(nonfinite_host, nf_dev_, size_t(B) * 4, hipMemcpyDeviceToHost, st_));
    *pcm_dev = pcm;
    return Fmax;
}

// f1: the decode in pieces. The pre-transformer runs once over every frame (it is bidirectional); everything behind it is
// causal, so the tail is evaluated chunk by chunk: chunk [f0, f1) takes the pre-transformer frames [f0 - H, f1) with
// H = tail_context_frames() and keeps the last (f1 - f0) * upsample samples. Every kept sample sees exactly the inputs it
// sees in the one-shot decode, through the same kernels and summation order: the PCM is bit-identical
// (tests/test_streaming.py). Each chunk's samples are copied to pcm_host ([B][Fmax * upsample], pinned) at their final
// place and chunk_done[k] is recorded behind the copy.
int CodecRunner::decode_chunked(const int32_t* codes_dev, int code_stride_frames, const std::vector<int>& frames, int chunk_frames,
                                float* pcm_host, std::vector<hipEvent_t>& chunk_done, int32_t* nonfinite_host, int32_t* nf_chunks_host) {
    const CodecDecoderConfig& dc = m_.cfg.codec;
    const int B = int(frames.size());
    int Fmax = 0;
    for (int f : frames) Fmax = std::max(Fmax, f);
    Q3_CHECK(Fmax > 0 && chunk_frames > 0, 3, "Invalid input: no frames to decode");
    Q3_CHECK(B <= kMaxRows, 3, "Invalid input: too many rows in one codec decode");
    // (the recomputed left context cannot recompute the synthesis filter's state, nor the analysis window in front of a chunk)
    Q3_CHECK(!formant_, 3, "Invalid input: the chunked exact decode is not offered on a handle with keep_formants");
    Q3_HIP(hipMemsetAsync(nf_dev_, 0, size_t(B) * 4, st_));
    const int H = tail_context_frames();
    const int n_chunks = ceil_div(Fmax, chunk_frames);
    const int Tc = std::min(Fmax, chunk_frames + H);  // frames per tail pass, at most
    const size_t per_frame = floats_per_frame();
    const size_t front_bytes = align_up(size_t(B) * Fmax * dc.latent_dim * sizeof(float), 256);
    // front: four buffers of [B][Fmax] x (widest front tensor); tail: four of [B][Tc] x per_frame; x_all keeps the front's result
    // rows per pass: like decode(), a batch whose activations exceed the scratch budget goes through in groups of rows (the
    // codes of a finished AR loop must never be lost to a scratch limit); x_all always holds every row
    const size_t per_row = std::max(size_t(Fmax) * front_floats_per_frame(), size_t(Tc) * per_frame) * sizeof(float);
    const int G = int(std::min<size_t>(size_t(B), std::max<size_t>(1, kScratchBudget / (4 * per_row))));
    const size_t big = align_up(size_t(G) * per_row, 256);
    const size_t pcm_bytes = align_up(size_t(G) * Tc * up_ * sizeof(float), 256);
    float* pcm = reinterpret_cast<float*>(buf_.grow(pcm_bytes + front_bytes + 4 * big));
    float* x_all = reinterpret_cast<float*>(buf_ + pcm_bytes);
    float* bufs[4];
    for (int i = 0; i < 4; ++i) bufs[i] = reinterpret_cast<float*>(buf_ + pcm_bytes + front_bytes + size_t(i) * big);
    // row lengths: the whole rows for the front, then per chunk the frames of [h0, f1) each row still has
    // (a time stretch: then the frames of [f0, f1) alone, for the stages that carry their state instead of recomputing it)
    std::vector<int32_t> lens((size_t)(B) * (1 + (stretch_ ? 2 : 1) * n_chunks));
    for (int b = 0; b < B; ++b) lens[size_t(b)] = frames[size_t(b)];
    for (int k = 0; k < n_chunks; ++k) {
        const int f0 = k * chunk_frames, f1 = std::min(Fmax, f0 + chunk_frames), h0 = std::max(0, f0 - H);
        for (int b = 0; b < B; ++b) lens[size_t(1 + k) * B + b] = std::max(0, std::min(frames[size_t(b)], f1) - h0);
        if (stretch_)
            for (int b = 0; b < B; ++b) lens[size_t(1 + n_chunks + k) * B + b] = std::max(0, std::min(frames[size_t(b)], f1) - f0);
    }
    upload_lens(lens.data(), int(lens.size()));
    // The time stretch cannot recompute its state word from left context: the word is carried from chunk to chunk, reset here
    // for chunk 0, and with it the stretched signal's last frame for the resampler behind it.
    const int64_t mid_stride = int64_t(1 + chunk_frames) * mid_;
    if (stretch_) {
        if (size_t(B) > ch_words_.capacity() || (resample_ && size_t(B) * size_t(mid_stride) > ch_mid_.capacity()))
            Q3_HIP(hipStreamSynchronize(st_));  // the old buffers may still be read
        Q3_HIP(hipMemsetAsync(ch_words_.grow(size_t(B)), 0, size_t(B) * 4, st_));
        if (resample_) Q3_HIP(hipMemsetAsync(ch_mid_.grow(size_t(B) * size_t(mid_stride)), 0, size_t(B) * size_t(mid_stride) * 4, st_));
    }
    while (int(chunk_done.size()) < n_chunks) {
        hipEvent_t e = nullptr;
        Q3_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        chunk_done.push_back(e);
    }
    const std::string none;
    const size_t row_in = size_t(dc.latent_dim) * sizeof(float);
    for (int r0 = 0; r0 < B; r0 += G) {
        Pass ps{};
        ps.nb = std::min(G, B - r0); ps.row0 = r0; ps.fr = lens_dev_ + r0; ps.stage = &none;
        run_front(ps, codes_dev + size_t(r0) * code_stride_frames * 16, code_stride_frames, Fmax, bufs);
        Q3_HIP(hipMemcpyAsync(x_all + size_t(r0) * Fmax * dc.latent_dim, bufs[0], size_t(ps.nb) * Fmax * row_in, hipMemcpyDeviceToDevice, st_));
    }
    for (int k = 0; k < n_chunks; ++k) {
        const int f0 = k * chunk_frames, f1 = std::min(Fmax, f0 + chunk_frames), h0 = std::max(0, f0 - H), T = f1 - h0;
        for (int r0 = 0; r0 < B; r0 += G) {
            Pass ps{};
            ps.nb = std::min(G, B - r0); ps.row0 = r0; ps.fr = lens_dev_ + size_t(1 + k) * B + r0; ps.stage = &none;
            Q3_HIP(hipMemcpy2DAsync(bufs[0], size_t(T) * row_in, x_all + (size_t(r0) * Fmax + h0) * dc.latent_dim, size_t(Fmax) * row_in,
                                    size_t(T) * row_in, size_t(ps.nb), hipMemcpyDeviceToDevice, st_));
            if (stretch_) {
                ps.ctx_frames = f0 - h0;
                ps.fr_new = lens_dev_ + size_t(1 + n_chunks + k) * B + r0;
                ps.carry = ch_words_ + r0;
                if (resample_) {
                    ps.mid_carry = ch_mid_ + size_t(r0) * size_t(mid_stride);
                    ps.mid_stride = mid_stride;
                }
            }
            Ring ring(bufs, big, size_t(ps.nb) * T);
            run_tail(ps, ring, bufs[0], T, pcm);
            if (ps.mid_carry && f1 - f0 == chunk_frames)  // (a short chunk is the last one)
                launch_roll_history(ps.mid_carry + mid_, mid_stride, int64_t(mid_), int64_t(chunk_frames) * mid_, ps.nb, st_);
            Q3_HIP(hipMemcpy2DAsync(pcm_host + (size_t(r0) * Fmax + f0) * up_, size_t(Fmax) * up_ * sizeof(float), pcm + size_t(f0 - h0) * up_,
                                    size_t(T) * up_ * sizeof(float), size_t(f1 - f0) * up_ * sizeof(float), size_t(ps.nb),
                                    hipMemcpyDeviceToHost, st_));
        }
        if (nf_chunks_host) Q3_HIP(hipMemcpyAsync(nf_chunks_host + size_t(k) * B, nf_dev_, size_t(B) * 4, hipMemcpyDeviceToHost, st_));
        Q3_HIP(hipEventRecord(chunk_done[size_t(k)], st_));
    }
    if (nonfinite_host) Q3_HIP(hipMemcpyAsync(nonfinite_host, nf_dev_, size_t(B) * 4, hipMemcpyDeviceToHost, st_));
    return n_chunks;
}

}  // namespace q3

// ---------------------------------------------------------------------------------------------------------------------
// streamed decode (row f1)
// ---------------------------------------------------------------------------------------------------------------------
namespace q3 {

// Frames of history a tail tensor must carry so that every causal conv finds its halo in it: (K - 1) * dilation rows at the
// tensor's rate, rounded up to whole frames (SpeechTokenizer.swift:298-301: left padding only).
int CodecRunner::hist_frames() const {
    const CodecDecoderConfig& dc = m_.cfg.codec;
    int need = 1, ppf = 1;
    for (int r : dc.upsampling_ratios) {
        ppf *= r;
        need = std::max(need, ceil_div(6, ppf));  // ConvNeXt depthwise k7
    }
    need = std::max(need, ceil_div(6, ppf));      // initConv k7
    for (int r : dc.upsample_rates) {
        need = std::max(need, 1);                 // transposed conv: one earlier input row
        ppf *= r;
        need = std::max(need, ceil_div(6 * 9, ppf));  // residual units, k7 with dilation up to 9
    }
    need = std::max(need, ceil_div(6, ppf));      // outConv k7
    return need;
}

void CodecRunner::stream_prefix() {
    Stream& S = stream_;
    S.off = 0;
    S.rolls.clear();
    if (S.dry) S.roll_offs.clear();
    for (auto& f : S.fbufs) f = reinterpret_cast<float*>(S.take(S.fbuf_floats * sizeof(float)));
    const size_t all = size_t(S.cfg.rows) * S.cfg.max_frames * m_.cfg.codec.latent_dim * sizeof(float);
    S.x_all = S.cfg.window < 0 ? reinterpret_cast<float*>(S.take(all)) : nullptr;
    S.lat = static_cast<float*>(S.get(size_t(m_.cfg.codec.latent_dim) * sizeof(float), false));
    S.pcm = static_cast<float*>(S.get(size_t(S.up) * sizeof(float), false));
}

void CodecRunner::stream_open(const StreamCfg& cfg) {
    Stream& S = stream_;
    Q3_CHECK(!S.open, 3, "Invalid input: a streamed decode is already open on this model");
    S.cfg = cfg;
    S.hist = hist_frames();
    Q3_CHECK(cfg.rows >= 1 && cfg.max_frames >= 1 && cfg.lookahead >= 0, 3, "Invalid input: streamed decode geometry");
    Q3_CHECK(cfg.chunk_frames >= S.hist, 3, "Invalid input: audio_chunk_frames of a streamed decode must be at least " + std::to_string(S.hist));
    S.Tal = S.hist + cfg.chunk_frames;
    S.own_hops = cfg.per_row && stream_own_hops();
    S.up = S.own_hops ? rs_plan_.max_spf() : up_;
    S.row_hs.assign(size_t(cfg.rows), stretch_ ? st_plan_.hs : 0);
    if (S.own_hops) Q3_CHECK(stretch_lookback(kStretchHsMax) <= S.hist * native_, 7, "internal error: time stretch history beyond the stream's margin");
    S.next_chunk = 0;
    S.front_done = false;
    S.lens_used = 0;
    const int n_chunks = ceil_div(cfg.max_frames, cfg.chunk_frames);
    // front scratch: the widest front tensor over the longest window
    Q3_CHECK(cfg.max_prefix >= 0 && (cfg.max_prefix == 0 || cfg.per_row), 3, "Invalid input: a reference prefix needs a slotted stream");
    const int Fwin =
        cfg.window < 0 ? cfg.max_frames : std::min(cfg.max_frames + cfg.max_prefix, cfg.window + cfg.chunk_frames + cfg.lookahead);
    S.fbuf_floats = size_t(cfg.rows) * Fwin * front_floats_per_frame();
    // Layout pass (no launches: the walk only counts), then one allocation. Whatever leaves this function -- the arena
    // allocation failing, a check inside run_tail -- the counting mode ends with it: nothing is launched while `dry` is set,
    // and a runner left in that state would turn every later decode of the model into launches of the glue kernels alone
    // (finite garbage, status OK).
    struct DryOff {
        Stream& s;
        ~DryOff() {
            s.dry = false;
            if (!s.open) s.rolls.clear();
        }
    } dry_off{S};
    S.dry = true;
    Pass ps{};
    ps.nb = cfg.rows;
    ps.hist_frames = S.hist;
    ps.own_hops = S.own_hops;
    stream_prefix();
    run_tail(ps, S, S.lat, S.Tal, S.pcm);
    const size_t need = align_up(S.off, 256);
    if (need > S.arena.capacity()) Q3_HIP(hipStreamSynchronize(st_));  // the old arena may still be read
    S.arena.grow(need);
    S.dry = false;
    stream_prefix();
    // history margins start as zeros: the causal left padding of the first chunk
    Q3_HIP(hipMemsetAsync(S.arena, 0, need, st_));
    const size_t slots = size_t(2) * n_chunks + 2;
    S.lens_host.grow(slots * cfg.rows);
    S.lens_dev.grow(slots * cfg.rows);
    Q3_CHECK(cfg.rows <= kMaxRows, 3, "Invalid input: too many rows in one codec decode");
    Q3_HIP(hipMemsetAsync(nf_dev_, 0, size_t(cfg.rows) * 4, st_));
    if (cfg.per_row) {
        Q3_CHECK(cfg.window >= 0, 3, "Invalid input: a slotted stream needs a sliding window (audio_window_frames >= 0)");
        Q3_CHECK(m_.cfg.codec.latent_dim % 4 == 0, 3, "Invalid input: a slotted stream needs a latent width of whole float4s");
        SlotPlanCfg pc;
        pc.rows = cfg.rows; pc.chunk = cfg.chunk_frames; pc.window = cfg.window; pc.lookahead = cfg.lookahead; pc.max_frames = cfg.max_frames;
        S.plan.open(pc);
        // the tensors with history, as one table for roll_history_rows (the counting pass recorded their places in the arena)
        std::vector<RollDesc> table;
        S.roll_max_ff = 0;
        S.state_bytes = 0;
        for (auto& r : S.roll_offs) {
            Q3_CHECK(r.first + size_t(cfg.rows) * S.Tal * r.second * 4 <= need, 7, "internal error: a streamed tensor outside its arena");
            table.push_back(RollDesc{reinterpret_cast<float*>(S.arena + r.first), int64_t(r.second), int64_t(S.state_bytes)});
            S.state_bytes += align_up(size_t(S.hist) * r.second * 4, 16);
            S.roll_max_ff = std::max<int64_t>(S.roll_max_ff, int64_t(r.second));
        }
        S.n_roll = int(table.size());
        if (table.size() * sizeof(RollDesc) > S.roll_desc.capacity()) Q3_HIP(hipStreamSynchronize(st_));
        S.roll_desc.grow(std::max<size_t>(table.size() * sizeof(RollDesc), 16));
        Q3_HIP(hipStreamSynchronize(st_));  // `table` is pageable stack memory: the copy below must not outlive it
        Q3_HIP(hipMemcpy(S.roll_desc, table.data(), table.size() * sizeof(RollDesc), hipMemcpyHostToDevice));
        const size_t R = size_t(cfg.rows);
        const size_t na = S.own_hops ? 6 : 5;  // (a hop per row as the sixth)
        S.ring_pcm.grow(size_t(kRingSlots) * R * cfg.chunk_frames * S.up);
        S.ring_nf.grow(size_t(kRingSlots) * R);
        S.ring_args_host.grow(size_t(kRingSlots) * na * R);
        S.ring_args_dev.grow(size_t(kRingSlots) * na * R);
        while (S.ring_ev.size() < size_t(2) * kRingSlots) {
            hipEvent_t e = nullptr;
            Q3_HIP(hipEventCreate(&e));
            S.ring_ev.push_back(e);
        }
        S.ring_busy.assign(size_t(kRingSlots), 0);
        S.ring_next = 0;
        S.quiet_args_host.grow(size_t(kQuietSlots) * na * R);
        S.quiet_args_dev.grow(size_t(kQuietSlots) * na * R);
        while (S.quiet_ev.size() < size_t(kQuietSlots)) {
            hipEvent_t e = nullptr;
            Q3_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            S.quiet_ev.push_back(e);
        }
        S.quiet_used.assign(size_t(kQuietSlots), 0);
        S.quiet_next = 0;
    }
    S.open = true;
}

void CodecRunner::stream_reset_row(int b, int prefix) {
    Stream& S = stream_;
    Q3_CHECK(S.open && S.cfg.per_row, 3, "Invalid input: no slotted stream is open");
    Q3_CHECK(b >= 0 && b < S.cfg.rows, 3, "Invalid input: row outside the slotted stream");
    Q3_CHECK(prefix >= 0 && prefix <= S.cfg.max_prefix, 3, "Invalid input: reference prefix longer than the stream was opened for");
    S.plan.reset_row(b, prefix);
    launch_roll_history_rows(reinterpret_cast<const RollDesc*>(static_cast<uint8_t*>(S.roll_desc)), S.n_roll, S.roll_max_ff, S.Tal, S.hist,
                             S.cfg.chunk_frames, nullptr, b, S.cfg.rows, nf_dev_, st_);
}

void CodecRunner::stream_set_row_hs(int b, int hs) {
    Stream& S = stream_;
    Q3_CHECK(S.open && S.cfg.per_row && b >= 0 && b < S.cfg.rows, 3, "Invalid input: row outside the slotted stream");
    Q3_CHECK(S.own_hops || hs == stretch_hs(), 7, "internal error: a hop per row in a stream that has one frame size");
    Q3_CHECK(hs >= kStretchHsMin && hs <= kStretchHsMax, 7, "internal error: a row's synthesis hop is not admissible");
    if (S.own_hops) S.row_hs[size_t(b)] = hs == kStretchHa ? 0 : hs;
}

void CodecRunner::stream_save_row(int b, uint8_t* blob_dev) {
    Stream& S = stream_;
    Q3_CHECK(S.open && S.cfg.per_row, 3, "Invalid input: no slotted stream is open");
    Q3_CHECK(b >= 0 && b < S.cfg.rows, 3, "Invalid input: row outside the slotted stream");
    launch_history_state_rows(reinterpret_cast<const RollDesc*>(static_cast<uint8_t*>(S.roll_desc)), S.n_roll, S.roll_max_ff, S.Tal, S.hist, b,
                              S.cfg.rows, blob_dev, false, nullptr, st_);
}

void CodecRunner::stream_row_flag(int b, int32_t* flag_host) {
    Q3_CHECK(stream_.open && b >= 0 && b < stream_.cfg.rows, 3, "Invalid input: row outside the slotted stream");
    Q3_HIP(hipMemcpyAsync(flag_host, nf_dev_ + b, 4, hipMemcpyDeviceToHost, st_));
}

void CodecRunner::stream_load_row(int b, int prefix, const uint8_t* blob_dev) {
    Stream& S = stream_;
    Q3_CHECK(S.open && S.cfg.per_row, 3, "Invalid input: no slotted stream is open");
    Q3_CHECK(b >= 0 && b < S.cfg.rows, 3, "Invalid input: row outside the slotted stream");
    Q3_CHECK(prefix >= 1 && prefix <= S.cfg.max_prefix, 3, "Invalid input: reference prefix longer than the stream was opened for");
    S.plan.reset_row(b, prefix);
    S.plan.skip_prefix(b);
    launch_history_state_rows(reinterpret_cast<const RollDesc*>(static_cast<uint8_t*>(S.roll_desc)), S.n_roll, S.roll_max_ff, S.Tal, S.hist, b,
                              S.cfg.rows, const_cast<uint8_t*>(blob_dev), true, nf_dev_, st_);
}

void CodecRunner::stream_release(int ring) {
    Q3_CHECK(ring >= 0 && ring < kRingSlots && stream_.ring_busy.size() == size_t(kRingSlots), 3, "Invalid input: no such ring slot");
    stream_.ring_busy[size_t(ring)] = 0;
}

bool CodecRunner::stream_push_rows(const int32_t* codes_dev, int code_stride_frames, const int* avail, const uint8_t* final_rows,
                                   std::vector<SlotPass>& out) {
    Stream& S = stream_;
    Q3_CHECK(S.open && S.cfg.per_row, 3, "Invalid input: no slotted stream is open");
    const CodecDecoderConfig& dc = m_.cfg.codec;
    const int B = S.cfg.rows, C = S.cfg.chunk_frames;
    const size_t lat = size_t(dc.latent_dim);
    const int Fwin = std::min(S.cfg.max_frames + S.cfg.max_prefix, S.cfg.window + C + S.cfg.lookahead);  // the front scratch's frames per row (stream_open)
    Q3_CHECK(code_stride_frames >= S.cfg.max_frames, 3, "Invalid input: code rows shorter than the stream's max_frames");
    const std::string none;
    std::vector<RowPlan> rows;
    for (;;) {
        bool any = false;
        for (int b = 0; b < B && !any; ++b) any = S.plan.decodable(b, std::min(avail[b], S.cfg.max_frames), final_rows && final_rows[b]);
        if (!any) return false;
        // a pass in which no row emits (reference prefixes alone) leaves the ring alone
        bool emits = false;
        for (int b = 0; b < B; ++b)
            emits = emits || (!S.plan.in_prefix(b) && S.plan.decodable(b, std::min(avail[b], S.cfg.max_frames), final_rows && final_rows[b]));
        if (emits && S.ring_busy[size_t(S.ring_next)]) return true;  // the oldest pass has not been taken yet
        const int slot = emits ? S.ring_next : S.quiet_next;
        S.plan.plan_pass(avail, final_rows, rows);
        // ---- per-row arguments of this pass; everything that becomes an address is checked here ----
        const size_t na = S.own_hops ? 6 : 5;
        int32_t* h = emits ? S.ring_args_host + size_t(slot) * na * B : S.quiet_args_host + size_t(slot) * na * B;
        int32_t* d = emits ? S.ring_args_dev + size_t(slot) * na * B : S.quiet_args_dev + size_t(slot) * na * B;
        if (!emits && S.quiet_used[size_t(slot)]) Q3_HIP(hipEventSynchronize(S.quiet_ev[size_t(slot)]));  // its last pass has read them
        int Fw = 0, max_take = 0;
        for (int b = 0; b < B; ++b) {
            const RowPlan& r = rows[size_t(b)];
            if (r.part) {
                Q3_CHECK(r.w0 >= 0 && r.wlen >= 1 && r.wlen <= Fwin && r.w0 + r.wlen <= code_stride_frames && r.take >= 1 && r.take <= C &&
                             r.f0 >= r.w0 && r.f0 - r.w0 + r.take <= r.wlen,
                         7, "internal error: a slotted pass outside its buffers");
            }
            h[0 * B + b] = r.part ? r.wlen : 0;
            h[1 * B + b] = r.part ? r.take : 0;
            h[2 * B + b] = r.part ? r.w0 : 0;
            h[3 * B + b] = r.part ? r.f0 - r.w0 : 0;
            h[4 * B + b] = r.part ? 1 : 0;  // roll the participants, leave the others
            if (S.own_hops) h[5 * B + b] = S.row_hs[size_t(b)];
            Fw = std::max(Fw, h[0 * B + b]);
            max_take = std::max(max_take, h[1 * B + b]);
        }
        hipEvent_t begun = nullptr, done = nullptr;
        if (emits) {
            S.ring_busy[size_t(slot)] = 1;
            S.ring_next = (slot + 1) % kRingSlots;
            begun = S.ring_ev[size_t(2) * slot];
            done = S.ring_ev[size_t(2) * slot + 1];
            Q3_HIP(hipEventRecord(begun, st_));
        } else {
            S.quiet_used[size_t(slot)] = 1;
            S.quiet_next = (slot + 1) % kQuietSlots;
        }
        // (the pinned arguments of a ring slot are rewritten only after the caller has waited for the slot's `done`)
        Q3_HIP(hipMemcpyAsync(d, h, na * B * 4, hipMemcpyHostToDevice, st_));
        Pass ps{};
        ps.nb = B;
        ps.stage = &none;
        // ---- pre-transformer over every participant's own window [w0_b, w0_b + wlen_b) ----
        ps.fr = d + 0 * B;
        run_front(ps, codes_dev, code_stride_frames, Fw, S.fbufs, d + 2 * B);
        launch_stream_take_chunk(S.fbufs[0], int64_t(Fw) * int64_t(lat), S.lat + size_t(S.hist) * lat, int64_t(S.Tal) * int64_t(lat), int(lat),
                                 max_take, d + 3 * B, d + 1 * B, B, st_);
        // ---- the causal tail over the chunks, state carried in the participants' margins ----
        ps.fr = d + 1 * B;
        ps.hist_frames = S.hist;
        if (S.own_hops) {
            ps.own_hops = true;
            ps.hs_rows = d + 5 * B;
        }
        stream_prefix();  // the same walk over the arena as in stream_open
        Q3_HIP(hipMemsetAsync(S.pcm, 0, size_t(B) * S.Tal * S.up * 4, st_));
        run_tail(ps, S, S.lat, S.Tal, S.pcm);
        Q3_CHECK(int(S.rolls.size()) == S.n_roll, 7, "internal error: the slotted stream's history table is stale");
        // (a row's take is below C at its last chunk and at the end of a reference prefix, after which more chunks follow)
        launch_roll_history_rows(reinterpret_cast<const RollDesc*>(static_cast<uint8_t*>(S.roll_desc)), S.n_roll, S.roll_max_ff, S.Tal, S.hist, C,
                                 d + 4 * B, -1, B, nullptr, st_, d + 1 * B);
        if (!emits) {
            Q3_HIP(hipEventRecord(S.quiet_ev[size_t(slot)], st_));
            continue;
        }
        const int up = S.up;
        float* pcm_slot = S.ring_pcm + size_t(slot) * B * C * up;
        int32_t* nf_slot = S.ring_nf + size_t(slot) * B;
        Q3_HIP(hipMemcpy2DAsync(pcm_slot, size_t(C) * up * sizeof(float), S.pcm + size_t(S.hist) * up, size_t(S.Tal) * up * sizeof(float),
                                size_t(C) * up * sizeof(float), size_t(B), hipMemcpyDeviceToHost, st_));
        Q3_HIP(hipMemcpyAsync(nf_slot, nf_dev_, size_t(B) * 4, hipMemcpyDeviceToHost, st_));
        Q3_HIP(hipEventRecord(done, st_));
        SlotPass sp;
        sp.ring = slot; sp.begun = begun; sp.done = done; sp.pcm = pcm_slot; sp.nf = nf_slot; sp.rows = rows;
        out.push_back(std::move(sp));
    }
}

void CodecRunner::stream_close(int32_t* nonfinite_host) {
    if (stream_.open && nonfinite_host)
        Q3_HIP(hipMemcpyAsync(nonfinite_host, nf_dev_, size_t(stream_.cfg.rows) * 4, hipMemcpyDeviceToHost, st_));
    stream_.open = false;  // the arena stays for the next stream of the same shape
}

int CodecRunner::stream_push(const int32_t* codes_dev, int code_stride_frames, const int* avail, const uint8_t* final_rows, float* pcm_host,
                             size_t pcm_row_stride, std::vector<hipEvent_t>& chunk_done, int32_t* nf_chunks_host) {
    Stream& S = stream_;
    Q3_CHECK(S.open, 3, "Invalid input: no streamed decode is open");
    const CodecDecoderConfig& dc = m_.cfg.codec;
    const int B = S.cfg.rows, C = S.cfg.chunk_frames, W = S.cfg.window, L = S.cfg.lookahead;
    const size_t lat = size_t(dc.latent_dim);
    auto lens_slot = [&](const std::vector<int32_t>& v) {
        Q3_CHECK((S.lens_used + 1) * B <= S.lens_dev.capacity(), 7, "internal error: streamed decode ran out of length slots");
        int32_t* h = S.lens_host + S.lens_used * B;
        int32_t* d = S.lens_dev + S.lens_used * B;
        std::memcpy(h, v.data(), size_t(B) * 4);
        Q3_HIP(hipMemcpyAsync(d, h, size_t(B) * 4, hipMemcpyHostToDevice, st_));
        ++S.lens_used;
        return d;
    };
    const std::string none;
    for (;;) {
        const int k = S.next_chunk, f0 = k * C, f1 = f0 + C;
        if (f0 >= S.cfg.max_frames) break;
        // decodable: every row either has its frames up to f1 + lookahead or will get no more; at least one row has a frame in it
        bool ready = true, any = false, all_final = true;
        int have = 0;
        for (int b = 0; b < B; ++b) {
            const bool fin = final_rows && final_rows[b];
            all_final = all_final && fin;
            if (!fin && avail[b] < std::min(S.cfg.max_frames, f1 + (W < 0 ? S.cfg.max_frames : L))) ready = false;
            any = any || avail[b] > f0;
            have = std::max(have, avail[b]);
        }
        if (!ready) break;
        if (!any) {
            if (all_final) break;  // nothing left anywhere
            break;
        }
        std::vector<int32_t> v((size_t)(B));
        Pass ps{};
        ps.nb = B;
        ps.stage = &none;
        // ---- pre-transformer over the window (or, window < 0, once over everything) ----
        int w0 = 0;
        if (W < 0) {
            if (!S.front_done) {
                for (int b = 0; b < B; ++b) v[size_t(b)] = avail[b];
                ps.fr = lens_slot(v);
                run_front(ps, codes_dev, code_stride_frames, S.cfg.max_frames, S.fbufs);
                Q3_HIP(hipMemcpyAsync(S.x_all, S.fbufs[0], size_t(B) * S.cfg.max_frames * lat * 4, hipMemcpyDeviceToDevice, st_));
                S.front_done = true;
            }
            Q3_HIP(hipMemcpy2DAsync(S.lat + size_t(S.hist) * lat, size_t(S.Tal) * lat * 4, S.x_all + size_t(f0) * lat,
                                    size_t(S.cfg.max_frames) * lat * 4, size_t(std::min(C, S.cfg.max_frames - f0)) * lat * 4, size_t(B),
                                    hipMemcpyDeviceToDevice, st_));
        } else {
            w0 = std::max(0, f0 - W);
            const int w1 = std::min(have, f1 + L), Fw = w1 - w0;
            for (int b = 0; b < B; ++b) v[size_t(b)] = std::max(0, std::min(avail[b], w1) - w0);
            ps.fr = lens_slot(v);
            run_front(ps, codes_dev + size_t(w0) * 16, code_stride_frames, Fw, S.fbufs);
            Q3_HIP(hipMemcpy2DAsync(S.lat + size_t(S.hist) * lat, size_t(S.Tal) * lat * 4, S.fbufs[0] + size_t(f0 - w0) * lat,
                                    size_t(Fw) * lat * 4, size_t(std::min(C, w1 - f0)) * lat * 4, size_t(B), hipMemcpyDeviceToDevice, st_));
        }
        // ---- the causal tail over the chunk, state carried in the tensors' margins ----
        for (int b = 0; b < B; ++b) v[size_t(b)] = std::max(0, std::min(avail[b], f1) - f0);
        ps.fr = lens_slot(v);
        ps.hist_frames = S.hist;
        stream_prefix();  // the same walk over the arena as in stream_open
        Q3_HIP(hipMemsetAsync(S.pcm, 0, size_t(B) * S.Tal * up_ * 4, st_));
        run_tail(ps, S, S.lat, S.Tal, S.pcm);
        for (auto& r : S.rolls)
            launch_roll_history(r.first + size_t(S.hist) * r.second, int64_t(S.Tal) * int64_t(r.second), int64_t(S.hist) * int64_t(r.second),
                                int64_t(C) * int64_t(r.second), B, st_);
        Q3_HIP(hipMemcpy2DAsync(pcm_host + size_t(f0) * up_, pcm_row_stride * sizeof(float), S.pcm + size_t(S.hist) * up_,
                                size_t(S.Tal) * up_ * sizeof(float), size_t(std::min(C, S.cfg.max_frames - f0)) * up_ * sizeof(float), size_t(B),
                                hipMemcpyDeviceToHost, st_));
        while (int(chunk_done.size()) <= k) {
            hipEvent_t e = nullptr;
            Q3_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            chunk_done.push_back(e);
        }
        if (nf_chunks_host) Q3_HIP(hipMemcpyAsync(nf_chunks_host + size_t(k) * B, nf_dev_, size_t(B) * 4, hipMemcpyDeviceToHost, st_));
        Q3_HIP(hipEventRecord(chunk_done[size_t(k)], st_));
        ++S.next_chunk;
    }
    return S.next_chunk;
}

}  // namespace q3
