// engine_debug.cc -- the block-level hooks (q3tts_debug_*) and the codec entry points that take a caller's codes. See engine.h.
#include "engine_stream.h"

#include "frontend.h"

namespace q3 {

void Engine::debug_frontend_stage(const float* audio, int64_t n_samples, const char* stage, float* out, int64_t cap, int* T, int* C) {
    Q3_CHECK(fe_ != nullptr, 1, "Model not initialized: Speech tokenizer encoder not available");
    Q3_CHECK(audio && n_samples > 0 && stage, 3, "Invalid input: empty audio or stage name");
    const float* a = upload_audio(audio, n_samples);
    StageCapture cap_s;
    cap_s.name = stage;
    static const char* kSpeaker[] = {"mel", "h0", "h1", "h2", "h3", "mfa", "pooled"};
    bool is_spk = false;
    for (const char* s : kSpeaker) is_spk = is_spk || cap_s.name == s;
    if (is_spk) {
        Q3_CHECK(m_->has_speaker_encoder, 1, "Model not initialized: Speaker encoder not available for this model");
        spk_f32_.grow(size_t(m_->cfg.talker.hidden_size));
        fe_->speaker_embedding(a, n_samples, spk_f32_, &cap_s);
    } else {
        Q3_CHECK(m_->has_codec_encoder, 1, "Model not initialized: Speech tokenizer encoder not available");
        const int Tq = fe_->encoded_frames(n_samples);
        ref_codes_dev_.grow(size_t(16) * Tq);
        fe_->encode(a, n_samples, ref_codes_dev_, &cap_s);
    }
    Q3_HIP(hipStreamSynchronize(st_));
    Q3_CHECK(!cap_s.data.empty(), 3, std::string("Invalid input: unknown front-end stage '") + stage + "'");
    Q3_CHECK(int64_t(cap_s.data.size()) <= cap, 3, "Invalid input: output buffer too small");
    std::memcpy(out, cap_s.data.data(), cap_s.data.size() * 4);
    *T = cap_s.T;
    *C = cap_s.C;
}

void Engine::debug_prepare_inputs(const q3tts_request& req, uint16_t* input_embeds, int cap_prompt, int* n_prompt,
                                  uint16_t* trailing, int cap_trailing, int* n_trailing, uint16_t* tts_pad) {
    q3tts_sampling sp{};
    q3tts_default_sampling(&sp);
    std::vector<ResolvedRequest> rr{resolve(req, sp)};
    if (rr[0].clone) prepare_clone_rows(rr);
    std::vector<int> np, nt;
    assemble_prompts(rr, np, nt);
    const int H = m_->cfg.talker.hidden_size;
    Q3_CHECK(np[0] <= cap_prompt && nt[0] <= cap_trailing, 3, "Invalid input: output buffers too small");
    Q3_HIP(hipStreamSynchronize(st_));
    Q3_HIP(hipMemcpy(input_embeds, prompt_, size_t(np[0]) * H * 2, hipMemcpyDeviceToHost));
    Q3_HIP(hipMemcpy(trailing, trailing_, size_t(nt[0]) * H * 2, hipMemcpyDeviceToHost));
    Q3_HIP(hipMemcpy(tts_pad, tts_pad_, size_t(H) * 2, hipMemcpyDeviceToHost));
    *n_prompt = np[0];
    *n_trailing = nt[0];
}

void Engine::debug_sample(const uint16_t* logits, int rows, int V, const q3tts_sampling& sp, const uint8_t* seen,
                          int suppress_lo, int suppress_hi, int eos_id, uint32_t row0, uint32_t draw, int32_t* tokens) {
    Q3_CHECK(rows >= 1 && rows <= Bm_ && V <= m_->cfg.talker.vocab_size, 3, "debug_sample: rows/V out of range");
    Q3_CHECK(draw % 16 == 0, 3, "debug_sample: draw must be a multiple of 16 (frame * 16)");
    const int Vt = m_->cfg.talker.vocab_size;
    Q3_HIP(hipMemcpy2D(tk_.logits, size_t(Vt) * 2, logits, size_t(V) * 2, size_t(V) * 2, size_t(rows), hipMemcpyHostToDevice));
    if (seen) Q3_HIP(hipMemcpy(seen_, seen, size_t(rows) * V, hipMemcpyHostToDevice));
    std::vector<int32_t> fr((size_t)(rows), int32_t(draw / 16)), big((size_t)(rows), 1 << 30);
    Q3_HIP(hipMemcpy(n_frames_, fr.data(), size_t(rows) * 4, hipMemcpyHostToDevice));
    Q3_HIP(hipMemcpy(max_frames_, big.data(), size_t(rows) * 4, hipMemcpyHostToDevice));
    Q3_HIP(hipMemset(finished_, 0, size_t(rows)));
    Q3_HIP(hipMemset(active_, 1, size_t(rows)));
    std::vector<SamplingParams> sph;
    for (int r = 0; r < rows; ++r) sph.push_back(fold_sampling(sp, r, row0));
    Q3_HIP(hipMemcpy(sp_dev_, sph.data(), sph.size() * sizeof(SamplingParams), hipMemcpyHostToDevice));
    SamplerArgs sa{};
    sa.logits = tk_.logits; sa.ldl = Vt; sa.V = V; sa.sp = sp_dev_;
    sa.is_talker = (eos_id >= 0 || suppress_hi > suppress_lo || seen) ? 1 : 0;
    sa.suppress_lo = suppress_lo; sa.suppress_hi = suppress_hi; sa.eos_id = eos_id;
    sa.seen = seen ? seen_ : nullptr; sa.cb = 0; sa.n_frames = n_frames_; sa.max_frames = max_frames_;
    sa.finished = finished_; sa.active = active_; sa.kv_len = kv_len_; sa.advance = 0;
    sa.cur_codes = cur_codes_; sa.codes = codes_; sa.Fmax = 0; sa.B = rows; sa.H = m_->cfg.talker.hidden_size;
    launch_sampler(sa, st_);
    Q3_HIP(hipStreamSynchronize(st_));
    std::vector<int32_t> cc((size_t)(rows) * 16);
    Q3_HIP(hipMemcpy(cc.data(), cur_codes_, cc.size() * 4, hipMemcpyDeviceToHost));
    for (int r = 0; r < rows; ++r) tokens[r] = cc[size_t(r) * 16];
    Q3_HIP(hipMemset(seen_, 0, size_t(rows) * V));
}

void Engine::debug_linear(const uint16_t* x, const uint16_t* W, const uint16_t* bias, int M, int K, int N, uint16_t* y) {
    Q3_CHECK(M >= 1 && M <= 1024 && K % 8 == 0 && N >= 1, 3, "debug_linear: unsupported shape");  // > 64 rows: the tall form
    const int Kp = int(align_up(size_t(K), 128)), Np = int(align_up(size_t(N), 16)), Mp = int(align_up(size_t(M), 16));
    uint16_t *dW = nullptr, *dWt = nullptr, *dx = nullptr, *dy = nullptr, *db = nullptr;
    Q3_HIP(hipMalloc(reinterpret_cast<void**>(&dW), size_t(N) * K * 2));
    Q3_HIP(hipMalloc(reinterpret_cast<void**>(&dWt), size_t(Np) * Kp * 2));
    Q3_HIP(hipMalloc(reinterpret_cast<void**>(&dx), size_t(Mp) * Kp * 2));
    Q3_HIP(hipMalloc(reinterpret_cast<void**>(&dy), size_t(Mp) * Np * 2));
    Q3_HIP(hipMalloc(reinterpret_cast<void**>(&db), size_t(Np) * 2));
    Q3_HIP(hipMemset(dWt, 0, size_t(Np) * Kp * 2));
    Q3_HIP(hipMemset(dx, 0, size_t(Mp) * Kp * 2));
    Q3_HIP(hipMemset(db, 0, size_t(Np) * 2));
    Q3_HIP(hipMemcpy(dW, W, size_t(N) * K * 2, hipMemcpyHostToDevice));
    uint16_t* dxl = nullptr;  // row-major staging, converted to the fragment-major operand layout
    Q3_HIP(hipMalloc(reinterpret_cast<void**>(&dxl), size_t(Mp) * Kp * 2));
    Q3_HIP(hipMemset(dxl, 0, size_t(Mp) * Kp * 2));
    Q3_HIP(hipMemcpy2D(dxl, size_t(Kp) * 2, x, size_t(K) * 2, size_t(K) * 2, size_t(M), hipMemcpyHostToDevice));
    launch_tile_rows(dxl, Kp, dx, Mp / 16, Mp, Kp, st_);
    if (bias) Q3_HIP(hipMemcpy(db, bias, size_t(N) * 2, hipMemcpyHostToDevice));
    launch_tile_weights(dW, N, K, dWt, Kp / 128, 0, 1, st_);
    LinearW L;
    L.w = dWt; L.bias = bias ? db : nullptr; L.N = N; L.K = K; L.Np = Np; L.Kp = Kp;
    GemmArgs ga{};
    ga.W = dWt; ga.x = dx; ga.xMB = Mp / 16; ga.M = M; ga.Mpad = Mp; ga.N = Np; ga.K = Kp; ga.epi = 0; ga.y = dy; ga.ldy = Np;
    ga.bias = L.bias; ga.ss_ld = Mp;
    launch_gemm_skinny(ga, st_);
    Q3_HIP(hipStreamSynchronize(st_));
    Q3_HIP(hipMemcpy2D(y, size_t(N) * 2, dy, size_t(Np) * 2, size_t(N) * 2, size_t(M), hipMemcpyDeviceToHost));
    for (void* p : {(void*)dW, (void*)dWt, (void*)dx, (void*)dxl, (void*)dy, (void*)db})
        if (p) (void)hipFree(p);
}

// The end of a frame against the resume of a starved row, on the caller's tables (q3tts.h): row 1 of a two-row step, once through
// frame_end_kernel with its text row there (run A), once with its text open and no row (it starves: run B1) and then through
// text_append_rows_kernel with that row as the appended text (run B2). Nothing of the engine's own state is touched.
void Engine::debug_text_resume(int H, int V, const uint16_t* tables, const int32_t* codes, const uint16_t* text, uint16_t* out_h,
                               float* out_ss, int32_t* out_state) {
    Q3_CHECK(H >= 128 && H <= 4096 && H % 128 == 0 && V >= 1 && V <= 4096, 3, "debug_text_resume: H must be a multiple of 128 up to 4096, V up to 4096");
    Q3_CHECK(tables && codes && text && out_h && out_ss && out_state, 3, "Invalid input: null argument");
    for (int g = 0; g < 16; ++g) Q3_CHECK(codes[g] >= 0 && codes[g] < V, 3, "debug_text_resume: code outside the tables");
    constexpr int B = 2, row = 1, Tmax = 2;
    DevBuf<uint16_t> d_tab, d_trailing, d_pad, d_h, d_hl, d_text;
    DevBuf<const uint16_t*> d_cp;
    DevBuf<int32_t> d_i32;  // cur_codes [2][16] | n_trailing | trailing_idx | n_frames | max_frames | cp_len  ([2] each)
    DevBuf<uint8_t> d_u8;   // finished | active | text_open | starved ([2] each)
    DevBuf<float> d_ss;
    DevBuf<TextAppendDesc> d_desc;
    d_tab.grow(size_t(16) * V * H);
    d_trailing.grow(size_t(B) * Tmax * H);
    d_pad.grow(size_t(H));
    d_h.grow(size_t(16) * H);
    d_hl.grow(size_t(16) * H);
    d_text.grow(size_t(H));
    d_cp.grow(15);
    d_i32.grow(32 + 10);
    d_u8.grow(8);
    d_ss.grow(B);
    d_desc.grow(1);
    Q3_HIP(hipMemcpy(d_tab, tables, size_t(16) * V * H * 2, hipMemcpyHostToDevice));
    Q3_HIP(hipMemcpy(d_text, text, size_t(H) * 2, hipMemcpyHostToDevice));
    Q3_HIP(hipMemset(d_pad, 0, size_t(H) * 2));
    std::vector<const uint16_t*> cp(15);
    for (int g = 1; g < 16; ++g) cp[size_t(g - 1)] = d_tab + size_t(g) * V * H;
    Q3_HIP(hipMemcpy(d_cp, cp.data(), 15 * sizeof(const uint16_t*), hipMemcpyHostToDevice));
    int32_t* cur = d_i32;
    int32_t *n_tr = cur + 32, *t_idx = n_tr + 2, *n_fr = t_idx + 2, *max_fr = n_fr + 2, *cp_len = max_fr + 2;
    uint8_t *fin = d_u8, *act = fin + 2, *topen = act + 2, *starved = topen + 2;
    FrameEndArgs fe{};
    fe.cur_codes = cur; fe.codec_emb = d_tab; fe.cp_emb = d_cp;
    fe.trailing = d_trailing; fe.n_trailing = n_tr; fe.trailing_idx = t_idx; fe.Tmax = Tmax;
    fe.tts_pad = d_pad; fe.h = d_h; fe.hMB = 1; fe.ss_out = d_ss; fe.H = H; fe.B = B; fe.groups = 16;
    fe.n_frames = n_fr; fe.max_frames = max_fr; fe.finished = fin; fe.active = act; fe.cp_len = cp_len;
    fe.text_open = topen; fe.starved = starved;
    auto reset = [&](int n_trailing, int open) {  // row 0: an empty slot; row 1: running, its frame's 16 codes decided
        std::vector<int32_t> hi(42, 0);
        for (int g = 0; g < 16; ++g) hi[size_t(16 + g)] = codes[g];
        hi[32 + row] = n_trailing;
        hi[38] = hi[39] = 100;  // max_frames
        hi[40] = hi[41] = 15;   // cp_len
        const uint8_t hu[8] = {1, 0, 0, 1, 0, uint8_t(open), 0, 0};
        const float hs[2] = {-1.f, -1.f};
        Q3_HIP(hipMemcpy(d_i32, hi.data(), hi.size() * 4, hipMemcpyHostToDevice));
        Q3_HIP(hipMemcpy(d_u8, hu, 8, hipMemcpyHostToDevice));
        Q3_HIP(hipMemcpy(d_ss, hs, 8, hipMemcpyHostToDevice));
        Q3_HIP(hipMemset(d_h, 0xEE, size_t(16) * H * 2));
        Q3_HIP(hipMemset(d_trailing, 0, size_t(B) * Tmax * H * 2));
    };
    auto read = [&](int k) {
        launch_untile_rows(d_h, 1, d_hl, H, 16, H, st_);
        Q3_HIP(hipStreamSynchronize(st_));
        Q3_HIP(hipMemcpy(out_h + size_t(k) * H, d_hl + size_t(row) * H, size_t(H) * 2, hipMemcpyDeviceToHost));
        float hs[2];
        int32_t hi[42];
        uint8_t hu[8];
        Q3_HIP(hipMemcpy(hs, d_ss, 8, hipMemcpyDeviceToHost));
        Q3_HIP(hipMemcpy(hi, d_i32, sizeof(hi), hipMemcpyDeviceToHost));
        Q3_HIP(hipMemcpy(hu, d_u8, 8, hipMemcpyDeviceToHost));
        out_ss[k] = hs[row];
        int32_t* o = out_state + size_t(k) * 8;
        o[0] = hi[36 + row]; o[1] = hi[34 + row]; o[2] = hi[32 + row]; o[3] = hu[row]; o[4] = hu[2 + row]; o[5] = hu[4 + row];
        o[6] = hu[6 + row]; o[7] = hi[40 + row];  // n_frames, trailing_idx, n_trailing, finished, active, text_open, starved, cp_len
    };
    reset(1, 0);  // A: the text row is there
    Q3_HIP(hipMemcpy(d_trailing + size_t(row) * Tmax * H, d_text, size_t(H) * 2, hipMemcpyDeviceToDevice));
    launch_frame_end(fe, st_);
    read(0);
    reset(0, 1);  // B1: it is not, and the text is open
    launch_frame_end(fe, st_);
    read(1);
    TextAppendDesc d{};  // B2: it arrives
    d.slot = row; d.src_row = 0; d.n_new = 1;
    Q3_HIP(hipMemcpy(d_desc, &d, sizeof(d), hipMemcpyHostToDevice));
    TextAppendArgs ta{};
    ta.desc = d_desc; ta.src = d_text; ta.eos_row = d_pad; ta.trailing = d_trailing; ta.n_trailing = n_tr; ta.text_open = topen;
    ta.max_frames = max_fr; ta.slots = B; ta.fe = fe;
    launch_text_append_rows(ta, &d, 1, st_);
    read(2);
}

// One launch_attn_decode on the caller's buffers (q3tts.h). Everything the kernels turn into an address -- cache lengths,
// block-table entries, the padding of a right-aligned chunk -- is checked here against the sizes the caller states.
void Engine::debug_build_decode_codes(const int32_t* refs, const int32_t* ref_T, const int32_t* gen, const int32_t* n_frames, int R,
                                      int gen_stride, int Fdec, bool misalign, int32_t* out) {
    size_t ref_total = 0;
    for (int r = 0; r < R; ++r) {
        Q3_CHECK(ref_T[r] >= 0 && n_frames[r] >= 0 && n_frames[r] <= gen_stride, 3, "Invalid input: frame counts out of range");
        ref_total += size_t(16) * ref_T[r];
    }
    Q3_CHECK(ref_total == 0 || refs, 3, "Invalid input: null argument");
    const size_t off = misalign ? 1 : 0, n_gen = size_t(R) * gen_stride * 16, n_out = size_t(R) * Fdec * 16;
    DevBuf<int32_t> d_ref, d_gen, d_out;
    DevBuf<DecodeRowDesc> d_desc;
    d_ref.grow(std::max<size_t>(ref_total, 1));
    d_gen.grow(n_gen + off);
    d_out.grow(n_out + off);
    d_desc.grow(size_t(R));
    if (ref_total) Q3_HIP(hipMemcpyAsync(d_ref, refs, ref_total * 4, hipMemcpyHostToDevice, st_));
    Q3_HIP(hipMemcpyAsync(d_gen + off, gen, n_gen * 4, hipMemcpyHostToDevice, st_));
    Q3_HIP(hipMemcpyAsync(d_out + off, out, n_out * 4, hipMemcpyHostToDevice, st_));
    std::vector<DecodeRowDesc> desc((size_t)(R));
    size_t at = 0;
    for (int r = 0; r < R; ++r) {
        desc[size_t(r)] = DecodeRowDesc{ref_T[r] > 0 ? d_ref + at : nullptr, d_gen + off + size_t(r) * gen_stride * 16, ref_T[r], n_frames[r], r, 0};
        at += size_t(16) * ref_T[r];
    }
    Q3_HIP(hipMemcpyAsync(d_desc, desc.data(), desc.size() * sizeof(DecodeRowDesc), hipMemcpyHostToDevice, st_));
    launch_build_decode_codes_rows(desc.data(), d_desc, R, d_out + off, R, Fdec, st_);
    Q3_HIP(hipMemcpyAsync(out, d_out + off, n_out * 4, hipMemcpyDeviceToHost, st_));
    Q3_HIP(hipStreamSynchronize(st_));
}

void Engine::debug_attention(const q3tts_attn_debug& d) {
    Q3_CHECK(d.qkv && d.qn_w && d.kn_w && d.rope_cos && d.rope_sin && d.kpool && d.vpool && d.out, 3, "debug_attention: null argument");
    Q3_CHECK(d.n_kv >= 1 && d.n_kv <= 64 && d.n_heads >= d.n_kv && d.n_heads % d.n_kv == 0 && d.n_heads / d.n_kv <= 4, 3,
             "debug_attention: unsupported GQA ratio");
    Q3_CHECK(d.B >= 1 && d.B <= 256, 3, "debug_attention: batch out of range");
    Q3_CHECK(d.chunk >= 0 && d.chunk <= 16, 3, "debug_attention: at most 16 positions per launch");
    Q3_CHECK(d.max_pages >= 1 && d.max_pages <= 64 && d.n_pages >= 1 && d.n_pages <= 4096 && d.n_pos >= 1 && d.n_pos <= 65536, 3,
             "debug_attention: sizes out of range");
    Q3_CHECK(d.fixed_len >= -1, 3, "debug_attention: fixed_len out of range");
    Q3_CHECK(d.fixed_len >= 0 || d.kv_len, 3, "debug_attention: kv_len missing");
    Q3_CHECK(d.identity_pages || d.block_table, 3, "debug_attention: block_table missing");
    Q3_CHECK(!d.identity_pages || d.B <= d.n_pages, 3, "debug_attention: identity_pages needs a page per row");
    const int B = d.B, C = std::max(d.chunk, 1), rows = C * B;
    const int cap = (d.identity_pages ? 1 : d.max_pages) * kPageTokens;
    for (int b = 0; b < B; ++b) {
        const int len0 = d.fixed_len >= 0 ? d.fixed_len : d.kv_len[b];
        int live = 1;  // the one-position kernel addresses the new token's slot and RoPE row whether or not it appends
        if (d.chunk > 1 && d.chunk_n_prompt) {
            const int64_t r0 = int64_t(d.chunk_r_base) + d.chunk_n_prompt[b];
            live = r0 < 0 ? int(std::max<int64_t>(0, C + r0)) : C;
        } else if (d.chunk > 1) {
            live = C;
        }
        Q3_CHECK(len0 >= 0 && len0 <= cap && len0 + live <= cap && len0 + live <= d.n_pos, 3,
                 "debug_attention: cache length beyond the pages or the RoPE tables");
        if (!d.identity_pages)
            for (int pg = 0; pg * kPageTokens < len0 + live; ++pg) {
                const int32_t e = d.block_table[size_t(b) * d.max_pages + pg];
                Q3_CHECK(e >= 0 && e < d.n_pages, 3, "debug_attention: block-table entry outside the pool");
            }
    }
    const int ld = (d.n_heads + 2 * d.n_kv) * kHeadDim, odim = d.n_heads * kHeadDim;
    const int Mp = int(align_up(size_t(rows), 16));
    const size_t pool = size_t(d.n_pages) * d.n_kv * kPageTokens * kHeadDim;
    const size_t tab = size_t(d.n_pos) * kHeadDim;
    DevBuf<uint16_t> qkv, w, rope, kp, vp, ot, ol;
    DevBuf<int32_t> ints;
    DevBuf<uint8_t> act;
    qkv.grow(size_t(rows) * ld);
    w.grow(2 * kHeadDim);
    rope.grow(2 * tab);
    kp.grow(pool);
    vp.grow(pool);
    ot.grow(size_t(Mp) * odim);
    ol.grow(size_t(rows) * odim);
    ints.grow(size_t(B) * (2 + d.max_pages));
    act.grow(size_t(B));
    int32_t *kv_len = ints, *n_prompt = kv_len + B, *bt = n_prompt + B;
    Q3_HIP(hipMemset(ints, 0, size_t(B) * (2 + d.max_pages) * 4));
    Q3_HIP(hipMemcpy(qkv, d.qkv, size_t(rows) * ld * 2, hipMemcpyHostToDevice));
    Q3_HIP(hipMemcpy(w, d.qn_w, kHeadDim * 2, hipMemcpyHostToDevice));
    Q3_HIP(hipMemcpy(w + kHeadDim, d.kn_w, kHeadDim * 2, hipMemcpyHostToDevice));
    Q3_HIP(hipMemcpy(rope, d.rope_cos, tab * 2, hipMemcpyHostToDevice));
    Q3_HIP(hipMemcpy(rope + tab, d.rope_sin, tab * 2, hipMemcpyHostToDevice));
    Q3_HIP(hipMemcpy(kp, d.kpool, pool * 2, hipMemcpyHostToDevice));
    Q3_HIP(hipMemcpy(vp, d.vpool, pool * 2, hipMemcpyHostToDevice));
    if (d.kv_len) Q3_HIP(hipMemcpy(kv_len, d.kv_len, size_t(B) * 4, hipMemcpyHostToDevice));
    if (d.chunk_n_prompt) Q3_HIP(hipMemcpy(n_prompt, d.chunk_n_prompt, size_t(B) * 4, hipMemcpyHostToDevice));
    if (d.block_table) Q3_HIP(hipMemcpy(bt, d.block_table, size_t(B) * d.max_pages * 4, hipMemcpyHostToDevice));
    if (d.active) Q3_HIP(hipMemcpy(act, d.active, size_t(B), hipMemcpyHostToDevice));
    Q3_HIP(hipMemset(ot, 0xff, size_t(Mp) * odim * 2));  // rows the kernel leaves alone come back as 0xFFFF
    AttnArgs at{};
    at.qkv = qkv; at.ld = ld; at.qn_w = w; at.kn_w = w + kHeadDim; at.eps = d.eps;
    at.rope_cos = rope; at.rope_sin = rope + tab;
    at.kpool = kp; at.vpool = vp;
    at.block_table = bt; at.max_pages = d.max_pages; at.kv_len = kv_len; at.active = d.active ? (const uint8_t*)act : nullptr;
    at.out = ot; at.outMB = Mp / 16; at.n_heads = d.n_heads; at.n_kv = d.n_kv; at.B = B;
    at.scale = d.scale;
    at.fixed_len = d.fixed_len; at.identity_pages = d.identity_pages ? 1 : 0;
    at.chunk = d.chunk; at.chunk_n_prompt = d.chunk_n_prompt ? n_prompt : nullptr; at.chunk_r_base = d.chunk_r_base;
    at.nt_kv = d.nt_kv ? 1 : 0;
    launch_attn_decode(at, st_);
    Q3_HIP(hipGetLastError());  // an instantiation the device cannot launch must not pass as "nothing written"
    launch_untile_rows(ot, Mp / 16, ol, odim, rows, odim, st_);
    Q3_HIP(hipStreamSynchronize(st_));
    Q3_HIP(hipMemcpy(d.out, ol, size_t(rows) * odim * 2, hipMemcpyDeviceToHost));
    Q3_HIP(hipMemcpy(d.kpool, kp, pool * 2, hipMemcpyDeviceToHost));
    Q3_HIP(hipMemcpy(d.vpool, vp, pool * 2, hipMemcpyDeviceToHost));
}

// q3tts_debug_gemm (q3tts.h): everything the kernels turn into an address is checked here against the sizes the caller states.
void Engine::debug_gemm_check(q3tts_gemm_debug& d, GemmArgs& ga, NormRowsArgs& na) {
    static const uint16_t dummy16 = 0;  // geometry_only: "this operand takes part" without a buffer
    static const uint32_t dummy32 = 0;
    d.rode = d.tall = d.tall_shape = d.split = d.mbw = d.nw = d.ch = d.np = d.gx = d.ntw = d.tm = 0;
    Q3_CHECK(d.mode == 0 || d.mode == 1, 3, "debug_gemm: unknown mode");
    const bool rider = d.mode == 1 || d.rider_M > 0;
    if (rider) {
        Q3_CHECK(d.rider_M >= 1 && d.rider_MB >= 1 && d.rider_MB <= 64 && d.rider_M <= 16 * d.rider_MB, 3, "debug_gemm: rider rows out of range");
        Q3_CHECK(d.rider_H >= 128 && d.rider_H <= 4096 && d.rider_H % 128 == 0, 3, "debug_gemm: rider_H must be a multiple of 128 up to 4096");
        Q3_CHECK(d.geometry_only || (d.rider_h && d.rider_w && d.rider_out), 3, "debug_gemm: null rider argument");
        if (d.rider_ss_in) Q3_CHECK(d.rider_ss_count >= 1 && d.rider_ss_count <= 256, 3, "debug_gemm: at most 256 partial sums of squares per rider row");
        na.hMB = na.outMB = d.rider_MB; na.eps = d.rider_eps; na.M = d.rider_M; na.H = d.rider_H;
        na.ss_count = d.rider_ss_in ? d.rider_ss_count : 0; na.ss_ld = 16 * d.rider_MB;
    }
    if (d.mode == 1) return;
    Q3_CHECK(d.epi == 0 || d.epi == 2 || d.epi == 3, 3, "debug_gemm: unknown epilogue");
    Q3_CHECK(d.M >= 1 && d.M <= 1024, 3, "debug_gemm: M out of range");
    Q3_CHECK(d.K >= 128 && d.K <= 8192 && d.K % 128 == 0, 3, "debug_gemm: K must be a multiple of 128 up to 8192");
    Q3_CHECK(d.N >= 8 && d.N <= 65536 && d.N % (d.epi == 2 ? 8 : 16) == 0, 3, "debug_gemm: N must be a multiple of 16 (epi 2: of 8)");
    const int Mp = int(align_up(size_t(d.M), 16));
    const bool tiled = d.epi != 0 || d.y_tiled;
    Q3_CHECK(d.xMB <= 64 && 16 * d.xMB >= Mp && d.yMB <= 64 && 16 * d.yMB >= Mp && d.ss_ld >= Mp && d.ss_ld <= 4096, 3,
             "debug_gemm: allocation smaller than the padded batch");
    Q3_CHECK(d.y_cols >= d.N && d.y_cols <= d.N + 1024 && d.y_cols % (tiled ? 128 : 8) == 0, 3, "debug_gemm: y_cols");
    Q3_CHECK(d.epi != 2 || (!d.has_bias && !d.act_silu), 3, "debug_gemm: the gate/up epilogue takes no bias or activation");
    Q3_CHECK(d.epi == 0 || !d.act_silu, 3, "debug_gemm: act_silu belongs to epi 0");
    Q3_CHECK(d.epi == 3 || (!d.resid && !d.ss_out), 3, "debug_gemm: resid / ss_out belong to epi 3");
    if (d.norm) Q3_CHECK(d.ss_count >= 1 && d.ss_count <= 4096 && d.norm_dim >= 1, 3, "debug_gemm: norm prologue sizes");
    if (!d.geometry_only) {
        Q3_CHECK(d.x && d.W && d.y, 3, "debug_gemm: null argument");
        Q3_CHECK((d.epi == 2) == (d.W_up != nullptr), 3, "debug_gemm: W_up goes with epi 2");
        Q3_CHECK((d.quant != 0) == (d.scales != nullptr) && (d.quant != 0) == (d.biases != nullptr), 3, "debug_gemm: scales / biases go with quant");
        if (d.epi == 2) Q3_CHECK((d.quant != 0) == (d.scales_up != nullptr) && (d.quant != 0) == (d.biases_up != nullptr), 3, "debug_gemm: scales / biases go with quant");
        Q3_CHECK((d.has_bias != 0) == (d.bias != nullptr), 3, "debug_gemm: bias goes with has_bias");
        Q3_CHECK((d.norm != 0) == (d.norm_w != nullptr) && (d.norm != 0) == (d.ss_in != nullptr), 3, "debug_gemm: norm_w / ss_in go with norm");
    }
    ga.Wsb = d.quant ? &dummy32 : nullptr;
    ga.xMB = d.xMB; ga.M = d.M; ga.Mpad = Mp; ga.N = d.N; ga.K = d.K; ga.epi = d.epi;
    ga.ldy = d.y_cols; ga.y_tiled = d.y_tiled ? 1 : 0; ga.yMB = d.yMB;
    ga.bias = d.has_bias ? &dummy16 : nullptr;
    ga.act_silu = d.act_silu ? 1 : 0;
    ga.norm_w = d.norm ? &dummy16 : nullptr;
    ga.ss_count = d.norm ? d.ss_count : 0; ga.ss_ld = d.ss_ld; ga.norm_dim = d.norm_dim; ga.norm_eps = d.norm_eps;
    ga.nt_weights = d.nt_weights ? 1 : 0; ga.resid = d.resid ? 1 : 0;
    const SkinnyGeom g = skinny_geometry(ga);
    d.tall = g.tall ? 1 : 0;
    if (g.tall) {
        d.tall_shape = gemm_tall_shape(ga);
    } else {
        Q3_CHECK(g.mbw >= 1 && g.mbw <= 4, 3, "debug_gemm: more than 4 row blocks per workgroup");
        d.split = g.split; d.mbw = g.mbw; d.nw = g.nw; d.ch = g.ch; d.np = g.np; d.gx = g.gx; d.ntw = g.ntw ? 1 : 0; d.tm = g.tm ? 1 : 0;
    }
    if (rider) d.rode = gemm_norm_rows_rides(ga, na) ? 1 : 0;
}

namespace {
// row-major [rows][cols] <-> the fragment-major activation layout (common.h act_tiled_offset); rows % 16 == 0, cols % 128 == 0
void host_tile(const uint16_t* src, std::vector<uint16_t>& dst, int rows, int cols) {
    dst.resize(size_t(rows) * cols);
    for (int m = 0; m < rows; ++m)
        for (int k = 0; k < cols; k += 8) std::memcpy(&dst[act_tiled_offset(m, k, rows / 16)], src + size_t(m) * cols + k, 16);
}
void host_untile(const std::vector<uint16_t>& src, uint16_t* dst, int rows, int cols) {
    for (int m = 0; m < rows; ++m)
        for (int k = 0; k < cols; k += 8) std::memcpy(dst + size_t(m) * cols + k, &src[act_tiled_offset(m, k, rows / 16)], 16);
}
}  // namespace

void Engine::debug_gemm(q3tts_gemm_debug& d) {
    GemmArgs ga{};
    NormRowsArgs na{};
    debug_gemm_check(d, ga, na);
    DevBuf<uint16_t> dx, dy, dbias, dnw, dsrc, dsc, dbi, rh, rw, rout;
    DevBuf<uint8_t> dWt;
    DevBuf<uint32_t> dWq, dsb;
    DevBuf<float> dssi, dsso, rssi, rsso;
    std::vector<uint16_t> tmp;
    auto up16 = [&](DevBuf<uint16_t>& b, const uint16_t* src, size_t n) {
        b.grow(n);
        Q3_HIP(hipMemcpy(b, src, n * 2, hipMemcpyHostToDevice));
    };
    const bool rider = d.mode == 1 || d.rider_M > 0;
    const int rrows = 16 * d.rider_MB;
    if (rider) {
        host_tile(d.rider_h, tmp, rrows, d.rider_H);
        up16(rh, tmp.data(), tmp.size());
        host_tile(d.rider_out, tmp, rrows, d.rider_H);
        up16(rout, tmp.data(), tmp.size());
        up16(rw, d.rider_w, size_t(d.rider_H));
        na.h = rh; na.w = rw; na.out = rout;
        if (d.rider_ss_in) {
            rssi.grow(size_t(d.rider_ss_count) * rrows);
            Q3_HIP(hipMemcpy(rssi, d.rider_ss_in, size_t(d.rider_ss_count) * rrows * 4, hipMemcpyHostToDevice));
            na.ss_in = rssi;
        }
        if (d.rider_ss_out) {
            rsso.grow(size_t(rrows));
            Q3_HIP(hipMemcpy(rsso, d.rider_ss_out, size_t(rrows) * 4, hipMemcpyHostToDevice));
            na.ss_out = rsso;
        }
    }
    const bool tiled = d.mode == 0 && (d.epi != 0 || d.y_tiled);
    const int yrows = 16 * d.yMB, n_tiles = d.mode == 0 ? (d.epi == 2 ? d.N / 8 : d.N / 16) : 0, KC = d.K / 128;
    const size_t n_ss_out = d.mode == 0 ? size_t(d.N / 16) * d.ss_ld : 0;
    if (d.mode == 0) {
        host_tile(d.x, tmp, 16 * d.xMB, d.K);
        up16(dx, tmp.data(), tmp.size());
        if (tiled) {
            host_tile(d.y, tmp, yrows, d.y_cols);
            up16(dy, tmp.data(), tmp.size());
        } else {
            up16(dy, d.y, size_t(yrows) * d.y_cols);
        }
        // the weights as the loader tiles them (model.cc put_linear): zeroed destination, one launch per source matrix
        const size_t wbytes = d.quant ? size_t(n_tiles) * 16 * d.K / 2 : size_t(n_tiles) * 16 * d.K * 2;
        dWt.grow(wbytes);
        Q3_HIP(hipMemset(dWt, 0, wbytes));
        if (d.quant) {
            dsb.grow(size_t(n_tiles) * KC * 64);
            Q3_HIP(hipMemset(dsb, 0, size_t(n_tiles) * KC * 64 * 4));
        }
        const int rpt = d.epi == 2 ? 8 : 16;
        for (int part = 0; part < (d.epi == 2 ? 2 : 1); ++part) {
            const void* W = part ? d.W_up : d.W;
            if (d.quant) {
                dWq.grow(size_t(d.N) * d.K / 8);
                Q3_HIP(hipMemcpy(dWq, W, size_t(d.N) * d.K / 8 * 4, hipMemcpyHostToDevice));
                up16(dsc, part ? d.scales_up : d.scales, size_t(d.N) * d.K / 64);
                up16(dbi, part ? d.biases_up : d.biases, size_t(d.N) * d.K / 64);
                launch_tile_int4(dWq, dsc, dbi, d.N, d.K, dWt, dsb, KC, 0, 1, st_, rpt, 8 * part);
            } else {
                up16(dsrc, static_cast<const uint16_t*>(W), size_t(d.N) * d.K);
                launch_tile_weights(dsrc, d.N, d.K, reinterpret_cast<uint16_t*>(static_cast<uint8_t*>(dWt)), KC, 0, 1, st_, rpt, 8 * part);
            }
            Q3_HIP(hipStreamSynchronize(st_));  // the staging buffers are reused
        }
        if (d.bias) up16(dbias, d.bias, size_t(d.N));
        if (d.norm) {
            up16(dnw, d.norm_w, size_t(d.K));
            dssi.grow(size_t(d.ss_count) * d.ss_ld);
            Q3_HIP(hipMemcpy(dssi, d.ss_in, size_t(d.ss_count) * d.ss_ld * 4, hipMemcpyHostToDevice));
        }
        if (d.ss_out) {
            dsso.grow(n_ss_out);
            Q3_HIP(hipMemcpy(dsso, d.ss_out, n_ss_out * 4, hipMemcpyHostToDevice));
        }
        ga.W = reinterpret_cast<const uint16_t*>(static_cast<uint8_t*>(dWt));
        ga.Wsb = d.quant ? static_cast<uint32_t*>(dsb) : nullptr;
        ga.x = dx; ga.y = dy;
        ga.bias = d.bias ? static_cast<uint16_t*>(dbias) : nullptr;
        ga.norm_w = d.norm ? static_cast<uint16_t*>(dnw) : nullptr;
        ga.ss_in = d.norm ? static_cast<float*>(dssi) : nullptr;
        ga.ss_out = d.ss_out ? static_cast<float*>(dsso) : nullptr;
    }
    bool launched = true;
    if (d.mode == 1) {
        launch_norm_rows(na, st_);
    } else if (rider) {
        launched = launch_gemm_skinny_with_norm_rows(ga, na, st_);
        Q3_CHECK(launched == (d.rode != 0), 7, "debug_gemm: the rider launch disagrees with gemm_norm_rows_rides");
    } else {
        launch_gemm_skinny(ga, st_);
    }
    Q3_HIP(hipGetLastError());  // an instantiation the device cannot launch must not pass as "nothing written"
    Q3_HIP(hipStreamSynchronize(st_));
    if (!launched) return;
    if (d.mode == 0) {
        if (tiled) {
            tmp.resize(size_t(yrows) * d.y_cols);
            Q3_HIP(hipMemcpy(tmp.data(), dy, tmp.size() * 2, hipMemcpyDeviceToHost));
            host_untile(tmp, d.y, yrows, d.y_cols);
        } else {
            Q3_HIP(hipMemcpy(d.y, dy, size_t(yrows) * d.y_cols * 2, hipMemcpyDeviceToHost));
        }
        if (d.ss_out) Q3_HIP(hipMemcpy(d.ss_out, dsso, n_ss_out * 4, hipMemcpyDeviceToHost));
    }
    if (rider) {
        tmp.resize(size_t(rrows) * d.rider_H);
        Q3_HIP(hipMemcpy(tmp.data(), rout, tmp.size() * 2, hipMemcpyDeviceToHost));
        host_untile(tmp, d.rider_out, rrows, d.rider_H);
        if (d.rider_ss_out) Q3_HIP(hipMemcpy(d.rider_ss_out, rsso, size_t(rrows) * 4, hipMemcpyDeviceToHost));
    }
}

// Codes a CALLER hands in (q3tts_codec_decode, q3tts_codec_decode_streamed) index the RVQ tables on the GPU: every code of every frame
// that will be decoded is checked against the tables as loaded. (Codes the engine sampled itself are inside by construction:
// the samplers draw below the vocabulary, the tables have at least that many rows.)
static void check_caller_codes(const CodecW& w, const int32_t* codes, const int32_t* n_frames, int batch, int max_frames) {
    for (int b = 0; b < batch; ++b)
        for (int f = 0; f < n_frames[b]; ++f) {
            const int32_t* c = codes + (size_t(b) * max_frames + f) * 16;
            Q3_CHECK(c[0] >= 0 && c[0] < w.cb_first_rows, 3, "Invalid input: first code outside the semantic codebook");
            for (size_t j = 0; j < w.cb_rest.size(); ++j)
                Q3_CHECK(c[1 + j] >= 0 && c[1 + j] < w.cb_rest_rows, 3, "Invalid input: code outside the acoustic codebook");
        }
}

void Engine::codec_decode(const int32_t* codes, const int32_t* n_frames, int batch, int max_frames, float* pcm,
                          int64_t* audio_lengths) {
    Q3_CHECK(m_->has_codec, 1, "Model not initialized: Speech tokenizer not loaded");
    Q3_CHECK(batch >= 1 && max_frames >= 1, 3, "Invalid input: empty codec batch");
    const int up = codec_->upsample();
    std::vector<int> frames((size_t)(batch));
    int Fmax = 0;
    for (int b = 0; b < batch; ++b) {
        Q3_CHECK(n_frames[b] >= 0 && n_frames[b] <= max_frames, 3, "Invalid input: n_frames out of range");
        frames[size_t(b)] = n_frames[b];
        Fmax = std::max(Fmax, n_frames[b]);
    }
    check_caller_codes(m_->codec, codes, n_frames, batch, max_frames);
    DevBuf<int32_t> dcodes;
    dcodes.grow(size_t(batch) * max_frames * 16);
    Q3_HIP(hipMemcpy(dcodes, codes, size_t(batch) * max_frames * 16 * 4, hipMemcpyHostToDevice));
    float* pcm_dev = nullptr;
    hipStream_t cst = codec_stream(false);
    PinnedBuf<int32_t> nf;  // rows whose waveform came out non-finite
    nf.grow(size_t(batch));
    std::memset(nf, 0, size_t(batch) * 4);
    Q3_HIP(hipEventRecord(ev_[2], cst));
    if (Fmax > 0) codec_->decode(dcodes, max_frames, frames, &pcm_dev, std::string(), nullptr, nullptr, nullptr, nf);
    Q3_HIP(hipEventRecord(ev_[3], cst));
    Q3_HIP(hipStreamSynchronize(cst));
    bool bad = false;
    for (int b = 0; b < batch; ++b) bad = bad || nf[b] != 0;
    if (bad && !codec_->fp32_convs()) {
        // an activation left the fp16 range of the default kernels: the whole call once more on the fp32 matrix cores (the
        // reference's range; redo_rows_fp32 does the same for rows of a generate call)
        std::memset(nf, 0, size_t(batch) * 4);
        codec_->decode(dcodes, max_frames, frames, &pcm_dev, std::string(), nullptr, nullptr, nullptr, nf, true);
        Q3_HIP(hipEventRecord(ev_[3], cst));
        Q3_HIP(hipStreamSynchronize(cst));
        bad = false;
        for (int b = 0; b < batch; ++b) bad = bad || nf[b] != 0;
    }
    if (bad) throw Error(4, kCodecRangeMsg);
    float ms = 0;
    Q3_HIP(hipEventElapsedTime(&ms, ev_[2], ev_[3]));
    timing.codec_ms = ms;
    for (int b = 0; b < batch; ++b) {
        const int F = frames[size_t(b)];
        if (F > 0)
            Q3_HIP(hipMemcpy(pcm + size_t(b) * max_frames * up, pcm_dev + size_t(b) * Fmax * up, size_t(F) * up * 4,
                             hipMemcpyDeviceToHost));
        int valid = 0;
        for (int f = 0; f < F; ++f) valid += codes[(size_t(b) * max_frames + f) * 16] > 0 ? 1 : 0;
        audio_lengths[b] = int64_t(valid) * up;  // SpeechTokenizer.swift:831-833
    }
}

void Engine::codec_decode_streamed(const int32_t* codes, const int32_t* n_frames, int batch, int max_frames, int chunk_frames, int window,
                                   int lookahead, float* pcm) {
    Q3_CHECK(m_->has_codec, 1, "Model not initialized: Speech tokenizer not loaded");
    Q3_CHECK(batch >= 1 && max_frames >= 1 && chunk_frames >= 1, 3, "Invalid input: empty codec batch");
    const int up = codec_->upsample();
    DevBuf<int32_t> dcodes;
    PinnedBuf<float> hpcm;
    struct Events {  // chunk_done of stream_push
        std::vector<hipEvent_t> v;
        ~Events() {
            for (auto e : v) (void)hipEventDestroy(e);
        }
    } done;
    dcodes.grow(size_t(batch) * max_frames * 16);
    Q3_HIP(hipMemcpy(dcodes, codes, size_t(batch) * max_frames * 16 * 4, hipMemcpyHostToDevice));
    hpcm.grow(size_t(batch) * max_frames * up);
    std::memset(hpcm, 0, size_t(batch) * max_frames * up * 4);
    std::vector<int> avail((size_t)(batch));
    std::vector<uint8_t> fin((size_t)(batch), 1);
    int Fmax = 0;
    for (int b = 0; b < batch; ++b) {
        Q3_CHECK(n_frames[b] >= 0 && n_frames[b] <= max_frames, 3, "Invalid input: n_frames out of range");
        avail[size_t(b)] = n_frames[b];
        Fmax = std::max(Fmax, n_frames[b]);
    }
    check_caller_codes(m_->codec, codes, n_frames, batch, max_frames);
    hipStream_t cst = codec_stream(false);
    CodecRunner::StreamCfg cfg;
    cfg.rows = batch; cfg.chunk_frames = chunk_frames; cfg.window = window; cfg.lookahead = lookahead; cfg.max_frames = std::max(Fmax, 1);
    codec_->stream_open(cfg);
    try {
        // as a stream would deliver them: frames become available chunk by chunk (window >= 0); all at once otherwise
        if (window >= 0) {
            std::vector<uint8_t> notyet((size_t)(batch), 0);
            for (int have = chunk_frames; have < Fmax + chunk_frames + lookahead; have += chunk_frames) {
                std::vector<int> a((size_t)(batch));
                for (int b = 0; b < batch; ++b) {
                    a[size_t(b)] = std::min(avail[size_t(b)], have);
                    notyet[size_t(b)] = a[size_t(b)] == avail[size_t(b)] ? 1 : 0;
                }
                codec_->stream_push(dcodes, max_frames, a.data(), notyet.data(), hpcm, size_t(max_frames) * up, done.v);
            }
        }
        codec_->stream_push(dcodes, max_frames, avail.data(), fin.data(), hpcm, size_t(max_frames) * up, done.v);
    } catch (...) {
        codec_->stream_close();
        throw;
    }
    codec_->stream_close();
    Q3_HIP(hipStreamSynchronize(cst));
    for (int b = 0; b < batch; ++b)
        std::memcpy(pcm + size_t(b) * max_frames * up, hpcm + size_t(b) * max_frames * up, size_t(n_frames[b]) * up * 4);
}

// The streamed decode of rows that carry a reference prefix (include/q3tts.h, "streamed clone rows"), through the slotted stream
// with every row reset at the start; the frames arrive a chunk per push, as a stream would deliver them.
void Engine::codec_decode_streamed_prefixed(const int32_t* codes, const int32_t* n_prefix, const int32_t* n_frames, int batch, int max_frames,
                                            int chunk_frames, int window, int lookahead, float* pcm) {
    Q3_CHECK(m_->has_codec, 1, "Model not initialized: Speech tokenizer not loaded");
    Q3_CHECK(batch >= 1 && max_frames >= 1 && chunk_frames >= 1 && window >= 0 && lookahead >= 0, 3, "Invalid input: empty codec batch");
    Q3_CHECK(batch <= Bm_, 3, "Invalid input: batch must be between 1 and max_batch");
    int Fmax = 0, Rmax = 0;
    std::vector<int32_t> total((size_t)(batch));
    for (int b = 0; b < batch; ++b) {
        Q3_CHECK(n_prefix[b] >= 0 && n_frames[b] >= 0 && int64_t(n_prefix[b]) + n_frames[b] <= max_frames, 3,
                 "Invalid input: n_prefix + n_frames out of range");
        total[size_t(b)] = n_prefix[b] + n_frames[b];
        Fmax = std::max(Fmax, n_frames[b]);
        Rmax = std::max(Rmax, n_prefix[b]);
    }
    check_caller_codes(m_->codec, codes, total.data(), batch, max_frames);
    check_stream_chunk(chunk_frames);
    const int up = codec_->upsample();
    DevBuf<int32_t> dcodes;
    dcodes.grow(size_t(batch) * max_frames * 16);
    Q3_HIP(hipMemcpy(dcodes, codes, size_t(batch) * max_frames * 16 * 4, hipMemcpyHostToDevice));
    SlotStream ss(*this, batch, chunk_frames, window, lookahead, std::max(Fmax, 1), false, Rmax);
    ss.hold = false;  // (as q3tts_codec_decode_streamed: the samples as the default kernels produce them)
    for (int b = 0; b < batch; ++b) ss.admit(b, b, std::max(Fmax, 1), n_prefix[b]);
    std::vector<int> avail((size_t)(batch));
    std::vector<uint8_t> fin((size_t)(batch));
    for (int have = chunk_frames;; have += chunk_frames) {
        bool all = true;
        for (int b = 0; b < batch; ++b) {
            avail[size_t(b)] = std::min(n_frames[b], have);
            fin[size_t(b)] = avail[size_t(b)] == n_frames[b] ? 1 : 0;
            all = all && fin[size_t(b)];
        }
        ss.push(dcodes, max_frames, avail.data(), fin.data());
        if (all) break;
    }
    for (int b = 0; b < batch; ++b) ss.retire(b, n_frames[b]);
    ss.finish();
    for (int b = 0; b < batch; ++b) {
        Q3_CHECK(ss.out[b].complete, 7, "internal error: a row of the prefixed stream was left incomplete");
        std::memcpy(pcm + size_t(b) * Fmax * up, ss.out[b].pcm.get(), size_t(n_frames[b]) * up * 4);
    }
}

// The slotted stream as a streamed queue drives it, without the talker: the schedule of stream_plan.h decides when a request
// takes a slot, how many frames it has at each push and when it is retired; the codes come from the caller.
void Engine::debug_codec_stream_slots(const int32_t* codes, const int32_t* n_frames, int n_reqs, int max_frames, int slots, int burst,
                                      int chunk_frames, int window, int lookahead, float* pcm) {
    Q3_CHECK(m_->has_codec, 1, "Model not initialized: Speech tokenizer not loaded");
    Q3_CHECK(n_reqs >= 1 && max_frames >= 1 && burst >= 1 && chunk_frames >= 1 && window >= 0 && lookahead >= 0, 3,
             "Invalid input: empty codec batch");
    Q3_CHECK(slots >= 1 && slots <= Bm_, 3, "Invalid input: slots must be between 1 and max_batch");
    for (int i = 0; i < n_reqs; ++i) Q3_CHECK(n_frames[i] >= 0 && n_frames[i] <= max_frames, 3, "Invalid input: n_frames out of range");
    check_caller_codes(m_->codec, codes, n_frames, n_reqs, max_frames);
    check_stream_chunk(chunk_frames);
    const int up = codec_->upsample();
    DevBuf<int32_t> all, scodes;  // every request's codes; the stream's own buffer [slots][max_frames][16]
    all.grow(size_t(n_reqs) * max_frames * 16);
    scodes.grow(size_t(slots) * max_frames * 16);
    Q3_HIP(hipMemcpy(all, codes, size_t(n_reqs) * max_frames * 16 * 4, hipMemcpyHostToDevice));
    SlotStream ss(*this, slots, chunk_frames, window, lookahead, max_frames, false);
    ss.hold = false;  // (as q3tts_codec_decode_streamed: the samples as the default kernels produce them)
    std::vector<int> copied((size_t)(slots), 0);
    replay_queue_schedule(
        n_frames, n_reqs, slots, burst,
        [&](int s, int r) {
            ss.admit(s, r, max_frames);
            copied[size_t(s)] = 0;
        },
        [&](const int* avail, const uint8_t* fin, const int* req) {
            for (int s = 0; s < slots; ++s) {  // on the codec stream itself: behind every pass that read the slot's earlier codes
                if (req[s] < 0 || avail[s] <= copied[size_t(s)]) continue;
                Q3_HIP(hipMemcpyAsync(scodes + (size_t(s) * max_frames + copied[size_t(s)]) * 16,
                                      all + (size_t(req[s]) * max_frames + copied[size_t(s)]) * 16, size_t(avail[s] - copied[size_t(s)]) * 64,
                                      hipMemcpyDeviceToDevice, ss.cst));
                copied[size_t(s)] = avail[s];
            }
            ss.push(scodes, max_frames, avail, fin);
            for (int s = 0; s < slots; ++s)
                if (req[s] >= 0 && fin[s]) ss.retire(s, avail[s]);
        });
    ss.finish();
    for (int i = 0; i < n_reqs; ++i) {
        Q3_CHECK(ss.out[i].complete, 7, "internal error: a request of the slotted stream was left incomplete");
        std::memcpy(pcm + size_t(i) * max_frames * up, ss.out[i].pcm.get(), size_t(n_frames[i]) * up * 4);
    }
}

void Engine::debug_codec_stage(const int32_t* codes, int n_frames, const char* stage, float* out, int64_t cap, int* T, int* C) {
    Q3_CHECK(m_->has_codec, 1, "Model not initialized: Speech tokenizer not loaded");
    DevBuf<int32_t> dcodes;
    dcodes.grow(size_t(n_frames) * 16);
    Q3_HIP(hipMemcpy(dcodes, codes, size_t(n_frames) * 16 * 4, hipMemcpyHostToDevice));
    std::vector<float> so;
    float* pcm_dev = nullptr;
    (void)codec_stream(false);
    codec_->decode(dcodes, n_frames, {n_frames}, &pcm_dev, stage, &so, T, C);
    Q3_CHECK(int64_t(so.size()) <= cap, 3, "debug_codec_stage: output buffer too small");
    std::memcpy(out, so.data(), so.size() * 4);
}

}  // namespace q3
