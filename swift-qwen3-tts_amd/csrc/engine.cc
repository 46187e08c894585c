// engine.cc -- generation driver. See engine.h.
#include "engine_stream.h"

#include "frontend.h"

namespace q3 {

namespace {
std::string lower(const std::string& s) {
    std::string o = s;
    for (auto& c : o) c = char(std::tolower((unsigned char)c));
    return o;
}
}  // namespace

Engine::Engine(Model* model, const q3tts_load_opts& opts, float pitch, bool keep_formants) : m_(model), opts_(opts) {
    Q3_HIP(hipSetDevice(m_->device));
    {
        // The AR loop is a chain of short dependent launches (latency), the codec decode a few hundred large ones
        // (matrix cores): the decode of a finished batch runs on its own stream so that the NEXT batch's AR loop can
        // overlap it (begin / end). Stream priorities alone do not help: a decode kernel's workgroups fill every CU and the
        // AR chain's workgroups then queue behind them (prefill 23 -> 165 ms, nothing gained). Confined to half of the CUs
        // (mask bits interleave over the XCDs) the decode takes 1.7x as long but leaves the chain room: 879 -> 826 ms
        // per pipelined step at 1.7B / batch 32 (96 CUs: 841, 160: 841, 192: 856). A decode that nothing overlaps
        // (generate(), codec_decode) uses the unmasked stream. q3tts_load_opts.codec_overlap_cus overrides the CU count.
        // (Half is the share beside ONE chain; a background job's decode gets a wider stream, prepare_job_pair.)
        int least = 0, greatest = 0;
        Q3_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
        Q3_HIP(hipStreamCreateWithPriority(&st_, hipStreamNonBlocking, greatest));
        Q3_HIP(hipStreamCreateWithPriority(&st_codec_, hipStreamNonBlocking, least));
        hipDeviceProp_t prop{};
        Q3_HIP(hipGetDeviceProperties(&prop, m_->device));
        int cus = prop.multiProcessorCount / 2;
        if (opts.codec_overlap_cus > 0) cus = opts.codec_overlap_cus;   // q3tts_load_opts: the caller's own tuning
        else if (opts.codec_overlap_cus < 0) cus = 0;
        cus = std::min(cus, prop.multiProcessorCount) / 8 * 8;
        if (cus > 0 && cus < prop.multiProcessorCount) st_codec_part_ = masked_stream(cus, prop.multiProcessorCount);
    }
    for (auto& J : jobs_) {
        for (auto& e : J.ev_codec) Q3_HIP(hipEventCreate(&e));
        Q3_HIP(hipEventCreate(&J.ev_begin));
        Q3_HIP(hipEventCreate(&J.ev_first_audio));
        std::memset(J.nf_host.grow(size_t(std::max(opts.max_batch, 1))), 0, size_t(std::max(opts.max_batch, 1)) * 4);
    }
    for (auto& e : ev_) Q3_HIP(hipEventCreate(&e));
    for (auto& e : burst_ev_) Q3_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (auto& e : ev_fe_) Q3_HIP(hipEventCreate(&e));
    Q3_HIP(hipEventCreateWithFlags(&fe_uploaded_, hipEventDisableTiming));
    Bm_ = opts.max_batch;
    // activation rows per launch (batch rows x positions): 256 rows run the code predictor's two-position step 0 as one pass up
    // to batch 128; a prefill chunk is up to 16 positions of every row, so the buffers hold 16 rows per batch row (the GEMMs
    // take them as row blocks of <= 64 on grid.y and stream the weights once per chunk: 32 x 48 prompt positions at 1.7B
    // 14.1 -> 11.0 ms against 8-position chunks; the chunk boundaries do not change a bit, tests/test_scheduling.py)
    Mp_ = std::getenv("Q3TTS_ROWS_64") ? 64 : std::max(256, 16 * int(align_up(size_t(opts.max_batch), 16)));
    Pcap_ = opts.max_prompt;
    Tcap_ = opts.max_prompt;
    Fcap_ = opts.max_frames;
    max_pages_ = ceil_div(Pcap_ + Fcap_ + 1, kPageTokens);
    n_pages_ = Bm_ * max_pages_;
    for (auto& kv : m_->cfg.talker.spk_id) speakers.push_back(kv.first);
    std::sort(speakers.begin(), speakers.end());
    alloc_workspace();
    if (std::getenv("Q3TTS_FRAME_STAMPS")) {
        Q3_HIP(hipMalloc(reinterpret_cast<void**>(&stamps_), 64 * 8));
        Q3_HIP(hipMemset(stamps_, 0, 64 * 8));
    }
    if (m_->has_codec)
        codec_ = std::make_unique<CodecRunner>(*m_, st_codec_, opts.codec_fp32 != 0, opts.output_sample_rate, opts.speed,
                                               opts.request_speeds != 0, pitch, keep_formants);
    if (m_->has_codec_encoder || m_->has_speaker_encoder) fe_ = std::make_unique<VoiceFrontEnd>(*m_, st_);
}

// mask bit i = CU (i / 8) of XCD (i % 8), CUs of an XCD numbered round-robin over its shader engines: the first `cus` bits are
// the same share of every shader engine of every XCD. (Every other CU instead -- whole shader engines -- left the AR chain's
// workgroups queueing on the busy engines: 1008 against 807 ms per step.)
hipStream_t Engine::masked_stream(int cus, int total) {
    std::vector<uint32_t> mask(size_t(ceil_div(total, 32)), 0u);
    for (int i = 0; i < cus; ++i) mask[size_t(i / 32)] |= 1u << (i % 32);
    hipStream_t st = nullptr;
    Q3_HIP(hipExtStreamCreateWithCUMask(&st, uint32_t(mask.size()), mask.data()));
    return st;
}

// This engine is one of an EngineGroup's two job contexts and jobs may run in the background (Engine::begin). Called at load:
// nothing here is left for a steady-state step.
void Engine::prepare_job_pair() {
    job_chains = 2;  // two jobs' chains submit at once: under the AQL ring they count as two
    // The decode's share of the chip was tuned beside ONE chain (half of the CUs, Engine::Engine), and a job whose frame loop
    // runs inside begin still gets that. Two background jobs reach their decodes together, so such a decode mostly runs beside
    // the other decode or one chain's tail, and the wider it is the sooner the next pair starts: 1.7B / batch 32 x 200 frames,
    // frames/s at 64 / 96 / 128 / 160 / 192 CUs / unconfined: 9101 / 10097 / 10934 / 11042 / 11213 / 11222
    // (profiles/r06_concurrent_jobs_ab.txt). A background job's decode therefore gets three quarters of the CUs: that keeps the
    // confinement for a chain that does run beside it at no measurable cost against none. The caller's own
    // codec_overlap_cus, when set, holds for every job.
    if (opts_.codec_overlap_cus != 0 || !st_codec_part_ || st_codec_wide_) return;
    hipDeviceProp_t prop{};
    Q3_HIP(hipGetDeviceProperties(&prop, m_->device));
    st_codec_wide_ = masked_stream(prop.multiProcessorCount * 3 / 4 / 8 * 8, prop.multiProcessorCount);
}

Engine::~Engine() {
    if (worker_.joinable()) {  // a back half that was begun runs to its end first: it uses everything destroyed below
        {
            std::lock_guard<std::mutex> lk(work_mu_);
            work_stop_ = true;
        }
        work_cv_.notify_all();
        worker_.join();
    }
    if (stager_.joinable()) {
        {
            std::lock_guard<std::mutex> lk(stage_mu_);
            stage_stop_ = true;
        }
        stage_cv_.notify_all();
        stager_.join();
    }
    for (auto& g : graphs_) (void)hipGraphExecDestroy(g.second);
    for (auto& g : qgraphs_) (void)hipGraphExecDestroy(g.second);
    for (auto& g : ographs_) (void)hipGraphExecDestroy(g.second);
    if (qws_) (void)hipFree(qws_);
    codec_.reset();
    fe_.reset();
    live_close();
    for (auto& L : fe_lanes_) {
        L.fe.reset();
        if (L.done) (void)hipEventDestroy(L.done);
        if (L.st) (void)hipStreamDestroy(L.st);
    }
    for (auto& J : jobs_) {
        for (auto& e : J.chunk_done)
            if (e) (void)hipEventDestroy(e);
        for (auto& e : J.ev_codec)
            if (e) (void)hipEventDestroy(e);
        if (J.ev_begin) (void)hipEventDestroy(J.ev_begin);
        if (J.ev_first_audio) (void)hipEventDestroy(J.ev_first_audio);
    }
    if (ws_) (void)hipFree(ws_);
    for (void* p : {(void*)forced_dev_, (void*)sampled_dev_, (void*)tl_dump_, (void*)cl_dump_})
        if (p) (void)hipFree(p);
    for (auto& e : ev_)
        if (e) (void)hipEventDestroy(e);
    for (auto& e : burst_ev_)
        if (e) (void)hipEventDestroy(e);
    for (auto& e : ev_fe_)
        if (e) (void)hipEventDestroy(e);
    if (fe_uploaded_) (void)hipEventDestroy(fe_uploaded_);
    if (stamps_) {  // phase times of the frame step, accumulated over every frame step this engine ran
        unsigned long long h[64];
        if (hipMemcpy(h, stamps_, sizeof(h), hipMemcpyDeviceToHost) == hipSuccess && h[0] > 0) {
            static const char* nm[] = {"", "talker layers", "codec_head + norm + sampler (+ proj)", "predictor pair pass",
                                       "pass-0 head + sampler", "predictor passes 1..14 (layers)", "their heads + samplers", "frame_end"};
            std::fprintf(stderr, "[q3tts frame stamps] %llu frame steps\n", h[0]);
            for (int k = 1; k < 8; ++k) std::fprintf(stderr, "  %-40s %8.1f us per step\n", nm[k], double(h[k]) / 100.0 / double(h[0]));
        }
        (void)hipFree(stamps_);
    }
    if (st_codec_wide_) (void)hipStreamDestroy(st_codec_wide_);
    if (st_codec_part_) (void)hipStreamDestroy(st_codec_part_);
    if (st_codec_) (void)hipStreamDestroy(st_codec_);
    if (st_) (void)hipStreamDestroy(st_);
}

// CodePredictor.swift:327-330 projects the embedding of every sampled code (H wide) down to the predictor's width before
// each of passes 1..14. The projection of a table row does not depend on anything else, so it is taken once per row at
// load -- by the very GEMM kernel the frame step would have launched, Mp_ codes at a time, so the rows (and their per-tile sums
// of squares for the next norm prologue) are bit-identical to projecting at run time -- and the frame step loses 14 launches.
// The tables are cut from the weights, which may arrive after load (weights_from_broadcast): first use, not load.
void Engine::build_cp_proj_tables() {
    if (cp_tables_ || !m_->has_cp_proj || std::getenv("Q3TTS_NO_PROJ_TABLES")) return;
    const TalkerConfig& t = m_->cfg.talker;
    const int H = t.hidden_size, CH = m_->cp.hidden, MBL = Mp_ / 16, Vc = t.cp.vocab_size, nss = CH / 16;
    const int ntab = t.num_code_groups - 2;  // embeddings 0..13 feed passes 1..14; the last code feeds nothing
    if (ntab <= 0) return;
    std::lock_guard<std::mutex> lock(m_->lazy_mutex);  // lanes share the model; the first one to generate builds
    if (m_->cp_pe.empty()) {
        for (int i = 0; i < ntab; ++i) {
            uint16_t* pe = nullptr;
            float* pss = nullptr;
            Q3_HIP(hipMalloc(reinterpret_cast<void**>(&pe), size_t(Vc) * CH * 2));
            m_->lazy_allocs.push_back(pe);
            Q3_HIP(hipMalloc(reinterpret_cast<void**>(&pss), size_t(Vc) * nss * 4));
            m_->lazy_allocs.push_back(pss);
            for (int c0 = 0; c0 < Vc; c0 += Mp_) {
                const int rows = std::min(Mp_, Vc - c0);
                launch_tile_rows(m_->cp_emb[size_t(i)] + size_t(c0) * H, H, cp_x_, MBL, rows, H, st_);
                GemmArgs p = gemm_args(m_->cp_proj, cp_x_, rows);
                p.epi = 3; p.y = cp_.h; p.yMB = MBL; p.resid = 0; p.ss_out = cp_.ss_a;
                launch_gemm_skinny(p, st_);
                launch_untile_rows(cp_.h, MBL, pe + size_t(c0) * CH, CH, rows, CH, st_);
                launch_ss_to_table(cp_.ss_a, Mp_, pss + size_t(c0) * nss, nss, rows, st_);
            }
            m_->cp_pe.push_back(pe);
            m_->cp_pss.push_back(pss);
        }
        Q3_HIP(hipStreamSynchronize(st_));
    }
    cp_tables_ = true;
}

void Engine::alloc_workspace() {
    const TalkerConfig& t = m_->cfg.talker;
    const int H = t.hidden_size, CH = t.cp.hidden_size, TH = t.text_hidden_size;
    const int qd = t.num_attention_heads * kHeadDim, kd = t.num_key_value_heads * kHeadDim;
    const int cqd = t.cp.num_attention_heads * kHeadDim, ckd = t.cp.num_key_value_heads * kHeadDim;
    const int L = t.num_hidden_layers, CL = t.cp.num_hidden_layers;
    kv_layer_stride_ = size_t(n_pages_) * t.num_key_value_heads * kPageTokens * kHeadDim;
    cp_kv_layer_stride_ = size_t(Bm_) * t.cp.num_key_value_heads * kPageTokens * kHeadDim;
    proj_cap_ = Bm_ * (2 * Pcap_ + 8);  // text + instruct or reference-text ids + the three tts tokens per row
    for (int pass = 0; pass < 2; ++pass) {
        Bump b{pass ? ws_ : nullptr};
        Bump& x = b;
        auto stream = [&](Stream& s, int hid, int q, int k, int inter_p, int vocab) {
            s.ld_qkv = q + 2 * k;
            s.ld_act = inter_p;
            s.ld_logits = vocab;
            s.h = x.take<uint16_t>(size_t(Mp_) * hid);
            s.xn = x.take<uint16_t>(size_t(Mp_) * hid);
            s.ss_a = x.take<float>(size_t(hid / 16) * Mp_);
            s.ss_b = x.take<float>(size_t(hid / 16) * Mp_);
            s.qkv = x.take<uint16_t>(size_t(Mp_) * s.ld_qkv);
            s.ao = x.take<uint16_t>(size_t(Mp_) * q);
            s.act = x.take<uint16_t>(size_t(Mp_) * inter_p);
            s.logits = b.take<uint16_t>(size_t(Mp_) * vocab);
        };
        stream(tk_, H, qd, kd, m_->talker.max_inter_p, t.vocab_size);
        stream(cp_, CH, cqd, ckd, m_->cp.max_inter_p, t.cp.vocab_size);
        cp_x_ = x.take<uint16_t>(size_t(Mp_) * H);
        cp_x2_ = x.take<uint16_t>(size_t(Mp_) * H);
        cp_ss2_ = x.take<float>(size_t(Mp_));
        kpool_ = b.take<uint16_t>(kv_layer_stride_ * L);
        vpool_ = b.take<uint16_t>(kv_layer_stride_ * L);
        cp_kpool_ = b.take<uint16_t>(cp_kv_layer_stride_ * CL);
        cp_vpool_ = b.take<uint16_t>(cp_kv_layer_stride_ * CL);
        block_table_ = b.take<int32_t>(size_t(Bm_) * max_pages_);
        cp_block_table_ = b.take<int32_t>(size_t(Bm_));
        kv_len_ = b.take<int32_t>(size_t(Bm_));
        cp_len_ = b.take<int32_t>(size_t(Bm_));
        n_frames_ = b.take<int32_t>(size_t(Bm_));
        max_frames_ = b.take<int32_t>(size_t(Bm_));
        trailing_idx_ = b.take<int32_t>(size_t(Bm_));
        n_trailing_ = b.take<int32_t>(size_t(Bm_));
        n_prompt_ = b.take<int32_t>(size_t(Bm_));
        cur_codes_ = b.take<int32_t>(size_t(Bm_) * 16);
        codes_ = b.take<int32_t>(size_t(Bm_) * Fcap_ * 16);
        active_ = b.take<uint8_t>(size_t(Bm_));
        finished_ = b.take<uint8_t>(size_t(Bm_));
        seen_ = b.take<uint8_t>(size_t(Bm_) * t.vocab_size);
        prompt_ = b.take<uint16_t>(size_t(Bm_) * Pcap_ * H);
        trailing_ = b.take<uint16_t>(size_t(Bm_) * Tcap_ * H);
        tts_pad_ = b.take<uint16_t>(size_t(H));
        sp_dev_ = b.take<SamplingParams>(size_t(Bm_));
        ids_dev_ = b.take<int32_t>(size_t(proj_cap_));
        proj_in_ = b.take<uint16_t>(size_t(64) * TH);
        proj_mid_ = b.take<uint16_t>(size_t(64) * TH);
        proj_out_ = b.take<uint16_t>(size_t(proj_cap_ + 64) * H);
        compose_a_ = b.take<int32_t>(size_t(3) * Bm_ * (Pcap_ + Tcap_));
        compose_b_ = nullptr;
        if (!pass) {
            ws_bytes_ = align_up(b.off, 256);
            Q3_HIP(hipMalloc(reinterpret_cast<void**>(&ws_), ws_bytes_));
            Q3_HIP(hipMemset(ws_, 0, ws_bytes_));
        }
    }
    std::vector<int32_t> cbt((size_t)(Bm_));  // code-predictor cache: one private page per row
    for (int i = 0; i < Bm_; ++i) cbt[size_t(i)] = i;
    Q3_HIP(hipMemcpy(cp_block_table_, cbt.data(), cbt.size() * 4, hipMemcpyHostToDevice));
}

GemmArgs Engine::gemm_args(const LinearW& L, const uint16_t* x, int M) const {
    GemmArgs a{};
    a.W = L.w;
    a.Wsb = L.sb;
    a.x = x;
    a.xMB = Mp_ / 16;
    a.M = M;
    a.Mpad = int(align_up(size_t(M), 16));
    a.N = L.Np;
    a.K = L.Kp;
    a.bias = L.bias;
    a.ss_ld = Mp_;
    return a;
}

// One pre-norm decoder layer = 5 launches (Talker.swift:451-469):
//   qkv GEMM [RMSNorm prologue] -> attention -> o_proj GEMM [residual + sum(h^2) epilogue]
//   -> gate/up GEMM [RMSNorm prologue, SwiGLU epilogue] -> down GEMM [residual + sum(h^2) epilogue]
// w.h is the fragment-major residual stream; ss_a holds the per-tile sums of squares of the rows
// entering a layer (`ss_count_in` partials for the first layer), ss_b those after o_proj.
void Engine::enqueue_layers(const StackW& s, Stream& w, int B, uint16_t* kpool, uint16_t* vpool, size_t layer_stride,
                            const int32_t* block_table, int max_pages, const int32_t* kv_len, const uint8_t* active,
                            int ss_count_in, int fixed_len, int chunk, const int32_t* chunk_n_prompt, int chunk_r_base) {
    const int H = s.hidden, MBL = Mp_ / 16, tiles = H / 16;
    const int M = B * (chunk > 1 ? chunk : 1);  // GEMM rows: chunk element p of batch row b is row p * B + b
    Q3_CHECK(M <= Mp_, 7, "internal error: chunk does not fit the activation buffers");
    // The RMSNorm prologue re-normalises all of x in every workgroup: VALU work on the critical path that grows with K and
    // with the row blocks per workgroup (0.8-1.3 us). Against a separate row-norm launch (4.5 us) it wins at both widths
    // since the norm-prologue kernels request x before the weight tiles, take at most two row blocks per workgroup and
    // the 6144-wide gate/up runs as one round of workgroups (gemm_decode.hip); wider stacks keep the row-norm kernel.
    // Above 64 rows per launch (prefill chunks) the prologue is repeated by (column tiles x row-block groups) workgroups --
    // 2048 of them for a 6144-wide gate/up at 256 rows, ~3 us of SIMD time each -- so the rows are normalised once by
    // the row kernel instead, from the SAME per-tile partials in the same order (NormRowsArgs::ss_in): bit-identical.
    const bool row_norm = M > 64;
    const bool prologue_qkv = H <= 2048 && !row_norm, prologue_mlp = H <= 2048 && !row_norm;
    // The talker's layer weights and KV cache are read once per frame step out of gigabytes; the code predictor's
    // 0.22 GB are read fifteen times per step. Non-temporal loads on the former leave the Infinity Cache (256 MB) to the
    // latter: measured 3.53 -> 3.42 ms per 1.7B frame step with both (either one alone: < 1 %; on the predictor's
    // weights as well: 3.62 ms). Q3TTS_NT=0 turns the hint off (diagnostics).
    const bool nt_off = debug_env().nt_off;
    const bool is_talker = &s == &m_->talker;
    const int ntw = is_talker && !nt_off ? 1 : 0;
    const int ntkv = ntw;
    auto norm_into_xn = [&](const uint16_t* nw, const float* ss, int ss_count) {
        NormRowsArgs n{};
        n.h = w.h; n.hMB = MBL; n.w = nw; n.eps = s.eps; n.out = w.xn; n.outMB = MBL; n.M = M; n.H = H;
        if (row_norm && H <= 2048) { n.ss_in = ss; n.ss_count = ss_count; n.ss_ld = Mp_; }
        launch_norm_rows(n, counted());
    };
    for (size_t l = 0; l < s.layers.size(); ++l) {
        const LayerW& L = s.layers[l];
        if (!prologue_qkv) norm_into_xn(L.ln1, w.ss_a, (l == 0) ? ss_count_in : tiles);
        GemmArgs q = gemm_args(L.qkv, prologue_qkv ? w.h : w.xn, M);
        q.epi = 0; q.y = w.qkv; q.ldy = w.ld_qkv; q.nt_weights = ntw;
        if (prologue_qkv) {
            q.norm_w = L.ln1; q.ss_in = w.ss_a; q.ss_count = (l == 0) ? ss_count_in : tiles; q.norm_dim = H; q.norm_eps = s.eps;
        }
        AttnArgs at{};
        at.qkv = w.qkv; at.ld = w.ld_qkv; at.qn_w = L.qn; at.kn_w = L.kn; at.eps = s.eps;
        at.rope_cos = s.rope_cos; at.rope_sin = s.rope_sin;
        at.kpool = kpool + l * layer_stride; at.vpool = vpool + l * layer_stride;
        at.block_table = block_table; at.max_pages = max_pages; at.kv_len = kv_len; at.active = active;
        at.out = w.ao; at.outMB = MBL; at.n_heads = s.n_heads; at.n_kv = s.n_kv; at.B = B;
        at.fixed_len = fixed_len; at.identity_pages = fixed_len >= 0 ? 1 : 0;
        at.chunk = chunk; at.chunk_n_prompt = chunk_n_prompt; at.chunk_r_base = chunk_r_base;
        at.scale = powf(float(kHeadDim), -0.5f);  // Talker.swift:179
        at.nt_kv = ntkv;
        launch_gemm_skinny(q, counted());
        launch_attn_decode(at, counted());
        GemmArgs o = gemm_args(L.o, w.ao, M);
        o.epi = 3; o.y = w.h; o.yMB = MBL; o.resid = 1; o.ss_out = w.ss_b; o.nt_weights = ntw;
        launch_gemm_skinny(o, counted());
        if (!prologue_mlp) norm_into_xn(L.ln2, w.ss_b, tiles);
        GemmArgs g = gemm_args(L.gateup, prologue_mlp ? w.h : w.xn, M);
        g.epi = 2; g.y = w.act; g.yMB = MBL; g.nt_weights = ntw;
        if (prologue_mlp) {
            g.norm_w = L.ln2; g.ss_in = w.ss_b; g.ss_count = tiles; g.norm_dim = H; g.norm_eps = s.eps;
        }
        launch_gemm_skinny(g, counted());
        GemmArgs d = gemm_args(L.down, w.act, M);
        d.epi = 3; d.y = w.h; d.yMB = MBL; d.resid = 1; d.ss_out = w.ss_a; d.nt_weights = ntw;
        launch_gemm_skinny(d, counted());
    }
}

void Engine::enqueue_talker_step(int B, bool with_head) {
    (void)with_head;
    enqueue_layers(m_->talker, tk_, B, kpool_, vpool_, kv_layer_stride_, block_table_, max_pages_, kv_len_, active_, 1, -1, 1, nullptr, 0);
}

// One code-predictor pass (CodePredictor.swift:320-339 without the head). `from_talker`: the input is
// the talker's final-normed hidden state (step 0, first position); otherwise it is the embedding the
// previous sampler gathered (fragment-major in cp_x_ when a projection follows, else straight in cp_.h).
void Engine::enqueue_cp_pass(int B, bool from_talker, int head, int cp_pos, bool projected) {
    const TalkerConfig& t = m_->cfg.talker;
    const int H = t.hidden_size, CH = m_->cp.hidden, MBL = Mp_ / 16;
    int ss_count = 1;
    // The talker's final norm (Talker.swift:573) is always a row kernel, so that every way of scheduling step 0 (two
    // passes, one two-position pass) rounds it identically.
    auto talker_norm_into = [&](uint16_t* dst, float* ss_out) {
        NormRowsArgs n{};
        n.h = tk_.h; n.hMB = MBL; n.w = m_->talker.final_norm; n.eps = m_->talker.eps;
        n.out = dst; n.outMB = MBL; n.ss_out = ss_out; n.M = B; n.H = H;
        launch_norm_rows(n, counted());
    };
    if (m_->has_cp_proj && projected) {  // the sampler gathered an already projected row and its sums (build_cp_proj_tables)
        ss_count = CH / 16;
    } else if (m_->has_cp_proj) {  // small_to_mtp_projection (biased), CodePredictor.swift:327-330
        if (from_talker) talker_norm_into(cp_x2_, nullptr);  // cp_x_ already holds embed(code0) for the second position
        GemmArgs p = gemm_args(m_->cp_proj, from_talker ? cp_x2_ : cp_x_, B);
        p.epi = 3; p.y = cp_.h; p.yMB = MBL; p.resid = 0; p.ss_out = cp_.ss_a;
        launch_gemm_skinny(p, counted());
        ss_count = CH / 16;
    } else if (from_talker) {
        talker_norm_into(cp_.h, cp_.ss_a);
    }  // else: the sampler wrote cp_.h and cp_.ss_a[0] itself
    // every row's predictor cache holds cp_pos tokens at this point (cp_len_ advances in lock-step, finished rows included)
    enqueue_layers(m_->cp, cp_, B, cp_kpool_, cp_vpool_, cp_kv_layer_stride_, cp_block_table_, 1, cp_len_, nullptr, ss_count, cp_pos, 1, nullptr, 0);
}

// The end-of-frame job's operands (row_jobs.h frame_end_job). The resume of a row that waited for its text
// (launch_text_append_rows) forms the same input from the same operands.
FrameEndArgs Engine::frame_end_args(int B) const {
    const TalkerConfig& t = m_->cfg.talker;
    FrameEndArgs fe{};
    fe.cur_codes = cur_codes_; fe.codec_emb = m_->codec_emb; fe.cp_emb = m_->cp_emb_dev;
    fe.trailing = trailing_; fe.n_trailing = n_trailing_; fe.trailing_idx = trailing_idx_; fe.Tmax = Tcap_;
    fe.tts_pad = tts_pad_; fe.h = tk_.h; fe.hMB = Mp_ / 16; fe.ss_out = tk_.ss_a; fe.H = t.hidden_size; fe.B = B; fe.groups = t.num_code_groups;
    fe.n_frames = n_frames_; fe.max_frames = max_frames_; fe.finished = finished_; fe.active = active_; fe.cp_len = cp_len_;
    fe.text_open = frame_text_open_; fe.starved = frame_text_open_ ? starved_ : nullptr;  // (a session's open-text requests only)
    return fe;
}

void Engine::enqueue_frame(int B, const DebugOpts* dbg) {
    struct Count {  // launches of this frame step, for q3tts_timing (the same count whether captured or launched eagerly)
        Engine* e;
        int B;
        ~Count() { e->frame_launches_[B] = e->launches_; }
    } count{this, B};
    launches_ = 0;
    const TalkerConfig& t = m_->cfg.talker;
    const int H = t.hidden_size, V = t.vocab_size, Vc = t.cp.vocab_size, CH = t.cp.hidden_size;
    const int groups = t.num_code_groups, MBL = Mp_ / 16;
    stamp(0);
    enqueue_talker_step(B, true);
    stamp(1);
    // where the samplers put the next code-predictor input
    uint16_t* next_x = m_->has_cp_proj ? cp_x_ : cp_.h;
    float* next_ss = m_->has_cp_proj ? nullptr : cp_.ss_a;
    // Predictor step 0 takes two positions, [talker hidden, embed(code0)] (Qwen3.swift:884-887). When 2 * B rows fit the
    // activation buffers they go through the stack together (rows 0..B-1 and B..2B-1, chunk attention), which saves a
    // whole pass of launches per frame; otherwise they are two passes.
    const bool pair = 2 * B <= Mp_;
    {   // final norm (prologue) + codec_head (Talker.swift:573, 644)
        GemmArgs hd = gemm_args(m_->codec_head, tk_.h, B);
        hd.epi = 0; hd.y = tk_.logits; hd.ldy = tk_.ld_logits;
        hd.norm_w = m_->talker.final_norm; hd.ss_in = tk_.ss_a; hd.ss_count = H / 16; hd.norm_dim = H; hd.norm_eps = m_->talker.eps;
        bool rode = false;
        if (pair) {
            // the predictor's first position -- the talker's final-normed hidden state (Talker.swift:573), materialised next to
            // the embedding -- reads what this GEMM reads: B extra workgroups of its launch instead of a launch of its own
            NormRowsArgs n{};
            n.h = tk_.h; n.hMB = MBL; n.w = m_->talker.final_norm; n.eps = m_->talker.eps;
            n.out = next_x; n.outMB = MBL; n.ss_out = next_ss; n.M = B; n.H = H;
            rode = launch_gemm_skinny_with_norm_rows(hd, n, st_);
            if (rode) ++launches_;  // one launch, counted only when it was made
            else launch_norm_rows(n, counted());
        }
        if (!rode) launch_gemm_skinny(hd, counted());
    }
    SamplerArgs sa{};
    sa.logits = tk_.logits; sa.ldl = tk_.ld_logits; sa.V = V; sa.sp = sp_dev_; sa.is_talker = 1;
    sa.suppress_lo = V - 1024; sa.suppress_hi = V; sa.eos_id = t.codec_eos_token_id;  // Qwen3.swift:829-835
    sa.seen = seen_; sa.cb = 0; sa.n_frames = n_frames_; sa.max_frames = max_frames_;
    sa.finished = finished_; sa.active = active_; sa.kv_len = kv_len_; sa.advance = 1; sa.advance_gate = active_;
    sa.cur_codes = cur_codes_; sa.codes = codes_; sa.Fmax = Fcap_;
    sa.forced = dbg ? forced_dev_ : nullptr; sa.forced_frames = dbg ? dbg->frames : 0;
    sa.sampled = dbg ? sampled_dev_ : nullptr;
    sa.emb = m_->codec_emb; sa.emb_ld = H; sa.next_MB = MBL; sa.H = H; sa.B = B;
    if (pair) {  // embed(code0) goes straight to the second row block of the pass input
        sa.next_x = next_x; sa.next_row0 = B; sa.next_ss = next_ss ? next_ss + B : nullptr;
    } else {
        // Without a projection a pass takes its input in cp_.h, which the first position (the talker hidden state) still
        // needs: stage the embedding in cp_x2_
        sa.next_x = m_->has_cp_proj ? cp_x_ : cp_x2_; sa.next_ss = m_->has_cp_proj ? nullptr : cp_ss2_;
    }
    sa.logits_dump = (dbg && dbg->talker_logits) ? tl_dump_ : nullptr; sa.dump_ld = V; sa.dump_off = 0;
    sa.row_key = frame_row_key_;
    if (pair) {
        launch_sampler(sa, counted());
        int ss_count = 1;
        if (m_->has_cp_proj) {  // small_to_mtp_projection over both positions (CodePredictor.swift:327-330)
            GemmArgs p = gemm_args(m_->cp_proj, cp_x_, 2 * B);
            p.epi = 3; p.y = cp_.h; p.yMB = MBL; p.resid = 0; p.ss_out = cp_.ss_a;
            launch_gemm_skinny(p, counted());
            ss_count = CH / 16;
        }
        stamp(2);
        enqueue_layers(m_->cp, cp_, B, cp_kpool_, cp_vpool_, cp_kv_layer_stride_, cp_block_table_, 1, cp_len_, nullptr, ss_count, 0, 2,
                       nullptr, 0);
        stamp(3);  // (no launch for cp_len_: the predictor's attention takes its cache length from the pass index, fixed_len)
    } else {
        launch_sampler(sa, counted());
        // code predictor, step 0 = [hidden, embed(code0)] run as two positions
        enqueue_cp_pass(B, true, -1, 0);
        if (!m_->has_cp_proj) {  // second position: move the staged embedding (and its sum of squares) into place
            launch_copy_rows(cp_x2_, 0, cp_.h, 0, 1, Mp_ * H, counted());
            launch_copy_rows(reinterpret_cast<const uint16_t*>(cp_ss2_), 0, reinterpret_cast<uint16_t*>(cp_.ss_a), 0, 1, Mp_ * 2, counted());
        }
    }
    const FrameEndArgs fe = frame_end_args(B);
    bool fe_done = false;
    for (int i = 0; i < groups - 1; ++i) {
        const bool second_of_pair = pair && i == 0;  // its stack forward already ran above; rows B..2B-1 hold it
        const int Mh = second_of_pair ? 2 * B : B;
        if (!second_of_pair) {
            enqueue_cp_pass(B, false, i, i + 1, cp_tables_ && i >= 1);
            stamp(5);
        }
        {
            GemmArgs lh = gemm_args(m_->lm_head[size_t(i)], cp_.h, Mh);
            lh.epi = 0; lh.y = cp_.logits; lh.ldy = cp_.ld_logits;
            lh.norm_w = m_->cp.final_norm; lh.ss_in = cp_.ss_a; lh.ss_count = CH / 16; lh.norm_dim = CH; lh.norm_eps = m_->cp.eps;
            launch_gemm_skinny(lh, counted());
        }
        SamplerArgs sc{};
        sc.logits = cp_.logits + (second_of_pair ? size_t(B) * cp_.ld_logits : 0); sc.ldl = cp_.ld_logits; sc.V = Vc; sc.sp = sp_dev_;
        sc.is_talker = 0;
        sc.eos_id = -1; sc.cb = i + 1; sc.n_frames = n_frames_; sc.max_frames = max_frames_;
        sc.finished = finished_; sc.active = active_; sc.kv_len = cp_len_; sc.advance = 1; sc.advance_gate = nullptr;
        sc.cur_codes = cur_codes_; sc.codes = codes_; sc.Fmax = Fcap_;
        sc.forced = dbg ? forced_dev_ : nullptr; sc.forced_frames = dbg ? dbg->frames : 0;
        sc.sampled = dbg ? sampled_dev_ : nullptr;
        if (i + 1 < groups - 1) {  // embedding of this code feeds the next pass (Qwen3.swift:889-892)
            sc.emb = m_->cp_emb[size_t(i)]; sc.emb_ld = H; sc.next_x = next_x; sc.next_MB = MBL; sc.next_ss = next_ss;
        }
        sc.H = H; sc.B = B;
        if (cp_tables_ && i + 1 < groups - 1) {  // projected row + its per-tile sums straight into the next pass's input
            sc.emb = m_->cp_pe[size_t(i)]; sc.emb_ld = CH; sc.H = CH; sc.next_x = cp_.h;
            sc.emb_ss = m_->cp_pss[size_t(i)]; sc.nss = CH / 16; sc.next_ss = cp_.ss_a; sc.next_ss_ld = Mp_;
        }
        sc.logits_dump = (dbg && dbg->cp_logits) ? cl_dump_ : nullptr; sc.dump_ld = (groups - 1) * Vc; sc.dump_off = i * Vc;
        sc.row_key = frame_row_key_;
        if (i == groups - 2 && Vc <= 2048) {  // the frame's last draw carries its row's end-of-frame job (Qwen3.swift:919-935; row_jobs.h)
            launch_sampler_with_frame_end(sc, fe, counted());
            fe_done = true;
        } else {
            launch_sampler(sc, counted());
        }
        stamp(second_of_pair ? 4 : 6);
    }
    if (!fe_done) launch_frame_end(fe, counted());
    stamp(7);
}

hipGraphExec_t Engine::frame_graph(int B) {
    // a queued frame step keys its samplers on row_key_ (frame_row_key_ set): a capture of its own
    // (and a session's, whose frame end reads text_open_, another one: the closed queue's step stays exactly what it was)
    std::map<int, hipGraphExec_t>& graphs = frame_text_open_ ? ographs_ : frame_row_key_ ? qgraphs_ : graphs_;
    auto it = graphs.find(B);
    if (it != graphs.end()) return it->second;
    hipGraph_t g = nullptr;
    Q3_HIP(hipStreamBeginCapture(st_, hipStreamCaptureModeThreadLocal));
    try {
        enqueue_frame(B, nullptr);
    } catch (...) {
        (void)hipStreamEndCapture(st_, &g);
        if (g) (void)hipGraphDestroy(g);
        throw;
    }
    Q3_HIP(hipStreamEndCapture(st_, &g));
    hipGraphExec_t ge = nullptr;
    Q3_HIP(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
    Q3_HIP(hipGraphDestroy(g));
    graphs[B] = ge;
    return ge;
}

// ------------------------------------------------------------------------------------------------
// request resolution: routing and validation of generate() (Qwen3.swift:1291-1373, 803-811, 303-319)
// ------------------------------------------------------------------------------------------------
void Engine::check_reference(const float* ref_audio, int64_t n_ref_samples, const int32_t* ref_text_ids, int n_ref_text_ids) const {
    Q3_CHECK(m_->has_codec, 1, "Model not initialized: Speech tokenizer not loaded");  // Qwen3.swift:1029-1031
    Q3_CHECK(m_->has_codec_encoder, 1,
             "Model not initialized: Voice cloning (ICL mode) requires the speech tokenizer encoder. Make sure to load a model "
             "with encoder weights.");  // :1033-1038
    Q3_CHECK(ref_audio && n_ref_samples > 0, 3, "Invalid input: reference audio is empty");
    {   // a NaN sample would spread through the encoders into every logit of the row
        bool finite = true;
        for (int64_t i = 0; i < n_ref_samples; ++i) finite = finite && (std::fabs(ref_audio[i]) <= 3.0e38f);
        Q3_CHECK(finite, 3, "Invalid input: reference audio holds non-finite samples");
    }
    Q3_CHECK(ref_text_ids && n_ref_text_ids >= 5, 3, "Invalid input: ref_text_ids must hold the chat-template tokens");
}

ResolvedRequest Engine::resolve(const q3tts_request& r, const q3tts_sampling& sp, const Voice* voice) const {
    const ModelConfig& cfg = m_->cfg;
    const TalkerConfig& t = cfg.talker;
    ResolvedRequest o;
    if (r.speed != 0.0f) {  // (a NaN is not 0 and fails the range below)
        Q3_CHECK(codec_ && codec_->request_speeds(), 3,
                 "Invalid input: q3tts_request.speed needs a handle loaded with q3tts_load_opts.request_speeds");
        const int hs = codec_->speed_plan().hs_of(r.speed);
        Q3_CHECK(hs != 0, 3, "Invalid input: q3tts_request.speed must be 0 (the handle's speed) or between 0.5 and 2.0");
        if (hs != codec_->stretch_hs()) {
            // streamed audio: the slotted stream has a hop per row. Not built: the chunked exact decode (audio_window_frames == 0)
            // and streams on a handle with an output rate (the resampler's input margin would have a frame size per row)
            Q3_CHECK(sp.audio_chunk_frames == 0 || (sp.audio_window_frames > 0 && codec_->stream_own_hops()), 3,
                     "Invalid input: a request speed other than the handle's with audio_chunk_frames > 0 needs audio_window_frames > 0 "
                     "(streamed audio) and a handle without output_sample_rate");
            o.hs = hs;
        }
    }
    Q3_CHECK(r.text_ids && r.n_text_ids >= 4, 3, "Invalid input: text_ids must hold the chat-template tokens");
    Q3_CHECK(r.route >= 0 && r.route <= 2, 3, "Invalid input: unknown q3tts_request.route");
    o.text_ids.assign(r.text_ids, r.text_ids + r.n_text_ids);
    const bool have_instruct = r.instruct_ids && r.n_instruct_ids > 0;
    const std::string type = cfg.tts_model_type;
    auto speaker_list = [&]() {
        std::string s;
        for (size_t i = 0; i < speakers.size(); ++i) s += (i ? ", " : "") + speakers[i];
        return s;
    };
    bool use_speaker = false, use_instruct = false;
    if (r.ref_audio != nullptr || voice) {  // generateVoiceClone (Qwen3.swift:1009-1046): no routing by model type, no speaker/instruct
        if (!voice) check_reference(r.ref_audio, r.n_ref_samples, r.ref_text_ids, r.n_ref_text_ids);  // (a voice passed them when it was made)
        Q3_CHECK(r.n_text_ids >= 8, 3, "Invalid input: text_ids must hold the chat-template tokens");
        Q3_CHECK(m_->codec_enc.bins <= t.vocab_size && m_->codec_enc.bins <= t.cp.vocab_size, 3,
                 "Invalid input: encoder codebook larger than the codec embedding tables");
        o.clone = true;
        if (voice) {
            o.voice = voice;
            o.ref_T = voice->ref_T;
            o.n_ref_samples = voice->n_ref_samples;
            o.ref_text_ids = voice->ref_text_ids;
        } else {
            o.ref_audio = r.ref_audio;
            o.n_ref_samples = r.n_ref_samples;
            o.ref_text_ids.assign(r.ref_text_ids, r.ref_text_ids + r.n_ref_text_ids);
        }
        const std::string lang = lower(r.language ? r.language : "auto");
        if (lang != "auto") {  // :515-519 (no dialect override on this path)
            auto it = t.codec_language_id.find(lang);
            if (it != t.codec_language_id.end()) o.language_id = it->second;
        }
        o.target_token_count = r.target_token_count;
        const int mt = r.max_tokens > 0 ? r.max_tokens : 2048;
        o.max_frames = sp.force_frames > 0 ? sp.force_frames : int(std::min<int64_t>(mt, std::max<int64_t>(75, int64_t(r.target_token_count) * 6)));  // :1051-1052
        for (int id : o.text_ids) Q3_CHECK(id >= 0 && id < t.text_vocab_size, 3, "Invalid input: text token id out of range");
        for (int id : o.ref_text_ids) Q3_CHECK(id >= 0 && id < t.text_vocab_size, 3, "Invalid input: reference text token id out of range");
        return o;
    }
    if (r.route == 1) {         // generateVoiceDesign(text:language:instruct:...) on any checkpoint (Qwen3.swift:587-620)
        use_instruct = true;
    } else if (r.route == 2) {  // generateCustomVoice(text:speaker:language:instruct:...) on any checkpoint (:783-811)
        Q3_CHECK(r.speaker != nullptr, 3, "Invalid input: generateCustomVoice requires 'speaker'");
        use_speaker = true;
        use_instruct = true;
    } else if (type == "custom_voice" || type == "base") {
        const char* nm = type == "custom_voice" ? "CustomVoice" : "Base";
        Q3_CHECK(r.speaker != nullptr, 3,
                 std::string("Invalid input: ") + nm + " model requires 'speaker' (e.g., 'Vivian', 'Ryan'). Available speakers: " + speaker_list());
        use_speaker = true;
        use_instruct = (type == "custom_voice");  // Base ignores instruct (Qwen3.swift:1352)
    } else {  // voice_design and unknown types (Qwen3.swift:1360-1371)
        if (type == "voice_design")
            Q3_CHECK(have_instruct, 3,
                     "Invalid input: VoiceDesign model requires 'instruct' to describe the voice (e.g., 'A cheerful young female voice with high pitch')");
        use_instruct = true;
    }
    if (use_speaker) {  // Qwen3.swift:803-811
        Q3_CHECK(t.has_spk_id, 3, "Invalid input: This model does not support CustomVoice. No speakers defined.");
        auto it = t.spk_id.find(lower(r.speaker));
        Q3_CHECK(it != t.spk_id.end(), 3,
                 std::string("Invalid input: Speaker '") + r.speaker + "' not found. Available speakers: " + speaker_list());
        o.speaker_token = it->second;
    }
    if (use_instruct && have_instruct) o.instruct_ids.assign(r.instruct_ids, r.instruct_ids + r.n_instruct_ids);
    const std::string lang = lower(r.language ? r.language : "auto");
    if (lang != "auto") {  // Qwen3.swift:304-308 (unknown names silently mean "no language")
        auto it = t.codec_language_id.find(lang);
        if (it != t.codec_language_id.end()) o.language_id = it->second;
    }
    if ((lang == "chinese" || lang == "auto") && use_speaker) {  // dialect override, Qwen3.swift:311-319
        auto d = t.spk_dialect.find(lower(r.speaker));
        if (d != t.spk_dialect.end()) {
            auto it = t.codec_language_id.find(d->second);
            if (it != t.codec_language_id.end()) o.language_id = it->second;
        }
    }
    o.target_token_count = r.target_token_count;
    const int mt = r.max_tokens > 0 ? r.max_tokens : 2048;
    o.max_frames = sp.force_frames > 0 ? sp.force_frames : int(std::min<int64_t>(mt, std::max<int64_t>(75, int64_t(r.target_token_count) * 6)));  // :822-823
    for (int id : o.text_ids) Q3_CHECK(id >= 0 && id < t.text_vocab_size, 3, "Invalid input: text token id out of range");
    for (int id : o.instruct_ids) Q3_CHECK(id >= 0 && id < t.text_vocab_size, 3, "Invalid input: instruct token id out of range");
    return o;
}

// ids -> text_projection(embedText(ids)) (Talker.swift:627-633, 475-487), 64 rows per GEMM pass
void Engine::project_rows(const std::vector<int32_t>& ids, int rows) {
    const TalkerConfig& t = m_->cfg.talker;
    const int TH = t.text_hidden_size, H = t.hidden_size;
    Q3_CHECK(rows <= proj_cap_, 3, "Invalid input: prompt too long for the configured max_prompt");
    Q3_HIP(hipMemcpyAsync(ids_dev_, ids.data(), size_t(rows) * 4, hipMemcpyHostToDevice, st_));
    for (int r0 = 0; r0 < rows; r0 += 64) {
        const int n = std::min(64, rows - r0);
        launch_gather_rows(m_->text_emb, TH, ids_dev_ + r0, m_->token_map, n, TH, proj_in_, TH, 4, st_);
        GemmArgs f1 = gemm_args(m_->fc1, proj_in_, n);
        f1.xMB = 4; f1.epi = 0; f1.y = proj_mid_; f1.y_tiled = 1; f1.yMB = 4; f1.act_silu = 1;
        launch_gemm_skinny(f1, st_);
        GemmArgs f2 = gemm_args(m_->fc2, proj_mid_, n);
        f2.xMB = 4; f2.epi = 0; f2.y = proj_out_ + size_t(r0) * H; f2.ldy = H;
        launch_gemm_skinny(f2, st_);
    }
}

void Engine::assemble_prompts(const std::vector<ResolvedRequest>& reqs, std::vector<int>& n_prompt, std::vector<int>& n_trailing,
                              const std::vector<int>* trailing_rows) {
    const ModelConfig& cfg = m_->cfg;
    const TalkerConfig& t = cfg.talker;
    const int H = t.hidden_size;
    const int n = int(reqs.size());
    std::vector<int32_t> ids;
    std::vector<int> text_off((size_t)(n)), instr_off((size_t)(n)), tts_off((size_t)(n));
    for (int b = 0; b < n; ++b) {
        const auto& r = reqs[size_t(b)];
        text_off[size_t(b)] = int(ids.size());
        ids.insert(ids.end(), r.text_ids.begin(), r.text_ids.end());
        instr_off[size_t(b)] = int(ids.size());  // doubles as the reference-text offset of voice-clone rows
        ids.insert(ids.end(), r.instruct_ids.begin(), r.instruct_ids.end());
        ids.insert(ids.end(), r.ref_text_ids.begin(), r.ref_text_ids.end());
        tts_off[size_t(b)] = int(ids.size());
        ids.push_back(cfg.tts_bos_token_id);  // Qwen3.swift:282-292
        ids.push_back(cfg.tts_eos_token_id);
        ids.push_back(cfg.tts_pad_token_id);
    }
    project_rows(ids, int(ids.size()));
    std::vector<int32_t> pa, pb, pd, ta, tb, td;  // (proj row, codec id or -1, destination row)
    n_prompt.assign(size_t(n), 0);
    n_trailing.assign(size_t(n), 0);
    for (int b = 0; b < n; ++b) {
        const auto& r = reqs[size_t(b)];
        const int trow = trailing_rows ? (*trailing_rows)[size_t(b)] : b;
        const int bos = tts_off[size_t(b)], eos = bos + 1, pad = bos + 2;
        std::vector<int> cp_ids;  // codec prefix, Qwen3.swift:322-359 / 527-561
        if (r.language_id < 0) cp_ids = {t.codec_nothink_id, t.codec_think_bos_id, t.codec_think_eos_id};
        else cp_ids = {t.codec_think_id, t.codec_think_bos_id, r.language_id, t.codec_think_eos_id};
        if (r.speaker_token >= 0) cp_ids.push_back(r.speaker_token);
        if (r.clone && m_->has_speaker_encoder) cp_ids.push_back(-2 - r.extra_base);  // x-vector row (:553-558)
        cp_ids.push_back(t.codec_pad_id);
        cp_ids.push_back(t.codec_bos_id);
        for (int id : cp_ids) Q3_CHECK(id < t.vocab_size && id != -1, 3, "Invalid input: codec prefix id out of range");
        const int nc = int(cp_ids.size());
        int p = 0;
        auto push = [&](int a, int c) {
            Q3_CHECK(p < Pcap_, 3, "Invalid input: prompt longer than max_prompt");
            pa.push_back(a);
            pb.push_back(c);
            pd.push_back(b * Pcap_ + p);
            ++p;
        };
        if (r.clone) {  // prepareICLGenerationInputs (Qwen3.swift:418-582)
            const int tl = int(r.text_ids.size()), rl = int(r.ref_text_ids.size()), ro = instr_off[size_t(b)];
            for (int i = 0; i < 3; ++i) push(text_off[size_t(b)] + i, -1);                     // role, :564-566
            for (int i = 0; i < nc - 1; ++i) push(i < nc - 2 ? pad : bos, cp_ids[size_t(i)]);  // :569-573
            for (int i = 3; i < rl - 2; ++i) push(ro + i, t.codec_pad_id);                     // reference text, :451, :505-506
            for (int i = 3; i < tl - 5; ++i) push(text_off[size_t(b)] + i, t.codec_pad_id);    // target text, :457
            push(eos, t.codec_pad_id);                                                         // :476
            push(pad, t.codec_bos_id);                                                         // :494-496, :509-510
            for (int f = 0; f < r.ref_T; ++f) push(pad, -2 - (r.extra_base + 1 + f));
            n_prompt[size_t(b)] = p;
            ta.push_back(pad);  // trailing text is just tts_pad (:579)
            tb.push_back(-1);
            td.push_back(trow * Tcap_);
            n_trailing[size_t(b)] = 1;
            continue;
        }
        for (int i = 0; i < int(r.instruct_ids.size()); ++i) push(instr_off[size_t(b)] + i, -1);  // :383-384
        for (int i = 0; i < 3; ++i) push(text_off[size_t(b)] + i, -1);                            // role, :371
        for (int i = 0; i < nc - 1; ++i) push(i < nc - 2 ? pad : bos, cp_ids[size_t(i)]);         // :375-379
        push(text_off[size_t(b)] + 3, cp_ids[size_t(nc - 1)]);                                    // :390
        Q3_CHECK(p <= Pcap_, 3, "Invalid input: prompt longer than max_prompt");
        n_prompt[size_t(b)] = p;
        const int tl = int(r.text_ids.size());
        int q = 0;
        auto pusht = [&](int a) {
            ta.push_back(a);
            tb.push_back(-1);
            td.push_back(trow * Tcap_ + q);
            ++q;
        };
        // (an open-text request carries no tail, n_tail = 0; while its text is open the tts_eos row is not there yet)
        if (tl - r.n_tail > 4)  // Qwen3.swift:394-406
            for (int i = 4; i < tl - r.n_tail; ++i) pusht(text_off[size_t(b)] + i);
        if (!r.text_open) pusht(eos);
        Q3_CHECK(q <= Tcap_, 3, "Invalid input: text longer than max_prompt");
        n_trailing[size_t(b)] = q;
    }
    auto run = [&](std::vector<int32_t>& a, std::vector<int32_t>& bb, std::vector<int32_t>& d, uint16_t* dst) {
        const size_t k = a.size();
        int32_t* da = compose_a_;
        int32_t* db = compose_a_ + k;
        int32_t* dd = compose_a_ + 2 * k;
        Q3_HIP(hipMemcpyAsync(da, a.data(), k * 4, hipMemcpyHostToDevice, st_));
        Q3_HIP(hipMemcpyAsync(db, bb.data(), k * 4, hipMemcpyHostToDevice, st_));
        Q3_HIP(hipMemcpyAsync(dd, d.data(), k * 4, hipMemcpyHostToDevice, st_));
        launch_compose_rows(proj_out_, H, m_->codec_emb, H, extra_, H, da, db, dd, dst, H, int(k), H, st_);
        Q3_HIP(hipStreamSynchronize(st_));  // host vectors are reused by the next call
    };
    run(pa, pb, pd, prompt_);
    run(ta, tb, td, trailing_);
    launch_copy_rows(proj_out_ + size_t(tts_off[0] + 2) * H, H, tts_pad_, H, 1, H, st_);
}

const float* Engine::upload_audio(const float* audio, int64_t n) {
    if (size_t(n) > ref_audio_dev_.capacity()) {
        Q3_HIP(hipStreamSynchronize(st_));
        ref_audio_dev_.grow(size_t(n));
    }
    Q3_HIP(hipMemcpyAsync(ref_audio_dev_, audio, size_t(n) * 4, hipMemcpyHostToDevice, st_));
    return ref_audio_dev_;
}

// Steps 1, 5 and 8 of prepareICLGenerationInputs (Qwen3.swift:436-444, 479-491, 521-525) for every voice-clone row:
// reference codes, the per-frame sums of their 16 embeddings and the speaker x-vector, all left on the device.
// A row whose reference is a voice skips all of it: its prompt rows and code rows are copied from the voice, device to device.
bool Engine::prepare_clone_rows(std::vector<ResolvedRequest>& reqs) {
    const int H = m_->cfg.talker.hidden_size;
    int n_clone = 0;  // rows that carry a waveform
    for (auto& r : reqs) n_clone += (r.clone && !r.voice) ? 1 : 0;
    Q3_CHECK(n_clone == 0 || fe_ != nullptr, 1, "Model not initialized: Speech tokenizer encoder not available");
    size_t total_codes = 0, total_rows = 0;
    for (auto& r : reqs) {
        if (!r.clone) continue;
        r.ref_T = r.voice ? r.voice->ref_T : fe_->encoded_frames(r.n_ref_samples);
        r.ref_off = int(total_codes);
        r.extra_base = int(total_rows);
        total_codes += size_t(16) * r.ref_T;
        total_rows += size_t(1) + r.ref_T;
    }
    ref_codes_dev_.grow(total_codes);
    extra_.grow(total_rows * H);
    for (auto& r : reqs) {
        if (!r.voice) continue;
        Q3_HIP(hipMemcpyAsync(extra_ + size_t(r.extra_base) * H, r.voice->rows_dev, size_t(1 + r.ref_T) * H * 2, hipMemcpyDeviceToDevice, st_));
        Q3_HIP(hipMemcpyAsync(ref_codes_dev_ + r.ref_off, r.voice->codes_dev, size_t(16) * r.ref_T * 4, hipMemcpyDeviceToDevice, st_));
    }
    if (n_clone == 0) return false;  // nothing to encode: the front-end lanes are neither created nor touched
    const int K = std::min(4, n_clone);
    while (int(fe_lanes_.size()) < K) {
        FeLane L;
        Q3_HIP(hipStreamCreateWithFlags(&L.st, hipStreamNonBlocking));
        Q3_HIP(hipEventCreateWithFlags(&L.done, hipEventDisableTiming));
        L.fe = std::make_unique<VoiceFrontEnd>(*m_, L.st);
        L.spk.grow(size_t(H));
        fe_lanes_.push_back(std::move(L));
    }
    // every clip zero-padded to the longest one: the (causal) codec encoder then runs ONCE over all of them
    int64_t S_max = 0;
    for (auto& r : reqs)
        if (r.clone && !r.voice) S_max = std::max<int64_t>(S_max, r.n_ref_samples);
    if (size_t(S_max) * n_clone > ref_audio_dev_.capacity()) {
        Q3_HIP(hipStreamSynchronize(st_));
        ref_audio_dev_.grow(size_t(S_max) * n_clone);
    }
    Q3_HIP(hipMemsetAsync(ref_audio_dev_, 0, size_t(S_max) * n_clone * 4, st_));
    std::vector<int64_t> valid, offs;  // samples per clip, offset of its codes
    int i = 0;
    for (auto& r : reqs) {
        if (!r.clone || r.voice) continue;
        Q3_HIP(hipMemcpyAsync(ref_audio_dev_ + size_t(i) * S_max, r.ref_audio, size_t(r.n_ref_samples) * 4, hipMemcpyHostToDevice, st_));
        valid.push_back(r.n_ref_samples);
        offs.push_back(r.ref_off);
        ++i;
    }
    Q3_HIP(hipEventRecord(fe_uploaded_, st_));
    // speaker x-vectors: not causal (reflect padding, statistics over the whole clip), so one clip at a time, a few side by side
    if (m_->has_speaker_encoder) {
        i = 0;
        for (auto& r : reqs) {
            if (!r.clone || r.voice) continue;
            FeLane& L = fe_lanes_[size_t(i % K)];
            if (i < K) Q3_HIP(hipStreamWaitEvent(L.st, fe_uploaded_, 0));
            // The x-vector is fp32; it enters the prompt in the talker's storage dtype like every other row
            // (the reference's MLX concat would instead promote the prompt to fp32).
            L.fe->speaker_embedding(ref_audio_dev_ + size_t(i) * S_max, r.n_ref_samples, L.spk);
            launch_f32_to_bf16(L.spk, extra_ + size_t(r.extra_base) * H, H, L.st);
            ++i;
        }
    }
    const size_t per_clip = size_t(S_max) * 64 * 4 * 3 + (size_t(1) << 20);  // rough scratch per clip (bytes)
    const int rows_per_pass = int(std::max<size_t>(1, std::min<size_t>(VoiceFrontEnd::kMaxClips, (size_t(16) << 30) / per_clip)));
    for (int lo = 0; lo < n_clone; lo += rows_per_pass) {
        const int nb = std::min(rows_per_pass, n_clone - lo);
        fe_->encode_batch(ref_audio_dev_ + size_t(lo) * S_max, nb, S_max, valid.data() + lo, offs.data() + lo, ref_codes_dev_);
    }
    for (auto& r : reqs) {
        if (!r.clone || r.voice) continue;
        launch_ref_embed_rows(ref_codes_dev_ + r.ref_off, r.ref_T, 16, m_->codec_emb, m_->cp_emb_dev, H,
                              extra_ + size_t(r.extra_base + 1) * H, H, st_);
    }
    if (m_->has_speaker_encoder)
        for (int k = 0; k < K; ++k) {  // the prompt assembly on st_ follows every lane
            Q3_HIP(hipEventRecord(fe_lanes_[size_t(k)].done, fe_lanes_[size_t(k)].st));
            Q3_HIP(hipStreamWaitEvent(st_, fe_lanes_[size_t(k)].done, 0));
        }
    return true;
}

int Engine::encoded_frames(int64_t n_samples) const {
    return (fe_ && m_->has_codec_encoder) ? fe_->encoded_frames(n_samples) : 0;
}

int Engine::codec_encode(const float* audio, int64_t n_samples, int32_t* codes, int cap_frames) {
    Q3_CHECK(fe_ && m_->has_codec_encoder, 1, "Model not initialized: Speech tokenizer encoder not available");
    Q3_CHECK(audio && n_samples > 0, 3, "Invalid input: empty audio");
    const int T = fe_->encoded_frames(n_samples);
    Q3_CHECK(T <= cap_frames, 3, "Invalid input: output buffer too small for the encoded frames");
    ref_codes_dev_.grow(size_t(16) * T);
    const float* a = upload_audio(audio, n_samples);
    Q3_HIP(hipEventRecord(ev_fe_[0], st_));
    fe_->encode(a, n_samples, ref_codes_dev_);
    Q3_HIP(hipEventRecord(ev_fe_[1], st_));
    Q3_HIP(hipStreamSynchronize(st_));
    Q3_HIP(hipMemcpy(codes, ref_codes_dev_, size_t(16) * T * 4, hipMemcpyDeviceToHost));
    float ms = 0;
    Q3_HIP(hipEventElapsedTime(&ms, ev_fe_[0], ev_fe_[1]));
    timing = q3tts_timing{};
    timing.frontend_ms = ms;
    return T;
}

void Engine::speaker_embedding(const float* audio, int64_t n_samples, float* out, int cap) {
    Q3_CHECK(fe_ && m_->has_speaker_encoder, 1, "Model not initialized: Speaker encoder not available for this model");
    Q3_CHECK(audio && n_samples > 0, 3, "Invalid input: empty audio");
    const int D = m_->speaker.enc_dim;
    Q3_CHECK(cap >= D, 3, "Invalid input: output buffer too small for the speaker embedding");
    spk_f32_.grow(size_t(m_->cfg.talker.hidden_size));
    const float* a = upload_audio(audio, n_samples);
    Q3_HIP(hipEventRecord(ev_fe_[0], st_));
    fe_->speaker_embedding(a, n_samples, spk_f32_);
    Q3_HIP(hipEventRecord(ev_fe_[1], st_));
    Q3_HIP(hipStreamSynchronize(st_));
    Q3_HIP(hipMemcpy(out, spk_f32_, size_t(D) * 4, hipMemcpyDeviceToHost));
    float ms = 0;
    Q3_HIP(hipEventElapsedTime(&ms, ev_fe_[0], ev_fe_[1]));
    timing = q3tts_timing{};
    timing.frontend_ms = ms;
}

const Engine::ResamplerDev& Engine::resampler(int in_rate, int out_rate) {
    Q3_CHECK(resample_pair_supported(in_rate, out_rate), 3,
             "Invalid input: unsupported sample-rate pair (one rate must be 24000, the other 8000, 12000, 16000, 22050, 32000, 44100 or 48000)");
    for (const auto& r : resamplers_)
        if (r->plan.in_rate == in_rate && r->plan.out_rate == out_rate) return *r;
    auto r = std::make_unique<ResamplerDev>();
    r->plan = make_resample_plan(in_rate, out_rate);
    const size_t n = align_up(r->plan.tab.size(), 4);
    std::vector<float> padded(n, 0.0f);
    std::copy(r->plan.tab.begin(), r->plan.tab.end(), padded.begin());
    Q3_HIP(hipMemcpy(r->tab.grow(n), padded.data(), n * 4, hipMemcpyHostToDevice));
    resamplers_.push_back(std::move(r));
    return *resamplers_.back();
}

const float* Engine::resample_upload(const float* audio, int64_t n, int in_rate, int out_rate, bool centred, int64_t* n_out) {
    const ResamplerDev& r = resampler(in_rate, out_rate);
    Q3_CHECK(audio && n > 0 && n <= (int64_t(1) << 28), 3, "Invalid input: resampling takes between 1 and 2^28 samples");
    const int64_t no = r.plan.out_len(n);
    const float* a = upload_audio(audio, n);
    if (size_t(no) > rs_out_dev_.capacity()) Q3_HIP(hipStreamSynchronize(st_));  // the old buffer may still be read
    rs_out_dev_.grow(size_t(no));
    rs_len_dev_.grow(1);
    const int32_t len = int32_t(n);
    Q3_HIP(hipStreamSynchronize(st_));  // `len` is pageable stack memory, and the device word may still feed an earlier launch
    Q3_HIP(hipMemcpy(rs_len_dev_, &len, 4, hipMemcpyHostToDevice));
    ResampleArgs ra{};
    ra.x = a; ra.x_bstride = 0;
    ra.y = rs_out_dev_; ra.y_bstride = 0;
    ra.len = rs_len_dev_; ra.len_mul = 1; ra.max_in = n;
    ra.tab = r.tab; ra.L = r.plan.L; ra.M = r.plan.M; ra.K = r.plan.K;
    ra.hist = 0; ra.centred = centred ? 1 : 0; ra.clamp = 0; ra.B = 1;
    launch_resample(ra, st_);
    *n_out = no;
    return rs_out_dev_;
}

void Engine::resample(const float* in, int64_t n_in, int in_rate, int out_rate, bool centred, float* out, int64_t cap, int64_t* n_out) {
    const ResamplerDev& r = resampler(in_rate, out_rate);  // (the pair is refused first, whatever else is wrong)
    Q3_CHECK(in && out && n_out && n_in > 0, 3, "Invalid input: empty audio");
    Q3_CHECK(n_in <= (int64_t(1) << 28), 3, "Invalid input: resampling takes between 1 and 2^28 samples");
    const int64_t no = r.plan.out_len(n_in);
    *n_out = no;
    Q3_CHECK(cap >= no, 3, "Invalid input: output buffer too small for the resampled audio");
    bool finite = true;
    for (int64_t i = 0; i < n_in; ++i) finite = finite && (std::fabs(in[i]) <= 3.0e38f);
    Q3_CHECK(finite, 3, "Invalid input: audio holds non-finite samples");
    int64_t got = 0;
    const float* y = resample_upload(in, n_in, in_rate, out_rate, centred, &got);
    Q3_HIP(hipStreamSynchronize(st_));
    Q3_HIP(hipMemcpy(out, y, size_t(got) * 4, hipMemcpyDeviceToHost));
}

void Engine::time_stretch(const float* in, int64_t n_in, float speed, bool causal, float* out, int64_t cap, int64_t* n_out) {
    // (the speed is refused first, whatever else is wrong, and before any GPU work)
    const int hs = stretch_choose_hs(double(speed));
    Q3_CHECK(hs != 0, 3, "Invalid input: speed must lie between 0.5 and 2.0");
    Q3_CHECK(in && out && n_out && n_in > 0, 3, "Invalid input: empty audio");
    Q3_CHECK(n_in <= (int64_t(1) << 26), 3, "Invalid input: time stretch takes between 1 and 2^26 samples");
    StretchDev* sd = nullptr;
    for (const auto& s : stretchers_)
        if (s->plan.hs == hs) sd = s.get();
    if (!sd) {
        auto s = std::make_unique<StretchDev>();
        s->plan = make_stretch_plan(hs);
        Q3_HIP(hipMemcpy(s->fade.grow(size_t(hs)), s->plan.fade.data(), size_t(hs) * 4, hipMemcpyHostToDevice));
        stretchers_.push_back(std::move(s));
        sd = stretchers_.back().get();
    }
    const int64_t no = sd->plan.out_len(n_in, causal);
    *n_out = no;
    Q3_CHECK(cap >= no, 3, "Invalid input: output buffer too small for the stretched audio");
    bool finite = true;
    for (int64_t i = 0; i < n_in; ++i) finite = finite && (std::fabs(in[i]) <= 3.0e38f);
    Q3_CHECK(finite, 3, "Invalid input: audio holds non-finite samples");
    if (no == 0) return;  // (causal form of less than one hop)
    const float* a = upload_audio(in, n_in);
    if (size_t(no) > rs_out_dev_.capacity()) Q3_HIP(hipStreamSynchronize(st_));  // the old buffer may still be read
    rs_out_dev_.grow(size_t(no));
    rs_len_dev_.grow(1);
    const int32_t len = int32_t(n_in);
    Q3_HIP(hipStreamSynchronize(st_));  // `len` is pageable stack memory, and the device word may still feed an earlier launch
    Q3_HIP(hipMemcpy(rs_len_dev_, &len, 4, hipMemcpyHostToDevice));
    StretchArgs sa{};
    sa.x = a; sa.y = rs_out_dev_;
    sa.len = rs_len_dev_; sa.len_mul = 1;
    sa.fade = sd->fade; sa.hs = hs; sa.delay = causal ? sd->plan.delay : 0;
    sa.causal = causal ? 1 : 0; sa.B = 1;
    launch_stretch(sa, st_);
    Q3_HIP(hipStreamSynchronize(st_));
    Q3_HIP(hipMemcpy(out, rs_out_dev_, size_t(no) * 4, hipMemcpyDeviceToHost));
}

void Engine::debug_stretch_rows(const float* x, const int32_t* lens, const int32_t* hops, int B, int64_t x_stride, float* y,
                                int64_t y_stride) {
    Q3_CHECK(B >= 1 && B <= 4096 && x_stride >= 1 && y_stride >= 1 && x_stride <= (int64_t(1) << 26) && y_stride <= (int64_t(1) << 27), 3,
             "Invalid input: debug_stretch_rows takes 1..4096 rows of at most 2^26 samples");
    for (int b = 0; b < B; ++b) {
        Q3_CHECK(hops[b] == 0 || (hops[b] >= kStretchHsMin && hops[b] <= kStretchHsMax), 3, "Invalid input: a hop must be 0 or lie in [240, 960]");
        Q3_CHECK(lens[b] >= 0 && lens[b] <= x_stride, 3, "Invalid input: a row is longer than x_stride");
        const int64_t no = hops[b] == 0 ? int64_t(lens[b]) : int64_t(lens[b] / kStretchHa) * hops[b];
        Q3_CHECK(no <= y_stride, 3, "Invalid input: a row's output does not fit y_stride");
    }
    // rows start at 16-byte boundaries on the device, as the tail's tensors do
    const int64_t xs = (x_stride + 3) & ~int64_t(3), ys = (y_stride + 3) & ~int64_t(3);
    if (dbg_fade_all_.capacity() == 0) {
        const std::vector<float> all = make_fade_all();
        Q3_HIP(hipMemcpy(dbg_fade_all_.grow(all.size()), all.data(), all.size() * 4, hipMemcpyHostToDevice));
    }
    DevBuf<float> dx, dy;
    DevBuf<int32_t> dl;
    dx.grow(size_t(B) * size_t(xs));
    dy.grow(size_t(B) * size_t(ys));
    dl.grow(size_t(2 * B));
    Q3_HIP(hipStreamSynchronize(st_));
    Q3_HIP(hipMemcpy2D(dx, size_t(xs) * 4, x, size_t(x_stride) * 4, size_t(x_stride) * 4, size_t(B), hipMemcpyHostToDevice));
    Q3_HIP(hipMemcpy2D(dy, size_t(ys) * 4, y, size_t(y_stride) * 4, size_t(y_stride) * 4, size_t(B), hipMemcpyHostToDevice));
    Q3_HIP(hipMemcpy(dl, lens, size_t(B) * 4, hipMemcpyHostToDevice));
    Q3_HIP(hipMemcpy(dl + B, hops, size_t(B) * 4, hipMemcpyHostToDevice));
    StretchArgs sa{};
    sa.x = dx; sa.x_bstride = xs;
    sa.y = dy; sa.y_bstride = ys;
    sa.len = dl; sa.len_mul = 1;
    sa.hs_rows = dl + B; sa.fade_all = dbg_fade_all_;
    sa.causal = 1; sa.B = B;
    launch_stretch(sa, st_);
    Q3_HIP(hipStreamSynchronize(st_));
    Q3_HIP(hipMemcpy2D(y, size_t(y_stride) * 4, dy, size_t(ys) * 4, size_t(y_stride) * 4, size_t(B), hipMemcpyDeviceToHost));
}

const Engine::ResamplerDev& Engine::ratio_resampler(int64_t in_units, int64_t out_units) {
    Q3_CHECK(in_units >= 1 && out_units >= 1 && in_units <= (int64_t(1) << 30) && out_units <= (int64_t(1) << 30), 3,
             "Invalid input: a resampling ratio takes two integers between 1 and 2^30");
    for (const auto& r : ratios_)
        if (r->plan.in_rate == int(in_units) && r->plan.out_rate == int(out_units)) return *r;
    // (sized before it is built: the table's L * 2K entries cost a Bessel series each)
    const PitchRatio pr = pitch_ratio(int(in_units), int(out_units), 1, 1);
    Q3_CHECK(int64_t(pr.L) * 2 * pr.K <= (int64_t(1) << 22), 3, "Invalid input: the ratio's phase table is larger than 16 MiB");
    Q3_CHECK(resample_ratio_lds_bytes(pr.L, pr.M, pr.K) <= 64 * 1024, 3, "Invalid input: the ratio's input span is larger than its LDS budget");
    auto r = std::make_unique<ResamplerDev>();
    r->plan = make_resample_plan(int(in_units), int(out_units));
    const std::vector<float> tab = resample_table_output_order(r->plan);
    Q3_HIP(hipMemcpy(r->tab.grow(tab.size()), tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
    ratios_.push_back(std::move(r));
    return *ratios_.back();
}

void Engine::pitch_shift(const float* in, int64_t n_in, float semitones, float* out, int64_t cap, int64_t* n_out) {
    // (the pitch is refused first, whatever else is wrong, and before any GPU work)
    const int hp = pitch_choose_hp(kStretchHa, semitones);
    Q3_CHECK(hp != 0, 3, "Invalid input: pitch must lie between -12 and 12 semitones");
    Q3_CHECK(in && out && n_out && n_in > 0, 3, "Invalid input: empty audio");
    Q3_CHECK(n_in <= (int64_t(1) << 26), 3, "Invalid input: pitch shift takes between 1 and 2^26 samples");
    const int64_t n_mid = (n_in * hp + kStretchHa - 1) / kStretchHa;  // the whole form's length at Hp
    const PitchRatio pr = pitch_ratio(hp, kStretchHa, 1, 1);
    const int64_t no = hp == kStretchHa ? n_in : (n_mid * pr.L + pr.M - 1) / pr.M;
    *n_out = no;
    Q3_CHECK(cap >= no, 3, "Invalid input: output buffer too small for the shifted audio");
    bool finite = true;
    for (int64_t i = 0; i < n_in; ++i) finite = finite && (std::fabs(in[i]) <= 3.0e38f);
    Q3_CHECK(finite, 3, "Invalid input: audio holds non-finite samples");
    if (hp == kStretchHa) {  // off: the samples as they are
        std::memcpy(out, in, size_t(n_in) * 4);
        return;
    }
    StretchDev* sd = nullptr;
    for (const auto& s : stretchers_)
        if (s->plan.hs == hp) sd = s.get();
    if (!sd) {
        auto s = std::make_unique<StretchDev>();
        s->plan = make_stretch_plan(hp);
        Q3_HIP(hipMemcpy(s->fade.grow(size_t(hp)), s->plan.fade.data(), size_t(hp) * 4, hipMemcpyHostToDevice));
        stretchers_.push_back(std::move(s));
        sd = stretchers_.back().get();
    }
    const ResamplerDev& r = ratio_resampler(hp, kStretchHa);
    const float* a = upload_audio(in, n_in);
    if (size_t(no) > rs_out_dev_.capacity() || size_t(n_mid) > ps_mid_dev_.capacity()) Q3_HIP(hipStreamSynchronize(st_));  // the old buffers may still be read
    rs_out_dev_.grow(size_t(no));
    ps_mid_dev_.grow(size_t(n_mid));
    rs_len_dev_.grow(2);
    const int32_t len[2] = {int32_t(n_in), int32_t(n_mid)};
    Q3_HIP(hipStreamSynchronize(st_));  // `len` is pageable stack memory, and the device words may still feed an earlier launch
    Q3_HIP(hipMemcpy(rs_len_dev_, len, 8, hipMemcpyHostToDevice));
    StretchArgs sa{};
    sa.x = a; sa.y = ps_mid_dev_;
    sa.len = rs_len_dev_; sa.len_mul = 1;
    sa.fade = sd->fade; sa.hs = hp; sa.delay = 0;
    sa.causal = 0; sa.B = 1;
    launch_stretch(sa, st_);
    ResampleArgs ra{};
    ra.x = ps_mid_dev_; ra.x_bstride = 0;
    ra.y = rs_out_dev_; ra.y_bstride = 0;
    ra.len = rs_len_dev_ + 1; ra.len_mul = 1; ra.max_in = n_mid;
    ra.tab = r.tab; ra.L = r.plan.L; ra.M = r.plan.M; ra.K = r.plan.K;
    ra.hist = 0; ra.centred = 1; ra.clamp = 0; ra.B = 1;
    launch_resample_ratio(ra, st_);
    Q3_HIP(hipStreamSynchronize(st_));
    Q3_HIP(hipMemcpy(out, rs_out_dev_, size_t(no) * 4, hipMemcpyDeviceToHost));
}

void Engine::debug_resample_ratio(const float* x, const int32_t* lens, int B, int64_t row_stride, int64_t in_units, int64_t out_units,
                                  bool centred, bool clamp, int hist, float* y, int64_t y_stride) {
    Q3_CHECK(B >= 1 && B <= 4096 && row_stride >= 1 && y_stride >= 1 && row_stride <= (int64_t(1) << 26) && y_stride <= (int64_t(1) << 27) &&
                 hist >= 0 && hist <= row_stride, 3,
             "Invalid input: debug_resample_ratio takes 1..4096 rows of at most 2^26 samples");
    const ResamplerDev& r = ratio_resampler(in_units, out_units);
    int64_t max_in = 0;
    for (int b = 0; b < B; ++b) {
        Q3_CHECK(lens[b] >= 0 && int64_t(hist) + lens[b] <= row_stride, 3, "Invalid input: a row is longer than row_stride");
        Q3_CHECK(r.plan.out_len(lens[b]) <= y_stride, 3, "Invalid input: a row's output does not fit y_stride");
        max_in = std::max<int64_t>(max_in, lens[b]);
    }
    // a row's first sample (behind its margin) starts at a 16-byte boundary on the device, as the tail's tensors do
    const int64_t hpad = (int64_t(hist) + 3) & ~int64_t(3);
    const int64_t xs = (hpad - hist + row_stride + 3) & ~int64_t(3), ys = (y_stride + 3) & ~int64_t(3);
    DevBuf<float> dx, dy;
    DevBuf<int32_t> dl;
    dx.grow(size_t(B) * size_t(xs));
    dy.grow(size_t(B) * size_t(ys));
    dl.grow(size_t(B));
    Q3_HIP(hipStreamSynchronize(st_));
    Q3_HIP(hipMemset(dx, 0, size_t(B) * size_t(xs) * 4));
    Q3_HIP(hipMemcpy2D(dx + (hpad - hist), size_t(xs) * 4, x, size_t(row_stride) * 4, size_t(row_stride) * 4, size_t(B), hipMemcpyHostToDevice));
    Q3_HIP(hipMemcpy2D(dy, size_t(ys) * 4, y, size_t(y_stride) * 4, size_t(y_stride) * 4, size_t(B), hipMemcpyHostToDevice));
    Q3_HIP(hipMemcpy(dl, lens, size_t(B) * 4, hipMemcpyHostToDevice));
    ResampleArgs ra{};
    ra.x = dx + hpad; ra.x_bstride = xs;
    ra.y = dy; ra.y_bstride = ys;
    ra.len = dl; ra.len_mul = 1; ra.max_in = max_in;
    ra.tab = r.tab; ra.L = r.plan.L; ra.M = r.plan.M; ra.K = r.plan.K;
    ra.hist = hist; ra.centred = centred ? 1 : 0; ra.clamp = clamp ? 1 : 0; ra.B = B;
    launch_resample_ratio(ra, st_);
    Q3_HIP(hipStreamSynchronize(st_));
    Q3_HIP(hipMemcpy2D(y, size_t(y_stride) * 4, dy, size_t(ys) * 4, size_t(y_stride) * 4, size_t(B), hipMemcpyDeviceToHost));
}

void Engine::pitch_shift_formants(const float* in, int64_t n_in, float semitones, float* out, int64_t cap, int64_t* n_out) {
    // (the pitch is refused first, whatever else is wrong, and before any GPU work)
    const int hp = pitch_choose_hp(kStretchHa, semitones);
    Q3_CHECK(hp != 0, 3, "Invalid input: pitch must lie between -12 and 12 semitones");
    if (hp == kStretchHa) {  // off: pitch_shift's copy, with its checks
        pitch_shift(in, n_in, semitones, out, cap, n_out);
        return;
    }
    Q3_CHECK(in && out && n_out && n_in > 0, 3, "Invalid input: empty audio");
    Q3_CHECK(n_in <= (int64_t(1) << 26), 3, "Invalid input: pitch shift takes between 1 and 2^26 samples");
    const int64_t n_mid = (n_in * hp + kStretchHa - 1) / kStretchHa;  // the whole form's length at Hp
    const PitchRatio pr = pitch_ratio(hp, kStretchHa, 1, 1);
    const int64_t no = (n_mid * pr.L + pr.M - 1) / pr.M;
    *n_out = no;
    Q3_CHECK(cap >= no, 3, "Invalid input: output buffer too small for the shifted audio");
    bool finite = true;
    for (int64_t i = 0; i < n_in; ++i) finite = finite && (std::fabs(in[i]) <= 3.0e38f);
    Q3_CHECK(finite, 3, "Invalid input: audio holds non-finite samples");
    StretchDev* sd = nullptr;
    for (const auto& s : stretchers_)
        if (s->plan.hs == hp) sd = s.get();
    if (!sd) {
        auto s = std::make_unique<StretchDev>();
        s->plan = make_stretch_plan(hp);
        Q3_HIP(hipMemcpy(s->fade.grow(size_t(hp)), s->plan.fade.data(), size_t(hp) * 4, hipMemcpyHostToDevice));
        stretchers_.push_back(std::move(s));
        sd = stretchers_.back().get();
    }
    const ResamplerDev& r = ratio_resampler(hp, kStretchHa);
    const FormantPlan fp = make_formant_plan(hp);
    std::vector<float> tabs(fp.win);
    tabs.insert(tabs.end(), fp.lag, fp.lag + kFormantOrder + 1);
    const int64_t hops = (n_mid + hp - 1) / hp;
    DevBuf<float> dtab, de, dcoef, dep;  // (freed behind the synchronisation below)
    dtab.grow(tabs.size());
    de.grow(size_t(n_mid));
    dcoef.grow(size_t(hops) * kFormantOrder);
    dep.grow(size_t(no));
    const float* a = upload_audio(in, n_in);
    if (size_t(no) > rs_out_dev_.capacity() || size_t(n_mid) > ps_mid_dev_.capacity()) Q3_HIP(hipStreamSynchronize(st_));  // the old buffers may still be read
    rs_out_dev_.grow(size_t(no));
    ps_mid_dev_.grow(size_t(n_mid));
    rs_len_dev_.grow(4);
    const int32_t len[3] = {int32_t(n_in), int32_t(n_mid), int32_t(no)};
    Q3_HIP(hipStreamSynchronize(st_));  // `len` is pageable stack memory, and the device words may still feed an earlier launch
    Q3_HIP(hipMemcpy(rs_len_dev_, len, 12, hipMemcpyHostToDevice));
    Q3_HIP(hipMemcpy(dtab, tabs.data(), tabs.size() * 4, hipMemcpyHostToDevice));
    StretchArgs sa{};
    sa.x = a; sa.y = ps_mid_dev_;
    sa.len = rs_len_dev_; sa.len_mul = 1;
    sa.fade = sd->fade; sa.hs = hp; sa.delay = 0;
    sa.causal = 0; sa.B = 1;
    launch_stretch(sa, st_);
    FormantAnalyseArgs fa{};
    fa.y = ps_mid_dev_; fa.len = rs_len_dev_ + 1; fa.len_mul = 1; fa.hist = 0; fa.hp = hp;
    fa.win = dtab; fa.lag = dtab + 2 * size_t(hp);
    fa.coef = dcoef; fa.e = de; fa.B = 1; fa.max_len = n_mid;
    launch_formant_analyse(fa, st_);
    ResampleArgs ra{};
    ra.x = de; ra.x_bstride = 0;
    ra.y = dep; ra.y_bstride = 0;
    ra.len = rs_len_dev_ + 1; ra.len_mul = 1; ra.max_in = n_mid;
    ra.tab = r.tab; ra.L = r.plan.L; ra.M = r.plan.M; ra.K = r.plan.K;
    ra.hist = 0; ra.centred = 1; ra.clamp = 0; ra.B = 1;
    launch_resample_ratio(ra, st_);
    FormantSynthArgs fs{};
    fs.ep = dep; fs.out = rs_out_dev_; fs.len = rs_len_dev_ + 2; fs.len_mul = 1; fs.ho = kStretchHa;
    fs.coef = dcoef; fs.clamp = 0; fs.B = 1; fs.max_len = no;
    launch_formant_synth(fs, st_);
    Q3_HIP(hipStreamSynchronize(st_));
    Q3_HIP(hipMemcpy(out, rs_out_dev_, size_t(no) * 4, hipMemcpyDeviceToHost));
}

void Engine::debug_formant_rows(int mode, int hp, int ho, const int32_t* lens, int B, const float* x, int64_t x_stride, int hist, float* coef,
                                int64_t coef_stride, const float* state_in, float* state_out, float* y, int64_t y_stride, bool clamp) {
    constexpr int P = kFormantOrder;
    Q3_CHECK(mode >= 0 && mode <= 2, 3, "Invalid input: debug_formant_rows mode must be 0 (analyse + whiten), 1 (synthesise) or 2 (both)");
    Q3_CHECK(hp >= kStretchHsMin && hp <= kStretchHsMax && ho >= kStretchHsMin && ho <= kStretchHsMax, 3,
             "Invalid input: debug_formant_rows takes hops between 240 and 960");
    Q3_CHECK(mode != 2 || hp == ho, 3, "Invalid input: debug_formant_rows runs both kernels with the identity in between only when Hp == Ho");
    Q3_CHECK(B >= 1 && B <= 4096 && x_stride >= 1 && y_stride >= 1 && coef_stride >= P && x_stride <= (int64_t(1) << 26) &&
                 y_stride <= (int64_t(1) << 26) && coef_stride <= (int64_t(1) << 26) && hist >= 0 && hist <= x_stride,
             3, "Invalid input: debug_formant_rows takes 1..4096 rows of at most 2^26 samples");
    Q3_CHECK(mode != 1 || hist == 0, 3, "Invalid input: debug_formant_rows synthesises rows without a margin (their history is the state)");
    Q3_CHECK(mode != 0 || (!state_in && !state_out), 3, "Invalid input: debug_formant_rows analyses without a state");
    const int hop = mode == 1 ? ho : hp;  // the hop the rows' lengths count in
    int64_t max_len = 0;
    for (int b = 0; b < B; ++b) {
        Q3_CHECK(lens[b] >= 0 && int64_t(hist) + lens[b] <= x_stride && lens[b] <= y_stride, 3, "Invalid input: a row is longer than its stride");
        Q3_CHECK((int64_t(lens[b]) + hop - 1) / hop * P <= coef_stride, 3, "Invalid input: a row's coefficients do not fit coef_stride");
        max_len = std::max<int64_t>(max_len, lens[b]);
    }
    const int64_t hpad = (int64_t(hist) + 3) & ~int64_t(3);
    const int64_t xs = (hpad - hist + x_stride + 3) & ~int64_t(3), ys = (y_stride + 3) & ~int64_t(3), cs = (coef_stride + 3) & ~int64_t(3);
    DevBuf<float> dx, dy, dc, dm, ds, dtab;
    DevBuf<int32_t> dl;
    dx.grow(size_t(B) * size_t(xs));
    dy.grow(size_t(B) * size_t(ys));
    dc.grow(size_t(B) * size_t(cs));
    dm.grow(size_t(B) * size_t(ys));  // mode 2: the whitened signal between the kernels
    ds.grow(size_t(B) * P);
    dl.grow(size_t(B));
    const FormantPlan fp = make_formant_plan(hp);
    std::vector<float> tabs(fp.win);
    tabs.insert(tabs.end(), fp.lag, fp.lag + P + 1);
    dtab.grow(tabs.size());
    Q3_HIP(hipStreamSynchronize(st_));
    Q3_HIP(hipMemcpy(dtab, tabs.data(), tabs.size() * 4, hipMemcpyHostToDevice));
    Q3_HIP(hipMemset(dx, 0, size_t(B) * size_t(xs) * 4));
    Q3_HIP(hipMemcpy2D(dx + (hpad - hist), size_t(xs) * 4, x, size_t(x_stride) * 4, size_t(x_stride) * 4, size_t(B), hipMemcpyHostToDevice));
    Q3_HIP(hipMemcpy2D(dy, size_t(ys) * 4, y, size_t(y_stride) * 4, size_t(y_stride) * 4, size_t(B), hipMemcpyHostToDevice));
    Q3_HIP(hipMemcpy2D(dm, size_t(ys) * 4, y, size_t(y_stride) * 4, size_t(y_stride) * 4, size_t(B), hipMemcpyHostToDevice));
    Q3_HIP(hipMemcpy2D(dc, size_t(cs) * 4, coef, size_t(coef_stride) * 4, size_t(coef_stride) * 4, size_t(B), hipMemcpyHostToDevice));
    if (state_in) Q3_HIP(hipMemcpy(ds, state_in, size_t(B) * P * 4, hipMemcpyHostToDevice));
    else Q3_HIP(hipMemset(ds, 0, size_t(B) * P * 4));
    Q3_HIP(hipMemcpy(dl, lens, size_t(B) * 4, hipMemcpyHostToDevice));
    if (mode != 1) {
        FormantAnalyseArgs fa{};
        fa.y = dx + hpad; fa.y_bstride = xs;
        fa.len = dl; fa.len_mul = 1; fa.hist = hist; fa.hp = hp;
        fa.win = dtab; fa.lag = dtab + 2 * size_t(hp);
        fa.coef = dc; fa.coef_bstride = cs;
        fa.e = mode == 0 ? dy : dm; fa.e_bstride = ys;
        fa.B = B; fa.max_len = max_len;
        launch_formant_analyse(fa, st_);
    }
    if (mode != 0) {
        FormantSynthArgs fs{};
        fs.ep = mode == 1 ? dx + hpad : dm; fs.ep_bstride = mode == 1 ? xs : ys;
        fs.out = dy; fs.out_bstride = ys;
        fs.len = dl; fs.len_mul = 1; fs.ho = ho;
        fs.coef = dc; fs.coef_bstride = cs;
        fs.clamp = clamp ? 1 : 0; fs.B = B; fs.max_len = max_len;
        fs.state_in = ds; fs.state_in_bstride = P;
        fs.state_out = ds; fs.state_out_bstride = P;
        launch_formant_synth(fs, st_);
    }
    Q3_HIP(hipStreamSynchronize(st_));
    Q3_HIP(hipMemcpy2D(y, size_t(y_stride) * 4, dy, size_t(ys) * 4, size_t(y_stride) * 4, size_t(B), hipMemcpyDeviceToHost));
    Q3_HIP(hipMemcpy2D(coef, size_t(coef_stride) * 4, dc, size_t(cs) * 4, size_t(coef_stride) * 4, size_t(B), hipMemcpyDeviceToHost));
    if (state_out) Q3_HIP(hipMemcpy(state_out, ds, size_t(B) * P * 4, hipMemcpyDeviceToHost));
}

std::unique_ptr<Voice> Engine::create_voice(const float* audio, int64_t n_samples, const int32_t* ref_text_ids, int n_ref_text_ids,
                                            int sample_rate) {
    const TalkerConfig& t = m_->cfg.talker;
    const int H = t.hidden_size;
    if (sample_rate != kResampleNative)
        Q3_CHECK(resample_pair_supported(sample_rate, kResampleNative), 3,
                 "Invalid input: a voice's sample_rate must be 8000, 12000, 16000, 22050, 24000, 32000, 44100 or 48000");
    check_reference(audio, n_samples, ref_text_ids, n_ref_text_ids);
    Q3_CHECK(fe_ != nullptr, 1, "Model not initialized: Speech tokenizer encoder not available");
    Q3_CHECK(m_->codec_enc.bins <= t.vocab_size && m_->codec_enc.bins <= t.cp.vocab_size, 3,
             "Invalid input: encoder codebook larger than the codec embedding tables");
    for (int i = 0; i < n_ref_text_ids; ++i)
        Q3_CHECK(ref_text_ids[i] >= 0 && ref_text_ids[i] < t.text_vocab_size, 3, "Invalid input: reference text token id out of range");
    auto v = std::make_unique<Voice>();
    const float* a = nullptr;
    if (sample_rate != kResampleNative) a = resample_upload(audio, n_samples, sample_rate, kResampleNative, true, &n_samples);
    else a = upload_audio(audio, n_samples);
    const int T = fe_->encoded_frames(n_samples);
    v->ref_T = T;
    v->n_ref_samples = n_samples;
    v->ref_text_ids.assign(ref_text_ids, ref_text_ids + n_ref_text_ids);
    v->codes_dev = v->codes_own.grow(size_t(16) * T);
    v->rows_dev = v->rows_own.grow(size_t(1 + T) * H);
    v->device_bytes = int64_t(size_t(16) * T * 4 + size_t(1 + T) * H * 2);
    Q3_HIP(hipEventRecord(ev_fe_[0], st_));
    fe_->encode(a, n_samples, v->codes_dev);
    if (m_->has_speaker_encoder) {  // fp32 x-vector, then the talker's storage dtype like every other prompt row (prepare_clone_rows)
        spk_f32_.grow(size_t(H));
        fe_->speaker_embedding(a, n_samples, spk_f32_);
        launch_f32_to_bf16(spk_f32_, v->rows_dev, H, st_);
    } else {
        Q3_HIP(hipMemsetAsync(v->rows_dev, 0, size_t(H) * 2, st_));  // (no prompt row names it)
    }
    launch_ref_embed_rows(v->codes_dev, T, 16, m_->codec_emb, m_->cp_emb_dev, H, v->rows_dev + size_t(H), H, st_);
    Q3_HIP(hipEventRecord(ev_fe_[1], st_));
    std::vector<int32_t> rows(size_t(16) * T);
    Q3_HIP(hipMemcpyAsync(rows.data(), v->codes_dev, rows.size() * 4, hipMemcpyDeviceToHost, st_));
    Q3_HIP(hipStreamSynchronize(st_));  // from here on the voice is read-only: any context, any lane
    v->code0.assign(rows.begin(), rows.begin() + T);
    v->codes_host.resize(size_t(T) * 16);
    for (int f = 0; f < T; ++f)
        for (int g = 0; g < 16; ++g) v->codes_host[size_t(f) * 16 + g] = rows[size_t(g) * T + f];
    float ms = 0;
    Q3_HIP(hipEventElapsedTime(&ms, ev_fe_[0], ev_fe_[1]));
    timing = q3tts_timing{};
    timing.frontend_ms = ms;
    return v;
}


// Prefill of n right-aligned prompts: positions 0 .. Pmax-2 through the talker's layers into the pages `block_table` names, then
// the last position loaded into w.h / w.ss_a (the first frame step consumes it). begin() runs it on the frame step's own
// activations and arrays; a queued admission on a sub-batch's (run_queued), so that the rows in flight keep theirs.
void Engine::enqueue_prefill(Stream& w, int n, int Pmax, const int32_t* block_table, int32_t* kv_len, const int32_t* n_prompt,
                             uint8_t* active) {
    const int H = m_->cfg.talker.hidden_size;
    PrefillLoadArgs pl{};
    pl.prompt = prompt_; pl.n_prompt = n_prompt; pl.Pmax = Pcap_; pl.H = H; pl.B = n; pl.h = w.h; pl.hMB = Mp_ / 16;
    pl.ss_out = w.ss_a; pl.active = active;
    // prompt_ rows are laid out with stride Pcap_; right alignment is relative to the longest prompt.
    // Positions 0 .. Pmax-2 go through the decode kernels C at a time (C * n <= Mp_ activation rows: the GEMMs stream
    // the weights once per chunk instead of once per position); rows whose prompt is shorter start inside a chunk.
    const int P1 = Pmax - 1;  // positions before the one the first frame step consumes
    int C = std::max(1, std::min(16, Mp_ / n));
    const int S = (P1 + C - 1) / C;
    for (int s = 0; s < S; ++s) {
        // element p of row b in chunk s is prompt position r = s*C - S*C + (n_prompt[b] - 1) + p
        const int r_base = s * C - S * C - 1;
        if (C == 1) {
            pl.step = s + (Pcap_ - Pmax);
            launch_prefill_load(pl, st_);
            enqueue_layers(m_->talker, w, n, kpool_, vpool_, kv_layer_stride_, block_table, max_pages_, kv_len, active, 1, -1, 1, nullptr, 0);
            launch_advance_len(kv_len, active, n, st_);
        } else {
            PrefillLoadArgs pc = pl;
            pc.step = r_base;
            launch_prefill_chunk_load(pc, C, st_);
            enqueue_layers(m_->talker, w, n, kpool_, vpool_, kv_layer_stride_, block_table, max_pages_, kv_len, nullptr, 1, -1,
                           C, n_prompt, r_base);
            launch_advance_len_chunk(kv_len, n_prompt, r_base, C, n, st_);
        }
    }
    pl.step = (Pmax - 1) + (Pcap_ - Pmax);  // the last prompt position: consumed by the first frame step
    launch_prefill_load(pl, st_);
}

// ------------------------------------------------------------------------------------------------
// generate
// ------------------------------------------------------------------------------------------------
void Engine::generate(const q3tts_request* reqs, int n, const q3tts_sampling& sp, q3tts_event_cb cb, void* user,
                      q3tts_result* results, const DebugOpts* dbg, const Voice* const* voices) {
    end(begin(reqs, n, sp, cb, user, dbg, false, false, voices), results);
}

// The codec runner's scratch is shared by both codec streams: before it moves to the other one, the one it ran on drains.
hipStream_t Engine::codec_stream(bool overlapped, bool wide) {
    hipStream_t want = overlapped && st_codec_part_ ? (wide && st_codec_wide_ ? st_codec_wide_ : st_codec_part_) : st_codec_;
    if (want != codec_->stream()) {
        Q3_HIP(hipStreamSynchronize(codec_->stream()));
        codec_->set_stream(want);
    }
    return want;
}

void Engine::check_stream_chunk(int chunk_frames) const {
    Q3_CHECK(m_->has_codec, 1, "Model not initialized: Speech tokenizer not loaded");
    const int hist = codec_->hist_frames();
    Q3_CHECK(chunk_frames >= hist, 3, "Invalid input: audio_chunk_frames of a streamed decode must be at least " + std::to_string(hist));
}

int Engine::begin(const q3tts_request* reqs, int n, const q3tts_sampling& sp, q3tts_event_cb cb, void* user, const DebugOpts* dbg,
                  bool overlapped, bool background, const Voice* const* voices) {
    Q3_HIP(hipSetDevice(m_->device));  // lanes run on their own host threads
    std::vector<ResolvedRequest> rr;
    double t_start = 0;
    const int slot = open_job(reqs, n, sp, dbg, rr, t_start, voices);
    bool any_clone = false;
    for (auto& r : rr) any_clone = any_clone || r.clone;
    Q3_HIP(hipEventRecord(ev_fe_[0], st_));
    // codec encoder + speaker encoder, once per request that carries a waveform (Qwen3.swift:443, :524)
    const bool frontend = any_clone && prepare_clone_rows(rr);
    Q3_HIP(hipEventRecord(ev_fe_[1], st_));
    std::vector<int> np, nt;
    assemble_prompts(rr, np, nt);
    const int Pmax = reserve_rows(rr, np, nt, sp);
    if (dbg) debug_buffers(n, *dbg);
    // ---- prefill: positions 0 .. Pmax-2 of the right-aligned prompts, then load the last one ----
    Q3_HIP(hipEventRecord(ev_[0], st_));
    enqueue_prefill(tk_, n, Pmax, block_table_, kv_len_, n_prompt_, active_);
    Q3_HIP(hipEventRecord(ev_[1], st_));
    Job& J = jobs_[slot];
    J.reset(n, codec_->upsample());
    {
        std::vector<int> hs;
        for (const auto& r : rr) hs.push_back(r.hs);
        set_row_speeds(J, hs);
    }
    J.chunk_frames = sp.audio_chunk_frames;
    J.frontend = frontend;
    J.busy = true;  // nothing below gives the slot back except end() -- or a back half that fails inside this call
    // The throughput jobs -- nobody listens for TOKEN events, nothing is streamed or dumped -- leave the frame loop to the
    // worker thread, so that the caller can begin the next batch on the other context while this chain runs.
    if (background && !cb && !dbg && sp.audio_chunk_frames == 0) {
        J.background = true;
        J.rr = std::move(rr);
        J.np = std::move(np);
        J.sp = sp;
        J.sp.per_request = nullptr;  // (the caller's array was read by reserve_rows above; it is theirs again once begin returns)
        J.overlapped = overlapped;
        J.t_start = t_start;
        std::lock_guard<std::mutex> lk(work_mu_);
        if (!worker_.joinable()) worker_ = std::thread([this] { worker_loop(); });
        J.back = 1;
        J.back_status = 0;
        J.back_err.clear();
        work_ = &J;
        work_cv_.notify_all();
        return slot;
    }
    try {
        // clone rows are streamed only on request (audio_stream_reference: their reference goes in front of their stream);
        // without it a batch with a clone row is decoded one-shot
        back_half(J, rr, np, sp, cb, user, dbg,
                  sp.audio_chunk_frames > 0 && sp.audio_window_frames > 0 && (!any_clone || sp.audio_stream_reference != 0) && !dbg, overlapped,
                  t_start);
    } catch (...) {
        J.busy = false;
        throw;
    }
    return slot;
}

void Engine::back_half(Job& J, const std::vector<ResolvedRequest>& rr, const std::vector<int>& np, const q3tts_sampling& sp,
                       q3tts_event_cb cb, void* user, const DebugOpts* dbg, bool streamed, bool overlapped, double t_start) {
    if (J.background && debug_env().fail_back_half) throw Error(7, "back half failed on request (Q3TTS_TEST_FAIL_BACK_HALF)");
    StreamedDecode sd(*this, J, streamed, sp, cb, user, rr, t_start);
    const int launched = frame_loop(J, rr, sp, cb, user, dbg, sd);
    hand_off(J, rr, sd, launched, overlapped);
    job_timing(J, np, launched);
    publish_job(J, cb, user, request_base, t_start, overlapped);  // a pipelined job: its rows are copied out while the next batch runs
}

void Engine::worker_loop() {
    std::unique_lock<std::mutex> lk(work_mu_);
    for (;;) {
        work_cv_.wait(lk, [&] { return work_ || work_stop_; });
        if (!work_) return;  // (stop: only once the job that was begun has run)
        Job& J = *work_;
        work_ = nullptr;
        lk.unlock();
        int status = 0;
        std::string err;
        try {
            Q3_HIP(hipSetDevice(m_->device));
            back_half(J, J.rr, J.np, J.sp, nullptr, nullptr, nullptr, false, J.overlapped, J.t_start);
        } catch (const Error& e) {
            status = e.status;
            err = e.what();
        } catch (const std::exception& e) {
            status = 7;
            err = e.what();
        } catch (...) {
            status = 7;
            err = "unknown exception in a job's frame loop";
        }
        lk.lock();
        J.back_status = status;
        J.back_err = err;
        J.back = 0;
        work_cv_.notify_all();
    }
}

void Engine::drain() {
    std::unique_lock<std::mutex> lk(work_mu_);
    work_cv_.wait(lk, [&] {
        for (const auto& J : jobs_)
            if (J.back) return false;
        return true;
    });
}

int Engine::open_job(const q3tts_request* reqs, int n, const q3tts_sampling& sp, const DebugOpts* dbg, std::vector<ResolvedRequest>& rr,
                     double& t_start, const Voice* const* voices) {
    Q3_CHECK(n >= 1 && n <= Bm_, 3, "Invalid input: batch size must be between 1 and max_batch");
    Q3_CHECK(m_->cfg.talker.num_code_groups == 16, 3, "Invalid input: num_code_groups must be 16");
    Q3_CHECK(sp.audio_chunk_frames >= 0, 3, "Invalid input: audio_chunk_frames must not be negative");
    if (sp.audio_chunk_frames > 0 && codec_ && codec_->keep_formants()) {
        // (before any GPU work) a job with chunks that will not be streamed -- no window, a clone row without
        // audio_stream_reference, a debug job: begin()'s own condition -- goes to the chunked exact decode, which recomputes its
        // left context and cannot recompute the synthesis filter's state
        bool any_clone = false;
        for (int i = 0; reqs && i < n; ++i) any_clone = any_clone || reqs[i].ref_audio != nullptr || (voices && voices[i]);
        const bool streamed = sp.audio_window_frames > 0 && (!any_clone || sp.audio_stream_reference != 0) && !dbg;
        Q3_CHECK(streamed, 3,
                 "Invalid input: audio_chunk_frames on a handle with keep_formants needs streamed audio: audio_window_frames > 0, and "
                 "audio_stream_reference for voice-clone rows (the chunked exact decode is not offered; or decode in one piece)");
    }
    if (sp.audio_chunk_frames > 0 && sp.audio_window_frames > 0 && m_->has_codec)  // before any GPU work (the stream would refuse it later)
        Q3_CHECK(sp.audio_chunk_frames >= codec_->hist_frames(), 3,
                 "Invalid input: audio_chunk_frames of a streamed decode must be at least " + std::to_string(codec_->hist_frames()));
    int slot = -1;  // any free slot: jobs may be ended in any order
    for (int i = 0; i < kJobSlots; ++i)
        if (!jobs_[i].busy && slot < 0) slot = i;
    Q3_CHECK(slot >= 0, 3, "Invalid input: two jobs are already outstanding (q3tts_generate_end must be called first)");
    t_start = now_s();
    Q3_HIP(hipEventRecord(jobs_[slot].ev_begin, st_));
    for (int i = 0; i < n; ++i) rr.push_back(resolve(reqs[i], sp, voices ? voices[i] : nullptr));
    if (dbg)
        for (auto& r : rr) r.max_frames = dbg->frames;
    for (auto& r : rr) Q3_CHECK(r.max_frames <= Fcap_, 3, "Invalid input: max_tokens exceeds the configured max_frames");
    if (m_->has_codec == false)
        throw Error(1, "Model not initialized: Speech tokenizer not loaded");  // Qwen3.swift:799-801
    return slot;
}

int Engine::reserve_rows(const std::vector<ResolvedRequest>& rr, const std::vector<int>& np, const std::vector<int>& nt,
                         const q3tts_sampling& sp) {
    const int n = int(rr.size());
    int Pmax = 0;
    for (int p : np) Pmax = std::max(Pmax, p);
    std::vector<int32_t> bt((size_t)(n) * max_pages_, 0), maxf((size_t)(n)), ntr((size_t)(n)), npr((size_t)(n));
    int next_page = 0;
    for (int b = 0; b < n; ++b) {
        const int need = ceil_div(np[size_t(b)] + rr[size_t(b)].max_frames + 1, kPageTokens);
        Q3_CHECK(need <= max_pages_ && next_page + need <= n_pages_, 3, "Invalid input: KV pool exhausted");
        for (int i = 0; i < need; ++i) bt[size_t(b) * max_pages_ + i] = next_page++;
        maxf[size_t(b)] = rr[size_t(b)].max_frames;
        ntr[size_t(b)] = nt[size_t(b)];
        npr[size_t(b)] = np[size_t(b)];
    }
    Q3_CHECK(Pmax + *std::max_element(maxf.begin(), maxf.end()) + 1 <= m_->talker.max_pos, 3,
             "Invalid input: sequence longer than the RoPE table");
    Q3_HIP(hipMemcpyAsync(block_table_, bt.data(), bt.size() * 4, hipMemcpyHostToDevice, st_));
    Q3_HIP(hipMemcpyAsync(max_frames_, maxf.data(), size_t(n) * 4, hipMemcpyHostToDevice, st_));
    Q3_HIP(hipMemcpyAsync(n_trailing_, ntr.data(), size_t(n) * 4, hipMemcpyHostToDevice, st_));
    Q3_HIP(hipMemcpyAsync(n_prompt_, npr.data(), size_t(n) * 4, hipMemcpyHostToDevice, st_));
    for (int32_t* p : {kv_len_, cp_len_, n_frames_, trailing_idx_}) Q3_HIP(hipMemsetAsync(p, 0, size_t(n) * 4, st_));
    Q3_HIP(hipMemsetAsync(active_, 0, size_t(n), st_));
    Q3_HIP(hipMemsetAsync(finished_, 0, size_t(n), st_));
    Q3_HIP(hipMemsetAsync(seen_, 0, size_t(n) * m_->cfg.talker.vocab_size, st_));
    Q3_HIP(hipMemsetAsync(codes_, 0, size_t(n) * Fcap_ * 16 * 4, st_));
    upload_sampling(sp, row_offset + sp.row_base, n);
    return Pmax;
}

void Engine::debug_buffers(int n, const DebugOpts& dbg) {
    const TalkerConfig& t = m_->cfg.talker;
    const int V = t.vocab_size, Vc = t.cp.vocab_size;
    for (void* p : {(void*)forced_dev_, (void*)sampled_dev_, (void*)tl_dump_, (void*)cl_dump_})
        if (p) (void)hipFree(p);
    forced_dev_ = sampled_dev_ = nullptr;
    tl_dump_ = cl_dump_ = nullptr;
    const size_t nf = size_t(n) * dbg.frames;
    if (dbg.forced_codes) {
        // teacher-forced codes are fed back as rows of the codec / predictor embedding tables
        for (size_t i = 0; i < nf * 16; ++i) {
            const int32_t c = dbg.forced_codes[i];
            Q3_CHECK(c >= 0 && c < ((i & 15) == 0 ? V : Vc), 3, "Invalid input: forced code outside its vocabulary");
        }
        Q3_HIP(hipMalloc(reinterpret_cast<void**>(&forced_dev_), nf * 16 * 4));
        Q3_HIP(hipMemcpy(forced_dev_, dbg.forced_codes, nf * 16 * 4, hipMemcpyHostToDevice));
    }
    Q3_HIP(hipMalloc(reinterpret_cast<void**>(&sampled_dev_), nf * 16 * 4));
    Q3_HIP(hipMemset(sampled_dev_, 0xff, nf * 16 * 4));
    if (dbg.talker_logits) Q3_HIP(hipMalloc(reinterpret_cast<void**>(&tl_dump_), nf * V * 2));
    if (dbg.cp_logits) Q3_HIP(hipMalloc(reinterpret_cast<void**>(&cl_dump_), nf * (t.num_code_groups - 1) * Vc * 2));
}

int Engine::frame_loop(Job& J, const std::vector<ResolvedRequest>& rr, const q3tts_sampling& sp, q3tts_event_cb cb, void* user,
                       const DebugOpts* dbg, StreamedDecode& sd) {
    const int n = J.n;
    const bool use_graph = opts_.use_graph && !dbg;
    build_cp_proj_tables();
    hipGraphExec_t ge = use_graph ? frame_graph(n) : nullptr;
    int frames_cap = 0;
    for (auto& r : rr) frames_cap = std::max(frames_cap, r.max_frames);
    std::vector<int32_t> h_nframes((size_t)(n), 0);
    std::vector<uint8_t> h_fin((size_t)(n), 0);
    std::vector<int> reported((size_t)(n), 0);
    int launched = 0;
    const bool fixed_len = sp.force_frames > 0 || dbg;
    // Frames are enqueued in bursts with at most two bursts in flight (event ring), so the AQL queue never fills:
    // a host thread blocked on queue back-pressure starves the other lanes' submissions (measured: lanes gave no
    // speed-up until the depth was bounded). Variable-length runs also poll the finished flags once per burst.
    const int burst_frames = std::max(1, max_inflight_frames / job_chains / 2);
    hipEvent_t ring[2] = {burst_ev_[0], burst_ev_[1]};
    int bursts = 0;
    bool done = false;
    while (!done && launched < frames_cap) {
        if (bursts >= 2) Q3_HIP(hipEventSynchronize(ring[bursts & 1]));  // burst (bursts-2) has drained
        int burst = std::min(burst_frames, frames_cap - launched);
        if (sd.on) {
            // a burst ends where the next chunk becomes decodable (its frames + the lookahead), so the chunk is issued behind
            // exactly the frames it needs instead of behind the rest of a full burst (first audio 139 -> 115 ms at 1.7B / batch 32)
            const int need = std::min(frames_cap, sd.next_need(launched, sp.audio_chunk_frames, std::max(0, sp.audio_lookahead_frames)));
            if (need > launched) burst = std::min(burst, need - launched);
        }
        for (int i = 0; i < burst; ++i) {
            if (use_graph) Q3_HIP(hipGraphLaunch(ge, st_));
            else enqueue_frame(n, dbg);
        }
        launched += burst;
        if (!(fixed_len && !cb)) {  // per-burst poll of the flags (async copies ordered after the burst)
            Q3_HIP(hipMemcpyAsync(h_nframes.data(), n_frames_, size_t(n) * 4, hipMemcpyDeviceToHost, st_));
            Q3_HIP(hipMemcpyAsync(h_fin.data(), finished_, size_t(n), hipMemcpyDeviceToHost, st_));
        }
        Q3_HIP(hipEventRecord(ring[bursts & 1], st_));
        ++bursts;
        if (fixed_len && !cb) {
            if (sd.on) {  // every row has exactly `launched` frames (nothing ends early)
                for (int b = 0; b < n; ++b) sd.avail[size_t(b)] = std::min(launched, rr[size_t(b)].max_frames);
                sd.feed(launched);
            }
            continue;
        }
        Q3_HIP(hipEventSynchronize(ring[(bursts - 1) & 1]));
        done = true;
        for (int b = 0; b < n; ++b) done = done && h_fin[size_t(b)];
        if (sd.on) {
            for (int b = 0; b < n; ++b) {
                sd.avail[size_t(b)] = h_nframes[size_t(b)];
                sd.fin[size_t(b)] = h_fin[size_t(b)];
            }
            sd.feed(launched);
            fire_chunks(J, J.n_chunks, &sd.avail, false);  // what has already landed on the host, without waiting
        }
        if (cb)  // .token events in generation order (Qwen3+Streaming.swift:24-27)
            for (int b = 0; b < n; ++b) emit_tokens(cb, user, b, request_base + b, h_nframes[size_t(b)], reported[size_t(b)]);
    }
    Q3_HIP(hipEventRecord(ev_[2], st_));
    Q3_HIP(hipMemcpyAsync(h_nframes.data(), n_frames_, size_t(n) * 4, hipMemcpyDeviceToHost, st_));
    Q3_HIP(hipStreamSynchronize(st_));
    if (dbg) {
        const TalkerConfig& t = m_->cfg.talker;
        const size_t nf = size_t(n) * dbg->frames;
        if (dbg->sampled) Q3_HIP(hipMemcpy(dbg->sampled, sampled_dev_, nf * 16 * 4, hipMemcpyDeviceToHost));
        if (dbg->talker_logits) Q3_HIP(hipMemcpy(dbg->talker_logits, tl_dump_, nf * t.vocab_size * 2, hipMemcpyDeviceToHost));
        if (dbg->cp_logits)
            Q3_HIP(hipMemcpy(dbg->cp_logits, cl_dump_, nf * (t.num_code_groups - 1) * t.cp.vocab_size * 2, hipMemcpyDeviceToHost));
    }
    J.frames.assign(h_nframes.begin(), h_nframes.end());
    return launched;
}

// ---- hand the codes to the codec decoder (Qwen3.swift:943-961) on its own stream ----
void Engine::hand_off(Job& J, const std::vector<ResolvedRequest>& rr, StreamedDecode& sd, int launched, bool overlapped) {
    const int n = J.n;
    bool any_clone = false;
    std::vector<int> dframes((size_t)(n), 0);  // frames the decoder sees per row: [reference ++] generated (:1176-1186)
    int Fdec = 0;
    for (int b = 0; b < n; ++b) {
        const int F = J.frames[size_t(b)];
        any_clone = any_clone || rr[size_t(b)].clone;
        J.ref_T[size_t(b)] = rr[size_t(b)].clone ? rr[size_t(b)].ref_T : 0;
        J.target_tokens[size_t(b)] = rr[size_t(b)].target_token_count;
        dframes[size_t(b)] = F > 0 ? F + J.ref_T[size_t(b)] : 0;
        Fdec = std::max(Fdec, dframes[size_t(b)]);
    }
    J.Fdec = sd.on ? (sd.ss ? sd.stride : Fcap_) : Fdec;  // (a streamed job's row stride was fixed before its lengths were known)
    J.codes_host.resize(size_t(n) * Fcap_ * 16);
    Q3_HIP(hipMemcpyAsync(J.codes_host.data(), codes_, J.codes_host.size() * 4, hipMemcpyDeviceToHost, st_));
    if (sd.on) {  // the remaining chunks: every row is final now
        for (int b = 0; b < n; ++b) {
            sd.avail[size_t(b)] = J.frames[size_t(b)];
            sd.fin[size_t(b)] = 1;
        }
        sd.feed(launched);
        if (sd.ss) sd.finish_prefixed();
        else codec_->stream_close(J.nf_host);
        Q3_HIP(hipStreamSynchronize(st_));
        Q3_HIP(hipEventRecord(J.ev_codec[1], sd.sst));
        J.decoded = Fdec > 0;
        return;
    }
    if (Fdec > 0) {
        // The decoder reads a copy owned by the job: the next begin() overwrites codes_ while this decode may still run.
        J.dec_codes.grow(size_t(n) * Fdec * 16);
        if (any_clone) {  // every row in one launch: [reference ++] generated. Frames behind a row's own are not written (nor were
                          // they by the per-row launches before): the decoder is given dframes and reads nothing beyond them
            J.row_desc.assign(size_t(n), DecodeRowDesc{});
            for (int b = 0; b < n; ++b) {
                const auto& r = rr[size_t(b)];
                if (J.frames[size_t(b)] == 0) continue;  // (F == 0: the row's descriptor writes nothing)
                J.row_desc[size_t(b)] = DecodeRowDesc{r.clone ? ref_codes_dev_ + r.ref_off : nullptr, codes_ + size_t(b) * Fcap_ * 16,
                                                      r.clone ? r.ref_T : 0, J.frames[size_t(b)], b, 0};
                if (r.voice) {
                    J.ref_code0[size_t(b)] = r.voice->code0;
                } else if (r.clone) {
                    J.ref_code0[size_t(b)].resize(size_t(r.ref_T));
                    Q3_HIP(hipMemcpyAsync(J.ref_code0[size_t(b)].data(), ref_codes_dev_ + r.ref_off, size_t(r.ref_T) * 4,
                                          hipMemcpyDeviceToHost, st_));
                }
            }
            Q3_HIP(hipMemcpyAsync(J.row_desc_dev.grow(size_t(n)), J.row_desc.data(), size_t(n) * sizeof(DecodeRowDesc), hipMemcpyHostToDevice, st_));
            launch_build_decode_codes_rows(J.row_desc.data(), J.row_desc_dev, n, J.dec_codes, n, Fdec, st_);
        } else {
            Q3_HIP(hipMemcpy2DAsync(J.dec_codes, size_t(Fdec) * 64, codes_, size_t(Fcap_) * 64, size_t(Fdec) * 64, size_t(n),
                                    hipMemcpyDeviceToDevice, st_));
        }
    }
    Q3_HIP(hipStreamSynchronize(st_));  // everything of this call on st_ is done; only the decode is still to come
    start_decode(J, dframes, overlapped, nullptr);
}

void Engine::start_decode(Job& J, const std::vector<int>& dframes, bool overlapped, const int32_t* codes_host) {
    hipStream_t cst = codec_stream(overlapped, J.background);
    Q3_HIP(hipEventRecord(J.ev_codec[0], cst));
    if (J.Fdec > 0) {
        const size_t floats = size_t(J.n) * J.Fdec * J.up;
        J.pcm_host.grow(floats);
        if (codes_host && J.voices.empty()) {
            J.dec_codes.grow(size_t(J.n) * J.Fdec * 16);
            Q3_HIP(hipMemcpy2DAsync(J.dec_codes, size_t(J.Fdec) * 64, codes_host, size_t(Fcap_) * 64, size_t(J.Fdec) * 64, size_t(J.n),
                                    hipMemcpyHostToDevice, cst));
        } else if (codes_host) {
            // Rows with a reference in front: J.Fdec may exceed Fcap_, the stride of codes_host. The generated codes are staged
            // as they lie on the host; one launch then writes every row behind its voice's reference frames, read from the voice.
            J.dec_codes.grow(size_t(J.n) * J.Fdec * 16);
            // (the builder writes a row's own frames only; what lies behind them is zero, as after the 2-D upload of the zeroed
            // codes_host above, although CodecRunner::decode is given dframes and reads no frame of a row beyond them)
            Q3_HIP(hipMemsetAsync(J.dec_codes, 0, size_t(J.n) * J.Fdec * 64, cst));
            J.gen_codes.grow(size_t(J.n) * Fcap_ * 16);
            int Fgen = 0;
            for (int b = 0; b < J.n; ++b) Fgen = std::max(Fgen, J.frames[size_t(b)]);
            Q3_CHECK(Fgen <= Fcap_, 7, "internal error: more generated frames than max_frames");
            Q3_HIP(hipMemcpy2DAsync(J.gen_codes, size_t(Fcap_) * 64, codes_host, size_t(Fcap_) * 64, size_t(Fgen) * 64, size_t(J.n),
                                    hipMemcpyHostToDevice, cst));
            J.row_desc.assign(size_t(J.n), DecodeRowDesc{});
            for (int b = 0; b < J.n; ++b) {
                const Voice* v = J.voices[size_t(b)];
                J.row_desc[size_t(b)] = DecodeRowDesc{v ? static_cast<const int32_t*>(v->codes_dev) : nullptr,
                                                      J.gen_codes + size_t(b) * Fcap_ * 16, v ? v->ref_T : 0, J.frames[size_t(b)], b, 0};
            }
            Q3_HIP(hipMemcpyAsync(J.row_desc_dev.grow(size_t(J.n)), J.row_desc.data(), size_t(J.n) * sizeof(DecodeRowDesc),
                                  hipMemcpyHostToDevice, cst));
            launch_build_decode_codes_rows(J.row_desc.data(), J.row_desc_dev, J.n, J.dec_codes, J.n, J.Fdec, cst);
        }
        if (J.chunk_frames > 0) {
            // pre-transformer once over all frames, then the causal tail chunk by chunk (codec.h decode_chunked)
            J.clear_chunk_flags(J.Fdec);
            J.n_chunks = codec_->decode_chunked(J.dec_codes, J.Fdec, dframes, J.chunk_frames, J.pcm_host, J.chunk_done, J.nf_host,
                                                J.nf_chunk_host);
        } else {
            float* pcm_dev = nullptr;
            codec_->decode(J.dec_codes, J.Fdec, dframes, &pcm_dev, std::string(), nullptr, nullptr, nullptr, J.nf_host, false,
                           J.row_hs.empty() ? nullptr : J.row_hs.data());
            Q3_HIP(hipMemcpyAsync(J.pcm_host, pcm_dev, floats * 4, hipMemcpyDeviceToHost, cst));
        }
        J.decoded = true;
    }
    Q3_HIP(hipEventRecord(J.ev_codec[1], cst));
}

void Engine::job_timing(Job& J, const std::vector<int>& np, int launched) {
    float ms = 0;
    Q3_HIP(hipEventElapsedTime(&ms, ev_[0], ev_[1]));
    J.timing.prefill_ms = ms;
    Q3_HIP(hipEventElapsedTime(&ms, ev_[1], ev_[2]));
    J.timing.decode_ms = ms;
    Q3_HIP(hipEventElapsedTime(&ms, ev_fe_[0], ev_fe_[1]));
    J.timing.frontend_ms = J.frontend ? ms : 0;  // (a call whose references are all voices has no front end to time)
    J.timing.frame_steps = launched;
    J.timing.launches_per_frame_step = launches_per_step(J.n);
    J.timing.rows = J.n;
    for (int b = 0; b < J.n; ++b) J.timing.kv_bytes_read += kv_bytes(np[size_t(b)], J.frames[size_t(b)]);
}

void Engine::publish_job(Job& J, q3tts_event_cb cb, void* user, int req_base, double t_start, bool stage) {
    J.cb = cb;
    J.user = user;
    J.request_base = req_base;
    J.t_start = t_start;
    J.seq = job_seq_++;
    J.busy = true;
    compute_cuts(J);
    std::lock_guard<std::mutex> lk(stage_mu_);
    J.stage_err.clear();
    J.stage = (stage && J.decoded) ? 1 : 0;
    if (J.stage == 1) {
        if (!stager_.joinable()) stager_ = std::thread([this] { staging_loop(); });
        stage_cv_.notify_all();
    }
}

void Engine::release_job(Job& J) {
    {   // a staging thread may still be copying into the rows
        std::unique_lock<std::mutex> lk(stage_mu_);
        stage_cv_.wait(lk, [&] { return J.stage != 1; });
    }
    J.st_pcm.clear();  // frees every row not handed over to a result
    J.st_codes.clear();
    J.back_status = 0;
    J.busy = false;
}

void Engine::Job::reset(int rows, int upsample) {
    n = rows;
    up = upsample;
    row_hs.clear();
    row_up.assign(size_t(n), upsample);
    Fdec = 0;
    frames.assign(size_t(n), 0);
    ref_T.assign(size_t(n), 0);
    target_tokens.assign(size_t(n), 0);
    ref_code0.assign(size_t(n), {});
    req_index.clear();  // (a queued call's decode batches used the slot with request indices of their own)
    row_out.clear();
    row_span.clear();
    held_from.assign(size_t(n), -1);
    std::memset(nf_host, 0, nf_host.capacity() * 4);
    n_chunks = chunk_frames = chunks_fired = 0;
    streamed = prefixed = decoded = background = frontend = false;
    voices.clear();
    t_first_audio = t_done = 0;
    timing = q3tts_timing{};
}

// the rows' non-finite flags behind every chunk of a decode in pieces (fire_chunks holds a row back from its first flagged chunk)
void Engine::Job::clear_chunk_flags(int frames) {
    const size_t slots = size_t(ceil_div(frames, chunk_frames) + 1) * size_t(n);
    std::memset(nf_chunk_host.grow(slots), 0, slots * 4);
}

void Engine::set_row_speeds(Job& J, const std::vector<int>& hs) {
    bool any = false;
    for (int h : hs) any = any || h != 0;
    if (!any) return;
    J.up = codec_->max_upsample();
    J.row_hs.assign(size_t(J.n), codec_->stretch_hs());
    for (int b = 0; b < J.n; ++b) {
        if (hs[size_t(b)] != 0) J.row_hs[size_t(b)] = hs[size_t(b)];
        J.row_up[size_t(b)] = codec_->upsample_of(J.row_hs[size_t(b)]);
    }
}

void check_row_sampling(const q3tts_sampling& sp, int n) {
    if (!sp.per_request) return;
    constexpr uint32_t kKnown = Q3TTS_ROW_TEMPERATURE | Q3TTS_ROW_TOP_K | Q3TTS_ROW_TOP_P | Q3TTS_ROW_REPETITION_PENALTY | Q3TTS_ROW_SEED;
    for (int i = 0; i < n; ++i) {
        const q3tts_row_sampling& r = sp.per_request[i];
        const std::string at = " (per_request[" + std::to_string(i) + "])";
        Q3_CHECK((r.set & ~kKnown) == 0, 3, "Invalid input: unknown bits in q3tts_row_sampling.set" + at);
        if (r.set & Q3TTS_ROW_TEMPERATURE) Q3_CHECK(std::isfinite(r.temperature), 3, "Invalid input: temperature must be finite" + at);
        if (r.set & Q3TTS_ROW_TOP_K) Q3_CHECK(r.top_k >= 0, 3, "Invalid input: top_k must not be negative" + at);
        if (r.set & Q3TTS_ROW_TOP_P)
            Q3_CHECK(std::isfinite(r.top_p) && r.top_p >= 0.f && r.top_p <= 1.f, 3, "Invalid input: top_p must be in [0, 1]" + at);
        if (r.set & Q3TTS_ROW_REPETITION_PENALTY)
            Q3_CHECK(std::isfinite(r.repetition_penalty) && r.repetition_penalty > 0.f, 3,
                     "Invalid input: repetition_penalty must be finite and positive" + at);
    }
}

SamplingParams fold_sampling(const q3tts_sampling& sp, int i, uint32_t row0) {
    SamplingParams o{sp.temperature, sp.top_k, sp.top_p, sp.repetition_penalty, sp.seed, row0, sp.force_frames > 0 ? 1 : 0};
    if (!sp.per_request) return o;
    const q3tts_row_sampling& r = sp.per_request[i];
    if (r.set & Q3TTS_ROW_TEMPERATURE) o.temperature = r.temperature;
    if (r.set & Q3TTS_ROW_TOP_K) o.top_k = r.top_k;
    if (r.set & Q3TTS_ROW_TOP_P) o.top_p = r.top_p;
    if (r.set & Q3TTS_ROW_REPETITION_PENALTY) o.rep_penalty = r.repetition_penalty;
    if (r.set & Q3TTS_ROW_SEED) o.seed = r.seed;
    return o;
}

void Engine::upload_sampling(const q3tts_sampling& sp, uint32_t row0, int n) {
    std::vector<SamplingParams> h;
    for (int b = 0; b < n; ++b) h.push_back(fold_sampling(sp, b, row0));
    Q3_HIP(hipMemcpyAsync(sp_dev_, h.data(), h.size() * sizeof(SamplingParams), hipMemcpyHostToDevice, st_));
}

int64_t Engine::kv_bytes(int n_prompt, int frames) const {
    const TalkerConfig& t = m_->cfg.talker;
    const int64_t per_tok = int64_t(t.num_hidden_layers) * t.num_key_value_heads * kHeadDim * 2 * 2;
    int64_t kvb = 0;
    for (int f = 0; f < frames; ++f) kvb += int64_t(n_prompt - 1 + f) * per_tok;
    return kvb;
}

int Engine::launches_per_step(int B) const {
    auto fl = frame_launches_.find(B);
    return fl == frame_launches_.end() ? 0 : fl->second;
}

std::unique_lock<std::mutex> Engine::cb_lock() {
    return cb_mutex ? std::unique_lock<std::mutex>(*cb_mutex) : std::unique_lock<std::mutex>();
}

void Engine::emit_tokens(q3tts_event_cb cb, void* user, int row, int request, int nf, int& reported) {
    if (nf <= reported) return;
    std::vector<int32_t> tmp((size_t)(nf - reported) * 16);
    Q3_HIP(hipMemcpy(tmp.data(), codes_ + (size_t(row) * Fcap_ + reported) * 16, tmp.size() * 4, hipMemcpyDeviceToHost));
    std::unique_lock<std::mutex> lk = cb_lock();
    for (int f = 0; f < nf - reported; ++f) {
        q3tts_event ev{};
        ev.kind = Q3TTS_EVENT_TOKEN;
        ev.request_index = request;
        ev.token = tmp[size_t(f) * 16];
        cb(user, &ev);
    }
    reported = nf;
}

// samples [cut, cut + ns) of row b's decoded stream are its audio: audioLengths = count(code0 > 0) * 1920, trimmed when
// 0 < valid < len (SpeechTokenizer.swift:831-833, Qwen3.swift:954-959); clone rows lose the reference's share
// (Qwen3.swift:1195-1199, Float arithmetic)
void Engine::compute_cuts(Job& J) {
    const int n = J.n;
    J.row_cut.assign(size_t(n), 0);
    J.row_ns.assign(size_t(n), 0);
    for (int b = 0; b < n; ++b) {
        const int F = J.frames[size_t(b)], up = J.row_up[size_t(b)];  // (the row's own samples per frame)
        if (F == 0 || !J.decoded) continue;
        const int32_t* codes = J.codes_host.data() + size_t(b) * Fcap_ * 16;
        int valid_tok = 0;
        for (int f = 0; f < F; ++f) valid_tok += codes[size_t(f) * 16] > 0 ? 1 : 0;
        for (int32_t c : J.ref_code0[size_t(b)]) valid_tok += c > 0 ? 1 : 0;
        const int ref_T = J.ref_T[size_t(b)], total_f = ref_T + F;
        int64_t ns = int64_t(total_f) * up;
        const int64_t valid = int64_t(valid_tok) * up;
        // (a streamed row has already delivered its chunks frame by frame when the count becomes known: its AUDIO is their
        // concatenation, untrimmed -- include/q3tts.h)
        if (!J.streamed && valid > 0 && valid < ns) ns = valid;
        int64_t cut = 0;
        if (J.prefixed) {
            // a clone row streamed behind its reference: the samples of its own frames, cut exactly (the Float proportion
            // below needs the final length, which is not known when the first chunk leaves)
            cut = int64_t(ref_T) * up;
        } else if (ref_T > 0) {
            cut = int64_t(float(ref_T) / float(std::max(total_f, 1)) * float(ns));
            if (!(cut > 0 && cut < ns)) cut = 0;
        }
        J.row_cut[size_t(b)] = cut;
        J.row_ns[size_t(b)] = ns - cut;
    }
}

// AUDIO_CHUNK events of chunks [J.chunks_fired, upto). known == nullptr: the rows' final cuts (compute_cuts) bound the pieces;
// otherwise row b has known[b] frames so far and nothing is cut in front (a streamed job, still inside its frame loop).
// wait = false delivers only what has already landed on the host.
void Engine::fire_chunks(Job& J, int upto, const std::vector<int>* known, bool wait) {
    const int n = J.n, up = J.up;
    for (int k = J.chunks_fired; k < upto; ++k) {
        if (wait) {
            Q3_HIP(hipEventSynchronize(J.chunk_done[size_t(k)]));
        } else {
            const hipError_t q = hipEventQuery(J.chunk_done[size_t(k)]);
            if (q == hipErrorNotReady) return;
            Q3_HIP(q);
        }
        J.chunks_fired = k + 1;
        if (J.nf_chunk_host)  // a row that has left the fp16 range delivers nothing more until end() has decoded it again
            for (int b = 0; b < n; ++b)
                if (J.held_from[size_t(b)] < 0 && J.nf_chunk_host[size_t(k) * n + b]) J.held_from[size_t(b)] = k;
        if (!J.cb) continue;
        const int64_t c0 = int64_t(k) * J.chunk_frames * up, c1 = std::min<int64_t>(int64_t(J.Fdec), int64_t(k + 1) * J.chunk_frames) * up;
        std::unique_lock<std::mutex> lk = cb_lock();
        for (int b = 0; b < n; ++b) {
            if (J.held_from[size_t(b)] >= 0) continue;
            const int64_t cut = known ? 0 : J.row_cut[size_t(b)];
            const int64_t len = known ? int64_t((*known)[size_t(b)]) * up : J.row_ns[size_t(b)];
            const int64_t lo = std::max(c0, cut), hi = std::min(c1, cut + len);
            if (hi <= lo) continue;
            audio_chunk(J.cb, J.user, J.request_base + b, J.pcm_host + size_t(b) * J.Fdec * up + lo, hi - lo, lo - cut);
        }
    }
}

void Engine::stage_rows(Job& J) {
    Q3_HIP(hipSetDevice(m_->device));
    Q3_HIP(hipEventSynchronize(J.ev_codec[1]));
    J.t_done = now_s();  // the job's own completion, not the moment end() happens to be called (a pipelined job's end()
                         // comes after the NEXT batch's whole frame loop)
    const int n = J.n;
    J.st_pcm.clear();
    J.st_pcm.resize(size_t(n));
    J.st_codes.clear();
    J.st_codes.resize(size_t(n));
    for (int b = 0; b < n; ++b) {
        const int F = J.frames[size_t(b)];
        if (F == 0 || !J.decoded) continue;
        const int64_t ns = J.row_ns[size_t(b)];
        J.st_codes[size_t(b)].reset(static_cast<int32_t*>(std::malloc(size_t(F) * 16 * 4)));
        J.st_pcm[size_t(b)].reset(static_cast<float*>(std::malloc(std::max<size_t>(size_t(ns) * 4, 4))));
        Q3_CHECK(J.st_codes[size_t(b)] && J.st_pcm[size_t(b)], 5, "out of host memory for the results");
        std::memcpy(J.st_codes[size_t(b)].get(), J.codes_host.data() + size_t(b) * Fcap_ * 16, size_t(F) * 16 * 4);
        std::memcpy(J.st_pcm[size_t(b)].get(), J.pcm_host + size_t(b) * J.Fdec * J.up + J.row_cut[size_t(b)], size_t(ns) * 4);
    }
}

void Engine::staging_loop() {
    std::unique_lock<std::mutex> lk(stage_mu_);
    for (;;) {
        Job* next = nullptr;
        for (auto& J : jobs_)
            if (J.stage == 1 && (!next || J.seq < next->seq)) next = &J;
        if (!next) {
            if (stage_stop_) return;
            stage_cv_.wait(lk);
            continue;
        }
        lk.unlock();
        int state = 2;
        std::string err;
        try {
            stage_rows(*next);
        } catch (const std::exception& e) {
            state = 3;
            err = e.what();
        }
        lk.lock();
        next->stage = state;
        next->stage_err = err;
        stage_cv_.notify_all();
    }
}

// The default codec kernels contract on the fp16 matrix cores (two planes per fp32 operand, codec_conv.hip): an activation
// beyond 65504 turns into inf / NaN, which out_conv flags per row. The reference computes in fp32 and decodes such inputs, so a
// flagged row is decoded AGAIN here on the fp32 matrix cores (the fp32 weights stay resident; 2.4x the time, for those rows
// only) and handed out like any other. A streamed row (audio_window_frames > 0) stopped delivering chunks at its first flagged
// one (fire_chunks): its remaining AUDIO_CHUNK events come from this decode -- the exact one-shot arithmetic -- and its AUDIO
// is what was delivered. Returns the rows that are non-finite even in fp32 (they fail with AUDIO_DECODING_FAILED).
Engine::ExactDecode Engine::decode_rows_fp32(const std::vector<int>& dframes, const std::function<void(int, int32_t*, hipStream_t)>& place,
                                             const std::vector<int>* hs) {
    const int R = int(dframes.size()), up = hs ? codec_->max_upsample() : codec_->upsample();
    ExactDecode d;
    d.up = up;
    for (int f : dframes) d.Fd = std::max(d.Fd, f);
    hipStream_t cst = codec_stream(false);
    DevBuf<int32_t> dcodes;
    dcodes.grow(size_t(R) * d.Fd * 16);
    std::memset(d.nf.grow(size_t(R)), 0, size_t(R) * 4);
    d.pcm.grow(size_t(R) * d.Fd * up);
    for (int i = 0; i < R; ++i) place(i, dcodes + size_t(i) * d.Fd * 16, cst);
    float* pcm_dev = nullptr;
    codec_->decode(dcodes, d.Fd, dframes, &pcm_dev, std::string(), nullptr, nullptr, nullptr, d.nf, true, hs ? hs->data() : nullptr);
    Q3_HIP(hipMemcpyAsync(d.pcm, pcm_dev, size_t(R) * d.Fd * up * 4, hipMemcpyDeviceToHost, cst));
    Q3_HIP(hipStreamSynchronize(cst));
    return d;
}

void Engine::refire_held(float* own, const float* src, int64_t at, int64_t ns, int64_t step, q3tts_event_cb cb, void* user, int index) {
    std::memcpy(own + at, src + at, size_t(ns - at) * 4);
    if (!cb) return;
    std::unique_lock<std::mutex> lk = cb_lock();
    for (int64_t lo = at; lo < ns; lo += step) audio_chunk(cb, user, index, own + lo, std::min(step, ns - lo), lo);
}

std::vector<int> Engine::redo_rows_fp32(Job& J) {
    std::vector<int> rows, bad;
    if (!J.decoded) return bad;
    for (int b = 0; b < J.n; ++b)
        if (J.nf_host[b] && J.frames[size_t(b)] > 0 && J.st_pcm[size_t(b)]) rows.push_back(b);
    if (rows.empty()) return bad;
    if (codec_->fp32_convs()) return rows;  // already the fp32 kernels: nothing wider to fall back to
    const int R = int(rows.size()), up = J.up;  // (the layout's samples per frame: the re-decode's is the job's)
    std::vector<int> dframes((size_t)(R)), hs;
    for (int i = 0; i < R; ++i) dframes[size_t(i)] = J.frames[size_t(rows[size_t(i)])] + J.ref_T[size_t(rows[size_t(i)])];
    if (!J.row_hs.empty())  // every row is decoded again at its own speed
        for (int b : rows) hs.push_back(J.row_hs[size_t(b)]);
    // the codes the first decode read: the job's own device copy ([reference ++] generated; row stride J.Fdec frames)
    const ExactDecode d = decode_rows_fp32(dframes, [&J, &rows, &dframes](int i, int32_t* dst, hipStream_t cst) {
        Q3_HIP(hipMemcpyAsync(dst, J.dec_codes + size_t(rows[size_t(i)]) * J.Fdec * 16, size_t(dframes[size_t(i)]) * 64,
                              hipMemcpyDeviceToDevice, cst));
    }, hs.empty() ? nullptr : &hs);
    const int Fd = d.Fd;
    const float* hpcm = d.pcm;
    for (int i = 0; i < R; ++i) {
        const int b = rows[size_t(i)];
        if (d.nf[i]) {
            bad.push_back(b);
            continue;
        }
        // decoded-stream coordinates: sample p of the decode is sample p - cut of the row's audio; chunk k covers
        // [k * step, (k + 1) * step). Chunks below `held` have been delivered from the first decode and stay as they are.
        const int64_t cut = J.row_cut[size_t(b)], ns = J.row_ns[size_t(b)];
        const int64_t step = int64_t(std::max(J.chunk_frames, 1)) * (J.prefixed ? J.row_up[size_t(b)] : up);
        if (J.prefixed) {  // chunks count from the row's own first frame: chunk k is samples [k * step, (k + 1) * step) of its audio
            refire_held(J.st_pcm[size_t(b)].get(), hpcm + size_t(i) * Fd * up + cut, std::min(ns, int64_t(std::max(0, J.held_from[size_t(b)])) * step),
                        ns, step, J.cb, J.user, J.request_base + b);
            continue;
        }
        const int held = J.n_chunks > 0 ? std::max(0, J.held_from[size_t(b)]) : 0;
        const int64_t from = J.n_chunks > 0 ? std::min(ns, std::max<int64_t>(0, int64_t(held) * step - cut)) : 0;
        float* pcm = J.st_pcm[size_t(b)].get();
        std::memcpy(pcm + from, hpcm + size_t(i) * Fd * up + cut + from, size_t(ns - from) * 4);
        if (J.cb && J.n_chunks > 0) {  // the pieces fire_chunks held back
            std::unique_lock<std::mutex> lk = cb_lock();
            for (int k = held; k < J.n_chunks; ++k) {
                const int64_t lo = std::max(int64_t(k) * step, cut), hi = std::min(int64_t(k + 1) * step, cut + ns);
                if (hi > lo) audio_chunk(J.cb, J.user, J.request_base + b, pcm + (lo - cut), hi - lo, lo - cut);
            }
        }
    }
    return bad;
}


void Engine::end(int job, q3tts_result* results) {
    Q3_CHECK(job >= 0 && job < kJobSlots && jobs_[job].busy, 3, "Invalid input: no such outstanding job");
    Job& J = jobs_[job];
    // Whatever happens below, the slot is released and rows staged for it are freed: a failure inside end() must not
    // leave the handle with a job nobody can end (q3tts_generate_end has already dropped the caller's handle by then).
    struct Release {
        Engine* e;
        Job* j;
        ~Release() { e->release_job(*j); }
    } release{this, &J};
    Q3_HIP(hipSetDevice(m_->device));
    {   // a back half on the worker thread: wait for it; what it threw is reported here, with its status
        std::unique_lock<std::mutex> lk(work_mu_);
        work_cv_.wait(lk, [&] { return J.back == 0; });
        if (J.back_status) throw Error(J.back_status, J.back_err);
    }
    const int n = J.n;
    const std::vector<int64_t>& row_ns = J.row_ns;
    if (J.n_chunks > 0) fire_chunks(J, J.n_chunks, nullptr, true);  // AUDIO_CHUNK events not delivered inside the loop
    {
        std::unique_lock<std::mutex> lk(stage_mu_);
        stage_cv_.wait(lk, [&] { return J.stage != 1; });
    }
    if (J.stage == 0) {
        try {
            stage_rows(J);
            J.stage = 2;
        } catch (const std::exception& e) {
            J.stage = 3;
            J.stage_err = e.what();
        }
    }
    if (J.stage == 3) throw Error(5, J.stage_err);
    // rows whose activations left the fp16 range of the default codec kernels: once more on the fp32 matrix cores
    const std::vector<int> still_bad = redo_rows_fp32(J);
    float ms = 0;
    Q3_HIP(hipEventElapsedTime(&ms, J.ev_codec[0], J.ev_codec[1]));
    J.timing.codec_ms = ms;  // on the codec stream: includes whatever the next batch's AR loop took away from it
    if (J.streamed && J.n_chunks > 0) {
        Q3_HIP(hipEventElapsedTime(&ms, J.ev_begin, J.ev_first_audio));
        J.timing.first_audio_ms = ms;
    }
    timing = J.timing;
    const double job_total = (J.t_done > 0 ? J.t_done : now_s()) - J.t_start;
    const double memory_gb = device_memory_gb();
    // a queued decode batch: row b is request req_index[b], timed from its admission to its retirement
    auto out = [&](int b) -> q3tts_result& { return J.row_out.empty() ? results[b] : *J.row_out[size_t(b)]; };
    for (int b = 0; b < n; ++b) {
        q3tts_result& r = out(b);
        const int F = J.frames[size_t(b)];
        fill_info(r, J.target_tokens[size_t(b)], F, J.row_span.empty() ? job_total : J.row_span[size_t(b)], memory_gb);
        if (F == 0 || !J.decoded) {  // Qwen3.swift:939-941
            r.status = Q3TTS_ERR_GENERATION_FAILED;
            continue;
        }
        if (std::find(still_bad.begin(), still_bad.end(), b) != still_bad.end()) {  // never hand out a waveform with holes in it
            r.status = Q3TTS_ERR_AUDIO_DECODING_FAILED;
            last_error = kCodecRangeMsg;
            continue;
        }
        r.n_frames = F;
        r.codes = J.st_codes[size_t(b)].release();  // ownership passes to the result (q3tts_result_free)
        r.n_samples = row_ns[size_t(b)];
        r.pcm = J.st_pcm[size_t(b)].release();
        r.status = Q3TTS_OK;
    }
    if (J.cb) {
        std::unique_lock<std::mutex> lk = cb_lock();
        for (int b = 0; b < n; ++b)
            if (out(b).status == Q3TTS_OK) emit_info_audio(J.cb, J.user, J.request_base + (J.req_index.empty() ? b : J.req_index[size_t(b)]), out(b));
    }
}

bool Engine::job_outstanding() const {
    for (const auto& J : jobs_)
        if (J.busy) return true;
    return false;
}

}  // namespace q3
