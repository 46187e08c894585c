// engine.cc -- generation driver. See engine.h.
#include "engine.h"

#include <algorithm>
#include <cctype>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <deque>
#include <functional>
#include <thread>

#include "codec.h"
#include "codec_kernels.h"
#include "frontend.h"

namespace q3 {

namespace {
std::string lower(const std::string& s) {
    std::string o = s;
    for (auto& c : o) c = char(std::tolower((unsigned char)c));
    return o;
}
const char* const kCodecRangeMsg =
    "Audio decoding failed: the codec decoder produced a non-finite waveform -- also on the fp32 matrix-core convolutions (the "
    "reference's range), which a row is re-decoded on when it leaves the fp16 range of the default two-plane kernels";
double now_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
struct Bump {
    uint8_t* base;
    size_t off = 0;
    template <class T>
    T* take(size_t n) {
        off = align_up(off, 256);
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += n * sizeof(T);
        return p;
    }
};
// one AUDIO_CHUNK event: n samples at pcm, sample `offset` of the request's audio (the caller holds Engine::cb_lock)
void audio_chunk(q3tts_event_cb cb, void* user, int request_index, const float* pcm, int64_t n, int64_t offset) {
    q3tts_event ev{};
    ev.kind = Q3TTS_EVENT_AUDIO_CHUNK;
    ev.request_index = request_index;
    ev.pcm = pcm;
    ev.n_samples = n;
    ev.sample_offset = offset;
    cb(user, &ev);
}
}  // namespace

Engine::Engine(Model* model, const q3tts_load_opts& opts) : m_(model), opts_(opts) {
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
    if (m_->has_codec) codec_ = std::make_unique<CodecRunner>(*m_, st_codec_, opts.codec_fp32 != 0, opts.output_sample_rate, opts.speed);
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
    v->codes_dev.grow(size_t(16) * T);
    v->rows_dev.grow(size_t(1 + T) * H);
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

// The audio side of a streamed queue: one slotted codec stream (codec.h) over the queue's slots on the confined codec stream,
// the passes in flight, and every request's PCM as its chunks land. A request is complete once it has been retired and its
// last chunk has been taken from the ring.
struct Engine::SlotStream {
    Engine& e;
    hipStream_t cst = nullptr;
    const int C, up;
    bool hold = true;  // a request stops taking chunks at its first one flagged non-finite (the engine re-decodes it in fp32)
    struct Out {       // one request
        MallocPtr<float> pcm;  // [cap frames * up]
        int frames = -1;       // its length, once retired
        int landed = 0;        // chunks taken from the ring
        int held_from = -1;    // first chunk held back
        bool complete = false;
        bool dropped = false;  // cancelled (a session): its chunks in flight land nowhere
    };
    std::unordered_map<int, Out> out;  // by request (its index in a closed call, its ticket in a session)
    std::vector<int> req_of_row;  // the request in row b, -1: none
    struct Flight {
        CodecRunner::SlotPass pass;
        std::vector<int> req;     // req_of_row when the pass was issued
    };
    std::deque<Flight> flights;
    std::vector<CodecRunner::SlotPass> issued;
    hipEvent_t ev_codes = nullptr, ev_pushed = nullptr;  // st_ -> cst: the codes are copied; cst -> st_: the last push has been read
    bool have_first = false;
    double codec_ms = 0, first_audio_ms = 0;
    double t_call = 0;  // host clock at the call's start (first_audio_ms counts from it); 0: not timed
    std::function<void(int, int, const float*, int64_t, int64_t)> on_chunk;  // request, chunk, samples, count, offset
    std::function<void(int)> on_complete;

    SlotStream(Engine& eng, int rows, int chunk, int window, int lookahead, int max_frames, bool overlapped, int max_prefix = 0)
        : e(eng), C(chunk), up(eng.codec_->upsample()), req_of_row(size_t(rows), -1) {
        for (hipEvent_t* ev : {&ev_codes, &ev_pushed}) Q3_HIP(hipEventCreateWithFlags(ev, hipEventDisableTiming));
        cst = e.codec_stream(overlapped);
        CodecRunner::StreamCfg cfg;
        cfg.rows = rows; cfg.chunk_frames = chunk; cfg.window = window; cfg.lookahead = lookahead; cfg.max_frames = max_frames;
        cfg.per_row = true;
        cfg.max_prefix = max_prefix;
        e.codec_->stream_open(cfg);
    }
    ~SlotStream() {  // whatever ends the call: the runner's stream is closed and nothing of it is still running
        if (e.codec_->streaming()) e.codec_->stream_close();
        (void)hipStreamSynchronize(cst);
        for (hipEvent_t ev : {ev_codes, ev_pushed})
            if (ev) (void)hipEventDestroy(ev);
    }
    // prefix: the reference frames in front of the row's codes (a streamed clone row); state: that prefix's saved tail state
    void admit(int row, int req, int cap_frames, int prefix = 0, const uint8_t* state = nullptr) {
        // on cst: behind the previous occupant's last chunk, in front of this one's first
        if (state) e.codec_->stream_load_row(row, prefix, state);
        else e.codec_->stream_reset_row(row, prefix);
        req_of_row[size_t(row)] = req;
        Out& o = out[req];
        o.pcm.reset(static_cast<float*>(std::malloc(std::max<size_t>(size_t(cap_frames) * up * 4, 4))));
        Q3_CHECK(o.pcm != nullptr, 5, "out of host memory for the results");
    }
    void check_complete(int req) {
        Out& o = out[req];
        if (o.complete || o.frames < 0 || o.landed < e.codec_->stream_chunks_of(o.frames)) return;
        o.complete = true;
        if (on_complete) on_complete(req);
    }
    // the oldest pass in flight, if it has landed (wait: whatever it takes): samples to the requests, ring slot given back
    bool take(bool wait) {
        if (flights.empty()) return false;
        Flight& f = flights.front();
        if (wait) {
            Q3_HIP(hipEventSynchronize(f.pass.done));
        } else {
            const hipError_t q = hipEventQuery(f.pass.done);
            if (q == hipErrorNotReady) return false;
            Q3_HIP(q);
        }
        float ms = 0;
        Q3_HIP(hipEventElapsedTime(&ms, f.pass.begun, f.pass.done));
        codec_ms += ms;
        if (!have_first && t_call > 0) {  // the first samples of any request are on the host
            first_audio_ms = (now_s() - t_call) * 1e3;
            have_first = true;
        }
        std::vector<int> touched;
        for (size_t b = 0; b < f.pass.rows.size(); ++b) {
            const RowPlan& r = f.pass.rows[b];
            if (!r.part || !r.emit) continue;  // (a chunk of a reference prefix delivers nothing)
            const int req = f.req[b];
            Out& o = out[req];
            if (o.dropped) continue;
            if (hold && o.held_from < 0 && f.pass.nf[b]) o.held_from = r.k;
            if (o.held_from < 0) {
                const int64_t off = int64_t(r.k) * C * up, n = int64_t(r.take) * up;
                std::memcpy(o.pcm.get() + off, f.pass.pcm + b * size_t(C) * up, size_t(n) * 4);
                if (on_chunk) on_chunk(req, r.k, o.pcm.get() + off, n, off);
            }
            ++o.landed;
            touched.push_back(req);
        }
        e.codec_->stream_release(f.pass.ring);
        flights.pop_front();
        for (int req : touched) check_complete(req);
        return true;
    }
    // every chunk that avail / fin now allow, on cst; a full ring is emptied from its oldest pass on
    void push(const int32_t* codes_dev, int code_stride_frames, const int* avail, const uint8_t* fin) {
        for (;;) {
            issued.clear();
            const bool more = e.codec_->stream_push_rows(codes_dev, code_stride_frames, avail, fin, issued);
            for (auto& p : issued) flights.push_back(Flight{std::move(p), req_of_row});
            if (!more) break;
            take(true);
        }
        Q3_HIP(hipEventRecord(ev_pushed, cst));
    }
    void retire(int row, int frames) {
        const int req = req_of_row[size_t(row)];
        req_of_row[size_t(row)] = -1;
        out[req].frames = frames;
        check_complete(req);
    }
    // the request in `row` is cancelled: the row is free (its next occupant resets it), what is in flight for it is dropped
    void drop(int row) {
        const int req = req_of_row[size_t(row)];
        req_of_row[size_t(row)] = -1;
        Out& o = out[req];
        o.dropped = true;
        o.pcm.reset();
    }
    bool in_flight(int req) const {
        for (const Flight& f : flights)
            for (size_t b = 0; b < f.pass.rows.size(); ++b)
                if (f.req[b] == req && f.pass.rows[b].part && f.pass.rows[b].emit) return true;
        return false;
    }
    void finish() {  // every pass taken, the runner's stream closed
        while (take(true)) {}
        e.codec_->stream_close();
        Q3_HIP(hipStreamSynchronize(cst));
    }
};

// A streamed decode (row f1): chunks of the waveform leave while the frame loop is still producing tokens.
struct Engine::StreamedDecode {
    Engine& e;
    Job& J;
    const bool on;
    hipStream_t sst = nullptr;
    std::vector<int> avail;    // frames of row b the decoder may read
    std::vector<uint8_t> fin;  // row b has all of its frames
    int copied = 0;            // frames [0, copied) of every row are in J.dec_codes
    // Clone rows streamed with their reference in front (q3tts_sampling.audio_stream_reference): the job's rows are the rows of
    // a slotted stream, each with its reference frames as prefix (none for a plain row); J.dec_codes holds ref ++ gen per row.
    std::unique_ptr<SlotStream> ss;
    std::vector<int> prefix;
    int stride = 0;  // frames per row of J.dec_codes and J.pcm_host

    StreamedDecode(Engine& eng, Job& job, bool streamed, const q3tts_sampling& sp, q3tts_event_cb cb, void* user,
                   const std::vector<ResolvedRequest>& rr, double t_start)
        : e(eng), J(job), on(streamed), avail(size_t(job.n), 0), fin(size_t(job.n), 0) {
        if (!on) return;
        J.cb = cb;         // fire_chunks delivers from inside the frame loop
        J.user = user;
        J.request_base = e.request_base;
        int ref_max = 0;
        bool any_clone = false;
        for (const auto& r : rr) {
            any_clone = any_clone || r.clone;
            if (r.clone) ref_max = std::max(ref_max, r.ref_T);
        }
        if (any_clone) {
            open_prefixed(sp, cb, user, rr, ref_max, t_start);
            return;
        }
        J.Fdec = e.Fcap_;  // row stride of the job's code and PCM buffers: the final lengths are not known yet
        J.dec_codes.grow(size_t(J.n) * e.Fcap_ * 16);
        J.pcm_host.grow(size_t(J.n) * e.Fcap_ * J.up);
        J.clear_chunk_flags(e.Fcap_);
        // the decode runs beside this batch's own frame loop: the confined stream, like a decode beside the next batch's
        sst = e.codec_stream(true);
        CodecRunner::StreamCfg cfg;
        cfg.rows = J.n; cfg.chunk_frames = sp.audio_chunk_frames; cfg.window = sp.audio_window_frames;
        cfg.lookahead = std::max(0, sp.audio_lookahead_frames); cfg.max_frames = e.Fcap_;
        Q3_HIP(hipEventRecord(J.ev_codec[0], sst));
        e.codec_->stream_open(cfg);
        J.streamed = true;
    }
    void open_prefixed(const q3tts_sampling& sp, q3tts_event_cb cb, void* user, const std::vector<ResolvedRequest>& rr, int ref_max,
                       double t_start) {
        stride = e.Fcap_ + ref_max;
        J.Fdec = stride;
        J.dec_codes.grow(size_t(J.n) * stride * 16);
        J.pcm_host.grow(size_t(J.n) * stride * J.up);
        ss = std::make_unique<SlotStream>(e, J.n, sp.audio_chunk_frames, sp.audio_window_frames, std::max(0, sp.audio_lookahead_frames),
                                          e.Fcap_, true, ref_max);
        sst = ss->cst;
        Q3_HIP(hipEventRecord(J.ev_codec[0], sst));
        ss->t_call = t_start;
        if (cb) {
            const int base = e.request_base;
            Engine* eng = &e;
            ss->on_chunk = [eng, cb, user, base](int req, int, const float* pcm, int64_t n, int64_t off) {
                std::unique_lock<std::mutex> lk = eng->cb_lock();
                audio_chunk(cb, user, base + req, pcm, n, off);
            };
        }
        // every clone row's reference frames to the front of its code row (the builder also moves one generated frame, which
        // does not exist yet: frame ref_T of the row, read by nothing before feed() has written it)
        prefix.assign(size_t(J.n), 0);
        J.row_desc.assign(size_t(J.n), DecodeRowDesc{});
        for (int b = 0; b < J.n; ++b) {
            const auto& r = rr[size_t(b)];
            if (!r.clone || r.ref_T <= 0) continue;
            prefix[size_t(b)] = r.ref_T;
            J.row_desc[size_t(b)] = DecodeRowDesc{e.ref_codes_dev_ + r.ref_off, e.codes_ + size_t(b) * e.Fcap_ * 16, r.ref_T, 1, b, 0};
        }
        Q3_HIP(hipMemcpyAsync(J.row_desc_dev.grow(size_t(J.n)), J.row_desc.data(), size_t(J.n) * sizeof(DecodeRowDesc), hipMemcpyHostToDevice,
                              e.st_));
        launch_build_decode_codes_rows(J.row_desc.data(), J.row_desc_dev, J.n, J.dec_codes, J.n, stride, e.st_);
        Q3_HIP(hipEventRecord(e.ev_[3], e.st_));
        Q3_HIP(hipStreamWaitEvent(sst, e.ev_[3], 0));
        for (int b = 0; b < J.n; ++b) ss->admit(b, b, e.Fcap_, prefix[size_t(b)]);
        ss->push(J.dec_codes, stride, avail.data(), fin.data());  // the prefixes need no generated frame: they start at once
        J.streamed = J.prefixed = true;
    }
    ~StreamedDecode() {  // an exception must not leave the runner's stream open
        ss.reset();
        if (on && e.codec_->streaming()) e.codec_->stream_close();
    }
    // the frame count at which the next chunk of a row that started with the job becomes decodable, given `launched` frame steps
    int next_need(int launched, int chunk, int lookahead) const {
        if (!ss) return (J.n_chunks + 1) * chunk + lookahead;
        const int k = launched < chunk + lookahead ? 0 : (launched - lookahead) / chunk;
        return (k + 1) * chunk + lookahead;
    }
    // frames [0, upto) of every row exist on the device once the copy below has run: hand them to the decoder, which issues
    // every chunk that avail / fin now allow
    void feed(int upto) {
        if (!on) return;
        if (ss) {
            if (upto > copied) {
                for (int b = 0; b < J.n; ++b)
                    Q3_HIP(hipMemcpyAsync(J.dec_codes + (size_t(b) * stride + prefix[size_t(b)] + copied) * 16,
                                          e.codes_ + (size_t(b) * e.Fcap_ + copied) * 16, size_t(upto - copied) * 64, hipMemcpyDeviceToDevice,
                                          e.st_));
                copied = upto;
                Q3_HIP(hipEventRecord(e.ev_[3], e.st_));
                Q3_HIP(hipStreamWaitEvent(sst, e.ev_[3], 0));
            }
            ss->push(J.dec_codes, stride, avail.data(), fin.data());
            while (ss->take(false)) {}  // what has already landed on the host leaves now
            return;
        }
        if (upto > copied) {
            Q3_HIP(hipMemcpy2DAsync(J.dec_codes + size_t(copied) * 16, size_t(e.Fcap_) * 64, e.codes_ + size_t(copied) * 16,
                                    size_t(e.Fcap_) * 64, size_t(upto - copied) * 64, size_t(J.n), hipMemcpyDeviceToDevice, e.st_));
            copied = upto;
            Q3_HIP(hipEventRecord(e.ev_[3], e.st_));
            Q3_HIP(hipStreamWaitEvent(sst, e.ev_[3], 0));
        }
        const int before = J.n_chunks;
        J.n_chunks = e.codec_->stream_push(J.dec_codes, e.Fcap_, avail.data(), fin.data(), J.pcm_host, size_t(e.Fcap_) * J.up,
                                           J.chunk_done, J.nf_chunk_host);
        if (before == 0 && J.n_chunks > 0) Q3_HIP(hipEventRecord(J.ev_first_audio, sst));  // behind chunk 0's copy to the host
    }
    // every row is final: the remaining chunks, then the rows' samples to where a decode of [reference ++ generated] has them
    void finish_prefixed() {
        for (int b = 0; b < J.n; ++b) ss->retire(b, J.frames[size_t(b)]);
        ss->finish();
        for (int b = 0; b < J.n; ++b) {
            const SlotStream::Out& o = ss->out[b];
            Q3_CHECK(o.complete, 7, "internal error: a row of the streamed job was left incomplete");
            std::memcpy(J.pcm_host + (size_t(b) * stride + prefix[size_t(b)]) * J.up, o.pcm.get(), size_t(J.frames[size_t(b)]) * J.up * 4);
            J.held_from[size_t(b)] = o.held_from;
            J.nf_host[b] = o.held_from >= 0 ? 1 : 0;
        }
        if (ss->have_first) J.timing.first_audio_ms = ss->first_audio_ms;
    }
};

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
            codec_->decode(J.dec_codes, J.Fdec, dframes, &pcm_dev, std::string(), nullptr, nullptr, nullptr, J.nf_host);
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
    const int n = J.n, up = J.up;
    J.row_cut.assign(size_t(n), 0);
    J.row_ns.assign(size_t(n), 0);
    for (int b = 0; b < n; ++b) {
        const int F = J.frames[size_t(b)];
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
std::vector<int> Engine::redo_rows_fp32(Job& J) {
    std::vector<int> rows, bad;
    if (!J.decoded) return bad;
    for (int b = 0; b < J.n; ++b)
        if (J.nf_host[b] && J.frames[size_t(b)] > 0 && J.st_pcm[size_t(b)]) rows.push_back(b);
    if (rows.empty()) return bad;
    if (codec_->fp32_convs()) return rows;  // already the fp32 kernels: nothing wider to fall back to
    const int R = int(rows.size()), up = J.up;
    std::vector<int> dframes((size_t)(R));
    int Fd = 0;
    for (int i = 0; i < R; ++i) {
        const int b = rows[size_t(i)];
        dframes[size_t(i)] = J.frames[size_t(b)] + J.ref_T[size_t(b)];
        Fd = std::max(Fd, dframes[size_t(i)]);
    }
    hipStream_t cst = codec_stream(false);
    DevBuf<int32_t> dcodes;
    PinnedBuf<int32_t> nf;
    PinnedBuf<float> hpcm;
    dcodes.grow(size_t(R) * Fd * 16);
    nf.grow(size_t(R));
    hpcm.grow(size_t(R) * Fd * up);
    std::memset(nf, 0, size_t(R) * 4);
    // the codes the first decode read: the job's own device copy ([reference ++] generated; row stride J.Fdec frames)
    for (int i = 0; i < R; ++i)
        Q3_HIP(hipMemcpyAsync(dcodes + size_t(i) * Fd * 16, J.dec_codes + size_t(rows[size_t(i)]) * J.Fdec * 16,
                              size_t(dframes[size_t(i)]) * 64, hipMemcpyDeviceToDevice, cst));
    float* pcm_dev = nullptr;
    codec_->decode(dcodes, Fd, dframes, &pcm_dev, std::string(), nullptr, nullptr, nullptr, nf, true);
    Q3_HIP(hipMemcpyAsync(hpcm, pcm_dev, size_t(R) * Fd * up * 4, hipMemcpyDeviceToHost, cst));
    Q3_HIP(hipStreamSynchronize(cst));
    for (int i = 0; i < R; ++i) {
        const int b = rows[size_t(i)];
        if (nf[i]) {
            bad.push_back(b);
            continue;
        }
        // decoded-stream coordinates: sample p of the decode is sample p - cut of the row's audio; chunk k covers
        // [k * step, (k + 1) * step). Chunks below `held` have been delivered from the first decode and stay as they are.
        const int64_t cut = J.row_cut[size_t(b)], ns = J.row_ns[size_t(b)], step = int64_t(std::max(J.chunk_frames, 1)) * up;
        if (J.prefixed) {  // chunks count from the row's own first frame: chunk k is samples [k * step, (k + 1) * step) of its audio
            float* own = J.st_pcm[size_t(b)].get();
            const int64_t at = std::min(ns, int64_t(std::max(0, J.held_from[size_t(b)])) * step);
            std::memcpy(own + at, hpcm + size_t(i) * Fd * up + cut + at, size_t(ns - at) * 4);
            if (J.cb) {
                std::unique_lock<std::mutex> lk = cb_lock();
                for (int64_t lo = at; lo < ns; lo += step) audio_chunk(J.cb, J.user, J.request_base + b, own + lo, std::min(step, ns - lo), lo);
            }
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
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    // a queued decode batch: row b is request req_index[b], timed from its admission to its retirement
    auto out = [&](int b) -> q3tts_result& { return J.row_out.empty() ? results[b] : *J.row_out[size_t(b)]; };
    auto ev_index = [&](int b) { return J.request_base + (J.req_index.empty() ? b : J.req_index[size_t(b)]); };
    for (int b = 0; b < n; ++b) {
        q3tts_result& r = out(b);
        std::memset(&r, 0, sizeof(r));
        const int F = J.frames[size_t(b)];
        const double total = J.row_span.empty() ? job_total : J.row_span[size_t(b)];
        r.info.prompt_token_count = J.target_tokens[size_t(b)];  // tokens of `text` (Qwen3+Streaming.swift:106)
        r.info.generation_token_count = F;
        r.info.prefill_time = 0;  // hard-coded in the reference (Qwen3+Streaming.swift:112)
        r.info.generate_time = total;
        r.info.tokens_per_second = total > 0 ? double(F) / total : 0;
        r.info.peak_memory_usage = double(total_b - free_b) / 1e9;
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
        for (int b = 0; b < n; ++b) {
            if (out(b).status != Q3TTS_OK) continue;
            q3tts_event ev{};
            ev.kind = Q3TTS_EVENT_INFO;
            ev.request_index = ev_index(b);
            ev.info = &out(b).info;
            J.cb(J.user, &ev);
            ev.kind = Q3TTS_EVENT_AUDIO;
            ev.info = nullptr;
            ev.pcm = out(b).pcm;
            ev.n_samples = out(b).n_samples;
            J.cb(J.user, &ev);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// continuous batching (q3tts_generate_queued)
// ------------------------------------------------------------------------------------------------
bool Engine::job_outstanding() const {
    for (const auto& J : jobs_)
        if (J.busy) return true;
    return false;
}

// resolve() plus every limit a request would otherwise hit inside the slot loop, on the host: the lengths are the ones
// assemble_prompts produces -- for an ordinary request, or with `voice` for the ICL prompt of a voice-clone request (a
// request that carries its clip as ref_audio is refused here: its front end has no place at a burst boundary)
ResolvedRequest Engine::check_queued(const q3tts_request& r, const q3tts_sampling& sp, const Voice* voice, bool open_text) const {
    const TalkerConfig& t = m_->cfg.talker;
    Q3_CHECK(r.ref_audio == nullptr, 3, "Invalid input: voice-clone requests (ref_audio) are not supported by q3tts_generate_queued");
    ResolvedRequest o = resolve(r, sp, voice);
    if (open_text) {  // role + content, no tail; the frame cap while the text is open is max_tokens (final_text_cap at the close)
        Q3_CHECK(!o.clone, 3, "Invalid input: an open-text request cannot be a voice-clone request");
        o.n_tail = 0;
        o.text_open = true;
        o.open_max_tokens = r.max_tokens > 0 ? r.max_tokens : 2048;
        o.open_force_frames = sp.force_frames;
        o.max_frames = sp.force_frames > 0 ? sp.force_frames : o.open_max_tokens;
        o.target_token_count = int(o.text_ids.size()) - 3;
    }
    Q3_CHECK(m_->has_codec, 1, "Model not initialized: Speech tokenizer not loaded");  // Qwen3.swift:799-801
    Q3_CHECK(o.max_frames <= Fcap_, 3, "Invalid input: max_tokens exceeds the configured max_frames");
    Q3_CHECK(o.language_id < t.vocab_size && o.speaker_token < t.vocab_size, 3, "Invalid input: codec prefix id out of range");
    const int tl = int(o.text_ids.size());
    int nc = (o.language_id < 0 ? 3 : 4) + (o.speaker_token >= 0 ? 1 : 0) + 2;  // codec prefix (Qwen3.swift:322-359)
    int np = int(o.instruct_ids.size()) + 3 + nc;                                // instruct, role, prefix, first text token
    int nt = (tl - o.n_tail > 4 ? tl - o.n_tail - 4 : 0) + 1;                    // trailing text + tts_eos (:394-406)
    if (o.clone) {  // the ICL prompt (assemble_prompts): role, prefix with the x-vector, reference text, target text, tts_eos,
                    // codec_bos, one row per reference frame; the trailing text is tts_pad alone
        nc += m_->has_speaker_encoder ? 1 : 0;
        np = 3 + (nc - 1) + (int(o.ref_text_ids.size()) - 5) + (tl - 8) + 2 + o.ref_T;
        nt = 1;
    }
    Q3_CHECK(np <= Pcap_, 3, "Invalid input: prompt longer than max_prompt");
    Q3_CHECK(nt <= Tcap_, 3, "Invalid input: text longer than max_prompt");
    Q3_CHECK(np + o.max_frames + 1 <= m_->talker.max_pos, 3, "Invalid input: sequence longer than the RoPE table");
    return o;
}

void Engine::ensure_queue_ws() {
    if (qws_) return;
    const TalkerConfig& t = m_->cfg.talker;
    const int H = t.hidden_size, qd = t.num_attention_heads * kHeadDim, kd = t.num_key_value_heads * kHeadDim;
    uint8_t* base = nullptr;
    for (int pass = 0; pass < 2; ++pass) {
        Bump b{base};
        // the talker's activations of a prefill: tk_'s shapes without the head's logits
        qk_.ld_qkv = qd + 2 * kd;
        qk_.ld_act = m_->talker.max_inter_p;
        qk_.ld_logits = 0;
        qk_.h = b.take<uint16_t>(size_t(Mp_) * H);
        qk_.xn = b.take<uint16_t>(size_t(Mp_) * H);
        qk_.ss_a = b.take<float>(size_t(H / 16) * Mp_);
        qk_.ss_b = b.take<float>(size_t(H / 16) * Mp_);
        qk_.qkv = b.take<uint16_t>(size_t(Mp_) * qk_.ld_qkv);
        qk_.ao = b.take<uint16_t>(size_t(Mp_) * qd);
        qk_.act = b.take<uint16_t>(size_t(Mp_) * qk_.ld_act);
        qk_.logits = nullptr;
        q_bt_ = b.take<int32_t>(size_t(Bm_) * max_pages_);
        q_kv_len_ = b.take<int32_t>(size_t(Bm_));
        q_n_prompt_ = b.take<int32_t>(size_t(Bm_));
        q_desc_ = b.take<AdmitDesc>(size_t(Bm_));
        row_key_ = b.take<uint32_t>(size_t(Bm_));
        q_text_desc_ = b.take<TextAppendDesc>(size_t(Bm_));
        q_active_ = b.take<uint8_t>(size_t(Bm_));
        text_open_ = b.take<uint8_t>(size_t(Bm_));
        starved_ = b.take<uint8_t>(size_t(Bm_));
        if (!pass) {
            const size_t bytes = align_up(b.off, 256);
            Q3_HIP(hipMalloc(reinterpret_cast<void**>(&base), bytes));
            Q3_HIP(hipMemset(base, 0, bytes));
        }
    }
    qws_ = base;
}

// One admitted request until its result is filled: what was resolved at its submission and, once its row is retired, what it
// generated (streamed: until its last chunk has landed; otherwise until its decode batch is delivered).
struct Engine::QLive {
    ResolvedRequest rr;
    int frames = 0;
    double span = 0;             // admission -> retirement
    std::vector<int32_t> codes;  // [frames][16]
};

void Engine::cancel_slots(uint64_t mask, int slots) { launch_cancel_rows(mask, finished_, active_, slots, st_); }

// What was appended to running open-text requests since the last boundary: the new ids go through text_projection like a
// prompt's (project_rows; row 0 of the pass is tts_eos, for the closes) and one launch puts them behind the slots' trailing
// text, closes the texts that ended and resumes the rows that waited (kernels.h TextAppendArgs). Text for a ticket that is in
// no slot any more -- retired, cancelled -- is dropped: the caller cannot know.
void Engine::apply_text_appends(QueueShared& q, std::vector<QSlot>& sl, std::unordered_map<int, QLive>& live) {
    std::vector<RequestSource::TextAppend> msgs;
    q.src->take_appends(msgs);
    const int S = int(sl.size());
    struct Add {
        std::vector<int32_t> ids;
        bool close = false;
    };
    std::vector<Add> add((size_t)(S));
    for (auto& m : msgs)
        for (int s = 0; s < S; ++s)
            if (sl[size_t(s)].req == m.ticket && sl[size_t(s)].open && !add[size_t(s)].close) {
                add[size_t(s)].ids.insert(add[size_t(s)].ids.end(), m.ids.begin(), m.ids.end());
                add[size_t(s)].close = m.final;
            }
    q_text_ids_.assign(1, m_->cfg.tts_eos_token_id);
    q_text_desc_host_.clear();
    for (int s = 0; s < S; ++s) {
        Add& a = add[size_t(s)];
        if (a.ids.empty() && !a.close) continue;
        QSlot& x = sl[size_t(s)];
        QLive& w = live.at(x.req);
        const int n_new = int(a.ids.size());
        // trailing rows = content - 1, + 1 for tts_eos at the close: at most Tcap_ content tokens (the session's append checked it)
        Q3_CHECK(x.n_content + n_new <= Tcap_, 7, "internal error: appended text beyond the trailing-text rows");
        TextAppendDesc d{};
        d.slot = s;
        d.src_row = int(q_text_ids_.size());
        d.n_new = n_new;
        q_text_ids_.insert(q_text_ids_.end(), a.ids.begin(), a.ids.end());
        x.n_content += n_new;
        w.rr.target_token_count = x.n_content;
        if (a.close) {
            // The cap the ordinary request would have had from its first frame on. The row cannot have passed it: a row forms
            // frame f + 1's input from content token f + 1, so starvation keeps its frames <= its content tokens n, it is below
            // max_tokens or it would have ended, and n < max(75, 6 n); with force_frames both caps are force_frames.
            d.close = 1;
            d.max_frames = final_text_cap(w.rr.open_max_tokens, w.rr.open_force_frames, x.n_content);
            x.open = false;
            x.cap = d.max_frames;
            w.rr.max_frames = d.max_frames;
            w.rr.text_open = false;
        }
        x.starved = false;  // (it has its next text row now -- a new one, or tts_eos: the launch below resumes it)
        q_text_desc_host_.push_back(d);
    }
    const int k = int(q_text_desc_host_.size());
    if (k > 0) {
        project_rows(q_text_ids_, int(q_text_ids_.size()));
        Q3_HIP(hipMemcpyAsync(q_text_desc_, q_text_desc_host_.data(), size_t(k) * sizeof(TextAppendDesc), hipMemcpyHostToDevice, st_));
        TextAppendArgs ta{};
        ta.desc = q_text_desc_; ta.src = proj_out_; ta.eos_row = proj_out_;
        ta.trailing = trailing_; ta.n_trailing = n_trailing_; ta.text_open = text_open_; ta.max_frames = max_frames_; ta.slots = S;
        ta.fe = frame_end_args(S);
        launch_text_append_rows(ta, q_text_desc_host_.data(), k, st_);
        Q3_HIP(hipStreamSynchronize(st_));  // (the staging vectors are reused by the next boundary; proj_out_ by the next admission)
    }
    int starved_now = 0;
    for (const QSlot& x : sl) starved_now += x.req >= 0 && x.starved ? 1 : 0;
    q.src->text_progress(starved_now, 0);
}

int Engine::admit(QueueShared& q, std::vector<QSlot>& sl, std::unordered_map<int, QLive>& live) {
    std::vector<ResolvedRequest> rr;
    std::vector<int> slots, idx;
    std::vector<uint32_t> keys;
    std::vector<SamplingParams> params;
    QueueItem item;
    for (int s = 0; s < int(sl.size()); ++s) {
        if (sl[size_t(s)].req >= 0) continue;
        if (!q.src->take(item)) break;
        rr.push_back(std::move(item.rr));
        slots.push_back(s);
        idx.push_back(item.ticket);
        keys.push_back(q.row_base + uint32_t(item.ticket));  // request t draws what q3tts_generate draws with row_base + t
        params.push_back(item.params);
    }
    const int k = int(rr.size());
    if (k == 0) return 0;
    {   // voice rows: their prompt rows (x-vector, reference frames) into extra_ for this sub-batch, device to device; no front end
        const int H = m_->cfg.talker.hidden_size;
        size_t rows = 0;
        for (auto& r : rr)
            if (r.voice) {
                r.extra_base = int(rows);
                rows += size_t(1) + r.ref_T;
            }
        Q3_CHECK(rows * H <= extra_.capacity(), 7, "internal error: voice rows beyond the queue's reservation");  // (run_queued)
        for (auto& r : rr)
            if (r.voice)
                Q3_HIP(hipMemcpyAsync(extra_ + size_t(r.extra_base) * H, r.voice->rows_dev, size_t(1 + r.ref_T) * H * 2,
                                      hipMemcpyDeviceToDevice, st_));
    }
    std::vector<int> np, nt;
    assemble_prompts(rr, np, nt, &slots);  // prompt_ rows 0..k-1; trailing text into the slots' rows (synchronises st_)
    int Pmax = 0;
    for (int p : np) Pmax = std::max(Pmax, p);
    // the sub-batch's arrays: block table (its slots' pages), cache lengths 0, prompt lengths, admission descriptors
    const size_t nbt = size_t(k) * max_pages_;
    q_host_.assign(nbt + 2 * size_t(k), 0);
    int32_t* hbt = q_host_.data();
    int32_t* hnp = hbt + nbt + k;
    q_desc_host_.assign(size_t(k), AdmitDesc{});
    AdmitDesc* hd = q_desc_host_.data();
    for (int j = 0; j < k; ++j) {
        const int s = slots[size_t(j)];
        for (int i = 0; i < max_pages_; ++i) hbt[size_t(j) * max_pages_ + i] = s * max_pages_ + i;
        hnp[j] = np[size_t(j)];
        hd[j] = AdmitDesc{s, nt[size_t(j)], rr[size_t(j)].max_frames, keys[size_t(j)], rr[size_t(j)].text_open ? 1 : 0, params[size_t(j)]};
    }
    Q3_HIP(hipMemcpyAsync(q_bt_, hbt, nbt * 4, hipMemcpyHostToDevice, st_));
    Q3_HIP(hipMemcpyAsync(q_kv_len_, hbt + nbt, size_t(k) * 4, hipMemcpyHostToDevice, st_));
    Q3_HIP(hipMemcpyAsync(q_n_prompt_, hnp, size_t(k) * 4, hipMemcpyHostToDevice, st_));
    Q3_HIP(hipMemcpyAsync(q_desc_, hd, size_t(k) * sizeof(AdmitDesc), hipMemcpyHostToDevice, st_));
    Q3_HIP(hipEventRecord(ev_[0], st_));
    enqueue_prefill(qk_, k, Pmax, q_bt_, q_kv_len_, q_n_prompt_, q_active_);
    AdmitArgs a{};
    a.desc = q_desc_; a.src_h = qk_.h; a.srcMB = Mp_ / 16; a.src_ss = qk_.ss_a; a.src_kv_len = q_kv_len_; a.src_n_prompt = q_n_prompt_;
    a.h = tk_.h; a.hMB = Mp_ / 16; a.ss = tk_.ss_a;
    a.H = m_->cfg.talker.hidden_size; a.V = m_->cfg.talker.vocab_size; a.Fmax = Fcap_; a.slots = Bm_;
    a.kv_len = kv_len_; a.n_prompt = n_prompt_; a.n_trailing = n_trailing_; a.max_frames = max_frames_; a.n_frames = n_frames_;
    a.cp_len = cp_len_; a.trailing_idx = trailing_idx_; a.cur_codes = cur_codes_; a.codes = codes_; a.row_key = row_key_;
    a.sp = sp_dev_;
    a.finished = finished_; a.active = active_; a.seen = seen_;
    a.text_open = text_open_; a.starved = starved_;
    launch_admit_rows(a, k, st_);
    Q3_HIP(hipEventRecord(ev_[1], st_));
    const double now = now_s();
    for (int j = 0; j < k; ++j) {
        QSlot& x = sl[size_t(slots[size_t(j)])];
        x = QSlot{};
        x.req = idx[size_t(j)];
        x.np = np[size_t(j)];
        x.t0 = now;
        x.cap = rr[size_t(j)].max_frames;
        x.open = rr[size_t(j)].text_open;
        x.n_content = int(rr[size_t(j)].text_ids.size()) - 3 - rr[size_t(j)].n_tail;
        live[idx[size_t(j)]].rr = std::move(rr[size_t(j)]);
    }
    return k;
}

// The slot loop. Slot s owns KV pages [s * max_pages_, (s + 1) * max_pages_) for the whole call. Every burst boundary:
//   retire   rows whose finished flag is up: codes copied to the host, slot freed; their decode waits for the codec stream
//   admit    free slots take the next requests (in request order), prefilled as a sub-batch of their own (admit())
//   burst    frame steps of all `slots` rows, ending no later than the frame at which the first running row reaches its cap
// and, while the burst runs, a decode batch that has landed is delivered (INFO / AUDIO, results) and, the codec stream being
// idle, every retired row waiting is decoded in one batch beside the frame loop (the confined stream of a pipelined job).
void Engine::run_queued(QueueShared& q, int S, const q3tts_sampling& sp, q3tts_event_cb cb, void* user) {
    Q3_HIP(hipSetDevice(m_->device));
    Q3_CHECK(S >= 1 && S <= Bm_, 3, "Invalid input: slots must be between 1 and max_batch");
    Q3_CHECK(!job_outstanding(), 3, "Invalid input: a q3tts_generate_begin job is outstanding (q3tts_generate_end must be called first)");
    ensure_queue_ws();
    {   // an admission's voice rows go through extra_: room for S rows with the longest reference, so that no boundary allocates
        if (q.voice_ref_max >= 0) extra_.grow(size_t(S) * (1 + q.voice_ref_max) * m_->cfg.talker.hidden_size);
    }
    const double t_call = now_s();
    // every slot starts empty: finished, inactive, an empty cache in its own pages
    std::vector<int32_t> bt(size_t(S) * max_pages_);
    for (size_t i = 0; i < bt.size(); ++i) bt[i] = int32_t(i);
    Q3_HIP(hipMemcpyAsync(block_table_, bt.data(), bt.size() * 4, hipMemcpyHostToDevice, st_));
    for (int32_t* p : {kv_len_, cp_len_, n_frames_, max_frames_, trailing_idx_, n_trailing_, n_prompt_})
        Q3_HIP(hipMemsetAsync(p, 0, size_t(S) * 4, st_));
    Q3_HIP(hipMemsetAsync(row_key_, 0, size_t(S) * 4, st_));
    Q3_HIP(hipMemsetAsync(active_, 0, size_t(S), st_));
    Q3_HIP(hipMemsetAsync(finished_, 1, size_t(S), st_));
    {  // every slot's entry holds the call's own values until an admission writes its request's (an empty slot's sampler returns early,
       // but reads its entry with the other operands first)
        q3tts_sampling call_wide = sp;
        call_wide.per_request = nullptr;
        upload_sampling(call_wide, 0u, S);
    }
    build_cp_proj_tables();
    struct KeyScope {
        Engine* e;
        ~KeyScope() { e->frame_row_key_ = nullptr; e->frame_text_open_ = nullptr; }
    } key_scope{this};
    frame_row_key_ = row_key_;  // the samplers of every frame step below key on the slots' request indices
    const bool open_text = q.src->open_text();
    if (open_text) {  // (a session) rows may starve: the frame end reads text_open_ and raises starved_
        Q3_HIP(hipMemsetAsync(text_open_, 0, size_t(S), st_));
        Q3_HIP(hipMemsetAsync(starved_, 0, size_t(S), st_));
        frame_text_open_ = text_open_;
    }
    hipGraphExec_t ge = opts_.use_graph ? frame_graph(S) : nullptr;
    Q3_HIP(hipStreamSynchronize(st_));

    std::vector<QSlot> sl((size_t)(S));
    std::unordered_map<int, QLive> live;  // every admitted request whose result is not filled yet, by ticket
    std::vector<int> settled;             // results filled since the last boundary: forgotten there
    std::deque<int> waiting;              // retired, decode not started
    int dec = -1;                 // job slot of the decode batch in flight (all are free: no begin job is outstanding)
    struct DecodeGuard {          // an exception leaves no job slot behind
        Engine* e;
        int* dec;
        ~DecodeGuard() {
            if (*dec < 0) return;
            (void)hipEventSynchronize(e->jobs_[*dec].ev_codec[1]);
            e->release_job(e->jobs_[*dec]);
        }
    } dec_guard{this, &dec};
    double codec_ms = 0;
    auto deliver = [&](bool wait) {  // end(): results[i] and INFO / AUDIO of every row of the batch (fp32 re-decode included)
        if (!wait) {
            std::lock_guard<std::mutex> lk(stage_mu_);
            if (jobs_[dec].stage == 1) return;  // the staging thread has not copied it out yet
        }
        const int j = dec;
        dec = -1;
        const std::vector<int> batch = jobs_[j].req_index;
        end(j, nullptr);
        codec_ms += timing.codec_ms;
        for (int t : batch) {
            q.src->complete(t);
            live.erase(t);
        }
    };
    auto decode = [&](bool overlapped) {  // every waiting row (up to max_batch) in one decode on the codec stream
        Job& J = jobs_[0];
        const int R = std::min(int(waiting.size()), Bm_);
        J.reset(R, codec_->upsample());
        J.req_index.assign(size_t(R), 0);
        J.row_out.assign(size_t(R), nullptr);
        J.row_span.assign(size_t(R), 0);
        J.codes_host.assign(size_t(R) * Fcap_ * 16, 0);
        std::vector<int> dframes((size_t)(R), 0);  // frames the decoder sees per row: [reference ++] generated, as hand_off
        std::vector<const Voice*> voices((size_t)(R), nullptr);
        bool any_voice = false;
        for (int b = 0; b < R; ++b) {
            const QLive& w = live.at(waiting[size_t(b)]);
            const ResolvedRequest& rq = w.rr;
            J.frames[size_t(b)] = w.frames;
            J.target_tokens[size_t(b)] = rq.target_token_count;
            J.req_index[size_t(b)] = waiting[size_t(b)];
            J.row_out[size_t(b)] = q.src->result(waiting[size_t(b)]);
            Q3_CHECK(J.row_out[size_t(b)] != nullptr, 7, "internal error: a retired request has no result to fill");
            J.row_span[size_t(b)] = w.span;
            std::copy(w.codes.begin(), w.codes.end(), J.codes_host.begin() + ptrdiff_t(size_t(b) * Fcap_ * 16));
            if (rq.voice) {  // compute_cuts then trims and cuts exactly as the static path does
                any_voice = true;
                voices[size_t(b)] = rq.voice;
                J.ref_T[size_t(b)] = rq.voice->ref_T;
                J.ref_code0[size_t(b)] = rq.voice->code0;
            }
            dframes[size_t(b)] = w.frames > 0 ? w.frames + J.ref_T[size_t(b)] : 0;
            J.Fdec = std::max(J.Fdec, dframes[size_t(b)]);
        }
        if (any_voice) J.voices = std::move(voices);
        waiting.erase(waiting.begin(), waiting.begin() + R);
        start_decode(J, dframes, overlapped, J.codes_host.data());
        dec = 0;
        publish_job(J, cb, user, 0, t_call, true);  // copied out by the staging thread while the frame loop goes on
    };

    // ---- streamed audio (audio_chunk_frames > 0 with audio_window_frames > 0): every request's chunks leave while it generates ----
    // A slotted codec stream over the S slots decodes them; retired rows do not go through the decode batches above: a
    // request's AUDIO is the concatenation of its chunks, INFO and AUDIO fire once the last one has landed. Only requests held
    // back at a chunk that left the fp16 range are decoded again (fp32), behind the loop.
    const bool streamed = sp.audio_chunk_frames > 0;
    const int up = codec_->upsample();
    DevBuf<int32_t> scodes;          // [S][Fcap][16]: the codes the stream reads, copied from codes_ burst by burst
    std::unique_ptr<SlotStream> ss;  // (its destructor closes the runner's stream whatever ends this call; it goes before scodes)
    std::vector<int> copied((size_t)(S), 0);   // frames [0, copied) of the slot's current request are in scodes
    std::vector<uint8_t> reused((size_t)(S), 0);  // the slot has had an earlier occupant whose codes the stream may still read
    std::vector<int> held;           // streamed: complete but held back, for the fp32 re-decode
    auto fill_result = [&](int req, q3tts_status status, float* pcm) {  // as end() fills a row; pcm: ownership passes
        const QLive& w = live.at(req);
        q3tts_result* rp = q.src->result(req);
        Q3_CHECK(rp != nullptr, 7, "internal error: a streamed request has no result to fill");
        q3tts_result& r = *rp;
        struct Settle {  // however this ends, the result is the source's from here on
            RequestSource* src;
            std::vector<int>* settled;
            int req;
            ~Settle() {
                src->complete(req);
                settled->push_back(req);
            }
        } settle_req{q.src, &settled, req};
        std::memset(&r, 0, sizeof(r));
        size_t free_b = 0, total_b = 0;
        (void)hipMemGetInfo(&free_b, &total_b);
        r.info.prompt_token_count = w.rr.target_token_count;
        r.info.generation_token_count = w.frames;
        r.info.generate_time = w.span;
        r.info.tokens_per_second = w.span > 0 ? double(w.frames) / w.span : 0;
        r.info.peak_memory_usage = double(total_b - free_b) / 1e9;
        r.status = status;
        if (status != Q3TTS_OK) {
            std::free(pcm);
            return;
        }
        r.codes = static_cast<int32_t*>(std::malloc(size_t(w.frames) * 16 * 4));
        if (!r.codes) {
            std::free(pcm);
            throw Error(5, "out of host memory for the results");
        }
        std::memcpy(r.codes, w.codes.data(), size_t(w.frames) * 16 * 4);
        r.n_frames = w.frames;
        r.n_samples = int64_t(w.frames) * up;  // all generated frames: what has left cannot be trimmed (include/q3tts.h)
        r.pcm = pcm;
        if (cb) {
            std::unique_lock<std::mutex> lk = cb_lock();
            q3tts_event ev{};
            ev.kind = Q3TTS_EVENT_INFO;
            ev.request_index = req;
            ev.info = &r.info;
            cb(user, &ev);
            ev.kind = Q3TTS_EVENT_AUDIO;
            ev.info = nullptr;
            ev.pcm = r.pcm;
            ev.n_samples = r.n_samples;
            cb(user, &ev);
        }
    };
    // Voice requests of a streamed queue (audio_stream_reference): a slot's code row holds the voice's reference frames, then the
    // generated ones. The reference is decoded as the row's prefix at the admission (nothing of it is delivered) unless the state
    // it leaves in the causal tail has been saved before: then one launch puts it back (PrefixCache).
    const int stride = Fcap_ + (streamed ? q.ref_max : 0);  // frames per row of scodes
    std::vector<int> prefix_of((size_t)(S), 0);           // reference frames in front of the slot's current request
    std::vector<DecodeRowDesc> ref_desc;                    // (read by the copy of an admission until that boundary's synchronisation)
    DevBuf<DecodeRowDesc> ref_desc_dev;
    struct PendingState {  // a state saved at this call's admissions: published once its prefix is known to have stayed finite
        std::shared_ptr<PrefixCache::Entry> entry;
        int32_t* flag = nullptr;  // its own entry of a block of state_flags
    };
    std::vector<PendingState> pending;
    std::vector<int32_t*> free_flags;  // entries of state_flags no pending state owns
    std::vector<std::shared_ptr<PrefixCache::Entry>> in_use;  // states restored in this call stay alive until its stream has drained
    // Pinned flags in blocks of 2 * slots: a saved state owns one from its save to settle(), which gives it back. A block never moves
    // (copies in flight write into it) and a further one is added when all are owned, so no admission ever waits for a flag.
    std::deque<PinnedBuf<int32_t>> state_flags;
    auto add_flags = [&] {
        const size_t n = size_t(2) * S;
        state_flags.emplace_back();
        int32_t* b = state_flags.back().grow(n);
        std::memset(b, 0, n * 4);
        for (size_t i = n; i-- > 0;) free_flags.push_back(b + i);
    };
    auto settle = [&](bool wait) {  // saved states whose save has run: into the cache, unless the prefix left the fp16 range
        for (size_t i = 0; i < pending.size();) {
            if (wait) {
                Q3_HIP(hipEventSynchronize(pending[i].entry->ready));
            } else {
                const hipError_t pq = hipEventQuery(pending[i].entry->ready);
                if (pq == hipErrorNotReady) {
                    ++i;
                    continue;
                }
                Q3_HIP(pq);
            }
            if (*pending[i].flag == 0) q.prefix_cache->publish(pending[i].entry);
            free_flags.push_back(pending[i].flag);
            pending.erase(pending.begin() + ptrdiff_t(i));
        }
    };
    // (behind ss->finish(): the runner's stream is closed, `outs` holds the stream's requests)
    auto redo_held = [&](std::unordered_map<int, SlotStream::Out>& outs) {
        // ---- requests held back at a chunk that left the fp16 range: once more on the fp32 matrix cores, as redo_rows_fp32 does
        // for a streamed job: chunks below the held one stay as delivered, the rest (events included) come from the exact decode
        for (size_t h0 = 0; h0 < held.size(); h0 += size_t(Bm_)) {
            const int R = int(std::min(held.size() - h0, size_t(Bm_)));
            // (a voice request streamed behind its reference: the decoder sees reference ++ generated, as in every clone decode,
            // and the request's samples start exactly ref_T frames in)
            std::vector<int> dframes((size_t)(R)), refs((size_t)(R), 0);
            int Fd = 0;
            for (int i = 0; i < R; ++i) {
                const ResolvedRequest& rq = live.at(held[h0 + i]).rr;
                if (rq.voice && q.stream_reference) refs[size_t(i)] = rq.voice->ref_T;
                Fd = std::max(Fd, dframes[size_t(i)] = refs[size_t(i)] + live.at(held[h0 + i]).frames);
            }
            PinnedBuf<int32_t> nf;
            PinnedBuf<float> hpcm;
            std::memset(nf.grow(size_t(R)), 0, size_t(R) * 4);
            const bool widest = codec_->fp32_convs();  // already the fp32 kernels: nothing wider to fall back to
            if (!widest) {
                hipStream_t cst = codec_stream(false);
                DevBuf<int32_t> dcodes;
                dcodes.grow(size_t(R) * Fd * 16);
                hpcm.grow(size_t(R) * Fd * up);
                for (int i = 0; i < R; ++i) {
                    const int ref = refs[size_t(i)];
                    if (ref > 0)
                        Q3_HIP(hipMemcpy(dcodes + size_t(i) * Fd * 16, live.at(held[h0 + i]).rr.voice->codes_host.data(), size_t(ref) * 64,
                                         hipMemcpyHostToDevice));
                    Q3_HIP(hipMemcpy(dcodes + (size_t(i) * Fd + ref) * 16, live.at(held[h0 + i]).codes.data(),
                                     size_t(dframes[size_t(i)] - ref) * 64, hipMemcpyHostToDevice));
                }
                float* pcm_dev = nullptr;
                codec_->decode(dcodes, Fd, dframes, &pcm_dev, std::string(), nullptr, nullptr, nullptr, nf, true);
                Q3_HIP(hipMemcpyAsync(hpcm, pcm_dev, size_t(R) * Fd * up * 4, hipMemcpyDeviceToHost, cst));
                Q3_HIP(hipStreamSynchronize(cst));
            }
            for (int i = 0; i < R; ++i) {
                const int req = held[h0 + i];
                SlotStream::Out& o = outs.at(req);
                if (widest || nf[i]) {  // never hand out a waveform with holes in it
                    fill_result(req, Q3TTS_ERR_AUDIO_DECODING_FAILED, o.pcm.release());
                    last_error = kCodecRangeMsg;
                    continue;
                }
                const int64_t step = int64_t(sp.audio_chunk_frames) * up, ns = int64_t(dframes[size_t(i)] - refs[size_t(i)]) * up;
                const int64_t from = std::min(ns, int64_t(o.held_from) * step);
                std::memcpy(o.pcm.get() + from, hpcm + (size_t(i) * Fd + refs[size_t(i)]) * up + from, size_t(ns - from) * 4);
                if (cb) {
                    std::unique_lock<std::mutex> lk = cb_lock();
                    for (int64_t lo = from; lo < ns; lo += step) audio_chunk(cb, user, req, o.pcm.get() + lo, std::min(step, ns - lo), lo);
                }
                fill_result(req, Q3TTS_OK, o.pcm.release());
            }
        }
        held.clear();
    };
    auto open_stream = [&] {
        ss.reset();
        ss = std::make_unique<SlotStream>(*this, S, sp.audio_chunk_frames, sp.audio_window_frames, std::max(0, sp.audio_lookahead_frames),
                                          Fcap_, true, q.ref_max);
        ss->t_call = t_call;
        if (cb)
            ss->on_chunk = [&](int req, int, const float* pcm, int64_t n, int64_t off) {
                std::unique_lock<std::mutex> lk = cb_lock();
                audio_chunk(cb, user, req, pcm, n, off);
            };
        ss->on_complete = [&](int req) {
            SlotStream::Out& o = ss->out[req];
            if (live.at(req).frames == 0) fill_result(req, Q3TTS_ERR_GENERATION_FAILED, o.pcm.release());  // Qwen3.swift:939-941
            else if (o.held_from >= 0) held.push_back(req);
            else fill_result(req, Q3TTS_OK, o.pcm.release());
        };
    };
    if (streamed) {
        scodes.grow(size_t(S) * stride * 16);
        if (q.prefix_cache) add_flags();
        open_stream();
    }

    const int burst_frames = std::max(1, max_inflight_frames / 2);
    std::vector<int32_t> h_nframes((size_t)(S), 0);
    std::vector<uint8_t> h_fin((size_t)(S), 0), h_starved((size_t)(S), 0);
    int64_t kvb = 0;
    int launched = 0, served = 0;
    double prefill_ms = 0;
    std::vector<int> cancels, zombies;  // zombies: cancelled streamed requests whose chunks may still be in flight
    Q3_HIP(hipEventRecord(ev_[2], st_));
    for (;;) {
        // ---- results filled at the last boundary are forgotten; cancelled rows (a session) leave their slots ----
        for (int t : settled) {
            live.erase(t);
            if (ss) ss->out.erase(t);
        }
        settled.clear();
        for (size_t i = 0; i < zombies.size();)
            if (!ss->in_flight(zombies[i])) {
                ss->out.erase(zombies[i]);
                zombies.erase(zombies.begin() + ptrdiff_t(i));
            } else {
                ++i;
            }
        if (q.src->has_cancels()) {
            q.src->take_cancels(cancels);
            uint64_t mask = 0;
            for (int t : cancels) {
                int s = -1;
                for (int i = 0; i < S; ++i)
                    if (sl[size_t(i)].req == t) s = i;
                if (s >= 0) {  // running: its slot is an empty one from this boundary on, and no event of it fires any more
                    mask |= uint64_t(1) << s;
                    if (streamed) {
                        ss->drop(s);
                        zombies.push_back(t);
                    }
                    sl[size_t(s)] = QSlot{};
                } else {
                    auto w = std::find(waiting.begin(), waiting.end(), t);
                    if (w == waiting.end()) continue;  // in a decode batch, or its last chunks are landing: it completes as it is
                    waiting.erase(w);
                }
                live.erase(t);
                q.src->complete_cancelled(t);
            }
            if (open_text) {  // (a cancelled row may have been one that waited for text)
                int starved_now = 0;
                for (const QSlot& x : sl) starved_now += x.req >= 0 && x.starved ? 1 : 0;
                q.src->text_progress(starved_now, 0);
            }
            cancel_slots(mask, S);  // on st_: in front of the admissions below and of the next read of the flags
        }
        // ---- admission: free slots in slot order take the next requests in request order ----
        std::vector<int> before;
        if (streamed)
            for (const QSlot& x : sl) before.push_back(x.req);
        const int admitted = admit(q, sl, live);
        served += admitted;
        if (streamed) {  // a new occupant: the row's chunks, history margins and non-finite flag start over, in codec-stream order
            settle(false);
            std::vector<int> fresh, primed;
            bool any_ref = false, wait_pushed = false;
            for (int s = 0; s < S; ++s)
                if (sl[size_t(s)].req >= 0 && before[size_t(s)] < 0) {
                    const ResolvedRequest& rq = live.at(sl[size_t(s)].req).rr;
                    fresh.push_back(s);
                    copied[size_t(s)] = 0;
                    prefix_of[size_t(s)] = rq.voice && q.stream_reference ? rq.ref_T : 0;
                    if (prefix_of[size_t(s)] > 0) {
                        any_ref = true;
                        wait_pushed = wait_pushed || reused[size_t(s)];
                    }
                }
            if (any_ref) {
                // the voices' reference frames to the front of their slots' code rows (the builder also moves one generated frame,
                // which does not exist yet: frame ref_T of the row, read by nothing before the copy below has written it). They
                // overwrite what the previous occupant's last chunks read: behind ev_pushed, like a new occupant's first frames.
                if (wait_pushed) Q3_HIP(hipStreamWaitEvent(st_, ss->ev_pushed, 0));
                ref_desc.assign(size_t(S), DecodeRowDesc{});
                for (int s : fresh) {
                    if (prefix_of[size_t(s)] == 0) continue;
                    const Voice* v = live.at(sl[size_t(s)].req).rr.voice;
                    ref_desc[size_t(s)] = DecodeRowDesc{static_cast<const int32_t*>(v->codes_dev), codes_ + size_t(s) * Fcap_ * 16, v->ref_T, 1, s, 0};
                    reused[size_t(s)] = 1;
                }
                Q3_HIP(hipMemcpyAsync(ref_desc_dev.grow(size_t(S)), ref_desc.data(), size_t(S) * sizeof(DecodeRowDesc), hipMemcpyHostToDevice, st_));
                launch_build_decode_codes_rows(ref_desc.data(), ref_desc_dev, S, scodes, S, stride, st_);
                Q3_HIP(hipEventRecord(ss->ev_codes, st_));
                Q3_HIP(hipStreamWaitEvent(ss->cst, ss->ev_codes, 0));
            }
            const size_t state_bytes = codec_->stream_state_bytes();
            for (int s : fresh) {
                const int req = sl[size_t(s)].req, R = prefix_of[size_t(s)];
                const ResolvedRequest& rq = live.at(req).rr;
                std::shared_ptr<PrefixCache::Entry> hit;
                if (R > 0 && q.prefix_cache)
                    hit = q.prefix_cache->find(rq.voice, sp.audio_chunk_frames, sp.audio_window_frames, std::max(0, sp.audio_lookahead_frames),
                                               codec_->stream_path(), state_bytes);
                if (hit) {
                    Q3_HIP(hipStreamWaitEvent(ss->cst, hit->ready, 0));
                    ss->admit(s, req, rq.max_frames, R, hit->blob);
                    ++q.prefix_cache->restored;
                    in_use.push_back(std::move(hit));
                } else {
                    ss->admit(s, req, rq.max_frames, R);
                    if (R > 0) primed.push_back(s);
                }
            }
            if (!primed.empty()) {
                // the prefixes need no generated frame: they are decoded now, before the row's first generated chunk can follow
                // them, and the state they leave is taken at once. The other rows have what the last push gave them.
                std::vector<int> have((size_t)(S), 0);
                std::vector<uint8_t> none((size_t)(S), 0);
                for (int s = 0; s < S; ++s) have[size_t(s)] = sl[size_t(s)].req >= 0 ? copied[size_t(s)] : 0;
                ss->push(scodes, stride, have.data(), none.data());
                for (int s : primed) {
                    Q3_CHECK(!codec_->stream_in_prefix(s), 7, "internal error: a reference prefix was left undecoded at its admission");
                    if (!q.prefix_cache || state_bytes == 0) continue;
                    const int req = sl[size_t(s)].req;
                    auto e = std::make_shared<PrefixCache::Entry>();
                    e->voice = live.at(req).rr.voice;
                    e->chunk = sp.audio_chunk_frames; e->window = sp.audio_window_frames; e->lookahead = std::max(0, sp.audio_lookahead_frames);
                    e->path = codec_->stream_path();
                    e->bytes = state_bytes;
                    e->blob.grow(state_bytes);
                    Q3_HIP(hipEventCreateWithFlags(&e->ready, hipEventDisableTiming));
                    if (free_flags.empty()) add_flags();  // (settle(false) above returned what it could)
                    int32_t* flag = free_flags.back();
                    free_flags.pop_back();
                    *flag = 0;
                    codec_->stream_save_row(s, e->blob);
                    codec_->stream_row_flag(s, flag);
                    Q3_HIP(hipEventRecord(e->ready, ss->cst));
                    pending.push_back(PendingState{std::move(e), flag});
                }
            }
        }
        // ---- open-text requests: what has been appended since the last boundary, in front of the burst, in stream order on st_ ----
        if (open_text && q.src->has_appends()) apply_text_appends(q, sl, live);
        // ---- burst: no longer than the first running row's remaining frames (its cap ends it on time) ----
        int running = 0, runnable = 0, burst = burst_frames;
        for (const QSlot& x : sl)
            if (x.req >= 0) {
                ++running;
                if (x.starved) continue;  // (waits for text on the device: it takes no frame step whatever is launched)
                ++runnable;
                burst = std::min(burst, x.cap - x.since);  // (an open-text row: the open cap, max_tokens, until its close)
            }
        if (running > 0 && runnable == 0) {
            // ---- every running row waits for text and nothing could be admitted: no frame step is launched. What has landed is
            // delivered -- decode batches of retired rows and, streamed, the chunks in flight (a starved row is not final: its
            // last chunks wait with it) -- and the thread sleeps until an append, a cancel, a request it can admit, or close.
            // (A streamed request held back for the fp32 re-decode waits until the session is idle: the stream cannot be closed
            // around rows that are still in it.)
            while (dec >= 0 || !waiting.empty()) {
                if (dec >= 0) deliver(true);
                else decode(false);
            }
            if (streamed) {
                while (ss->take(true)) {}
                settle(true);
            }
            if (!settled.empty()) continue;  // (forgotten at the top of the loop)
            bool can_admit = false;
            for (const QSlot& x : sl) can_admit = can_admit || x.req < 0;
            q.src->wait_for_text(can_admit);
            continue;
        }
        if (running == 0) {
            if (!q.src->open_ended()) break;
            // ---- a session with nothing running: everything retired is delivered, then the thread sleeps until a submit ----
            while (dec >= 0 || !waiting.empty()) {
                if (dec >= 0) deliver(true);
                else decode(false);
            }
            if (streamed) {
                while (ss->take(true)) {}
                settle(true);
                if (!held.empty()) {  // (the fp32 re-decode needs the runner: the slotted stream is closed around it)
                    std::unordered_map<int, SlotStream::Out> outs = std::move(ss->out);
                    ss->finish();
                    in_use.clear();
                    redo_held(outs);
                    open_stream();
                    zombies.clear();
                    std::fill(reused.begin(), reused.end(), uint8_t(0));
                }
            }
            if (!settled.empty()) continue;  // (forgotten at the top of the loop)
            if (!q.src->wait_for_work()) break;
            continue;
        }
        burst = std::max(burst, 1);
        for (int f = 0; f < burst; ++f) {
            if (ge) Q3_HIP(hipGraphLaunch(ge, st_));
            else enqueue_frame(S, nullptr);
        }
        launched += burst;
        q.src->progress(burst, admitted);
        Q3_HIP(hipMemcpyAsync(h_nframes.data(), n_frames_, size_t(S) * 4, hipMemcpyDeviceToHost, st_));
        Q3_HIP(hipMemcpyAsync(h_fin.data(), finished_, size_t(S), hipMemcpyDeviceToHost, st_));
        if (open_text) Q3_HIP(hipMemcpyAsync(h_starved.data(), starved_, size_t(S), hipMemcpyDeviceToHost, st_));
        Q3_HIP(hipEventRecord(burst_ev_[0], st_));
        // ---- while the burst runs: deliver the decode batch that has landed, start the next one ----
        if (dec >= 0) deliver(false);
        if (dec < 0 && !waiting.empty()) decode(true);
        if (streamed) {  // chunks that have landed leave while the burst runs, without waiting for them
            for (;;) {
                const hipError_t bq = hipEventQuery(burst_ev_[0]);
                if (bq != hipErrorNotReady) {
                    Q3_HIP(bq);
                    break;
                }
                if (!ss->take(false)) std::this_thread::yield();
            }
        }
        Q3_HIP(hipEventSynchronize(burst_ev_[0]));
        if (open_text) {
            // A starved row carries the finished flag of a parked row (row_jobs.h frame_end_job) without having ended: neither the
            // retirement nor the stream's last chunks may take it for a finished one.
            int starved_now = 0, events = 0;
            for (int s = 0; s < S; ++s) {
                QSlot& x = sl[size_t(s)];
                const bool st = x.req >= 0 && h_starved[size_t(s)] != 0;
                if (st) {
                    h_fin[size_t(s)] = 0;
                    ++starved_now;
                    if (!x.starved) ++events;
                }
                x.starved = st;
            }
            q.src->text_progress(starved_now, events);
        }
        if (streamed) {
            // ---- the new frames of every running slot into the stream's own code buffer, then every chunk they allow ----
            // A continuing request's new frames lie behind everything an issued pass reads (windows end at the frames that
            // had been copied). A NEW occupant's first frames overwrite what the previous occupant's last chunks read: that
            // copy waits for ev_pushed, recorded on the codec stream behind the latest push -- the one that issued them.
            bool first_copy = false;
            for (int s = 0; s < S; ++s)
                first_copy = first_copy || (sl[size_t(s)].req >= 0 && copied[size_t(s)] == 0 && reused[size_t(s)] && h_nframes[size_t(s)] > 0);
            if (first_copy) Q3_HIP(hipStreamWaitEvent(st_, ss->ev_pushed, 0));
            std::vector<int> avail((size_t)(S), 0);
            bool any_copy = false;
            for (int s = 0; s < S; ++s) {
                if (sl[size_t(s)].req < 0) continue;
                const int nf = std::min(h_nframes[size_t(s)], Fcap_);
                avail[size_t(s)] = nf;
                if (nf > copied[size_t(s)]) {
                    const size_t at = (size_t(s) * Fcap_ + copied[size_t(s)]) * 16;
                    const size_t to = (size_t(s) * stride + prefix_of[size_t(s)] + copied[size_t(s)]) * 16;  // behind the reference
                    Q3_HIP(hipMemcpyAsync(scodes + to, codes_ + at, size_t(nf - copied[size_t(s)]) * 64, hipMemcpyDeviceToDevice, st_));
                    copied[size_t(s)] = nf;
                    reused[size_t(s)] = 1;
                    any_copy = true;
                }
            }
            if (any_copy) {
                Q3_HIP(hipEventRecord(ss->ev_codes, st_));
                Q3_HIP(hipStreamWaitEvent(ss->cst, ss->ev_codes, 0));
            }
            std::vector<uint8_t> fin((size_t)(S), 0);
            for (int s = 0; s < S; ++s) fin[size_t(s)] = sl[size_t(s)].req >= 0 && h_fin[size_t(s)] ? 1 : 0;
            ss->push(scodes, stride, avail.data(), fin.data());  // a retiring row's remaining chunks are all issued here
        }
        if (admitted) {
            float ms = 0;
            Q3_HIP(hipEventElapsedTime(&ms, ev_[0], ev_[1]));
            prefill_ms += ms;
        }
        // ---- TOKEN events (generation order), retirement ----
        bool any_retired = false;
        std::vector<int> retiring;  // streamed: rows retired at this boundary
        const double now = now_s();
        for (int s = 0; s < S; ++s) {
            QSlot& x = sl[size_t(s)];
            if (x.req < 0) continue;
            const int nf = h_nframes[size_t(s)];
            x.since = x.open || x.starved ? nf : x.since + burst;  // (a row that waited for text has taken fewer steps than were launched)
            if (cb) emit_tokens(cb, user, s, x.req, nf, x.reported);
            if (!h_fin[size_t(s)]) continue;
            // copied out before the slot's next admission resets its row (stream order on st_)
            QLive& w = live.at(x.req);
            if (!streamed) waiting.push_back(x.req);
            w.frames = nf;
            w.span = now - x.t0;
            w.codes.assign((size_t)(nf) * 16, 0);
            if (nf > 0)
                Q3_HIP(hipMemcpyAsync(w.codes.data(), codes_ + size_t(s) * Fcap_ * 16, size_t(nf) * 64, hipMemcpyDeviceToHost, st_));
            kvb += kv_bytes(x.np, nf);
            if (streamed) retiring.push_back(s);
            x = QSlot{};
            any_retired = true;
        }
        if (any_retired) Q3_HIP(hipStreamSynchronize(st_));
        for (int s : retiring) ss->retire(s, std::min(h_nframes[size_t(s)], Fcap_));  // (complete at once when its chunks have landed)
    }
    Q3_HIP(hipEventRecord(ev_[3], st_));
    Q3_HIP(hipStreamSynchronize(st_));
    // ---- the last decode batches: nothing overlaps them any more ----
    while (dec >= 0 || !waiting.empty()) {
        if (dec >= 0) deliver(true);
        else decode(false);
    }
    double first_audio_ms = 0;
    if (streamed) {
        zombies.clear();
        ss->finish();  // the passes still in flight; every request is complete behind this
        settle(true);
        in_use.clear();
        codec_ms = ss->codec_ms;
        first_audio_ms = ss->first_audio_ms;
        redo_held(ss->out);
    }
    q3tts_timing tm{};
    float loop_ms = 0;
    Q3_HIP(hipEventElapsedTime(&loop_ms, ev_[2], ev_[3]));
    tm.prefill_ms = prefill_ms;
    tm.decode_ms = std::max(0.0, double(loop_ms) - prefill_ms);
    tm.codec_ms = codec_ms;
    tm.first_audio_ms = first_audio_ms;
    tm.frame_steps = launched;
    tm.rows = served;
    tm.kv_bytes_read = kvb;
    tm.launches_per_frame_step = launches_per_step(S);
    timing = tm;
}

// ------------------------------------------------------------------------------------------------
// block-level hooks
// ------------------------------------------------------------------------------------------------
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
    d.rode = d.tall = d.tall_shape = d.split = d.mbw = d.nw = d.ch = d.np = d.gx = d.ntw = 0;
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
        d.split = g.split; d.mbw = g.mbw; d.nw = g.nw; d.ch = g.ch; d.np = g.np; d.gx = g.gx; d.ntw = g.ntw ? 1 : 0;
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

void Engine::check_stream_chunk(int chunk_frames) const {
    Q3_CHECK(m_->has_codec, 1, "Model not initialized: Speech tokenizer not loaded");
    const int hist = codec_->hist_frames();
    Q3_CHECK(chunk_frames >= hist, 3, "Invalid input: audio_chunk_frames of a streamed decode must be at least " + std::to_string(hist));
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


// ------------------------------------------------------------------------------------------------
// EngineGroup
// ------------------------------------------------------------------------------------------------
EngineGroup::EngineGroup(std::unique_ptr<Model> model, const q3tts_load_opts& opts) : model_(std::move(model)), opts_(opts) {
    int lanes = opts.n_streams;
    // Measured: a lane's frame step takes ~4-5 ms whatever its batch size (latency-bound chain), and
    // n concurrent chains overlap by 1.6x (n=2) / 2.2x (n=4). Splitting ONE batch into lanes therefore never pays -- each
    // lane's chain is as long as the whole batch's. Two WHOLE batches on two chains do: that is the second job context below.
    if (lanes <= 0) lanes = 1;
    lanes = std::max(1, std::min(lanes, opts.max_batch));
    q3tts_load_opts lo = opts;
    lo.max_batch = ceil_div(opts.max_batch, lanes);
    for (int i = 0; i < lanes; ++i) {
        lanes_.push_back(std::make_unique<Engine>(model_.get(), lo));
        lanes_.back()->cb_mutex = &cb_mutex_;
        // keep the sum of queued kernel packets of all lanes well under the 16k-entry AQL queue (~650 nodes per frame)
        lanes_.back()->max_inflight_frames = std::max(2, 12000 / 650 / lanes);
    }
    speakers = lanes_[0]->speakers;
    if (lanes == 1) {
        // The second job context: a full engine of its own (stream, workspace, KV pool, frame graphs, codec runner) on the
        // shared model. Allocated here, at load, so that no steady-state step allocates; include/q3tts.h states the memory.
        ctx1_ = std::make_unique<Engine>(model_.get(), lo);
        ctx1_->cb_mutex = &cb_mutex_;
        background_ = !debug_env().serial_jobs;  // (the serial switch: both contexts exist and alternate, on the parent's schedule)
        if (background_)
            for (Engine* e : {lanes_[0].get(), ctx1_.get()}) e->prepare_job_pair();
    }
}

EngineGroup::~EngineGroup() {  // jobs begun and never ended: each engine lets its worker finish before its streams go
    session_.reset();  // (an open session is closed without drain: its loop thread is joined before the engines go)
    ctx1_.reset();
    lanes_.clear();
}

Engine* EngineGroup::free_context() {
    Engine* c[2] = {lanes_[0].get(), ctx1_.get()};
    for (int k = 1; k <= 2; ++k) {
        const int i = (last_ctx_ + k) & 1;
        if (c[i]->job_outstanding()) continue;
        last_ctx_ = i;
        c[i]->row_offset = 0;
        c[i]->request_base = 0;
        return c[i];
    }
    throw Error(3, "Invalid input: two jobs are already outstanding (q3tts_generate_end must be called first)");
}

int EngineGroup::begin(const q3tts_request* reqs, int n, const q3tts_sampling& sp, q3tts_event_cb cb, void* user, bool more_follows) {
    Q3_CHECK(n >= 1 && n <= opts_.max_batch, 3, "Invalid input: batch size must be between 1 and max_batch");
    check_row_sampling(sp, n);
    if (lanes_.size() == 1) {
        Engine* e = free_context();
        return (e == ctx1_.get() ? Engine::kJobSlots : 0) + e->begin(reqs, n, sp, cb, user, nullptr, more_follows, background_);
    }
    int slot = -1;
    for (int i = 0; i < Engine::kJobSlots; ++i)
        if (!parked_[i].busy) slot = i;
    Q3_CHECK(slot >= 0, 3, "Invalid input: two jobs are already outstanding (q3tts_generate_end must be called first)");
    parked_[slot].results.assign(size_t(n), q3tts_result{});
    generate(reqs, n, sp, cb, user, parked_[slot].results.data(), nullptr);
    parked_[slot].timing = timing;
    parked_[slot].busy = true;
    return slot;
}

void EngineGroup::end(int job, q3tts_result* results) {
    if (lanes_.size() == 1) {
        Q3_CHECK(job >= 0 && job < 2 * Engine::kJobSlots, 3, "Invalid input: no such outstanding job");
        Engine& e = job >= Engine::kJobSlots ? *ctx1_ : *lanes_[0];
        e.end(job % Engine::kJobSlots, results);
        timing = e.timing;
        return;
    }
    Q3_CHECK(job >= 0 && job < Engine::kJobSlots && parked_[job].busy, 3, "Invalid input: no such outstanding job");
    std::copy(parked_[job].results.begin(), parked_[job].results.end(), results);  // buffers change owner
    timing = parked_[job].timing;
    parked_[job].results.clear();
    parked_[job].busy = false;
}

template <class F>
void EngineGroup::run_lanes(int L, bool serial, F&& fn) {
    std::vector<std::string> errs((size_t)(L));
    std::vector<int> codes((size_t)(L), 0);
    auto run = [&](int i) {
        try {
            fn(i);
        } catch (const Error& ex) {
            errs[size_t(i)] = ex.what();
            codes[size_t(i)] = ex.status;
        } catch (const std::exception& ex) {
            errs[size_t(i)] = ex.what();
            codes[size_t(i)] = 7;
        }
    };
    if (serial) {
        for (int i = 0; i < L; ++i) run(i);
    } else {
        std::vector<std::thread> th;
        for (int i = 0; i < L; ++i) th.emplace_back(run, i);
        for (auto& t : th) t.join();
    }
    for (int i = 0; i < L; ++i)
        if (codes[size_t(i)]) throw Error(codes[size_t(i)], errs[size_t(i)]);
}

Voice* EngineGroup::create_voice(const float* audio, int64_t n_samples, const int32_t* ref_text_ids, int n_ref_text_ids, int sample_rate) {
    std::unique_ptr<Voice> v = lane0().create_voice(audio, n_samples, ref_text_ids, n_ref_text_ids, sample_rate);
    timing = lanes_[0]->timing;
    v->owner = this;
    voices_.push_back(std::move(v));
    return voices_.back().get();
}

bool EngineGroup::mine(const Voice* v) const {
    for (const auto& p : voices_)
        if (p.get() == v) return true;
    return false;
}

void EngineGroup::free_voice(Voice* v) {
    for (size_t i = 0; i < voices_.size(); ++i)
        if (voices_[i].get() == v) {
            prefix_cache_.drop(v);  // (no call is running: a saved state is read only inside a queued call)
            voices_.erase(voices_.begin() + ptrdiff_t(i));
            return;
        }
}

void EngineGroup::check_voices(const q3tts_request* reqs, int n, const Voice* const* voices) const {
    if (!voices) return;
    for (int i = 0; i < n; ++i) {
        if (!voices[i]) continue;
        Q3_CHECK(mine(voices[i]), 3,
                 "Invalid input: the voice of request " + std::to_string(i) + " was not created on this model handle (or has been freed)");
        Q3_CHECK(reqs[i].ref_audio == nullptr && reqs[i].ref_text_ids == nullptr, 3,
                 "Invalid input: request " + std::to_string(i) + " names a voice and carries ref_audio / ref_text_ids as well");
    }
}

void EngineGroup::generate(const q3tts_request* reqs, int n, const q3tts_sampling& sp, q3tts_event_cb cb, void* user,
                           q3tts_result* results, const DebugOpts* dbg, const Voice* const* voices) {
    Q3_CHECK(n >= 1 && n <= opts_.max_batch, 3, "Invalid input: batch size must be between 1 and max_batch");
    check_row_sampling(sp, n);
    check_voices(reqs, n, voices);
    const int L = int(lanes_.size());
    // contiguous split: lane i takes rows [lo_i, hi_i)
    std::vector<int> lo((size_t)(L + 1), 0);
    const int per = n / L, rem = n % L;
    for (int i = 0; i < L; ++i) lo[size_t(i) + 1] = lo[size_t(i)] + per + (i < rem ? 1 : 0);
    std::vector<Engine*> eng((size_t)(L));
    for (int i = 0; i < L; ++i) eng[size_t(i)] = lanes_[size_t(i)].get();
    if (L == 1) eng[0] = free_context();  // one lane: the call runs on the context that has no job outstanding
    run_lanes(L, L == 1 || n == 1, [&](int i) {
        const int a = lo[size_t(i)], b = lo[size_t(i) + 1];
        if (b <= a) return;
        Engine& e = *eng[size_t(i)];
        e.row_offset = uint32_t(a);
        e.request_base = a;
        DebugOpts d;
        const DebugOpts* dp = nullptr;
        if (dbg) {  // slice the per-row debug arrays
            const TalkerConfig& t = model_->cfg.talker;
            d = *dbg;
            const size_t fr = size_t(dbg->frames);
            if (d.forced_codes) d.forced_codes += size_t(a) * fr * 16;
            if (d.sampled) d.sampled += size_t(a) * fr * 16;
            if (d.talker_logits) d.talker_logits += size_t(a) * fr * t.vocab_size;
            if (d.cp_logits) d.cp_logits += size_t(a) * fr * (t.num_code_groups - 1) * t.cp.vocab_size;
            dp = &d;
        }
        q3tts_sampling ls = sp;  // the lane's rows are requests [a, b): their entries of the per-request array
        if (ls.per_request) ls.per_request += a;
        e.generate(reqs + a, b - a, ls, cb, user, results + a, dp, voices ? voices + a : nullptr);
    });
    // aggregate timing: lanes run concurrently, so spans are maxima and volumes are sums
    timing = q3tts_timing{};
    for (int i = 0; i < L; ++i) {
        if (lo[size_t(i) + 1] <= lo[size_t(i)]) continue;
        const q3tts_timing& t = eng[size_t(i)]->timing;
        timing.prefill_ms = std::max(timing.prefill_ms, t.prefill_ms);
        timing.decode_ms = std::max(timing.decode_ms, t.decode_ms);
        timing.codec_ms = std::max(timing.codec_ms, t.codec_ms);
        timing.frontend_ms = std::max(timing.frontend_ms, t.frontend_ms);
        timing.first_audio_ms = std::max(timing.first_audio_ms, t.first_audio_ms);
        timing.frame_steps = std::max(timing.frame_steps, t.frame_steps);
        timing.launches_per_frame_step = std::max(timing.launches_per_frame_step, t.launches_per_frame_step);
        timing.rows += t.rows;
        timing.kv_bytes_read += t.kv_bytes_read;
    }
}

namespace {
// q3tts_generate_queued's request source: the call's list, handed out in index order (every lane's loop takes from it)
struct ClosedSource : RequestSource {
    const std::vector<ResolvedRequest>* reqs = nullptr;
    std::vector<SamplingParams> params;  // [n] every request's folded sampling parameters
    q3tts_result* results = nullptr;
    std::atomic<int> next{0};
    bool take(QueueItem& out) override {
        if (next.load() >= int(reqs->size())) return false;
        const int i = next.fetch_add(1);
        if (i >= int(reqs->size())) return false;
        out.ticket = i;
        out.rr = (*reqs)[size_t(i)];
        out.params = params[size_t(i)];
        return true;
    }
    q3tts_result* result(int ticket) override { return results + ticket; }
};
}  // namespace

// what a closed queue and a session check alike before the slot loop starts (status 3, nothing touched)
void EngineGroup::check_queue_open(int slots, const q3tts_sampling& sp) const {
    Q3_CHECK(slots >= 1 && slots <= opts_.max_batch, 3, "Invalid input: slots must be between 1 and max_batch");
    // chunks cut after a request's end (audio_window_frames == 0) give a queue nothing: its AUDIO already leaves as soon as it is decoded
    Q3_CHECK(sp.audio_chunk_frames == 0 || sp.audio_window_frames > 0, 3,
             "Invalid input: audio_chunk_frames is not supported by q3tts_generate_queued (each request's audio is delivered whole)");
    bool outstanding = false;
    for (const auto& p : parked_) outstanding = outstanding || p.busy;
    for (const auto& l : lanes_) outstanding = outstanding || l->job_outstanding();
    outstanding = outstanding || (ctx1_ && ctx1_->job_outstanding());  // (the queued path itself runs on the first context alone)
    Q3_CHECK(!outstanding, 3, "Invalid input: a q3tts_generate_begin job is outstanding (q3tts_generate_end must be called first)");
    Q3_CHECK(model_->cfg.talker.num_code_groups == 16, 3, "Invalid input: num_code_groups must be 16");
    Q3_CHECK(sp.audio_stream_reference == 0 || (sp.audio_chunk_frames > 0 && sp.audio_window_frames > 0), 3,
             "Invalid input: audio_stream_reference needs audio_chunk_frames > 0 and audio_window_frames > 0 in q3tts_generate_queued");
}

void EngineGroup::generate_queued(const q3tts_request* reqs, int n, int slots, const q3tts_sampling& sp, q3tts_event_cb cb, void* user,
                                  q3tts_result* results, const Voice* const* voices) {
    Q3_CHECK(n >= 1, 3, "Invalid input: n_reqs must be at least 1");
    check_queue_open(slots, sp);
    check_row_sampling(sp, n);
    check_voices(reqs, n, voices);
    if (voices && sp.audio_chunk_frames > 0 && sp.audio_stream_reference == 0)  // (only on request: the result differs from the one-shot
                                                                                 // clone decode in trim and cut, include/q3tts.h)
        for (int i = 0; i < n; ++i)
            Q3_CHECK(!voices[i], 3, "Invalid input: streamed audio (audio_chunk_frames > 0) is not supported for voice requests by "
                                    "q3tts_generate_queued_voices");
    // every request is checked before any GPU work: a bad one late in the queue must not fail after the others were delivered
    std::vector<ResolvedRequest> rr;
    rr.reserve(size_t(n));
    for (int i = 0; i < n; ++i) {
        try {
            rr.push_back(lanes_[0]->check_queued(reqs[i], sp, voices ? voices[i] : nullptr));
        } catch (const Error& e) {
            throw Error(e.status, std::string(e.what()) + " (request " + std::to_string(i) + ")");
        }
    }
    if (sp.audio_chunk_frames > 0)  // a streamed queue: the causal tail's history must fit into a chunk (as a streamed q3tts_generate)
        lanes_[0]->check_stream_chunk(sp.audio_chunk_frames);
    ClosedSource src;
    src.reqs = &rr;
    src.results = results;
    for (int i = 0; i < n; ++i) src.params.push_back(fold_sampling(sp, i, 0u));  // (a queued slot keys on row_key_, not on row0)
    QueueShared q;
    q.src = &src;
    q.row_base = sp.row_base;
    for (const auto& r : rr)
        if (r.voice) q.voice_ref_max = std::max(q.voice_ref_max, r.ref_T);
    if (sp.audio_stream_reference != 0 && sp.audio_chunk_frames > 0) {
        q.stream_reference = true;
        q.ref_max = std::max(0, q.voice_ref_max);
        q.prefix_cache = debug_env().no_prefix_cache ? nullptr : &prefix_cache_;
    }
    // each lane runs a slot pool of its own; all of them take requests from the one queue
    const int L = int(lanes_.size());
    std::vector<int> pool((size_t)(L));
    for (int i = 0; i < L; ++i) pool[size_t(i)] = slots / L + (i < slots % L ? 1 : 0);
    run_lanes(L, L == 1 || slots == 1, [&](int i) {
        if (pool[size_t(i)] > 0) lanes_[size_t(i)]->run_queued(q, pool[size_t(i)], sp, cb, user);
    });
    // lanes run concurrently: spans are maxima; volumes (frame-step replays, prefills, decodes, bytes) are sums
    timing = q3tts_timing{};
    for (int i = 0; i < L; ++i) {
        if (pool[size_t(i)] == 0) continue;
        const q3tts_timing& t = lanes_[size_t(i)]->timing;
        timing.prefill_ms += t.prefill_ms;
        timing.decode_ms = std::max(timing.decode_ms, t.decode_ms);
        timing.codec_ms += t.codec_ms;
        if (t.first_audio_ms > 0) timing.first_audio_ms = timing.first_audio_ms > 0 ? std::min(timing.first_audio_ms, t.first_audio_ms) : t.first_audio_ms;
        timing.frame_steps += t.frame_steps;
        timing.launches_per_frame_step = std::max(timing.launches_per_frame_step, t.launches_per_frame_step);
        timing.kv_bytes_read += t.kv_bytes_read;
    }
    timing.rows = n;
}

// ------------------------------------------------------------------------------------------------
// serving session (q3tts_session_*)
// ------------------------------------------------------------------------------------------------
static void free_one_result(q3tts_result* r) {
    std::free(r->pcm);
    std::free(r->codes);
    r->pcm = nullptr;
    r->codes = nullptr;
}

Session::Session(EngineGroup& g, Engine& lane, const q3tts_session_opts& so, const q3tts_sampling& sp, q3tts_event_cb cb, void* user)
    : g_(g), lane_(lane), slots_(so.slots), max_ref_frames_(std::max(0, so.max_ref_frames)), sp_(sp), cb_(cb), user_(user),
      queue_(so.max_pending, &free_one_result) {
    sp_.per_request = nullptr;  // (a submit brings its own overrides)
    thread_ = std::thread([this] { loop(); });
}

Session::~Session() {
    try {
        (void)close(false);
    } catch (const std::exception&) {  // (destroyed from its own callback: nothing can join the thread from there)
        if (thread_.joinable()) thread_.detach();
    }
}

std::string Session::error() const {
    std::lock_guard<std::mutex> lk(err_mu_);
    return error_;
}

void Session::loop() {
    int status = 0;
    std::string what;
    try {
        QueueShared q;
        q.src = this;
        q.row_base = sp_.row_base;
        q.voice_ref_max = max_ref_frames_ > 0 ? max_ref_frames_ : -1;
        if (sp_.audio_stream_reference != 0 && sp_.audio_chunk_frames > 0) {
            q.stream_reference = true;
            q.ref_max = max_ref_frames_;
            q.prefix_cache = debug_env().no_prefix_cache ? nullptr : &g_.prefix_cache();
        }
        lane_.run_queued(q, slots_, sp_, cb_, user_);
    } catch (const Error& e) {
        status = e.status;
        what = e.what();
    } catch (const std::exception& e) {
        status = 7;
        what = e.what();
    }
    if (status) {  // every pending and running ticket completes with it; submit and close return it from here on
        {
            std::lock_guard<std::mutex> lk(err_mu_);
            error_ = what;
        }
        queue_.fail(status);
    }
}

void Session::submit(const q3tts_request& r, const Voice* voice, const q3tts_row_sampling* rs, int64_t* ticket) {
    if (voice) {
        Q3_CHECK(g_.mine(voice), 3, "Invalid input: the voice was not created on this model handle (or has been freed)");
        Q3_CHECK(r.ref_audio == nullptr && r.ref_text_ids == nullptr, 3,
                 "Invalid input: the request names a voice and carries ref_audio / ref_text_ids as well");
        Q3_CHECK(voice->ref_T <= max_ref_frames_, 3,
                 "Invalid input: the voice's reference is longer than the session's max_ref_frames");
        Q3_CHECK(sp_.audio_chunk_frames == 0 || sp_.audio_stream_reference != 0, 3,
                 "Invalid input: streamed audio (audio_chunk_frames > 0) is not supported for voice requests unless the session "
                 "was opened with audio_stream_reference");
    }
    q3tts_sampling one = sp_;
    one.per_request = rs;
    check_row_sampling(one, 1);
    Item it;
    it.rr = lane_.check_queued(r, sp_, voice);
    it.params = fold_sampling(one, 0, 0u);  // (a queued slot keys on its ticket, not on row0)
    const int st = queue_.submit(std::move(it), ticket);
    if (st == Q3TTS_ERR_BUSY) throw Error(st, "Session busy: max_pending requests are already waiting");
    if (st == Q3TTS_OK) return;
    const std::string why = error();
    throw Error(st, why.empty() ? std::string("Invalid input: the session is closing or has run out of tickets") : why);
}

void Session::submit_open(const q3tts_request& r, const q3tts_row_sampling* rs, int64_t* ticket) {
    Q3_CHECK(r.ref_audio == nullptr && r.ref_text_ids == nullptr, 3,
             "Invalid input: an open-text request cannot be a voice-clone request (the ICL prompt holds the whole text)");
    Q3_CHECK(r.text_ids && r.n_text_ids >= 4, 3,
             "Invalid input: text_ids of an open-text request must hold the 3 role tokens and at least one content token (no tail)");
    q3tts_sampling one = sp_;
    one.per_request = rs;
    check_row_sampling(one, 1);
    Item it;
    it.rr = lane_.check_queued(r, sp_, nullptr, true);
    it.params = fold_sampling(one, 0, 0u);
    const int n_content = int(it.rr.text_ids.size()) - 3;
    const int st = queue_.submit(std::move(it), ticket, true, n_content, lane_.text_cap());
    if (st == Q3TTS_ERR_BUSY) throw Error(st, "Session busy: max_pending requests are already waiting");
    if (st == Q3TTS_OK) return;
    const std::string why = error();
    throw Error(st, why.empty() ? std::string("Invalid input: the session is closing or has run out of tickets") : why);
}

void Session::append_text(int64_t ticket, const int32_t* ids, int32_t n, bool final) {
    Q3_CHECK(n >= 0 && (n == 0 || ids), 3, "Invalid input: n must not be negative (and ids not null)");
    const int V = g_.model().cfg.talker.text_vocab_size;  // (the token map, where there is one, has an entry for each of them)
    for (int32_t i = 0; i < n; ++i) Q3_CHECK(ids[i] >= 0 && ids[i] < V, 3, "Invalid input: text token id out of range");
    std::string why;
    const int st = queue_.append_text(ticket, ids, n, final, &why);
    if (st == Q3TTS_OK) return;
    if (why.empty()) why = error();
    throw Error(st, why.empty() ? std::string("Invalid input: the append was refused") : why);
}

void Session::take_appends(std::vector<TextAppend>& out) {
    std::vector<SessionQueue<Item>::TextMsg> msgs;
    queue_.take_appends(msgs);
    out.clear();
    for (auto& m : msgs) {
        out.emplace_back();
        out.back().ticket = int(m.ticket);
        out.back().ids = std::move(m.ids);
        out.back().final = m.final;
    }
}

void Session::wait(int64_t ticket, int32_t timeout_ms, q3tts_result* out, int32_t* ready) {
    Q3_CHECK(!on_loop_thread(), 3, "Invalid input: q3tts_session_wait inside an event callback would wait for the thread it runs on");
    Q3_CHECK(out && ready, 3, "Invalid input: null argument");
    const int st = queue_.wait(ticket, timeout_ms, out, ready);
    Q3_CHECK(st == Q3TTS_OK, st, "Invalid input: no such ticket (never given out, or its result has been collected)");
}

int Session::close(bool drain) {
    Q3_CHECK(!on_loop_thread(), 3, "Invalid input: q3tts_session_close inside an event callback would join the thread it runs on");
    queue_.close(drain);
    if (thread_.joinable()) thread_.join();
    return queue_.failed();
}

bool Session::take(QueueItem& out) {
    int64_t t = -1;
    Item it;
    SessionQueue<Item>::TextTake text;
    if (!queue_.take(&t, &it, &text)) return false;
    if (text.open) {  // what was appended while it waited is part of its text; closed already: the ordinary request it now is
        it.rr.text_ids.insert(it.rr.text_ids.end(), text.early.begin(), text.early.end());
        it.rr.target_token_count = int(it.rr.text_ids.size()) - 3;
        if (text.closed) {
            it.rr.text_open = false;
            it.rr.max_frames = final_text_cap(it.rr.open_max_tokens, it.rr.open_force_frames, it.rr.target_token_count);
        }
    }
    out.ticket = int(t);
    out.rr = std::move(it.rr);
    out.params = it.params;
    return true;
}

void Session::take_cancels(std::vector<int>& out) {
    std::vector<int64_t> t;
    queue_.take_cancels(t);
    out.assign(t.begin(), t.end());
}

Session* EngineGroup::open_session(const q3tts_session_opts& so, const q3tts_sampling& sp, q3tts_event_cb cb, void* user) {
    Q3_CHECK(!session_, 3, "Invalid input: a session is already open on this model handle");
    Q3_CHECK(lanes_.size() == 1, 3, "Invalid input: q3tts_session_open is not supported with n_streams > 1");
    Q3_CHECK(so.max_pending >= 0 && so.max_ref_frames >= 0, 3, "Invalid input: max_pending / max_ref_frames must not be negative");
    check_queue_open(so.slots, sp);
    if (sp.audio_chunk_frames > 0) lanes_[0]->check_stream_chunk(sp.audio_chunk_frames);
    lanes_[0]->drain();
    session_ = std::make_unique<Session>(*this, *lanes_[0], so, sp, cb, user);
    return session_.get();
}

int EngineGroup::close_session(bool drain) {
    if (!session_) return 0;
    const int st = session_->close(drain);  // (throws, and leaves the session open, when called from its own callback)
    if (st) last_error = session_->error();
    session_.reset();
    return st;
}

}  // namespace q3
