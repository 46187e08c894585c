// engine_queue.cc -- continuous batching (q3tts_generate_queued, q3tts_session_*): the slot loop. See engine.h.
#include "engine_stream.h"
#include "frontend.h"

namespace q3 {

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
    q.src->text_progress(starved_count(sl), 0);
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

// The slot loop of one run_queued call. Slot s owns KV pages [s * max_pages_, (s + 1) * max_pages_) for the whole call. Every
// burst boundary:
//   retire   rows whose finished flag is up: codes copied to the host, slot freed; their decode waits for the codec stream
//   admit    free slots take the next requests (in request order), prefilled as a sub-batch of their own (admit())
//   burst    frame steps of all `slots` rows, ending no later than the frame at which the first running row reaches its cap
// and, while the burst runs, a decode batch that has landed is delivered (INFO / AUDIO, results) and, the codec stream being
// idle, every retired row waiting is decoded in one batch beside the frame loop (the confined stream of a pipelined job).
// Per call and per lane: the lanes of a closed queue each run one of their own against the shared QueueShared.
struct Engine::QueueRun {
    struct Audio;
    Engine& e;
    QueueShared& q;
    const int S;
    const q3tts_sampling& sp;
    const q3tts_event_cb cb;
    void* const user;
    const double t_call;
    const bool open_text;  // (a session) rows may starve: the frame end reads text_open_ and raises starved_
    const int up, burst_frames;  // up: the handle's samples per frame
    int up_of(const ResolvedRequest& rq) const { return rq.hs ? e.codec_->upsample_of(rq.hs) : up; }  // the request's own
    // ---- destruction order: members go in reverse, so whatever ends the call
    //   audio     first: its SlotStream closes the runner's stream and drains the codec stream before the buffers its passes
    //             read and write are freed (the same order inside Audio);
    //   dec_guard then gives back the job slot of a decode batch an exception left in flight;
    //   keys      last: the samplers' row keys and the open-text flags are the engine's own again.
    struct Keys {  // the samplers of every frame step of the call key on the slots' request indices
        Engine& e;
        Keys(Engine& eng, bool open_text) : e(eng) {
            e.frame_row_key_ = e.row_key_;
            if (open_text) e.frame_text_open_ = e.text_open_;
        }
        ~Keys() { e.frame_row_key_ = nullptr; e.frame_text_open_ = nullptr; }
    } keys;
    std::vector<QSlot> sl;
    std::unordered_map<int, QLive> live;  // every admitted request whose result is not filled yet, by ticket
    std::vector<int> settled;             // results filled since the last boundary: forgotten there
    std::deque<int> waiting;              // retired, decode not started
    int dec = -1;  // job slot of the decode batch in flight (all are free: no begin job is outstanding)
    struct DecodeGuard {
        QueueRun& r;
        ~DecodeGuard() {
            if (r.dec < 0) return;
            (void)hipEventSynchronize(r.e.jobs_[r.dec].ev_codec[1]);
            r.e.release_job(r.e.jobs_[r.dec]);
        }
    } dec_guard{*this};
    hipGraphExec_t ge = nullptr;
    std::vector<int32_t> h_nframes;
    std::vector<uint8_t> h_fin, h_starved;
    std::vector<int> cancels;
    int64_t kvb = 0;
    int launched = 0, served = 0;
    double prefill_ms = 0, codec_ms = 0;
    std::unique_ptr<Audio> audio;  // streamed audio (audio_chunk_frames > 0), else nullptr

    QueueRun(Engine& eng, QueueShared& shared, int slots, const q3tts_sampling& sampling, q3tts_event_cb cb_, void* user_, double t0);
    void loop();
    q3tts_timing finish();

    const bool live_voices;  // (a session with live voices) front ends run on the engine's live lanes beside the slot loop
    std::vector<RequestSource::VoiceJob> vjobs;
    int burst_steps = 0;  // the burst in flight: its frame steps, its launch time, whether a voice job ran beside it
    bool burst_beside = false;
    double burst_t0 = 0;
    void voices_boundary();
    void launch_voice_jobs();
    void forget_settled();
    void apply_cancels();
    int admit_boundary();
    bool idle(bool all_starved);
    void launch_burst(int burst, int admitted);
    void while_burst_runs();
    void read_back(int burst);
    void retire();
    void deliver(bool wait);
    void decode(bool overlapped);
    void drain_decodes() {
        while (dec >= 0 || !waiting.empty()) {
            if (dec >= 0) deliver(true);
            else decode(false);
        }
    }
    void fill_result(int req, q3tts_status status, float* pcm);
};

// ---- streamed audio (audio_chunk_frames > 0 with audio_window_frames > 0): every request's chunks leave while it generates ----
// A slotted codec stream over the S slots decodes them; retired rows do not go through the decode batches: a request's AUDIO is
// the concatenation of its chunks, INFO and AUDIO fire once the last one has landed. Only requests held back at a chunk that
// left the fp16 range are decoded again (fp32), behind the loop.
// Voice requests (audio_stream_reference): a slot's code row holds the voice's reference frames, then the generated ones. The
// reference is decoded as the row's prefix at the admission (nothing of it is delivered) unless the state it leaves in the
// causal tail has been saved before: then one launch puts it back (PrefixCache).
struct Engine::QueueRun::Audio {
    QueueRun& r;
    Engine& e;
    const int S, stride;      // frames per row of scodes
    DevBuf<int32_t> scodes;   // [S][stride][16]: the codes the stream reads, copied from codes_ burst by burst
    std::vector<int> held;    // complete but held back, for the fp32 re-decode
    std::vector<int> zombies;  // cancelled requests whose chunks may still be in flight
    std::vector<int> avail, n_ref;  // per slot, a boundary's staging
    std::vector<uint8_t> fin;
    std::vector<const int32_t*> ref;
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
    std::unique_ptr<SlotStream> ss;  // (last: destroyed first, see QueueRun)

    explicit Audio(QueueRun& run)
        : r(run), e(run.e), S(run.S), stride(e.Fcap_ + run.q.ref_max), avail(size_t(S), 0), n_ref(size_t(S), 0), fin(size_t(S), 0),
          ref(size_t(S), nullptr) {
        scodes.grow(size_t(S) * stride * 16);
        if (r.q.prefix_cache) add_flags();
        open();
        // a session with live voices: the place of every pool slot's saved state, once, before the loop's first boundary
        VoicePool* pool = r.q.prefix_cache ? r.q.src->voice_pool() : nullptr;
        if (pool && pool->state_bytes == 0 && e.codec_->stream_state_bytes() > 0) {
            pool->state_bytes = align_up(e.codec_->stream_state_bytes(), 256);
            pool->states.grow(size_t(pool->n_slots) * pool->state_bytes);
        }
    }
    void open() {
        ss.reset();
        ss = std::make_unique<SlotStream>(e, S, r.sp.audio_chunk_frames, r.sp.audio_window_frames, std::max(0, r.sp.audio_lookahead_frames),
                                          e.Fcap_, true, r.q.ref_max);
        ss->t_call = r.t_call;
        if (r.cb)
            ss->on_chunk = [this](int req, int, const float* pcm, int64_t n, int64_t off) {
                std::unique_lock<std::mutex> lk = e.cb_lock();
                audio_chunk(r.cb, r.user, req, pcm, n, off);
            };
        ss->on_complete = [this](int req) {
            SlotStream::Out& o = ss->out[req];
            if (r.live.at(req).frames == 0) r.fill_result(req, Q3TTS_ERR_GENERATION_FAILED, o.pcm.release());  // Qwen3.swift:939-941
            else if (o.held_from >= 0) held.push_back(req);
            else r.fill_result(req, Q3TTS_OK, o.pcm.release());
        };
    }
    void add_flags() {
        const size_t n = size_t(2) * S;
        state_flags.emplace_back();
        int32_t* b = state_flags.back().grow(n);
        std::memset(b, 0, n * 4);
        for (size_t i = n; i-- > 0;) free_flags.push_back(b + i);
    }
    void settle(bool wait);
    void forget(const std::vector<int>& settled);
    void admit_rows(const std::vector<int>& fresh);
    void save_states(const std::vector<int>& primed, PrefixCache::Key key);
    void feed();
    void take_all() {  // every chunk in flight, whatever it takes
        while (ss->take(true)) {}
        settle(true);
    }
    void redo_held(std::unordered_map<int, SlotStream::Out>& outs);
    void redo_held_and_reopen();
    // a voice is being released: a state of it whose save has not settled yet must never be published -- the next voice may get
    // this one's address
    void drop_voice(const Voice* v) {
        for (PendingState& p : pending)
            if (p.entry->voice == v) p.entry->of(nullptr);
    }
};

// saved states whose save has run: into the cache, unless the prefix left the fp16 range
void Engine::QueueRun::Audio::settle(bool wait) {
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
        if (*pending[i].flag == 0 && pending[i].entry->voice) r.q.prefix_cache->publish(pending[i].entry);  // (voice gone: drop_voice)
        free_flags.push_back(pending[i].flag);
        pending.erase(pending.begin() + ptrdiff_t(i));
    }
}

void Engine::QueueRun::Audio::forget(const std::vector<int>& settled) {
    for (int t : settled) ss->out.erase(t);
    for (size_t i = 0; i < zombies.size();)
        if (!ss->in_flight(zombies[i])) {
            ss->out.erase(zombies[i]);
            zombies.erase(zombies.begin() + ptrdiff_t(i));
        } else {
            ++i;
        }
}

// New occupants of the slots `fresh`: the row's chunks, history margins and non-finite flag start over, in codec-stream order.
void Engine::QueueRun::Audio::admit_rows(const std::vector<int>& fresh) {
    settle(false);  // (before this boundary's admissions take flags)
    bool any_ref = false;
    std::fill(n_ref.begin(), n_ref.end(), 0);
    for (int s : fresh) {
        const ResolvedRequest& rq = r.live.at(r.sl[size_t(s)].req).rr;
        if (!rq.voice || !r.q.stream_reference || rq.ref_T <= 0) continue;
        ref[size_t(s)] = rq.voice->codes_dev;
        n_ref[size_t(s)] = rq.ref_T;
        any_ref = true;
    }
    // the voices' reference frames to the front of their slots' code rows: behind ev_pushed where the row had an occupant
    if (any_ref) ss->stage_prefixes(ref.data(), n_ref.data(), e.codes_, e.Fcap_, scodes, stride, e.st_);
    PrefixCache::Key key{nullptr, 0, r.sp.audio_chunk_frames, r.sp.audio_window_frames, std::max(0, r.sp.audio_lookahead_frames),
                         e.codec_->stream_path(), e.codec_->stream_state_bytes()};
    std::vector<int> primed;
    for (int s : fresh) {
        const int req = r.sl[size_t(s)].req, R = n_ref[size_t(s)];
        const ResolvedRequest& rq = r.live.at(req).rr;
        key.of(rq.voice);
        key.hs = rq.hs;  // (a state is valid for the hop it was made with: keyed, so a voice has one per hop in use)
        std::shared_ptr<PrefixCache::Entry> hit = R > 0 && r.q.prefix_cache ? r.q.prefix_cache->find(key) : nullptr;
        if (hit) {
            Q3_HIP(hipStreamWaitEvent(ss->cst, hit->ready, 0));
            ss->admit(s, req, rq.max_frames, R, hit->blob, rq.hs);
            ++r.q.prefix_cache->restored;
            in_use.push_back(std::move(hit));
        } else {
            ss->admit(s, req, rq.max_frames, R, nullptr, rq.hs);
            if (R > 0) primed.push_back(s);
        }
    }
    if (primed.empty()) return;
    // the prefixes need no generated frame: they are decoded now, before the row's first generated chunk can follow them, and
    // the state they leave is taken at once. The other rows have what the last push gave them.
    for (int s = 0; s < S; ++s) avail[size_t(s)] = r.sl[size_t(s)].req >= 0 ? ss->copied[size_t(s)] : 0;
    std::fill(fin.begin(), fin.end(), uint8_t(0));
    ss->push(scodes, stride, avail.data(), fin.data());
    save_states(primed, key);
}

// the tail states the primed prefixes have just left, right behind the push that decoded them
void Engine::QueueRun::Audio::save_states(const std::vector<int>& primed, PrefixCache::Key key) {
    for (int s : primed) {
        Q3_CHECK(!e.codec_->stream_in_prefix(s), 7, "internal error: a reference prefix was left undecoded at its admission");
        if (!r.q.prefix_cache || key.bytes == 0) continue;
        const Voice* vc = r.live.at(r.sl[size_t(s)].req).rr.voice;
        // A session-made voice keeps one state, in its pool slot's place (no allocation here, and none to free when the voice
        // goes); an anonymous one none, since no other ticket can name it. Every further admission of such a voice primes again.
        const bool pooled = vc->pool && vc->pool_slot >= 0 && vc->pool.get() == r.q.src->voice_pool();
        if (pooled && (vc->anonymous || vc->state_taken || key.bytes > vc->pool->state_bytes)) continue;
        auto n = std::make_shared<PrefixCache::Entry>();
        key.of(vc);
        key.hs = r.live.at(r.sl[size_t(s)].req).rr.hs;
        static_cast<PrefixCache::Key&>(*n) = key;
        if (pooled) {
            const_cast<Voice*>(vc)->state_taken = true;  // (this thread alone reads and writes it)
            n->pool = vc->pool;
            n->blob = vc->pool->states + size_t(vc->pool_slot) * vc->pool->state_bytes;
        } else {
            n->blob = n->own.grow(key.bytes);
        }
        Q3_HIP(hipEventCreateWithFlags(&n->ready, hipEventDisableTiming));
        if (free_flags.empty()) add_flags();  // (settle(false) returned what it could)
        int32_t* flag = free_flags.back();
        free_flags.pop_back();
        *flag = 0;
        e.codec_->stream_save_row(s, n->blob);
        e.codec_->stream_row_flag(s, flag);
        Q3_HIP(hipEventRecord(n->ready, ss->cst));
        pending.push_back(PendingState{std::move(n), flag});
    }
}

// the new frames of every running slot into the stream's own code buffer, then every chunk they allow
void Engine::QueueRun::Audio::feed() {
    for (int s = 0; s < S; ++s) {
        const bool on = r.sl[size_t(s)].req >= 0;
        avail[size_t(s)] = on ? std::min(r.h_nframes[size_t(s)], e.Fcap_) : 0;
        fin[size_t(s)] = on && r.h_fin[size_t(s)] ? 1 : 0;
    }
    ss->stage_frames(avail.data(), e.codes_, e.Fcap_, scodes, stride, e.st_);
    ss->push(scodes, stride, avail.data(), fin.data());  // a retiring row's remaining chunks are all issued here
}

// Requests held back at a chunk that left the fp16 range: once more on the fp32 matrix cores, as redo_rows_fp32 does for a
// streamed job: chunks below the held one stay as delivered, the rest (events included) come from the exact decode.
// (Behind ss->finish(): the runner's stream is closed, `outs` holds the stream's requests.)
void Engine::QueueRun::Audio::redo_held(std::unordered_map<int, SlotStream::Out>& outs) {
    for (size_t h0 = 0; h0 < held.size(); h0 += size_t(e.Bm_)) {
        const int R = int(std::min(held.size() - h0, size_t(e.Bm_)));
        // (a voice request streamed behind its reference: the decoder sees reference ++ generated, as in every clone decode,
        // and the request's samples start exactly ref_T frames in)
        std::vector<int> dframes((size_t)(R)), refs((size_t)(R), 0);
        std::vector<const QLive*> w((size_t)(R));
        for (int i = 0; i < R; ++i) {
            w[size_t(i)] = &r.live.at(held[h0 + i]);
            if (w[size_t(i)]->rr.voice && r.q.stream_reference) refs[size_t(i)] = w[size_t(i)]->rr.voice->ref_T;
            dframes[size_t(i)] = refs[size_t(i)] + w[size_t(i)]->frames;
        }
        const bool widest = e.codec_->fp32_convs();  // already the fp32 kernels: nothing wider to fall back to
        std::vector<int> hs;  // every request is decoded again at its own speed
        bool own = false;
        for (int i = 0; i < R; ++i) {
            own = own || w[size_t(i)]->rr.hs != 0;
            hs.push_back(w[size_t(i)]->rr.hs ? w[size_t(i)]->rr.hs : e.codec_->stretch_hs());
        }
        ExactDecode d;
        if (!widest)
            d = e.decode_rows_fp32(dframes, [&w, &refs, &dframes](int i, int32_t* dst, hipStream_t) {
                const int ref = refs[size_t(i)];
                if (ref > 0) Q3_HIP(hipMemcpy(dst, w[size_t(i)]->rr.voice->codes_host.data(), size_t(ref) * 64, hipMemcpyHostToDevice));
                Q3_HIP(hipMemcpy(dst + size_t(ref) * 16, w[size_t(i)]->codes.data(), size_t(dframes[size_t(i)] - ref) * 64, hipMemcpyHostToDevice));
            }, own ? &hs : nullptr);
        for (int i = 0; i < R; ++i) {
            const int req = held[h0 + i];
            SlotStream::Out& o = outs.at(req);
            if (widest || d.nf[i]) {  // never hand out a waveform with holes in it
                r.fill_result(req, Q3TTS_ERR_AUDIO_DECODING_FAILED, o.pcm.release());
                e.last_error = kCodecRangeMsg;
                continue;
            }
            const int64_t rup = r.up_of(w[size_t(i)]->rr);  // (the request's own samples per frame; d.up is the decode's layout)
            const int64_t step = int64_t(r.sp.audio_chunk_frames) * rup, ns = int64_t(w[size_t(i)]->frames) * rup;
            e.refire_held(o.pcm.get(), d.pcm + size_t(i) * d.Fd * d.up + size_t(refs[size_t(i)]) * rup, std::min(ns, int64_t(o.held_from) * step), ns, step,
                          r.cb, r.user, req);
            r.fill_result(req, Q3TTS_OK, o.pcm.release());
        }
    }
    held.clear();
}

// (a session that is idle) the fp32 re-decode needs the runner: the slotted stream is closed around it
void Engine::QueueRun::Audio::redo_held_and_reopen() {
    std::unordered_map<int, SlotStream::Out> outs = std::move(ss->out);
    ss->finish();
    in_use.clear();
    redo_held(outs);
    open();  // (no row of the new stream has had an occupant)
    zombies.clear();
}

Engine::QueueRun::QueueRun(Engine& eng, QueueShared& shared, int slots, const q3tts_sampling& sampling, q3tts_event_cb cb_, void* user_,
                           double t0)
    : e(eng), q(shared), S(slots), sp(sampling), cb(cb_), user(user_), t_call(t0), open_text(shared.src->open_text()),
      up(eng.codec_->upsample()), burst_frames(std::max(1, eng.max_inflight_frames / 2)), keys(eng, open_text), sl(size_t(slots)),
      h_nframes(size_t(slots), 0), h_fin(size_t(slots), 0), h_starved(size_t(slots), 0), live_voices(shared.src->live_voices()) {
    if (open_text) {
        Q3_HIP(hipMemsetAsync(e.text_open_, 0, size_t(S), e.st_));
        Q3_HIP(hipMemsetAsync(e.starved_, 0, size_t(S), e.st_));
    }
    ge = e.opts_.use_graph ? e.frame_graph(S) : nullptr;
    Q3_HIP(hipStreamSynchronize(e.st_));
    if (sp.audio_chunk_frames > 0) audio = std::make_unique<Audio>(*this);
}

// as end() fills a row; pcm: ownership passes
void Engine::QueueRun::fill_result(int req, q3tts_status status, float* pcm) {
    const QLive& w = live.at(req);
    q3tts_result* rp = q.src->result(req);
    Q3_CHECK(rp != nullptr, 7, "internal error: a streamed request has no result to fill");
    MallocPtr<float> own(pcm);
    struct Settle {  // however this ends, the result is the source's from here on
        QueueRun& r;
        int req;
        ~Settle() {
            r.q.src->complete(req);
            r.settled.push_back(req);
        }
    } settle_req{*this, req};
    fill_info(*rp, w.rr.target_token_count, w.frames, w.span, device_memory_gb());
    rp->status = status;
    if (status != Q3TTS_OK) return;
    rp->codes = static_cast<int32_t*>(std::malloc(size_t(w.frames) * 16 * 4));
    if (!rp->codes) throw Error(5, "out of host memory for the results");
    std::memcpy(rp->codes, w.codes.data(), size_t(w.frames) * 16 * 4);
    rp->n_frames = w.frames;
    rp->n_samples = int64_t(w.frames) * up_of(w.rr);  // all generated frames: what has left cannot be trimmed (include/q3tts.h)
    rp->pcm = own.release();
    if (!cb) return;
    std::unique_lock<std::mutex> lk = e.cb_lock();
    emit_info_audio(cb, user, req, *rp);
}

// end(): results[i] and INFO / AUDIO of every row of the batch (fp32 re-decode included)
void Engine::QueueRun::deliver(bool wait) {
    if (!wait) {
        std::lock_guard<std::mutex> lk(e.stage_mu_);
        if (e.jobs_[dec].stage == 1) return;  // the staging thread has not copied it out yet
    }
    const int j = dec;
    dec = -1;
    const std::vector<int> batch = e.jobs_[j].req_index;
    e.end(j, nullptr);
    codec_ms += e.timing.codec_ms;
    for (int t : batch) {
        q.src->complete(t);
        live.erase(t);
    }
}

// every waiting row (up to max_batch) in one decode on the codec stream
void Engine::QueueRun::decode(bool overlapped) {
    Job& J = e.jobs_[0];
    const int R = std::min(int(waiting.size()), e.Bm_), Fcap = e.Fcap_;
    J.reset(R, up);
    {
        std::vector<int> hs;
        for (int b = 0; b < R; ++b) hs.push_back(live.at(waiting[size_t(b)]).rr.hs);
        e.set_row_speeds(J, hs);
    }
    J.req_index.assign(size_t(R), 0);
    J.row_out.assign(size_t(R), nullptr);
    J.row_span.assign(size_t(R), 0);
    J.codes_host.assign(size_t(R) * Fcap * 16, 0);
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
        std::copy(w.codes.begin(), w.codes.end(), J.codes_host.begin() + ptrdiff_t(size_t(b) * Fcap * 16));
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
    e.start_decode(J, dframes, overlapped, J.codes_host.data());
    dec = 0;
    e.publish_job(J, cb, user, 0, t_call, true);  // copied out by the staging thread while the frame loop goes on
}

// results filled at the last boundary are forgotten
void Engine::QueueRun::forget_settled() {
    for (int t : settled) live.erase(t);
    if (audio) audio->forget(settled);
    settled.clear();
}

// cancelled rows (a session) leave their slots
void Engine::QueueRun::apply_cancels() {
    q.src->take_cancels(cancels);
    uint64_t mask = 0;
    for (int t : cancels) {
        int s = -1;
        for (int i = 0; i < S; ++i)
            if (sl[size_t(i)].req == t) s = i;
        if (s >= 0) {  // running: its slot is an empty one from this boundary on, and no event of it fires any more
            mask |= uint64_t(1) << s;
            if (audio) {
                audio->ss->drop(s);
                audio->zombies.push_back(t);
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
    if (open_text) q.src->text_progress(starved_count(sl), 0);  // (a cancelled row may have been one that waited for text)
    e.cancel_slots(mask, S);  // on st_: in front of the admissions below and of the next read of the flags
}

// admission: free slots in slot order take the next requests in request order; streamed: their rows of the stream start over
int Engine::QueueRun::admit_boundary() {
    std::vector<int> fresh;
    if (audio)
        for (int s = 0; s < S; ++s)
            if (sl[size_t(s)].req < 0) fresh.push_back(s);
    const int admitted = e.admit(q, sl, live);
    served += admitted;
    if (audio) {
        fresh.erase(std::remove_if(fresh.begin(), fresh.end(), [this](int s) { return sl[size_t(s)].req < 0; }), fresh.end());
        audio->admit_rows(fresh);
    }
    return admitted;
}

// No frame step can be launched: every running row waits for text and nothing could be admitted (all_starved), or nothing runs
// at all. What has landed is delivered -- decode batches of retired rows and, streamed, the chunks in flight (a starved row is
// not final: its last chunks wait with it) -- and the thread sleeps: all_starved, until an append, a cancel, a request it can
// admit, or close; with nothing running, until a submit. A streamed request held back for the fp32 re-decode waits until
// nothing runs: the stream cannot be closed around rows that are still in it. false: the call is over.
bool Engine::QueueRun::idle(bool all_starved) {
    if (!all_starved && !q.src->open_ended()) return false;
    if (live_voices) {  // no row takes a frame step: waiting jobs start at once, and a job in flight is simply waited for
        launch_voice_jobs();
        if (e.live_in_flight() > 0) {
            if (!all_starved) {
                e.live_poll(*q.src, true);
                return true;
            }
            // rows are waiting for text: their appends, cancels and landed chunks must not wait for a lane, so the lanes are
            // polled at boundaries a millisecond apart while a job is in flight (no frame step is taken for it)
            drain_decodes();
            if (audio) audio->take_all();
            if (!settled.empty()) return true;
            bool room = false;
            for (const QSlot& x : sl) room = room || x.req < 0;
            q.src->wait_for_text(room, 1);
            return true;
        }
    }
    drain_decodes();
    if (audio) {
        audio->take_all();
        if (!all_starved && !audio->held.empty()) audio->redo_held_and_reopen();
    }
    if (!settled.empty()) return true;  // (forgotten at the top of the loop)
    if (!all_starved) return q.src->wait_for_work();
    bool can_admit = false;
    for (const QSlot& x : sl) can_admit = can_admit || x.req < 0;
    q.src->wait_for_text(can_admit);
    return true;
}

void Engine::QueueRun::launch_burst(int burst, int admitted) {
    for (int f = 0; f < burst; ++f) {
        if (ge) Q3_HIP(hipGraphLaunch(ge, e.st_));
        else e.enqueue_frame(S, nullptr);
    }
    launched += burst;
    q.src->progress(burst, admitted);
    if (live_voices) {  // (its end is seen in while_burst_runs)
        burst_steps = burst;
        burst_beside = e.live_in_flight() > 0;
        burst_t0 = now_s();
    }
    Q3_HIP(hipMemcpyAsync(h_nframes.data(), e.n_frames_, size_t(S) * 4, hipMemcpyDeviceToHost, e.st_));
    Q3_HIP(hipMemcpyAsync(h_fin.data(), e.finished_, size_t(S), hipMemcpyDeviceToHost, e.st_));
    if (open_text) Q3_HIP(hipMemcpyAsync(h_starved.data(), e.starved_, size_t(S), hipMemcpyDeviceToHost, e.st_));
    Q3_HIP(hipEventRecord(e.burst_ev_[0], e.st_));
}

// while the burst runs: deliver the decode batch that has landed, start the next one
void Engine::QueueRun::while_burst_runs() {
    if (live_voices) {
        launch_voice_jobs();
        burst_beside = burst_beside || e.live_in_flight() > 0;  // (a job launched now runs beside this burst)
    }
    if (dec >= 0) deliver(false);
    if (dec < 0 && !waiting.empty()) decode(true);
    if (audio) {  // chunks that have landed leave while the burst runs, without waiting for them
        for (;;) {
            const hipError_t bq = hipEventQuery(e.burst_ev_[0]);
            if (bq != hipErrorNotReady) {
                Q3_HIP(bq);
                break;
            }
            if (!audio->ss->take(false)) std::this_thread::yield();
        }
    }
    Q3_HIP(hipEventSynchronize(e.burst_ev_[0]));
    if (live_voices) q.src->burst_done(burst_steps, (now_s() - burst_t0) * 1e3, burst_beside);
}

// the burst's flags on the host: rows that wait for text are no finished ones, and have taken fewer steps than were launched
void Engine::QueueRun::read_back(int burst) {
    const StarveCount c = after_burst(sl, burst, h_nframes.data(), h_fin.data(), h_starved.data(), open_text);
    if (open_text) q.src->text_progress(c.starved_now, c.starve_events);
}

// Live voices at a boundary: the lanes' events are polled (never waited for), and the voices nothing uses any more give their
// places back. Neither touches the device: no synchronisation, no allocation, no free.
void Engine::QueueRun::voices_boundary() {
    if (e.live_in_flight() > 0) e.live_poll(*q.src, false);
    q.src->release_voices([this](const Voice* v) {
        if (audio) audio->drop_voice(v);
    });
}

// waiting front-end jobs onto the free lanes (while a burst runs, or at once when no row runs)
void Engine::QueueRun::launch_voice_jobs() {
    const int free_lanes = int(e.live_lanes_.size()) - e.live_in_flight();
    if (free_lanes <= 0 || !q.src->has_voice_work()) return;
    q.src->take_voice_jobs(vjobs, free_lanes);
    for (RequestSource::VoiceJob& j : vjobs)
        for (LiveLane& L : e.live_lanes_)
            if (L.id < 0) {
                e.live_launch(L, j);
                break;
            }
    vjobs.clear();
}

// TOKEN events (generation order), retirement
void Engine::QueueRun::retire() {
    bool any_retired = false;
    std::vector<int> retiring;  // streamed: rows retired at this boundary
    const double now = now_s();
    for (int s = 0; s < S; ++s) {
        QSlot& x = sl[size_t(s)];
        if (x.req < 0) continue;
        const int nf = h_nframes[size_t(s)];
        if (cb) e.emit_tokens(cb, user, s, x.req, nf, x.reported);
        if (!h_fin[size_t(s)]) continue;
        // copied out before the slot's next admission resets its row (stream order on st_)
        QLive& w = live.at(x.req);
        if (!audio) waiting.push_back(x.req);
        w.frames = nf;
        w.span = now - x.t0;
        w.codes.assign((size_t)(nf) * 16, 0);
        if (nf > 0)
            Q3_HIP(hipMemcpyAsync(w.codes.data(), e.codes_ + size_t(s) * e.Fcap_ * 16, size_t(nf) * 64, hipMemcpyDeviceToHost, e.st_));
        kvb += e.kv_bytes(x.np, nf);
        if (audio) retiring.push_back(s);
        x = QSlot{};
        any_retired = true;
    }
    if (any_retired) Q3_HIP(hipStreamSynchronize(e.st_));  // (the codes are on the host before the stream takes a row for complete)
    for (int s : retiring) audio->ss->retire(s, std::min(h_nframes[size_t(s)], e.Fcap_));  // (complete at once when its chunks have landed)
}

void Engine::QueueRun::loop() {
    Q3_HIP(hipEventRecord(e.ev_[2], e.st_));
    for (;;) {
        forget_settled();
        if (q.src->has_cancels()) apply_cancels();
        if (live_voices) voices_boundary();  // in front of the admission: it sees the voices that have just become ready
        const int admitted = admit_boundary();
        // open-text requests: what has been appended since the last boundary, in front of the burst, in stream order on st_
        if (open_text && q.src->has_appends()) e.apply_text_appends(q, sl, live);
        const BurstPlan p = burst_length(sl, burst_frames);
        if (p.runnable == 0) {
            if (!idle(p.running > 0)) break;
            continue;
        }
        launch_burst(p.burst, admitted);
        while_burst_runs();
        read_back(p.burst);
        if (audio) audio->feed();
        if (admitted) {
            float ms = 0;
            Q3_HIP(hipEventElapsedTime(&ms, e.ev_[0], e.ev_[1]));
            prefill_ms += ms;
        }
        retire();
    }
}

// the last decode batches (nothing overlaps them any more), the stream's last passes and held requests; the call's timing
q3tts_timing Engine::QueueRun::finish() {
    Q3_HIP(hipEventRecord(e.ev_[3], e.st_));
    Q3_HIP(hipStreamSynchronize(e.st_));
    drain_decodes();
    q3tts_timing tm{};
    if (audio) {
        audio->zombies.clear();
        audio->ss->finish();  // the passes still in flight; every request is complete behind this
        audio->settle(true);
        audio->in_use.clear();
        codec_ms = audio->ss->codec_ms;
        tm.first_audio_ms = audio->ss->first_audio_ms;
        audio->redo_held(audio->ss->out);
    }
    float loop_ms = 0;
    Q3_HIP(hipEventElapsedTime(&loop_ms, e.ev_[2], e.ev_[3]));
    tm.prefill_ms = prefill_ms;
    tm.decode_ms = std::max(0.0, double(loop_ms) - prefill_ms);
    tm.codec_ms = codec_ms;
    tm.frame_steps = launched;
    tm.rows = served;
    tm.kv_bytes_read = kvb;
    tm.launches_per_frame_step = e.launches_per_step(S);
    return tm;
}

void Engine::run_queued(QueueShared& q, int S, const q3tts_sampling& sp, q3tts_event_cb cb, void* user) {
    Q3_HIP(hipSetDevice(m_->device));
    Q3_CHECK(S >= 1 && S <= Bm_, 3, "Invalid input: slots must be between 1 and max_batch");
    Q3_CHECK(!job_outstanding(), 3, "Invalid input: a q3tts_generate_begin job is outstanding (q3tts_generate_end must be called first)");
    ensure_queue_ws();
    // an admission's voice rows go through extra_: room for S rows with the longest reference, so that no boundary allocates
    if (q.voice_ref_max >= 0) extra_.grow(size_t(S) * (1 + q.voice_ref_max) * m_->cfg.talker.hidden_size);
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
    // every slot's entry holds the call's own values until an admission writes its request's (an empty slot's sampler returns
    // early, but reads its entry with the other operands first)
    q3tts_sampling call_wide = sp;
    call_wide.per_request = nullptr;
    upload_sampling(call_wide, 0u, S);
    build_cp_proj_tables();
    QueueRun run(*this, q, S, sp, cb, user, t_call);  // keys set, frame graph, the upload above waited for, streamed: the stream opened
    run.loop();
    if (run.live_voices) live_poll(*q.src, true);  // (a close without drain: the launched jobs finish)
    timing = run.finish();
}

// ------------------------------------------------------------------------------------------------
// live voices: Engine::create_voice's sequence on a lane of its own, enqueued and polled by the slot loop
// ------------------------------------------------------------------------------------------------
int64_t Engine::check_voice_clip(const float* audio, int64_t n_samples, const int32_t* ref_text_ids, int n_ref_text_ids, int sample_rate) const {
    const TalkerConfig& t = m_->cfg.talker;
    if (sample_rate != kResampleNative)
        Q3_CHECK(resample_pair_supported(sample_rate, kResampleNative), 3,
                 "Invalid input: a voice's sample_rate must be 8000, 12000, 16000, 22050, 24000, 32000, 44100 or 48000");
    check_reference(audio, n_samples, ref_text_ids, n_ref_text_ids);
    Q3_CHECK(fe_ != nullptr, 1, "Model not initialized: Speech tokenizer encoder not available");
    Q3_CHECK(m_->codec_enc.bins <= t.vocab_size && m_->codec_enc.bins <= t.cp.vocab_size, 3,
             "Invalid input: encoder codebook larger than the codec embedding tables");
    for (int i = 0; i < n_ref_text_ids; ++i)
        Q3_CHECK(ref_text_ids[i] >= 0 && ref_text_ids[i] < t.text_vocab_size, 3, "Invalid input: reference text token id out of range");
    int64_t n24 = n_samples;
    if (sample_rate != kResampleNative) {
        Q3_CHECK(n_samples <= (int64_t(1) << 28), 3, "Invalid input: resampling takes between 1 and 2^28 samples");
        const int g = resample_detail::gcd(sample_rate, kResampleNative);
        const int64_t L = kResampleNative / g, M = sample_rate / g;
        n24 = (n_samples * L + M - 1) / M;
    }
    fe_->check_clip(n24);
    return n24;
}

void Engine::live_open(int lanes, int max_ref_frames) {
    Q3_HIP(hipSetDevice(m_->device));
    Q3_CHECK(fe_ != nullptr && m_->has_codec_encoder, 1, "Model not initialized: Speech tokenizer encoder not available");
    const int H = m_->cfg.talker.hidden_size;
    // the longest clip whose encoding has max_ref_frames frames, and the longest one at another rate that resamples to it
    int64_t n24 = 0;
    for (int64_t step = int64_t(1) << 23; step > 0; step >>= 1)
        if (n24 + step <= (int64_t(1) << 24) && fe_->encoded_frames(n24 + step) <= max_ref_frames) n24 += step;
    Q3_CHECK(n24 >= 1, 3, "Invalid input: max_ref_frames admits no clip");
    live_max_24_ = n24;
    live_max_in_ = 2 * n24 + 8;  // (48 kHz: two input samples per 24 kHz sample)
    for (int rate : {8000, 12000, 16000, 22050, 32000, 44100, 48000}) (void)resampler(rate, kResampleNative);  // tables on the device now
    live_close();  // (lanes a failed open left behind)
    live_lanes_.resize(size_t(lanes));
    for (LiveLane& L : live_lanes_) {
        Q3_HIP(hipStreamCreateWithFlags(&L.fe.st, hipStreamNonBlocking));
        Q3_HIP(hipEventCreateWithFlags(&L.fe.done, hipEventDisableTiming));
        Q3_HIP(hipEventCreate(&L.t0));
        Q3_HIP(hipEventCreate(&L.t1));
        L.fe.fe = std::make_unique<VoiceFrontEnd>(*m_, L.fe.st);
        L.fe.fe->reserve(live_max_24_);
        L.fe.spk.grow(size_t(H));
        L.in.grow(size_t(live_max_in_));
        L.a24.grow(size_t(live_max_24_));
        L.len.grow(4);
        L.stage_len = align_up(size_t(live_max_in_) * 4, 256);
        L.stage_codes = L.stage_len + 256;
        L.stage.grow(L.stage_codes + size_t(max_ref_frames) * 64);
    }
}

void Engine::live_close() {
    if (live_lanes_.empty()) return;
    (void)hipSetDevice(m_->device);
    for (LiveLane& L : live_lanes_) {
        if (L.fe.st) (void)hipStreamSynchronize(L.fe.st);
        if (L.fe.done) (void)hipEventDestroy(L.fe.done);
        if (L.t0) (void)hipEventDestroy(L.t0);
        if (L.t1) (void)hipEventDestroy(L.t1);
        L.fe.fe.reset();
        if (L.fe.st) (void)hipStreamDestroy(L.fe.st);
    }
    live_lanes_.clear();
}

int Engine::live_in_flight() const {
    int n = 0;
    for (const LiveLane& L : live_lanes_) n += L.id >= 0;
    return n;
}

// Upload, the centred resample for a clip at another rate, encode, speaker embedding, f32 -> bf16, the reference frames'
// embedding sums, the codes back to pinned memory, an event: everything enqueued on the lane's stream, nothing waited for.
void Engine::live_launch(LiveLane& L, RequestSource::VoiceJob& job) {
    const int H = m_->cfg.talker.hidden_size;
    Voice& v = *job.voice;
    const int64_t n_in = int64_t(job.clip.size()), n24 = v.n_ref_samples;
    const int T = v.ref_T;
    Q3_CHECK(n_in <= live_max_in_ && n24 <= live_max_24_ && size_t(T) * 64 <= L.stage.capacity() - L.stage_codes, 7,
             "internal error: a live voice's clip beyond the lanes' reservation");
    hipStream_t st = L.fe.st;
    std::memcpy(L.stage, job.clip.data(), size_t(n_in) * 4);
    job.clip = std::vector<float>();
    Q3_HIP(hipMemcpyAsync(L.in, L.stage, size_t(n_in) * 4, hipMemcpyHostToDevice, st));
    const float* a = L.in;
    if (job.rate != kResampleNative) {
        const ResamplerDev& r = resampler(job.rate, kResampleNative);  // (built by live_open)
        int32_t* hl = reinterpret_cast<int32_t*>(L.stage + L.stage_len);
        *hl = int32_t(n_in);
        Q3_HIP(hipMemcpyAsync(L.len, hl, 4, hipMemcpyHostToDevice, st));
        ResampleArgs ra{};
        ra.x = L.in; ra.x_bstride = 0;
        ra.y = L.a24; ra.y_bstride = 0;
        ra.len = L.len; ra.len_mul = 1; ra.max_in = n_in;
        ra.tab = r.tab; ra.L = r.plan.L; ra.M = r.plan.M; ra.K = r.plan.K;
        ra.hist = 0; ra.centred = 1; ra.clamp = 0; ra.B = 1;
        launch_resample(ra, st);
        a = L.a24;
    }
    Q3_HIP(hipEventRecord(L.t0, st));
    L.fe.fe->encode(a, n24, v.codes_dev);
    if (m_->has_speaker_encoder) {
        L.fe.fe->speaker_embedding(a, n24, L.fe.spk);
        launch_f32_to_bf16(L.fe.spk, v.rows_dev, H, st);
    } else {
        Q3_HIP(hipMemsetAsync(v.rows_dev, 0, size_t(H) * 2, st));
    }
    launch_ref_embed_rows(v.codes_dev, T, 16, m_->codec_emb, m_->cp_emb_dev, H, v.rows_dev + size_t(H), H, st);
    Q3_HIP(hipEventRecord(L.t1, st));
    Q3_HIP(hipMemcpyAsync(L.stage + L.stage_codes, v.codes_dev, size_t(16) * T * 4, hipMemcpyDeviceToHost, st));
    Q3_HIP(hipEventRecord(L.fe.done, st));
    L.id = job.id;
    L.voice = job.voice;
}

void Engine::live_poll(RequestSource& src, bool wait) {
    for (LiveLane& L : live_lanes_) {
        if (L.id < 0) continue;
        if (wait) {
            Q3_HIP(hipEventSynchronize(L.fe.done));
        } else {
            const hipError_t pq = hipEventQuery(L.fe.done);
            if (pq == hipErrorNotReady) continue;
            Q3_HIP(pq);
        }
        Voice& v = *L.voice;
        const int T = v.ref_T;
        const int32_t* rows = reinterpret_cast<const int32_t*>(L.stage + L.stage_codes);  // [16][T]
        v.code0.assign(rows, rows + T);
        v.codes_host.resize(size_t(T) * 16);
        for (int f = 0; f < T; ++f)
            for (int g = 0; g < 16; ++g) v.codes_host[size_t(f) * 16 + g] = rows[size_t(g) * T + f];
        float ms = 0;
        Q3_HIP(hipEventElapsedTime(&ms, L.t0, L.t1));
        v.state.store(Voice::kReady, std::memory_order_release);  // from here on the voice is read-only: any context, any lane
        const int64_t id = L.id;
        L.id = -1;
        L.voice = nullptr;
        src.voice_done(id, double(ms));
    }
}

}  // namespace q3
