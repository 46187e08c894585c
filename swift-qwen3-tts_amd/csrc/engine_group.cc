// engine_group.cc -- EngineGroup (the model and its engines), the closed queue's request source and the serving session. See engine.h.
#include "engine.h"

#include <algorithm>

#include "codec.h"

namespace q3 {

// ------------------------------------------------------------------------------------------------
// EngineGroup
// ------------------------------------------------------------------------------------------------
EngineGroup::EngineGroup(std::unique_ptr<Model> model, const q3tts_load_opts& opts, float pitch, bool keep_formants) : model_(std::move(model)), opts_(opts) {
    int lanes = opts.n_streams;
    // Measured: a lane's frame step takes ~4-5 ms whatever its batch size (latency-bound chain), and
    // n concurrent chains overlap by 1.6x (n=2) / 2.2x (n=4). Splitting ONE batch into lanes therefore never pays -- each
    // lane's chain is as long as the whole batch's. Two WHOLE batches on two chains do: that is the second job context below.
    if (lanes <= 0) lanes = 1;
    lanes = std::max(1, std::min(lanes, opts.max_batch));
    q3tts_load_opts lo = opts;
    lo.max_batch = ceil_div(opts.max_batch, lanes);
    for (int i = 0; i < lanes; ++i) {
        lanes_.push_back(std::make_unique<Engine>(model_.get(), lo, pitch, keep_formants));
        lanes_.back()->cb_mutex = &cb_mutex_;
        // keep the sum of queued kernel packets of all lanes well under the 16k-entry AQL queue (~650 nodes per frame)
        lanes_.back()->max_inflight_frames = std::max(2, 12000 / 650 / lanes);
    }
    speakers = lanes_[0]->speakers;
    if (lanes == 1) {
        // The second job context: a full engine of its own (stream, workspace, KV pool, frame graphs, codec runner) on the
        // shared model. Allocated here, at load, so that no steady-state step allocates; include/q3tts.h states the memory.
        ctx1_ = std::make_unique<Engine>(model_.get(), lo, pitch, keep_formants);
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
    return adopt_voice(std::move(v));
}

Voice* EngineGroup::adopt_voice(std::unique_ptr<Voice> v) {
    std::lock_guard<std::mutex> lk(voices_mu_);
    v->owner = this;
    voices_.push_back(std::move(v));
    return voices_.back().get();
}

bool EngineGroup::mine(const Voice* v) const {
    std::lock_guard<std::mutex> lk(voices_mu_);
    for (const auto& p : voices_)
        if (p.get() == v) return true;
    return false;
}

void EngineGroup::free_voice(Voice* v) {
    std::unique_ptr<Voice> gone;
    {
        std::lock_guard<std::mutex> lk(voices_mu_);
        for (size_t i = 0; i < voices_.size(); ++i)
            if (voices_[i].get() == v) {
                // (no call that reads the voice is running: a saved state is read only inside a queued call; a session releases a
                // voice only when no ticket names it)
                prefix_cache_.drop(v);
                gone = std::move(voices_[i]);
                voices_.erase(voices_.begin() + ptrdiff_t(i));
                break;
            }
    }
}

void EngineGroup::check_voices(const q3tts_request* reqs, int n, const Voice* const* voices) const {
    if (!voices) return;
    for (int i = 0; i < n; ++i) {
        if (!voices[i]) continue;
        Q3_CHECK(mine(voices[i]), 3,
                 "Invalid input: the voice of request " + std::to_string(i) + " was not created on this model handle (or has been freed)");
        Q3_CHECK(voices[i]->state.load(std::memory_order_acquire) == Voice::kReady, 3,
                 "Invalid input: the voice of request " + std::to_string(i) + " was abandoned by a session closed without drain");
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

Session::Session(EngineGroup& g, Engine& lane, const q3tts_session_opts_ex& so, const q3tts_sampling& sp, q3tts_event_cb cb, void* user)
    : g_(g), lane_(lane), slots_(so.base.slots), max_ref_frames_(std::max(0, so.base.max_ref_frames)), live_voices_(so.live_voices),
      max_voices_(so.live_voices > 0 ? (so.max_voices > 0 ? so.max_voices : 4 * so.base.slots) : 0), sp_(sp), cb_(cb), user_(user),
      queue_(so.base.max_pending, &free_one_result) {
    sp_.per_request = nullptr;  // (a submit brings its own overrides)
    if (live_voices_ > 0) {  // everything a live voice needs on the device, now: no boundary allocates
        const size_t H = size_t(g_.model().cfg.talker.hidden_size);
        pool_ = std::make_shared<VoicePool>(max_voices_, align_up(size_t(64) * max_ref_frames_, 256) + 2 * H * (size_t(1) + max_ref_frames_));
        lane_.live_open(live_voices_, max_ref_frames_);
        queue_.enable_voices(live_voices_, max_voices_);
    }
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

int64_t Session::voice_id(const Voice* v) const {
    std::lock_guard<std::mutex> lk(vmu_);
    auto it = vids_.find(v);
    return it == vids_.end() ? -1 : it->second;
}

Voice* Session::create_voice(const float* audio, int64_t n_samples, int sample_rate, const int32_t* ref_text_ids, int n_ref_text_ids,
                             bool anonymous) {
    Q3_CHECK(live_voices_ > 0, 3, "Invalid input: the session was opened without live_voices (q3tts_session_open_ex)");
    const int64_t n24 = lane_.check_voice_clip(audio, n_samples, ref_text_ids, n_ref_text_ids, sample_rate);
    const int T = lane_.encoded_frames(n24);
    Q3_CHECK(T >= 1 && T <= max_ref_frames_, 3, "Invalid input: the clip is longer than the session's max_ref_frames");
    const size_t H = size_t(g_.model().cfg.talker.hidden_size);
    auto v = std::make_unique<Voice>();
    v->state.store(Voice::kPending);
    v->ref_T = T;
    v->n_ref_samples = n24;
    v->ref_text_ids.assign(ref_text_ids, ref_text_ids + n_ref_text_ids);
    v->device_bytes = int64_t(size_t(16) * T * 4 + size_t(1 + T) * H * 2);
    v->anonymous = anonymous;
    ClipJob job;
    job.clip.assign(audio, audio + n_samples);
    job.rate = sample_rate;
    // one creator at a time from here on: a call that is about to be refused for live_voices holds its slot where no other
    // creator can miss it
    std::unique_lock<std::mutex> lk(vmu_);
    const int slot = pool_->take();
    if (slot < 0) throw Error(Q3TTS_ERR_BUSY, "Session busy: max_voices voices are alive");
    v->pool = pool_;
    v->pool_slot = slot;
    uint8_t* base = pool_->mem + size_t(slot) * pool_->slot_bytes;
    v->codes_dev = reinterpret_cast<int32_t*>(base);
    v->rows_dev = reinterpret_cast<uint16_t*>(base + align_up(size_t(64) * max_ref_frames_, 256));
    int64_t id = -1;
    const int st = queue_.submit_voice(std::move(job), v.get(), &id, anonymous);
    if (st == Q3TTS_OK) {  // (vmu_ is held: a release on the loop thread finds the voice in vids_ and among the group's)
        Voice* p = g_.adopt_voice(std::move(v));
        vids_[p] = id;
        return p;
    }
    v.reset();  // (never launched: its place goes back, still under vmu_)
    lk.unlock();
    if (st == Q3TTS_ERR_BUSY) throw Error(st, "Session busy: live_voices front-end jobs are in flight, or max_voices voices are alive");
    const std::string why = error();
    throw Error(st, why.empty() ? std::string("Invalid input: the session is closing") : why);
}

void Session::voice_wait(const Voice* v, int32_t timeout_ms, int32_t* ready) {
    Q3_CHECK(!on_loop_thread(), 3, "Invalid input: q3tts_session_voice_wait inside an event callback would wait for the thread it runs on");
    Q3_CHECK(v && ready, 3, "Invalid input: null argument");
    const int64_t id = voice_id(v);
    Q3_CHECK(id >= 0, 3, "Invalid input: not a voice of this session (or it has been released)");
    const int st = queue_.voice_wait(id, timeout_ms, ready);
    if (st == Q3TTS_ERR_CANCELLED) throw Error(st, "Cancelled: the voice's front end was abandoned");
    Q3_CHECK(st == Q3TTS_OK, st, "Invalid input: the voice has been freed");
}

void Session::free_voice(const Voice* v, bool count) {
    const int64_t id = voice_id(v);
    Q3_CHECK(id >= 0, 3, "Invalid input: not a voice of this session (or it has been released)");
    Q3_CHECK(queue_.free_voice(id, count) == Q3TTS_OK, 3, "Invalid input: the voice has been freed already");
}

int Session::take_voice_jobs(std::vector<VoiceJob>& out, int max) {
    std::vector<SessionQueue<Item, ClipJob>::VoiceTake> jobs;
    queue_.take_voice_jobs(jobs, max);
    out.clear();
    for (auto& j : jobs) {
        out.emplace_back();
        out.back().id = j.id;
        out.back().voice = static_cast<Voice*>(j.tag);
        out.back().clip = std::move(j.job.clip);
        out.back().rate = j.job.rate;
    }
    return int(out.size());
}

// on the loop thread, at a boundary: host memory and the pool's free list alone (a session-made voice's saved state lies in its
// pool slot's place and is recycled with it)
void Session::release_voices(const std::function<void(const Voice*)>& before) {
    std::vector<std::pair<int64_t, void*>> rel;
    queue_.take_voice_releases(rel);
    for (auto& kv : rel) {
        Voice* v = static_cast<Voice*>(kv.second);
        if (before) before(v);
        {
            std::lock_guard<std::mutex> lk(vmu_);
            vids_.erase(v);
        }
        g_.free_voice(v);
        queue_.voice_released(kv.first);
    }
}

void Session::submit(const q3tts_request& r, const Voice* voice, const q3tts_row_sampling* rs, int64_t* ticket) {
    if (r.ref_audio != nullptr && live_voices_ > 0) {  // an anonymous voice, this ticket's alone: freed when the ticket is done
        Q3_CHECK(!voice, 3, "Invalid input: the request names a voice and carries ref_audio / ref_text_ids as well");
        const Voice* av = create_voice(r.ref_audio, r.n_ref_samples, kResampleNative, r.ref_text_ids, r.n_ref_text_ids, true);
        q3tts_request named = r;
        named.ref_audio = nullptr;
        named.n_ref_samples = 0;
        named.ref_text_ids = nullptr;
        named.n_ref_text_ids = 0;
        try {
            submit_checked(named, av, rs, ticket);
        } catch (...) {
            free_voice(av, false);
            throw;
        }
        free_voice(av, false);
        return;
    }
    submit_checked(r, voice, rs, ticket);
}

void Session::submit_checked(const q3tts_request& r, const Voice* voice, const q3tts_row_sampling* rs, int64_t* ticket) {
    int64_t vid = -1;
    if (voice) {
        Q3_CHECK(g_.mine(voice), 3, "Invalid input: the voice was not created on this model handle (or has been freed)");
        vid = voice_id(voice);
        Q3_CHECK(vid >= 0 || voice->state.load(std::memory_order_acquire) == Voice::kReady, 3,
                 "Invalid input: the voice was abandoned by a session closed without drain");
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
    const int st = queue_.submit(std::move(it), ticket, false, 0, 0, vid);
    if (st == Q3TTS_ERR_BUSY) throw Error(st, "Session busy: max_pending requests are already waiting");
    if (st == Q3TTS_OK) return;
    const std::string why = error();
    if (vid >= 0 && why.empty()) throw Error(st, "Invalid input: the voice has been freed or abandoned (or the session is closing)");
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
    std::vector<SessionQueue<Item, ClipJob>::TextMsg> msgs;
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
    if (live_voices_ > 0) {  // behind the loop: the lanes go, and what the queue still knows of the voices is settled
        lane_.live_close();
        std::vector<SessionQueue<Item, ClipJob>::VoiceLeft> left;
        queue_.retire_voices(left);
        for (auto& l : left) {
            Voice* v = static_cast<Voice*>(l.tag);
            if (l.freed) g_.free_voice(v);
            else v->state.store(l.state == int(SessionQueue<Item, ClipJob>::VoiceReady) ? Voice::kReady : Voice::kAbandoned);
        }
        std::lock_guard<std::mutex> lk(vmu_);
        vids_.clear();
    }
    return queue_.failed();
}

bool Session::take(QueueItem& out) {
    int64_t t = -1;
    Item it;
    SessionQueue<Item, ClipJob>::TextTake text;
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

Session* EngineGroup::open_session(const q3tts_session_opts_ex& sx, const q3tts_sampling& sp, q3tts_event_cb cb, void* user) {
    const q3tts_session_opts& so = sx.base;
    Q3_CHECK(!session_, 3, "Invalid input: a session is already open on this model handle");
    Q3_CHECK(lanes_.size() == 1, 3, "Invalid input: q3tts_session_open is not supported with n_streams > 1");
    Q3_CHECK(so.max_pending >= 0 && so.max_ref_frames >= 0, 3, "Invalid input: max_pending / max_ref_frames must not be negative");
    Q3_CHECK(sx.live_voices >= 0 && sx.live_voices <= 4, 3, "Invalid input: live_voices must be between 0 and 4");
    Q3_CHECK(sx.max_voices >= 0 && sx.max_voices <= 65536, 3, "Invalid input: max_voices must be between 0 and 65536");
    if (sx.live_voices > 0) {
        Q3_CHECK(so.max_ref_frames > 0, 3, "Invalid input: live_voices needs max_ref_frames > 0 (it bounds a clip)");
        Q3_CHECK(model_->has_codec_encoder, 1,
                 "Model not initialized: live voices require the speech tokenizer encoder. Make sure to load a model with encoder weights.");
    }
    check_queue_open(so.slots, sp);
    if (sp.audio_chunk_frames > 0) lanes_[0]->check_stream_chunk(sp.audio_chunk_frames);
    lanes_[0]->drain();
    session_ = std::make_unique<Session>(*this, *lanes_[0], sx, sp, cb, user);
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
