// api.cc -- extern "C" surface declared in include/q3tts.h. No exception crosses the boundary:
// every entry point returns a q3tts_status and records the message for q3tts_last_error().
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "codec.h"
#include "comm.h"
#include "engine.h"
#include "tokenizer.h"

using q3::EngineGroup;

struct q3tts_session {  // the handle q3tts_session_open gives out: the model's one session (EngineGroup::session())
    q3tts_model* m = nullptr;
};

struct q3tts_model {
    std::unique_ptr<EngineGroup> eng;
    std::unique_ptr<q3tts_session> session;
    // "Calls on one handle are serialised by the caller" (q3tts.h; the reference's model object is not re-entrant either). The
    // contract is checked, not assumed: a call that finds the handle inside another thread's call fails with INVALID_INPUT instead
    // of racing on the engine's state. Nested calls from the SAME thread (an event callback asking for q3tts_model_info) pass.
    std::atomic<std::thread::id> owner{std::thread::id()};
    std::atomic<int> depth{0};
};
struct q3tts_tokenizer {
    q3::BpeTokenizer tok;
};

namespace {
thread_local std::string g_load_error;
thread_local const q3tts_model* g_refused = nullptr;  // this thread's last call on that handle found it in use (HandleUse)
// submit / cancel / wait / get_stats run on any thread at once, so a refusal's message is kept per thread, not in the handle's
// one string: q3tts_last_error gives a thread the message of ITS last refused session call until its next call on the handle
thread_local std::string g_session_error;
thread_local const q3tts_model* g_session_refused = nullptr;
const char* const kBusyMsg =
    "Invalid input: the model handle is inside another thread's call (calls on one handle must be serialised by the caller)";

struct HandleUse {  // the handle's one-caller-at-a-time contract (struct q3tts_model)
    q3tts_model* m;
    bool mine = false;
    explicit HandleUse(q3tts_model* model) : m(model) {
        if (!m) return;
        const std::thread::id me = std::this_thread::get_id();
        std::thread::id none;
        if (m->owner.load(std::memory_order_acquire) == me || m->owner.compare_exchange_strong(none, me, std::memory_order_acq_rel)) {
            m->depth.fetch_add(1, std::memory_order_relaxed);
            mine = true;
        }
    }
    ~HandleUse() {
        if (m && mine && m->depth.fetch_sub(1, std::memory_order_relaxed) == 1) m->owner.store(std::thread::id(), std::memory_order_release);
    }
};

// q3tts_voice is q3::Voice behind the boundary
q3::Voice* voice_of(q3tts_voice* v) { return reinterpret_cast<q3::Voice*>(v); }
const q3::Voice* voice_of(const q3tts_voice* v) { return reinterpret_cast<const q3::Voice*>(v); }

// uses_engine: the call needs an engine, which an open session's loop thread owns: refused without touching the GPU
template <class F>
q3tts_status guarded(q3tts_model* m, F&& f, bool uses_engine = true) {
    HandleUse use(m);
    if (m && !use.mine) {
        g_refused = m;  // (not written to the engine's last_error: that string belongs to the call that is running)
        return Q3TTS_ERR_INVALID_INPUT;
    }
    if (m && g_refused == m) g_refused = nullptr;
    if (m && g_session_refused == m) g_session_refused = nullptr;
    if (m && uses_engine && m->eng && m->eng->session()) {
        m->eng->last_error = "Invalid input: a session is open on this model handle (q3tts_session_close must be called first)";
        return Q3TTS_ERR_INVALID_INPUT;
    }
    try {
        // every call on a handle runs with the handle's GPU current, whatever the calling thread had selected (a process may hold one
        // handle per GPU; allocations and per-device kernel attributes inside the call belong to THIS device)
        if (m && m->eng) Q3_HIP(hipSetDevice(m->eng->model().device));
        f();
        return Q3TTS_OK;
    } catch (const q3::Error& e) {
        if (m && m->eng) m->eng->last_error = e.what();
        else g_load_error = e.what();
        return static_cast<q3tts_status>(e.status);
    } catch (const std::exception& e) {
        if (m && m->eng) m->eng->last_error = e.what();
        else g_load_error = e.what();
        return Q3TTS_ERR_DEVICE;
    }
}
// a session call that takes the session's own lock instead of the handle's one-caller check
template <class F>
q3tts_status session_call(const q3tts_session* s, F&& f) {
    if (!s || !s->m || !s->m->eng || !s->m->eng->session()) return Q3TTS_ERR_INVALID_INPUT;
    EngineGroup& g = *s->m->eng;
    q3tts_status st = Q3TTS_OK;
    try {
        f(*g.session());
        if (g_session_refused == s->m) g_session_refused = nullptr;
        return Q3TTS_OK;
    } catch (const q3::Error& e) {
        g_session_error = e.what();
        st = static_cast<q3tts_status>(e.status);
    } catch (const std::exception& e) {
        g_session_error = e.what();
        st = Q3TTS_ERR_DEVICE;
    }
    g_session_refused = s->m;  // (the handle's own string is not touched: other threads' calls may be reading or writing theirs)
    return st;
}
}  // namespace

extern "C" {

void q3tts_default_load_opts(q3tts_load_opts* o) {
    std::memset(o, 0, sizeof(*o));
    o->device = 0;
    o->max_batch = 1;
    o->max_frames = 2048;
    o->max_prompt = 512;
    o->use_graph = 1;
    o->weights_from_broadcast = 0;
    o->n_streams = 0;
    o->codec_overlap_cus = 0;
    o->codec_fp32 = 0;
    o->output_sample_rate = 0;
    o->speed = 0.0f;
    o->request_speeds = 0;
}

void q3tts_default_load_opts_ex(q3tts_load_opts_ex* o) {
    std::memset(o, 0, sizeof(*o));
    q3tts_default_load_opts(&o->base);
    o->pitch = 0.0f;
}

void q3tts_default_load_opts_ex2(q3tts_load_opts_ex2* o) {
    std::memset(o, 0, sizeof(*o));
    q3tts_default_load_opts_ex(&o->ex);
    o->keep_formants = 0;
}

void q3tts_default_sampling(q3tts_sampling* s) {  // Qwen3.swift:1296-1299
    s->temperature = 0.9f;
    s->top_k = 50;
    s->top_p = 1.0f;
    s->repetition_penalty = 1.05f;
    s->seed = 0;
    s->force_frames = 0;
    s->audio_chunk_frames = 0;
    s->audio_window_frames = 0;
    s->audio_lookahead_frames = 4;
    s->row_base = 0;
    s->per_request = nullptr;
    s->audio_stream_reference = 0;
}

q3tts_status q3tts_model_load(const char* model_dir, const q3tts_load_opts* opts, q3tts_model** out) {
    q3tts_load_opts_ex ex;
    q3tts_default_load_opts_ex(&ex);
    if (opts) ex.base = *opts;
    return q3tts_model_load_ex(model_dir, &ex, out);
}

q3tts_status q3tts_model_load_ex(const char* model_dir, const q3tts_load_opts_ex* opts, q3tts_model** out) {
    q3tts_load_opts_ex2 ex2;
    q3tts_default_load_opts_ex2(&ex2);
    if (opts) ex2.ex = *opts;
    return q3tts_model_load_ex2(model_dir, &ex2, out);
}

q3tts_status q3tts_model_load_ex2(const char* model_dir, const q3tts_load_opts_ex2* opts, q3tts_model** out) {
    if (out) *out = nullptr;
    return guarded(nullptr, [&] {
        Q3_CHECK(model_dir && out, 3, "Invalid input: null argument");
        q3::debug_env_reload();  // the launchers' diagnostic switches are read here, once per load (kernels.h DebugEnv)
        q3tts_load_opts_ex2 ex2;
        if (opts) ex2 = *opts;
        else q3tts_default_load_opts_ex2(&ex2);
        const q3tts_load_opts_ex& ex = ex2.ex;
        const int32_t keep_formants = ex2.keep_formants;
        const q3tts_load_opts& o = ex.base;
        const float pitch = ex.pitch;
        Q3_CHECK(o.max_batch >= 1 && o.max_batch <= 64, 3, "Invalid input: max_batch must be in 1..64");
        Q3_CHECK(o.max_frames >= 1 && o.max_prompt >= 16, 3, "Invalid input: max_frames / max_prompt too small");
        // (a NaN fails every comparison: refused like a value out of range, and before the first call into the GPU runtime)
        Q3_CHECK(o.speed == 0.0f || (o.speed >= 0.5f && o.speed <= 2.0f), 3, "Invalid input: speed must be 0 (off) or between 0.5 and 2.0");
        Q3_CHECK(q3::pitch_semitones_valid(pitch), 3, "Invalid input: pitch must be 0 (off) or between -12 and 12 semitones");
        Q3_CHECK(pitch == 0.0f || o.request_speeds == 0, 3,
                 "Invalid input: pitch and request_speeds cannot be combined (a table per pair of hops)");
        Q3_CHECK(keep_formants == 0 || keep_formants == 1, 3, "Invalid input: keep_formants must be 0 or 1");
        Q3_CHECK(keep_formants == 0 || o.output_sample_rate == 0 || o.output_sample_rate == q3::kResampleNative, 3,
                 "Invalid input: keep_formants needs output_sample_rate 0 or 24000 (the synthesis filter runs at 24 kHz spacing)");
        if (pitch != 0.0f && (o.output_sample_rate == 0 || o.output_sample_rate == q3::kResampleNative ||
                                q3::resample_rate_supported(o.output_sample_rate))) {
            // no Hp in [240, 960]: refused here when no frame of 1 to 8 hops admits the combination (the codec's own frame is
            // known only once the checkpoint is read; the runner checks again with it)
            const int rate = o.output_sample_rate ? o.output_sample_rate : q3::kResampleNative;
            const int g = q3::resample_detail::gcd(q3::kResampleNative, rate);
            bool some = false;
            for (int hops = 1; hops <= 8; ++hops) some = some || q3::pitch_choose(pitch, o.speed, hops, rate / g, q3::kResampleNative / g).status == 0;
            Q3_CHECK(some, 3, "Invalid input: no hop in [240, 960] for this pitch and speed");
        }
        int ndev = 0;
        hipError_t e = hipGetDeviceCount(&ndev);
        Q3_CHECK(e == hipSuccess && ndev > 0, 7, "no HIP device available: this engine has no CPU fallback");
        Q3_CHECK(o.device >= 0 && o.device < ndev, 3, "Invalid input: device ordinal out of range");
        Q3_CHECK(o.output_sample_rate == 0 || o.output_sample_rate == q3::kResampleNative || q3::resample_rate_supported(o.output_sample_rate), 3,
                 "Invalid input: output_sample_rate must be 0, 8000, 12000, 16000, 22050, 24000, 32000, 44100 or 48000");
        q3::LoadOptions lo;
        lo.device = o.device;
        lo.max_pos_talker = o.max_prompt + o.max_frames + 8;
        lo.skip_tensor_data = o.weights_from_broadcast != 0;
        auto model = q3::load_model(model_dir, lo);
        auto h = std::make_unique<q3tts_model>();
        h->eng = std::make_unique<EngineGroup>(std::move(model), o, pitch, keep_formants != 0);
        *out = h.release();
    });
}

void q3tts_model_free(q3tts_model* m) {
    if (g_refused == m) g_refused = nullptr;  // (a later handle may be allocated at the same address)
    if (g_session_refused == m) g_session_refused = nullptr;
    if (m && m->eng) {  // an open session is closed first, without drain
        try {
            (void)m->eng->close_session(false);
        } catch (const std::exception&) {
        }
    }
    delete m;
}

const char* q3tts_last_error(const q3tts_model* m) {
    if (m && g_refused == m) return kBusyMsg;
    if (m && g_session_refused == m) return g_session_error.c_str();
    if (m && m->eng) return m->eng->last_error.c_str();
    return g_load_error.c_str();
}

q3tts_status q3tts_model_arena(q3tts_model* m, void** device_ptr, size_t* bytes) {
    return guarded(m, [&] {
        Q3_CHECK(m && device_ptr && bytes, 3, "Invalid input: null argument");
        *device_ptr = m->eng->model().arena;
        *bytes = m->eng->model().arena_bytes;
    });
}

q3tts_status q3tts_comm_get_unique_id(q3tts_comm_id* out) {
    return guarded(nullptr, [&] {
        Q3_CHECK(out, 3, "Invalid input: null argument");
        q3::comm_unique_id(out);
    });
}

q3tts_status q3tts_model_broadcast(q3tts_model* m, const q3tts_comm_id* id, int32_t rank, int32_t world, int32_t root) {
    return guarded(m, [&] {
        Q3_CHECK(m && id, 3, "Invalid input: null argument");
        q3::Model& md = m->eng->model();
        q3::comm_broadcast_arena(md.device, md.arena, md.arena_bytes, *id, rank, world, root);
    });
}

q3tts_status q3tts_model_arena_checksum(q3tts_model* m, uint64_t* out) {
    return guarded(m, [&] {
        Q3_CHECK(m && out, 3, "Invalid input: null argument");
        q3::Model& md = m->eng->model();
        *out = q3::arena_checksum(md.device, md.arena, md.arena_bytes);
    });
}

q3tts_status q3tts_model_get_info(const q3tts_model* m, q3tts_model_info* out) {
    return guarded(const_cast<q3tts_model*>(m), [&] {
        Q3_CHECK(m && out, 3, "Invalid input: null argument");
        std::memset(out, 0, sizeof(*out));
        const q3::Model& md = m->eng->model();
        const q3::ModelConfig& c = md.cfg;
        std::strncpy(out->tts_model_type, c.tts_model_type.c_str(), sizeof(out->tts_model_type) - 1);
        // the handle's output side: what the codec runner hands out (q3tts_load_opts.output_sample_rate)
        const q3::CodecRunner* cr = m->eng->codec_runner();
        out->sample_rate = cr ? cr->output_rate() : c.sample_rate;
        // supportsVoiceCloning: base model with a codec encoder (Qwen3.swift:1210-1214); hasVoiceCloning: speaker encoder (:61-63)
        out->supports_voice_cloning = (c.tts_model_type == "base" && md.has_codec && md.has_codec_encoder) ? 1 : 0;
        out->has_voice_cloning = md.has_speaker_encoder ? 1 : 0;
        out->speaker_embedding_dim = md.has_speaker_encoder ? md.speaker.enc_dim : 0;
        out->hidden_size = c.talker.hidden_size;
        out->num_layers = c.talker.num_hidden_layers;
        out->vocab_size = c.talker.vocab_size;
        out->text_vocab_size = c.talker.text_vocab_size;
        out->num_code_groups = c.talker.num_code_groups;
        out->cp_hidden_size = c.talker.cp.hidden_size;
        out->cp_num_layers = c.talker.cp.num_hidden_layers;
        out->cp_vocab_size = c.talker.cp.vocab_size;
        out->codec_eos_token_id = c.talker.codec_eos_token_id;
        out->samples_per_frame = cr ? cr->upsample() : (c.has_codec ? c.codec.total_upsample() : c.decode_upsample_rate);
        out->max_samples_per_frame = cr ? cr->max_upsample() : out->samples_per_frame;
        out->max_batch = m->eng->opts().max_batch;
        out->weight_bytes = md.step_weight_bytes;
    }, false);
}

int32_t q3tts_model_num_speakers(const q3tts_model* m) { return m ? int32_t(m->eng->speakers.size()) : 0; }
const char* q3tts_model_speaker_name(const q3tts_model* m, int32_t i) {
    if (!m || i < 0 || size_t(i) >= m->eng->speakers.size()) return nullptr;
    return m->eng->speakers[size_t(i)].c_str();
}

// q3tts_generate / _queued (slots < 0: the static path) with or without a voice per request
static q3tts_status generate_any(q3tts_model* m, const q3tts_request* reqs, const q3tts_voice* const* voices, bool with_voices,
                                 int32_t n_reqs, int32_t slots, const q3tts_sampling* sampling, q3tts_event_cb cb, void* user,
                                 q3tts_result* results) {
    return guarded(m, [&] {
        Q3_CHECK(m && reqs && results && (voices || !with_voices), 3, "Invalid input: null argument");
        q3tts_sampling sp;
        if (sampling) sp = *sampling;
        else q3tts_default_sampling(&sp);
        std::memset(results, 0, sizeof(q3tts_result) * size_t(n_reqs > 0 ? n_reqs : 0));
        std::vector<const q3::Voice*> vs;
        for (int i = 0; with_voices && i < n_reqs; ++i) vs.push_back(voice_of(voices[i]));
        const q3::Voice* const* vp = with_voices ? vs.data() : nullptr;
        if (slots < 0) m->eng->generate(reqs, n_reqs, sp, cb, user, results, nullptr, vp);
        else m->eng->generate_queued(reqs, n_reqs, slots, sp, cb, user, results, vp);
        for (int i = 0; i < n_reqs; ++i)
            if (results[i].status == Q3TTS_ERR_GENERATION_FAILED)
                m->eng->last_error = "Generation failed: No tokens generated";  // Qwen3.swift:940
    });
}

q3tts_status q3tts_generate(q3tts_model* m, const q3tts_request* reqs, int32_t n_reqs, const q3tts_sampling* sampling,
                            q3tts_event_cb cb, void* user, q3tts_result* results) {
    return generate_any(m, reqs, nullptr, false, n_reqs, -1, sampling, cb, user, results);
}

q3tts_status q3tts_generate_queued(q3tts_model* m, const q3tts_request* reqs, int32_t n_reqs, int32_t slots,
                                   const q3tts_sampling* sampling, q3tts_event_cb cb, void* user, q3tts_result* results) {
    return generate_any(m, reqs, nullptr, false, n_reqs, slots < 0 ? 0 : slots, sampling, cb, user, results);
}

q3tts_status q3tts_voice_create(q3tts_model* m, const float* ref_audio, int64_t n_ref_samples, const int32_t* ref_text_ids,
                                int32_t n_ref_text_ids, q3tts_voice** out) {
    if (out) *out = nullptr;
    return guarded(m, [&] {
        Q3_CHECK(m && out, 3, "Invalid input: null argument");
        *out = reinterpret_cast<q3tts_voice*>(m->eng->create_voice(ref_audio, n_ref_samples, ref_text_ids, n_ref_text_ids));
    });
}

q3tts_status q3tts_voice_create_rate(q3tts_model* m, const float* ref_audio, int64_t n_ref_samples, int32_t sample_rate,
                                     const int32_t* ref_text_ids, int32_t n_ref_text_ids, q3tts_voice** out) {
    if (out) *out = nullptr;
    return guarded(m, [&] {
        Q3_CHECK(m && out, 3, "Invalid input: null argument");
        *out = reinterpret_cast<q3tts_voice*>(m->eng->create_voice(ref_audio, n_ref_samples, ref_text_ids, n_ref_text_ids, sample_rate));
    });
}

q3tts_status q3tts_resample(q3tts_model* m, const float* in, int64_t n_in, int32_t in_rate, int32_t out_rate, int32_t centred, float* out,
                            int64_t cap, int64_t* n_out) {
    return guarded(m, [&] {
        Q3_CHECK(m && in && out && n_out, 3, "Invalid input: null argument");
        m->eng->lane0().resample(in, n_in, in_rate, out_rate, centred != 0, out, cap, n_out);
    });
}

q3tts_status q3tts_model_get_speed(const q3tts_model* m, float* effective_speed, int32_t* hs, int32_t* delay_samples) {
    return guarded(const_cast<q3tts_model*>(m), [&] {
        Q3_CHECK(m, 3, "Invalid input: null argument");
        const q3::CodecRunner* cr = m->eng->codec_runner();
        const int h = cr ? cr->stretch_hs() : q3::kStretchHa;
        if (effective_speed) *effective_speed = float(double(q3::kStretchHa) / double(h));
        if (hs) *hs = h;
        if (delay_samples) *delay_samples = cr ? cr->stretch_delay_samples() : 0;
    }, false);
}

q3tts_status q3tts_model_get_pitch(const q3tts_model* m, float* effective_semitones, int32_t* hp, int32_t* ho, int32_t* delay_samples) {
    return guarded(const_cast<q3tts_model*>(m), [&] {
        Q3_CHECK(m, 3, "Invalid input: null argument");
        const q3::CodecRunner* cr = m->eng->codec_runner();
        const int o = cr ? cr->stretch_hs() : q3::kStretchHa, p = cr ? cr->pitch_hp() : o;
        if (effective_semitones) *effective_semitones = p == o ? 0.0f : float(q3::pitch_effective_semitones(p, o));
        if (hp) *hp = p;
        if (ho) *ho = o;
        if (delay_samples) *delay_samples = cr ? cr->pitch_delay_out_samples() : 0;
    }, false);
}

q3tts_status q3tts_pitch_shift(q3tts_model* m, const float* in, int64_t n_in, float semitones, float* out, int64_t cap, int64_t* n_out) {
    return guarded(m, [&] {
        Q3_CHECK(m && in && out && n_out, 3, "Invalid input: null argument");
        m->eng->lane0().pitch_shift(in, n_in, semitones, out, cap, n_out);
    });
}

q3tts_status q3tts_model_get_keep_formants(const q3tts_model* m, int32_t* on) {
    return guarded(const_cast<q3tts_model*>(m), [&] {
        Q3_CHECK(m, 3, "Invalid input: null argument");
        const q3::CodecRunner* cr = m->eng->codec_runner();
        if (on) *on = (cr && cr->keep_formants()) ? 1 : 0;
    }, false);
}

q3tts_status q3tts_pitch_shift_formants(q3tts_model* m, const float* in, int64_t n_in, float semitones, float* out, int64_t cap,
                                        int64_t* n_out) {
    return guarded(m, [&] {
        Q3_CHECK(m && in && out && n_out, 3, "Invalid input: null argument");
        m->eng->lane0().pitch_shift_formants(in, n_in, semitones, out, cap, n_out);
    });
}

q3tts_status q3tts_request_speed_info(const q3tts_model* m, float speed, float* effective_speed, int32_t* hs, int32_t* delay_samples,
                                      int32_t* samples_per_frame) {
    return guarded(const_cast<q3tts_model*>(m), [&] {
        Q3_CHECK(m, 3, "Invalid input: null argument");
        const q3::CodecRunner* cr = m->eng->codec_runner();
        Q3_CHECK(cr != nullptr, 1, "Model not initialized: Speech tokenizer not loaded");
        int h = cr->stretch_hs();
        if (speed != 0.0f) {  // (a NaN is not 0 and fails the range)
            Q3_CHECK(cr->request_speeds(), 3, "Invalid input: q3tts_request.speed needs a handle loaded with q3tts_load_opts.request_speeds");
            h = cr->speed_plan().hs_of(speed);
            Q3_CHECK(h != 0, 3, "Invalid input: q3tts_request.speed must be 0 (the handle's speed) or between 0.5 and 2.0");
        }
        if (effective_speed) *effective_speed = float(double(q3::kStretchHa) / double(h));
        if (hs) *hs = h;
        if (delay_samples) *delay_samples = h == q3::kStretchHa ? 0 : q3::stretch_delay(h);
        if (samples_per_frame) *samples_per_frame = speed == 0.0f ? cr->upsample() : cr->upsample_of(h);
    }, false);
}

q3tts_status q3tts_time_stretch(q3tts_model* m, const float* in, int64_t n_in, float speed, int32_t causal, float* out, int64_t cap,
                                int64_t* n_out) {
    return guarded(m, [&] {
        Q3_CHECK(m && in && out && n_out, 3, "Invalid input: null argument");
        m->eng->lane0().time_stretch(in, n_in, speed, causal != 0, out, cap, n_out);
    });
}

void q3tts_voice_free(q3tts_model* m, q3tts_voice* v) {
    if (!m || !v) return;
    (void)guarded(m, [&] { m->eng->free_voice(voice_of(v)); });
}

q3tts_status q3tts_voice_get_info(const q3tts_voice* v, q3tts_voice_info* out) {
    if (!v || !out) return Q3TTS_ERR_INVALID_INPUT;
    const q3::Voice& x = *voice_of(v);
    out->ref_frames = x.ref_T;
    out->ref_text_tokens = int32_t(x.ref_text_ids.size());
    out->n_ref_samples = x.n_ref_samples;
    out->device_bytes = x.device_bytes;
    return Q3TTS_OK;
}

q3tts_status q3tts_generate_voices(q3tts_model* m, const q3tts_request* reqs, const q3tts_voice* const* voices, int32_t n_reqs,
                                   const q3tts_sampling* sampling, q3tts_event_cb cb, void* user, q3tts_result* results) {
    return generate_any(m, reqs, voices, true, n_reqs, -1, sampling, cb, user, results);
}

q3tts_status q3tts_generate_queued_voices(q3tts_model* m, const q3tts_request* reqs, const q3tts_voice* const* voices, int32_t n_reqs,
                                          int32_t slots, const q3tts_sampling* sampling, q3tts_event_cb cb, void* user,
                                          q3tts_result* results) {
    return generate_any(m, reqs, voices, true, n_reqs, slots < 0 ? 0 : slots, sampling, cb, user, results);
}

struct q3tts_job {
    int slot = -1;
    int n = 0;
};

q3tts_status q3tts_generate_begin(q3tts_model* m, const q3tts_request* reqs, int32_t n_reqs, const q3tts_sampling* sampling,
                                  q3tts_event_cb cb, void* user, int32_t more_follows, q3tts_job** job) {
    return guarded(m, [&] {
        Q3_CHECK(m && reqs && job, 3, "Invalid input: null argument");
        *job = nullptr;
        q3tts_sampling sp;
        if (sampling) sp = *sampling;
        else q3tts_default_sampling(&sp);
        auto j = std::make_unique<q3tts_job>();
        j->slot = m->eng->begin(reqs, n_reqs, sp, cb, user, more_follows != 0);
        j->n = n_reqs;
        *job = j.release();
    });
}

q3tts_status q3tts_generate_end(q3tts_model* m, q3tts_job* job, q3tts_result* results) {
    return guarded(m, [&] {
        Q3_CHECK(m && job && results, 3, "Invalid input: null argument");
        std::unique_ptr<q3tts_job> j(job);  // the job is released whatever happens
        std::memset(results, 0, sizeof(q3tts_result) * size_t(j->n > 0 ? j->n : 0));
        m->eng->end(j->slot, results);
        for (int i = 0; i < j->n; ++i)
            if (results[i].status == Q3TTS_ERR_GENERATION_FAILED)
                m->eng->last_error = "Generation failed: No tokens generated";  // Qwen3.swift:940
    });
}

// ---- serving session: submit / cancel / wait / get_stats take the session's own lock, not the handle's one-caller check ----
q3tts_status q3tts_session_open(q3tts_model* m, const q3tts_session_opts* opts, const q3tts_sampling* sampling, q3tts_event_cb cb,
                                void* user, q3tts_session** out) {
    if (out) *out = nullptr;
    if (!opts) return guarded(m, [&] { Q3_CHECK(false, 3, "Invalid input: null argument"); }, false);
    q3tts_session_opts_ex ex;
    std::memset(&ex, 0, sizeof(ex));
    ex.base = *opts;  // live_voices 0: exactly the session without live voices
    return q3tts_session_open_ex(m, &ex, sampling, cb, user, out);
}

q3tts_status q3tts_session_open_ex(q3tts_model* m, const q3tts_session_opts_ex* opts, const q3tts_sampling* sampling, q3tts_event_cb cb,
                                   void* user, q3tts_session** out) {
    if (out) *out = nullptr;
    return guarded(m, [&] {
        Q3_CHECK(m && opts && out, 3, "Invalid input: null argument");
        q3tts_sampling sp;
        if (sampling) sp = *sampling;
        else q3tts_default_sampling(&sp);
        m->eng->open_session(*opts, sp, cb, user);
        m->session = std::make_unique<q3tts_session>();
        m->session->m = m;
        *out = m->session.get();
    }, false);
}

q3tts_status q3tts_session_voice_create(q3tts_session* s, const float* ref_audio, int64_t n_ref_samples, int32_t sample_rate,
                                        const int32_t* ref_text_ids, int32_t n_ref_text_ids, q3tts_voice** out) {
    if (out) *out = nullptr;
    return session_call(s, [&](q3::Session& x) {
        Q3_CHECK(out, 3, "Invalid input: null argument");
        *out = reinterpret_cast<q3tts_voice*>(x.create_voice(ref_audio, n_ref_samples, sample_rate, ref_text_ids, n_ref_text_ids));
    });
}

q3tts_status q3tts_session_voice_wait(q3tts_session* s, const q3tts_voice* v, int32_t timeout_ms, int32_t* ready) {
    if (ready) *ready = 0;
    return session_call(s, [&](q3::Session& x) { x.voice_wait(voice_of(v), timeout_ms, ready); });
}

q3tts_status q3tts_session_voice_free(q3tts_session* s, q3tts_voice* v) {
    return session_call(s, [&](q3::Session& x) {
        Q3_CHECK(v, 3, "Invalid input: null argument");
        x.free_voice(voice_of(v));
    });
}

q3tts_status q3tts_session_get_voice_stats(const q3tts_session* s, q3tts_session_voice_stats* out) {
    return session_call(s, [&](q3::Session& x) {
        Q3_CHECK(out, 3, "Invalid input: null argument");
        x.voice_stats(out);
    });
}

q3tts_status q3tts_session_submit(q3tts_session* s, const q3tts_request* req, const q3tts_voice* voice, const q3tts_row_sampling* rs,
                                  int64_t* ticket) {
    return session_call(s, [&](q3::Session& x) {
        Q3_CHECK(req && ticket, 3, "Invalid input: null argument");
        x.submit(*req, voice_of(voice), rs, ticket);
    });
}

q3tts_status q3tts_session_cancel(q3tts_session* s, int64_t ticket) {
    return session_call(s, [&](q3::Session& x) {
        Q3_CHECK(x.cancel(ticket) == Q3TTS_OK, 3, "Invalid input: no such ticket");
    });
}

q3tts_status q3tts_session_wait(q3tts_session* s, int64_t ticket, int32_t timeout_ms, q3tts_result* out, int32_t* ready) {
    return session_call(s, [&](q3::Session& x) { x.wait(ticket, timeout_ms, out, ready); });
}

q3tts_status q3tts_session_get_stats(const q3tts_session* s, q3tts_session_stats* out) {
    return session_call(s, [&](q3::Session& x) {
        Q3_CHECK(out, 3, "Invalid input: null argument");
        x.stats(out);
    });
}

q3tts_status q3tts_session_submit_open(q3tts_session* s, const q3tts_request* req, const q3tts_row_sampling* rs, int64_t* ticket) {
    return session_call(s, [&](q3::Session& x) {
        Q3_CHECK(req && ticket, 3, "Invalid input: null argument");
        x.submit_open(*req, rs, ticket);
    });
}

q3tts_status q3tts_session_append_text(q3tts_session* s, int64_t ticket, const int32_t* ids, int32_t n, int32_t final) {
    return session_call(s, [&](q3::Session& x) { x.append_text(ticket, ids, n, final != 0); });
}

q3tts_status q3tts_session_get_text_stats(const q3tts_session* s, q3tts_session_text_stats* out) {
    return session_call(s, [&](q3::Session& x) {
        Q3_CHECK(out, 3, "Invalid input: null argument");
        x.text_stats(out);
    });
}

q3tts_status q3tts_session_close(q3tts_session* s, int32_t drain) {
    if (!s || !s->m) return Q3TTS_ERR_INVALID_INPUT;
    q3tts_model* m = s->m;
    return guarded(m, [&] {
        Q3_CHECK(m->session.get() == s && m->eng->session(), 3, "Invalid input: no such session");
        const int st = m->eng->close_session(drain != 0);  // (throws from inside a callback: the session stays open)
        m->session.reset();
        if (st) throw q3::Error(st, m->eng->last_error);
    }, false);
}

void q3tts_pcm_to_int16(const float* pcm, int64_t n_samples, int16_t* out) {
    for (int64_t i = 0; i < n_samples; ++i) {
        const float clamped = std::fmax(-1.0f, std::fmin(1.0f, pcm[i]));  // main.swift:159
        out[i] = static_cast<int16_t>(clamped * 32767.0f);                // Int16(Float): toward zero (:160)
    }
}

q3tts_status q3tts_write_wav(const char* path, const float* pcm, int64_t n_samples, int32_t sample_rate) {
    return guarded(nullptr, [&] {
        Q3_CHECK(path && (pcm || n_samples == 0) && n_samples >= 0 && sample_rate > 0, 3, "Invalid input: null argument");
        Q3_CHECK(n_samples <= (int64_t(0xffffffffu) - 36) / 2, 3, "Invalid input: too many samples for a RIFF file");
        std::vector<uint8_t> d;
        d.reserve(size_t(44 + n_samples * 2));
        auto u32 = [&](uint32_t v) { for (int i = 0; i < 4; ++i) d.push_back(uint8_t(v >> (8 * i))); };
        auto u16 = [&](uint16_t v) { d.push_back(uint8_t(v)); d.push_back(uint8_t(v >> 8)); };
        auto tag = [&](const char* t) { d.insert(d.end(), t, t + 4); };
        tag("RIFF"); u32(uint32_t(36 + n_samples * 2)); tag("WAVE");          // main.swift:138-142
        tag("fmt "); u32(16); u16(1); u16(1); u32(uint32_t(sample_rate));      // :145-149
        u32(uint32_t(sample_rate) * 2); u16(2); u16(16);                       // :150-152
        tag("data"); u32(uint32_t(n_samples * 2));                             // :155-156
        std::vector<int16_t> s16(static_cast<size_t>(n_samples));
        q3tts_pcm_to_int16(pcm, n_samples, s16.data());
        for (int16_t v : s16) u16(uint16_t(v));
        FILE* f = std::fopen(path, "wb");
        Q3_CHECK(f != nullptr, 3, std::string("Invalid input: cannot open ") + path);
        const size_t w = std::fwrite(d.data(), 1, d.size(), f);
        const int rc = std::fclose(f);
        Q3_CHECK(w == d.size() && rc == 0, 3, std::string("Invalid input: short write to ") + path);
    });
}

void q3tts_result_free(q3tts_result* results, int32_t n) {
    if (!results) return;
    for (int i = 0; i < n; ++i) {
        std::free(results[i].pcm);
        std::free(results[i].codes);
        results[i].pcm = nullptr;
        results[i].codes = nullptr;
    }
}

q3tts_status q3tts_codec_decode(q3tts_model* m, const int32_t* codes, const int32_t* n_frames, int32_t batch,
                                int32_t max_frames, float* pcm, int64_t* audio_lengths) {
    return guarded(m, [&] {
        Q3_CHECK(m && codes && n_frames && pcm && audio_lengths, 3, "Invalid input: null argument");
        m->eng->lane0().codec_decode(codes, n_frames, batch, max_frames, pcm, audio_lengths);
        m->eng->timing.codec_ms = m->eng->lane0().timing.codec_ms;
    });
}

q3tts_status q3tts_codec_encode(q3tts_model* m, const float* audio, int64_t n_samples, int32_t* codes, int32_t cap_frames,
                                int32_t* n_frames) {
    return guarded(m, [&] {
        Q3_CHECK(m && audio && codes && n_frames, 3, "Invalid input: null argument");
        *n_frames = m->eng->lane0().codec_encode(audio, n_samples, codes, cap_frames);
        m->eng->timing = m->eng->lane0().timing;
    });
}

int32_t q3tts_codec_encoded_frames(const q3tts_model* m, int64_t n_samples) {
    if (!m || n_samples <= 0 || n_samples > (int64_t(1) << 24)) return 0;
    return m->eng->lane0().encoded_frames(n_samples);
}

q3tts_status q3tts_speaker_embedding(q3tts_model* m, const float* audio, int64_t n_samples, int32_t sample_rate, float* out,
                                     int32_t cap) {
    return guarded(m, [&] {
        Q3_CHECK(m && audio && out, 3, "Invalid input: null argument");
        Q3_CHECK(sample_rate == 24000, 3,
                 "Invalid input: Only 24kHz audio is supported for speaker embedding extraction");  // Qwen3.swift:223-225
        m->eng->lane0().speaker_embedding(audio, n_samples, out, cap);
        m->eng->timing = m->eng->lane0().timing;
    });
}

q3tts_status q3tts_debug_frontend_stage(q3tts_model* m, const float* audio, int64_t n_samples, const char* stage, float* out,
                                        int64_t cap_floats, int32_t* T, int32_t* C) {
    return guarded(m, [&] {
        Q3_CHECK(m && audio && stage && out && T && C, 3, "Invalid input: null argument");
        m->eng->lane0().debug_frontend_stage(audio, n_samples, stage, out, cap_floats, T, C);
    });
}

q3tts_status q3tts_tokenizer_load(const char* path, q3tts_tokenizer** out) {
    return guarded(nullptr, [&] {
        Q3_CHECK(path && out, 3, "Invalid input: null argument");
        auto t = std::make_unique<q3tts_tokenizer>();
        const std::string p = path;
        if (p.size() > 5 && p.compare(p.size() - 5, 5, ".json") == 0) t->tok.load_json_file(p);
        else t->tok.load(p);
        *out = t.release();
    });
}
void q3tts_tokenizer_free(q3tts_tokenizer* t) { delete t; }
q3tts_status q3tts_tokenizer_encode(const q3tts_tokenizer* t, const char* utf8, int32_t* ids, int32_t cap, int32_t* n) {
    return guarded(nullptr, [&] {
        Q3_CHECK(t && utf8 && n, 3, "Invalid input: null argument");
        const std::vector<int32_t> v = t->tok.encode(utf8);
        *n = int32_t(v.size());
        Q3_CHECK(ids == nullptr || cap >= *n, 3, "Invalid input: output buffer too small for the token ids");
        if (ids) std::memcpy(ids, v.data(), v.size() * 4);
    });
}

q3tts_status q3tts_last_timing(const q3tts_model* m, q3tts_timing* out) {
    if (!m || !out) return Q3TTS_ERR_INVALID_INPUT;
    *out = m->eng->timing;
    return Q3TTS_OK;
}

q3tts_status q3tts_debug_prepare_inputs(q3tts_model* m, const q3tts_request* req, uint16_t* input_embeds,
                                        int32_t cap_prompt, int32_t* n_prompt, uint16_t* trailing, int32_t cap_trailing,
                                        int32_t* n_trailing, uint16_t* tts_pad) {
    return guarded(m, [&] {
        Q3_CHECK(m && req && input_embeds && n_prompt && trailing && n_trailing && tts_pad, 3, "Invalid input: null argument");
        m->eng->lane0().debug_prepare_inputs(*req, input_embeds, cap_prompt, n_prompt, trailing, cap_trailing, n_trailing, tts_pad);
    });
}

q3tts_status q3tts_debug_generate_forced(q3tts_model* m, const q3tts_request* reqs, int32_t n_reqs,
                                         const q3tts_sampling* sampling, const int32_t* forced_codes, int32_t n_frames,
                                         uint16_t* talker_logits, uint16_t* cp_logits, int32_t* sampled) {
    return guarded(m, [&] {
        Q3_CHECK(m && reqs && n_frames > 0, 3, "Invalid input: null argument");
        q3tts_sampling sp;
        if (sampling) sp = *sampling;
        else q3tts_default_sampling(&sp);
        q3::DebugOpts d;
        d.forced_codes = forced_codes;
        d.frames = n_frames;
        d.talker_logits = talker_logits;
        d.cp_logits = cp_logits;
        d.sampled = sampled;
        std::vector<q3tts_result> res((size_t)(n_reqs));
        m->eng->generate(reqs, n_reqs, sp, nullptr, nullptr, res.data(), &d);
        q3tts_result_free(res.data(), n_reqs);
    });
}

q3tts_status q3tts_debug_sample(q3tts_model* m, const uint16_t* logits, int32_t rows, int32_t V,
                                const q3tts_sampling* sampling, const uint8_t* seen, int32_t suppress_lo,
                                int32_t suppress_hi, int32_t eos_id, uint32_t row0, uint32_t draw, int32_t* tokens) {
    return guarded(m, [&] {
        Q3_CHECK(m && logits && sampling && tokens, 3, "Invalid input: null argument");
        q3::check_row_sampling(*sampling, rows);
        m->eng->lane0().debug_sample(logits, rows, V, *sampling, seen, suppress_lo, suppress_hi, eos_id, row0, draw, tokens);
    });
}

q3tts_status q3tts_debug_text_resume(q3tts_model* m, int32_t H, int32_t V, const uint16_t* tables, const int32_t* codes,
                                     const uint16_t* text_row, uint16_t* out_h, float* out_ss, int32_t* out_state) {
    return guarded(m, [&] {
        Q3_CHECK(m, 3, "Invalid input: null argument");
        m->eng->lane0().debug_text_resume(H, V, tables, codes, text_row, out_h, out_ss, out_state);
    });
}

q3tts_status q3tts_debug_linear(q3tts_model* m, const uint16_t* x, const uint16_t* W, const uint16_t* bias, int32_t M,
                                int32_t K, int32_t N, uint16_t* y) {
    return guarded(m, [&] {
        Q3_CHECK(m && x && W && y, 3, "Invalid input: null argument");
        m->eng->lane0().debug_linear(x, W, bias, M, K, N, y);
    });
}

q3tts_status q3tts_debug_attention(q3tts_model* m, const q3tts_attn_debug* a) {
    return guarded(m, [&] {
        Q3_CHECK(m && a, 3, "Invalid input: null argument");
        m->eng->lane0().debug_attention(*a);
    });
}

q3tts_status q3tts_debug_gemm(q3tts_model* m, q3tts_gemm_debug* a) {
    if (a && a->geometry_only) {  // host code only: no model, no GPU
        return guarded(nullptr, [&] {
            q3::GemmArgs ga{};
            q3::NormRowsArgs na{};
            q3::Engine::debug_gemm_check(*a, ga, na);
        });
    }
    return guarded(m, [&] {
        Q3_CHECK(m && a, 3, "Invalid input: null argument");
        m->eng->lane0().debug_gemm(*a);
    });
}

q3tts_status q3tts_debug_conv(q3tts_model* m, q3tts_conv_debug* a) {
    if (a && a->geometry_only) {  // host code only: no model, no GPU
        return guarded(nullptr, [&] { q3::Engine::debug_conv_check(*a); });
    }
    return guarded(m, [&] {
        Q3_CHECK(m && a, 3, "Invalid input: null argument");
        m->eng->lane0().debug_conv(*a);
    });
}

q3tts_status q3tts_debug_rowop(q3tts_model* m, q3tts_rowop_debug* a) {
    if (a && a->check_only) {  // host code only: no model, no GPU
        return guarded(nullptr, [&] { q3::Engine::debug_rowop_check(*a); });
    }
    return guarded(m, [&] {
        Q3_CHECK(m && a, 3, "Invalid input: null argument");
        m->eng->lane0().debug_rowop(*a);
    });
}

q3tts_status q3tts_debug_lmop(q3tts_model* m, q3tts_lmop_debug* a) {
    if (a && a->check_only) {  // host code only: no model, no GPU
        return guarded(nullptr, [&] { q3::Engine::debug_lmop_check(*a); });
    }
    return guarded(m, [&] {
        Q3_CHECK(m && a, 3, "Invalid input: null argument");
        m->eng->lane0().debug_lmop(*a);
    });
}

q3tts_status q3tts_codec_decode_streamed(q3tts_model* m, const int32_t* codes, const int32_t* n_frames, int32_t batch, int32_t max_frames,
                                         int32_t chunk_frames, int32_t window, int32_t lookahead, float* pcm) {
    return guarded(m, [&] {
        Q3_CHECK(m && codes && n_frames && pcm, 3, "Invalid input: null argument");
        m->eng->lane0().codec_decode_streamed(codes, n_frames, batch, max_frames, chunk_frames, window, lookahead, pcm);
    });
}

q3tts_status q3tts_codec_decode_streamed_prefixed(q3tts_model* m, const int32_t* codes, const int32_t* n_prefix, const int32_t* n_frames,
                                                  int32_t batch, int32_t max_frames, int32_t chunk_frames, int32_t window, int32_t lookahead,
                                                  float* pcm) {
    return guarded(m, [&] {
        Q3_CHECK(m && codes && n_prefix && n_frames && pcm, 3, "Invalid input: null argument");
        m->eng->lane0().codec_decode_streamed_prefixed(codes, n_prefix, n_frames, batch, max_frames, chunk_frames, window, lookahead, pcm);
    });
}

q3tts_status q3tts_debug_prefix_states(q3tts_model* m, int32_t* n_states, int64_t* device_bytes, int64_t* n_restored) {
    return guarded(m, [&] {
        Q3_CHECK(m && n_states && device_bytes && n_restored, 3, "Invalid input: null argument");
        m->eng->prefix_cache().stats(n_states, device_bytes, n_restored);
    });
}

q3tts_status q3tts_debug_stretch_rows(q3tts_model* m, const float* x, const int32_t* lens, const int32_t* hops, int32_t B, int64_t x_stride,
                                      float* y, int64_t y_stride) {
    return guarded(m, [&] {
        Q3_CHECK(m && x && lens && hops && y, 3, "Invalid input: null argument");
        m->eng->lane0().debug_stretch_rows(x, lens, hops, B, x_stride, y, y_stride);
    });
}

q3tts_status q3tts_debug_resample_ratio(q3tts_model* m, const float* x, const int32_t* lens, int32_t B, int64_t row_stride, int64_t in_units,
                                        int64_t out_units, int32_t centred, int32_t clamp, int32_t hist, float* y, int64_t y_stride) {
    return guarded(m, [&] {
        Q3_CHECK(m && x && lens && y, 3, "Invalid input: null argument");
        m->eng->lane0().debug_resample_ratio(x, lens, B, row_stride, in_units, out_units, centred != 0, clamp != 0, hist, y, y_stride);
    });
}

q3tts_status q3tts_debug_formant_rows(q3tts_model* m, int32_t mode, int32_t hp, int32_t ho, const int32_t* lens, int32_t B, const float* x,
                                      int64_t x_stride, int32_t hist, float* coef, int64_t coef_stride, const float* state_in, float* state_out,
                                      float* y, int64_t y_stride, int32_t clamp) {
    return guarded(m, [&] {
        Q3_CHECK(m && lens && x && coef && y, 3, "Invalid input: null argument");
        m->eng->lane0().debug_formant_rows(mode, hp, ho, lens, B, x, x_stride, hist, coef, coef_stride, state_in, state_out, y, y_stride, clamp != 0);
    });
}

q3tts_status q3tts_debug_codec_stream_slots(q3tts_model* m, const int32_t* codes, const int32_t* n_frames, int32_t n_reqs, int32_t max_frames,
                                            int32_t slots, int32_t burst, int32_t chunk_frames, int32_t window, int32_t lookahead, float* pcm) {
    return guarded(m, [&] {
        Q3_CHECK(m && codes && n_frames && pcm, 3, "Invalid input: null argument");
        m->eng->lane0().debug_codec_stream_slots(codes, n_frames, n_reqs, max_frames, slots, burst, chunk_frames, window, lookahead, pcm);
    });
}

q3tts_status q3tts_debug_build_decode_codes(q3tts_model* m, const int32_t* refs, const int32_t* ref_T, const int32_t* gen,
                                            const int32_t* n_frames, int32_t R, int32_t gen_stride, int32_t Fdec, int32_t misalign,
                                            int32_t* out) {
    return guarded(m, [&] {
        Q3_CHECK(m && ref_T && gen && n_frames && out && R >= 1 && gen_stride >= 1 && Fdec >= 1, 3, "Invalid input: null argument");
        m->eng->lane0().debug_build_decode_codes(refs, ref_T, gen, n_frames, R, gen_stride, Fdec, misalign != 0, out);
    });
}

void q3tts_debug_set_codec_scratch(uint64_t bytes) { q3::CodecRunner::set_scratch_budget(size_t(bytes)); }

void q3tts_debug_reload_env(void) { q3::debug_env_reload(); }

q3tts_status q3tts_debug_codec_stage(q3tts_model* m, const int32_t* codes, int32_t n_frames, const char* stage,
                                     float* out, int64_t cap_floats, int32_t* T, int32_t* C) {
    return guarded(m, [&] {
        Q3_CHECK(m && codes && stage && out && T && C && n_frames > 0, 3, "Invalid input: null argument");
        m->eng->lane0().debug_codec_stage(codes, n_frames, stage, out, cap_floats, T, C);
    });
}

}  // extern "C"
