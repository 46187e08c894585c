// engine.h -- host-side generation driver on top of the HIP kernels.
//
// Mirrors the reference's generation driver (/root/reference/Sources/Qwen3TTS/Models/Qwen3.swift:
// prompt assembly :259-409, AR loop :847-936 / :640-729, routing :1291-1373, decode + trim
// :943-961) with batching added: rows are independent sequences with their own KV pages,
// repetition sets and RNG streams.
#pragma once
#include <atomic>
#include <cstdlib>
#include <functional>
#include <map>
#include <memory>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/q3tts.h"
#include "kernels.h"
#include "model.h"
#include "pitch_plan.h"
#include "queue_slots.h"
#include "resample_plan.h"
#include "session_queue.h"
#include "stretch_plan.h"

namespace q3 {

struct DebugOpts {
    const int32_t* forced_codes = nullptr;  // host [n][frames][16]
    int frames = 0;
    uint16_t* talker_logits = nullptr;  // host [n][frames][V]
    uint16_t* cp_logits = nullptr;      // host [n][frames][groups-1][Vcp]
    int32_t* sampled = nullptr;         // host [n][frames][16]
};

// The device memory of the voices a session makes while it runs (q3tts_session_voice_create): `slots` places of `slot_bytes`
// each, allocated when the session opens so that no boundary allocates or frees. A voice holds its place, and through the shared
// pointer the pool, until the voice goes: voices outlive the session that made them.
// `states`: one saved prefix state (PrefixCache) per slot for a streamed session, allocated once by the session's stream when the
// loop starts (state_bytes is the codec stream's to say) and recycled with the slot: a session-made voice keeps at most one
// state, in its slot's place, so the state memory of a session is bounded and nothing is allocated or freed for it at a boundary.
struct VoicePool {
    DevBuf<uint8_t> mem;
    size_t slot_bytes = 0;
    const int n_slots;
    DevBuf<uint8_t> states;  // [n_slots][state_bytes], or empty
    size_t state_bytes = 0;
    std::mutex mu;
    std::vector<int> free_slots;
    VoicePool(int slots, size_t bytes) : slot_bytes(align_up(bytes, 256)), n_slots(slots) {
        mem.grow(size_t(slots) * slot_bytes);
        for (int i = slots; i-- > 0;) free_slots.push_back(i);
    }
    int take() {  // -1: none free
        std::lock_guard<std::mutex> lk(mu);
        if (free_slots.empty()) return -1;
        const int s = free_slots.back();
        free_slots.pop_back();
        return s;
    }
    void give(int s) {
        std::lock_guard<std::mutex> lk(mu);
        free_slots.push_back(s);
    }
};

// A reusable voice prompt (q3tts_voice): one reference clip and its transcript, encoded once (Engine::create_voice, or a
// session's live lane) and then read-only, so that every job context and every lane may read it. The device buffers hold what
// prepare_clone_rows produces for a waveform row; the host copies spare the requests that name the voice any device-to-host copy.
struct Voice {
    enum State { kReady = 0, kPending = 1, kAbandoned = 2 };
    const void* owner = nullptr;        // the EngineGroup it was created on
    // Counts up over every voice of the process: what identifies a voice in PrefixCache beside its address, which a later voice
    // may get again (the allocator's choice) as it may get the same pool slot.
    uint64_t serial = next_serial();
    // a session-made voice is a voice from its creation on; its device rows and host code copies are valid once kReady
    std::atomic<int> state{kReady};
    int ref_T = 0;                      // reference frames
    int64_t n_ref_samples = 0;
    std::vector<int32_t> ref_text_ids;
    int32_t* codes_dev = nullptr;       // [16][ref_T]
    uint16_t* rows_dev = nullptr;       // [1 + ref_T][H] bf16: x-vector row (zeros without a speaker encoder), then the frames' embedding sums
    DevBuf<int32_t> codes_own;          // what the two point into: buffers of its own (q3tts_voice_create) ...
    DevBuf<uint16_t> rows_own;
    std::shared_ptr<VoicePool> pool;    // ... or a place in a session's pool
    int pool_slot = -1;
    bool anonymous = false;             // made for one ref_audio ticket: no other ticket can restore a state of it, so none is saved
    bool state_taken = false;           // (the session's loop thread) its slot's place in pool->states holds a state of it
    ~Voice() {
        if (pool && pool_slot >= 0) pool->give(pool_slot);
    }
    static uint64_t next_serial() {
        static std::atomic<uint64_t> n{0};
        return ++n;
    }
    std::vector<int32_t> codes_host;    // [ref_T][16] frame-major, as the decoder reads them
    std::vector<int32_t> code0;         // [ref_T] first code row (valid-length count of the end trim)
    int64_t device_bytes = 0;
};

struct ResolvedRequest {
    std::vector<int32_t> text_ids, instruct_ids;
    int speaker_token = -1;  // row of the codec embedding table, -1: none
    int language_id = -1;    // -1: none ("auto" without dialect)
    int max_frames = 0;
    int target_token_count = 0;
    // voice clone (generateVoiceClone, Qwen3.swift:1009-1203)
    bool clone = false;
    std::vector<int32_t> ref_text_ids;
    const float* ref_audio = nullptr;  // caller memory, valid during the call
    int64_t n_ref_samples = 0;
    int ref_T = 0;        // reference frames (filled by prepare_clone_rows)
    int extra_base = 0;   // first row of this request in extra_: speaker x-vector, then ref_T embedding sums
    int ref_off = 0;      // offset of this request's [16][ref_T] codes in ref_codes_dev_
    const Voice* voice = nullptr;  // clone row whose reference is a voice: no waveform, no front end (ref_T known at once)
    // A session's open-text request (q3tts_session_submit_open): text_ids = role + the content so far, without the 5 tail tokens
    // (n_tail = 0). text_open: the text may still grow; max_frames is then the open cap (max_tokens) and open_max_tokens /
    // open_force_frames give final_text_cap() what it needs at the close.
    // q3tts_request.speed on a handle with request_speeds: the request's own synthesis hop (480: no stretch); 0: the handle's
    // (also when the request's hop is the handle's own)
    int hs = 0;
    int n_tail = 5;
    bool text_open = false;
    int open_max_tokens = 0, open_force_frames = 0;
};
// the reference's frame cap (Qwen3.swift:822-823) for n_content content tokens
inline int final_text_cap(int max_tokens, int force_frames, int n_content) {
    return force_frames > 0 ? force_frames : int(std::min<int64_t>(max_tokens, std::max<int64_t>(75, int64_t(n_content) * 6)));
}

// q3tts_sampling.per_request: the set fields of its n entries are checked on the host, before any GPU work (status 3)
void check_row_sampling(const q3tts_sampling& sp, int n);
// request i's parameters as the sampler reads them: the call's values with per_request[i]'s set fields folded in
SamplingParams fold_sampling(const q3tts_sampling& sp, int i, uint32_t row0);

class CodecRunner;
class VoiceFrontEnd;

struct FreeDeleter {
    void operator()(void* p) const { std::free(p); }
};
template <class T>
using MallocPtr = std::unique_ptr<T, FreeDeleter>;  // std::malloc'd host memory

// What a voice's reference leaves behind in the codec decoder's causal tail when it is decoded as the prefix of a streamed
// request (CodecRunner::stream_save_row): taken the first time the voice is streamed with a geometry, put back with one launch
// at every later admission instead of decoding the reference again. A voice is read-only, so the state depends on the voice,
// on (chunk, window, lookahead) and on the codec path (two-plane / float16 / fp32 kernels; `bytes` guards the layout) alone --
// not on the row, the row count or the lane. Kept beside the group's voices, read by any lane, dropped with the voice.
struct PrefixCache {
    struct Key {
        const Voice* voice = nullptr;
        uint64_t serial = 0;  // Voice::serial (of() sets both)
        int chunk = 0, window = 0, lookahead = 0, path = 0;
        size_t bytes = 0;
        int hs = 0;  // the synthesis hop the state was made with (its state word is that hop's); 0: the handle's
        void of(const Voice* v) {
            voice = v;
            serial = v ? v->serial : 0;
        }
        bool operator==(const Key& o) const {
            return hs == o.hs && voice == o.voice && serial == o.serial && chunk == o.chunk && window == o.window && lookahead == o.lookahead && path == o.path && bytes == o.bytes;
        }
    };
    struct Entry : Key {
        DevBuf<uint8_t> own;               // the state's memory: its own ...
        std::shared_ptr<VoicePool> pool;   // ... or its voice's place in a session's pool (kept alive with the entry)
        uint8_t* blob = nullptr;
        hipEvent_t ready = nullptr;  // behind the save: a restore on another stream waits for it
        ~Entry() {
            if (ready) (void)hipEventDestroy(ready);
        }
    };
    std::mutex mu;
    std::vector<std::shared_ptr<Entry>> entries;
    std::atomic<int64_t> restored{0};  // admissions served from a saved state since the model was loaded (q3tts_debug_prefix_states)
    std::shared_ptr<Entry> find(const Key& k) {
        std::lock_guard<std::mutex> lk(mu);
        for (auto& e : entries)
            if (*e == k) return e;
        return nullptr;
    }
    void publish(std::shared_ptr<Entry> n) {  // (two lanes may have primed the same voice side by side: the first one stays)
        std::lock_guard<std::mutex> lk(mu);
        for (auto& e : entries)
            if (*e == *n) return;
        entries.push_back(std::move(n));
    }
    void drop(const Voice* v) {
        std::lock_guard<std::mutex> lk(mu);
        for (size_t i = entries.size(); i-- > 0;)
            if (entries[i]->voice == v) entries.erase(entries.begin() + ptrdiff_t(i));
    }
    void stats(int32_t* n_entries, int64_t* bytes, int64_t* n_restored) {
        std::lock_guard<std::mutex> lk(mu);
        *n_entries = int32_t(entries.size());
        *bytes = 0;
        for (auto& e : entries) *bytes += int64_t(e->bytes);
        *n_restored = restored.load();
    }
};

// One request as the slot loop admits it: its ticket (the closed call: its index), what check_queued resolved, and its folded
// sampling parameters (an admission writes them to its slot).
struct QueueItem {
    int ticket = -1;
    ResolvedRequest rr;
    SamplingParams params{};
};

// Where the slot loop (Engine::run_queued) gets its requests and leaves their results. q3tts_generate_queued implements it over
// its request list; a session (q3tts_session_*) over a locked deque that other threads fill while the loop runs. A request's
// random stream is keyed by its ticket, so which lane or slot serves it, and when, does not matter.
struct RequestSource {
    virtual ~RequestSource() = default;
    // the next request in ticket order; false: none now (called from every lane's loop)
    virtual bool take(QueueItem& out) = 0;
    // where ticket's result goes: a stable address the loop alone writes until complete(ticket)
    virtual q3tts_result* result(int ticket) = 0;
    virtual void complete(int) {}
    // ---- an open source (a session) ----
    virtual bool open_ended() const { return false; }  // requests may arrive while the loop runs: an idle loop waits for them
    // the loop has nothing running and has flushed everything: sleeps until a request waits (true) or the source ends (false)
    virtual bool wait_for_work() { return false; }
    virtual bool has_cancels() { return false; }
    virtual void take_cancels(std::vector<int>& out) { out.clear(); }  // running tickets to drop at this boundary
    virtual void complete_cancelled(int) {}
    virtual void progress(int /*frame_steps*/, int /*admissions*/) {}
    // ---- open-text requests (a session) ----
    struct TextAppend {
        int ticket = -1;
        std::vector<int32_t> ids;  // content tokens, already checked
        bool final = false;        // the text ends behind them
    };
    virtual bool open_text() const { return false; }  // requests may be admitted with their text still open
    virtual bool has_appends() { return false; }
    virtual void take_appends(std::vector<TextAppend>& out) { out.clear(); }  // for running tickets, in arrival order
    // every running row waits for text: sleeps until a boundary has something to do (an append, a cancel, a request while can_admit, close)
    // timeout_ms >= 0: at the latest after that long (a voice job is in flight: its lane has to be polled)
    virtual void wait_for_text(bool /*can_admit*/, int /*timeout_ms*/ = -1) {}
    virtual void text_progress(int /*starved_now*/, int /*starve_events*/) {}
    // ---- live voices (a session opened with live_voices > 0) ----
    struct VoiceJob {  // one clip's front end, as q3tts_session_voice_create copied it
        int64_t id = -1;
        Voice* voice = nullptr;    // its place is taken: ref_T, n_ref_samples (24 kHz) and the device pointers are set
        std::vector<float> clip;   // at `rate`
        int rate = 24000;
    };
    virtual bool live_voices() const { return false; }
    virtual bool has_voice_work() { return false; }                               // jobs to launch or voices to release
    virtual int take_voice_jobs(std::vector<VoiceJob>& out, int /*max*/) { out.clear(); return 0; }
    virtual void voice_done(int64_t /*id*/, double /*frontend_ms*/) {}           // (the voice's host copies are filled)
    // voices nothing uses any more: released here, on the loop thread; before(v) runs first for each (the stream disowns the
    // states of v it has not published yet)
    virtual VoicePool* voice_pool() { return nullptr; }  // where session-made voices and their saved states live
    virtual void release_voices(const std::function<void(const Voice*)>& /*before*/) {}
    virtual void burst_done(int /*frame_steps*/, double /*ms*/, bool /*beside a voice job*/) {}
};

// What the lanes of one slot loop share: the request source and what was fixed before the loop started.
struct QueueShared {
    RequestSource* src = nullptr;
    uint32_t row_base = 0;
    int voice_ref_max = -1;  // longest reference (frames) of a voice request the source may hand out: sizes the voice rows of an
                             // admission once, before the loop; -1: no voice requests
    // streamed audio for voice requests (q3tts_sampling.audio_stream_reference): the longest reference (the
    // stream's code rows hold reference ++ generated) and where the references' tail states are kept (nullptr: always decode them)
    bool stream_reference = false;
    int ref_max = 0;
    PrefixCache* prefix_cache = nullptr;
};

class Engine {
  public:
    // One lane: a slice of the batch with its own stream, workspace, KV pool and frame graph.
    // pitch: q3tts_load_opts_ex.pitch; keep_formants: q3tts_load_opts_ex2.keep_formants
    Engine(Model* model, const q3tts_load_opts& opts, float pitch = 0.0f, bool keep_formants = false);
    ~Engine();

    Model& model() { return *m_; }
    const q3tts_load_opts& opts() const { return opts_; }
    std::string last_error;
    q3tts_timing timing{};

    // voices: [n] or nullptr; a non-null entry makes request i a voice-clone request whose reference is that voice
    void generate(const q3tts_request* reqs, int n, const q3tts_sampling& sp, q3tts_event_cb cb, void* user,
                  q3tts_result* results, const DebugOpts* dbg, const Voice* const* voices = nullptr);
    // generate() in two halves (q3tts_generate_begin / _end). The front half of begin -- input checks, voice front end, prompt
    // assembly, row reservation, prefill enqueued -- always runs on the caller's thread, so whatever can refuse a request
    // refuses it inside begin. The back half -- frame loop, hand-off to the codec stream, timing -- runs there too when the job
    // has an event callback, DebugOpts or chunked audio, or when `background` is false: begin then returns once the AR loop
    // has finished and the decode of its codes is queued. Otherwise the back half runs
    // on this engine's worker thread and begin returns as soon as the prefill is enqueued; end waits for the back half and
    // rethrows what it threw. end then waits for the PCM and fills the results. Jobs may end in any order; at most kJobSlots
    // are outstanding. An EngineGroup with one lane keeps two engines (contexts) and gives each job the free one, so the AR
    // loops of two outstanding background jobs run side by side, each chain on a stream of its own.
    static constexpr int kJobSlots = 2;
    int begin(const q3tts_request* reqs, int n, const q3tts_sampling& sp, q3tts_event_cb cb, void* user, const DebugOpts* dbg,
              bool overlapped,  // overlapped: another batch's AR loop is expected to run beside this one's decode
              bool background = false, const Voice* const* voices = nullptr);
    void end(int job, q3tts_result* results);
    bool job_outstanding() const;
    int text_cap() const { return Tcap_; }  // rows of a slot's trailing text: the most content tokens an open-text request may hold
    void prepare_job_pair();  // at load, by an EngineGroup that will run background jobs on its two contexts
    void drain();             // returns once no back half is queued or running on the worker thread
    // Continuous batching (q3tts_generate_queued). check_queued resolves one request (with `voice`: a voice-clone request, whose
    // ICL prompt length it computes) and applies every limit the slot loop would hit (prompt, trailing text, max_frames, RoPE
    // range) on the host, before any GPU work. run_queued keeps `slots`
    // rows in flight: at each burst boundary finished rows are retired (codes copied out, decode queued on the codec stream
    // beside the frame loop) and their slots take the next requests of `q`, prefilled as a sub-batch of their own.
    ResolvedRequest check_queued(const q3tts_request& r, const q3tts_sampling& sp, const Voice* voice = nullptr,
                                 bool open_text = false) const;  // open_text: a session's open-text request (role + content, no tail)
    void check_stream_chunk(int chunk_frames) const;  // a streamed decode's chunk must hold the causal tail's history
    void run_queued(QueueShared& q, int slots, const q3tts_sampling& sp, q3tts_event_cb cb, void* user);
    void debug_prepare_inputs(const q3tts_request& req, uint16_t* input_embeds, int cap_prompt, int* n_prompt,
                              uint16_t* trailing, int cap_trailing, int* n_trailing, uint16_t* tts_pad);
    void debug_sample(const uint16_t* logits, int rows, int V, const q3tts_sampling& sp, const uint8_t* seen,
                      int suppress_lo, int suppress_hi, int eos_id, uint32_t row0, uint32_t draw, int32_t* tokens);
    void debug_text_resume(int H, int V, const uint16_t* tables, const int32_t* codes, const uint16_t* text, uint16_t* out_h,
                           float* out_ss, int32_t* out_state);
    void debug_linear(const uint16_t* x, const uint16_t* W, const uint16_t* bias, int M, int K, int N, uint16_t* y);
    void debug_attention(const q3tts_attn_debug& a);
    // q3tts_debug_gemm: the host checks and the geometry need neither an engine nor a GPU (geometry_only); returns the GemmArgs
    // and NormRowsArgs the launch will carry, still without pointers
    static void debug_gemm_check(q3tts_gemm_debug& d, GemmArgs& ga, NormRowsArgs& na);
    void debug_gemm(q3tts_gemm_debug& d);
    // q3tts_debug_conv (conv_debug.cc): likewise -- the check fills the geometry outputs from the launchers' dispatch functions
    static void debug_conv_check(q3tts_conv_debug& d);
    void debug_conv(q3tts_conv_debug& d);
    // q3tts_debug_rowop (rowop_debug.cc): one launch of a codec_misc.hip / voice_frontend.hip launcher; the check is host code
    static void debug_rowop_check(const q3tts_rowop_debug& d);
    void debug_rowop(q3tts_rowop_debug& d);
    // q3tts_debug_lmop (lmop_debug.cc): one launch of a sampler.hip / lm_misc.hip launcher; the check is host code
    static void debug_lmop_check(const q3tts_lmop_debug& d);
    void debug_lmop(q3tts_lmop_debug& d);
    void debug_build_decode_codes(const int32_t* refs, const int32_t* ref_T, const int32_t* gen, const int32_t* n_frames, int R,
                                  int gen_stride, int Fdec, bool misalign, int32_t* out);
    void codec_decode(const int32_t* codes, const int32_t* n_frames, int batch, int max_frames, float* pcm,
                      int64_t* audio_lengths);
    void codec_decode_streamed(const int32_t* codes, const int32_t* n_frames, int batch, int max_frames, int chunk_frames, int window,
                               int lookahead, float* pcm);
    void codec_decode_streamed_prefixed(const int32_t* codes, const int32_t* n_prefix, const int32_t* n_frames, int batch, int max_frames,
                                        int chunk_frames, int window, int lookahead, float* pcm);
    // q3tts_debug_codec_stream_slots: the slotted stream of a streamed queue driven by the queue's schedule without the talker
    void debug_codec_stream_slots(const int32_t* codes, const int32_t* n_frames, int n_reqs, int max_frames, int slots, int burst,
                                  int chunk_frames, int window, int lookahead, float* pcm);
    void debug_codec_stage(const int32_t* codes, int n_frames, const char* stage, float* out, int64_t cap, int* T, int* C);
    // voice-clone front end (SpeechTokenizer.swift:841-846; Qwen3.swift:222-249); host buffers in and out
    int codec_encode(const float* audio, int64_t n_samples, int32_t* codes, int cap_frames);
    int encoded_frames(int64_t n_samples) const;
    void speaker_embedding(const float* audio, int64_t n_samples, float* out, int cap);
    // q3tts_voice_create: what prepare_clone_rows runs for one clip, into buffers the voice owns; synchronises before it returns
    // sample_rate != 24000: the clip is uploaded at its own rate and resampled on the device (centred form, no clamp) in front
    // of the encoders; Voice::n_ref_samples counts 24 kHz samples
    std::unique_ptr<Voice> create_voice(const float* audio, int64_t n_samples, const int32_t* ref_text_ids, int n_ref_text_ids,
                                        int sample_rate = 24000);
    // q3tts_resample: host buffers through kernels/resample.hip; one of the rates is 24000 (resample_plan.h)
    void resample(const float* in, int64_t n_in, int in_rate, int out_rate, bool centred, float* out, int64_t cap, int64_t* n_out);
    // q3tts_time_stretch: a 24 kHz host buffer through kernels/stretch.hip (stretch_plan.h); causal: the decoder stage's form
    void time_stretch(const float* in, int64_t n_in, float speed, bool causal, float* out, int64_t cap, int64_t* n_out);
    // q3tts_debug_stretch_rows: the kernel's per-row path (a hop per row, the fade tables of every hop) on host rows, causal form
    void debug_stretch_rows(const float* x, const int32_t* lens, const int32_t* hops, int B, int64_t x_stride, float* y, int64_t y_stride);
    // q3tts_pitch_shift: a 24 kHz host buffer through the whole, undelayed form of a pitched handle's two stages -- the time
    // stretch whole at Hp (pitch_plan.h, Ho = 480), then the centred general-ratio resampler Hp -> 480
    void pitch_shift(const float* in, int64_t n_in, float semitones, float* out, int64_t cap, int64_t* n_out);
    // q3tts_debug_resample_ratio: kernels/resample_ratio.hip on host rows, any positive integer pair
    void debug_resample_ratio(const float* x, const int32_t* lens, int B, int64_t row_stride, int64_t in_units, int64_t out_units, bool centred,
                              bool clamp, int hist, float* y, int64_t y_stride);
    // q3tts_pitch_shift_formants: pitch_shift with the formant stage (formant_plan.h formant_shift_reference): the whole stretch
    // at Hp, analyse + whiten, the centred resampler Hp -> 480, synthesise; not clipped
    void pitch_shift_formants(const float* in, int64_t n_in, float semitones, float* out, int64_t cap, int64_t* n_out);
    // q3tts_debug_formant_rows: kernels/formant.hip on host rows (include/q3tts.h states the modes)
    void debug_formant_rows(int mode, int hp, int ho, const int32_t* lens, int B, const float* x, int64_t x_stride, int hist, float* coef,
                            int64_t coef_stride, const float* state_in, float* state_out, float* y, int64_t y_stride, bool clamp);
    void debug_frontend_stage(const float* audio, int64_t n_samples, const char* stage, float* out, int64_t cap, int* T, int* C);

    // ---- live voices (a session opened with live_voices > 0; engine_queue.cc) ----
    // the host checks of create_voice (status 1 / 3), callable from any thread: nothing of the engine's state is written.
    // Returns the clip's samples at 24 kHz
    int64_t check_voice_clip(const float* audio, int64_t n_samples, const int32_t* ref_text_ids, int n_ref_text_ids, int sample_rate) const;
    // `lanes` front ends on non-blocking streams of their own, each with scratch, device buffers and pinned staging for a clip of
    // max_ref_frames frames at any supported rate; the resamplers' tables. Before the session's loop starts / behind its end
    void live_open(int lanes, int max_ref_frames);
    void live_close();

    std::vector<std::string> speakers;  // sorted (Qwen3.swift:965-971)
    const CodecRunner* codec_runner() const { return codec_.get(); }  // nullptr: the checkpoint has no codec decoder

  private:
    Model* m_;
  public:
    uint32_t row_offset = 0;       // global index of this lane's first row (RNG stream id)
    std::mutex* cb_mutex = nullptr;  // serialises event callbacks across lanes
    int request_base = 0;          // added to request_index in events
    int max_inflight_frames = 16;  // frame steps queued but not finished (two bursts of half this)
    int job_chains = 1;            // contexts whose begin / end jobs may submit at once: each job's frame loop keeps to its share of
                                   // max_inflight_frames (the queued path runs alone on the first context and keeps all of it)
  private:
    q3tts_load_opts opts_;
    hipStream_t st_ = nullptr;
    hipStream_t st_codec_ = nullptr;       // codec decode that nothing overlaps (lower priority than st_)
    hipStream_t st_codec_part_ = nullptr;  // codec decode beside the next batch's AR loop: confined to half of the CUs
    hipStream_t st_codec_wide_ = nullptr;  // the same for a background job, whose decode runs beside the other job's: three quarters
    hipStream_t masked_stream(int cus, int total);
    hipStream_t codec_stream(bool overlapped, bool wide = false);
    hipEvent_t ev_[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t burst_ev_[2] = {nullptr, nullptr};
    hipEvent_t ev_fe_[2] = {nullptr, nullptr};
    hipEvent_t fe_uploaded_ = nullptr;
    int Bm_ = 0, Mp_ = 0;  // max batch, padded to 16
    int Pcap_ = 0, Tcap_ = 0, Fcap_ = 0, max_pages_ = 0, n_pages_ = 0;

    // device workspace (one allocation)
    uint8_t* ws_ = nullptr;
    size_t ws_bytes_ = 0;
    struct Stream {  // activation buffers of one decoder stack
        uint16_t *h, *xn, *qkv, *ao, *act, *logits;  // h, xn, ao, act: fragment-major; qkv, logits: row-major
        float *ss_a, *ss_b;                     // per-tile sums of squares of h ([H/16][Mp])
        int ld_qkv, ld_act, ld_logits;
    } tk_{}, cp_{};
    uint16_t* cp_x_ = nullptr;   // fragment-major [Mp][H] code-predictor input before the projection
    uint16_t* cp_x2_ = nullptr;
    // small_to_mtp_projection applied to every row of the code predictor's embedding tables at load (by the decode GEMM
    // itself, so rows are bit-identical to projecting at run time); kept in the Model, see Model::cp_pe
    bool cp_tables_ = false;  // the samplers hand projected rows (Model::cp_pe) straight to the next pass
    void build_cp_proj_tables();  // staged embedding of code 0 (second position of predictor step 0)
    float* cp_ss2_ = nullptr;
    uint16_t *kpool_ = nullptr, *vpool_ = nullptr, *cp_kpool_ = nullptr, *cp_vpool_ = nullptr;
    size_t kv_layer_stride_ = 0, cp_kv_layer_stride_ = 0;
    int32_t *block_table_ = nullptr, *cp_block_table_ = nullptr;
    int32_t *kv_len_ = nullptr, *cp_len_ = nullptr, *n_frames_ = nullptr, *max_frames_ = nullptr;
    int32_t *trailing_idx_ = nullptr, *n_trailing_ = nullptr, *n_prompt_ = nullptr, *cur_codes_ = nullptr, *codes_ = nullptr;
    uint8_t *active_ = nullptr, *finished_ = nullptr, *seen_ = nullptr;
    uint16_t *prompt_ = nullptr, *trailing_ = nullptr, *tts_pad_ = nullptr;
    SamplingParams* sp_dev_ = nullptr;  // [max_batch] row b's sampling parameters (a queued call: slot b's)
    // prompt-assembly scratch
    int32_t* ids_dev_ = nullptr;
    uint16_t *proj_in_ = nullptr, *proj_mid_ = nullptr, *proj_out_ = nullptr;
    int proj_cap_ = 0;
    int32_t *compose_a_ = nullptr, *compose_b_ = nullptr;
    // debug buffers (allocated on demand)
    int32_t *forced_dev_ = nullptr, *sampled_dev_ = nullptr;
    uint16_t *tl_dump_ = nullptr, *cl_dump_ = nullptr;

    // One slot per outstanding job: everything the second half (codec decode -> results) needs after the next begin()
    // has started to overwrite the engine's per-call state.
    struct Job {
        std::atomic<bool> busy{false};
        uint64_t seq = 0;                 // begin order
        // a back half on the worker thread: what it needs once begin() has returned (the caller's request memory is only
        // valid during begin), and how it ended
        std::vector<ResolvedRequest> rr;
        std::vector<int> np;
        q3tts_sampling sp{};
        bool overlapped = false;
        bool frontend = false;    // some row's reference was a waveform: timing.frontend_ms is the front end's time (else 0)
        bool background = false;  // the back half runs on the worker thread (and the decode on the wider masked stream)
        int back = 0;         // 1: queued for or running on the worker thread (work_mu_)
        int back_status = 0;  // q3::Error status the back half ended with (0: it finished)
        std::string back_err;
        int n = 0, Fdec = 0, up = 0;  // up: samples per frame of the PCM buffers' layout (the slowest row's when rows have hops of their own)
        std::vector<int> row_hs;      // rows with speeds of their own: row b's synthesis hop; empty: every row at the handle's
        std::vector<int> row_up;      // [n] row b's samples per frame (== up unless row_hs)
        std::vector<int> frames, ref_T, target_tokens, n_prompt;
        std::vector<int> req_index;   // queued decode batch: row b is request req_index[b] (results / events); empty: row b
        std::vector<q3tts_result*> row_out;  // queued decode batch: where row b's result goes (end() is given no array)
        std::vector<double> row_span; // queued decode batch: admission -> retirement of row b (generate_time); empty: the job's
        std::vector<std::vector<int32_t>> ref_code0;  // first code row of each reference (valid-length count)
        std::vector<int32_t> codes_host;  // [n][Fcap][16]
        DevBuf<int32_t> dec_codes;        // [n][Fdec][16]: what the decoder reads (reference ++ generated for clone rows)
        std::vector<const Voice*> voices; // queued decode batch: row b's voice (nullptr: none); empty: no row has one
        DevBuf<int32_t> gen_codes;        // queued decode batch with voice rows: codes_host on the device, [n][Fcap][16]
        std::vector<DecodeRowDesc> row_desc;  // launch_build_decode_codes_rows: the rows' descriptors (alive until the slot is reused)
        DevBuf<DecodeRowDesc> row_desc_dev;
        PinnedBuf<float> pcm_host;        // [n][Fdec * up]
        hipEvent_t ev_codec[2] = {nullptr, nullptr};
        PinnedBuf<int32_t> nf_host;        // [max_batch]: rows whose waveform came out non-finite (CodecRunner::decode)
        PinnedBuf<int32_t> nf_chunk_host;  // [chunks][n]: the same flags behind every chunk of a decode in pieces
        std::vector<int> held_from;  // streamed job: first chunk of row b that is held back for the fp32 re-decode (-1: none)
        hipEvent_t ev_begin = nullptr, ev_first_audio = nullptr;  // request in / first streamed chunk on the host
        std::vector<hipEvent_t> chunk_done;  // chunked decode (audio_chunk_frames > 0): one per chunk, behind its copy
        int n_chunks = 0, chunk_frames = 0;
        bool streamed = false;   // audio_window_frames > 0: chunks were decoded (and partly delivered) inside the frame loop
        bool prefixed = false;   // streamed through a slotted stream with the clone rows' references in front (audio_stream_reference):
                                 // rows of Fdec = max_frames + longest reference frames, a row's audio behind ref_T * up samples
        int chunks_fired = 0;    // AUDIO_CHUNK events already delivered for chunks [0, chunks_fired)
        double t_first_audio = 0;
        q3tts_timing timing{};
        double t_start = 0, t_done = 0;  // begin() entered / PCM on the host (stage_rows)
        q3tts_event_cb cb = nullptr;
        void* user = nullptr;
        int request_base = 0;
        bool decoded = false;
        // results of the rows: cut computed when the codes are known; PCM and codes copied out of the job's buffers once
        // the decode has finished -- by the staging thread for a pipelined job (so that end() hands over pointers while
        // the next batch's frame loop keeps the device busy), inside end() otherwise
        std::vector<int64_t> row_cut, row_ns;
        std::vector<MallocPtr<float>> st_pcm;  // std::malloc'd: a result's buffers until q3tts_result_free
        std::vector<MallocPtr<int32_t>> st_codes;
        int stage = 0;  // 0: not staged, 1: queued for the staging thread, 2: staged, 3: staging failed (stage_err)
        std::string stage_err;
        void reset(int rows, int upsample);  // every per-batch field, before a batch takes the slot
        void clear_chunk_flags(int frames);  // nf_chunk_host for a decode of `frames` frames in chunks of chunk_frames
    } jobs_[kJobSlots];
    // a job's codec decode on the codec stream (ev_codec[0], decode -- in chunks when J.chunk_frames > 0 --, PCM to pcm_host,
    // ev_codec[1]); codes_host: [n][Fcap][16] copied in on that stream first (behind their voices' reference frames for the
    // rows of J.voices); nullptr: J.dec_codes holds the codes already
    void start_decode(Job& J, const std::vector<int>& dframes, bool overlapped, const int32_t* codes_host);
    // the job is outstanding: cuts, then handed to the staging thread when `stage` and there is PCM to copy
    void publish_job(Job& J, q3tts_event_cb cb, void* user, int request_base, double t_start, bool stage);
    void release_job(Job& J);  // waits for the staging thread, frees the rows not handed over, frees the slot
    void compute_cuts(Job& J);
    // AUDIO_CHUNK events of chunks [J.chunks_fired, upto); rows are clipped to known[b] frames (their final length when known)
    void fire_chunks(Job& J, int upto, const std::vector<int>* known, bool wait);
    std::unique_lock<std::mutex> cb_lock();  // held while events are delivered: callbacks of all lanes are serialised
    // TOKEN events of frames [reported, nf) of row `row` of codes_ (request `request`), in generation order
    void emit_tokens(q3tts_event_cb cb, void* user, int row, int request, int nf, int& reported);
    void stage_rows(Job& J);   // waits for the decode, then copies; throws
    // rows whose waveform left the fp16 range of the default codec kernels are decoded again on the fp32 matrix cores
    // (the reference's range) before end() hands them out; returns the rows that are non-finite even then
    std::vector<int> redo_rows_fp32(Job& J);
    // its mechanical part, shared with a streamed queue's held requests: rows of dframes[i] frames, whose codes place(i, dst,
    // cst) puts on the device, through the exact decode on codec_stream(false); returns with the PCM on the host
    struct ExactDecode {
        PinnedBuf<float> pcm;   // [rows][Fd * up]
        PinnedBuf<int32_t> nf;  // [rows]: non-finite even so
        int Fd = 0, up = 0;     // up: samples per frame of pcm's layout
    };
    // hs (optional): the rows' own synthesis hops (Job::row_hs)
    ExactDecode decode_rows_fp32(const std::vector<int>& dframes, const std::function<void(int, int32_t*, hipStream_t)>& place,
                                 const std::vector<int>* hs = nullptr);
    // the rows' own hops (ResolvedRequest::hs, 0: the handle's) into a job that has just been reset
    void set_row_speeds(Job& J, const std::vector<int>& hs);
    // a streamed request held back at the chunk that starts at sample `at`: samples [at, ns) of its audio from the exact decode
    // (src: its sample 0 there), then the AUDIO_CHUNK events it is still owed, in steps of `step` samples
    void refire_held(float* own, const float* src, int64_t at, int64_t ns, int64_t step, q3tts_event_cb cb, void* user, int index);
    void staging_loop();
    std::thread stager_;
    std::mutex stage_mu_;
    std::condition_variable stage_cv_;
    bool stage_stop_ = false;
    uint64_t job_seq_ = 0;

    unsigned long long* stamps_ = nullptr;  // Q3TTS_FRAME_STAMPS=1: [0] frame steps, [k] ticks of phase k, [63] last stamp
    void stamp(int k) {
        if (stamps_) launch_stamp(stamps_, stamps_ + 63, k, counted());
    }
    // The stream every launch site of the frame step (and of the prefill, which shares the layer code) enqueues on: st_, with
    // the launch counted for q3tts_timing.launches_per_frame_step.
    hipStream_t counted() {
        ++launches_;
        return st_;
    }
    int launches_ = 0;                         // launches enqueued since enqueue_frame last reset it
    std::map<int, int> frame_launches_;        // launches of one frame step, keyed by batch size (q3tts_timing)
    std::map<int, hipGraphExec_t> graphs_;  // keyed by batch size
    std::unique_ptr<CodecRunner> codec_;
    std::unique_ptr<VoiceFrontEnd> fe_;
    // voice-clone scratch (grown on demand)
    DevBuf<float> ref_audio_dev_;
    DevBuf<int32_t> ref_codes_dev_;
    DevBuf<uint16_t> extra_;  // [rows][H] bf16: speaker x-vectors and reference-frame embedding sums
    DevBuf<float> spk_f32_;
    // Clone rows are independent and their front-end kernels are small: a few of them run side by side, each on its
    // own stream with its own scratch.
    struct FeLane {
        hipStream_t st = nullptr;
        hipEvent_t done = nullptr;
        std::unique_ptr<VoiceFrontEnd> fe;
        DevBuf<float> spk;
    };
    std::vector<FeLane> fe_lanes_;
    // A live-voice lane: FeLane plus what lets create_voice's sequence run on it without an allocation or a wait
    struct LiveLane {
        FeLane fe;
        hipEvent_t t0 = nullptr, t1 = nullptr;  // around the front end's kernels (timed)
        DevBuf<float> in, a24;                  // the clip at its own rate / at 24 kHz
        DevBuf<int32_t> len;
        PinnedBuf<uint8_t> stage;               // the clip, its length word, the codes read back
        size_t stage_codes = 0, stage_len = 0;  // byte offsets in stage
        int64_t id = -1;                        // the job in flight (-1: free)
        Voice* voice = nullptr;
    };
    std::vector<LiveLane> live_lanes_;
    int64_t live_max_in_ = 0, live_max_24_ = 0;
    int live_in_flight() const;
    void live_launch(LiveLane& L, RequestSource::VoiceJob& job);
    // lanes whose job has finished: the voice's host copies filled, src told; wait: every lane in flight, whatever it takes
    void live_poll(RequestSource& src, bool wait);
    const float* upload_audio(const float* audio, int64_t n);
    // the polyphase filters this engine has been asked for, tables on the device (built on first use)
    struct ResamplerDev {
        ResamplePlan plan;
        DevBuf<float> tab;
    };
    std::vector<std::unique_ptr<ResamplerDev>> resamplers_;
    DevBuf<float> rs_out_dev_;
    DevBuf<int32_t> rs_len_dev_;
    struct StretchDev {  // the same for the synthesis hops q3tts_time_stretch has been asked for
        StretchPlan plan;
        DevBuf<float> fade;
    };
    std::vector<std::unique_ptr<StretchDev>> stretchers_;
    DevBuf<float> dbg_fade_all_;  // debug_stretch_rows: the fade tables of every hop, uploaded at its first call
    const ResamplerDev& resampler(int in_rate, int out_rate);
    // the general-ratio filters (kernels/resample_ratio.hip) q3tts_pitch_shift and q3tts_debug_resample_ratio have been asked
    // for: the plan of the pair as given, the table in output order on the device
    std::vector<std::unique_ptr<ResamplerDev>> ratios_;
    const ResamplerDev& ratio_resampler(int64_t in_units, int64_t out_units);
    DevBuf<float> ps_mid_dev_;  // pitch_shift: the stretched signal between its two stages
    // `audio` (host, n samples at in_rate, finite) -> device buffer of *n_out samples at out_rate, queued on st_
    const float* resample_upload(const float* audio, int64_t n, int in_rate, int out_rate, bool centred, int64_t* n_out);
    bool prepare_clone_rows(std::vector<ResolvedRequest>& reqs);  // true: the front end ran (some row carried a waveform)

    void alloc_workspace();
    ResolvedRequest resolve(const q3tts_request& r, const q3tts_sampling& sp, const Voice* voice = nullptr) const;
    // the checks of a voice-clone reference that do not depend on the request's text (resolve, create_voice)
    void check_reference(const float* ref_audio, int64_t n_ref_samples, const int32_t* ref_text_ids, int n_ref_text_ids) const;
    // ---- the steps of begin() ----
    // input checks, a free job slot (returned; ev_begin recorded), the resolved requests
    int open_job(const q3tts_request* reqs, int n, const q3tts_sampling& sp, const DebugOpts* dbg, std::vector<ResolvedRequest>& rr,
                 double& t_start, const Voice* const* voices);
    // block table, per-row limits and lengths, cleared per-row state, sampling parameters; returns the longest prompt
    int reserve_rows(const std::vector<ResolvedRequest>& rr, const std::vector<int>& np, const std::vector<int>& nt,
                     const q3tts_sampling& sp);
    void debug_buffers(int n, const DebugOpts& dbg);
    struct StreamedDecode;
    struct SlotStream;  // the audio side of a streamed queue (run_queued) and of q3tts_debug_codec_stream_slots
    // the bursts of frame steps with their TOKEN events and streamed chunks; fills J.frames, returns the frame steps
    int frame_loop(Job& J, const std::vector<ResolvedRequest>& rr, const q3tts_sampling& sp, q3tts_event_cb cb, void* user,
                   const DebugOpts* dbg, StreamedDecode& sd);
    void hand_off(Job& J, const std::vector<ResolvedRequest>& rr, StreamedDecode& sd, int launched, bool overlapped);
    // frame_loop, hand_off, job_timing, publish_job: on the caller's thread inside begin, or on the worker thread
    void back_half(Job& J, const std::vector<ResolvedRequest>& rr, const std::vector<int>& np, const q3tts_sampling& sp,
                   q3tts_event_cb cb, void* user, const DebugOpts* dbg, bool streamed, bool overlapped, double t_start);
    void worker_loop();  // one long-lived thread per engine, started by the first background job
    std::thread worker_;
    std::mutex work_mu_;
    std::condition_variable work_cv_;
    Job* work_ = nullptr;  // the job whose back half the worker takes next
    bool work_stop_ = false;
    void job_timing(Job& J, const std::vector<int>& np, int launched);
    void upload_sampling(const q3tts_sampling& sp, uint32_t row0, int n);  // sp_dev_[0, n) on st_: entry b = fold_sampling(sp, b, row0)
    int64_t kv_bytes(int n_prompt, int frames) const;  // talker KV bytes the frame steps of one row read
    int launches_per_step(int B) const;
    // builds prompt_/trailing_/tts_pad_ for rows [0,n); fills host-side lengths. trailing_rows: row of trailing_ that
    // request b's trailing text goes to (queued admission: its slot); nullptr: row b
    void assemble_prompts(const std::vector<ResolvedRequest>& reqs, std::vector<int>& n_prompt, std::vector<int>& n_trailing,
                          const std::vector<int>* trailing_rows = nullptr);
    // positions 0 .. Pmax-2 of n right-aligned prompts (prompt_ rows 0..n-1) through the talker into the pages of `block_table`,
    // then the last position loaded into w.h / w.ss_a
    void enqueue_prefill(Stream& w, int n, int Pmax, const int32_t* block_table, int32_t* kv_len, const int32_t* n_prompt,
                         uint8_t* active);
    void project_rows(const std::vector<int32_t>& ids, int rows);  // ids -> proj_out_[rows][H]
    void enqueue_layers(const StackW& s, Stream& w, int B, uint16_t* kpool, uint16_t* vpool, size_t layer_stride,
                        const int32_t* block_table, int max_pages, const int32_t* kv_len, const uint8_t* active,
                        int ss_count_in, int fixed_len, int chunk, const int32_t* chunk_n_prompt, int chunk_r_base);
    void enqueue_talker_step(int B, bool with_head);
    void enqueue_cp_pass(int B, bool from_talker, int head, int cp_pos, bool projected = false);  // head: lm_head index or -1; cp_pos: tokens already cached
    void enqueue_frame(int B, const DebugOpts* dbg);
    FrameEndArgs frame_end_args(int B) const;
    hipGraphExec_t frame_graph(int B);
    // ---- continuous batching (run_queued) ----
    const uint32_t* frame_row_key_ = nullptr;  // non-null while a queued frame step is enqueued: the samplers key on it
    std::map<int, hipGraphExec_t> qgraphs_;   // frame_graph() while frame_row_key_ is set, keyed by slot count
    uint8_t* qws_ = nullptr;  // allocated at the first queued call
    Stream qk_{};             // activations of an admission's prefill (the frame step's tk_ carries the running rows)
    int32_t *q_bt_ = nullptr, *q_kv_len_ = nullptr, *q_n_prompt_ = nullptr;  // the admitted sub-batch
    uint8_t* q_active_ = nullptr;
    AdmitDesc* q_desc_ = nullptr;
    std::vector<AdmitDesc> q_desc_host_;
    uint32_t* row_key_ = nullptr;  // [max_batch] random key of every slot
    // open-text requests (a session): the frame step reads text_open_ and raises starved_ (row_jobs.h frame_end_job) only while
    // frame_text_open_ is set -- the closed queue, static batches and begin / end jobs pass nullptr and capture graphs of their own
    uint8_t *text_open_ = nullptr, *starved_ = nullptr;  // [max_batch]
    const uint8_t* frame_text_open_ = nullptr;
    std::map<int, hipGraphExec_t> ographs_;  // frame_graph() while frame_text_open_ is set, keyed by slot count
    TextAppendDesc* q_text_desc_ = nullptr;  // [max_batch]
    std::vector<TextAppendDesc> q_text_desc_host_;
    std::vector<int32_t> q_text_ids_;        // staging of a boundary's new ids (alive until the launch has been waited for)
    std::vector<int32_t> q_host_;  // staging of the sub-batch's arrays (alive until the next boundary's sync)
    void ensure_queue_ws();
    struct QueueRun;  // the slot loop of one run_queued call (engine_queue.cc); its slots are QSlot (queue_slots.h)
    struct QLive;
    // a boundary's appends (run_queued): new text rows and closes for the slots' open-text requests, one launch on st_
    void apply_text_appends(QueueShared& q, std::vector<QSlot>& sl, std::unordered_map<int, QLive>& live);
    // free slots of `sl` in slot order take the next requests of q (prompts, prefill and admit_rows_kernel as a sub-batch of
    // their own); returns how many were admitted. `live` takes every admitted request by ticket
    int admit(QueueShared& q, std::vector<QSlot>& sl, std::unordered_map<int, QLive>& live);
    void cancel_slots(uint64_t mask, int slots);  // one launch on st_: the listed slots are finished and inactive
    GemmArgs gemm_args(const LinearW& L, const uint16_t* x, int M) const;
};


class Session;

// The object behind q3tts_model: the model plus its engines. With n_streams > 1 they are lanes: q3tts_generate splits its
// rows contiguously over them, each lane driven by its own host thread on its own HIP stream. That never pays (a lane's
// frame step does not shrink with its rows) and stays as documented. With one lane (the default) the
// group holds TWO full-size engines, the job contexts: chains on different streams do overlap (1.6x for two), so two whole
// batches, each on a context of its own, are what the two-deep pipeline runs side by side (Engine::begin).
class EngineGroup {
  public:
    EngineGroup(std::unique_ptr<Model> model, const q3tts_load_opts& opts, float pitch = 0.0f, bool keep_formants = false);
    Model& model() { return *model_; }
    ~EngineGroup();
    Engine& lane0() {  // the engine behind the single-engine entry points; a back half still running on it finishes first
        lanes_[0]->drain();
        return *lanes_[0];
    }
    int n_lanes() const { return int(lanes_.size()); }
    const CodecRunner* codec_runner() const { return lanes_[0]->codec_runner(); }  // (every lane's runner has the same geometry)
    const q3tts_load_opts& opts() const { return opts_; }
    void generate(const q3tts_request* reqs, int n, const q3tts_sampling& sp, q3tts_event_cb cb, void* user,
                  q3tts_result* results, const DebugOpts* dbg, const Voice* const* voices = nullptr);
    // q3tts_voice_create / _free: the group owns its voices (whatever is still alive goes with it). A voice of another group,
    // or one already freed, is not `mine`
    Voice* create_voice(const float* audio, int64_t n_samples, const int32_t* ref_text_ids, int n_ref_text_ids, int sample_rate = 24000);
    void free_voice(Voice* v);
    Voice* adopt_voice(std::unique_ptr<Voice> v);  // a voice made elsewhere (a session's) joins the group's
    bool mine(const Voice* v) const;
    PrefixCache& prefix_cache() { return prefix_cache_; }
    // Two-deep pipeline (Engine::begin / end); the job id names the context and its slot. With more than one lane a job runs
    // to completion inside begin.
    int begin(const q3tts_request* reqs, int n, const q3tts_sampling& sp, q3tts_event_cb cb, void* user, bool more_follows);
    void end(int job, q3tts_result* results);
    // q3tts_generate_queued: every request checked up front; `slots` rows split over the lanes, one shared queue
    void generate_queued(const q3tts_request* reqs, int n, int slots, const q3tts_sampling& sp, q3tts_event_cb cb, void* user,
                         q3tts_result* results, const Voice* const* voices = nullptr);
    // q3tts_session_*: one session at a time; while it is open its loop thread owns the first context (api.cc refuses the
    // entry points that would use an engine). close_session joins the thread and returns the status the loop failed with (0: none)
    Session* open_session(const q3tts_session_opts_ex& so, const q3tts_sampling& sp, q3tts_event_cb cb, void* user);
    Session* session() const { return session_.get(); }
    int close_session(bool drain);
    std::string last_error;
    q3tts_timing timing{};
    std::vector<std::string> speakers;

  private:
    std::unique_ptr<Session> session_;
    // what a closed queue and a session check alike before the slot loop starts
    void check_queue_open(int slots, const q3tts_sampling& sp) const;
    // fn(i) for lanes 0..L-1, each on a thread of its own unless `serial`; then the first failed lane's Error is rethrown
    template <class F>
    static void run_lanes(int L, bool serial, F&& fn);
    struct Parked {  // lanes > 1: finished results waiting for end()
        bool busy = false;
        std::vector<q3tts_result> results;
        q3tts_timing timing{};
    } parked_[Engine::kJobSlots];
    std::unique_ptr<Model> model_;
    q3tts_load_opts opts_;
    std::mutex cb_mutex_;
    std::vector<std::unique_ptr<Engine>> lanes_;
    mutable std::mutex voices_mu_;  // (a session's threads create, name and free voices side by side)
    std::vector<std::unique_ptr<Voice>> voices_;
    PrefixCache prefix_cache_;  // the voices' tail states for streamed requests; a voice's entries go with it (free_voice)
    void check_voices(const q3tts_request* reqs, int n, const Voice* const* voices) const;  // status 3 before any GPU work
    // one lane: the second job context (lanes_[0] is the first). A job takes a context without an outstanding job, the one
    // that was not used last first, so that plain q3tts_generate calls alternate and a host's warm-up calls warm both.
    std::unique_ptr<Engine> ctx1_;
    int last_ctx_ = 1;
    bool background_ = false;  // jobs without a callback run their back half on the context's worker (off: Q3TTS_SERIAL_JOBS)
    Engine* free_context();  // throws when both contexts have a job outstanding
};

// A serving session (q3tts_session_*): the slot loop of the first context on a thread of its own, fed from a SessionQueue that
// any thread may submit to while the loop runs. The loop is Engine::run_queued, the one q3tts_generate_queued runs, with the
// session as its request source: ticket t is what index t is to a closed call.
class Session final : public RequestSource {
  public:
    struct Item {  // a submitted request as the queue holds it: self-contained (check_queued copied what the caller pointed at)
        ResolvedRequest rr;
        SamplingParams params{};
    };
    struct ClipJob {  // a live voice's front-end job as the queue holds it
        std::vector<float> clip;
        int rate = 24000;
    };
    Session(EngineGroup& g, Engine& lane, const q3tts_session_opts_ex& so, const q3tts_sampling& sp, q3tts_event_cb cb, void* user);
    ~Session() override;  // closes without drain
    // every check of a queued request on the calling thread; throws Error (3: refused, 9: max_pending waiting, or what the loop failed with)
    void submit(const q3tts_request& r, const Voice* voice, const q3tts_row_sampling* rs, int64_t* ticket);
    // open-text requests (include/q3tts.h): every check on the calling thread; throws Error 3 on a refusal, which changes nothing
    void submit_open(const q3tts_request& r, const q3tts_row_sampling* rs, int64_t* ticket);
    void append_text(int64_t ticket, const int32_t* ids, int32_t n, bool final);
    void text_stats(q3tts_session_text_stats* s) const { queue_.text_stats(s); }
    int cancel(int64_t ticket) { return queue_.cancel(ticket); }
    // live voices (include/q3tts.h "Live voices"): any thread; each throws Error on a refusal, which changes nothing
    Voice* create_voice(const float* audio, int64_t n_samples, int sample_rate, const int32_t* ref_text_ids, int n_ref_text_ids,
                        bool anonymous = false);
    void voice_wait(const Voice* v, int32_t timeout_ms, int32_t* ready);
    void free_voice(const Voice* v, bool count = true);
    void voice_stats(q3tts_session_voice_stats* s) const { queue_.voice_stats(s); }
    void wait(int64_t ticket, int32_t timeout_ms, q3tts_result* out, int32_t* ready);
    void stats(q3tts_session_stats* s) const { queue_.stats(s); }
    int close(bool drain);  // joins the loop thread; the status it failed with, or 0
    bool on_loop_thread() const { return std::this_thread::get_id() == thread_.get_id(); }
    std::string error() const;

    bool take(QueueItem& out) override;
    q3tts_result* result(int ticket) override { return queue_.result(ticket); }
    void complete(int ticket) override { queue_.complete(ticket); }
    bool open_ended() const override { return true; }
    bool wait_for_work() override { return queue_.wait_for_work(); }
    bool has_cancels() override { return queue_.has_cancels(); }
    void take_cancels(std::vector<int>& out) override;
    void complete_cancelled(int ticket) override { queue_.complete_cancelled(ticket); }
    void progress(int frame_steps, int admissions) override { queue_.progress(frame_steps, admissions); }
    bool open_text() const override { return true; }
    bool has_appends() override { return queue_.has_appends(); }
    void take_appends(std::vector<TextAppend>& out) override;
    void wait_for_text(bool can_admit, int timeout_ms = -1) override { queue_.wait_for_text(can_admit, timeout_ms); }
    void text_progress(int starved_now, int starve_events) override { queue_.text_progress(starved_now, starve_events); }
    bool live_voices() const override { return live_voices_ > 0; }
    VoicePool* voice_pool() override { return pool_.get(); }
    bool has_voice_work() override { return queue_.has_voice_work(); }
    int take_voice_jobs(std::vector<VoiceJob>& out, int max) override;
    void voice_done(int64_t id, double frontend_ms) override { queue_.voice_done(id, frontend_ms); }
    void release_voices(const std::function<void(const Voice*)>& before) override;
    void burst_done(int frame_steps, double ms, bool beside) override { queue_.burst_done(frame_steps, ms, beside); }

  private:
    void loop();
    int64_t voice_id(const Voice* v) const;  // -1: not a voice this session made (or released already)
    void submit_checked(const q3tts_request& r, const Voice* voice, const q3tts_row_sampling* rs, int64_t* ticket);
    EngineGroup& g_;
    Engine& lane_;
    const int slots_, max_ref_frames_, live_voices_, max_voices_;
    std::shared_ptr<VoicePool> pool_;  // max_voices_ places; the voices keep it alive behind the session
    mutable std::mutex vmu_;
    std::unordered_map<const Voice*, int64_t> vids_;  // the voices this session made and has not released

    q3tts_sampling sp_;
    q3tts_event_cb cb_;
    void* user_;
    SessionQueue<Item, ClipJob> queue_;
    mutable std::mutex err_mu_;
    std::string error_;  // what the loop thread failed with
    std::thread thread_;
};

}  // namespace q3
