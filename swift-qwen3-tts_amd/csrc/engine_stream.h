// engine_stream.h -- private to the engine sources (engine.cc, engine_queue.cc, engine_debug.cc): the clock, the workspace bump
// allocator and the AUDIO_CHUNK event they share, the slotted codec stream of a streamed queue, the streamed decode of a job, and
// a queued request between its admission and its result.
#pragma once
#include "engine.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <deque>

#include "codec.h"
#include "codec_kernels.h"

namespace q3 {

inline const char* const kCodecRangeMsg =
    "Audio decoding failed: the codec decoder produced a non-finite waveform -- also on the fp32 matrix-core convolutions (the "
    "reference's range), which a row is re-decoded on when it leaves the fp16 range of the default two-plane kernels";
inline double now_s() {
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
inline void audio_chunk(q3tts_event_cb cb, void* user, int request_index, const float* pcm, int64_t n, int64_t offset) {
    q3tts_event ev{};
    ev.kind = Q3TTS_EVENT_AUDIO_CHUNK;
    ev.request_index = request_index;
    ev.pcm = pcm;
    ev.n_samples = n;
    ev.sample_offset = offset;
    cb(user, &ev);
}
inline double device_memory_gb() {  // q3tts_generation_info.peak_memory_usage: what the device has in use now
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    return double(total_b - free_b) / 1e9;
}
// A result as every path starts it: zeroed, then its info. span: what generate_time reports (the job's time, or the request's
// from its admission to its retirement)
inline void fill_info(q3tts_result& r, int target_tokens, int frames, double span, double memory_gb) {
    std::memset(&r, 0, sizeof(r));
    r.info.prompt_token_count = target_tokens;  // tokens of `text` (Qwen3+Streaming.swift:106)
    r.info.generation_token_count = frames;
    r.info.prefill_time = 0;  // hard-coded in the reference (Qwen3+Streaming.swift:112)
    r.info.generate_time = span;
    r.info.tokens_per_second = span > 0 ? double(frames) / span : 0;
    r.info.peak_memory_usage = memory_gb;
}
// the INFO + AUDIO pair that ends a request that succeeded (the caller holds Engine::cb_lock)
inline void emit_info_audio(q3tts_event_cb cb, void* user, int index, const q3tts_result& r) {
    q3tts_event ev{};
    ev.kind = Q3TTS_EVENT_INFO;
    ev.request_index = index;
    ev.info = &r.info;
    cb(user, &ev);
    ev.kind = Q3TTS_EVENT_AUDIO;
    ev.info = nullptr;
    ev.pcm = r.pcm;
    ev.n_samples = r.n_samples;
    cb(user, &ev);
}

// The audio side of a streamed queue: one slotted codec stream (codec.h) over the queue's slots on the confined codec stream,
// the passes in flight, and every request's PCM as its chunks land. A request is complete once it has been retired and its
// last chunk has been taken from the ring.
struct Engine::SlotStream {
    Engine& e;
    hipStream_t cst = nullptr;
    const int C, up;      // up: samples per frame of a ring slot's rows (the slowest row's where rows have hops of their own)
    const int handle_up;  // what a request without a speed of its own gets
    bool hold = true;  // a request stops taking chunks at its first one flagged non-finite (the engine re-decodes it in fp32)
    struct Out {       // one request
        MallocPtr<float> pcm;  // [cap frames * up]
        int up = 0;            // the request's own samples per frame
        int frames = -1;       // its length, once retired
        int landed = 0;        // chunks taken from the ring
        int held_from = -1;    // first chunk held back
        bool complete = false;
        bool dropped = false;  // cancelled (a session): its chunks in flight land nowhere
    };
    std::unordered_map<int, Out> out;  // by request (its index in a closed call, its ticket in a session)
    std::vector<int> req_of_row;  // the request in row b, -1: none
    // The caller's code buffer ([rows][stride][16]) as stage_prefixes / stage_frames fill it, per row: `prefix` reference frames,
    // then generated frames [0, copied); reused: written for an occupant before, the last push's passes may still read it.
    std::vector<int> copied, prefix;
    std::vector<uint8_t> reused;
    bool recycle = true;  // rows take new occupants (a queue); false: the rows of one job, which nothing overwrites
    std::vector<DecodeRowDesc> desc;  // (read by stage_prefixes' upload until its stream is next synchronised)
    DevBuf<DecodeRowDesc> desc_dev;
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
        : e(eng), C(chunk), up(eng.codec_->stream_upsample()), handle_up(eng.codec_->upsample()), req_of_row(size_t(rows), -1), copied(size_t(rows), 0),
          prefix(size_t(rows), 0), reused(size_t(rows), 0) {
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
    // hs: the request's own synthesis hop (ResolvedRequest::hs), 0: the handle's
    void admit(int row, int req, int cap_frames, int n_prefix = 0, const uint8_t* state = nullptr, int hs = 0) {
        // on cst: behind the previous occupant's last chunk, in front of this one's first
        if (e.codec_->stream_own_hops()) e.codec_->stream_set_row_hs(row, hs ? hs : e.codec_->stretch_hs());
        if (state) e.codec_->stream_load_row(row, n_prefix, state);
        else e.codec_->stream_reset_row(row, n_prefix);
        req_of_row[size_t(row)] = req;
        copied[size_t(row)] = 0;
        prefix[size_t(row)] = n_prefix;
        Out& o = out[req];
        o.up = hs ? e.codec_->upsample_of(hs) : handle_up;
        o.pcm.reset(static_cast<float*>(std::malloc(std::max<size_t>(size_t(cap_frames) * o.up * 4, 4))));
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
                const int64_t off = int64_t(r.k) * C * o.up, n = int64_t(r.take) * o.up;  // (the row's samples lie at the start of its part)
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
    void codes_staged(hipStream_t st) {  // ev_codes behind a boundary's copies on st; cst waits for it before the push reads them
        Q3_HIP(hipEventRecord(ev_codes, st));
        Q3_HIP(hipStreamWaitEvent(cst, ev_codes, 0));
    }
    // New occupants' reference frames ref[b] ([16][n_ref[b]] on the device; 0: none) to the front of their rows, on st, before
    // their admit(). The builder also moves one frame of gen that does not exist yet: frame n_ref[b] of the row, read by nothing
    // before stage_frames has written it. They overwrite what the previous occupant's last chunks read: behind ev_pushed.
    void stage_prefixes(const int32_t* const* ref, const int* n_ref, const int32_t* gen, int gen_stride, int32_t* codes, int stride,
                        hipStream_t st) {
        const size_t R = req_of_row.size();
        bool wait = false;
        desc.assign(R, DecodeRowDesc{});
        for (size_t b = 0; b < R; ++b) {
            if (n_ref[b] <= 0) continue;
            desc[b] = DecodeRowDesc{ref[b], gen + b * gen_stride * 16, n_ref[b], 1, int(b), 0};
            wait = wait || reused[b];
            reused[b] = recycle;
        }
        if (wait) Q3_HIP(hipStreamWaitEvent(st, ev_pushed, 0));
        Q3_HIP(hipMemcpyAsync(desc_dev.grow(R), desc.data(), R * sizeof(DecodeRowDesc), hipMemcpyHostToDevice, st));
        launch_build_decode_codes_rows(desc.data(), desc_dev, int(R), codes, int(R), stride, st);
        codes_staged(st);
    }
    // Frames [copied, upto[b]) of every row of gen ([rows][gen_stride][16]) to behind the row's prefix, on st. A continuing
    // occupant's lie behind everything an issued pass reads. A NEW occupant's first frames overwrite what the previous one's
    // last chunks read: that copy waits for ev_pushed, recorded on cst behind the latest push -- the one that issued them.
    void stage_frames(const int* upto, const int32_t* gen, int gen_stride, int32_t* codes, int stride, hipStream_t st) {
        const size_t R = req_of_row.size();
        bool first = false, any = false;
        for (size_t b = 0; b < R; ++b) first = first || (upto[b] > 0 && copied[b] == 0 && reused[b]);
        if (first) Q3_HIP(hipStreamWaitEvent(st, ev_pushed, 0));
        for (size_t b = 0; b < R; ++b) {
            if (upto[b] <= copied[b]) continue;
            Q3_HIP(hipMemcpyAsync(codes + (b * stride + prefix[b] + copied[b]) * 16, gen + (b * gen_stride + copied[b]) * 16,
                                  size_t(upto[b] - copied[b]) * 64, hipMemcpyDeviceToDevice, st));
            copied[b] = upto[b];
            reused[b] = recycle;
            any = true;
        }
        if (any) codes_staged(st);
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
        if (any_clone || !J.row_hs.empty()) {  // (rows with hops of their own: the slotted stream has a hop per row)
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
        ss->recycle = false;
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
        // every clone row's reference frames to the front of its code row
        std::vector<const int32_t*> ref(size_t(J.n), nullptr);
        std::vector<int> n_ref(size_t(J.n), 0);
        for (int b = 0; b < J.n; ++b)
            if (rr[size_t(b)].clone && rr[size_t(b)].ref_T > 0) {
                ref[size_t(b)] = e.ref_codes_dev_ + rr[size_t(b)].ref_off;
                n_ref[size_t(b)] = rr[size_t(b)].ref_T;
            }
        if (ref_max > 0) ss->stage_prefixes(ref.data(), n_ref.data(), e.codes_, e.Fcap_, J.dec_codes, stride, e.st_);
        for (int b = 0; b < J.n; ++b) ss->admit(b, b, e.Fcap_, n_ref[size_t(b)], nullptr, rr[size_t(b)].hs);
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
            if (upto > copied) {  // (every row alike, whatever its own length)
                ss->stage_frames(std::vector<int>(size_t(J.n), upto).data(), e.codes_, e.Fcap_, J.dec_codes, stride, e.st_);
                copied = upto;
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
            const size_t rup = size_t(J.row_up[size_t(b)]);  // (the row's own samples per frame; J.up is the layout's)
            std::memcpy(J.pcm_host + size_t(b) * stride * J.up + size_t(ss->prefix[size_t(b)]) * rup, o.pcm.get(),
                        size_t(J.frames[size_t(b)]) * rup * 4);
            J.held_from[size_t(b)] = o.held_from;
            J.nf_host[b] = o.held_from >= 0 ? 1 : 0;
        }
        if (ss->have_first) J.timing.first_audio_ms = ss->first_audio_ms;
    }
};

// One admitted request until its result is filled: what was resolved at its submission and, once its row is retired, what it
// generated (streamed: until its last chunk has landed; otherwise until its decode batch is delivered).
struct Engine::QLive {
    ResolvedRequest rr;
    int frames = 0;
    double span = 0;             // admission -> retirement
    std::vector<int32_t> codes;  // [frames][16]
};

}  // namespace q3
