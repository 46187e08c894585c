// session_queue.h -- the host-only bookkeeping of a serving session (include/q3tts.h, q3tts_session_*): ticket assignment, the
// pending requests, cancel marks, the result store and wait / notify. No HIP include, so
// tests/native/session_queue_driver.cc compiles it with a plain C++ compiler and runs it under the sanitizers.
//
// Producers (any thread): submit, cancel, wait, stats, close. One consumer (the session's loop thread): take / wait_for_work /
// take_cancels / result / complete / fail. A ticket is Pending (accepted, in the deque), Running (handed to the consumer) or Done
// (its result is filled and waits to be claimed); a claimed ticket is forgotten.
//
// Open-text tickets (submit with open = true, q3tts_session_submit_open): the request's text grows through append_text until an
// append closes it. Text for a Pending ticket is kept beside the stored request and handed out with it (take); text for a Running
// one goes into the append mailbox, which the consumer empties at its boundaries (take_appends); text for a Done or claimed one is
// dropped. The consumer sleeps in wait_for_text() while every row it runs waits for text; an append, a cancel, a submit it
// could admit, or close wakes it.
//
// Live voices (enable_voices, q3tts_session_voice_*): a voice is Queued (its front-end job waits in the mailbox), Running (the
// consumer has launched it), Ready or Abandoned (a close without drain, or a failure, came first). A ticket may name a voice in
// any state but Abandoned; take() hands out only tickets whose voice is Ready and passes over the others, so they hold nobody
// back. A voice counts the tickets that name it, pending and running; free_voice() only marks it, and the consumer is given it
// for release (take_voice_releases) once nothing uses it and its job is neither waiting behind a use nor running.
#pragma once
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <deque>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/q3tts.h"

// gcc 11's thread sanitizer runtime does not see through pthread_cond_clockwait, which a steady-clock timed wait becomes, and then
// reports the mutex as never released. A build under that sanitizer (the test driver's) waits against the system clock instead,
// which is pthread_cond_timedwait; every other build waits against the steady clock, so that a step of the wall clock does not
// stretch or shorten a timeout.
#if defined(__SANITIZE_THREAD__)
#define Q3_SESSION_WAIT_CLOCK std::chrono::system_clock
#elif defined(__has_feature)
#if __has_feature(thread_sanitizer)
#define Q3_SESSION_WAIT_CLOCK std::chrono::system_clock
#endif
#endif
#ifndef Q3_SESSION_WAIT_CLOCK
#define Q3_SESSION_WAIT_CLOCK std::chrono::steady_clock
#endif

namespace q3 {

template <class Req, class VoiceJob = int>
class SessionQueue {
  public:
    using FreeFn = void (*)(q3tts_result*);  // frees what a result points at (q3tts_result_free of one result)
    static constexpr int kDefaultPending = 1024;

    SessionQueue(int max_pending, FreeFn free_fn) : max_pending_(max_pending > 0 ? max_pending : kDefaultPending), free_(free_fn) {}
    ~SessionQueue() {  // unclaimed results go with the queue
        for (auto& kv : entries_)
            if (kv.second.state == Done) free_(&kv.second.res);
    }
    SessionQueue(const SessionQueue&) = delete;
    SessionQueue& operator=(const SessionQueue&) = delete;

    // ---- producers ----
    // The t-th accepted submit gets ticket t. A refused one (BUSY, closing, failed) consumes no ticket.
    // open: an open-text ticket holding n_content content tokens so far, at most text_cap in all.
    // voice >= 0: the ticket names that voice (submit_voice), which must be alive, not freed and not abandoned.
    int submit(Req&& r, int64_t* ticket, bool open = false, int n_content = 0, int text_cap = 0, int64_t voice = -1) {
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (failed_) return failed_;
            if (closing_) return Q3TTS_ERR_INVALID_INPUT;
            if (next_ > int64_t(INT32_MAX)) return Q3TTS_ERR_INVALID_INPUT;  // events carry the ticket as an int32
            VoiceEntry* ve = nullptr;
            if (voice >= 0) {
                auto vi = voices_.find(voice);
                if (vi == voices_.end() || vi->second.freed || vi->second.state == VoiceAbandoned) return Q3TTS_ERR_INVALID_INPUT;
                ve = &vi->second;
            }
            if (int(pending_.size()) >= max_pending_) return Q3TTS_ERR_BUSY;
            const int64_t t = next_++;
            Entry& e = entries_[t];
            e.req = std::move(r);
            e.voice = voice;
            if (ve) ++ve->use;
            e.open = open;
            e.n_content = n_content;
            e.text_cap = text_cap;
            kind_.push_back(open ? kOpen : kPlain);
            pending_.push_back(t);
            ++submitted_;
            if (ticket) *ticket = t;
        }
        work_cv_.notify_one();
        return Q3TTS_OK;
    }
    // Pending: never handed out, Done at once with CANCELLED. Running: marked, the consumer completes it at its next boundary.
    // Done, claimed or already marked: nothing changes. A ticket that was never given out: INVALID_INPUT.
    int cancel(int64_t ticket) {
        bool done = false, marked = false;
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (ticket < 0 || ticket >= next_) return Q3TTS_ERR_INVALID_INPUT;
            auto it = entries_.find(ticket);
            if (it == entries_.end()) return Q3TTS_OK;  // claimed
            Entry& e = it->second;
            if (e.state == Pending) {
                pending_.erase(std::find(pending_.begin(), pending_.end(), ticket));
                finish_locked(e, Q3TTS_ERR_CANCELLED, true);
                done = true;
            } else if (e.state == Running && !e.cancel) {
                e.cancel = true;
                cancels_.push_back(ticket);
                marked = true;
            }
        }
        if (marked || done) work_cv_.notify_all();  // (a consumer whose rows all wait for text sleeps on it; done: a voice may have lost its last use)
        if (done) done_cv_.notify_all();
        return Q3TTS_OK;
    }
    // One append of an open-text request, and the wake-up of a consumer that waits for it.
    struct TextMsg {
        int64_t ticket = -1;
        std::vector<int32_t> ids;
        bool final = false;
    };
    // n >= 0 content tokens behind the ticket's text; final closes it. INVALID_INPUT, with nothing changed and *why saying so: a
    // ticket never given out, one from a plain submit, one whose text is closed, n < 0, more content than text_cap. A ticket that is
    // Done or claimed (it ended early, hit its cap or was cancelled -- the race is the caller's to lose): OK, and the text is dropped.
    int append_text(int64_t ticket, const int32_t* ids, int32_t n, bool final, std::string* why = nullptr) {
        auto refuse = [&](const char* w) {
            if (why) *why = w;
            return int(Q3TTS_ERR_INVALID_INPUT);
        };
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (failed_) return failed_;
            if (ticket < 0 || ticket >= next_) return refuse("Invalid input: no such ticket");
            if (kind_[size_t(ticket)] == kPlain) return refuse("Invalid input: the ticket is not an open-text request");
            if (kind_[size_t(ticket)] == kClosed) return refuse("Invalid input: the ticket's text has been closed");
            if (n < 0 || (n > 0 && !ids)) return refuse("Invalid input: n must not be negative");
            auto it = entries_.find(ticket);
            if (it == entries_.end() || it->second.state == Done) return Q3TTS_OK;  // dropped
            Entry& e = it->second;
            if (e.n_content + int64_t(n) > int64_t(e.text_cap)) return refuse("Invalid input: text longer than max_prompt");
            e.n_content += n;
            appended_tokens_ += n;
            if (final) kind_[size_t(ticket)] = kClosed;
            if (e.state == Pending) {
                e.early.insert(e.early.end(), ids, ids + n);
            } else if (n > 0 || final) {
                appends_.emplace_back();
                appends_.back().ticket = ticket;
                appends_.back().ids.assign(ids, ids + n);
                appends_.back().final = final;
            }
        }
        work_cv_.notify_all();
        return Q3TTS_OK;
    }
    void text_stats(q3tts_session_text_stats* s) const {
        std::lock_guard<std::mutex> lk(mu_);
        std::memset(s, 0, sizeof(*s));
        for (const auto& kv : entries_)
            if (kv.second.open && kv.second.state != Done && kind_[size_t(kv.first)] == kOpen) ++s->open;
        s->starved = starved_;
        s->appended_tokens = appended_tokens_;
        s->starve_events = starve_events_;
    }
    // *ready = 1: the result is the caller's and the ticket is forgotten. *ready = 0 (timeout): nothing is touched.
    int wait(int64_t ticket, int32_t timeout_ms, q3tts_result* out, int32_t* ready) {
        if (ready) *ready = 0;
        std::unique_lock<std::mutex> lk(mu_);
        auto settled = [&] {
            auto it = entries_.find(ticket);
            return it == entries_.end() || it->second.state == Done;
        };
        if (entries_.find(ticket) == entries_.end()) return Q3TTS_ERR_INVALID_INPUT;
        if (timeout_ms < 0) done_cv_.wait(lk, settled);
        else done_cv_.wait_until(lk, Q3_SESSION_WAIT_CLOCK::now() + std::chrono::milliseconds(timeout_ms), settled);
        auto it = entries_.find(ticket);
        if (it == entries_.end()) return Q3TTS_ERR_INVALID_INPUT;  // (another waiter claimed it)
        if (it->second.state != Done) return Q3TTS_OK;
        if (out) *out = it->second.res;
        else free_(&it->second.res);
        entries_.erase(it);
        if (ready) *ready = 1;
        return Q3TTS_OK;
    }
    void stats(q3tts_session_stats* s) const {
        std::lock_guard<std::mutex> lk(mu_);
        std::memset(s, 0, sizeof(*s));
        s->submitted = submitted_;
        s->pending = int64_t(pending_.size());
        s->running = running_;
        s->completed = completed_;
        s->cancelled = cancelled_;
        s->frame_steps = frame_steps_;
        s->admissions = admissions_;
    }
    // No submit is accepted any more. drain: everything accepted still runs; otherwise every pending ticket is cancelled at once
    // and every running one is marked. The consumer's wait_for_work() returns false once nothing is pending.
    void close(bool drain) {
        {
            std::lock_guard<std::mutex> lk(mu_);
            closing_ = true;
            if (drain) {  // every open text is closed first: the ticket then ends as if its last append had been final
                for (auto& kv : entries_) {
                    if (kv.second.state == Done || kind_[size_t(kv.first)] != kOpen) continue;
                    kind_[size_t(kv.first)] = kClosed;
                    if (kv.second.state == Running) {
                        appends_.emplace_back();
                        appends_.back().ticket = kv.first;
                        appends_.back().final = true;
                    }
                }
            }
            if (!drain) {
                for (int64_t t : pending_) finish_locked(entries_[t], Q3TTS_ERR_CANCELLED, true);
                pending_.clear();
                for (auto& kv : entries_)
                    if (kv.second.state == Running && !kv.second.cancel) {
                        kv.second.cancel = true;
                        cancels_.push_back(kv.first);
                    }
                abandon_voices_locked(false);  // jobs not launched yet; the launched ones finish (they are short)
            }
        }
        work_cv_.notify_all();
        done_cv_.notify_all();
        voice_cv_.notify_all();
    }
    int failed() const {
        std::lock_guard<std::mutex> lk(mu_);
        return failed_;
    }

    // ---- the consumer ----
    // the next pending request in ticket order (it is Running from here on); false: none is waiting now
    // An open-text ticket as take() hands it out: the content that arrived while it was pending, and whether its text is closed
    // already (it is then an ordinary request). From here on its appends go through the mailbox.
    struct TextTake {
        bool open = false, closed = false;
        std::vector<int32_t> early;
    };
    bool take(int64_t* ticket, Req* out, TextTake* text = nullptr) {
        std::lock_guard<std::mutex> lk(mu_);
        if (pending_.empty() || failed_) return false;
        auto first = first_admissible_locked();  // (without voices: the front)
        if (first == pending_.end()) return false;
        const int64_t t = *first;
        pending_.erase(first);
        Entry& e = entries_[t];
        e.state = Running;
        *out = std::move(e.req);
        e.req = Req();
        if (text) {
            text->open = e.open;
            text->closed = kind_[size_t(t)] == kClosed;
            text->early = std::move(e.early);
        }
        e.early = std::vector<int32_t>();
        *ticket = t;
        ++running_;
        return true;
    }
    // nothing is running: sleeps until a request is pending (true) or the queue is closing with none left (false)
    // (with live voices: a request that can be admitted, a voice job to launch or a voice to release)
    bool wait_for_work() {
        std::unique_lock<std::mutex> lk(mu_);
        auto work = [&] { return first_admissible_locked() != pending_.end() || !vjobs_.empty() || !vreleases_.empty(); };
        work_cv_.wait(lk, [&] { return work() || closing_ || failed_; });
        return work() && !failed_;
    }
    // Every running row waits for text: sleeps until there is something to do at a boundary -- an append or a cancel in the
    // mailboxes, a pending request while `can_admit`, or the first look after close() -- and never spins: each of these is consumed by
    // the boundary that follows.
    // timeout_ms >= 0: returns after that long at the latest (the consumer has something of its own to poll)
    void wait_for_text(bool can_admit, int timeout_ms = -1) {
        std::unique_lock<std::mutex> lk(mu_);
        auto due = [&] {
            return !appends_.empty() || !cancels_.empty() || (can_admit && first_admissible_locked() != pending_.end()) ||
                   !vjobs_.empty() || !vreleases_.empty() || (closing_ && !close_seen_) || failed_;
        };
        if (timeout_ms < 0) work_cv_.wait(lk, due);
        else if (!work_cv_.wait_until(lk, Q3_SESSION_WAIT_CLOCK::now() + std::chrono::milliseconds(timeout_ms), due)) return;
        if (closing_) close_seen_ = true;
    }
    bool has_appends() const {
        std::lock_guard<std::mutex> lk(mu_);
        return !appends_.empty();
    }
    void take_appends(std::vector<TextMsg>& out) {  // in arrival order
        std::lock_guard<std::mutex> lk(mu_);
        out.assign(std::make_move_iterator(appends_.begin()), std::make_move_iterator(appends_.end()));
        appends_.clear();
    }
    void text_progress(int starved_now, int starve_events) {
        std::lock_guard<std::mutex> lk(mu_);
        starved_ = starved_now;
        starve_events_ += starve_events;
    }
    bool has_cancels() const {
        std::lock_guard<std::mutex> lk(mu_);
        return !cancels_.empty();
    }
    void take_cancels(std::vector<int64_t>& out) {  // running tickets marked since the last call
        std::lock_guard<std::mutex> lk(mu_);
        out.assign(cancels_.begin(), cancels_.end());
        cancels_.clear();
    }
    // A running ticket's result: a stable address that only the consumer writes until complete(). nullptr: not running.
    q3tts_result* result(int64_t ticket) {
        std::lock_guard<std::mutex> lk(mu_);
        auto it = entries_.find(ticket);
        return it != entries_.end() && it->second.state == Running ? &it->second.res : nullptr;
    }
    void complete(int64_t ticket) {  // its result is filled (status included)
        {
            std::lock_guard<std::mutex> lk(mu_);
            auto it = entries_.find(ticket);
            if (it == entries_.end() || it->second.state != Running) return;
            --running_;
            finish_locked(it->second, it->second.res.status, false);
        }
        done_cv_.notify_all();
    }
    void complete_cancelled(int64_t ticket) {  // whatever the consumer had put into its result is freed
        {
            std::lock_guard<std::mutex> lk(mu_);
            auto it = entries_.find(ticket);
            if (it == entries_.end() || it->second.state != Running) return;
            --running_;
            finish_locked(it->second, Q3TTS_ERR_CANCELLED, true);
        }
        done_cv_.notify_all();
    }
    // the consumer has failed: every pending and running ticket completes with `status`, and every later submit returns it
    void fail(int status) {
        {
            std::lock_guard<std::mutex> lk(mu_);
            failed_ = status;
            pending_.clear();
            cancels_.clear();
            for (auto& kv : entries_) {
                Entry& e = kv.second;
                if (e.state == Done) continue;
                if (e.state == Running) --running_;
                finish_locked(e, status, true);
            }
            abandon_voices_locked(true);
        }
        work_cv_.notify_all();
        done_cv_.notify_all();
        voice_cv_.notify_all();
    }
    void progress(int frame_steps, int admissions) {
        std::lock_guard<std::mutex> lk(mu_);
        frame_steps_ += frame_steps;
        admissions_ += admissions;
    }

    // ---- live voices ----
    enum VoiceState { VoiceQueued, VoiceRunning, VoiceReady, VoiceAbandoned };
    struct VoiceTake {  // a job as the consumer takes it; tag: what submit_voice was given (the consumer's handle of the voice)
        int64_t id = -1;
        void* tag = nullptr;
        VoiceJob job{};
    };
    // live: front-end jobs waiting or running at most; max_alive: voices not yet released at most. Before the first submit_voice.
    void enable_voices(int live, int max_alive) {
        std::lock_guard<std::mutex> lk(mu_);
        live_voices_ = live;
        max_voices_ = max_alive;
    }
    // A new voice and its front-end job. BUSY: live jobs are waiting or running, or max_alive voices are alive. anonymous: made
    // for one ticket (counted apart).
    int submit_voice(VoiceJob&& job, void* tag, int64_t* id, bool anonymous = false) {
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (failed_) return failed_;
            if (closing_ || live_voices_ <= 0) return Q3TTS_ERR_INVALID_INPUT;
            if (int(vjobs_.size()) + v_running_ >= live_voices_ || int(voices_.size()) >= max_voices_) return Q3TTS_ERR_BUSY;
            const int64_t v = v_next_++;
            VoiceEntry& e = voices_[v];
            e.job = std::move(job);
            e.tag = tag;
            vjobs_.push_back(v);
            ++v_created_;
            if (anonymous) ++v_anonymous_;
            if (id) *id = v;
        }
        work_cv_.notify_all();
        return Q3TTS_OK;
    }
    // The voice can be named no more. It is released at once when nothing uses it (a job still waiting is dropped: the voice is
    // Abandoned), otherwise when its last ticket completes and its job has finished; count: such a free is a deferred one.
    int free_voice(int64_t id, bool count = true) {
        {
            std::lock_guard<std::mutex> lk(mu_);
            auto it = voices_.find(id);
            if (it == voices_.end() || it->second.freed) return Q3TTS_ERR_INVALID_INPUT;
            VoiceEntry& e = it->second;
            e.freed = true;
            if (e.state == VoiceQueued && e.use == 0) {
                vjobs_.erase(std::find(vjobs_.begin(), vjobs_.end(), id));
                e.state = VoiceAbandoned;
                e.job = VoiceJob();
            }
            if (!release_if_unused_locked(id, e) && count) ++v_deferred_;
        }
        work_cv_.notify_all();
        voice_cv_.notify_all();
        return Q3TTS_OK;
    }
    // *ready = 1: Ready. CANCELLED: Abandoned. *ready = 0 and OK: timeout. INVALID_INPUT: no such voice, or freed.
    int voice_wait(int64_t id, int32_t timeout_ms, int32_t* ready) {
        if (ready) *ready = 0;
        std::unique_lock<std::mutex> lk(mu_);
        auto settled = [&] {
            auto it = voices_.find(id);
            return it == voices_.end() || it->second.freed || it->second.state == VoiceReady || it->second.state == VoiceAbandoned;
        };
        if (voices_.find(id) == voices_.end()) return Q3TTS_ERR_INVALID_INPUT;
        if (timeout_ms < 0) voice_cv_.wait(lk, settled);
        else voice_cv_.wait_until(lk, Q3_SESSION_WAIT_CLOCK::now() + std::chrono::milliseconds(timeout_ms), settled);
        auto it = voices_.find(id);
        if (it == voices_.end() || it->second.freed) return Q3TTS_ERR_INVALID_INPUT;
        if (it->second.state == VoiceAbandoned) return Q3TTS_ERR_CANCELLED;
        if (it->second.state == VoiceReady && ready) *ready = 1;
        return Q3TTS_OK;
    }
    int voice_state(int64_t id) const {  // -1: no such voice
        std::lock_guard<std::mutex> lk(mu_);
        auto it = voices_.find(id);
        return it == voices_.end() ? -1 : int(it->second.state);
    }
    void voice_stats(q3tts_session_voice_stats* s) const {
        std::lock_guard<std::mutex> lk(mu_);
        std::memset(s, 0, sizeof(*s));
        s->created = v_created_;
        s->ready = v_ready_;
        s->in_flight = int64_t(vjobs_.size()) + v_running_;
        s->alive = int64_t(voices_.size());  // (a voice on its way out holds its place until the consumer's next boundary)
        s->deferred_frees = v_deferred_;
        s->anonymous = v_anonymous_;
        s->frontend_ms_sum = fe_ms_sum_;
        s->frame_steps_beside = steps_beside_;
        s->burst_ms_beside = burst_ms_beside_;
        s->burst_ms_alone = burst_ms_alone_;
    }
    // the consumer: up to `max` waiting jobs in arrival order (Running from here on)
    int take_voice_jobs(std::vector<VoiceTake>& out, int max) {
        std::lock_guard<std::mutex> lk(mu_);
        out.clear();
        while (int(out.size()) < max && !vjobs_.empty() && !failed_) {
            const int64_t v = vjobs_.front();
            vjobs_.pop_front();
            VoiceEntry& e = voices_[v];
            e.state = VoiceRunning;
            ++v_running_;
            out.emplace_back();
            out.back().id = v;
            out.back().tag = e.tag;
            out.back().job = std::move(e.job);
            e.job = VoiceJob();
        }
        return int(out.size());
    }
    bool has_voice_work() const {
        std::lock_guard<std::mutex> lk(mu_);
        return !vjobs_.empty() || !vreleases_.empty();
    }
    void voice_done(int64_t id, double frontend_ms) {  // the consumer: the job has finished, the voice is Ready
        {
            std::lock_guard<std::mutex> lk(mu_);
            auto it = voices_.find(id);
            if (it == voices_.end() || it->second.state != VoiceRunning) return;
            it->second.state = VoiceReady;
            --v_running_;
            ++v_ready_;
            fe_ms_sum_ += frontend_ms;
            (void)release_if_unused_locked(id, it->second);
        }
        voice_cv_.notify_all();
        work_cv_.notify_all();
    }
    // the consumer: voices to release now (each is handed out once); voice_released() forgets one and frees its place
    void take_voice_releases(std::vector<std::pair<int64_t, void*>>& out) {
        std::lock_guard<std::mutex> lk(mu_);
        out.clear();
        for (int64_t v : vreleases_) out.emplace_back(v, voices_[v].tag);
        vreleases_.clear();
    }
    void voice_released(int64_t id) {
        std::lock_guard<std::mutex> lk(mu_);
        voices_.erase(id);
    }
    // a burst of n frame steps took the consumer `ms` from its launch to its end; beside: a voice job was in flight meanwhile
    void burst_done(int n, double ms, bool beside) {
        std::lock_guard<std::mutex> lk(mu_);
        if (beside) {
            steps_beside_ += n;
            burst_ms_beside_ += ms;
        } else {
            burst_ms_alone_ += ms;
        }
    }
    // Behind the consumer's end: what the queue still knows of -- voices freed but not released (first) and voices never freed
    // (state: their VoiceState) -- is the caller's from here on; pending tickets that could not run any more are cancelled.
    struct VoiceLeft {
        int64_t id = -1;
        void* tag = nullptr;
        int state = 0;
        bool freed = false;
    };
    void retire_voices(std::vector<VoiceLeft>& out) {
        {
            std::lock_guard<std::mutex> lk(mu_);
            for (int64_t t : pending_) finish_locked(entries_[t], Q3TTS_ERR_CANCELLED, true);
            pending_.clear();
            abandon_voices_locked(true);
            out.clear();
            for (auto& kv : voices_) {
                out.emplace_back();
                out.back().id = kv.first;
                out.back().tag = kv.second.tag;
                out.back().state = int(kv.second.state);
                out.back().freed = kv.second.freed;
            }
            voices_.clear();
            vreleases_.clear();
        }
        done_cv_.notify_all();
        voice_cv_.notify_all();
    }

  private:
    enum State { Pending, Running, Done };
    enum Kind : uint8_t { kPlain, kOpen, kClosed };  // kOpen: an open-text ticket whose text is not closed yet
    struct Entry {
        State state = Pending;
        bool cancel = false;
        bool open = false;           // submitted as an open-text request
        int n_content = 0, text_cap = 0;
        std::vector<int32_t> early;  // content appended while Pending
        int64_t voice = -1;          // the voice it names (counted in that voice's use until the ticket is Done)
        Req req{};
        q3tts_result res{};
    };
    struct VoiceEntry {
        VoiceState state = VoiceQueued;
        bool freed = false, releasing = false;
        int64_t use = 0;  // tickets that name it, Pending or Running
        void* tag = nullptr;
        VoiceJob job{};
    };
    // the first pending ticket whose voice, if it names one, is Ready
    typename std::deque<int64_t>::iterator first_admissible_locked() {
        if (voices_.empty()) return pending_.begin();
        for (auto it = pending_.begin(); it != pending_.end(); ++it) {
            const int64_t v = entries_[*it].voice;
            if (v < 0) return it;
            auto vi = voices_.find(v);
            if (vi != voices_.end() && vi->second.state == VoiceReady) return it;
        }
        return pending_.end();
    }
    bool release_if_unused_locked(int64_t id, VoiceEntry& e) {
        if (!e.freed || e.use > 0 || e.releasing || (e.state != VoiceReady && e.state != VoiceAbandoned)) return false;
        e.releasing = true;
        vreleases_.push_back(id);
        return true;
    }
    // every waiting job is dropped; all: the launched ones count as lost too (the consumer has failed or ended)
    void abandon_voices_locked(bool all) {
        for (auto& kv : voices_) {
            VoiceEntry& e = kv.second;
            if (e.state == VoiceQueued || (all && e.state == VoiceRunning)) {
                if (e.state == VoiceRunning) --v_running_;
                e.state = VoiceAbandoned;
                e.job = VoiceJob();
                (void)release_if_unused_locked(kv.first, e);
            }
        }
        vjobs_.clear();
    }
    void finish_locked(Entry& e, int status, bool wipe) {  // wipe: the result carries nothing but the status
        e.state = Done;
        e.req = Req();
        e.early = std::vector<int32_t>();
        if (e.voice >= 0) {  // (notified by the caller, with done_cv_: the consumer looks at its next boundary anyway)
            auto vi = voices_.find(e.voice);
            if (vi != voices_.end()) {
                --vi->second.use;
                (void)release_if_unused_locked(e.voice, vi->second);
            }
            e.voice = -1;
        }
        if (wipe) {
            free_(&e.res);
            std::memset(&e.res, 0, sizeof(e.res));
        }
        e.res.status = static_cast<q3tts_status>(status);
        if (status == Q3TTS_ERR_CANCELLED) ++cancelled_;
        else ++completed_;
    }

    mutable std::mutex mu_;
    std::condition_variable work_cv_, done_cv_, voice_cv_;
    const int max_pending_;
    const FreeFn free_;
    std::map<int64_t, Entry> entries_;  // every ticket that is not claimed yet
    std::deque<int64_t> pending_;       // in ticket order
    std::deque<int64_t> cancels_;
    std::deque<TextMsg> appends_;       // text for Running tickets, in arrival order
    std::vector<uint8_t> kind_;         // by ticket, for every ticket ever given out (a claimed ticket is still refused correctly)
    int64_t starved_ = 0, appended_tokens_ = 0, starve_events_ = 0;
    bool close_seen_ = false;
    int64_t next_ = 0;
    int64_t submitted_ = 0, running_ = 0, completed_ = 0, cancelled_ = 0, frame_steps_ = 0, admissions_ = 0;
    bool closing_ = false;
    int failed_ = 0;
    // live voices
    int live_voices_ = 0, max_voices_ = 0, v_running_ = 0;
    std::map<int64_t, VoiceEntry> voices_;  // every voice that has not been released
    std::deque<int64_t> vjobs_;             // Queued, in arrival order
    std::deque<int64_t> vreleases_;
    int64_t v_next_ = 0, v_created_ = 0, v_ready_ = 0, v_deferred_ = 0, v_anonymous_ = 0, steps_beside_ = 0;
    double fe_ms_sum_ = 0, burst_ms_beside_ = 0, burst_ms_alone_ = 0;
};

}  // namespace q3
