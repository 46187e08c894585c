// session_voice_driver.cc -- the live-voice bookkeeping of csrc/session_queue.h alone: voices that are named before they are
// ready, freed while they are in use, and abandoned by a close.
//
//   usage: session_voice_driver [producers] [per_producer] [live_voices] [max_voices]
//
// A prologue on one thread, where every state is certain, checks:
//   1. without voices, take order is ticket order
//   2. BUSY comes at the live_voices limit (waiting and running jobs count) and at the max_voices limit (a freed voice holds
//      its place until the consumer has released it)
//   3. a ticket is not handed out before its voice is Ready, and the tickets behind it are handed out meanwhile
//   4. a voice freed while a ticket uses it is released once, after that ticket completed; it can be named no more, and the
//      refused submit consumes no ticket
//   5. voice_wait: ready, timeout, freed, abandoned
//   6. close without drain abandons the waiting jobs and lets the launched one finish
// Then producers create voices (retrying on BUSY), submit tickets that name them at once, wait for half of the voices, free
// them at once and cancel some tickets, while one consumer launches the jobs on `live_voices` lanes, marks each voice ready a
// random number of rounds later, runs the tickets and releases what the queue hands it. Checked there: no ticket is taken
// before its voice is ready (3), every voice is released exactly once and never while the consumer runs a ticket of it (4),
// every wait wakes, the counters add up. A last round closes without drain under load and checks that every voice_wait
// wakes and that nothing leaks (the jobs own heap memory: the address sanitizer sees a leak).
// Built with -fsanitize=address,undefined and with -fsanitize=thread by tests/test_session_voices_host.py.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <thread>
#include <vector>

#include "session_queue.h"

namespace {
void free_result(q3tts_result* r) {
    std::free(r->pcm);
    std::free(r->codes);
    r->pcm = nullptr;
    r->codes = nullptr;
}

struct VoiceRec {  // the consumer's handle of a voice (the queue carries it as the tag)
    std::atomic<int> ready{0}, released{0}, running{0};
};
struct Req {
    VoiceRec* voice = nullptr;
    int seq = -1;
};
struct Job {
    std::vector<float> clip;  // heap memory that must go with the job, wherever it ends
};
using Queue = q3::SessionQueue<Req, Job>;

int fail(const char* what) {
    std::fprintf(stderr, "session_voice_driver: %s\n", what);
    return 1;
}
Job job() {
    Job j;
    j.clip.assign(256, 0.5f);
    return j;
}
int prologue() {
    {   // (1)
        Queue q(0, &free_result);
        for (int i = 0; i < 5; ++i) {
            int64_t t = -1;
            if (q.submit(Req{nullptr, i}, &t) != Q3TTS_OK || t != i) return fail("tickets do not count from 0");
        }
        for (int i = 0; i < 5; ++i) {
            int64_t t = -1;
            Req r;
            if (!q.take(&t, &r) || t != i || r.seq != i) return fail("take order is not ticket order");
            q.complete_cancelled(t);
        }
        int64_t v = -1;
        if (q.submit_voice(job(), nullptr, &v) != Q3TTS_ERR_INVALID_INPUT) return fail("a voice on a queue without live voices");
    }
    Queue q(0, &free_result);
    q.enable_voices(2, 3);
    VoiceRec rec[6];
    int64_t A = -1, B = -1, Cv = -1, D = -1, X = -1;
    std::vector<Queue::VoiceTake> jobs;
    std::vector<std::pair<int64_t, void*>> rel;
    q3tts_session_voice_stats vs;
    // (2)
    if (q.submit_voice(job(), &rec[0], &A) != Q3TTS_OK || q.submit_voice(job(), &rec[1], &B) != Q3TTS_OK) return fail("submit_voice");
    if (q.submit_voice(job(), &rec[2], &X) != Q3TTS_ERR_BUSY) return fail("no BUSY with live_voices jobs waiting");
    if (q.take_voice_jobs(jobs, 4) != 2 || jobs[0].id != A || jobs[1].id != B || jobs[0].tag != &rec[0] || jobs[0].job.clip.size() != 256)
        return fail("take_voice_jobs");
    if (q.submit_voice(job(), &rec[2], &X) != Q3TTS_ERR_BUSY) return fail("no BUSY with live_voices jobs running");
    q.voice_done(A, 1.5);
    if (q.submit_voice(job(), &rec[2], &Cv) != Q3TTS_OK) return fail("a finished job did not make room");
    q.voice_done(B, 2.5);
    if (q.take_voice_jobs(jobs, 4) != 1 || jobs[0].id != Cv) return fail("the third job");
    q.voice_done(Cv, 1.0);
    if (q.submit_voice(job(), &rec[3], &X) != Q3TTS_ERR_BUSY) return fail("no BUSY with max_voices alive");
    if (q.free_voice(A) != Q3TTS_OK || q.free_voice(A) != Q3TTS_ERR_INVALID_INPUT) return fail("free_voice");
    if (q.submit_voice(job(), &rec[3], &X) != Q3TTS_ERR_BUSY) return fail("a freed voice gave up its place before its release");
    q.voice_stats(&vs);
    if (vs.alive != 3 || vs.deferred_frees != 0 || vs.created != 3 || vs.ready != 3 || vs.frontend_ms_sum != 5.0) return fail("voice_stats");
    q.take_voice_releases(rel);
    if (rel.size() != 1 || rel[0].first != A || rel[0].second != &rec[0]) return fail("take_voice_releases");
    q.voice_released(A);
    q.take_voice_releases(rel);
    if (!rel.empty()) return fail("a voice was handed out for release twice");
    if (q.submit_voice(job(), &rec[3], &D) != Q3TTS_OK) return fail("a released voice did not make room");
    // (3) t0 names D (waiting), t1 is plain, t2 names B (ready)
    int64_t t0 = -1, t1 = -1, t2 = -1, t = -1;
    Req r;
    if (q.submit(Req{&rec[3], 0}, &t0, false, 0, 0, D) != Q3TTS_OK || q.submit(Req{nullptr, 1}, &t1) != Q3TTS_OK ||
        q.submit(Req{&rec[1], 2}, &t2, false, 0, 0, B) != Q3TTS_OK)
        return fail("submit with a voice");
    if (!q.take(&t, &r) || t != t1) return fail("the ticket behind a waiting voice was held back");
    if (!q.take(&t, &r) || t != t2) return fail("a ticket with a ready voice was held back");
    if (q.take(&t, &r)) return fail("a ticket was handed out before its voice was ready");
    // (4)
    if (q.free_voice(B) != Q3TTS_OK) return fail("free of a voice in use");
    q.voice_stats(&vs);
    if (vs.deferred_frees != 1) return fail("deferred_frees");
    q.take_voice_releases(rel);
    if (!rel.empty()) return fail("a voice in use was released");
    int64_t tx = -1;
    if (q.submit(Req{&rec[1], 3}, &tx, false, 0, 0, B) != Q3TTS_ERR_INVALID_INPUT) return fail("a freed voice was named");
    q.result(t2)->status = Q3TTS_OK;
    q.complete(t2);
    q.take_voice_releases(rel);
    if (rel.size() != 1 || rel[0].first != B) return fail("the last ticket's completion did not release the voice");
    q.voice_released(B);
    if (q.submit(Req{nullptr, 4}, &tx) != Q3TTS_OK || tx != 3) return fail("a refused submit consumed a ticket");
    // (5)
    int32_t ready = 0;
    if (q.voice_wait(Cv, 0, &ready) != Q3TTS_OK || !ready) return fail("voice_wait on a ready voice");
    if (q.voice_wait(D, 1, &ready) != Q3TTS_OK || ready) return fail("voice_wait on a waiting voice");
    if (q.voice_wait(A, 0, &ready) != Q3TTS_ERR_INVALID_INPUT) return fail("voice_wait on a released voice");
    // t0's voice becomes ready: it is handed out, in front of the later plain ticket
    if (q.take_voice_jobs(jobs, 4) != 1 || jobs[0].id != D) return fail("the fourth job");
    q.voice_done(D, 0.5);
    if (!q.take(&t, &r) || t != t0 || r.voice != &rec[3]) return fail("a ready voice's ticket was not handed out in ticket order");
    // (6) E is launched, F waits: close without drain abandons F alone
    int64_t E = -1, F = -1;
    if (q.free_voice(Cv) != Q3TTS_OK) return fail("free_voice");
    q.take_voice_releases(rel);
    q.voice_released(Cv);
    if (q.submit_voice(job(), &rec[4], &E) != Q3TTS_OK) return fail("submit_voice E");
    if (q.take_voice_jobs(jobs, 1) != 1) return fail("job E");
    if (q.submit_voice(job(), &rec[5], &F) != Q3TTS_OK) return fail("submit_voice F");
    q.close(false);
    if (q.voice_wait(F, -1, &ready) != Q3TTS_ERR_CANCELLED) return fail("an abandoned voice's wait");
    if (q.voice_state(E) != int(Queue::VoiceRunning)) return fail("close abandoned a launched job");
    q.voice_done(E, 0.5);
    if (q.voice_wait(E, -1, &ready) != Q3TTS_OK || !ready) return fail("a launched job did not finish behind close");
    if (q.submit_voice(job(), &rec[0], &X) != Q3TTS_ERR_INVALID_INPUT) return fail("a closing queue took a voice");
    std::vector<int64_t> marks;
    q.take_cancels(marks);
    for (int64_t c : marks) q.complete_cancelled(c);
    if (q.wait_for_work()) return fail("a closed queue still had work");
    if (q.free_voice(F) != Q3TTS_OK) return fail("an abandoned voice can be freed");
    std::vector<Queue::VoiceLeft> left;
    q.retire_voices(left);
    if (left.size() != 3) return fail("retire_voices");  // D and E alive, F freed and not yet released
    for (auto& l : left)
        if ((l.id == F) != l.freed || (l.id == F && l.state != int(Queue::VoiceAbandoned)) || (l.id != F && l.state != int(Queue::VoiceReady)))
            return fail("what retire_voices says of a voice");
    return 0;
}

struct Lane {
    int64_t id = -1;
    VoiceRec* rec = nullptr;
    int rounds = 0;
};

// One consumer over `lanes` lanes. Ends when wait_for_work() says so and no lane is busy.
void consume(Queue& q, int lanes, std::atomic<int>& errors, std::atomic<long>& released) {
    std::mt19937 rng(7);
    std::vector<Lane> lane((size_t)lanes);
    std::vector<Queue::VoiceTake> jobs;
    std::vector<std::pair<int64_t, void*>> rel;
    std::vector<std::pair<int64_t, VoiceRec*>> running;
    std::vector<int64_t> marks;
    auto done = [&](size_t i) {
        if (running[i].second) --running[i].second->running;
        running.erase(running.begin() + (long)i);
    };
    for (;;) {
        int busy = 0;
        for (Lane& l : lane) {  // poll
            if (l.id < 0) continue;
            if (--l.rounds > 0) {
                ++busy;
                continue;
            }
            l.rec->ready = 1;
            q.voice_done(l.id, 1.0);
            l.id = -1;
        }
        q.take_voice_releases(rel);
        for (auto& kv : rel) {
            VoiceRec* v = static_cast<VoiceRec*>(kv.second);
            if (v->released.fetch_add(1) != 0 || v->running.load() != 0) ++errors;  // once, and never under a running ticket
            q.voice_released(kv.first);
            ++released;
        }
        int free_lanes = 0;
        for (Lane& l : lane) free_lanes += l.id < 0;
        q.take_voice_jobs(jobs, free_lanes);
        for (auto& j : jobs)
            for (Lane& l : lane)
                if (l.id < 0) {
                    if (j.job.clip.size() != 256) ++errors;
                    l.id = j.id;
                    l.rec = static_cast<VoiceRec*>(j.tag);
                    l.rounds = 1 + int(rng() % 4);
                    ++busy;
                    break;
                }
        int64_t t = -1;
        Req r;
        while (running.size() < 3 && q.take(&t, &r)) {
            if (r.voice) {
                if (!r.voice->ready.load() || r.voice->released.load()) ++errors;  // never before Ready, never after its release
                ++r.voice->running;
            }
            running.emplace_back(t, r.voice);
        }
        q.take_cancels(marks);
        for (int64_t c : marks)
            for (size_t i = 0; i < running.size(); ++i)
                if (running[i].first == c) {
                    q.complete_cancelled(c);
                    done(i);
                    break;
                }
        if (!running.empty()) {
            q3tts_result* res = q.result(running.front().first);
            if (res) res->status = Q3TTS_OK;
            const int64_t id = running.front().first;
            done(0);  // (the device has finished with the voice before the ticket completes)
            q.complete(id);
            continue;
        }
        if (busy) {
            std::this_thread::yield();
            continue;
        }
        if (!q.wait_for_work()) break;
    }
}
}  // namespace

int main(int argc, char** argv) {
    const int P = argc > 1 ? std::atoi(argv[1]) : 4;
    const int K = argc > 2 ? std::atoi(argv[2]) : 100;
    const int live = argc > 3 ? std::atoi(argv[3]) : 2;
    const int max_voices = argc > 4 ? std::atoi(argv[4]) : 5;
    if (int rc = prologue()) return rc;
    std::atomic<int> errors{0};
    std::atomic<long> released{0}, busy_seen{0};
    {   // producers and one consumer; closed with drain
        Queue q(0, &free_result);
        q.enable_voices(live, max_voices);
        std::vector<std::unique_ptr<VoiceRec>> recs((size_t)(P * K));
        for (auto& p : recs) p = std::make_unique<VoiceRec>();
        std::thread consumer([&] { consume(q, live, errors, released); });
        std::vector<std::thread> producers;
        for (int p = 0; p < P; ++p)
            producers.emplace_back([&, p] {
                for (int k = 0; k < K; ++k) {
                    VoiceRec* rec = recs[(size_t)(p * K + k)].get();
                    int64_t v = -1;
                    for (;;) {
                        const int st = q.submit_voice(job(), rec, &v);
                        if (st == Q3TTS_OK) break;
                        if (st != Q3TTS_ERR_BUSY) {
                            ++errors;
                            return;
                        }
                        ++busy_seen;
                        std::this_thread::yield();
                    }
                    int64_t t[3] = {-1, -1, -1};
                    if (q.submit(Req{rec, 0}, &t[0], false, 0, 0, v) != Q3TTS_OK) ++errors;  // named before it is ready
                    if (q.submit(Req{nullptr, 1}, &t[1]) != Q3TTS_OK) ++errors;
                    if (q.submit(Req{rec, 2}, &t[2], false, 0, 0, v) != Q3TTS_OK) ++errors;
                    if (k % 2) {
                        int32_t ready = 0;
                        if (q.voice_wait(v, -1, &ready) != Q3TTS_OK || !ready) ++errors;
                    }
                    if (q.free_voice(v) != Q3TTS_OK) ++errors;  // at once: its tickets still complete
                    int64_t tx = -1;
                    if (q.submit(Req{rec, 3}, &tx, false, 0, 0, v) != Q3TTS_ERR_INVALID_INPUT) ++errors;
                    if (k % 3 == 0 && q.cancel(t[2]) != Q3TTS_OK) ++errors;
                    for (int i = 0; i < 3; ++i) {
                        q3tts_result res{};
                        int32_t ready = 0;
                        while (!ready)
                            if (q.wait(t[i], 50, &res, &ready) != Q3TTS_OK) {
                                ++errors;
                                break;
                            }
                        if (ready && res.status != Q3TTS_OK && !(i == 2 && k % 3 == 0 && res.status == Q3TTS_ERR_CANCELLED)) ++errors;
                    }
                }
            });
        for (auto& t : producers) t.join();
        q.close(true);
        consumer.join();
        std::vector<Queue::VoiceLeft> left;
        q.retire_voices(left);
        q3tts_session_voice_stats vs;
        q.voice_stats(&vs);
        if (!left.empty() || vs.alive != 0 || vs.in_flight != 0) return fail("voices were left behind a drained close");
        if (vs.created != P * K || released.load() != P * K) return fail("not every voice was released exactly once");
        for (auto& p : recs)
            if (p->released.load() != 1) return fail("a voice was not released exactly once");
        q3tts_session_stats s;
        q.stats(&s);
        if (s.submitted != 3L * P * K || s.pending != 0 || s.running != 0 || s.completed + s.cancelled != s.submitted) return fail("the counters do not add up");
    }
    for (int round = 0; round < 8; ++round) {  // close without drain under load: every waiter wakes, nothing leaks
        Queue q(0, &free_result);
        q.enable_voices(live, max_voices);
        std::vector<std::unique_ptr<VoiceRec>> recs((size_t)P);
        for (auto& p : recs) p = std::make_unique<VoiceRec>();
        std::atomic<long> rel2{0};
        std::atomic<int> started{0};
        std::thread consumer([&] { consume(q, live, errors, rel2); });
        std::vector<std::thread> waiters;
        for (int p = 0; p < P; ++p)
            waiters.emplace_back([&, p] {
                int64_t v = -1, t = -1;
                const int st = q.submit_voice(job(), recs[(size_t)p].get(), &v);
                ++started;
                if (st != Q3TTS_OK) return;  // BUSY, or closed already
                (void)q.submit(Req{recs[(size_t)p].get(), 0}, &t, false, 0, 0, v);
                int32_t ready = 0;
                const int w = q.voice_wait(v, -1, &ready);  // wakes: ready, or abandoned by the close
                if (!((w == Q3TTS_OK && ready) || w == Q3TTS_ERR_CANCELLED)) ++errors;
                if (t >= 0) {
                    q3tts_result res{};
                    if (q.wait(t, -1, &res, &ready) != Q3TTS_OK || !ready) ++errors;
                    if (w == Q3TTS_ERR_CANCELLED && res.status != Q3TTS_ERR_CANCELLED) ++errors;  // never ran on a lost voice
                }
            });
        while (started.load() < (round % 2 ? P : 1)) std::this_thread::yield();
        q.close(false);
        for (auto& t : waiters) t.join();
        consumer.join();
        std::vector<Queue::VoiceLeft> left;
        q.retire_voices(left);
        for (auto& l : left)
            if (l.freed || (l.state != int(Queue::VoiceReady) && l.state != int(Queue::VoiceAbandoned))) return fail("a voice behind a close without drain");
        q3tts_session_stats s;
        q.stats(&s);
        if (s.pending != 0 || s.running != 0 || s.completed + s.cancelled != s.submitted) return fail("the counters behind a close without drain");
    }
    if (errors.load()) return fail("a property failed (see the numbered checks in the source)");
    std::printf("ok voices %d released %ld busy %ld\n", P * K, released.load(), busy_seen.load());
    return 0;
}
