// session_queue_driver.cc -- csrc/session_queue.h alone, with several producers, one consumer and one canceller.
//
//   usage: session_queue_driver [producers] [per_producer] [max_pending]
//
// Producers submit (retrying on BUSY), then wait for every ticket they were given. The consumer plays the slot loop: it takes
// requests, completes them with two malloc'd buffers each, drops the running ones the canceller marked, and sleeps in
// wait_for_work() when nothing is pending. The canceller cancels every third ticket as soon as it exists. Checked, with a
// non-zero exit and a line on stderr when one fails:
//   1. tickets are dense and ordered      every ticket 0..N-1 is given out exactly once, a producer's tickets ascend
//   2. take order equals ticket order     the consumer sees strictly ascending tickets
//   3. a cancelled pending ticket is never handed out
//   4. every wait wakes                   every producer collects every one of its tickets (status OK or CANCELLED)
//   5. results are freed exactly once     buffers allocated == buffers freed (claimed ones by the producers, unclaimed ones by
//                                         the queue's destructor); the address sanitizer sees a double free or a leak
// Built with -fsanitize=address,undefined and with -fsanitize=thread by tests/test_session_host.py.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <thread>
#include <vector>

#include "session_queue.h"

namespace {
std::atomic<long> g_allocs{0}, g_frees{0};

void free_result(q3tts_result* r) {
    if (r->pcm) ++g_frees;
    if (r->codes) ++g_frees;
    std::free(r->pcm);
    std::free(r->codes);
    r->pcm = nullptr;
    r->codes = nullptr;
}

struct Req {
    int producer = -1, seq = -1;
};

int fail(const char* what) {
    std::fprintf(stderr, "session_queue_driver: %s\n", what);
    return 1;
}
}  // namespace

int main(int argc, char** argv) {
    const int P = argc > 1 ? std::atoi(argv[1]) : 4;
    const int K = argc > 2 ? std::atoi(argv[2]) : 200;
    const int max_pending = argc > 3 ? std::atoi(argv[3]) : 16;
    const int N = P * K;
    std::atomic<int> errors{0};
    std::atomic<long> submitted{0};
    {   // (3) on one thread, where "pending" is certain: of five waiting tickets, 1 and 3 are cancelled; 0, 2, 4 are handed out
        q3::SessionQueue<Req> q(0, &free_result);
        for (int i = 0; i < 5; ++i) {
            int64_t t = -1;
            Req r;
            r.producer = 0;
            r.seq = i;
            if (q.submit(std::move(r), &t) != Q3TTS_OK || t != i) return fail("tickets do not count from 0");
        }
        if (q.cancel(1) != Q3TTS_OK || q.cancel(3) != Q3TTS_OK || q.cancel(3) != Q3TTS_OK) return fail("cancel of a pending ticket");
        for (int64_t want : {0, 2, 4}) {
            int64_t t = -1;
            Req r;
            if (!q.take(&t, &r) || t != want || r.seq != want) return fail("a cancelled pending ticket was handed out");
        }
        int64_t t = -1;
        Req r;
        if (q.take(&t, &r)) return fail("more tickets than were submitted");
        q3tts_result res{};
        int32_t ready = 0;
        if (q.wait(1, 0, &res, &ready) != Q3TTS_OK || !ready || res.status != Q3TTS_ERR_CANCELLED) return fail("a cancelled ticket's result");
        if (q.wait(0, 0, &res, &ready) != Q3TTS_OK || ready) return fail("a running ticket was ready");
        q.close(false);  // 0, 2, 4 are running: marked, and dropped by the consumer
        std::vector<int64_t> marks;
        q.take_cancels(marks);
        if (marks.size() != 3) return fail("close without drain did not mark the running tickets");
        for (int64_t c : marks) q.complete_cancelled(c);
        if (q.wait_for_work()) return fail("a closed queue still had work");
        q3tts_session_stats s;
        q.stats(&s);
        if (s.cancelled != 5 || s.running != 0) return fail("the counters of the cancel prologue");
    }
    std::vector<std::vector<int64_t>> tickets((size_t)P);
    {
        q3::SessionQueue<Req> q(max_pending, &free_result);

        std::thread consumer([&] {
            int64_t last = -1;
            std::vector<int64_t> running, marks;
            for (;;) {
                int64_t t = -1;
                Req r;
                while (running.size() < 3 && q.take(&t, &r)) {
                    if (t <= last) ++errors;  // (2)
                    last = t;
                    if (r.producer < 0 || r.seq < 0) ++errors;  // the payload travels with its ticket
                    running.push_back(t);
                }
                q.take_cancels(marks);
                for (int64_t c : marks)
                    for (size_t i = 0; i < running.size(); ++i)
                        if (running[i] == c) {
                            q.complete_cancelled(c);
                            running.erase(running.begin() + (long)i);
                            break;
                        }
                if (!running.empty()) {  // the oldest running request finishes
                    const int64_t done = running.front();
                    running.erase(running.begin());
                    q3tts_result* res = q.result(done);
                    if (!res) {
                        ++errors;
                    } else {
                        res->pcm = static_cast<float*>(std::malloc(64));
                        res->codes = static_cast<int32_t*>(std::malloc(64));
                        g_allocs += 2;
                        res->n_frames = 1;
                        res->status = Q3TTS_OK;
                        q.complete(done);
                    }
                    q.progress(1, 1);
                    continue;
                }
                if (!q.wait_for_work()) break;
            }
        });

        std::thread canceller([&] {
            int64_t next = 0;
            while (next < N) {
                if (next >= submitted.load()) {
                    std::this_thread::yield();
                    continue;
                }
                if (q.cancel(next) != Q3TTS_OK) ++errors;
                if (q.cancel(next) != Q3TTS_OK) ++errors;  // twice is fine
                next += 3;
            }
            if (q.cancel(int64_t(N) + 5) != Q3TTS_ERR_INVALID_INPUT) ++errors;
            if (q.cancel(-1) != Q3TTS_ERR_INVALID_INPUT) ++errors;
        });

        std::vector<std::thread> producers;
        for (int p = 0; p < P; ++p)
            producers.emplace_back([&, p] {
                for (int k = 0; k < K; ++k) {
                    int64_t t = -1;
                    for (;;) {
                        Req r;
                        r.producer = p;
                        r.seq = k;
                        const int st = q.submit(std::move(r), &t);
                        if (st == Q3TTS_OK) break;
                        if (st != Q3TTS_ERR_BUSY) {
                            ++errors;
                            return;
                        }
                        std::this_thread::yield();
                    }
                    ++submitted;
                    if (!tickets[(size_t)p].empty() && t <= tickets[(size_t)p].back()) ++errors;  // (1) ascending per producer
                    tickets[(size_t)p].push_back(t);
                }
                // (4) all but the last ticket are collected; a timed wait that may come back empty is retried
                for (size_t i = 0; i + 1 < tickets[(size_t)p].size(); ++i) {
                    q3tts_result res{};
                    int32_t ready = 0;
                    while (!ready)
                        if (q.wait(tickets[(size_t)p][i], 50, &res, &ready) != Q3TTS_OK) {
                            ++errors;
                            break;
                        }
                    if (!ready) continue;
                    if (res.status == Q3TTS_OK) {
                        if (!res.pcm || !res.codes) ++errors;
                    } else if (res.status != Q3TTS_ERR_CANCELLED || res.pcm || res.codes) {
                        ++errors;  // (3) a cancelled ticket carries nothing
                    }
                    free_result(&res);
                    int32_t again = 0;
                    if (q.wait(tickets[(size_t)p][i], 0, &res, &again) != Q3TTS_ERR_INVALID_INPUT) ++errors;  // forgotten
                }
            });
        for (auto& t : producers) t.join();
        canceller.join();
        q.close(true);  // drain: the last tickets finish, then the consumer's wait_for_work() returns false
        consumer.join();
        int64_t t = -1;
        if (q.submit(Req{}, &t) != Q3TTS_ERR_INVALID_INPUT) ++errors;  // closed
        q3tts_session_stats s;
        q.stats(&s);
        if (s.submitted != N || s.pending != 0 || s.running != 0 || s.completed + s.cancelled != N) return fail("the counters do not add up");
        if (s.completed == 0) return fail("no ticket completed");  // (how many cancels came in time is up to the scheduler)
        // the P unclaimed tickets (each producer's last) stay with the queue: its destructor frees their buffers
    }
    std::set<int64_t> all;
    for (auto& v : tickets) all.insert(v.begin(), v.end());
    if ((int)all.size() != N || *all.begin() != 0 || *all.rbegin() != N - 1) return fail("tickets are not dense");  // (1)
    if (errors.load()) return fail("a property failed (see the numbered checks in the source)");
    if (g_allocs.load() != g_frees.load()) return fail("a result's buffers were not freed exactly once");  // (5)
    std::printf("ok tickets %d allocs %ld frees %ld\n", N, g_allocs.load(), g_frees.load());
    return 0;
}
