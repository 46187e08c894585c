// session_text_driver.cc -- the open-text state of csrc/session_queue.h alone: several producers, one consumer, one canceller.
//
//   usage: session_text_driver [producers] [per_producer] [max_pending]
//
// First, on one thread, where every state is certain: text appended before take comes out with the request (in order, with its
// close); text appended after take goes through the mailbox; every refusal (unknown ticket, plain ticket, closed text, n < 0,
// more than the capacity) changes nothing; an append for a done or collected ticket is accepted and dropped; close(drain)
// closes the open texts; a consumer that waits with only starved rows is woken by an append, a cancel and close.
// Then with threads: every producer submits open-text tickets and feeds them in pieces while the consumer -- the slot loop in
// small: three slots, rows that wait for text, wait_for_text() when all of them do -- takes them, so that appends land before
// and after take at random; a canceller cancels every fifth ticket while its text is still arriving. Checked, with a non-zero
// exit and a line on stderr when one fails:
//   1. no append is refused or lost       every append of the producers returns OK, and a ticket that completes has received
//                                         exactly its text, in order, whichever way each piece took
//   2. every wait wakes                   the consumer never sleeps through an append, a cancel or close; every producer collects
//                                         every one of its tickets (status OK or CANCELLED)
//   3. results are freed exactly once     as session_queue_driver.cc
// Built with -fsanitize=address,undefined and with -fsanitize=thread by tests/test_session_open_text_host.py.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
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
    int producer = -1, seq = -1, total = 0;  // total: content tokens of the whole text (the first one is in the request)
};
using Queue = q3::SessionQueue<Req>;

int32_t token(int seq, int j) { return int32_t(seq * 64 + j); }
int total_of(int seq) { return 1 + seq % 9; }

int fail(const char* what) {
    std::fprintf(stderr, "session_text_driver: %s\n", what);
    return 1;
}

#define EXPECT(c)                    \
    do {                             \
        if (!(c)) return fail(#c);   \
    } while (0)

int single_thread() {
    const int32_t ids[6] = {11, 12, 13, 14, 15, 16};
    q3tts_session_text_stats ts{};
    {   // before take, after take, refusals
        Queue q(0, &free_result);
        int64_t plain = -1, a = -1, b = -1;
        EXPECT(q.submit(Req{}, &plain) == Q3TTS_OK && plain == 0);
        EXPECT(q.submit(Req{}, &a, true, 1, 6) == Q3TTS_OK && a == 1);
        EXPECT(q.submit(Req{}, &b, true, 1, 6) == Q3TTS_OK && b == 2);
        std::string why;
        EXPECT(q.append_text(7, ids, 1, false, &why) == Q3TTS_ERR_INVALID_INPUT && !why.empty());
        EXPECT(q.append_text(-1, ids, 1, false) == Q3TTS_ERR_INVALID_INPUT);
        EXPECT(q.append_text(plain, ids, 1, false) == Q3TTS_ERR_INVALID_INPUT);
        EXPECT(q.append_text(a, ids, -1, false) == Q3TTS_ERR_INVALID_INPUT);
        EXPECT(q.append_text(a, ids, 6, false) == Q3TTS_ERR_INVALID_INPUT);  // 1 + 6 > 6
        q.text_stats(&ts);
        EXPECT(ts.open == 2 && ts.appended_tokens == 0);
        EXPECT(q.append_text(a, ids, 3, false) == Q3TTS_OK);
        EXPECT(q.append_text(a, nullptr, 0, false) == Q3TTS_OK);
        EXPECT(q.append_text(a, ids + 3, 2, true) == Q3TTS_OK);  // exactly full, and closed
        EXPECT(q.append_text(a, ids, 1, false) == Q3TTS_ERR_INVALID_INPUT);
        EXPECT(q.append_text(a, nullptr, 0, true) == Q3TTS_ERR_INVALID_INPUT);
        EXPECT(!q.has_appends());
        q.text_stats(&ts);
        EXPECT(ts.open == 1 && ts.appended_tokens == 5);
        int64_t t = -1;
        Req r;
        Queue::TextTake tt;
        EXPECT(q.take(&t, &r, &tt) && t == plain && !tt.open && tt.early.empty());
        EXPECT(q.take(&t, &r, &tt) && t == a && tt.open && tt.closed);
        EXPECT(tt.early == std::vector<int32_t>(ids, ids + 5));
        EXPECT(q.take(&t, &r, &tt) && t == b && tt.open && !tt.closed && tt.early.empty());
        EXPECT(q.append_text(b, ids, 2, false) == Q3TTS_OK);  // running: the mailbox
        EXPECT(q.append_text(b, nullptr, 0, false) == Q3TTS_OK && q.append_text(b, ids + 2, 1, false) == Q3TTS_OK);
        EXPECT(q.append_text(b, ids, 3, false) == Q3TTS_ERR_INVALID_INPUT);  // 4 + 3 > 6, nothing changed
        EXPECT(q.has_appends());
        std::vector<Queue::TextMsg> msgs;
        q.take_appends(msgs);
        EXPECT(msgs.size() == 2 && msgs[0].ticket == b && msgs[0].ids == std::vector<int32_t>(ids, ids + 2) && !msgs[0].final);
        EXPECT(msgs[1].ids == std::vector<int32_t>(ids + 2, ids + 3) && !q.has_appends());
        // done, then collected: accepted and dropped
        q.result(b)->status = Q3TTS_OK;
        q.complete(b);
        EXPECT(q.append_text(b, ids, 1, false) == Q3TTS_OK && !q.has_appends());
        q3tts_result res{};
        int32_t ready = 0;
        EXPECT(q.wait(b, 0, &res, &ready) == Q3TTS_OK && ready == 1);
        EXPECT(q.append_text(b, ids, 1, true) == Q3TTS_OK && !q.has_appends());
        q.text_stats(&ts);
        EXPECT(ts.open == 0 && ts.appended_tokens == 8);
        q.text_progress(2, 1);
        q.text_progress(1, 2);
        q.text_stats(&ts);
        EXPECT(ts.starved == 1 && ts.starve_events == 3);
    }
    {   // close(drain): a pending and a running open ticket both end as if `final` had been sent; a cancelled one is left alone
        Queue q(0, &free_result);
        int64_t run = -1, pend = -1, gone = -1, t = -1;
        Req r;
        Queue::TextTake tt;
        EXPECT(q.submit(Req{}, &run, true, 1, 8) == Q3TTS_OK && q.take(&t, &r, &tt) && t == run);
        EXPECT(q.submit(Req{}, &pend, true, 1, 8) == Q3TTS_OK && q.submit(Req{}, &gone, true, 1, 8) == Q3TTS_OK);
        EXPECT(q.cancel(gone) == Q3TTS_OK);
        q.close(true);
        EXPECT(q.append_text(run, ids, 1, false) == Q3TTS_ERR_INVALID_INPUT && q.append_text(pend, ids, 1, false) == Q3TTS_ERR_INVALID_INPUT);
        EXPECT(q.append_text(gone, ids, 1, false) == Q3TTS_OK);
        std::vector<Queue::TextMsg> msgs;
        q.take_appends(msgs);
        EXPECT(msgs.size() == 1 && msgs[0].ticket == run && msgs[0].final && msgs[0].ids.empty());
        EXPECT(q.take(&t, &r, &tt) && t == pend && tt.open && tt.closed);
        q.wait_for_text(false);  // the first look after close returns at once ...
        q.complete_cancelled(run);
        q.complete_cancelled(pend);
    }
    {   // a consumer that waits with only starved rows: an append, a cancel and close each wake it
        Queue q(0, &free_result);
        int64_t a = -1, t = -1;
        Req r;
        EXPECT(q.submit(Req{}, &a, true, 1, 8) == Q3TTS_OK && q.take(&t, &r));
        for (int round = 0; round < 3; ++round) {
            std::atomic<int> woke{0};
            std::thread consumer([&] {
                q.wait_for_text(false);
                woke = 1;
            });
            if (round == 0) {
                if (q.append_text(a, ids, 1, false) != Q3TTS_OK) return fail("append refused");
            } else if (round == 1) {
                if (q.cancel(a) != Q3TTS_OK) return fail("cancel refused");
            } else {
                q.close(false);
            }
            consumer.join();
            EXPECT(woke == 1);
            std::vector<Queue::TextMsg> msgs;
            std::vector<int64_t> cancels;
            q.take_appends(msgs);
            q.take_cancels(cancels);
            EXPECT(round != 0 || msgs.size() == 1);
            EXPECT(round != 1 || (cancels.size() == 1 && cancels[0] == a));
        }
        q.complete_cancelled(a);
    }
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    const int P = argc > 1 ? std::atoi(argv[1]) : 4;
    const int K = argc > 2 ? std::atoi(argv[2]) : 100;
    const int max_pending = argc > 3 ? std::atoi(argv[3]) : 16;
    const int N = P * K, S = 3;
    if (single_thread()) return 1;

    std::atomic<int> errors{0};
    std::atomic<long> submitted{0}, dropped{0}, completed_ok{0};
    {
        Queue q(max_pending, &free_result);
        std::thread consumer([&] {
            struct Row {
                Req req;
                std::vector<int32_t> ids;
                bool closed = false;
            };
            std::map<int64_t, Row> rows;
            std::vector<int64_t> cancels;
            std::vector<Queue::TextMsg> msgs;
            for (;;) {
                q.take_cancels(cancels);
                for (int64_t t : cancels)
                    if (rows.erase(t)) q.complete_cancelled(t);
                while (int(rows.size()) < S) {
                    int64_t t = -1;
                    Row row;
                    Queue::TextTake tt;
                    if (!q.take(&t, &row.req, &tt)) break;
                    if (!tt.open) ++errors;
                    row.ids = std::move(tt.early);
                    row.closed = tt.closed;
                    rows[t] = std::move(row);
                }
                q.take_appends(msgs);
                for (auto& m : msgs) {
                    auto it = rows.find(m.ticket);
                    if (it == rows.end()) {  // cancelled meanwhile
                        ++dropped;
                        continue;
                    }
                    if (it->second.closed) ++errors;  // nothing may follow a close
                    it->second.ids.insert(it->second.ids.end(), m.ids.begin(), m.ids.end());
                    it->second.closed = m.final;
                }
                bool any = false;
                for (auto it = rows.begin(); it != rows.end();) {
                    if (!it->second.closed) {
                        ++it;
                        continue;
                    }
                    const Row& row = it->second;  // (1) exactly its text, in order
                    bool good = int(row.ids.size()) == row.req.total - 1;
                    for (int j = 0; good && j < int(row.ids.size()); ++j) good = row.ids[size_t(j)] == token(row.req.seq, j + 1);
                    if (!good) ++errors;
                    q3tts_result* res = q.result(it->first);
                    if (res) {
                        res->status = Q3TTS_OK;
                        res->codes = static_cast<int32_t*>(std::malloc(16));
                        res->pcm = static_cast<float*>(std::malloc(16));
                        g_allocs += 2;
                    }
                    q.complete(it->first);
                    ++completed_ok;
                    it = rows.erase(it);
                    any = true;
                }
                q.text_progress(int(rows.size()), 0);
                if (any) continue;
                if (rows.empty()) {
                    if (!q.wait_for_work()) break;
                    continue;
                }
                q.wait_for_text(int(rows.size()) < S);  // every row waits for text
            }
        });
        std::thread canceller([&] {
            for (int64_t t = 2; t < N; t += 5) {
                while (submitted.load() <= t) std::this_thread::yield();
                if (q.cancel(t) != Q3TTS_OK) ++errors;
            }
        });
        std::vector<std::thread> producers;
        for (int p = 0; p < P; ++p)
            producers.emplace_back([&, p] {
                std::vector<int64_t> mine;
                for (int k = 0; k < K; ++k) {
                    const int seq = p * K + k, total = total_of(seq);
                    Req r;
                    r.producer = p;
                    r.seq = seq;
                    r.total = total;
                    int64_t t = -1;
                    for (;;) {
                        const int st = q.submit(Req(r), &t, true, 1, 16);
                        if (st == Q3TTS_OK) break;
                        if (st != Q3TTS_ERR_BUSY) {
                            ++errors;
                            return;
                        }
                        std::this_thread::yield();
                    }
                    ++submitted;
                    if (!mine.empty() && t <= mine.back()) ++errors;
                    mine.push_back(t);
                    // its text in pieces of 1..3 tokens, the last one final (a one-token text: an empty final append)
                    for (int j = 1; j < total || total == 1;) {
                        const int n = total == 1 ? 0 : std::min(1 + (seq + j) % 3, total - j);
                        int32_t piece[3];
                        for (int i = 0; i < n; ++i) piece[i] = token(seq, j + i);
                        const bool final_piece = j + n >= total;
                        if (q.append_text(t, piece, n, final_piece) != Q3TTS_OK) ++errors;  // (1): never refused, cancelled or not
                        j += n;
                        if (final_piece) break;
                    }
                }
                for (int64_t t : mine) {  // (2)
                    q3tts_result res{};
                    int32_t ready = 0;
                    if (q.wait(t, 60000, &res, &ready) != Q3TTS_OK || !ready) {
                        ++errors;
                        continue;
                    }
                    if (res.status != Q3TTS_OK && res.status != Q3TTS_ERR_CANCELLED) ++errors;
                    free_result(&res);
                }
            });
        for (auto& t : producers) t.join();
        canceller.join();
        q.close(true);
        consumer.join();
        q3tts_session_text_stats ts{};
        q.text_stats(&ts);
        if (ts.open != 0) ++errors;
    }
    if (errors.load()) return fail("a check failed in the threaded run");
    if (g_allocs.load() != g_frees.load()) return fail("results were not freed exactly once");
    std::printf("ok tickets=%d completed=%ld dropped_appends=%ld\n", N, completed_ok.load(), dropped.load());
    return 0;
}
