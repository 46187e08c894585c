// stream_plan.h -- which rows of a slotted codec stream decode which chunk in the next pass (codec.h, StreamCfg::per_row).
// Host arithmetic alone: no HIP include, so tests/native/stream_plan_driver.cc compiles it with a plain C++ compiler.
//
// Chunk k of a request with n frames covers frames [kC, min(n, (k+1)C)); its pre-transformer window is
// [max(0, kC - W), min(n, (k+1)C + L)); it is decodable once the request has (k+1)C + L frames or is final. Rows of a queue
// are admitted at different moments, so every row carries its own chunk index; a pass decodes one chunk for each row that has
// one and leaves the others alone.
//
// A voice-clone row carries a reference prefix of R frames in front of its generated ones (include/q3tts.h, "streamed clone
// rows"): its code row holds S = ref ++ gen. Prefix chunk j covers S[jC, min(R, (j+1)C)) with the window
// [max(0, jC - W), min(R, (j+1)C + L)) -- lookahead stops at R, so the prefix depends on nothing but the reference -- is
// decodable at once and emits nothing. Generated chunk k then covers S[R + kC, min(R + n, R + (k+1)C)) with the window
// [max(0, R + kC - W), min(R + n, R + (k+1)C + L)), which reaches back into the reference while kC < W. R = 0 is the above.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace q3 {

struct SlotPlanCfg {
    int rows = 0, chunk = 0, window = 0, lookahead = 0, max_frames = 0;
};

struct RowPlan {  // one row of one pass
    int part = 0;   // 1: the row decodes chunk k in this pass; 0: it is left alone (every length 0, not rolled)
    int k = 0;      // chunk index: among the generated chunks when emit, among the prefix chunks otherwise
    int emit = 1;   // 0: a chunk of the row's reference prefix, whose samples are never delivered
    // The frames below are positions in the row's code buffer, which holds the prefix in front of the generated frames.
    int f0 = 0;     // first frame of the chunk
    int w0 = 0;     // first frame of the pre-transformer window (the RVQ gather starts here)
    int wlen = 0;   // frames of the window: [w0, w0 + wlen)
    int take = 0;   // frames of the chunk: [f0, f0 + take), at offset f0 - w0 inside the window
};

class SlotPlanner {
  public:
    void open(const SlotPlanCfg& cfg) {
        cfg_ = cfg;
        next_.assign(size_t(cfg.rows), 0);
        live_.assign(size_t(cfg.rows), 0);
        prefix_.assign(size_t(cfg.rows), 0);
    }
    const SlotPlanCfg& cfg() const { return cfg_; }
    // a new request takes row b: its chunks count from 0 again. A row takes part in no pass before its first reset.
    // prefix > 0: the row's code buffer starts with that many reference frames, decoded first and never delivered.
    void reset_row(int b, int prefix = 0) {
        next_[size_t(b)] = 0;
        live_[size_t(b)] = 1;
        prefix_[size_t(b)] = std::max(0, prefix);
    }
    // the row's prefix has been decoded before and its state put back (codec.h, stream_load_row): straight to generated chunk 0
    void skip_prefix(int b) { next_[size_t(b)] = prefix_chunks(b); }
    int next_chunk(int b) const { return next_[size_t(b)]; }  // prefix chunks count as well
    int prefix_of(int b) const { return prefix_[size_t(b)]; }
    int prefix_chunks(int b) const { return chunks_of(prefix_[size_t(b)]); }
    bool in_prefix(int b) const { return live_[size_t(b)] && next_[size_t(b)] < prefix_chunks(b); }
    // chunks a request of n frames has
    int chunks_of(int n) const { return n <= 0 ? 0 : (n + cfg_.chunk - 1) / cfg_.chunk; }
    bool decodable(int b, int avail, bool fin) const {
        if (!live_[size_t(b)]) return false;
        if (in_prefix(b)) return true;  // the reference is there from the start
        const int f0 = (next_[size_t(b)] - prefix_chunks(b)) * cfg_.chunk;
        if (avail <= f0 || f0 >= cfg_.max_frames) return false;
        return fin || avail >= std::min(cfg_.max_frames, f0 + cfg_.chunk + cfg_.lookahead);
    }
    // The next pass over rows with avail[b] frames (fin[b]: the row gets no more). Returns the number of rows taking part
    // (0: nothing is decodable, `out` is all zeros) and moves those rows on to their next chunk.
    int plan_pass(const int* avail, const uint8_t* fin, std::vector<RowPlan>& out) {
        out.assign(size_t(cfg_.rows), RowPlan{});
        int parts = 0;
        for (int b = 0; b < cfg_.rows; ++b) {
            const int a = std::min(avail[b], cfg_.max_frames);
            if (!decodable(b, a, fin && fin[b])) continue;
            RowPlan& r = out[size_t(b)];
            const int R = prefix_[size_t(b)], P = prefix_chunks(b);
            r.part = 1;
            r.emit = next_[size_t(b)] >= P ? 1 : 0;
            r.k = r.emit ? next_[size_t(b)] - P : next_[size_t(b)];
            r.f0 = r.emit ? R + r.k * cfg_.chunk : r.k * cfg_.chunk;
            const int end = r.emit ? R + a : R;  // the frames the chunk and its lookahead may reach
            r.w0 = std::max(0, r.f0 - cfg_.window);
            r.wlen = std::min(end, r.f0 + cfg_.chunk + cfg_.lookahead) - r.w0;
            r.take = std::min(end, r.f0 + cfg_.chunk) - r.f0;
            ++next_[size_t(b)];
            ++parts;
        }
        return parts;
    }

  private:
    SlotPlanCfg cfg_;
    std::vector<int> next_, prefix_;
    std::vector<uint8_t> live_;
};

// The schedule of a queue without the talker (q3tts_debug_codec_stream_slots, the planner's test driver): requests take free
// slots in index order; every running request gains `burst` frames per step; one that reaches its count is final, is retired
// behind that step's push, and its slot is reset and refilled. admit(slot, request) is called when a request takes a slot,
// push(avail, fin, request_of_slot) once per step.
template <class Admit, class Push>
void replay_queue_schedule(const int32_t* counts, int n_reqs, int slots, int burst, Admit&& admit, Push&& push) {
    std::vector<int> req(size_t(slots), -1), avail(size_t(slots), 0);
    std::vector<uint8_t> fin(size_t(slots), 0);
    int next = 0;
    for (;;) {
        int running = 0;
        for (int s = 0; s < slots; ++s) {
            if (req[size_t(s)] < 0 && next < n_reqs) {
                req[size_t(s)] = next++;
                avail[size_t(s)] = 0;
                fin[size_t(s)] = 0;
                admit(s, req[size_t(s)]);
            }
            if (req[size_t(s)] >= 0) ++running;
        }
        if (running == 0) return;
        for (int s = 0; s < slots; ++s) {
            if (req[size_t(s)] < 0) continue;
            const int n = counts[req[size_t(s)]];
            avail[size_t(s)] = std::min(n, avail[size_t(s)] + burst);
            fin[size_t(s)] = avail[size_t(s)] >= n ? 1 : 0;
        }
        push(avail.data(), fin.data(), req.data());
        for (int s = 0; s < slots; ++s)
            if (req[size_t(s)] >= 0 && fin[size_t(s)]) {
                req[size_t(s)] = -1;
                avail[size_t(s)] = 0;  // an empty slot has no frames: it takes part in nothing until its next admission
                fin[size_t(s)] = 0;
            }
    }
}

}  // namespace q3
