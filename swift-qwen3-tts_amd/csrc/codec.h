// codec.h -- neural codec decoder runner (codes -> PCM at 24 kHz or at the handle's output rate) on the HIP kernels in
// kernels/codec_conv.hip, kernels/codec_misc.hip, kernels/stretch.hip, kernels/resample.hip, kernels/resample_ratio.hip and
// kernels/formant.hip. Mirrors Qwen3TTSSpeechTokenizerDecoder
// (/root/reference/Sources/Qwen3TTS/Models/SpeechTokenizer.swift:754-784).
#pragma once
#include <string>
#include <vector>

#include "formant_plan.h"
#include "model.h"
#include "pitch_plan.h"
#include "request_speed_plan.h"
#include "resample_plan.h"
#include "stream_plan.h"
#include "stretch_plan.h"

namespace q3 {

class CodecRunner {
  public:
    // output_rate: 0 or 24000 -- the decoder's own rate, nothing is added to the tail. Another supported rate
    // (resample_plan.h): out_conv writes the 24 kHz signal into one more tail tensor and the causal polyphase FIR behind it
    // writes the PCM, `upsample()` samples per frame at that rate. Being one more causal conv of the tail, the stage carries
    // its history from chunk to chunk like the others: every statement below about samples, strides and bit-identity holds
    // with upsample() counting output samples.
    // speed: 0 or 1 -- off, nothing is added. Otherwise (0.5 .. 2; stretch_plan.h chooses the synthesis hop Hs, the one nearest
    // to 480 / speed that leaves whole samples per frame at the output rate) the time stretch sits behind out_conv and in front
    // of the resampler: one more causal stage, 4 Hs samples per frame, whose state besides its input's margin is one word per
    // row (d of the last hop). In a stream the word lives in a tail tensor of its own, one 16-byte entry per frame, so whatever
    // rolls, zeroes, saves or restores margins carries it like any other history; decode_chunked, which recomputes its left
    // context, cannot recompute the word and carries it (and the resampler's input margin) from chunk to chunk.
    // request_speeds: rows of one decode() may speak at speeds of their own (request_speed_plan.h). The fade tables of every
    // hop go to the device here, once; a decode without a hop table is the handle's own, untouched.
    // pitch: 0 -- off, nothing is added. Otherwise semitones in [-12, 12] (pitch_plan.h): with Ho the hop the handle would have
    // had (480, or the speed's) and Hp the integer nearest to Ho * 2^(pitch / 12), the stretch runs at Hs = Hp (no stretch stage
    // when Hp == 480) and ONE resampler behind it, Hp * M -> Ho * L on kernels/resample_ratio.hip, does pitch and output rate
    // together: the same pair of stages as a speed with an output rate, so every statement above holds with mid samples per
    // frame 4 Hp and upsample() that of the handle without a pitch. Hp == Ho is off. Not together with request_speeds.
    // keep_formants (formant_plan.h; kernels/formant.hip): on a pitched handle at 24 kHz the tail becomes out_conv -> stretch
    // (if Hp != 480) -> analyse / whiten -> the resampler, unclamped, into a tail tensor -> synthesise + clip -> PCM. Four more
    // tail tensors: the whitened signal e (4 Hp floats per frame, with a margin: the FIR reads back into it), the coefficients
    // (hops * P floats per frame), the unclipped e' (a frame of output samples) and the synthesis filter's state, one entry
    // of P floats per frame with a margin, carried like the stretch's word. A saved prefix state grows by the two margins:
    // hist_frames() * (align16(4 Hp * 4) + align16(P * 4)) bytes. Without a pitch (or Hp == Ho) the option adds nothing.
    // decode_chunked is refused on such a handle: its recomputed context cannot recompute the filter's state.
    CodecRunner(const Model& m, hipStream_t st, bool fp32_convs = false, int output_rate = 0, float speed = 0.0f,
                bool request_speeds = false, float pitch = 0.0f, bool keep_formants = false);
    // codes_dev: [B][code_stride_frames][16] int32 on the device; rows decode frames[b] frames.
    // pcm_dev receives [B][Fmax*upsample] float32 (Fmax = max(frames)); returns Fmax.
    // If `stage` is non-empty the activation after that stage is copied to stage_out ([B][T][C]).
    // nonfinite_host (pinned, one int per row, optional): set to 1 behind the decode for rows whose waveform came out
    // non-finite -- with the default fp16 two-plane convs that is what an activation beyond 65504 turns into (codec_conv.hip);
    // the fp32 matrix-core path (q3tts_load_opts.codec_fp32) has the reference's range.
    // force_fp32: this call contracts on the fp32 matrix cores whatever the runner's default (the engine re-decodes rows
    // that left the fp16 range this way, so that a checkpoint with large activations still gets the reference's waveform).
    // row_hs (host [B], a handle with request_speeds; nullptr: every row at the handle's speed, the layout above): row b's
    // synthesis hop (480: no stretch for that row). pcm_dev then receives [B][Fmax * max_upsample()], row b's
    // frames[b] * upsample_of(row_hs[b]) samples packed at the start of its part; the arithmetic of a row is that of a handle
    // loaded with the row's speed, bit for bit.
    int decode(const int32_t* codes_dev, int code_stride_frames, const std::vector<int>& frames, float** pcm_dev,
               const std::string& stage = std::string(), std::vector<float>* stage_out = nullptr, int* stage_T = nullptr,
               int* stage_C = nullptr, int32_t* nonfinite_host = nullptr, bool force_fp32 = false, const int* row_hs = nullptr);
    bool fp32_convs() const { return fp32_mfma_; }
    // The same decode with the causal tail (everything behind the pre-transformer) evaluated `chunk_frames` frames at a
    // time (row f1 of SURVEY 8f): each chunk's samples land in pcm_host ([B][Fmax * upsample], pinned host memory) at
    // their final place and chunk_done[k] is recorded behind chunk k's copy. Bit-identical to decode(). Returns the
    // number of chunks; chunk k covers frames [k * chunk_frames, min(Fmax, (k + 1) * chunk_frames)).
    int decode_chunked(const int32_t* codes_dev, int code_stride_frames, const std::vector<int>& frames, int chunk_frames,
                       float* pcm_host, std::vector<hipEvent_t>& chunk_done, int32_t* nonfinite_host = nullptr,
                       int32_t* nf_chunks_host = nullptr);  // (per-chunk flags as in stream_push)
    int tail_context_frames() const;
    static void set_scratch_budget(size_t bytes);  // test hook: forces the row-group paths of decode / decode_chunked (0: default)

    // ---- streamed decode (row f1: audio while tokens are still being generated) -------------------------------------
    // The causal tail keeps its own state between chunks: every tensor a causal conv reads lives in a persistent buffer
    // with `hist_frames()` frames of margin in front, into which the last frames of a chunk are rolled, so chunk k + 1
    // reads exactly the rows the one-shot decode would -- nothing is recomputed and the tail is bit-identical to decode().
    // The pre-transformer is bidirectional over the whole utterance in the reference (SpeechTokenizer.swift:763); a stream
    // cannot wait for the end, so chunk [f0, f1) is computed from a window of frames [f0 - window, f1 + lookahead) (what
    // exists of it): an approximation whose distance from the one-shot decode tests/test_streaming.py measures and bounds.
    // window < 0: the pre-transformer runs ONCE over all frames (needs every code up front; exact, for tests and offline use).
    struct StreamCfg {
        int rows = 0, chunk_frames = 0, window = 0, lookahead = 0, max_frames = 0;
        bool per_row = false;  // a slotted stream (below): rows are slots of a queue, each at a chunk phase of its own
        int max_prefix = 0;    // slotted stream: the longest reference prefix a row may be reset with (code rows hold prefix ++ frames)
    };
    void stream_open(const StreamCfg& cfg);
    // Rows have avail[b] frames so far (final[b]: the row will get no more). Decodes every chunk that has become decodable;
    // chunk k's samples go to pcm_host + b * pcm_row_stride + k * chunk_frames * upsample() and chunk_done[k] is recorded
    // behind the copy (events are created as needed). Returns the number of chunks issued so far. codes: device
    // [rows][code_stride_frames][16], frames below avail[b] final. No host synchronisation.
    // nf_chunks_host (pinned, optional): [chunk][rows] -- the rows' non-finite flags as they stand behind chunk k, copied in
    // front of chunk_done[k], so that a caller can hold a row's pieces back from the first chunk that left the fp16 range.
    int stream_push(const int32_t* codes_dev, int code_stride_frames, const int* avail, const uint8_t* final_rows, float* pcm_host,
                    size_t pcm_row_stride, std::vector<hipEvent_t>& chunk_done, int32_t* nf_chunks_host = nullptr);
    void stream_close(int32_t* nonfinite_host = nullptr);
    // ---- slotted stream (StreamCfg::per_row; window >= 0): the rows are the slots of a continuous-batching queue ------------
    // Requests enter and leave rows at different moments, so every row has its own next chunk (stream_plan.h decides who
    // decodes what); a pass decodes one chunk for each row that has one and leaves the others alone: length 0 in every
    // kernel, margins not rolled, nothing of theirs written. A row's result is what a lock-step stream over that row alone
    // produces, bit for bit. The samples of a pass go to a pinned ring slot [rows][chunk_frames * upsample] with the rows'
    // non-finite flags as they stand behind the pass and an event behind both; the caller scatters them and gives the slot back.
    struct SlotPass {
        int ring = -1;                // ring slot, to be handed to stream_release once the samples have been taken
        hipEvent_t begun = nullptr, done = nullptr;  // in front of the pass / behind its copies to the host (timing enabled)
        const float* pcm = nullptr;   // [rows][chunk_frames * upsample], valid behind `done`
        const int32_t* nf = nullptr;  // [rows]
        std::vector<RowPlan> rows;    // who took part, with which chunk
    };
    // A new request takes row b: its chunks count from 0, its history margins in every tensor with history and its non-finite
    // flag are cleared ON THE CODEC STREAM -- behind the previous occupant's last chunk (issued by an earlier push), in front of
    // the new occupant's first. A row takes part in no pass before its first reset.
    // prefix > 0 (a streamed voice-clone row, include/q3tts.h): the row's code row starts with that many reference frames. They
    // are decoded first, chunk by chunk like any others and with the lookahead stopping at the reference's end, and carry the
    // tail's state into the first generated chunk; their samples are delivered nowhere (RowPlan::emit == 0) and a pass in
    // which no row emits takes no ring slot and is not appended to stream_push_rows' `out`.
    void stream_reset_row(int b, int prefix = 0);
    // Request speeds in a slotted stream (a handle with request_speeds and no output rate: stream_own_hops()): every row has a
    // synthesis hop of its own, the handle's until stream_set_row_hs says otherwise -- called for a new occupant in front of its
    // reset / load; it holds for the passes issued from then on. The tensors with history in front of the stretch (out_conv's
    // signal, the state words) have the decoder's own frame size whatever the hop, so margins roll, zero, save and restore as
    // they did; the PCM behind the stretch carries no margin and has frames of the slowest row's size (stream_upsample()), a
    // row's take * upsample_of(hs) samples packed at the start of its part of a ring slot. A saved state is valid for the hop it
    // was made with (the state word is that hop's).
    bool stream_own_hops() const { return rs_ && !resample_; }
    int stream_upsample() const { return stream_own_hops() ? rs_plan_.max_spf() : up_; }
    void stream_set_row_hs(int b, int hs);
    // The state a row's occupant has left in the tail -- its margins in every tensor with history -- as one blob of
    // stream_state_bytes() bytes of device memory (16-byte aligned), saved or restored with one launch on the codec stream.
    // A row whose prefix has been decoded (stream_in_prefix(b) false after the pushes that decoded it) saved into a blob, and a
    // later row -- of any index, in any slotted stream of the same chunk / window / lookahead and codec path -- reset by
    // stream_load_row with the same prefix continue identically, bit for bit: the prefix passes are skipped.
    size_t stream_state_bytes() const { return stream_.state_bytes; }
    bool stream_in_prefix(int b) const { return stream_.plan.in_prefix(b); }
    void stream_save_row(int b, uint8_t* blob_dev);
    // row b's non-finite flag as it stands on the codec stream, to pinned host memory (a prefix that raised it is not worth keeping)
    void stream_row_flag(int b, int32_t* flag_host);
    // which kernels the tail of a stream runs on: 0 two-plane fp16, 1 the float16 MainDecoder, 2 the fp32 matrix cores
    int stream_path() const { return fp32_mfma_ ? 2 : (m_.codec.f16_main && !no_h1_ ? 1 : 0); }
    void stream_load_row(int b, int prefix, const uint8_t* blob_dev);
    // Rows have avail[b] frames of their current request in codes_dev [rows][code_stride_frames][16] (final_rows[b]: no more
    // will come). Issues passes until no row has a decodable chunk (returns false) or the ring is full (returns true: take a
    // pass, release it, push again). Issued passes are appended to `out`, oldest first. No host synchronisation.
    bool stream_push_rows(const int32_t* codes_dev, int code_stride_frames, const int* avail, const uint8_t* final_rows,
                          std::vector<SlotPass>& out);
    void stream_release(int ring);
    int stream_chunks_of(int frames) const { return stream_.plan.chunks_of(frames); }
    static constexpr int kRingSlots = 8;
    static constexpr int kQuietSlots = 8;
    bool streaming() const { return stream_.open; }
    int hist_frames() const;
    int upsample() const { return up_; }            // PCM samples per frame at the output rate
    int native_upsample() const { return native_; }  // the decoder's own samples per frame (1920)
    // request speeds (request_speed_plan.h): whether rows may have hops of their own, the plan, a hop's samples per frame and
    // the slowest row's, which sizes what holds rows of mixed speeds
    bool request_speeds() const { return rs_; }
    const RequestSpeedPlan& speed_plan() const { return rs_plan_; }
    int upsample_of(int hs) const { return rs_plan_.spf(hs); }
    int max_upsample() const { return rs_ ? rs_plan_.max_spf() : up_; }
    int output_rate() const { return out_rate_; }  // (a pitched handle resamples whatever its rate: resample_ does not tell)
    // the speaking rate of this handle: its hop Ho (480: off; on a pitched handle the stretch itself runs at pitch_hp()),
    // effective speed 480 / Ho, the stretch stage's delay D in 24 kHz samples
    int stretch_hs() const { return ho_; }
    int stretch_delay_samples() const { return stretch_ ? st_plan_.delay : 0; }
    // the pitch of this handle (pitch_plan.h): the hop in front of the resampler (== stretch_hs(): off), the delay of the
    // stretch and the FIR together in output samples
    int pitch_hp() const { return pitched_ ? pitch_hp_ : ho_; }
    int pitch_delay_out_samples() const { return pitch_delay_; }
    bool keep_formants() const { return formant_; }  // the formant stage runs (the option on a handle whose pitch is on)
    hipStream_t stream() const { return st_; }
    void set_stream(hipStream_t st) { st_ = st; }  // the caller drains the old stream first (shared scratch)

  private:
    struct Pass {  // one pass of kernels over `nb` rows
        int nb = 0;
        int row0 = 0;         // first row of this pass in the call's batch (non-finite flags)
        int hist_frames = 0;  // streamed decode: tensors carry this many frames of history in front of their first row
        const int32_t* fr = nullptr;  // device: valid frames per row
        // decode_chunked with a time stretch: the first ctx_frames frames of every row are recomputed context. The stages with
        // carried state run on the fr_new[b] frames behind them alone, the context supplying their input's history.
        int ctx_frames = 0;
        const int32_t* fr_new = nullptr;  // device: new frames per row
        int32_t* carry = nullptr;         // device [nb]: the stretch's state word per row, read and written
        float* mid_carry = nullptr;       // the resampler's input: [nb][mid_stride], one frame of margin in front of the new frames
        int64_t mid_stride = 0;
        // rows with hops of their own (decode with row_hs): device [nb] hop per row, 0 for a row without a stretch, and
        // [nb] samples per frame in front of the resampler; every tensor behind the stretch then has max-sized frames
        bool own_hops = false;  // (set without the tables in stream_open's counting pass)
        const int32_t* hs_rows = nullptr;
        const int32_t* mid_rows = nullptr;
        const std::string* stage = nullptr;
        std::vector<float>* stage_out = nullptr;
        int* stage_T = nullptr;
        int* stage_C = nullptr;
    };
    // Every launch of the tail goes through here: the counting pass of stream_open (stream_.dry) walks the tail for its
    // tensors alone, so nothing inside `f` is evaluated then -- neither the launch nor the addresses it is given.
    template <class F>
    void launch(F&& f) {
        if (!stream_.dry) f();
    }
    void conv(const Pass& ps, const struct ConvW& cw, const float* x, int Tmax, int ppf, float* out, const struct SnakeW* sn,
              const float* res, int act, const struct SnakeW* post = nullptr, float* out2 = nullptr);
    // the same on the float16 tensors of a float16 speech tokenizer's MainDecoder (codec_conv_h1.hip); x: float16, or fp32 when x_f32
    void conv_h1(const Pass& ps, const struct ConvW& cw, const void* x, bool x_f32, int Tmax, int ppf, uint16_t* out, const uint16_t* res,
                 const struct SnakeW* post, uint16_t* out2);
    // one DecoderResidualUnit of a narrow block in one launch, when fused_block() says so; out2: the next block's SnakeBeta copy
    bool fused_block(const CodecW::Block& Bk, float) const;
    bool fused_block(const CodecW::Block& Bk, uint16_t) const;
    void resunit(const Pass& ps, const CodecW::Res& R, int C, int Tmax, int ppf, const float* y, float* out, float* out2, const struct SnakeW* after);
    void resunit(const Pass& ps, const CodecW::Res& R, int C, int Tmax, int ppf, const uint16_t* y, uint16_t* out, uint16_t* out2,
                 const struct SnakeW* after);
    void capture(const Pass& ps, const char* name, const float* t, int T, int C);
    void capture(const Pass& ps, const char* name, const uint16_t* t, int T, int C);
    // first_frame (device [nb], slotted stream): row b's window starts at that frame of its code row; nullptr: at frame 0
    void run_front(const Pass& ps, const int32_t* codes, int code_stride_frames, int Fmax, float* const* bufs,
                   const int32_t* first_frame = nullptr);
    // The causal tail. `in`: the pre-transformer's frames, `Trows` rows per batch row in every tensor (streams: history
    // margin + chunk); the tensors in between come from `mem`: a Ring over the four scratch buffers, or the open Stream.
    struct Ring;
    template <class Mem>
    void run_tail(const Pass& ps, Mem& mem, float* in, int Trows, float* pcm);
    struct Stream {
        bool open = false, dry = false;  // dry: the counting pass of stream_open (no memory behind the tensors, no launches)
        StreamCfg cfg;
        int hist = 0, Tal = 0;       // margin frames, frames per allocation (hist + chunk)
        bool own_hops = false;       // slotted stream with a hop per row
        int up = 0;                  // samples per frame of the PCM tensor and the ring slots
        std::vector<int32_t> row_hs; // [rows] the hop table's entries (0: the row is copied)
        int next_chunk = 0;
        bool front_done = false;     // window < 0: the pre-transformer ran over all frames
        DevBuf<uint8_t> arena;
        size_t off = 0;
        std::vector<std::pair<float*, size_t>> rolls;  // (allocation base, frame floats) of the tensors with history
        float *lat = nullptr, *pcm = nullptr, *x_all = nullptr;
        float* fbufs[4] = {nullptr, nullptr, nullptr, nullptr};
        size_t fbuf_floats = 0;
        PinnedBuf<int32_t> lens_host;  // one slot per (chunk, kind): never reused inside a stream
        DevBuf<int32_t> lens_dev;
        size_t lens_used = 0;
        // slotted stream
        SlotPlanner plan;
        std::vector<std::pair<size_t, size_t>> roll_offs;  // (arena offset, frame floats) of `rolls`, from the counting pass
        DevBuf<uint8_t> roll_desc;     // RollDesc table of `rolls` (codec_kernels.h)
        int n_roll = 0;
        int64_t roll_max_ff = 0;
        PinnedBuf<float> ring_pcm;     // [kRingSlots][rows][chunk * upsample]
        PinnedBuf<int32_t> ring_nf;    // [kRingSlots][rows]
        PinnedBuf<int32_t> ring_args_host;  // [kRingSlots][5][rows]: window lengths, takes, first frames, chunk offsets, roll modes
        DevBuf<int32_t> ring_args_dev;
        std::vector<hipEvent_t> ring_ev;    // two per slot: begun, done
        std::vector<uint8_t> ring_busy;
        int ring_next = 0;
        // passes in which no row emits (reference prefixes alone) take their arguments from a pool of their own
        size_t state_bytes = 0;
        PinnedBuf<int32_t> quiet_args_host;  // [kQuietSlots][5][rows]
        DevBuf<int32_t> quiet_args_dev;
        std::vector<hipEvent_t> quiet_ev;    // behind the pass that read the slot's arguments
        std::vector<uint8_t> quiet_used;
        int quiet_next = 0;
        ~Stream() {
            for (auto e : ring_ev) (void)hipEventDestroy(e);
            for (auto e : quiet_ev) (void)hipEventDestroy(e);
        }
        uint8_t* take(size_t bytes);  // bump allocation (same order in stream_open's two passes and in every chunk)
        // the tail's next persistent tensor of Tal frames per row; one a later causal conv reads back into gets its margin rolled
        void* get(size_t frame_bytes, bool reads_back);
        void put(const void*) {}
    } stream_;
    void stream_prefix();  // rewinds the arena and lays out its fixed part: front buffers, x_all, lat, pcm
    size_t front_floats_per_frame() const;
    size_t floats_per_frame() const;
    void upload_lens(const int32_t* lens, int n);
    static constexpr int kMaxRows = 4096;
    const Model& m_;
    hipStream_t st_;
    int up_ = 1920;      // samples per frame of the PCM handed out (== native_ unless an output rate was asked for)
    int native_ = 1920;  // samples per frame behind out_conv
    bool resample_ = false;
    int out_rate_ = kResampleNative;  // the rate of the PCM handed out
    ResamplePlan out_plan_;   // 24000 -> output rate (a pitched handle: Hp * M -> Ho * L)
    DevBuf<float> out_tab_;   // its phase table on the device (a pitched handle: in output order, for resample_ratio.hip)
    int ho_ = kStretchHa;     // the speaking rate's hop
    bool pitched_ = false;    // the resampler is the general-ratio one and the stretch, if any, runs at pitch_hp_
    int pitch_hp_ = kStretchHa, pitch_delay_ = 0;
    bool formant_ = false;    // keep_formants on a pitched handle: analyse / whiten in front of the resampler, synthesise behind it
    DevBuf<float> fm_win_;    // FormantPlan's tables on the device: win [2 Hp], then lag [P + 1]
    int mid_ = 1920;          // samples per frame behind the time stretch == in front of the resampler (4 Hs, or native_)
    bool stretch_ = false;
    StretchPlan st_plan_;
    DevBuf<float> st_fade_;   // its fade table on the device
    bool rs_ = false;             // request speeds
    RequestSpeedPlan rs_plan_;
    DevBuf<float> fade_all_;      // the fade tables of every hop (request_speed_plan.h)
    DevBuf<int32_t> rowhs_dev_;   // decode with row_hs: [2][B] hops and mid frame sizes
    PinnedBuf<int32_t> rowhs_host_;
    static constexpr int kStateWords = 4;  // int32s per frame of the stretch's state tensor (the word and padding to 16 bytes)
    DevBuf<int32_t> ch_words_;  // decode_chunked: [B] state words carried from chunk to chunk
    DevBuf<float> ch_mid_;      // decode_chunked: [B][(1 + chunk) * mid_] stretched signal with one frame of margin
    bool no_h1_ = false;      // Q3TTS_CODEC_NO_F16=1: a float16 speech tokenizer through the up-cast (fp32-equivalent) path
    bool no_fuse_ = false;    // Q3TTS_CODEC_NO_FUSE=1: residual units of the narrow blocks as two launches each
    bool fp32_mfma_ = false;  // Q3TTS_CODEC_FP32=1: contract on the fp32 matrix-core path instead of the split one
    DevBuf<uint8_t> buf_;         // scratch of decode / decode_chunked
    DevBuf<int32_t> lens_dev_;
    PinnedBuf<int32_t> lens_host_;
    DevBuf<int32_t> nf_dev_;      // [kMaxRows] non-finite flags of the decode in flight (out_conv)
};

}  // namespace q3
