/*
 * q3tts.h -- C ABI of the MI355X-native Qwen3-TTS engine (libq3tts_hip.so).
 *
 * The reference (AtomGradient/swift-qwen3-tts) has no FFI boundary of its own: Swift calls the
 * mlx-swift API directly. This header is the boundary a Swift shim binds
 * to so that `Qwen3TTSModel` / `.generate` / `.generateStream` keep their signatures while the
 * MLX/Metal backend is replaced by hand-written HIP. Each entry point cites the reference
 * interface it replaces (paths relative to /root/reference/Sources/Qwen3TTS/). The Swift-side
 * binding is shown in INTEGRATION.md.
 *
 * Conventions: plain pointers and sizes, opaque handle, int status codes, no exceptions and no
 * torch/HIP types across the boundary. Tokenisation stays on the caller's side
 * (swift-transformers in the reference, Qwen3.swift:274-275): the engine takes token ids.
 * One q3tts_model per GPU; calls on one handle are serialised by the caller (the reference
 * model object is not re-entrant either). The library checks this: a call that finds the handle
 * inside another thread's call returns Q3TTS_ERR_INVALID_INPUT at once (nested calls from the
 * same thread, e.g. from an event callback running on the calling thread, are fine).
 */
#ifndef Q3TTS_H
#define Q3TTS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define Q3TTS_ABI_VERSION 4

typedef struct q3tts_model q3tts_model;

/* Status codes 1..5 map 1:1 to AudioGenerationError (Core/GenerationTypes.swift:63-84). */
typedef enum {
    Q3TTS_OK = 0,
    Q3TTS_ERR_MODEL_NOT_INITIALIZED = 1, /* .modelNotInitialized  "Model not initialized: ..." */
    Q3TTS_ERR_GENERATION_FAILED = 2,     /* .generationFailed     "Generation failed: ..."     */
    Q3TTS_ERR_INVALID_INPUT = 3,         /* .invalidInput         "Invalid input: ..."         */
    Q3TTS_ERR_AUDIO_DECODING_FAILED = 4, /* .audioDecodingFailed                               */
    Q3TTS_ERR_AUDIO_ENCODING_FAILED = 5, /* .audioEncodingFailed                               */
    Q3TTS_ERR_IO = 6,     /* checkpoint/config read or parse failure (thrown Foundation errors) */
    Q3TTS_ERR_DEVICE = 7, /* HIP runtime failure; the engine never falls back to the CPU        */
    Q3TTS_ERR_CANCELLED = 8, /* new: the request was cancelled (q3tts_session_cancel / close without drain) */
    Q3TTS_ERR_BUSY = 9       /* new: q3tts_session_submit: max_pending requests are already waiting */
} q3tts_status;

typedef struct {
    int32_t device;     /* HIP device ordinal */
    int32_t max_batch;  /* rows per q3tts_generate call, 1..64 (reference: always 1) */
    int32_t max_frames; /* upper bound on codec frames per row; sizes the paged KV pool (default 2048) */
    int32_t max_prompt; /* upper bound on prompt positions per row (default 512) */
    int32_t use_graph;  /* 1: replay the per-frame step as a hipGraph (default); 0: eager launches */
    int32_t weights_from_broadcast; /* 1: allocate the weight arena but do not read tensor data from
                                       disk; the caller fills it (RCCL broadcast from rank 0) via
                                       q3tts_model_arena before the first generate */
    int32_t n_streams;  /* lanes the batch is split over (own HIP stream + hipGraph + host thread each);
                           0 = default (1). Results do not depend on it (rows are independent). With more than one
                           lane q3tts_generate_begin runs its job to completion (TOKEN, INFO and AUDIO events fire inside
                           begin) and q3tts_generate_end only hands the results over: nothing overlaps.
                           With one lane (the default) the handle holds TWO job contexts, each with the whole per-batch state
                           at max_batch x (max_prompt + max_frames) -- activation workspace, paged KV pool, per-row state, frame
                           graphs, codec scratch -- so that two outstanding jobs generate side by side (q3tts_generate_begin).
                           The second context is allocated at load and costs what the first one does: the KV pool,
                           max_batch x ceil((max_prompt + max_frames + 1) / 64) pages of 64 tokens x layers x kv heads x 128 x
                           2 (K, V) x 2 bytes, is the large part, the codec decoder's scratch (grown by the first decode on
                           each context) the other. For the 1.7B talker, measured:
                           at max_batch 32, max_frames 208, max_prompt 128 the second context adds 1.5 GiB at load (1.4 GiB of
                           it KV pool) and 19.1 GiB once it has decoded 32 x 200 frames (the codec scratch); at the defaults
                           (max_batch 1, max_frames 2048, max_prompt 512) 0.3 GiB at load and 0.9 GiB after a 200-frame call */
    int32_t codec_overlap_cus; /* compute units a codec decode is confined to while other batches' frame loops run beside it
                           (q3tts_generate_begin with more_follows != 0); multiple of 8; 0 = default (tuned for a 1.7B
                           talker at batch 32: half of the CUs for a job whose AR loop ran inside begin, three quarters for
                           a background job), n > 0 = that many for every job, -1 = never confine. Results do not depend
                           on it */
    int32_t codec_fp32;  /* 1: the codec decoder's convolutions on the fp32 matrix cores (the reference's arithmetic range, 2.4x the
                           time) instead of fp16 matrix cores with every fp32 operand split into two fp16 planes (same accuracy,
                           activations limited to |x| < 65504: a decode that leaves that range reports
                           Q3TTS_ERR_AUDIO_DECODING_FAILED for the row instead of a waveform). Default 0 */
    int32_t output_sample_rate; /* new (the reference speaks 24 kHz only): the rate of every waveform this handle hands out.
                           0 (default) or 24000: the decoder's own rate -- nothing is added, the samples are what a handle
                           loaded without this field gives, bit for bit. 8000, 12000, 16000, 22050, 32000, 44100 or 48000:
                           the decoder's causal tail gets one more causal stage, the polyphase FIR defined under "Sample
                           rates" below, in its causal form, and q3tts_model_info.sample_rate / .samples_per_frame report
                           the rate and 1920 * rate / 24000 (640, 960, 1280, 1764, 2560, 3528, 3840). Everything this header
                           counts in samples or states as "* 1920" then counts samples at that rate with that many per
                           frame: pcm buffers and AUDIO_CHUNK.sample_offset, the end trim count(code0 > 0) * samples_per_frame,
                           the clone cut R * samples_per_frame. Every guarantee in this header holds unchanged at the
                           handle's rate -- streamed equals one-shot (window < 0), queued equals alone, session equals queued,
                           bit for bit -- because the stage carries its history from chunk to chunk like the other causal
                           convs of the tail, and the one-shot decode uses the same causal form. The output is therefore
                           delayed by K input samples (K: below): 2.1 ms at 8 kHz, 0.7 ms at 48 kHz. The result is clipped to
                           [-1, 1] again (the FIR overshoots). Non-finite flags still come from the 24 kHz signal. A saved
                           prefix state of a voice grows by the stage's margin, 3 x 1920 x 4 bytes. Per handle, not per
                           call: every buffer behind the tail is sized at load by samples per frame. Any other value is
                           Q3TTS_ERR_INVALID_INPUT at load */
    float speed;        /* new (the reference has no speaking rate): how fast this handle speaks, pitch preserved. 0 (default) or
                           1.0: off -- nothing is added, the samples are what a handle loaded without this field gives, bit for
                           bit. 0.5 .. 2.0: the decoder's causal tail gets the time stretch defined under "Speaking rate"
                           below, in its causal form, behind out_conv and in front of the output-rate stage. The synthesis hop
                           Hs is the integer in [240, 960] nearest to 480 / speed (ties toward 480) for which a frame holds a
                           whole number of samples at output_sample_rate (4 * Hs * L % M == 0; without an output rate every
                           integer); q3tts_model_get_speed reports it and the effective speed 480 / Hs. A frame then yields
                           4 * Hs samples at 24 kHz: q3tts_model_info.samples_per_frame is 4 * Hs * rate / 24000 and everything
                           this header counts in samples follows it, as with output_sample_rate. Every guarantee holds unchanged
                           -- streamed equals one-shot (window < 0), the chunked exact decode equals one-shot, queued equals
                           alone, session equals queued, a voice's saved prefix state continues identically, bit for bit: the
                           stage carries its input's margin and one int32 per row (the last hop's offset) from chunk to chunk.
                           The causal form delays the audio by D 24 kHz samples (0 at 2x, 80 at 1.5x, 480 at 0.8x, 1200 at
                           0.5x): a waveform starts with about D * Hs / 480 samples of silence and its last D input samples are
                           not spoken (no flush). Hs == 480 is off. This is the handle's speed: what a request without a speed
                           of its own gets (request_speeds below). Outside [0.5, 2.0], NaN or infinite:
                           Q3TTS_ERR_INVALID_INPUT at load, before any GPU work */
    int32_t request_speeds; /* new: non-zero makes the handle admit q3tts_request.speed ("Speaking rate per request" below). The
                           fade tables of every hop in [240, 960] go to the device once, at load (2.8 MB), and what holds rows of
                           different speeds is sized for the slowest, 4 * 960 * L / M samples per frame
                           (q3tts_model_info.max_samples_per_frame). 0 (default): the handle allocates and launches what it
                           did, and a request with a speed is Q3TTS_ERR_INVALID_INPUT. With the option and no request speed
                           the samples are those of the same handle without it, bit for bit */
} q3tts_load_opts;

void q3tts_default_load_opts(q3tts_load_opts* o);

/* new: the load options with what has been added since q3tts_load_opts was last pinned. q3tts_load_opts keeps its layout and
 * its last field (existing callers and tests pin both), so a later option lives here, behind the options it extends, and is
 * given to q3tts_model_load_ex. q3tts_model_load(dir, opts, out) is q3tts_model_load_ex with `base` = *opts and every
 * extension at its default. */
typedef struct {
    q3tts_load_opts base; /* every option above, with its meaning and checks */
    float pitch;        /* this handle's pitch in semitones at an unchanged duration
                           ("Pitch" below). 0 (default): off -- nothing is added, launched or allocated, the samples are what a
                           handle loaded without this field gives, bit for bit. Otherwise in [-12, 12]: with Ho the hop the
                           handle would have had (480, or the Hs of `speed`) and rho = 2^(pitch / 12), Hp is the integer nearest
                           to Ho * rho, ties toward Ho; Hp == Ho is off as well. The time stretch then runs at Hs = Hp and one
                           resampler behind it takes Hp * M samples to Ho * L (L / M: output_sample_rate / 24000), so
                           samples_per_frame, n_samples and every count in samples are those of the same handle without a
                           pitch, every frequency is multiplied by Hp / Ho (q3tts_model_get_pitch reports the effective
                           12 log2(Hp / Ho)), and every guarantee of `speed` with `output_sample_rate` holds, bit for bit.
                           Q3TTS_ERR_INVALID_INPUT at load: a pitch outside [-12, 12], NaN or infinite, or together with
                           request_speeds (both before any GPU work); no Hp in [240, 960] for this speed (never clamped:
                           speed 0.5 leaves no room upward, speed 2 none downward); a codec frame that is not a whole number
                           of 480-sample hops. Formants move with the pitch: beyond a few semitones the voice changes
                           (q3tts_load_opts_ex2.keep_formants keeps them) */
} q3tts_load_opts_ex;

void q3tts_default_load_opts_ex(q3tts_load_opts_ex* o); /* q3tts_default_load_opts for `base`, pitch 0 */

/* Qwen3TTSModel.fromPretrained(_:) (Models/Qwen3.swift:1382-1452) + postLoadHook (:1455-1495,
 * minus the text tokenizer, which stays with the caller). */
q3tts_status q3tts_model_load(const char* model_dir, const q3tts_load_opts* opts, q3tts_model** out);
q3tts_status q3tts_model_load_ex(const char* model_dir, const q3tts_load_opts_ex* opts, q3tts_model** out);

/* new: q3tts_load_opts_ex is pinned in its turn (its last field is `pitch`); what comes later lives behind the whole of it and is
 * given to q3tts_model_load_ex2. q3tts_model_load_ex(dir, opts, out) is q3tts_model_load_ex2 with `ex` = *opts and
 * keep_formants = 0. */
typedef struct {
    q3tts_load_opts_ex ex; /* every option above, with its meaning and checks */
    int32_t keep_formants; /* 0 (default): off. 1: a pitch of this handle keeps the formants ("Formant preservation" below): the
                              spectral envelope is estimated per hop by linear prediction, taken off in front of the pitch
                              resampler and put back behind it, so the excitation moves and the voice stays. With pitch 0, or a
                              pitch whose Hp == Ho, nothing is added, launched or allocated and the samples are those of the
                              handle without the option, bit for bit. Sample counts never change. Q3TTS_ERR_INVALID_INPUT at load,
                              before any GPU work: a value other than 0 / 1; 1 with an output_sample_rate other than 0 / 24000
                              (the synthesis filter runs at 24 kHz spacing; a second rate stage behind it is not offered). On
                              such a handle a q3tts_generate with audio_chunk_frames > 0 that would not be streamed -- no
                              audio_window_frames, or a voice-clone row without audio_stream_reference: the chunked exact decode
                              -- is Q3TTS_ERR_INVALID_INPUT, before any GPU work: stream it, or decode in one piece */
} q3tts_load_opts_ex2;

void q3tts_default_load_opts_ex2(q3tts_load_opts_ex2* o); /* q3tts_default_load_opts_ex for `ex`, keep_formants 0 */
q3tts_status q3tts_model_load_ex2(const char* model_dir, const q3tts_load_opts_ex2* opts, q3tts_model** out);
void q3tts_model_free(q3tts_model* m);

/* Message of the last failure on this handle (NULL handle: last load failure on this thread).
 * Texts match the reference's error descriptions (GenerationTypes.swift:70-83). */
const char* q3tts_last_error(const q3tts_model* m);

/* Device weight arena (one contiguous allocation; layout is a pure function of the config, so
 * rank 0 can broadcast it to replicas at load: SURVEY.md section 8e). */
q3tts_status q3tts_model_arena(q3tts_model* m, void** device_ptr, size_t* bytes);

typedef struct {
    char tts_model_type[32]; /* Qwen3TTSModel.ttsModelType (Qwen3.swift:1269-1271) */
    int32_t sample_rate;     /* .sampleRate (Qwen3.swift:1262-1264): 24000, or q3tts_load_opts.output_sample_rate when set */
    int32_t supports_voice_cloning; /* .supportsVoiceCloning (Qwen3.swift:1210-1214) */
    int32_t has_voice_cloning;      /* .hasVoiceCloning (Qwen3.swift:61-63) */
    int32_t hidden_size, num_layers, vocab_size, text_vocab_size, num_code_groups;
    int32_t cp_hidden_size, cp_num_layers, cp_vocab_size;
    int32_t codec_eos_token_id;
    int32_t samples_per_frame; /* decodeUpsampleRate, 1920; at another output rate 1920 * sample_rate / 24000 */
    int32_t max_batch;
    int64_t weight_bytes;      /* distinct bytes streamed per decode step (roofline accounting) */
    int32_t speaker_embedding_dim; /* enc_dim of the speaker encoder, 0 when absent */
    int32_t max_samples_per_frame; /* new: samples per frame of the slowest request the handle admits: 4 * 960 * sample_rate /
                                      24000 with q3tts_load_opts.request_speeds, samples_per_frame (the handle's own, what a
                                      request without a speed gets) otherwise */
} q3tts_model_info;
q3tts_status q3tts_model_get_info(const q3tts_model* m, q3tts_model_info* out);

/* ---- multi-GPU (new: the reference is single-device, Qwen3.swift:1382-1470) ----------------------------------------------------
 * Utterances are independent, so a job shards by rows: one process (or handle) and one full replica per GPU, NO collective on
 * the data path. The only exchange is at load: rank `root` reads the checkpoint, every other rank loads with
 * q3tts_load_opts.weights_from_broadcast = 1 (config only, empty arena) and receives the arena -- whose layout is a pure
 * function of the config -- in one RCCL broadcast over xGMI. Recipe for a host without Python:
 *   rank 0: q3tts_comm_get_unique_id(&id); ship the 128 bytes to the other ranks (file, socket, MPI, environment ...)
 *   all   : q3tts_model_broadcast(model, &id, rank, world, 0);   // collective: every rank must call it
 *   rank r: q3tts_generate(rows [r * B, (r + 1) * B), q3tts_sampling.row_base = r * B)   // draws what one big call would
 * RCCL is opened at run time (librccl.so.1); single-GPU callers never need it. Status DEVICE (7) carries RCCL's message. */
typedef struct { char bytes[128]; } q3tts_comm_id; /* == ncclUniqueId */
q3tts_status q3tts_comm_get_unique_id(q3tts_comm_id* out);
q3tts_status q3tts_model_broadcast(q3tts_model* m, const q3tts_comm_id* id, int32_t rank, int32_t world, int32_t root);
/* 64-bit sum of the arena's 32-bit words (device-side reduction): equal on every rank after the broadcast. */
q3tts_status q3tts_model_arena_checksum(q3tts_model* m, uint64_t* out);

/* Qwen3TTSModel.supportedSpeakers, sorted (Qwen3.swift:965-971). */
int32_t q3tts_model_num_speakers(const q3tts_model* m);
const char* q3tts_model_speaker_name(const q3tts_model* m, int32_t i);

/* One utterance. Mirrors the arguments of generate(text:speaker:instruct:language:...)
 * (Qwen3.swift:1291-1301) after tokenisation:
 *   text_ids      = tokens of "<|im_start|>assistant\n{text}<|im_end|>\n<|im_start|>assistant\n" (:274-275)
 *   instruct_ids  = tokens of "<|im_start|>user\n{instruct}<|im_end|>\n" or NULL (:364-365)
 *   target_token_count = tokens of {text} alone, for the max-token cap (:822-823) */
typedef struct {
    const int32_t* text_ids;
    int32_t n_text_ids;
    const int32_t* instruct_ids;
    int32_t n_instruct_ids;
    int32_t target_token_count;
    const char* speaker;  /* NULL = none */
    const char* language; /* NULL = "auto" */
    int32_t max_tokens;   /* 0 = 2048 (reference default) */
    float speed;          /* new: this request's speaking rate ("Speaking rate per request" below). 0 (default): the handle's.
                             Otherwise in [0.5, 2.0], on a handle loaded with request_speeds; 1.0 is "no stretch for this
                             request", whatever the handle's own speed. The field lies in what was padding behind max_tokens:
                             sizeof(q3tts_request) and Q3TTS_ABI_VERSION are unchanged, and a caller that zeroes the struct
                             (as every example here does) asks for the handle's speed */
    /* Voice clone -- generateVoiceClone(text:referenceAudio:referenceText:language:...) (Qwen3.swift:1009-1020).
     * ref_audio != NULL selects it; speaker / instruct_ids are then ignored, as in the reference.
     *   ref_audio     = reference waveform, 24 kHz mono float32 (host memory, read during the call; a NaN or infinite
     *                   sample is Q3TTS_ERR_INVALID_INPUT). A clip at another rate goes through a voice
     *                   (q3tts_voice_create_rate) or through q3tts_resample first: this field has no rate of its own
     *   ref_text_ids  = tokens of "<|im_start|>assistant\n{referenceText}<|im_end|>\n" (:448-449)
     * The reference's default repetition penalty on this path is 1.5 (:1017), against 1.05 for generate(): a batch that mixes
     * both gives each request its own through q3tts_sampling.per_request (Q3TTS_ROW_REPETITION_PENALTY).
     * Result: pcm = audio of the target text only (reference part cut proportionally, :1195-1199),
     * codes = generated frames only. */
    const float* ref_audio;
    int64_t n_ref_samples;
    const int32_t* ref_text_ids;
    int32_t n_ref_text_ids;
    int32_t route; /* 0: generate() -- the prompt builder is chosen by tts_model_type and its requirements are enforced
                      (Qwen3.swift:1302-1372). 1: generateVoiceDesign called directly (:587-597): no speaker, instruct optional,
                      whatever the checkpoint's type. 2: generateCustomVoice called directly (:783-794): the speaker is
                      required and validated against talker_config.spk_id (:803-811), instruct optional. Ignored for
                      voice-clone requests (ref_audio != NULL) */
} q3tts_request;

/* Sampling parameters of ONE request of a call (new: the reference samples one utterance per call, so its arguments are
 * per request by construction). `set` names the fields that override the call's q3tts_sampling for this request; the others
 * are ignored and the request inherits the call's values. A set seed replaces the seed of the request's random stream
 * (seed, row_base + i); the stream's key, row_base + i, stays.
 * Checked before any GPU work, the engine staying usable (Q3TTS_ERR_INVALID_INPUT): bits of `set` other than the five below;
 * of the set fields, a temperature, top_p or repetition_penalty that is NaN or infinite, top_k < 0, repetition_penalty <= 0,
 * top_p outside [0, 1] (top_p <= 0 keeps its meaning of "no top-p"). */
#define Q3TTS_ROW_TEMPERATURE        1u
#define Q3TTS_ROW_TOP_K              2u
#define Q3TTS_ROW_TOP_P              4u
#define Q3TTS_ROW_REPETITION_PENALTY 8u
#define Q3TTS_ROW_SEED               16u
typedef struct {
    uint32_t set;   /* which fields below override the call's q3tts_sampling for this request */
    float temperature;
    int32_t top_k;
    float top_p;
    float repetition_penalty;
    uint64_t seed;
} q3tts_row_sampling;

/* Defaults as generate(): 0.9 / 50 / 1.0 / 1.05 (Qwen3.swift:1296-1299). */
typedef struct {
    float temperature; /* <= 0: greedy argmax (Qwen3.swift:182-185) */
    int32_t top_k;
    float top_p;
    float repetition_penalty;
    uint64_t seed;        /* new: the reference draws from MLX's global key and has no seed API */
    int32_t force_frames; /* bench only: mask EOS and emit exactly this many frames per row */
    int32_t audio_chunk_frames; /* new (the reference decodes one-shot, README.md:140): > 0 delivers the waveform in pieces of
                                   this many codec frames through AUDIO_CHUNK events as the causal tail of the decoder
                                   produces them, before INFO / AUDIO; the samples are bit-identical to the one-shot decode */
    int32_t audio_window_frames; /* 0 (default): the chunks above are cut after the last token, from the exact decode.
                                   > 0 (with audio_chunk_frames > 0): audio leaves WHILE tokens are still being generated. The
                                   decoder's pre-transformer is bidirectional over the whole utterance (SpeechTokenizer.swift:763),
                                   so a chunk is then computed from the frames that exist: this many frames of left context and
                                   audio_lookahead_frames to the right; everything behind the pre-transformer is causal and
                                   carries its state from chunk to chunk (exact). The arithmetic is pinned against the oracle's
                                   restatement of exactly this definition (OracleModel.codec_decode_streamed, PCM within 1e-4:
                                   tests/test_streaming.py). Its distance from the ONE-SHOT waveform is a property of the
                                   checkpoint -- how much of the signal the pre-transformer's attention carries -- and is
                                   not guaranteed: 1.6e-2 max / 1 % of the signal r.m.s. at window 32 / lookahead 4 on the synthetic
                                   full-width checkpoint (reported by the test), zero with a window over
                                   everything. AUDIO then carries the concatenation of the chunks -- all generated frames: the
                                   reference's end trim to count(code0 > 0) frames (SpeechTokenizer.swift:831-833) cannot apply
                                   to samples that have already left. audio_chunk_frames must be at
                                   least the causal tail's history (3 frames for the shipped decoder geometry; checked before any
                                   GPU work). A call with a voice-clone row (ref_audio or a voice) falls back to 0 for the whole
                                   batch unless audio_stream_reference is set. With it a clone row, whose decoder runs over
                                   [reference ++ generated] frames (Qwen3.swift:1178-1186), is streamed with its R reference
                                   frames as a prefix of its stream (the definition is at q3tts_codec_decode_streamed_prefixed):
                                   the prefix is decoded in chunks of its own whose lookahead stops at frame R and whose
                                   samples are never delivered; generated chunk k covers frames [R + kC, R + (k+1)C) of
                                   ref ++ gen, its window reaches back into the reference while kC < window, and it is
                                   decodable once the row has (k+1)C + lookahead generated frames or is final. The row's
                                   audio is the causal tail's output from sample R * 1920 on: AUDIO_CHUNK.sample_offset =
                                   k * C * 1920, AUDIO is the concatenation, n * 1920 samples for n generated frames, no end
                                   trim (as for every streamed row), and the cut is exactly R * 1920 where the one-shot clone
                                   path's Float proportion (Qwen3.swift:1195-1199) needs the final length and can differ by a
                                   sample. Plain rows of such a batch are streamed exactly as without the flag. Also honoured by
                                   q3tts_generate_queued, per request: every request of the queue is streamed as if alone */
    int32_t audio_lookahead_frames; /* frames to the right of a chunk that must exist before it is decoded (default 4) */
    uint32_t row_base;    /* new: global index of reqs[0] in a job whose rows are sharded over several processes (one
                             replica per GPU). A row's random stream is keyed by (seed, row_base + row index), so a sharded
                             job draws what the same rows would draw in one call. Default 0 */
    const q3tts_row_sampling* per_request; /* new: [n_reqs] (q3tts_debug_sample: [rows]) or NULL (default): request i samples
                             with the call's values above with per_request[i]'s set fields folded in. force_frames, the
                             audio_* fields and row_base stay call-wide. Read only during the call (q3tts_generate_begin:
                             during begin, like reqs). Row independence holds for every entry point that takes a
                             q3tts_sampling -- q3tts_generate, _begin / _end (foreground and background),
                             q3tts_generate_queued (streamed or not, any n_streams), q3tts_debug_generate_forced and
                             q3tts_debug_sample: results[i] is bit-identical in codes, pcm, n_frames, n_samples and status to
                             q3tts_generate of reqs[i] alone, with per_request == NULL, the call's sampling with row i's set
                             fields folded in, and row_base = sampling->row_base + i. The frame graphs do not depend on
                             the values: no call re-captures one because parameters changed */
    int32_t audio_stream_reference; /* new, 0 (default): voice-clone rows are never streamed while they generate (see
                             audio_window_frames and the voices comment). 1, with audio_chunk_frames > 0 and audio_window_frames > 0:
                             clone rows -- ref_audio rows and voices alike -- are streamed with their reference in front of their
                             stream, as q3tts_codec_decode_streamed_prefixed defines it. Call-wide, like the other audio_* fields */
} q3tts_sampling;
void q3tts_default_sampling(q3tts_sampling* s);

/* AudioGenerationInfo (Core/GenerationTypes.swift:15-21). */
typedef struct {
    int32_t prompt_token_count;
    int32_t generation_token_count;
    double prefill_time;
    double generate_time;
    double tokens_per_second;
    double peak_memory_usage; /* GB */
} q3tts_gen_info;

/* enum AudioGeneration { token, info, audio } (Core/GenerationTypes.swift:51-58). Per request the
 * order is TOKEN* (EOS is not reported: Qwen3.swift:868-871), INFO, AUDIO -- the order
 * generateStream yields them (Qwen3+Streaming.swift:24-27,118-120). */
typedef enum {
    Q3TTS_EVENT_TOKEN = 0, Q3TTS_EVENT_INFO = 1, Q3TTS_EVENT_AUDIO = 2,
    Q3TTS_EVENT_AUDIO_CHUNK = 3 /* only with q3tts_sampling.audio_chunk_frames > 0: samples [sample_offset, +n_samples) of
                                   the request's final audio, in order, between the last TOKEN and INFO */
} q3tts_event_kind;
typedef struct {
    q3tts_event_kind kind;
    int32_t request_index;
    int32_t token;              /* TOKEN */
    const q3tts_gen_info* info; /* INFO  */
    const float* pcm;           /* AUDIO, AUDIO_CHUNK: valid during the callback */
    int64_t n_samples;
    int64_t sample_offset;      /* AUDIO_CHUNK: position of pcm[0] in the request's final audio */
} q3tts_event;
typedef void (*q3tts_event_cb)(void* user, const q3tts_event* ev);

typedef struct {
    q3tts_status status; /* per-request outcome (e.g. GENERATION_FAILED "No tokens generated") */
    float* pcm;          /* mono float32 at q3tts_model_info.sample_rate (24 kHz by default), trimmed as Qwen3.swift:954-959; engine-owned */
    int64_t n_samples;
    int32_t* codes;      /* [n_frames][num_code_groups]; engine-owned */
    int32_t n_frames;
    q3tts_gen_info info;
} q3tts_result;

/* generate / generateStream (Qwen3.swift:1291-1373, Qwen3+Streaming.swift:8-125) for n_reqs
 * utterances at once (row-independent: each row equals the batch-1 result for that request).
 * `cb` may be NULL. `results` has n_reqs entries, released with q3tts_result_free. */
q3tts_status q3tts_generate(q3tts_model* m, const q3tts_request* reqs, int32_t n_reqs,
                            const q3tts_sampling* sampling, q3tts_event_cb cb, void* user,
                            q3tts_result* results);
void q3tts_result_free(q3tts_result* results, int32_t n);

/* q3tts_generate in two halves, for callers with a queue of batches (the reference has neither batches nor a queue:
 * its generate() decodes one-shot after the loop, Qwen3.swift:943-959, which is what each job still does).
 *   begin: input checks, voice front end, prompt assembly and prefill of this batch, on the calling thread: whatever can
 *          refuse a request refuses it here, and a begin that fails leaves the other job and both job slots as they were.
 *          With `cb` != NULL (or audio_chunk_frames > 0) the AR loop runs inside begin as well: TOKEN events fire here,
 *          on the calling thread, and begin returns once the codes exist and their codec decode has been queued on the
 *          job's codec stream. With `cb` == NULL and audio_chunk_frames == 0 (a throughput job: nobody listens) begin
 *          returns as soon as the prefill is queued -- BEFORE the codes exist -- and the AR loop runs on a thread owned by
 *          the job's context. `reqs` is only read during begin either way.
 *   end:   waits for the AR loop and the decode, fills `results` (n_reqs entries of the begin call), fires INFO and AUDIO
 *          events, and releases the job. A failure of a background AR loop is reported here, with its status; the job
 *          slot is released whatever end returns.
 * A second begin may be issued before the first job's end. The handle has two job contexts (q3tts_load_opts.n_streams) and
 * a job takes the free one, so the second job's AR loop -- a latency-bound chain of small launches that cannot fill the
 * chip alone -- runs beside the first job's AR loop when both are background jobs, and beside its decode (matrix-core
 * work) in any case. At most 2 jobs may be outstanding per model handle; results do not depend on the interleaving (jobs
 * share nothing but the weights; the decode reads job-owned copies of the codes). q3tts_generate == begin + end, with the
 * AR loop on the calling thread; successive calls alternate between the two contexts. q3tts_last_timing describes the job
 * that was ENDED last. q3tts_model_free with jobs begun and never ended lets their AR loops finish first. The entry points
 * that work on one engine (q3tts_codec_decode / _encode / _encoded_frames, q3tts_speaker_embedding, the q3tts_debug_* calls)
 * use the first context and wait for a background AR loop still running on it.
 * `more_follows` != 0 says that another begin will be issued before this job's end: the decode is then confined to part
 * of the chip so that the next batch's launch chain keeps room (a decode that fills every CU stalls that chain and
 * nothing is gained); 0 (the last batch of a queue) lets the decode use the whole chip. Results do not depend on it. */
typedef struct q3tts_job q3tts_job;
q3tts_status q3tts_generate_begin(q3tts_model* m, const q3tts_request* reqs, int32_t n_reqs,
                                  const q3tts_sampling* sampling, q3tts_event_cb cb, void* user, int32_t more_follows,
                                  q3tts_job** job);
q3tts_status q3tts_generate_end(q3tts_model* m, q3tts_job* job, q3tts_result* results);

/* Continuous batching (new: the reference has no batches, Qwen3.swift:847-936 generates one utterance at a time). Runs
 * n_reqs requests (any number >= 1) with at most `slots` rows in flight, 1 <= slots <= max_batch: a slot whose row finishes
 * (EOS or its max_tokens cap) takes the next request in index order, so rows of different lengths do not wait for the
 * longest one of a batch. results[i] (n_reqs entries, freed with q3tts_result_free) is bit-identical in codes, pcm,
 * n_frames, n_samples and status to what q3tts_generate returns for reqs[i] with row_base = sampling->row_base + i: request
 * i draws from random stream (seed, row_base + i), whatever slot or lane serves it.
 * Events, per request with request_index = i: TOKEN*, INFO, AUDIO. A request's INFO and AUDIO fire as soon as its audio is
 * decoded, which can be before later requests have started; the interleaving across requests is unspecified.
 * Streamed audio (sampling->audio_chunk_frames > 0 AND audio_window_frames > 0): every request's audio leaves in pieces
 * while it generates, each request as if it had been streamed alone.
 *   - results[i] (codes, pcm, n_frames, n_samples, status) is bit-identical to what q3tts_generate returns for reqs[i] alone
 *     with the same sampling (streaming fields included) and row_base = sampling->row_base + i; slot, lane, admission burst and
 *     whichever other rows share a decoder pass do not change it. Equivalently pcm is q3tts_codec_decode_streamed(codes_i,
 *     audio_chunk_frames, audio_window_frames, audio_lookahead_frames). As in a streamed q3tts_generate, AUDIO carries all
 *     generated frames: n_samples = n_frames * samples_per_frame, no end trim.
 *   - Chunks are per request: chunk k of a request with n frames covers frames [kC, min(n, (k+1)C)), its pre-transformer
 *     window is [max(0, kC - W), min(n, (k+1)C + L)), and it is decodable once the request has (k+1)C + L frames or is final.
 *   - Events per request: TOKEN* and AUDIO_CHUNK* interleaved, then INFO, then AUDIO. AUDIO_CHUNK carries request_index = i and
 *     sample_offset = k * C * samples_per_frame, in order; the pieces concatenate to AUDIO. INFO and AUDIO fire once the
 *     request's last chunk has landed on the host.
 *   - A request whose chunk leaves the fp16 range follows the rule of a streamed q3tts_generate: it delivers nothing more from
 *     its first flagged chunk on, is decoded again on the fp32 matrix cores once the queue has drained (its remaining
 *     AUDIO_CHUNK events, INFO and AUDIO leave then), and only if that fails too ends in AUDIO_DECODING_FAILED -- alone.
 *   - n_streams > 1: each lane streams its own slots; results do not depend on the lane count.
 * Every request is checked before any GPU work (prompt length, max_tokens <= max_frames, speaker, route, RoPE range). Refused
 * with Q3TTS_ERR_INVALID_INPUT before any GPU work, the engine staying usable: slots outside 1..max_batch, a voice-clone request
 * (ref_audio != NULL), audio_chunk_frames > 0 with audio_window_frames == 0 (chunks cut after a request's end give a queue
 * nothing: its AUDIO already leaves as soon as it is decoded), audio_chunk_frames > 0 below the causal tail's history (as a
 * streamed q3tts_generate), a q3tts_generate_begin job outstanding on the handle. force_frames keeps its meaning.
 * A request whose first token is EOS fails alone (GENERATION_FAILED), as does a row whose decode leaves the fp16 range even
 * on the fp32 re-decode (AUDIO_DECODING_FAILED); the others are delivered.
 * q3tts_last_timing afterwards: frame_steps = frame-step replays, prefill_ms = sum of all admission prefills, codec_ms = sum
 * of the decode batches (streamed: of the stream's passes), rows = n_reqs; streamed: first_audio_ms = time from the call to
 * the first AUDIO_CHUNK samples of any request on the host. A request's q3tts_gen_info times run from its admission to its
 * retirement (the burst boundary at which its finished row was seen), not over the whole call. */
q3tts_status q3tts_generate_queued(q3tts_model* m, const q3tts_request* reqs, int32_t n_reqs, int32_t slots,
                                   const q3tts_sampling* sampling, q3tts_event_cb cb, void* user, q3tts_result* results);

/* Reusable voice prompts (new: the reference encodes the clip inside every generateVoiceClone call, Qwen3.swift:436-444,
 * 521-525). A voice is one reference clip and its transcript, encoded ONCE and held on the device: what a voice-clone request
 * needs from its reference -- the 16 code rows of the clip, the prompt rows made of them (the speaker x-vector and one embedding
 * sum per reference frame) -- plus host copies of the codes and of the reference text. Requests then name it, and a request that
 * does costs no more to admit than an ordinary one: no upload, no codec encoder, no speaker encoder, no copy back to the host.
 * That is what lets q3tts_generate_queued_voices serve voice-clone requests, which q3tts_generate_queued refuses.
 *   q3tts_voice_create: ref_audio / ref_text_ids as in q3tts_request, with every check a voice-clone request gets (status 1
 *     without the speech tokenizer encoder; 3 for an empty clip, a non-finite sample, fewer than 5 or out-of-range reference-text
 *     ids, an encoder codebook beyond the embedding tables). It synchronises before it returns; from then on the voice is read-only
 *     and may be named by any number of requests, in any call on this handle, whichever job context, lane or slot serves them.
 *     Like the other entry points that work on one engine it uses the first context and waits for a background AR loop on it.
 *     q3tts_last_timing afterwards: frontend_ms of this clip.
 *   q3tts_voice_free: releases the voice's buffers. Freeing a voice while a call that names it is running (a q3tts_generate_begin
 *     job included, until its end) is a caller error. q3tts_model_free releases the voices still alive; their pointers are dead
 *     after it.
 *   q3tts_voice_get_info: device_bytes = 64 * ref_frames (codes) + 2 * hidden_size * (1 + ref_frames) (prompt rows).
 * voices[i] == NULL: request i is what it is without this argument (q3tts_generate_voices with every entry NULL behaves as
 * q3tts_generate). voices[i] != NULL: request i is a voice-clone request whose reference is that voice; speaker, instruct_ids
 * and route are ignored, as for ref_audio.
 * For both entry points results[i] is bit-identical -- status, codes, pcm, n_frames, n_samples -- to what q3tts_generate returns
 * for reqs[i] alone with ref_audio / ref_text_ids set to the voice's clip and text, the call's sampling with per_request[i]
 * folded in and row_base = sampling->row_base + i, whatever slot, lane, admission burst or decode batch serves it.
 * q3tts_last_timing.frontend_ms is 0 for a call whose clone rows are all voices. Events and everything else as
 * q3tts_generate / q3tts_generate_queued.
 * Refused with Q3TTS_ERR_INVALID_INPUT before any GPU work, the engine staying usable: a voice created on another model handle
 * (or already freed); a voice together with ref_audio or ref_text_ids on the same request; an ICL prompt longer than max_prompt
 * (the queue computes the length in its pre-flight check); and for q3tts_generate_queued_voices also audio_chunk_frames > 0 with
 * any non-NULL voice unless sampling->audio_stream_reference is set (a streamed voice row differs from the one-shot clone result
 * in trim and cut, so it is streamed only on request), audio_stream_reference without audio_chunk_frames > 0 and
 * audio_window_frames > 0, and a request that carries ref_audio (as q3tts_generate_queued).
 * q3tts_generate_voices with the streaming fields set treats voice rows as it treats ref_audio rows.
 * Streamed voice requests (audio_stream_reference = 1 with audio_chunk_frames > 0 and audio_window_frames > 0; the arithmetic
 * is defined at q3tts_sampling.audio_window_frames and q3tts_codec_decode_streamed_prefixed): in a static call and in the queue
 * alike a voice row's reference frames go in front of its stream as a prefix that delivers nothing. results[i] is then
 * bit-identical to q3tts_generate of reqs[i] alone in its ref_audio form with the same sampling (the flag included) and
 * row_base = sampling->row_base + i; per request the events are TOKEN and AUDIO_CHUNK interleaved, then INFO, then AUDIO. A
 * voice is read-only, so what its reference leaves in the decoder's causal tail depends on the voice, on (audio_chunk_frames,
 * audio_window_frames, audio_lookahead_frames) and on the codec kernels in use alone: the queue decodes the prefix at the first
 * admission that streams the voice with that geometry, keeps the state on the device beside the voice, and every later
 * admission -- any slot, lane or call -- puts it back with one launch instead of decoding the reference again. A state is the
 * tail's history margin of every tensor a causal conv reads back into -- 3 frames of each for the shipped decoder geometry, so
 * 3 x the summed frame bytes of those tensors per (voice, geometry), the float16 tensors of a float16 speech tokenizer at half
 * the fp32 size (q3tts_debug_prefix_states reports the bytes held); it is not part of q3tts_voice_info.device_bytes, whose
 * formula stands, and goes with the voice in q3tts_voice_free. A prefix whose activations left the fp16 range of the default kernels is not kept: its request
 * is held from its first chunk and decoded again on the fp32 matrix cores like any held streamed request -- one shot over
 * reference ++ generated, cut at R * 1920, untrimmed. Q3TTS_NO_PREFIX_CACHE=1 decodes every prefix anew (same samples). */
typedef struct q3tts_voice q3tts_voice;
q3tts_status q3tts_voice_create(q3tts_model* m, const float* ref_audio, int64_t n_ref_samples, const int32_t* ref_text_ids,
                                int32_t n_ref_text_ids, q3tts_voice** out);
/* The same for a clip at `sample_rate` Hz (8000, 12000, 16000, 22050, 32000, 44100 or 48000; 24000 is q3tts_voice_create): the
 * clip is uploaded at its own rate, resampled to 24 kHz on the device -- the centred form of "Sample rates" below, no delay, no
 * clip -- and handed to the same front end. What q3tts_voice_create(q3tts_resample(clip)) gives, without the round trip.
 * Another rate is Q3TTS_ERR_INVALID_INPUT. q3tts_voice_info.n_ref_samples counts 24 kHz samples: ceil(n * 24000 / rate). */
q3tts_status q3tts_voice_create_rate(q3tts_model* m, const float* ref_audio, int64_t n_ref_samples, int32_t sample_rate,
                                     const int32_t* ref_text_ids, int32_t n_ref_text_ids, q3tts_voice** out);
void q3tts_voice_free(q3tts_model* m, q3tts_voice* v);
typedef struct {
    int32_t ref_frames, ref_text_tokens;
    int64_t n_ref_samples, device_bytes; /* n_ref_samples: of the 24 kHz clip the encoders saw */
} q3tts_voice_info;
q3tts_status q3tts_voice_get_info(const q3tts_voice* v, q3tts_voice_info* out);
q3tts_status q3tts_generate_voices(q3tts_model* m, const q3tts_request* reqs, const q3tts_voice* const* voices, int32_t n_reqs,
                                   const q3tts_sampling* sampling, q3tts_event_cb cb, void* user, q3tts_result* results);
q3tts_status q3tts_generate_queued_voices(q3tts_model* m, const q3tts_request* reqs, const q3tts_voice* const* voices,
                                          int32_t n_reqs, int32_t slots, const q3tts_sampling* sampling, q3tts_event_cb cb,
                                          void* user, q3tts_result* results);

/* Serving session (new: the reference generates one utterance per call). q3tts_generate_queued takes its whole request list up
 * front; a session is the same slot loop with an open end: requests are submitted, cancelled and collected one by one while the
 * loop runs. The frame step, the admission prefill and the decoder are the closed queue's.
 * Tickets and determinism: the t-th ACCEPTED submit (t = 0, 1, ...) gets ticket t, and its result is bit-identical -- status,
 * codes, pcm, n_frames, n_samples -- to q3tts_generate (q3tts_generate_voices for a voice) of that request alone with the
 * session's sampling, `rs` folded in, and row_base = sampling->row_base + t: whatever its arrival time, its slot, what else was
 * running, whether the session was idle before it, and whatever was cancelled around it. Equivalently it is results[t] of
 * q3tts_generate_queued[_voices] over the same requests in ticket order. The streamed forms carry over, each request as if
 * streamed alone: audio_chunk_frames > 0 with audio_window_frames > 0, and audio_stream_reference for voices, whose saved
 * prefix states are reused as the closed queue reuses them. Events carry request_index = ticket (an int32: a session refuses
 * submits past ticket 2^31 - 1) and are otherwise the closed queue's.
 * Threads: q3tts_session_open starts one thread that the session owns. It runs the slot loop, and the event callbacks fire on
 * it. submit, cancel, wait and get_stats may be called from any thread, concurrently: the session has a lock of its own and the
 * one-caller-per-handle rule does not apply to them. submit and cancel may also be called from inside an event callback; they
 * never wait for the loop. wait and close from inside a callback would wait for the thread they run on and are refused
 * (INVALID_INPUT). open and close follow the one-caller-per-handle rule; no other session call may be running when close is.
 *   q3tts_session_open: `slots` rows in flight, 1..max_batch. `max_pending`: accepted requests not yet admitted that the session
 *     holds (0: 1024). `max_ref_frames`: the longest voice reference (frames) a submit may name; it sizes the voice rows of an
 *     admission and, streamed, the stream's code rows once, here, so that no boundary allocates; 0: no voice requests. `sampling`
 *     (NULL: defaults) holds for the whole session; per_request is ignored (a submit brings its own `rs`). Refused with
 *     INVALID_INPUT: slots outside 1..max_batch, a q3tts_generate_begin job outstanding, a session already open, the streaming
 *     fields a closed queue refuses, and, for now, a handle loaded with n_streams > 1 (lanes are not done).
 *   q3tts_session_submit: checks the request on the calling thread exactly as q3tts_generate_queued checks each of its requests
 *     (route, speaker, prompt length, max_tokens <= max_frames, RoPE range; ref_audio is refused; a voice must belong to the handle
 *     and have ref_frames <= max_ref_frames; `rs`, or NULL, gets the checks of q3tts_sampling.per_request). A refused submit
 *     consumes no ticket and leaves the session running. Q3TTS_ERR_BUSY when max_pending requests are waiting. The request and
 *     everything it points at are copied before submit returns. While rows are running the request is admitted at the next
 *     burst boundary; an idle session's thread sleeps on a condition variable -- no frame step, no spinning -- until a submit.
 *   q3tts_session_cancel: a pending ticket is never admitted. A running one leaves its slot at the next burst boundary (one
 *     launch marks the row finished and inactive on the device) and the slot is refilled like any freed slot; from that boundary
 *     on no event fires for the ticket, a streamed request's chunks in flight are dropped, and its result has status
 *     Q3TTS_ERR_CANCELLED and no codes or pcm. A ticket whose row has already been retired completes as it is. Cancelling a
 *     completed or cancelled ticket returns OK and changes nothing; a ticket never given out is INVALID_INPUT. No other
 *     ticket's result changes.
 *   q3tts_session_wait: timeout_ms < 0 waits for ever. *ready = 1: the result is the caller's (q3tts_result_free) and the ticket
 *     is forgotten -- a second wait on it is INVALID_INPUT. *ready = 0 (timeout): nothing is touched. The session holds a result
 *     until it is waited for or the session is closed.
 *   q3tts_session_get_stats: submitted = tickets given out; pending = accepted, not admitted; running = admitted, result not
 *     filled yet; completed / cancelled = results filled with any other status / with CANCELLED; frame_steps and admissions
 *     count since open.
 *   q3tts_session_close: drain != 0 finishes everything accepted; drain == 0 cancels everything pending and running. Either way
 *     it joins the thread and frees the unclaimed results, and the pointer is dead. q3tts_model_free closes an open session
 *     first, without drain, and the pointer is dead after it as well: as with close, no other session call may be running, or
 *     be started later, on a session that is being closed or whose model is being freed (such a call reads freed memory; it
 *     is not answered with INVALID_INPUT). A server stops its submitting threads before it frees the model.
 * While a session is open every other entry point that uses the engine (q3tts_generate*, q3tts_generate_begin, q3tts_codec_*,
 * q3tts_voice_create / _free, q3tts_speaker_embedding, q3tts_debug_*, the arena calls) returns INVALID_INPUT ("a session is open")
 * without touching the GPU, and the session goes on: voices are created before open (or by the session itself: "Live voices"
 * below). q3tts_model_get_info, q3tts_last_error,
 * q3tts_voice_get_info, the tokenizer and q3tts_last_timing stay available.
 * q3tts_last_error and the session calls: a submit, cancel, wait or get_stats that is refused keeps its message for the thread
 * that made the call. q3tts_last_error(model) on that thread returns it until the thread's next call on the handle or session
 * succeeds; other threads' refusals, which may happen at the same moment, do not disturb it, and the handle's own message (that
 * of open, close and every other entry point) is not touched by them.
 * Failure: a device error on the loop thread completes every pending and running ticket with that status; submit and close
 * return it from then on, and q3tts_last_error carries the message (after submit: on the submitting thread, as above). */
typedef struct q3tts_session q3tts_session;
typedef struct {
    int32_t slots;          /* rows in flight, 1..max_batch */
    int32_t max_pending;    /* accepted but not yet admitted requests the session holds; 0 = default (1024) */
    int32_t max_ref_frames; /* longest voice reference (frames) a submit may name; 0 = no voice requests */
} q3tts_session_opts;
typedef struct {
    int64_t submitted, pending, running, completed, cancelled;
    int64_t frame_steps, admissions; /* since open */
} q3tts_session_stats;
q3tts_status q3tts_session_open(q3tts_model* m, const q3tts_session_opts* opts, const q3tts_sampling* sampling, q3tts_event_cb cb,
                                void* user, q3tts_session** out);
q3tts_status q3tts_session_submit(q3tts_session* s, const q3tts_request* req, const q3tts_voice* voice /* or NULL */,
                                  const q3tts_row_sampling* rs /* or NULL */, int64_t* ticket);
q3tts_status q3tts_session_cancel(q3tts_session* s, int64_t ticket);
q3tts_status q3tts_session_wait(q3tts_session* s, int64_t ticket, int32_t timeout_ms /* <0: for ever */, q3tts_result* out,
                                int32_t* ready);
q3tts_status q3tts_session_get_stats(const q3tts_session* s, q3tts_session_stats* out);
q3tts_status q3tts_session_close(q3tts_session* s, int32_t drain);

/* Open-text requests (new): a request whose text arrives while it is being spoken -- a voice agent whose text comes out of a
 * language model token by token. The model does not need the text early: on the generate / CustomVoice / VoiceDesign routes the
 * prompt holds only the first content token (Qwen3.swift:371-406) and every later one is consumed one per frame (:919-935).
 * Contract: the result of an open-text ticket t is bit-identical -- status, codes, pcm, n_frames, n_samples -- to q3tts_generate of
 * the ORDINARY request alone: the same role tokens, all the content tokens that were submitted and appended, any 5 tail tokens,
 * target_token_count = the number of content tokens, the same sampling, row_base = sampling->row_base + t. This holds whatever
 * the timing: text that all arrived before the admission, text appended from a TOKEN callback, text appended after the row had
 * run dry, any number of pieces of any sizes. The streamed forms carry over as for every session request.
 * Starvation: a row that needs a text row that has not arrived, and whose text is still open, starves: the frame in flight
 * completes (its codes count, its TOKEN fires), and then the row forms no next input, takes no frame step, draws no random number
 * and appends nothing to its cache until text arrives; it resumes at the first burst boundary after that with exactly the input
 * the ordinary request would have formed. It never falls back to tts_pad, which is the reference's input for text that has ENDED.
 * Streamed chunks that are decodable leave while a row is starved. When every running row is starved and nothing can be admitted
 * the session thread sleeps on its condition variable like an idle session -- no frame step, no spinning -- until an append, a
 * cancel, a submit or close.
 *   q3tts_session_submit_open: text_ids = the 3 role tokens + >= 1 content tokens and NO 5-token tail (n_text_ids >= 4);
 *     target_token_count is ignored. Every check of q3tts_session_submit for a request without a voice applies; ref_audio is
 *     refused as there, and so is a voice, which this call cannot name (the ICL prompt of a clone holds the whole text,
 *     Qwen3.swift:501-512). max_tokens (0 = 2048) must be <= max_frames: while the text is open it is the row's frame cap, and at
 *     the close the cap becomes the reference's min(max_tokens, max(75, 6 * n_content)) (:822-823) -- which the row cannot have
 *     passed, since starvation keeps its frames <= its content tokens.
 *   q3tts_session_append_text: n >= 0 content token ids behind the ticket's text; final != 0 closes the text (n == 0 with final:
 *     just close). Copied before it returns. Any thread, also from inside an event callback; it never waits for the loop.
 *     INVALID_INPUT, with nothing changed and the session carrying on: a ticket never given out, a ticket from q3tts_session_submit,
 *     a ticket whose text is closed, an id outside the text vocabulary, content beyond the trailing-text capacity (max_prompt rows,
 *     the tts_eos row included: at most max_prompt content tokens), n < 0. A ticket that has completed or was cancelled
 *     already (EOS sampled early, cap hit, cancel): OK, and the text is dropped, as cancel treats a completed ticket -- the race
 *     is inherent. Text for a ticket that is still pending is joined to the stored request; one closed before its admission
 *     is admitted as the ordinary request it now is.
 *   q3tts_session_close(drain != 0) closes every open text first: such a ticket ends as if `final` had been sent. drain == 0 and
 *     q3tts_session_cancel work as for every ticket; a starved row is cancellable.
 *   q3tts_session_get_text_stats: open = tickets accepted whose text is not closed and whose result is not filled; starved =
 *     running rows waiting for text now; appended_tokens = tokens accepted by append_text, starve_events = times a row ran dry,
 *     both since open. */
typedef struct {
    int64_t open, starved, appended_tokens, starve_events;
} q3tts_session_text_stats;
q3tts_status q3tts_session_submit_open(q3tts_session* s, const q3tts_request* req, const q3tts_row_sampling* rs /* or NULL */,
                                       int64_t* ticket);
q3tts_status q3tts_session_append_text(q3tts_session* s, int64_t ticket, const int32_t* ids, int32_t n, int32_t final);
q3tts_status q3tts_session_get_text_stats(const q3tts_session* s, q3tts_session_text_stats* out);

/* Live voices (new): a session that makes voices, and takes ref_audio requests, while it runs -- a voice-clone server adds a
 * speaker without stopping every other speaker's audio. The front end of a clip (upload, the centred resample for a clip at
 * another rate, codec encoder, speaker encoder, prompt rows: what q3tts_voice_create[_rate] runs) is enqueued by the loop thread
 * on one of `live_voices` streams of its own, beside the frame steps, and polled at the burst boundaries; the loop never waits
 * for it while a row is running, and a boundary neither synchronises the device nor allocates or frees device memory for it:
 * the lanes' scratch, their pinned staging and a pool of `max_voices` voice slots are made at open, and in a streamed session
 * (audio_stream_reference) one saved prefix state per slot when the loop starts. A session-made voice keeps at most one saved
 * state -- the first (geometry, speed) it is streamed with; a further one is decoded at every admission -- in its slot's place,
 * which goes to the next voice with the slot: a session's state memory is bounded by max_voices and nothing is allocated or freed
 * for it while the session runs. An anonymous voice (a ref_audio submit) saves none: no other ticket could use it. (A voice made
 * by q3tts_voice_create before open keeps its states in memory of their own, allocated at its first streamed admission, as
 * before.)
 * Contract: a session-made voice holds the very bits q3tts_voice_create[_rate] gives for the same clip, text and rate on this
 * handle, whatever ran beside its front end. So ticket t stays bit-identical to the request generated alone at row_base + t,
 * whether it names a session-made voice (reference: q3tts_generate_voices with an ordinary voice of the clip) or brought its
 * clip as ref_audio (reference: q3tts_generate of that request), streamed forms included. A ticket whose voice is not ready is
 * not admitted and does not hold back the tickets behind it; without such tickets, admission order stays ticket order.
 *   q3tts_session_open_ex: q3tts_session_open with `live_voices` front-end jobs in flight at most (0..4; 0: exactly the session
 *     q3tts_session_open gives, which passes 0) and `max_voices` session-made voices alive at once, anonymous ones included
 *     (0: 4 * slots). base.max_ref_frames bounds a clip as it bounds a voice and must be > 0 with live_voices > 0. live_voices > 0
 *     on a model without the speech-tokenizer encoder: MODEL_NOT_INITIALIZED. Otherwise INVALID_INPUT as q3tts_session_open.
 *   q3tts_session_voice_create: any thread, also from inside an event callback; it never waits for the loop. Every host check
 *     of q3tts_voice_create[_rate] runs on the calling thread, and encoded_frames(samples at 24 kHz) <= max_ref_frames. The
 *     clip and the text ids are copied, and the handle returned at once is a voice from that moment: q3tts_voice_get_info
 *     answers (ref_frames, n_ref_samples and device_bytes are known on the host) and q3tts_session_submit may name it.
 *     Q3TTS_ERR_BUSY: live_voices jobs are waiting or running, or max_voices voices are alive. INVALID_INPUT on a session opened
 *     without live_voices. A refused call leaves the session running.
 *   q3tts_session_voice_wait: blocks until the voice's front end is done; *ready = 0 on timeout (timeout_ms < 0: for ever).
 *     Refused inside a callback, like q3tts_session_wait. Q3TTS_ERR_CANCELLED: the job was abandoned by a close without drain.
 *   q3tts_session_voice_free: any thread. The voice can be named no more; its slot and its saved prefix states are released
 *     at the first boundary at which no pending or running ticket names it, and the tickets already accepted complete unchanged.
 *   q3tts_session_submit with ref_audio / ref_text_ids on a session with live_voices > 0: accepted (24 kHz, as q3tts_request says).
 *     The session makes an anonymous voice for the ticket -- it counts against both limits -- and frees it when the ticket
 *     retires, is cancelled, or the session closes. Streamed: the rules of voice rows (audio_stream_reference). With
 *     live_voices == 0 the refusal stands as it was.
 *   q3tts_session_get_voice_stats: created = voices accepted since open (anonymous ones included), ready = front ends finished,
 *     in_flight = jobs waiting or running now, alive = voices holding a slot now, deferred_frees = q3tts_session_voice_free calls
 *     that could not release at once, anonymous = voices made for ref_audio submits, frontend_ms_sum = the jobs' device time by
 *     their lanes' events, frame_steps_beside = frame steps of the bursts during which at least one job was in flight (in flight
 *     when the burst was launched, or launched while it ran), burst_ms_beside / burst_ms_alone = the loop thread's time from
 *     launching a burst to seeing it finished, summed over those bursts / over all the others.
 * Lifetime: a ready session-made voice is an ordinary voice of the handle. After q3tts_session_close it may be passed to
 * q3tts_generate_voices, q3tts_generate_queued_voices, a later session and q3tts_voice_free; q3tts_model_free releases what is
 * left. Close with drain finishes the accepted jobs. Close without drain lets launched jobs finish (they are short) and abandons
 * the others: such a voice is refused wherever a voice is named (INVALID_INPUT) and still has to be freed. q3tts_voice_create /
 * _free stay refused while a session is open. */
typedef struct {
    q3tts_session_opts base;
    int32_t live_voices; /* front-end jobs in flight, 0..4; 0 = no live voices */
    int32_t max_voices;  /* session-made voices alive at once; 0 = 4 * slots */
} q3tts_session_opts_ex;
typedef struct {
    int64_t created, ready, in_flight, alive, deferred_frees, anonymous;
    double frontend_ms_sum;
    int64_t frame_steps_beside;
    double burst_ms_beside, burst_ms_alone; /* host time of the bursts counted in frame_steps_beside / of all the others */
} q3tts_session_voice_stats;
q3tts_status q3tts_session_open_ex(q3tts_model* m, const q3tts_session_opts_ex* opts, const q3tts_sampling* sampling, q3tts_event_cb cb,
                                   void* user, q3tts_session** out);
q3tts_status q3tts_session_voice_create(q3tts_session* s, const float* ref_audio, int64_t n_ref_samples, int32_t sample_rate,
                                        const int32_t* ref_text_ids, int32_t n_ref_text_ids, q3tts_voice** out);
q3tts_status q3tts_session_voice_wait(q3tts_session* s, const q3tts_voice* v, int32_t timeout_ms /* <0: for ever */, int32_t* ready);
q3tts_status q3tts_session_voice_free(q3tts_session* s, q3tts_voice* v);
q3tts_status q3tts_session_get_voice_stats(const q3tts_session* s, q3tts_session_voice_stats* out);

/* ---- Sample rates (new: the reference speaks and hears 24 kHz only) -----------------------------------------------------
 * One polyphase FIR serves the output side (q3tts_load_opts.output_sample_rate) and the input side (q3tts_voice_create_rate,
 * q3tts_resample). Supported pairs: one side is 24000, the other 8000, 12000, 16000, 22050, 32000, 44100 or 48000.
 * For in -> out Hz: g = gcd(in, out), L = out / g, M = in / g, s = 0.945 * min(1, L / M), half width K = ceil(16 / s) input
 * samples (17 .. 51), 2K taps per phase. Tap i (0 .. 2K-1) of phase r (0 .. L-1) belongs to k = i - K + 1 and sits at
 * t = k - r / L:   g(t) = s * sinc(s t) * I0(8.6 * sqrt(1 - (t / K)^2)) / I0(8.6) for |t| < K, otherwise 0, with
 * sinc(x) = sin(pi x) / (pi x); computed in double, each phase normalised to sum 1 in double, then rounded to fp32.
 * Output sample n has q = floor(n M / L) and r = (n M) mod L:
 *     centred: y[n] = sum_i tab[r][i] * x[q - K + 1 + i]          causal: y[n] = sum_i tab[r][i] * x[q - 2K + 1 + i]
 * The causal form is the centred one delayed by K input samples and reads nothing beyond x[q]. Samples outside the signal are
 * zero; the output has ceil(n_in * L / M) samples. The sum runs in fp32 with fmaf, one accumulator, i ascending: every output
 * has one fixed arithmetic order, whatever the launch geometry. 16 zero crossings, Kaiser beta 8.6 and roll-off 0.945 are a
 * design choice: pass-band ripple at most 0.0101 dB up to 0.40 x the lower rate, at least 71.6 dB of attenuation from 0.55 x the
 * lower rate upward, -16 dB at exactly half the lower rate (the transition band straddles Nyquist).
 *
 * q3tts_resample: `in` (host, n_in >= 1 samples at in_rate) through the device kernel to `out` (host, `cap` samples of room);
 * *n_out = ceil(n_in * L / M). centred != 0: the centred form (no delay; what a reference clip gets); 0: the causal form with
 * nothing in front of the clip (what the decoder's output stage computes for a whole utterance, without its clip to [-1, 1]).
 * Q3TTS_ERR_INVALID_INPUT, the engine staying usable: an unsupported pair, a NaN or infinite sample, cap < *n_out (which is
 * still set). One engine entry point like q3tts_codec_decode: one caller per handle, refused while a session is open. */
q3tts_status q3tts_resample(q3tts_model* m, const float* in, int64_t n_in, int32_t in_rate, int32_t out_rate, int32_t centred,
                            float* out, int64_t cap, int64_t* n_out);

/* ---- Speaking rate (new: the reference has none) ---------------------------------------------------------------------------
 * WSOLA in crossfade form at 24 kHz (q3tts_load_opts.speed, q3tts_time_stretch). Analysis hop Ha = 480 (4 per frame), search
 * radius Delta = 240, synthesis hop Hs in [240, 960]: speed = Ha / Hs. Fade f[n] = 0.5 - 0.5 cos(pi (n + 0.5) / Hs), n < Hs,
 * in double, rounded to fp32. Delay D = max(0, Delta + Hs - Ha, Delta + 2 Hs - 2 Ha) in the causal form, 0 in the whole form.
 * Hop m = 0, 1, ...:   cont[n] = x[p_{m-1} + Hs + n], p_{-1} = -D - Hs, d_0 = 0; for m > 0 and d in [-Delta, Delta]
 * c(d) = sum_n cont[n] * x[m Ha + d - D + n] (fp32, one accumulator, fmaf, n ascending); d_m is the best c with the candidates
 * visited as 0, -1, +1, -2, +2, ... and replaced on strictly greater only (ties: smallest |d|, then the negative one; a NaN
 * never wins); p_m = m Ha + d_m - D; y[m Hs + n] = fmaf(f[n], x[p_m + n] - cont[n], cont[n]). Every sample is a convex
 * combination of two input samples, rounded once: the [-1, 1] range of the decoder's output survives. With D as above hop m
 * reads nothing beyond x[m Ha + Ha - 1], so output frame f depends on input up to the end of frame f alone.
 * Causal form: samples in front of the signal are zero, floor(n_in / Ha) hops, floor(n_in / Ha) * Hs samples out; the output
 * is the input delayed by D, so it starts with about D Hs / Ha samples of silence and the last D input samples are lost.
 * Whole form: D = 0, reads behind the end are zero, ceil(n_in / Ha) hops, cut to ceil(n_in Hs / Ha) samples.
 *
 * q3tts_model_get_speed: the handle's effective speed 480 / Hs (1.0: off), Hs (480: off) and D (any pointer may be NULL).
 * q3tts_time_stretch: `in` (host, n_in >= 1 samples at 24 kHz) through the device kernel to `out` (host, `cap` samples of
 * room); Hs is the integer nearest to 480 / speed (ties toward 480; the handle's output rate plays no part; speed 1.0 is
 * Hs = 480, which still aligns and crossfades). causal != 0: the causal form with nothing in front (what the decoder's stage
 * computes for a whole utterance); 0: the whole form. Q3TTS_ERR_INVALID_INPUT, the engine staying usable: speed outside
 * [0.5, 2.0], NaN or infinite (refused before any GPU work), a NaN or infinite sample, n_in above 2^26, cap < *n_out (which
 * is still set). One engine entry point like q3tts_resample: one caller per handle, refused while a session is open. */
q3tts_status q3tts_model_get_speed(const q3tts_model* m, float* effective_speed, int32_t* hs, int32_t* delay_samples);
q3tts_status q3tts_time_stretch(q3tts_model* m, const float* in, int64_t n_in, float speed, int32_t causal, float* out, int64_t cap,
                                int64_t* n_out);

/* ---- Pitch (new) -----------------------------------------------------------------------------------------------------------
 * q3tts_load_opts_ex.pitch, q3tts_pitch_shift: the time stretch above at Hs = Hp followed by the polyphase FIR of "Sample rates"
 * for the ratio L' / M' = (Ho * L) / (Hp * M) reduced -- the same filter definition for any pair of integers: cutoff
 * 0.945 * min(1, L' / M') of the input Nyquist, K' = ceil(16 / that factor) (at most 204), 2K' taps per phase. The decoder uses the
 * causal forms of both; Hp == 480 (for example speed 1.25 with pitch +3.86) runs no stretch stage at all.
 * q3tts_model_get_pitch: the effective shift 12 log2(Hp / Ho) in semitones (0: off), Hp, Ho (equal: off) and the delay of the two
 * stages in output samples, ceil((D(Hp) * Hp / 480 + K') * L' / M') with D of "Speaking rate" (0 when Hp == 480 or off) -- the
 * stretch's D 24 kHz samples are D * Hp / 480 samples in front of the FIR, which adds its K'. Any pointer may be NULL. On a
 * pitched handle q3tts_model_get_speed keeps reporting the speaking rate, 480 / Ho and Ho.
 * q3tts_pitch_shift: `in` (host, n_in >= 1 samples at 24 kHz) through the whole, undelayed forms -- the whole stretch at Hp
 * (Ho = 480), then the centred FIR Hp -> 480, not clipped -- to `out` (host, `cap` samples of room); *n_out =
 * ceil(ceil(n_in * Hp / 480) * L' / M') is always set. Hp == 480 (semitones 0): a copy. Q3TTS_ERR_INVALID_INPUT, the engine
 * staying usable: semitones outside [-12, 12], NaN or infinite; n_in < 1 or > 2^26; non-finite samples; cap too small. One
 * engine entry point like q3tts_time_stretch: one caller per handle, refused while a session is open. A pitch per request and a
 * pitch per q3tts_codec_decode* call are not offered; formant preservation is the option below. */
q3tts_status q3tts_model_get_pitch(const q3tts_model* m, float* effective_semitones, int32_t* hp, int32_t* ho, int32_t* delay_samples);
q3tts_status q3tts_pitch_shift(q3tts_model* m, const float* in, int64_t n_in, float semitones, float* out, int64_t cap, int64_t* n_out);

/* ---- Formant preservation (new) ---------------------------------------------------------------------------------------------
 * q3tts_load_opts_ex2.keep_formants on a handle whose pitch is on (Hp != Ho, output rate 24000). The mid signal y is the
 * resampler's input, Hp samples per hop; hop h covers mid samples [h Hp, (h+1) Hp) and output samples [h Ho, (h+1) Ho). Per hop:
 * a periodic Hann window of 2 Hp samples over y[(h-1) Hp, (h+1) Hp), the fp32 autocorrelation r[0..24], a Gaussian lag window of
 * 60 Hz, r[0] *= 1 + 1e-4, Levinson-Durbin of order 24 in fp32 -> a_h[1..24] (all 0, the hop passing through, when r[0] < 1e-9,
 * a reflection coefficient reaches 1 or the error leaves (0, inf)); e[n] = y[n] + sum_k a_h[k] y[n-k] goes through the
 * resampler (unclipped); z[n] = e'[n] - sum_k a_h[k] z[n-k] over output hop h, pcm = clip(z). The tail is out_conv -> stretch
 * (if Hp != 480) -> analyse / whiten -> resampler -> synthesise + clip; one-shot decodes, lock-step and slotted streams, voices'
 * saved prefix states (which grow by hist * (align16(16 Hp) + align16(96)) bytes: the margins of e and of the filter's state) and
 * the held-request re-decode carry it bit for bit, as they carry the stretch. csrc/formant_plan.h is the definition, summation
 * orders included; kernels/formant.hip equals it bit for bit.
 * q3tts_model_get_keep_formants: *on = 1 when the stage runs on this handle (the option with a pitch that is on), else 0.
 * q3tts_pitch_shift_formants: q3tts_pitch_shift with the stage -- the whole stretch at Hp, analyse + whiten, the centred FIR
 * Hp -> 480, synthesise, not clipped; same arguments, lengths and refusals. Hp == 480: a copy. */
q3tts_status q3tts_model_get_keep_formants(const q3tts_model* m, int32_t* on);
q3tts_status q3tts_pitch_shift_formants(q3tts_model* m, const float* in, int64_t n_in, float semitones, float* out, int64_t cap,
                                        int64_t* n_out);

/* ---- Speaking rate per request (new) ---------------------------------------------------------------------------------------
 * On a handle loaded with q3tts_load_opts.request_speeds a request may set q3tts_request.speed. It then gets, bit for bit, what
 * a handle loaded with speed = that value (and the same output_sample_rate) gives for the request alone -- status, codes,
 * n_frames, pcm, n_samples -- whatever the other rows of the batch speak at; the codes never depend on the speed. Hs is chosen
 * by the rule of q3tts_load_opts.speed with the handle's L / M (the nearest admissible hop, never a refusal for
 * admissibility); 1.0 is Hs = 480: no stretch for that request. Results count in the request's own samples per frame,
 * 4 * Hs * L / M: n_samples follows the end trim count(code0 > 0) * samples_per_frame with it, a voice request's cut likewise.
 * Honoured by q3tts_generate, q3tts_generate_begin / _end, q3tts_generate_queued, q3tts_generate_voices,
 * q3tts_generate_queued_voices, q3tts_session_submit and q3tts_session_submit_open, with the audio delivered whole and with
 * streamed audio (audio_window_frames > 0): every AUDIO_CHUNK of the request -- sample_offset = k * C * its own samples per
 * frame, n_samples, bytes -- is what the request streamed alone on the handle of its speed delivers, whichever request held
 * the slot before; a voice's saved prefix state is kept per hop. NOT BUILT, Q3TTS_ERR_INVALID_INPUT for a request whose hop
 * differs from the handle's: the chunked exact decode (audio_chunk_frames > 0 with audio_window_frames == 0) and streamed audio
 * on a handle with output_sample_rate (the resampler's input margin would need a frame size per row). A request speed whose
 * hop is the handle's own is the handle's path and is accepted everywhere.
 * Q3TTS_ERR_INVALID_INPUT before any GPU work, the engine and the session staying usable: a non-zero speed on a handle without
 * request_speeds; a NaN, an infinity or a value outside [0.5, 2.0]. q3tts_session_submit / _submit_open check on the calling
 * thread. q3tts_codec_decode*, q3tts_time_stretch and the debug entry points take no request and keep the handle's speed.
 *
 * q3tts_request_speed_info: what a request at `speed` gets on this handle (0: the handle's own) -- the effective speed 480 / Hs,
 * Hs, D in 24 kHz samples and the samples per frame at the output rate; any pointer may be NULL. Host arithmetic alone: no
 * engine entry, available while a session is open. On a handle without request_speeds every non-zero speed is refused. */
q3tts_status q3tts_request_speed_info(const q3tts_model* m, float speed, float* effective_speed, int32_t* hs, int32_t* delay_samples,
                                      int32_t* samples_per_frame);

/* Qwen3TTSSpeechTokenizer.decode (Models/SpeechTokenizer.swift:823-836): codes
 * [batch][max_frames][num_code_groups] -> pcm [batch][max_frames*1920] (caller-allocated),
 * audio_lengths[batch] = count(code0 > 0) * 1920. n_frames[b] <= max_frames are the valid rows. Every code of a valid row is
 * a row of its RVQ table: one outside it is Q3TTS_ERR_INVALID_INPUT (checked on the host before anything is uploaded). */
q3tts_status q3tts_codec_decode(q3tts_model* m, const int32_t* codes, const int32_t* n_frames,
                                int32_t batch, int32_t max_frames, float* pcm, int64_t* audio_lengths);

/* The same decode the way a stream produces it (q3tts_sampling.audio_window_frames): chunks of `chunk_frames` frames, the causal
 * tail carrying its state between them, the pre-transformer over [chunk start - window, chunk end + lookahead) -- or, with
 * window < 0, once over all frames, which makes the result bit-identical to q3tts_codec_decode. For tests and for callers that
 * hold a code sequence and want the bounded-latency arithmetic. */
q3tts_status q3tts_codec_decode_streamed(q3tts_model* m, const int32_t* codes, const int32_t* n_frames, int32_t batch,
                                         int32_t max_frames, int32_t chunk_frames, int32_t window, int32_t lookahead, float* pcm);

/* The streamed decode of rows that carry a reference prefix: the arithmetic of a streamed voice-clone row. The reference has no
 * streaming decode; its one-shot clone decode runs over [reference ++ generated] frames and cuts the reference's samples
 * (Qwen3.swift:1178-1199). Row b of `codes` ([batch][max_frames][16]) holds S = ref ++ gen: R = n_prefix[b] reference frames, then
 * n = n_frames[b] generated ones, R + n <= max_frames. With C / W / L = chunk_frames / window / lookahead (window >= 0):
 *   - prefix chunk j covers S[jC, min(R, (j+1)C)); its pre-transformer window is [max(0, jC - W), min(R, (j+1)C + L)) -- the
 *     lookahead stops at R, so the prefix depends on nothing but the reference and (C, W, L); its samples are never delivered;
 *   - generated chunk k covers S[R + kC, min(R + n, R + (k+1)C)); its window is [max(0, R + kC - W), min(R + n, R + (k+1)C + L)),
 *     which reaches back into the reference while kC < W;
 *   - the causal tail runs over the prefix latents, then the generated ones, with carried state; the row's audio is what it
 *     gives from sample R * 1920 on: n * 1920 samples, no end trim, the cut exactly R * 1920.
 * pcm is [batch][Fmax * 1920] with Fmax = max over b of n_frames[b]; row b's first n_frames[b] * 1920 samples are written. It
 * runs through the slotted stream that serves the queue (batch <= max_batch), every row reset at the start, so a row's samples
 * do not depend on the rows beside it; a row with R == 0 is q3tts_codec_decode_streamed of its codes, bit for bit. */
q3tts_status q3tts_codec_decode_streamed_prefixed(q3tts_model* m, const int32_t* codes, const int32_t* n_prefix, const int32_t* n_frames,
                                                  int32_t batch, int32_t max_frames, int32_t chunk_frames, int32_t window,
                                                  int32_t lookahead, float* pcm);

/* Qwen3TTSSpeechTokenizer.encode (Models/SpeechTokenizer.swift:841-846 -> SpeechTokenizerEncoder.swift:1031-1056):
 * 24 kHz mono float32 waveform -> codes [16][*n_frames] int32 (code row major, as the reference returns
 * [1, 16, time]); cap_frames = capacity of `codes` in frames (q3tts_codec_encoded_frames gives the exact count). */
q3tts_status q3tts_codec_encode(q3tts_model* m, const float* audio, int64_t n_samples, int32_t* codes,
                                int32_t cap_frames, int32_t* n_frames);
int32_t q3tts_codec_encoded_frames(const q3tts_model* m, int64_t n_samples);

/* Qwen3TTSModel.extractSpeakerEmbedding(_:sampleRate:) (Models/Qwen3.swift:222-249): log-mel (n_fft 1024, hop 256,
 * 128 mels) -> ECAPA-TDNN (Models/SpeakerEncoder.swift:364-394). out [enc_dim] float32; sample_rate must be 24000
 * (:223-225). */
q3tts_status q3tts_speaker_embedding(q3tts_model* m, const float* audio, int64_t n_samples, int32_t sample_rate,
                                     float* out, int32_t cap);

/* 16-bit PCM as the reference's CLI writes it (Sources/Qwen3TTSDemo/main.swift:134-165): each sample is clamped to
 * [-1, 1], multiplied by 32767 in Float and converted with Int16(_:), i.e. truncated toward zero (:158-162).
 * q3tts_write_wav writes the same 44-byte RIFF/WAVE header (PCM, mono, 16 bit) followed by those samples. Host code. */
void q3tts_pcm_to_int16(const float* pcm, int64_t n_samples, int16_t* out);
q3tts_status q3tts_write_wav(const char* path, const float* pcm, int64_t n_samples, int32_t sample_rate);

/* Text tokeniser: the Qwen2 byte-level BPE that the checkpoints ship as tokenizer.json (or vocab.json + merges.txt),
 * which the reference loads through swift-transformers (`AutoTokenizer.from(modelFolder:)`, Models/Qwen3.swift:1458) and
 * calls at :274-275, :364-365, :448-457, :822. Optional: callers that tokenise themselves never touch it. `path` is a
 * model directory or a tokenizer.json file. encode = tokenizer.encode(text:) (no special tokens are added by the Qwen2
 * post-processor); ids == NULL only counts. Host code, no GPU. */
typedef struct q3tts_tokenizer q3tts_tokenizer;
q3tts_status q3tts_tokenizer_load(const char* path, q3tts_tokenizer** out);
void q3tts_tokenizer_free(q3tts_tokenizer* t);
q3tts_status q3tts_tokenizer_encode(const q3tts_tokenizer* t, const char* utf8, int32_t* ids, int32_t cap, int32_t* n);

/* Timing of the last q3tts_generate / q3tts_codec_decode on this handle, measured with HIP events
 * on the engine's own stream (bench.py's roofline object reads these). */
typedef struct {
    double prefill_ms;
    double decode_ms;       /* all frame steps */
    double codec_ms;
    int32_t frame_steps;    /* frame-step launches in decode_ms */
    int32_t rows;
    int64_t kv_bytes_read;  /* algorithmic KV bytes read over all frame steps */
    double frontend_ms;     /* voice clone: codec encoder + speaker encoder over all rows of the call */
    double first_audio_ms;  /* streamed decode: request in -> first AUDIO_CHUNK samples on the host (0 when nothing streamed) */
    int32_t launches_per_frame_step; /* kernel launches (graph nodes) of ONE frame step at this call's batch size: the chain decode_ms
                                        is made of is frame_steps x this many dependent launches */
} q3tts_timing;
q3tts_status q3tts_last_timing(const q3tts_model* m, q3tts_timing* out);

/* ---------------------------------------------------------------------------------------------
 * Test hooks: block-level entry points used by tests/ to compare each stage with the oracle.
 * Not part of the drop-in surface. All bf16 buffers are raw uint16 bit patterns, host memory.
 * ------------------------------------------------------------------------------------------- */

/* prepareGenerationInputs (Qwen3.swift:259-409). Outputs (caller-allocated, capacities in rows):
 * input_embeds [*n_prompt][H], trailing [*n_trailing][H], tts_pad [H]. */
q3tts_status q3tts_debug_prepare_inputs(q3tts_model* m, const q3tts_request* req,
                                        uint16_t* input_embeds, int32_t cap_prompt, int32_t* n_prompt,
                                        uint16_t* trailing, int32_t cap_trailing, int32_t* n_trailing,
                                        uint16_t* tts_pad);

/* Teacher-forced generation: same kernels as q3tts_generate, but the tokens fed back are
 * forced_codes [n_reqs][n_frames][groups]; per-frame logits are returned:
 * talker_logits [n_reqs][n_frames][V], cp_logits [n_reqs][n_frames][groups-1][Vcp] (either may be
 * NULL). Sampled tokens (what the sampler would have chosen) go to sampled [n_reqs][n_frames][groups]. */
q3tts_status q3tts_debug_generate_forced(q3tts_model* m, const q3tts_request* reqs, int32_t n_reqs,
                                         const q3tts_sampling* sampling, const int32_t* forced_codes,
                                         int32_t n_frames, uint16_t* talker_logits, uint16_t* cp_logits,
                                         int32_t* sampled);

/* sampleToken (Qwen3.swift:130-213) on caller-supplied logits [rows][V] (bf16) with the engine's
 * sampler kernel. seen [rows][V] uint8 may be NULL. */
q3tts_status q3tts_debug_sample(q3tts_model* m, const uint16_t* logits, int32_t rows, int32_t V,
                                const q3tts_sampling* sampling, const uint8_t* seen,
                                int32_t suppress_lo, int32_t suppress_hi, int32_t eos_id,
                                uint32_t row0, uint32_t draw, int32_t* tokens);

/* The talker input a resumed open-text row gets against the one the end of its frame would have formed (q3tts_session_submit_open):
 * tables [16][V][H] bf16 (codec embedding, then the 15 code-predictor tables), codes [16], text_row [H]; H a multiple of 128 up
 * to 4096, V <= 4096. Row 1 of a two-row step runs (0) through the end-of-frame kernel with its text row there, (1) through it
 * with its text open and no row -- it starves -- and (2) from that state through the append launch with text_row as the new
 * text. out_h [3][H], out_ss [3] (the row's sum of squares; -1: not written), out_state [3][8] = n_frames, trailing_idx,
 * n_trailing, finished, active, text_open, starved, cp_len after each. (0) and (2) must agree in every bit of h and ss. The call
 * allocates its own device buffers and frees them; it touches neither the model's weights nor its caches. */
q3tts_status q3tts_debug_text_resume(q3tts_model* m, int32_t H, int32_t V, const uint16_t* tables, const int32_t* codes,
                                     const uint16_t* text_row, uint16_t* out_h, float* out_ss, int32_t* out_state);

/* Skinny bf16 GEMM used by every Linear on the decode path (Talker.swift:183-186,413-415):
 * y[M][N] = x[M][K] W[N][K]^T (+bias), M <= 64. */
q3tts_status q3tts_debug_linear(q3tts_model* m, const uint16_t* x, const uint16_t* W, const uint16_t* bias,
                                int32_t M, int32_t K, int32_t N, uint16_t* y);

/* One launch of the decode attention (csrc/kernels/attn_decode.hip: per-head QK RMSNorm -> RoPE -> KV append -> GQA
 * attention over the paged cache) on caller-supplied buffers, through the product's own launch_attn_decode, so that the
 * (GQA ratio, wide, nt_kv, chunk) dispatch picks the kernel instantiation exactly as a frame step would. The call allocates
 * its own device buffers and frees them; it touches neither the model's weights nor its caches. Every argument is checked
 * on the host (INVALID_INPUT): n_heads / n_kv in 1..4, chunk <= 16, every block-table entry a live position can reach
 * in [0, n_pages), kv_len (or fixed_len) + the live positions <= max_pages * 64 (64 with identity_pages) and <= n_pos,
 * identity_pages implies B <= n_pages.
 *   rows = max(chunk, 1) * B; qkv/out row of chunk element p of batch row b is p * B + b.
 *   kpool / vpool are read (initial contents) and written back WHOLE after the launch, so a caller sees every slot that
 *   was or was not written. out comes back untiled; a row the kernel did not write (padding of a right-aligned chunk)
 *   holds 0xFFFF in every element. */
typedef struct {
    int32_t n_heads, n_kv, B;
    float eps, scale;
    int32_t max_pages;       /* block_table columns */
    int32_t fixed_len;       /* >= 0: every row's cache holds this many tokens (kv_len ignored); -1: kv_len */
    int32_t identity_pages;  /* 1: row b owns page b (block_table ignored) */
    int32_t chunk;           /* 0 / 1: one position per row; 2..16: that many consecutive positions per row */
    int32_t chunk_r_base;    /* with chunk_n_prompt: element p of row b is prompt position chunk_r_base + chunk_n_prompt[b] + p */
    int32_t nt_kv;
    int32_t n_pos;           /* rows of the RoPE tables */
    int32_t n_pages;         /* pages of each pool */
    const uint16_t* qkv;             /* [rows][(n_heads + 2 n_kv) * 128] bf16 */
    const uint16_t* qn_w;            /* [128] */
    const uint16_t* kn_w;            /* [128] */
    const uint16_t* rope_cos;        /* [n_pos][128] */
    const uint16_t* rope_sin;
    const int32_t* kv_len;           /* [B] */
    const uint8_t* active;           /* [B] or NULL */
    const int32_t* block_table;      /* [B][max_pages] */
    const int32_t* chunk_n_prompt;   /* [B] or NULL (every chunk element is live) */
    uint16_t* kpool;                 /* in / out [n_pages][n_kv][64][128] */
    uint16_t* vpool;
    uint16_t* out;                   /* out [rows][n_heads * 128] row-major */
} q3tts_attn_debug;
q3tts_status q3tts_debug_attention(q3tts_model* m, const q3tts_attn_debug* a);

/* One launch of the decode GEMM (csrc/kernels/gemm_decode.hip, gemm_prefill.hip) on caller-supplied host buffers, through the
 * product's own launchers -- launch_gemm_skinny, or launch_gemm_skinny_with_norm_rows when a rider is given -- so that
 * skinny_geometry / gemm_tall_takes pick the kernel instantiation exactly as a frame step would. Everything GemmArgs can
 * express can be stated here. The weights are handed over as a checkpoint holds them and tiled by the loader's own
 * launch_tile_weights / launch_tile_int4 with the loader's arguments (csrc/model.cc put_linear; epi 2: gate and up separately,
 * eight rows per tile at tile rows 0 and 8). The call allocates its own device buffers and frees them; it touches neither the
 * model's weights nor its caches. Every argument is checked on the host (INVALID_INPUT) before anything is launched:
 *   K a multiple of 128 up to 8192; N a multiple of 16 (epi 2: of 8, N counts output columns); 1 <= M <= 1024;
 *   16 * xMB >= Mpad (= M rounded up to 16), 16 * yMB >= Mpad, ss_ld >= Mpad; y_cols >= N, a multiple of 8, and of 128 where
 *   y is fragment-major on the device (epi 2, epi 3, y_tiled); epi in {0, 2, 3}; bias / act_silu not with epi 2;
 *   norm: norm_w, ss_in, 1 <= ss_count <= 4096, norm_dim >= 1; rider: 1 <= rider_M <= 16 * rider_MB <= 1024, rider_H a multiple
 *   of 128 up to 4096, rider_ss_count in 1..256 when rider_ss_in is set.
 * The caller sees every activation row-major; the call converts to and from the fragment-major device layouts itself.
 *   x [16 * xMB][K] (rows >= M are uploaded too: the kernels must ignore them);
 *   y [16 * yMB][y_cols] is uploaded whole as the caller filled it and returned whole (the hidden-state form, epi 3, is in
 *   place), and so is ss_out [N / 16][ss_ld] when given: a sentinel shows what was and was not written;
 *   rider_h [16 * rider_MB][rider_H], rider_out the same shape (in / out), rider_ss_out [16 * rider_MB] (in / out) or NULL,
 *   rider_ss_in [rider_ss_count][16 * rider_MB] or NULL.
 * mode 0: the GEMM (rider_M > 0: with the rider; `rode` reports whether the launch carried it -- if not, nothing was launched).
 * mode 1: launch_norm_rows alone on the rider fields (the GEMM fields are ignored).
 * geometry_only != 0: nothing is allocated or launched and no buffer pointer is read; only the geometry outputs are filled
 * from norm / quant / has_bias and the sizes. This works without a GPU and with m == NULL. */
typedef struct {
    int32_t mode, geometry_only;
    int32_t M, K, N;
    int32_t xMB, yMB, ss_ld, y_cols;
    int32_t epi, act_silu, resid, nt_weights, y_tiled;
    int32_t norm, quant, has_bias;   /* which optional operands take part (the pointers below must agree) */
    int32_t ss_count, norm_dim;
    float norm_eps;
    int32_t rider_M, rider_H, rider_MB, rider_ss_count;
    float rider_eps;
    /* outputs */
    int32_t rode;                    /* mode 0 with a rider: 1 when launch_gemm_skinny_with_norm_rows launched */
    int32_t tall;                    /* the tall form takes it: tall_shape 2 (128 x 64) or 3 (64 x 64); the rest is 0 */
    int32_t tall_shape;
    int32_t split, mbw, nw, ch, np, gx, ntw;  /* SkinnyGeom (csrc/kernels.h) */
    int32_t tm;                      /* SkinnyGeom::tm: a gate/up workgroup takes its tiles one by one (fills what was padding) */
    /* inputs */
    const uint16_t* x;
    const void* W;                   /* bf16 [N][K], or uint32 [N][K / 8] with quant; epi 2: the gate matrix */
    const uint16_t* scales;          /* quant: bf16 [N][K / 64] */
    const uint16_t* biases;
    const void* W_up;                /* epi 2: the up matrix, with its scales / biases */
    const uint16_t* scales_up;
    const uint16_t* biases_up;
    const uint16_t* bias;            /* [N] */
    const uint16_t* norm_w;          /* [K] */
    const float* ss_in;              /* [ss_count][ss_ld] */
    const uint16_t* rider_h;
    const uint16_t* rider_w;         /* [rider_H] */
    const float* rider_ss_in;
    /* in / out */
    uint16_t* y;
    float* ss_out;                   /* or NULL */
    uint16_t* rider_out;
    float* rider_ss_out;             /* or NULL */
} q3tts_gemm_debug;
q3tts_status q3tts_debug_gemm(q3tts_model* m, q3tts_gemm_debug* a);

/* One launch of a codec-decoder convolution (csrc/kernels/codec_conv.hip, codec_conv_h1.hip, the out-convs of codec_misc.hip and
 * codec_conv_h1.hip) on caller-supplied host buffers, through the product's own launcher, so that the launcher's dispatch picks
 * the kernel instantiation exactly as a decode would. kind:
 *   0  launch_conv_gemm      split == 0: conv_gemm_kernel (fp32 MFMA); split != 0: the two fp16 planes and row scales are attached
 *                            (conv_gemm_h2_kernel, its prologue form, or conv_pw_h2_kernel for K == 1 without a prologue)
 *   1  launch_resunit        out = x + conv2(act2(conv1(act1(x)))); Cin == N == C, ldx == ldo == C; w conv1 [C][K][C], w2 conv2 [C][C],
 *                            bias / bias2, snake_* = act1, act2_*, post_* [C] for out2
 *   2  launch_conv_gemm_h1   float16 tensors as uint16 bit patterns (x fp32 with x_f32); w, bias hold float16-exact values
 *   3  launch_resunit_h1     kind 1 on float16 tensors (K == 7, C == 96)
 *   4  launch_out_conv       SnakeBeta(snake_*) -> k7 conv Cin -> 1 (w [7][Cin], bias [1]) -> clip: pcm [B][Tmax], nonfinite [B] or NULL
 *   5  launch_out_conv_h1    kind 4 on a float16 tensor (bias optional)
 * Everything ConvGemmArgs, ResUnitArgs, ConvH1Args and ResUnitH1Args (csrc/codec_kernels.h) express can be stated. The weights
 * are handed over as a checkpoint holds them -- fp32 [N][K][Cin] -- and SnakeBeta as raw alpha / beta; the call packs them with
 * the loader's own code (csrc/model.cc pack_conv_h2, pack_conv_h2_perm, pack_conv_h1, pack_conv_h1_perm, snake_params,
 * snake_params_f16). It allocates its own device buffers and frees them; it touches neither the model's weights nor its caches.
 * Buffers, as a streamed decode lays them out: every activation is [B][Tmax][ld] where Tmax counts the ALLOCATION's rows; row 0 of
 * a sequence sits `margin` >= hist rows in (the last `hist` rows in front of it are what a causal conv reads as the previous
 * chunk's last rows; rows in front of those must not be read), batch entry b has frames[b] * ppf valid positions and
 * margin + frames[b] * ppf <= Tmax. pcm [B][Tmax] is indexed like the rows. x, x2 ([Tmax][ldx2], B == 1)
 * and res are uploaded whole; out, out2, pcm and nonfinite are uploaded as the caller filled them and returned whole, so that a
 * sentinel shows what was and was not written. res_is_out != 0: the residual is read from out's device buffer (res is ignored).
 * Every argument is checked on the host (INVALID_INPUT) before anything is launched: the launchers' own conditions
 * ((K - 1) * dil <= 56; Cin, N, ldx, ldo, ldr, ldx2 multiples of 4, for kinds 2 / 3 Cin and ldx of 8; x2 only with B == 1;
 * out2 with post_alpha, post_beta and post_C > 0, a multiple of 4 dividing N; kind 2: K in {1, 2, 7}, x_f32 only with K == 7 and
 * a 128-wide tile; kinds 1 / 3: the fused units' supported (C, K, dil) and out != x), ld >= channels, act in 0..5, pre_act in
 * 0..1, 0 <= shift <= (K - 1) * dil, prologue fields only with kind 0, reflect only where every mirrored index stays inside
 * [0, T) for every row, and the sizes above.
 * geometry_only != 0: nothing is allocated or launched and no buffer is read (pointers only say which operands take part); the
 * geometry outputs are filled from the code the launchers switch on (ConvDispatch). Works without a GPU and with m == NULL. */
typedef struct {
    int32_t kind, geometry_only, split;
    int32_t B, Tmax, ppf, hist, margin;
    int32_t Cin, N, K, dil;
    int32_t ldx, ldo, ldr, ldx2;
    int32_t act, pre_act, shift, reflect, post_C;
    int32_t x_f32, res_is_out;
    /* outputs: the launch (csrc/codec_kernels.h ConvDispatch) */
    int32_t family;                  /* 0 conv_gemm_kernel, 1 conv_gemm_h2_kernel, 2 conv_pw_h2_kernel, 3 resunit_h2_kernel,
                                        4 conv_gemm_h1_kernel, 5 resunit_h1_kernel, 6 out_conv_kernel, 7 out_conv_h1_kernel */
    int32_t BN;                      /* output channels per workgroup */
    int32_t pro, pw_depth, KT, X32, CT2, PT, wdb;  /* the template arguments that apply to the family, else 0 */
    int32_t grid_x, grid_y, grid_z;
    int64_t lds_bytes;               /* dynamic LDS */
    /* inputs */
    const int32_t* frames;           /* [B] */
    const void* x;
    const float* x2;
    const float* w;
    const float* w2;
    const float* bias;
    const float* bias2;
    const float* scale;              /* kind 0: [N] */
    const float* snake_alpha;        /* [Cin]: the prologue (kind 0), act1 (1, 3), the out-conv's SnakeBeta (4, 5) */
    const float* snake_beta;
    const float* act2_alpha;         /* [C], kinds 1 and 3 */
    const float* act2_beta;
    const float* post_alpha;         /* [post_C] (kinds 1, 3: [C]) */
    const float* post_beta;
    const void* res;
    /* in / out */
    void* out;
    void* out2;
    float* pcm;
    int32_t* nonfinite;
} q3tts_conv_debug;
q3tts_status q3tts_debug_conv(q3tts_model* m, q3tts_conv_debug* a);

/* One launch of a non-GEMM row kernel of the codec decoder (csrc/kernels/codec_misc.hip) or of the voice-clone front end
 * (csrc/kernels/voice_frontend.hip) on caller-supplied host buffers, through the product's own launch_* function. The call
 * allocates its own device buffers and frees them; it touches neither the model's weights nor its caches. Read-only operands
 * (in[]) are uploaded whole; every output and in/out buffer (io[]) is uploaded as the caller filled it and returned whole, so
 * that a sentinel shows what was and was not written. Device tables of pointers (cb_rest, cb / c2, RollDesc) are built from
 * offsets the caller gives into one pool; rvq_encode's codebooks are handed over as a checkpoint holds them ([bins][dim]) and
 * transposed with the loader's own code (csrc/model.h transpose_codebook). A slot an op does not name must be NULL; a named
 * slot holds exactly the bytes its shape states ("pool": any whole number of floats) unless marked optional ("?").
 * Per op: p[] and f[] in order, then the in[] and io[] slots in order. Sizes in elements; fp32 unless stated; i32 / i64 = int32_t /
 * int64_t.
 *    0 rvq_gather          p: B, Fmax, code_stride_frames (csf), n_rest, inner, rows_first, rows_rest
 *                          in: codes i32 [B][csf][16], cb_first [rows_first][inner], cb_rest pool, frames i32 [B], first_frame? i32 [B],
 *                          cb_rest offsets i64 [n_rest]; io: out [B][Fmax][2 inner]
 *    1 rmsnorm_f32         p: B, Tmax, ppf, C; f: eps; in: x [B][Tmax][C], w [C], frames i32 [B]; io: out [B][Tmax][C]
 *    2 dwconv_ln           p: B, Tmax, ppf, C, hist, margin; f: eps; in: x [B][Tmax][C], dw_w [C][7], dw_b [C], ln_w [C], ln_b [C],
 *                          frames i32 [B]; io: out [B][Tmax][C]
 *    3 silu_mul_f32        p: B, Tmax, ppf, I; in: gu [B][Tmax][2 I], frames i32 [B]; io: out [B][Tmax][I]
 *    4 attn_full_f32       p: B, Tmax, heads; in: qkv [B][Tmax][3 heads 64], frames i32 [B]; io: out [B][Tmax][heads 64]
 *    5 roll_history        p: B, bstride, keep, chunk; io: buf [(B - 1) bstride + keep + chunk]
 *    6 roll_history_rows   p: B, Tal, hist, chunk, n_desc, only_row; in: desc i64 [n_desc][3], mode? i32 [B], take? i32 [B];
 *                          io: pool, nonfinite? i32 [B]
 *    7 history_state_rows  p: B, Tal, hist, n_desc, row, load; in: desc i64 [n_desc][3]; io: pool, blob pool (bytes), nonfinite? i32 [B]
 *    8 stream_take_chunk   p: B, front_bstride, lat_bstride, latent, max_take, lat_off; in: front [B][front_bstride], off i32 [B],
 *                          take i32 [B]; io: lat [B][lat_bstride]
 *    9 enc_init_conv       p: B, S, C, K, out_bstride; in: audio [B][S], w [C][K], bias [C]; io: out [B][out_bstride]
 *   10 layernorm_f32       p: B, T, C, x_bstride, out_bstride; f: eps; in: x [B][x_bstride], w [C], b [C]; io: out [B][out_bstride]
 *   11 rope_qk_f32         p: B, T, heads; in: cos [T][32], sin [T][32]; io: qkv [B][T][3 heads 64]
 *   12 attn_causal_f32     p: B, T, heads; in: qkv [B][T][3 heads 64]; io: out [B][T][heads 64]
 *   13 rvq_encode          p: B, Tmax, ldx, x_bstride, dim, bins, n_layers, layer0, xcol; in: x [B][x_bstride], valid i32 [B],
 *                          code_off i64 [B], cb pool, c2 pool, cb offsets i64 [n_layers], c2 offsets i64 [n_layers]; io: codes i32 pool
 *   14 log_mel             p: T, ld, nfreq, n_mels; in: spec [T][ld], fb [nfreq][n_mels]; io: out [T][n_mels]
 *   15 time_stats          p: T, C, ld; f: eps; in: x [T][ld]; io: mean [C], std? [C]
 *   16 scale_res           p: T, C, ldx, ldr, ldo; in: x [T][ldx], se [C], res [T][ldr]; io: out [T][ldo]
 *   17 asp_concat          p: T, C; in: x [T][C], mean [C], std [C]; io: out [T][3 C]
 *   18 asp_pool            p: T, C; f: eps; in: att [T][C], x [T][C]; io: pooled [2 C]
 *   19 mask_tail           p: B, Tpad, C, bstride; in: valid i32 [B]; io: x [B][bstride]
 *   20 copy2d_f32          p: T, C, lds, ldd; in: src [T][lds]; io: dst [T][ldd]
 * Layouts as a decode has them. Ops 1-4: batch entry b has frames[b] * ppf valid rows (op 4: frames[b]). Op 2: row 0 of a
 * sequence sits `margin` >= hist rows into the allocation's Tmax rows, margin + frames[b] * ppf <= Tmax; out is laid out the same.
 * Op 5: row b's `keep` margin floats start at b * bstride, its chunk behind them. Ops 6, 7: desc[i] = {offset of tensor i in
 * the pool (floats), frame_floats, state_off (bytes into the blob)}, tensor i is [B][Tal][frame_floats]; mode / take / nonfinite
 * given or NULL as launch_roll_history_rows takes them. Op 8: lat row b starts lat_off floats into its lat_bstride. Op 13: the
 * kernel reads columns xcol .. xcol + dim of x's rows; cb offsets point at [bins][dim] tables in the cb pool, c2 offsets at
 * [bins] in the c2 pool; row b owns codes[code_off[b] .. code_off[b] + (layer0 + n_layers) * valid[b]).
 * Every argument that becomes an address, a grid size or an LDS size is checked on the host before anything is launched
 * (Q3TTS_ERR_INVALID_INPUT): the slot sizes against the strides and counts given; the launchers' own conditions (dwconv_ln
 * C <= 4096, enc_init_conv K <= 17, rvq_encode dim <= 4096, latent % 4, keep % 4, chunk >= hist && Tal == hist + chunk, head width
 * 64 by construction); 16-byte alignment of whatever a kernel loads as float4 (strides, offsets, keep, chunk in whole float4s);
 * off + take inside the front buffer; code ranges disjoint and inside codes; table ranges inside their pools; dynamic LDS
 * (dim, nfreq floats) <= 64 KiB; frames / valid / take / mode / first_frame values inside the buffers they index.
 * check_only != 0 runs only these checks: no GPU is needed and m may be NULL. */
typedef struct {
    int32_t op, check_only;
    int32_t p[16];
    float f[4];
    const void* in[8];
    int64_t in_bytes[8];
    void* io[4];
    int64_t io_bytes[4];
} q3tts_rowop_debug;
q3tts_status q3tts_debug_rowop(q3tts_model* m, q3tts_rowop_debug* a);

/* One launch of a row kernel of the LM side of the frame step (csrc/kernels/sampler.hip, csrc/kernels/lm_misc.hip with the jobs of
 * csrc/kernels/row_jobs.h) on caller-supplied host buffers, through the product's own launch_* function; op 1 with `split` makes
 * two launches. The contract of q3tts_debug_rowop: the call allocates and frees its own device buffers and touches neither weights
 * nor caches nor the engine's loop state; in[] is uploaded whole; every io[] buffer is uploaded as the caller filled it and
 * returned whole, so that a sentinel shows what was and was not written; device tables of pointers (cp_emb[15]) are built from
 * offsets into one caller pool; a slot an op does not name must be NULL; a named slot holds exactly the bytes its shape states
 * ("pool": any whole number of bf16) unless marked optional ("?"). The three record types below are the kernels' own
 * (csrc/kernels.h SamplingParams, AdmitDesc, TextAppendDesc), handed over as they lie in device memory.
 * Per op: p[] by index, then the in[] and io[] slots by index. Sizes in elements; bf16 = raw bits in uint16_t; i32 / u32 / i64 / u8
 * / f32 as named; "tiled MB" = the fragment-major activation layout of csrc/common.h act_tiled_offset with MB row blocks,
 * [MB * 16 * H] elements.
 *    0 sampler             p: 0 B, 1 V, 2 ldl, 3 is_talker, 4 suppress_lo, 5 suppress_hi, 6 eos_id, 7 cb, 8 advance, 9 Fmax,
 *                             10 forced_frames (ff), 11 emb_rows, 12 emb_ld, 13 H (0: no gather), 14 next_MB, 15 next_row0, 16 nss,
 *                             17 next_ss_ld, 18 dump_ld, 19 dump_off
 *                          in: 0 logits bf16 [B][ldl], 1 sp q3tts_lm_sampling_params [B], 2 max_frames? i32 [B], 3 advance_gate? u8 [B],
 *                             4 forced? i32 [B][ff][16], 5 emb bf16 [emb_rows][emb_ld] (H > 0), 6 emb_ss? f32 [emb_rows][nss],
 *                             7 row_key? u32 [B]
 *                          io: 0 n_frames i32 [B], 1 finished u8 [B], 2 active u8 [B], 3 kv_len i32 [B], 4 cur_codes i32 [B][16],
 *                             5 codes i32 [B][Fmax][16] (Fmax > 0), 6 seen? u8 [B][V], 7 sampled? i32 [B][ff][16],
 *                             8 logits_dump? bf16 [B][ff][dump_ld], 9 next_x bf16 tiled next_MB (H > 0),
 *                             10 next_ss: f32 [nss][next_ss_ld] with emb_ss, else next_ss? f32 [B]
 *    1 sampler + frame end the slots of op 0 (a code-predictor draw: is_talker 0, V <= 2048, cb = groups - 1) and those of op 2;
 *                          p: 26 split (0: launch_sampler_with_frame_end; 1: launch_sampler, then launch_frame_end on the same
 *                             arguments), 27 cp_len_is_kv_len (1: io 14 is NULL and the frame end's cp_len is the sampler's
 *                             kv_len, as in the frame step)
 *    2 frame_end           p: 0 B, 20 H, 21 groups, 22 Tmax, 23 hMB, 24 Vt (rows of codec_emb), 25 Vcp (rows of a cp_emb table)
 *                          in: 2 max_frames i32 [B], 8 tables bf16 pool, 9 offsets i64 [groups + 1] (codec_emb [Vt][H], cp_emb[0 ..
 *                             groups - 2] [Vcp][H], tts_pad [H]), 10 trailing bf16 [B][Tmax][H], 11 n_trailing i32 [B],
 *                             12 text_open? u8 [B]
 *                          io: 0 n_frames, 1 finished, 2 active, 4 cur_codes (read only), 11 trailing_idx i32 [B],
 *                             12 h bf16 tiled hMB, 13 ss_out f32 [B], 14 cp_len i32 [B], 15 starved? u8 [B] (with text_open)
 *    3 gather_rows         p: 0 n, 1 rows, 2 ld, 3 dim, 4 ldo, 5 out_MB (0: row-major), 6 map_n
 *                          in: 0 table bf16 [rows][ld], 1 ids i32 [n], 2 token_map? i32 [map_n]; io: 0 out bf16 [n][ldo] or tiled out_MB
 *    4 tile_rows           p: 0 rows, 1 dim, 2 lds, 3 dstMB; in: 0 src bf16 [rows][lds]; io: 0 dst bf16 tiled dstMB
 *    5 untile_rows         p: 0 rows, 1 dim, 2 srcMB, 3 ldd; in: 0 src bf16 tiled srcMB; io: 0 dst bf16 [rows][ldd]
 *    6 add_rows            p: 0 rows, 1 dim, 2 lda, 3 ldb (0: one row for all), 4 ldo
 *                          in: 0 a bf16 [rows][lda], 1 b bf16 [rows][ldb] or [dim]; io: 0 out bf16 [rows][ldo]
 *    7 compose_rows        p: 0 n, 1 dim, 2 proj_rows, 3 ldp, 4 table_rows, 5 ldt, 6 extra_rows, 7 lde, 8 dst_rows, 9 ldd
 *                          in: 0 proj bf16 [proj_rows][ldp], 1 table bf16 [table_rows][ldt], 2 extra? bf16 [extra_rows][lde],
 *                             3 a i32 [n], 4 b i32 [n], 5 dst_row i32 [n]; io: 0 dst bf16 [dst_rows][ldd]
 *    8 ref_embed_rows      p: 0 T, 1 groups, 2 H, 3 ldo, 4 Vt, 5 Vcp
 *                          in: 0 codes i32 [groups][T], 1 tables bf16 pool, 2 offsets i64 [groups]; io: 0 out bf16 [T][ldo]
 *    9 f32_to_bf16         p: 0 n; in: 0 x f32 [n]; io: 0 out bf16 [n]
 *   10 ss_to_table         p: 0 rows, 1 nss, 2 ss_ld; in: 0 ss f32 [nss][ss_ld]; io: 0 dst f32 [rows][nss]
 *   11 copy_rows           p: 0 rows, 1 dim, 2 lds, 3 ldd; in: 0 src bf16 [(rows - 1) lds + dim]; io: 0 dst bf16 [(rows - 1) ldd + dim]
 *   12 prefill_load        p: 0 B, 1 Pmax, 2 step, 3 H, 4 hMB
 *                          in: 0 prompt bf16 [B][Pmax][H], 1 n_prompt i32 [B]; io: 0 h bf16 tiled hMB, 1 ss_out f32 [B], 2 active u8 [B]
 *   13 prefill_chunk_load  p: 0 B, 1 Pmax, 2 r_base, 3 H, 4 hMB, 5 C; in: as op 12; io: 0 h bf16 tiled hMB, 1 ss_out f32 [C B]
 *   14 advance_len         p: 0 B; in: 0 active? u8 [B]; io: 0 kv_len i32 [B]
 *   15 advance_len_chunk   p: 0 B, 1 r_base, 2 C; in: 0 n_prompt i32 [B]; io: 0 kv_len i32 [B]
 *   16 admit_rows          p: 0 k, 1 slots, 2 H, 3 V, 4 Fmax, 5 srcMB, 6 hMB
 *                          in: 0 desc q3tts_lm_admit_desc [k], 1 src_h bf16 tiled srcMB, 2 src_ss f32 [k], 3 src_kv_len i32 [k],
 *                             4 src_n_prompt i32 [k]
 *                          io: 0 h bf16 tiled hMB, 1 ss f32 [slots], 2 kv_len, 3 n_prompt, 4 n_trailing, 5 max_frames, 6 n_frames,
 *                             7 cp_len, 8 trailing_idx (i32 [slots] each), 9 cur_codes i32 [slots][16], 10 codes i32 [slots][Fmax][16],
 *                             11 row_key u32 [slots], 12 sp q3tts_lm_sampling_params [slots], 13 finished u8 [slots], 14 active u8
 *                             [slots], 15 seen u8 [slots][V], 16 text_open? u8 [slots], 17 starved? u8 [slots]
 *   17 text_append_rows    p: 0 k, 1 slots, 2 H, 3 Tmax, 4 groups, 5 hMB, 6 Vt, 7 Vcp, 8 src_rows
 *                          in: 0 desc q3tts_lm_text_desc [k], 1 src bf16 [src_rows][H], 2 eos_row bf16 [H], 3 tables bf16 pool,
 *                             4 offsets i64 [groups + 1] (as op 2), 5 cur_codes i32 [slots][16]
 *                          io: 0 trailing bf16 [slots][Tmax][H], 1 n_trailing i32 [slots], 2 text_open u8 [slots], 3 max_frames i32
 *                             [slots], 4 trailing_idx i32 [slots], 5 h bf16 tiled hMB, 6 ss_out f32 [slots], 7 cp_len i32 [slots],
 *                             8 starved u8 [slots], 9 finished u8 [slots], 10 active u8 [slots]
 *   18 cancel_rows         p: 0 slots, 1 mask bits 0..31, 2 mask bits 32..63, 3 n (length of the two arrays, slots <= n <= 64)
 *                          io: 0 finished u8 [n], 1 active u8 [n]
 * Every argument that becomes an address, a grid size or an index is checked on the host before anything is launched
 * (Q3TTS_ERR_INVALID_INPUT): the slot sizes against the strides and counts given; B, slots and k within 1..64; V <= 4096; H % 8 for
 * what a kernel moves in 16-byte pieces (H, dim, ld*, emb_ld, table offsets) and H % 128 for every tiled buffer; rows of a tiled
 * buffer (B, n, C B, k, slots, next_row0 + B) inside its MB * 16; every value a kernel uses as an index: n_frames >= 0, forced
 * entries and the codes of cur_codes inside the tables they select (op 0 with a gather: emb_rows >= V, any token may be drawn;
 * op 1: V within the last group's table), eos_id in -1 .. V - 1, ids / token_map / a / b / dst_row / codes inside their tables,
 * n_trailing within 0..Tmax and trailing_idx >= 0, n_prompt within 0..Pmax and the prompt position a launch loads below Pmax,
 * slot numbers inside 0..slots and distinct (admit_rows also takes -1: the row is skipped), src_row + n_new <= src_rows and
 * n_new + close <= Tmax (a descriptor that fits on its own but not behind the slot's n_trailing goes through: the kernel skips it),
 * dump_off + V <= dump_ld, next_ss_ld >= next_row0 + B, ss_ld >= rows; table ranges inside their pools.
 * check_only != 0 runs only these checks: no GPU is needed and m may be NULL. */
typedef struct {
    float temperature;
    int32_t top_k;
    float top_p;
    float rep_penalty;
    uint64_t seed;
    uint32_t row0;
    int32_t mask_eos;
} q3tts_lm_sampling_params;
typedef struct {
    int32_t slot, n_trailing, max_frames;
    uint32_t row_key;
    int32_t text_open;
    int32_t pad_;
    q3tts_lm_sampling_params sp;
} q3tts_lm_admit_desc;
typedef struct {
    int32_t slot, src_row, n_new, close, max_frames, pad_;
} q3tts_lm_text_desc;
typedef struct {
    int32_t op, check_only;
    int32_t p[32];
    const void* in[14];
    int64_t in_bytes[14];
    void* io[18];
    int64_t io_bytes[18];
} q3tts_lmop_debug;
q3tts_status q3tts_debug_lmop(q3tts_model* m, q3tts_lmop_debug* a);

/* Codec decoder with intermediate activations (SpeechTokenizer.swift:754-784) for one utterance:
 * stage names: "quantizer","pre_conv","pre_transformer","upsample0","upsample1","init_conv",
 * "block0".."block3". Output is channels-last [T][C] float32; *T,*C receive the shape. */
q3tts_status q3tts_debug_codec_stage(q3tts_model* m, const int32_t* codes, int32_t n_frames,
                                     const char* stage, float* out, int64_t cap_floats, int32_t* T, int32_t* C);

/* The voices' saved tail states (the voices comment above, "streamed voice requests"): how many are held on this handle, their
 * device bytes, and how many admissions have been served from one since the model was loaded (a test hook). */
q3tts_status q3tts_debug_prefix_states(q3tts_model* m, int32_t* n_states, int64_t* device_bytes, int64_t* n_restored);

/* The time stretch kernel on B host rows with a hop per row, in the causal form with nothing in front (a test hook for the
 * per-row path of "Speaking rate per request"; works on any handle). x [B][x_stride] at 24 kHz with lens[b] <= x_stride valid
 * samples, hops[b] in [240, 960] (480 aligns and crossfades like any other hop, as in q3tts_time_stretch; 0: the row is
 * copied). y [B][y_stride] is uploaded as the caller filled it and comes back whole: row b receives floor(lens[b] / 480) *
 * hops[b] samples (lens[b] for a copied row), a row of length 0 nothing. A row that does not fit y_stride, a hop outside the
 * range or B outside 1..4096 is Q3TTS_ERR_INVALID_INPUT. */
q3tts_status q3tts_debug_stretch_rows(q3tts_model* m, const float* x, const int32_t* lens, const int32_t* hops, int32_t B,
                                      int64_t x_stride, float* y, int64_t y_stride);

/* The general-ratio resampler (kernels/resample_ratio.hip) on B host rows, for any pair of positive integers in_units ->
 * out_units (a test hook; works on any handle): the filter of "Pitch" for L' / M' = out_units / in_units reduced. x
 * [B][row_stride]: row b holds `hist` samples in front (read where the filter reaches back beyond the row's first sample; 0:
 * none) and then lens[b] valid samples, hist + lens[b] <= row_stride. centred != 0: the centred form, otherwise the causal one;
 * clamp != 0: the result is clipped to [-1, 1]. y [B][y_stride] is uploaded as the caller filled it and comes back whole: row b
 * receives ceil(lens[b] * L' / M') samples, a row of length 0 nothing. Q3TTS_ERR_INVALID_INPUT: a row that does not fit, B
 * outside 1..4096, a pair whose table exceeds 16 MiB or whose 256-output input span exceeds 64 KiB. */
q3tts_status q3tts_debug_resample_ratio(q3tts_model* m, const float* x, const int32_t* lens, int32_t B, int64_t row_stride, int64_t in_units,
                                        int64_t out_units, int32_t centred, int32_t clamp, int32_t hist, float* y, int64_t y_stride);

/* The two kernels of "Formant preservation" (kernels/formant.hip) on B host rows (a test hook; works on any handle), hops hp and
 * ho in [240, 960]. mode 0: analyse + whiten -- x [B][x_stride], row b holding `hist` samples in front and then lens[b] mid
 * samples; coef [B][coef_stride] receives 24 floats per hop (ceil(lens[b] / hp) hops), y [B][y_stride] the whitened lens[b]
 * samples. mode 1: synthesise with given coefficients -- x rows hold lens[b] samples of e' (hist must be 0), coef is read
 * (ceil(lens[b] / ho) hops), state_in [B][24] (NULL: zeros) is the rows' last 24 values of z in front, state_out [B][24] (NULL:
 * not wanted) those behind, y receives z, clipped to [-1, 1] when clamp != 0. mode 2: both with the identity in between, only
 * when hp == ho -- x as in mode 0, coef written, states as in mode 1, y receives z. coef and y are uploaded as the caller
 * filled them and come back whole; a row of length 0 touches nothing. Q3TTS_ERR_INVALID_INPUT: a mode, hop or B (1..4096) out
 * of range, mode 2 with hp != ho, a row that does not fit its strides, a state given to mode 0, a margin given to mode 1. */
q3tts_status q3tts_debug_formant_rows(q3tts_model* m, int32_t mode, int32_t hp, int32_t ho, const int32_t* lens, int32_t B, const float* x,
                                      int64_t x_stride, int32_t hist, float* coef, int64_t coef_stride, const float* state_in, float* state_out,
                                      float* y, int64_t y_stride, int32_t clamp);

/* The slotted codec stream of a streamed q3tts_generate_queued, driven by the queue's schedule without the talker (a test hook:
 * the real layer widths in seconds). codes [n_reqs][max_frames][16], n_frames[n_reqs] <= max_frames. Requests take the free ones
 * of `slots` rows (1..max_batch) in index order; every running request gains `burst` frames per step; one that reaches its count
 * is final, is retired behind that step's chunks, and its slot is reset and refilled. pcm [n_reqs][max_frames * 1920] receives
 * every request's samples: bit-identical to q3tts_codec_decode_streamed(codes_i, chunk_frames, window, lookahead) of it alone.
 * Codes are checked against the RVQ tables on the host as in q3tts_codec_decode; chunk_frames below the causal tail's history,
 * window < 0 or slots outside 1..max_batch are Q3TTS_ERR_INVALID_INPUT. */
q3tts_status q3tts_debug_codec_stream_slots(q3tts_model* m, const int32_t* codes, const int32_t* n_frames, int32_t n_reqs,
                                            int32_t max_frames, int32_t slots, int32_t burst, int32_t chunk_frames, int32_t window,
                                            int32_t lookahead, float* pcm);

/* build_decode_codes_rows (the one launch that writes the decoder's input [reference ++ generated] for every row of a decode
 * batch) on caller-supplied rows, through the product's launcher. refs: the rows' reference codes one after the other, row r's
 * as [16][ref_T[r]] (ref_T[r] == 0: a row without a reference); gen [R][gen_stride][16] with n_frames[r] <= gen_stride valid
 * frames; out [R][Fdec][16] is uploaded as the caller filled it and comes back whole, so a caller sees what was and was not
 * written (a row with n_frames[r] == 0 writes nothing). misalign != 0 places gen and out 4 bytes off a 16-byte boundary on the
 * device, which takes the launch through its 4-byte loads and stores. ref_T[r] + n_frames[r] > Fdec is Q3TTS_ERR_DEVICE
 * (the launcher's own bounds check). */
q3tts_status q3tts_debug_build_decode_codes(q3tts_model* m, const int32_t* refs, const int32_t* ref_T, const int32_t* gen,
                                            const int32_t* n_frames, int32_t R, int32_t gen_stride, int32_t Fdec, int32_t misalign,
                                            int32_t* out);

/* Activation scratch the codec decoder may use per pass (default 24 GB; 0 restores it): a small value forces the paths that
 * take a large batch through in groups of rows. Process-wide. */
void q3tts_debug_set_codec_scratch(uint64_t bytes);

/* The launchers' diagnostic switches (Q3TTS_GEMM_NO_ROW_SPLIT, Q3TTS_NO_TALL_GEMM, Q3TTS_NT, ...: csrc/kernels.h DebugEnv)
 * are read from the environment once per q3tts_model_load, not per launch; a test that changes one on a live model calls
 * this afterwards. Process-wide; not to be called while a generate call is running. */
void q3tts_debug_reload_env(void);

/* Voice-clone front end with intermediate activations for one waveform. Codec encoder stages
 * (SpeechTokenizerEncoder.swift:1031-1056): "init_conv","layer0".."layer3","seanet","transformer","downsample",
 * "rvq_first_in","rvq_rest_in"; speaker encoder stages (SpeakerEncoder.swift:364-394): "mel","h0".."h3","mfa",
 * "pooled". Output is channels-last [T][C] float32. */
q3tts_status q3tts_debug_frontend_stage(q3tts_model* m, const float* audio, int64_t n_samples, const char* stage,
                                        float* out, int64_t cap_floats, int32_t* T, int32_t* C);

#ifdef __cplusplus
}
#endif
#endif /* Q3TTS_H */
