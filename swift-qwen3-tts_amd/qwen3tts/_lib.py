"""ctypes binding of include/q3tts.h (libq3tts_hip.so). The library is the product; this module
only marshals arguments. It fails loudly when the HIP extension is missing -- there is no CPU
fallback and nothing here touches oracle/."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# Q3TTS_LIB: another build of the same library (A/B measurements of a kernel change inside one gpurun call)
LIB_PATH = os.environ.get("Q3TTS_LIB") or os.path.join(_HERE, "libq3tts_hip.so")

u16p = C.POINTER(C.c_uint16)
i32p = C.POINTER(C.c_int32)
f32p = C.POINTER(C.c_float)
u8p = C.POINTER(C.c_uint8)


class LoadOpts(C.Structure):
    _fields_ = [("device", C.c_int32), ("max_batch", C.c_int32), ("max_frames", C.c_int32),
                ("max_prompt", C.c_int32), ("use_graph", C.c_int32), ("weights_from_broadcast", C.c_int32),
                ("n_streams", C.c_int32), ("codec_overlap_cus", C.c_int32), ("codec_fp32", C.c_int32),
                ("output_sample_rate", C.c_int32), ("speed", C.c_float), ("request_speeds", C.c_int32)]


class LoadOptsEx(C.Structure):  # q3tts_load_opts_ex: the options above and what has been added behind them
    _fields_ = [("base", LoadOpts), ("pitch", C.c_float)]


class LoadOptsEx2(C.Structure):  # q3tts_load_opts_ex2: q3tts_load_opts_ex whole, and what has been added behind it
    _fields_ = [("ex", LoadOptsEx), ("keep_formants", C.c_int32)]


class CommId(C.Structure):  # q3tts_comm_id == ncclUniqueId
    _fields_ = [("bytes", C.c_char * 128)]


class ModelInfo(C.Structure):
    _fields_ = [("tts_model_type", C.c_char * 32), ("sample_rate", C.c_int32),
                ("supports_voice_cloning", C.c_int32), ("has_voice_cloning", C.c_int32),
                ("hidden_size", C.c_int32), ("num_layers", C.c_int32), ("vocab_size", C.c_int32),
                ("text_vocab_size", C.c_int32), ("num_code_groups", C.c_int32),
                ("cp_hidden_size", C.c_int32), ("cp_num_layers", C.c_int32), ("cp_vocab_size", C.c_int32),
                ("codec_eos_token_id", C.c_int32), ("samples_per_frame", C.c_int32), ("max_batch", C.c_int32),
                ("weight_bytes", C.c_int64), ("speaker_embedding_dim", C.c_int32), ("max_samples_per_frame", C.c_int32)]


class Request(C.Structure):
    _fields_ = [("text_ids", i32p), ("n_text_ids", C.c_int32), ("instruct_ids", i32p),
                ("n_instruct_ids", C.c_int32), ("target_token_count", C.c_int32), ("speaker", C.c_char_p),
                ("language", C.c_char_p), ("max_tokens", C.c_int32), ("speed", C.c_float),
                ("ref_audio", f32p), ("n_ref_samples", C.c_int64), ("ref_text_ids", i32p),
                ("n_ref_text_ids", C.c_int32), ("route", C.c_int32)]


ROW_TEMPERATURE, ROW_TOP_K, ROW_TOP_P, ROW_REPETITION_PENALTY, ROW_SEED = 1, 2, 4, 8, 16  # q3tts_row_sampling.set


class RowSampling(C.Structure):  # q3tts_row_sampling
    _fields_ = [("set", C.c_uint32), ("temperature", C.c_float), ("top_k", C.c_int32), ("top_p", C.c_float),
                ("repetition_penalty", C.c_float), ("seed", C.c_uint64)]


class Sampling(C.Structure):
    _fields_ = [("temperature", C.c_float), ("top_k", C.c_int32), ("top_p", C.c_float),
                ("repetition_penalty", C.c_float), ("seed", C.c_uint64), ("force_frames", C.c_int32), ("audio_chunk_frames", C.c_int32),
                ("audio_window_frames", C.c_int32), ("audio_lookahead_frames", C.c_int32), ("row_base", C.c_uint32),
                ("per_request", C.POINTER(RowSampling)), ("audio_stream_reference", C.c_int32)]


class GenInfo(C.Structure):
    _fields_ = [("prompt_token_count", C.c_int32), ("generation_token_count", C.c_int32),
                ("prefill_time", C.c_double), ("generate_time", C.c_double), ("tokens_per_second", C.c_double),
                ("peak_memory_usage", C.c_double)]


class Event(C.Structure):
    _fields_ = [("kind", C.c_int), ("request_index", C.c_int32), ("token", C.c_int32),
                ("info", C.POINTER(GenInfo)), ("pcm", f32p), ("n_samples", C.c_int64), ("sample_offset", C.c_int64)]


EVENT_CB = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(Event))


class Result(C.Structure):
    _fields_ = [("status", C.c_int), ("pcm", f32p), ("n_samples", C.c_int64), ("codes", i32p),
                ("n_frames", C.c_int32), ("info", GenInfo)]


class Timing(C.Structure):
    _fields_ = [("prefill_ms", C.c_double), ("decode_ms", C.c_double), ("codec_ms", C.c_double),
                ("frame_steps", C.c_int32), ("rows", C.c_int32), ("kv_bytes_read", C.c_int64),
                ("frontend_ms", C.c_double), ("first_audio_ms", C.c_double), ("launches_per_frame_step", C.c_int32)]


class VoiceInfo(C.Structure):  # q3tts_voice_info
    _fields_ = [("ref_frames", C.c_int32), ("ref_text_tokens", C.c_int32), ("n_ref_samples", C.c_int64),
                ("device_bytes", C.c_int64)]


class SessionOpts(C.Structure):  # q3tts_session_opts
    _fields_ = [("slots", C.c_int32), ("max_pending", C.c_int32), ("max_ref_frames", C.c_int32)]


class SessionStats(C.Structure):  # q3tts_session_stats
    _fields_ = [("submitted", C.c_int64), ("pending", C.c_int64), ("running", C.c_int64), ("completed", C.c_int64),
                ("cancelled", C.c_int64), ("frame_steps", C.c_int64), ("admissions", C.c_int64)]


class SessionOptsEx(C.Structure):  # q3tts_session_opts_ex
    _fields_ = [("base", SessionOpts), ("live_voices", C.c_int32), ("max_voices", C.c_int32)]


class SessionVoiceStats(C.Structure):  # q3tts_session_voice_stats
    _fields_ = [("created", C.c_int64), ("ready", C.c_int64), ("in_flight", C.c_int64), ("alive", C.c_int64),
                ("deferred_frees", C.c_int64), ("anonymous", C.c_int64), ("frontend_ms_sum", C.c_double),
                ("frame_steps_beside", C.c_int64), ("burst_ms_beside", C.c_double), ("burst_ms_alone", C.c_double)]


class SessionTextStats(C.Structure):  # q3tts_session_text_stats
    _fields_ = [("open", C.c_int64), ("starved", C.c_int64), ("appended_tokens", C.c_int64), ("starve_events", C.c_int64)]


ERR_CANCELLED, ERR_BUSY = 8, 9  # q3tts_status: a cancelled request's result; submit with max_pending requests waiting


class AttnDebug(C.Structure):  # q3tts_attn_debug
    _fields_ = [("n_heads", C.c_int32), ("n_kv", C.c_int32), ("B", C.c_int32), ("eps", C.c_float), ("scale", C.c_float),
                ("max_pages", C.c_int32), ("fixed_len", C.c_int32), ("identity_pages", C.c_int32), ("chunk", C.c_int32),
                ("chunk_r_base", C.c_int32), ("nt_kv", C.c_int32), ("n_pos", C.c_int32), ("n_pages", C.c_int32),
                ("qkv", u16p), ("qn_w", u16p), ("kn_w", u16p), ("rope_cos", u16p), ("rope_sin", u16p),
                ("kv_len", i32p), ("active", u8p), ("block_table", i32p), ("chunk_n_prompt", i32p),
                ("kpool", u16p), ("vpool", u16p), ("out", u16p)]


class GemmDebug(C.Structure):  # q3tts_gemm_debug
    _fields_ = [("mode", C.c_int32), ("geometry_only", C.c_int32), ("M", C.c_int32), ("K", C.c_int32), ("N", C.c_int32),
                ("xMB", C.c_int32), ("yMB", C.c_int32), ("ss_ld", C.c_int32), ("y_cols", C.c_int32),
                ("epi", C.c_int32), ("act_silu", C.c_int32), ("resid", C.c_int32), ("nt_weights", C.c_int32), ("y_tiled", C.c_int32),
                ("norm", C.c_int32), ("quant", C.c_int32), ("has_bias", C.c_int32), ("ss_count", C.c_int32), ("norm_dim", C.c_int32),
                ("norm_eps", C.c_float),
                ("rider_M", C.c_int32), ("rider_H", C.c_int32), ("rider_MB", C.c_int32), ("rider_ss_count", C.c_int32),
                ("rider_eps", C.c_float),
                ("rode", C.c_int32), ("tall", C.c_int32), ("tall_shape", C.c_int32),
                ("split", C.c_int32), ("mbw", C.c_int32), ("nw", C.c_int32), ("ch", C.c_int32), ("np", C.c_int32), ("gx", C.c_int32),
                ("ntw", C.c_int32), ("tm", C.c_int32),
                ("x", u16p), ("W", C.c_void_p), ("scales", u16p), ("biases", u16p), ("W_up", C.c_void_p), ("scales_up", u16p),
                ("biases_up", u16p), ("bias", u16p), ("norm_w", u16p), ("ss_in", f32p), ("rider_h", u16p), ("rider_w", u16p),
                ("rider_ss_in", f32p),
                ("y", u16p), ("ss_out", f32p), ("rider_out", u16p), ("rider_ss_out", f32p)]


class ConvDebug(C.Structure):  # q3tts_conv_debug
    _fields_ = [("kind", C.c_int32), ("geometry_only", C.c_int32), ("split", C.c_int32),
                ("B", C.c_int32), ("Tmax", C.c_int32), ("ppf", C.c_int32), ("hist", C.c_int32), ("margin", C.c_int32),
                ("Cin", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("dil", C.c_int32),
                ("ldx", C.c_int32), ("ldo", C.c_int32), ("ldr", C.c_int32), ("ldx2", C.c_int32),
                ("act", C.c_int32), ("pre_act", C.c_int32), ("shift", C.c_int32), ("reflect", C.c_int32), ("post_C", C.c_int32),
                ("x_f32", C.c_int32), ("res_is_out", C.c_int32),
                ("family", C.c_int32), ("BN", C.c_int32), ("pro", C.c_int32), ("pw_depth", C.c_int32), ("KT", C.c_int32),
                ("X32", C.c_int32), ("CT2", C.c_int32), ("PT", C.c_int32), ("wdb", C.c_int32),
                ("grid_x", C.c_int32), ("grid_y", C.c_int32), ("grid_z", C.c_int32), ("lds_bytes", C.c_int64),
                ("frames", i32p), ("x", C.c_void_p), ("x2", f32p), ("w", f32p), ("w2", f32p), ("bias", f32p), ("bias2", f32p),
                ("scale", f32p), ("snake_alpha", f32p), ("snake_beta", f32p), ("act2_alpha", f32p), ("act2_beta", f32p),
                ("post_alpha", f32p), ("post_beta", f32p), ("res", C.c_void_p),
                ("out", C.c_void_p), ("out2", C.c_void_p), ("pcm", f32p), ("nonfinite", i32p)]


class RowopDebug(C.Structure):  # q3tts_rowop_debug
    _fields_ = [("op", C.c_int32), ("check_only", C.c_int32), ("p", C.c_int32 * 16), ("f", C.c_float * 4),
                ("in", C.c_void_p * 8), ("in_bytes", C.c_int64 * 8), ("io", C.c_void_p * 4), ("io_bytes", C.c_int64 * 4)]


ROWOPS = ("rvq_gather", "rmsnorm_f32", "dwconv_ln", "silu_mul_f32", "attn_full_f32", "roll_history", "roll_history_rows",
          "history_state_rows", "stream_take_chunk", "enc_init_conv", "layernorm_f32", "rope_qk_f32", "attn_causal_f32", "rvq_encode",
          "log_mel", "time_stats", "scale_res", "asp_concat", "asp_pool", "mask_tail", "copy2d_f32")  # q3tts_rowop_debug.op


def rowop(handle, op, p, f, ins, ios, check_only=False):
    """q3tts_debug_rowop (the slot table: include/q3tts.h). op: a name of ROWOPS; p / f: the int and float parameters; ins: the
    read-only operands and ios: the in/out buffers, numpy arrays or None, in slot order. The in/out arrays are written in place.
    check_only: the host checks alone (handle may be None; no GPU). Returns the status."""
    a = RowopDebug(op=ROWOPS.index(op), check_only=1 if check_only else 0)
    for i, v in enumerate(p):
        a.p[i] = int(v)
    for i, v in enumerate(f):
        a.f[i] = float(v)
    inp = getattr(a, "in")  # (the header's name is a Python keyword)
    for i, v in enumerate(ins):
        if v is not None:
            assert v.flags["C_CONTIGUOUS"]
            inp[i], a.in_bytes[i] = v.ctypes.data, v.nbytes
    for i, v in enumerate(ios):
        if v is not None:
            assert v.flags["C_CONTIGUOUS"] and v.flags["WRITEABLE"]
            a.io[i], a.io_bytes[i] = v.ctypes.data, v.nbytes
    return lib().q3tts_debug_rowop(handle, C.byref(a))


class LmSamplingParams(C.Structure):  # q3tts_lm_sampling_params (csrc/kernels.h SamplingParams)
    _fields_ = [("temperature", C.c_float), ("top_k", C.c_int32), ("top_p", C.c_float), ("rep_penalty", C.c_float),
                ("seed", C.c_uint64), ("row0", C.c_uint32), ("mask_eos", C.c_int32)]


class LmAdmitDesc(C.Structure):  # q3tts_lm_admit_desc (csrc/kernels.h AdmitDesc)
    _fields_ = [("slot", C.c_int32), ("n_trailing", C.c_int32), ("max_frames", C.c_int32), ("row_key", C.c_uint32),
                ("text_open", C.c_int32), ("pad_", C.c_int32), ("sp", LmSamplingParams)]


class LmTextDesc(C.Structure):  # q3tts_lm_text_desc (csrc/kernels.h TextAppendDesc)
    _fields_ = [("slot", C.c_int32), ("src_row", C.c_int32), ("n_new", C.c_int32), ("close", C.c_int32),
                ("max_frames", C.c_int32), ("pad_", C.c_int32)]


class LmopDebug(C.Structure):  # q3tts_lmop_debug
    _fields_ = [("op", C.c_int32), ("check_only", C.c_int32), ("p", C.c_int32 * 32),
                ("in", C.c_void_p * 14), ("in_bytes", C.c_int64 * 14), ("io", C.c_void_p * 18), ("io_bytes", C.c_int64 * 18)]


LMOPS = ("sampler", "sampler_frame_end", "frame_end", "gather_rows", "tile_rows", "untile_rows", "add_rows", "compose_rows",
         "ref_embed_rows", "f32_to_bf16", "ss_to_table", "copy_rows", "prefill_load", "prefill_chunk_load", "advance_len",
         "advance_len_chunk", "admit_rows", "text_append_rows", "cancel_rows")  # q3tts_lmop_debug.op


def lmop(handle, op, p, ins, ios, check_only=False):
    """q3tts_debug_lmop (the slot table: include/q3tts.h). op: a name of LMOPS; p: {index: value} of the int parameters; ins / ios:
    {slot: numpy array} of the read-only operands and of the in/out buffers. The in/out arrays are written in place.
    check_only: the host checks alone (handle may be None; no GPU). Returns the status."""
    a = LmopDebug(op=LMOPS.index(op), check_only=1 if check_only else 0)
    for i, v in p.items():
        a.p[i] = int(v)
    inp = getattr(a, "in")  # (the header's name is a Python keyword)
    for i, v in ins.items():
        if v is not None:
            assert v.flags["C_CONTIGUOUS"]
            inp[i], a.in_bytes[i] = v.ctypes.data, v.nbytes
    for i, v in ios.items():
        if v is not None:
            assert v.flags["C_CONTIGUOUS"] and v.flags["WRITEABLE"]
            a.io[i], a.io_bytes[i] = v.ctypes.data, v.nbytes
    return lib().q3tts_debug_lmop(handle, C.byref(a))


_lib = None


def lib() -> C.CDLL:
    """Loads libq3tts_hip.so; raises if it has not been built (python __graft_entry__.py build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build the HIP engine first "
                           "(make -C swift-qwen3-tts_amd); there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.q3tts_default_load_opts.argtypes = [C.POINTER(LoadOpts)]
    L.q3tts_default_sampling.argtypes = [C.POINTER(Sampling)]
    L.q3tts_model_load.argtypes = [C.c_char_p, C.POINTER(LoadOpts), C.POINTER(vp)]
    L.q3tts_model_free.argtypes = [vp]
    L.q3tts_model_free.restype = None
    L.q3tts_last_error.argtypes = [vp]
    L.q3tts_last_error.restype = C.c_char_p
    L.q3tts_model_arena.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.q3tts_model_get_info.argtypes = [vp, C.POINTER(ModelInfo)]
    L.q3tts_comm_get_unique_id.argtypes = [C.POINTER(CommId)]
    L.q3tts_model_broadcast.argtypes = [vp, C.POINTER(CommId), C.c_int32, C.c_int32, C.c_int32]
    L.q3tts_model_arena_checksum.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.q3tts_model_num_speakers.argtypes = [vp]
    L.q3tts_model_speaker_name.argtypes = [vp, C.c_int32]
    L.q3tts_model_speaker_name.restype = C.c_char_p
    L.q3tts_generate.argtypes = [vp, C.POINTER(Request), C.c_int32, C.POINTER(Sampling), EVENT_CB, vp,
                                 C.POINTER(Result)]
    L.q3tts_generate_queued.argtypes = [vp, C.POINTER(Request), C.c_int32, C.c_int32, C.POINTER(Sampling), EVENT_CB, vp,
                                        C.POINTER(Result)]
    L.q3tts_voice_create.argtypes = [vp, f32p, C.c_int64, i32p, C.c_int32, C.POINTER(vp)]
    if hasattr(L, "q3tts_resample"):  # (absent from an older build loaded through Q3TTS_LIB for an A/B run)
        L.q3tts_voice_create_rate.argtypes = [vp, f32p, C.c_int64, C.c_int32, i32p, C.c_int32, C.POINTER(vp)]
        L.q3tts_resample.argtypes = [vp, f32p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, f32p, C.c_int64, C.POINTER(C.c_int64)]
    if hasattr(L, "q3tts_time_stretch"):  # (the same)
        L.q3tts_model_get_speed.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.q3tts_time_stretch.argtypes = [vp, f32p, C.c_int64, C.c_float, C.c_int32, f32p, C.c_int64, C.POINTER(C.c_int64)]
    L.q3tts_voice_free.argtypes = [vp, vp]
    L.q3tts_voice_free.restype = None
    L.q3tts_voice_get_info.argtypes = [vp, C.POINTER(VoiceInfo)]
    L.q3tts_generate_voices.argtypes = [vp, C.POINTER(Request), C.POINTER(vp), C.c_int32, C.POINTER(Sampling), EVENT_CB, vp,
                                        C.POINTER(Result)]
    L.q3tts_generate_queued_voices.argtypes = [vp, C.POINTER(Request), C.POINTER(vp), C.c_int32, C.c_int32, C.POINTER(Sampling),
                                               EVENT_CB, vp, C.POINTER(Result)]
    if hasattr(L, "q3tts_session_open"):  # (absent from an older build loaded through Q3TTS_LIB for an A/B run)
        L.q3tts_session_open.argtypes = [vp, C.POINTER(SessionOpts), C.POINTER(Sampling), EVENT_CB, vp, C.POINTER(vp)]
        L.q3tts_session_submit.argtypes = [vp, C.POINTER(Request), vp, C.POINTER(RowSampling), C.POINTER(C.c_int64)]
        L.q3tts_session_cancel.argtypes = [vp, C.c_int64]
        L.q3tts_session_wait.argtypes = [vp, C.c_int64, C.c_int32, C.POINTER(Result), i32p]
        L.q3tts_session_get_stats.argtypes = [vp, C.POINTER(SessionStats)]
        L.q3tts_session_close.argtypes = [vp, C.c_int32]
    if hasattr(L, "q3tts_session_open_ex"):  # (absent from an older build loaded through Q3TTS_LIB for an A/B run)
        L.q3tts_session_open_ex.argtypes = [vp, C.POINTER(SessionOptsEx), C.POINTER(Sampling), EVENT_CB, vp, C.POINTER(vp)]
        L.q3tts_session_voice_create.argtypes = [vp, f32p, C.c_int64, C.c_int32, i32p, C.c_int32, C.POINTER(vp)]
        L.q3tts_session_voice_wait.argtypes = [vp, vp, C.c_int32, i32p]
        L.q3tts_session_voice_free.argtypes = [vp, vp]
        L.q3tts_session_get_voice_stats.argtypes = [vp, C.POINTER(SessionVoiceStats)]
    if hasattr(L, "q3tts_session_submit_open"):  # (absent from an older build loaded through Q3TTS_LIB for an A/B run)
        L.q3tts_session_submit_open.argtypes = [vp, C.POINTER(Request), C.POINTER(RowSampling), C.POINTER(C.c_int64)]
        L.q3tts_session_append_text.argtypes = [vp, C.c_int64, i32p, C.c_int32, C.c_int32]
        L.q3tts_session_get_text_stats.argtypes = [vp, C.POINTER(SessionTextStats)]
        L.q3tts_debug_text_resume.argtypes = [vp, C.c_int32, C.c_int32, u16p, i32p, u16p, u16p, f32p, i32p]
    L.q3tts_generate_begin.argtypes = [vp, C.POINTER(Request), C.c_int32, C.POINTER(Sampling), EVENT_CB, vp, C.c_int32, C.POINTER(vp)]
    L.q3tts_generate_end.argtypes = [vp, vp, C.POINTER(Result)]
    L.q3tts_pcm_to_int16.argtypes = [f32p, C.c_int64, C.POINTER(C.c_int16)]
    L.q3tts_pcm_to_int16.restype = None
    L.q3tts_write_wav.argtypes = [C.c_char_p, f32p, C.c_int64, C.c_int32]
    L.q3tts_result_free.argtypes = [C.POINTER(Result), C.c_int32]
    L.q3tts_result_free.restype = None
    L.q3tts_codec_decode.argtypes = [vp, i32p, i32p, C.c_int32, C.c_int32, f32p, C.POINTER(C.c_int64)]
    L.q3tts_codec_decode_streamed.argtypes = [vp, i32p, i32p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, f32p]
    if hasattr(L, "q3tts_codec_decode_streamed_prefixed"):  # (absent from an older build loaded through Q3TTS_LIB for an A/B run)
        L.q3tts_codec_decode_streamed_prefixed.argtypes = [vp, i32p, i32p, i32p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                           f32p]
    if hasattr(L, "q3tts_request_speed_info"):
        L.q3tts_request_speed_info.argtypes = [vp, C.c_float, C.POINTER(C.c_float), i32p, i32p, i32p]
        L.q3tts_debug_stretch_rows.argtypes = [vp, f32p, i32p, i32p, C.c_int32, C.c_int64, f32p, C.c_int64]
    if hasattr(L, "q3tts_pitch_shift"):  # (absent from an older build loaded through Q3TTS_LIB for an A/B run)
        L.q3tts_default_load_opts_ex.argtypes = [C.POINTER(LoadOptsEx)]
        L.q3tts_default_load_opts_ex.restype = None
        L.q3tts_model_load_ex.argtypes = [C.c_char_p, C.POINTER(LoadOptsEx), C.POINTER(vp)]
        L.q3tts_model_get_pitch.argtypes = [vp, C.POINTER(C.c_float), i32p, i32p, i32p]
        L.q3tts_pitch_shift.argtypes = [vp, f32p, C.c_int64, C.c_float, f32p, C.c_int64, C.POINTER(C.c_int64)]
        L.q3tts_debug_resample_ratio.argtypes = [vp, f32p, i32p, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                                 f32p, C.c_int64]
    if hasattr(L, "q3tts_pitch_shift_formants"):  # (absent from an older build loaded through Q3TTS_LIB for an A/B run)
        L.q3tts_default_load_opts_ex2.argtypes = [C.POINTER(LoadOptsEx2)]
        L.q3tts_default_load_opts_ex2.restype = None
        L.q3tts_model_load_ex2.argtypes = [C.c_char_p, C.POINTER(LoadOptsEx2), C.POINTER(vp)]
        L.q3tts_model_get_keep_formants.argtypes = [vp, i32p]
        L.q3tts_pitch_shift_formants.argtypes = [vp, f32p, C.c_int64, C.c_float, f32p, C.c_int64, C.POINTER(C.c_int64)]
        L.q3tts_debug_formant_rows.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, i32p, C.c_int32, f32p, C.c_int64, C.c_int32, f32p, C.c_int64,
                                               f32p, f32p, f32p, C.c_int64, C.c_int32]
    if hasattr(L, "q3tts_debug_prefix_states"):
        L.q3tts_debug_prefix_states.argtypes = [vp, i32p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    if hasattr(L, "q3tts_debug_codec_stream_slots"):  # (absent from an older build loaded through Q3TTS_LIB for an A/B run)
        L.q3tts_debug_codec_stream_slots.argtypes = [vp, i32p, i32p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                     C.c_int32, f32p]
    L.q3tts_debug_set_codec_scratch.argtypes = [C.c_uint64]
    L.q3tts_debug_set_codec_scratch.restype = None
    L.q3tts_debug_reload_env.argtypes = []
    L.q3tts_debug_reload_env.restype = None
    L.q3tts_last_timing.argtypes = [vp, C.POINTER(Timing)]
    L.q3tts_codec_encode.argtypes = [vp, f32p, C.c_int64, i32p, C.c_int32, i32p]
    L.q3tts_codec_encoded_frames.argtypes = [vp, C.c_int64]
    L.q3tts_speaker_embedding.argtypes = [vp, f32p, C.c_int64, C.c_int32, f32p, C.c_int32]
    L.q3tts_debug_frontend_stage.argtypes = [vp, f32p, C.c_int64, C.c_char_p, f32p, C.c_int64, i32p, i32p]
    L.q3tts_tokenizer_load.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.q3tts_tokenizer_free.argtypes = [vp]
    L.q3tts_tokenizer_free.restype = None
    L.q3tts_tokenizer_encode.argtypes = [vp, C.c_char_p, i32p, C.c_int32, i32p]
    L.q3tts_debug_prepare_inputs.argtypes = [vp, C.POINTER(Request), u16p, C.c_int32, i32p, u16p, C.c_int32,
                                             i32p, u16p]
    L.q3tts_debug_generate_forced.argtypes = [vp, C.POINTER(Request), C.c_int32, C.POINTER(Sampling), i32p,
                                              C.c_int32, u16p, u16p, i32p]
    L.q3tts_debug_sample.argtypes = [vp, u16p, C.c_int32, C.c_int32, C.POINTER(Sampling), u8p, C.c_int32,
                                     C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, i32p]
    L.q3tts_debug_linear.argtypes = [vp, u16p, u16p, u16p, C.c_int32, C.c_int32, C.c_int32, u16p]
    L.q3tts_debug_attention.argtypes = [vp, C.POINTER(AttnDebug)]
    if hasattr(L, "q3tts_debug_gemm"):  # (absent from an older build loaded through Q3TTS_LIB for an A/B run)
        L.q3tts_debug_gemm.argtypes = [vp, C.POINTER(GemmDebug)]
    if hasattr(L, "q3tts_debug_conv"):  # (absent from an older build loaded through Q3TTS_LIB for an A/B run)
        L.q3tts_debug_conv.argtypes = [vp, C.POINTER(ConvDebug)]
    if hasattr(L, "q3tts_debug_rowop"):  # (absent from an older build loaded through Q3TTS_LIB for an A/B run)
        L.q3tts_debug_rowop.argtypes = [vp, C.POINTER(RowopDebug)]
    if hasattr(L, "q3tts_debug_lmop"):  # (absent from an older build loaded through Q3TTS_LIB for an A/B run)
        L.q3tts_debug_lmop.argtypes = [vp, C.POINTER(LmopDebug)]
    if hasattr(L, "q3tts_debug_build_decode_codes"):  # (absent from an older build loaded through Q3TTS_LIB for an A/B run)
        L.q3tts_debug_build_decode_codes.argtypes = [vp, i32p, i32p, i32p, i32p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, i32p]
    L.q3tts_debug_codec_stage.argtypes = [vp, i32p, C.c_int32, C.c_char_p, f32p, C.c_int64, i32p, i32p]
    _lib = L
    return L


GEOM_FIELDS = ("rode", "tall", "tall_shape", "split", "mbw", "nw", "ch", "np", "gx", "ntw", "tm")


def gemm_geometry(**kw) -> dict:
    """q3tts_debug_gemm with geometry_only = 1: the launch skinny_geometry / gemm_tall_takes choose for these sizes and options
    (GemmDebug's scalar fields as keywords). Host code only: needs neither a model nor a GPU. Raises ValueError on
    INVALID_INPUT."""
    a = GemmDebug(geometry_only=1, **kw)
    st = lib().q3tts_debug_gemm(None, C.byref(a))
    if st != 0:
        raise ValueError("q3tts_debug_gemm refused the arguments (status %d): %r" % (st, kw))
    return {f: int(getattr(a, f)) for f in GEOM_FIELDS}


CONV_GEOM_FIELDS = ("family", "BN", "pro", "pw_depth", "KT", "X32", "CT2", "PT", "wdb", "grid_x", "grid_y", "grid_z", "lds_bytes")
CONV_OPERANDS = ("x2", "bias", "bias2", "scale", "snake", "act2", "post", "res", "out", "out2", "w2", "pcm", "nonfinite")


def conv_geometry(frames=None, **kw) -> dict:
    """q3tts_debug_conv with geometry_only = 1: the launch the conv launchers' dispatch functions choose (ConvDebug's scalar fields
    as keywords; the names of CONV_OPERANDS as truthy keywords say which optional operands take part; frames: the rows' frame
    counts, checked when given). Host code only: needs neither a model nor a GPU. Raises ValueError on INVALID_INPUT."""
    ops = {k: kw.pop(k, False) for k in CONV_OPERANDS}
    a = ConvDebug(geometry_only=1, **kw)
    one = (C.c_float * 4)()
    fp = C.cast(one, f32p)
    a.w = fp
    for name in ("x2", "bias", "bias2", "scale", "w2", "pcm"):
        if ops[name]:
            setattr(a, name, fp)
    for name in ("snake", "act2", "post"):
        if ops[name]:
            setattr(a, name + "_alpha", fp)
            setattr(a, name + "_beta", fp)
    for name in ("res", "out", "out2"):
        if ops[name]:
            setattr(a, name, C.cast(one, C.c_void_p))
    if ops["nonfinite"]:
        a.nonfinite = C.cast(one, i32p)
    fr = None
    if frames is not None:
        fr = (C.c_int32 * len(frames))(*frames)
        a.frames = C.cast(fr, i32p)
    st = lib().q3tts_debug_conv(None, C.byref(a))
    if st != 0:
        raise ValueError("q3tts_debug_conv refused the arguments (status %d): %r" % (st, kw))
    return {f: int(getattr(a, f)) for f in CONV_GEOM_FIELDS}


def reload_debug_env() -> None:
    """The launchers read their diagnostic switches (Q3TTS_*) once per model load; after changing one on a live model call this."""
    lib().q3tts_debug_reload_env()
