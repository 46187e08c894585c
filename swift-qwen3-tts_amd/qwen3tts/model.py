"""Host-side mirror of the reference's public surface on top of the C ABI.

Names and argument meaning follow /root/reference/Sources/Qwen3TTS/Models/Qwen3.swift
(`Qwen3TTSModel.fromPretrained` :1382, `generate` :1291-1301, `supportedSpeakers` :965-971) and
Qwen3+Streaming.swift (`generateStream` :8-18) with the event enum of
Core/GenerationTypes.swift:51-58. Tokenisation stays outside the engine like in the reference
(swift-transformers there): callers pass token ids, or a `tokenizer` callable text -> ids.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import dataclass
from typing import Callable, Iterator, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib as L


class Qwen3TTSError(RuntimeError):
    """AudioGenerationError (GenerationTypes.swift:63-84); `.status` is the q3tts_status code."""

    def __init__(self, status: int, message: str):
        super().__init__(message)
        self.status = status


@dataclass
class AudioGenerationInfo:  # GenerationTypes.swift:15-21
    prompt_token_count: int
    generation_token_count: int
    prefill_time: float
    generate_time: float
    tokens_per_second: float
    peak_memory_usage: float

    @property
    def summary(self) -> str:
        """AudioGenerationInfo.summary (GenerationTypes.swift:39-45): the same three lines and number formats."""
        return ("Prompt:     %d tokens, %.2f tokens/s, %.3fs\n"
                "Generation: %d tokens, %.2f tokens/s, %.3fs\n"
                "Peak Memory Usage: %s GB" % (self.prompt_token_count, self.prompt_token_count / max(self.prefill_time, 0.001),
                                              self.prefill_time, self.generation_token_count, self.tokens_per_second,
                                              self.generate_time, repr(float(self.peak_memory_usage))))


@dataclass
class RequestSampling:
    """Sampling parameters of one request of a call (q3tts_row_sampling): a field that is None inherits the call's value.
    A seed replaces the seed of the request's random stream; the stream's key (row_base + request index) stays."""
    temperature: Optional[float] = None
    top_k: Optional[int] = None
    top_p: Optional[float] = None
    repetition_penalty: Optional[float] = None
    seed: Optional[int] = None


@dataclass
class GenerationRequest:
    """One utterance after tokenisation (see q3tts_request in include/q3tts.h)."""
    text_ids: Sequence[int]
    target_token_count: int
    instruct_ids: Optional[Sequence[int]] = None
    speaker: Optional[str] = None
    language: str = "auto"
    max_tokens: int = 2048
    # voice clone (generateVoiceClone, Qwen3.swift:1009-1020): 24 kHz mono float32 + tokens of
    # "<|im_start|>assistant\n{referenceText}<|im_end|>\n"
    ref_audio: Optional[np.ndarray] = None
    ref_text_ids: Optional[Sequence[int]] = None
    # 0: generate() (routed by tts_model_type); 1 / 2: generateVoiceDesign / generateCustomVoice called directly (q3tts.h)
    route: int = 0
    # this request's own sampling parameters (None: the call's); a static batch or a queue may mix them freely
    sampling: Optional[RequestSampling] = None
    # a reusable voice prompt (Qwen3TTSModel.create_voice): the request is then a voice-clone request whose reference is that
    # voice -- no ref_audio / ref_text_ids beside it; speaker, instruct_ids and route are ignored
    voice: Optional["Voice"] = None
    # this request's speaking rate (q3tts_request.speed): 0 = the handle's; 0.5 .. 2.0 on a model loaded with
    # request_speeds=True, 1.0 meaning "no stretch for this request"
    speed: float = 0.0


@dataclass
class GenerationResult:
    audio: np.ndarray  # float32 [n_samples] at the model's sample_rate (24 kHz by default)
    codes: np.ndarray  # int32 [n_frames][16]
    info: AudioGenerationInfo
    status: int = 0


class Voice:
    """A reference clip and its transcript, encoded once and held on the device (q3tts_voice). Requests name it through
    GenerationRequest.voice; it stays usable until close() (or the end of a `with` block), or until its model is closed.
    Closing a voice while a call that names it is running is an error of the caller."""

    def __init__(self, model: "Qwen3TTSModel", handle: C.c_void_p, session: Optional["Session"] = None):
        self._model, self._h = model, handle
        self._session = session  # the session that made it (Session.create_voice): its free and its wait while it is open
        vi = L.VoiceInfo()
        model._check(model._lib.q3tts_voice_get_info(handle, C.byref(vi)))
        self.info = vi  # ref_frames, ref_text_tokens, n_ref_samples, device_bytes

    def wait(self, timeout: Optional[float] = None) -> "Voice":
        """A session-made voice: waits until its front end is done (q3tts_session_voice_wait). TimeoutError when `timeout`
        seconds pass first; status 8 (Qwen3TTSError) when a close without drain abandoned it; status 3 once the session has
        closed (there is nothing to wait on: every job it had accepted has finished or been abandoned). A voice of
        Qwen3TTSModel.create_voice is ready from the start."""
        sess = self._session
        if not self._h:
            raise Qwen3TTSError(3, "Invalid input: the voice has been closed")
        if sess is None:
            return self
        if not sess._h:
            raise Qwen3TTSError(3, "Invalid input: the session that made the voice has been closed")
        ready = C.c_int32(0)
        ms = -1 if timeout is None else max(0, int(round(timeout * 1000)))
        self._model._check(self._model._lib.q3tts_session_voice_wait(sess._handle(), self._h, ms, C.byref(ready)))
        if not ready.value:
            raise TimeoutError("the voice was not ready after %s s" % (timeout,))
        return self

    def close(self):
        sess = self._session
        if self._h and sess is not None and sess._h and self._model._h:  # while its session is open: the session's free
            self._model._lib.q3tts_session_voice_free(sess._h, self._h)
        elif self._h and self._model._h:  # (a closed model has released its voices already)
            self._model._lib.q3tts_voice_free(self._model._h, self._h)
        self._h = None

    def __enter__(self) -> "Voice":
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def chat_template_ids(tokenizer: Callable[[str], List[int]], text: str, instruct: Optional[str] = None) -> dict:
    """The three tokenisations the reference performs (Qwen3.swift:274-275, 364-365, 822)."""
    out = {"text_ids": tokenizer(f"<|im_start|>assistant\n{text}<|im_end|>\n<|im_start|>assistant\n"),
           "target_token_count": len(tokenizer(text))}
    if instruct:
        out["instruct_ids"] = tokenizer(f"<|im_start|>user\n{instruct}<|im_end|>\n")
    return out


class _ResultBlock:
    """Owns one q3tts_result array; frees it when the last view over its rows is gone."""

    def __init__(self, lib, res, n):
        self._lib, self._res, self._n = lib, res, n

    def __del__(self):
        try:
            self._lib.q3tts_result_free(self._res, self._n)
        except Exception:  # interpreter shutdown
            pass


class _RowBuf:
    """One row's buffer for numpy (__array_interface__): the array's base is this object, which keeps the block alive."""

    def __init__(self, block, ptr, shape, typestr):
        self._block = block
        self.__array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 3}


class Qwen3TTSModel:
    def __init__(self, handle: C.c_void_p, lib):
        self._h = handle
        self._lib = lib
        info = L.ModelInfo()
        self._check(lib.q3tts_model_get_info(self._h, C.byref(info)))
        self.info = info
        self.tokenizer: Optional[Callable[[str], List[int]]] = None
        self.last_info: Optional[AudioGenerationInfo] = None  # .info of the last call's first request

    # -- loading ---------------------------------------------------------------------------------
    @classmethod
    def from_pretrained(cls, model_path: str, device: int = 0, max_batch: int = 1, max_frames: int = 2048,
                        max_prompt: int = 512, use_graph: bool = True,
                        weights_from_broadcast: bool = False, n_streams: int = 0,
                        codec_overlap_cus: int = 0, codec_fp32: bool = False,
                        output_sample_rate: int = 0, speed: float = 0.0, request_speeds: bool = False,
                        pitch: float = 0.0, keep_formants: bool = False) -> "Qwen3TTSModel":
        """output_sample_rate (q3tts_load_opts.output_sample_rate): 0 = 24000; 8000, 12000, 16000, 22050, 32000, 44100 or
        48000 make every waveform of this handle leave at that rate (sample_rate and info.samples_per_frame report it).
        speed (q3tts_load_opts.speed): 0 or 1.0 = off; 0.5 .. 2.0 make this handle speak that much faster, pitch preserved,
        through the time stretch in the decoder's tail (`speed`, `stretch_hs` and `stretch_delay_samples` report what was
        chosen, info.samples_per_frame follows).
        request_speeds (q3tts_load_opts.request_speeds): the handle admits GenerationRequest.speed, a speaking rate per
        request (`request_speed_info` tells what one becomes; info.max_samples_per_frame is the slowest request's).
        pitch (q3tts_load_opts_ex.pitch): 0 = off; -12 .. 12 semitones shift this handle's pitch at an unchanged duration
        (`pitch_info` reports what was chosen; sample counts are those of the handle without it). Not with request_speeds.
        keep_formants (q3tts_load_opts_ex2.keep_formants): the pitch keeps the voice's formants -- a linear-prediction envelope
        per hop, taken off in front of the pitch resampler and put back behind it (`keep_formants_info` tells whether the stage
        runs: it needs a pitch that is on). 24 kHz output only."""
        lib = L.lib()
        o = L.LoadOpts()
        lib.q3tts_default_load_opts(C.byref(o))
        o.device, o.max_batch, o.max_frames, o.max_prompt = device, max_batch, max_frames, max_prompt
        o.use_graph = 1 if use_graph else 0
        o.weights_from_broadcast = 1 if weights_from_broadcast else 0
        o.n_streams = n_streams
        o.codec_overlap_cus = codec_overlap_cus
        o.codec_fp32 = 1 if codec_fp32 else 0
        o.output_sample_rate = int(output_sample_rate)
        o.speed = float(speed)
        o.request_speeds = 1 if request_speeds else 0
        h = C.c_void_p()
        if keep_formants is not False:  # (anything but the default goes to the library, which refuses what is not 0 / 1)
            if not hasattr(lib, "q3tts_model_load_ex2"):
                raise Qwen3TTSError(3, "Invalid input: this build of the library has no keep_formants option")
            ex2 = L.LoadOptsEx2()
            lib.q3tts_default_load_opts_ex2(C.byref(ex2))
            ex2.ex.base, ex2.ex.pitch, ex2.keep_formants = o, float(pitch), int(keep_formants)
            st = lib.q3tts_model_load_ex2(model_path.encode(), C.byref(ex2), C.byref(h))
        elif pitch == 0.0:  # (a float comparison: a NaN goes on to be refused below)
            st = lib.q3tts_model_load(model_path.encode(), C.byref(o), C.byref(h))
        else:
            if not hasattr(lib, "q3tts_model_load_ex"):
                raise Qwen3TTSError(3, "Invalid input: this build of the library has no pitch option")
            ex = L.LoadOptsEx()
            lib.q3tts_default_load_opts_ex(C.byref(ex))
            ex.base, ex.pitch = o, float(pitch)
            st = lib.q3tts_model_load_ex(model_path.encode(), C.byref(ex), C.byref(h))
        if st != 0:
            raise Qwen3TTSError(st, (lib.q3tts_last_error(None) or b"").decode())
        m = cls(h, lib)
        # AutoTokenizer.from(modelFolder:) in postLoadHook (Qwen3.swift:1456-1459): the engine's own BPE when the files exist
        if any(os.path.exists(os.path.join(model_path, f)) for f in ("tokenizer.json", "vocab.json")):
            m.tokenizer = NativeTokenizer(model_path)
        return m

    def close(self):
        if self._h:
            self._lib.q3tts_model_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st: int):
        if st != 0:
            raise Qwen3TTSError(st, (self._lib.q3tts_last_error(self._h) or b"").decode())

    # -- properties (Qwen3.swift:1262-1271, 965-971, 1210-1214) -----------------------------------
    @property
    def sample_rate(self) -> int:
        return self.info.sample_rate

    def _speed(self):
        s, hs, d = C.c_float(0), C.c_int32(0), C.c_int32(0)
        self._check(self._lib.q3tts_model_get_speed(self._h, C.byref(s), C.byref(hs), C.byref(d)))
        return float(s.value), int(hs.value), int(d.value)

    @property
    def speed(self) -> float:
        """The effective speaking rate 480 / Hs of this handle (1.0: the time stretch is off)."""
        return self._speed()[0]

    @property
    def stretch_hs(self) -> int:
        """The time stretch's synthesis hop Hs (480: off); a frame yields 4 * Hs samples at 24 kHz."""
        return self._speed()[1]

    @property
    def stretch_delay_samples(self) -> int:
        """The delay D of the causal time stretch in 24 kHz samples (q3tts.h, "Speaking rate")."""
        return self._speed()[2]

    def request_speed_info(self, speed: float) -> Tuple[float, int, int, int]:
        """q3tts_request_speed_info: what a request at `speed` gets on this handle (0: the handle's own) -- the effective
        speed 480 / Hs, Hs, the delay D in 24 kHz samples and its samples per frame at the output rate. Host arithmetic alone."""
        s, hs, d, spf = C.c_float(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._check(self._lib.q3tts_request_speed_info(self._h, float(speed), C.byref(s), C.byref(hs), C.byref(d), C.byref(spf)))
        return float(s.value), int(hs.value), int(d.value), int(spf.value)

    def pitch_info(self) -> Tuple[float, int, int, int]:
        """q3tts_model_get_pitch: the effective shift 12 log2(Hp / Ho) in semitones (0: off), the hop Hp in front of the
        resampler, the handle's hop Ho (equal: off) and the delay of the two stages in output samples."""
        s, hp, ho, d = C.c_float(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._check(self._lib.q3tts_model_get_pitch(self._h, C.byref(s), C.byref(hp), C.byref(ho), C.byref(d)))
        return float(s.value), int(hp.value), int(ho.value), int(d.value)

    def keep_formants_info(self) -> bool:
        """q3tts_model_get_keep_formants: whether the formant-preserving stage runs on this handle (the option with a pitch that is
        on)."""
        on = C.c_int32(0)
        self._check(self._lib.q3tts_model_get_keep_formants(self._h, C.byref(on)))
        return bool(on.value)

    def debug_formant_rows(self, mode: int, hp: int, ho: int, x: np.ndarray, lens: Sequence[int], coef: np.ndarray, y: np.ndarray,
                           hist: int = 0, state_in: Optional[np.ndarray] = None, want_state: bool = False, clamp: bool = False):
        """q3tts_debug_formant_rows: kernels/formant.hip on host rows x [B][x_stride] (mode 0: analyse + whiten, 1: synthesise
        with `coef`, 2: both, Hp == Ho). Returns (y, coef, state behind or None) as the kernels left them."""
        x = np.ascontiguousarray(x, np.float32)
        y = np.ascontiguousarray(y, np.float32).copy()
        coef = np.ascontiguousarray(coef, np.float32).copy()
        ln = np.ascontiguousarray(lens, np.int32)
        si = None if state_in is None else np.ascontiguousarray(state_in, np.float32)
        so = np.zeros((x.shape[0], 24), np.float32) if want_state else None
        self._check(self._lib.q3tts_debug_formant_rows(
            self._h, int(mode), int(hp), int(ho), ln.ctypes.data_as(L.i32p), x.shape[0], x.ctypes.data_as(L.f32p), x.shape[1], int(hist),
            coef.ctypes.data_as(L.f32p), coef.shape[1], None if si is None else si.ctypes.data_as(L.f32p),
            None if so is None else so.ctypes.data_as(L.f32p), y.ctypes.data_as(L.f32p), y.shape[1], 1 if clamp else 0))
        return y, coef, so

    def debug_resample_ratio(self, x: np.ndarray, lens: Sequence[int], in_units: int, out_units: int, y: np.ndarray,
                             centred: bool = False, clamp: bool = False, hist: int = 0) -> np.ndarray:
        """q3tts_debug_resample_ratio: the general-ratio resampler on host rows x [B][row_stride], each `hist` samples of
        margin followed by lens[b] samples; y [B][y_stride] comes back with what each row wrote."""
        x = np.ascontiguousarray(x, np.float32)
        y = np.ascontiguousarray(y, np.float32).copy()
        ln = np.ascontiguousarray(lens, np.int32)
        self._check(self._lib.q3tts_debug_resample_ratio(self._h, x.ctypes.data_as(L.f32p), ln.ctypes.data_as(L.i32p), x.shape[0], x.shape[1],
                                                         int(in_units), int(out_units), 1 if centred else 0, 1 if clamp else 0, int(hist),
                                                         y.ctypes.data_as(L.f32p), y.shape[1]))
        return y

    def debug_stretch_rows(self, x: np.ndarray, lens: Sequence[int], hops: Sequence[int], y: np.ndarray) -> np.ndarray:
        """q3tts_debug_stretch_rows: the stretch kernel's per-row path on host rows x [B][x_stride]; y [B][y_stride] comes back
        with what each row wrote."""
        x = np.ascontiguousarray(x, np.float32)
        y = np.ascontiguousarray(y, np.float32).copy()
        ln = np.ascontiguousarray(lens, np.int32)
        hp = np.ascontiguousarray(hops, np.int32)
        self._check(self._lib.q3tts_debug_stretch_rows(self._h, x.ctypes.data_as(L.f32p), ln.ctypes.data_as(L.i32p), hp.ctypes.data_as(L.i32p),
                                                       x.shape[0], x.shape[1], y.ctypes.data_as(L.f32p), y.shape[1]))
        return y

    @property
    def tts_model_type(self) -> str:
        return self.info.tts_model_type.decode()

    @property
    def supported_speakers(self) -> List[str]:
        n = self._lib.q3tts_model_num_speakers(self._h)
        return [self._lib.q3tts_model_speaker_name(self._h, i).decode() for i in range(n)]

    @property
    def supports_voice_cloning(self) -> bool:
        return bool(self.info.supports_voice_cloning)

    def arena(self) -> Tuple[int, int]:
        p, n = C.c_void_p(), C.c_size_t()
        self._check(self._lib.q3tts_model_arena(self._h, C.byref(p), C.byref(n)))
        return int(p.value), int(n.value)

    @staticmethod
    def comm_unique_id() -> bytes:
        """q3tts_comm_get_unique_id: 128 bytes that rank 0 ships to the other ranks of a sharded job (any channel)."""
        cid = L.CommId()
        st = L.lib().q3tts_comm_get_unique_id(C.byref(cid))
        if st != 0:
            raise Qwen3TTSError(st, (L.lib().q3tts_last_error(None) or b"").decode())
        return C.string_at(C.addressof(cid), 128)  # (c_char arrays stop at the first NUL when read as .bytes)

    def broadcast_weights(self, comm_id: bytes, rank: int, world: int, root: int = 0) -> None:
        """q3tts_model_broadcast: the load-time RCCL broadcast of the weight arena (collective: every rank calls it)."""
        assert len(comm_id) == 128
        cid = L.CommId()
        C.memmove(C.addressof(cid), comm_id, 128)
        self._check(self._lib.q3tts_model_broadcast(self._h, C.byref(cid), rank, world, root))

    def arena_checksum(self) -> int:
        v = C.c_uint64()
        self._check(self._lib.q3tts_model_arena_checksum(self._h, C.byref(v)))
        return int(v.value)

    def create_voice(self, ref_audio: np.ndarray, ref_text_ids: Sequence[int], sample_rate: int = 24000) -> Voice:
        """q3tts_voice_create / _create_rate: encodes the reference clip (mono float32 at sample_rate) once -- codec encoder,
        speaker encoder, the prompt rows made of them -- and keeps the result on the device. A clip at another supported rate
        than 24000 is resampled on the device first (centred form). ref_text_ids as GenerationRequest.ref_text_ids."""
        ra = np.ascontiguousarray(np.asarray(ref_audio, np.float32).reshape(-1))
        rt = np.ascontiguousarray(ref_text_ids, np.int32)
        h = C.c_void_p()
        if int(sample_rate) == 24000:
            self._check(self._lib.q3tts_voice_create(self._h, ra.ctypes.data_as(L.f32p), ra.size, rt.ctypes.data_as(L.i32p),
                                                     rt.size, C.byref(h)))
        else:
            self._check(self._lib.q3tts_voice_create_rate(self._h, ra.ctypes.data_as(L.f32p), ra.size, int(sample_rate),
                                                          rt.ctypes.data_as(L.i32p), rt.size, C.byref(h)))
        return Voice(self, h)

    def resample(self, audio: np.ndarray, in_rate: int, out_rate: int, centred: bool = True) -> np.ndarray:
        """q3tts_resample: the engine's polyphase FIR on the device (include/q3tts.h, "Sample rates"). One of the rates is
        24000. centred: no delay (reference clips); otherwise the causal form the decoder's output stage uses."""
        a = np.ascontiguousarray(np.asarray(audio, np.float32).reshape(-1))
        g = math.gcd(int(in_rate), int(out_rate)) if in_rate > 0 and out_rate > 0 else 1
        cap = max(1, -(-a.size * (int(out_rate) // g) // max(1, int(in_rate) // g)))
        out = np.zeros(cap, np.float32)
        n = C.c_int64(0)
        self._check(self._lib.q3tts_resample(self._h, a.ctypes.data_as(L.f32p), a.size, int(in_rate), int(out_rate),
                                             1 if centred else 0, out.ctypes.data_as(L.f32p), out.size, C.byref(n)))
        return out[: n.value]

    def time_stretch(self, audio: np.ndarray, speed: float, causal: bool = False) -> np.ndarray:
        """q3tts_time_stretch: the engine's pitch-preserving time stretch on the device, for 24 kHz audio (include/q3tts.h,
        "Speaking rate"). causal: the delayed form the decoder's stage uses; otherwise the whole form (no delay)."""
        a = np.ascontiguousarray(np.asarray(audio, np.float32).reshape(-1))
        out = np.zeros(max(1, 2 * a.size + 960), np.float32)  # (Hs <= 960 = 2 Ha, one hop of rounding)
        n = C.c_int64(0)
        self._check(self._lib.q3tts_time_stretch(self._h, a.ctypes.data_as(L.f32p), a.size, float(speed), 1 if causal else 0,
                                                 out.ctypes.data_as(L.f32p), out.size, C.byref(n)))
        return out[: n.value]

    def pitch_shift(self, audio: np.ndarray, semitones: float, keep_formants: bool = False) -> np.ndarray:
        """q3tts_pitch_shift: 24 kHz audio shifted by `semitones` at (nearly) its duration, on the device: the whole time
        stretch at Hp = round(480 * 2^(semitones / 12)), then the centred resampler Hp -> 480 (include/q3tts.h, "Pitch").
        keep_formants: q3tts_pitch_shift_formants, the same with the formant-preserving stage around the resampler."""
        a = np.ascontiguousarray(np.asarray(audio, np.float32).reshape(-1))
        out = np.zeros(a.size + 8, np.float32)  # (two roundings up, at most 2 + 480 / Hp samples over n_in)
        n = C.c_int64(0)
        fn = self._lib.q3tts_pitch_shift_formants if keep_formants else self._lib.q3tts_pitch_shift
        self._check(fn(self._h, a.ctypes.data_as(L.f32p), a.size, float(semitones), out.ctypes.data_as(L.f32p),
                                                out.size, C.byref(n)))
        return out[: n.value]

    @staticmethod
    def _voices(reqs: Sequence[GenerationRequest]):
        """The q3tts_voice* array of a call, or None when no request names a voice."""
        vs = [getattr(r, "voice", None) for r in reqs]
        if not any(v is not None for v in vs):
            return None
        arr = (C.c_void_p * len(reqs))()
        for i, v in enumerate(vs):
            if v is None:
                continue
            if not v._h:
                raise Qwen3TTSError(3, "Invalid input: the voice of request %d has been closed" % i)
            arr[i] = v._h
        return arr

    def last_timing(self) -> L.Timing:
        t = L.Timing()
        self._lib.q3tts_last_timing(self._h, C.byref(t))
        return t

    # -- generation --------------------------------------------------------------------------------
    def _marshal(self, reqs: Sequence[GenerationRequest]):
        arr = (L.Request * len(reqs))()
        keep = []
        for i, r in enumerate(reqs):
            t = np.ascontiguousarray(r.text_ids, np.int32)
            keep.append(t)
            arr[i].text_ids = t.ctypes.data_as(L.i32p)
            arr[i].n_text_ids = t.size
            if r.instruct_ids is not None and len(r.instruct_ids):
                ii = np.ascontiguousarray(r.instruct_ids, np.int32)
                keep.append(ii)
                arr[i].instruct_ids = ii.ctypes.data_as(L.i32p)
                arr[i].n_instruct_ids = ii.size
            arr[i].target_token_count = int(r.target_token_count)
            arr[i].speaker = r.speaker.encode() if r.speaker is not None else None
            arr[i].language = (r.language or "auto").encode()
            arr[i].max_tokens = int(r.max_tokens)
            arr[i].speed = float(getattr(r, "speed", 0.0) or 0.0)
            arr[i].route = int(getattr(r, "route", 0))
            if r.ref_audio is not None:
                ra = np.ascontiguousarray(np.asarray(r.ref_audio, np.float32).reshape(-1))
                rt = np.ascontiguousarray(r.ref_text_ids if r.ref_text_ids is not None else [], np.int32)
                keep += [ra, rt]
                arr[i].ref_audio = ra.ctypes.data_as(L.f32p)
                arr[i].n_ref_samples = ra.size
                arr[i].ref_text_ids = rt.ctypes.data_as(L.i32p)
                arr[i].n_ref_text_ids = rt.size
            elif r.ref_text_ids is not None and getattr(r, "voice", None) is not None:
                rt = np.ascontiguousarray(r.ref_text_ids, np.int32)  # (passed on as given: the library refuses it beside a voice)
                keep.append(rt)
                arr[i].ref_text_ids = rt.ctypes.data_as(L.i32p)
                arr[i].n_ref_text_ids = rt.size
        return arr, keep

    @staticmethod
    def _row_sampling(rows: Sequence[Optional[RequestSampling]]):
        """The q3tts_row_sampling array of a call, or None when no request carries parameters of its own."""
        if not any(r is not None for r in rows):
            return None
        arr = (L.RowSampling * len(rows))()
        for i, r in enumerate(rows):
            if r is None:
                continue
            for bit, name in ((L.ROW_TEMPERATURE, "temperature"), (L.ROW_TOP_K, "top_k"), (L.ROW_TOP_P, "top_p"),
                              (L.ROW_REPETITION_PENALTY, "repetition_penalty"), (L.ROW_SEED, "seed")):
                v = getattr(r, name)
                if v is not None:
                    arr[i].set |= bit
                    setattr(arr[i], name, v)
        return arr

    @classmethod
    def _sampling(cls, temperature, top_k, top_p, repetition_penalty, seed, force_frames, audio_chunk_frames=0,
                  audio_window_frames=0, audio_lookahead_frames=4, row_base=0, reqs=None, audio_stream_reference=0) -> L.Sampling:
        """`reqs`: the call's requests; their `sampling` fields become per_request (the array rides on the returned struct,
        which therefore has to stay alive for as long as the library reads it: the call, or begin)."""
        s = L.Sampling()
        rows = cls._row_sampling([getattr(r, "sampling", None) for r in reqs]) if reqs is not None else None
        if rows is not None:
            s._rows = rows
            s.per_request = C.cast(rows, C.POINTER(L.RowSampling))
        s.temperature, s.top_k, s.top_p = temperature, top_k, top_p
        s.repetition_penalty, s.seed, s.force_frames = repetition_penalty, seed, force_frames
        s.audio_chunk_frames = audio_chunk_frames
        s.audio_window_frames, s.audio_lookahead_frames = audio_window_frames, audio_lookahead_frames
        s.row_base = row_base
        s.audio_stream_reference = int(audio_stream_reference)
        return s

    def generate_batch(self, reqs: Sequence[GenerationRequest], temperature: float = 0.9, top_k: int = 50,
                       top_p: float = 1.0, repetition_penalty: float = 1.05, seed: int = 0, force_frames: int = 0,
                       on_event: Optional[Callable[[int, str, object], None]] = None,
                       audio_chunk_frames: int = 0, audio_window_frames: int = 0,
                       audio_lookahead_frames: int = 4, row_base: int = 0, audio_stream_reference: int = 0) -> List[GenerationResult]:
        """n utterances in one call (row-independent). `on_event(request_index, kind, payload)` receives
        ("token", id) / ("info", AudioGenerationInfo) / ("audio", ndarray) in the reference's order; with
        audio_chunk_frames > 0 also ("audio_chunk", (sample_offset, ndarray)) pieces of the final audio, in order,
        between the last token and info (the decoder's causal tail run chunk by chunk; same samples). With
        audio_window_frames > 0 as well the pieces leave while tokens are still being generated (q3tts.h: the
        pre-transformer then sees a sliding window; the waveform is within a stated tolerance of the one-shot decode).
        A batch with a voice-clone row is streamed that way only with audio_stream_reference=1: a clone row's reference then
        goes in front of its stream (codec_decode_streamed_prefixed); without it such a batch is decoded one-shot."""
        arr, keep = self._marshal(reqs)
        s = self._sampling(temperature, top_k, top_p, repetition_penalty, seed, force_frames, audio_chunk_frames,
                           audio_window_frames, audio_lookahead_frames, row_base, reqs=reqs, audio_stream_reference=audio_stream_reference)
        cb = self._event_cb(on_event)
        res = (L.Result * len(reqs))()
        voices = self._voices(reqs)
        if voices is not None:
            st = self._lib.q3tts_generate_voices(self._h, arr, voices, len(reqs), C.byref(s), cb, None, res)
        else:
            st = self._lib.q3tts_generate(self._h, arr, len(reqs), C.byref(s), cb, None, res)
        del keep
        return self._collect(st, res, len(reqs))

    def generate_queued(self, reqs: Sequence[GenerationRequest], slots: Optional[int] = None, temperature: float = 0.9,
                        top_k: int = 50, top_p: float = 1.0, repetition_penalty: float = 1.05, seed: int = 0,
                        force_frames: int = 0, on_event: Optional[Callable[[int, str, object], None]] = None,
                        audio_chunk_frames: int = 0, audio_window_frames: int = 0, audio_lookahead_frames: int = 4,
                        row_base: int = 0, audio_stream_reference: int = 0) -> List[GenerationResult]:
        """Continuous batching (q3tts_generate_queued): any number of requests with at most `slots` rows in flight (default
        max_batch); a finished row's slot takes the next request. Result i is bit-identical to generate_batch([reqs[i]],
        row_base=row_base + i) with the same keywords. Events as generate_batch's, except that a request's ("info", ...) /
        ("audio", ...) arrive as soon as its audio is decoded. With audio_chunk_frames > 0 and audio_window_frames > 0 every
        request's audio is streamed as if it ran alone: ("audio_chunk", (offset, samples)) events carry its request index and
        leave while it generates, "info" / "audio" once its last chunk has landed. Refused: voice-clone requests that carry
        ref_audio (requests that name a `voice` are served, q3tts_generate_queued_voices; with streamed audio only when
        audio_stream_reference=1, which puts a voice's reference in front of its request's stream),
        audio_chunk_frames > 0 without a window (audio_window_frames == 0) or below the decoder's history."""
        arr, keep = self._marshal(reqs)
        s = self._sampling(temperature, top_k, top_p, repetition_penalty, seed, force_frames, audio_chunk_frames,
                           audio_window_frames, audio_lookahead_frames, row_base, reqs=reqs, audio_stream_reference=audio_stream_reference)
        cb = self._event_cb(on_event)
        res = (L.Result * len(reqs))()
        n_slots = int(self.info.max_batch) if slots is None else int(slots)
        voices = self._voices(reqs)
        if voices is not None:
            st = self._lib.q3tts_generate_queued_voices(self._h, arr, voices, len(reqs), n_slots, C.byref(s), cb, None, res)
        else:
            st = self._lib.q3tts_generate_queued(self._h, arr, len(reqs), n_slots, C.byref(s), cb, None, res)
        del keep
        return self._collect(st, res, len(reqs))

    @staticmethod
    def _event_cb(on_event):
        if not on_event:
            return C.cast(None, L.EVENT_CB)

        def _cb(_user, evp):
            ev = evp.contents
            if ev.kind == 3:
                on_event(ev.request_index, "audio_chunk",
                         (int(ev.sample_offset), np.ctypeslib.as_array(ev.pcm, shape=(ev.n_samples,)).copy()))
            elif ev.kind == 0:
                on_event(ev.request_index, "token", int(ev.token))
            elif ev.kind == 1:
                i = ev.info.contents
                on_event(ev.request_index, "info", AudioGenerationInfo(
                    i.prompt_token_count, i.generation_token_count, i.prefill_time, i.generate_time,
                    i.tokens_per_second, i.peak_memory_usage))
            else:
                on_event(ev.request_index, "audio", np.ctypeslib.as_array(ev.pcm, shape=(ev.n_samples,)).copy())

        return L.EVENT_CB(_cb)

    def _collect(self, st, res, n, set_last: bool = True) -> List[GenerationResult]:
        """Results as numpy arrays that VIEW the library's buffers (49 MB of PCM per 32 x 16 s batch: no second copy); the
        buffers go back through q3tts_result_free when the last array over them is collected."""
        block = _ResultBlock(self._lib, res, n)
        self._check(st)
        out = []
        for i in range(n):
            r = res[i]
            inf = r.info
            info = AudioGenerationInfo(inf.prompt_token_count, inf.generation_token_count, inf.prefill_time,
                                       inf.generate_time, inf.tokens_per_second, inf.peak_memory_usage)
            if r.status != 0 or not r.pcm or not r.codes:
                out.append(GenerationResult(np.zeros(0, np.float32), np.zeros((0, 16), np.int32), info, r.status))
                continue
            audio = np.asarray(_RowBuf(block, C.cast(r.pcm, C.c_void_p).value, (int(r.n_samples),), "<f4"))
            codes = np.asarray(_RowBuf(block, C.cast(r.codes, C.c_void_p).value, (int(r.n_frames), 16), "<i4"))
            out.append(GenerationResult(audio, codes, info, 0))
        if set_last:
            self.last_info = out[0].info if out else None
        return out

    def open_session(self, slots: Optional[int] = None, max_pending: int = 0, max_ref_frames: int = 0,
                     on_event: Optional[Callable[[int, str, object], None]] = None, temperature: float = 0.9, top_k: int = 50,
                     top_p: float = 1.0, repetition_penalty: float = 1.05, seed: int = 0, force_frames: int = 0,
                     audio_chunk_frames: int = 0, audio_window_frames: int = 0, audio_lookahead_frames: int = 4, row_base: int = 0,
                     audio_stream_reference: int = 0, live_voices: int = 0, max_voices: int = 0) -> "Session":
        """q3tts_session_open[_ex]: the slot loop of generate_queued on a thread of its own, with an open end. Requests are
        submitted, cancelled and collected one by one while it runs; ticket t's result is bit-identical to
        generate_batch([request], row_base=row_base + t) with the session's keywords and the request's own `sampling`.
        `on_event(ticket, kind, payload)` fires on the session's thread. While the session is open the model's other
        generating calls are refused (status 3); voices are created before it is opened, and `max_ref_frames` bounds the
        references a submit may name. With `live_voices` > 0 (front-end jobs in flight, at most 4) the session also makes
        voices while it runs (Session.create_voice) and takes requests that carry `ref_audio`; `max_voices` bounds the
        session-made voices alive at once (0: 4 * slots)."""
        s = self._sampling(temperature, top_k, top_p, repetition_penalty, seed, force_frames, audio_chunk_frames,
                           audio_window_frames, audio_lookahead_frames, row_base, audio_stream_reference=audio_stream_reference)
        o = L.SessionOpts(int(self.info.max_batch) if slots is None else int(slots), int(max_pending), int(max_ref_frames))
        cb = self._event_cb(on_event)
        h = C.c_void_p()
        if int(live_voices) == 0 and int(max_voices) == 0:
            self._check(self._lib.q3tts_session_open(self._h, C.byref(o), C.byref(s), cb, None, C.byref(h)))
        else:
            ox = L.SessionOptsEx(o, int(live_voices), int(max_voices))
            self._check(self._lib.q3tts_session_open_ex(self._h, C.byref(ox), C.byref(s), cb, None, C.byref(h)))
        return Session(self, h, cb)

    def generate_batch_begin(self, reqs: Sequence[GenerationRequest], temperature: float = 0.9, top_k: int = 50,
                             top_p: float = 1.0, repetition_penalty: float = 1.05, seed: int = 0, force_frames: int = 0,
                             on_event: Optional[Callable[[int, str, object], None]] = None, audio_chunk_frames: int = 0,
                             more_follows: bool = True, row_base: int = 0):
        """First half of generate_batch (q3tts_generate_begin). Input checks, prompt assembly and prefill happen here, so
        a bad request raises here. With on_event the AR loop runs inside this call too (TOKEN events fire here) and the job
        is returned once the codes exist and their codec decode is queued. Without on_event (and without audio_chunk_frames)
        the job is returned as soon as the prefill is queued and the AR loop runs on a library thread: the next batch may be
        begun at once, it takes the model's other job context, and the two AR loops run side by side on the GPU. Either
        way the next batch's AR loop overlaps this batch's decode. At most two jobs may be outstanding; a failure of a
        background AR loop is raised by generate_batch_end; last_timing() describes the job ended last.
        more_follows=False (the last batch of a queue) lets the decode use the whole chip instead of leaving room for a
        next batch."""
        if self._voices(reqs) is not None:  # (q3tts.h: voices arrive through generate_batch and generate_queued only)
            raise Qwen3TTSError(3, "Invalid input: requests that name a voice are not supported by generate_batch_begin")
        arr, keep = self._marshal(reqs)
        s = self._sampling(temperature, top_k, top_p, repetition_penalty, seed, force_frames, audio_chunk_frames, row_base=row_base,
                           reqs=reqs)
        cb = self._event_cb(on_event)
        job = C.c_void_p()
        self._check(self._lib.q3tts_generate_begin(self._h, arr, len(reqs), C.byref(s), cb, None, 1 if more_follows else 0,
                                                   C.byref(job)))
        del keep, s  # request memory and the per-request sampling array are only read during begin
        return (job, len(reqs), cb)  # the callback object must outlive the job (INFO / AUDIO fire in end)

    def generate_batch_end(self, job) -> List[GenerationResult]:
        handle, n, _cb = job
        res = (L.Result * n)()
        return self._collect(self._lib.q3tts_generate_end(self._h, handle, res), res, n)

    def _request_from_text(self, text, speaker, instruct, language, max_tokens, text_ids, instruct_ids,
                           target_token_count) -> GenerationRequest:
        if text_ids is None:
            if self.tokenizer is None:
                raise Qwen3TTSError(1, "Model not initialized: Tokenizer not loaded")  # Qwen3.swift:265-267
            t = chat_template_ids(self.tokenizer, text, instruct)
            text_ids, target_token_count = t["text_ids"], t["target_token_count"]
            instruct_ids = t.get("instruct_ids")
        return GenerationRequest(text_ids, int(target_token_count or 0), instruct_ids, speaker, language, max_tokens)

    def generate(self, text: Optional[str] = None, speaker: Optional[str] = None, instruct: Optional[str] = None,
                 language: str = "auto", temperature: float = 0.9, top_k: int = 50, top_p: float = 1.0,
                 repetition_penalty: float = 1.05, max_tokens: int = 2048, *, seed: int = 0,
                 text_ids: Optional[Sequence[int]] = None, instruct_ids: Optional[Sequence[int]] = None,
                 target_token_count: Optional[int] = None) -> np.ndarray:
        """generate(text:speaker:instruct:language:temperature:topK:topP:repetitionPenalty:maxTokens:)
        (Qwen3.swift:1291-1301). Returns float32 samples at 24 kHz."""
        req = self._request_from_text(text, speaker, instruct, language, max_tokens, text_ids, instruct_ids,
                                      target_token_count)
        r = self.generate_batch([req], temperature, top_k, top_p, repetition_penalty, seed)[0]
        if r.status != 0:
            raise Qwen3TTSError(r.status, "Generation failed: No tokens generated")
        return r.audio

    def generate_voice_design(self, text: Optional[str] = None, language: str = "auto", instruct: Optional[str] = None,
                              temperature: float = 0.9, top_k: int = 50, top_p: float = 1.0,
                              repetition_penalty: float = 1.05, max_tokens: int = 2048,
                              on_token: Optional[Callable[[int], None]] = None, *, seed: int = 0, text_ids=None,
                              instruct_ids=None, target_token_count=None) -> np.ndarray:
        """generateVoiceDesign(text:language:instruct:...:onToken:) (Qwen3.swift:587-597); on_token sees every first-codebook
        id as it is generated (:698)."""
        req = self._request_from_text(text, None, instruct, language, max_tokens, text_ids, instruct_ids, target_token_count)
        req.route = 1  # the named prompt builder whatever the checkpoint's type, as the reference's direct call
        return self._one(req, temperature, top_k, top_p, repetition_penalty, seed, on_token)

    def generate_custom_voice(self, text: Optional[str] = None, speaker: str = "", language: str = "auto",
                              instruct: Optional[str] = None, temperature: float = 0.9, top_k: int = 50,
                              top_p: float = 1.0, repetition_penalty: float = 1.05, max_tokens: int = 2048,
                              on_token: Optional[Callable[[int], None]] = None, *, seed: int = 0, text_ids=None,
                              instruct_ids=None, target_token_count=None) -> np.ndarray:
        """generateCustomVoice(text:speaker:language:instruct:...:onToken:) (Qwen3.swift:783-794)."""
        req = self._request_from_text(text, speaker, instruct, language, max_tokens, text_ids, instruct_ids, target_token_count)
        req.route = 2
        return self._one(req, temperature, top_k, top_p, repetition_penalty, seed, on_token)

    def _one(self, req, temperature, top_k, top_p, repetition_penalty, seed, on_token) -> np.ndarray:
        cb = (lambda i, k, p: on_token(p) if k == "token" else None) if on_token else None
        r = self.generate_batch([req], temperature, top_k, top_p, repetition_penalty, seed, on_event=cb)[0]
        if r.status != 0:
            raise Qwen3TTSError(r.status, "Generation failed: No tokens generated")
        return r.audio

    def generate_stream(self, text: Optional[str] = None, speaker: Optional[str] = None,
                        instruct: Optional[str] = None, language: str = "auto", temperature: float = 0.9,
                        top_k: int = 50, top_p: float = 1.0, repetition_penalty: float = 1.05,
                        max_tokens: int = 2048, *, seed: int = 0, text_ids=None, instruct_ids=None,
                        target_token_count=None) -> Iterator[Tuple[str, object]]:
        """generateStream (Qwen3+Streaming.swift:8-125): yields ("token", id)..., ("info", info), ("audio", pcm)."""
        req = self._request_from_text(text, speaker, instruct, language, max_tokens, text_ids, instruct_ids,
                                      target_token_count)
        events: List[Tuple[str, object]] = []
        res = self.generate_batch([req], temperature, top_k, top_p, repetition_penalty, seed,
                                  on_event=lambda i, k, p: events.append((k, p)))
        if res[0].status != 0:
            raise Qwen3TTSError(res[0].status, "Generation failed: No tokens generated")
        yield from events

    def generate_voice_clone(self, text: Optional[str] = None, reference_audio: Optional[np.ndarray] = None,
                             reference_text: Optional[str] = None, language: str = "auto", temperature: float = 0.9,
                             top_k: int = 50, top_p: float = 1.0, repetition_penalty: float = 1.5,
                             max_tokens: int = 2048, *, seed: int = 0, text_ids: Optional[Sequence[int]] = None,
                             ref_text_ids: Optional[Sequence[int]] = None,
                             target_token_count: Optional[int] = None, sample_rate: Optional[int] = None) -> np.ndarray:
        """generateVoiceClone(text:referenceAudio:referenceText:language:...) (Qwen3.swift:1009-1203): repetition
        penalty defaults to 1.5 on this path. Returns the audio of `text` only. sample_rate: the reference clip's rate; given
        and not 24000, the clip is resampled on the device first (without it the clip is taken as 24 kHz, as before)."""
        if sample_rate is not None and int(sample_rate) != 24000:
            reference_audio = self.resample(reference_audio, int(sample_rate), 24000, centred=True)
        if text_ids is None:
            if self.tokenizer is None:
                raise Qwen3TTSError(1, "Model not initialized: Tokenizer not loaded")  # Qwen3.swift:424-426
            t = chat_template_ids(self.tokenizer, text)
            text_ids, target_token_count = t["text_ids"], t["target_token_count"]
            ref_text_ids = self.tokenizer(f"<|im_start|>assistant\n{reference_text}<|im_end|>\n")
        req = GenerationRequest(text_ids, int(target_token_count or 0), None, None, language, max_tokens,
                                ref_audio=reference_audio, ref_text_ids=ref_text_ids)
        r = self.generate_batch([req], temperature, top_k, top_p, repetition_penalty, seed)[0]
        if r.status != 0:
            raise Qwen3TTSError(r.status, "Generation failed: No tokens generated")
        return r.audio

    # -- codec only ------------------------------------------------------------------------------
    def codec_encode(self, audio: np.ndarray) -> np.ndarray:
        """Qwen3TTSSpeechTokenizer.encode (SpeechTokenizer.swift:841-846): waveform [S] -> codes [16][T] int32."""
        a = np.ascontiguousarray(np.asarray(audio, np.float32).reshape(-1))
        cap = max(1, int(self._lib.q3tts_codec_encoded_frames(self._h, a.size)))
        codes = np.zeros((16, cap), np.int32)
        n = C.c_int32(0)
        self._check(self._lib.q3tts_codec_encode(self._h, a.ctypes.data_as(L.f32p), a.size, codes.ctypes.data_as(L.i32p),
                                                 cap, C.byref(n)))
        return codes.reshape(-1)[: 16 * n.value].reshape(16, n.value)

    def extract_speaker_embedding(self, audio: np.ndarray, sample_rate: int = 24000) -> np.ndarray:
        """extractSpeakerEmbedding (Qwen3.swift:222-249) -> float32 [enc_dim]."""
        a = np.ascontiguousarray(np.asarray(audio, np.float32).reshape(-1))
        out = np.zeros(max(1, self.info.speaker_embedding_dim), np.float32)
        self._check(self._lib.q3tts_speaker_embedding(self._h, a.ctypes.data_as(L.f32p), a.size, sample_rate,
                                                      out.ctypes.data_as(L.f32p), out.size))
        return out

    def debug_frontend_stage(self, audio: np.ndarray, stage: str, cap_floats: int = 1 << 26) -> np.ndarray:
        a = np.ascontiguousarray(np.asarray(audio, np.float32).reshape(-1))
        out = np.zeros(cap_floats, np.float32)
        T, Cc = C.c_int32(0), C.c_int32(0)
        self._check(self._lib.q3tts_debug_frontend_stage(self._h, a.ctypes.data_as(L.f32p), a.size, stage.encode(),
                                                         out.ctypes.data_as(L.f32p), out.size, C.byref(T), C.byref(Cc)))
        return out[: T.value * Cc.value].reshape(T.value, Cc.value).copy()

    def codec_decode(self, codes: np.ndarray, n_frames: Optional[Sequence[int]] = None):
        """Qwen3TTSSpeechTokenizer.decode (SpeechTokenizer.swift:823-836). codes [B][F][16] int32."""
        codes = np.ascontiguousarray(codes, np.int32)
        if codes.ndim == 2:
            codes = codes[None]
        B, F, _ = codes.shape
        nf = np.ascontiguousarray(n_frames if n_frames is not None else [F] * B, np.int32)
        up = self.info.samples_per_frame
        pcm = np.zeros((B, F * up), np.float32)
        lens = np.zeros(B, np.int64)
        self._check(self._lib.q3tts_codec_decode(self._h, codes.ctypes.data_as(L.i32p), nf.ctypes.data_as(L.i32p), B, F,
                                                 pcm.ctypes.data_as(L.f32p), lens.ctypes.data_as(C.POINTER(C.c_int64))))
        return pcm, lens

    # -- test hooks -------------------------------------------------------------------------------
    def codec_decode_streamed(self, codes: np.ndarray, chunk_frames: int, window: int, lookahead: int = 4,
                              n_frames: Optional[Sequence[int]] = None) -> np.ndarray:
        """The decode the way a stream produces it (q3tts_codec_decode_streamed): window < 0 = pre-transformer over all
        frames (bit-identical to codec_decode); otherwise a sliding window. Returns pcm [batch][max_frames * 1920]."""
        codes = np.ascontiguousarray(codes, np.int32)
        if codes.ndim == 2:
            codes = codes[None]
        B, F, G = codes.shape
        nf = np.asarray(n_frames if n_frames is not None else [F] * B, np.int32)
        pcm = np.zeros((B, F * self.info.samples_per_frame), np.float32)
        self._check(self._lib.q3tts_codec_decode_streamed(self._h, codes.ctypes.data_as(L.i32p), nf.ctypes.data_as(L.i32p), B, F,
                                                          chunk_frames, window, lookahead, pcm.ctypes.data_as(L.f32p)))
        return pcm

    def codec_decode_streamed_prefixed(self, codes: np.ndarray, n_prefix: Sequence[int], n_frames: Sequence[int], chunk_frames: int,
                                       window: int, lookahead: int = 4) -> np.ndarray:
        """The streamed decode of rows that carry a reference prefix, as a streamed voice-clone row is decoded
        (q3tts_codec_decode_streamed_prefixed): codes [batch][max_frames][16] hold n_prefix[b] reference frames, then n_frames[b]
        generated ones. Returns pcm [batch][max(n_frames) * 1920]: row b's first n_frames[b] * 1920 samples, the reference's cut."""
        codes = np.ascontiguousarray(codes, np.int32)
        B, F, G = codes.shape
        npre, nf = np.asarray(n_prefix, np.int32), np.asarray(n_frames, np.int32)
        assert npre.shape == (B,) and nf.shape == (B,) and G == 16
        pcm = np.zeros((B, max(int(nf.max()), 0) * self.info.samples_per_frame), np.float32)
        self._check(self._lib.q3tts_codec_decode_streamed_prefixed(self._h, codes.ctypes.data_as(L.i32p), npre.ctypes.data_as(L.i32p),
                                                                   nf.ctypes.data_as(L.i32p), B, F, int(chunk_frames), int(window),
                                                                   int(lookahead), pcm.ctypes.data_as(L.f32p)))
        return pcm

    def debug_prefix_states(self) -> Tuple[int, int, int]:
        """The voices' saved tail states for streamed requests (q3tts_debug_prefix_states): how many are held, their device
        bytes, and how many admissions have been served from one since the model was loaded."""
        n, b, r = C.c_int32(0), C.c_int64(0), C.c_int64(0)
        self._check(self._lib.q3tts_debug_prefix_states(self._h, C.byref(n), C.byref(b), C.byref(r)))
        return n.value, b.value, r.value

    def debug_codec_stream_slots(self, codes: np.ndarray, n_frames: Sequence[int], slots: int, burst: int, chunk_frames: int,
                                 window: int, lookahead: int) -> np.ndarray:
        """The slotted codec stream of a streamed queue without the talker (q3tts_debug_codec_stream_slots): codes
        [n_reqs][max_frames][16]; requests take `slots` rows in order and gain `burst` frames per step. Returns pcm
        [n_reqs][max_frames * 1920], request i equal to codec_decode_streamed of it alone."""
        codes = np.ascontiguousarray(codes, np.int32)
        N, F, G = codes.shape
        nf = np.asarray(n_frames, np.int32)
        assert nf.shape == (N,) and G == 16
        pcm = np.zeros((N, F * self.info.samples_per_frame), np.float32)
        self._check(self._lib.q3tts_debug_codec_stream_slots(self._h, codes.ctypes.data_as(L.i32p), nf.ctypes.data_as(L.i32p), N, F,
                                                             int(slots), int(burst), int(chunk_frames), int(window), int(lookahead),
                                                             pcm.ctypes.data_as(L.f32p)))
        return pcm

    def debug_prepare_inputs(self, req: GenerationRequest):
        arr, keep = self._marshal([req])
        H = self.info.hidden_size
        cap = 1024
        ie = np.zeros((cap, H), np.uint16)
        tr = np.zeros((cap, H), np.uint16)
        pad = np.zeros((H,), np.uint16)
        n1, n2 = C.c_int32(), C.c_int32()
        self._check(self._lib.q3tts_debug_prepare_inputs(self._h, arr, ie.ctypes.data_as(L.u16p), cap, C.byref(n1),
                                                         tr.ctypes.data_as(L.u16p), cap, C.byref(n2),
                                                         pad.ctypes.data_as(L.u16p)))
        del keep
        return ie[: n1.value].copy(), tr[: n2.value].copy(), pad

    def debug_generate_forced(self, reqs: Sequence[GenerationRequest], forced_codes: np.ndarray, temperature=0.0,
                              top_k=50, top_p=1.0, repetition_penalty=1.05, seed=0, row_base=0):
        arr, keep = self._marshal(reqs)
        n = len(reqs)
        forced = np.ascontiguousarray(forced_codes, np.int32).reshape(n, -1, 16)
        F = forced.shape[1]
        V, Vc, G = self.info.vocab_size, self.info.cp_vocab_size, self.info.num_code_groups
        tl = np.zeros((n, F, V), np.uint16)
        cl = np.zeros((n, F, G - 1, Vc), np.uint16)
        sampled = np.zeros((n, F, 16), np.int32)
        s = self._sampling(temperature, top_k, top_p, repetition_penalty, seed, 0, row_base=row_base, reqs=reqs)
        self._check(self._lib.q3tts_debug_generate_forced(
            self._h, arr, n, C.byref(s), forced.ctypes.data_as(L.i32p), F, tl.ctypes.data_as(L.u16p),
            cl.ctypes.data_as(L.u16p), sampled.ctypes.data_as(L.i32p)))
        del keep
        return tl, cl, sampled

    def debug_sample(self, logits: np.ndarray, temperature=0.9, top_k=50, top_p=1.0, repetition_penalty=1.0,
                     seed=0, seen: Optional[np.ndarray] = None, suppress=(0, 0), eos_id=-1, row0=0, draw=0,
                     mask_eos=False, per_row: Optional[Sequence[Optional[RequestSampling]]] = None):
        """`per_row`: one RequestSampling (or None) per row of `logits`, folded into the keywords like a request's."""
        logits = np.ascontiguousarray(logits, np.uint16)
        rows, V = logits.shape
        s = self._sampling(temperature, top_k, top_p, repetition_penalty, seed, 1 if mask_eos else 0)
        if per_row is not None:
            assert len(per_row) == rows
            s._rows = self._row_sampling(per_row)
            if s._rows is not None:
                s.per_request = C.cast(s._rows, C.POINTER(L.RowSampling))
        toks = np.zeros(rows, np.int32)
        sp = np.ascontiguousarray(seen, np.uint8).ctypes.data_as(L.u8p) if seen is not None else None
        self._check(self._lib.q3tts_debug_sample(self._h, logits.ctypes.data_as(L.u16p), rows, V, C.byref(s), sp,
                                                 suppress[0], suppress[1], eos_id, row0, draw,
                                                 toks.ctypes.data_as(L.i32p)))
        return toks

    def debug_text_resume(self, tables: np.ndarray, codes, text_row: np.ndarray):
        """q3tts_debug_text_resume: tables [16][V][H] bf16 bits, codes [16], text_row [H] -> (h [3][H] uint16, ss [3], state [3][8])
        for (0) the end of a frame with its text row, (1) the same frame starving, (2) its resume by the append launch."""
        tables = np.ascontiguousarray(tables, np.uint16)
        _, V, H = tables.shape
        codes = np.ascontiguousarray(codes, np.int32)
        text_row = np.ascontiguousarray(text_row, np.uint16)
        assert tables.shape[0] == 16 and codes.shape == (16,) and text_row.shape == (H,)
        h, ss, state = np.zeros((3, H), np.uint16), np.zeros(3, np.float32), np.zeros((3, 8), np.int32)
        self._check(self._lib.q3tts_debug_text_resume(self._h, H, V, tables.ctypes.data_as(L.u16p), codes.ctypes.data_as(L.i32p),
                                                      text_row.ctypes.data_as(L.u16p), h.ctypes.data_as(L.u16p),
                                                      ss.ctypes.data_as(L.f32p), state.ctypes.data_as(L.i32p)))
        return h, ss, state

    def debug_linear(self, x: np.ndarray, W: np.ndarray, bias: Optional[np.ndarray] = None) -> np.ndarray:
        x = np.ascontiguousarray(x, np.uint16)
        W = np.ascontiguousarray(W, np.uint16)
        M, K = x.shape
        N = W.shape[0]
        y = np.zeros((M, N), np.uint16)
        bp = np.ascontiguousarray(bias, np.uint16).ctypes.data_as(L.u16p) if bias is not None else None
        self._check(self._lib.q3tts_debug_linear(self._h, x.ctypes.data_as(L.u16p), W.ctypes.data_as(L.u16p), bp, M, K, N,
                                                 y.ctypes.data_as(L.u16p)))
        return y

    def debug_attention(self, qkv: np.ndarray, qn_w: np.ndarray, kn_w: np.ndarray, rope_cos: np.ndarray, rope_sin: np.ndarray,
                        kpool: np.ndarray, vpool: np.ndarray, *, n_heads: int, n_kv: int, B: int, kv_len=None, active=None,
                        block_table=None, max_pages: int = 1, eps: float = 1e-6, scale: float = 128.0 ** -0.5,
                        fixed_len: int = -1, identity_pages: int = 0, chunk: int = 0, chunk_n_prompt=None,
                        chunk_r_base: int = 0, nt_kv: int = 0):
        """One launch of the decode attention on these buffers (q3tts_debug_attention). qkv [max(chunk, 1) * B][(n_heads +
        2 n_kv) * 128], pools [n_pages][n_kv][64][128], all bf16 bit patterns. Returns (out [rows][n_heads * 128], kpool,
        vpool): the pools as the launch left them; the arguments are not modified."""
        rows = max(chunk, 1) * B
        u16 = lambda x: np.ascontiguousarray(x, np.uint16)
        i32 = lambda x: None if x is None else np.ascontiguousarray(x, np.int32)
        qkv, qn_w, kn_w, rope_cos, rope_sin = u16(qkv), u16(qn_w), u16(kn_w), u16(rope_cos), u16(rope_sin)
        kpool, vpool = u16(kpool).copy(), u16(vpool).copy()
        if qkv.shape != (rows, (n_heads + 2 * n_kv) * 128) or qn_w.shape != (128,) or kn_w.shape != (128,):
            raise ValueError("debug_attention: qkv / norm weight shape")
        if rope_cos.ndim != 2 or rope_cos.shape[1] != 128 or rope_sin.shape != rope_cos.shape:
            raise ValueError("debug_attention: RoPE table shape")
        if kpool.ndim != 4 or kpool.shape[1:] != (n_kv, 64, 128) or vpool.shape != kpool.shape:
            raise ValueError("debug_attention: pool shape")
        kv_len, block_table, chunk_n_prompt = i32(kv_len), i32(block_table), i32(chunk_n_prompt)
        active = None if active is None else np.ascontiguousarray(active, np.uint8)
        for arr, shape in ((kv_len, (B,)), (active, (B,)), (block_table, (B, max_pages)), (chunk_n_prompt, (B,))):
            if arr is not None and arr.shape != shape:
                raise ValueError("debug_attention: per-row argument shape")
        out = np.zeros((rows, n_heads * 128), np.uint16)
        ptr = lambda x, t: None if x is None else x.ctypes.data_as(t)
        a = L.AttnDebug(n_heads, n_kv, B, eps, scale, max_pages, fixed_len, identity_pages, chunk, chunk_r_base, nt_kv,
                        rope_cos.shape[0], kpool.shape[0], ptr(qkv, L.u16p), ptr(qn_w, L.u16p), ptr(kn_w, L.u16p),
                        ptr(rope_cos, L.u16p), ptr(rope_sin, L.u16p), ptr(kv_len, L.i32p), ptr(active, L.u8p),
                        ptr(block_table, L.i32p), ptr(chunk_n_prompt, L.i32p), ptr(kpool, L.u16p), ptr(vpool, L.u16p),
                        ptr(out, L.u16p))
        self._check(self._lib.q3tts_debug_attention(self._h, C.byref(a)))
        return out, kpool, vpool

    def debug_gemm(self, *, x=None, W=None, y=None, M=0, epi=0, W_up=None, scales=None, biases=None, scales_up=None, biases_up=None,
                   bias=None, norm_w=None, ss_in=None, norm_dim=0, norm_eps=1e-6, ss_out=None, act_silu=0, resid=0, nt_weights=0,
                   y_tiled=0, N=None, rider=None, mode=0):
        """One launch of the decode GEMM on these host buffers (q3tts_debug_gemm); bf16 operands as uint16 bit patterns.
        x [16 * xMB][K]; W [N][K] bf16, or uint32 [N][K / 8] with scales / biases [N][K / 64] (int4); epi 2: W the gate and W_up
        the up matrix; y [16 * yMB][y_cols] and ss_out [N / 16][ss_ld] as the caller filled them (copied, returned as the launch
        left them); ss_in [ss_count][ss_ld]. N defaults to W's rows. rider: dict(h [16 * MB][H], w [H], out like h, M, eps,
        ss_in [count][16 * MB] or None, ss_out [16 * MB] or None); mode 1 runs launch_norm_rows alone on it.
        Returns a dict: y, ss_out, rider_out, rider_ss_out (those that apply) and the geometry fields (_lib.GEOM_FIELDS)."""
        u16 = lambda v: None if v is None else np.ascontiguousarray(v, np.uint16)
        f32 = lambda v: None if v is None else np.ascontiguousarray(v, np.float32)
        ptr = lambda v, t: None if v is None else v.ctypes.data_as(t)
        a = L.GemmDebug(mode=mode)
        keep = []
        if mode == 0:
            quant = scales is not None
            x, y = u16(x), u16(y).copy()
            Wg = np.ascontiguousarray(W, np.uint32 if quant else np.uint16)
            Wu = None if W_up is None else np.ascontiguousarray(W_up, np.uint32 if quant else np.uint16)
            K = x.shape[1]
            N = Wg.shape[0] if N is None else N
            if Wg.shape != (N, K // 8 if quant else K) or (Wu is not None and Wu.shape != Wg.shape) or x.shape[0] % 16 or y.shape[0] % 16:
                raise ValueError("debug_gemm: operand shape")
            sc, bi, scu, biu, bias, norm_w = u16(scales), u16(biases), u16(scales_up), u16(biases_up), u16(bias), u16(norm_w)
            for v in (sc, bi, scu, biu):
                if v is not None and v.shape != (N, K // 64):
                    raise ValueError("debug_gemm: scales / biases shape")
            ss_in, ss_out = f32(ss_in), (None if ss_out is None else f32(ss_out).copy())
            ss_ld = ss_in.shape[1] if ss_in is not None else (ss_out.shape[1] if ss_out is not None else y.shape[0])
            if (bias is not None and bias.shape != (N,)) or (norm_w is not None and norm_w.shape != (K,)) or \
                    (ss_out is not None and ss_out.shape != (N // 16, ss_ld)) or (ss_in is not None and ss_in.ndim != 2):
                raise ValueError("debug_gemm: per-column / per-row operand shape")
            a.M, a.K, a.N, a.xMB, a.yMB, a.ss_ld, a.y_cols = M, K, N, x.shape[0] // 16, y.shape[0] // 16, ss_ld, y.shape[1]
            a.epi, a.act_silu, a.resid, a.nt_weights, a.y_tiled = epi, act_silu, resid, nt_weights, y_tiled
            a.norm, a.quant, a.has_bias = int(norm_w is not None), int(quant), int(bias is not None)
            a.ss_count, a.norm_dim, a.norm_eps = (ss_in.shape[0] if ss_in is not None else 0), norm_dim, norm_eps
            a.x, a.W, a.scales, a.biases = ptr(x, L.u16p), Wg.ctypes.data_as(C.c_void_p), ptr(sc, L.u16p), ptr(bi, L.u16p)
            a.W_up = None if Wu is None else Wu.ctypes.data_as(C.c_void_p)
            a.scales_up, a.biases_up, a.bias, a.norm_w = ptr(scu, L.u16p), ptr(biu, L.u16p), ptr(bias, L.u16p), ptr(norm_w, L.u16p)
            a.ss_in, a.y, a.ss_out = ptr(ss_in, L.f32p), ptr(y, L.u16p), ptr(ss_out, L.f32p)
            keep += [x, y, Wg, Wu, sc, bi, scu, biu, bias, norm_w, ss_in, ss_out]
        r_out = r_sso = None
        if rider is not None:
            rh, rw, r_out = u16(rider["h"]), u16(rider["w"]), u16(rider["out"]).copy()
            r_ssi = f32(rider.get("ss_in"))
            r_sso = None if rider.get("ss_out") is None else f32(rider["ss_out"]).copy()
            H = rh.shape[1]
            if rh.shape[0] % 16 or r_out.shape != rh.shape or rw.shape != (H,) or (r_ssi is not None and r_ssi.shape[1:] != (rh.shape[0],)) \
                    or (r_sso is not None and r_sso.shape != (rh.shape[0],)):
                raise ValueError("debug_gemm: rider shape")
            a.rider_M, a.rider_H, a.rider_MB, a.rider_eps = rider["M"], H, rh.shape[0] // 16, rider.get("eps", 1e-6)
            a.rider_ss_count = r_ssi.shape[0] if r_ssi is not None else 0
            a.rider_h, a.rider_w, a.rider_ss_in = ptr(rh, L.u16p), ptr(rw, L.u16p), ptr(r_ssi, L.f32p)
            a.rider_out, a.rider_ss_out = ptr(r_out, L.u16p), ptr(r_sso, L.f32p)
            keep += [rh, rw, r_ssi]
        self._check(self._lib.q3tts_debug_gemm(self._h, C.byref(a)))
        del keep
        res = {f: int(getattr(a, f)) for f in L.GEOM_FIELDS}
        res.update(y=y if mode == 0 else None, ss_out=ss_out if mode == 0 else None, rider_out=r_out, rider_ss_out=r_sso)
        return res

    def debug_conv(self, kind, *, frames, x, w, K, dil=1, ppf=1, hist=0, margin=None, split=0, Cin=None, N=None, w2=None, bias=None, bias2=None,
                   scale=None, snake=None, act2=None, post=None, post_C=0, res=None, res_is_out=0, out=None, out2=None, x2=None,
                   act=0, pre_act=0, shift=0, reflect=0, x_f32=0, pcm=None, nonfinite=None):
        """One launch of a codec conv launcher on these host buffers (q3tts_debug_conv; kind as in q3tts.h). x [B][Tmax][ldx]
        (float32, or float16 bit patterns as uint16 for kinds 2 / 3 / 5 without x_f32), Tmax = the allocation's rows with the
        sequences `margin` (default hist) rows in; w float32 [N][K][Cin]; snake / act2 / post: (alpha, beta) pairs of raw SnakeBeta parameters;
        out / out2 [B][Tmax][ldo], pcm [B][Tmax] and nonfinite [B] as the caller filled them (copied, returned as the launch left
        them). Cin / N default to w's shape. Returns a dict: out, out2, pcm, nonfinite (those given) and _lib.CONV_GEOM_FIELDS."""
        f32 = lambda v: None if v is None else np.ascontiguousarray(v, np.float32)
        h1 = kind in (2, 3, 5)
        act_t = lambda v, f=False: None if v is None else np.ascontiguousarray(v, np.float32 if (f or not h1) else np.uint16)
        ptr = lambda v, t=L.f32p: None if v is None else v.ctypes.data_as(t)
        x, w, w2, bias, bias2, scale, x2 = act_t(x, bool(x_f32)), f32(w), f32(w2), f32(bias), f32(bias2), f32(scale), f32(x2)
        res = act_t(res)
        out, out2 = (None if out is None else act_t(out).copy()), (None if out2 is None else act_t(out2).copy())
        pcm = None if pcm is None else f32(pcm).copy()
        nonfinite = None if nonfinite is None else np.ascontiguousarray(nonfinite, np.int32).copy()
        frames = np.ascontiguousarray(frames, np.int32)
        if x.ndim != 3 or x.shape[0] != frames.shape[0] or w.ndim != 3 or w.shape[1] != K:
            raise ValueError("debug_conv: operand shape")
        B, Tmax, ldx = x.shape
        Cin = w.shape[2] if Cin is None else Cin
        N = w.shape[0] if N is None else N
        for v in (out, out2, res):
            if v is not None and (v.ndim != 3 or v.shape[:2] != (B, Tmax)):
                raise ValueError("debug_conv: out / out2 / res shape")
        if (out is not None and out2 is not None and out.shape != out2.shape) or (x2 is not None and (x2.ndim != 2 or x2.shape[0] != Tmax)) or \
                (pcm is not None and pcm.shape != (B, Tmax)) or (nonfinite is not None and nonfinite.shape != (B,)) or \
                (w2 is not None and w2.shape != (N, N)) or w.shape != (1 if kind >= 4 else N, K, Cin):
            raise ValueError("debug_conv: operand shape")
        pairs = []
        for pr, n in ((snake, Cin), (act2, N), (post, N if kind in (1, 3) else post_C)):
            if pr is None:
                pairs += [None, None]
                continue
            al, be = f32(pr[0]), f32(pr[1])
            if al.shape != (n,) or be.shape != (n,):
                raise ValueError("debug_conv: SnakeBeta parameter shape")
            pairs += [al, be]
        for v, n in ((bias, 1 if kind >= 4 else N), (bias2, N), (scale, N)):
            if v is not None and v.shape != (n,):
                raise ValueError("debug_conv: per-channel operand shape")
        o = out if out is not None else out2
        a = L.ConvDebug(kind=kind, split=split, B=B, Tmax=Tmax, ppf=ppf, hist=hist, margin=hist if margin is None else margin, Cin=Cin, N=N, K=K, dil=dil, ldx=ldx,
                        ldo=0 if o is None else o.shape[2], ldr=(o.shape[2] if res_is_out else (0 if res is None else res.shape[2])),
                        ldx2=0 if x2 is None else x2.shape[1], act=act, pre_act=pre_act, shift=shift, reflect=reflect, post_C=post_C,
                        x_f32=x_f32, res_is_out=res_is_out)
        vp = C.c_void_p
        a.frames, a.x, a.x2, a.w, a.w2 = ptr(frames, L.i32p), ptr(x, vp), ptr(x2), ptr(w), ptr(w2)
        a.bias, a.bias2, a.scale = ptr(bias), ptr(bias2), ptr(scale)
        a.snake_alpha, a.snake_beta, a.act2_alpha, a.act2_beta, a.post_alpha, a.post_beta = [ptr(v) for v in pairs]
        a.res, a.out, a.out2, a.pcm, a.nonfinite = ptr(res, vp), ptr(out, vp), ptr(out2, vp), ptr(pcm), ptr(nonfinite, L.i32p)
        self._check(self._lib.q3tts_debug_conv(self._h, C.byref(a)))
        r = {f: int(getattr(a, f)) for f in L.CONV_GEOM_FIELDS}
        r.update(out=out, out2=out2, pcm=pcm, nonfinite=nonfinite)
        return r

    def debug_rowop(self, op, p, f=(), ins=(), ios=()):
        """One launch of a row kernel's launcher on these host buffers (q3tts_debug_rowop; the slot table per op: q3tts.h). op: a
        name of _lib.ROWOPS; ins: read-only numpy arrays (or None) in slot order; ios: the in/out arrays, copied, launched on and
        returned as the launch left them."""
        ios = [None if v is None else np.ascontiguousarray(v).copy() for v in ios]
        ins = [None if v is None else np.ascontiguousarray(v) for v in ins]
        self._check(L.rowop(self._h, op, p, f, ins, ios))
        return ios

    def debug_lmop(self, op, p, ins=None, ios=None):
        """One launch of a frame-step row kernel's launcher on these host buffers (q3tts_debug_lmop; the slot table per op:
        q3tts.h). op: a name of _lib.LMOPS; p: {index: value}; ins: {slot: read-only numpy array}; ios: {slot: in/out array},
        copied, launched on and returned (a dict by slot) as the launch left them."""
        ios = {i: np.ascontiguousarray(v).copy() for i, v in (ios or {}).items() if v is not None}
        ins = {i: np.ascontiguousarray(v) for i, v in (ins or {}).items() if v is not None}
        self._check(L.lmop(self._h, op, p, ins, ios))
        return ios

    def debug_codec_stage(self, codes: np.ndarray, stage: str) -> np.ndarray:
        codes = np.ascontiguousarray(codes, np.int32).reshape(-1, 16)
        F = codes.shape[0]
        cap = F * self.info.samples_per_frame * 128
        out = np.zeros(cap, np.float32)
        T, Cc = C.c_int32(), C.c_int32()
        self._check(self._lib.q3tts_debug_codec_stage(self._h, codes.ctypes.data_as(L.i32p), F, stage.encode(),
                                                      out.ctypes.data_as(L.f32p), cap, C.byref(T), C.byref(Cc)))
        return out[: T.value * Cc.value].reshape(T.value, Cc.value).copy()


class Session:
    """An open serving session (Qwen3TTSModel.open_session). submit / result / cancel / stats may be called from any thread,
    submit and cancel also from inside `on_event`; result and close may not (they would wait for the thread they run on)."""

    def __init__(self, model: Qwen3TTSModel, handle: C.c_void_p, cb):
        self._model, self._h, self._cb = model, handle, cb  # (the callback object lives as long as the session's thread)

    def _handle(self):
        if not self._h or not self._model._h:
            raise Qwen3TTSError(3, "Invalid input: the session has been closed")
        return self._h

    def submit(self, request: GenerationRequest, **row_sampling) -> int:
        """Returns the request's ticket. Keywords (temperature, top_k, top_p, repetition_penalty, seed) override
        `request.sampling` for this submit; `request.voice` is honoured. Status 9 (Qwen3TTSError) when max_pending wait."""
        m = self._model
        arr, keep = m._marshal([request])
        rs = RequestSampling(**row_sampling) if row_sampling else getattr(request, "sampling", None)
        rows = m._row_sampling([rs])
        voice = getattr(request, "voice", None)
        if voice is not None and not voice._h:
            raise Qwen3TTSError(3, "Invalid input: the voice of the request has been closed")
        t = C.c_int64(-1)
        st = m._lib.q3tts_session_submit(self._handle(), arr, voice._h if voice is not None else None,
                                         rows if rows is not None else None, C.byref(t))
        del keep
        m._check(st)
        return int(t.value)

    def submit_open(self, request: GenerationRequest, **row_sampling) -> int:
        """q3tts_session_submit_open: an open-text request. `request.text_ids` holds the 3 role tokens and the content that is
        there already (at least one token) and NO 5-token tail; target_token_count is ignored. The rest of the text arrives
        through append_text; the result equals the ordinary request over the whole text alone. A request with a voice or
        reference audio is refused (status 3)."""
        m = self._model
        if getattr(request, "voice", None) is not None:
            raise Qwen3TTSError(3, "Invalid input: an open-text request cannot name a voice (the ICL prompt holds the whole text)")
        arr, keep = m._marshal([request])
        rs = RequestSampling(**row_sampling) if row_sampling else getattr(request, "sampling", None)
        rows = m._row_sampling([rs])
        t = C.c_int64(-1)
        st = m._lib.q3tts_session_submit_open(self._handle(), arr, rows if rows is not None else None, C.byref(t))
        del keep
        m._check(st)
        return int(t.value)

    def append_text(self, ticket: int, ids, final: bool = False) -> None:
        """More content token ids for an open-text ticket; final=True closes its text. May be called from any thread and from
        inside `on_event`. Text for a ticket that has already completed or was cancelled is dropped without an error."""
        a = np.ascontiguousarray(ids, np.int32).reshape(-1)
        self._model._check(self._model._lib.q3tts_session_append_text(self._handle(), int(ticket), a.ctypes.data_as(L.i32p),
                                                                       int(a.size), 1 if final else 0))

    def close_text(self, ticket: int) -> None:
        """The ticket's text ends with what has been appended."""
        self.append_text(ticket, [], final=True)

    def text_stats(self) -> L.SessionTextStats:
        s = L.SessionTextStats()
        self._model._check(self._model._lib.q3tts_session_get_text_stats(self._handle(), C.byref(s)))
        return s

    def result(self, ticket: int, timeout: Optional[float] = None) -> GenerationResult:
        """Waits for the ticket's result and takes it (a second call for the same ticket is status 3). A cancelled
        request's result has status 8 and no audio. TimeoutError when `timeout` seconds pass first."""
        m = self._model
        res = (L.Result * 1)()
        ready = C.c_int32(0)
        ms = -1 if timeout is None else max(0, int(round(timeout * 1000)))
        st = m._lib.q3tts_session_wait(self._handle(), int(ticket), ms, res, C.byref(ready))
        if st == 0 and not ready.value:
            raise TimeoutError("ticket %d was not ready after %s s" % (ticket, timeout))
        if st != 0:
            m._check(st)
        return m._collect(0, res, 1, set_last=False)[0]

    def cancel(self, ticket: int) -> None:
        self._model._check(self._model._lib.q3tts_session_cancel(self._handle(), int(ticket)))

    def stats(self) -> L.SessionStats:
        s = L.SessionStats()
        self._model._check(self._model._lib.q3tts_session_get_stats(self._handle(), C.byref(s)))
        return s

    def create_voice(self, ref_audio: np.ndarray, ref_text_ids: Sequence[int], sample_rate: int = 24000) -> Voice:
        """q3tts_session_voice_create on a session opened with live_voices > 0: the clip's front end runs beside the rows in
        flight. Returns at once; the voice may be named by submit before it is ready (the request is admitted once it is),
        Voice.wait() blocks until then. Any thread, also from inside `on_event`. Status 9 (Qwen3TTSError) when live_voices
        jobs are in flight or max_voices voices are alive. After the session has closed the voice is an ordinary voice of
        the model."""
        m = self._model
        ra = np.ascontiguousarray(np.asarray(ref_audio, np.float32).reshape(-1))
        rt = np.ascontiguousarray(ref_text_ids, np.int32)
        h = C.c_void_p()
        m._check(m._lib.q3tts_session_voice_create(self._handle(), ra.ctypes.data_as(L.f32p), ra.size, int(sample_rate),
                                                   rt.ctypes.data_as(L.i32p), rt.size, C.byref(h)))
        return Voice(m, h, self)

    def voice_stats(self) -> L.SessionVoiceStats:
        s = L.SessionVoiceStats()
        self._model._check(self._model._lib.q3tts_session_get_voice_stats(self._handle(), C.byref(s)))
        return s

    def close(self, drain: bool = True) -> None:
        """drain: everything accepted finishes first; otherwise whatever is pending or running is cancelled. Results not
        collected before are gone."""
        if self._h and self._model._h:
            h, self._h = self._h, None
            st = self._model._lib.q3tts_session_close(h, 1 if drain else 0)
            if st == 3 and self._model._h:  # refused (called from on_event): the session is still open
                self._h = h
            self._model._check(st)
        self._h = None if not self._model._h else self._h

    def __enter__(self) -> "Session":
        return self

    def __exit__(self, *exc):
        self.close(drain=exc[0] is None)


class NativeTokenizer:
    """The engine's own Qwen2 byte-level BPE (csrc/tokenizer.cc) behind q3tts_tokenizer_*: a callable text -> ids, usable
    as `Qwen3TTSModel.tokenizer`. `path` is a model directory or a tokenizer.json file."""

    def __init__(self, path: str):
        self._lib = L.lib()
        h = C.c_void_p()
        st = self._lib.q3tts_tokenizer_load(path.encode(), C.byref(h))
        if st != 0:
            raise Qwen3TTSError(st, (self._lib.q3tts_last_error(None) or b"").decode())
        self._h = h

    def __call__(self, text: str) -> List[int]:
        n = C.c_int32(0)
        raw = text.encode("utf-8")
        cap = max(16, len(raw) + 8)  # a token covers at least one byte
        ids = np.zeros(cap, np.int32)
        st = self._lib.q3tts_tokenizer_encode(self._h, raw, ids.ctypes.data_as(L.i32p), cap, C.byref(n))
        if st != 0:
            raise Qwen3TTSError(st, (self._lib.q3tts_last_error(None) or b"").decode())
        return ids[: n.value].tolist()

    def close(self):
        if getattr(self, "_h", None):
            self._lib.q3tts_tokenizer_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
