"""Streamed voice-clone audio: a clone row's decoder runs over [reference ++ generated] frames, so a streamed clone row carries
a reference prefix in front of its stream (include/q3tts.h, q3tts_codec_decode_streamed_prefixed). The prefix is decoded chunk
by chunk with its lookahead stopping at the reference's end, delivers nothing, and leaves the causal tail's state for the first
generated chunk, whose pre-transformer window reaches back into the reference.

The reference has no streaming decode, so the arithmetic is pinned against the definition restated here from the oracle's own
two halves (OracleModel._codec_front / _codec_tail, the functions codec_decode_streamed is made of)."""
import ctypes as C
import dataclasses
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SPF = 1920
C_, W_, L_ = 4, 16, 2


# ---------------------------------------------------------------------------------------------------
# CPU: the ABI
# ---------------------------------------------------------------------------------------------------
def test_the_prefixed_decode_is_exported():
    from qwen3tts import _lib
    L = C.CDLL(_lib.LIB_PATH)
    assert hasattr(L, "q3tts_codec_decode_streamed_prefixed") and hasattr(L, "q3tts_debug_prefix_states")
    assert _lib.lib().q3tts_codec_decode_streamed_prefixed.argtypes is not None  # the prototype resolves against the library


def test_sampling_mirror_has_the_headers_layout_and_the_flag_defaults_to_zero(tmp_path):
    """q3tts_sampling with audio_stream_reference as its LAST field against the ctypes mirror, as a C compiler lays the header
    out; the ABI version and the request's size have not moved; q3tts_default_sampling leaves the flag at 0."""
    from qwen3tts import _lib as L
    fields = [f for f, _ in L.Sampling._fields_]
    assert fields[-1] == "audio_stream_reference" and fields[-2] == "per_request"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "q3tts.h"', 'int main(void) {',
             '  printf("%zu %zu %d\\n", sizeof(q3tts_sampling), sizeof(q3tts_request), Q3TTS_ABI_VERSION);']
    lines += ['  printf("%%zu\\n", offsetof(q3tts_sampling, %s));' % f for f in fields]
    lines += ['  return 0;', '}']
    src = tmp_path / "sampling.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "sampling"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert out[0] == C.sizeof(L.Sampling) and out[1] == C.sizeof(L.Request) == 88 and out[2] == 4
    assert out[3:] == [getattr(L.Sampling, f).offset for f in fields]
    s = L.Sampling()
    s.audio_stream_reference = 7
    L.lib().q3tts_default_sampling(C.byref(s))
    assert s.audio_stream_reference == 0


# ---------------------------------------------------------------------------------------------------
# GPU: the arithmetic of a prefixed row, codec alone
# ---------------------------------------------------------------------------------------------------
def oracle_prefixed(om, S, R, n, chunk, window, look, f16=False):
    """The definition: S [R + n][16] = ref ++ gen -> the n * 1920 samples of the generated frames."""
    S = np.asarray(S, np.int64)[:R + n]
    lat = []
    for j in range((R + chunk - 1) // chunk):       # prefix chunks: nothing beyond the reference is seen
        f0, f1 = j * chunk, min(R, (j + 1) * chunk)
        w0, w1 = max(0, f0 - window), min(R, (j + 1) * chunk + look)
        lat.append(om._codec_front(S[w0:w1])[f0 - w0:f1 - w0])
    for k in range((n + chunk - 1) // chunk):       # generated chunks: the window reaches back into the reference
        f0, f1 = R + k * chunk, min(R + n, R + (k + 1) * chunk)
        w0, w1 = max(0, f0 - window), min(R + n, R + (k + 1) * chunk + look)
        lat.append(om._codec_front(S[w0:w1])[f0 - w0:f1 - w0])
    tail = om._codec_tail16 if f16 else om._codec_tail
    return tail(np.ascontiguousarray(np.concatenate(lat, 0)))[R * SPF:]


# (reference frames, generated frames) per row: R mod C in {0, 1, C - 1, none}; 1 is below the tail's history of 3 frames. The
# generated lengths end in a chunk of 1, of 3 and of 2, and 5 < C + L is final before its first chunk has its lookahead.
ROWS = [(4, 9), (13, 11), (7, 14), (0, 5)]
FMAX = 24


def _full_codec_dir(tmp_path_factory, name):
    """The decoder at the real layer widths (the recipe of tests/test_streaming.py's full_codec_model)."""
    import json
    import os
    from qwen3tts import synth
    d = str(tmp_path_factory.mktemp(name))
    p = synth.preset("tiny-a")
    p["speech_tokenizer"]["decoder_config"] = synth._codec_cfg(False)
    p["config"]["talker_config"]["code_predictor_config"]["vocab_size"] = 2048
    os.makedirs(os.path.join(d, "speech_tokenizer"), exist_ok=True)
    g = synth._Gen(1234, False)
    json.dump(p["config"], open(os.path.join(d, "config.json"), "w"))
    json.dump(p["speech_tokenizer"], open(os.path.join(d, "speech_tokenizer", "config.json"), "w"))
    synth.save_safetensors(os.path.join(d, "model.safetensors"), synth.talker_tensors(p["config"], g))
    synth.save_safetensors(os.path.join(d, "speech_tokenizer", "model.safetensors"),
                           synth.codec_tensors(p["speech_tokenizer"]["decoder_config"], g, out_wstd=synth.FULL_WIDTH_OUT_WSTD))
    return d


@pytest.fixture(scope="module")
def codec_cases(tmp_path_factory):
    """which -> (model, checkpoint directory, codes [4][FMAX][16]): the tiny decoder, the real layer widths, a float16 tokenizer."""
    from qwen3tts import Qwen3TTSModel, synth
    dirs = {"tiny": str(tmp_path_factory.mktemp("clone_stream") / "tiny-base"), "full": _full_codec_dir(tmp_path_factory, "clone_stream_full"),
            "f16": str(tmp_path_factory.mktemp("clone_stream_h"))}
    synth.write_checkpoint(dirs["tiny"], "tiny-base", seed=4321)
    synth.write_checkpoint(dirs["f16"], "tiny-h", seed=1234)
    out = {}
    for which, d in dirs.items():
        m = Qwen3TTSModel.from_pretrained(d, max_batch=4, max_frames=64, max_prompt=160 if which == "tiny" else 64)
        hi = min(m.info.cp_vocab_size, 2048)
        codes = np.zeros((len(ROWS), FMAX, 16), np.int32)
        rng = np.random.default_rng(29)
        for b, (R, n) in enumerate(ROWS):
            codes[b, :R + n] = rng.integers(1, hi, size=(R + n, 16))
        out[which] = (m, d, codes)
    yield out
    for m, _, _ in out.values():
        m.close()


_GOT = {}


def _prefixed(codec_cases, which):
    """The four rows in one call: computed once per model, left unchanged."""
    if which not in _GOT:
        m, _, codes = codec_cases[which]
        _GOT[which] = m.codec_decode_streamed_prefixed(codes, [r for r, _ in ROWS], [n for _, n in ROWS], C_, W_, L_)
    return _GOT[which]


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["tiny", "full"])
def test_prefixed_stream_is_the_definition(codec_cases, which):
    """PCM within 1e-4 absolute of the definition on every sample of every row (the bar of the streamed decode,
    tests/test_streaming.py), and the row without a prefix IS q3tts_codec_decode_streamed of its codes."""
    from oracle import oracle as O
    m, d, codes = codec_cases[which]
    om = O.OracleModel(d)
    got = _prefixed(codec_cases, which)
    assert got.shape == (len(ROWS), max(n for _, n in ROWS) * SPF)
    for b, (R, n) in enumerate(ROWS):
        want = oracle_prefixed(om, codes[b], R, n, C_, W_, L_)
        assert want.shape == (n * SPF,)
        err = np.abs(got[b, :n * SPF] - want)
        print("%s row %d (R %d, n %d): max error %.3e, signal max %.3f" % (which, b, R, n, err.max(), np.abs(want).max()))
        assert np.abs(want).max() > 1e-3
        assert err.max() <= 1e-4, (which, b, float(err.max()))
    b0 = next(b for b, (R, _) in enumerate(ROWS) if R == 0)
    n0 = ROWS[b0][1]
    assert np.array_equal(got[b0, :n0 * SPF], m.codec_decode_streamed(codes[b0:b0 + 1, :n0], C_, W_, L_)[0])


@pytest.mark.gpu
def test_prefixed_stream_of_a_float16_tokenizer(codec_cases):
    """The float16 MainDecoder (codec_conv_h1 path: float16 tensors carry the history) against the definition with the oracle's
    float16 tail, at the float16 bar of tests/test_codec_f16.py: within 1.5x / 1.25x (max / r.m.s.) of the oracle's own
    float16-to-fp32 distance, capped at 2e-2 / 4e-3."""
    from oracle import oracle as O
    m, d, codes = codec_cases["f16"]
    om = O.OracleModel(d)
    assert om.codec_f16
    got = _prefixed(codec_cases, "f16")
    for b, (R, n) in enumerate(ROWS):
        if R % C_ != 1:  # (the oracle's float16 and fp32 readings take seconds per row: the row whose prefix ends in ONE frame,
            continue     # below the tail's history, where the float16 tensors' margins are rolled onto themselves)
        want = oracle_prefixed(om, codes[b], R, n, C_, W_, L_, f16=True)
        ref32 = oracle_prefixed(om, codes[b], R, n, C_, W_, L_)
        err, floor = np.abs(got[b, :n * SPF] - want), np.abs(want - ref32)
        print("row %d: engine vs float16 oracle max %.2e rms %.2e | float16 vs fp32 oracle max %.2e rms %.2e"
              % (b, err.max(), np.sqrt((err ** 2).mean()), floor.max(), np.sqrt((floor ** 2).mean())))
        assert err.max() <= 1.5 * floor.max() + 1e-3 and np.sqrt((err ** 2).mean()) <= 1.25 * np.sqrt((floor ** 2).mean()) + 1e-4
        assert err.max() <= 2e-2 and np.sqrt((err ** 2).mean()) <= 4e-3


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["tiny", "full", "f16"])
def test_prefixed_rows_do_not_depend_on_their_neighbours(codec_cases, which):
    """Each row alone, and two rows at other phases of their prefixes side by side, give the row's samples of the call over
    all four, bit for bit: whichever rows share a pass -- a prefix chunk beside a generated one, a short chunk beside a full
    one -- a row's margins are rolled by its own take alone."""
    m, _, codes = codec_cases[which]
    got = _prefixed(codec_cases, which)
    for b, (R, n) in enumerate(ROWS):
        alone = m.codec_decode_streamed_prefixed(codes[b:b + 1], [R], [n], C_, W_, L_)
        assert np.array_equal(alone[0], got[b, :n * SPF]), (which, b)
    for pair in ((1, 3), (2, 0), (3, 2)):
        sub = m.codec_decode_streamed_prefixed(codes[list(pair)], [ROWS[b][0] for b in pair], [ROWS[b][1] for b in pair], C_, W_, L_)
        for i, b in enumerate(pair):
            n = ROWS[b][1]
            assert np.array_equal(sub[i, :n * SPF], got[b, :n * SPF]), (which, pair, b)


@pytest.mark.gpu
def test_prefixed_decode_refuses_rows_beyond_their_buffer(codec_cases):
    m, _, codes = codec_cases["tiny"]
    for R, n in ((FMAX, 1), (-1, 4), (4, -1)):
        with pytest.raises(Exception):
            m.codec_decode_streamed_prefixed(codes[:1], [R], [n], C_, W_, L_)
    with pytest.raises(Exception):
        m.codec_decode_streamed_prefixed(codes[:1], [4], [9], 2, W_, L_)  # a chunk below the tail's history
    R, n = ROWS[0]
    assert np.array_equal(m.codec_decode_streamed_prefixed(codes[:1], [R], [n], C_, W_, L_)[0], _prefixed(codec_cases, "tiny")[0, :n * SPF])


# ---------------------------------------------------------------------------------------------------
# GPU: the engine -- static batches, the queue, the voices' saved tail states
# ---------------------------------------------------------------------------------------------------
LOAD = dict(max_batch=4, max_frames=64, max_prompt=160)
SAMPLED = dict(temperature=0.9, top_k=40, repetition_penalty=1.5, seed=77)
STREAM = dict(audio_chunk_frames=C_, audio_window_frames=W_, audio_lookahead_frames=L_)
CLIPS = [(0, 0.3), (1, 1.0), (2, 0.5)]  # (row of the synthetic clip and reference text, seconds): 4 / 13 / 7 reference frames


def _clip(k):
    from qwen3tts import synth
    row, seconds = CLIPS[k]
    return synth.synthetic_reference_audio(row, seconds)


def _prompt(row, n_text=10):
    from qwen3tts import synth
    return synth.synthetic_prompt(row, n_text=n_text, text_vocab=1000, im_start=1000, im_end=1001)


def _ref_text(k):
    return _prompt(CLIPS[k][0])["ref_text_ids"]


class Engine:
    """A loaded tiny-base model with the three voices made on it."""

    def __init__(self, d, **kw):
        from qwen3tts import Qwen3TTSModel
        self.m = Qwen3TTSModel.from_pretrained(d, **{**LOAD, **kw})
        self.voices = [self.m.create_voice(_clip(k), _ref_text(k)) for k in range(len(CLIPS))]

    def close(self):
        for v in self.voices:
            v.close()
        self.m.close()


@pytest.fixture(scope="module")
def base_dir(tmp_path_factory):
    from qwen3tts import synth
    d = str(tmp_path_factory.mktemp("clone_stream_engine") / "tiny-base")
    synth.write_checkpoint(d, "tiny-base", seed=4321)
    return d


@pytest.fixture(scope="module")
def engines(base_dir):
    out = {g: Engine(base_dir, use_graph=g) for g in (True, False)}
    yield out
    for e in out.values():
        e.close()


def _voice_req(e, k, row, n_text, max_tokens):
    from qwen3tts import GenerationRequest
    p = _prompt(row, n_text)
    return GenerationRequest(p["text_ids"], p["target_token_count"], None, None, "english", max_tokens, voice=e.voices[k])


def _plain_req(row, n_text, max_tokens):
    from qwen3tts import GenerationRequest
    p = _prompt(row, n_text)
    return GenerationRequest(p["text_ids"], p["target_token_count"], None, None, "english", max_tokens, route=1)


def _clip_of(e, r):
    return next(k for k in range(len(CLIPS)) if r.voice is e.voices[k])


def _audio_form(e, r):
    """The request with its voice's clip and text as ref_audio / ref_text_ids (a request without a voice: itself)."""
    if r.voice is None:
        return r
    k = _clip_of(e, r)
    return dataclasses.replace(r, voice=None, ref_audio=_clip(k), ref_text_ids=_ref_text(k))


def _same(got, want):
    assert got.status == want.status
    assert got.codes.shape == want.codes.shape and np.array_equal(got.codes, want.codes)
    assert got.audio.shape == want.audio.shape and np.array_equal(got.audio, want.audio)


class Events:
    def __init__(self):
        self.log = []  # (request, kind, payload)

    def __call__(self, i, kind, payload):
        self.log.append((i, kind, payload))

    def check(self, got, streamed=True):
        """Per request: TOKEN* and AUDIO_CHUNK* interleaved, then INFO, then AUDIO; the chunks are consecutive pieces of
        C_ frames at offsets k * C_ * 1920 and concatenate to AUDIO."""
        for i, g in enumerate(got):
            mine = [(k, p) for (j, k, p) in self.log if j == i]
            kinds = [k for k, _ in mine]
            if g.status != 0:
                assert g.status == 2 and kinds == []
                continue
            assert kinds[-2:] == ["info", "audio"] and set(kinds[:-2]) <= {"token", "audio_chunk"}, (i, kinds)
            assert kinds.count("token") == g.codes.shape[0]
            chunks = [p for k, p in mine if k == "audio_chunk"]
            if streamed:
                assert [o for o, _ in chunks] == [k * C_ * SPF for k in range(len(chunks))], i
                assert len(chunks) == -(-g.codes.shape[0] // C_)
                assert np.array_equal(np.concatenate([c for _, c in chunks]), g.audio), i
                assert g.audio.size == g.codes.shape[0] * SPF  # every generated frame, nothing trimmed

    def first_chunk_before_last_token(self, i):
        kinds = [k for (j, k, _) in self.log if j == i]
        return kinds.index("audio_chunk") < len(kinds) - 1 - kinds[::-1].index("token")


@pytest.mark.gpu
def test_the_clips_give_every_prefix_residue(engines):
    """The three clips give reference lengths that are a multiple of the chunk, one frame more (below the tail's history of 3
    frames: the roll of a short chunk overlaps itself) and one frame less."""
    e = engines[True]
    R = [v.info.ref_frames for v in e.voices]
    assert R == [e.m._lib.q3tts_codec_encoded_frames(e.m._h, _clip(k).size) for k in range(3)]
    assert sorted(r % C_ for r in R) == [0, 1, C_ - 1], R


@pytest.mark.gpu
@pytest.mark.parametrize("force", [9, 14, 0])
def test_static_batch_streams_its_clone_rows(engines, force):
    """Two voices, a ref_audio row and a plain row in one q3tts_generate_voices call with the flag: 9 forced frames end in a
    chunk of 1, 14 in a chunk of 2; without forced lengths the rows are ragged, capped by max_tokens, the ref_audio row at
    5 < C + L frames (final before its first chunk has its lookahead)."""
    e = engines[True]
    m = e.m
    caps = [64, 64, 64, 64] if force else [18, 11, 5, 13]
    batch = [_voice_req(e, 0, row=0, n_text=8, max_tokens=caps[0]), _voice_req(e, 1, row=1, n_text=11, max_tokens=caps[1]),
             _audio_form(e, _voice_req(e, 2, row=2, n_text=6, max_tokens=caps[2])), _plain_req(row=3, n_text=9, max_tokens=caps[3])]
    clips = [0, 1, 2, None]
    kw = dict(SAMPLED, force_frames=force)
    want = m.generate_batch(batch, **kw)  # unstreamed
    ev = Events()
    got = m.generate_batch(batch, on_event=ev, audio_stream_reference=1, **STREAM, **kw)
    assert m.last_timing().first_audio_ms > 0
    if force:
        assert [g.codes.shape[0] for g in got] == [force] * 4
    else:
        assert all(0 < g.codes.shape[0] <= c for g, c in zip(got, caps)) and len({g.codes.shape[0] for g in got}) > 1
    ev.check(got)
    for i, k in enumerate(clips):
        assert got[i].status == 0 and np.array_equal(got[i].codes, want[i].codes)
        n = got[i].codes.shape[0]
        if k is None:  # the plain row: what it is streamed to without the flag, alone
            alone = m.generate_batch([batch[i]], row_base=i, **STREAM, **kw)[0]
            _same(got[i], alone)
            assert np.array_equal(got[i].audio, m.codec_decode_streamed(got[i].codes[None], C_, W_, L_)[0][:n * SPF])
            continue
        ref = m.codec_encode(_clip(k)).T  # [R][16]
        R = ref.shape[0]
        S = np.concatenate([ref, got[i].codes], 0).astype(np.int32)
        assert np.array_equal(got[i].audio, m.codec_decode_streamed_prefixed(S[None], [R], [n], C_, W_, L_)[0]), i
        if n == 14:
            assert ev.first_chunk_before_last_token(i), i
    # without the flag: today's result -- a batch with a clone row is decoded one-shot, whatever the window says
    ev0 = Events()
    old = m.generate_batch(batch, on_event=ev0, **STREAM, **kw)
    for a, b in zip(old, want):
        _same(a, b)
    ev0.check(old, streamed=False)


def _queue_reqs(e):
    """Eight requests for three slots: voices of all three clips (a slot's next occupant has another voice, or none), plain
    requests in between, lengths 1 .. 20 so that rows retire at different boundaries."""
    return [_voice_req(e, 0, row=0, n_text=8, max_tokens=20), _voice_req(e, 1, row=1, n_text=11, max_tokens=5),
            _plain_req(row=2, n_text=6, max_tokens=12), _voice_req(e, 2, row=3, n_text=5, max_tokens=17),
            _voice_req(e, 1, row=4, n_text=9, max_tokens=9), _plain_req(row=5, n_text=10, max_tokens=14),
            _voice_req(e, 0, row=6, n_text=7, max_tokens=1), _voice_req(e, 2, row=7, n_text=7, max_tokens=11)]


def _alone(e, r, i):
    return e.m.generate_batch([_audio_form(e, r)], row_base=i, audio_stream_reference=1, **STREAM, **SAMPLED)[0]


@pytest.fixture(scope="module")
def queue_want(engines):
    """The yardstick of the queue tests, computed once: every request's ref_audio form, streamed alone at its index."""
    e = engines[True]
    return [_alone(e, r, i) for i, r in enumerate(_queue_reqs(e))]


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [True, False])
def test_streamed_queue_equals_each_request_alone(engines, queue_want, graph):
    e = engines[graph]
    reqs = _queue_reqs(e)
    ev = Events()
    got = e.m.generate_queued(reqs, slots=3, on_event=ev, audio_stream_reference=1, **STREAM, **SAMPLED)
    want = queue_want if graph else [_alone(e, r, i) for i, r in enumerate(reqs)]
    for i in range(len(reqs)):
        _same(got[i], want[i])
    assert sum(1 for g in got if g.status == 0) >= 6
    ev.check(got)
    assert e.m.last_timing().first_audio_ms > 0


@pytest.mark.gpu
def test_streamed_queue_on_two_lanes(base_dir, queue_want):
    two = Engine(base_dir, n_streams=2)
    try:
        ev = Events()
        got = two.m.generate_queued(_queue_reqs(two), slots=3, on_event=ev, audio_stream_reference=1, **STREAM, **SAMPLED)
        for i in range(len(got)):
            _same(got[i], queue_want[i])
        ev.check(got)
    finally:
        two.close()


@pytest.mark.gpu
def test_a_saved_prefix_state_changes_nothing(engines, monkeypatch):
    """The same voice request three times in one queued call (the second and third admission find the state the first one
    saved), the call again (every admission finds it), once more with Q3TTS_NO_PREFIX_CACHE=1 (every admission decodes the
    reference), and with the voice freed and made again: bit-identical throughout, and equal to the request streamed alone.
    q3tts_debug_prefix_states tells which admissions were served from a saved state."""
    from qwen3tts import _lib
    e = engines[True]
    m = e.m
    kw = dict(audio_stream_reference=1, **STREAM, **SAMPLED)
    proto = _voice_req(e, 1, row=2, n_text=9, max_tokens=10)

    def run(voice):  # one slot: an admission comes after its predecessor's whole request; then two slots
        r = dataclasses.replace(proto, voice=voice)
        return m.generate_queued([r, r, r], slots=1, **kw) + m.generate_queued([r, r, r], slots=2, **kw)

    with m.create_voice(_clip(1), _ref_text(1)) as voice:  # (a voice no earlier test has streamed)
        n0, _, r0 = m.debug_prefix_states()
        first = run(voice)
        # one state for (voice, C, W, L): of the six admissions the first decoded the reference and saved it, the others found it
        n1, bytes1, r1 = m.debug_prefix_states()
        assert n1 == n0 + 1 and bytes1 > 0 and r1 - r0 == 5
        again = run(voice)
        assert m.debug_prefix_states() == (n1, bytes1, r1 + 6)
        monkeypatch.setenv("Q3TTS_NO_PREFIX_CACHE", "1")
        _lib.reload_debug_env()
        try:
            primed = run(voice)
            assert m.debug_prefix_states() == (n1, bytes1, r1 + 6)  # nothing restored, nothing saved
        finally:
            monkeypatch.delenv("Q3TTS_NO_PREFIX_CACHE")
            _lib.reload_debug_env()
    assert m.debug_prefix_states()[0] == n0  # the state went with its voice
    with m.create_voice(_clip(1), _ref_text(1)) as voice:  # the next one may live at the same address: nothing stale is found
        remade = run(voice)
        assert m.debug_prefix_states()[2] == r1 + 6 + 5
    assert all(g.status == 0 and g.codes.shape[0] > 0 for g in first)
    for i, g in enumerate(first[:3]):
        _same(g, _alone(e, proto, i))
    for a, b in zip(first[:3], first[3:]):
        _same(a, b)
    for other in (again, primed, remade):
        for a, b in zip(first, other):
            _same(a, b)


@pytest.mark.gpu
def test_refusals_come_before_any_gpu_work(engines):
    from qwen3tts import Qwen3TTSError
    e = engines[True]
    m = e.m
    reqs = _queue_reqs(e)[:3]
    kw = dict(audio_stream_reference=1, **STREAM, **SAMPLED)
    want = m.generate_queued(reqs, slots=2, **kw)

    def refused(call, word):
        seen = []
        with pytest.raises(Qwen3TTSError) as x:
            call(lambda i, k, p: seen.append(k))
        assert x.value.status == 3 and word in str(x.value), str(x.value)
        assert seen == []
        for g, w in zip(m.generate_queued(reqs, slots=2, **kw), want):  # the engine is still usable
            _same(g, w)

    refused(lambda cb: m.generate_queued(reqs, slots=2, on_event=cb, audio_stream_reference=1, audio_chunk_frames=C_, audio_window_frames=0,
                                         **SAMPLED), "audio_chunk_frames")
    refused(lambda cb: m.generate_queued(reqs, slots=2, on_event=cb, audio_stream_reference=1, **SAMPLED), "audio_stream_reference")
    # without the flag a streamed queue still refuses voices, in the words it has always used
    refused(lambda cb: m.generate_queued(reqs, slots=2, on_event=cb, **STREAM, **SAMPLED), "streamed audio")
    # q3tts_generate_queued (no voices) refuses ref_audio rows, with or without the flag
    plain = [r for r in reqs if r.voice is None] + [_audio_form(e, reqs[0])]
    refused(lambda cb: m.generate_queued(plain, slots=2, on_event=cb, **kw), "voice-clone")
    refused(lambda cb: m.generate_queued(plain, slots=2, on_event=cb, **SAMPLED), "voice-clone")
