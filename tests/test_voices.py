"""Reusable voice prompts (q3tts_voice): a reference clip and its transcript encoded once, then named by requests of
q3tts_generate_voices and q3tts_generate_queued_voices. A request that names a voice must come out bit-identical -- status,
codes, audio, generation count -- to q3tts_generate of the same request alone with the voice's clip and text as ref_audio /
ref_text_ids and row_base = its index, whatever batch, slot, lane, admission burst or decode batch serves it; a call whose
clone rows are all voices runs no front end; bad calls are refused before any GPU work and leave the engine usable."""
import ctypes as C
import dataclasses
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("q3tts_voice_create", "q3tts_voice_free", "q3tts_voice_get_info", "q3tts_generate_voices", "q3tts_generate_queued_voices")


# ---------------------------------------------------------------------------------------------------
# CPU: the ABI
# ---------------------------------------------------------------------------------------------------
def test_voice_symbols_are_exported_and_the_request_keeps_its_size():
    from qwen3tts import _lib
    L = C.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(L, name), name
    assert C.sizeof(_lib.Request) == 88
    _lib.lib()  # the prototypes of the five resolve against the library


def test_voice_info_mirror_has_the_headers_layout(tmp_path):
    """q3tts_voice_info against its ctypes mirror as a C compiler lays the header out; the ABI version has not moved."""
    from qwen3tts import _lib as L
    fields = [f for f, _ in L.VoiceInfo._fields_]
    assert fields == ["ref_frames", "ref_text_tokens", "n_ref_samples", "device_bytes"]
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "q3tts.h"', 'int main(void) {',
             '  printf("%zu %zu %d\\n", sizeof(q3tts_voice_info), sizeof(q3tts_request), Q3TTS_ABI_VERSION);']
    lines += ['  printf("%%zu\\n", offsetof(q3tts_voice_info, %s));' % f for f in fields]
    lines += ['  return 0;', '}']
    src = tmp_path / "voice.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "voice"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert out[0] == C.sizeof(L.VoiceInfo) and out[1] == 88 and out[2] == 4
    assert out[3:] == [getattr(L.VoiceInfo, f).offset for f in fields]


def test_generation_request_takes_a_voice_and_marshals_none_by_default():
    from qwen3tts import GenerationRequest, Qwen3TTSModel
    r = GenerationRequest([1, 2, 3], 1)
    assert r.voice is None and Qwen3TTSModel._voices([r, r]) is None


# ---------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------
LOAD = dict(max_batch=4, max_frames=64, max_prompt=160)
GREEDY = dict(temperature=0.0, repetition_penalty=1.0)
SAMPLED = dict(temperature=0.9, top_k=40, repetition_penalty=1.5, seed=77)
CLIPS = [(0, 0.5), (1, 1.0), (2, 0.3)]  # (row of the synthetic clip and reference text, seconds): three lengths, three texts


@pytest.fixture(scope="module")
def base_dir(tmp_path_factory):
    from qwen3tts import synth
    d = str(tmp_path_factory.mktemp("voices") / "tiny-base")
    synth.write_checkpoint(d, "tiny-base", seed=4321)
    return d


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
    """A loaded model with the three voices made on it."""

    def __init__(self, base_dir, **kw):
        from qwen3tts import Qwen3TTSModel
        self.m = Qwen3TTSModel.from_pretrained(base_dir, **{**LOAD, **kw})
        self.voices = [self.m.create_voice(_clip(k), _ref_text(k)) for k in range(len(CLIPS))]

    def close(self):
        for v in self.voices:
            v.close()
        self.m.close()


@pytest.fixture(scope="module")
def engines(base_dir):
    out = {g: Engine(base_dir, use_graph=g) for g in (True, False)}
    yield out
    for e in out.values():
        e.close()


def _voice_req(e, k, row, n_text, max_tokens, sampling=None):
    from qwen3tts import GenerationRequest
    p = _prompt(row, n_text)
    return GenerationRequest(p["text_ids"], p["target_token_count"], None, None, "english", max_tokens, voice=e.voices[k], sampling=sampling)


def _plain_req(row, n_text, max_tokens, sampling=None):
    """An ordinary request the Base checkpoint admits: the voice-design prompt builder called directly (route 1)."""
    from qwen3tts import GenerationRequest
    p = _prompt(row, n_text)
    return GenerationRequest(p["text_ids"], p["target_token_count"], None, None, "english", max_tokens, route=1, sampling=sampling)


def _audio_form(r):
    """The request with its voice's clip and text as ref_audio / ref_text_ids (a request without a voice: itself)."""
    if r.voice is None:
        return r
    k = next(k for k in range(len(CLIPS)) if r.voice.info.n_ref_samples == _clip(k).size)
    return dataclasses.replace(r, voice=None, ref_audio=_clip(k), ref_text_ids=_ref_text(k))


def _alone(m, r, i, kw):
    """q3tts_generate of the ref_audio form alone at row_base = i: the yardstick of every equality below."""
    a = dataclasses.replace(_audio_form(r), sampling=None)
    s = r.sampling
    over = {f.name: getattr(s, f.name) for f in dataclasses.fields(s) if getattr(s, f.name) is not None} if s is not None else {}
    return m.generate_batch([a], row_base=i, **{**kw, **over})[0]


def _same(got, want):
    assert got.status == want.status
    assert got.codes.shape == want.codes.shape and np.array_equal(got.codes, want.codes)
    assert got.audio.shape == want.audio.shape and np.array_equal(got.audio, want.audio)
    assert got.info.generation_token_count == want.info.generation_token_count


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [GREEDY, SAMPLED], ids=["greedy", "sampled"])
def test_static_batch_equals_each_request_alone(engines, kw):
    """Voice A, voice B, a ref_audio row with A's clip and an ordinary row in one batch; then the smallest generated part
    behind a reference prefix (max_tokens = 1)."""
    e = engines[True]
    m = e.m
    batch = [_voice_req(e, 0, row=0, n_text=8, max_tokens=12), _voice_req(e, 1, row=1, n_text=11, max_tokens=9),
             _audio_form(_voice_req(e, 0, row=2, n_text=6, max_tokens=7)), _plain_req(row=3, n_text=9, max_tokens=10)]
    got = m.generate_batch(batch, **kw)
    assert m.last_timing().frontend_ms > 0  # (one row carried a waveform)
    for i, r in enumerate(batch):
        _same(got[i], _alone(m, r, i, kw))
    assert any(g.status == 0 and g.codes.shape[0] > 0 for g in got[:2])
    one = _voice_req(e, 1, row=4, n_text=7, max_tokens=1)
    g = m.generate_batch([one], **kw)[0]
    _same(g, _alone(m, one, 0, kw))
    assert g.codes.shape[0] <= 1


@pytest.mark.gpu
@pytest.mark.parametrize("misalign", [0, 1], ids=["16-byte", "4-byte"])
def test_decode_code_builder_matches_a_host_copy(engines, misalign):
    """build_decode_codes_rows against the per-row definition out[f] = f < Tref ? ref[:, f] : gen[f - Tref], restated in numpy:
    rows with and without a reference, Tref and F odd, a row of more than one block (4 * (Tref + F) > 256), F == 0 (writes
    nothing, reference or not), F == 1, a row that fills Fdec exactly; frames nobody wrote keep the caller's pattern. Both
    instantiations: 16-byte accesses, and 4-byte ones for buffers 4 bytes off a 16-byte boundary."""
    m = engines[True].m
    rng = np.random.default_rng(5)
    ref_T = np.array([13, 0, 38, 7, 0, 70, 5], np.int32)
    n_frames = np.array([9, 11, 1, 0, 0, 30, 59], np.int32)
    R, gen_stride, Fdec = len(ref_T), 64, 100
    assert int((ref_T + n_frames).max()) == Fdec and 4 * Fdec > 256
    refs = [rng.integers(0, 2048, size=(16, int(t)), dtype=np.int32) for t in ref_T]
    gen = rng.integers(0, 2048, size=(R, gen_stride, 16), dtype=np.int32)
    want = np.full((R, Fdec, 16), -7, np.int32)
    for r in range(R):
        if n_frames[r] == 0:
            continue
        want[r, :ref_T[r]] = refs[r].T
        want[r, ref_T[r]:ref_T[r] + n_frames[r]] = gen[r, :n_frames[r]]
    flat = np.ascontiguousarray(np.concatenate([x.reshape(-1) for x in refs]))
    out = np.full((R, Fdec, 16), -7, np.int32)
    from qwen3tts import _lib as L
    p = lambda a: a.ctypes.data_as(L.i32p)
    m._check(m._lib.q3tts_debug_build_decode_codes(m._h, p(flat), p(ref_T), p(gen), p(n_frames), R, gen_stride, Fdec, misalign, p(out)))
    assert np.array_equal(out, want)
    # a row beyond the buffer is refused by the launcher before anything runs
    st = m._lib.q3tts_debug_build_decode_codes(m._h, p(flat), p(ref_T), p(gen), p(n_frames), R, gen_stride, Fdec - 1, misalign, p(out[:, :Fdec - 1].copy()))
    assert st == 7 and b"outside the decoder's code buffer" in m._lib.q3tts_last_error(m._h)


@pytest.mark.gpu
def test_a_voice_skips_the_front_end(engines):
    e = engines[True]
    m = e.m
    for k, v in enumerate(e.voices):
        n = _clip(k).size
        assert v.info.n_ref_samples == n and v.info.ref_text_tokens == len(_ref_text(k))
        assert v.info.ref_frames == m._lib.q3tts_codec_encoded_frames(m._h, n) > 0
        assert v.info.device_bytes == 64 * v.info.ref_frames + 2 * m.info.hidden_size * (1 + v.info.ref_frames)
    reqs = [_voice_req(e, 0, row=0, n_text=8, max_tokens=6), _voice_req(e, 2, row=1, n_text=5, max_tokens=6)]
    m.generate_batch(reqs, **GREEDY)
    assert m.last_timing().frontend_ms == 0
    m.generate_batch([_audio_form(r) for r in reqs], **GREEDY)
    assert m.last_timing().frontend_ms > 0
    with e.m.create_voice(_clip(2), _ref_text(2)) as v:  # context-manager use; a second voice of the same clip equals the first
        r = dataclasses.replace(reqs[1], voice=v)
        _same(m.generate_batch([r], **GREEDY)[0], m.generate_batch(reqs[1:], **GREEDY)[0])
    assert v._h is None


def _queue_reqs(e, rp=None):
    """Seven requests for two slots: three voices (clips of three lengths), max_tokens 5..30, ordinary requests in between, so
    that a slot's second occupant has another voice, or none, than its first."""
    from qwen3tts import RequestSampling
    sv = RequestSampling(repetition_penalty=rp[0]) if rp else None
    sp = RequestSampling(repetition_penalty=rp[1]) if rp else None
    return [_voice_req(e, 0, row=0, n_text=8, max_tokens=30, sampling=sv), _voice_req(e, 1, row=1, n_text=11, max_tokens=5, sampling=sv),
            _plain_req(row=2, n_text=6, max_tokens=12, sampling=sp), _voice_req(e, 2, row=3, n_text=5, max_tokens=17, sampling=sv),
            _voice_req(e, 1, row=4, n_text=9, max_tokens=8, sampling=sv), _plain_req(row=5, n_text=10, max_tokens=23, sampling=sp),
            _voice_req(e, 0, row=6, n_text=7, max_tokens=11, sampling=sv)]


def _check_events(events, got):
    for i, g in enumerate(got):
        kinds = [k for (j, k) in events if j == i]
        if g.status != 0:  # (first token EOS: fails alone, reports nothing)
            assert g.status == 2 and kinds == []
            continue
        assert kinds == ["token"] * g.codes.shape[0] + ["info", "audio"], (i, kinds)


@pytest.fixture(scope="module")
def queue_want(engines):
    """The yardstick of the queue tests, computed once: every request's ref_audio form alone at its index."""
    e = engines[True]
    return [_alone(e.m, r, i, SAMPLED) for i, r in enumerate(_queue_reqs(e))]


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [True, False])
def test_queue_equals_each_request_alone(engines, queue_want, graph):
    e = engines[graph]
    reqs = _queue_reqs(e)
    events = []
    got = e.m.generate_queued(reqs, slots=2, on_event=lambda i, k, p: events.append((i, k)), **SAMPLED)
    assert len(got) == 7 and e.m.last_timing().rows == 7
    want = queue_want if graph else [_alone(e.m, r, i, SAMPLED) for i, r in enumerate(reqs)]
    for i in range(7):
        _same(got[i], want[i])
    assert sum(1 for g in got if g.status == 0) >= 5
    _check_events(events, got)


@pytest.mark.gpu
def test_queue_lanes_and_per_request_penalties_change_nothing(base_dir, engines, queue_want):
    e = engines[True]
    two = Engine(base_dir, n_streams=2)
    try:
        events = []
        got = two.m.generate_queued(_queue_reqs(two), slots=4, on_event=lambda i, k, p: events.append((i, k)), **SAMPLED)
        for i in range(7):
            _same(got[i], queue_want[i])
        _check_events(events, got)
    finally:
        two.close()
    # the reference's defaults side by side: 1.5 on voice rows, 1.05 elsewhere
    reqs = _queue_reqs(e, rp=(1.5, 1.05))
    kw = {**SAMPLED, "repetition_penalty": 1.2}
    got = e.m.generate_queued(reqs, slots=2, **kw)
    for i, r in enumerate(reqs):
        _same(got[i], _alone(e.m, r, i, kw))


@pytest.mark.gpu
def test_refusals_leave_the_engine_usable(base_dir, engines):
    from qwen3tts import Qwen3TTSError, Qwen3TTSModel
    e = engines[True]
    m = e.m
    reqs = _queue_reqs(e)[:3]
    want = m.generate_queued(reqs, slots=2, **SAMPLED)

    def still_fine():
        for g, w in zip(m.generate_queued(reqs, slots=2, **SAMPLED), want):
            _same(g, w)

    def refused(call, word, status=3):
        with pytest.raises(Qwen3TTSError) as x:
            call()
        assert x.value.status == status and word in str(x.value), str(x.value)
        still_fine()

    other = Qwen3TTSModel.from_pretrained(base_dir, max_batch=1, max_frames=16, max_prompt=160)
    try:
        foreign = other.create_voice(_clip(0), _ref_text(0))
        bad = dataclasses.replace(reqs[0], voice=foreign)
        refused(lambda: m.generate_batch([bad], **SAMPLED), "not created on this model")
        refused(lambda: m.generate_queued(reqs + [bad], slots=2, **SAMPLED), "not created on this model")
    finally:
        other.close()
    both = dataclasses.replace(reqs[0], ref_audio=_clip(0), ref_text_ids=_ref_text(0))
    refused(lambda: m.generate_batch([both], **SAMPLED), "names a voice")
    refused(lambda: m.generate_queued([both], slots=2, **SAMPLED), "names a voice")
    text_too = dataclasses.replace(reqs[0], ref_text_ids=_ref_text(0))
    refused(lambda: m.generate_batch([text_too], **SAMPLED), "names a voice")
    refused(lambda: m.generate_queued(reqs, slots=2, audio_chunk_frames=4, audio_window_frames=16, **SAMPLED), "streamed audio")
    refused(lambda: m.generate_queued(reqs + [_audio_form(reqs[0])], slots=2, **SAMPLED), "voice-clone")
    # an ICL prompt longer than max_prompt, at the LAST index: refused by the pre-flight check, before the first TOKEN event
    from qwen3tts import synth
    with m.create_voice(synth.synthetic_reference_audio(5, 14.0), _ref_text(0)) as long_voice:
        assert long_voice.info.ref_frames > LOAD["max_prompt"]
        last = dataclasses.replace(reqs[0], voice=long_voice)
        seen = []
        refused(lambda: m.generate_queued(reqs + [last], slots=2, on_event=lambda i, k, p: seen.append(k), **SAMPLED), "max_prompt")
        assert seen == []
        with pytest.raises(Qwen3TTSError) as x:
            m.generate_queued(reqs + [last], slots=2, **SAMPLED)
        assert "request 3" in str(x.value)
        refused(lambda: m.generate_batch([last], **SAMPLED), "max_prompt")
    # q3tts_voice_create applies a clone request's own checks
    refused(lambda: m.create_voice(np.zeros(0, np.float32), _ref_text(0)), "empty")
    nan = _clip(0).copy()
    nan[100] = np.nan
    refused(lambda: m.create_voice(nan, _ref_text(0)), "non-finite")
    refused(lambda: m.create_voice(_clip(0), _ref_text(0)[:4]), "ref_text_ids")
    refused(lambda: m.create_voice(_clip(0), _ref_text(0)[:-1] + [10 ** 6]), "out of range")


@pytest.mark.gpu
def test_voice_create_needs_the_encoder(ckpt_dirs):
    from qwen3tts import Qwen3TTSError, Qwen3TTSModel
    m = Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-a"], max_batch=1, max_frames=16, max_prompt=64)
    try:
        with pytest.raises(Qwen3TTSError) as x:
            m.create_voice(_clip(0), _ref_text(0))
        assert x.value.status == 1 and "speech tokenizer encoder" in str(x.value)
    finally:
        m.close()


@pytest.mark.gpu
def test_a_voice_request_whose_first_token_is_eos_fails_alone(tmp_path, engines):
    """The recipe of test_queued.py on the Base checkpoint: the victim's first token becomes the EOS id of a second copy of the
    checkpoint. Its row then has F == 0 behind a reference prefix -- a decode descriptor that writes nothing, a slot that is
    retired at the first burst boundary and refilled -- beside healthy voice rows, in the queue and in a static batch. The victim
    fails alone with GENERATION_FAILED and reports nothing; every healthy row is delivered, starts with the token it starts with
    on the unmodified checkpoint, and equals the same voice request run alone at its index: the victim beside it changes nothing.
    (That a voice request equals its ref_audio form is the business of the tests above.)"""
    from qwen3tts import synth
    e = engines[True]
    kw = dict(temperature=0.9, top_k=50, seed=2)

    def four(eng):
        return [_voice_req(eng, i % 3, row=i, n_text=6 + i, max_tokens=12) for i in range(4)]

    first = [int(r.codes[0, 0]) if r.codes.shape[0] else -1 for r in e.m.generate_queued(four(e), slots=2, **kw)]
    victim = next(i for i in range(4) if first[i] >= 0 and any(f >= 0 and f != first[i] for f in first))
    others = [i for i in range(4) if first[i] >= 0 and first[i] != first[victim]]
    d = str(tmp_path / "eos_first")
    synth.write_checkpoint(d, "tiny-base", seed=4321)
    cfg_path = os.path.join(d, "config.json")
    cfg = json.load(open(cfg_path))
    cfg["talker_config"]["codec_eos_token_id"] = first[victim]
    json.dump(cfg, open(cfg_path, "w"))
    x = Engine(d)
    try:
        reqs = four(x)
        kinds = {i: [] for i in range(4)}
        runs = [x.m.generate_queued(reqs, slots=2, on_event=lambda i, k, p: kinds[i].append(k), **kw), x.m.generate_batch(reqs, **kw)]
        assert kinds[victim] == []
        for res in runs:
            assert res[victim].status == 2 and res[victim].audio.size == 0 and res[victim].codes.shape == (0, 16)
            for i in others:
                assert res[i].status == 0 and res[i].codes.shape[0] >= 1 and int(res[i].codes[0, 0]) == first[i]
                _same(res[i], x.m.generate_batch([reqs[i]], row_base=i, **kw)[0])
        for i in others:
            assert kinds[i][-2:] == ["info", "audio"]
        assert b"Generation failed: No tokens generated" in x.m._lib.q3tts_last_error(x.m._h)
    finally:
        x.close()
