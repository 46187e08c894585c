"""Streamed audio in a continuous-batching queue (q3tts_generate_queued with audio_chunk_frames > 0 and audio_window_frames > 0):
every request's audio leaves in chunks while it generates, and request i comes out bit-identical to that request streamed
alone (generate_batch([r], row_base=i, <same streaming keywords>)) -- which is codec_decode_streamed of its codes -- whatever
slot, lane, admission burst or neighbours in a decoder pass it had. All comparisons are bit-exact."""
import json
import os

import numpy as np
import pytest

from conftest import tiny_request

pytestmark = pytest.mark.gpu

C_, W_, L_ = 8, 16, 2
STREAM = dict(audio_chunk_frames=C_, audio_window_frames=W_, audio_lookahead_frames=L_)
SPF = 1920
SAMPLINGS = [dict(temperature=0.0, repetition_penalty=1.0), dict(temperature=0.9, top_k=40, repetition_penalty=1.05, seed=77)]


def _req(row, n_text, max_tokens, speaker="aiden", language="english", n_instruct=0):
    from qwen3tts import GenerationRequest
    r = tiny_request(row=row, n_text=n_text, n_instruct=n_instruct, speaker=speaker, language=language)
    return GenerationRequest(r["text_ids"], r["target_token_count"], r["instruct_ids"], r["speaker"], r["language"], max_tokens)


def _mixed():
    """10 requests: prompt lengths, speakers, languages, instruct and max_tokens (5..40) all vary (as tests/test_queued.py)."""
    spk = ["aiden", "vivian", "eric"]
    lang = ["english", "auto", "chinese", "english", "auto"]
    mt = [23, 5, 40, 11, 7, 33, 17, 6, 28, 14]
    return [_req(row=i, n_text=5 + (3 * i) % 11, max_tokens=mt[i], speaker=spk[i % 3], language=lang[i % 5],
                 n_instruct=(4 if i % 4 == 2 else 0)) for i in range(10)]


def _same(got, want):
    assert got.status == want.status
    assert got.codes.shape == want.codes.shape and np.array_equal(got.codes, want.codes)
    assert got.audio.shape == want.audio.shape and np.array_equal(got.audio, want.audio)
    assert got.info.generation_token_count == want.info.generation_token_count


def _load(d, **kw):
    from qwen3tts import Qwen3TTSModel
    return Qwen3TTSModel.from_pretrained(d, max_batch=4, max_frames=64, max_prompt=96, **kw)


@pytest.fixture(scope="module")
def models(ckpt_dirs):
    out = {g: _load(ckpt_dirs["tiny-b"], use_graph=g) for g in (True, False)}
    yield out
    for m in out.values():
        m.close()


_ALONE = {}


def _alone(m, tag, reqs, kw):
    """Every request streamed alone with row_base = its index: computed once per (model, request set, sampling), shared."""
    key = (id(m), tag, tuple(sorted(kw.items())))
    if key not in _ALONE:
        _ALONE[key] = [m.generate_batch([r], row_base=i, **kw, **STREAM)[0] for i, r in enumerate(reqs)]
    return _ALONE[key]


def _collector():
    ev = []
    return ev, (lambda i, k, p: ev.append((i, k, p)))


def _check_events(events, res, n_reqs):
    """Per request: TOKEN / AUDIO_CHUNK interleaved, then INFO, then AUDIO; offsets k * C * 1920 in order; ceil(F / C) pieces
    that concatenate to AUDIO."""
    for i in range(n_reqs):
        mine = [(k, p) for (j, k, p) in events if j == i]
        F = res[i].codes.shape[0]
        if F == 0:
            assert res[i].status == 2 and mine == []
            continue
        kinds = [k for k, _ in mine]
        assert kinds[-2:] == ["info", "audio"], (i, kinds)
        assert set(kinds[:-2]) <= {"token", "audio_chunk"} and kinds.count("token") == F, (i, kinds)
        pieces = [p for k, p in mine if k == "audio_chunk"]
        assert len(pieces) == -(-F // C_), (i, F, len(pieces))
        assert [o for o, _ in pieces] == [k * C_ * SPF for k in range(len(pieces))], i
        cat = np.concatenate([p for _, p in pieces])
        assert np.array_equal(cat, res[i].audio) and cat.size == F * SPF, i
        assert np.array_equal(mine[-1][1], res[i].audio)


def _different_phases_back_to_back(events):
    """Two requests whose chunks at DIFFERENT chunk indices were delivered back to back (one run of AUDIO_CHUNK events, nothing
    between): rows of one pass, or of passes of one push, sitting at different chunk phases."""
    for (i, k, p), (j, k2, p2) in zip(events, events[1:]):
        if k == k2 == "audio_chunk" and i != j and p[0] != p2[0]:
            return True
    return False


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("kw", SAMPLINGS, ids=["greedy", "sampled"])
def test_streamed_queue_equals_each_request_alone(models, graph, kw):
    m = models[graph]
    reqs = _mixed()
    events, on_event = _collector()
    got = m.generate_queued(reqs, slots=3, on_event=on_event, **kw, **STREAM)
    assert len(got) == len(reqs) and m.last_timing().rows == len(reqs)
    want = _alone(m, "mixed", reqs, kw)
    frames = [g.codes.shape[0] for g in got]
    print("frames", frames, "first_audio_ms %.1f codec_ms %.1f" % (m.last_timing().first_audio_ms, m.last_timing().codec_ms))
    for i in range(len(reqs)):
        _same(got[i], want[i])
        n = frames[i]
        if n:
            assert got[i].audio.size == n * SPF  # all generated frames, no end trim
            assert np.array_equal(got[i].audio, m.codec_decode_streamed(got[i].codes[None], C_, W_, L_)[0][:n * SPF])
    _check_events(events, got, len(reqs))
    # the set covers the corners, read off the results: shorter than one chunk, an exact multiple, two phases side by side
    assert any(0 < f < C_ for f in frames), frames
    assert any(f > 0 and f % C_ == 0 for f in frames), frames
    assert _different_phases_back_to_back(events)
    assert m.last_timing().first_audio_ms > 0


def _long_and_shorts(m):
    reqs = [_req(row=0, n_text=9, max_tokens=60)] + [_req(row=1 + i, n_text=5 + i, max_tokens=6 + i) for i in range(9)]
    # a seed under which the long request really is long (the tiny checkpoint draws EOS now and then)
    seed = next(s for s in range(5, 50) if m.generate_batch(reqs[:1], temperature=0.9, top_k=50, seed=s)[0].codes.shape[0] >= 40)
    return reqs, dict(temperature=0.9, top_k=50, seed=seed)


@pytest.mark.parametrize("slots", [1, 2])
def test_slot_reuse_leaks_nothing(models, slots):
    """One long request beside nine short ones: the shorts pass through the same slot one after another, so a history margin
    or a non-finite flag left by the previous occupant, or a bystander row rolled by somebody else's pass, shows as a request
    that differs from itself alone."""
    m = models[True]
    reqs, kw = _long_and_shorts(m)
    events, on_event = _collector()
    res = m.generate_queued(reqs, slots=slots, on_event=on_event, **kw, **STREAM)
    want = _alone(m, "long", reqs, kw)
    for i in range(len(reqs)):
        _same(res[i], want[i])
    _check_events(events, res, len(reqs))
    if slots == 2:
        order = [(j, k) for (j, k, _) in events]
        last_long_token = max(n for n, (j, k) in enumerate(order) if j == 0 and k == "token")
        first_long_chunk = min(n for n, (j, k) in enumerate(order) if j == 0 and k == "audio_chunk")
        first_short_audio = min(n for n, (j, k) in enumerate(order) if j > 0 and k == "audio")
        assert first_long_chunk < last_long_token      # audio leaves while the request still generates
        assert first_short_audio < last_long_token     # and a short one is done long before the long one ends


def test_lanes_change_nothing(ckpt_dirs, models):
    reqs = _mixed()
    kw = SAMPLINGS[1]
    one = models[True].generate_queued(reqs, slots=4, **kw, **STREAM)
    two = _load(ckpt_dirs["tiny-b"], n_streams=2)
    try:
        events, on_event = _collector()
        got = two.generate_queued(reqs, slots=4, on_event=on_event, **kw, **STREAM)
    finally:
        two.close()
    for a, b in zip(got, one):
        _same(a, b)
    _check_events(events, got, len(reqs))
    for a, b in zip(one, _alone(models[True], "mixed", reqs, kw)):
        _same(a, b)


def test_refusals_leave_the_engine_usable(models):
    from qwen3tts import GenerationRequest, Qwen3TTSError, synth
    m = models[True]
    kw = SAMPLINGS[1]
    reqs = [_req(row=i, n_text=6 + i, max_tokens=8 + 3 * i) for i in range(3)]
    seen = []
    on_event = lambda i, k, p: seen.append(k)  # noqa: E731
    bad = [(dict(slots=2, audio_chunk_frames=8, audio_window_frames=0), "audio_chunk_frames"),  # chunks without a window
           (dict(slots=2, audio_chunk_frames=2, audio_window_frames=16), "audio_chunk_frames"),  # below the tail's history (3)
           (dict(slots=5, **STREAM), "slots"), (dict(slots=0, **STREAM), "slots")]
    for extra, word in bad:
        with pytest.raises(Qwen3TTSError) as e:
            m.generate_queued(reqs, on_event=on_event, **{**kw, **extra})
        assert e.value.status == 3 and word in str(e.value), extra
    p = synth.synthetic_prompt(0, n_text=10, text_vocab=1000, im_start=1000, im_end=1001)
    clone = GenerationRequest(p["text_ids"], p["target_token_count"], None, None, "english",
                              ref_audio=synth.synthetic_reference_audio(0, 0.5), ref_text_ids=p["ref_text_ids"])
    with pytest.raises(Qwen3TTSError) as e:
        m.generate_queued(reqs + [clone], slots=2, on_event=on_event, **kw, **STREAM)
    assert e.value.status == 3 and "voice-clone" in str(e.value)
    want = [m.generate_batch([r], row_base=i, **kw)[0] for i, r in enumerate(reqs)]
    job = m.generate_batch_begin(reqs[:1], **kw)
    try:
        with pytest.raises(Qwen3TTSError) as e:
            m.generate_queued(reqs, slots=2, on_event=on_event, **kw, **STREAM)
        assert e.value.status == 3 and "outstanding" in str(e.value)
    finally:
        _same(m.generate_batch_end(job)[0], want[0])
    assert seen == []  # refused before any GPU work: not one event
    for i, g in enumerate(m.generate_queued(reqs, slots=2, **kw)):  # the plain queue still equals each request alone
        _same(g, want[i])
    streamed = _alone(m, "three", reqs, kw)
    for i, g in enumerate(m.generate_queued(reqs, slots=2, **kw, **STREAM)):  # and so does the streamed one
        _same(g, streamed[i])


# ---- the slotted stream alone (q3tts_debug_codec_stream_slots): tiny and real layer widths, fp32 and float16 tokenizers ----
def _full_codec_dir(tmp_path_factory, name):
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
def codec_models(ckpt_dirs, tmp_path_factory):
    from qwen3tts import synth
    h = str(tmp_path_factory.mktemp("tiny_h_slots"))
    synth.write_checkpoint(h, "tiny-h", seed=1234)  # a float16 speech tokenizer (tests/test_codec_f16.py)
    out = {"tiny": _load(ckpt_dirs["tiny-b"]), "full": _load(_full_codec_dir(tmp_path_factory, "full_codec_slots")), "f16": _load(h)}
    yield out
    for m in out.values():
        m.close()


_HOOK_REF = {}


def _hook_case(m, which):
    """Random codes for 7 requests of 1..40 frames and each one's streamed decode alone: computed once per model, left unchanged."""
    if which not in _HOOK_REF:
        rng = np.random.default_rng(11)
        F = [40, 1, 8, 23, 16, 5, 31]  # a full buffer, one frame, one chunk exactly, odd, two chunks exactly, below a chunk, odd
        hi = min(m.info.cp_vocab_size, 2048)
        codes = np.zeros((len(F), 40, 16), np.int32)
        for b, f in enumerate(F):
            codes[b, :f] = rng.integers(1, hi, size=(f, 16))
        want = [m.codec_decode_streamed(codes[b:b + 1, :f], C_, W_, L_)[0] for b, f in enumerate(F)]
        _HOOK_REF[which] = (F, codes, want)
    return _HOOK_REF[which]


@pytest.mark.parametrize("burst", [1, 9, 64])
@pytest.mark.parametrize("slots", [1, 2, 3])
@pytest.mark.parametrize("which", ["tiny", "full", "f16"])
def test_slotted_stream_equals_each_request_streamed_alone(codec_models, which, slots, burst):
    """burst 64: every request is final on arrival, so all of its chunks leave in one push (more passes than the ring has slots)."""
    m = codec_models[which]
    F, codes, want = _hook_case(m, which)
    got = m.debug_codec_stream_slots(codes, F, slots, burst, C_, W_, L_)
    for b, f in enumerate(F):
        assert np.array_equal(got[b, :f * SPF], want[b]), (which, slots, burst, b)
        assert np.abs(want[b]).max() > 0


def test_hook_checks_its_arguments(codec_models):
    from qwen3tts import Qwen3TTSError
    m = codec_models["tiny"]
    F, codes, want = _hook_case(m, "tiny")
    bad = codes.copy()
    bad[3, 2, 5] = 1 << 20  # outside the RVQ tables
    for args in ((bad, F, 2, 9, C_, W_, L_), (codes, F, 5, 9, C_, W_, L_), (codes, F, 2, 9, 2, W_, L_), (codes, [41] + F[1:], 2, 9, C_, W_, L_)):
        with pytest.raises(Qwen3TTSError) as e:
            m.debug_codec_stream_slots(*args)
        assert e.value.status == 3
    assert np.array_equal(m.debug_codec_stream_slots(codes, F, 2, 9, C_, W_, L_)[0, :F[0] * SPF], want[0])


def test_existing_stream_entries_are_unchanged(codec_models):
    """rvq_gather without a per-row first frame and the lock-step stream: with the pre-transformer over everything
    (window < 0) the streamed decode still IS the one-shot decode, and a streamed generate_batch still is codec_decode_streamed."""
    for which in ("tiny", "full"):
        m = codec_models[which]
        F, codes, _ = _hook_case(m, which)
        one_shot, _ = m.codec_decode(codes, n_frames=F)
        got = m.codec_decode_streamed(codes, C_, -1, n_frames=F)
        for b, f in enumerate(F):
            assert np.array_equal(got[b, :f * SPF], one_shot[b, :f * SPF]), (which, b)
    m = codec_models["tiny"]
    reqs = _mixed()[:3]
    for r in m.generate_batch(reqs, **SAMPLINGS[1], **STREAM):
        n = r.codes.shape[0]
        if n:
            assert np.array_equal(r.audio, m.codec_decode_streamed(r.codes[None], C_, W_, L_)[0][:n * SPF])


def test_out_of_range_request_is_held_and_redecoded(tmp_path):
    """A checkpoint whose decoder leaves the fp16 range (tests/test_codec_range.py's recipe: a bias far beyond 65504). Every
    request of a streamed queue then stops its chunks at its first flagged one and is delivered from the fp32 re-decode,
    exactly as the same request streamed alone; nothing non-finite ever leaves, and the pieces still concatenate to AUDIO."""
    from safetensors.numpy import load_file, save_file
    from qwen3tts import Qwen3TTSModel, synth
    d = str(tmp_path / "m")
    synth.write_checkpoint(d, "tiny-a", seed=1234)
    f = os.path.join(d, "speech_tokenizer", "model.safetensors")
    t = load_file(f)
    key = [k for k in t if k.endswith("decoder.0.conv.bias") or k.endswith("initConv.conv.bias")]
    assert key
    t[key[0]] = (t[key[0]].astype(np.float32) + np.float32(3.0e5)).astype(t[key[0]].dtype)
    save_file(t, f)
    reqs = [_req(row=i, n_text=6 + i, max_tokens=[20, 6, 13, 9][i]) for i in range(4)]
    kw = dict(temperature=0.9, top_k=50, seed=3)
    m = Qwen3TTSModel.from_pretrained(d, max_batch=2, max_frames=32, max_prompt=64)
    try:
        want = [m.generate_batch([r], row_base=i, **kw, **STREAM)[0] for i, r in enumerate(reqs)]
        events, on_event = _collector()
        got = m.generate_queued(reqs, slots=2, on_event=on_event, **kw, **STREAM)
        for i in range(len(reqs)):
            _same(got[i], want[i])
            assert got[i].status != 0 or np.isfinite(got[i].audio).all()
        assert any(g.status == 0 and g.codes.shape[0] > 0 for g in got)
        _check_events(events, got, len(reqs))
    finally:
        m.close()
