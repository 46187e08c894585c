"""Live voices (q3tts_session_open_ex with live_voices > 0): a session that makes voices, and takes ref_audio requests, while
it runs. The front end of a clip runs on a stream of its own beside the slot loop; a session-made voice must hold the very
bits Qwen3TTSModel.create_voice gives for the clip, so ticket t stays bit-identical to the request generated alone at
row_base = t -- in its ref_audio form, whole and streamed -- whatever ran beside the front end. `want` is computed on the same
handle before the session opens. Every wait carries a timeout, so a defect fails instead of hanging."""
import dataclasses
import threading
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WAIT = 60  # seconds: every wait below
C_, W_, L_ = 8, 32, 4
STREAM = dict(audio_chunk_frames=C_, audio_window_frames=W_, audio_lookahead_frames=L_)  # the geometry of tests/test_session.py
STREAMED = dict(audio_stream_reference=1, **STREAM)
CLIPS = [(0, 0.3), (2, 0.5)]  # (row of the synthetic clip and reference text, seconds): 4 and 7 reference frames
LONGEST = 7
VSAMPLED = dict(temperature=0.9, top_k=40, repetition_penalty=1.5, seed=77)
TEXTS = [(0, 8, 21), (1, 11, 26), (0, 6, 19), (1, 9, 23)]  # (clip, text tokens, max_tokens) of request i


def _clip(k):
    from qwen3tts import synth
    return synth.synthetic_reference_audio(*CLIPS[k])


def _prompt(row, n_text=10):
    from qwen3tts import synth
    return synth.synthetic_prompt(row, n_text=n_text, text_vocab=1000, im_start=1000, im_end=1001)


def _ref_text(k):
    return _prompt(CLIPS[k][0])["ref_text_ids"]


def _audio_req(i, k=None, max_tokens=None):
    """Request i in its ref_audio form (clip k, default TEXTS[i]'s)."""
    from qwen3tts import GenerationRequest
    kk, n_text, mt = TEXTS[i % len(TEXTS)]
    k = kk if k is None else k
    p = _prompt(i, n_text)
    return GenerationRequest(p["text_ids"], p["target_token_count"], None, None, "english", mt if max_tokens is None else max_tokens,
                             ref_audio=_clip(k), ref_text_ids=_ref_text(k))


def _named(r, voice):
    return dataclasses.replace(r, ref_audio=None, ref_text_ids=None, voice=voice)


def _same(got, want):
    assert got.status == want.status
    assert got.codes.shape == want.codes.shape and np.array_equal(got.codes, want.codes)
    assert got.audio.shape == want.audio.shape and np.array_equal(got.audio, want.audio)
    assert got.info.generation_token_count == want.info.generation_token_count


def _info(v):
    return (v.info.ref_frames, v.info.ref_text_tokens, v.info.n_ref_samples, v.info.device_bytes)


def _until(cond):
    """(a voice on its way out gives its place back at the loop's next boundary, not when its last result is handed over)"""
    t0 = time.monotonic()
    while not cond():
        assert time.monotonic() - t0 < WAIT
        time.sleep(0.002)


@pytest.fixture(scope="module")
def live(tmp_path_factory):
    from qwen3tts import Qwen3TTSModel, synth
    d = str(tmp_path_factory.mktemp("session_live_voices") / "tiny-base")
    synth.write_checkpoint(d, "tiny-base", seed=4321)
    m = Qwen3TTSModel.from_pretrained(d, max_batch=4, max_frames=64, max_prompt=160)
    voices = [m.create_voice(_clip(k), _ref_text(k)) for k in range(2)]
    assert [v.info.ref_frames for v in voices] == [4, LONGEST]
    yield m, voices
    for v in voices:
        v.close()
    m.close()


_ALONE = {}


def _alone(m, i, t, k=None, max_tokens=None, **form):
    """Request i (clip k) alone at row_base = t in its ref_audio form: computed once, shared, never changed."""
    key = (id(m), i, t, k, max_tokens, tuple(sorted(form.items())))
    if key not in _ALONE:
        _ALONE[key] = m.generate_batch([_audio_req(i, k, max_tokens)], row_base=t, **form, **VSAMPLED)[0]
    return _ALONE[key]


# ---------------------------------------------------------------------------------------------------
# 1. a voice made while rows run
# ---------------------------------------------------------------------------------------------------
def test_a_voice_made_while_rows_run(live):
    m, voices = live
    want = [_alone(m, 0, 0), _alone(m, 2, 1), _alone(m, 1, 2), _alone(m, 3, 3)]  # tickets 0, 1: clip 0; tickets 2, 3: clip 1
    assert want[0].codes.shape[0] > 0
    state = {"tokens": 0, "voice": None, "tickets": [], "error": None}
    both_in = threading.Event()

    def on_event(i, kind, payload):
        if i != 0 or kind != "token":
            return
        state["tokens"] += 1
        if state["tokens"] != 1:
            return
        try:
            assert both_in.wait(WAIT)
            v = s.create_voice(_clip(1), _ref_text(1))  # the loop thread is here: the voice cannot be ready yet
            state["voice"] = v
            state["tickets"] = [s.submit(_named(_audio_req(1), v)), s.submit(_named(_audio_req(3), v))]
        except Exception as e:  # (an exception must not cross the C callback)
            state["error"] = e

    s = m.open_session(slots=2, max_ref_frames=LONGEST, live_voices=2, on_event=on_event, **VSAMPLED)
    try:
        assert [s.submit(_named(_audio_req(0), voices[0])), s.submit(_named(_audio_req(2), voices[0]))] == [0, 1]
        both_in.set()
        got = [s.result(0, timeout=WAIT)]
        assert state["error"] is None and state["tickets"] == [2, 3], state
        got += [s.result(t, timeout=WAIT) for t in (1, 2, 3)]
        sv = state["voice"]
        sv.wait(timeout=WAIT)
        vs = s.voice_stats()
        assert (vs.created, vs.ready, vs.in_flight, vs.alive, vs.anonymous) == (1, 1, 0, 1, 0)
        assert vs.frontend_ms_sum > 0
        print("frame_steps_beside", vs.frame_steps_beside, "frontend_ms_sum", vs.frontend_ms_sum)  # (whether a burst overlapped is timing)
        s.close()
    finally:
        s.close(drain=False)
    for t in range(4):
        _same(got[t], want[t])
    # behind the session the voice is an ordinary voice of the handle
    assert _info(sv) == _info(voices[1])
    _same(m.generate_batch([_named(_audio_req(1), sv)], row_base=2, **VSAMPLED)[0], want[2])
    sv.close()


# ---------------------------------------------------------------------------------------------------
# 2. ref_audio submits
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("streamed", [False, True], ids=["whole", "streamed"])
def test_ref_audio_submits(live, streamed):
    m, _ = live
    form = STREAMED if streamed else {}
    want = [_alone(m, t, t, **form) for t in range(3)]
    n0 = m.debug_prefix_states()[0]
    s = m.open_session(slots=2, max_ref_frames=LONGEST, live_voices=2, **form, **VSAMPLED)
    try:
        alive0 = s.voice_stats().alive
        assert [s.submit(_audio_req(0)), s.submit(_audio_req(1))] == [0, 1]
        got = [s.result(0, timeout=WAIT)]
        assert s.submit(_audio_req(2)) == 2  # (ticket 0's job has finished: at most one is in flight)
        got += [s.result(t, timeout=WAIT) for t in (1, 2)]
        _until(lambda: s.voice_stats().alive == alive0)
        vs = s.voice_stats()
        assert (vs.anonymous, vs.created, vs.ready, vs.in_flight) == (3, 3, 3, 0)
        s.close()
    finally:
        s.close(drain=False)
    for t in range(3):
        _same(got[t], want[t])
    assert m.debug_prefix_states()[0] == n0  # an anonymous voice saves no prefix state: no other ticket could use it


# ---------------------------------------------------------------------------------------------------
# 3. a clip at another rate
# ---------------------------------------------------------------------------------------------------
def test_a_16_khz_clip(live):
    m, _ = live
    clip = _clip(0)  # (the same samples, taken as 16 kHz: 10800 samples at 24 kHz, 6 frames)
    ov = m.create_voice(clip, _ref_text(0), sample_rate=16000)
    r = _audio_req(0)
    want = m.generate_batch([_named(r, ov)], row_base=0, **VSAMPLED)[0]
    s = m.open_session(slots=2, max_ref_frames=8, live_voices=1, **VSAMPLED)
    try:
        sv = s.create_voice(clip, _ref_text(0), sample_rate=16000)
        assert _info(sv) == _info(ov)
        assert s.submit(_named(r, sv)) == 0
        got = s.result(0, timeout=WAIT)
        s.close()
    finally:
        s.close(drain=False)
    _same(got, want)
    _same(m.generate_batch([_named(r, sv)], row_base=0, **VSAMPLED)[0], want)
    sv.close()
    ov.close()


# ---------------------------------------------------------------------------------------------------
# 4. free while in use; the next voice gets the slot
# ---------------------------------------------------------------------------------------------------
def test_free_while_in_use_and_slot_reuse(live):
    from qwen3tts import Qwen3TTSError, Voice
    m, _ = live
    want = [_alone(m, 0, 0, **STREAMED), _alone(m, 1, 1, **STREAMED)]
    n0 = m.debug_prefix_states()[0]
    s = m.open_session(slots=2, max_ref_frames=LONGEST, live_voices=1, max_voices=1, **STREAMED, **VSAMPLED)
    ghost = Voice.__new__(Voice)  # the freed voice's handle, to name it once more
    ghost._model, ghost._session, ghost._h = m, None, None
    try:
        sv = s.create_voice(_clip(0), _ref_text(0))
        assert s.submit(_named(_audio_req(0), sv)) == 0
        ghost._h, ghost.info = sv._h, sv.info
        sv.close()  # at once: the ticket still completes, the voice can be named no more
        with pytest.raises(Qwen3TTSError) as e:
            s.submit(_named(_audio_req(1), ghost))
        assert e.value.status == 3
        ghost._h = None
        _same(s.result(0, timeout=WAIT), want[0])
        assert s.voice_stats().deferred_frees == 1
        _until(lambda: s.voice_stats().alive == 0)
        # max_voices = 1: the next voice takes the same place; what the first one's reference left in the decoder's tail must
        # not be taken for the second one's
        sv2 = s.create_voice(_clip(1), _ref_text(1))
        assert s.submit(_named(_audio_req(1), sv2)) == 1  # (the refused submit used no ticket)
        _same(s.result(1, timeout=WAIT), want[1])
        s.close()
    finally:
        ghost._h = None
        s.close(drain=False)
    # the freed voice's saved state went with it; the second voice keeps its one, in the pool slot's place, until it is closed
    assert m.debug_prefix_states()[0] == n0 + 1
    sv2.close()
    assert m.debug_prefix_states()[0] == n0


# ---------------------------------------------------------------------------------------------------
# 5. an idle session
# ---------------------------------------------------------------------------------------------------
def test_an_idle_session_makes_a_voice_without_a_frame_step(live):
    m, voices = live
    want = _alone(m, 1, 0)
    s = m.open_session(slots=2, max_ref_frames=LONGEST, live_voices=1, **VSAMPLED)
    try:
        before = s.stats().frame_steps
        sv = s.create_voice(_clip(1), _ref_text(1))
        sv.wait(timeout=WAIT)
        vs = s.voice_stats()
        assert (vs.ready, vs.in_flight, vs.frame_steps_beside) == (1, 0, 0)
        assert s.stats().frame_steps == before
        assert s.submit(_named(_audio_req(1), sv)) == 0
        _same(s.result(0, timeout=WAIT), want)
        s.close()
    finally:
        s.close(drain=False)
    assert _info(sv) == _info(voices[1])
    sv.close()


# ---------------------------------------------------------------------------------------------------
# 6. limits and refusals
# ---------------------------------------------------------------------------------------------------
def test_limits_and_refusals_leave_everything_usable(live, ckpt_dirs):
    from qwen3tts import Qwen3TTSError, Qwen3TTSModel, synth
    m, voices = live
    N = 12
    want = [_alone(m, 0, t, max_tokens=6) for t in range(N)]  # the plain ticket: request 0 on the ready-made voice, 6 frames
    nxt = {"t": 0}

    def still_fine(s):
        t = s.submit(_named(_audio_req(0, max_tokens=6), voices[0]))
        assert t == nxt["t"]  # (no refusal used a ticket)
        _same(s.result(t, timeout=WAIT), want[t])
        nxt["t"] += 1

    def refused(fn, status=3, word=None):
        with pytest.raises(Qwen3TTSError) as e:
            fn()
        assert e.value.status == status, (e.value.status, str(e.value))
        if word:
            assert word in str(e.value), str(e.value)

    state = {"tokens": 0, "wait": None, "made": [], "error": None}

    def on_event(i, kind, payload):
        if i != 0 or kind != "token":
            return
        state["tokens"] += 1
        if state["tokens"] != 1:
            return
        try:
            # the loop thread is here, so no job is launched or finished: live_voices = 1 refuses the second voice
            a = s.create_voice(_clip(0), _ref_text(0))
            state["made"].append(a)
            try:
                a.wait(timeout=0)  # would wait for the thread it runs on
            except Qwen3TTSError as e:
                state["wait"] = e.status
            try:
                state["made"].append(s.create_voice(_clip(1), _ref_text(1)))
            except Qwen3TTSError as e:
                state["made"].append(("refused", e.status))
        except Exception as e:
            state["error"] = e

    s = m.open_session(slots=1, max_ref_frames=LONGEST, live_voices=1, max_voices=2, on_event=on_event, **VSAMPLED)
    try:
        still_fine(s)
        assert state["error"] is None and state["wait"] == 3, state
        assert len(state["made"]) == 2 and state["made"][1] == ("refused", 9), state
        a = state["made"][0]
        a.wait(timeout=WAIT)
        still_fine(s)
        b = s.create_voice(_clip(1), _ref_text(1))
        b.wait(timeout=WAIT)
        refused(lambda: s.create_voice(_clip(0), _ref_text(0)), status=9)  # max_voices = 2 are alive
        still_fine(s)
        b.close()
        _until(lambda: s.voice_stats().alive == 1)
        refused(lambda: s.create_voice(synth.synthetic_reference_audio(1, 1.0), _ref_text(0)), word="max_ref_frames")
        still_fine(s)
        bad = _clip(0).copy()
        bad[100] = np.nan
        refused(lambda: s.create_voice(bad, _ref_text(0)), word="non-finite")
        still_fine(s)
        refused(lambda: s.create_voice(_clip(0), _ref_text(0), sample_rate=11025), word="sample_rate")
        still_fine(s)
        refused(lambda: s.create_voice(_clip(0), [1, 2, 3, 4]), word="ref_text_ids")
        still_fine(s)
        vs = s.voice_stats()
        assert (vs.created, vs.alive, vs.in_flight) == (2, 1, 0)  # nothing that was refused left a trace
        a.close()
        s.close()
    finally:
        s.close(drain=False)
    # ---- a session opened without live_voices is exactly the session it was ----
    s = m.open_session(slots=1, max_ref_frames=LONGEST, **VSAMPLED)
    nxt["t"] = 0
    try:
        refused(lambda: s.create_voice(_clip(0), _ref_text(0)), word="live_voices")
        still_fine(s)
        refused(lambda: s.submit(_audio_req(1)), word="voice-clone")
        still_fine(s)
        s.close()
    finally:
        s.close(drain=False)
    # ---- open ----
    refused(lambda: m.open_session(slots=1, max_ref_frames=LONGEST, live_voices=5, **VSAMPLED), word="live_voices")
    refused(lambda: m.open_session(slots=1, max_ref_frames=0, live_voices=1, **VSAMPLED), word="max_ref_frames")
    _same(m.generate_batch([_audio_req(0, max_tokens=6)], row_base=0, **VSAMPLED)[0], want[0])
    ma = Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-a"], max_batch=2, max_frames=32, max_prompt=64)
    try:
        refused(lambda: ma.open_session(slots=1, max_ref_frames=4, live_voices=1), status=1)
        ma.open_session(slots=1).close()  # and the handle takes a session still
    finally:
        ma.close()


# ---------------------------------------------------------------------------------------------------
# 7. close without drain
# ---------------------------------------------------------------------------------------------------
def test_close_without_drain_with_jobs_outstanding(live):
    """One voice is made at ticket 0's first token and a second one a burst later, when the first one's job has been launched.
    The callback that made the second one does not return before the close without drain has begun: the loop thread is in
    it, so the second job cannot have been launched and must be abandoned. A thread that waits for that voice (through the
    library, inside the held callback, while the session is certain to exist) sees CANCELLED -- that is also how the callback
    learns that the close has begun. The launched job finishes. Afterwards the abandoned voice is refused wherever a voice is
    named, both voices can be freed, and the engine is usable."""
    import ctypes as C
    from qwen3tts import Qwen3TTSError
    m, voices = live
    want = _alone(m, 0, 0)
    assert want.codes.shape[0] >= 2
    state = {"tokens": 0, "made": [], "error": None, "wait": None}
    second_in, waited = threading.Event(), threading.Event()
    second_at = min(10, want.codes.shape[0])

    def on_event(i, kind, payload):
        if i != 0 or kind != "token":
            return
        state["tokens"] += 1
        try:
            if state["tokens"] == 1:
                state["made"].append(s.create_voice(_clip(0), _ref_text(0)))
            elif state["tokens"] == second_at:  # (a burst is 9 frame steps: at 10 the loop has been through while_burst_runs since)
                b = s.create_voice(_clip(1), _ref_text(1))
                state["made"].append(b)
                h = s._h  # (Session.close clears it before it calls the library)

                def waiter():
                    ready = C.c_int32(0)
                    state["wait"] = (m._lib.q3tts_session_voice_wait(h, b._h, WAIT * 1000, C.byref(ready)), ready.value)
                    waited.set()

                threading.Thread(target=waiter).start()
                second_in.set()
                assert waited.wait(WAIT)  # the close has abandoned the job; the session lives while this callback runs
        except Exception as e:
            state["error"] = e
            second_in.set()

    s = m.open_session(slots=2, max_ref_frames=LONGEST, live_voices=2, on_event=on_event, **VSAMPLED)
    closer = threading.Thread(target=lambda: s.close(drain=False))
    try:
        assert s.submit(_named(_audio_req(0), voices[0])) == 0
        assert second_in.wait(WAIT) and state["error"] is None, state
        closer.start()
        closer.join(WAIT)
        assert not closer.is_alive()
    finally:
        if not closer.is_alive():
            s.close(drain=False)
    assert state["error"] is None and len(state["made"]) == 2, state
    assert state["wait"] == (8, 0), state  # Q3TTS_ERR_CANCELLED through q3tts_session_voice_wait
    outcomes = []
    for k, v in enumerate(state["made"]):
        with pytest.raises(Qwen3TTSError) as e:  # the session is gone: nothing to wait on
            v.wait(timeout=0)
        assert e.value.status == 3
        assert _info(v) == _info(voices[k])
        try:  # ready (then it is the clip's voice) or abandoned (then it is refused wherever a voice is named)
            _same(m.generate_batch([_named(_audio_req(k), v)], row_base=k, **VSAMPLED)[0], _alone(m, k, k))
            outcomes.append("ready")
        except Qwen3TTSError as e:
            assert e.status == 3 and "abandoned" in str(e), str(e)
            outcomes.append("abandoned")
    print("voices", outcomes)
    assert outcomes[1] == "abandoned"
    if second_at == 10:  # the first job had been launched: it finished
        assert outcomes[0] == "ready"
    s2 = m.open_session(slots=1, max_ref_frames=LONGEST, **VSAMPLED)  # a later session refuses the abandoned voice as well
    try:
        with pytest.raises(Qwen3TTSError) as e:
            s2.submit(_named(_audio_req(1), state["made"][1]))
        assert e.value.status == 3 and "abandoned" in str(e.value)
        s2.close()
    finally:
        s2.close(drain=False)
    for v in state["made"]:
        v.close()
    _same(m.generate_batch([_audio_req(0)], row_base=0, **VSAMPLED)[0], want)
