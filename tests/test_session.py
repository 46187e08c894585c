"""Serving session (q3tts_session_*): the slot loop of q3tts_generate_queued with an open end. Requests are submitted,
cancelled and collected one by one while the loop runs on the session's own thread. Ticket t must come out bit-identical to
that request alone at row_base = t -- and to results[t] of the closed queue over the same requests -- whatever its arrival
time, its slot, what ran beside it, whether the session was idle before it and what was cancelled around it. An idle session
launches nothing; a cancelled request leaves its slot at the next burst boundary and reports nothing from there on; bad calls
are refused and leave the session and the engine usable. Every wait carries a timeout, so a defect fails instead of hanging."""
import dataclasses
import threading
import time

import numpy as np
import pytest

from conftest import tiny_request

pytestmark = pytest.mark.gpu

BURST = 9   # frame steps per burst of a one-lane engine (engine_queue.cc: max_inflight_frames / 2)
WAIT = 60   # seconds: every result() below
SPF = 1920
C_, W_, L_ = 8, 32, 4
STREAM = dict(audio_chunk_frames=C_, audio_window_frames=W_, audio_lookahead_frames=L_)
SAMPLINGS = [dict(temperature=0.0, repetition_penalty=1.0), dict(temperature=0.9, top_k=40, repetition_penalty=1.05, seed=77)]
SAMPLED = SAMPLINGS[1]


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


@pytest.fixture(scope="module")
def models(ckpt_dirs):
    from qwen3tts import Qwen3TTSModel
    out = {g: Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], max_batch=4, max_frames=64, max_prompt=96, use_graph=g)
           for g in (True, False)}
    yield out
    for m in out.values():
        m.close()


_ALONE = {}


def _alone(m, reqs, kw, row_base=0, **extra):
    """Every request alone at row_base + its index, computed once per (model, sampling, streaming form) and shared."""
    key = (id(m), tuple(sorted(kw.items())), row_base, tuple(sorted(extra.items())), len(reqs))
    if key not in _ALONE:
        _ALONE[key] = [m.generate_batch([r], row_base=row_base + i, **kw, **extra)[0] for i, r in enumerate(reqs)]
    return _ALONE[key]


class Log:
    def __init__(self):
        self.events = []  # (ticket, kind, payload)

    def __call__(self, i, kind, payload):
        self.events.append((i, kind, payload))

    def kinds(self, t):
        return [k for (i, k, _) in self.events if i == t]


# ---------------------------------------------------------------------------------------------------
# 1. equals alone, whatever the arrival
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph,kw,row_base", [(True, SAMPLINGS[0], 0), (True, SAMPLINGS[1], 0), (False, SAMPLINGS[1], 0),
                                               (True, SAMPLINGS[1], 100)], ids=["greedy", "sampled", "sampled-eager", "row_base"])
def test_equals_alone_whatever_the_arrival(models, graph, kw, row_base):
    """Three waves through a 3-slot session: four requests at once, three more from the callback at ticket 0's 5th TOKEN (its
    last one, should it be shorter), three more once the session has gone idle and has to wake."""
    m = models[graph]
    reqs = _mixed()
    alone = _alone(m, reqs, kw, row_base)
    closed = m.generate_queued(reqs, slots=3, row_base=row_base, **kw)
    trigger = min(5, alone[0].codes.shape[0])
    state = {"tokens": 0, "wave2": [], "error": None}
    wave1_in = threading.Event()  # (the callback's submits follow the first wave's, so that the tickets are the indices)
    log = Log()

    def on_event(i, kind, payload):
        log(i, kind, payload)
        if i == 0 and kind == "token":
            state["tokens"] += 1
            if state["tokens"] == trigger:
                try:
                    assert wave1_in.wait(WAIT)
                    state["wave2"] = [s.submit(r) for r in reqs[4:7]]
                except Exception as e:  # (an exception must not cross the C callback)
                    state["error"] = e

    s = m.open_session(slots=3, on_event=on_event, row_base=row_base, **kw)
    try:
        wave1 = [s.submit(r) for r in reqs[:4]]
        wave1_in.set()
        assert wave1 == [0, 1, 2, 3]
        if trigger == 0:
            state["wave2"] = [s.submit(r) for r in reqs[4:7]]
        got = {0: s.result(0, timeout=WAIT)}
        assert state["error"] is None and state["wave2"] == [4, 5, 6], state
        for t in range(1, 7):
            got[t] = s.result(t, timeout=WAIT)
        st = s.stats()
        assert (st.running, st.pending, st.submitted) == (0, 0, 7)  # idle: the loop thread sleeps until the next submit
        assert [s.submit(r) for r in reqs[7:]] == [7, 8, 9]
        for t in range(7, 10):
            got[t] = s.result(t, timeout=WAIT)
        st = s.stats()
        assert st.completed == 10 and st.cancelled == 0 and st.admissions == 10
        s.close()
    finally:
        s.close(drain=False)
    for t in range(10):
        _same(got[t], alone[t])
        _same(got[t], closed[t])
        if got[t].status == 0:
            assert log.kinds(t) == ["token"] * got[t].codes.shape[0] + ["info", "audio"], t


# ---------------------------------------------------------------------------------------------------
# 2. idle is idle
# ---------------------------------------------------------------------------------------------------
def test_an_idle_session_launches_nothing(models):
    m = models[True]
    reqs = _mixed()
    alone = _alone(m, reqs, SAMPLED)
    s = m.open_session(slots=3, **SAMPLED)
    try:
        assert s.submit(reqs[0]) == 0
        _same(s.result(0, timeout=WAIT), alone[0])
        before = s.stats().frame_steps
        time.sleep(0.3)
        st = s.stats()
        assert st.frame_steps == before and st.running == 0
        assert s.submit(reqs[1]) == 1
        _same(s.result(1, timeout=WAIT), alone[1])
        assert s.stats().frame_steps > before or alone[1].codes.shape[0] == 0
        s.close()
    finally:
        s.close(drain=False)


# ---------------------------------------------------------------------------------------------------
# 3. concurrent submit
# ---------------------------------------------------------------------------------------------------
def test_concurrent_submits_get_dense_tickets(models):
    m = models[True]
    reqs = _mixed() + _mixed()[:2]
    mine = {k: [] for k in range(4)}  # thread -> [(ticket, request index)]
    errors = []
    s = m.open_session(slots=4, **SAMPLED)
    try:
        def producer(k):
            try:
                for j in range(3):
                    i = 3 * k + j
                    mine[k].append((s.submit(reqs[i]), i))
            except Exception as e:
                errors.append(e)

        th = [threading.Thread(target=producer, args=(k,)) for k in range(4)]
        for t in th:
            t.start()
        for t in th:
            t.join(WAIT)
        assert not errors, errors
        which = dict(p for v in mine.values() for p in v)
        assert sorted(which) == list(range(12))
        for v in mine.values():
            assert [t for t, _ in v] == sorted(t for t, _ in v)  # a thread's tickets ascend
        got = {t: s.result(t, timeout=WAIT) for t in range(12)}
        s.close()
    finally:
        s.close(drain=False)
    for t in range(12):
        _same(got[t], m.generate_batch([reqs[which[t]]], row_base=t, **SAMPLED)[0])


def test_concurrent_refusals_keep_their_own_messages(models):
    """Refused session calls on several threads at once: each thread reads the message of its own refusal (q3tts_last_error is
    per thread for them), and the session goes on."""
    from qwen3tts import Qwen3TTSError
    m = models[True]
    reqs = _mixed()
    alone = _alone(m, reqs, SAMPLED)
    errors = []
    s = m.open_session(slots=2, **SAMPLED)
    try:
        calls = [(lambda: s.submit(_req(row=9, n_text=6, max_tokens=65)), "max_frames"),
                 (lambda: s.submit(reqs[1], top_p=1.5), "top_p"),
                 (lambda: s.cancel(999), "ticket"),
                 (lambda: s.result(999, timeout=0), "ticket")]

        def worker(fn, word):
            try:
                for _ in range(50):
                    try:
                        fn()
                        errors.append("accepted")
                    except Qwen3TTSError as e:
                        if e.status != 3 or word not in str(e):
                            errors.append((word, e.status, str(e)))
            except Exception as e:
                errors.append(e)

        th = [threading.Thread(target=worker, args=c) for c in calls]
        for t in th:
            t.start()
        assert s.submit(reqs[0]) == 0  # beside them
        for t in th:
            t.join(WAIT)
        assert not errors, errors[:3]
        _same(s.result(0, timeout=WAIT), alone[0])
        assert s.stats().submitted == 1
        s.close()
    finally:
        s.close(drain=False)


# ---------------------------------------------------------------------------------------------------
# 4. cancel
# ---------------------------------------------------------------------------------------------------
def test_cancel_running_and_pending(models):
    """slots = 2. Ticket 0 is long and is cancelled from the callback at its 3rd TOKEN; a ticket submitted and cancelled inside
    one callback is certainly still pending (the loop thread is inside that callback)."""
    from qwen3tts import Qwen3TTSError
    m = models[True]
    reqs = [_req(row=0, n_text=9, max_tokens=60)] + [_req(row=1 + i, n_text=5 + i, max_tokens=6) for i in range(5)]
    # a seed under which the long request really is long (the search of test_slots_are_refilled_and_audio_leaves_early)
    seed = next((x for x in range(5, 50) if m.generate_batch(reqs[:1], temperature=0.9, top_k=50, seed=x)[0].codes.shape[0] >= 40), None)
    assert seed is not None, "no seed in 5..49 makes the long request generate 40 frames"
    kw = dict(temperature=0.9, top_k=50, seed=seed)
    state = {"tokens": 0, "pending": None, "error": None}
    first_in = threading.Event()  # (the callback's submit follows the first five, so that its ticket is 5)
    log = Log()

    def on_event(i, kind, payload):
        log(i, kind, payload)
        if i != 0 or kind != "token":
            return
        state["tokens"] += 1
        try:
            if state["tokens"] == 1:
                assert first_in.wait(WAIT)
                state["pending"] = s.submit(reqs[5])
                s.cancel(state["pending"])
            if state["tokens"] == 3:
                s.cancel(0)
        except Exception as e:
            state["error"] = e

    s = m.open_session(slots=2, on_event=on_event, **kw)
    try:
        first = [s.submit(r) for r in reqs[:5]]
        first_in.set()
        assert first == [0, 1, 2, 3, 4]
        r0 = s.result(0, timeout=WAIT)
        assert state["error"] is None and state["pending"] == 5, state
        assert r0.status == 8 and r0.codes.shape == (0, 16) and r0.audio.size == 0
        rp = s.result(5, timeout=WAIT)
        assert rp.status == 8 and rp.codes.shape == (0, 16) and log.kinds(5) == []
        late = s.submit(reqs[5])  # the same request again, now served
        assert late == 6
        got = {t: s.result(t, timeout=WAIT) for t in (1, 2, 3, 4, 6)}
        s.cancel(0)  # twice, and a completed one: OK, nothing changes
        s.cancel(1)
        with pytest.raises(Qwen3TTSError) as e:
            s.cancel(999)
        assert e.value.status == 3
        st = s.stats()
        assert (st.cancelled, st.completed, st.running, st.pending) == (2, 5, 0, 0)
        assert st.frame_steps < 60, st.frame_steps  # the long request's slot did not run to its cap of 60 ...
        assert st.admissions == 6, st.admissions    # ... and was refilled: every ticket but the pending one was admitted, two slots
        s.close()
    finally:
        s.close(drain=False)
    k0 = log.kinds(0)
    assert set(k0) == {"token"} and 3 <= len(k0) <= 3 + BURST, k0  # no INFO, no AUDIO; at most the burst that was being reported
    for t, i in ((1, 1), (2, 2), (3, 3), (4, 4), (6, 5)):
        _same(got[t], m.generate_batch([reqs[i]], row_base=t, **kw)[0])


# ---------------------------------------------------------------------------------------------------
# 5. streamed
# ---------------------------------------------------------------------------------------------------
def _check_chunks(log, t, g):
    mine = [(k, p) for (i, k, p) in log.events if i == t]
    kinds = [k for k, _ in mine]
    if g.status != 0:
        assert g.status == 2 and kinds == []
        return
    assert kinds[-2:] == ["info", "audio"] and set(kinds[:-2]) <= {"token", "audio_chunk"}, (t, kinds)
    assert kinds.count("token") == g.codes.shape[0]
    chunks = [p for k, p in mine if k == "audio_chunk"]
    assert [o for o, _ in chunks] == [k * C_ * SPF for k in range(len(chunks))], t
    assert len(chunks) == -(-g.codes.shape[0] // C_)
    assert np.array_equal(np.concatenate([c for _, c in chunks]), g.audio), t
    assert np.array_equal(mine[-1][1], g.audio)


def test_streamed_session_equals_each_request_streamed_alone(models):
    m = models[True]
    reqs = _mixed()
    alone = _alone(m, reqs, SAMPLED, 0, **STREAM)
    closed = m.generate_queued(reqs, slots=3, **STREAM, **SAMPLED)
    log = Log()
    s = m.open_session(slots=3, on_event=log, **STREAM, **SAMPLED)
    try:
        assert [s.submit(r) for r in reqs[:6]] == list(range(6))
        got = {t: s.result(t, timeout=WAIT) for t in range(6)}
        assert s.stats().running == 0
        assert [s.submit(r) for r in reqs[6:]] == [6, 7, 8, 9]  # after an idle spell
        got.update({t: s.result(t, timeout=WAIT) for t in range(6, 10)})
        s.close()
    finally:
        s.close(drain=False)
    for t in range(10):
        _same(got[t], alone[t])
        _same(got[t], closed[t])
        _check_chunks(log, t, got[t])
        n = got[t].codes.shape[0]
        if n:
            assert np.array_equal(got[t].audio, m.codec_decode_streamed(got[t].codes[None], C_, W_, L_)[0][:n * SPF])


def test_a_streamed_request_cancelled_midway_leaves_an_exact_slot(models):
    """One slot, so the next ticket takes the very row -- stream state, code row, chunk counters -- the cancelled one left."""
    m = models[True]
    reqs = [_req(row=0, n_text=9, max_tokens=60), _req(row=1, n_text=7, max_tokens=30), _req(row=2, n_text=6, max_tokens=13)]
    seed = next((x for x in range(5, 50) if m.generate_batch(reqs[:1], temperature=0.9, top_k=50, seed=x)[0].codes.shape[0] >= 40), None)
    assert seed is not None, "no seed in 5..49 makes the long request generate 40 frames"
    kw = dict(temperature=0.9, top_k=50, seed=seed)
    state = {"tokens": 0, "at": None, "error": None}
    log = Log()

    def on_event(i, kind, payload):
        log(i, kind, payload)
        if i == 0 and kind == "token":
            state["tokens"] += 1
            if state["tokens"] == 2 * BURST + 2:  # in the third burst: chunks 0 and 1 have been issued, more are in flight
                try:
                    s.cancel(0)
                    state["at"] = len(log.events)
                except Exception as e:
                    state["error"] = e

    s = m.open_session(slots=1, on_event=on_event, **STREAM, **kw)
    try:
        assert [s.submit(r) for r in reqs] == [0, 1, 2]
        r0 = s.result(0, timeout=WAIT)
        got = {t: s.result(t, timeout=WAIT) for t in (1, 2)}
        s.close()
    finally:
        s.close(drain=False)
    assert state["error"] is None and state["at"] is not None
    assert r0.status == 8 and r0.codes.shape == (0, 16) and r0.audio.size == 0
    after = [k for (i, k, _) in log.events[state["at"]:] if i == 0]
    assert set(after) <= {"token"} and len(after) <= BURST, after  # nothing but the burst that was being reported
    assert "info" not in log.kinds(0) and "audio" not in log.kinds(0)
    for t in (1, 2):
        _same(got[t], m.generate_batch([reqs[t]], row_base=t, **STREAM, **kw)[0])
        _check_chunks(log, t, got[t])


# ---------------------------------------------------------------------------------------------------
# 6. voices
# ---------------------------------------------------------------------------------------------------
CLIPS = [(0, 0.3), (2, 0.5)]  # (row of the synthetic clip and reference text, seconds): 4 and 7 reference frames
VSAMPLED = dict(temperature=0.9, top_k=40, repetition_penalty=1.5, seed=77)


def _clip(k):
    from qwen3tts import synth
    return synth.synthetic_reference_audio(*CLIPS[k])


def _prompt(row, n_text=10):
    from qwen3tts import synth
    return synth.synthetic_prompt(row, n_text=n_text, text_vocab=1000, im_start=1000, im_end=1001)


@pytest.fixture(scope="module")
def voiced(tmp_path_factory):
    from qwen3tts import Qwen3TTSModel, synth
    d = str(tmp_path_factory.mktemp("session_voices") / "tiny-base")
    synth.write_checkpoint(d, "tiny-base", seed=4321)
    m = Qwen3TTSModel.from_pretrained(d, max_batch=4, max_frames=64, max_prompt=160)
    voices = [m.create_voice(_clip(k), _prompt(CLIPS[k][0])["ref_text_ids"]) for k in range(2)]
    yield m, voices
    for v in voices:
        v.close()
    m.close()


def _voice_reqs(voices):
    from qwen3tts import GenerationRequest
    out = []
    for i, (k, n_text, mt) in enumerate([(0, 8, 21), (1, 11, 26), (0, 6, 19), (1, 9, 23)]):
        p = _prompt(i, n_text)
        out.append(GenerationRequest(p["text_ids"], p["target_token_count"], None, None, "english", mt, voice=voices[k]))
    return out


def _audio_form(r, voices):
    k = voices.index(r.voice)
    return dataclasses.replace(r, voice=None, ref_audio=_clip(k), ref_text_ids=_prompt(CLIPS[k][0])["ref_text_ids"])


@pytest.mark.parametrize("streamed", [False, True], ids=["whole", "streamed"])
def test_voices_in_a_session(voiced, streamed):
    from qwen3tts import Qwen3TTSError
    m, voices = voiced
    reqs = _voice_reqs(voices)
    form = dict(audio_stream_reference=1, **STREAM) if streamed else {}
    want = [m.generate_batch([_audio_form(r, voices)], row_base=t, **form, **VSAMPLED)[0] for t, r in enumerate(reqs)]
    longest = max(v.info.ref_frames for v in voices)
    n0, _, r0 = m.debug_prefix_states()
    s = m.open_session(slots=1, max_ref_frames=longest, **form, **VSAMPLED)  # one slot: the admissions come one after another
    try:
        assert [s.submit(r) for r in reqs] == [0, 1, 2, 3]
        got = [s.result(t, timeout=WAIT) for t in range(4)]
        s.close()
    finally:
        s.close(drain=False)
    for t in range(4):
        _same(got[t], want[t])
    n1, _, r1 = m.debug_prefix_states()
    if streamed:  # each voice's reference was decoded at its first admission and put back at its second
        assert (n1 - n0, r1 - r0) == (2, 2)
    else:
        assert (n1 - n0, r1 - r0) == (0, 0)
    # a voice beyond max_ref_frames is refused at submit and uses no ticket
    short = min(v.info.ref_frames for v in voices)
    assert short < longest
    s = m.open_session(slots=2, max_ref_frames=short, **form, **VSAMPLED)
    try:
        with pytest.raises(Qwen3TTSError) as e:
            s.submit(reqs[1])
        assert e.value.status == 3 and "max_ref_frames" in str(e.value)
        assert s.submit(reqs[0]) == 0
        _same(s.result(0, timeout=WAIT), want[0])
        s.close()
    finally:
        s.close(drain=False)


# ---------------------------------------------------------------------------------------------------
# 7. refusals leave everything usable
# ---------------------------------------------------------------------------------------------------
def test_refusals_leave_the_session_and_the_engine_usable(models, ckpt_dirs):
    from qwen3tts import GenerationRequest, Qwen3TTSError, Qwen3TTSModel, synth
    m = models[True]
    kw = SAMPLED
    reqs = _mixed()
    alone = _alone(m, reqs, kw)

    def refused(fn, status=3, word=None):
        with pytest.raises(Qwen3TTSError) as e:
            fn()
        assert e.value.status == status, (e.value.status, str(e.value))
        if word:
            assert word in str(e.value), str(e.value)

    # ---- open ----
    refused(lambda: m.open_session(slots=0, **kw), word="slots")
    refused(lambda: m.open_session(slots=5, **kw), word="slots")
    refused(lambda: m.open_session(slots=2, audio_chunk_frames=4, **kw), word="audio_chunk_frames")
    job = m.generate_batch_begin(reqs[:1], **kw)
    try:
        refused(lambda: m.open_session(slots=2, **kw), word="outstanding")
    finally:
        _same(m.generate_batch_end(job)[0], alone[0])

    state = {"wait": None, "busy": [], "error": None, "tokens": 0}

    def on_event(i, kind, payload):
        if i != 0 or kind != "token":
            return
        state["tokens"] += 1
        if state["tokens"] != 1:
            return
        try:
            try:  # wait from inside a callback would wait for the thread it runs on
                s.result(0, timeout=0)
            except Qwen3TTSError as e:
                state["wait"] = e.status
            # the loop thread is here, so whatever is submitted now stays pending: max_pending = 2 refuses the third
            for r in reqs[1:4]:
                try:
                    state["busy"].append(s.submit(r))
                except Qwen3TTSError as e:
                    state["busy"].append(("refused", e.status))
        except Exception as e:
            state["error"] = e

    s = m.open_session(slots=1, max_pending=2, on_event=on_event, **kw)
    try:
        refused(lambda: m.open_session(slots=2, **kw), word="already open")  # a second open
        assert s.submit(reqs[0]) == 0
        # ---- the engine's other entry points, while the session runs ----
        refused(lambda: m.generate_batch(reqs[:1], **kw), word="session is open")
        refused(lambda: m.generate_queued(reqs[:2], slots=2, **kw), word="session is open")
        refused(lambda: m.create_voice(synth.synthetic_reference_audio(0, 0.3), [1, 2, 3, 4, 5, 6]), word="session is open")
        refused(lambda: m.codec_decode(np.zeros((1, 4, 16), np.int32)), word="session is open")
        assert m.sample_rate == 24000 and m.last_timing() is not None  # what stays available
        # ---- submits that are refused use no ticket ----
        p = synth.synthetic_prompt(0, n_text=10, text_vocab=1000, im_start=1000, im_end=1001)
        clone = GenerationRequest(p["text_ids"], p["target_token_count"], None, None, "english",
                                  ref_audio=synth.synthetic_reference_audio(0, 0.5), ref_text_ids=p["ref_text_ids"])
        refused(lambda: s.submit(clone), word="voice-clone")
        refused(lambda: s.submit(_req(row=9, n_text=6, max_tokens=8, speaker="nobody")))
        refused(lambda: s.submit(_req(row=9, n_text=6, max_tokens=65)), word="max_frames")
        refused(lambda: s.submit(reqs[1], top_p=1.5), word="top_p")
        _same(s.result(0, timeout=WAIT), alone[0])
        assert state["error"] is None and state["wait"] == 3, state
        assert state["busy"] == [1, 2, ("refused", 9)], state
        for t in (1, 2):
            _same(s.result(t, timeout=WAIT), alone[t])
        refused(lambda: s.result(1, timeout=0))  # collected: forgotten
        assert s.submit(reqs[3]) == 3            # the refused submits used no ticket
        _same(s.result(3, timeout=WAIT), alone[3])
        assert s.submit(_req(row=4, n_text=9, max_tokens=60)) == 4
        with pytest.raises(TimeoutError):
            s.result(4, timeout=0)
        # ---- close without drain, work outstanding ----
        s.submit(reqs[5])
        s.close(drain=False)
        refused(lambda: s.result(4, timeout=0))
        refused(lambda: s.submit(reqs[0]))
    finally:
        s.close(drain=False)
    _same(m.generate_batch(reqs[:1], **kw)[0], alone[0])
    for i, g in enumerate(m.generate_queued(reqs[:3], slots=2, **kw)):
        _same(g, alone[i])
    # ---- a model closed with a session open ----
    m2 = Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], max_batch=2, max_frames=64, max_prompt=96)
    s2 = m2.open_session(slots=2, **kw)
    s2.submit(_req(row=0, n_text=9, max_tokens=60))
    s2.submit(reqs[1])
    t0 = time.time()
    m2.close()
    assert time.time() - t0 < WAIT
    refused(lambda: s2.stats())
