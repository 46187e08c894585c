"""Open-text requests of a serving session (q3tts_session_submit_open / _append_text): a request whose text arrives while it is
being spoken. Whatever the timing -- all text before the admission, text fed from the TOKEN callback, text that arrives after
the row ran dry and sat waiting, any pieces of any sizes -- ticket t must come out bit-identical to the ORDINARY request over
the whole text alone at row_base = t. A row that needs text that has not arrived starves: it takes no frame step, and a session
whose running rows all starve launches nothing. Every wait carries a timeout, so a defect fails instead of hanging; the starve
tests observe the state through q3tts_session_get_text_stats, they do not race for it."""
import threading
import time

import numpy as np
import pytest

from conftest import tiny_request

pytestmark = pytest.mark.gpu

BURST = 9   # frame steps per burst of a one-lane engine (engine_queue.cc: max_inflight_frames / 2)
WAIT = 60   # seconds: every wait below
SPF = 1920
C_, W_, L_ = 8, 32, 4
STREAM = dict(audio_chunk_frames=C_, audio_window_frames=W_, audio_lookahead_frames=L_)
SAMPLINGS = [dict(temperature=0.0, repetition_penalty=1.0), dict(temperature=0.9, top_k=40, repetition_penalty=1.05, seed=77)]
SAMPLED = SAMPLINGS[1]
MAX_PROMPT = 96


def _parts(row, n_content):
    ids = list(tiny_request(row=row, n_text=n_content)["text_ids"])
    return ids[:3], ids[3:3 + n_content], ids[3 + n_content:]


def _whole(row, n_content, max_tokens, upto=None):
    """The ordinary request over the first `upto` content tokens (all of them by default)."""
    from qwen3tts import GenerationRequest
    role, content, tail = _parts(row, n_content)
    content = content[:n_content if upto is None else upto]
    return GenerationRequest(role + content + tail, len(content), None, "aiden", "english", max_tokens)


def _open(row, n_content, max_tokens, first):
    """(the open-text request holding the first `first` content tokens, the content that follows)"""
    from qwen3tts import GenerationRequest
    role, content, _ = _parts(row, n_content)
    return GenerationRequest(role + content[:first], 0, None, "aiden", "english", max_tokens), content[first:]


def _same(got, want):
    assert got.status == want.status
    assert got.codes.shape == want.codes.shape and np.array_equal(got.codes, want.codes)
    assert got.audio.shape == want.audio.shape and np.array_equal(got.audio, want.audio)
    assert got.info.generation_token_count == want.info.generation_token_count


def _until(cond, what):
    end = time.monotonic() + WAIT
    while not cond():
        assert time.monotonic() < end, "timed out waiting for " + what
        time.sleep(0.002)


def _starved(s, n, events=None):
    def ok():
        st = s.text_stats()
        return st.starved == n and (events is None or st.starve_events >= events)
    _until(ok, "starved == %d" % n)


@pytest.fixture(scope="module")
def models(ckpt_dirs):
    from qwen3tts import Qwen3TTSModel
    out = {g: Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], max_batch=4, max_frames=64, max_prompt=MAX_PROMPT, use_graph=g)
           for g in (True, False)}
    yield out
    for m in out.values():
        m.close()


class Log:
    def __init__(self):
        self.events = []  # (ticket, kind, payload)

    def __call__(self, i, kind, payload):
        self.events.append((i, kind, payload))

    def of(self, t):
        return [(k, p) for (i, k, p) in self.events if i == t]


# ---------------------------------------------------------------------------------------------------
# 1. dry and resume
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph,kw", [(True, SAMPLINGS[0]), (True, SAMPLINGS[1]), (False, SAMPLINGS[0]), (False, SAMPLINGS[1])],
                         ids=["greedy", "sampled", "greedy-eager", "sampled-eager"])
def test_dry_and_resume(models, graph, kw):
    """One request of 24 content tokens fed as 1 + 2 + 7 + 14: the row runs dry after each piece (the 7 are less than a burst, so it
    dries in the middle of one), a session whose only row is dry launches nothing, and the result is the whole request's."""
    m = models[graph]
    N, F = 24, 30
    want = m.generate_batch([_whole(0, N, 40)], row_base=0, force_frames=F, **kw)[0]
    req, rest = _open(0, N, 40, first=1)
    s = m.open_session(slots=2, force_frames=F, **kw)
    try:
        assert s.submit_open(req) == 0
        _starved(s, 1, events=1)
        assert s.text_stats().open == 1
        before = s.stats().frame_steps
        time.sleep(0.2)
        assert s.stats().frame_steps == before  # a starved session launches nothing
        s.append_text(0, rest[:2])
        _starved(s, 1, events=2)
        s.append_text(0, rest[2:9])
        _starved(s, 1, events=3)
        s.append_text(0, rest[9:], final=True)
        got = s.result(0, timeout=WAIT)
        st = s.text_stats()
        assert st.starve_events >= 3 and st.starved == 0 and st.open == 0 and st.appended_tokens == N - 1
        s.close()
    finally:
        s.close(drain=False)
    assert want.codes.shape[0] == F
    _same(got, want)


# ---------------------------------------------------------------------------------------------------
# 2. all text before the admission
# ---------------------------------------------------------------------------------------------------
def test_all_text_before_admission(models):
    """slots=1 and a blocker running: the open request gets all its pieces and its close while it is pending (from the blocker's
    first TOKEN callback: the loop thread is inside it, so nothing can be admitted meanwhile). It equals the request alone, and
    plain submit of the whole request."""
    m = models[True]
    N, F = 17, 22
    blocker, whole = _whole(1, 9, 40), _whole(2, N, 40)
    want = m.generate_batch([whole], row_base=1, force_frames=F, **SAMPLED)[0]
    req, rest = _open(2, N, 40, first=3)
    open_in = threading.Event()
    state = {"fed": False, "error": None}

    def on_event(i, kind, payload):
        if i == 0 and kind == "token" and not state["fed"]:
            state["fed"] = True
            try:
                assert open_in.wait(WAIT)
                assert s.stats().pending == 1
                s.append_text(1, rest[:1])
                s.append_text(1, rest[1:6])
                s.append_text(1, [])
                s.append_text(1, rest[6:])
                s.close_text(1)
            except Exception as e:  # (an exception must not cross the C callback)
                state["error"] = e

    s = m.open_session(slots=1, on_event=on_event, force_frames=F, **SAMPLED)
    try:
        assert s.submit(blocker) == 0
        assert s.submit_open(req) == 1
        open_in.set()
        got = s.result(1, timeout=WAIT)
        assert state["error"] is None and state["fed"], state
        assert s.text_stats().starve_events == 0
        s.close()
    finally:
        s.close(drain=False)
    _same(got, want)
    s = m.open_session(slots=1, force_frames=F, **SAMPLED)
    try:
        assert [s.submit(blocker), s.submit(whole)] == [0, 1]
        plain = s.result(1, timeout=WAIT)
        s.close()
    finally:
        s.close(drain=False)
    _same(got, plain)


# ---------------------------------------------------------------------------------------------------
# 3. fed from the callback
# ---------------------------------------------------------------------------------------------------
def test_fed_from_the_token_callback(models):
    """One token appended per TOKEN event of the ticket itself. TOKEN events fire at burst boundaries, a burst's worth at a time,
    so a request that starts BURST + 1 tokens deep stays exactly ahead of the need: it never starves."""
    m = models[True]
    N, F = 28, 32
    want = m.generate_batch([_whole(3, N, 40)], row_base=0, force_frames=F, **SAMPLED)[0]
    req, rest = _open(3, N, 40, first=BURST + 1)
    state = {"next": 0, "error": None}

    def on_event(i, kind, payload):
        if i == 0 and kind == "token" and state["next"] < len(rest):
            try:
                k = state["next"]
                state["next"] = k + 1
                s.append_text(0, rest[k:k + 1], final=(k + 1 == len(rest)))
            except Exception as e:
                state["error"] = e

    s = m.open_session(slots=2, on_event=on_event, force_frames=F, **SAMPLED)
    try:
        assert s.submit_open(req) == 0
        got = s.result(0, timeout=WAIT)
        assert state["error"] is None and state["next"] == len(rest), state
        st = s.text_stats()
        assert st.starve_events == 0 and st.appended_tokens == len(rest)
        s.close()
    finally:
        s.close(drain=False)
    _same(got, want)


# ---------------------------------------------------------------------------------------------------
# 4. beside others, one cancelled while starved
# ---------------------------------------------------------------------------------------------------
def test_beside_others_and_cancelled_while_starved(models):
    m = models[True]
    F, NA, NB = 26, 24, 12
    plain0, plain3 = _whole(4, 9, 40), _whole(7, 14, 40)
    alone = {0: m.generate_batch([plain0], row_base=0, force_frames=F, **SAMPLED)[0],
             1: m.generate_batch([_whole(5, NA, 40)], row_base=1, force_frames=F, **SAMPLED)[0],
             3: m.generate_batch([plain3], row_base=3, force_frames=F, **SAMPLED)[0]}
    a, rest_a = _open(5, NA, 40, first=1)
    b, rest_b = _open(6, NB, 40, first=1)
    log = Log()
    s = m.open_session(slots=3, on_event=log, force_frames=F, **SAMPLED)
    try:
        assert [s.submit(plain0), s.submit_open(a), s.submit_open(b), s.submit(plain3)] == [0, 1, 2, 3]
        _starved(s, 2, events=2)
        s.append_text(2, rest_b[:3])
        _starved(s, 2, events=3)
        s.cancel(2)  # while it waits for text
        got2 = s.result(2, timeout=WAIT)
        n_events_2 = len(log.of(2))
        _starved(s, 1)
        s.append_text(1, rest_a[:1])
        _starved(s, 1, events=4)
        s.append_text(1, rest_a[1:4])
        _starved(s, 1, events=5)
        s.append_text(1, rest_a[4:14])
        s.append_text(1, rest_a[14:], final=True)
        got = {t: s.result(t, timeout=WAIT) for t in (0, 1, 3)}
        s.append_text(2, rest_b[3:5])  # a cancelled ticket: dropped, no error
        s.close()
    finally:
        s.close(drain=False)
    assert got2.status == 8
    assert len(log.of(2)) == n_events_2  # no event after the boundary that cancelled it
    assert [k for k, _ in log.of(2)] == ["token"] * n_events_2
    for t in (0, 1, 3):
        _same(got[t], alone[t])


# ---------------------------------------------------------------------------------------------------
# 5. streamed
# ---------------------------------------------------------------------------------------------------
def test_streamed_chunks_leave_while_starved(models):
    m = models[True]
    N, F, first = 20, 28, 12
    want = m.generate_batch([_whole(8, N, 40)], row_base=0, force_frames=F, **SAMPLED, **STREAM)[0]
    req, rest = _open(8, N, 40, first=first)
    log = Log()
    s = m.open_session(slots=2, on_event=log, force_frames=F, **SAMPLED, **STREAM)
    try:
        assert s.submit_open(req) == 0
        _starved(s, 1, events=1)
        # `first` frames exist: chunk 0 (frames 0..C-1, lookahead up to C + L <= first) is decodable and leaves while the row waits
        _until(lambda: any(k == "audio_chunk" for k, _ in log.of(0)), "a chunk while starved")
        st = s.text_stats()
        assert st.starved == 1 and [k for k, _ in log.of(0)].count("token") == first
        assert not any(k in ("info", "audio") for k, _ in log.of(0))  # a starved row is not final
        s.append_text(0, rest, final=True)
        got = s.result(0, timeout=WAIT)
        s.close()
    finally:
        s.close(drain=False)
    _same(got, want)
    mine = log.of(0)
    kinds = [k for k, _ in mine]
    assert kinds[-2:] == ["info", "audio"] and kinds.count("token") == F
    chunks = [p for k, p in mine if k == "audio_chunk"]
    assert [o for o, _ in chunks] == [k * C_ * SPF for k in range(len(chunks))]
    assert len(chunks) == -(-F // C_)
    assert np.array_equal(np.concatenate([c for _, c in chunks]), got.audio)
    assert np.array_equal(mine[-1][1], got.audio)


# ---------------------------------------------------------------------------------------------------
# 6. the cap at the close
# ---------------------------------------------------------------------------------------------------
def test_cap_at_close_and_cap_hit_while_open(models):
    """No force_frames here: the caps are the requests' own. (a) 5 content tokens, max_tokens 40, closed early: the cap becomes
    min(40, max(75, 30)) = 40. (b) max_tokens 6 with 7 content tokens: the row hits its cap while its text is still open, and
    an append after that is accepted and dropped."""
    m = models[True]
    want_a = m.generate_batch([_whole(9, 5, 40)], row_base=0, **SAMPLED)[0]
    want_b = m.generate_batch([_whole(10, 12, 6, upto=7)], row_base=1, **SAMPLED)[0]
    a, rest_a = _open(9, 5, 40, first=2)
    b, rest_b = _open(10, 12, 6, first=7)
    s = m.open_session(slots=2, **SAMPLED)
    try:
        assert s.submit_open(a) == 0
        s.append_text(0, rest_a, final=True)
        assert s.submit_open(b) == 1
        _until(lambda: s.stats().completed >= 2, "both results")
        before = s.text_stats().appended_tokens
        s.append_text(1, rest_b[:3])  # its row ended at the cap: OK, dropped
        assert s.text_stats().appended_tokens == before
        got_a, got_b = s.result(0, timeout=WAIT), s.result(1, timeout=WAIT)
        s.append_text(1, rest_b[3:], final=True)  # collected: still OK, still dropped
        s.close()
    finally:
        s.close(drain=False)
    _same(got_a, want_a)
    _same(got_b, want_b)
    assert got_b.status != 0 or got_b.codes.shape[0] <= 6


# ---------------------------------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------------------------------
def test_refusals_leave_the_session_serving(models):
    from qwen3tts import GenerationRequest, Qwen3TTSError
    m = models[True]
    plain = _whole(11, 9, 12)
    want = {t: m.generate_batch([plain], row_base=t, **SAMPLED)[0] for t in (0, 2, 3)}
    role, content, tail = _parts(12, MAX_PROMPT + 8)

    def refused(fn, word=None):
        with pytest.raises(Qwen3TTSError) as e:
            fn()
        assert e.value.status == 3, e.value
        if word:
            assert word in str(e.value), e.value

    s = m.open_session(slots=2, **SAMPLED)
    try:
        assert s.submit(plain) == 0
        refused(lambda: s.submit_open(GenerationRequest(role, 0, None, "aiden", "english", 40)), word="role")
        clone = GenerationRequest(role + content[:4], 0, None, "aiden", "english", 40)
        clone.ref_audio = np.zeros(2400, np.float32)
        clone.ref_text_ids = role + content[:4] + tail[:2]
        refused(lambda: s.submit_open(clone))
        voiced = GenerationRequest(role + content[:4], 0, None, "aiden", "english", 40)
        voiced.voice = object()
        refused(lambda: s.submit_open(voiced), word="voice")
        refused(lambda: s.submit_open(GenerationRequest(role + content[:4], 0, None, "aiden", "english", 65)), word="max_tokens")
        assert s.submit_open(GenerationRequest(role + content[:4], 0, None, "aiden", "english", 40)) == 1  # no refusal took a ticket
        refused(lambda: s.append_text(0, content[4:6]), word="open-text")      # a plain ticket
        refused(lambda: s.append_text(7, content[4:6]), word="no such ticket")  # never given out
        refused(lambda: s.append_text(-1, content[4:6]), word="no such ticket")
        refused(lambda: s.append_text(1, [3, 1024]), word="out of range")       # text_vocab_size of the fixture is 1024
        refused(lambda: s.append_text(1, [-1]), word="out of range")
        # the trailing text holds max_prompt rows, the tts_eos row included: at most max_prompt content tokens
        room = MAX_PROMPT - 4
        refused(lambda: s.append_text(1, content[4:4 + room + 1]), word="max_prompt")
        assert s.text_stats().appended_tokens == 0  # a refused append changes nothing
        s.append_text(1, content[4:4 + room])        # exactly full: accepted
        refused(lambda: s.append_text(1, content[:1]), word="max_prompt")
        s.close_text(1)
        refused(lambda: s.append_text(1, content[:1]), word="closed")
        refused(lambda: s.close_text(1), word="closed")
        assert s.submit(plain) == 2
        got = {t: s.result(t, timeout=WAIT) for t in (0, 1, 2)}
        refused(lambda: s.append_text(1, content[:1]), word="closed")  # collected, and still known as closed
        assert s.submit(plain) == 3
        got[3] = s.result(3, timeout=WAIT)
        s.close()
    finally:
        s.close(drain=False)
    for t in (0, 2, 3):
        _same(got[t], want[t])
    full = GenerationRequest(role + content[:MAX_PROMPT] + tail, MAX_PROMPT, None, "aiden", "english", 40)
    _same(got[1], m.generate_batch([full], row_base=1, **SAMPLED)[0])


# ---------------------------------------------------------------------------------------------------
# 8. close(drain=True) closes the open texts
# ---------------------------------------------------------------------------------------------------
def test_draining_close_ends_an_open_starved_ticket(models):
    """close(drain=True) frees the results nobody collected, so the ticket is judged by its events: its TOKENs are the ordinary
    request's first codes and its AUDIO is that request's audio."""
    m = models[True]
    N, F = 6, 12
    want = m.generate_batch([_whole(13, N, 40)], row_base=0, force_frames=F, **SAMPLED)[0]
    req, _ = _open(13, N, 40, first=N)
    log = Log()
    s = m.open_session(slots=2, on_event=log, force_frames=F, **SAMPLED)
    try:
        assert s.submit_open(req) == 0
        _starved(s, 1, events=1)
        s.close(drain=True)
    finally:
        s.close(drain=False)
    mine = log.of(0)
    assert [k for k, _ in mine] == ["token"] * F + ["info", "audio"]
    assert [p for k, p in mine if k == "token"] == want.codes[:, 0].tolist()
    assert np.array_equal(mine[-1][1], want.audio)


# ---------------------------------------------------------------------------------------------------
# 9. the resume launch forms the input the end of the frame forms
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [384, 2048, 2176], ids=["tiny-H", "H2048", "second-trip"])
def test_resume_input_equals_frame_end_input(models, H):
    """The same codes and text row through frame_end_job and through the append launch's resume (q3tts_debug_text_resume): equal in
    every bit, at the fixture's hidden size, at 2048 (every thread of the 256 x 8 loop busy) and past it (the loop's second trip)."""
    m = models[True]
    V = 64
    rng = np.random.Generator(np.random.PCG64(H))
    tables = (rng.standard_normal((16, V, H)).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    text = (rng.standard_normal(H).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    codes = rng.integers(0, V, size=16).astype(np.int32)
    h, ss, state = m.debug_text_resume(tables, codes, text)
    names = ["n_frames", "trailing_idx", "n_trailing", "finished", "active", "text_open", "starved", "cp_len"]
    st = [dict(zip(names, row.tolist())) for row in state]
    assert st[0] == dict(n_frames=1, trailing_idx=1, n_trailing=1, finished=0, active=1, text_open=0, starved=0, cp_len=0)
    # starved: the frame counts, no input is formed, the row is parked
    assert st[1] == dict(n_frames=1, trailing_idx=0, n_trailing=0, finished=1, active=0, text_open=1, starved=1, cp_len=0)
    assert (h[1] == 0xEEEE).all() and ss[1] == -1.0
    assert st[2] == dict(n_frames=1, trailing_idx=1, n_trailing=1, finished=0, active=1, text_open=1, starved=0, cp_len=0)
    assert np.array_equal(h[0], h[2]) and ss[0].tobytes() == ss[2].tobytes()
    # and it is the sum it should be: text + the 16 rows, left to right, every add rounded to bf16
    def f32(u):
        return (u.astype(np.uint32) << 16).view(np.float32)

    def rbf(x):
        b = x.astype(np.float32).view(np.uint32)
        return (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)

    acc = f32(tables[0, codes[0]])
    for g in range(1, 16):
        acc = rbf(acc + f32(tables[g, codes[g]]))
    assert np.array_equal(rbf(f32(text) + acc), f32(h[0]))
