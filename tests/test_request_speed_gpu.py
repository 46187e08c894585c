"""Speaking rate per request (q3tts_request.speed on a handle loaded with request_speeds, include/q3tts.h "Speaking rate per
request"): a request at speed s gets, byte for byte, what a handle loaded with speed = s gives for that request alone at
row_base + i -- status, codes, n_frames, pcm, n_samples -- whatever the other rows speak at.

The reference of every comparison is the existing handle-speed path: one handle per reference speed is loaded, used and
freed in turn. Covered: the audio delivered whole and streamed (every AUDIO_CHUNK's offset, length and bytes) in the static
batch, begin / end, the queue with slots reused at other speeds, the session with an open-text ticket, voices with their
saved prefix states, an output rate, the fp32 re-decode, and the kernel's per-row path against the NumPy restatement of
tests/test_stretch_plan.py. Not built and refused (pinned here): a hop other than the handle's with the chunked exact decode
(audio_chunk_frames > 0 without a window) or with streamed audio on a handle that has an output rate."""
import dataclasses
import shutil

import numpy as np
import pytest

from conftest import tiny_request
from test_stretch_plan import choose_hs, delay, seeded_signal, stretch

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not shutil.which("g++"), reason="g++ is not installed")]

LOAD = dict(max_batch=4, max_frames=96, max_prompt=96)
C_, W_, L_ = 8, 32, 4
STREAM = dict(audio_chunk_frames=C_, audio_window_frames=W_, audio_lookahead_frames=L_)
KW = dict(temperature=0.9, top_k=40, seed=21)
CAPS = [5, 9, 12, 7]                       # ragged rows of the static batch
SPEEDS4 = [None, 0.8, 1.25, 2.0]
QSPEEDS = [2.0, 0.5, 0.5, 2.0, None, 1.25]  # 2 slots, equal lengths: slot 0 goes 2.0 -> 0.5 -> unset, slot 1 0.5 -> 2.0 -> 1.25
QF = 9


def _req(i, cap, speed=None):
    from qwen3tts import GenerationRequest
    return GenerationRequest(**tiny_request(row=i, n_text=6 + i), max_tokens=cap, speed=speed or 0.0)


def _keep(r):
    return (r.status, np.array(r.codes), np.array(r.audio))


def _alone(ckpt, speed, jobs, **load):
    """[(request, row_base, keywords)] each alone on a handle loaded with `speed` (None: the default handle), freed afterwards."""
    from qwen3tts import Qwen3TTSModel
    m = Qwen3TTSModel.from_pretrained(ckpt, speed=speed or 0.0, **{**LOAD, **load})
    try:
        return [_keep(m.generate_batch([dataclasses.replace(r, speed=0.0)], row_base=i, **kw)[0]) for r, i, kw in jobs]
    finally:
        m.close()


def _events():
    ev = []
    return ev, (lambda i, k, p: ev.append((i, k, p)))


def _chunks(ev, i):
    return [(int(p[0]), p[1].size, p[1].tobytes()) for j, k, p in ev if j == i and k == "audio_chunk"]


def _alone_streamed(ckpt, speed, jobs, **load):
    """_alone with every AUDIO_CHUNK: [((status, codes, audio), [(offset, length, bytes)])]."""
    from qwen3tts import Qwen3TTSModel
    m = Qwen3TTSModel.from_pretrained(ckpt, speed=speed or 0.0, **{**LOAD, **load})
    try:
        out = []
        for r, i, kw in jobs:
            ev, cb = _events()
            res = _keep(m.generate_batch([dataclasses.replace(r, speed=0.0)], row_base=i, on_event=cb, **kw)[0])
            out.append((res, _chunks(ev, 0)))
        return out
    finally:
        m.close()


def _same_streamed(got, ev, i, want, spf, what):
    """Result and every AUDIO_CHUNK (offset, length, bytes) as the reference's; offsets k * C * spf; the pieces are AUDIO."""
    _same(got, want[0], what)
    mine = _chunks(ev, i)
    assert mine == want[1], what
    assert [c[0] for c in mine] == [k * C_ * spf for k in range(len(mine))], what
    assert b"".join(c[2] for c in mine) == got.audio.tobytes(), what


def _same(got, want, what):
    assert got.status == want[0], what
    assert got.codes.shape == want[1].shape and np.array_equal(got.codes, want[1]), what
    assert got.audio.size == want[2].size and got.audio.tobytes() == want[2].tobytes(), what


@pytest.fixture(scope="module")
def mixed(ckpt_dirs):
    from qwen3tts import Qwen3TTSModel
    m = Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], request_speeds=True, **LOAD)
    yield m
    m.close()


@pytest.fixture(scope="module")
def static_refs(ckpt_dirs):
    """The static batch's requests, each alone on the handle of its speed."""
    reqs = [_req(i, c, s) for i, (c, s) in enumerate(zip(CAPS, SPEEDS4))]
    refs = [_alone(ckpt_dirs["tiny-b"], s, [(reqs[i], i, KW)])[0] for i, s in enumerate(SPEEDS4)]
    return reqs, refs


# ---- the interface ------------------------------------------------------------------------------------------------------
def test_info_and_request_speed_info(mixed):
    assert (mixed.info.samples_per_frame, mixed.info.max_samples_per_frame, mixed.stretch_hs) == (1920, 3840, 480)
    for s in (0.5, 0.8, 1.0, 1.25, 1.5, 2.0):
        hs = choose_hs(s)
        eff, h, d, spf = mixed.request_speed_info(s)
        assert (h, d, spf) == (hs, 0 if hs == 480 else delay(hs), 4 * hs) and abs(eff - 480.0 / hs) < 1e-6
    assert mixed.request_speed_info(0.0) == (1.0, 480, 0, 1920)


# ---- 1. static batch ----------------------------------------------------------------------------------------------------
def test_static_batch_of_mixed_speeds_equals_each_request_alone(mixed, static_refs):
    reqs, refs = static_refs
    frames = [r[1].shape[0] for r in refs]
    print("frames", frames)
    assert len(set(frames)) > 1 and all(f > 0 for f in frames)
    got = mixed.generate_batch(reqs, **KW)
    for i, s in enumerate(SPEEDS4):
        _same(got[i], refs[i], (i, s))
        spf = 4 * choose_hs(s) if s else 1920
        assert got[i].audio.size == int((got[i].codes[:, 0] > 0).sum()) * spf  # the end trim counts the request's own frames
    # the codes never depend on the speed
    plain = mixed.generate_batch([dataclasses.replace(r, speed=0.0) for r in reqs], **KW)
    for i in range(4):
        assert np.array_equal(plain[i].codes, got[i].codes)
    # the same batch through begin / end (with events: the frame loop inside begin; without: on the worker thread)
    for on_event in (None, lambda *a: None):
        job = mixed.generate_batch_begin(reqs, on_event=on_event, **KW)
        out = mixed.generate_batch_end(job)
        for i, s in enumerate(SPEEDS4):
            _same(out[i], refs[i], ("begin/end", i, s))


def test_row_groups_keep_the_rows_own_hops(mixed, static_refs):
    """A scratch budget so short that every row is a group of its own: the hop table is indexed by the row of the batch."""
    from qwen3tts import _lib
    reqs, refs = static_refs
    _lib.lib().q3tts_debug_set_codec_scratch(1 << 20)
    try:
        got = mixed.generate_batch(reqs, **KW)
    finally:
        _lib.lib().q3tts_debug_set_codec_scratch(0)
    for i, s in enumerate(SPEEDS4):
        _same(got[i], refs[i], (i, s))


# ---- 3. the queue: slots reused at other speeds ---------------------------------------------------------------------------
def test_queue_slots_reused_at_other_speeds(mixed, ckpt_dirs):
    reqs = [_req(i, 40, s) for i, s in enumerate(QSPEEDS)]
    kw = dict(force_frames=QF, **KW)
    want = {}
    for s in sorted(set(QSPEEDS), key=lambda v: v or 0):
        idx = [i for i, v in enumerate(QSPEEDS) if v == s]
        for i, r in zip(idx, _alone(ckpt_dirs["tiny-b"], s, [(reqs[i], i, kw) for i in idx])):
            want[i] = r
    got = mixed.generate_queued(reqs, slots=2, **kw)
    for i, s in enumerate(QSPEEDS):
        _same(got[i], want[i], (i, s))
        assert got[i].codes.shape[0] == QF
    # ragged lengths as well (requests retire at different boundaries; a decode batch holds whoever waits)
    caps = [9, 33, 20, 8, 17, 12]
    reqs = [_req(i, c, s) for i, (c, s) in enumerate(zip(caps, QSPEEDS))]
    got = mixed.generate_queued(reqs, slots=2, **KW)
    for s in sorted(set(QSPEEDS), key=lambda v: v or 0):
        idx = [i for i, v in enumerate(QSPEEDS) if v == s]
        for i, r in zip(idx, _alone(ckpt_dirs["tiny-b"], s, [(reqs[i], i, KW) for i in idx])):
            _same(got[i], r, ("ragged", i, s))


def test_queue_results_do_not_depend_on_the_lane_count(mixed, ckpt_dirs):
    """n_streams = 2: the closed queue's lanes each serve their own slots with their own codec runner (and its hop tables); the
    results are those of the one-lane handle, which the test above pins against each request alone."""
    from qwen3tts import Qwen3TTSModel
    caps = [9, 33, 20, 8, 17, 12]
    reqs = [_req(i, c, s) for i, (c, s) in enumerate(zip(caps, QSPEEDS))]
    want = [_keep(r) for r in mixed.generate_queued(reqs, slots=2, **KW)]
    m = Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], request_speeds=True, n_streams=2, **LOAD)
    try:
        got = m.generate_queued(reqs, slots=4, **KW)
        for i, s in enumerate(QSPEEDS):
            _same(got[i], want[i], ("lanes", i, s))
    finally:
        m.close()


# ---- 4. the session ---------------------------------------------------------------------------------------------------
def test_session_tickets_at_their_own_speeds(mixed, ckpt_dirs):
    from qwen3tts import GenerationRequest
    F, N = 14, 12
    kw = dict(force_frames=F, **KW)
    speeds = [1.25, None, 2.0]
    plain = [_req(i, 40, s) for i, s in enumerate(speeds)]
    ids = list(tiny_request(row=7, n_text=N)["text_ids"])
    role, content, tail = ids[:3], ids[3:3 + N], ids[3 + N:]
    whole = GenerationRequest(role + content + tail, N, None, "aiden", "english", 40)
    opened = GenerationRequest(role + content[:3], 0, None, "aiden", "english", 40, speed=0.8)
    want = {t: _alone(ckpt_dirs["tiny-b"], s, [(plain[t], t, kw)])[0] for t, s in enumerate(speeds)}
    want[3] = _alone(ckpt_dirs["tiny-b"], 0.8, [(whole, 3, kw)])[0]
    s = mixed.open_session(slots=2, **kw)
    try:
        assert [s.submit(plain[0]), s.submit(plain[1])] == [0, 1]
        assert s.submit(plain[2]) == 2  # while rows run
        assert s.submit_open(opened) == 3
        assert mixed.request_speed_info(0.8)[1] == 600  # host-only: available while the session is open
        s.append_text(3, content[3:5])
        s.append_text(3, content[5:9])
        s.append_text(3, content[9:], final=True)
        for t in range(4):
            _same(s.result(t, timeout=60), want[t], ("ticket", t))
    finally:
        s.close()


# ---- 5. voices (a Base checkpoint) ----------------------------------------------------------------------------------------
def test_voice_requests_at_their_own_speeds(tmp_path):
    from qwen3tts import GenerationRequest, Qwen3TTSModel, synth
    d = str(tmp_path / "tiny-base")
    synth.write_checkpoint(d, "tiny-base", seed=4321)
    load = dict(max_batch=4, max_frames=64, max_prompt=160)
    clip = synth.synthetic_reference_audio(1, 1.0)
    ref_ids = synth.synthetic_prompt(1, n_text=10, text_vocab=1000, im_start=1000, im_end=1001)["ref_text_ids"]
    prompts = [synth.synthetic_prompt(2 + i, n_text=9, text_vocab=1000, im_start=1000, im_end=1001) for i in range(3)]
    kw = dict(temperature=0.9, top_k=40, repetition_penalty=1.5, seed=77)
    speeds = [0.8, None, 1.25]

    def reqs_for(v):
        return [GenerationRequest(p["text_ids"], p["target_token_count"], None, None, "english", 10, voice=v, speed=s or 0.0)
                for p, s in zip(prompts, speeds)]

    want = []
    for i, s in enumerate(speeds):
        m = Qwen3TTSModel.from_pretrained(d, speed=s or 0.0, **load)
        try:
            with m.create_voice(clip, ref_ids) as v:
                r = dataclasses.replace(reqs_for(v)[i], speed=0.0)
                want.append((_keep(m.generate_batch([r], row_base=i, **kw)[0])))
        finally:
            m.close()
    m = Qwen3TTSModel.from_pretrained(d, request_speeds=True, **load)
    try:
        with m.create_voice(clip, ref_ids) as v:
            reqs = reqs_for(v)
            got = m.generate_batch(reqs, **kw)
            queued = m.generate_queued(reqs, slots=2, **kw)
            for i, s in enumerate(speeds):
                assert want[i][0] == 0 and want[i][1].shape[0] > 0
                _same(got[i], want[i], ("voices", i, s))
                _same(queued[i], want[i], ("queued voices", i, s))
    finally:
        m.close()


# ---- 6. an output rate ------------------------------------------------------------------------------------------------------
def test_request_speeds_at_16_khz(ckpt_dirs):
    """The admissible hops are multiples of 3 at 16 kHz: 1.25 -> 384, 0.8 -> 600; a row's frame in front of the resampler is
    its own 4 Hs samples and the resampler starts every frame at phase 0."""
    from qwen3tts import Qwen3TTSModel
    speeds = [1.25, 0.8, None]
    reqs = [_req(i, c, s) for i, (c, s) in enumerate(zip([11, 6, 9], speeds))]
    want = [_alone(ckpt_dirs["tiny-b"], s, [(reqs[i], i, KW)], output_sample_rate=16000)[0] for i, s in enumerate(speeds)]
    m = Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], request_speeds=True, output_sample_rate=16000, **LOAD)
    try:
        assert (m.info.sample_rate, m.info.samples_per_frame, m.info.max_samples_per_frame) == (16000, 1280, 2560)
        for s, hs in ((1.25, 384), (0.8, 600)):
            assert choose_hs(s, 4, 2, 3) == hs and m.request_speed_info(s)[1:] == (hs, delay(hs), 4 * hs * 2 // 3)
        got = m.generate_batch(reqs, **KW)
        for i, s in enumerate(speeds):
            _same(got[i], want[i], ("16 kHz", i, s))
            spf = m.request_speed_info(s or 0.0)[3]
            assert got[i].audio.size == int((got[i].codes[:, 0] > 0).sum()) * spf
    finally:
        m.close()


# ---- 7. nothing changed -----------------------------------------------------------------------------------------------------
def test_no_request_speed_is_the_default_handle(mixed, ckpt_dirs):
    from qwen3tts import Qwen3TTSModel
    reqs = [_req(i, c) for i, c in enumerate(CAPS)]
    ev_a, ev_m = [], []
    A = Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], **LOAD)
    try:
        assert A.info.max_samples_per_frame == A.info.samples_per_frame == 1920
        want = [_keep(r) for r in A.generate_batch(reqs, **KW)]
        want_st = [_keep(r) for r in A.generate_batch(reqs, on_event=lambda i, k, p: ev_a.append((i, k, p)), **KW, **STREAM)]
    finally:
        A.close()
    got = mixed.generate_batch(reqs, **KW)
    got_st = mixed.generate_batch(reqs, on_event=lambda i, k, p: ev_m.append((i, k, p)), **KW, **STREAM)
    for i in range(4):
        _same(got[i], want[i], i)
        _same(got_st[i], want_st[i], ("streamed", i))
    chunks = lambda ev: [(i, p[0], p[1].tobytes()) for i, k, p in ev if k == "audio_chunk"]
    assert chunks(ev_a) == chunks(ev_m) and len(chunks(ev_m)) >= 4


def test_a_handle_with_its_own_speed_and_request_speeds(ckpt_dirs):
    """speed = 1.25 and request_speeds: an unset request speaks at 1.25, a request at 1.0 gets the plain decode, a request at
    1.25 is the handle's own path (streamed audio included)."""
    from qwen3tts import Qwen3TTSModel
    reqs = [_req(0, 9), _req(1, 7, 1.0), _req(2, 11, 1.25), _req(3, 6, 0.5)]
    want = [_alone(ckpt_dirs["tiny-b"], s, [(reqs[i], i, KW)])[0] for i, s in enumerate([1.25, None, 1.25, 0.5])]
    want_st = _alone(ckpt_dirs["tiny-b"], 1.25, [(reqs[2], 2, dict(**KW, **STREAM))])[0]
    m = Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], speed=1.25, request_speeds=True, **LOAD)
    try:
        assert (m.info.samples_per_frame, m.info.max_samples_per_frame, m.stretch_hs) == (1536, 3840, 384)
        assert m.request_speed_info(0.0)[1:] == (384, delay(384), 1536) and m.request_speed_info(1.0)[1:] == (480, 0, 1920)
        got = m.generate_batch(reqs, **KW)
        for i in range(4):
            _same(got[i], want[i], i)
        _same(m.generate_batch([reqs[2]], row_base=2, **KW, **STREAM)[0], want_st, "the handle's own hop, streamed")
    finally:
        m.close()


# ---- 8. the kernel's per-row path -----------------------------------------------------------------------------------------------
def test_stretch_kernel_with_a_hop_per_row_equals_the_definition(mixed, ckpt_dirs):
    from qwen3tts import Qwen3TTSModel
    hops, lens = [240, 437, 480, 960], [0, 480, 1921, 4097]
    x = np.stack([seeded_signal(max(lens), 300 + b) for b in range(4)])
    fill = np.float32(7.0)
    y0 = np.full((4, 8 * 960 + 5), fill, np.float32)
    A = Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], **LOAD)  # (the hook works on any handle)
    try:
        outs = [mixed.debug_stretch_rows(x, lens, hops, y0), A.debug_stretch_rows(x, lens, hops, y0)]
    finally:
        A.close()
    for y in outs:
        assert np.array_equal(y[0], y0[0])  # a row of length 0 touches nothing
        for b in range(1, 4):
            want, _, _ = stretch(x[b, :lens[b]], hops[b], True)
            n = (lens[b] // 480) * hops[b]
            assert want.size == n > 0
            assert np.array_equal(y[b, :n].view(np.uint32), want.view(np.uint32)), (b, hops[b])
            assert (y[b, n:] == fill).all(), b  # nothing behind the row's last hop
    # hop 0: the row is copied (a request at speed 1 beside stretched rows)
    y = mixed.debug_stretch_rows(x, [481, 0, 4097, 960], [0, 0, 0, 600], y0)
    assert np.array_equal(y[0, :481], x[0, :481]) and (y[0, 481:] == fill).all() and np.array_equal(y[1], y0[1])
    assert np.array_equal(y[2, :4097], x[2, :4097]) and (y[2, 4097:] == fill).all()
    assert np.array_equal(y[3, :1200].view(np.uint32), stretch(x[3, :960], 600, True)[0].view(np.uint32))


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(mixed, ckpt_dirs, static_refs):
    from qwen3tts import Qwen3TTSModel
    from qwen3tts.model import Qwen3TTSError
    reqs, refs = static_refs

    def refused(fn, word):
        with pytest.raises(Qwen3TTSError) as e:
            fn()
        assert e.value.status == 3 and word in str(e.value), str(e.value)

    def good(m=mixed):
        _same(m.generate_batch([reqs[2]], row_base=2, **KW)[0], refs[2], "after a refusal")

    for bad in (float("nan"), float("inf"), float("-inf"), 0.4999, 2.0001, -1.0):
        r = dataclasses.replace(reqs[1], speed=bad)
        refused(lambda: mixed.generate_batch([reqs[0], r], **KW), "between 0.5 and 2.0")
        good()
        refused(lambda: mixed.generate_queued([reqs[0], r], slots=2, **KW), "between 0.5 and 2.0")
        refused(lambda: mixed.request_speed_info(bad), "between 0.5 and 2.0")
    good()
    refused(lambda: mixed.generate_batch_begin([dataclasses.replace(reqs[1], speed=3.0)], **KW), "between 0.5 and 2.0")
    good()
    # not built: another hop than the handle's with the chunked exact decode, or streamed on a handle with an output rate
    refused(lambda: mixed.generate_batch([reqs[1]], audio_chunk_frames=8, **KW), "audio_window_frames")
    good()
    R = Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], request_speeds=True, output_sample_rate=16000, **LOAD)
    try:
        refused(lambda: R.generate_batch([reqs[1]], **KW, **STREAM), "output_sample_rate")
        refused(lambda: R.generate_queued([reqs[1]], slots=1, **KW, **STREAM), "output_sample_rate")
        assert R.generate_batch([reqs[1]], **KW)[0].status == 0
    finally:
        R.close()
    s = mixed.open_session(slots=2, **KW)
    try:
        refused(lambda: s.submit(dataclasses.replace(reqs[1], speed=float("nan"))), "between 0.5 and 2.0")
        refused(lambda: s.submit_open(dataclasses.replace(reqs[1], text_ids=list(reqs[1].text_ids)[:5], speed=9.0)), "between 0.5 and 2.0")
        assert s.submit(reqs[2]) == 0  # no refusal took a ticket; the session is usable
        got = s.result(0, timeout=60)
        assert got.status == 0 and got.codes.shape[0] > 0 and got.audio.size % (4 * 384) == 0  # (reqs[2] speaks at 1.25)
    finally:
        s.close()
    good()
    # a handle without request_speeds refuses every request speed and stays usable
    A = Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], **LOAD)
    try:
        refused(lambda: A.generate_batch([reqs[2]], **KW), "request_speeds")
        refused(lambda: A.generate_queued([reqs[2]], slots=1, **KW), "request_speeds")
        refused(lambda: A.request_speed_info(1.25), "request_speeds")
        assert A.request_speed_info(0.0) == (1.0, 480, 0, 1920)
        plain = A.generate_batch([dataclasses.replace(reqs[2], speed=0.0)], row_base=2, **KW)[0]
        assert plain.status == 0 and np.array_equal(plain.codes, refs[2][1])
    finally:
        A.close()


# ---- 2. streamed batch ----------------------------------------------------------------------------------------------------
F_ST = 21  # (the streamed cases of tests/test_stretch_gpu.py: force_frames 21, chunk 8, window 32, lookahead 4)


def test_streamed_static_batch_of_mixed_speeds(mixed, ckpt_dirs):
    caps = [37, 5, 22, 13]
    reqs = [_req(i, c, s) for i, (c, s) in enumerate(zip(caps, SPEEDS4))]
    kw = dict(**KW, **STREAM)
    want = [_alone_streamed(ckpt_dirs["tiny-b"], s, [(reqs[i], i, kw)])[0] for i, s in enumerate(SPEEDS4)]
    ev, cb = _events()
    got = mixed.generate_batch(reqs, on_event=cb, **kw)
    print("frames", [g.codes.shape[0] for g in got])
    assert max(g.codes.shape[0] for g in got) > 2 * C_
    for i, s in enumerate(SPEEDS4):
        _same_streamed(got[i], ev, i, want[i], mixed.request_speed_info(s or 0.0)[3], (i, s))


# ---- 3. slot reuse, streamed --------------------------------------------------------------------------------------------------
def test_streamed_queue_slots_reused_at_other_speeds(mixed, ckpt_dirs):
    """2 slots, 6 requests of equal length: slot 0 goes 2.0 -> 0.5 -> unset and its neighbour 0.5 -> 2.0 -> 1.25 -- the smallest
    shape at which a margin, a state word or a frame size left by the previous occupant shows."""
    reqs = [_req(i, 40, s) for i, s in enumerate(QSPEEDS)]
    kw = dict(force_frames=F_ST, **KW, **STREAM)
    want = {}
    for s in sorted(set(QSPEEDS), key=lambda v: v or 0):
        idx = [i for i, v in enumerate(QSPEEDS) if v == s]
        for i, r in zip(idx, _alone_streamed(ckpt_dirs["tiny-b"], s, [(reqs[i], i, kw) for i in idx])):
            want[i] = r
    ev, cb = _events()
    got = mixed.generate_queued(reqs, slots=2, on_event=cb, **kw)
    for i, s in enumerate(QSPEEDS):
        assert got[i].codes.shape[0] == F_ST
        _same_streamed(got[i], ev, i, want[i], mixed.request_speed_info(s or 0.0)[3], (i, s))
    # ragged lengths: rows retire and are refilled at different boundaries
    caps = [9, 33, 20, 8, 17, 12]
    reqs = [_req(i, c, s) for i, (c, s) in enumerate(zip(caps, QSPEEDS))]
    kw = dict(**KW, **STREAM)
    ev, cb = _events()
    got = mixed.generate_queued(reqs, slots=2, on_event=cb, **kw)
    for s in sorted(set(QSPEEDS), key=lambda v: v or 0):
        idx = [i for i, v in enumerate(QSPEEDS) if v == s]
        for i, r in zip(idx, _alone_streamed(ckpt_dirs["tiny-b"], s, [(reqs[i], i, kw) for i in idx])):
            _same_streamed(got[i], ev, i, r, mixed.request_speed_info(s or 0.0)[3], ("ragged", i, s))


# ---- 4. the session, streamed ---------------------------------------------------------------------------------------------------
def test_streamed_session_tickets_at_their_own_speeds(mixed, ckpt_dirs):
    from qwen3tts import GenerationRequest
    N = 12
    kw = dict(force_frames=F_ST, **KW, **STREAM)
    speeds = [1.25, None, 2.0]
    plain = [_req(i, 40, s) for i, s in enumerate(speeds)]
    ids = list(tiny_request(row=7, n_text=N)["text_ids"])
    role, content, tail = ids[:3], ids[3:3 + N], ids[3 + N:]
    whole = GenerationRequest(role + content + tail, N, None, "aiden", "english", 40)
    opened = GenerationRequest(role + content[:3], 0, None, "aiden", "english", 40, speed=0.8)
    want = {t: _alone_streamed(ckpt_dirs["tiny-b"], s, [(plain[t], t, kw)])[0] for t, s in enumerate(speeds)}
    want[3] = _alone_streamed(ckpt_dirs["tiny-b"], 0.8, [(whole, 3, kw)])[0]
    ev, cb = _events()
    s = mixed.open_session(slots=2, on_event=cb, **kw)
    try:
        assert [s.submit(plain[0]), s.submit(plain[1])] == [0, 1]
        assert s.submit(plain[2]) == 2  # while rows run
        assert s.submit_open(opened) == 3
        s.append_text(3, content[3:5])
        s.append_text(3, content[5:9])
        s.append_text(3, content[9:], final=True)
        got = [s.result(t, timeout=60) for t in range(4)]
    finally:
        s.close()
    for t, sp in enumerate(speeds + [0.8]):
        _same_streamed(got[t], ev, t, want[t], mixed.request_speed_info(sp or 0.0)[3], ("ticket", t))


# ---- 5. voices, streamed behind their reference: the saved prefix state is keyed by the hop --------------------------------------
def test_streamed_voice_requests_and_their_prefix_states(tmp_path):
    from qwen3tts import GenerationRequest, Qwen3TTSModel, synth
    d = str(tmp_path / "tiny-base")
    synth.write_checkpoint(d, "tiny-base", seed=4321)
    load = dict(max_batch=4, max_frames=64, max_prompt=160)
    clip = synth.synthetic_reference_audio(1, 1.0)
    ref_ids = synth.synthetic_prompt(1, n_text=10, text_vocab=1000, im_start=1000, im_end=1001)["ref_text_ids"]
    prompts = [synth.synthetic_prompt(2 + i, n_text=9, text_vocab=1000, im_start=1000, im_end=1001) for i in range(3)]
    kw = dict(audio_stream_reference=1, temperature=0.9, top_k=40, repetition_penalty=1.5, seed=77, **STREAM)
    speeds = [1.25, None, 1.25]

    def reqs_for(v):
        return [GenerationRequest(p["text_ids"], p["target_token_count"], None, None, "english", 10, voice=v, speed=s or 0.0)
                for p, s in zip(prompts, speeds)]

    want = {}
    for s in (1.25, None):
        m = Qwen3TTSModel.from_pretrained(d, speed=s or 0.0, **load)
        try:
            with m.create_voice(clip, ref_ids) as v:
                for i, r in enumerate(reqs_for(v)):
                    if speeds[i] != s:
                        continue
                    ev, cb = _events()
                    res = _keep(m.generate_batch([dataclasses.replace(r, speed=0.0)], row_base=i, on_event=cb, **kw)[0])
                    want[i] = (res, _chunks(ev, 0))
        finally:
            m.close()
    m = Qwen3TTSModel.from_pretrained(d, request_speeds=True, **load)
    try:
        with m.create_voice(clip, ref_ids) as v:
            reqs = reqs_for(v)
            n0, _, r0 = m.debug_prefix_states()
            ev, cb = _events()
            got = m.generate_queued(reqs, slots=1, on_event=cb, **kw)  # one slot: the requests follow each other
            n1, _, r1 = m.debug_prefix_states()
            # a state per hop (1.25's and the handle's); the third request, at 1.25 again, is served from the first one's state
            assert (n1 - n0, r1 - r0) == (2, 1)
            for i, s in enumerate(speeds):
                assert want[i][0][0] == 0 and want[i][0][1].shape[0] > 0
                _same_streamed(got[i], ev, i, want[i], m.request_speed_info(s or 0.0)[3], ("voices", i, s))
            # the static batch with the references in front, and every state now restored
            ev, cb = _events()
            got = m.generate_batch(reqs, on_event=cb, **kw)
            for i, s in enumerate(speeds):
                _same_streamed(got[i], ev, i, want[i], m.request_speed_info(s or 0.0)[3], ("static voices", i, s))
            ev, cb = _events()
            got = m.generate_queued(reqs, slots=2, on_event=cb, **kw)
            n2, _, r2 = m.debug_prefix_states()
            assert (n2, r2 - r1) == (n1, 3)
            for i, s in enumerate(speeds):
                _same_streamed(got[i], ev, i, want[i], m.request_speed_info(s or 0.0)[3], ("restored", i, s))
    finally:
        m.close()


# ---- the fp32 re-decode of a row that left the fp16 range runs at the request's own speed -----------------------------------------
def test_fp32_redecode_at_the_requests_own_speed(tmp_path):
    """tests/test_codec_range.py's checkpoint: every row leaves the fp16 range and is decoded again on the fp32 matrix cores.
    The re-decode batch is indexed by its own rows, the hops by the job's: each request must come back at its own hop, whole
    and from the streamed queue's held requests."""
    from test_codec_range import _big_bias_checkpoint
    from qwen3tts import Qwen3TTSModel
    d = _big_bias_checkpoint(tmp_path)
    load = dict(max_batch=4, max_frames=32, max_prompt=64)
    speeds = [2.0, None, 0.8]
    reqs = [_req(i, c, s) for i, (c, s) in enumerate(zip([20, 6, 13], speeds))]
    kw_st = dict(**KW, **STREAM)
    want, want_st = [], []
    for i, s in enumerate(speeds):
        want.append(_alone(d, s, [(reqs[i], i, KW)], **load)[0])
        want_st.append(_alone_streamed(d, s, [(reqs[i], i, kw_st)], **load)[0])
    m = Qwen3TTSModel.from_pretrained(d, request_speeds=True, **load)
    try:
        got = m.generate_batch(reqs, **KW)
        ev, cb = _events()
        got_st = m.generate_queued(reqs, slots=2, on_event=cb, **kw_st)
        assert any(w[0] == 0 and w[1].shape[0] > 0 for w in want)
        for i, s in enumerate(speeds):
            _same(got[i], want[i], ("whole", i, s))
            assert got[i].status != 0 or np.isfinite(got[i].audio).all()
            _same_streamed(got_st[i], ev, i, want_st[i], m.request_speed_info(s or 0.0)[3], ("streamed", i, s))
    finally:
        m.close()
