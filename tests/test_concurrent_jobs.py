"""Two job contexts per model handle: a q3tts_generate_begin without an event callback leaves its frame loop to the context's
worker thread, so the AR loops of two outstanding jobs run side by side on streams of their own. Jobs are independent -- own
workspace, KV pool, random streams, job-owned copies of the codes -- so none of this may change a bit of any row."""
import json
import os
import subprocess
import sys
import threading

import pytest

from conftest import tiny_request

pytestmark = pytest.mark.gpu

LOAD = dict(max_batch=6, max_frames=64, max_prompt=96)


def _req(max_tokens=2048, **kw):
    from qwen3tts import GenerationRequest
    r = tiny_request(**kw)
    return GenerationRequest(r["text_ids"], r["target_token_count"], r["instruct_ids"], r["speaker"], r["language"], max_tokens)


def _same(got, want):
    assert len(got) == len(want)
    for x, y in zip(got, want):
        assert x.status == y.status
        assert x.codes.shape == y.codes.shape and (x.codes == y.codes).all()
        assert x.audio.shape == y.audio.shape and (x.audio == y.audio).all()


def _three_jobs(forced):
    """Different batch sizes, prompts, seeds and lengths per job; sampled (T = 0.9, top-k)."""
    cap = 2048 if forced else 40  # without force_frames a row ends at EOS or at its max_tokens
    batches = [[_req(row=i + 10 * k, n_text=5 + 2 * i + k, max_tokens=cap) for i in range(3 + k)] for k in range(3)]
    kws = [dict(temperature=0.9, top_k=40, repetition_penalty=1.05, seed=50 + k) for k in range(3)]
    if forced:
        for k in range(3):
            kws[k]["force_frames"] = 20 + 7 * k
    return batches, kws


def _interleaved(m, batches, kws, a_first):
    ja = m.generate_batch_begin(batches[0], **kws[0])
    jb = m.generate_batch_begin(batches[1], **kws[1])
    if a_first:
        ra = m.generate_batch_end(ja)
        jc = m.generate_batch_begin(batches[2], **kws[2])
        rb = m.generate_batch_end(jb)
    else:
        rb = m.generate_batch_end(jb)
        jc = m.generate_batch_begin(batches[2], **kws[2])
        ra = m.generate_batch_end(ja)
    rc = m.generate_batch_end(jc)
    return [ra, rb, rc]


@pytest.mark.parametrize("a_first", [True, False], ids=["end_a_first", "end_b_first"])
@pytest.mark.parametrize("forced", [True, False], ids=["force_frames", "eos"])
def test_background_jobs_equal_plain_calls_and_the_serial_switch(ckpt_dirs, monkeypatch, forced, a_first):
    """[begin A, begin B, end A, begin C, end B, end C] (and with the first two ends swapped), no callbacks: every row's codes
    and PCM bit-equal to three plain generate_batch calls, and to the same sequence with Q3TTS_SERIAL_JOBS=1 (every frame loop on
    the caller's thread)."""
    from qwen3tts import Qwen3TTSModel, _lib
    batches, kws = _three_jobs(forced)
    monkeypatch.delenv("Q3TTS_SERIAL_JOBS", raising=False)
    m = Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], **LOAD)
    try:
        want = [m.generate_batch(b, **kw) for b, kw in zip(batches, kws)]
        frames = [r.codes.shape[0] for res in want for r in res]
        print("frames per row:", frames)
        if not forced:
            assert len(set(frames)) > 2, frames  # rows really end at different frames
        got = _interleaved(m, batches, kws, a_first)
        for g, w in zip(got, want):
            _same(g, w)
        got = _interleaved(m, batches, kws, a_first)  # both contexts warm now: once more, in the steady state
        for g, w in zip(got, want):
            _same(g, w)
    finally:
        m.close()
    monkeypatch.setenv("Q3TTS_SERIAL_JOBS", "1")
    s = Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], **LOAD)
    try:
        for g, w in zip(_interleaved(s, batches, kws, a_first), want):
            _same(g, w)
    finally:
        s.close()
        monkeypatch.delenv("Q3TTS_SERIAL_JOBS", raising=False)
        _lib.reload_debug_env()  # the switch is process-wide and read at model load: leave the default behind


def test_a_job_with_a_callback_runs_beside_a_background_job(ckpt_dirs):
    """A job with on_event keeps its contract to the letter while a background job runs on the other context: TOKEN events
    inside begin, INFO / AUDIO inside end, all on the calling thread; both jobs' results as plain calls give them."""
    from qwen3tts import Qwen3TTSModel
    batches, kws = _three_jobs(True)
    m = Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], **LOAD)
    try:
        want = [m.generate_batch(b, **kw) for b, kw in zip(batches[:2], kws[:2])]
        me = threading.get_ident()
        events, threads, in_begin = [], set(), []
        phase = ["begin"]

        def on_event(i, kind, payload):
            events.append((i, kind))
            threads.add(threading.get_ident())
            in_begin.append((kind, phase[0]))

        ja = m.generate_batch_begin(batches[0], **dict(kws[0], force_frames=48))  # long: still running while B generates
        jb = m.generate_batch_begin(batches[1], on_event=on_event, **kws[1])
        phase[0] = "end"
        rb = m.generate_batch_end(jb)
        ra = m.generate_batch_end(ja)
        _same(rb, want[1])
        _same(ra, m.generate_batch(batches[0], **dict(kws[0], force_frames=48)))
        assert threads == {me}
        F = kws[1]["force_frames"]
        for i in range(len(batches[1])):
            assert [k for (r, k) in events if r == i] == ["token"] * F + ["info", "audio"]
        assert all(ph == ("begin" if kind == "token" else "end") for kind, ph in in_begin)
    finally:
        m.close()


def test_a_refused_begin_beside_a_background_job(ckpt_dirs):
    """Whatever can refuse a request refuses it inside begin, on the caller's thread: status 3 from begin itself while a
    background job runs; that job ends undisturbed and two further begins succeed."""
    from qwen3tts import Qwen3TTSError, Qwen3TTSModel
    m = Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], max_batch=4, max_frames=48, max_prompt=64)
    try:
        a = [_req(row=i, n_text=5 + i) for i in range(3)]
        b = [_req(row=7 + i, n_text=6 + i) for i in range(2)]
        kw = dict(temperature=0.9, top_k=40, seed=9, force_frames=40)
        want_a, want_b = m.generate_batch(a, **kw), m.generate_batch(b, **kw)
        ja = m.generate_batch_begin(a, **kw)
        bad_speaker = _req(row=1, n_text=5)
        bad_speaker.speaker = "nobody"
        too_long = _req(row=2, n_text=80)
        for bad in ([bad_speaker], [a[0], too_long]):
            with pytest.raises(Qwen3TTSError) as e:
                m.generate_batch_begin(bad, **kw)
            assert e.value.status == 3
        _same(m.generate_batch_end(ja), want_a)
        j1 = m.generate_batch_begin(b, **kw)
        j2 = m.generate_batch_begin(a, more_follows=False, **kw)
        with pytest.raises(Qwen3TTSError):  # two outstanding: a third is refused, and refusing it disturbs nothing
            m.generate_batch_begin(b, **kw)
        _same(m.generate_batch_end(j2), want_a)
        _same(m.generate_batch_end(j1), want_b)
    finally:
        m.close()


def test_a_row_that_fails_in_the_background_is_reported_by_end(tmp_path, ckpt_dirs):
    """A failure that only the frame loop can find -- a row whose first sampled token is EOS ("Generation failed: No tokens
    generated") -- happens on the worker thread and is reported by end: that row has status 2, the others are delivered, the
    slot is free again."""
    from qwen3tts import Qwen3TTSModel, synth
    kw = dict(temperature=0.9, top_k=50, seed=2)
    reqs = [_req(row=i, n_text=6 + i, max_tokens=12) for i in range(4)]
    plain = Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-a"], max_batch=4, max_frames=32, max_prompt=64)
    try:
        first = [int(r.codes[0, 0]) for r in plain.generate_batch(reqs, **kw)]
    finally:
        plain.close()
    victim = 1
    others = [i for i in range(4) if first[i] != first[victim]]
    assert others, first
    d = str(tmp_path / "eos_first")
    synth.write_checkpoint(d, "tiny-a", seed=1234)
    cfg_path = os.path.join(d, "config.json")
    cfg = json.load(open(cfg_path))
    cfg["talker_config"]["codec_eos_token_id"] = first[victim]
    json.dump(cfg, open(cfg_path, "w"))
    e = Qwen3TTSModel.from_pretrained(d, max_batch=4, max_frames=32, max_prompt=64)
    try:
        want = e.generate_batch(reqs, **kw)
        j1 = e.generate_batch_begin(reqs, **kw)
        j2 = e.generate_batch_begin(reqs[:2], **kw)
        r1 = e.generate_batch_end(j1)
        assert r1[victim].status == 2 and r1[victim].audio.size == 0 and r1[victim].codes.shape == (0, 16)
        assert b"Generation failed: No tokens generated" in e._lib.q3tts_last_error(e._h)
        for i in others:
            assert r1[i].status == 0 and int(r1[i].codes[0, 0]) == first[i]
        _same(r1, want)
        j3 = e.generate_batch_begin(reqs, **kw)  # the slot of the job that held a failed row is free again
        _same(e.generate_batch_end(j2), want[:2])
        _same(e.generate_batch_end(j3), want)
    finally:
        e.close()


def test_model_freed_with_two_background_jobs_outstanding():
    """q3tts_model_free while both contexts' worker threads are inside their frame loops: the workers finish before the streams
    go, and the next model of the process generates the same rows. In a child process: this path fails by crashing or hanging."""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "_free_background_worker.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-1000:] + r.stderr[-3000:]


def test_a_begin_without_a_callback_returns_before_the_frame_loop_has_run(ckpt_dirs, monkeypatch):
    """Results are equal on either path, so that the background path is TAKEN has to be seen in time: 190 forced frames are some
    hundred frame steps of host-paced work. With a warm context a begin without a callback returns after the prefill is queued
    (a small part of begin + end), while with Q3TTS_SERIAL_JOBS=1 the same begin holds the whole frame loop (most of it). The
    bounds are a quarter and a half: far from both (begin is ~1 % of the job in the background, > 90 % on the caller's thread)."""
    import time
    from qwen3tts import Qwen3TTSModel, _lib
    reqs = [_req(row=i, n_text=6 + i) for i in range(4)]
    kw = dict(temperature=0.9, top_k=40, seed=3, force_frames=190)
    share = {}
    for serial in (False, True):
        if serial:
            monkeypatch.setenv("Q3TTS_SERIAL_JOBS", "1")
        else:
            monkeypatch.delenv("Q3TTS_SERIAL_JOBS", raising=False)
        m = Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], max_batch=4, max_frames=200, max_prompt=64)
        try:
            for _ in range(2):  # both contexts warm: graphs captured, buffers grown
                m.generate_batch(reqs, **kw)
            t0 = time.perf_counter()
            j = m.generate_batch_begin(reqs, more_follows=False, **kw)
            t1 = time.perf_counter()
            m.generate_batch_end(j)
            t2 = time.perf_counter()
            share[serial] = (t1 - t0) / (t2 - t0)
        finally:
            m.close()
    monkeypatch.delenv("Q3TTS_SERIAL_JOBS", raising=False)
    _lib.reload_debug_env()
    print("begin's share of begin + end: background %.3f, serial %.3f" % (share[False], share[True]))
    assert share[False] < 0.25 and share[True] > 0.5, share


def test_a_back_half_that_throws_is_rethrown_by_end_and_frees_the_slot(ckpt_dirs, monkeypatch):
    """Every check that can refuse a request lies in begin's front half, so no request makes the back half throw; what is left
    there are runtime failures. Q3TTS_TEST_FAIL_BACK_HALF=1 makes a background back half throw on the host, before it launches
    anything: begin has already succeeded, the error comes out of end with its status and message, both slots are released (a
    third begin is refused while they are held, accepted afterwards), and the next model of the process is untouched."""
    from qwen3tts import Qwen3TTSError, Qwen3TTSModel, _lib
    reqs = [_req(row=i, n_text=6 + i) for i in range(3)]
    kw = dict(temperature=0.9, top_k=40, seed=4, force_frames=12)
    monkeypatch.setenv("Q3TTS_TEST_FAIL_BACK_HALF", "1")
    m = Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], max_batch=4, max_frames=32, max_prompt=64)
    try:
        j1 = m.generate_batch_begin(reqs, **kw)
        j2 = m.generate_batch_begin(reqs[:2], **kw)
        with pytest.raises(Qwen3TTSError) as e:
            m.generate_batch_begin(reqs, **kw)
        assert e.value.status == 3 and "outstanding" in str(e.value)
        for j in (j2, j1):
            with pytest.raises(Qwen3TTSError) as e:
                m.generate_batch_end(j)
            assert e.value.status == 7 and "Q3TTS_TEST_FAIL_BACK_HALF" in str(e.value)
        j3 = m.generate_batch_begin(reqs, **kw)  # both slots are free again
        j4 = m.generate_batch_begin(reqs, **kw)
        for j in (j3, j4):
            with pytest.raises(Qwen3TTSError):
                m.generate_batch_end(j)
        want = m.generate_batch(reqs, on_event=lambda i, k, p: None, **kw)  # a job with a callback never takes the worker
        assert all(r.status == 0 for r in want)
    finally:
        m.close()
        monkeypatch.delenv("Q3TTS_TEST_FAIL_BACK_HALF", raising=False)
        _lib.reload_debug_env()
    m = Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], max_batch=4, max_frames=32, max_prompt=64)
    try:
        j = m.generate_batch_begin(reqs, **kw)
        _same(m.generate_batch_end(j), want)
    finally:
        m.close()
