"""Continuous batching (q3tts_generate_queued): a slot whose row finishes takes the next queued request. Request i must come
out bit-identical to q3tts_generate of that request alone with row_base = i, whatever slot, lane or admission served it; slots
are refilled (fewer frame steps than static batches); INFO / AUDIO leave as soon as a request is decoded; bad calls are
refused before any GPU work and leave the engine usable."""
import json
import os

import numpy as np
import pytest

from conftest import tiny_request

pytestmark = pytest.mark.gpu

BURST = 9  # frame steps per burst of a one-lane engine (engine_queue.cc: max_inflight_frames / 2); EOS is seen at a burst boundary


def _req(row, n_text, max_tokens, speaker="aiden", language="english", n_instruct=0):
    from qwen3tts import GenerationRequest
    r = tiny_request(row=row, n_text=n_text, n_instruct=n_instruct, speaker=speaker, language=language)
    return GenerationRequest(r["text_ids"], r["target_token_count"], r["instruct_ids"], r["speaker"], r["language"], max_tokens)


def _mixed():
    """10 requests: prompt lengths, speakers, languages, instruct and max_tokens (5..40) all vary."""
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


SAMPLINGS = [dict(temperature=0.0, repetition_penalty=1.0), dict(temperature=0.9, top_k=40, repetition_penalty=1.05, seed=77)]


@pytest.fixture(scope="module")
def models(ckpt_dirs):
    from qwen3tts import Qwen3TTSModel
    out = {g: Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], max_batch=4, max_frames=64, max_prompt=96, use_graph=g)
           for g in (True, False)}
    yield out
    for m in out.values():
        m.close()


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("kw", SAMPLINGS, ids=["greedy", "sampled"])
def test_queued_equals_each_request_alone(models, graph, kw):
    m = models[graph]
    reqs = _mixed()
    got = m.generate_queued(reqs, slots=3, **kw)
    assert len(got) == len(reqs) and m.last_timing().rows == len(reqs)
    for i, r in enumerate(reqs):
        _same(got[i], m.generate_batch([r], row_base=i, **kw)[0])
    # static batches carrying the same row bases draw the same streams
    for lo in range(0, len(reqs), 3):
        for j, w in enumerate(m.generate_batch(reqs[lo:lo + 3], row_base=lo, **kw)):
            _same(got[lo + j], w)
    # a sampling row_base shifts every request's stream by the same amount
    shifted = m.generate_queued(reqs[:4], slots=2, row_base=100, **kw)
    for i in range(4):
        _same(shifted[i], m.generate_batch([reqs[i]], row_base=100 + i, **kw)[0])


def test_lanes_change_nothing(ckpt_dirs, models):
    from qwen3tts import Qwen3TTSModel
    reqs = _mixed()
    kw = SAMPLINGS[1]
    one = models[True].generate_queued(reqs, slots=4, **kw)
    two = Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], max_batch=4, max_frames=64, max_prompt=96, n_streams=2)
    try:
        got = two.generate_queued(reqs, slots=4, **kw)
    finally:
        two.close()
    for a, b in zip(got, one):
        _same(a, b)


def _makespans(frames, slots):
    """In-order makespan with `slots` rows refilled at once, and static batches of `slots` rows in order."""
    free = [0] * slots
    for f in frames:
        k = int(np.argmin(free))
        free[k] += f
    m_q = max(free)
    m_s = sum(max(frames[i:i + slots]) for i in range(0, len(frames), slots))
    return m_q, m_s


def test_slots_are_refilled_and_audio_leaves_early(models):
    """One long request (60 frames) and nine short ones (6): two slots serve the shorts one after another beside the long one,
    so the call takes about the long request's frames instead of the pairwise sum. A short request's AUDIO arrives before the
    long request's last TOKEN: rows are decoded and delivered while the frame loop goes on."""
    m = models[True]
    reqs = [_req(row=0, n_text=9, max_tokens=60)] + [_req(row=1 + i, n_text=5 + i, max_tokens=6) for i in range(9)]
    # a seed under which the long request really is long (the tiny checkpoint draws EOS now and then)
    seed = next(s for s in range(5, 50) if m.generate_batch(reqs[:1], temperature=0.9, top_k=50, seed=s)[0].codes.shape[0] >= 40)
    events = []
    res = m.generate_queued(reqs, slots=2, temperature=0.9, top_k=50, seed=seed, on_event=lambda i, k, p: events.append((i, k)))
    frames = [r.codes.shape[0] for r in res]
    caps = [60] + [6] * 9
    m_q, m_s = _makespans(frames, 2)
    assert m_q < m_s, (frames, m_q, m_s)
    eos_rows = sum(1 for f, c in zip(frames, caps) if f < c)  # each may hold its slot up to one burst past its end
    steps = m.last_timing().frame_steps
    assert steps <= m_q + BURST * eos_rows, (steps, m_q, eos_rows, frames)
    assert steps < m_s, (steps, m_s)
    for i, r in enumerate(res):
        kinds = [k for (j, k) in events if j == i]
        if frames[i] == 0:  # first token EOS (the tiny checkpoint draws it now and then): fails alone, reports nothing
            assert r.status == 2 and kinds == []
            continue
        assert r.status == 0
        assert kinds == ["token"] * frames[i] + ["info", "audio"], (i, kinds)
    order = [(j, k) for (j, k) in events]
    last_long_token = max(n for n, (j, k) in enumerate(order) if j == 0 and k == "token")
    first_short_audio = min(n for n, (j, k) in enumerate(order) if j > 0 and k == "audio")
    assert first_short_audio < last_long_token


def test_edges_refusals_leave_the_engine_usable(models):
    from qwen3tts import GenerationRequest, Qwen3TTSError, synth
    m = models[True]
    kw = SAMPLINGS[1]
    reqs = [_req(row=i, n_text=6 + i, max_tokens=8 + 3 * i) for i in range(3)]
    want = [m.generate_batch([r], row_base=i, **kw)[0] for i, r in enumerate(reqs)]
    for i, g in enumerate(m.generate_queued(reqs, slots=1, **kw)):       # one slot: strictly one request after another
        _same(g, want[i])
    for i, g in enumerate(m.generate_queued(reqs[:2], slots=4, **kw)):   # more slots than requests: the rest stay empty
        _same(g, want[i])

    p = synth.synthetic_prompt(0, n_text=10, text_vocab=1000, im_start=1000, im_end=1001)
    clone = GenerationRequest(p["text_ids"], p["target_token_count"], None, None, "english",
                              ref_audio=synth.synthetic_reference_audio(0, 0.5), ref_text_ids=p["ref_text_ids"])
    job = m.generate_batch_begin(reqs[:1], **kw)
    try:
        with pytest.raises(Qwen3TTSError) as e:
            m.generate_queued(reqs, slots=2, **kw)
        assert e.value.status == 3 and "outstanding" in str(e.value)
    finally:
        _same(m.generate_batch_end(job)[0], want[0])
    bad = [(dict(slots=5), "slots"), (dict(slots=0), "slots"), (dict(slots=2, audio_chunk_frames=4), "audio_chunk_frames")]
    for extra, word in bad:
        with pytest.raises(Qwen3TTSError) as e:
            m.generate_queued(reqs, **{**kw, **extra})
        assert e.value.status == 3 and word in str(e.value)
    with pytest.raises(Qwen3TTSError) as e:
        m.generate_queued(reqs + [clone], slots=2, **kw)
    assert e.value.status == 3 and "voice-clone" in str(e.value)
    # a bad request at the LAST index is refused before anything runs: no TOKEN event at all
    seen = []
    for last in (_req(row=9, n_text=6, max_tokens=65), _req(row=9, n_text=6, max_tokens=8, speaker="nobody")):
        with pytest.raises(Qwen3TTSError) as e:
            m.generate_queued(reqs * 3 + [last], slots=2, on_event=lambda i, k, p: seen.append(k), **kw)
        assert e.value.status == 3 and "request 9" in str(e.value)
    assert seen == []
    for i, g in enumerate(m.generate_queued(reqs, slots=2, **kw)):
        _same(g, want[i])


def test_a_request_whose_first_token_is_eos_fails_alone(tmp_path, ckpt_dirs):
    from qwen3tts import Qwen3TTSModel, synth
    kw = dict(temperature=0.9, top_k=50, seed=2)
    reqs = [_req(row=i, n_text=6 + i, max_tokens=12) for i in range(4)]
    plain = Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-a"], max_batch=4, max_frames=32, max_prompt=64)
    try:
        first = [int(r.codes[0, 0]) for r in plain.generate_queued(reqs, slots=2, **kw)]
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
        kinds = {i: [] for i in range(4)}
        res = e.generate_queued(reqs, slots=2, on_event=lambda i, k, p: kinds[i].append(k), **kw)
        assert res[victim].status == 2 and res[victim].audio.size == 0 and res[victim].codes.shape == (0, 16)
        assert kinds[victim] == []
        for i in others:
            assert res[i].status == 0 and res[i].codes.shape[0] >= 1 and int(res[i].codes[0, 0]) == first[i]
            assert kinds[i][-2:] == ["info", "audio"]
            _same(res[i], e.generate_batch([reqs[i]], row_base=i, **kw)[0])
        assert b"Generation failed: No tokens generated" in e._lib.q3tts_last_error(e._h)
    finally:
        e.close()
