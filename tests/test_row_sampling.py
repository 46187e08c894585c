"""Per-request sampling parameters (q3tts_sampling.per_request): whatever entry point serves it -- a static batch, the queue
(any slot, lane, streamed or not), a background job, the teacher-forced hook -- request i comes out bit-identical to
q3tts_generate of it alone under the call's values with its own overrides folded in and row_base + i. An array that sets
nothing is the same as none; bad entries are refused before any GPU work and leave the engine usable."""
import ctypes as C

import numpy as np
import pytest

from conftest import tiny_request

pytestmark = pytest.mark.gpu

P = [dict(temperature=0.0, repetition_penalty=1.0),                          # P0 greedy
     dict(temperature=0.9, top_k=40, repetition_penalty=1.05, seed=77),      # P1 sampled
     dict(temperature=0.7, top_k=5, top_p=0.6, repetition_penalty=1.3),      # P2 top-k + top-p
     dict(temperature=1.0, top_k=0, top_p=0.8, seed=5)]                      # P3 top-p over the whole vocabulary
STREAM = dict(audio_chunk_frames=8, audio_window_frames=32, audio_lookahead_frames=4)
# the queue's assignment: the first three admissions (one per slot) are sampled, the next three greedy -- request 3 takes a
# slot that a sampled request has just left -- and the last four ask for top-p; with one slot the chain is strict
# (2 -> 3 sampled -> greedy, 5 -> 6 greedy -> top-p)
QUEUE_SETS = [1, 1, 1, 0, 0, 0, 2, 3, 2, 3]


def _req(row, n_text, max_tokens, speaker="aiden", language="english", n_instruct=0, sampling=None):
    from qwen3tts import GenerationRequest, RequestSampling
    r = tiny_request(row=row, n_text=n_text, n_instruct=n_instruct, speaker=speaker, language=language)
    return GenerationRequest(r["text_ids"], r["target_token_count"], r["instruct_ids"], r["speaker"], r["language"], max_tokens,
                             sampling=RequestSampling(**sampling) if sampling is not None else None)


def _mixed(sets):
    """tests/test_queued.py's ten requests (prompt lengths, speakers, languages, instruct and max_tokens all vary), request i
    carrying parameter set P[sets[i]] (sets None, or no entry i: no parameters of its own)."""
    spk = ["aiden", "vivian", "eric"]
    lang = ["english", "auto", "chinese", "english", "auto"]
    mt = [23, 5, 40, 11, 7, 33, 17, 6, 28, 14]
    return [_req(row=i, n_text=5 + (3 * i) % 11, max_tokens=mt[i], speaker=spk[i % 3], language=lang[i % 5],
                 n_instruct=(4 if i % 4 == 2 else 0), sampling=P[sets[i]] if sets is not None and i < len(sets) else None)
            for i in range(10)]


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


@pytest.fixture(scope="module")
def alone(models):
    """Every queue request alone under its own set, as call-wide keywords: the reference of the queue tests, computed once."""
    plain = _mixed(None)
    out = {}
    for name, extra in (("whole", {}), ("streamed", STREAM)):
        out[name] = [models[True].generate_batch([plain[i]], row_base=i, **P[QUEUE_SETS[i]], **extra)[0] for i in range(10)]
    return out


@pytest.mark.parametrize("graph", [True, False])
def test_static_batch_equals_each_row_alone(models, graph):
    m = models[graph]
    plain = _mixed(None)[:4]
    reqs = _mixed([0, 1, 2, 3])[:4]
    got = m.generate_batch(reqs)
    for i in range(4):
        _same(got[i], m.generate_batch([plain[i]], row_base=i, **P[i])[0])
    call_wide = m.generate_batch(plain)
    differ = sum(1 for g, w in zip(got, call_wide) if g.codes.shape != w.codes.shape or not np.array_equal(g.codes, w.codes))
    assert differ >= 2, differ


@pytest.mark.parametrize("graph,slots", [(True, 3), (False, 3), (True, 1)])
def test_queue_equals_each_request_alone(models, alone, graph, slots):
    got = models[graph].generate_queued(_mixed(QUEUE_SETS), slots=slots)
    for i in range(10):
        _same(got[i], alone["whole"][i])


def test_queue_over_two_lanes(ckpt_dirs, alone):
    from qwen3tts import Qwen3TTSModel
    two = Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], max_batch=4, max_frames=64, max_prompt=96, n_streams=2)
    try:
        got = two.generate_queued(_mixed(QUEUE_SETS), slots=3)
        static = two.generate_batch(_mixed(QUEUE_SETS)[:4])  # rows 2, 3 are the second lane's: its slice of the array
    finally:
        two.close()
    for i in range(10):
        _same(got[i], alone["whole"][i])
    for i in range(4):
        _same(static[i], alone["whole"][i])


def test_streamed_queue_equals_each_request_streamed_alone(models, alone):
    got = models[True].generate_queued(_mixed(QUEUE_SETS), slots=3, **STREAM)
    for i in range(10):
        _same(got[i], alone["streamed"][i])


def test_inheritance(models):
    from qwen3tts import RequestSampling
    m = models[True]
    kw = P[1]
    plain = _mixed(None)[:3]
    want = m.generate_batch(plain, **kw)

    def with_rows(rows):
        reqs = _mixed(None)[:3]
        for r, s in zip(reqs, rows):
            r.sampling = s
        return reqs

    for g, w in zip(m.generate_batch(with_rows([RequestSampling()] * 3), **kw), want):  # an array that sets nothing
        _same(g, w)
    for g, w in zip(m.generate_batch(with_rows([RequestSampling(**kw)] * 3), **kw), want):  # the call's own values again
        _same(g, w)
    for g, w in zip(m.generate_queued(with_rows([RequestSampling(), None, RequestSampling(**kw)]), slots=2, **kw), want):
        _same(g, w)
    # only the seed: the sampled rows change, a greedy row does not
    base = m.generate_batch(with_rows([RequestSampling(temperature=0.0), None, None]), **kw)
    seeded = m.generate_batch(with_rows([RequestSampling(temperature=0.0, seed=9), RequestSampling(seed=9), RequestSampling(seed=9)]),
                              **kw)
    _same(seeded[0], base[0])
    for i in (1, 2):
        assert seeded[i].codes.shape != base[i].codes.shape or not np.array_equal(seeded[i].codes, base[i].codes)
        _same(seeded[i], m.generate_batch([plain[i]], row_base=i, **{**kw, "seed": 9})[0])


def test_background_job_copies_the_array_during_begin(models):
    """q3tts_generate_begin without a callback returns before the codes exist; the caller's per_request array is its own
    again from then on, like reqs."""
    from qwen3tts import _lib as L
    m = models[True]
    reqs = _mixed([0, 1, 2, 3])[:4]
    want = m.generate_batch(reqs)
    arr, keep = m._marshal(reqs)
    s = m._sampling(0.9, 50, 1.0, 1.05, 0, 0, reqs=reqs)
    job = C.c_void_p()
    m._check(m._lib.q3tts_generate_begin(m._h, arr, 4, C.byref(s), C.cast(None, L.EVENT_CB), None, 0, C.byref(job)))
    C.memset(s._rows, 0xff, C.sizeof(s._rows))  # unknown bits, NaN, negative top-k: nothing may read it any more
    got = m.generate_batch_end((job, 4, None))
    del keep
    for g, w in zip(got, want):
        _same(g, w)


def test_teacher_forced(models):
    m = models[True]
    plain = _mixed(None)[:3]
    reqs = _mixed([0, 1, 2])[:3]
    F = 6
    rng = np.random.default_rng(3)
    forced = np.concatenate([rng.integers(0, 2048, (3, F, 1)), rng.integers(0, m.info.cp_vocab_size, (3, F, 15))], axis=2).astype(np.int32)
    tl, cl, sampled = m.debug_generate_forced(reqs, forced, row_base=20)
    tl0, cl0, sampled0 = m.debug_generate_forced(plain, forced, row_base=20)
    assert np.array_equal(tl, tl0) and np.array_equal(cl, cl0)  # the parameters do not reach the logits
    assert not np.array_equal(sampled, sampled0)
    for i in range(3):
        _, _, one = m.debug_generate_forced([plain[i]], forced[i:i + 1], row_base=20 + i, **P[i])
        assert np.array_equal(sampled[i], one[0]), i


def _raw(m, reqs, rows, queued):
    """The call with a hand-made q3tts_row_sampling array (what RequestSampling cannot express: unknown bits)."""
    from qwen3tts import _lib as L
    arr, keep = m._marshal(reqs)
    s = m._sampling(0.9, 50, 1.0, 1.05, 0, 0)
    s.per_request = C.cast(rows, C.POINTER(L.RowSampling))
    res = (L.Result * len(reqs))()
    none = C.cast(None, L.EVENT_CB)
    if queued:
        st = m._lib.q3tts_generate_queued(m._h, arr, len(reqs), 2, C.byref(s), none, None, res)
    else:
        st = m._lib.q3tts_generate(m._h, arr, len(reqs), C.byref(s), none, None, res)
    del keep
    return m._collect(st, res, len(reqs))


def test_refusals_leave_the_engine_usable(models):
    from qwen3tts import Qwen3TTSError, RequestSampling
    from qwen3tts import _lib as L
    m = models[True]
    good = _mixed([0, 1, 2, 3])[:3]
    want = m.generate_batch(good)
    bad = [dict(temperature=float("nan")), dict(temperature=float("inf")), dict(top_p=float("nan")), dict(top_p=-0.1),
           dict(top_p=1.5), dict(repetition_penalty=float("inf")), dict(repetition_penalty=float("nan")),
           dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(top_k=-1)]
    seen = []
    for kw in bad:
        for call in (m.generate_batch, lambda r, **k: m.generate_queued(r, slots=2, **k)):
            reqs = _mixed([0, 1, 2, 3])[:3]
            reqs[2].sampling = RequestSampling(**kw)  # the LAST request: refused before anything runs
            with pytest.raises(Qwen3TTSError) as e:
                call(reqs, on_event=lambda i, k, p: seen.append(k))
            assert e.value.status == 3 and "per_request[2]" in str(e.value), (kw, str(e.value))
    for queued in (False, True):
        rows = (L.RowSampling * 3)()
        rows[1].set = 32
        with pytest.raises(Qwen3TTSError) as e:
            _raw(m, good, rows, queued)
        assert e.value.status == 3 and "per_request[1]" in str(e.value)
    assert seen == []
    # the edges of the rules are inside: top_p 0 (no top-p) and 1, top_k 0, an unset field is not looked at
    reqs = _mixed(None)[:3]
    reqs[0].sampling = RequestSampling(top_p=0.0, top_k=0)
    reqs[1].sampling = RequestSampling(top_p=1.0)
    rows = (L.RowSampling * 3)()
    rows[2].temperature = float("nan")  # set == 0
    assert all(r.status in (0, 2) for r in m.generate_batch(reqs))
    for g, w in zip(_raw(m, _mixed(None)[:3], rows, False), m.generate_batch(_mixed(None)[:3])):
        _same(g, w)
    for g, w in zip(m.generate_batch(good), want):
        _same(g, w)
    for g, w in zip(m.generate_queued(good, slots=2), want):
        _same(g, w)
