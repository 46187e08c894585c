"""Formant preservation on the device: the two kernels of csrc/kernels/formant.hip against the definition (csrc/formant_plan.h
through its stand-alone driver) bit for bit, q3tts_pitch_shift_formants against formant_shift_reference, the decoder with
keep_formants against the causal definition applied to the default handle's 24 kHz decode, the stream, queue, session and
prefix-state guarantees, the handles on which the option adds nothing, refusals and the command line.

Equality is exact throughout: every sum has a fixed order that the kernels follow (formant_plan.h states them)."""
import os
import re
import shutil

import numpy as np
import pytest

from test_formant_plan import (P, ROUND_TRIP_BOUNDS, formant_driver, header_analyse, header_formant_causal,  # noqa: F401  (a fixture)
                               header_formant_shift, header_synth, shared_vowel)
from test_pitch_plan import choose_hp
from test_stretch_plan import seeded_signal

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not shutil.which("g++"), reason="g++ is not installed")]

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LOAD = dict(max_batch=4, max_frames=96, max_prompt=96)
C_, W_, L_ = 8, 32, 4
STREAM = dict(audio_chunk_frames=C_, audio_window_frames=W_, audio_lookahead_frames=L_)
F_ROWS = [37, 5, 22]
F_DEF = [7, 12]
PAIRS = [(509, 480), (360, 480), (719, 480), (480, 384), (960, 480), (240, 480)]
# key -> (load options, Ho, Hp); the same handle without a pitch
HANDLES = {"+4": (dict(pitch=4.0), 480, 605), "-5": (dict(pitch=-5.0), 480, 360), "+4@1.25": (dict(pitch=4.0, speed=1.25), 384, 484)}
PLAIN = {"+4": "A", "-5": "A", "+4@1.25": "1.25"}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def models(ckpt_dirs):
    from qwen3tts import Qwen3TTSModel
    out = {"A": Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], **LOAD),
           "1.25": Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], speed=1.25, **LOAD)}
    for key, (kw, _, _) in HANDLES.items():
        out[key] = Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], keep_formants=True, **kw, **LOAD)
    yield out
    for m in out.values():
        m.close()


def _codes(model, rows, seed):
    rng = np.random.default_rng(seed)
    hi = min(model.info.cp_vocab_size, 2048)
    c = np.zeros((len(rows), max(rows), 16), np.int32)
    for b, f in enumerate(rows):
        c[b, :f] = rng.integers(1, hi, size=(f, 16))
    return c


@pytest.fixture(scope="module")
def codes(models):
    return _codes(models["A"], F_ROWS, 11)


@pytest.fixture(scope="module")
def short(models):
    """(codes, the default handle's 24 kHz decode of them), computed once and shared."""
    c = _codes(models["A"], F_DEF, 12)
    pcm, lens = models["A"].codec_decode(c, n_frames=F_DEF)
    pcm.setflags(write=False)
    return c, pcm, lens


def _row_sets(hop):
    """Three rows per launch: nothing / one sample / P samples; around one hop; two hops and a bit, three frames and a bit."""
    return [[0, 1, P], [hop - 1, hop, hop + 1], [2 * hop + 5, 3 * 4 * hop + 5, 2 * hop + 5]]


# ---- 1. the kernels against the definition ------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%d-%d" % p)
def test_analyse_and_whiten_equal_the_definition(models, formant_driver, tmp_path, pair):  # noqa: F811
    """Rows of noise at every length that takes another path (a row that must touch nothing, one shorter than the order, the
    hop's edges, a short last hop, more than a frame), then a silent, an impulse and a DC row (the fallbacks and the slowest
    decaying autocorrelation), then rows behind a margin. Samples behind a row's end and, without `hist`, in front of its start
    must read as zero: both hold noise here."""
    m = models["A"]
    hp, ho = pair
    cases = [(lens, 0, None) for lens in _row_sets(hp)]
    n_sp = 2 * hp + 5
    special = np.zeros((3, n_sp), np.float32)
    special[1, hp + 7] = 0.75
    special[2] = 0.25
    cases.append(([n_sp] * 3, 0, special))
    cases.append(([hp + 1, 2 * hp + 5, 0], hp + P + 3, None))
    for lens, hist, fixed in cases:
        rng = np.random.default_rng(hp + 7 * hist + sum(lens))
        stride = hist + max(lens) + 9
        x = rng.uniform(-0.9, 0.9, (3, stride)).astype(np.float32)
        if fixed is not None:
            x[:, :fixed.shape[1]] = fixed
        hops = [-(-n // hp) for n in lens]
        y0 = np.full((3, max(lens) + 5), 7.0, np.float32)
        c0 = np.full((3, max(hops) * P + 3), 7.0, np.float32)
        y, coef, _ = m.debug_formant_rows(0, hp, ho, x, lens, c0, y0, hist=hist)
        for b, n in enumerate(lens):
            assert (y[b, n:] == 7.0).all() and (coef[b, hops[b] * P:] == 7.0).all(), (lens, b)  # nothing behind the row's outputs
            if n == 0:
                continue
            want_c, want_e, ok = header_analyse(formant_driver, tmp_path, hp, x[b, :hist + n], hist=hist)
            assert np.array_equal(bits(coef[b, :hops[b] * P]), bits(want_c.reshape(-1))), (lens, hist, b)
            assert np.array_equal(bits(y[b, :n]), bits(want_e)), (lens, hist, b, int((bits(y[b, :n]) != bits(want_e)).sum()))
            if fixed is not None and b < 2:  # the silent row falls back at every hop; the impulse row is white (a = 0 either way)
                assert not coef[b, :hops[b] * P].any() and np.array_equal(y[b, :n], x[b, :n])
                assert b == 1 or not ok.any()


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%d-%d" % p)
def test_synthesis_equals_the_definition_and_hands_its_state_on(models, formant_driver, tmp_path, pair):  # noqa: F811
    m = models["A"]
    hp, ho = pair
    # coefficients of a vowel at Hp per hop: a filter that rings (and is stable: Levinson's own)
    v = shared_vowel(110)
    coef_all, _, _ = header_analyse(formant_driver, tmp_path, hp, v[6000:6000 + 16 * hp])
    for lens in _row_sets(ho):
        rng = np.random.default_rng(ho + sum(lens))
        hops = [-(-n // ho) for n in lens]
        x = rng.uniform(-0.05, 0.05, (3, max(lens) + 9)).astype(np.float32)
        coef = np.full((3, max(hops) * P + 3), 7.0, np.float32)
        for b in range(3):
            coef[b, :hops[b] * P] = coef_all[b:b + hops[b]].reshape(-1)
        s_in = rng.uniform(-0.3, 0.3, (3, P)).astype(np.float32)
        y0 = np.full((3, max(lens) + 5), 7.0, np.float32)
        y, _, s_out = m.debug_formant_rows(1, hp, ho, x, lens, coef, y0, state_in=s_in, want_state=True)
        yc, _, _ = m.debug_formant_rows(1, hp, ho, x, lens, coef, y0, state_in=s_in, clamp=True)
        for b, n in enumerate(lens):
            assert (y[b, n:] == 7.0).all(), (lens, b)
            if n == 0:
                assert np.array_equal(s_out[b], s_in[b])  # a row of length 0 touches nothing, its state included
                continue
            want, want_s = header_synth(formant_driver, tmp_path, ho, x[b, :n], coef[b, :hops[b] * P], state=s_in[b])
            assert np.array_equal(bits(y[b, :n]), bits(want)), (lens, b, int((bits(y[b, :n]) != bits(want)).sum()))
            assert np.array_equal(bits(s_out[b]), bits(want_s)), (lens, b)
            assert np.array_equal(bits(yc[b, :n]), bits(np.clip(want, -1.0, 1.0))), (lens, b)
    # two launches with the state handed on against one launch: cut at a frame's end (and rows of different lengths)
    lens, cut = [3 * 4 * ho + 5, 2 * 4 * ho, 4 * ho + 1], 4 * ho
    rng = np.random.default_rng(3 * ho)
    hops = [-(-n // ho) for n in lens]
    x = rng.uniform(-0.05, 0.05, (3, max(lens))).astype(np.float32)
    coef = np.zeros((3, max(hops) * P), np.float32)
    for b in range(3):
        coef[b, :hops[b] * P] = coef_all[:hops[b]].reshape(-1)
    y0 = np.zeros((3, max(lens)), np.float32)
    whole, _, s_whole = m.debug_formant_rows(1, hp, ho, x, lens, coef, y0, want_state=True)
    first, _, s1 = m.debug_formant_rows(1, hp, ho, x[:, :cut], [cut] * 3, coef[:, :4 * P], y0[:, :cut], want_state=True)
    rest_lens = [n - cut for n in lens]
    rest, _, s2 = m.debug_formant_rows(1, hp, ho, np.ascontiguousarray(x[:, cut:]), rest_lens, np.ascontiguousarray(coef[:, 4 * P:]),
                                       np.ascontiguousarray(y0[:, cut:]), state_in=s1, want_state=True)
    for b, n in enumerate(lens):
        assert np.array_equal(bits(np.concatenate([first[b], rest[b, :n - cut]])), bits(whole[b, :n])), b
        assert np.array_equal(bits(s2[b]), bits(s_whole[b])), b


@pytest.mark.parametrize("kind", ("noise", "vowel"))
def test_round_trip_on_the_device(models, formant_driver, tmp_path, kind):  # noqa: F811
    """Hp == Ho, both kernels with the identity in between: the input again within the bound measured on the definition, and the
    definition's own result bit for bit."""
    m = models["A"]
    for hp in (240, 480, 960):
        n = 10 * hp + 17
        x = np.random.default_rng(hp).uniform(-0.5, 0.5, n).astype(np.float32) if kind == "noise" else shared_vowel(110)[6000:6000 + n]
        rows = np.stack([x, x[::-1], 0.5 * x])
        z, coef, _ = m.debug_formant_rows(2, hp, hp, rows, [n, n - hp - 3, n], np.zeros((3, 11 * P), np.float32), np.zeros((3, n), np.float32))
        assert float(np.max(np.abs(z[0] - x))) <= ROUND_TRIP_BOUNDS[kind], (kind, hp)
        want_c, want_e, _ = header_analyse(formant_driver, tmp_path, hp, x)
        want_z, _ = header_synth(formant_driver, tmp_path, hp, want_e, want_c)
        assert np.array_equal(bits(coef[0]), bits(want_c.reshape(-1))) and np.array_equal(bits(z[0]), bits(want_z))


def test_the_row_hook_refuses_what_does_not_fit(models):
    from qwen3tts.model import Qwen3TTSError
    m = models["A"]
    x, c, y = np.zeros((1, 600), np.float32), np.zeros((1, 2 * P), np.float32), np.zeros((1, 600), np.float32)
    for kw in (dict(mode=3), dict(mode=-1), dict(hp=239), dict(ho=961), dict(mode=2, hp=480, ho=384), dict(lens=[601]), dict(lens=[-1]),
               dict(lens=[1000], x=np.zeros((1, 1000), np.float32)),                # does not fit y
               dict(lens=[600], c=np.zeros((1, P), np.float32)),                    # two hops, room for one
               dict(mode=1, hist=4), dict(mode=0, state_in=np.zeros((1, P), np.float32))):
        a = dict(mode=0, hp=480, ho=480, lens=[600], x=x, c=c, hist=0, state_in=None)
        a.update(kw)
        with pytest.raises(Qwen3TTSError) as e:
            m.debug_formant_rows(a["mode"], a["hp"], a["ho"], a["x"], a["lens"], a["c"], y, hist=a["hist"], state_in=a["state_in"])
        assert e.value.status == 3, kw
    assert m.debug_formant_rows(0, 480, 480, x, [600], c, y)[0].shape == (1, 600)


# ---- 2. q3tts_pitch_shift_formants against the definition --------------------------------------------------------------------
@pytest.mark.parametrize("semitones", (-5, 3, 7))
def test_pitch_shift_formants_equals_the_definition(models, formant_driver, tmp_path, semitones):  # noqa: F811
    m = models["A"]
    hp = choose_hp(480, semitones)
    for n in (1, 479, 5000):
        x = seeded_signal(n, 2000 + n)
        got = m.pitch_shift(x, semitones, keep_formants=True)
        want = header_formant_shift(formant_driver, tmp_path, hp, x)
        assert got.size == want.size == m.pitch_shift(x, semitones).size and abs(got.size - n) <= 2
        assert np.array_equal(bits(got), bits(want)), (semitones, n)
    x = seeded_signal(700, 5)
    assert np.array_equal(m.pitch_shift(x, 0.0, keep_formants=True), x)  # Hp == 480: a copy


# ---- 3. the decoder with keep_formants is the definition ---------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(HANDLES))
def test_decoder_with_kept_formants_is_the_definition(models, short, formant_driver, tmp_path, key):  # noqa: F811
    _, ho, hp = HANDLES[key]
    B, Pl = models[key], models[PLAIN[key]]
    spf = 4 * ho
    assert B.keep_formants_info() and not Pl.keep_formants_info() and B.pitch_info()[1:3] == (hp, ho)
    assert (B.sample_rate, B.info.samples_per_frame) == (24000, spf) == (Pl.sample_rate, Pl.info.samples_per_frame)
    c, pcm24, _ = short
    got, lens = B.codec_decode(c, n_frames=F_DEF)
    _, plain_lens = Pl.codec_decode(c, n_frames=F_DEF)
    assert got.shape == (2, max(F_DEF) * spf) and np.array_equal(lens, plain_lens)
    for b, f in enumerate(F_DEF):
        want = header_formant_causal(formant_driver, tmp_path, hp, ho, pcm24[b, :f * 1920])
        assert want.size == f * spf
        assert np.array_equal(bits(got[b, :f * spf]), bits(want)), (key, b, int((bits(got[b, :f * spf]) != bits(want)).sum()))


# ---- 4. the guarantees carry over, bit for bit --------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["+4", "+4@1.25"])
@pytest.mark.parametrize("chunk", [3, 8])
def test_streamed_decode_equals_one_shot(models, codes, chunk, key):
    B = models[key]
    spf = B.info.samples_per_frame
    want, _ = B.codec_decode(codes, n_frames=F_ROWS)
    got = B.codec_decode_streamed(codes, chunk, -1, n_frames=F_ROWS)
    for b, f in enumerate(F_ROWS):
        assert np.array_equal(got[b, :f * spf], want[b, :f * spf]), (chunk, b)


def test_slotted_stream_equals_each_request_streamed_alone(models):
    B = models["+4"]
    F = [9, 33, 20, 8, 17]
    c = _codes(B, F, 5)
    got = B.debug_codec_stream_slots(c, F, 2, 5, C_, W_, L_)
    for i, f in enumerate(F):
        alone = B.codec_decode_streamed(c[i:i + 1, :f], C_, W_, L_)[0]
        assert np.array_equal(got[i, :f * 1920], alone[:f * 1920]), i


def test_streamed_queue_and_session_equal_each_request_alone(models):
    from conftest import tiny_request
    from qwen3tts import GenerationRequest
    B = models["+4"]
    caps = [9, 33, 20, 8]
    reqs = [GenerationRequest(**tiny_request(row=i, n_text=6 + i), max_tokens=c) for i, c in enumerate(caps)]
    kw = dict(temperature=0.9, top_k=50, seed=21)
    got = B.generate_queued(reqs, slots=2, **kw, **STREAM)
    alone = [B.generate_batch([r], row_base=i, **kw, **STREAM)[0] for i, r in enumerate(reqs)]
    assert any(g.codes.shape[0] > C_ for g in got)
    for i in range(len(reqs)):
        assert got[i].status == alone[i].status and np.array_equal(got[i].codes, alone[i].codes)
        assert np.array_equal(got[i].audio, alone[i].audio) and got[i].audio.size == got[i].codes.shape[0] * 1920, i
    s = B.open_session(slots=2, **kw, **STREAM)
    try:
        assert [s.submit(r) for r in reqs[:3]] == [0, 1, 2]
        for t in range(3):
            r = s.result(t, timeout=60)
            assert r.status == alone[t].status and np.array_equal(r.codes, alone[t].codes) and np.array_equal(r.audio, alone[t].audio), t
    finally:
        s.close()


def test_a_saved_prefix_state_with_kept_formants(tmp_path):
    """One streamed voice served twice -- first decoding its reference, then from the saved state: equal results. The state is
    larger than the same pitched handle's without the option by the margins of the two tensors with history that the stage adds,
    hist_frames * (align16(4 Hp * 4) + align16(P * 4)) = 3 * (4 * 605 * 4 + 96) bytes: the whitened signal and the filter's
    state."""
    from qwen3tts import GenerationRequest, Qwen3TTSModel, synth
    d = str(tmp_path / "tiny-base")
    synth.write_checkpoint(d, "tiny-base", seed=4321)
    load = dict(max_batch=4, max_frames=64, max_prompt=160)

    def prompt(row, n_text=10):
        return synth.synthetic_prompt(row, n_text=n_text, text_vocab=1000, im_start=1000, im_end=1001)

    clip, ids = synth.synthetic_reference_audio(1, 1.0), prompt(1)["ref_text_ids"]
    p = prompt(2, 9)
    kw = dict(audio_stream_reference=1, temperature=0.9, top_k=40, repetition_penalty=1.5, seed=77, **STREAM)
    grown, audio = {}, {}
    for key, opts in (("+4", dict(pitch=4.0)), ("kept", dict(pitch=4.0, keep_formants=True))):
        m = Qwen3TTSModel.from_pretrained(d, **opts, **load)
        try:
            with m.create_voice(clip, ids) as v:
                r = GenerationRequest(p["text_ids"], p["target_token_count"], None, None, "english", 10, voice=v)
                n0, b0, r0 = m.debug_prefix_states()
                first = m.generate_queued([r], slots=1, **kw)[0]
                n1, b1, r1 = m.debug_prefix_states()
                again = m.generate_queued([r], slots=1, **kw)[0]
                n2, b2, r2 = m.debug_prefix_states()
                assert (n1, r1) == (n0 + 1, r0) and (n2, b2, r2) == (n1, b1, r1 + 1)  # decoded and saved, then restored
                assert first.status == 0 and first.codes.shape[0] > 0 and first.audio.size == first.codes.shape[0] * 1920
                assert np.array_equal(first.codes, again.codes) and np.array_equal(first.audio, again.audio)
                grown[key], audio[key] = b1 - b0, first
        finally:
            m.close()
    assert grown["kept"] - grown["+4"] == 3 * (4 * 605 * 4 + P * 4)
    assert np.array_equal(audio["kept"].codes, audio["+4"].codes) and not np.array_equal(audio["kept"].audio, audio["+4"].audio)


# ---- 5. the option without a pitch that is on adds nothing ----------------------------------------------------------------------
def test_keep_formants_without_a_pitch_is_the_default_decode(ckpt_dirs, models, codes):
    from qwen3tts import Qwen3TTSModel
    A = models["A"]
    want, want_lens = A.codec_decode(codes, n_frames=F_ROWS)
    want_stream = A.codec_decode_streamed(codes, 8, -1, n_frames=F_ROWS)
    for pitch in (0.0, 0.001):  # off, and Hp == Ho
        Z = Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], pitch=pitch, keep_formants=True, **LOAD)
        try:
            assert not Z.keep_formants_info() and Z.pitch_info() == (0.0, 480, 480, 0)
            assert Z.debug_prefix_states() == A.debug_prefix_states()
            pcm, lens = Z.codec_decode(codes, n_frames=F_ROWS)
            assert pcm.tobytes() == want.tobytes() and np.array_equal(lens, want_lens)
            assert Z.codec_decode_streamed(codes, 8, -1, n_frames=F_ROWS).tobytes() == want_stream.tobytes()
        finally:
            Z.close()
    S = models["1.25"]
    Z = Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], pitch=0.001, speed=1.25, keep_formants=True, **LOAD)
    try:
        assert not Z.keep_formants_info() and Z.pitch_info() == (0.0, 384, 384, 0)
        assert Z.codec_decode(codes, n_frames=F_ROWS)[0].tobytes() == S.codec_decode(codes, n_frames=F_ROWS)[0].tobytes()
    finally:
        Z.close()


# ---- 6. refusals, and the command line ------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_usable(models, ckpt_dirs, codes):
    from conftest import tiny_request
    from qwen3tts import GenerationRequest, Qwen3TTSModel
    from qwen3tts.model import Qwen3TTSError
    B = models["+4"]
    want, _ = B.codec_decode(codes, n_frames=F_ROWS)
    req = GenerationRequest(**tiny_request(row=1), max_tokens=40)
    whole = B.generate_batch([req], temperature=0.0, force_frames=9)[0]
    # the chunked exact decode (audio_chunk_frames without a window) is not offered with keep_formants
    with pytest.raises(Qwen3TTSError) as e:
        B.generate_batch([req], temperature=0.0, force_frames=9, audio_chunk_frames=3, on_event=lambda *a: None)
    assert e.value.status == 3 and "keep_formants" in str(e.value)
    again = B.generate_batch([req], temperature=0.0, force_frames=9)[0]
    assert np.array_equal(again.codes, whole.codes) and np.array_equal(again.audio, whole.audio) and whole.audio.size > 0
    streamed = B.generate_batch([req], temperature=0.0, force_frames=9, on_event=lambda *a: None, **STREAM)[0]
    assert np.array_equal(streamed.codes, whole.codes) and streamed.audio.size == whole.audio.size
    for kw in (dict(pitch=4.0, keep_formants=2), dict(pitch=4.0, keep_formants=-1), dict(pitch=4.0, keep_formants=True, output_sample_rate=16000),
               dict(keep_formants=True, output_sample_rate=48000), dict(pitch=4.0, keep_formants=True, request_speeds=True)):
        with pytest.raises(Qwen3TTSError) as e:
            Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], **kw, **LOAD)
        assert e.value.status == 3, kw
    x = seeded_signal(1500, 3)
    for bad in (12.001, float("nan")):
        with pytest.raises(Qwen3TTSError) as e:
            B.pitch_shift(x, bad, keep_formants=True)
        assert e.value.status == 3
    assert B.codec_decode(codes, n_frames=F_ROWS)[0].tobytes() == want.tobytes()


def test_a_clone_row_with_chunks_and_no_streamed_reference_is_refused(tmp_path):
    """audio_chunk_frames with a window streams only when no row is a voice clone, or audio_stream_reference is set; otherwise
    the job goes to the chunked exact decode, which a handle with keep_formants does not offer: INVALID_INPUT before any GPU
    work, with a stretch stage (+4: Hp = 605) and without one (+3.86 at speed 1.25: Hp = 480, Ho = 384), for a waveform and for a
    voice. The same requests are served in one piece, and streamed with audio_stream_reference."""
    from qwen3tts import GenerationRequest, Qwen3TTSModel, synth
    from qwen3tts.model import Qwen3TTSError
    d = str(tmp_path / "tiny-base")
    synth.write_checkpoint(d, "tiny-base", seed=4321)

    def prompt(row, n_text=10):
        return synth.synthetic_prompt(row, n_text=n_text, text_vocab=1000, im_start=1000, im_end=1001)

    clip, ids = synth.synthetic_reference_audio(1, 1.0), prompt(1)["ref_text_ids"]
    p = prompt(2, 9)
    kw = dict(temperature=0.9, top_k=40, repetition_penalty=1.5, seed=77)
    for opts, hp, ho in ((dict(pitch=4.0), 605, 480), (dict(pitch=3.86, speed=1.25), 480, 384)):
        m = Qwen3TTSModel.from_pretrained(d, keep_formants=True, max_batch=4, max_frames=64, max_prompt=160, **opts)
        try:
            assert m.keep_formants_info() and m.pitch_info()[1:3] == (hp, ho)
            with m.create_voice(clip, ids) as v:
                by_clip = GenerationRequest(p["text_ids"], p["target_token_count"], None, None, "english", 10, ref_audio=clip, ref_text_ids=ids)
                by_voice = GenerationRequest(p["text_ids"], p["target_token_count"], None, None, "english", 10, voice=v)
                for r in (by_clip, by_voice):
                    for mode in (STREAM, dict(audio_chunk_frames=C_)):
                        with pytest.raises(Qwen3TTSError) as e:
                            m.generate_batch([r], on_event=lambda *a: None, **kw, **mode)
                        assert e.value.status == 3 and "keep_formants" in str(e.value), (opts, mode)
                whole = m.generate_batch([by_clip], **kw)[0]
                assert whole.status == 0 and whole.audio.size == whole.codes.shape[0] * 4 * ho > 0
                streamed = m.generate_batch([by_clip], on_event=lambda *a: None, audio_stream_reference=1, **kw, **STREAM)[0]
                assert streamed.status == 0 and np.array_equal(streamed.codes, whole.codes) and streamed.audio.size == whole.audio.size
        finally:
            m.close()


def test_fp32_redecode_of_held_requests_with_kept_formants(tmp_path):
    """tests/test_codec_range.py's checkpoint: every row leaves the fp16 range and is decoded again on the fp32 matrix cores,
    through the same tail -- the formant stage included. Whole: the samples of a handle loaded with codec_fp32. From the streamed
    queue (the held requests' re-decode): each request equals the same request streamed alone."""
    from conftest import tiny_request
    from test_codec_range import _big_bias_checkpoint
    from qwen3tts import GenerationRequest, Qwen3TTSModel
    d = _big_bias_checkpoint(tmp_path)
    load = dict(max_batch=4, max_frames=32, max_prompt=64, pitch=4.0, keep_formants=True)
    reqs = [GenerationRequest(**tiny_request(row=i, n_text=6 + i), max_tokens=c) for i, c in enumerate([20, 6, 13])]
    kw = dict(temperature=0.9, top_k=50, seed=21)
    m = Qwen3TTSModel.from_pretrained(d, codec_fp32=True, **load)
    try:
        want = m.generate_batch(reqs, **kw)
    finally:
        m.close()
    assert any(w.status == 0 and w.codes.shape[0] > 0 and np.isfinite(w.audio).all() and np.abs(w.audio).max() > 0 for w in want)
    m = Qwen3TTSModel.from_pretrained(d, **load)  # the default (fp16 two-plane) kernels
    try:
        assert m.keep_formants_info()
        got = m.generate_batch(reqs, **kw)
        got_st = m.generate_queued(reqs, slots=2, **kw, **STREAM)
        for i, r in enumerate(reqs):
            assert got[i].status == want[i].status and np.array_equal(got[i].codes, want[i].codes), i
            assert np.isfinite(got[i].audio).all() and np.array_equal(got[i].audio, want[i].audio), i
            alone = m.generate_batch([r], row_base=i, **kw, **STREAM)[0]
            assert got_st[i].status == alone.status and np.array_equal(got_st[i].codes, alone.codes), i
            assert np.isfinite(got_st[i].audio).all() and np.array_equal(got_st[i].audio, alone.audio), i
    finally:
        m.close()


def test_cli_with_kept_formants(tmp_path, capsys):
    from qwen3tts import synth
    from qwen3tts.__main__ import main
    d = str(tmp_path / "model")
    synth.write_checkpoint(d, "tiny-b", seed=1234)
    shutil.copy(os.path.join(GOLD, "tokenizer.json"), os.path.join(d, "tokenizer.json"))
    out = str(tmp_path / "out.wav")
    rc = main(["--model", d, "--text", "Hello there, it's a test.", "--speaker", "aiden", "--language", "english", "--temperature", "0",
               "--max-tokens", "9", "--output", out, "--pitch", "4", "--keep-formants"])
    assert rc == 0
    text = capsys.readouterr().out
    assert re.search(r"Pitch: \+4\.0\d+ semitones \(hop 605 resampled to 480, delay \d+ samples\), formants kept", text)
    n = int(re.search(r"Generated (\d+) samples", text).group(1))
    assert n > 0 and n % 1920 == 0 and os.path.getsize(out) == 44 + 2 * n
