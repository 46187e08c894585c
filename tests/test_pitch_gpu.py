"""Pitch per handle on the device: the general-ratio resampler (csrc/kernels/resample_ratio.hip) against resample_reference,
q3tts_pitch_shift against the definition, the decoder at a pitch (q3tts_load_opts_ex.pitch) against the definition applied to the
default handle's 24 kHz decode, the stream, queue and prefix-state guarantees at a pitch, the default handle unchanged, refusals
and the command line.

The references are the headers themselves through their stand-alone drivers (tests/test_resample_plan.py, tests/test_pitch_plan.py).
Equality is exact throughout: every output is one fmaf chain in a fixed order behind a stretch whose choices are a total order."""
import ctypes as C
import math
import os
import shutil
import struct

import numpy as np
import pytest

from test_pitch_plan import choose_hp, delay_out, header_shift, pitch_driver, ratio, ratio_of  # noqa: F401  (pitch_driver: a fixture)
from test_resample_plan import driver, header_run  # noqa: F401  (driver: the resampler header's, a fixture)
from test_stretch_plan import seeded_signal

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not shutil.which("g++"), reason="g++ is not installed")]

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LOAD = dict(max_batch=4, max_frames=96, max_prompt=96)
C_, W_, L_ = 8, 32, 4
STREAM = dict(audio_chunk_frames=C_, audio_window_frames=W_, audio_lookahead_frames=L_)
F_ROWS = [37, 5, 22]   # the stream guarantees (device against device)
F_DEF = [7, 12]        # the definition: 2 ragged rows
# key -> (load options, Ho, Hp, output rate)
HANDLES = {
    "+2": (dict(pitch=2.0), 480, 539, 24000),
    "-3": (dict(pitch=-3.0), 480, 404, 24000),
    "+2@1.25": (dict(pitch=2.0, speed=1.25), 384, 431, 24000),
    "+2@16k": (dict(pitch=2.0, output_sample_rate=16000), 480, 539, 16000),
    "pure": (dict(pitch=3.86, speed=1.25), 384, 480, 24000),  # Hp == 480: no stretch stage
}
PLAIN = {"+2": "A", "-3": "A", "+2@1.25": "1.25", "+2@16k": "16k", "pure": "1.25"}  # the same handle without a pitch


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def models(ckpt_dirs):
    from qwen3tts import Qwen3TTSModel
    out = {"A": Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], **LOAD),
           "1.25": Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], speed=1.25, **LOAD),
           "16k": Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], output_sample_rate=16000, **LOAD)}
    for key, (kw, _, _, _) in HANDLES.items():
        out[key] = Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], **kw, **LOAD)
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
    c = _codes(models["A"], F_ROWS, 11)
    c[0, [3, 30], 0] = 0  # two frames that the end trim does not count
    return c


@pytest.fixture(scope="module")
def short(models):
    """(codes, the default handle's 24 kHz decode of them), computed once and shared."""
    c = _codes(models["A"], F_DEF, 12)
    c[1, 4, 0] = 0
    pcm, lens = models["A"].codec_decode(c, n_frames=F_DEF)
    pcm.setflags(write=False)
    return c, pcm, lens


# ---- 4. the general kernel against resample_reference ------------------------------------------------------------------------
# (in_units, out_units, the Hp behind the pair): the first table over 64 KiB; the largest table; K' = 204 and the longest span;
# L' = 2; +7 semitones
PAIRS = [(509, 480, 509), (958 * 80, 940 * 147, 958), (2880, 240, 240), (1, 2, 480), (719, 480, 719)]


@pytest.mark.parametrize("with_hist", (False, True), ids=("bare", "hist"))
@pytest.mark.parametrize("centred", (True, False), ids=("centred", "causal"))
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%d-%d" % p[:2])
def test_general_kernel_equals_the_reference(models, driver, tmp_path, pair, centred, with_hist):
    """Ragged rows of 0, 1, 255 and 257 input samples (the tile edges at 256 outputs for ratios near 1, a row that must touch
    nothing), then rows of 3 * 4 * Hp + 5 samples and of more than two tiles of outputs whatever the ratio. Samples behind a
    row's end and, without `hist`, in front of its start must read as zero: both hold noise here."""
    m = models["A"]
    in_u, out_u, hp = pair
    L2, M2, K2 = ratio(in_u, out_u, 1, 1)
    hist = 2 * K2 + 3 if with_hist else 0
    n_long = 3 * 4 * hp + 5
    for lens in ([0, 1, 255, 257], [n_long, max(n_long, 600 * M2 // L2 + 7)]):
        rng = np.random.default_rng(1000 * hist + sum(lens))
        stride = hist + max(lens) + 9
        x = rng.uniform(-0.9, 0.9, (len(lens), stride)).astype(np.float32)
        ylen = -(-max(lens) * L2 // M2) + 5
        y0 = np.full((len(lens), ylen), 7.0, np.float32)
        got = m.debug_resample_ratio(x, lens, in_u, out_u, y0, centred=centred, clamp=True, hist=hist)
        for b, n in enumerate(lens):
            n_out = -(-n * L2 // M2)
            assert (got[b, n_out:] == 7.0).all(), (lens, b)  # nothing behind the row's outputs (length 0: nothing at all)
            if n == 0:
                continue
            want, _ = header_run(driver, tmp_path, in_u, out_u, x[b, hist:hist + n], centred, front=x[b, :hist], clamp=True)
            assert want.size == n_out
            assert np.array_equal(bits(got[b, :n_out]), bits(want)), (lens, b, int((bits(got[b, :n_out]) != bits(want)).sum()))


def test_general_kernel_refuses_what_does_not_fit(models):
    from qwen3tts.model import Qwen3TTSError
    m = models["A"]
    x = np.zeros((1, 64), np.float32)
    for pair in ((0, 1), (1, 0), (-3, 2), (100000, 1), (1 << 31, 3)):  # not positive; a 256-output span beyond 64 KiB; too large
        with pytest.raises(Qwen3TTSError) as e:
            m.debug_resample_ratio(x, [64], pair[0], pair[1], np.zeros((1, 8), np.float32))
        assert e.value.status == 3, pair
    with pytest.raises(Qwen3TTSError):
        m.debug_resample_ratio(x, [64], 1, 2, np.zeros((1, 127), np.float32))  # one sample short
    assert m.debug_resample_ratio(x, [64], 1, 2, np.zeros((1, 128), np.float32)).shape == (1, 128)


# ---- 5. q3tts_pitch_shift against the definition ----------------------------------------------------------------------------
@pytest.mark.parametrize("semitones", (-12, -1, 1, 7, 12))
def test_pitch_shift_equals_the_definition(models, pitch_driver, tmp_path, semitones):
    m = models["A"]
    hp = choose_hp(480, semitones)
    L2, M2, _ = ratio(hp, 480, 1, 1)
    for n in (1, 479, 1920, 5000):
        x = seeded_signal(n, 2000 + n)
        got = m.pitch_shift(x, semitones)
        want = header_shift(pitch_driver, tmp_path, hp, hp, 480, x, causal=False)
        assert got.size == want.size == -(-(-(-n * hp // 480)) * L2 // M2) and abs(got.size - n) <= 2
        assert np.array_equal(bits(got), bits(want)), (semitones, n)
    x = seeded_signal(700, 5)
    assert np.array_equal(m.pitch_shift(x, 0.0), x) and np.array_equal(m.pitch_shift(x, 0.001), x)  # Hp == 480: a copy


# ---- 6. / 7. the decoder at a pitch is the definition ------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(HANDLES))
def test_decoder_at_a_pitch_is_the_definition(models, short, pitch_driver, tmp_path, key):
    """The causal stretch at Hp (none for "pure") followed by the causal plan Hp * M -> Ho * L, clipped, on the default handle's
    24 kHz waveform; sample counts are those of the same handle without a pitch."""
    _, ho, hp, rate = HANDLES[key]
    B, P = models[key], models[PLAIN[key]]
    L, M = ratio_of(rate)
    L2, M2, K2 = ratio(hp, ho, L, M)
    spf = 4 * ho * L // M
    eff, got_hp, got_ho, d = B.pitch_info()
    assert (got_hp, got_ho, d) == (hp, ho, delay_out(hp, L2, M2, K2)) and abs(eff - 12 * math.log2(hp / ho)) < 1e-5
    assert (B.stretch_hs, abs(B.speed - 480.0 / ho) < 1e-6, B.sample_rate, B.info.samples_per_frame) == (ho, True, rate, spf)
    assert (P.stretch_hs, P.sample_rate, P.info.samples_per_frame, P.pitch_info()) == (ho, rate, spf, (0.0, ho, ho, 0))
    if key == "pure":  # the stretch contributes no delay: the FIR's K' through L' / M' alone
        assert d == -(-K2 * L2 // M2) == 18 and (L2, M2, K2) == (4, 5, 22)
    c, pcm24, _ = short
    got, lens = B.codec_decode(c, n_frames=F_DEF)
    _, plain_lens = P.codec_decode(c, n_frames=F_DEF)
    assert got.shape == (2, max(F_DEF) * spf) and np.array_equal(lens, plain_lens)
    for b, f in enumerate(F_DEF):
        want = header_shift(pitch_driver, tmp_path, hp, hp * M, ho * L, pcm24[b, :f * 1920], causal=True, clamp=True)
        assert want.size == f * spf
        assert np.array_equal(bits(got[b, :f * spf]), bits(want)), (key, b, int((bits(got[b, :f * spf]) != bits(want)).sum()))
        assert lens[b] == int((c[b, :f, 0] > 0).sum()) * spf
    assert lens[1] == (F_DEF[1] - 1) * spf


def test_codes_and_sample_counts_do_not_depend_on_the_pitch(models):
    from conftest import tiny_request
    from qwen3tts import GenerationRequest
    req = GenerationRequest(**tiny_request(row=1), max_tokens=40)
    want = models["A"].generate_batch([req], temperature=0.0, force_frames=9)[0]
    for key in ("+2", "-3"):
        got = models[key].generate_batch([req], temperature=0.0, force_frames=9)[0]
        assert got.status == want.status and np.array_equal(got.codes, want.codes) and got.audio.size == want.audio.size > 0
        assert not np.array_equal(got.audio, want.audio)


# ---- 8. the guarantees carry over, bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["+2", "+2@16k"])
@pytest.mark.parametrize("chunk", [3, 8])
def test_streamed_decode_equals_one_shot(models, codes, chunk, key):
    B = models[key]
    spf = B.info.samples_per_frame
    want, _ = B.codec_decode(codes, n_frames=F_ROWS)
    got = B.codec_decode_streamed(codes, chunk, -1, n_frames=F_ROWS)
    for b, f in enumerate(F_ROWS):
        assert np.array_equal(got[b, :f * spf], want[b, :f * spf]), (chunk, b)


def test_pure_resample_handle_streams_and_chunks_like_one_shot(models, codes):
    """Hp == 480: no state word and no carried stretched signal; the FIR's margin is out_conv's own tensor."""
    from conftest import tiny_request
    from qwen3tts import GenerationRequest
    B = models["pure"]
    want, _ = B.codec_decode(codes, n_frames=F_ROWS)
    got = B.codec_decode_streamed(codes, 3, -1, n_frames=F_ROWS)
    for b, f in enumerate(F_ROWS):
        assert np.array_equal(got[b, :f * 1536], want[b, :f * 1536]), b
    req = GenerationRequest(**tiny_request(row=1), max_tokens=40)
    whole = B.generate_batch([req], temperature=0.0, force_frames=21)[0]
    piece = B.generate_batch([req], temperature=0.0, force_frames=21, audio_chunk_frames=3, on_event=lambda *a: None)[0]
    assert np.array_equal(piece.codes, whole.codes) and np.array_equal(piece.audio, whole.audio) and whole.audio.size > 8 * 1536


@pytest.mark.parametrize("key", ["+2", "+2@16k"])
def test_chunked_exact_decode_equals_one_shot(models, key):
    from conftest import tiny_request
    from qwen3tts import GenerationRequest
    B = models[key]
    spf = B.info.samples_per_frame
    req = GenerationRequest(**tiny_request(row=1), max_tokens=40)
    want = B.generate_batch([req], temperature=0.0, force_frames=21)[0]
    for chunk in (8, 3):
        ev = []
        got = B.generate_batch([req], temperature=0.0, force_frames=21, audio_chunk_frames=chunk,
                               on_event=lambda i, k, p: ev.append((k, p)))[0]
        assert np.array_equal(got.codes, want.codes) and np.array_equal(got.audio, want.audio), chunk
        assert got.audio.size == int((got.codes[:, 0] > 0).sum()) * spf > 8 * spf
        pieces = [p for k, p in ev if k == "audio_chunk"]
        assert [o for o, _ in pieces] == [k * chunk * spf for k in range(len(pieces))] and len(pieces) >= 2
        assert np.array_equal(np.concatenate([p for _, p in pieces]), got.audio)


def test_chunked_exact_decode_of_ragged_rows_in_row_groups(models):
    from conftest import tiny_request
    from qwen3tts import GenerationRequest, _lib
    B = models["+2@16k"]
    reqs = [GenerationRequest(**tiny_request(row=i, n_text=5 + i), max_tokens=c) for i, c in enumerate([30, 11, 22, 17])]
    kw = dict(temperature=0.9, top_k=40, seed=5)
    want = B.generate_batch(reqs, **kw)
    frames = [w.codes.shape[0] for w in want]
    assert max(frames) > 16 and len(set(frames)) > 1
    got = B.generate_batch(reqs, audio_chunk_frames=8, on_event=lambda *a: None, **kw)
    _lib.lib().q3tts_debug_set_codec_scratch(1 << 20)
    try:
        grouped = B.generate_batch(reqs, audio_chunk_frames=8, on_event=lambda *a: None, **kw)
    finally:
        _lib.lib().q3tts_debug_set_codec_scratch(0)
    for i in range(4):
        assert np.array_equal(got[i].codes, want[i].codes) and np.array_equal(got[i].audio, want[i].audio), i
        assert np.array_equal(grouped[i].audio, want[i].audio), i


@pytest.mark.parametrize("key", ["+2", "+2@16k"])
def test_slotted_stream_equals_each_request_streamed_alone(models, key):
    B = models[key]
    spf = B.info.samples_per_frame
    F = [9, 33, 20, 8, 17]
    c = _codes(B, F, 5)
    got = B.debug_codec_stream_slots(c, F, 2, 5, C_, W_, L_)
    for i, f in enumerate(F):
        alone = B.codec_decode_streamed(c[i:i + 1, :f], C_, W_, L_)[0]
        assert np.array_equal(got[i, :f * spf], alone[:f * spf]), i


def test_streamed_queue_equals_each_request_alone(models):
    from conftest import tiny_request
    from qwen3tts import GenerationRequest
    B = models["+2"]
    caps = [9, 33, 20, 8, 17]
    reqs = [GenerationRequest(**tiny_request(row=i, n_text=6 + i), max_tokens=c) for i, c in enumerate(caps)]
    kw = dict(temperature=0.9, top_k=50, seed=21)
    ev = []
    got = B.generate_queued(reqs, slots=2, on_event=lambda i, k, p: ev.append((i, k, p)), **kw, **STREAM)
    frames = [g.codes.shape[0] for g in got]
    assert any(f > C_ for f in frames)
    for i, r in enumerate(reqs):
        alone = B.generate_batch([r], row_base=i, **kw, **STREAM)[0]
        assert got[i].status == alone.status and np.array_equal(got[i].codes, alone.codes)
        assert np.array_equal(got[i].audio, alone.audio), i
        if frames[i] == 0:
            continue
        assert got[i].audio.size == frames[i] * 1920
        pieces = [p for (j, k, p) in ev if j == i and k == "audio_chunk"]
        assert [o for o, _ in pieces] == [k * C_ * 1920 for k in range(-(-frames[i] // C_))], i
        assert np.array_equal(np.concatenate([p for _, p in pieces]), got[i].audio), i


@pytest.fixture(scope="module")
def base_models(tmp_path_factory):
    from qwen3tts import Qwen3TTSModel, synth
    d = str(tmp_path_factory.mktemp("pitch_base") / "tiny-base")
    synth.write_checkpoint(d, "tiny-base", seed=4321)
    kw = dict(max_batch=4, max_frames=64, max_prompt=160)
    out = {"A": Qwen3TTSModel.from_pretrained(d, **kw), "+2": Qwen3TTSModel.from_pretrained(d, pitch=2.0, **kw)}
    yield out
    for m in out.values():
        m.close()


def test_a_saved_prefix_state_at_a_pitch(base_models):
    """One streamed voice served twice on the pitched handle -- first decoding its reference, then from the saved state: equal
    results. The state is larger than the default handle's by the margins of the three tensors the two stages add: out_conv's
    24 kHz signal (3 frames x 1920 samples x 4 bytes), the state word's tensor (3 x 16 bytes) and the stretched signal in front
    of the resampler (3 frames x 4 * 539 samples x 4 bytes)."""
    from qwen3tts import GenerationRequest, synth

    def prompt(row, n_text=10):
        return synth.synthetic_prompt(row, n_text=n_text, text_vocab=1000, im_start=1000, im_end=1001)

    clip, ids = synth.synthetic_reference_audio(1, 1.0), prompt(1)["ref_text_ids"]
    p = prompt(2, 9)
    kw = dict(audio_stream_reference=1, temperature=0.9, top_k=40, repetition_penalty=1.5, seed=77, **STREAM)
    grown = {}
    for key in ("A", "+2"):
        m = base_models[key]
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
            grown[key] = b1 - b0
    assert grown["+2"] - grown["A"] == 3 * 1920 * 4 + 3 * 16 + 3 * 4 * 539 * 4


# ---- 9. a pitch of 0, and one whose Hp equals Ho, are the handle without the field ---------------------------------------------
def test_pitch_zero_and_hp_equal_ho_are_the_default_decode(ckpt_dirs, models, codes):
    from qwen3tts import Qwen3TTSModel, _lib
    o = _lib.LoadOptsEx()
    _lib.lib().q3tts_default_load_opts_ex(C.byref(o))
    assert o.pitch == 0.0
    A = models["A"]
    want, want_lens = A.codec_decode(codes, n_frames=F_ROWS)
    want_stream = A.codec_decode_streamed(codes, 8, -1, n_frames=F_ROWS)
    assert choose_hp(480, 0.001) == 480 and choose_hp(480, -0.0015) == 480
    for pitch in (0.0, 0.001, -0.0015):
        Z = Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], pitch=pitch, **LOAD)
        try:
            assert Z.pitch_info() == (0.0, 480, 480, 0) == A.pitch_info()
            assert (Z.speed, Z.stretch_hs, Z.sample_rate, Z.info.samples_per_frame, Z.info.max_samples_per_frame) == (1.0, 480, 24000, 1920, 1920)
            assert Z.debug_prefix_states() == A.debug_prefix_states()
            pcm, lens = Z.codec_decode(codes, n_frames=F_ROWS)
            assert pcm.tobytes() == want.tobytes() and np.array_equal(lens, want_lens)
            assert Z.codec_decode_streamed(codes, 8, -1, n_frames=F_ROWS).tobytes() == want_stream.tobytes()
        finally:
            Z.close()
    # ... and with a speed and an output rate: Hp == Ho == 384 is the speed's handle
    S = models["1.25"]
    Z = Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], pitch=0.001, speed=1.25, **LOAD)
    try:
        assert Z.pitch_info() == (0.0, 384, 384, 0) and Z.info.samples_per_frame == 1536
        assert Z.codec_decode(codes, n_frames=F_ROWS)[0].tobytes() == S.codec_decode(codes, n_frames=F_ROWS)[0].tobytes()
    finally:
        Z.close()


# ---- 10. refusals, and the command line ------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_usable(models, ckpt_dirs, pitch_driver, tmp_path):
    from qwen3tts import Qwen3TTSModel, _lib as L
    from qwen3tts.model import Qwen3TTSError
    m = models["A"]
    x = seeded_signal(1500, 3)
    ref = header_shift(pitch_driver, tmp_path, 509, 509, 480, x, causal=False)

    def good():
        assert np.array_equal(m.pitch_shift(x, 1.0), ref)

    good()
    for bad in (12.001, -12.001, 100.0, float("nan"), float("inf"), float("-inf")):
        with pytest.raises(Qwen3TTSError) as e:
            m.pitch_shift(x, bad)
        assert e.value.status == 3
        good()
    xn = x.copy()
    xn[700] = np.nan
    with pytest.raises(Qwen3TTSError) as e:
        m.pitch_shift(xn, 1.0)
    assert e.value.status == 3
    good()
    out = np.zeros(ref.size - 1, np.float32)  # one sample short
    n = C.c_int64(0)
    st = m._lib.q3tts_pitch_shift(m._h, x.ctypes.data_as(L.f32p), x.size, 1.0, out.ctypes.data_as(L.f32p), out.size, C.byref(n))
    assert st == 3 and n.value == ref.size and not out.any()
    good()
    for kw in (dict(pitch=12.5), dict(pitch=float("nan")), dict(pitch=float("inf")), dict(pitch=2.0, request_speeds=True),
               dict(pitch=12.0, speed=0.8), dict(pitch=-1.0, speed=2.0), dict(pitch=2.0, output_sample_rate=11025)):
        with pytest.raises(Qwen3TTSError) as e:
            Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], **kw, **LOAD)
        assert e.value.status == 3, kw
    good()


def test_a_codec_frame_that_is_not_whole_hops_refuses_a_pitch(tmp_path):
    """upsample_rates 8 x 5 x 4 x 2 behind the 2 x 2 stages: 1280 samples per frame, not a multiple of 480. The handle loads and
    decodes as before; a pitch is INVALID_INPUT at load, a pitch of 0 is not."""
    import json
    from qwen3tts import Qwen3TTSModel, synth
    from qwen3tts.model import Qwen3TTSError
    d = str(tmp_path / "frame1280")
    p = synth.preset("tiny-b")
    p["speech_tokenizer"]["decoder_config"]["upsample_rates"] = [8, 5, 4, 2]
    os.makedirs(os.path.join(d, "speech_tokenizer"))
    g = synth._Gen(1234, False)
    json.dump(p["config"], open(os.path.join(d, "config.json"), "w"))
    json.dump(p["speech_tokenizer"], open(os.path.join(d, "speech_tokenizer", "config.json"), "w"))
    synth.save_safetensors(os.path.join(d, "model.safetensors"), synth.talker_tensors(p["config"], g))
    synth.save_safetensors(os.path.join(d, "speech_tokenizer", "model.safetensors"), synth.codec_tensors(p["speech_tokenizer"]["decoder_config"], g))
    for pitch in (2.0, -12.0):
        with pytest.raises(Qwen3TTSError) as e:
            Qwen3TTSModel.from_pretrained(d, pitch=pitch, **LOAD)
        assert e.value.status == 3 and "480-sample hops" in str(e.value)
    Z = Qwen3TTSModel.from_pretrained(d, pitch=0.0, **LOAD)
    try:
        assert Z.info.samples_per_frame == 1280 and Z.pitch_info() == (0.0, 480, 480, 0)
        pcm, lens = Z.codec_decode(_codes(Z, [5], 3))
        assert pcm.shape == (1, 5 * 1280) and np.isfinite(pcm).all()
    finally:
        Z.close()


def test_cli_with_a_pitch(tmp_path, capsys):
    import re
    from qwen3tts import synth
    from qwen3tts.__main__ import main
    d = str(tmp_path / "model")
    synth.write_checkpoint(d, "tiny-b", seed=1234)
    shutil.copy(os.path.join(GOLD, "tokenizer.json"), os.path.join(d, "tokenizer.json"))
    out = str(tmp_path / "out.wav")
    rc = main(["--model", d, "--text", "Hello there, it's a test.", "--speaker", "aiden", "--language", "english", "--temperature", "0",
               "--max-tokens", "9", "--output", out, "--pitch", "2"])
    assert rc == 0
    text = capsys.readouterr().out
    L2, M2, K2 = ratio(539, 480, 1, 1)
    assert "Pitch: +2.0070 semitones (hop 539 resampled to 480, delay %d samples)" % delay_out(539, L2, M2, K2) in text
    n = int(re.search(r"Generated (\d+) samples", text).group(1))
    raw = open(out, "rb").read()
    assert struct.unpack("<IHHIIHH", raw[16:36]) == (16, 1, 1, 24000, 48000, 2, 16)
    assert struct.unpack("<I", raw[40:44])[0] == 2 * n == len(raw) - 44
    assert n > 0 and n % 1920 == 0
