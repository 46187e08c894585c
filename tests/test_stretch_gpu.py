"""The time stretch on the device (csrc/kernels/stretch.hip): q3tts_time_stretch against the definition, exactly; the decoder
at a speed (q3tts_load_opts.speed) against the definition applied to the default handle's 24 kHz decode; the stream, queue and
prefix-state guarantees at a speed; speed together with an output rate; the default handle unchanged; refusals.

The reference is the NumPy restatement of tests/test_stretch_plan.py (pinned there against the header's stretch_reference).
Equality is exact throughout: every output has one arithmetic order and the choice of d is a total order."""
import ctypes as C
import os
import shutil
import struct

import numpy as np
import pytest

from test_resample_plan import apply, driver, fp32_bound, header_table  # noqa: F401  (driver: the resampler header's, a fixture)
from test_stretch_plan import HS_CASES, LENGTHS, choose_hs, delay, out_len, seeded_signal, stretch

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not shutil.which("g++"), reason="g++ is not installed")]

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LOAD = dict(max_batch=4, max_frames=96, max_prompt=96)
C_, W_, L_ = 8, 32, 4
STREAM = dict(audio_chunk_frames=C_, audio_window_frames=W_, audio_lookahead_frames=L_)
F_ROWS = [37, 5, 22]    # the stream guarantees (device against device)
F_SHORT = [11, 3, 6]    # the definition (the restatement walks every hop in NumPy)
SPEEDS = {1.25: 384, 0.8: 600}


@pytest.fixture(scope="module")
def models(ckpt_dirs):
    """tiny-b handles: "A" default, one per speed of SPEEDS, and 1.25 at 16 kHz."""
    from qwen3tts import Qwen3TTSModel
    out = {"A": Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], **LOAD)}
    for s in SPEEDS:
        out[s] = Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], speed=s, **LOAD)
    out["1.25@16k"] = Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], speed=1.25, output_sample_rate=16000, **LOAD)
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
    c = _codes(models["A"], F_SHORT, 12)
    c[0, 4, 0] = 0
    pcm, lens = models["A"].codec_decode(c, n_frames=F_SHORT)
    pcm.setflags(write=False)
    return c, pcm, lens


# ---- 1. q3tts_time_stretch against the definition ------------------------------------------------------------------------
@pytest.mark.parametrize("hs", HS_CASES)
def test_time_stretch_equals_the_definition(models, hs):
    m = models["A"]
    speed = 480.0 / hs
    assert choose_hs(speed) == hs
    for n in LENGTHS:
        x = seeded_signal(n, 1000 + n)
        for causal in (False, True):
            got = m.time_stretch(x, speed, causal=causal)
            want, _, _ = stretch(x, hs, causal)
            assert got.size == out_len(n, hs, causal) == want.size
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (hs, n, causal)
    # six frames, with the diagnostic: hops whose best and runner-up c are closer than the fp32 accumulation bound allows to
    # tell apart (each of the Hs fmafs rounds once, every partial sum is at most sum |terms|). Reported, not asserted: the
    # choice is defined on the fp32 values, and equality is required regardless.
    x = seeded_signal(6 * 1920, 77)
    st = {}
    want, _, ds = stretch(x, hs, True, stats=st)
    got = m.time_stretch(x, speed, causal=True)
    undecidable = sum(1 for g, mag in zip(st["gap"], st["mag"]) if g < 2.0 * hs * 2.0 ** -24 * mag)
    print("Hs %d: %d of %d hops undecidable within the fp32 accumulation bound; d = %s" % (hs, undecidable, len(ds), ds))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_refusals_leave_the_engine_usable(models, ckpt_dirs):
    from qwen3tts import Qwen3TTSModel, _lib as L
    from qwen3tts.model import Qwen3TTSError
    m = models["A"]
    x = seeded_signal(1500, 3)
    ref, _, _ = stretch(x, 384, False)

    def good():
        assert np.array_equal(m.time_stretch(x, 1.25), ref)

    good()
    for bad in (0.0, 0.4999, 2.0001, -1.0, float("nan"), float("inf"), float("-inf")):
        with pytest.raises(Qwen3TTSError) as e:
            m.time_stretch(x, bad)
        assert e.value.status == 3
        good()
    xn = x.copy()
    xn[700] = np.nan
    with pytest.raises(Qwen3TTSError) as e:
        m.time_stretch(xn, 1.25)
    assert e.value.status == 3
    good()
    out = np.zeros(ref.size - 1, np.float32)  # one sample short
    n = C.c_int64(0)
    st = m._lib.q3tts_time_stretch(m._h, x.ctypes.data_as(L.f32p), x.size, 1.25, 0, out.ctypes.data_as(L.f32p), out.size, C.byref(n))
    assert st == 3 and n.value == ref.size and not out.any()
    good()
    for bad in (0.3, 2.5, -1.0, float("nan"), float("inf")):
        with pytest.raises(Qwen3TTSError) as e:
            Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], speed=bad, **LOAD)
        assert e.value.status == 3
    good()


# ---- 2. the decoder at a speed -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("speed", sorted(SPEEDS))
def test_decoder_at_a_speed_is_the_definition(models, short, speed):
    hs = SPEEDS[speed]
    B = models[speed]
    spf = 4 * hs
    assert B.stretch_hs == hs and abs(B.speed - 480.0 / hs) < 1e-6 and B.stretch_delay_samples == delay(hs)
    assert B.sample_rate == 24000 and B.info.samples_per_frame == spf
    A = models["A"]
    assert (A.speed, A.stretch_hs, A.stretch_delay_samples, A.info.samples_per_frame) == (1.0, 480, 0, 1920)
    c, pcm24, lens24 = short
    got, lens = B.codec_decode(c, n_frames=F_SHORT)
    assert got.shape == (3, max(F_SHORT) * spf)
    for b, f in enumerate(F_SHORT):  # ragged rows
        want, _, _ = stretch(pcm24[b, :f * 1920], hs, True)
        assert want.size == f * spf
        assert np.array_equal(got[b, :f * spf].view(np.uint32), want.view(np.uint32)), (speed, b)
        assert lens[b] == int((c[b, :f, 0] > 0).sum()) * spf and lens24[b] * spf == lens[b] * 1920
        assert np.abs(got[b, :f * spf]).max() <= 1.0
    assert lens[0] == (F_SHORT[0] - 1) * spf


def test_speed_with_an_output_rate_is_the_resampler_on_the_stretched_signal(models, driver, codes):
    """1.25 at 16 kHz: Hs = 384 again (a multiple of 3), 4 * 384 * 2 / 3 = 1024 samples per frame; the PCM is the causal
    resampler's definition (its own fp32 accumulation bound) applied to the 1.25 handle's 24 kHz PCM, which test 2 pins."""
    B, S = models["1.25@16k"], models[1.25]
    assert (B.stretch_hs, B.sample_rate, B.info.samples_per_frame) == (384, 16000, 1024)
    Lr, Mr, K, tab32 = header_table(driver, 24000, 16000)
    mid, _ = S.codec_decode(codes, n_frames=F_ROWS)
    got, lens = B.codec_decode(codes, n_frames=F_ROWS)
    tol = fp32_bound(tab32, K, 1.0)
    for b, f in enumerate(F_ROWS):
        want = apply(tab32, Lr, Mr, K, mid[b, :f * 1536], centred=False, clamp=True)
        err = float(np.abs(got[b, :f * 1024] - want).max())
        print("row %d: max err %.3g, bound %.3g" % (b, err, tol))
        assert want.size == f * 1024 and err <= tol
        assert lens[b] == int((codes[b, :f, 0] > 0).sum()) * 1024


# ---- 3. the stream guarantees carry over, bit for bit ------------------------------------------------------------------------
@pytest.mark.parametrize("key", [1.25, 0.8, "1.25@16k"])
@pytest.mark.parametrize("chunk", [3, 8, 16])
def test_streamed_decode_equals_one_shot(models, codes, chunk, key):
    B = models[key]
    spf = B.info.samples_per_frame
    want, _ = B.codec_decode(codes, n_frames=F_ROWS)
    got = B.codec_decode_streamed(codes, chunk, -1, n_frames=F_ROWS)
    for b, f in enumerate(F_ROWS):
        assert np.array_equal(got[b, :f * spf], want[b, :f * spf]), (chunk, b)


@pytest.mark.parametrize("key", [1.25, "1.25@16k"])
def test_chunked_exact_decode_equals_one_shot(models, key):
    """AUDIO_CHUNK pieces cut from the exact decode behind the last token (audio_window_frames == 0: decode_chunked, which
    carries the stage's state word -- and the resampler's input behind it -- from chunk to chunk)."""
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
    """Four rows of different lengths through decode_chunked, whole and with a scratch budget so short that every row is a group
    of its own: the carried state word and the carried resampler input are per row, whatever the grouping."""
    from conftest import tiny_request
    from qwen3tts import GenerationRequest, _lib
    B = models["1.25@16k"]
    reqs = [GenerationRequest(**tiny_request(row=i, n_text=5 + i), max_tokens=c) for i, c in enumerate([30, 11, 22, 17])]
    kw = dict(temperature=0.9, top_k=40, seed=5)
    want = B.generate_batch(reqs, **kw)
    frames = [w.codes.shape[0] for w in want]
    print("frames", frames)
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


def test_prefixed_stream_without_a_prefix_is_the_plain_stream(models, codes):
    B = models[1.25]
    plain = B.codec_decode_streamed(codes, C_, W_, L_, n_frames=F_ROWS)
    pre = B.codec_decode_streamed_prefixed(codes, [0, 0, 0], F_ROWS, C_, W_, L_)
    for b, f in enumerate(F_ROWS):
        assert np.array_equal(pre[b, :f * 1536], plain[b, :f * 1536]), b


@pytest.mark.parametrize("key", [0.8, "1.25@16k"])
def test_slotted_stream_equals_each_request_streamed_alone(models, key):
    """The queue's slotted stream without the talker: 5 requests of 9 / 33 / 20 / 8 / 17 frames on 2 slots -- a new request takes
    a row whose state word its predecessor left behind, bystander rows keep theirs."""
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
    B = models[1.25]
    caps = [9, 33, 20, 8, 17]
    reqs = [GenerationRequest(**tiny_request(row=i, n_text=6 + i), max_tokens=c) for i, c in enumerate(caps)]
    kw = dict(temperature=0.9, top_k=50, seed=21)
    ev = []
    got = B.generate_queued(reqs, slots=2, on_event=lambda i, k, p: ev.append((i, k, p)), **kw, **STREAM)
    frames = [g.codes.shape[0] for g in got]
    print("frames", frames)
    assert any(f > C_ for f in frames)
    for i, r in enumerate(reqs):
        alone = B.generate_batch([r], row_base=i, **kw, **STREAM)[0]
        assert got[i].status == alone.status and np.array_equal(got[i].codes, alone.codes)
        assert np.array_equal(got[i].audio, alone.audio), i
        if frames[i] == 0:
            continue
        assert got[i].audio.size == frames[i] * 1536
        pieces = [p for (j, k, p) in ev if j == i and k == "audio_chunk"]
        assert [o for o, _ in pieces] == [k * C_ * 1536 for k in range(-(-frames[i] // C_))], i
        assert np.array_equal(np.concatenate([p for _, p in pieces]), got[i].audio), i


# ---- 4. speed 0 and 1.0 are the handle without the field -----------------------------------------------------------------
def test_speed_zero_and_one_are_the_default_decode(ckpt_dirs, models, codes):
    from qwen3tts import Qwen3TTSModel, _lib
    o = _lib.LoadOpts()
    _lib.lib().q3tts_default_load_opts(C.byref(o))
    assert o.speed == 0.0 and o.output_sample_rate == 0
    want, want_lens = models["A"].codec_decode(codes, n_frames=F_ROWS)
    for speed in (0.0, 1.0):
        Z = Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], speed=speed, **LOAD)
        try:
            assert (Z.speed, Z.stretch_hs, Z.sample_rate, Z.info.samples_per_frame) == (1.0, 480, 24000, 1920)
            pcm, lens = Z.codec_decode(codes, n_frames=F_ROWS)
            assert pcm.tobytes() == want.tobytes() and np.array_equal(lens, want_lens)
            got = Z.codec_decode_streamed(codes, 8, -1, n_frames=F_ROWS)
            for b, f in enumerate(F_ROWS):
                assert np.array_equal(got[b, :f * 1920], pcm[b, :f * 1920])
        finally:
            Z.close()


# ---- 5. a voice's saved prefix state (a Base checkpoint: tiny-b has no voice-clone front end) ------------------------------
@pytest.fixture(scope="module")
def base_models(tmp_path_factory):
    from qwen3tts import Qwen3TTSModel, synth
    d = str(tmp_path_factory.mktemp("stretch_base") / "tiny-base")
    synth.write_checkpoint(d, "tiny-base", seed=4321)
    kw = dict(max_batch=4, max_frames=64, max_prompt=160)
    out = {"A": Qwen3TTSModel.from_pretrained(d, **kw), 1.25: Qwen3TTSModel.from_pretrained(d, speed=1.25, **kw)}
    yield out
    for m in out.values():
        m.close()


def _prompt(row, n_text=10):
    from qwen3tts import synth
    return synth.synthetic_prompt(row, n_text=n_text, text_vocab=1000, im_start=1000, im_end=1001)


def test_a_saved_prefix_state_at_a_speed(base_models):
    """One streamed voice served twice on the 1.25 handle -- first decoding its reference, then from the saved state: equal
    results. The state is larger than the default handle's by the margins of the two tensors the stage adds: out_conv's 24 kHz
    signal (3 frames x 1920 samples x 4 bytes) and the state word's tensor (3 frames x 16 bytes)."""
    from qwen3tts import GenerationRequest, synth
    clip, ids = synth.synthetic_reference_audio(1, 1.0), _prompt(1)["ref_text_ids"]
    p = _prompt(2, 9)
    kw = dict(audio_stream_reference=1, temperature=0.9, top_k=40, repetition_penalty=1.5, seed=77, **STREAM)
    grown = {}
    for key, spf in (("A", 1920), (1.25, 1536)):
        m = base_models[key]
        with m.create_voice(clip, ids) as v:
            r = GenerationRequest(p["text_ids"], p["target_token_count"], None, None, "english", 10, voice=v)
            n0, b0, r0 = m.debug_prefix_states()
            first = m.generate_queued([r], slots=1, **kw)[0]
            n1, b1, r1 = m.debug_prefix_states()
            again = m.generate_queued([r], slots=1, **kw)[0]
            n2, b2, r2 = m.debug_prefix_states()
            assert (n1, r1) == (n0 + 1, r0) and (n2, b2, r2) == (n1, b1, r1 + 1)  # decoded and saved, then restored
            assert first.status == 0 and first.codes.shape[0] > 0 and first.audio.size == first.codes.shape[0] * spf
            assert np.array_equal(first.codes, again.codes) and np.array_equal(first.audio, again.audio)
            grown[key] = b1 - b0
    assert grown[1.25] - grown["A"] == 3 * 1920 * 4 + 3 * 16


# ---- 6. the command line -----------------------------------------------------------------------------------------------------
def test_cli_with_a_speed(tmp_path, capsys):
    import re
    from qwen3tts import synth
    from qwen3tts.__main__ import main
    d = str(tmp_path / "model")
    synth.write_checkpoint(d, "tiny-b", seed=1234)
    shutil.copy(os.path.join(GOLD, "tokenizer.json"), os.path.join(d, "tokenizer.json"))
    out = str(tmp_path / "out.wav")
    rc = main(["--model", d, "--text", "Hello there, it's a test.", "--speaker", "aiden", "--language", "english", "--temperature", "0",
               "--max-tokens", "9", "--output", out, "--speed", "1.5"])
    assert rc == 0
    text = capsys.readouterr().out
    assert "Speed: 1.5000x (synthesis hop 320, delay 80 samples)" in text
    n = int(re.search(r"Generated (\d+) samples", text).group(1))
    raw = open(out, "rb").read()
    assert struct.unpack("<IHHIIHH", raw[16:36]) == (16, 1, 1, 24000, 48000, 2, 16)
    assert struct.unpack("<I", raw[40:44])[0] == 2 * n == len(raw) - 44
    assert n > 0 and n % 1280 == 0
