"""The polyphase resampler on the device (csrc/kernels/resample.hip): q3tts_resample block parity for every supported pair, the
decoder at another output rate (q3tts_load_opts.output_sample_rate) against the definition applied to the 24 kHz decode, the
stream guarantees at that rate, and voices made from clips at their own rate.

The reference is the NumPy float64 restatement of tests/test_resample_plan.py on the header's fp32 table; the tolerance is the
fp32 accumulation bound computed from that table (fp32_bound), never a constant."""
import math
import os
import shutil
import struct

import numpy as np
import pytest

from test_resample_plan import PAIRS, apply, driver, fp32_bound, header_table, out_len  # noqa: F401  (driver: a fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not shutil.which("g++"), reason="g++ is not installed")]

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LOAD = dict(max_batch=4, max_frames=96, max_prompt=96)
RATES = (16000, 44100)  # 16000: the telephony case; 44100: the largest L (147)
C_, W_, L_ = 8, 32, 4
STREAM = dict(audio_chunk_frames=C_, audio_window_frames=W_, audio_lookahead_frames=L_)
F_ROWS = [37, 5, 22]


@pytest.fixture(scope="module")
def models(ckpt_dirs):
    """tiny-b handles: "A" at the default rate, one per rate of RATES."""
    from qwen3tts import Qwen3TTSModel
    out = {"A": Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], **LOAD)}
    for r in RATES:
        out[r] = Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], output_sample_rate=r, **LOAD)
    yield out
    for m in out.values():
        m.close()


@pytest.fixture(scope="module")
def codes(models):
    rng = np.random.default_rng(11)
    hi = min(models["A"].info.cp_vocab_size, 2048)
    c = np.zeros((3, max(F_ROWS), 16), np.int32)
    for b, f in enumerate(F_ROWS):
        c[b, :f] = rng.integers(1, hi, size=(f, 16))
    c[0, [3, 30], 0] = 0  # two frames that the end trim does not count
    return c


@pytest.fixture(scope="module")
def native_pcm(models, codes):
    """The 24 kHz decode of `codes`, computed once and shared."""
    pcm, lens = models["A"].codec_decode(codes, n_frames=F_ROWS)
    pcm.setflags(write=False)
    return pcm, lens


# ---- 1. block parity through q3tts_resample ------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%d-%d" % p)
def test_resample_block_parity(models, driver, pair):
    m = models["A"]
    L, M, K, tab32 = header_table(driver, *pair)
    rng = np.random.default_rng(pair[0] + pair[1])
    for n in (1, 2 * K - 1, 2 * K, 4097, 1920):  # edge zero-fill, a tile boundary, a partial last workgroup, one frame
        x = (0.1 * rng.standard_normal(n)).astype(np.float32)
        for centred in (True, False):
            got = m.resample(x, pair[0], pair[1], centred=centred)
            want = apply(tab32, L, M, K, x, centred)
            tol = fp32_bound(tab32, K, float(np.abs(x).max()))
            err = float(np.abs(got - want).max())
            print("%d->%d n=%d %s: max err %.3g, bound %.3g" % (pair[0], pair[1], n, "centred" if centred else "causal", err, tol))
            assert got.size == out_len(n, L, M) and err <= tol, (pair, n, centred, err, tol)


def test_resample_refusals_leave_the_engine_usable(models, driver):
    from qwen3tts import _lib as L_
    from qwen3tts.model import Qwen3TTSError
    import ctypes as C
    m = models["A"]
    x = (0.1 * np.random.default_rng(2).standard_normal(500)).astype(np.float32)
    L, M, K, tab32 = header_table(driver, 24000, 16000)

    def good():
        got = m.resample(x, 24000, 16000)
        assert np.abs(got - apply(tab32, L, M, K, x, True)).max() <= fp32_bound(tab32, K, float(np.abs(x).max()))

    good()
    for bad in ((24000, 11025), (16000, 48000), (24000, 24000), (0, 24000)):
        with pytest.raises(Qwen3TTSError) as e:
            m.resample(x, *bad)
        assert e.value.status == 3
        good()
    xn = x.copy()
    xn[250] = np.nan
    with pytest.raises(Qwen3TTSError) as e:
        m.resample(xn, 24000, 16000)
    assert e.value.status == 3
    good()
    out = np.zeros(out_len(x.size, L, M) - 1, np.float32)  # one sample short
    n = C.c_int64(0)
    st = m._lib.q3tts_resample(m._h, x.ctypes.data_as(L_.f32p), x.size, 24000, 16000, 1, out.ctypes.data_as(L_.f32p), out.size, C.byref(n))
    assert st == 3 and n.value == out_len(x.size, L, M) and not out.any()
    good()


# ---- 2. the decoder at another rate ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
def test_decoder_at_another_rate_is_the_definition(models, driver, codes, native_pcm, rate):
    B = models[rate]
    spf = 1920 * rate // 24000
    assert B.sample_rate == rate and B.info.samples_per_frame == spf
    assert models["A"].sample_rate == 24000 and models["A"].info.samples_per_frame == 1920
    L, M, K, tab32 = header_table(driver, 24000, rate)
    pcm24, lens24 = native_pcm
    got, lens = B.codec_decode(codes, n_frames=F_ROWS)
    assert got.shape == (3, max(F_ROWS) * spf)
    tol = fp32_bound(tab32, K, 1.0)
    for b, f in enumerate(F_ROWS):
        want = apply(tab32, L, M, K, pcm24[b, :f * 1920], centred=False, clamp=True)
        err = float(np.abs(got[b, :f * spf] - want).max())
        print("rate %d row %d: max err %.3g, bound %.3g" % (rate, b, err, tol))
        assert want.size == f * spf and err <= tol, (rate, b, err, tol)
        assert lens[b] == int((codes[b, :f, 0] > 0).sum()) * spf and lens24[b] * spf == lens[b] * 1920
    assert lens[0] == (F_ROWS[0] - 2) * spf


# ---- 3. the stream guarantees carry over, bit for bit ------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [3, 8, 16])
def test_streamed_decode_equals_one_shot_at_16k(models, codes, chunk):
    B = models[16000]
    want, _ = B.codec_decode(codes, n_frames=F_ROWS)
    got = B.codec_decode_streamed(codes, chunk, -1, n_frames=F_ROWS)
    for b, f in enumerate(F_ROWS):
        assert np.array_equal(got[b, :f * 1280], want[b, :f * 1280]), (chunk, b)


def test_chunked_delivery_equals_one_shot_at_16k(models):
    """AUDIO_CHUNK pieces cut from the exact decode behind the last token (audio_window_frames == 0: decode_chunked)."""
    from conftest import tiny_request
    from qwen3tts import GenerationRequest
    B = models[16000]
    req = GenerationRequest(**tiny_request(row=1), max_tokens=40)
    want = B.generate_batch([req], temperature=0.0, force_frames=21)[0]
    ev = []
    got = B.generate_batch([req], temperature=0.0, force_frames=21, audio_chunk_frames=8, on_event=lambda i, k, p: ev.append((k, p)))[0]
    assert np.array_equal(got.codes, want.codes) and np.array_equal(got.audio, want.audio)
    assert got.audio.size == int((got.codes[:, 0] > 0).sum()) * 1280 > 8 * 1280  # the end trim, in output samples
    pieces = [p for k, p in ev if k == "audio_chunk"]
    assert [o for o, _ in pieces] == [k * 8 * 1280 for k in range(len(pieces))] and len(pieces) >= 2
    assert np.array_equal(np.concatenate([p for _, p in pieces]), got.audio)


def test_prefixed_stream_without_a_prefix_is_the_plain_stream_at_16k(models, codes):
    B = models[16000]
    plain = B.codec_decode_streamed(codes, C_, W_, L_, n_frames=F_ROWS)
    pre = B.codec_decode_streamed_prefixed(codes, [0, 0, 0], F_ROWS, C_, W_, L_)
    for b, f in enumerate(F_ROWS):
        assert np.array_equal(pre[b, :f * 1280], plain[b, :f * 1280]), b


def test_slotted_stream_at_16k_equals_each_request_streamed_alone(models):
    """The queue's slotted stream without the talker: 5 requests of 9 / 33 / 20 / 8 / 17 frames on 2 slots."""
    B = models[16000]
    F = [9, 33, 20, 8, 17]
    rng = np.random.default_rng(5)
    hi = min(B.info.cp_vocab_size, 2048)
    c = np.zeros((5, max(F), 16), np.int32)
    for i, f in enumerate(F):
        c[i, :f] = rng.integers(1, hi, size=(f, 16))
    got = B.debug_codec_stream_slots(c, F, 2, 5, C_, W_, L_)
    for i, f in enumerate(F):
        alone = B.codec_decode_streamed(c[i:i + 1, :f], C_, W_, L_)[0]
        assert np.array_equal(got[i, :f * 1280], alone[:f * 1280]), i


def test_streamed_queue_at_16k_equals_each_request_alone(models):
    """generate_queued streamed with (8, 32, 4), 5 requests on 2 slots with caps of 9 / 33 / 20 / 8 / 17 frames: each request
    equals itself generated alone, AUDIO_CHUNK k sits at k * 8 * 1280 and the pieces concatenate to AUDIO. (force_frames is
    call-wide, so the lengths are set through max_tokens; a request may end below its cap.)"""
    from conftest import tiny_request
    from qwen3tts import GenerationRequest
    B = models[16000]
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
        assert got[i].audio.size == frames[i] * 1280
        pieces = [p for (j, k, p) in ev if j == i and k == "audio_chunk"]
        assert [o for o, _ in pieces] == [k * C_ * 1280 for k in range(-(-frames[i] // C_))], i
        assert np.array_equal(np.concatenate([p for _, p in pieces]), got[i].audio), i


# ---- 4. output_sample_rate = 0 is the handle without the field -------------------------------------------------------------
def test_rate_zero_and_24000_are_the_native_decode(ckpt_dirs, models, codes, native_pcm):
    from qwen3tts import Qwen3TTSModel, _lib
    import ctypes as C
    o = _lib.LoadOpts()
    _lib.lib().q3tts_default_load_opts(C.byref(o))
    assert o.output_sample_rate == 0
    for rate in (0, 24000):
        Z = Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], output_sample_rate=rate, **LOAD)
        try:
            assert Z.sample_rate == 24000 and Z.info.samples_per_frame == 1920
            pcm, lens = Z.codec_decode(codes, n_frames=F_ROWS)
            assert np.array_equal(pcm, native_pcm[0]) and np.array_equal(lens, native_pcm[1])
            got = Z.codec_decode_streamed(codes, 8, -1, n_frames=F_ROWS)
            for b, f in enumerate(F_ROWS):
                assert np.array_equal(got[b, :f * 1920], pcm[b, :f * 1920])
        finally:
            Z.close()
    from qwen3tts.model import Qwen3TTSError
    with pytest.raises(Qwen3TTSError) as e:
        Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], output_sample_rate=11025, **LOAD)
    assert e.value.status == 3


# ---- 5. voices, and the saved prefix state (a Base checkpoint: tiny-b has no voice-clone front end) -------------------------------
@pytest.fixture(scope="module")
def base_models(tmp_path_factory):
    from qwen3tts import Qwen3TTSModel, synth
    d = str(tmp_path_factory.mktemp("resample_base") / "tiny-base")
    synth.write_checkpoint(d, "tiny-base", seed=4321)
    kw = dict(max_batch=4, max_frames=64, max_prompt=160)
    out = {"A": Qwen3TTSModel.from_pretrained(d, **kw), 16000: Qwen3TTSModel.from_pretrained(d, output_sample_rate=16000, **kw)}
    yield out
    for m in out.values():
        m.close()


def _prompt(row, n_text=10):
    from qwen3tts import synth
    return synth.synthetic_prompt(row, n_text=n_text, text_vocab=1000, im_start=1000, im_end=1001)


def test_a_voice_from_a_16k_clip(base_models):
    from qwen3tts import GenerationRequest, synth
    m = base_models["A"]
    clip16k = synth.synthetic_reference_audio(1, 1.0)[:12000]  # any waveform will do: it is declared to be 16 kHz
    ids = _prompt(1)["ref_text_ids"]
    p = _prompt(3, 9)

    def gen(v):
        r = GenerationRequest(p["text_ids"], p["target_token_count"], None, None, "english", 12, voice=v)
        return m.generate_batch([r], temperature=0.0, repetition_penalty=1.5, force_frames=10)[0]

    with m.create_voice(clip16k, ids, sample_rate=16000) as at_rate, \
            m.create_voice(m.resample(clip16k, 16000, 24000), ids) as by_hand, m.create_voice(clip16k, ids) as as_24k:
        assert at_rate.info.n_ref_samples == math.ceil(clip16k.size * 3 / 2) == by_hand.info.n_ref_samples
        assert at_rate.info.ref_frames == by_hand.info.ref_frames and as_24k.info.n_ref_samples == clip16k.size
        a, b, c = gen(at_rate), gen(by_hand), gen(as_24k)
        assert a.status == 0 and np.array_equal(a.codes, b.codes) and np.array_equal(a.audio, b.audio)
        assert as_24k.info.ref_frames != at_rate.info.ref_frames
        assert not (np.array_equal(a.codes, c.codes) and np.array_equal(a.audio, c.audio))
    from qwen3tts.model import Qwen3TTSError
    with pytest.raises(Qwen3TTSError) as e:
        m.create_voice(clip16k, ids, sample_rate=11025)
    assert e.value.status == 3


def test_a_saved_prefix_state_at_16k(base_models):
    """One streamed voice served twice on the 16 kHz handle -- first decoding its reference, then from the saved state: equal
    results, and the state is larger than the default handle's by the resampler's margin, 3 frames x 1920 samples x 4 bytes."""
    from qwen3tts import GenerationRequest, synth
    clip, ids = synth.synthetic_reference_audio(1, 1.0), _prompt(1)["ref_text_ids"]
    p = _prompt(2, 9)
    kw = dict(audio_stream_reference=1, temperature=0.9, top_k=40, repetition_penalty=1.5, seed=77, **STREAM)
    grown = {}
    for key, spf in (("A", 1920), (16000, 1280)):
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
    assert grown[16000] - grown["A"] == 3 * 1920 * 4


# ---- 6. the command line -----------------------------------------------------------------------------------------------------
def test_cli_writes_an_8k_wav(tmp_path, capsys):
    import re
    from qwen3tts import synth
    from qwen3tts.__main__ import main
    d = str(tmp_path / "model")
    synth.write_checkpoint(d, "tiny-b", seed=1234)
    shutil.copy(os.path.join(GOLD, "tokenizer.json"), os.path.join(d, "tokenizer.json"))
    out = str(tmp_path / "out.wav")
    rc = main(["--model", d, "--text", "Hello there, it's a test.", "--speaker", "aiden", "--language", "english", "--temperature", "0",
               "--max-tokens", "9", "--output", out, "--output-sample-rate", "8000"])
    assert rc == 0
    n = int(re.search(r"Generated (\d+) samples", capsys.readouterr().out).group(1))
    raw = open(out, "rb").read()
    assert struct.unpack("<IHHIIHH", raw[16:36]) == (16, 1, 1, 8000, 16000, 2, 16)
    assert struct.unpack("<I", raw[40:44])[0] == 2 * n == len(raw) - 44
    assert n > 0 and n % 640 == 0
