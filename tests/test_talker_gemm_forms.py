"""The tile-major gate/up forms of the decode GEMM (csrc/kernels/gemm_body.inc TM) and the switch that selects the forms before
them (Q3TTS_GEMM_PARENT_FORMS=1, kernels.h DebugEnv), through q3tts_debug_gemm as tests/test_gemm_block.py uses it.

Every case is one launch with the switch off and one with it on. The two outputs are compared bit for bit (`==` on the raw
bf16 / fp32 words, sentinel rows and columns included), and the default launch goes through test_gemm_block.check_output:
the float64 reference of that file under its bars (no bar is restated or widened here), sentinels intact, and the bits of a row
content equal in every launch that carries it.

Cases.
  * The small matrix: M 17 and 32 (a ragged and a full second row block), K 256 and 768, N 48 and (gate/up) 40 -- a ragged last
    gate/up tile pair --, and K 6144 for the hidden-state store without prologue (the CH = 6 form of down_proj); with and without
    the norm prologue, the residual, the bias and non-temporal weights. At these widths no workgroup carries several tiles, so both
    launches run the same kernels: what is checked is that the body every form shares computes what it did.
  * The wide gate/up cases reach the two tile-major kernels themselves (asserted through the reported geometry: two row blocks,
    NP 3 with two chunks per wave and non-temporal weights -- the 1.7B talker's launch --, NP 2 with one chunk per wave -- the code
    predictor's): K 1152 / 640 (ragged chunk counts: waves without a second / a first chunk) and K 2048 / 1024 (the real ones), at
    4120 / 2056 columns (a last workgroup with missing tiles) and at widths that divide evenly.
  * One generation on the tiny checkpoint, 2 rows x 6 frames: codes and PCM equal with the switch on and off."""
import numpy as np
import pytest

import test_gemm_block as gb
from conftest import tiny_request

SWITCH = "Q3TTS_GEMM_PARENT_FORMS"


def _set_switch(monkeypatch, on):
    from qwen3tts import _lib
    if on:
        monkeypatch.setenv(SWITCH, "1")
    else:
        monkeypatch.delenv(SWITCH, raising=False)
    _lib.reload_debug_env()


@pytest.fixture
def switch(monkeypatch):
    for k in gb.ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    yield lambda on: _set_switch(monkeypatch, on)
    _set_switch(monkeypatch, False)


def small_cases(epi):
    """The small matrix for one epilogue: (norm, case) pairs."""
    out = []
    for norm in (0, 1):
        for K in (256, 768) + ((6144,) if (epi == 3 and not norm) else ()):
            for M in (17, 32):
                for N in (48, 40) if epi == 2 else (48,):
                    for nt in (0, 1):
                        for bias in (False, True) if epi != 2 else (False,):
                            for resid in (False, True) if epi == 3 else (False,):
                                name = "k%d-m%d-n%d%s%s%s%s" % (K, M, N, "-norm" if norm else "", "-nt" if nt else "", "-bias" if bias else "",
                                                               "-resid" if resid else "")
                                out.append((norm, gb._case(name, K, M, N, nt=nt, bias=bias, resid=resid, ss_out=(epi == 3), pad=(M == 17))))
    return out


def wide_cases():
    """Gate/up launches of several tiles per workgroup: (case, tile-major expected with the switch off)."""
    out = []
    for K, N, nt in ((1152, 4120, 1), (2048, 4120, 1), (2048, 4128, 1), (640, 2056, 0), (1024, 2056, 0), (1024, 2064, 0)):
        for M in (17, 32):
            out.append((gb._case("gu-k%d-m%d-n%d%s" % (K, M, N, "-nt" if nt else ""), K, M, N, nt=nt, pad=(M == 17)), True))
    # neighbours that keep the chunk-major kernels: one row block, the other pairing of NP and non-temporal loads
    out.append((gb._case("gu-k1152-m16-n4120-nt", 1152, 16, 4120, nt=1), False))
    out.append((gb._case("gu-k1152-m32-n4120", 1152, 32, 4120, nt=0), False))
    out.append((gb._case("gu-k640-m32-n2056-nt", 640, 32, 2056, nt=1), False))
    return out


def seed_wide_weights(K):
    """test_gemm_block draws 4192 weight rows only for its own two wide K and 80 for every other, and caches them for the
    process: the real K of the two launches get 4192 rows here whatever an earlier test module left in the cache. Returns what
    the cache held, for the caller to put back."""
    before = {}
    for which in ("g", "u"):
        key = (K, 0, which)
        before[key] = gb._WEIGHTS.get(key)
        rng = np.random.default_rng(1000 * K + ord(which))
        gb._WEIGHTS[key] = dict(W=gb.f2b(rng.standard_normal((4192, K)) * 0.03))
    return before


def launch(m, p, c, epi, norm):
    """One q3tts_debug_gemm launch of case c on pool p, as test_gemm_block.run_case builds it."""
    d = gb.dims(c, epi)
    M, N, K = c["M"], c["N"], c["K"]
    rm = gb.rowmap(c)
    x = np.full((d["xrows"], K), gb.SENT, np.uint16)
    x[:M] = p.h[rm]
    y = np.full((d["yrows"], d["y_cols"]), gb.SENT, np.uint16)
    if c["resid"]:
        y[:M, :N] = p.h_old[rm][:, :N]
    kw = dict(x=x, y=y, M=M, epi=epi, N=N, W=p.wg["W"][:N], resid=int(c["resid"]), nt_weights=c["nt"])
    if epi == 2:
        kw.update(W_up=p.wu["W"][:N])
    if c["bias"]:
        kw.update(bias=p.bias[:N])
    if c["ss_out"]:
        kw.update(ss_out=gb.sent_f32((N // 16, d["ss_ld"])))
    if norm:
        ss_in = gb.sent_f32((p.ssc, d["ss_ld"])).copy()
        ss_in[:, :M] = p.P[rm].T
        kw.update(norm_w=p.norm_w, ss_in=ss_in, norm_dim=K, norm_eps=gb.EPS)
    return m.debug_gemm(**kw), rm, d


def both_ways(m, switch, epi, norm, c, stats, nmax=None):
    p = gb.pool(epi, norm, 0, c["K"], c["gain"], c["ssc"], nmax)
    switch(True)
    old, _, _ = launch(m, p, c, epi, norm)
    switch(False)
    new, rm, d = launch(m, p, c, epi, norm)
    assert (new["y"] == old["y"]).all(), (c["name"], "y differs from the parent form in %d elements" % int((new["y"] != old["y"]).sum()))
    if c["ss_out"]:
        assert (new["ss_out"].view(np.uint32) == old["ss_out"].view(np.uint32)).all(), (c["name"], "ss_out differs from the parent form")
    variant = (c["K"], c["gain"], c["ssc"], nmax) + gb.variant_of(c)
    gb.check_output(c["name"], p, c, rm, new["y"], new["ss_out"], d, variant, stats)
    return old, new


@pytest.mark.gpu
@pytest.mark.parametrize("epi", [0, 2, 3])
def test_small_matrix_equals_the_parent_forms_and_the_float64_block(gb_engines, switch, epi):
    stats = dict(worst=0.0, worst_ss=0.0, compared=0)
    cases = small_cases(epi)
    for norm, c in cases:
        old, new = both_ways(gb_engines, switch, epi, norm, c, stats)
        if c["K"] == 6144:
            assert (new["nw"], new["ch"], new["mbw"], new["ntw"]) == (8, 6, 1, c["nt"]), c["name"]
    print("talker gemm forms, epi %d: %d cases, %d outputs, worst |a - r| / bar = %.3f" % (epi, len(cases), stats["compared"], stats["worst"]))
    gb._POOLS.clear()


@pytest.mark.gpu
def test_tile_major_kernels_equal_the_parent_forms_and_the_float64_block(gb_engines, switch):
    from qwen3tts import _lib
    stats = dict(worst=0.0, worst_ss=0.0, compared=0)
    gb._POOLS.clear()   # (a pool built by an earlier test module holds that module's weights)
    before = {}
    for K in (1024, 2048):
        before.update(seed_wide_weights(K))
    try:
        for c, tm in wide_cases():
            old, new = both_ways(gb_engines, switch, 2, 1, c, stats, nmax=4192)
            assert new["np"] == old["np"] == (3 if c["N"] > 4096 else 2) and new["gx"] == old["gx"], c["name"]
            # which kernel ran: the geometry the launcher reports for these arguments, with and without the switch
            d = gb.dims(c, 2)
            g = dict(M=c["M"], K=c["K"], N=c["N"], xMB=d["xrows"] // 16, yMB=d["yrows"] // 16, ss_ld=d["ss_ld"], y_cols=d["y_cols"], epi=2,
                     nt_weights=c["nt"], norm=1, quant=0, ss_count=gb.default_ss_count(c["K"]), norm_dim=c["K"])
            assert bool(_lib.gemm_geometry(**g)["tm"]) == tm, c["name"]
            switch(True)
            assert _lib.gemm_geometry(**g)["tm"] == 0, c["name"]
            switch(False)
        print("talker gemm forms, tile-major: %d outputs, worst |a - r| / bar = %.3f" % (stats["compared"], stats["worst"]))
    finally:
        gb._POOLS.clear()
        for key, w in before.items():
            if w is None:
                gb._WEIGHTS.pop(key, None)
            else:
                gb._WEIGHTS[key] = w


def test_the_switch_selects_the_parent_forms_in_the_geometry(switch):
    """Host code only: the two 32-row gate/up launches of the frame step are tile-major by default and chunk-major with the switch;
    int4 weights, one row block and every other epilogue never are."""
    from qwen3tts import _lib
    base = dict(M=32, xMB=2, yMB=2, ss_ld=32, norm_dim=2048)
    talker = dict(base, K=2048, N=6144, y_cols=6144, epi=2, nt_weights=1, norm=1, quant=0, ss_count=128)
    predictor = dict(base, K=1024, N=3072, y_cols=3072, epi=2, nt_weights=0, norm=1, quant=0, ss_count=64)
    for on in (False, True):
        switch(on)
        for kw, np_, ch, gx in ((talker, 3, 2, 256), (predictor, 2, 1, 192)):
            g = _lib.gemm_geometry(**kw)
            assert (g["mbw"], g["nw"], g["ch"], g["np"], g["gx"]) == (2, 8, ch, np_, gx) and g["tm"] == (0 if on else 1)
            assert _lib.gemm_geometry(**dict(kw, quant=1))["tm"] == 0
            assert _lib.gemm_geometry(**dict(kw, M=16, xMB=1, yMB=1))["tm"] == 0
            assert _lib.gemm_geometry(**dict(kw, norm=0, ss_count=0))["tm"] == 0
        assert _lib.gemm_geometry(**dict(talker, epi=0, N=4096, y_cols=4096))["tm"] == 0


@pytest.fixture(scope="module")
def gb_engines(ckpt_dirs):
    from qwen3tts import Qwen3TTSModel
    m = Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-a"], max_batch=1, max_frames=8, max_prompt=16)
    yield m
    m.close()


@pytest.mark.gpu
def test_tiny_generation_is_equal_with_the_switch_on_and_off(ckpt_dirs, monkeypatch):
    """2 rows x 6 frames on the tiny checkpoint: codes and PCM bit-equal under either set of forms (the switch is read at load)."""
    from qwen3tts import GenerationRequest, Qwen3TTSModel, _lib
    reqs = []
    for row in range(2):
        r = tiny_request(row=row, n_text=9 + row)
        reqs.append(GenerationRequest(r["text_ids"], r["target_token_count"], r["instruct_ids"], r["speaker"], r["language"]))
    res = {}
    try:
        for on in (False, True):
            if on:
                monkeypatch.setenv(SWITCH, "1")
            else:
                monkeypatch.delenv(SWITCH, raising=False)
            m = Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], max_batch=2, max_frames=16, max_prompt=64)
            try:
                res[on] = m.generate_batch(reqs, temperature=0.9, top_k=40, repetition_penalty=1.05, seed=7, force_frames=6)
            finally:
                m.close()
    finally:
        monkeypatch.delenv(SWITCH, raising=False)
        _lib.reload_debug_env()
    for a, b in zip(res[False], res[True]):
        assert a.codes.shape == (6, 16) and (a.codes == b.codes).all()
        assert a.audio.size > 0 and a.audio.shape == b.audio.shape and (a.audio == b.audio).all()
