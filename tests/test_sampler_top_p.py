"""The sampler's top-p stage sorts and walks only the elements that are still finite (sampler.hip, stage 6) and reads its
parameters per row. Both must leave every token exactly where the oracle's full-width o_sample_token puts it: the grid below
walks the power-of-two edges of the compacted sort (1, 2, 50, 63, 64, 65, 1000 survivors) and the full path (top-k off), on
logits with many exact ties at the top-k threshold and inside the survivors."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS = 8
EOS = 2150
TOP_K = [1, 2, 50, 63, 64, 65, 1000, 0]
TOP_P = [0.05, 0.6, 0.95]
DRAWS = (0, 16, 160)
# (name, V, suppress range, eos, repetition flags): the talker's draw and the code predictor's
VOCABS = {"talker-3072": (3072, (3072 - 1024, 3072), EOS, True), "plain-2048": (2048, (0, 0), -1, False)}


def f2b(x):
    from qwen3tts import synth
    return synth.f32_to_bf16_bits(np.asarray(x, np.float32))


@pytest.fixture(scope="module")
def engine(ckpt_dirs):
    from qwen3tts import Qwen3TTSModel
    m = Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], max_batch=ROWS, max_frames=16, max_prompt=32)
    yield m
    m.close()


def _logits(V, eos, seed):
    """bf16 logits on a grid of 0.1 (many equal keys). exp(logit) is what top-p sums, unnormalised, so every row is shifted
    down by a different amount: the cumulative sum crosses 1 - top_p early in one row, deep inside the survivors in another
    and never in a third."""
    rng = np.random.default_rng(seed)
    x = np.round(rng.standard_normal((ROWS, V)) * 1.5, 1) - (2.0 + 1.5 * np.arange(ROWS))[:, None]
    if eos >= 0:
        x[ROWS - 2, eos] = -30.0      # EOS far below any top-k cut: saved before top-k, restored behind top-p
        x[ROWS - 1, :] = -np.inf      # nothing finite but EOS
        x[ROWS - 1, eos] = 1.0
    else:
        x[ROWS - 1, :] = -np.inf      # three finite elements, two of them equal
        x[ROWS - 1, [7, 900, 2047]] = [-0.5, -0.5, 0.25]
    return f2b(x)


def _oracle(logits, r, V, T, k, p, rep, seen, sup, eos, seed, row0, draw):
    from oracle import oracle as O
    return O.lib().o_sample_token(O._p16(logits[r]), V, C.c_float(T), k, C.c_float(p), C.c_float(rep),
                                  seen[r].ctypes.data_as(O.u8p) if seen is not None else None, sup[0], sup[1], eos, 0,
                                  C.c_uint64(seed), row0 + r, draw)


@pytest.mark.parametrize("T", [0.5, 1.0])
@pytest.mark.parametrize("p", TOP_P)
@pytest.mark.parametrize("vocab", sorted(VOCABS))
def test_top_p_grid_bit_exact(engine, vocab, p, T):
    """(one case per vocabulary, top-p and temperature: the oracle's top-k is quadratic in V, a few seconds for the 8 top-k
    values x 3 draws x 8 rows of a case)"""
    V, sup, eos, flags = VOCABS[vocab]
    logits = _logits(V, eos, seed=11 + V)
    seen = (np.random.default_rng(5).random((ROWS, V)) < 0.05).astype(np.uint8) if flags else None
    rep = 1.05 if flags else 1.0
    bad = []
    for k in TOP_K:
        for draw in DRAWS:
            got = engine.debug_sample(logits, temperature=T, top_k=k, top_p=p, repetition_penalty=rep, seed=77, seen=seen,
                                      suppress=sup, eos_id=eos, row0=3, draw=draw).tolist()
            exp = [_oracle(logits, r, V, T, k, p, rep, seen, sup, eos, 77, 3, draw) for r in range(ROWS)]
            if got != exp:
                bad.append((k, p, draw, got, exp))
    assert not bad, bad[:4]


@pytest.mark.parametrize("vocab", sorted(VOCABS))
def test_every_row_its_own_parameters(engine, vocab):
    """One launch, eight rows, eight different (top_k, top_p, T, seed): row r equals the oracle under row r's values."""
    from qwen3tts import RequestSampling
    V, sup, eos, flags = VOCABS[vocab]
    logits = _logits(V, eos, seed=23 + V)
    seen = (np.random.default_rng(6).random((ROWS, V)) < 0.05).astype(np.uint8) if flags else None
    rep = 1.05 if flags else 1.0
    rows = [(50, 0.6, 0.9, 1), (0, 0.95, 1.0, 2), (1, 0.05, 0.5, 3), (64, 0.6, 0.7, 4), (65, 0.95, 1.0, 5), (1000, 0.05, 0.5, 6),
            (63, 0.6, 1.0, 7), (2, 0.95, 0.8, 8)]
    per_row = [RequestSampling(temperature=t, top_k=k, top_p=p, seed=s) for (k, p, t, s) in rows]
    for draw in DRAWS:
        # the call-wide values are ones no row uses: greedy, so a row that missed its override shows
        got = engine.debug_sample(logits, temperature=0.0, top_k=7, top_p=1.0, repetition_penalty=rep, seed=99, seen=seen,
                                  suppress=sup, eos_id=eos, row0=5, draw=draw, per_row=per_row).tolist()
        exp = [_oracle(logits, r, V, t, k, p, rep, seen, sup, eos, s, 5, draw) for r, (k, p, t, s) in enumerate(rows)]
        assert got == exp, (draw, got, exp)
        greedy = engine.debug_sample(logits, temperature=0.0, top_k=7, top_p=1.0, repetition_penalty=rep, seed=99, seen=seen,
                                     suppress=sup, eos_id=eos, row0=5, draw=draw).tolist()
    assert got != greedy  # (the overrides did something)
