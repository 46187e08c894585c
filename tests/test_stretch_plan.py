"""The host-only definition of the engine's time stretch (csrc/stretch_plan.h): constants, choice of the synthesis hop, one hop.

`stretch` below restates the definition of include/q3tts.h ("Speaking rate") in NumPy, with an fp32 fmaf emulated in float64
(exact product, sum rounded to odd, then to fp32). It must equal the header's stretch_reference exactly -- there the emulation
is pinned against the real fmaf -- and tests/test_stretch_gpu.py imports it as the reference of the device kernel."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "swift-qwen3-tts_amd", "csrc")

HA, DELTA, HS_MIN, HS_MAX = 480, 240, 240, 960
HS_CASES = (240, 320, 437, 600, 960)
LENGTHS = (1, 479, 480, 481, 961, 1920, 4097)
OTHER_RATES = (8000, 12000, 16000, 22050, 32000, 44100, 48000)

pytestmark = pytest.mark.skipif(not shutil.which("g++"), reason="g++ is not installed")


# ---- the restatement ------------------------------------------------------------------------------------------------
def delay(hs):
    return max(0, DELTA + hs - HA, DELTA + 2 * hs - 2 * HA)


def lookback(hs):
    return delay(hs) + DELTA + max(0, HA - hs)


def fade(hs):
    return (0.5 - 0.5 * np.cos(np.pi * (np.arange(hs, dtype=np.float64) + 0.5) / hs)).astype(np.float32)


def out_len(n_in, hs, causal):
    return (n_in // HA) * hs if causal else -(-n_in * hs // HA)


def choose_hs(speed, hops=4, L=1, M=1):
    if not (0.5 <= speed <= 2.0):
        return 0
    want = 480.0 / speed
    ok = [h for h in range(HS_MIN, HS_MAX + 1) if hops * h * L % M == 0]
    return min(ok, key=lambda h: (abs(h - want), abs(h - HA)))


def fmaf32(a, b, c):
    """fp32 fmaf(a, b, c) of float32 arrays, exactly: the product is exact in float64; the float64 sum is rounded to odd (its
    error comes from TwoSum), which the final rounding to fp32 (29 bits fewer) cannot tell from the exact sum."""
    p = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
    c = np.asarray(c, np.float32).astype(np.float64)
    s = p + c
    t = s - p
    e = (p - (s - t)) + (c - t)
    even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
    s = np.where((e != 0) & even, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def stretch(x, hs, causal, front=None, state=0, stats=None):
    """(y, state word behind the row, [d_m]). x: the row; `front`: the samples in front of it (causal form; everything else
    outside the row is zero). stats (a dict, optional) receives per hop the gap between the best and the runner-up c, the
    bound sum_n |cont[n] x[..]| of the winner's terms (for the fp32 accumulation bound) and the largest index read."""
    x = np.asarray(x, np.float32)
    front = np.zeros(0, np.float32) if (front is None or not causal) else np.asarray(front, np.float32)
    n_in = x.size
    D = delay(hs) if causal else 0
    hops = n_in // HA if causal else -(-n_in // HA)
    n_out = out_len(n_in, hs, causal)
    pad = 2 * HS_MAX + 2 * HA + DELTA + 2048
    xp = np.concatenate([np.zeros(pad, np.float32), front, x, np.zeros(pad, np.float32)])
    base = pad + front.size  # index of x[0] in xp
    f = fade(hs)
    y = np.zeros(hops * hs, np.float32)
    word, ds = int(state) if causal else 0, []
    order = np.array([(-2 * d - 1) if d < 0 else 2 * d for d in range(-DELTA, DELTA + 1)])
    for m in range(hops):
        first = word == 0
        c0 = -D if first else (m - 1) * HA + (word - DELTA - 1) - D + hs
        cont = xp[base + c0: base + c0 + hs]
        best, top = 0, c0 + hs - 1
        if not first:
            w0 = m * HA - DELTA - D
            win = xp[base + w0: base + w0 + hs + 2 * DELTA]
            acc = np.zeros(2 * DELTA + 1, np.float32)
            for n in range(hs):
                acc = fmaf32(np.float32(cont[n]), win[n: n + 2 * DELTA + 1], acc)
            c = np.where(np.isnan(acc), -np.inf, acc.astype(np.float64))
            rank = np.lexsort((order, -c))  # greatest c first, then the earlier place in the visiting order
            best = int(rank[0]) - DELTA
            top = max(top, w0 + hs + 2 * DELTA - 1)
            if stats is not None:
                mag = float(np.abs(cont.astype(np.float64) * win[rank[0]: rank[0] + hs].astype(np.float64)).sum())
                stats.setdefault("gap", []).append(float(c[rank[0]] - c[rank[1]]))
                stats.setdefault("mag", []).append(mag)
        if stats is not None:
            stats.setdefault("top", []).append(top)
        pm = m * HA + best - D
        y[m * hs: (m + 1) * hs] = fmaf32(f, xp[base + pm: base + pm + hs] - cont, cont)
        word = best + DELTA + 1
        ds.append(best)
    return y[:n_out], word, ds


def seeded_signal(n, seed):
    """Harmonics of a seeded pitch plus noise of amplitude 1e-3 .. 2e-3 (no sample comes near the denormals), |x| < 1."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    f0 = rng.uniform(80.0, 300.0)
    x = sum(a * np.sin(2.0 * np.pi * f0 * k * t / 24000.0 + rng.uniform(0, 2 * np.pi)) for k, a in ((1, 0.3), (2, 0.2), (3, 0.1), (5, 0.05)))
    noise = rng.uniform(1e-3, 2e-3, n) * np.where(rng.integers(0, 2, n) > 0, 1.0, -1.0)
    return (x + noise).astype(np.float32)


# ---- the header through its driver --------------------------------------------------------------------------------------
def _build(out, flags):
    deps = [os.path.join(NATIVE, "stretch_plan_driver.cc"), os.path.join(CSRC, "stretch_plan.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        # no HIP include path and no platform define: the definition must stay host-only
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I" + CSRC, deps[0], "-o", out])
    return out


@pytest.fixture(scope="module")
def driver():
    return _build(os.path.join(NATIVE, "_build", "stretch_plan_driver"), [])


def header_plan(driver, hs, env=None):
    out = subprocess.run([driver, "plan", str(hs)], capture_output=True, text=True, timeout=60, check=True, env=env).stdout.splitlines()
    D, look = (int(v) for v in out[0].split())
    tab = np.array([int(w, 16) for w in out[1].split()], dtype=np.uint32).view(np.float32)
    return D, look, tab


def header_choose(driver, speed, hops=4, L=1, M=1):
    out = subprocess.run([driver, "choose", speed if isinstance(speed, str) else repr(float(speed)), str(hops), str(L), str(M)],
                         capture_output=True, text=True, timeout=60, check=True).stdout
    return int(out.split()[0])


def header_run(driver, tmp_path, hs, x, causal, front=None, state=0, env=None):
    front = np.zeros(0, np.float32) if front is None else np.asarray(front, np.float32)
    fx, fy = str(tmp_path / "x.f32"), str(tmp_path / "y.f32")
    np.concatenate([front, np.asarray(x, np.float32)]).tofile(fx)
    r = subprocess.run([driver, "run", str(hs), "1" if causal else "0", str(front.size), str(state), str(len(x)), fx, fy],
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    y = np.fromfile(fy, np.float32)
    out = [int(v) for v in r.stdout.split()]
    assert y.size == out[0]
    return y, out[1], out[2:], r.stderr


def test_fmaf_emulation_on_hard_cases():
    """Against exact rational arithmetic, among others where the float64 sum lands on an fp32 tie that the exact sum misses by
    less than a float64 rounding ((1 + u)(1 - u) + 2^24 + 2 with u = 2^-23): only the round-to-odd step decides those."""
    from fractions import Fraction
    u = 2.0 ** -23
    cases = [(1 + u, 1 - u, 2.0 ** 24 + 2), (1 + u, 1 + u, 2.0 ** 24 + 2), (1 + u, 1 + u, 2.0 ** -24), (1 + u, 1 - u, -1.0),
             (1 + u, -(1 - u), -(2.0 ** 24 + 2)), (3.0, 1 + u, 2.0 ** 25 + 4)]
    rng = np.random.default_rng(11)
    cases += [tuple(rng.standard_normal(3) * 10.0 ** rng.integers(-3, 4)) for _ in range(200)]
    for a, b, c in cases:
        a, b, c = np.float32(a), np.float32(b), np.float32(c)
        fr = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
        near = np.float32(float(fr))  # (rounded twice: only a starting point, the neighbours decide)
        cand = {np.nextafter(near, np.float32(-np.inf)), near, np.nextafter(near, np.float32(np.inf))}
        want = min(cand, key=lambda v: (abs(Fraction(float(v)) - fr), int(np.float32(v).view(np.uint32)) & 1))
        assert fmaf32(a, b, c) == want, (a, b, c)
    assert fmaf32(np.float32(1 + u), np.float32(1 - u), np.float32(2.0 ** 24 + 2)) == np.float32(2.0 ** 24 + 2)


@pytest.mark.parametrize("hs", HS_CASES)
def test_plan_constants_and_fade(driver, hs):
    D, look, tab = header_plan(driver, hs)
    assert D == delay(hs) and look == lookback(hs) and look <= 1440
    assert np.array_equal(tab, fade(hs))
    assert tab.min() > 0.0 and tab.max() < 1.0  # a convex combination: the [-1, 1] range of the input survives
    assert {240: 0, 320: 80, 600: 480, 960: 1200}.get(hs, D) == D  # 2x, 1.5x, 0.8x, 0.5x


@pytest.mark.parametrize("causal", (False, True), ids=("whole", "causal"))
@pytest.mark.parametrize("hs", HS_CASES)
def test_restatement_equals_the_header_exactly(driver, tmp_path, hs, causal):
    for n in LENGTHS:
        x = seeded_signal(n, 1000 + n)
        y, word, ds, _ = header_run(driver, tmp_path, hs, x, causal)
        ry, rword, rds = stretch(x, hs, causal)
        assert y.size == out_len(n, hs, causal) == ry.size
        assert ds == rds and np.array_equal(y.view(np.uint32), ry.view(np.uint32))
        if causal:
            assert word == rword


@pytest.mark.parametrize("hs", HS_CASES)
def test_delay_makes_every_hop_causal(hs):
    """The largest index hop m may read: the end of cont behind d_{m-1} = +Delta, the end of the search window, the end of the
    chosen segment -- all at most m Ha + Ha - 1. Analytically for the worst d, and as the restatement actually reads."""
    D = delay(hs)
    for m in range(1, 12):
        cont_end = (m - 1) * HA + DELTA - D + 2 * hs - 1
        window_end = m * HA + DELTA - D + hs - 1
        assert max(cont_end, window_end) <= m * HA + HA - 1
    assert -D + hs - 1 <= HA - 1  # hop 0
    st = {}
    stretch(seeded_signal(8 * HA, 5), hs, True, stats=st)
    assert all(top <= m * HA + HA - 1 for m, top in enumerate(st["top"]))
    # and D is the smallest such delay: one less breaks the bound for some hop (or is already 0)
    assert D == 0 or max(DELTA - (D - 1) + 2 * hs - 1 - HA, DELTA - (D - 1) + hs - 1) > HA - 1


@pytest.mark.parametrize("hs", HS_CASES)
def test_whole_and_causal_agree_up_to_the_delay(driver, tmp_path, hs):
    # a periodic input (period 200 samples = 120 Hz and harmonics)
    t = np.arange(10 * HA, dtype=np.float64)
    x = (0.4 * np.sin(2 * np.pi * t / 200.0) + 0.2 * np.sin(2 * np.pi * 3 * t / 200.0 + 0.7)).astype(np.float32)
    D = delay(hs)
    yc, _, dc, _ = header_run(driver, tmp_path, hs, x, True)
    yw, _, dw, _ = header_run(driver, tmp_path, hs, np.concatenate([np.zeros(D, np.float32), x]), False)
    assert yc.size == (x.size // HA) * hs and yw.size >= yc.size
    assert dc == dw[: len(dc)] and np.array_equal(yc, yw[: yc.size])  # the causal form is the whole form of the delayed input


def test_output_lengths(driver, tmp_path):
    for hs in (240, 437, 960):
        for n in LENGTHS:
            x = seeded_signal(n, 7)
            assert header_run(driver, tmp_path, hs, x, False)[0].size == -(-n * hs // HA)
            assert header_run(driver, tmp_path, hs, x, True)[0].size == (n // HA) * hs


def test_choice_of_the_synthesis_hop(driver):
    for s in (0.5, 0.8, 1.0, 1.25, 1.5, 2.0, 480 / 437, 0.7071, 1.999):
        assert header_choose(driver, s) == choose_hs(s) == int(round(480.0 / s)) or abs(480.0 / s % 1 - 0.5) < 1e-9
    assert [header_choose(driver, s) for s in (0.5, 0.8, 1.0, 1.25, 1.5, 2.0)] == [960, 600, 480, 384, 320, 240]
    for hs in HS_CASES:
        assert header_choose(driver, 480.0 / hs) == hs
    # every output rate: the chosen hop leaves whole samples per frame behind the L / M resampler, and is the nearest such
    for rate in OTHER_RATES:
        g = math.gcd(24000, rate)
        L, M = rate // g, 24000 // g
        for s in (0.5, 0.77, 0.8, 1.1, 1.25, 1.5, 1.9, 2.0):
            hs = header_choose(driver, s, 4, L, M)
            assert hs == choose_hs(s, 4, L, M) and HS_MIN <= hs <= HS_MAX and 4 * hs * L % M == 0
            assert all(abs(h - 480.0 / s) >= abs(hs - 480.0 / s) for h in range(HS_MIN, HS_MAX + 1) if 4 * h * L % M == 0)
        assert header_choose(driver, 1.0, 4, L, M) == 480  # "off" is admissible at every rate
    # ties go toward 480: at 22050 Hz the admissible hops are the multiples of 40
    L, M = 147, 160
    for want, expect in ((500, 480), (460, 480), (540, 520), (420, 440), (660, 640), (300, 320)):
        s = 480.0 / want
        assert 480.0 / s == want  # the tie is exact in double
        assert header_choose(driver, repr(s), 4, L, M) == expect == choose_hs(s, 4, L, M)
    # refusals
    for s in ("0.49999", "2.00001", "0", "-1", "nan", "inf", "-inf", "1e9"):
        assert header_choose(driver, s) == 0


@pytest.mark.parametrize("hs", (240, 437, 960))
def test_zero_and_constant_rows_choose_d_zero(driver, tmp_path, hs):
    """Every candidate ties (all c equal): the visiting order must leave d = 0. Pins the tie-break."""
    for x in (np.zeros(6 * HA, np.float32), np.full(6 * HA, 0.25, np.float32)):
        front = x[: lookback(hs)]  # (the constant row with its own samples in front: no edge inside the search window)
        y, _, ds, _ = header_run(driver, tmp_path, hs, x, True, front=front)
        assert ds == [0] * 6
        assert np.array_equal(y, stretch(x, hs, True, front=front)[0])
    y, _, ds, _ = header_run(driver, tmp_path, hs, np.zeros(6 * HA, np.float32), False)
    assert ds == [0] * 6 and not y.any()


@pytest.mark.parametrize("hs", HS_CASES)
def test_a_row_continued_with_its_state_word_equals_the_row_in_one_piece(driver, tmp_path, hs):
    x = seeded_signal(12 * HA, 21)
    whole, word, ds, _ = header_run(driver, tmp_path, hs, x, True)
    for cut_hops in (4, 8):
        cut = cut_hops * HA
        a, wa, da, _ = header_run(driver, tmp_path, hs, x[:cut], True)
        b, wb, db, _ = header_run(driver, tmp_path, hs, x[cut:], True, front=x[cut - lookback(hs) if cut >= lookback(hs) else 0: cut], state=wa)
        assert wa == da[-1] + DELTA + 1 and wb == word and da + db == ds
        assert np.array_equal(np.concatenate([a, b]), whole)
        # the restatement continues the same way
        rb = stretch(x[cut:], hs, True, front=x[max(0, cut - lookback(hs)): cut], state=wa)
        assert np.array_equal(rb[0], b) and rb[1] == wb


# ---- pitch preservation ---------------------------------------------------------------------------------------------
# Measured with the committed header (whole form, 1.5 s sines of amplitude 0.5, the first and last 2000 output samples left
# out); DESIGN.md section 12 records the figures. Bounds: the measured worst case over the five hops, plus a margin.
# Measured worst cases: 85 Hz 0.133 Hz / 5.52 % (Hs 240), 110 Hz 0.023 Hz / 4.82 % (240), 200 Hz 0.066 Hz / 3.94 % (437: the
# correlation is not normalised, and 437 samples are no whole number of 120-sample periods), 437 Hz 0.061 Hz / 2.28 % (960),
# 1000 Hz 0.004 Hz / 0.10 % (960). The residual bound is the measured value times 1.5, the peak bound 0.2 Hz throughout.
PITCH_BOUNDS = {  # Hz: (peak offset in Hz, residual r.m.s. / signal r.m.s.)
    85: (0.2, 0.083),
    110: (0.2, 0.073),
    200: (0.2, 0.06),
    437: (0.2, 0.035),
    1000: (0.2, 0.0015),
}


def pitch_figures(y, freq):
    """(offset of the dominant spectral peak from freq in Hz, r.m.s. of y minus its best-fit sine at the peak / r.m.s. of y)."""
    y = np.asarray(y, np.float64)[2000:-2000]
    nfft = 1 << 21
    spec = np.abs(np.fft.rfft(y * np.hanning(y.size), nfft))
    peak = float(np.argmax(spec)) * 24000.0 / nfft
    t = np.arange(y.size) / 24000.0

    def residual(f):
        A = np.stack([np.sin(2 * np.pi * f * t), np.cos(2 * np.pi * f * t)], axis=1)
        coef, *_ = np.linalg.lstsq(A, y, rcond=None)
        return float(np.sqrt(((y - A @ coef) ** 2).mean()))

    best, span = peak, 0.25  # the best-fit sine: its frequency refined around the peak, three grids of 11
    for _ in range(3):
        grid = best + span * np.linspace(-1.0, 1.0, 11)
        best = float(grid[int(np.argmin([residual(f) for f in grid]))])
        span /= 5.0
    return abs(peak - freq), residual(best) / float(np.sqrt((y ** 2).mean()))


@pytest.mark.parametrize("freq", sorted(PITCH_BOUNDS))
def test_pitch_is_preserved(driver, tmp_path, freq):
    x = (0.5 * np.sin(2.0 * np.pi * freq * np.arange(36000) / 24000.0)).astype(np.float32)
    worst = (0.0, 0.0)
    for hs in HS_CASES:
        y, _, _, _ = header_run(driver, tmp_path, hs, x, False)
        off, res = pitch_figures(y, freq)
        print(f"pitch {freq} Hz, Hs {hs}: peak off by {off:.3f} Hz, residual {100 * res:.2f} % of the signal")
        worst = (max(worst[0], off), max(worst[1], res))
    assert worst[0] <= PITCH_BOUNDS[freq][0] and worst[1] <= PITCH_BOUNDS[freq][1]


def _have_sanitizers():
    if not shutil.which("gcc"):
        return False
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    return os.path.isabs(asan) and os.path.exists(asan)


@pytest.mark.skipif(not _have_sanitizers(), reason="gcc / g++ with libasan are not installed")
def test_driver_under_address_and_undefined_sanitizers(tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined: both forms at the lengths where the edge zero-fill
    matters, with and without a margin and a state word in front, and the choice of the hop at its edges."""
    san = _build(os.path.join(NATIVE, "_build", "stretch_plan_driver_san"),
                 ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=0:abort_on_error=0:exitcode=97",
           "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1:exitcode=98"}
    for hs in (240, 437, 960):
        D, look, tab = header_plan(san, hs, env=env)
        assert tab.size == hs
        for n in LENGTHS:
            x = seeded_signal(n, 50 + n)
            for causal, front, state in ((False, None, 0), (True, None, 0), (True, x[:look], DELTA + 1 + 17)):
                y, _, _, err = header_run(san, tmp_path, hs, x, causal, front=front, state=state, env=env)
                assert "runtime error" not in err and "AddressSanitizer" not in err, err[-4000:]
                assert y.size == out_len(n, hs, causal)
    for s in ("0.5", "2", "nan", "1e300", "-0.0"):
        r = subprocess.run([san, "choose", s, "4", "147", "160"], capture_output=True, text=True, timeout=60, env=env)
        assert r.returncode == 0 and "runtime error" not in r.stderr, r.stderr[-4000:]
