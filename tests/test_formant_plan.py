"""The definition of the formant-preserving pitch stage (csrc/formant_plan.h) through its stand-alone driver: Levinson-Durbin
against a float64 restatement and on every fallback branch, the analyse + whiten -> synthesise round trip, the independence of the
synthesis from how a row is cut into pieces, and what the stage is for: the envelope peaks of synthetic vowels stay where they
were while the fundamental moves (DESIGN.md section 13 holds the tables). tests/test_formant_gpu.py imports the driver's modes as
the reference of the device path."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_pitch_plan import choose_hp, header_shift, pitch_driver  # noqa: F401  (the fixture of the plain shift)
from test_stretch_plan import _have_sanitizers

pytestmark = pytest.mark.skipif(not shutil.which("g++"), reason="g++ is not installed")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "swift-qwen3-tts_amd", "csrc")
P = 24
FORMANTS = ((700.0, 90.0), (1220.0, 110.0), (2600.0, 160.0))


# ---- the header through its driver --------------------------------------------------------------------------------------
def _build(out, flags):
    deps = [os.path.join(NATIVE, "formant_plan_driver.cc")] + [os.path.join(CSRC, h) for h in ("formant_plan.h", "pitch_plan.h", "stretch_plan.h",
                                                                                              "resample_plan.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        # no HIP include path and no platform define: the arithmetic must stay host-only; a multiply and an add round apart
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-I" + CSRC, deps[0], "-o", out])
    return out


@pytest.fixture(scope="module")
def formant_driver():
    return _build(os.path.join(NATIVE, "_build", "formant_plan_driver"), [])


def _run(drv, *args, env=None):
    r = subprocess.run([drv, *map(str, args)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return r.stdout


def header_levinson(drv, tmp_path, r, env=None):
    """(ok, a[0..P]) of formant_levinson on r[0..P]"""
    fr, fa = str(tmp_path / "fr.f32"), str(tmp_path / "fa.f32")
    np.asarray(r, np.float32).tofile(fr)
    ok = int(_run(drv, "levinson", fr, fa, env=env).split()[0])
    return bool(ok), np.fromfile(fa, np.float32)


def header_analyse(drv, tmp_path, hp, x, hist=0, env=None):
    """(coef [hops][P], e [n], ok [hops]) of formant_analyse_whiten on a row whose first `hist` samples lie in front of it"""
    fx, fc, fe = str(tmp_path / "fx.f32"), str(tmp_path / "fc.f32"), str(tmp_path / "fe.f32")
    x = np.asarray(x, np.float32)
    x.tofile(fx)
    out = _run(drv, "analyse", hp, x.size - hist, hist, fx, fc, fe, env=env).split()
    hops = int(out[0])
    coef, e = np.fromfile(fc, np.float32).reshape(hops, P), np.fromfile(fe, np.float32)
    assert e.size == x.size - hist
    return coef, e, np.array([int(v) for v in out[1:]], bool)


def header_synth(drv, tmp_path, ho, ep, coef, piece=0, state=None, env=None):
    """(z unclipped, state behind) of formant_synthesise in pieces of `piece` samples (0: one piece)"""
    fe, fc, fz, fs, fo = (str(tmp_path / n) for n in ("se.f32", "sc.f32", "sz.f32", "ss.f32", "so.f32"))
    np.asarray(ep, np.float32).tofile(fe)
    np.asarray(coef, np.float32).tofile(fc)
    if state is not None:
        np.asarray(state, np.float32).tofile(fs)
    _run(drv, "synth", ho, len(ep), piece, fe, fc, fz, fs if state is not None else "-", fo, env=env)
    return np.fromfile(fz, np.float32), np.fromfile(fo, np.float32)


def header_formant_shift(drv, tmp_path, hp, x, env=None):
    fx, fy = str(tmp_path / "hx.f32"), str(tmp_path / "hy.f32")
    np.asarray(x, np.float32).tofile(fx)
    out = _run(drv, "shift", hp, len(x), fx, fy, env=env)
    y = np.fromfile(fy, np.float32)
    assert y.size == int(out.split()[0])
    return y


def header_formant_causal(drv, tmp_path, hp, ho, x, env=None):
    """The decoder's tail on a 24 kHz waveform of whole hops: causal stretch at hp, analyse + whiten, causal FIR hp -> ho,
    synthesise at ho, clipped."""
    fx, fy = str(tmp_path / "cx.f32"), str(tmp_path / "cy.f32")
    np.asarray(x, np.float32).tofile(fx)
    out = _run(drv, "causal", hp, ho, len(x), fx, fy, env=env)
    y = np.fromfile(fy, np.float32)
    assert y.size == int(out.split()[0])
    return y


# ---- signals and the float64 restatement ------------------------------------------------------------------------------
def vowel(f0, n=36000, peak=0.5):
    """An impulse train at f0 through resonators at 700 / 1220 / 2600 Hz (bandwidths 90 / 110 / 160 Hz), in cascade."""
    x = np.zeros(n)
    x[(np.arange(0, n * f0 / 24000.0) * 24000.0 / f0).astype(int)] = 1.0
    for f, bw in FORMANTS:
        r = np.exp(-np.pi * bw / 24000.0)
        a1, a2 = -2.0 * r * np.cos(2.0 * np.pi * f / 24000.0), r * r
        y = np.zeros(n)
        for i in range(n):
            y[i] = x[i] - a1 * (y[i - 1] if i >= 1 else 0.0) - a2 * (y[i - 2] if i >= 2 else 0.0)
        x = y
    return (peak * x / np.max(np.abs(x))).astype(np.float32)


_VOWELS = {}


def shared_vowel(f0):
    if f0 not in _VOWELS:
        _VOWELS[f0] = vowel(f0)
        _VOWELS[f0].setflags(write=False)
    return _VOWELS[f0]


def levinson64(r, order=P):
    a, err = np.zeros(order + 1), float(r[0])
    a[0] = 1.0
    for i in range(1, order + 1):
        k = -(r[i] + np.dot(a[1:i], r[i - 1:0:-1])) / err
        a[1:i + 1] = np.concatenate([a[1:i] + k * a[i - 1:0:-1], [k]])
        err *= 1.0 - k * k
    return a


def analyse64(block, hp):
    """a[0..P] of one windowed block of 2 hp samples in float64: the restatement of formant_analyse"""
    n = 2 * hp
    w = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)).astype(np.float32).astype(np.float64) * np.asarray(block, np.float64)
    r = np.array([np.dot(w[k:], w[:n - k]) for k in range(P + 1)])
    lag = np.exp(-0.5 * (2.0 * np.pi * 60.0 * np.arange(P + 1) / 24000.0) ** 2).astype(np.float32).astype(np.float64)
    r = r * lag
    r[0] *= float(np.float32(1.0001))
    return levinson64(r), r


def envelope_peaks(x, near):
    """The peaks of the order-24 LPC envelope of x (float64, Hann window, the lag window and floor of the definition) nearest to
    the frequencies `near`, on a 1 Hz grid."""
    x = np.asarray(x, np.float64)
    w = x * np.hanning(x.size)
    spec = np.abs(np.fft.rfft(w, 1 << 17)) ** 2
    r = np.fft.irfft(spec)[:P + 1]
    r = r * np.exp(-0.5 * (2.0 * np.pi * 60.0 * np.arange(P + 1) / 24000.0) ** 2)
    r[0] *= 1.0001
    a = levinson64(r)
    env = -np.log(np.abs(np.fft.rfft(a, 24000)))  # 1 Hz per bin
    peaks = np.array([i for i in range(1, env.size - 1) if env[i] > env[i - 1] and env[i] >= env[i + 1]], float)
    return [float(peaks[np.argmin(np.abs(peaks - f))]) for f in near]


def f0_of(y, expect):
    """The autocorrelation peak of y near 24000 / expect samples, refined by a parabola."""
    y = np.asarray(y, np.float64)
    spec = np.abs(np.fft.rfft(y, 1 << 17)) ** 2
    r = np.fft.irfft(spec)
    lag0 = 24000.0 / expect
    lo, hi = int(lag0 * 0.8), int(lag0 * 1.2) + 2
    i = lo + int(np.argmax(r[lo:hi]))
    d = 0.5 * (r[i - 1] - r[i + 1]) / (r[i - 1] - 2.0 * r[i] + r[i + 1])
    return i + d


# ---- 1. Levinson-Durbin ---------------------------------------------------------------------------------------------------
# fp32 against float64 on the coefficients of one hop. Measured worst |a32 - a64| over the cases below: noise 3.18e-8 (largest
# |a| 0.145), vowels 2.81e-3 (largest |a| 1.88: a vowel's normal equations are ill-conditioned, the lag window and the 1e-4
# floor bound it). Bounds: 1.5 x.
LEVINSON_BOUNDS = {"noise": 4.8e-8, "vowel": 4.3e-3}


@pytest.mark.parametrize("kind", ("noise", "vowel"))
def test_levinson_against_float64(formant_driver, tmp_path, kind):
    worst, amax = 0.0, 0.0
    for hp in (360, 480, 719):
        if kind == "noise":
            x = np.random.default_rng(hp).uniform(-0.5, 0.5, 6 * hp).astype(np.float32)
        else:
            x = shared_vowel(110 if hp != 480 else 180)[6000:6000 + 6 * hp]
        coef, e, ok = header_analyse(formant_driver, tmp_path, hp, x)
        assert ok.all() and coef.shape == (6, P)
        for h in range(1, 6):
            a64, _ = analyse64(x[(h - 1) * hp:(h + 1) * hp], hp)
            worst = max(worst, float(np.max(np.abs(coef[h] - a64[1:]))))
            amax = max(amax, float(np.max(np.abs(a64[1:]))))
    print(f"levinson fp32 against float64 on {kind}: worst |a32 - a64| {worst:.3e}, largest |a| {amax:.3f} (bound {LEVINSON_BOUNDS[kind]:.1e})")
    assert worst <= LEVINSON_BOUNDS[kind]


DC_ROUND_TRIP_BOUND = 1.8e-7  # 1.5 x the 1.19e-7 measured on the reference (four ulps of 0.25)


def test_levinson_fallbacks(formant_driver, tmp_path):
    """Every branch that gives up: a is exactly 0 behind a[0] and the hop passes through unchanged."""
    hp = 480
    zero = np.zeros(4 * hp, np.float32)
    imp = zero.copy()
    imp[2 * hp + 7] = 1.0e-5  # r[0] = (1e-5 w)^2 < 1e-9: below the floor
    imp1 = zero.copy()
    imp1[2 * hp + 7] = 1.0    # above the floor: r[k] = 0 behind r[0], every reflection coefficient is 0
    dc = np.full(4 * hp, 0.25, np.float32)
    for name, x in (("silence", zero), ("impulse", imp)):
        coef, e, ok = header_analyse(formant_driver, tmp_path, hp, x)
        assert not ok.any() and not coef.any(), name
        assert np.array_equal(e, x), name
    coef, e, ok = header_analyse(formant_driver, tmp_path, hp, imp1)
    assert not coef.any() and np.array_equal(e, imp1)
    # a DC hop: the windowed block is one Hann bump, r decays slowly and Levinson runs; it must not blow up, and whichever way
    # it goes the round trip below holds. The fallbacks of the recursion itself, on r given directly:
    coef, e, ok = header_analyse(formant_driver, tmp_path, hp, dc)
    print("DC hop: ok", ok, "largest |a|", np.abs(coef).max(axis=1))
    assert np.isfinite(coef).all() and np.isfinite(e).all()
    # what the definition does on DC, pinned: no fallback at any hop (the Hann window, the lag window and the 1e-4 floor keep
    # every |k| below 1); largest |a| measured 1.0053 (hop 0, half a window) and 0.3668 (the hops inside), bounded at 1.5 x;
    # and the round trip returns the row (worst |z - y| measured 1.19e-7, bounded at 1.5 x)
    assert ok.all()
    amax = np.abs(coef).max(axis=1)
    assert amax[0] <= 1.508 and (amax[1:] <= 0.5502).all() and (amax > 0.1).all()
    z, _ = header_synth(formant_driver, tmp_path, hp, e, coef)
    print("DC round trip: worst |z - y|", float(np.max(np.abs(z - dc))))
    assert float(np.max(np.abs(z - dc))) <= DC_ROUND_TRIP_BOUND
    r = np.zeros(P + 1, np.float32)
    r[0] = 1.0
    cases = {"inf at a lag": (7, np.inf), "nan at a lag": (3, np.nan), "|k| >= 1": (1, 1.0), "|k| > 1": (2, -3.0), "r0 inf": (0, np.inf),
             "r0 nan": (0, np.nan), "r0 below the floor": (0, 1e-10), "r0 negative": (0, -1.0)}
    for name, (i, v) in cases.items():
        rr = r.copy()
        rr[i] = v
        ok, a = header_levinson(formant_driver, tmp_path, rr)
        assert not ok and a[0] == 1.0 and not a[1:].any(), name
    # err <= 0 without |k| >= 1 cannot happen in exact arithmetic (err > 0 and |k| < 1 keep err > 0); in fp32 1 - k * k rounds
    # to 0 for |k| within 2^-25 of 1
    rr = r.copy()
    rr[1] = np.float32(1.0) - np.float32(2.0 ** -24)
    ok, a = header_levinson(formant_driver, tmp_path, rr)
    assert not ok and not a[1:].any()
    ok, a = header_levinson(formant_driver, tmp_path, r)  # white: fine, and nothing to remove
    assert ok and a[0] == 1.0 and not a[1:].any()


# ---- 2. round trip ----------------------------------------------------------------------------------------------------------
# analyse + whiten, then synthesise with the same coefficients at Hp == Ho: the input again. Measured on the reference, worst
# |z - y| over Hp in {240, 480, 960}: noise 2.98e-7 (amplitude 0.5), vowel 1.96e-6 (peak 0.5: the synthesis filter's gain at the
# formants multiplies the whitening's fp32 rounding). Bounds: 1.5 x.
ROUND_TRIP_BOUNDS = {"noise": 4.5e-7, "vowel": 2.95e-6}


@pytest.mark.parametrize("kind", ("noise", "vowel"))
def test_round_trip(formant_driver, tmp_path, kind):
    worst = 0.0
    for hp in (240, 480, 960):
        n = 10 * hp + 17
        x = np.random.default_rng(hp).uniform(-0.5, 0.5, n).astype(np.float32) if kind == "noise" else shared_vowel(110)[6000:6000 + n]
        coef, e, ok = header_analyse(formant_driver, tmp_path, hp, x)
        z, _ = header_synth(formant_driver, tmp_path, hp, e, coef)
        worst = max(worst, float(np.max(np.abs(z - x))))
    print(f"round trip on {kind}: worst |z - y| {worst:.3e} (bound {ROUND_TRIP_BOUNDS[kind]:.1e})")
    assert worst <= ROUND_TRIP_BOUNDS[kind]


# ---- 3. chunk independence ------------------------------------------------------------------------------------------------
def test_synthesis_in_pieces_equals_one_piece(formant_driver, tmp_path):
    ho, hp = 480, 571
    x = shared_vowel(180)[6000:6000 + 12 * 4 * hp + 5]
    coef, e, ok = header_analyse(formant_driver, tmp_path, hp, x)
    ep = np.random.default_rng(5).uniform(-0.05, 0.05, 12 * 4 * ho).astype(np.float32)
    whole, s_whole = header_synth(formant_driver, tmp_path, ho, ep, coef[:12 * 4])
    assert np.abs(whole).max() > 0.05  # the filter does something
    for frames in (1, 3, 8):
        z, s = header_synth(formant_driver, tmp_path, ho, ep, coef[:12 * 4], piece=frames * 4 * ho)
        assert z.tobytes() == whole.tobytes() and s.tobytes() == s_whole.tobytes(), frames
    assert s_whole.tobytes() == whole[-P:].tobytes()
    # a state in front: the first samples differ, and a row continued from the state of its first part equals the row whole
    first, s1 = header_synth(formant_driver, tmp_path, ho, ep[:5 * ho], coef[:5])
    rest, _ = header_synth(formant_driver, tmp_path, ho, ep[5 * ho:], coef[5:12 * 4], state=s1)
    assert np.concatenate([first, rest]).tobytes() == whole.tobytes()


# ---- 4. what the stage is for: the formants stay, the fundamental moves ---------------------------------------------------
FORMANT_HPS = (360, 571, 640, 719)  # -5, +3, +5, +7 semitones
# r.m.s. of the output over the input's, per case: measured 0.574 .. 1.049 (the loss on upward shifts: the excitation's
# harmonics thin out under a fixed envelope). Bound: the measured range widened by a quarter of its width on either side.
LEVEL_RANGE = (0.574, 1.049)
LEVEL_BOUNDS = (LEVEL_RANGE[0] - 0.25 * (LEVEL_RANGE[1] - LEVEL_RANGE[0]), LEVEL_RANGE[1] + 0.25 * (LEVEL_RANGE[1] - LEVEL_RANGE[0]))


@pytest.mark.parametrize("f0", (110, 180))
def test_formants_stay_and_pitch_moves(formant_driver, pitch_driver, tmp_path, f0):  # noqa: F811
    x = shared_vowel(f0)
    cut = slice(6000, -6000)
    own = envelope_peaks(x[cut], [f for f, _ in FORMANTS])
    for (f, _), got in zip(FORMANTS, own):
        assert abs(got - f) < 0.05 * f  # the reading finds the resonators it was given
    for hp in FORMANT_HPS:
        plain = header_shift(pitch_driver, tmp_path, hp, hp, 480, x, causal=False)
        kept = header_formant_shift(formant_driver, tmp_path, hp, x)
        assert kept.size == plain.size and abs(kept.size - x.size) <= 2
        # the new form: the peak nearest to the input's own. The plain shift: the peak the formant moved to, the one nearest to
        # the input's own times Hp / 480 (at Hp = 719 the 700 Hz resonance lands at 1048 Hz, 170 Hz from where the 1220 Hz one
        # was: read by nearness to the input's peak, the shifted signal would show the wrong resonance as the 1220 Hz formant)
        pk_plain, pk_kept = envelope_peaks(plain[cut], [o * hp / 480.0 for o in own]), envelope_peaks(kept[cut], own)
        for (f, _), o, pp, pkp in zip(FORMANTS, own, pk_plain, pk_kept):
            disp = f * abs(hp / 480.0 - 1.0)
            print(f"formant {f:.0f} Hz, f0 {f0}, Hp {hp}: input {o:.0f}, plain {pp:.0f}, kept {pkp:.0f} Hz: "
                  f"{abs(pkp - o) / disp:.3f} of the displacement {disp:.0f} Hz (plain {abs(pp - o) / disp:.3f})")
            assert abs(pkp - o) < 0.5 * disp, (f, f0, hp)
            assert abs(pp - o) > 0.5 * disp, (f, f0, hp)
        # ... and, for the outer formants, where no other resonance can be mistaken for them, the issue's own reading: the plain
        # shift's peak NEAREST to the input's own is beyond half the displacement as well
        near = envelope_peaks(plain[cut], own)
        for i in (0, 2):
            disp = FORMANTS[i][0] * abs(hp / 480.0 - 1.0)
            print(f"formant {FORMANTS[i][0]:.0f} Hz, f0 {f0}, Hp {hp}: plain shift's peak nearest to the input's {own[i]:.0f}: {near[i]:.0f} Hz "
                  f"({abs(near[i] - own[i]) / disp:.3f} of the displacement)")
            assert abs(near[i] - own[i]) > 0.5 * disp, (FORMANTS[i][0], f0, hp)
        want = f0 * hp / 480.0
        lag = f0_of(kept[cut], want)
        level = float(np.sqrt(np.mean(kept[cut].astype(np.float64) ** 2) / np.mean(x[cut].astype(np.float64) ** 2)))
        print(f"f0 {f0}, Hp {hp}: period {lag:.2f} samples (want {24000.0 / want:.2f}), r.m.s. out / in {level:.3f}")
        assert abs(lag - 24000.0 / want) <= 0.01 * 24000.0 / want, (f0, hp)
        assert LEVEL_BOUNDS[0] <= level <= LEVEL_BOUNDS[1], (f0, hp, level)


@pytest.mark.skipif(not _have_sanitizers(), reason="gcc / g++ with libasan are not installed")
def test_driver_under_address_and_undefined_sanitizers(tmp_path):
    san = _build(os.path.join(NATIVE, "_build", "formant_plan_driver_san"), ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=0:abort_on_error=0:exitcode=97",
           "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1:exitcode=98"}
    x = np.random.default_rng(3).uniform(-0.5, 0.5, 2500).astype(np.float32)
    for hp, n, hist in ((240, 2500, 0), (509, 1, 0), (960, 2500 - 984, 984), (480, 24, 3), (719, 0, 0)):
        coef, e, ok = header_analyse(san, tmp_path, hp, x[:n + hist], hist=hist, env=env)
        z, s = header_synth(san, tmp_path, hp, e, coef, piece=hp, env=env)
        assert z.size == n and s.size == P
    r = np.zeros(P + 1, np.float32)
    for v in (0.0, np.inf, np.nan, 1.0):
        r[0] = v
        header_levinson(san, tmp_path, r, env=env)
    assert header_formant_shift(san, tmp_path, 509, x, env=env).size > 0
    assert header_formant_causal(san, tmp_path, 509, 480, x[:1920], env=env).size == 1920
    assert header_formant_causal(san, tmp_path, 480, 384, x[:1920], env=env).size == 1536
    assert header_formant_shift(san, tmp_path, 509, x[:1], env=env).size == 2  # ceil(ceil(509 / 480) * 480 / 509)
    assert header_formant_shift(san, tmp_path, 480, x[:7], env=env).tobytes() == x[:7].tobytes()
