"""The host-only choice of a pitched handle's numbers (csrc/pitch_plan.h) through its stand-alone driver: Hp against a Python
restatement, the refusals, the invariants over every admissible (rate, Ho, Hp), and the pitch and purity of shifted sines on the
definition (stretch_reference whole at Hp, then resample_reference centred Hp -> 480). tests/test_pitch_gpu.py imports the
driver's `shift` as the reference of the device path."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_stretch_plan import OTHER_RATES, _have_sanitizers, choose_hs, delay, pitch_figures

pytestmark = pytest.mark.skipif(not shutil.which("g++"), reason="g++ is not installed")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "swift-qwen3-tts_amd", "csrc")
N_TRIPLES = 2118240


# ---- the restatement ------------------------------------------------------------------------------------------------
def ratio_of(rate):
    g = math.gcd(24000, rate)
    return rate // g, 24000 // g


def choose_hp(ho, semitones):
    """The integer nearest to ho * 2^(s / 12), ties toward ho; 0 outside [240, 960] or for a pitch outside [-12, 12]."""
    s = float(np.float32(semitones))
    if not (-12.0 <= s <= 12.0):
        return 0
    want = ho * math.pow(2.0, s / 12.0)
    lo, hi = math.floor(want), math.ceil(want)
    if want - lo == hi - want:
        hp = lo if abs(lo - ho) <= abs(hi - ho) else hi
    else:
        hp = lo if want - lo < hi - want else hi
    return hp if 240 <= hp <= 960 else 0


def ratio(hp, ho, L, M):
    """(L', M', K') of the one resampler Hp * M -> Ho * L."""
    g = math.gcd(hp * M, ho * L)
    L2, M2 = ho * L // g, hp * M // g
    return L2, M2, int(math.ceil(16.0 / (0.945 * min(1.0, L2 / M2))))


def delay_out(hp, L2, M2, K2):
    d = 0 if hp == 480 else delay(hp)
    return -(-(d * hp + 480 * K2) * L2 // (480 * M2))


# ---- the header through its driver --------------------------------------------------------------------------------------
def _build(out, flags):
    deps = [os.path.join(NATIVE, "pitch_plan_driver.cc")] + [os.path.join(CSRC, h) for h in ("pitch_plan.h", "stretch_plan.h", "resample_plan.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        # no HIP include path and no platform define: the arithmetic must stay host-only
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I" + CSRC, deps[0], "-o", out])
    return out


@pytest.fixture(scope="module")
def pitch_driver():
    return _build(os.path.join(NATIVE, "_build", "pitch_plan_driver"), [])


def _run(drv, *args, env=None):
    r = subprocess.run([drv, *map(str, args)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return r.stdout


def header_choose(drv, semitones, speed=0.0, hops=4, L=1, M=1, env=None):
    """(status, ho, hp, L', M', K', table bytes, delay in output samples, effective semitones)"""
    v = _run(drv, "choose", semitones if isinstance(semitones, str) else repr(float(semitones)), repr(float(speed)), hops, L, M, env=env).split()
    return tuple(int(x) for x in v[:8]) + (float(v[8]),)


def header_shift(drv, tmp_path, hp, in_units, out_units, x, causal, clamp=False, env=None):
    """stretch_reference at hp (none at 480), then resample_reference in_units -> out_units, both causal or both whole / centred."""
    fx, fy = str(tmp_path / "px.f32"), str(tmp_path / "py.f32")
    np.asarray(x, np.float32).tofile(fx)
    out = _run(drv, "shift", hp, in_units, out_units, 1 if causal else 0, 1 if clamp else 0, len(x), fx, fy, env=env)
    y = np.fromfile(fy, np.float32)
    assert y.size == int(out.split()[0])
    return y


# ---- 1. the choice of Hp ------------------------------------------------------------------------------------------------
def test_choice_of_hp(pitch_driver):
    # the ends: an octave down halves 480, an octave up doubles it; both stay inside [240, 960] only at Ho = 480
    assert header_choose(pitch_driver, -12)[:3] == (0, 480, 240) and header_choose(pitch_driver, 12)[:3] == (0, 480, 960)
    assert header_choose(pitch_driver, 1)[:7] == (0, 480, 509, 480, 509, 18, 69120)  # the first table over 64 KiB
    for s in (-12, -7, -5, -3, -1, -0.01, 0.01, 1, 2, 3, 5, 7, 11.99, 12):
        st, ho, hp, L2, M2, K2, tb, d, eff = header_choose(pitch_driver, s)
        assert (st, ho) == (0, 480) and hp == choose_hp(480, s) == int(round(480 * 2 ** (s / 12.0)))
        assert (L2, M2, K2) == ratio(hp, 480, 1, 1) and tb == L2 * 2 * K2 * 4
        if hp != 480:
            assert abs(eff - 12 * math.log2(hp / 480)) < 1e-12 and abs(eff - s) < 12 * math.log2((hp + 0.5) / (hp - 0.5))
            assert d == delay_out(hp, L2, M2, K2)
        else:
            assert (eff, d) == (0.0, 0)  # Hp == Ho is off
    # with a speed, at 24 kHz and at 16 and 44.1 kHz: Ho is the speed's own hop at that rate, Hp the nearest integer to Ho * rho
    for rate in (24000, 16000, 44100):
        L, M = ratio_of(rate)
        for speed in (0.8, 1.25):
            ho_want = choose_hs(speed, 4, L, M)
            for s in (-3, -1, 2, 3.86, 5):
                st, ho, hp, L2, M2, K2, tb, d, eff = header_choose(pitch_driver, s, speed, 4, L, M)
                assert ho == ho_want and hp == (choose_hp(ho, s) or ho) and st == (0 if choose_hp(ho, s) else 3), (rate, speed, s)
                if st == 0 and hp != ho:
                    assert (L2, M2, K2) == ratio(hp, ho, L, M) and d == delay_out(hp, L2, M2, K2)
                    assert (4 * ho * L // M) % L2 == 0 and 4 * ho * L // M * M2 == 4 * hp * L2
    assert header_choose(pitch_driver, 3.86, 1.25)[:6] == (0, 384, 480, 4, 5, 22)  # the pure-resample case: Hp == 480
    assert header_choose(pitch_driver, 2, 1.25, 4, 2, 3)[:3] == (0, 384, 431)


def test_ties_go_toward_ho(pitch_driver):
    """Exact ties exist at the octaves of an odd Ho (2^-1 and 2^1 are exact in double): 481 / 2 = 240.5 goes to 241."""
    def hp(ho, s):
        return int(_run(pitch_driver, "hp", ho, repr(float(s))).split()[0])
    assert hp(481, -12) == 241 == choose_hp(481, -12) and hp(959, -12) == 480 == choose_hp(959, -12)
    assert hp(481, 12) == 0 and hp(480, 12) == 960 and hp(479, 12) == 958
    for ho in (240, 383, 384, 437, 600, 960):
        for s in (-12, -6.5, -1, 0, 1, 6.5, 12):
            assert hp(ho, s) == choose_hp(ho, s), (ho, s)
        assert hp(ho, 0) == ho


def test_refusals(pitch_driver):
    for bad in ("nan", "inf", "-inf", "12.001", "-12.001", "1e30", "-13"):
        assert header_choose(pitch_driver, bad)[0] == 1, bad
        assert int(_run(pitch_driver, "hp", 480, bad).split()[0]) == 0
    assert header_choose(pitch_driver, 1, 0.4)[0] == 2 and header_choose(pitch_driver, 1, 2.5)[0] == 2  # the speed's own refusal
    # no Hp in [240, 960]: never clamped
    assert header_choose(pitch_driver, 12, 0.8)[:3] == (3, 600, 600)     # 1200
    assert header_choose(pitch_driver, 1, 0.5)[:3] == (3, 960, 960)      # 1017
    assert header_choose(pitch_driver, -1, 2.0)[:3] == (3, 240, 240)     # 227
    assert header_choose(pitch_driver, -12, 1.25)[:3] == (3, 384, 384)   # 192
    assert header_choose(pitch_driver, 0, 0.5)[:3] == (0, 960, 960)      # a pitch of 0 is never refused
    assert header_choose(pitch_driver, 0.001)[:3] == (0, 480, 480)       # Hp == Ho: off, not refused


def test_invariants_over_every_admissible_triple(pitch_driver):
    """All (rate, Ho, Hp) with Ho admissible at the rate and Hp != Ho (the sweep takes a fraction of a second): L' divides the
    output frame, a frame in is a frame out, q stays inside the frame, the margins (3 frames of history) hold, the table is at
    most 939 624 bytes, K' at most 204 and the 256-output span at most 13 904 bytes."""
    lines = _run(pitch_driver, "sweep", 3, 1, 1).splitlines()
    triples, checked, bad, max_tab, max_k, max_span = (int(v) for v in lines[0].split())
    assert triples == checked == N_TRIPLES and bad == 0
    assert (max_tab, max_k, max_span) == (939624, 204, 13904)
    assert tuple(int(v) for v in lines[2].split()) == (8000, 240, 960)  # K' = 204: the ratio 1 / 12
    assert ratio(958, 940, 147, 80) == (6909, 3832, 17) and 6909 * 34 * 4 == 939624
    # the plans the device tests use: pitch_ratio agrees with make_resample_plan, and the output-order table with the plan's
    for pair, want in (((509, 480), (480, 509, 18)), ((958 * 80, 940 * 147), (6909, 3832, 17)), ((2880, 240), (1, 12, 204)),
                       ((1, 2), (2, 1, 17)), ((719, 480), (480, 719, 26))):
        out = _run(pitch_driver, "plan", *pair).split()
        assert tuple(int(v) for v in out[:3]) == want and out[3] == "ok", pair


# ---- 2. pitch quality on the definition -------------------------------------------------------------------------------
# The whole form on 1.5 s sines of amplitude 0.5 (the procedure of tests/test_stretch_plan.py): the
# spectral peak must sit at f * Hp / 480 within 0.2 * Hp / 480 Hz -- the stretch's committed 0.2 Hz, which a resampler scales
# exactly -- and the residual against the least-squares sine is bounded at 1.5 x its worst measured value per sine
# (DESIGN.md section 13 holds the table).
PITCH_SEMITONES = (-5, -1, 1, 3, 7)
# Measured worst cases (peak offset / residual): 110 Hz 0.022 Hz / 3.12 % (-1), 200 Hz 0.013 Hz / 2.48 % (-1), 437 Hz 0.055 Hz /
# 3.36 % (-5), 1000 Hz 0.004 Hz / 0.123 % (+7).
PITCH_RESIDUAL_BOUNDS = {110: 0.0469, 200: 0.0371, 437: 0.0504, 1000: 0.00185}


@pytest.mark.parametrize("freq", sorted(PITCH_RESIDUAL_BOUNDS))
def test_shifted_sines(pitch_driver, tmp_path, freq):
    x = (0.5 * np.sin(2.0 * np.pi * freq * np.arange(36000) / 24000.0)).astype(np.float32)
    worst = 0.0
    for s in PITCH_SEMITONES:
        hp = choose_hp(480, s)
        y = header_shift(pitch_driver, tmp_path, hp, hp, 480, x, causal=False)
        assert abs(y.size - x.size) <= 2
        off, res = pitch_figures(y, freq * hp / 480.0)
        print(f"pitch {freq} Hz at {s:+d} semitones (Hp {hp}): peak {freq * hp / 480.0:.2f} Hz off by {off:.3f} Hz "
              f"(bound {0.2 * hp / 480.0:.3f}), residual {100 * res:.2f} % of the signal")
        assert off <= 0.2 * hp / 480.0, (freq, s)
        worst = max(worst, res)
    assert worst <= PITCH_RESIDUAL_BOUNDS[freq]


@pytest.mark.skipif(not _have_sanitizers(), reason="gcc / g++ with libasan are not installed")
def test_driver_under_address_and_undefined_sanitizers(tmp_path):
    san = _build(os.path.join(NATIVE, "_build", "pitch_plan_driver_san"), ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=0:abort_on_error=0:exitcode=97",
           "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1:exitcode=98"}
    for s in ("0", "-12", "12", "nan", "1e30", "-0.0", "3.86"):
        for speed in (0.0, 0.5, 1.25, 2.0):
            header_choose(san, s, speed, 4, 147, 160, env=env)
    _run(san, "sweep", 3, 10, 7, env=env)
    _run(san, "plan", 2880, 240, env=env)
    x = np.random.default_rng(3).uniform(-0.5, 0.5, 2500).astype(np.float32)
    for hp, pair, causal in ((509, (509, 480), False), (240, (240, 480), True), (480, (5, 4), True), (960, (2880, 240), False)):
        y = header_shift(san, tmp_path, hp, *pair, x, causal, clamp=True, env=env)
        assert y.size > 0
    assert header_shift(san, tmp_path, 509, 509, 480, x[:1], False, env=env).size == 2  # ceil(ceil(509 / 480) * 480 / 509)
