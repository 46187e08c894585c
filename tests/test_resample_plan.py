"""The host-only definition of the engine's polyphase resampler (csrc/resample_plan.h): pairs, taps, index arithmetic.

`plan` / `apply` below restate the definition of include/q3tts.h ("Sample rates") in NumPy float64. The header's table must
equal the restatement rounded to fp32 within 1 ulp; the restatement itself is checked against an independent implementation
(scipy.signal.resample_poly fed the interleaved prototype), against the filter figures the header states, and against an
analytic sine. tests/test_resample_gpu.py imports the restatement as the reference of the device kernel."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "swift-qwen3-tts_amd", "csrc")

OTHER_RATES = (8000, 12000, 16000, 22050, 32000, 44100, 48000)
PAIRS = [(24000, r) for r in OTHER_RATES] + [(r, 24000) for r in OTHER_RATES]  # the 14 supported pairs

pytestmark = pytest.mark.skipif(not shutil.which("g++"), reason="g++ is not installed")


# ---- the restatement ------------------------------------------------------------------------------------------------
def plan(in_rate, out_rate):
    """(L, M, K, tab [L][2K] float64): tap i of phase r sits at t = (i - K + 1) - r / L of
    g(t) = s sinc(s t) I0(8.6 sqrt(1 - (t / K)^2)) / I0(8.6), each phase normalised to sum 1."""
    g = math.gcd(in_rate, out_rate)
    L, M = out_rate // g, in_rate // g
    s = 0.945 * min(1.0, L / M)
    K = int(math.ceil(16.0 / s))
    t = (np.arange(2 * K, dtype=np.float64) - K + 1)[None, :] - np.arange(L, dtype=np.float64)[:, None] / L
    inside = np.abs(t) < K
    w = s * np.sinc(s * t) * np.i0(8.6 * np.sqrt(np.maximum(0.0, 1.0 - (t / K) ** 2))) / np.i0(8.6)
    w = np.where(inside, w, 0.0)
    return L, M, K, w / w.sum(axis=1, keepdims=True)


def out_len(n_in, L, M):
    return -(-n_in * L // M)


def apply(tab, L, M, K, x, centred, front=None, clamp=False):
    """y[n] = sum_i tab[r][i] x[q - K + 1 + i] (centred) or x[q - 2K + 1 + i] (causal), q = floor(n M / L), r = n M mod L, in
    float64. `front`: the samples in front of x (a stream's margin); everything else outside x is zero."""
    x = np.asarray(x, np.float64)
    tab = np.asarray(tab, np.float64)
    front = np.zeros(0) if front is None else np.asarray(front, np.float64)
    xp = np.concatenate([np.zeros(2 * K), front, x, np.zeros(K + 1)])
    base = 2 * K + front.size  # index of x[0] in xp
    n = np.arange(out_len(x.size, L, M), dtype=np.int64)
    q, r = n * M // L, n * M % L
    j0 = q - (K if centred else 2 * K) + 1 + base
    y = np.zeros(n.size)
    for lo in range(0, n.size, 1 << 16):  # (bounded temporaries)
        sl = slice(lo, lo + (1 << 16))
        y[sl] = (tab[r[sl]] * xp[j0[sl, None] + np.arange(2 * K)[None, :]]).sum(axis=1)
    return np.clip(y, -1.0, 1.0) if clamp else y


def fp32_bound(tab32, K, xmax):
    """|fp32 fmaf chain - exact sum| over 2K taps: (2K + 2) * 2^-24 * max_r sum_i |tab[r][i]| * max|x|. A fmaf rounds once and
    every partial sum is at most sum_i |tab[r][i]| * max|x|, so the chain is off by at most 2K half-ulps of that; the two more
    cover the float64 reference's own rounding and the comparison's."""
    return (2 * K + 2) * 2.0 ** -24 * float(np.abs(np.asarray(tab32, np.float64)).sum(axis=1).max()) * xmax


# ---- the header through its driver --------------------------------------------------------------------------------------
def _build(out, flags):
    deps = [os.path.join(NATIVE, "resample_plan_driver.cc"), os.path.join(CSRC, "resample_plan.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        # no HIP include path and no platform define: the definition must stay host-only
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I" + CSRC, deps[0], "-o", out])
    return out


@pytest.fixture(scope="module")
def driver():
    return _build(os.path.join(NATIVE, "_build", "resample_plan_driver"), [])


def header_table(driver, in_rate, out_rate, env=None):
    out = subprocess.run([driver, "table", str(in_rate), str(out_rate)], capture_output=True, text=True, timeout=60, check=True,
                         env=env).stdout.splitlines()
    L, M, K = (int(v) for v in out[0].split())
    tab = np.array([[int(w, 16) for w in line.split()] for line in out[1:]], dtype=np.uint32).view(np.float32)
    assert tab.shape == (L, 2 * K)
    return L, M, K, tab


def header_run(driver, tmp_path, in_rate, out_rate, x, centred, front=None, clamp=False, env=None):
    front = np.zeros(0, np.float32) if front is None else np.asarray(front, np.float32)
    fx, fy = str(tmp_path / "x.f32"), str(tmp_path / "y.f32")
    np.concatenate([front, np.asarray(x, np.float32)]).tofile(fx)
    r = subprocess.run([driver, "run", str(in_rate), str(out_rate), "1" if centred else "0", str(front.size), "1" if clamp else "0",
                        str(len(x)), fx, fy], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    y = np.fromfile(fy, np.float32)
    assert y.size == int(r.stdout.split()[0])
    return y, r.stderr


def test_only_the_fourteen_pairs_are_supported(driver):
    out = subprocess.run([driver, "pairs"], capture_output=True, text=True, timeout=60, check=True).stdout.split()
    got = sorted(zip(map(int, out[0::2]), map(int, out[1::2])))
    assert got == sorted(PAIRS)
    for rate in OTHER_RATES:
        assert 1920 * rate % 24000 == 0  # a frame holds a whole number of samples at every supported rate
    assert [1920 * r // 24000 for r in OTHER_RATES] == [640, 960, 1280, 1764, 2560, 3528, 3840]


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%d-%d" % p)
def test_header_table_is_the_restatement_rounded_to_fp32(driver, pair):
    L, M, K, tab = header_table(driver, *pair)
    rL, rM, rK, rtab = plan(*pair)
    assert (L, M, K) == (rL, rM, rK)
    assert 17 <= K <= 51 and L * 2 * K <= 147 * 38
    want = rtab.astype(np.float32)
    assert (np.abs(tab.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))).all()  # within 1 ulp
    assert np.abs(tab.astype(np.float64).sum(axis=1) - 1.0).max() < 1e-6


def prototype(L, K, tab):
    """The phases interleaved into one filter at L x the input rate: tap (r, k) sits at index k L - r + K L of 2 K L + 1."""
    h = np.zeros(2 * K * L + 1)
    k = np.arange(2 * K) - K + 1
    for r in range(L):
        h[k * L - r + K * L] = tab[r]
    return h


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%d-%d" % p)
def test_restatement_against_scipy_resample_poly(pair):
    signal = pytest.importorskip("scipy.signal")
    L, M, K, tab = plan(*pair)
    x = np.random.default_rng(7).uniform(-1.0, 1.0, 3000)
    want = signal.resample_poly(x, L, M, window=prototype(L, K, tab) / L)  # (scipy multiplies given taps by `up`)
    got = apply(tab, L, M, K, x, centred=True)
    assert got.size == want.size == out_len(x.size, L, M)
    assert np.abs(got - want).max() < 1e-13  # float64 sums of <= 102 terms below 1 in two different orders


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%d-%d" % p)
def test_prototype_response(pair):
    """Pass band: ripple at most 0.02 dB up to 0.40 x the lower rate; stop band: at most -70 dB from 0.55 x the lower rate."""
    L, M, K, tab = plan(*pair)
    h = prototype(L, K, tab.astype(np.float32).astype(np.float64))
    nfft = 1 << 19
    H = np.abs(np.fft.rfft(h, nfft)) / L
    f = np.arange(H.size) * (pair[0] * L / nfft)  # Hz: the prototype runs at L x the input rate
    low = min(pair)
    db = 20.0 * np.log10(np.maximum(H, 1e-12))
    assert np.abs(db[f <= 0.40 * low]).max() <= 0.02
    assert db[f >= 0.55 * low].max() <= -70.0


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%d-%d" % p)
def test_sine_against_the_analytic_sine_and_header_against_restatement(driver, tmp_path, pair):
    L, M, K, tab32 = header_table(driver, *pair)
    n_in = 4000
    x = (0.5 * np.sin(2.0 * np.pi * 1000.0 * np.arange(n_in) / pair[0])).astype(np.float32)
    y, _ = header_run(driver, tmp_path, pair[0], pair[1], x, centred=True)
    edge = (2 * K * L) // M + 2  # outputs whose taps reach beyond the clip
    m = np.arange(y.size)[edge:-edge]
    want = 0.5 * np.sin(2.0 * np.pi * 1000.0 * m / pair[1])
    assert m.size > 500 and np.abs(y[edge:-edge] - want).max() <= 5e-5
    # the header's own evaluation (fp32 fmaf chain) against the restatement in float64 on the same fp32 table
    ref = apply(tab32, L, M, K, x, centred=True)
    assert np.abs(y - ref).max() <= fp32_bound(tab32, K, 0.5)


@pytest.mark.parametrize("pair", [(24000, 8000), (24000, 22050), (44100, 24000), (8000, 24000)], ids=lambda p: "%d-%d" % p)
def test_causal_form_is_the_centred_one_delayed_and_reads_the_margin(driver, tmp_path, pair):
    L, M, K, tab32 = header_table(driver, *pair)
    rng = np.random.default_rng(3)
    x = (0.1 * rng.standard_normal(3000)).astype(np.float32)
    # delayed by K input samples: the causal output of [x] equals the centred output of [K zeros ++ x] over its length
    yc, _ = header_run(driver, tmp_path, pair[0], pair[1], x, centred=False)
    yd, _ = header_run(driver, tmp_path, pair[0], pair[1], np.concatenate([np.zeros(K, np.float32), x]), centred=True)
    assert yd.size >= yc.size and np.array_equal(yc, yd[: yc.size])
    assert np.abs(yc - apply(tab32, L, M, K, x, centred=False)).max() <= fp32_bound(tab32, K, float(np.abs(x).max()))
    # a row continued behind its margin equals the one-shot run: split at a multiple of M input samples (phase 0 again)
    cut = 7 * M * 20
    tail, _ = header_run(driver, tmp_path, pair[0], pair[1], x[cut:], centred=False, front=x[cut - (2 * K - 1): cut])
    assert np.array_equal(tail, yc[cut * L // M:])
    # the clip keeps a NaN and bounds the overshoot
    big = np.where(rng.standard_normal(600) > 0, 1.0, -1.0).astype(np.float32)
    yo, _ = header_run(driver, tmp_path, pair[0], pair[1], big, centred=False, clamp=True)
    assert np.abs(yo).max() <= 1.0 and np.abs(apply(tab32, L, M, K, big, centred=False)).max() > 1.0
    big[300] = np.nan
    yo, _ = header_run(driver, tmp_path, pair[0], pair[1], big, centred=False, clamp=True)
    assert np.isnan(yo).any()


def _have_sanitizers():
    if not shutil.which("gcc"):
        return False
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    return os.path.isabs(asan) and os.path.exists(asan)


@pytest.mark.skipif(not _have_sanitizers(), reason="gcc / g++ with libasan are not installed")
def test_driver_under_address_and_undefined_sanitizers(tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined: every pair's table, and both forms at the lengths
    where the edge zero-fill matters (1, 2K - 1, 2K, 4097), with and without a margin in front."""
    san = _build(os.path.join(NATIVE, "_build", "resample_plan_driver_san"),
                 ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=0:abort_on_error=0:exitcode=97",
           "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1:exitcode=98"}
    rng = np.random.default_rng(5)
    for pair in PAIRS:
        L, M, K, tab32 = header_table(san, *pair, env=env)
        for n in (1, 2 * K - 1, 2 * K, 4097):
            x = (0.1 * rng.standard_normal(n)).astype(np.float32)
            for centred, front in ((True, None), (False, None), (False, x[: 2 * K - 1])):
                y, err = header_run(san, tmp_path, pair[0], pair[1], x, centred, front=front, env=env)
                assert "runtime error" not in err and "AddressSanitizer" not in err, err[-4000:]
                ref = apply(tab32, L, M, K, x, centred, front=front)
                assert y.size == out_len(n, L, M) and np.abs(y - ref).max() <= fp32_bound(tab32, K, float(np.abs(x).max()))
