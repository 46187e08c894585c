"""Speaking rate per request, host side (no GPU): the new fields of include/q3tts.h and their ctypes mirror, the arithmetic of
csrc/request_speed_plan.h through its stand-alone driver against the restatement of tests/test_stretch_plan.py, the refusals
that need no device, and the driver under ASan / UBSan."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from test_stretch_plan import OTHER_RATES, _have_sanitizers, choose_hs, fade

pytestmark = pytest.mark.skipif(not shutil.which("g++"), reason="g++ is not installed")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "swift-qwen3-tts_amd", "csrc")
SPEEDS = (0.5, 0.8, 1.0, 1.25, 1.5, 2.0)


def _build(out, flags):
    deps = [os.path.join(NATIVE, "request_speed_driver.cc"), os.path.join(CSRC, "request_speed_plan.h"), os.path.join(CSRC, "stretch_plan.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        # no HIP include path and no platform define: the arithmetic must stay host-only
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I" + CSRC, deps[0], "-o", out])
    return out


@pytest.fixture(scope="module")
def driver():
    return _build(os.path.join(NATIVE, "_build", "request_speed_driver"), [])


def _ratio(rate):
    g = int(np.gcd(24000, rate))
    return rate // g, 24000 // g


def _info(drv, speed, L, M, handle_hs=480, env=None):
    r = subprocess.run([drv, "info", speed if isinstance(speed, str) else repr(float(speed)), "4", str(L), str(M), str(handle_hs)],
                       capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return [int(v) for v in r.stdout.split()]


def test_the_new_fields_exist_in_the_header_and_the_mirror():
    """request_speeds and max_samples_per_frame are the last fields of their structs. q3tts_request.speed is not: three
    existing tests pin sizeof(q3tts_request) == 88 and Q3TTS_ABI_VERSION == 4, so the field takes the four bytes of padding
    behind max_tokens and the struct keeps its size (tests/test_abi.py compares every offset with the C compiler's)."""
    from qwen3tts import _lib as L
    assert L.LoadOpts._fields_[-1] == ("request_speeds", C.c_int32)
    assert L.ModelInfo._fields_[-1] == ("max_samples_per_frame", C.c_int32)
    names = [f[0] for f in L.Request._fields_]
    assert "speed" in names and dict((f[0], f[1]) for f in L.Request._fields_)["speed"] is C.c_float
    assert C.sizeof(L.Request) == 88 and L.Request.speed.offset == L.Request.max_tokens.offset + 4
    assert L.Request().speed == 0.0 and L.LoadOpts().request_speeds == 0
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "q3tts.h")).read(), flags=re.S)
    assert re.search(r"int32_t\s+request_speeds;\s*}\s*q3tts_load_opts;", src)
    assert re.search(r"int32_t\s+max_samples_per_frame;\s*}\s*q3tts_model_info;", src)
    assert re.search(r"float\s+speed;", src.split("q3tts_request;")[0].rsplit("typedef struct", 1)[1])
    assert "q3tts_request_speed_info" in src and "q3tts_debug_stretch_rows" in src


def test_defaults_and_the_python_surface():
    from qwen3tts import GenerationRequest, Qwen3TTSModel, _lib as L
    import inspect
    o = L.LoadOpts()
    o.request_speeds = 7
    L.lib().q3tts_default_load_opts(C.byref(o))
    assert o.request_speeds == 0 and o.speed == 0.0
    assert GenerationRequest([1, 2, 3, 4], 1).speed == 0.0
    assert inspect.signature(Qwen3TTSModel.from_pretrained).parameters["request_speeds"].default is False
    assert hasattr(Qwen3TTSModel, "request_speed_info")


@pytest.mark.parametrize("rate", (24000,) + OTHER_RATES)
def test_a_requests_hop_is_the_handles_rule(driver, rate):
    """hs_of is stretch_choose_hs with the handle's L / M -- the restatement's choose_hs -- at every supported output rate;
    samples per frame are 4 Hs L / M exactly; the slowest row's size the buffers."""
    L_, M_ = _ratio(rate)
    for s in SPEEDS:
        hs, spf, mid, max_spf, max_mid = _info(driver, s, L_, M_)
        want = choose_hs(s, 4, L_, M_)
        assert hs == want and 240 <= hs <= 960 and (4 * hs * L_) % M_ == 0, (rate, s)
        assert spf == 4 * hs * L_ // M_ and mid == 4 * hs
        assert max_spf == 4 * 960 * L_ // M_ == 3840 * rate // 24000 and max_mid == 3840 and spf <= max_spf
    assert _info(driver, 1.0, L_, M_)[0] == 480  # "off" is admissible at every rate
    # speed 0 is the handle's own hop, whatever it is
    assert _info(driver, 0.0, L_, M_, handle_hs=600)[:2] == [600, 4 * 600 * L_ // M_]


def test_refused_speeds(driver):
    for bad in ("nan", "inf", "-inf", "0.4999", "2.0001", "-1", "1e300", "-0.5"):
        assert _info(driver, bad, 2, 3)[0] == 0, bad
    # the C entry without a handle: INVALID_INPUT, nothing touched
    from qwen3tts import _lib as L
    s, hs, d, spf = C.c_float(-1), C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    assert L.lib().q3tts_request_speed_info(None, 1.25, C.byref(s), C.byref(hs), C.byref(d), C.byref(spf)) == 3
    assert (hs.value, d.value, spf.value) == (-1, -1, -1)


def test_rows_of_mixed_speeds_lie_packed_and_apart(driver):
    for rate in (24000, 16000, 44100):
        L_, M_ = _ratio(rate)
        hops = [choose_hs(s, 4, L_, M_) for s in (2.0, 0.5, 1.0, 0.8, 1.25)]
        F = 7
        out = subprocess.run([driver, "place", str(L_), str(M_), str(F), *map(str, hops)], capture_output=True, text=True, timeout=60, check=True)
        rows = [tuple(int(v) for v in l.split()) for l in out.stdout.splitlines()]
        stride = F * 3840 * rate // 24000
        assert rows == [(b * stride, b * stride + F * 4 * h * L_ // M_) for b, h in enumerate(hops)]
        assert rows[1][1] == 2 * stride  # the slowest row fills its part exactly


@pytest.mark.parametrize("hs", (240, 437, 480, 960))
def test_the_all_hops_fade_table(driver, hs):
    out = subprocess.run([driver, "fade", str(hs)], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    assert int(out[0]) == (hs - 240) * 960
    tab = np.array([int(w, 16) for w in out[1].split()], dtype=np.uint32).view(np.float32)
    assert tab.size == 960 and np.array_equal(tab[:hs], fade(hs)) and not tab[hs:].any()


@pytest.mark.skipif(not _have_sanitizers(), reason="gcc / g++ with libasan are not installed")
def test_driver_under_address_and_undefined_sanitizers():
    san = _build(os.path.join(NATIVE, "_build", "request_speed_driver_san"), ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=0:abort_on_error=0:exitcode=97",
           "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1:exitcode=98"}
    for s in ("0", "0.5", "2", "nan", "1e300", "-0.0", "1.25"):
        _info(san, s, 147, 160, env=env)
    for args in (["place", "2", "3", "9", "240", "960", "480", "600"], ["fade", "240"], ["fade", "960"]):
        r = subprocess.run([san, *args], capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
