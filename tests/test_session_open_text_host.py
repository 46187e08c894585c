"""Open-text requests without a GPU: the C ABI additions (symbols, the stats struct's layout, the pinned ABI version and request
size) and the text state of the session's host-only bookkeeping (csrc/session_queue.h) under the sanitizers.

tests/native/session_text_driver.cc has its own main over session_queue.h alone. It is built and run once with the address
and undefined-behaviour sanitizers and once with the thread sanitizer, as its own process; nothing loaded into Python is
instrumented."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "swift-qwen3-tts_amd", "csrc")

SYMBOLS = ["q3tts_session_submit_open", "q3tts_session_append_text", "q3tts_session_get_text_stats", "q3tts_debug_text_resume"]


def test_open_text_symbols_are_exported():
    from qwen3tts import _lib as L
    lib = C.CDLL(L.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(lib, name), name


def test_text_stats_layout_and_the_pinned_abi(tmp_path):
    """q3tts_session_text_stats against the ctypes mirror, as a C99 compiler lays the header out; the new entry points have the
    prototypes the header promises; Q3TTS_ABI_VERSION is still 4 and q3tts_request still 88 bytes."""
    from qwen3tts import _lib as L
    mirror = L.SessionTextStats
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "q3tts.h"',
             'static q3tts_status (*p_open)(q3tts_session*, const q3tts_request*, const q3tts_row_sampling*, int64_t*) = q3tts_session_submit_open;',
             'static q3tts_status (*p_append)(q3tts_session*, int64_t, const int32_t*, int32_t, int32_t) = q3tts_session_append_text;',
             'static q3tts_status (*p_stats)(const q3tts_session*, q3tts_session_text_stats*) = q3tts_session_get_text_stats;',
             'int main(void) {', '  (void)p_open; (void)p_append; (void)p_stats;',
             '  printf("%d %zu %zu\\n", Q3TTS_ABI_VERSION, sizeof(q3tts_request), sizeof(q3tts_session_text_stats));']
    lines += ['  printf("%%zu\\n", offsetof(q3tts_session_text_stats, %s));' % f for f, _ in mirror._fields_]
    lines += ['  return 0;', '}']
    src = tmp_path / "text_abi.c"
    src.write_text("\n".join(lines))
    obj = tmp_path / "text_abi.o"
    # compiled and run for the numbers; the prototypes are checked by the compiler (the object is not linked against the library)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(obj)])
    exe = tmp_path / "text_abi"
    stub = tmp_path / "stub.c"
    stub.write_text('#include "q3tts.h"\n'
                    'q3tts_status q3tts_session_submit_open(q3tts_session* s, const q3tts_request* r, const q3tts_row_sampling* rs, int64_t* t)'
                    ' { (void)s; (void)r; (void)rs; (void)t; return Q3TTS_OK; }\n'
                    'q3tts_status q3tts_session_append_text(q3tts_session* s, int64_t t, const int32_t* i, int32_t n, int32_t f)'
                    ' { (void)s; (void)t; (void)i; (void)n; (void)f; return Q3TTS_OK; }\n'
                    'q3tts_status q3tts_session_get_text_stats(const q3tts_session* s, q3tts_session_text_stats* o)'
                    ' { (void)s; (void)o; return Q3TTS_OK; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(obj), str(stub),
                           "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert out[:2] == [4, 88]
    assert C.sizeof(L.Request) == 88
    assert out[2] == C.sizeof(mirror) == 32
    assert out[3:] == [getattr(mirror, f).offset for f, _ in mirror._fields_]
    assert [f for f, _ in mirror._fields_] == ["open", "starved", "appended_tokens", "starve_events"]


def test_python_surface():
    from qwen3tts import Session
    for name in ("submit_open", "append_text", "close_text", "text_stats"):
        assert callable(getattr(Session, name))


def _sanitized(flags):
    probe = subprocess.run(["g++", "-x", "c++", "-", "-o", os.devnull, "-pthread", *flags], input="int main(){return 0;}",
                           capture_output=True, text=True)
    return probe.returncode == 0


@pytest.mark.skipif(not shutil.which("g++"), reason="g++ is not installed")
@pytest.mark.parametrize("name,flags", [("asan_ubsan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]),
                                        ("tsan", ["-fsanitize=thread"])])
def test_session_text_driver_under_sanitizers(name, flags):
    if not _sanitized(flags):
        pytest.skip("g++ cannot link with " + flags[0])
    out = os.path.join(NATIVE, "_build", "session_text_driver_" + name)
    deps = [os.path.join(NATIVE, "session_text_driver.cc"), os.path.join(CSRC, "session_queue.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        # no HIP include path and no platform define: the session's bookkeeping must stay host-only
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-pthread", *flags, "-I" + CSRC, deps[0], "-o", out])
    for args in (["4", "100", "16"], ["6", "40", "2"], ["1", "60", "0"]):
        r = subprocess.run([out, *args], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.startswith("ok"), (args, r.stdout, r.stderr[-2000:])
