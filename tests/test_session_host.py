"""The serving session without a GPU: the C ABI additions (symbols, struct layouts, status codes) and the session's host-only
bookkeeping (csrc/session_queue.h) under the sanitizers.

tests/native/session_queue_driver.cc has its own main over session_queue.h alone: several producer threads, one consumer and
one canceller. It checks that tickets are dense and ordered, that take-next order equals ticket order, that a cancelled pending
ticket is never handed out, that every wait wakes, and that results are freed exactly once. It is built and run once with the
address and undefined-behaviour sanitizers and once with the thread sanitizer; nothing loaded into Python is instrumented."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "swift-qwen3-tts_amd", "csrc")

SESSION_SYMBOLS = ["q3tts_session_open", "q3tts_session_submit", "q3tts_session_cancel", "q3tts_session_wait",
                   "q3tts_session_get_stats", "q3tts_session_close"]


def test_session_symbols_are_exported():
    from qwen3tts import _lib as L
    lib = C.CDLL(L.LIB_PATH)
    for name in SESSION_SYMBOLS:
        assert hasattr(lib, name), name


def test_session_structs_have_the_headers_layout(tmp_path):
    """q3tts_session_opts / q3tts_session_stats and the two new status codes against the ctypes mirror, as a C99 compiler lays
    the header out; the ABI version the existing tests pin has not moved."""
    from qwen3tts import _lib as L
    structs = [("q3tts_session_opts", L.SessionOpts), ("q3tts_session_stats", L.SessionStats)]
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "q3tts.h"', 'int main(void) {',
             '  q3tts_session* s = NULL;', '  (void)s;',
             '  printf("%d %d %d\\n", Q3TTS_ABI_VERSION, (int)Q3TTS_ERR_CANCELLED, (int)Q3TTS_ERR_BUSY);']
    for cname, mirror in structs:
        lines.append('  printf("%%zu\\n", sizeof(%s));' % cname)
        lines += ['  printf("%%zu\\n", offsetof(%s, %s));' % (cname, f) for f, _ in mirror._fields_]
    lines += ['  return 0;', '}']
    src = tmp_path / "session_abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "session_abi"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert out[:3] == [4, 8, 9]
    assert (L.ERR_CANCELLED, L.ERR_BUSY) == (8, 9)
    want = []
    for _, mirror in structs:
        want.append(C.sizeof(mirror))
        want += [getattr(mirror, f).offset for f, _ in mirror._fields_]
    assert out[3:] == want


def test_python_surface():
    from qwen3tts import Qwen3TTSModel, Session
    assert callable(Qwen3TTSModel.open_session)
    for name in ("submit", "result", "cancel", "stats", "close", "__enter__", "__exit__"):
        assert callable(getattr(Session, name))


def _sanitized(flags):
    probe = subprocess.run(["g++", "-x", "c++", "-", "-o", os.devnull, "-pthread", *flags], input="int main(){return 0;}",
                           capture_output=True, text=True)
    return probe.returncode == 0


@pytest.mark.skipif(not shutil.which("g++"), reason="g++ is not installed")
@pytest.mark.parametrize("name,flags", [("asan_ubsan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]),
                                        ("tsan", ["-fsanitize=thread"])])
def test_session_queue_driver_under_sanitizers(name, flags):
    if not _sanitized(flags):
        pytest.skip("g++ cannot link with " + flags[0])
    out = os.path.join(NATIVE, "_build", "session_queue_driver_" + name)
    deps = [os.path.join(NATIVE, "session_queue_driver.cc"), os.path.join(CSRC, "session_queue.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        # no HIP include path and no platform define: the session's bookkeeping must stay host-only
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-pthread", *flags, "-I" + CSRC, deps[0], "-o", out])
    for args in (["4", "200", "16"], ["6", "50", "2"], ["1", "100", "0"]):
        r = subprocess.run([out, *args], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.startswith("ok"), (args, r.stdout, r.stderr[-2000:])
