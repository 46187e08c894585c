"""Live voices of a serving session without a GPU: the C ABI additions (symbols, struct layouts, an unmoved ABI version), the
Python surface, and the session's host-only voice bookkeeping (csrc/session_queue.h) under the sanitizers.

tests/native/session_voice_driver.cc has its own main over session_queue.h alone (its header lists what it checks). It is built
and run once with the address and undefined-behaviour sanitizers and once with the thread sanitizer, as
tests/test_session_host.py does its driver; nothing loaded into Python is instrumented."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "swift-qwen3-tts_amd", "csrc")

VOICE_SYMBOLS = ["q3tts_session_open_ex", "q3tts_session_voice_create", "q3tts_session_voice_wait", "q3tts_session_voice_free",
                 "q3tts_session_get_voice_stats"]


def test_live_voice_symbols_are_exported():
    from qwen3tts import _lib as L
    lib = C.CDLL(L.LIB_PATH)
    for name in VOICE_SYMBOLS:
        assert hasattr(lib, name), name


def test_live_voice_structs_have_the_headers_layout(tmp_path):
    """q3tts_session_opts_ex / q3tts_session_voice_stats against the ctypes mirrors, as a C99 compiler lays the header out; the
    structs that were there keep their sizes and the ABI version has not moved."""
    from qwen3tts import _lib as L
    structs = [("q3tts_session_opts_ex", L.SessionOptsEx), ("q3tts_session_voice_stats", L.SessionVoiceStats)]
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "q3tts.h"', 'int main(void) {',
             '  printf("%d %zu %zu\\n", Q3TTS_ABI_VERSION, sizeof(q3tts_session_opts), sizeof(q3tts_session_stats));']
    for cname, mirror in structs:
        lines.append('  printf("%%zu\\n", sizeof(%s));' % cname)
        lines += ['  printf("%%zu\\n", offsetof(%s, %s));' % (cname, f) for f, _ in mirror._fields_]
    lines += ['  return 0;', '}']
    src = tmp_path / "session_voice_abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "session_voice_abi"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert out[:3] == [4, C.sizeof(L.SessionOpts), C.sizeof(L.SessionStats)]
    want = []
    for _, mirror in structs:
        want.append(C.sizeof(mirror))
        want += [getattr(mirror, f).offset for f, _ in mirror._fields_]
    assert out[3:] == want
    assert L.SessionOptsEx.base.offset == 0 and C.sizeof(L.SessionOptsEx) == C.sizeof(L.SessionOpts) + 8


def test_python_surface():
    from qwen3tts import Qwen3TTSModel, Session, Voice
    sig = inspect.signature(Qwen3TTSModel.open_session)
    assert sig.parameters["live_voices"].default == 0 and sig.parameters["max_voices"].default == 0
    for name in ("create_voice", "voice_stats"):
        assert callable(getattr(Session, name))
    assert inspect.signature(Session.create_voice).parameters["sample_rate"].default == 24000
    for name in ("wait", "close"):
        assert callable(getattr(Voice, name))


def _sanitized(flags):
    probe = subprocess.run(["g++", "-x", "c++", "-", "-o", os.devnull, "-pthread", *flags], input="int main(){return 0;}",
                           capture_output=True, text=True)
    return probe.returncode == 0


@pytest.mark.skipif(not shutil.which("g++"), reason="g++ is not installed")
@pytest.mark.parametrize("name,flags", [("asan_ubsan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]),
                                        ("tsan", ["-fsanitize=thread"])])
def test_session_voice_driver_under_sanitizers(name, flags):
    if not _sanitized(flags):
        pytest.skip("g++ cannot link with " + flags[0])
    out = os.path.join(NATIVE, "_build", "session_voice_driver_" + name)
    deps = [os.path.join(NATIVE, "session_voice_driver.cc"), os.path.join(CSRC, "session_queue.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        # no HIP include path and no platform define: the session's bookkeeping must stay host-only
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-pthread", *flags, "-I" + CSRC, deps[0], "-o", out])
    # producers, voices per producer, live_voices, max_voices
    for args in (["4", "60", "2", "5"], ["6", "25", "1", "1"], ["2", "40", "4", "16"]):
        r = subprocess.run([out, *args], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.startswith("ok"), (args, r.stdout, r.stderr[-2000:])
