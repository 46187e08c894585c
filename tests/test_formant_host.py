"""Formant preservation, host side (no GPU): q3tts_load_opts_ex2, whose keep_formants sits directly behind the whole of
q3tts_load_opts_ex, and its ctypes mirror as a C compiler lays the header out; the pinned structs, ABI version and request size
unchanged; the new symbols and the Python surface; and the load-time refusals, reported before any GPU work -- on a machine
without a device they must come back as INVALID_INPUT, not as "no HIP device"."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.skipif(not shutil.which("gcc"), reason="gcc is not installed")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("q3tts_default_load_opts_ex2", "q3tts_model_load_ex2", "q3tts_model_get_keep_formants", "q3tts_pitch_shift_formants",
           "q3tts_debug_formant_rows")


def test_keep_formants_sits_behind_the_whole_of_the_extended_load_options(tmp_path):
    from qwen3tts import _lib as L
    assert L.LoadOptsEx2._fields_ == [("ex", L.LoadOptsEx), ("keep_formants", C.c_int32)]
    assert L.LoadOptsEx._fields_ == [("base", L.LoadOpts), ("pitch", C.c_float)]  # pinned, untouched
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "q3tts.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %d\\n", sizeof(q3tts_load_opts_ex2), offsetof(q3tts_load_opts_ex2, keep_formants),\n'
                   '         offsetof(q3tts_load_opts_ex2, ex), sizeof(q3tts_load_opts_ex), offsetof(q3tts_load_opts_ex, pitch),\n'
                   '         sizeof(q3tts_request), Q3TTS_ABI_VERSION);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, off, off_ex, ex, off_pitch, req, abi = (int(v) for v in subprocess.check_output([str(exe)], text=True).split())
    assert (size, off, off_ex) == (C.sizeof(L.LoadOptsEx2), L.LoadOptsEx2.keep_formants.offset, 0)
    assert ex == C.sizeof(L.LoadOptsEx) == off_pitch + 4  # pitch still ends q3tts_load_opts_ex
    assert off == ex and off + 4 == size                   # keep_formants directly behind it, nothing behind keep_formants
    assert abi == 4 and req == 88 == C.sizeof(L.Request)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "q3tts.h")).read(), flags=re.S)
    assert re.search(r"q3tts_load_opts_ex\s+ex;\s*int32_t\s+keep_formants;\s*}\s*q3tts_load_opts_ex2;", text)
    for name in SYMBOLS:
        assert name in text and hasattr(L.lib(), name), name


def test_defaults_and_the_python_surface():
    from qwen3tts import Qwen3TTSModel, _lib as L
    o = L.LoadOptsEx2()
    o.keep_formants, o.ex.pitch, o.ex.base.max_frames = 1, 5.0, 7
    L.lib().q3tts_default_load_opts_ex2(C.byref(o))
    assert o.keep_formants == 0 and o.ex.pitch == 0.0 and o.ex.base.speed == 0.0 and o.ex.base.max_frames == 2048 and o.ex.base.use_graph == 1
    assert inspect.signature(Qwen3TTSModel.from_pretrained).parameters["keep_formants"].default is False
    assert inspect.signature(Qwen3TTSModel.pitch_shift).parameters["keep_formants"].default is False
    for name in ("keep_formants_info", "debug_formant_rows"):
        assert hasattr(Qwen3TTSModel, name)
    # the entry points without a handle: INVALID_INPUT, nothing touched
    on = C.c_int32(-1)
    assert L.lib().q3tts_model_get_keep_formants(None, C.byref(on)) == 3 and on.value == -1
    n = C.c_int64(-1)
    assert L.lib().q3tts_pitch_shift_formants(None, None, 0, 1.0, None, 0, C.byref(n)) == 3 and n.value == -1
    assert L.lib().q3tts_debug_formant_rows(None, 0, 480, 480, None, 1, None, 1, 0, None, 24, None, None, None, 1, 0) == 3


def test_the_cli_and_the_bench_tool_offer_the_option():
    import sys
    env = {**os.environ, "PYTHONPATH": os.path.join(ROOT, "swift-qwen3-tts_amd")}
    out = subprocess.run([sys.executable, "-m", "qwen3tts", "--help"], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0 and "--keep-formants" in out.stdout
    assert "--keep-formants" in open(os.path.join(ROOT, "tools", "queued_bench.py")).read()


def test_load_time_refusals_need_no_gpu(tmp_path):
    """Refused before the first call into the GPU runtime and before the checkpoint is read (the directory does not exist):
    keep_formants other than 0 / 1, and keep_formants with an output rate other than 24000."""
    from qwen3tts import Qwen3TTSModel
    from qwen3tts.model import Qwen3TTSError
    nowhere = str(tmp_path / "no_such_checkpoint")

    def load(**kw):
        with pytest.raises(Qwen3TTSError) as e:
            Qwen3TTSModel.from_pretrained(nowhere, **kw)
        return e.value.status, str(e.value)

    for bad in (2, -1, 7, 1 << 20):
        st, msg = load(pitch=4.0, keep_formants=bad)
        assert st == 3 and "keep_formants must be 0 or 1" in msg, bad
        st, msg = load(keep_formants=bad)
        assert st == 3 and "keep_formants must be 0 or 1" in msg, bad
    for rate in (8000, 16000, 22050, 44100, 48000):
        for pitch in (4.0, 0.0):
            st, msg = load(pitch=pitch, keep_formants=True, output_sample_rate=rate)
            assert st == 3 and "keep_formants needs output_sample_rate 0 or 24000" in msg, (rate, pitch)
    # the pitch's own refusals stay what they were
    st, msg = load(pitch=13.0, keep_formants=True)
    assert st == 3 and "pitch must be" in msg
    st, msg = load(pitch=2.0, keep_formants=True, request_speeds=True)
    assert st == 3 and "request_speeds" in msg
    # admissible combinations pass these checks: whatever stops the load then is not one of them
    for kw in (dict(keep_formants=True), dict(pitch=4.0, keep_formants=True), dict(pitch=-5.0, keep_formants=True, output_sample_rate=24000),
               dict(pitch=4.0, speed=1.25, keep_formants=True), dict(pitch=4.0, keep_formants=0), dict(pitch=4.0, keep_formants=1)):
        st, msg = load(**kw)
        assert "keep_formants" not in msg and "pitch must" not in msg, (kw, msg)
