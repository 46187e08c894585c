"""Pitch per handle, host side (no GPU): q3tts_load_opts_ex, whose last field the pitch is, and its ctypes mirror as a C compiler
lays the header out, the unchanged ABI version and request size, the Python surface, and the load-time refusals that are reported before any GPU
work -- on a machine without a device they must come back as INVALID_INPUT, not as "no HIP device"."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.skipif(not shutil.which("gcc"), reason="gcc is not installed")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pitch_is_the_last_field_of_the_extended_load_options(tmp_path):
    """q3tts_load_opts keeps its layout and its last field (tests/test_request_speed_host.py pins request_speeds there): the
    pitch is the last field of q3tts_load_opts_ex, directly behind the whole of q3tts_load_opts. The compiled header and the
    ctypes mirrors agree on both structs."""
    from qwen3tts import _lib as L
    assert L.LoadOptsEx._fields_ == [("base", L.LoadOpts), ("pitch", C.c_float)]
    assert L.LoadOpts._fields_[-1][0] == "request_speeds" and "pitch" not in [f[0] for f in L.LoadOpts._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "q3tts.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %d\\n", sizeof(q3tts_load_opts_ex), offsetof(q3tts_load_opts_ex, pitch),\n'
                   '         offsetof(q3tts_load_opts_ex, base), sizeof(q3tts_load_opts), offsetof(q3tts_load_opts, request_speeds),\n'
                   '         sizeof(q3tts_request), Q3TTS_ABI_VERSION);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, off, off_base, base, off_rs, req, abi = (int(v) for v in subprocess.check_output([str(exe)], text=True).split())
    assert (size, off, off_base) == (C.sizeof(L.LoadOptsEx), L.LoadOptsEx.pitch.offset, 0)
    assert base == C.sizeof(L.LoadOpts) == off_rs + 4  # request_speeds still ends q3tts_load_opts
    assert off == base and off + 4 == size             # pitch directly behind it, nothing behind pitch
    assert abi == 4 and req == 88 == C.sizeof(L.Request)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "q3tts.h")).read(), flags=re.S)
    assert re.search(r"q3tts_load_opts\s+base;\s*float\s+pitch;\s*}\s*q3tts_load_opts_ex;", text)
    for name in ("q3tts_model_load_ex", "q3tts_default_load_opts_ex", "q3tts_model_get_pitch", "q3tts_pitch_shift", "q3tts_debug_resample_ratio"):
        assert name in text and hasattr(L.lib(), name)


def test_defaults_and_the_python_surface():
    from qwen3tts import Qwen3TTSModel, _lib as L
    o = L.LoadOptsEx()
    o.pitch, o.base.max_frames = 5.0, 7
    L.lib().q3tts_default_load_opts_ex(C.byref(o))
    assert o.pitch == 0.0 and o.base.speed == 0.0 and o.base.request_speeds == 0 and o.base.max_frames == 2048 and o.base.use_graph == 1
    assert inspect.signature(Qwen3TTSModel.from_pretrained).parameters["pitch"].default == 0.0
    for name in ("pitch_info", "pitch_shift", "debug_resample_ratio"):
        assert hasattr(Qwen3TTSModel, name)
    # the entry points without a handle: INVALID_INPUT, nothing touched
    s, hp = C.c_float(-1), C.c_int32(-1)
    assert L.lib().q3tts_model_get_pitch(None, C.byref(s), C.byref(hp), None, None) == 3 and hp.value == -1
    n = C.c_int64(-1)
    assert L.lib().q3tts_pitch_shift(None, None, 0, 1.0, None, 0, C.byref(n)) == 3 and n.value == -1


def test_load_time_refusals_need_no_gpu(tmp_path):
    """Refused before the first call into the GPU runtime and before the checkpoint is read (the directory does not exist): a
    pitch out of range, NaN or infinite; a pitch together with request_speeds; no Hp in [240, 960] for the speed. (A codec frame
    that is not whole 480-sample hops is known only from the checkpoint: the runner refuses it, tests/test_pitch_gpu.py.)"""
    from qwen3tts import Qwen3TTSModel
    from qwen3tts.model import Qwen3TTSError
    nowhere = str(tmp_path / "no_such_checkpoint")

    def load(**kw):
        with pytest.raises(Qwen3TTSError) as e:
            Qwen3TTSModel.from_pretrained(nowhere, **kw)
        return e.value.status, str(e.value)

    for bad in (12.001, -12.001, 13, -100, float("nan"), float("inf"), float("-inf")):
        st, msg = load(pitch=bad)
        assert st == 3 and "pitch must be" in msg, bad
    st, msg = load(pitch=2.0, request_speeds=True)
    assert st == 3 and "request_speeds" in msg
    for kw in (dict(pitch=12.0, speed=0.8), dict(pitch=1.0, speed=0.5), dict(pitch=-1.0, speed=2.0), dict(pitch=-12.0, speed=1.25),
               dict(pitch=12.0, speed=0.8, output_sample_rate=16000)):
        st, msg = load(**kw)
        assert st == 3 and "no hop in [240, 960]" in msg, kw
    # admissible combinations pass these checks: whatever stops the load then is not a pitch refusal
    for kw in (dict(pitch=0.0), dict(pitch=2.0), dict(pitch=-12.0), dict(pitch=12.0), dict(pitch=3.86, speed=1.25),
               dict(pitch=2.0, output_sample_rate=16000), dict(pitch=0.0, request_speeds=True)):
        st, msg = load(**kw)
        assert "pitch" not in msg and "no hop" not in msg, (kw, msg)
