"""q3tts_default_sampling leaves per_request NULL, so a caller that never heard of per-request parameters gets the behaviour
it had. (tests/test_abi.py compares the layouts of q3tts_row_sampling and the grown q3tts_sampling with the header.)"""
import ctypes as C


def test_default_sampling_has_no_per_request_array():
    from qwen3tts import _lib as L
    s = L.Sampling()
    C.memset(C.byref(s), 0xff, C.sizeof(s))
    L.lib().q3tts_default_sampling(C.byref(s))
    assert not s.per_request
    assert (round(s.temperature, 3), s.top_k, s.top_p, round(s.repetition_penalty, 3), s.seed, s.row_base) == (0.9, 50, 1.0, 1.05, 0, 0)


def test_request_sampling_marshals_only_what_is_set():
    from qwen3tts import GenerationRequest, Qwen3TTSModel, RequestSampling
    from qwen3tts import _lib as L
    reqs = [GenerationRequest([1, 2, 3], 1), GenerationRequest([1, 2, 3], 1, sampling=RequestSampling(top_p=0.5, seed=2 ** 40)),
            GenerationRequest([1, 2, 3], 1, sampling=RequestSampling())]
    assert reqs[0].sampling is None and GenerationRequest([1], 1, None, "a", "b", 7, None, None, 2).route == 2
    s = Qwen3TTSModel._sampling(0.9, 50, 1.0, 1.05, 0, 0, reqs=reqs)
    rows = s.per_request
    assert [rows[i].set for i in range(3)] == [0, L.ROW_TOP_P | L.ROW_SEED, 0]
    assert rows[1].top_p == 0.5 and rows[1].seed == 2 ** 40
    assert not Qwen3TTSModel._sampling(0.9, 50, 1.0, 1.05, 0, 0, reqs=reqs[:1]).per_request


def test_row_sampling_mirror_has_the_headers_layout(tmp_path):
    """q3tts_row_sampling and its Q3TTS_ROW_* bits against the ctypes mirror, as a C compiler lays the header out."""
    import os
    import subprocess
    from qwen3tts import _lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = [f for f, _ in L.RowSampling._fields_]
    bits = ["TEMPERATURE", "TOP_K", "TOP_P", "REPETITION_PENALTY", "SEED"]
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "q3tts.h"', 'int main(void) {',
             '  printf("%zu %d\\n", sizeof(q3tts_row_sampling), Q3TTS_ABI_VERSION);']
    lines += ['  printf("%%zu\\n", offsetof(q3tts_row_sampling, %s));' % f for f in fields]
    lines += ['  printf("%%u\\n", Q3TTS_ROW_%s);' % b for b in bits]
    lines += ['  return 0;', '}']
    src = tmp_path / "row.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "row"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).split()
    assert int(out[0]) == C.sizeof(L.RowSampling) and int(out[1]) == 4
    assert [int(x) for x in out[2:2 + len(fields)]] == [getattr(L.RowSampling, f).offset for f in fields]
    assert [int(x) for x in out[2 + len(fields):]] == [getattr(L, "ROW_" + b) for b in bits]
