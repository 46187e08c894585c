"""In-kernel timeline of the talker's 32-row decode GEMMs (gate/up, down_proj and qkv), from the diagnostic library
(`make -C swift-qwen3-tts_amd TIMELINE=1`, csrc/kernels/gemm_body.inc): per-wave clock stamps of the first and the last workgroup of
the LAST such launch of a short generation on the bench's 1.7B checkpoint (hipGraph replay, one job alone), once with the parent's
forms (Q3TTS_GEMM_PARENT_FORMS=1) and once with the default ones.

    Q3TTS_LIB=swift-qwen3-tts_amd/qwen3tts/libq3tts_hip_timeline.so python tools/gemm_timeline.py [--frames 12] > timeline.txt

Times are microseconds after the earliest wave start of the launch's first workgroup (100 MHz clock: steps of 0.01 us). The
stamps fence the scheduler, so read shares, not the launch's length."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "swift-qwen3-tts_amd")]

FORMS = ["gate/up <2,2,8,2,true,false,3,true>, chunk-major (parent)", "gate/up <2,2,8,2,true,false,3,true,TM>, tile-major",
         "down_proj <1,3,8,6,false,false,1,true>", "qkv <2,0,8,2,true,false,1,true>"]
STAMPS = ["start", "prologue", "mfma first", "mfma last", "partials", "reduced", "stored"]   # stamps 0..6; 7 = first tile reduced


def table(raw, out, forms):
    for f in forms:   # (the buffer keeps an earlier run's stamps of a form this run did not launch)
        name = FORMS[f]
        t = [[[raw[((f * 2 + g) * 8 + w) * 8 + k] for k in range(8)] for w in range(8)] for g in range(2)]
        if not any(t[0][w][6] for w in range(8)):
            continue
        t0 = min(t[0][w][0] for w in range(8))
        print("\n## %s" % name, file=out)
        print("%-16s %s   first tile reduced" % ("workgroup wave", " ".join("%11s" % s for s in STAMPS)), file=out)
        for g, gname in enumerate(("first", "last")):
            for w in range(8):
                r = t[g][w]
                cells = " ".join("%11.2f" % ((r[k] - t0) / 100.0) for k in range(7))
                first = "%11.2f" % ((r[7] - t0) / 100.0) if r[7] else "%11s" % "-"
                print("%-5s %-10d %s   %s" % (gname, w, cells, first), file=out)
        seg = []
        for k in range(1, 7):
            d = [t[g][w][k] - t[g][w][k - 1] for g in range(2) for w in range(8)]
            seg.append("%s %.2f" % (STAMPS[k], sum(d) / len(d) / 100.0))
        life = [t[g][w][6] - t[g][w][0] for g in range(2) for w in range(8)]
        print("mean segment (us, ending at): %s | wave life %.2f" % (", ".join(seg), sum(life) / len(life) / 100.0), file=out)


def run(parent, frames, out):
    from bench import build_requests, ensure_checkpoint
    from qwen3tts import Qwen3TTSModel, _lib
    if parent:
        os.environ["Q3TTS_GEMM_PARENT_FORMS"] = "1"
    else:
        os.environ.pop("Q3TTS_GEMM_PARENT_FORMS", None)
    _lib.reload_debug_env()
    lib = _lib.lib()
    if not hasattr(lib, "q3tts_debug_gemm_timeline"):
        sys.exit("the loaded library has no timeline: build with TIMELINE=1 and point Q3TTS_LIB at it")
    ckpt = ensure_checkpoint("1.7b", 0, None)
    m = Qwen3TTSModel.from_pretrained(ckpt, device=0, max_batch=32, max_frames=frames + 8, max_prompt=128)
    reqs = build_requests("1.7b", 0, 32, 32, 16)
    for _ in range(3):   # calls alternate between two contexts: the third replays the first one's captured frame graphs
        m.generate_batch(reqs, temperature=0.9, top_k=50, top_p=1.0, repetition_penalty=1.05, seed=1234, force_frames=frames)
    raw = (C.c_ulonglong * (4 * 2 * 8 * 8))()
    lib.q3tts_debug_gemm_timeline.argtypes = [C.POINTER(C.c_ulonglong)]
    st = lib.q3tts_debug_gemm_timeline(raw)
    m.close()
    if st != 0:
        sys.exit("q3tts_debug_gemm_timeline failed: %d" % st)
    print("\n# %s forms, 1.7B, 32 rows, %d frames, last launch of each form" % ("parent (Q3TTS_GEMM_PARENT_FORMS=1)" if parent else "default", frames), file=out)
    table(list(raw), out, (0, 2, 3) if parent else (1, 2, 3))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=12)
    a = ap.parse_args()
    run(True, a.frames, sys.stdout)
    run(False, a.frames, sys.stdout)
