"""bench.py's plain run and --dump-outputs on CPU: the one-process control path with the engine replaced by the stand-in of
tests/_bench_dry.py (Q3TTS_BENCH_DRY=1), and the dump writer on hand-made results (ragged rows, a sample under the budget)."""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_times_the_given_steps_and_dumps_the_last_one(tmp_path):
    env = dict(os.environ, Q3TTS_BENCH_DRY="1")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1", "--frames", "8",
           "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d
    assert d["steps"] == 4 and "streaming" not in d and "cpu_baseline" not in d  # both only with --full
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 * d["steps"] - 32 * 8 * 4) < 1e-6 * 32 * 8 * 4
    codes = np.load(tmp_path / "out" / "codes.npy")
    assert codes.dtype == np.float32 and codes.shape == (32, 8, 16)
    assert (np.load(tmp_path / "out" / "frames.npy") == 8).all()


def test_dump_pads_ragged_rows_and_samples_rows_beyond_the_budget(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import bench

    def res(frames, samples, status=0):
        return SimpleNamespace(codes=np.arange(frames * 16, dtype=np.int32).reshape(frames, 16),
                               audio=np.full(samples, 0.5, np.float32), status=status)

    rows = [res(3, 30), res(5, 50), res(0, 0, status=2), res(4, 40)]
    bench.dump_outputs(str(tmp_path / "all"), rows)
    codes = np.load(tmp_path / "all" / "codes.npy")
    audio = np.load(tmp_path / "all" / "audio.npy")
    assert codes.shape == (4, 5, 16) and audio.shape == (4, 50)
    assert (codes[0, :3] == rows[0].codes).all() and (codes[0, 3:] == -1).all() and (codes[2] == -1).all()
    assert (audio[0, :30] == 0.5).all() and (audio[0, 30:] == 0).all()
    assert list(np.load(tmp_path / "all" / "status.npy")) == [0, 0, 2, 0]
    assert list(np.load(tmp_path / "all" / "audio_rows.npy")) == [0, 1, 2, 3]

    many = [res(2, 1000) for _ in range(40)]
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 20_000)
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), many)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    picked = np.load(tmp_path / "a" / "audio_rows.npy")
    assert 0 < picked.size < 40 and total <= 20_000
    assert (picked == np.load(tmp_path / "b" / "audio_rows.npy")).all()  # the sample is fixed
    assert np.load(tmp_path / "a" / "codes.npy").shape == (40, 2, 16)  # codes are always whole
