"""Child process of tests/test_concurrent_jobs.py::test_model_freed_with_two_background_jobs_outstanding (a crash here must not
take the test run with it)."""
import os
import sys
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "swift-qwen3-tts_amd"))
sys.path.insert(0, HERE)
import tempfile
from qwen3tts import Qwen3TTSModel, GenerationRequest, synth
from conftest import tiny_request
d = tempfile.mkdtemp(); synth.write_checkpoint(d, "tiny-b", seed=1234)
def req(row, n):
    r = tiny_request(row=row, n_text=n)
    return GenerationRequest(r["text_ids"], r["target_token_count"], r["instruct_ids"], r["speaker"], r["language"])
load = dict(max_batch=4, max_frames=200, max_prompt=64)
m = Qwen3TTSModel.from_pretrained(d, **load)
kw = dict(temperature=0.9, top_k=40, seed=9, force_frames=190)
want = m.generate_batch([req(0, 6), req(1, 7)], **kw)
m.generate_batch([req(2, 6)], **kw)  # (the second context's graph: the jobs below go straight into their frame loops)
j1 = m.generate_batch_begin([req(0, 6), req(1, 7)], **kw)  # no callbacks: both frame loops run on the workers
j2 = m.generate_batch_begin([req(2, 6)], more_follows=False, **kw)
m.close()          # two background jobs outstanding, never ended
print("closed with two background jobs outstanding")
m = Qwen3TTSModel.from_pretrained(d, **load)
got = m.generate_batch([req(0, 6), req(1, 7)], **kw)
assert all((a.codes == b.codes).all() and (a.audio == b.audio).all() for a, b in zip(got, want))
m.close()
print("ok")
