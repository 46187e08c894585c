"""The slotted stream's planner (csrc/stream_plan.h) for rows that carry a reference prefix -- streamed voice-clone rows.

A driver of its own (tests/native/stream_plan_prefix_driver.cc) replays the queue's schedule with a prefix per request. The
definition (include/q3tts.h, q3tts_codec_decode_streamed_prefixed) is restated in clone_chunks below; per request the planner
must issue exactly that sequence: every prefix chunk before any generated one, prefix chunks with no generated frame at all,
generated chunks no sooner than their lookahead allows. With prefix 0 everything is what tests/test_stream_plan.py pins."""
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "swift-qwen3-tts_amd", "csrc")

pytestmark = pytest.mark.skipif(not shutil.which("g++"), reason="g++ is not installed")


def _build(name):
    out = os.path.join(NATIVE, "_build", name)
    deps = [os.path.join(NATIVE, name + ".cc"), os.path.join(CSRC, "stream_plan.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        # no HIP include path and no platform define: the planner must stay host-only
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I" + CSRC, deps[0], "-o", out])
    return out


@pytest.fixture(scope="module")
def driver():
    return _build("stream_plan_prefix_driver")


def clone_chunks(R, n, C, W, L):
    """(emit, k, f0, w0, window length, take) of a row with R reference frames in front of n generated ones, in code-buffer
    coordinates (the buffer holds ref ++ gen): the prefix's lookahead stops at R, a generated window reaches back into it."""
    out = []
    for j in range((R + C - 1) // C):
        f0 = j * C
        w0 = max(0, f0 - W)
        out.append((0, j, f0, w0, min(R, f0 + C + L) - w0, min(R, f0 + C) - f0))
    for k in range((n + C - 1) // C):
        f0 = R + k * C
        w0 = max(0, f0 - W)
        out.append((1, k, f0, w0, min(R + n, f0 + C + L) - w0, min(R + n, f0 + C) - f0))
    return out


def _replay(driver, cases):
    text = "".join("%d %d %d %d %d %d %d %s\n" % (C, W, L, F, s, b, len(n), " ".join("%d %d" % rn for rn in n))
                   for C, W, L, F, s, b, n in cases)
    out = subprocess.run([driver], input=text, capture_output=True, text=True, timeout=120, check=True).stdout
    parsed, cur = [], None
    for line in out.splitlines():
        w = line.split()
        if w[0] == "case":
            cur = []
        elif w[0] == "end":
            parsed.append(cur)
        else:
            cur.append((w[0], [int(x) for x in w[1:]]))
    assert len(parsed) == len(cases)
    return parsed


def _cases():
    rng = random.Random(4131)
    cases = []
    # the issue's geometry: every prefix residue against chunk 4 (0, 1 -- below the tail's history of 3 --, C - 1), ragged counts
    for slots, burst in ((1, 1), (3, 2), (4, 5), (2, 64)):
        cases.append((4, 16, 2, 64, slots, burst, [(R, n) for R in (0, 1, 4, 7, 13) for n in (1, 5, 9, 14)]))
    for _ in range(200):
        C, W, L = rng.randint(3, 16), rng.randint(0, 32), rng.randint(0, 6)
        reqs = [(rng.choice([0, 0, 1, C - 1, C, C + 1, rng.randint(1, 40)]), rng.randint(1, 60)) for _ in range(rng.randint(1, 10))]
        cases.append((C, W, L, 64, rng.randint(1, 4), rng.randint(1, 12), reqs))
    return cases


def test_prefixed_rows_follow_the_definition(driver):
    cases = _cases()
    for (C, W, L, F, slots, burst, reqs), log in zip(cases, _replay(driver, cases)):
        tag = (C, W, L, slots, burst, reqs)
        occupant, got, state = {}, {i: [] for i in range(len(reqs))}, None
        probe = []
        for kind, v in log:
            if kind == "probe":
                probe.append(tuple(v))
            elif kind == "push":
                state = list(zip(v[0::2], v[1::2]))
            elif kind == "admit":
                s, r = v
                if s in occupant:  # the previous occupant had every chunk issued before its slot was handed on
                    assert got[occupant[s]] == clone_chunks(*reqs[occupant[s]], C, W, L), ("slot reused early", tag)
                occupant[s] = r
            elif kind == "row":
                s, r, k, f0, w0, wlen, take, emit = v
                assert occupant.get(s) == r, ("a row took part before its reset", tag)
                R = reqs[r][0]
                avail, fin = state[s]
                if emit:
                    # nothing is emitted before the prefix is through, and no generated chunk leaves before it is decodable
                    assert [c[0] for c in got[r]].count(0) == (R + C - 1) // C, ("audio before the prefix was through", tag)
                    assert fin or avail >= (k + 1) * C + L, ("a chunk left before it was decodable", tag)
                    assert w0 + wlen <= R + avail and f0 + take <= R + avail, ("a window past the frames that exist", tag)
                else:
                    assert w0 + wlen <= R and f0 + take <= R, ("a prefix chunk beyond the reference", tag)
                got[r].append((emit, k, f0, w0, wlen, take))
        for i, (R, n) in enumerate(reqs):
            assert got[i] == clone_chunks(R, n, C, W, L), (i, R, n, tag)
        # with no generated frame at all, request 0 is given its whole prefix and nothing else
        R0 = reqs[0][0]
        assert probe == [(k, f0, w0, wlen, take, 0) for _, k, f0, w0, wlen, take in clone_chunks(R0, 0, C, W, L)], tag


def test_prefix_zero_is_the_plain_planner(driver):
    """The same schedules through the driver of tests/test_stream_plan.py (no prefix argument anywhere) and through this one
    with prefix 0: the same admissions, pushes and passes, field for field, and every row emits."""
    plain = _build("stream_plan_driver")
    rng = random.Random(77)
    cases = [(rng.randint(3, 16), rng.randint(0, 32), rng.randint(0, 6), 64, rng.randint(1, 4), rng.randint(1, 12),
              [rng.randint(1, 60) for _ in range(rng.randint(1, 12))]) for _ in range(100)]
    text = "".join("%d %d %d %d %d %d %d %s\n" % (C, W, L, F, s, b, len(n), " ".join(map(str, n))) for C, W, L, F, s, b, n in cases)
    want = subprocess.run([plain], input=text, capture_output=True, text=True, timeout=120, check=True).stdout.splitlines()
    got = []
    for case in _replay(driver, [(C, W, L, F, s, b, [(0, c) for c in n]) for C, W, L, F, s, b, n in cases]):
        got.append("case")
        for kind, v in case:
            assert kind != "probe"  # no prefix: nothing is decodable without a frame
            if kind == "row":
                assert v[-1] == 1
                v = v[:-1]
            got.append(" ".join([kind] + [str(x) for x in v]))
        got.append("end")
    assert got == want
