"""The host-only planner of the slotted codec stream (csrc/stream_plan.h): which rows of a queue decode which chunk in a pass.

A small driver (tests/native/stream_plan_driver.cc) replays the queue's schedule -- requests take free slots in order, running
requests gain `burst` frames per step, a finished one is retired and its slot reset and refilled -- and prints every pass. Per
request the sequence of (k, f0, w0, window length, take) must be the chunk definition of include/q3tts.h, restated below;
every chunk is issued exactly once and in order, no row takes part before its reset, and no pass is empty."""
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "swift-qwen3-tts_amd", "csrc")

pytestmark = pytest.mark.skipif(not shutil.which("g++"), reason="g++ is not installed")


@pytest.fixture(scope="module")
def driver():
    out = os.path.join(NATIVE, "_build", "stream_plan_driver")
    deps = [os.path.join(NATIVE, "stream_plan_driver.cc"), os.path.join(CSRC, "stream_plan.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        # no HIP include path and no platform define: the planner must stay host-only
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I" + CSRC, deps[0], "-o", out])
    return out


def chunks_of(n, C, W, L):
    """The chunk definition: chunk k of a request with n frames covers [kC, min(n, (k+1)C)), its window is
    [max(0, kC - W), min(n, (k+1)C + L))."""
    out = []
    for k in range((n + C - 1) // C):
        f0 = k * C
        w0 = max(0, f0 - W)
        out.append((k, f0, w0, min(n, f0 + C + L) - w0, min(n, f0 + C) - f0))
    return out


def _cases(seed, count):
    rng = random.Random(seed)
    cases = []
    for _ in range(count):
        C, W, L = rng.randint(3, 16), rng.randint(0, 32), rng.randint(0, 6)
        slots, burst = rng.randint(1, 4), rng.randint(1, 12)
        counts = [rng.randint(1, 60) for _ in range(rng.randint(1, 12))]
        cases.append((C, W, L, 64, slots, burst, counts))
    # the corners by hand: a request shorter than a chunk, an exact multiple, everything final on arrival, one slot
    cases.append((8, 16, 2, 64, 3, 9, [23, 5, 40, 11, 7, 33, 16, 6, 28, 14]))
    cases.append((8, 16, 2, 64, 1, 64, [40, 1, 8, 16]))
    cases.append((3, 0, 0, 64, 2, 1, [1, 2, 3, 4, 60]))
    return cases


def _replay(driver, cases):
    text = "".join("%d %d %d %d %d %d %d %s\n" % (C, W, L, F, s, b, len(n), " ".join(map(str, n))) for C, W, L, F, s, b, n in cases)
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


def test_planner_follows_the_chunk_definition(driver):
    cases = _cases(20260, 300)
    for (C, W, L, F, slots, burst, counts), log in zip(cases, _replay(driver, cases)):
        tag = (C, W, L, slots, burst, counts)
        occupant = {}                     # slot -> request, from the admissions
        got = {i: [] for i in range(len(counts))}
        admitted = []
        in_pass, rows_in_pass, state = False, 0, None
        for kind, v in log + [("push", [])]:  # (the sentinel closes the last pass)
            if kind in ("pass", "push", "admit"):
                assert not in_pass or rows_in_pass > 0, ("an empty pass", tag)
                in_pass, rows_in_pass, seen_slots = kind == "pass", 0, set()
            if kind == "push":
                state = list(zip(v[0::2], v[1::2]))
            elif kind == "admit":
                s, r = v
                # the previous occupant had every chunk issued before its slot was handed on
                if s in occupant:
                    assert got[occupant[s]] == chunks_of(counts[occupant[s]], C, W, L), ("slot reused early", tag)
                occupant[s] = r
                admitted.append(r)
            elif kind == "row":
                s, r, k, f0, w0, wlen, take = v
                assert in_pass and 0 <= s < slots
                assert occupant.get(s) == r, ("a row took part before its reset", tag)
                assert s not in seen_slots, ("a row twice in one pass", tag)
                seen_slots.add(s)
                rows_in_pass += 1
                avail, fin = state[s]
                assert fin or avail >= (k + 1) * C + L, ("a chunk left before it was decodable", tag)
                assert w0 + wlen <= avail and f0 + take <= avail, ("a window past the frames that exist", tag)
                got[r].append((k, f0, w0, wlen, take))
        assert admitted == list(range(len(counts))), tag  # free slots take the requests in order
        for i, n in enumerate(counts):
            assert got[i] == chunks_of(n, C, W, L), (i, n, tag)  # every chunk exactly once, in order, as defined


def test_a_chunk_leaves_at_the_first_push_that_allows_it(driver):
    """burst 1, one slot: chunk k of a 20-frame request is issued at the push at which frame (k+1)C + L arrives -- neither
    before nor later -- and the rest at the push that finds the request final."""
    C, W, L, n = 4, 8, 3, 20
    (log,) = _replay(driver, [(C, W, L, 64, 1, 1, [n])])
    avail, issued_at = 0, {}
    for kind, v in log:
        if kind == "push":
            avail = v[0]
        elif kind == "row":
            issued_at[v[2]] = avail
    assert issued_at == {k: min(n, (k + 1) * C + L) for k in range(n // C)}
