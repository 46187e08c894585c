"""The host-only bookkeeping of the slot loop (csrc/queue_slots.h): how long the next burst is, what a burst's read-back does to
the slots, and how many rows wait for text.

A small driver (tests/native/queue_slots_driver.cc) applies burst_length, after_burst and starved_count to slots given on its
stdin. The rules are restated below in a few lines of Python; the hand-written cases pin the corners, a seeded sweep the rest.
The driver is built twice: plainly, and with AddressSanitizer + UBSan (stand-alone, nothing is loaded into Python)."""
import os
import random
import shutil
import subprocess
from collections import namedtuple

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "swift-qwen3-tts_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

pytestmark = pytest.mark.skipif(not shutil.which("g++"), reason="g++ is not installed")

# a slot and what the burst's read-back holds for it: frame count, finished flag, starved byte
Slot = namedtuple("Slot", "req since cap open starved nframes fin sbyte")
EMPTY = Slot(-1, 0, 0, 0, 0, 0, 1, 0)


def _sanitized():
    probe = subprocess.run(["g++", "-x", "c++", "-", "-o", os.devnull, *SAN], input="int main(){return 0;}", capture_output=True,
                           text=True)
    return probe.returncode == 0


@pytest.fixture(scope="module", params=["plain", "asan_ubsan"])
def driver(request):
    flags = SAN if request.param == "asan_ubsan" else []
    if flags and not _sanitized():
        pytest.skip("g++ cannot link with " + SAN[0])
    out = os.path.join(NATIVE, "_build", "queue_slots_driver_" + request.param)
    deps = [os.path.join(NATIVE, "queue_slots_driver.cc"), os.path.join(CSRC, "queue_slots.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        # no HIP include path and no platform define: the slot bookkeeping must stay host-only
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I" + CSRC, deps[0], "-o", out])
    return out


def expected(burst_frames, open_text, slots):
    """The rules: the burst is the smallest of burst_frames and cap - since over occupied rows that do not wait for text, at
    least 1 when there is such a row. Behind the burst an occupied row whose starved byte is set waits for text: its finished
    flag is cleared, and it is an event if it did not wait before; a closed queue ignores the byte. A row that is open or
    waits has taken as many steps as it has frames; any other row all that were launched."""
    occupied = [x for x in slots if x.req >= 0]
    runnable = [x for x in occupied if not x.starved]
    burst = min([burst_frames] + [x.cap - x.since for x in runnable])
    if runnable:
        burst = max(burst, 1)
    now = events = 0
    rows = []
    for x in slots:
        starved, fin = bool(x.starved), x.fin
        if open_text:
            starved = x.req >= 0 and x.sbyte != 0
            if starved:
                fin = 0
                now += 1
                events += 0 if x.starved else 1
        since = x.since
        if x.req >= 0:
            since = x.nframes if (x.open or starved) else x.since + burst
        rows.append((since, int(starved), fin))
    count = sum(1 for x, r in zip(slots, rows) if x.req >= 0 and r[1])
    return (len(occupied), len(runnable), burst), (now, events, count), rows


def run(driver, cases):
    text = "".join("%d %d %d\n%s" % (bf, int(ot), len(sl), "".join(" ".join(str(int(v)) for v in x) + "\n" for x in sl))
                   for bf, ot, sl in cases)
    out = subprocess.run([driver], input=text, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [[int(v) for v in ln.split()[1:]] for ln in out.stdout.splitlines()]
    got, at = [], 0
    for _, _, sl in cases:
        got.append((tuple(lines[at]), tuple(lines[at + 1]), [tuple(r) for r in lines[at + 2:at + 2 + len(sl)]]))
        at += 2 + len(sl)
    assert at == len(lines)
    return got


def test_burst_length_by_hand(driver):
    cases = [
        (8, False, [EMPTY, EMPTY, EMPTY]),                                       # all empty
        (8, False, [Slot(0, 0, 5, 0, 0, 5, 1, 0)]),                               # the cap ends the burst
        (8, True, [Slot(0, 7, 7, 1, 0, 7, 0, 0)]),                                # an open row at its open cap: still one step
        (8, True, [Slot(0, 9, 10, 1, 1, 9, 1, 1), Slot(1, 0, 20, 0, 0, 8, 0, 0)]),  # the starved row's remainder of 1 bounds nothing
        (8, True, [Slot(0, 3, 10, 1, 1, 3, 1, 1), EMPTY, Slot(2, 4, 9, 1, 1, 4, 1, 1)]),  # every occupied row waits
    ]
    got = run(driver, cases)
    assert [g[0] for g in got] == [(0, 0, 8), (1, 1, 5), (1, 1, 1), (2, 1, 8), (2, 0, 8)]
    assert [g[0] for g in got] == [expected(*c)[0] for c in cases]


def test_after_burst_by_hand(driver):
    open_rows = [
        Slot(0, 2, 50, 1, 0, 4, 1, 1),   # becomes starved: an event, its finished flag is masked, since = its frames
        Slot(1, 4, 50, 1, 1, 4, 1, 1),   # stays starved: no event
        Slot(2, 4, 50, 1, 1, 9, 0, 0),   # resumes
        Slot(3, 0, 50, 0, 0, 6, 1, 0),   # a closed-text row that finished: its flag stays
        Slot(-1, 0, 0, 0, 0, 0, 1, 1),   # an empty slot's byte counts for nothing
    ]
    closed = [Slot(0, 2, 50, 0, 0, 8, 1, 1), Slot(1, 0, 50, 1, 0, 3, 0, 0)]  # closed queue: the byte is ignored; an open row's since
    got = run(driver, [(6, True, open_rows), (6, False, closed)])
    plan, after, rows = got[0]
    assert plan == (4, 2, 6) and after == (2, 1, 2)
    assert rows == [(4, 1, 0), (4, 1, 0), (9, 0, 0), (6, 0, 1), (0, 0, 1)]
    plan, after, rows = got[1]
    assert plan == (2, 2, 6) and after == (0, 0, 0)
    assert rows == [(8, 0, 1), (3, 0, 0)]  # since + burst for the closed row; the frame count, not 0 + 6, for the open one
    assert got[0] == expected(6, True, open_rows) and got[1] == expected(6, False, closed)


def test_random_sweep_follows_the_rules(driver):
    rng = random.Random(20261)
    cases = []
    for _ in range(200):
        slots = []
        for s in range(rng.randint(1, 8)):
            if rng.random() < 0.25:
                slots.append(Slot(-1, 0, 0, 0, 0, rng.randint(0, 5), rng.randint(0, 1), rng.randint(0, 1)))
                continue
            cap = rng.randint(1, 40)
            since = rng.randint(0, cap)
            slots.append(Slot(s + 10, since, cap, rng.randint(0, 1), int(rng.random() < 0.3), rng.randint(0, cap), rng.randint(0, 1),
                              int(rng.random() < 0.4)))
        cases.append((rng.randint(1, 12), rng.random() < 0.7, slots))
    for case, got in zip(cases, run(driver, cases)):
        assert got == expected(*case), case
