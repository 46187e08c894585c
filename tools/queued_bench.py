#!/usr/bin/env python3
"""Continuous batching against static batches.

  python tools/queued_bench.py [--preset 1.7b] [--slots 32] [--requests 256] [--stream CHUNK,WINDOW,LOOKAHEAD] [--mixed-sampling]
  python tools/queued_bench.py --preset 1.7b-base --voices 4 [--slots 32] [--requests 256] [--stream CHUNK,WINDOW,LOOKAHEAD]

Two workloads on bench.py's synthetic checkpoint and request builder:
  ragged   max_tokens uniform in 50..400 (seeded), temperature 0.9, seed 1234: rows end at their caps (or EOS) at different frames
  uniform  force_frames = 200: every row has the same length, so continuous batching can only lose (admission costs)
and two paths for each:
  static   pipelined q3tts_generate_begin / _end batches of `slots` requests in request order, row_base = first request's index
  queued   one q3tts_generate_queued call with `slots` rows in flight
Prints, per run, frames/s (generated frames over the wall time of the whole workload, codec decode included), frame steps,
prefill and codec milliseconds, and whether every request's codes and PCM are bit-identical between the two paths.
--stream CHUNK,WINDOW,LOOKAHEAD adds, on the ragged workload, the queue with streamed audio (audio_chunk_frames / audio_window_frames /
audio_lookahead_frames) next to the same run without it, both with an event callback: frames/s of each, and per request the time
from its admission to its first AUDIO_CHUNK (streamed) or to its AUDIO (not streamed), median and worst. A request's admission is
its last TOKEN's arrival (the burst boundary that retired it) minus its generate_time (admission -> retirement).
--mixed-sampling gives the ragged workload's requests parameters of their own (q3tts_sampling.per_request), four sets in turn:
the call's, greedy, top-k 20 / top-p 0.9 / T 0.7 with a seed, and repetition penalty 1.5; static and queued must still agree bit
for bit, and the queue's rows now include top-p rows beside the others in every frame step.
--request-speeds S1,S2,... loads the handle with q3tts_load_opts.request_speeds and deals the speeds round robin over the requests
(q3tts_request.speed): static and queued must still agree bit for bit. With --stream the
streamed queue serves them too (every ring slot then holds rows of the slowest request's frame size, printed in bytes); on a handle
with --output-sample-rate only speeds whose hop is the handle's are streamed, and the streamed run is skipped otherwise.
--output-sample-rate R, --speed S and --pitch P load the handle with those options (q3tts_load_opts): every path then runs with the
stages they add to the codec tail.
--voices N (a Base checkpoint) runs the ragged workload as voice-clone requests with N reference clips (3 s each) shared round-robin:
  static   pipelined batches whose requests carry their clip as ref_audio (every batch encodes its clips again)
  queued   one q3tts_generate_queued call whose requests name one of N voices made once by create_voice
alternating --repeat times, with frames/s, frontend / prefill / codec milliseconds of each and the bit-identity of the two.
--voices N --stream CHUNK,WINDOW,LOOKAHEAD then also streams the voices queue (audio_stream_reference = 1: a voice's reference goes in
front of its request's stream): the voices' saved tail states against Q3TTS_NO_PREFIX_CACHE=1 (every admission decodes its
reference again), alternating --repeat times, with frames/s and per request the time from admission to first AUDIO_CHUNK, median
and worst, and whether the two agree bit for bit.
--session [--arrivals RATE] runs the ragged workload through a serving session (q3tts_session_*): requests are submitted one by
one, open-loop, with exponential gaps of mean 1 / RATE seconds from a fixed seed (RATE = inf, the default: all at once), and
collected by ticket. Printed: frames/s over the time from the first submit to the last completion, and per request the time from
its submit to its completion (its AUDIO event; without a callback: when its result was collected, in ticket order) -- median, p95
and max over the requests that succeeded; with --stream also from its submit to its first AUDIO_CHUNK. The same requests as one closed q3tts_generate_queued call, with the same callback, stand next
to it (every request "submitted" at the call). With RATE = inf the session and the closed call also alternate --repeat times
WITHOUT a callback, which is the saturated-throughput comparison, and their results are compared bit for bit.
--session --text-rate TOK_PER_S feeds every request's text the way a language model would hand it over: content token j of each
request arrives j / TOK_PER_S seconds after its first one, from a feeder thread. Two ways to serve that, alternating --repeat times:
  open    q3tts_session_submit_open at the first token, q3tts_session_append_text for every later one (the last one final)
  whole   q3tts_session_submit of the whole request once its last token has arrived -- what a caller can do without open text
Printed per run: the time from a request's first token to its first AUDIO_CHUNK (--stream; its AUDIO otherwise), median, p95 and max,
to its completion, the session's starve events, and whether the two ways agree bit for bit (they must: same tickets).
--session --live-voices K --new-voice-every N (a Base checkpoint, e.g. --preset 1.7b-base; with --arrivals and --stream) serves the
ragged workload as voice requests over 4 known clips, where every N-th arrival brings a clip nobody has seen. Two ways, alternating
--repeat times:
  live     a session opened with live_voices = K: the new clip goes to Session.create_voice at its arrival and its request names
           the voice at once; the front end runs beside the rows in flight
  before   what a session without live voices allows: the voices of ALL clips are created before the session opens, and that time
           is counted in front (of the wall time, and of every new-clip request's time to first audio)
Printed per run: frames/s, the time from a new clip's arrival to the first AUDIO_CHUNK of its request (its AUDIO without --stream),
the session's frontend_ms_sum, the frame-step rate of the bursts during which at least one front-end job was in flight
(frame_steps_beside / burst_ms_beside, the loop thread's own times) against the rate of the other bursts, and the time from
create_voice to ready. Every result is checked bit for bit against the
closed form, one q3tts_generate_queued_voices call over voices made by q3tts_voice_create.
"""
from __future__ import annotations

import argparse
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "swift-qwen3-tts_amd"))

import bench  # noqa: E402  (checkpoint synthesis and request builder of the headline benchmark)


def run_static(model, reqs, slots, kw):
    """Pipelined begin / end batches in request order (bench.py's pipeline): the next batch's frame loop overlaps the decode
    of the one before."""
    out, steps, pre, codec, fe = [], 0, 0.0, 0.0, 0.0
    batches = [(lo, reqs[lo:lo + slots]) for lo in range(0, len(reqs), slots)]
    t0 = time.perf_counter()
    job = model.generate_batch_begin(batches[0][1], row_base=batches[0][0], more_follows=len(batches) > 1, **kw)
    for k in range(len(batches)):
        nxt = None
        if k + 1 < len(batches):
            lo, b = batches[k + 1]
            nxt = model.generate_batch_begin(b, row_base=lo, more_follows=k + 2 < len(batches), **kw)
        out += model.generate_batch_end(job)
        tm = model.last_timing()
        steps += tm.frame_steps
        pre += tm.prefill_ms
        codec += tm.codec_ms
        fe += tm.frontend_ms
        job = nxt
    return out, time.perf_counter() - t0, steps, pre, codec, fe


def run_queued(model, reqs, slots, kw):
    t0 = time.perf_counter()
    out = model.generate_queued(reqs, slots=slots, **kw)
    dt = time.perf_counter() - t0
    tm = model.last_timing()
    return out, dt, tm.frame_steps, tm.prefill_ms, tm.codec_ms, tm.frontend_ms


def run_queued_timed(model, reqs, slots, kw):
    """The queued path with a callback that stamps every request's last TOKEN, first AUDIO_CHUNK and AUDIO."""
    last_token, first_chunk, audio = {}, {}, {}

    def on_event(i, kind, payload):
        t = time.perf_counter()
        if kind == "token":
            last_token[i] = t
        elif kind == "audio_chunk":
            first_chunk.setdefault(i, t)
        elif kind == "audio":
            audio[i] = t

    t0 = time.perf_counter()
    out = model.generate_queued(reqs, slots=slots, on_event=on_event, **kw)
    dt = time.perf_counter() - t0
    tm = model.last_timing()
    first = first_chunk if first_chunk else audio
    lat = [first[i] - (last_token[i] - out[i].info.generate_time) for i in range(len(reqs)) if i in first and i in last_token]
    return out, dt, tm, np.asarray(lat)


def _pct(x):
    x = np.asarray(x) * 1e3
    return f"median {np.median(x):8.1f} ms  p95 {np.percentile(x, 95):8.1f} ms  max {x.max():8.1f} ms" if x.size else "none"


def run_session(model, reqs, slots, kw, rate, timed):
    """The requests through a session at `rate` arrivals per second (inf: all at once). Returns results, wall time, and, when
    `timed`, per request submit -> completion and submit -> first AUDIO_CHUNK (seconds)."""
    n = len(reqs)
    submit_t, done_t, first_chunk = [0.0] * n, {}, {}

    def on_event(i, kind, payload):
        if kind == "audio_chunk":
            first_chunk.setdefault(i, time.perf_counter())
        elif kind == "audio":
            done_t[i] = time.perf_counter()

    gaps = np.random.default_rng(4321).exponential(1.0 / rate, size=n) if np.isfinite(rate) else np.zeros(n)
    s = model.open_session(slots=slots, max_pending=n, on_event=on_event if timed else None, **kw)
    try:
        t0 = time.perf_counter()
        due = t0
        for i, r in enumerate(reqs):
            due += gaps[i]
            while True:  # open loop: the arrival times do not depend on how the session is doing
                now = time.perf_counter()
                if now >= due:
                    break
                time.sleep(min(due - now, 0.002))
            submit_t[i] = time.perf_counter()
            assert s.submit(r) == i
        out = []
        for i in range(n):
            out.append(s.result(i, timeout=600))
            if not timed:
                done_t[i] = time.perf_counter()  # (no callback: when its result was collected)
        dt = time.perf_counter() - t0
        st = s.stats()
        s.close()
    finally:
        s.close(drain=False)
    done = np.asarray([done_t[i] - submit_t[i] for i in range(n) if i in done_t])  # (a failed request has no AUDIO event)
    first = np.asarray([first_chunk[i] - submit_t[i] for i in range(n) if i in first_chunk])
    return out, dt, st, done, first


def run_closed_timed(model, reqs, slots, kw):
    """The same requests as one closed call with the same stamps: every request counts as submitted when the call starts."""
    done_t, first_chunk = {}, {}

    def on_event(i, kind, payload):
        if kind == "audio_chunk":
            first_chunk.setdefault(i, time.perf_counter())
        elif kind == "audio":
            done_t[i] = time.perf_counter()

    t0 = time.perf_counter()
    out = model.generate_queued(reqs, slots=slots, on_event=on_event, **kw)
    dt = time.perf_counter() - t0
    done = np.asarray([done_t[i] - t0 for i in range(len(reqs)) if i in done_t])
    first = np.asarray([first_chunk[i] - t0 for i in range(len(reqs)) if i in first_chunk])
    return out, dt, done, first


def run_session_bench(model, args, ragged, warm, sampling):
    rate = float(args.arrivals)
    kw = dict(sampling)
    if args.stream:
        c, w, l = (int(x) for x in args.stream.split(","))
        kw.update(audio_chunk_frames=c, audio_window_frames=w, audio_lookahead_frames=l)
    run_session(model, warm, args.slots, kw, float("inf"), True)  # warm-up: the session's thread, the stream arena
    run_closed_timed(model, warm, args.slots, kw)
    same = lambda a, b: all(x.status == y.status and np.array_equal(x.codes, y.codes) and np.array_equal(x.audio, y.audio) for x, y in zip(a, b))
    tag = f"--stream {args.stream}" if args.stream else "whole audio"
    print(f"# session, {len(ragged)} ragged requests, slots {args.slots}, arrivals {args.arrivals}/s, {tag}", flush=True)
    if not np.isfinite(rate):
        for rep in range(args.repeat):  # saturated throughput: no callback on either side
            a, da, _, _, _ = run_session(model, ragged, args.slots, kw, rate, False)
            t0 = time.perf_counter()
            b = model.generate_queued(ragged, slots=args.slots, **kw)
            db = time.perf_counter() - t0
            fa, fb = (sum(int(r.codes.shape[0]) for r in x) for x in (a, b))
            print(f"run {rep} no callback: session frames/s {fa / da:9.1f} (wall {da:7.3f} s)   closed frames/s {fb / db:9.1f} (wall {db:7.3f} s)   "
                  f"session / closed {(fa / da) / (fb / db):.4f}   bit-identical: {same(a, b)}", flush=True)
    out, dt, st, done, first = run_session(model, ragged, args.slots, kw, rate, True)
    frames = sum(int(r.codes.shape[0]) for r in out)
    print(f"session  frames {frames:7d}  wall {dt:8.3f} s  frames/s {frames / dt:9.1f}  frame_steps {st.frame_steps:6d}  admissions {st.admissions:4d}  "
          f"failed {sum(1 for r in out if r.status != 0)}", flush=True)
    print(f"session  submit -> completion:        {_pct(done)}", flush=True)
    if args.stream:
        print(f"session  submit -> first AUDIO_CHUNK: {_pct(first)}", flush=True)
    cout, cdt, cdone, cfirst = run_closed_timed(model, ragged, args.slots, kw)
    cframes = sum(int(r.codes.shape[0]) for r in cout)
    print(f"closed   frames {cframes:7d}  wall {cdt:8.3f} s  frames/s {cframes / cdt:9.1f}   (one q3tts_generate_queued call, same callback)", flush=True)
    print(f"closed   call -> completion:          {_pct(cdone)}", flush=True)
    if args.stream:
        print(f"closed   call -> first AUDIO_CHUNK:   {_pct(cfirst)}", flush=True)
    print(f"bit-identical codes + pcm, session against the closed call: {same(out, cout)}", flush=True)


def run_text_fed(model, reqs, slots, kw, rate, open_text):
    """Every request's content token j arrives j / rate seconds after the run's start. open_text: submit_open at the first token and
    one append per later token; otherwise plain submit once the last token is there. Returns results, first token -> first audio,
    first token -> completion (seconds), and the session's text stats."""
    from qwen3tts import GenerationRequest
    n = len(reqs)
    first_audio, done_t = {}, {}
    first_kind = "audio_chunk" if kw.get("audio_chunk_frames", 0) > 0 else "audio"

    def on_event(i, kind, payload):
        t = time.perf_counter()
        if kind == first_kind:
            first_audio.setdefault(i, t)
        if kind == "audio":
            done_t[i] = t

    content = [list(r.text_ids[3:-5]) for r in reqs]
    longest = max(len(c) for c in content)
    s = model.open_session(slots=slots, max_pending=n, on_event=on_event, **kw)
    errors = []
    try:
        t0 = time.perf_counter()

        def feeder():
            try:
                for j in range(longest):
                    due = t0 + j / rate
                    while True:
                        now = time.perf_counter()
                        if now >= due:
                            break
                        time.sleep(min(due - now, 0.001))
                    for i, r in enumerate(reqs):
                        c = content[i]
                        if j >= len(c):
                            continue
                        last = j == len(c) - 1
                        if open_text:
                            if j == 0:
                                head = GenerationRequest(list(r.text_ids[:4]), 0, r.instruct_ids, r.speaker, r.language, r.max_tokens)
                                assert s.submit_open(head) == i
                                if last:
                                    s.close_text(i)
                            else:
                                s.append_text(i, c[j:j + 1], final=last)
                        elif last:
                            s.submit(r)
            except Exception as e:  # (reported by the caller's thread)
                errors.append(e)

        th = threading.Thread(target=feeder)
        th.start()
        th.join()
        if errors:
            raise errors[0]
        out = [s.result(i, timeout=600) for i in range(n)]
        ts = s.text_stats()
        s.close()
    finally:
        s.close(drain=False)
    first = np.asarray([first_audio[i] - t0 for i in range(n) if i in first_audio])
    done = np.asarray([done_t[i] - t0 for i in range(n) if i in done_t])
    return out, first, done, ts


def run_text_rate_bench(model, args, reqs, warm, sampling):
    rate = float(args.text_rate)
    kw = dict(sampling)
    if args.stream:
        c, w, l = (int(x) for x in args.stream.split(","))
        kw.update(audio_chunk_frames=c, audio_window_frames=w, audio_lookahead_frames=l)
    run_text_fed(model, warm, args.slots, kw, 1e9, True)  # warm-up: the session's graph, the stream arena
    run_text_fed(model, warm, args.slots, kw, 1e9, False)
    what = "first AUDIO_CHUNK" if args.stream else "AUDIO"
    tag = f"--stream {args.stream}" if args.stream else "whole audio"
    print(f"# session, {len(reqs)} requests of {len(reqs[0].text_ids) - 8} content tokens arriving at {args.text_rate} tokens/s each, "
          f"slots {args.slots}, {tag}", flush=True)
    same = lambda a, b: all(x.status == y.status and np.array_equal(x.codes, y.codes) and np.array_equal(x.audio, y.audio) for x, y in zip(a, b))
    for rep in range(args.repeat):
        res = {}
        for name, open_text in (("open", True), ("whole", False)):
            out, first, done, ts = run_text_fed(model, reqs, args.slots, kw, rate, open_text)
            res[name] = out
            print(f"run {rep} {name:5s} first token -> {what}: {_pct(first)}", flush=True)
            print(f"run {rep} {name:5s} first token -> completion:   {_pct(done)}   starve events {ts.starve_events}  "
                  f"appended tokens {ts.appended_tokens}  failed {sum(1 for r in out if r.status != 0)}", flush=True)
        print(f"run {rep} bit-identical codes + pcm, open text against whole submits: {same(res['open'], res['whole'])}", flush=True)


def run_live_voices(model, args):
    """--session --live-voices K --new-voice-every N: see the module's docstring."""
    from qwen3tts import GenerationRequest, synth
    n, every, known_n = args.requests, args.new_voice_every, 4
    base = bench.build_requests(args.preset, 0, n, args.n_text, 0)
    caps = np.random.default_rng(1234).integers(50, 401, size=n)
    new_at = [i for i in range(n) if every > 0 and i % every == every - 1]
    clip_of = {i: known_n + j for j, i in enumerate(new_at)}  # request -> its clip (the others: i % known_n)
    n_clips = known_n + len(new_at)
    clips = [synth.synthetic_reference_audio(k, 3.0) for k in range(n_clips)]
    texts = [base[k % n].ref_text_ids for k in range(n_clips)]
    kw = dict(temperature=0.9, top_k=50, top_p=1.0, repetition_penalty=1.5, seed=1234)
    if args.stream:
        c, w, l = (int(x) for x in args.stream.split(","))
        kw.update(audio_chunk_frames=c, audio_window_frames=w, audio_lookahead_frames=l, audio_stream_reference=1)
    first_kind = "audio_chunk" if args.stream else "audio"
    rate = float(args.arrivals)
    gaps = np.random.default_rng(4321).exponential(1.0 / rate, size=n) if np.isfinite(rate) else np.zeros(n)
    req = lambda i, v, cap=None: GenerationRequest(base[i].text_ids, 100, None, None, base[i].language, int(caps[i] if cap is None else cap), voice=v)
    same = lambda a, b: all(x.status == y.status and np.array_equal(x.codes, y.codes) and np.array_equal(x.audio, y.audio) for x, y in zip(a, b))
    ref = {"max": 0}  # the longest reference in frames (known once the closed form's voices exist)

    def serve(live):
        first, spans, lock = {}, [], threading.Lock()

        def on_event(i, kind, payload):
            if kind == first_kind:
                first.setdefault(i, time.perf_counter())

        voices = [model.create_voice(clips[k], texts[k]) for k in range(known_n if live else n_clips)]
        front_new = 0.0  # (the known clips' voices exist before the service starts, either way)
        if not live:  # the new clips' share of the time in front: measured on its own
            t1 = time.perf_counter()
            for v in [model.create_voice(clips[k], texts[k]) for k in range(known_n, n_clips)]:
                v.close()
            front_new = time.perf_counter() - t1
        s = model.open_session(slots=args.slots, max_pending=n, max_ref_frames=ref["max"], on_event=on_event,
                               live_voices=args.live_voices if live else 0, max_voices=(n_clips if live else 0), **kw)
        arrive, watchers, made = {}, [], []
        try:
            t0 = time.perf_counter()
            due = t0
            for i in range(n):
                due += gaps[i]
                while time.perf_counter() < due:
                    time.sleep(min(max(due - time.perf_counter(), 0), 0.002))
                arrive[i] = time.perf_counter()
                if i in clip_of and live:
                    while True:
                        try:
                            v = s.create_voice(clips[clip_of[i]], texts[clip_of[i]])
                            break
                        except Exception as e:  # BUSY: live_voices jobs in flight
                            if getattr(e, "status", 0) != 9:
                                raise
                            time.sleep(0.001)
                    made.append(v)

                    def watch(v=v, t=arrive[i]):
                        v.wait(timeout=600)
                        with lock:
                            spans.append((t, time.perf_counter()))

                    watchers.append(threading.Thread(target=watch))
                    watchers[-1].start()
                else:
                    v = voices[clip_of[i]] if i in clip_of else voices[i % known_n]
                assert s.submit(req(i, v)) == i
            out = [s.result(i, timeout=600) for i in range(n)]
            dt = time.perf_counter() - t0
            for th in watchers:
                th.join()
            st, vs = s.stats(), (s.voice_stats() if live else None)
            s.close()
        finally:
            s.close(drain=False)
        for v in voices + made:
            v.close()
        lat = np.asarray([first[i] - arrive[i] + front_new for i in new_at if i in first])
        beside = None
        if live and vs.burst_ms_beside > 0 and vs.burst_ms_alone > 0:  # the loop thread's own burst times
            ready = np.asarray([b - a for a, b in spans])
            beside = (vs.frame_steps_beside / vs.burst_ms_beside * 1e3, (st.frame_steps - vs.frame_steps_beside) / vs.burst_ms_alone * 1e3,
                      vs.burst_ms_beside, ready)
        wall = dt + front_new
        return out, wall, lat, vs, beside

    print(f"# {args.preset} bf16, {n} voice requests, slots {args.slots}, arrivals {args.arrivals}/s, "
          f"{'--stream ' + args.stream if args.stream else 'whole audio'}, every {every}th arrival a new 3 s clip "
          f"({len(new_at)} of them), live_voices {args.live_voices}", flush=True)
    # the closed form: voices made by create_voice, one generate_queued call
    voices = [model.create_voice(clips[k], texts[k]) for k in range(n_clips)]
    ref["max"] = max(v.info.ref_frames for v in voices)
    model.generate_queued([req(i, voices[i % known_n], 8) for i in range(2 * args.slots)], slots=args.slots, **kw)  # warm-up
    closed = model.generate_queued([req(i, voices[clip_of.get(i, i % known_n)]) for i in range(n)], slots=args.slots, **kw)
    for v in voices:
        v.close()
    for rep_i in range(args.repeat):
        for name, live in (("live", True), ("before", False)):
            out, wall, lat, vs, beside = serve(live)
            frames = sum(int(r.codes.shape[0]) for r in out)
            print(f"run {rep_i} {name:6s} frames {frames:7d}  wall {wall:8.3f} s  frames/s {frames / wall:9.1f}  "
                  f"new clip -> first {first_kind.upper()}: {_pct(lat)}  failed {sum(1 for r in out if r.status != 0)}  "
                  f"bit-identical to the closed form: {same(out, closed)}", flush=True)
            if vs is not None:
                print(f"run {rep_i} {name:6s} frontend_ms_sum {vs.frontend_ms_sum:8.1f} ms over {vs.created} voices  frame_steps_beside "
                      f"{vs.frame_steps_beside}", flush=True)
            if beside is not None:
                print(f"run {rep_i} {name:6s} frame steps/s in bursts with a job in flight {beside[0]:8.1f} (over {beside[2]:7.1f} ms)   "
                      f"in the others {beside[1]:8.1f}   ratio {beside[0] / beside[1]:.3f}   create_voice -> ready: {_pct(beside[3])}", flush=True)


def run_voices(model, args):
    """The ragged workload as voice-clone requests: static ref_audio batches against the queue with voices."""
    from qwen3tts import GenerationRequest, synth
    clips = [synth.synthetic_reference_audio(k, 3.0) for k in range(args.voices)]
    base = bench.build_requests(args.preset, 0, args.requests, args.n_text, 0)
    texts = [base[k].ref_text_ids for k in range(args.voices)]
    t0 = time.perf_counter()
    voices = [model.create_voice(clips[k], texts[k]) for k in range(args.voices)]
    print(f"# {args.voices} voices created in {(time.perf_counter() - t0) * 1e3:.1f} ms, "
          f"{sum(v.info.device_bytes for v in voices)} device bytes, {[v.info.ref_frames for v in voices]} reference frames", flush=True)
    caps = np.random.default_rng(1234).integers(50, 401, size=args.requests)
    as_audio, as_voice = [], []
    for i, (r, c) in enumerate(zip(base, caps)):
        k = i % args.voices
        as_audio.append(GenerationRequest(r.text_ids, 100, None, None, r.language, int(c), ref_audio=clips[k], ref_text_ids=texts[k]))
        as_voice.append(GenerationRequest(r.text_ids, 100, None, None, r.language, int(c), voice=voices[k]))
    kw = dict(temperature=0.9, top_k=50, top_p=1.0, repetition_penalty=1.5, seed=1234)
    short = lambda rs: [type(r)(r.text_ids, r.target_token_count, None, None, r.language, 8, ref_audio=r.ref_audio,
                                ref_text_ids=r.ref_text_ids, voice=r.voice) for r in rs[:2 * args.slots]]
    run_static(model, short(as_audio), args.slots, kw)  # warm-up: frame graphs, projected tables, codec and front-end scratch
    run_queued(model, short(as_voice), args.slots, kw)
    print(f"# {args.preset} bf16, {args.requests} voice-clone requests, {args.voices} clips of 3 s, slots {args.slots}; "
          "frames/s = generated frames / wall time (front end and codec included)")
    last = {}
    for rep in range(args.repeat):
        for path in ("static", "queued"):
            if path == "static":
                out, dt, steps, pre, codec, fe = run_static(model, as_audio, args.slots, kw)
            else:
                out, dt, steps, pre, codec, fe = run_queued(model, as_voice, args.slots, kw)
            frames = sum(int(r.codes.shape[0]) for r in out)
            last[path] = out
            print(f"run {rep} {path:6s} frames {frames:7d}  wall {dt:8.3f} s  frames/s {frames / dt:9.1f}  frame_steps {steps:6d}  "
                  f"frontend {fe:8.1f} ms  prefill {pre:8.1f} ms  codec {codec:8.1f} ms  failed {sum(1 for r in out if r.status != 0)}", flush=True)
    same = all(x.status == y.status and np.array_equal(x.codes, y.codes) and np.array_equal(x.audio, y.audio)
               for x, y in zip(last["static"], last["queued"]))
    print(f"bit-identical codes + pcm, all {args.requests} requests, ref_audio batches against the queue with voices: {same}", flush=True)
    if args.stream:
        run_voices_streamed(model, args, as_voice, short(as_voice), kw)
    for v in voices:
        v.close()


def run_voices_streamed(model, args, reqs, warm, kw):
    """The voices queue with streamed audio: admissions served from the voices' saved tail states against admissions that decode
    their reference prefix every time."""
    from qwen3tts import _lib
    c, w, l = (int(x) for x in args.stream.split(","))
    skw = dict(kw, audio_chunk_frames=c, audio_window_frames=w, audio_lookahead_frames=l, audio_stream_reference=1)
    run_queued_timed(model, warm, args.slots, skw)  # stream arena, pinned ring; every voice's state is saved here
    n, b, _ = model.debug_prefix_states()
    print(f"# streamed voices --stream {args.stream}: {n} saved tail states, {b} device bytes", flush=True)
    last = {}
    try:
        for rep in range(args.repeat):
            for name in ("restored", "primed"):
                if name == "primed":
                    os.environ["Q3TTS_NO_PREFIX_CACHE"] = "1"
                else:
                    os.environ.pop("Q3TTS_NO_PREFIX_CACHE", None)
                _lib.reload_debug_env()
                before = model.debug_prefix_states()[2]
                out, dt, tm, lat = run_queued_timed(model, reqs, args.slots, skw)
                frames = sum(int(r.codes.shape[0]) for r in out)
                last[name] = out
                print(f"run {rep} streamed voices {name:8s} frames {frames:7d}  wall {dt:8.3f} s  frames/s {frames / dt:9.1f}  "
                      f"codec {tm.codec_ms:8.1f} ms  first_audio {tm.first_audio_ms:7.1f} ms  admission -> first AUDIO_CHUNK: median "
                      f"{np.median(lat) * 1e3:7.1f} ms  worst {lat.max() * 1e3:7.1f} ms  admissions restored "
                      f"{model.debug_prefix_states()[2] - before}  failed {sum(1 for r in out if r.status != 0)}", flush=True)
    finally:
        os.environ.pop("Q3TTS_NO_PREFIX_CACHE", None)
        _lib.reload_debug_env()
    same = all(x.status == y.status and np.array_equal(x.codes, y.codes) and np.array_equal(x.audio, y.audio)
               for x, y in zip(last["restored"], last["primed"]))
    print(f"bit-identical codes + pcm, all {len(reqs)} requests, saved states against decoding every prefix: {same}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="1.7b")
    ap.add_argument("--slots", type=int, default=32)
    ap.add_argument("--requests", type=int, default=256)
    ap.add_argument("--n-text", type=int, default=32)
    ap.add_argument("--mixed-sampling", action="store_true", help="ragged workload: four per-request parameter sets in turn")
    ap.add_argument("--stream", default=None, metavar="CHUNK,WINDOW,LOOKAHEAD", help="also run the ragged queue with streamed audio")
    ap.add_argument("--voices", type=int, default=0, metavar="N", help="Base checkpoint: voice-clone requests, N voices shared round-robin")
    ap.add_argument("--repeat", type=int, default=3, help="--voices / --session: how often the two paths alternate")
    ap.add_argument("--session", action="store_true", help="the ragged workload through a serving session (see --arrivals)")
    ap.add_argument("--arrivals", default="inf", metavar="RATE", help="--session: requests per second, exponential gaps; inf: all at once")
    ap.add_argument("--text-rate", default=None, metavar="TOK_PER_S",
                    help="--session: every request's content arrives at this rate; open-text requests against whole submits")
    ap.add_argument("--live-voices", type=int, default=0, metavar="K",
                    help="--session on a Base checkpoint: a session with K front-end lanes against voices created before open")
    ap.add_argument("--new-voice-every", type=int, default=8, metavar="N", help="--live-voices: every N-th arrival brings a new clip")
    ap.add_argument("--output-sample-rate", type=int, default=0, metavar="R",
                    help="load the model with q3tts_load_opts.output_sample_rate = R (0: the decoder's own 24000)")
    ap.add_argument("--speed", type=float, default=0.0, metavar="S",
                    help="load the model with q3tts_load_opts.speed = S (0: off; 0.5 .. 2.0: the time stretch in the decoder's tail)")
    ap.add_argument("--pitch", type=float, default=0.0, metavar="SEMITONES",
                    help="load the model with q3tts_load_opts_ex.pitch (0: off; -12 .. 12: the stretch at Hp and the general-ratio resampler)")
    ap.add_argument("--keep-formants", action="store_true",
                    help="load the model with q3tts_load_opts_ex2.keep_formants (with --pitch: analyse / whiten and synthesise around the resampler)")
    ap.add_argument("--request-speeds", default=None, metavar="S1,S2,...",
                    help="load the model with q3tts_load_opts.request_speeds and deal these speeds round robin over the requests "
                         "(q3tts_request.speed; 0: the handle's)")
    ap.add_argument("--only-stream", action="store_true", help="with --stream: skip the static / queued comparison in front of it")
    args = ap.parse_args()
    from qwen3tts import Qwen3TTSModel, RequestSampling
    rate_kw = dict(output_sample_rate=args.output_sample_rate) if args.output_sample_rate else {}
    if args.speed:
        rate_kw["speed"] = args.speed
    if args.pitch:
        rate_kw["pitch"] = args.pitch
    if args.keep_formants:
        rate_kw["keep_formants"] = True
    req_speeds = [float(s) for s in args.request_speeds.split(",")] if args.request_speeds else []
    if req_speeds:
        rate_kw["request_speeds"] = True

    ckpt = bench.ensure_checkpoint(args.preset, 0, None)
    if args.session and args.live_voices > 0:
        model = Qwen3TTSModel.from_pretrained(ckpt, max_batch=args.slots, max_frames=408, max_prompt=192, **rate_kw)
        run_live_voices(model, args)
        model.close()
        return
    if args.voices > 0:  # (an ICL prompt carries the reference text and one row per reference frame: 3 s are 38 frames)
        model = Qwen3TTSModel.from_pretrained(ckpt, max_batch=args.slots, max_frames=408, max_prompt=192, **rate_kw)
        run_voices(model, args)
        model.close()
        return
    model = Qwen3TTSModel.from_pretrained(ckpt, max_batch=args.slots, max_frames=408, max_prompt=128, **rate_kw)
    n_instruct = 16 if args.preset == "1.7b" else 0
    base = bench.build_requests(args.preset, 0, args.requests, args.n_text, n_instruct)
    rng = np.random.default_rng(1234)
    caps = rng.integers(50, 401, size=args.requests)
    ragged = []
    for r, c in zip(base, caps):
        # max_tokens is the cap; target_token_count only lifts the max(75, 6 x target) floor above it (Qwen3.swift:822-823)
        ragged.append(type(r)(r.text_ids, 100, r.instruct_ids, r.speaker, r.language, int(c)))
    if args.mixed_sampling:
        sets = [None, RequestSampling(temperature=0.0), RequestSampling(temperature=0.7, top_k=20, top_p=0.9, seed=99),
                RequestSampling(repetition_penalty=1.5)]
        for i, r in enumerate(ragged):
            r.sampling = sets[i % 4]
    if req_speeds:
        for reqs in (ragged, base):
            for i, r in enumerate(reqs):
                r.speed = req_speeds[i % len(req_speeds)]
        hops = sorted({model.request_speed_info(s)[1] for s in req_speeds})
        extra = (model.info.max_samples_per_frame - model.info.samples_per_frame) * 4
        print(f"# request speeds {req_speeds} -> synthesis hops {hops} (the handle's: {model.stretch_hs}); PCM buffers of mixed jobs hold "
              f"{model.info.max_samples_per_frame} samples per frame, {extra} bytes per row and frame more than the handle's own", flush=True)
    sampling = dict(temperature=0.9, top_k=50, top_p=1.0, repetition_penalty=1.05, seed=1234)
    workloads = [("ragged", ragged, dict(sampling)), ("uniform", base, dict(sampling, force_frames=200))]

    # warm-up: both frame graphs captured, projected tables built, codec scratch grown
    warm = [type(r)(r.text_ids, r.target_token_count, r.instruct_ids, r.speaker, r.language, 8, speed=r.speed) for r in base[:2 * args.slots]]
    run_static(model, warm, args.slots, sampling)
    run_queued(model, warm, args.slots, sampling)

    if args.session and args.text_rate:
        # (an open-text request's target_token_count is its content count: the whole requests it is compared with say the same)
        fed = [type(r)(r.text_ids, len(r.text_ids) - 8, r.instruct_ids, r.speaker, r.language, r.max_tokens) for r in ragged]
        fed_warm = [type(r)(r.text_ids, len(r.text_ids) - 8, r.instruct_ids, r.speaker, r.language, 8) for r in base[:args.slots]]
        run_text_rate_bench(model, args, fed, fed_warm, sampling)
        model.close()
        return
    if args.session:
        run_session_bench(model, args, ragged, warm, sampling)
        model.close()
        return
    print(f"# {args.preset} bf16, {args.requests} requests, slots {args.slots}, output {model.sample_rate} Hz "
          f"({model.info.samples_per_frame} samples per frame); frames/s = generated frames / wall time (codec included)")
    for name, reqs, kw in ([] if args.only_stream and args.stream else workloads):
        res = {}
        for path, fn in (("static", run_static), ("queued", run_queued)):
            out, dt, steps, pre, codec, _ = fn(model, reqs, args.slots, kw)
            frames = sum(int(r.codes.shape[0]) for r in out)
            res[path] = (out, dt, steps, frames)
            print(f"{name:8s} {path:6s} frames {frames:7d}  wall {dt:8.3f} s  frames/s {frames / dt:9.1f}  frame_steps {steps:6d}  "
                  f"prefill {pre:8.1f} ms  codec {codec:8.1f} ms  failed {sum(1 for r in out if r.status != 0)}", flush=True)
        (a, da, sa, fa), (b, db, sb, fb) = res["static"], res["queued"]
        same = all(x.status == y.status and np.array_equal(x.codes, y.codes) and np.array_equal(x.audio, y.audio) for x, y in zip(a, b))
        print(f"{name:8s} bit-identical codes + pcm, all {len(a)} requests: {same}   queued / static: frame_steps {sb / sa:.3f}  "
              f"frames/s {(fb / db) / (fa / da):.3f}", flush=True)
    if args.stream:
        c, w, l = (int(x) for x in args.stream.split(","))
        skw = dict(audio_chunk_frames=c, audio_window_frames=w, audio_lookahead_frames=l)
        # (on a handle with an output rate a request speed at another hop than the handle's is served with whole audio only)
        streamable = not args.output_sample_rate or all(model.request_speed_info(s)[1] == model.stretch_hs for s in req_speeds)
        if req_speeds and streamable:
            ring = 8 * args.slots * c * 4  # CodecRunner::kRingSlots pinned slots of [slots][chunk * samples per frame] floats
            print(f"# pinned ring: {ring * model.info.max_samples_per_frame} bytes ({ring * model.info.samples_per_frame} without "
                  f"request_speeds)", flush=True)
        if streamable:
            run_queued_timed(model, warm, args.slots, dict(sampling, **skw))  # stream arena, pinned ring
        else:
            print("# --request-speeds with a hop other than the handle's at an output rate: the streamed run is skipped", flush=True)
        rows = {}
        for name, kw in (("queued", dict(sampling)), ("streamed", dict(sampling, **skw)))[:2 if streamable else 1]:
            out, dt, tm, lat = run_queued_timed(model, ragged, args.slots, kw)
            frames = sum(int(r.codes.shape[0]) for r in out)
            rows[name] = (out, frames / dt)
            what = "admission -> first AUDIO_CHUNK" if name == "streamed" else "admission -> AUDIO"
            print(f"ragged   {name:8s} (callback) frames {frames:7d}  wall {dt:8.3f} s  frames/s {frames / dt:9.1f}  frame_steps {tm.frame_steps:6d}  "
                  f"codec {tm.codec_ms:8.1f} ms  first_audio {tm.first_audio_ms:7.1f} ms  {what}: median {np.median(lat) * 1e3:7.1f} ms  "
                  f"worst {lat.max() * 1e3:7.1f} ms  failed {sum(1 for r in out if r.status != 0)}", flush=True)
        if not streamable:
            model.close()
            return
        same = all(np.array_equal(x.codes, y.codes) for x, y in zip(rows["queued"][0], rows["streamed"][0]))
        print(f"ragged   streamed --stream {args.stream}: same codes as the queue without it: {same}   frames/s streamed / queued: "
              f"{rows['streamed'][1] / rows['queued'][1]:.3f}", flush=True)
    model.close()


if __name__ == "__main__":
    main()
