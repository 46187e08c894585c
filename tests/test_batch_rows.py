"""The engine's own glue at real batch and slot counts: every batch row and every queue slot equals the request run alone.

The block tests hold every kernel family against a float64 reference; what sits between those blocks and the product is host
code that decides, per launch, a row's place in the fragment-major buffers (Mp_ / 16 row blocks, ss_ld = Mp_), its block-table
row and random-stream key, the prefill chunk length, whether the predictor's step 0 is one pair pass or two passes, the
sub-batch prefill of an admission and admit_rows into a slot, and the codec's row groups. The contract (DESIGN.md, and
qwen3tts/model.py generate_queued): request i of a call equals generate_batch([request], row_base=row_base + i) -- status,
codes and the float32 words of the audio, no tolerance. 80 requests per tiny checkpoint (ragged prompts, speakers, languages,
instructs, one prompt per 16 rows long enough to put its KV cache on two pages, caps of 4 / 9 / 6 / 12 frames) are run alone
once per keyword set and shared by every test below.

The host decisions, restated from the code (host_decisions below):
    Mp   = 64 with Q3TTS_ROWS_64, else max(256, 16 * round_up(max_batch, 16))            engine.cc:54
    C    = max(1, min(16, Mp // B))      prefill positions per launch                     engine.cc:1219
    pair = 2 * B <= Mp                   step 0 of the predictor as one two-position pass engine.cc:421
    M    = B * C rows per prefill launch; M > 64 takes launch_norm_rows and, where it applies, the tall GEMM instead of the
           norm prologue (engine.cc:302); C > 8 is attn_chunk_kernel's CMAX 16 class, 2..8 its CMAX 8 class (attn_decode.hip:222)
A handle that can hold 64 rows has Mp = 1024, not 256: its buffers hold 16 rows per batch row, so WITHOUT the switch every
batch of the list below prefills C = 16 positions per launch and runs the pair pass (the chunk lengths 15, 8, 7, 5 that
256 // B would give exist for no handle: max_batch <= 16 is the only way to Mp = 256, and then B <= 16 gives C = 16). The
shorter chunks, C == 1 and the two-pass step 0 are reached with Q3TTS_ROWS_64 = 1 alone, which is why the test of that switch
runs the whole batch list and not only 32 / 33 / 64: it is the only place where C is 12, 4, 3, 2 and 1 and where CMAX 8 runs.
test_case_table_reaches_the_host_decisions asserts exactly that, on the CPU.

The queue tests cannot read a request's slot (no event or statistic carries it). They rest on the admission order of
engine_queue.cc ("free slots in slot order take the next requests in request order", Engine::admit) and restate the slot
loop's three decisions in simulate_slots(): which requests an admission takes, how long a burst is (queue_slots.h
burst_length), when a row's finished flag is seen (a burst boundary). The restatement is checked against the engine through
q3tts_timing.frame_steps (every burst's length enters it), and the refills at high slots are read off it."""
import threading

import numpy as np
import pytest

from conftest import tiny_request

NAMES = ["tiny-a", "tiny-b"]                 # tiny-a: H = 256 = predictor hidden, no small_to_mtp_projection; tiny-b: H = 384, one
BS = [1, 2, 4, 5, 15, 16, 17, 31, 32, 33, 48, 49, 63, 64]
N_REQS, MAX_BATCH, MAX_FRAMES, MAX_PROMPT = 80, 64, 16, 128
CAPS = (4, 9, 6, 12)                         # max_tokens by request index mod 4
LONG_ROW = 7                                 # request i % 16 == 7: an instruct of 56 ids, a prompt of more than 64 positions
QUEUES = [(16, 24), (17, 26), (33, 45), (64, 80)]   # (slots, requests)
BURST = 9                                    # frame steps per burst of a one-lane engine (engine_queue.cc: max_inflight_frames / 2)
WAIT = 60                                    # seconds: every wait of the session test
SEED = 21
FORCED = dict(temperature=0.9, top_k=30, top_p=0.95, repetition_penalty=1.05, seed=SEED, force_frames=8)
FREE = dict(temperature=0.9, top_k=30, top_p=0.95, repetition_penalty=1.05, seed=SEED)
GREEDY = dict(temperature=0.0, force_frames=8)
KWS = {"forced": FORCED, "free": FREE, "greedy": GREEDY}
STREAM = dict(audio_chunk_frames=8, audio_window_frames=32, audio_lookahead_frames=4)
ROWS_ENV = "Q3TTS_ROWS_64"


# ---------------------------------------------------------------------------------------------------
# the host decisions, restated
# ---------------------------------------------------------------------------------------------------
def host_decisions(B, max_batch=MAX_BATCH, rows64=False):
    Mp = 64 if rows64 else max(256, 16 * (-(-max_batch // 16) * 16))   # engine.cc:54
    C = max(1, min(16, Mp // B))                                       # engine.cc:1219
    pair = 2 * B <= Mp                                                 # engine.cc:421
    return Mp, C, pair


def queue_caps(S, N):
    """max_tokens per request of a queue case: requests S-8 .. S-1 get the shortest cap, so the first slots to come free
    through a cap are the highest ones and the refills (requests S .. N-1) start there."""
    return [4 if S - 8 <= i < S else (9, 6, 12)[i % 3] for i in range(N)]


def simulate_slots(frames, caps, S, burst_frames=BURST):
    """The slot loop of engine_queue.cc for a closed one-lane queue, on the host: `frames` are the requests' frame counts
    alone. A row raises its finished flag at the step that reaches its cap, or at the step after its last frame (the one that
    draws EOS); the host sees the flag at the next burst boundary. Returns ({request: slot}, frame steps launched)."""
    N = len(frames)
    need = [f + 1 if f < c else c for f, c in zip(frames, caps)]
    slots, since, placed, nxt, steps = [None] * S, [0] * S, {}, 0, 0
    while True:
        for s in range(S):                                  # Engine::admit: free slots in slot order, requests in order
            if slots[s] is None and nxt < N:
                slots[s], since[s], placed[nxt] = nxt, 0, s
                nxt += 1
        running = [s for s in range(S) if slots[s] is not None]
        if not running:
            return placed, steps
        burst = max(1, min([burst_frames] + [caps[slots[s]] - since[s] for s in running]))   # queue_slots.h burst_length
        steps += burst
        for s in running:
            since[s] += burst                               # after_burst
            if since[s] >= need[slots[s]]:                  # retire()
                slots[s] = None


def _decision_table():
    """(B, rows64) of every generate_batch call the GPU tests below make on a 64-row handle."""
    return [(B, False) for B in BS] + [(B, True) for B in BS]


def test_case_table_reaches_the_host_decisions():
    """The batch list is the set of edges of the host decisions; this holds it to that (see the module docstring for why the
    short chunks belong to the Q3TTS_ROWS_64 half of the table)."""
    seen = {r: [host_decisions(B, rows64=r) + (B,) for B, rr in _decision_table() if rr == r] for r in (False, True)}
    assert {Mp for Mp, _, _, _ in seen[False]} == {1024} and {Mp for Mp, _, _, _ in seen[True]} == {64}
    assert {C for _, C, _, _ in seen[False]} == {16}
    assert {C for _, C, _, _ in seen[True]} == {16, 12, 4, 3, 2, 1}
    for r in (False, True):
        assert all(B * C <= Mp for Mp, C, _, B in seen[r])              # Q3_CHECK(M <= Mp_), engine.cc:294
    C_all = {C for r in seen for _, C, _, _ in seen[r]}
    assert any(C > 8 for C in C_all) and any(2 <= C <= 8 for C in C_all)   # both CMAX classes of attn_chunk_kernel
    assert 1 in C_all                                                      # the one-position prefill branch (engine.cc:1224)
    assert all(p for _, _, p, _ in seen[False])
    assert {B for _, _, p, B in seen[True] if not p} == {33, 48, 49, 63, 64} and any(p for _, _, p, _ in seen[True])
    assert {-(-B // 16) for B in BS} == {1, 2, 3, 4}                       # row blocks a frame step's rows take
    MC = [B * C for _, C, _, B in seen[False]]
    assert max(m for m in MC if m <= 64) == 64 and min(m for m in MC if m > 64) == 80   # prologue at B <= 4, row-norm from B = 5
    assert max(MC) == 1024
    # the queue's admissions prefill a sub-batch of k <= S rows through the same function: the same C
    assert all(host_decisions(k)[1] == 16 for k in range(1, 65))
    # lanes: n_streams = 2 gives each lane max_batch 32
    assert host_decisions(32, max_batch=32) == (512, 16, True)
    # the batch sizes of tests/test_gpu_parity.py test_scheduling_modes_agree, whose docstring states them
    assert host_decisions(3, max_batch=40) == (768, 16, True) and host_decisions(40, max_batch=40) == (768, 16, True)


def test_queue_cases_are_what_the_docstring_says():
    """simulate_slots on made-up frame counts: nobody draws EOS, so the first boundary comes at 4 steps, frees exactly the
    slots S-8 .. S-1 and the refills S .. S+7 land there in order."""
    for S, N in QUEUES:
        caps = queue_caps(S, N)
        assert len(caps) == N and sorted(set(caps)) == [4, 6, 9, 12] and all(c <= MAX_FRAMES for c in caps)
        assert [i for i, c in enumerate(caps[:S]) if c == 4] == list(range(S - 8, S))
        placed, steps = simulate_slots(caps, caps, S)
        assert sorted(placed) == list(range(N)) and all(placed[i] == i for i in range(S))
        assert [placed[S + j] for j in range(min(8, N - S))] == list(range(S - 8, S))[:N - S]
        assert steps >= 12
    # EOS behind the 2nd frame is drawn at step 3 and seen at the boundary behind step 4 (request 0's cap); the zero-frame
    # request 2 takes its slot and is gone at the next boundary, 5 steps on, where request 1 reaches its cap
    placed, steps = simulate_slots([2, 9, 0, 5], [4, 9, 9, 9], 2)
    assert placed == {0: 0, 1: 1, 2: 0, 3: 0} and steps == 4 + 5 + 9


def _layer_gemms(H, CH=256):
    """(name, K, N, epi, norm prologue possible, keywords) of the frame step's GEMMs on the tiny checkpoints
    (qwen3tts/synth.py: 4 + 2 + 2 heads of 128, intermediate 512, talker vocabulary 3072, predictor 256 wide and 256 codes)."""
    out = []
    for tag, K, ntw in (("talker", H, 1), ("predictor", CH, 0)):
        out += [(tag + ".qkv", K, 1024, 0, True, dict(nt_weights=ntw)), (tag + ".o", 512, K, 3, False, dict(nt_weights=ntw, resid=1)),
                (tag + ".gateup", K, 512, 2, True, dict(nt_weights=ntw)), (tag + ".down", 512, K, 3, False, dict(nt_weights=ntw, resid=1))]
    out += [("codec_head", H, 3072, 0, True, {}), ("lm_head", CH, 256, 0, True, {})]
    if H != CH:
        out.append(("cp_proj", H, CH, 3, False, dict(has_bias=1)))
    return out


def test_gemm_launch_classes_the_tiny_widths_reach():
    """skinny_geometry / gemm_tall_takes (host code) over every GEMM of a frame step and of a prefill chunk at the tiny
    checkpoints' K and N, for every batch of the table: one, two and three row blocks per workgroup occur, the row split over
    grid.y from 1 to 4 and beyond, and both the skinny and the tall kernel. FOUR row blocks per workgroup cannot be reached at these
    widths: skinny_geometry keeps four only for a launch without the norm prologue whose column tiles do not fit a split
    (N / 16 > 128, i.e. N > 2048, gemm_decode.hip:157-164), and the only such N here (the 3072-wide codec head) carries the
    prologue. tests/test_gemm_block.py reaches that class at the block level ("pf-np2", "pf-np4")."""
    from qwen3tts import _lib
    seen = set()
    for H in (256, 384):
        for B, rows64 in _decision_table():
            Mp, C, pair = host_decisions(B, rows64=rows64)
            for M, stacks in ((B, ("talker", "predictor", "codec_head", "lm_head", "cp_proj")), (2 * B if pair else B, ("predictor", "lm_head", "cp_proj")),
                              (B * C, ("talker",))):
                for name, K, N, epi, can_norm, kw in _layer_gemms(H):
                    if name.split(".")[0] not in stacks:
                        continue
                    norm = int(can_norm and (M <= 64 or name in ("codec_head", "lm_head")))   # engine.cc:302-303; the heads always
                    g = _lib.gemm_geometry(M=M, K=K, N=N, xMB=Mp // 16, yMB=Mp // 16, ss_ld=Mp, y_cols=-(-N // 128) * 128 if epi else N,
                                           epi=epi, norm=norm, quant=0, ss_count=K // 16 if norm else 0, norm_dim=K, **kw)
                    seen.add((g["mbw"], g["split"], g["tall"]))
    skinny = {(mbw, split) for mbw, split, tall in seen if not tall}
    assert any(tall for _, _, tall in seen) and skinny
    assert {mbw for mbw, _ in skinny} == {1, 2, 3}                     # 4: see the docstring
    assert {split for _, split in skinny} >= {1, 2, 3, 4}


# ---------------------------------------------------------------------------------------------------
# the reference set
# ---------------------------------------------------------------------------------------------------
def _request(i, max_tokens=None):
    from qwen3tts import GenerationRequest
    long_row = i % 16 == LONG_ROW
    r = tiny_request(row=i, n_text=5 + (7 * i) % 11, n_instruct=56 if long_row else (3 if i % 5 == 0 else 0),
                     speaker=["aiden", "vivian", "eric"][i % 3], language=["english", "auto", "chinese"][i % 3])
    return GenerationRequest(r["text_ids"], r["target_token_count"], r["instruct_ids"], r["speaker"], r["language"],
                             CAPS[i % 4] if max_tokens is None else max_tokens)


class Kept:
    """A result kept for the module: copies, so that no view over the library's buffers outlives its call."""

    def __init__(self, r):
        self.status, self.codes, self.audio = int(r.status), np.array(r.codes, np.int32), np.array(r.audio, np.float32)
        self.frames = int(self.codes.shape[0])


def _equal(got, want, what):
    assert got.status == want.status, what
    assert got.codes.shape == want.codes.shape and np.array_equal(got.codes, want.codes), what
    a, b = np.ascontiguousarray(got.audio, np.float32), want.audio
    assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), what   # the raw float32 words
    if want.status != 0:
        assert want.frames == 0 and a.size == 0, what


def _load(d, **kw):
    from qwen3tts import Qwen3TTSModel
    return Qwen3TTSModel.from_pretrained(d, max_batch=MAX_BATCH, max_frames=MAX_FRAMES, max_prompt=MAX_PROMPT, **kw)


class World:
    """The default handles of both checkpoints and every request alone on them, computed once per (checkpoint, keywords,
    request, cap) and left unchanged."""

    def __init__(self, ckpt_dirs):
        self.dirs = ckpt_dirs
        self.models = {n: _load(ckpt_dirs[n]) for n in NAMES}
        self._solo = {}

    def solo(self, name, kw_name, i, max_tokens=None, row_base=None, extra=()):
        cap = CAPS[i % 4] if max_tokens is None else max_tokens
        base = i if row_base is None else row_base
        key = (name, kw_name, i, cap, base, extra)
        if key not in self._solo:
            r = self.models[name].generate_batch([_request(i, cap)], row_base=base, **KWS[kw_name], **dict(extra))[0]
            self._solo[key] = Kept(r)
        return self._solo[key]

    def close(self):
        for m in self.models.values():
            m.close()


@pytest.fixture(scope="module")
def world(ckpt_dirs):
    w = World(ckpt_dirs)
    yield w
    w.close()


def _check_batch(world, m, name, kw_name, B, what=""):
    got = m.generate_batch([_request(i) for i in range(B)], **KWS[kw_name])
    assert len(got) == B
    for i in range(B):
        _equal(got[i], world.solo(name, kw_name, i), "%s %s B=%d row %d %s" % (name, kw_name, B, i, what))
    return got


# ---------------------------------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_the_reference_set_is_what_the_tests_need(world, name):
    """Forced rows all have their 8 frames; of the 80 free-running rows at most a quarter fail alone (first token EOS), some
    end before their cap and some at it; the long prompts really pass one 64-token KV page."""
    m = world.models[name]
    forced = [world.solo(name, "forced", i) for i in range(N_REQS)]
    assert all(r.status == 0 and r.frames == 8 for r in forced)
    free = [world.solo(name, "free", i) for i in range(N_REQS)]
    frames = [r.frames for r in free]
    print(name, "free-running frames alone:", frames)
    zero = sum(1 for f in frames if f == 0)
    assert zero <= N_REQS // 4, (zero, frames)
    for i, r in enumerate(free):
        assert r.status == (0 if r.frames else 2) and r.frames <= CAPS[i % 4]
    assert any(0 < f < CAPS[i % 4] for i, f in enumerate(frames)) and any(f == CAPS[i % 4] for i, f in enumerate(frames))
    for i in range(LONG_ROW, N_REQS, 16):
        ie, _, _ = m.debug_prepare_inputs(_request(i))
        assert 64 < ie.shape[0] <= MAX_PROMPT, (i, ie.shape)
    assert m.debug_prepare_inputs(_request(0))[0].shape[0] < 64


@pytest.mark.gpu
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("kw_name", ["forced", "free"])
@pytest.mark.parametrize("name", NAMES)
def test_batch_matrix(world, name, kw_name, B):
    """Every row i < B of generate_batch(reqs[:B]) equals request i alone: row blocks 16 | 17, 32 | 33, 48 | 49, 64; the norm
    prologue (B * 16 <= 64 rows per prefill launch, B <= 4) against launch_norm_rows and the tall GEMM (B = 5 ..); prefill
    launches of up to 1024 rows; a prompt on two KV pages in every row block; free-running, finished rows beside running ones
    at every position and rows that fail alone with the status they have alone."""
    _check_batch(world, world.models[name], name, kw_name, B)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [33, 64])
@pytest.mark.parametrize("name", NAMES)
def test_placement(world, name, B):
    """Greedy decoding does not depend on the random-stream key, so a request may sit in any row: with the requests reversed,
    request j at row B-1-j equals its greedy result alone (at row_base 0)."""
    m = world.models[name]
    got = m.generate_batch([_request(j) for j in reversed(range(B))], **GREEDY)
    for j in range(B):
        _equal(got[B - 1 - j], world.solo(name, "greedy", j, row_base=0), "%s B=%d request %d at row %d" % (name, B, j, B - 1 - j))


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_64_activation_rows_per_launch(world, name, monkeypatch):
    """Q3TTS_ROWS_64 = 1 before the load: Mp_ = 64, so the prefill takes 12, 4, 3, 2 positions per launch and, from B = 33,
    one (prefill_load + advance_len per position), and from B = 33 the predictor's step 0 is two passes -- without a projection
    (tiny-a) staged through cp_x2_ / cp_ss2_ and two copy_rows launches. Every row of every batch of the list equals the
    request alone on the DEFAULT handle, forced and free-running. That the two-pass branch really ran is read off
    q3tts_timing.launches_per_frame_step: the pair pass saves a whole pass of launches, so B = 33 counts more than B = 32."""
    from qwen3tts import _lib
    for kw_name in ("forced", "free"):      # (before the switch is set: these run on the default handle)
        for i in range(MAX_BATCH):
            world.solo(name, kw_name, i)
    monkeypatch.setenv(ROWS_ENV, "1")
    m = None
    try:
        m = _load(world.dirs[name])
        launches = {}
        for B in BS:
            for kw_name in ("forced", "free"):
                _check_batch(world, m, name, kw_name, B, "(64 rows per launch)")
            launches[B] = m.last_timing().launches_per_frame_step
        print(name, "launches per frame step:", launches)
        assert launches[33] > launches[32] > 0 and launches[64] > launches[32], launches
    finally:
        if m is not None:
            m.close()
        monkeypatch.delenv(ROWS_ENV, raising=False)
        _lib.reload_debug_env()   # the switches are process-wide and read at model load: leave the defaults behind


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_lanes_and_eager(world, name):
    """n_streams = 2 splits max_batch into 32 + 32 rows on two engines (Mp_ = 512 each): B = 33 and B = 64 equal the requests
    alone on the one-lane handle. Without the frame graph (use_graph = False) B = 33 does too."""
    for i in range(MAX_BATCH):
        world.solo(name, "forced", i), world.solo(name, "free", i)
    two = _load(world.dirs[name], n_streams=2)
    try:
        for B in (33, 64):
            for kw_name in ("forced", "free"):
                _check_batch(world, two, name, kw_name, B, "(two lanes)")
    finally:
        two.close()
    eager = _load(world.dirs[name], use_graph=False)
    try:
        for kw_name in ("forced", "free"):
            _check_batch(world, eager, name, kw_name, 33, "(eager)")
    finally:
        eager.close()


@pytest.mark.gpu
@pytest.mark.parametrize("S,N", QUEUES)
@pytest.mark.parametrize("name", NAMES)
def test_queue_at_real_slot_counts(world, name, S, N):
    """generate_queued with 16, 17, 33 and 64 slots, free-running: request i equals itself alone. Requests S-8 .. S-1 carry the
    shortest cap, so the highest slots come free first and requests S .. N-1 are admitted -- through the qk_ sub-batch and
    admit_rows -- into slots of row blocks 1..3. No event carries a request's slot: where each request lands is read off
    simulate_slots (the admission order of Engine::admit), which is held against the engine by the call's frame steps."""
    m = world.models[name]
    caps = queue_caps(S, N)
    want = [world.solo(name, "free", i, caps[i]) for i in range(N)]
    got = m.generate_queued([_request(i, caps[i]) for i in range(N)], slots=S, **FREE)
    assert len(got) == N
    tm = m.last_timing()
    assert tm.rows == N
    for i in range(N):
        _equal(got[i], want[i], "%s slots=%d request %d" % (name, S, i))
    placed, steps = simulate_slots([w.frames for w in want], caps, S)
    refills = sorted(placed[i] for i in range(S, N))
    print(name, "slots", S, "refilled slots", refills, "frame steps", tm.frame_steps, "simulated", steps)
    assert tm.frame_steps == steps, (tm.frame_steps, steps)
    if S > 16:
        assert any(s >= (32 if S == 64 else 16) for s in refills), refills
    assert max(refills) >= S - 8, refills


def _check_events(events, res, n_reqs, spf):
    """Per request (tests/test_queued_stream.py): TOKEN / AUDIO_CHUNK interleaved, then INFO, then AUDIO; chunk k at sample
    k * 8 * samples_per_frame, in order; ceil(F / 8) pieces that concatenate to AUDIO."""
    C_ = STREAM["audio_chunk_frames"]
    for i in range(n_reqs):
        mine = [(k, p) for (j, k, p) in events if j == i]
        F = res[i].codes.shape[0]
        if F == 0:
            assert res[i].status == 2 and mine == [], i
            continue
        kinds = [k for k, _ in mine]
        assert kinds[-2:] == ["info", "audio"], (i, kinds)
        assert set(kinds[:-2]) <= {"token", "audio_chunk"} and kinds.count("token") == F, (i, kinds)
        pieces = [p for k, p in mine if k == "audio_chunk"]
        assert len(pieces) == -(-F // C_), (i, F, len(pieces))
        assert [o for o, _ in pieces] == [k * C_ * spf for k in range(len(pieces))], i
        cat = np.concatenate([p for _, p in pieces])
        assert cat.size == F * spf and np.array_equal(cat.view(np.uint32), np.ascontiguousarray(res[i].audio).view(np.uint32)), i
        assert np.array_equal(mine[-1][1], res[i].audio), i


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_streamed_queue_at_17_slots(world, name):
    """The slotted codec stream with a slot in the second row block: 26 requests on 17 slots, audio streamed as (8, 32, 4).
    Each request equals itself streamed alone; its chunks sit at k * 8 * samples_per_frame and concatenate to its audio."""
    m = world.models[name]
    S, N = 17, 26
    caps = queue_caps(S, N)
    extra = tuple(sorted(STREAM.items()))
    want = [world.solo(name, "free", i, caps[i], extra=extra) for i in range(N)]
    events = []
    got = m.generate_queued([_request(i, caps[i]) for i in range(N)], slots=S, on_event=lambda i, k, p: events.append((i, k, p)),
                            **FREE, **STREAM)
    assert len(got) == N and m.last_timing().rows == N
    for i in range(N):
        _equal(got[i], want[i], "%s streamed request %d" % (name, i))
        assert want[i].codes.shape == world.solo(name, "free", i, caps[i]).codes.shape   # streaming does not change the codes
        assert np.array_equal(want[i].codes, world.solo(name, "free", i, caps[i]).codes)
    _check_events(events, got, N, int(m.info.samples_per_frame))
    # the first admission fills the slots in order: request 16 sits in slot 16, the stream's second row block, and has audio
    assert want[16].frames > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_cancel_above_bit_31(world, name):
    """A session with 40 slots and 40 requests of 30 forced frames each (a handle of its own: max_frames 32). Ticket t sits in
    slot t: the callback holds the loop at ticket 0's first boundary until all 40 are submitted, nothing has retired by then
    (a row needs 30 steps, a burst is 9), and the admission behind it fills the remaining slots in ticket order. At ticket 0's
    12th TOKEN -- its second boundary, 18 steps at most -- tickets 33 and 39 are cancelled while they run: bits 33 and 39 of
    the 64-bit mask of cancel_rows. Those two report what tests/test_session.py asserts for a cancelled request; the other 38
    equal themselves alone."""
    from qwen3tts import Qwen3TTSModel
    n, victims = 40, (33, 39)
    kw = dict(FORCED, force_frames=30)
    m = Qwen3TTSModel.from_pretrained(world.dirs[name], max_batch=n, max_frames=32, max_prompt=MAX_PROMPT)
    try:
        reqs = [_request(i, 30) for i in range(n)]
        alone = [Kept(m.generate_batch([reqs[i]], row_base=i, **kw)[0]) for i in range(n)]
        assert all(a.frames == 30 for a in alone)
        state = {"tokens": 0, "error": None}
        all_in = threading.Event()
        events = []

        def on_event(i, kind, payload):
            events.append((i, kind))
            if i != 0 or kind != "token":
                return
            state["tokens"] += 1
            try:
                if state["tokens"] == 1:
                    assert all_in.wait(WAIT)
                if state["tokens"] == 12:
                    for t in victims:
                        s.cancel(t)
            except Exception as e:   # (an exception must not cross the C callback)
                state["error"] = e

        s = m.open_session(slots=n, on_event=on_event, **kw)
        try:
            assert [s.submit(r) for r in reqs] == list(range(n))
            all_in.set()
            got = {t: s.result(t, timeout=WAIT) for t in range(n)}
            assert state["error"] is None, state
            st = s.stats()
            assert (st.cancelled, st.completed, st.running, st.pending, st.admissions) == (2, n - 2, 0, 0, n)
            s.close()
        finally:
            s.close(drain=False)
        for t in range(n):
            kinds = [k for (i, k) in events if i == t]
            if t in victims:
                r = got[t]
                assert r.status == 8 and r.codes.shape == (0, 16) and r.audio.size == 0, t
                assert set(kinds) == {"token"} and BURST <= len(kinds) <= 2 * BURST, (t, kinds)   # no INFO, no AUDIO
            else:
                _equal(got[t], alone[t], "%s ticket %d" % (name, t))
                assert kinds == ["token"] * 30 + ["info", "audio"], (t, kinds)
    finally:
        m.close()


def _ragged_codes(B, seed):
    """Codes as tests/test_gpu_parity.py test_codec_batch_ragged_and_length_rule draws them, frame counts 1 .. 16 all present."""
    rng = np.random.default_rng(seed)
    F = [1 + (5 * b + 3) % MAX_FRAMES for b in range(B)]
    codes = np.zeros((B, MAX_FRAMES, 16), np.int32)
    for b, f in enumerate(F):
        codes[b, :f, 0] = rng.integers(1, 2048, f)
        codes[b, :f, 1:] = rng.integers(0, 256, (f, 15))
    return codes, F


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_codec_alone(world, name):
    """codec_decode of 17 and of 64 ragged rows: each row's samples and length equal the row decoded alone; with the scratch
    budget cut to 1 MB the 64 rows go through in row groups and come out with the same bits."""
    from qwen3tts import _lib
    m = world.models[name]
    spf = int(m.info.samples_per_frame)
    codes, F = _ragged_codes(64, 11)
    assert set(F) == set(range(1, MAX_FRAMES + 1))
    alone = []
    for b, f in enumerate(F):
        pcm, lens = m.codec_decode(codes[b:b + 1, :f])
        alone.append((pcm[0].copy(), int(lens[0])))

    def check(pcm, lens, B, what):
        for b in range(B):
            a, w = np.ascontiguousarray(pcm[b, :F[b] * spf]), alone[b][0]
            assert np.array_equal(a.view(np.uint32), w.view(np.uint32)), (name, what, b)
            assert int(lens[b]) == alone[b][1] == F[b] * spf, (name, what, b)

    for B in (17, 64):
        pcm, lens = m.codec_decode(codes[:B], F[:B])
        check(pcm, lens, B, "B=%d" % B)
    _lib.lib().q3tts_debug_set_codec_scratch(1 << 20)
    try:
        pcm, lens = m.codec_decode(codes, F)
    finally:
        _lib.lib().q3tts_debug_set_codec_scratch(0)
    check(pcm, lens, 64, "row groups")
