"""Block-level parity of the fused sampler (csrc/kernels/sampler.hip: sampler_kernel<1024, 2048, false>, <1024, 4096, false>,
<1024, 4096, true> and sampler_fend_kernel, the last draw of a frame with the end-of-frame job of csrc/kernels/row_jobs.h riding
along) through q3tts_debug_lmop ops 0 and 1: one launch of the product's own launcher per case on caller-built buffers (the slot
table: include/q3tts.h), and everything the launch writes compared, not the token alone.

References.
  token      oracle o_sample_token on the row's bf16 logits, bit-exact, with draw = n_frames[b] * 16 + cb and row = row_key[b], or
             sp[b].row0 + b without keys. A plain (code-predictor) launch ignores the suppress range, EOS, mask_eos and the
             repetition flags whatever the arguments hold; the oracle is called without them.
  state      a numpy restatement (sampler_ref below) of the loop bookkeeping the kernel folds in (the reference's talker loop:
             generatedTokens.append, the EOS break in front of the code store, codeTokens.append): cur_codes, codes, seen,
             finished, active, kv_len, sampled, logits_dump, n_frames -- every array whole and ==, so a write to a neighbouring
             row or a stale flag shows as a changed sentinel. A row that enters finished writes nothing, except kv_len += 1 exactly
             when `advance` is set and no advance_gate is given.
  next_x     the table row of the code used (forced, else drawn) at act_tiled_offset(b + next_row0, ., next_MB), restated from
             csrc/common.h in tests/_lm_block.py; every other element keeps its sentinel.
  next_ss    with emb_ss the exact copy emb_ss[used][j] -> next_ss[j * next_ss_ld + b + next_row0]; without, the float64 sum of
             squares of the row under (H + 1) 2^-24 sum x^2 (the squares of bf16 values are exact in fp32 and each of the H - 1
             additions rounds once, in whatever order: DESIGN.md section 2; derived from the code, never a constant floor).
  frame end  op 1: sampler_ref, then tests/_lm_block.py frame_end_ref (the restatement test_lmrow_block.py checks on its own).
             The rider form and the split form (launch_sampler, then launch_frame_end) return every array bit-equal, ss_out
             included: both run next_input_row and block_sum_first256 on the same values. cp_len is the sampler's kv_len array as
             in the frame step, so a finished row's advance (+1) is reset to 0 by both forms.

NaN logits. Only the kernel's own written rule is held: a row of all NaN gives token 0 (sampler.hip "every logit NaN"), compared
with the literal 0, and every index written from it is in range. The oracle is not asked; in one sub-case it differs: a talker
row with top-p on and an EOS returns eos_id there, because its top-p cuts every NaN to -inf, step 7 restores the (NaN) EOS logit
and the categorical stage takes the first candidate it meets, while the kernel's arg-max never takes a NaN. Neither side is
changed here. (What this test did find and the kernel now handles: a greedy talker row took the first index of the suppressed
range, whose -inf beat every NaN -- token 2048 of 3072 instead of 0.) No other input holds a NaN.

The CPU part (no marker) runs every case's check_only call (the case table is launchable), the host refusals, the reference's own
invariants on every case (the token inside the vocabulary and never a suppressed index while a live one exists; greedy rows equal a
numpy arg-max; cur_codes holds the forced code or the token) and the dispatch table: every instantiation is reached. The GPU part
runs the same cases through the launchers and prints WORST (error / bar of the sums of squares)."""
import ctypes as C
import functools

import numpy as np
import pytest

from _lm_block import (WORST, b2f, bf_noise, check_only, compare, f2b, frame_end_ref, job, launch, mutate, rng_of, sent,
                       sp_rows, ss_bar, table_pool, tiled_index)

NEG = -np.inf


# ---------------------------------------------------------------------------------------------
# logits
# ---------------------------------------------------------------------------------------------
def grid(key, V, shift=2.0):
    """the 0.1-grid of test_sampler_top_p.py: many equal keys; exp(logit) is what top-p sums, unnormalised, so rows are shifted"""
    return np.round(rng_of("grid", key, V).standard_normal(V) * 1.5, 1) - shift


def equal_row(V, v=-1.5):
    return np.full(V, v)


def ties_row(V):
    """equal values on both sides of a lane (63 | 64), a slice (1023 | 1024) and a 2048 (2047 | 2048) boundary, above everything else"""
    x = grid("ties", V, 6.0)
    for (i, j), v in (((63, 64), 5.0), ((1023, 1024), 4.0), ((2047, 2048), 3.0)):
        if j < V:
            x[i] = x[j] = v
    return x


def greedy_ties_row(V):
    """one maximum at three indices in three slices of 1024; the lowest index belongs to the highest thread of the three"""
    x = grid("gties", V, 4.0)
    for i in (1030, 2050, 3074):
        if i < V:
            x[i] = 9.0
    if V <= 1030:
        x[[V // 3, V // 2]] = 9.0
    return x


def only(V, idx, v=1.0):
    x = np.full(V, NEG)
    if idx is not None:
        x[idx] = v
    return x


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------
def R(logits, T=0.9, k=50, p=1.0, rep=1.0, seed=77, frame=0, finished=0, active=1, gate=1, key=None):
    return dict(logits=logits, T=T, k=k, p=p, rep=rep, seed=seed, frame=frame, finished=finished, active=active, gate=gate, key=key)


def case(name, V, rows, talker=0, sup=(0, 0), eos=-1, mask_eos=0, cb=0, advance=0, Fmax=4, use_gate=False, use_keys=False, row0=3,
         seen=False, ff=0, forced=False, sampled=False, dump=0, H=0, next_row0=0, next_MB=None, emb_ld=None, nss=0, ss_ld=0, want_ss=True,
         ldl=None, fe=None, key=None):
    return dict(key=key or name, name=name, V=V, rows=rows, talker=talker, sup=sup, eos=eos, mask_eos=mask_eos, cb=cb, advance=advance, Fmax=Fmax,
                use_gate=use_gate, use_keys=use_keys, row0=row0, seen=seen, ff=ff, forced=forced, sampled=sampled, dump=dump, H=H,
                next_row0=next_row0, next_MB=next_MB, emb_ld=emb_ld, nss=nss, ss_ld=ss_ld, want_ss=want_ss, ldl=ldl or V + 8 * (V % 3), fe=fe)


def sweep_rows(V, key):
    return [R(grid((key, 0), V), T=0.0), R(grid((key, 1), V, 3.5), T=0.9, k=50 if V > 50 else 0, p=1.0, seed=5),
            R(grid((key, 2), V, 5.0), T=1.0, k=0, p=0.6, seed=6), R(equal_row(V), T=-1.0), R(greedy_ties_row(V), T=0.0)]


def kp_rows(V, key):
    """top_k {0, 1, V - 1, V, V + 1} x top_p {0, 0.05, 0.999, 1.0}, the temperature walking {1e-3, 0.9}; greedy rows of both signs"""
    rows = [R(grid((key, "g", 0), V), T=-1.0, k=1, p=0.05), R(grid((key, "g", 1), V), T=0.0, k=V - 1, p=0.999)]
    n = 0
    for k in (0, 1, V - 1, V, V + 1):
        for p in (0.0, 0.05, 0.999, 1.0):
            rows.append(R(grid((key, n % 3), V, 2.0 + 1.5 * (n % 4)), T=(1e-3, 0.9)[n % 2], k=k, p=p, seed=100 + n, frame=n % 3))
            n += 1
    return rows


def talker_rows(V, key, eos):
    rows = [R(grid((key, 0), V), T=0.0, rep=1.05), R(grid((key, 1), V, 3.0), T=0.9, k=50, p=1.0, rep=1.05, seed=8),
            R(grid((key, 2), V, 4.0), T=0.7, k=0, p=0.6, rep=1.0, seed=9), R(grid((key, 3), V, 2.5), T=0.9, k=65, p=0.95, rep=1.3, seed=10, frame=2)]
    if eos >= 0:
        rows.append(R(only(V, eos), T=0.9, k=50, p=0.6, seed=11))   # nothing finite but EOS
        rows.append(R(only(V, eos), T=0.0))
    return rows


def gather_case(name, H, with_table, **kw):
    V, B = 48, 17
    rows = [R(grid((name, b), V), T=(0.0, 0.9)[b % 2], k=(0, 5)[b % 2], seed=b, frame=b % 3) for b in range(B)]
    return case(name, V, rows, H=H, next_row0=B, next_MB=3, nss=H // 16 if with_table else 0, ss_ld=40 if with_table else 0, **kw)


def fe_spec(groups, open_text):
    """the five rows of the rider-against-split cases: finished | at max_frames - 1 | text | tts_pad | (open text) starving"""
    return dict(groups=groups, H=256, Tmax=3, hMB=1, Vt=24, Vcp=40, n_trailing=[2, 3, 2, 1, 1], trailing_idx=[0, 1, 1, 1, 1],
                max_frames=[50, 3, 50, 50, 50], text_open=[0, 0, 0, 0, 1] if open_text else None)


@functools.lru_cache(maxsize=None)
def cases():
    cs = []
    for V in (1, 2, 255, 1024, 1025, 2047, 2048, 2049, 3000, 4095, 4096):
        cs.append(case("plain-V%d" % V, V, sweep_rows(V, ("sweep", V))))
    for V, talker in ((2047, 0), (3000, 0), (3072, 1)):
        sup = (V - 1024, V) if talker else (0, 0)
        cs.append(case("kp-%s-V%d" % ("talker" if talker else "plain", V), V, kp_rows(V, ("kp", V)), talker=talker, sup=sup,
                       eos=V - 900 if talker else -1, seen=bool(talker)))
    for V, talker in ((2048, 0), (4096, 0), (3072, 1)):
        ks = (1, 2, 65, 1025, V - 1)
        rows = [R(equal_row(V), T=0.9, k=k, p=1.0, seed=20 + i) for i, k in enumerate(ks)] + [R(equal_row(V), T=0.8, k=65, p=0.6, seed=31)]
        rows += [R(ties_row(V), T=0.9, k=k, p=1.0, seed=40 + k) for k in (1, 3, 5)] + [R(ties_row(V), T=0.0), R(greedy_ties_row(V), T=-1.0)]
        rows += [R(only(V, None), T=0.9), R(only(V, None), T=0.0), R(only(V, None), T=0.9, k=0, p=0.5)]
        cs.append(case("ties-%s-V%d" % ("talker" if talker else "plain", V), V, rows, talker=talker, sup=(V - 1024, V) if talker else (0, 0),
                       eos=5 if talker else -1))
    for V in (300, 3000, 3072):
        lo = max(0, V - 1024)
        for eos in ([V - 10, -1] if lo == 0 else [V - 10, 7, -1]):
            for mask in (0, 1):
                cs.append(case("talker-V%d-eos%d-mask%d" % (V, eos, mask), V, talker_rows(V, ("talker", V, eos, mask), eos), talker=1, sup=(lo, V),
                               eos=eos, mask_eos=mask, seen=True, advance=1, H=128, next_MB=1))
    for cb in (0, 1, 7, 15):   # frames 0, 1, 10 against Fmax = 5: the last stores no code
        rows = [R(grid(("cb", cb, f), 2048, 3.0), T=0.9, k=50, seed=cb, frame=f) for f in (0, 1, 10)]
        cs.append(case("cb%d" % cb, 2048, rows, cb=cb, Fmax=5, use_keys=cb in (1, 15), row0=0 if cb == 1 else 9))
    # row states. talker: live | not active | finished | lands on EOS | finished; plain without and with a gate
    tr = [R(grid("st0", 300), T=0.0), R(grid("st1", 300), T=0.0, active=0), R(grid("st2", 300), finished=1, active=0), R(only(300, 295), T=0.9, k=0),
          R(grid("st4", 300), finished=1)]
    for adv in (0, 1):
        cs.append(case("talker-states-adv%d" % adv, 300, tr, talker=1, sup=(0, 300), eos=295, seen=True, advance=adv, H=128, next_MB=1))
    pr = [R(grid("ps0", 255), T=0.0), R(grid("ps1", 255), finished=1), R(grid("ps2", 255), T=0.9, gate=0), R(grid("ps3", 255), finished=1, gate=0)]
    for adv, g in ((1, False), (1, True), (0, False)):
        cs.append(case("plain-states-adv%d-gate%d" % (adv, g), 255, pr, cb=3, advance=adv, use_gate=g))
    # teacher forcing, the record of what was drawn and the logits dump: frames 0, 1 inside forced_frames = 2, frame 3 behind
    fr = [R(grid(("tf", f), 1025, 3.0), T=0.9, k=10, seed=f, frame=f) for f in (0, 1, 3)]
    cs.append(case("forced-plain", 1025, fr, cb=7, ff=2, forced=True, sampled=True, dump=1025 + 8 + 3, H=128, next_MB=1))
    cs.append(case("forced-talker", 300, [R(grid(("tft", f), 300), T=0.0, frame=f) for f in (0, 1, 3)], talker=1, sup=(0, 300), eos=295, seen=True,
                   ff=2, forced=True, sampled=True, dump=300 + 8, H=128, next_MB=1))
    cs.append(case("sampled-only", 255, fr_small(), cb=2, ff=2, sampled=True))
    for H in (128, 1024, 2176):
        cs.append(gather_case("gather-H%d" % H, H, False, emb_ld=H + 8 if H == 128 else None))
        cs.append(gather_case("gather-table-H%d" % H, H, True))
    cs.append(gather_case("gather-no-ss", 128, False, want_ss=False))
    # a row equals itself alone: row 17 of 33 against one row with the same key
    big = [R(grid(("alone", b), 2048, 3.0), T=0.9, k=50, p=0.9, seed=3, frame=1, key=1000 + b) for b in range(33)]
    cs.append(case("row17-of-33", 2048, big, use_keys=True, cb=4, H=128, next_MB=3, key="alone"))
    cs.append(case("row17-alone", 2048, [big[17]], use_keys=True, cb=4, H=128, next_MB=1, key="alone"))
    # the rider against the two launches it replaces
    for groups in (2, 16):
        for open_text in (False, True):
            fe = fe_spec(groups, open_text)
            rows = [R(grid(("fe", b), fe["Vcp"]), T=0.9, k=5, seed=b, frame=(7, 2, 4, 5, 6)[b], finished=int(b == 0)) for b in range(5)]
            for split in (0, 1):
                cs.append(case("fend-g%d-open%d-split%d" % (groups, open_text, split), fe["Vcp"], rows, cb=groups - 1, advance=1, Fmax=8,
                               H=128, next_MB=1, fe=dict(fe, split=split), key=("fend", groups, open_text)))
    return cs


def fr_small():
    return [R(grid(("so", f), 255), T=0.9, k=3, seed=f, frame=f) for f in (0, 1, 2)]


def nan_cases():
    cs = []
    nan = lambda V: np.full(V, np.nan)
    rows = lambda V: [R(nan(V), T=0.0), R(nan(V), T=0.9, k=50), R(nan(V), T=0.9, k=0, p=0.6), R(nan(V), T=0.9, k=65, p=0.6), R(nan(V), T=-1.0, k=1)]
    cs.append(case("nan-plain-2048", 2048, rows(2048), H=128, next_MB=1))
    cs.append(case("nan-plain-3000", 3000, rows(3000), H=128, next_MB=1))
    cs.append(case("nan-talker", 3072, rows(3072), talker=1, sup=(2048, 3072), eos=2150, seen=True, H=128, next_MB=1))
    return cs


# the launcher's dispatch (sampler.hip launch_sampler, launch_sampler_with_frame_end), restated
def instantiation(c):
    if c["fe"] is not None and not c["fe"]["split"]:
        return "fend<1024,2048>"
    if not c["talker"] and c["V"] <= 2048:
        return "plain<1024,2048>"
    return "talker<1024,4096>" if c["talker"] else "plain<1024,4096>"


# ---------------------------------------------------------------------------------------------
# a case -> the call
# ---------------------------------------------------------------------------------------------
def build(c):
    B, V, H = len(c["rows"]), c["V"], c["H"]
    rows = c["rows"]
    logits = sent((B, c["ldl"]), np.uint16)
    for b, r in enumerate(rows):
        logits[b, :V] = f2b(r["logits"])
    sp = sp_rows([(r["T"], r["k"], r["p"], r["rep"], r["seed"], c["row0"], c["mask_eos"]) for r in rows])
    i32 = lambda v: np.array(v, np.int32)
    u8 = lambda v: np.array(v, np.uint8)
    emb_rows = max(V, 1)
    p = {0: B, 1: V, 2: c["ldl"], 3: c["talker"], 4: c["sup"][0], 5: c["sup"][1], 6: c["eos"], 7: c["cb"], 8: c["advance"], 9: c["Fmax"], 10: c["ff"],
         11: emb_rows if H else 0, 12: (c["emb_ld"] or H), 13: H, 14: c["next_MB"] or 0, 15: c["next_row0"], 16: c["nss"], 17: c["ss_ld"], 18: c["dump"],
         19: 8 if c["dump"] else 0}
    ins = {0: logits, 1: sp, 2: i32([1 << 20] * B)}
    if c["use_gate"]:
        ins[3] = u8([r["gate"] for r in rows])
    if c["forced"]:
        ins[4] = rng_of("forced", c["name"]).integers(0, V, (B, c["ff"], 16)).astype(np.int32)
    if c["use_keys"]:
        ins[7] = np.array([r["key"] if r["key"] is not None else 0x80000000 + 17 * b for b, r in enumerate(rows)], np.uint32)
    ios = {0: i32([r["frame"] for r in rows]), 1: u8([r["finished"] for r in rows]), 2: u8([r["active"] for r in rows]),
           3: i32([100 + b for b in range(B)]), 4: sent((B, 16), np.int32)}
    if c["Fmax"]:
        ios[5] = sent((B, c["Fmax"], 16), np.int32)
    if c["seen"]:
        ios[6] = (rng_of("seen", c["name"]).random((B, V)) < 0.05).astype(np.uint8)
    if c["sampled"]:
        ios[7] = sent((B, c["ff"], 16), np.int32)
    if c["dump"]:
        ios[8] = sent((B, c["ff"], c["dump"]), np.uint16)
    if H:
        emb = sent((emb_rows, p[12]), np.uint16)
        emb[:, :H] = bf_noise(("emb", c["key"]), (emb_rows, H))
        ins[5] = emb
        ios[9] = sent(c["next_MB"] * 16 * H, np.uint16)
        if c["nss"]:
            ins[6] = rng_of("embss", c["key"]).random((emb_rows, c["nss"])).astype(np.float32)
            ios[10] = sent((c["nss"], c["ss_ld"]), np.float32)
        elif c["want_ss"]:
            ios[10] = sent(B, np.float32)
    op, fe = "sampler", c["fe"]
    if fe is not None:
        op = "sampler_frame_end"
        pool, offs, tables, pad = table_pool(("fe", fe["groups"]), fe["groups"], fe["H"], fe["Vt"], fe["Vcp"])
        p.update({20: fe["H"], 21: fe["groups"], 22: fe["Tmax"], 23: fe["hMB"], 24: fe["Vt"], 25: fe["Vcp"], 26: fe["split"], 27: 1})
        ins[2] = i32(fe["max_frames"])
        ins.update({8: pool, 9: offs, 10: bf_noise("trailing", (B, fe["Tmax"], fe["H"])), 11: i32(fe["n_trailing"])})
        cur = rng_of("cur", fe["groups"]).integers(0, fe["Vt"], (B, 16)).astype(np.int32)
        ios[4] = cur
        ios[3] = i32([0] * B)   # cp_len: the frame end's array is the sampler's kv_len
        ios.update({11: i32(fe["trailing_idx"]), 12: sent(fe["hMB"] * 16 * fe["H"], np.uint16), 13: sent(B, np.float32)})
        if fe["text_open"] is not None:
            ins[12] = u8(fe["text_open"])
            ios[15] = u8([0] * B)
        c = dict(c, fe=dict(fe, tables=tables, tts_pad=pad, trailing=ins[10]))
    return job(op, p, ins, ios, case=c)


def oracle_token(c, b, logits_row, seen_row):
    from oracle import oracle as O
    r, V = c["rows"][b], c["V"]
    talker = bool(c["talker"])
    key = (r["key"] if r["key"] is not None else 0x80000000 + 17 * b) if c["use_keys"] else (c["row0"] + b) & 0xFFFFFFFF
    lo, hi = (max(0, c["sup"][0]), c["sup"][1]) if talker else (0, 0)
    row = np.ascontiguousarray(logits_row[:V])
    seen = np.ascontiguousarray(seen_row) if (talker and seen_row is not None) else None
    return int(O.lib().o_sample_token(O._p16(row), V, C.c_float(r["T"]), int(r["k"]), C.c_float(r["p"]), C.c_float(r["rep"]),
                                      seen.ctypes.data_as(O.u8p) if seen is not None else None, lo, hi, c["eos"] if talker else -1,
                                      c["mask_eos"] if talker else 0, C.c_uint64(r["seed"]), key, r["frame"] * 16 + c["cb"]))


def sampler_ref(j, token=oracle_token):
    """What the launch must leave in every io slot: ({slot: array}, {slot: {index: (sum, bar)}}, tokens)."""
    c, p, ins = j["case"], j["p"], j["ins"]
    st = {s: np.array(v, copy=True) for s, v in j["ios"].items()}
    B, V, cb, H = p[0], p[1], p[7], p[13]
    talker, advance, Fmax, ff = bool(p[3]), bool(p[8]), p[9], p[10]
    gate, forced = ins.get(3), ins.get(4)
    sums, toks = {}, []
    for b in range(B):
        if st[1][b]:
            if advance and gate is None:
                st[3][b] += 1
            toks.append(None)
            continue
        frame = int(st[0][b])
        if 8 in st and frame < ff:
            st[8][b, frame, p[19]:p[19] + V] = ins[0][b, :V]
        tok = token(c, b, ins[0][b], st[6][b].copy() if 6 in st else None)
        toks.append(tok)
        used = int(forced[b, frame, cb]) if forced is not None and frame < ff else tok
        if 7 in st and frame < ff:
            st[7][b, frame, cb] = tok
        st[4][b, cb] = used
        if talker:
            if 6 in st:
                st[6][b, used] = 1
            if advance and st[2][b]:
                st[3][b] += 1
            if used == p[6]:
                st[1][b], st[2][b] = 1, 0
            elif frame < Fmax:
                st[5][b, frame, 0] = used
        else:
            if advance and (gate is None or gate[b]):
                st[3][b] += 1
            if frame < Fmax:
                st[5][b, frame, cb] = used
        if H:
            row = ins[5][used, :H]
            st[9][tiled_index([b + p[15]], H, p[14])[0]] = row
            if 6 in ins:
                st[10][:, b + p[15]] = ins[6][used]
            elif 10 in st:
                sums.setdefault(10, {})[b] = ss_bar(b2f(row).astype(np.float64), H)
    fe = c["fe"]
    if fe is not None:
        st["cp"] = st[3]
        frame_end_ref(dict(fe, n_trailing=ins[11], max_frames=ins[2], text_open=ins.get(12)), st, sums)
        del st["cp"]
    return st, sums, toks


@functools.lru_cache(maxsize=None)
def reference(i):
    j = build(cases()[i])
    return (j,) + sampler_ref(j)


def case_ids():
    return [c["name"] for c in cases()]


# ---------------------------------------------------------------------------------------------
# CPU part
# ---------------------------------------------------------------------------------------------
def test_every_case_is_launchable():
    for c in cases() + nan_cases():
        assert check_only(build(c)) == 0, c["name"]


def test_case_table_reaches_every_instantiation():
    seen = {instantiation(c) for c in cases()}
    assert seen == {"plain<1024,2048>", "plain<1024,4096>", "talker<1024,4096>", "fend<1024,2048>"}
    table = {(0, 1): "plain<1024,2048>", (0, 2048): "plain<1024,2048>", (0, 2049): "plain<1024,4096>", (0, 4096): "plain<1024,4096>",
             (1, 300): "talker<1024,4096>", (1, 3072): "talker<1024,4096>"}
    for (talker, V), name in table.items():
        assert instantiation(dict(talker=talker, V=V, fe=None)) == name
        assert any(c["talker"] == talker and c["V"] == V for c in cases()), (talker, V)


@pytest.mark.parametrize("i", range(len(cases())), ids=case_ids())
def test_reference_agrees_with_itself(i):
    """The restatement against the oracle's token, every case: the token is an index of the vocabulary, never a suppressed one while
    a live one exists, a greedy row's is the first maximum of the processed row; cur_codes holds it (or the forced code); a row that
    lands on EOS stores no code; nothing of a finished row moves but its kv_len."""
    j, st, sums, toks = reference(i)
    c, p, ins, io0 = j["case"], j["p"], j["ins"], j["ios"]
    V, cb = p[1], p[7]
    for b, (r, tok) in enumerate(zip(c["rows"], toks)):
        if tok is None:
            for s in st:
                if s != 3 and st[s].shape[0] == p[0] and c["fe"] is None:
                    assert st[s][b].tobytes() == io0[s][b].tobytes(), (c["name"], b, s)
            continue
        assert 0 <= tok < V
        x = b2f(ins[0][b, :V]).astype(np.float64)
        if c["talker"]:
            dead = np.zeros(V, bool)
            dead[max(0, p[4]):p[5]] = True
            if p[6] >= 0:
                dead[p[6]] = bool(c["mask_eos"])
            live = ~dead & (x > NEG)
            if live.any():
                assert live[tok] or tok == p[6], (c["name"], b, tok)
            if r["T"] <= 0 and (r["rep"] == 1.0 or 6 not in io0):
                y = np.where(dead, NEG, x)
                assert tok == int(np.argmax(y)), (c["name"], b)
        elif r["T"] <= 0:
            assert tok == int(np.argmax(x)), (c["name"], b)
        elif (x > NEG).any():
            assert x[tok] > NEG
        frame = r["frame"]
        forced = ins.get(4)
        used = int(forced[b, frame, cb]) if forced is not None and frame < p[10] else tok
        assert st[4][b, cb] == used
        if c["talker"] and used == p[6]:
            assert st[1][b] == 1 and st[2][b] == 0 and np.array_equal(st[5][b], io0[5][b])
    if c["fe"] is not None:   # the two forms of a frame's end share one reference
        k = next(n for n, o in enumerate(cases()) if o["name"] == c["name"][:-1] + str(1 - c["fe"]["split"]))
        for s in st:
            assert st[s].tobytes() == reference(k)[1][s].tobytes(), s


def test_bf16_chain_restatement_matches_the_oracle():
    """rbf of tests/_lm_block.py against the oracle's conversion: random values, ties to even, both infinities"""
    from oracle import oracle as O
    x = np.concatenate([rng_of("chain").standard_normal(4096).astype(np.float32) * 37,
                        np.array([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0xBF808000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0, 0x80000000],
                                 np.uint32).view(np.float32)])
    assert np.array_equal(f2b(x), O.f32_to_bf16(x))


REFUSED = {
    "V-4097": lambda j: mutate(j, p={1: 4097, 2: 4104}),
    "ldl-below-V": lambda j: mutate(j, p={2: j["p"][1] - 1}),
    "B-65": lambda j: mutate(j, p={0: 65}),
    "cb-16": lambda j: mutate(j, p={7: 16}),
    "eos-at-V": lambda j: mutate(j, p={6: j["p"][1]}),
    "logits-size": lambda j: mutate(j, ins={0: j["ins"][0][:, :-1].copy()}),
    "sp-size": lambda j: mutate(j, ins={1: j["ins"][1][:-1].copy()}),
    "n-frames-negative": lambda j: mutate(j, ios={0: -np.abs(j["ios"][0]) - 1}),
    "forced-code-at-V": lambda j: mutate(j, ins={4: np.full_like(j["ins"][4], j["p"][1])}),
    "H-not-128": lambda j: mutate(j, p={13: 120}),
    "emb-ld-below-H": lambda j: mutate(j, p={12: 120}),
    "emb-rows-below-V": lambda j: mutate(j, p={11: j["p"][1] - 1}, ins={5: j["ins"][5][:-1].copy()}),
    "next-row0-outside": lambda j: mutate(j, p={15: 16}),
    "dump-off": lambda j: mutate(j, p={19: j["p"][18] - j["p"][1] + 1}),
    "unnamed-slot": lambda j: mutate(j, ios={17: np.zeros(4, np.uint8)}),
    "null-kv-len": lambda j: mutate(j, ios={3: None}),
}
REFUSED_FE = {
    "rider-on-a-talker-draw": lambda j: mutate(j, p={3: 1}),
    "rider-cb": lambda j: mutate(j, p={7: j["p"][7] - 1}),
    "rider-V-over-table": lambda j: mutate(j, p={25: j["p"][1] - 1}),
    "groups-17": lambda j: mutate(j, p={21: 17}),
    "hMB-0": lambda j: mutate(j, p={23: 0}),
    "cur-code-outside": lambda j: mutate(j, ios={4: j["ios"][4] + 1000}),
    "n-trailing-over-Tmax": lambda j: mutate(j, ins={11: j["ins"][11] + 2}),
    "table-outside-pool": lambda j: mutate(j, ins={9: j["ins"][9] + len(j["ins"][8])}),
    "table-misaligned": lambda j: mutate(j, ins={9: j["ins"][9] + 1}),
    "text-open-without-starved": lambda j: mutate(j, ins={12: np.zeros(j["p"][0], np.uint8)}, ios={15: None}),
    "own-cp-len-missing": lambda j: mutate(j, p={27: 0}),
}


@pytest.mark.parametrize("name", list(REFUSED) + list(REFUSED_FE))
def test_host_refusals(name):
    """Every refusal precedes allocation: check_only with m == NULL returns INVALID_INPUT, and the job it was made from is accepted."""
    by = {c["name"]: c for c in cases()}
    j = build(by["forced-plain"] if name in REFUSED else by["fend-g16-open0-split0"])
    assert check_only(j) == 0
    assert check_only((REFUSED.get(name) or REFUSED_FE[name])(j)) == 3, name


# ---------------------------------------------------------------------------------------------
# GPU part
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine(ckpt_dirs):
    from qwen3tts import Qwen3TTSModel
    m = Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-b"], max_batch=1, max_frames=8, max_prompt=16)
    yield m
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(cases())), ids=case_ids())
def test_sampler_block_matches_its_reference(engine, i):
    """One launch (op 1 split: two) of the product's launcher: every returned array against the reference, whole."""
    j, st, sums, _ = reference(i)
    got = launch(engine, j)
    compare("sampler:" + j["case"]["name"], got, st, sums)
    print("GPU, worst error / bar: next_ss / ss_out %.4f" % WORST.get("sampler", 0.0))


@pytest.mark.gpu
@pytest.mark.parametrize("groups", [2, 16])
@pytest.mark.parametrize("open_text", [0, 1])
def test_rider_equals_split(engine, groups, open_text):
    """launch_sampler_with_frame_end against launch_sampler then launch_frame_end on the same arguments: every returned array
    bit-equal, the sums of squares included -- a finished row's cp_len too (0 in both; the rider once left the advance's 1)."""
    by = {c["name"]: n for n, c in enumerate(cases())}
    a, b = (launch(engine, reference(by["fend-g%d-open%d-split%d" % (groups, open_text, s)])[0]) for s in (0, 1))
    compare("rider-split", a, b)
    assert a[3][0] == 0 and a[1][0] == 1   # the finished row: advanced by the draw, reset by the frame's end


@pytest.mark.gpu
def test_a_row_equals_itself_alone(engine):
    by = {c["name"]: n for n, c in enumerate(cases())}
    big, one = (launch(engine, reference(by[n])[0]) for n in ("row17-of-33", "row17-alone"))
    H = 128
    for s in (0, 1, 2, 3, 4, 5):
        assert np.array_equal(big[s][17] - (17 if s == 3 else 0), one[s][0]), s
    assert np.array_equal(big[9][tiled_index([17], H, 3)[0]], one[9][tiled_index([0], H, 1)[0]])
    assert big[10][17].tobytes() == one[10][0].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(nan_cases())), ids=[c["name"] for c in nan_cases()])
def test_all_nan_row_gives_token_zero(engine, i):
    """The kernel's written rule, against the literal 0 (the module docstring's NaN note): the bookkeeping of a drawn 0 follows."""
    j = build(nan_cases()[i])
    st, sums, toks = sampler_ref(j, token=lambda *a: 0)
    assert toks == [0] * len(toks)
    got = launch(engine, j)
    assert (got[4][:, j["p"][7]] == 0).all() and (got[5][:, 0, 0] == 0).all()
    compare("sampler:" + j["case"]["name"], got, st, sums)


@pytest.mark.gpu
def test_refused_arguments_launch_nothing(engine):
    """With a live model: a refused call (status 3) raises, and a good call afterwards works."""
    from qwen3tts import Qwen3TTSError
    by = {c["name"]: n for n, c in enumerate(cases())}
    j, st, sums, _ = reference(by["forced-plain"])
    bad = REFUSED["forced-code-at-V"](j)
    with pytest.raises(Qwen3TTSError) as e:
        launch(engine, bad)
    assert e.value.status == 3
    compare("sampler:forced-plain", launch(engine, j), st, sums)
