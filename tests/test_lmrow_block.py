"""Block-level parity of the row kernels of the LM side of the frame step (csrc/kernels/lm_misc.hip with the jobs of
csrc/kernels/row_jobs.h) through q3tts_debug_lmop ops 2-18: one launch of the product's own launcher per case on caller-built
buffers (the slot table: include/q3tts.h). Everything here is a copy, an integer update or a bf16 add, so every returned buffer is
compared whole and == on raw bytes with a numpy restatement written here, sentinels included: what a launch does not own keeps
its bits. The only bars are on the fp32 sums of squares (ss_out of frame_end, prefill_load and prefill_chunk_load): the float64
sum under (H + 1) 2^-24 sum x^2 -- the squares of bf16 values are exact in fp32, each of the H - 1 additions rounds once in
whatever order (derived from the code, never a constant floor); a padding row's sum is exactly 0.

  frame_end           text row (or tts_pad) + the groups' embedding rows, left to right, every add rounded to bf16 (the
                      restatement of test_session_open_text.py); n_frames + 1, the max_frames cap, an open row without text
                      starves (no input formed, parked as finished with starved up); a finished row: cp_len = 0 and nothing else
  gather_rows         out[i] = table[token_map[ids[i]]] row-major or tiled; tile_rows / untile_rows against the offset function and
                      as a round trip; copy_rows with the engine's stride-0 single row; ss_to_table the transpose
  add_rows            bf16(a + b), one rounding, ldb = 0 broadcasts; compose_rows b = -1 copy, b >= 0 table, b <= -2 extra
  ref_embed_rows      the left-to-right chain over [groups][T] codes; f32_to_bf16 round to nearest even
  prefill_load        row b loads position step - (Pmax - n_prompt[b]); a row that has not started gets active = 0 and loads its
                      position 0; prefill_chunk_load row m = p B + b, positions r < 0 are zero rows with ss = 0
  advance_len(_chunk) kv_len += 1 for active rows; += C - min(max(-r0, 0), C)
  admit_rows          the listed slots' rows of every array, and no other slot's; slot -1 writes nothing
  text_append_rows    append, close (the EOS row, text_open down, max_frames), the resume of a starved row (from the source row, or
                      the EOS row when n_new = 0), a descriptor that does not fit behind n_trailing writes nothing
  cancel_rows         finished up, active down for the mask's bits below `slots`; mask 0 launches nothing

The CPU part (no marker) runs every case's check_only call and the host refusals, one per class of check, and holds the shared
restatements to themselves; the GPU part launches every case and prints WORST."""
import functools

import numpy as np
import pytest

from _lm_block import (ADMIT, SP, TEXT, WORST, b2f, bf_noise, check_only, compare, f2b, frame_end_ref, job, launch, layout_is_a_bijection, mutate,
                       next_input, rbf, rng_of, sent, ss_bar, table_pool, tiled_index)

i32 = lambda v: np.array(v, np.int32)
u8 = lambda v: np.array(v, np.uint8)
U16, F32 = np.uint16, np.float32


def copies(ios):
    return {s: np.array(v, copy=True) for s, v in ios.items()}


def tiled_store(buf, rows, H, MB, values):
    buf.reshape(-1)[tiled_index(rows, H, MB)] = values


# ---------------------------------------------------------------------------------------------
# the ops: each returns [(job, expected io, sums)]
# ---------------------------------------------------------------------------------------------
def frame_end_jobs():
    out = []
    for groups, H, B, open_text in ((16, 128, 17, True), (2, 2176, 64, False), (1, 2048, 1, False), (16, 2048, 17, False), (2, 128, 64, True)):
        key = ("frame_end", groups, H, B)
        Tmax, hMB, Vt, Vcp = 3, -(-B // 16), 24, 40
        pool, offs, tables, pad = table_pool(key, groups, H, Vt, Vcp)
        kind = np.arange(B) % 6   # 0 text | 1 tts_pad (or starving) | 2 cap | 3 finished | 4 cap and no text | 5 text at the last row
        n_trailing = i32(np.where(kind == 5, 3, 2))
        ti = i32(np.select([(kind == 0) | (kind == 2), kind == 5], [0, 2], 2))
        n_frames = i32(3 + np.arange(B))
        max_frames = i32(np.where((kind == 2) | (kind == 4), n_frames + 1, 10 ** 6))
        fin, act = u8(kind == 3), u8(kind != 3)
        trailing = bf_noise((key, "trailing"), (B, Tmax, H))
        cur = rng_of(key, "cur").integers(0, Vt, (B, 16)).astype(np.int32)
        text_open = u8((np.arange(B) % 2) == 1) if open_text else None
        p = {0: B, 20: H, 21: groups, 22: Tmax, 23: hMB, 24: Vt, 25: Vcp}
        ins = {2: max_frames, 8: pool, 9: offs, 10: trailing, 11: n_trailing}
        ios = {0: n_frames, 1: fin, 2: act, 4: cur, 11: ti, 12: sent(hMB * 16 * H, U16), 13: sent(B, F32), 14: i32(5 + np.arange(B))}
        if open_text:
            ins[12] = text_open
            ios[15] = u8([0] * B)
        j = job("frame_end", p, ins, ios)
        st, sums = copies(ios), {}
        st["cp"] = st[14]
        frame_end_ref(dict(tables=tables, tts_pad=pad, trailing=trailing, n_trailing=n_trailing, max_frames=max_frames, text_open=text_open,
                           groups=groups, hMB=hMB, H=H), st, sums)
        del st["cp"]
        out.append((j, st, sums))
    return out


def gather_jobs():
    out = []
    for n, rows, dim, ld, ldo, MB, map_n in ((20, 31, 136, 144, 152, 0, 0), (20, 31, 136, 136, 136, 0, 50), (20, 31, 256, 264, 0, 2, 0), (33, 9, 128, 128, 0, 3, 12)):
        key = ("gather", n, dim, MB, map_n)
        table = sent((rows, ld), U16)
        table[:, :dim] = bf_noise(key, (rows, dim))
        r = rng_of(key)
        tmap = r.integers(0, rows, map_n).astype(np.int32) if map_n else None
        ids = r.integers(0, map_n or rows, n).astype(np.int32)
        o = sent(MB * 16 * dim, U16) if MB else sent((n, ldo), U16)
        j = job("gather_rows", {0: n, 1: rows, 2: ld, 3: dim, 4: ldo, 5: MB, 6: map_n}, {0: table, 1: ids, 2: tmap}, {0: o})
        e = o.copy()
        src = table[tmap[ids] if map_n else ids, :dim]
        if MB:
            tiled_store(e, np.arange(n), dim, MB, src)
        else:
            e[:, :dim] = src
        out.append((j, {0: e}, None))
    return out


def tile_jobs():
    rows, dim, ld, MB = 20, 256, 264, 2
    x = sent((rows, ld), U16)
    x[:, :dim] = bf_noise("tile", (rows, dim))
    t = sent(MB * 16 * dim, U16)
    e = t.copy()
    tiled_store(e, np.arange(rows), dim, MB, x[:, :dim])
    back = sent((rows, ld), U16)
    eb = back.copy()
    eb[:, :dim] = x[:, :dim]
    return [(job("tile_rows", {0: rows, 1: dim, 2: ld, 3: MB}, {0: x}, {0: t}), {0: e}, None),
            (job("untile_rows", {0: rows, 1: dim, 2: MB, 3: ld}, {0: e}, {0: back}), {0: eb}, None)]   # (of the tiled reference: the round trip)


def add_jobs():
    out = []
    rows, dim = 5, 100
    for lda, ldb, ldo in ((104, 0, 112), (100, 108, 100)):
        a, b = bf_noise(("add", "a", ldb), (rows, lda)), bf_noise(("add", "b", ldb), (rows, ldb) if ldb else dim)
        a[0, :4] = [0x3F80, 0x3F81, 0x7F80, 0xFF80]          # (1 | 1 + 2^-7) + 2^-8: ties, to even down and up; the infinities
        (b if ldb == 0 else b[0])[:4] = [0x3B80, 0x3B80, 0x3F80, 0x3F80]
        o = sent((rows, ldo), U16)
        e = o.copy()
        e[:, :dim] = f2b(b2f(a[:, :dim]) + b2f(b[:dim] if ldb == 0 else b[:, :dim]))
        out.append((job("add_rows", {0: rows, 1: dim, 2: lda, 3: ldb, 4: ldo}, {0: a, 1: b}, {0: o}), {0: e}, None))
    return out


def compose_jobs():
    n, dim, ldp, ldt, lde, ldd = 6, 72, 80, 72, 88, 96
    proj, table, extra = bf_noise("cproj", (7, ldp)), bf_noise("ctable", (5, ldt)), bf_noise("cextra", (3, lde))
    a, b, dst_row = i32([6, 0, 3, 3, 1, 2]), i32([-1, 4, -2, -4, 0, -1]), i32([2, 0, 7, 5, 1, 4])
    o = sent((9, ldd), U16)
    e = o.copy()
    for i in range(n):
        pa = b2f(proj[a[i], :dim])
        if b[i] == -1:
            e[dst_row[i], :dim] = proj[a[i], :dim]
        else:
            pb = table[b[i], :dim] if b[i] >= 0 else extra[-2 - b[i], :dim]
            e[dst_row[i], :dim] = f2b(pa + b2f(pb))
    p = {0: n, 1: dim, 2: 7, 3: ldp, 4: 5, 5: ldt, 6: 3, 7: lde, 8: 9, 9: ldd}
    j = job("compose_rows", p, {0: proj, 1: table, 2: extra, 3: a, 4: b, 5: dst_row}, {0: o})
    # without the extra table: rows of the first two kinds only
    keep = b >= -1
    p2 = dict(p)
    p2.update({0: int(keep.sum()), 6: 0, 7: 0})
    j2 = job("compose_rows", p2, {0: proj, 1: table, 3: a[keep], 4: b[keep], 5: dst_row[keep]}, {0: o})
    e2 = o.copy()
    e2[dst_row[keep]] = e[dst_row[keep]]
    return [(j, {0: e}, None), (j2, {0: e2}, None)]


def ref_embed_jobs():
    out = []
    for groups, ldo in ((1, 104), (16, 96), (16, 104)):
        T, H, Vt, Vcp = 5, 96, 11, 13
        pool, offs, tables, _ = table_pool(("ref_embed", groups), groups, H, Vt, Vcp)
        r = rng_of("ref_embed", groups, ldo)
        codes = np.concatenate([r.integers(0, Vt, (1, T)), r.integers(0, Vcp, (groups - 1, T))]).astype(np.int32)
        o = sent((T, ldo), U16)
        e = o.copy()
        for t in range(T):
            e[t, :H] = next_input(tables, codes[:, t], groups, np.zeros(H, U16))   # (+ 0: exact)
        out.append((job("ref_embed_rows", {0: T, 1: groups, 2: H, 3: ldo, 4: Vt, 5: Vcp}, {0: codes, 1: pool, 2: offs[:groups].copy()}, {0: o}), {0: e}, None))
    return out


def f32_to_bf16_jobs():
    out = []
    edge = np.array([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0xBF808000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0, 0x80000000], np.uint32).view(F32)
    for n in (1, 255, 256, 257):
        x = (rng_of("f2b", n).standard_normal(n) * 100).astype(F32)
        x[:min(n, edge.size)] = edge[:n] if n < edge.size else edge
        if n == 1:
            x[0] = edge[0]
        o = sent(n, U16)
        out.append((job("f32_to_bf16", {0: n}, {0: x}, {0: o}), {0: f2b(x)}, None))
    return out


def ss_to_table_jobs():
    rows, nss, ld = 7, 37, 9   # 259 elements: one more than a block, three in the second
    ss = rng_of("sstt").random((nss, ld)).astype(F32)
    o = sent((rows, nss), F32)
    return [(job("ss_to_table", {0: rows, 1: nss, 2: ld}, {0: ss}, {0: o}), {0: np.ascontiguousarray(ss[:, :rows].T)}, None)]


def copy_jobs():
    out = []
    for rows, dim, lds, ldd in ((1, 16 * 128, 0, 0), (3, 128, 136, 144), (3, 128, 0, 128)):   # the first: the engine's whole-buffer copy
        src = bf_noise(("copy", rows, lds), (rows - 1) * lds + dim)
        o = sent((rows - 1) * ldd + dim, U16)
        e = o.copy()
        for r in range(rows):
            e[r * ldd:r * ldd + dim] = src[r * lds:r * lds + dim]
        out.append((job("copy_rows", {0: rows, 1: dim, 2: lds, 3: ldd}, {0: src}, {0: o}), {0: e}, None))
    return out


def prefill_jobs():
    out = []
    B, Pmax, H, hMB = 5, 6, 256, 1
    prompt = bf_noise("prompt", (B, Pmax, H))
    n_prompt = i32([6, 3, 1, 0, 4])
    for step in (0, 3, 5):
        ios = {0: sent(hMB * 16 * H, U16), 1: sent(B, F32), 2: sent(B, np.uint8)}
        e, sums = copies(ios), {1: {}}
        for b in range(B):
            idx = step - (Pmax - int(n_prompt[b]))
            row = prompt[b, max(idx, 0)]   # a row that has not started loads its position 0 (and is not active)
            tiled_store(e[0], [b], H, hMB, row)
            e[2][b] = 1 if idx >= 0 else 0
            sums[1][b] = ss_bar(b2f(row).astype(np.float64), H)
        out.append((job("prefill_load", {0: B, 1: Pmax, 2: step, 3: H, 4: hMB}, {0: prompt, 1: n_prompt}, ios), e, sums))
    Pmax, hMB = 8, 2
    prompt = bf_noise("prompt-chunk", (B, Pmax, H))
    n_prompt = i32([8, 3, 1, 5, 2])
    for C, r_base in ((4, -5), (1, -2)):
        ios = {0: sent(hMB * 16 * H, U16), 1: sent(C * B, F32)}
        e, sums = copies(ios), {1: {}}
        for pp in range(C):
            for b in range(B):
                r, m = r_base + int(n_prompt[b]) + pp, pp * B + b
                row = prompt[b, r] if r >= 0 else np.zeros(H, U16)
                tiled_store(e[0], [m], H, hMB, row)
                sums[1][m] = ss_bar(b2f(row).astype(np.float64), H)
        out.append((job("prefill_chunk_load", {0: B, 1: Pmax, 2: r_base, 3: H, 4: hMB, 5: C}, {0: prompt, 1: n_prompt}, ios), e, sums))
    return out


def advance_jobs():
    out = []
    for B, given in ((1, False), (64, False), (64, True), (1, True)):
        kv = i32(10 + 3 * np.arange(B))
        act = u8((np.arange(B) % 3) != 1) if given else None
        e = kv + (act if given else 1)
        out.append((job("advance_len", {0: B}, {0: act}, {0: kv}), {0: e.astype(np.int32)}, None))
    B, C, r_base = 5, 4, -6
    n_prompt = i32([1, 3, 6, 8, 2])   # r0 = -5 (below -C), -3 (inside), 0, 2, -4 (= -C)
    r0 = r_base + n_prompt
    p0 = np.where(r0 < 0, np.minimum(-r0, C), 0)
    kv = i32([7, 8, 9, 10, 11])
    out.append((job("advance_len_chunk", {0: B, 1: r_base, 2: C}, {0: n_prompt}, {0: kv}), {0: (kv + C - p0).astype(np.int32)}, None))
    return out


def admit_jobs():
    out = []
    k, slots, H, V, Fmax, srcMB, hMB = 3, 6, 128, 50, 3, 1, 1
    for with_text in (False, True):
        r = rng_of("admit", with_text)
        desc = np.zeros(k, ADMIT)
        for jn, s in enumerate((4, -1, 1)):
            desc[jn] = (s, 5 + jn, 40 + jn, 9000 + jn, jn % 2 if with_text else 0, 0, (0.5 + jn, 10 + jn, 0.9, 1.05, 1234567890123 + jn, 3, jn % 2))
        src_h = bf_noise(("admit-h", with_text), srcMB * 16 * H)
        src_ss, src_kv, src_np = r.random(k).astype(F32), i32([21, 22, 23]), i32([31, 32, 33])
        noise = lambda dt, shape: r.integers(1, 100, shape).astype(dt)
        ios = {0: bf_noise("admit-dst", hMB * 16 * H), 1: r.random(slots).astype(F32)}
        for s in range(2, 9):
            ios[s] = noise(np.int32, slots)
        ios.update({9: noise(np.int32, (slots, 16)), 10: noise(np.int32, (slots, Fmax, 16)), 11: noise(np.uint32, slots), 13: u8([1] * slots), 14: u8([0] * slots),
                    15: noise(np.uint8, (slots, V))})
        sp = np.zeros(slots, SP)
        sp["seed"], sp["top_k"] = 99, 7
        ios[12] = sp
        if with_text:
            ios[16], ios[17] = u8([3] * slots), u8([1] * slots)
        e = copies(ios)
        for jn in range(k):
            s = int(desc[jn]["slot"])
            if s < 0:
                continue
            e[0][tiled_index([s], H, hMB)[0]] = src_h[tiled_index([jn], H, srcMB)[0]]
            e[1][s], e[2][s], e[3][s] = src_ss[jn], src_kv[jn], src_np[jn]
            e[4][s], e[5][s], e[6][s], e[7][s], e[8][s] = desc[jn]["n_trailing"], desc[jn]["max_frames"], 0, 0, 0
            e[9][s], e[10][s], e[11][s], e[12][s] = 0, 0, desc[jn]["row_key"], desc[jn]["sp"]
            e[13][s], e[14][s], e[15][s] = 0, 1, 0
            if with_text:
                e[16][s], e[17][s] = 1 if desc[jn]["text_open"] else 0, 0
        out.append((job("admit_rows", {0: k, 1: slots, 2: H, 3: V, 4: Fmax, 5: srcMB, 6: hMB}, {0: desc, 1: src_h, 2: src_ss, 3: src_kv, 4: src_np}, ios), e, None))
    return out


def text_append_jobs():
    slots, H, Tmax, groups, hMB, Vt, Vcp, src_rows = 7, 128, 4, 16, 1, 24, 40, 6
    key = "text_append"
    pool, offs, tables, pad = table_pool(key, groups, H, Vt, Vcp)
    src, eos_row = bf_noise((key, "src"), (src_rows, H)), bf_noise((key, "eos"), H)
    cur = rng_of(key, "cur").integers(0, Vt, (slots, 16)).astype(np.int32)
    # slot 0 append | 1 close | 2 starved, resumes on the EOS row (n_new 0, close) | 3 does not fit | 4 starved, resumes on a source row | 5, 6 not listed
    desc = np.zeros(5, TEXT)
    for n, d in enumerate(((0, 0, 2, 0, 0, 0), (1, 2, 1, 1, 77, 0), (2, 0, 0, 1, 88, 0), (3, 3, 2, 0, 0, 0), (4, 4, 2, 0, 0, 0))):
        desc[n] = d
    ios = {0: bf_noise((key, "trailing"), (slots, Tmax, H)), 1: i32([1, 2, 2, 3, 1, 2, 0]), 2: u8([1] * slots), 3: i32([1000 + s for s in range(slots)]),
           4: i32([0, 1, 2, 3, 1, 2, 0]), 5: sent(hMB * 16 * H, U16), 6: sent(slots, F32), 7: i32([15] * slots), 8: u8([0, 0, 1, 1, 1, 1, 0]),
           9: u8([0, 0, 1, 1, 1, 1, 0]), 10: u8([1, 1, 0, 0, 0, 0, 1])}
    e, sums = copies(ios), {6: {}}
    for d in desc:
        s, nt = int(d["slot"]), int(ios[1][d["slot"]])
        add = int(d["n_new"]) + int(d["close"])
        if nt + add > Tmax:
            continue
        for r in range(add):
            e[0][s, nt + r] = src[d["src_row"] + r] if r < d["n_new"] else eos_row
        ti = int(ios[4][s])
        resume = ios[8][s] != 0 and add > 0 and ti == nt
        e[1][s] = nt + add
        if d["close"]:
            e[2][s], e[3][s] = 0, d["max_frames"]
        if resume:
            row = next_input(tables, cur[s], groups, src[d["src_row"]] if d["n_new"] > 0 else eos_row)
            tiled_store(e[5], [s], H, hMB, row)
            sums[6][s] = ss_bar(b2f(row).astype(np.float64), H)
            e[4][s], e[7][s], e[8][s], e[9][s], e[10][s] = ti + 1, 0, 0, 0, 1
    assert sorted(sums[6]) == [2, 4]
    p = {0: len(desc), 1: slots, 2: H, 3: Tmax, 4: groups, 5: hMB, 6: Vt, 7: Vcp, 8: src_rows}
    return [(job("text_append_rows", p, {0: desc, 1: src, 2: eos_row, 3: pool, 4: offs, 5: cur}, ios), e, sums)]


def cancel_jobs():
    out = []
    for slots, mask in ((64, (1 << 63) | 1), (10, (1 << 63) | (1 << 10) | (1 << 9) | 4), (64, 0), (1, 0xFFFFFFFFFFFFFFFF)):
        fin, act = u8([0] * 64), u8([1] * 64)
        ef, ea = fin.copy(), act.copy()
        for s in range(slots):
            if (mask >> s) & 1:
                ef[s], ea[s] = 1, 0
        lo, hi = mask & 0xFFFFFFFF, mask >> 32
        signed = lambda v: v - (1 << 32) if v >= (1 << 31) else v
        out.append((job("cancel_rows", {0: slots, 1: signed(lo), 2: signed(hi), 3: 64}, {}, {0: fin, 1: act}), {0: ef, 1: ea}, None))
    return out


OPS = {"frame_end": frame_end_jobs, "gather_rows": gather_jobs, "tile_untile_rows": tile_jobs, "add_rows": add_jobs, "compose_rows": compose_jobs,
       "ref_embed_rows": ref_embed_jobs, "f32_to_bf16": f32_to_bf16_jobs, "ss_to_table": ss_to_table_jobs, "copy_rows": copy_jobs,
       "prefill_loads": prefill_jobs, "advance_lens": advance_jobs, "admit_rows": admit_jobs, "text_append_rows": text_append_jobs,
       "cancel_rows": cancel_jobs}


@functools.lru_cache(maxsize=None)
def jobs_of(name):
    return OPS[name]()


# ---------------------------------------------------------------------------------------------
# CPU part
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(OPS))
def test_every_case_is_launchable(name):
    for j, exp, _ in jobs_of(name):
        assert check_only(j) == 0, (name, j["p"])
        assert set(exp) == {s for s, v in j["ios"].items() if v is not None}


def test_case_tables_reach_every_op():
    from qwen3tts import _lib
    reached = {j["op"] for name in OPS for j, _, _ in jobs_of(name)}
    assert reached == set(_lib.LMOPS[2:])   # (ops 0 and 1: test_sampler_block.py)


def test_restatements_agree_with_themselves():
    """The layout function is a bijection of a buffer; the bf16 chain of next_input equals the chain written out in float64 with a
    rounding per add (a bf16 sum of two bf16 values is exact in float64); a job's expectation never touches a sentinel it should
    not: the expected frame_end input rows cover exactly the rows that form an input."""
    layout_is_a_bijection()
    tables = [bf_noise(("self", g), (4, 64)) for g in range(16)]
    codes, text = [g % 4 for g in range(16)], bf_noise("self-text", 64)
    acc = b2f(tables[0][0]).astype(np.float64)
    for g in range(1, 16):
        acc = rbf((acc + b2f(tables[g][codes[g]]).astype(np.float64)).astype(np.float32)).astype(np.float64)
    want = f2b((b2f(text).astype(np.float64) + acc).astype(np.float32))
    assert np.array_equal(next_input(tables, codes, 16, text), want)
    for j, exp, sums in jobs_of("frame_end"):
        B, H, hMB = j["p"][0], j["p"][20], j["p"][23]
        written = np.zeros(hMB * 16 * H, bool)
        written[tiled_index(sorted(sums[13]), H, hMB).ravel()] = True
        assert np.array_equal(exp[12] != j["ios"][12], written)
        fin = j["ios"][1] != 0
        assert not set(np.flatnonzero(fin)) & set(sums[13]) and (exp[14] == 0).all()


def _by_op(op, n=0):
    return [j for name in OPS for j, _, _ in jobs_of(name) if j["op"] == op][n]


REFUSED = {
    "unknown-op": None,
    "parameter-out-of-range": lambda: mutate(_by_op("f32_to_bf16"), p={9: 1 << 25}),
    "buffer-size": lambda: mutate(_by_op("f32_to_bf16", 1), p={0: 254}),
    "unnamed-slot": lambda: mutate(_by_op("ss_to_table"), ins={3: np.zeros(4, F32)}),
    "null-argument": lambda: mutate(_by_op("add_rows"), ins={1: None}),
    "gather-dim-mod8": lambda: mutate(_by_op("gather_rows"), p={3: 132}),
    "gather-id-outside": lambda: mutate(_by_op("gather_rows"), ins={1: _by_op("gather_rows")["ins"][1] + 31}),
    "gather-token-map-outside": lambda: mutate(_by_op("gather_rows", 1), ins={2: _by_op("gather_rows", 1)["ins"][2] + 31}),
    "gather-tiled-dim-mod128": lambda: mutate(_by_op("gather_rows", 2), p={3: 136}),
    "gather-rows-over-MB": lambda: mutate(_by_op("gather_rows", 2), p={5: 1}, ios={0: sent(16 * 256, U16)}),
    "tile-ld-below-dim": lambda: mutate(_by_op("tile_rows"), p={2: 248}, ins={0: sent((20, 248), U16)}),
    "add-ldb-below-dim": lambda: mutate(_by_op("add_rows", 1), p={3: 96}, ins={1: sent((5, 96), U16)}),
    "compose-a-outside": lambda: mutate(_by_op("compose_rows"), ins={3: i32([7, 0, 3, 3, 1, 2])}),
    "compose-b-outside-extra": lambda: mutate(_by_op("compose_rows"), ins={4: i32([-1, 4, -2, -5, 0, -1])}),
    "compose-b-without-extra": lambda: mutate(_by_op("compose_rows", 1), ins={4: i32([-1, 4, -2, -1])}),
    "compose-dst-twice": lambda: mutate(_by_op("compose_rows"), ins={5: i32([2, 0, 7, 2, 1, 4])}),
    "ref-embed-code-outside": lambda: mutate(_by_op("ref_embed_rows", 1), ins={0: _by_op("ref_embed_rows", 1)["ins"][0] + 12}),
    "ss-ld-below-rows": lambda: mutate(_by_op("ss_to_table"), p={2: 6}, ins={0: np.zeros((37, 6), F32)}),
    "copy-ldd-0-two-rows": lambda: mutate(_by_op("copy_rows", 2), p={3: 0}, ios={0: sent(128, U16)}),
    "prefill-position-at-Pmax": lambda: mutate(_by_op("prefill_load"), p={2: 6}),
    "prefill-n-prompt-over-Pmax": lambda: mutate(_by_op("prefill_load"), ins={1: i32([7, 3, 1, 0, 4])}),
    "prefill-chunk-rows-over-MB": lambda: mutate(_by_op("prefill_chunk_load"), p={4: 1}, ios={0: sent(16 * 256, U16)}),
    "prefill-chunk-position-at-Pmax": lambda: mutate(_by_op("prefill_chunk_load"), p={2: -3}),
    "advance-B-65": lambda: mutate(_by_op("advance_len", 1), p={0: 65}, ios={0: i32([0] * 65)}),
    "admit-slot-outside": lambda: _admit_slot(6),
    "admit-slot-twice": lambda: _admit_slot(4, at=2),
    "admit-H-mod128": lambda: mutate(_by_op("admit_rows"), p={2: 120}),
    "text-slot-twice": lambda: _text_desc(1, slot=0),
    "text-src-rows": lambda: _text_desc(4, src_row=5),
    "text-n-new-over-Tmax": lambda: _text_desc(0, n_new=5, src_row=0),
    "text-n-trailing-over-Tmax": lambda: mutate(_by_op("text_append_rows"), ios={1: i32([1, 2, 2, 5, 1, 2, 0])}),
    "text-cur-code-outside": lambda: mutate(_by_op("text_append_rows"), ins={5: _by_op("text_append_rows")["ins"][5] + 24}),
    "cancel-slots-65": lambda: mutate(_by_op("cancel_rows"), p={0: 65}),
    "cancel-n-below-slots": lambda: mutate(_by_op("cancel_rows"), p={3: 32}, ios={0: u8([0] * 32), 1: u8([1] * 32)}),
    "frame-end-H-mod128": lambda: mutate(_by_op("frame_end"), p={20: 120}),
    "frame-end-trailing-idx-negative": lambda: mutate(_by_op("frame_end"), ios={11: i32([-1] * 17)}),
}


def _admit_slot(slot, at=0):
    j = _by_op("admit_rows")
    d = j["ins"][0].copy()
    d[at]["slot"] = slot
    return mutate(j, ins={0: d})


def _text_desc(at, **kw):
    j = _by_op("text_append_rows")
    d = j["ins"][0].copy()
    for k, v in kw.items():
        d[at][k] = v
    return mutate(j, ins={0: d})


@pytest.mark.parametrize("name", list(REFUSED))
def test_host_refusals(name):
    """Every refusal precedes allocation: check_only with m == NULL returns INVALID_INPUT (the jobs they are made from are accepted:
    test_every_case_is_launchable)."""
    from qwen3tts import _lib
    if REFUSED[name] is None:
        a = _lib.LmopDebug(op=19, check_only=1)
        assert _lib.lib().q3tts_debug_lmop(None, a) == 3
        return
    assert check_only(REFUSED[name]()) == 3, name


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
@pytest.mark.parametrize("name", list(OPS))
def test_lmrow_block_matches_its_reference(engine, name):
    """Every job of the op: one launch of the product's launcher, every returned buffer whole against the restatement."""
    WORST.pop(name, None)
    for n, (j, exp, sums) in enumerate(jobs_of(name)):
        compare("%s:%s-%d" % (name, j["op"], n), launch(engine, j), exp, sums)
    print("GPU, worst error / bar: %s %.4f" % (name, WORST.get(name, 0.0)))


@pytest.mark.gpu
def test_tile_untile_round_trip(engine):
    (jt, et, _), (ju, eu, _) = jobs_of("tile_untile_rows")
    t = launch(engine, jt)[0]
    back = launch(engine, mutate(ju, ins={0: t}))[0]
    assert np.array_equal(back[:, :256], jt["ins"][0][:, :256])


@pytest.mark.gpu
def test_refused_arguments_launch_nothing(engine):
    """With a live model: a refused call (status 3) raises, and a good call afterwards works."""
    from qwen3tts import Qwen3TTSError
    with pytest.raises(Qwen3TTSError) as e:
        launch(engine, REFUSED["gather-id-outside"]())
    assert e.value.status == 3
    j, exp, sums = jobs_of("gather_rows")[0]
    compare("gather_rows:after-refusal", launch(engine, j), exp, sums)
