"""What tests/test_sampler_block.py and tests/test_lmrow_block.py share: the records and layouts of q3tts_debug_lmop
(include/q3tts.h) restated in numpy, sentinels, the bf16 arithmetic of the kernels, the end-of-frame job's reference and the
comparison of a launch's returned buffers with what a reference expects. No test lives here."""
import zlib

import numpy as np

E = 2.0 ** -24                      # half an fp32 step
SENT32 = 0x7FC12345                 # a NaN pattern no kernel produces
SENT16 = 0x7FC5                     # the same for bf16
SENT_I = -777                       # for integers that are never used as an index
SENT_U8 = 0xA5
F32 = np.float32
WORST = {}                          # name -> worst error / bar of a sum of squares seen in this process

# csrc/kernels.h SamplingParams, AdmitDesc, TextAppendDesc as they lie in memory (tests/test_abi.py holds the C layout to these)
SP = np.dtype([("temperature", "<f4"), ("top_k", "<i4"), ("top_p", "<f4"), ("rep_penalty", "<f4"), ("seed", "<u8"), ("row0", "<u4"),
               ("mask_eos", "<i4")], align=True)
ADMIT = np.dtype([("slot", "<i4"), ("n_trailing", "<i4"), ("max_frames", "<i4"), ("row_key", "<u4"), ("text_open", "<i4"), ("pad_", "<i4"),
                  ("sp", SP)], align=True)
TEXT = np.dtype([("slot", "<i4"), ("src_row", "<i4"), ("n_new", "<i4"), ("close", "<i4"), ("max_frames", "<i4"), ("pad_", "<i4")])
assert SP.itemsize == 32 and ADMIT.itemsize == 56 and TEXT.itemsize == 24


def rng_of(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def sp_rows(rows):
    """[(temperature, top_k, top_p, rep_penalty, seed, row0, mask_eos), ...] -> SamplingParams [B]"""
    a = np.zeros(len(rows), SP)
    for i, r in enumerate(rows):
        a[i] = r
    return a


# ---- bf16 ---------------------------------------------------------------------------------------
def f2b(x):
    """fp32 -> bf16 bits, round to nearest even (finite values and infinities; a NaN stays a NaN)"""
    b = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(np.asarray(x, F32))
    return np.where(nan, np.uint16(0x7FC0), r).astype(np.uint16)


def b2f(b):
    return (np.asarray(b, np.uint16).astype(np.uint32) << 16).view(F32)


def rbf(x):
    return b2f(f2b(x))


def bf_noise(key, shape, scale=1.0):
    return f2b(rng_of("bf", key).standard_normal(shape).astype(F32) * F32(scale))


# ---- sentinels ----------------------------------------------------------------------------------
def sent(shape, dtype):
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        a = np.empty(shape, np.uint32)
        a[...] = SENT32
        return a.view(F32)
    fill = {np.dtype(np.uint16): SENT16, np.dtype(np.int32): SENT_I, np.dtype(np.uint8): SENT_U8, np.dtype(np.uint32): 0xDEADBEEF}[dtype]
    return np.full(shape, fill, dtype)


def raw(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(-1)


# ---- the fragment-major activation layout (csrc/common.h act_tiled_offset) ---------------------
def tiled_offset(m, k, MB):
    m, k = np.asarray(m, np.int64), np.asarray(k, np.int64)
    return ((((k >> 7) * MB + (m >> 4)) * 4 + ((k >> 3) & 3)) * 64 + (((k >> 5) & 3) * 16 + (m & 15))) * 8 + (k & 7)


def tiled_index(rows, H, MB):
    """[len(rows)][H] element offsets of these rows"""
    return tiled_offset(np.asarray(rows)[:, None], np.arange(H)[None, :], MB)


def layout_is_a_bijection():
    for MB, H in ((1, 128), (3, 256)):
        idx = tiled_index(np.arange(MB * 16), H, MB).ravel()
        assert np.array_equal(np.sort(idx), np.arange(MB * 16 * H))


# ---- one call -----------------------------------------------------------------------------------
def job(op, p, ins=None, ios=None, **meta):
    return dict(op=op, p=dict(p), ins=dict(ins or {}), ios=dict(ios or {}), **meta)


def check_only(j):
    from qwen3tts import _lib
    ios = {i: (None if v is None else np.ascontiguousarray(v).copy()) for i, v in j["ios"].items()}
    ins = {i: (None if v is None else np.ascontiguousarray(v)) for i, v in j["ins"].items()}
    return _lib.lmop(None, j["op"], j["p"], ins, ios, check_only=True)


def launch(engine, j):
    return engine.debug_lmop(j["op"], j["p"], j["ins"], j["ios"])


def mutate(j, p=None, ins=None, ios=None):
    k = dict(j, p=dict(j["p"]), ins=dict(j["ins"]), ios=dict(j["ios"]))
    k["p"].update(p or {})
    k["ins"].update(ins or {})
    k["ios"].update(ios or {})
    return k


# ---- comparison ---------------------------------------------------------------------------------
def ss_bar(x64, H):
    """fp32 sum of the squares of H bf16 values in any order: the squares are exact (8-bit significands), each of the H - 1
    additions rounds once, so the result lies within (H - 1) e of the sum; the bar of DESIGN.md section 2 is (H + 1) e sum x^2."""
    s = float((x64 * x64).sum())
    return s, (H + 1) * E * s


def compare(name, got, exp, sums=None):
    """got / exp: {slot: array}. Every slot equal on raw bytes, except the float32 entries listed in sums: {slot: {index: (ref,
    bar)}}, which lie within their bar of the float64 reference -- and every other entry of those slots keeps its bits."""
    sums = sums or {}
    assert set(got) == set(exp), (name, sorted(got), sorted(exp))
    for s in sorted(exp):
        g, e = np.ascontiguousarray(got[s]), np.ascontiguousarray(exp[s])
        assert g.shape == e.shape and g.dtype == e.dtype, "%s: slot %d comes back as %s %s" % (name, s, g.dtype, g.shape)
        if s in sums:
            g, e = g.copy().reshape(-1), e.copy().reshape(-1)
            for i, (ref, bar) in sums[s].items():
                v = float(g[i])
                assert np.isfinite(v), "%s: slot %d[%d] is not finite" % (name, s, i)
                err = abs(v - ref)
                assert err <= bar, "%s: slot %d[%d] leaves its bar: error %.4g, bar %.4g" % (name, s, i, err, bar)
                if bar > 0:
                    WORST[name.split(":")[0]] = max(WORST.get(name.split(":")[0], 0.0), err / bar)
                g[i] = e[i] = 0
        a, b = raw(g), raw(e)
        if not np.array_equal(a, b):
            i = np.flatnonzero(a != b)
            w = i[0] // g.dtype.itemsize
            raise AssertionError("%s: slot %d: %d bytes differ, the first in element %d: got %r, expected %r"
                                 % (name, s, i.size, w, g.reshape(-1)[w], e.reshape(-1)[w]))


# ---- the end-of-frame job (row_jobs.h next_input_row, frame_end_job; lm_misc.hip frame_end_kernel) -----------------------------
def next_input(tables, codes, groups, text):
    """text + (codec_emb[c0] + cp_emb[0][c1] + ...), left to right, every add rounded to bf16. tables: [groups] arrays of bf16
    bits [V][H]; returns bf16 bits [H]."""
    acc = b2f(tables[0][codes[0]])
    for g in range(1, groups):
        acc = rbf(acc + b2f(tables[g][codes[g]]))
    return f2b(b2f(text) + acc)


def frame_end_ref(c, st, sums, h_slot=12, ss_slot=13, entry_finished=None):
    """c: tables, tts_pad, trailing, n_trailing, max_frames, text_open (or None), groups, hMB, H. st: {slot: array}, updated in
    place: 0 n_frames, 1 finished, 2 active, 4 cur_codes, 11 trailing_idx, 12 h, 13 ss_out, `cp` cp_len, 15 starved."""
    B, H = st[0].shape[0], c["H"]
    fin0 = st[1].copy() if entry_finished is None else entry_finished
    hflat = st[h_slot].reshape(-1)
    for b in range(B):
        if fin0[b]:
            st["cp"][b] = 0
            continue
        ti = int(st[11][b])
        has_text = ti < c["n_trailing"][b]
        starve = (not has_text) and c["text_open"] is not None and c["text_open"][b] != 0
        if not starve:
            text = c["trailing"][b, ti] if has_text else c["tts_pad"]
            row = next_input(c["tables"], st[4][b], c["groups"], text)
            hflat[tiled_index([b], H, c["hMB"])[0]] = row
            sums.setdefault(ss_slot, {})[b] = ss_bar(b2f(row).astype(np.float64), H)
        if has_text:
            st[11][b] = ti + 1
        nf = int(st[0][b]) + 1
        st[0][b] = nf
        if nf >= c["max_frames"][b]:
            st[1][b], st[2][b] = 1, 0
        elif starve:
            st[1][b], st[2][b], st[15][b] = 1, 0, 1
        st["cp"][b] = 0


def table_pool(key, groups, H, Vt, Vcp, gap=8):
    """codec_emb [Vt][H], cp_emb [groups - 1][Vcp][H] and tts_pad [H] in one pool of bf16, in reverse order with gaps of sentinel.
    Returns pool, offsets i64 [groups + 1], tables (views by group), tts_pad."""
    sizes = [Vt * H] + [Vcp * H] * (groups - 1) + [H]
    offs, at = [0] * len(sizes), gap
    for g in reversed(range(len(sizes))):
        offs[g] = at
        at += sizes[g] + gap
    pool = sent(at, np.uint16)
    tables = []
    for g in range(groups):
        t = bf_noise((key, "table", g), (Vt if g == 0 else Vcp, H))
        pool[offs[g]:offs[g] + t.size] = t.ravel()
        tables.append(t)
    pad = bf_noise((key, "pad"), H)
    pool[offs[groups]:offs[groups] + H] = pad
    return pool, np.array(offs, np.int64), tables, pad
