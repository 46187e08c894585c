"""Block-level parity of the decode attention (csrc/kernels/attn_decode.hip, attn_body.inc) through q3tts_debug_attention:
one launch of the product's own launch_attn_decode per case, on caller-built buffers, against a float64 reference written here.

Per case three things are compared:
  V appended   bit-exact, and every pool slot that is not a live new position keeps its sentinel (a NaN pattern) bit for bit:
               inactive rows, padded chunk elements, other rows' pages, pages behind the block table.
  K appended   equal or adjacent bf16 values (the wave reduction's order of sum(x^2) can move rstd by an fp32 ulp), fewer than
               2 % of the elements differing.
  out          against float64 softmax(scale q.k) V over the cache contents the kernel itself left (read back), bar
               |a - r| <= 2^-7 * max(|r|, 2^-10 * max|V| of that head's keys): one bf16 ulp of the element.

The CPU part (no marker) runs the same case generator and reference against a float32 restatement of the kernels' walk (16 or 32
lane groups striding over the positions, per-group online softmax, log-sum-exp merge, one bf16 rounding) for the whole matrix,
so the inputs are known to stay inside the bar without the kernel.

Instantiations launch_attn_decode can dispatch, and the case that runs each (rep = n_heads / n_kv; wide = max_pages > 1 and
rep <= 2; the chunk kernels take CMAX 8 for chunk <= 8 and 16 above):
  attn_decode_kernel<1,256>        one-2x2-p1-*        attn_decode_kernel<1,512>        one-2x2-p4-*
  attn_decode_kernel<2,256>        one-4x2-p1-*, one-16x8-p1-*, one-4x2-p1-nt (nt_kv is ignored when not wide)
  attn_decode_kernel<2,512>        one-4x2-p4-*, one-16x8-p4-*       attn_decode_kernel<2,512,NT>  one-4x2-p4-nt, one-16x8-p4-nt
  attn_decode_kernel<3,256>        one-3x1-p1-*, one-3x1-p4-*        attn_decode_kernel<4,256>     one-4x1-*, one-8x2-*
  attn_chunk_kernel<1,256,8|16>    chunk-2x2-p1-c{2,4,8 | 9,16}      attn_chunk_kernel<1,512,8|16>  chunk-2x2-p4-c*
  attn_chunk_kernel<2,256,8|16>    chunk-4x2-p1-c*, chunk-16x8-p1-c* attn_chunk_kernel<2,512,8|16>  chunk-4x2-p4-c*, chunk-16x8-p4-c*
  attn_chunk_kernel<3,256,8|16>    chunk-3x1-p{1,4}-c*               attn_chunk_kernel<4,256,8|16>  chunk-4x1-p{1,4}-c*, chunk-8x2-p{1,4}-c*
  code-predictor form (fixed_len, identity_pages): cp-*, and cp-*-c2 for the two-position step 0."""
import zlib

import numpy as np
import pytest

from conftest import bf16_to_f32

PAGE, D = 64, 128
ULP = 2.0 ** -7
SENT = 0x7FC1  # a NaN: a slot that must not be read poisons `out`, a slot that must not be written keeps these bits
N_POS = 272
EPS = 1e-6
SCALE = float(np.float32(128.0 ** -0.5))
SHAPES = [(2, 2), (4, 2), (16, 8), (3, 1), (4, 1), (8, 2)]


def f2b(x):
    from qwen3tts import synth
    return synth.f32_to_bf16_bits(np.ascontiguousarray(x, np.float32))


def rb(x):
    return bf16_to_f32(f2b(x))


def rope_tables():
    inv = 1e6 ** (-np.arange(64, dtype=np.float64) / 64.0)
    ang = np.arange(N_POS, dtype=np.float64)[:, None] * inv[None, :]
    ang = np.concatenate([ang, ang], -1)
    return f2b(np.cos(ang)), f2b(np.sin(ang))


def norm_rope(x_bits, w_bits, cos_bits, sin_bits):
    """Per-head RMSNorm + RoPE at the oracle's rounding points: n = bf16(x*rstd), y = bf16(n*w), bf16(bf16(y*cos) +
    bf16(rot*sin)), fp32 in between as in attn_body.inc / q3tts_oracle.c (sum(x^2) itself in float64). [..., 128] bits."""
    x, w = bf16_to_f32(x_bits), bf16_to_f32(w_bits)
    c, s = bf16_to_f32(cos_bits), bf16_to_f32(sin_bits)
    ss = (x.astype(np.float64) ** 2).sum(-1, keepdims=True).astype(np.float32)
    rstd = np.float32(1.0) / np.sqrt(ss / np.float32(D) + np.float32(EPS))
    y = rb(rb(x * rstd) * w)
    rot = np.concatenate([-y[..., 64:], y[..., :64]], -1)
    return f2b(rb(y * c) + rb(rot * s))


# ---------------------------------------------------------------------------------------------
# the case matrix
# ---------------------------------------------------------------------------------------------
# (cache length, score profile) of a row. Peaks sit on the edge position under test: a peaked row hides every other key.
PLAN_P4 = [(63, "peak_last"), (64, "peak_last"), (65, "peak_last"), (63, "peak_new"), (64, "peak_new"), (65, "peak_new"),
           (65, "peak63"), (65, "peak64"), (128, "peak64"), (200, "peak_last"), (0, "peak_new"), (0, "uniform"), (1, "peak0"),
           (127, "peak_new"), (128, "peak_last"), (200, "ramp"), (127, "equal"), (200, "uniform"), (15, "peak_new"),
           (16, "peak_last"), (31, "peak_new"), (32, "peak_last"), (200, "peak0"), (128, "peak63"), (65, "ramp"), (127, "uniform"),
           (64, "peak63"), (32, "equal"), (1, "peak_new"), (200, "peak_new"), (31, "uniform"), (15, "ramp"), (128, "peak_new")]
PLAN_P1 = [(63, "peak_last"), (63, "peak_new"), (0, "peak_new"), (0, "uniform"), (1, "peak0"), (1, "peak_last"), (15, "peak_new"),
           (16, "peak_new"), (16, "peak_last"), (31, "peak_new"), (31, "peak_last"), (32, "peak0"), (32, "ramp"), (63, "ramp"),
           (15, "equal"), (63, "equal"), (31, "uniform"), (32, "peak_new"), (63, "peak0"), (1, "peak_new"), (15, "peak_last"),
           (16, "uniform"), (63, "uniform"), (32, "peak_last"), (1, "equal"), (15, "peak0"), (16, "ramp"), (31, "equal"),
           (0, "equal"), (63, "peak_new"), (32, "uniform"), (31, "ramp"), (16, "peak0")]
CHUNK_PROFILES = ["peak_new", "uniform", "peak_last", "peak0", "ramp", "equal", "peak63", "peak64"]


def _specs():
    out = []
    k = 0
    batches = [1, 3, 17, 33]
    for (nh, nkv) in SHAPES:
        for mp in (1, 4):
            for nt in ((0, 1) if (nh, nkv) in ((16, 8), (4, 2)) else (0,)):
                for gain in ("lo", "hi"):
                    B = batches[k % 4]
                    if nkv == 8 and B > 3:  # keep the pools small: the 8-kv-head shape takes the small batches
                        B = 3 if B == 17 else 1
                    plan = PLAN_P4 if mp > 1 else PLAN_P1
                    rows = [plan[(b + 5 * k) % len(plan)] for b in range(B)]
                    act = None
                    if B >= 3 and k % 2 == 0:
                        act = [0 if b % 4 == 1 else 1 for b in range(B)]
                    out.append(dict(name="one-%dx%d-p%d-%s%s-b%d" % (nh, nkv, mp, "nt" if nt else "pl", gain, B), n_heads=nh, n_kv=nkv, B=B,
                                    max_pages=mp, nt_kv=nt, chunk=0, rows=rows, gain=gain, active=act))
                    k += 1
    # the code predictor's form: the cache length is a launch constant and row b owns page b
    for i, ((nh, nkv), fl, B) in enumerate([((4, 2), 0, 3), ((4, 2), 16, 17), ((16, 8), 7, 3), ((3, 1), 1, 1), ((4, 1), 15, 17),
                                            ((2, 2), 16, 3), ((8, 2), 2, 33)]):
        prof = ["peak_new", "peak_last", "uniform", "peak0", "ramp", "equal"]
        out.append(dict(name="cp-%dx%d-f%d-b%d" % (nh, nkv, fl, B), n_heads=nh, n_kv=nkv, B=B, max_pages=1, nt_kv=0, chunk=0,
                        rows=[(fl, prof[(b + i) % 6]) for b in range(B)], gain="hi" if i % 2 else "lo", active=None, fixed_len=fl))
    for i, ((nh, nkv), B) in enumerate([((4, 2), 3), ((16, 8), 1), ((4, 1), 17)]):  # step 0: [hidden, embed(code0)] together
        out.append(dict(name="cp-%dx%d-c2-b%d" % (nh, nkv, B), n_heads=nh, n_kv=nkv, B=B, max_pages=1, nt_kv=0, chunk=2,
                        rows=[(0, ["peak_new", "uniform", "peak0"][(b + i) % 3]) for b in range(B)], gain="hi" if i % 2 else "lo",
                        active=None, fixed_len=0))
    # chunks: every (rep, wide) with CMAX 8 and 16; right-aligned prompts with a padding of 0, 1, C-1 and C in one launch
    small, big = [2, 4, 8], [9, 16]
    j = 0
    for (nh, nkv) in SHAPES:
        for mp in (1, 4):
            for k, (C, aligned, gain) in enumerate([(small[j % 3], j % 3 != 1, "hi" if j % 4 >= 2 else "lo"),
                                                    (big[(j // 2 + j) % 2], j % 3 != 2, "hi" if j % 4 in (1, 2) else "lo")]):
                B = 5 if aligned else [1, 3, 17][(j + k) % 3]
                if nkv == 8 and B > 5:
                    B = 3
                if mp > 1:  # the chunk straddles position 64 or 128, or starts exactly on it
                    lens = [64 - C // 2, 128 - 1, 64, 128 - C + 1, 63, 0, 65, 127 - C // 2]
                else:
                    lens = [0, 64 - C, 1, 17, 31, 64 - C - 1, 16, 33]
                rows = [(lens[(b + j) % 8], CHUNK_PROFILES[(b + 3 * j + k) % 8]) for b in range(B)]
                pad = [[0, 1, C - 1, C, C // 2][b] for b in range(B)] if aligned else None
                out.append(dict(name="chunk-%dx%d-p%d-c%d-%s-b%d" % (nh, nkv, mp, C, "ra" if aligned else "all", B), n_heads=nh, n_kv=nkv,
                                B=B, max_pages=mp, nt_kv=0, chunk=C, rows=rows, gain=gain, active=None, pad=pad))
            j += 1
    return out


SPECS = _specs()
SPEC_IDS = [s["name"] for s in SPECS]
CHUNK_SPECS = [s for s in SPECS if s["chunk"] > 1]


class Case:
    pass


def make_case(spec):
    """Buffers of one launch: qkv rows, norm gains, pools with the rows' histories (everything else SENT), block table;
    the reference's own q / k / v of every live element and the pools it expects afterwards."""
    c = Case()
    c.spec = spec
    rng = np.random.default_rng(zlib.crc32(spec["name"].encode()))
    nh, nkv, B, mp = spec["n_heads"], spec["n_kv"], spec["B"], spec["max_pages"]
    rep = nh // nkv
    C = max(spec["chunk"], 1)
    c.fixed_len = spec.get("fixed_len", -1)
    c.identity = 1 if c.fixed_len >= 0 else 0
    hi = spec["gain"] == "hi"
    c.qn_w = f2b(rng.uniform(4, 8, D) if hi else 1 + 0.1 * rng.standard_normal(D))
    c.kn_w = f2b(bf16_to_f32(c.qn_w) * 0.9)
    gk = float(bf16_to_f32(c.kn_w).mean())
    c.cos, c.sin = rope_tables()
    c.kv_len = np.array([r[0] for r in spec["rows"]], np.int32)
    c.active = None if spec.get("active") is None else np.array(spec["active"], np.uint8)
    pad = spec.get("pad")
    if pad is not None:  # element p of row b is prompt position r_base + n_prompt[b] + p, skipped while negative
        c.r_base = -7
        c.n_prompt = np.array([7 - p for p in pad], np.int32)
    else:
        c.r_base, c.n_prompt = 0, None
    c.p0 = np.array(pad if pad is not None else [0] * B, np.int32)
    if c.identity:
        c.n_pages, c.bt = B + 2, np.arange(B, dtype=np.int32)[:, None].copy()
    else:
        c.n_pages = B * mp + 3  # three pages no row owns
        while True:
            c.bt = rng.permutation(c.n_pages)[: B * mp].reshape(B, mp).astype(np.int32)
            if not (c.bt.ravel() == np.arange(B * mp)).any() or B * mp == 1:
                break
        if B * mp == 1:
            c.bt[0, 0] = 2
    ld = (nh + 2 * nkv) * D
    rows = C * B
    qkv = rng.standard_normal((rows, ld)).astype(np.float32)
    for b in range(B):
        prof = spec["rows"][b][1]
        base = rng.standard_normal((nkv, D)).astype(np.float32)  # the heads of a group (and the elements of a chunk) point one way
        for p in range(C):
            r = p * B + b
            for kv in range(nkv):
                for j in range(rep):
                    h = kv * rep + j
                    qkv[r, h * D:(h + 1) * D] = base[kv] + 0.05 * rng.standard_normal(D) + (0.3 * rng.standard_normal(D) if p else 0)
                ks = slice(nh * D + kv * D, nh * D + (kv + 1) * D)
                if prof == "peak_new":
                    qkv[r, ks] = qkv[r, kv * rep * D:(kv * rep + 1) * D]
                elif prof == "equal":
                    qkv[r, ks] = 0.0
            qkv[r, (nh + nkv) * D:] *= 0.25 + 1.5 * rng.random()
    c.qkv = f2b(qkv)
    # positions and the reference's q / k / v of every element
    c.pos = np.full((C, B), -1, np.int64)
    for b in range(B):
        for p in range(int(c.p0[b]), C):
            c.pos[p, b] = c.kv_len[b] + (p - c.p0[b])
    posc = np.maximum(c.pos, 0).reshape(rows)
    q3 = c.qkv.reshape(rows, nh + 2 * nkv, D)
    c.q = norm_rope(q3[:, :nh], c.qn_w, c.cos[posc][:, None], c.sin[posc][:, None])           # [rows][nh][D]
    c.k = norm_rope(q3[:, nh:nh + nkv], c.kn_w, c.cos[posc][:, None], c.sin[posc][:, None])  # [rows][nkv][D]
    c.v = q3[:, nh + nkv:].copy()
    # pools: histories, sentinel everywhere else
    c.kpool = np.full((c.n_pages, nkv, PAGE, D), SENT, np.uint16)
    c.vpool = np.full((c.n_pages, nkv, PAGE, D), SENT, np.uint16)
    for b in range(B):
        T, prof = int(c.kv_len[b]), spec["rows"][b][1]
        if T == 0:
            continue
        kh = rng.standard_normal((T, nkv, D)) * gk
        vh = rng.standard_normal((T, nkv, D)) * (0.25 + 1.5 * rng.random((T, 1, 1)))
        first = int(c.p0[b]) * B + b if c.p0[b] < C else b
        qref = bf16_to_f32(c.q[first]).astype(np.float64)[::rep]  # [nkv][D]: first head of each group, first live element
        qq = (qref ** 2).sum(-1, keepdims=True)
        sigma = SCALE * np.sqrt(qq) * gk  # spread of a random key's score
        tstar = {"peak0": 0, "peak_last": T - 1, "peak63": min(63, T - 1), "peak64": min(64, T - 1)}.get(prof)
        if tstar is not None:
            kh[tstar] = qref * (12.0 * sigma / (SCALE * qq))
        elif prof == "ramp":  # scores rise with t: every step of a lane group rescales
            kh[:] = qref[None] * (0.25 * np.arange(T)[:, None, None] * sigma / (SCALE * qq))[..., :]
        elif prof == "equal":
            kh[:] = 0.0
        for t in range(T):
            pg = c.bt[b, t // PAGE]
            c.kpool[pg, :, t % PAGE] = f2b(kh[t])
            c.vpool[pg, :, t % PAGE] = f2b(vh[t])
    c.kpool_exp, c.vpool_exp = c.kpool.copy(), c.vpool.copy()
    c.live = np.zeros(c.kpool.shape[:3], bool)  # slots the launch must write
    for p in range(C):
        for b in range(B):
            if c.pos[p, b] < 0 or (c.active is not None and not c.active[b]):
                continue
            t = int(c.pos[p, b])
            pg = c.bt[b, t // PAGE]
            c.kpool_exp[pg, :, t % PAGE] = c.k[p * B + b]
            c.vpool_exp[pg, :, t % PAGE] = c.v[p * B + b]
            c.live[pg, :, t % PAGE] = True
    return c


def row_keys(c, kp, vp, p, b):
    """Keys / values [pos + 1][n_kv][D] (bits) of chunk element p of row b, from the pools as given; the new token of a row
    that does not append comes from the reference's own k / v."""
    t = int(c.pos[p, b])
    idx = np.arange(t + 1)
    K = kp[c.bt[b, idx // PAGE], :, idx % PAGE]
    V = vp[c.bt[b, idx // PAGE], :, idx % PAGE]
    if c.active is not None and not c.active[b]:
        K, V = K.copy(), V.copy()
        K[t], V[t] = c.k[p * c.spec["B"] + b], c.v[p * c.spec["B"] + b]
    return K, V


def reference_out(c, kp, vp):
    """float64 softmax(scale q.k) V per live row; returns (r [rows][nh][D], floor [rows][nh], live [rows])."""
    nh, nkv, B = c.spec["n_heads"], c.spec["n_kv"], c.spec["B"]
    rep = nh // nkv
    C = max(c.spec["chunk"], 1)
    r = np.zeros((C * B, nh, D))
    floor = np.zeros((C * B, nh))
    live = np.zeros(C * B, bool)
    for p in range(C):
        for b in range(B):
            if c.pos[p, b] < 0:
                continue
            row = p * B + b
            live[row] = True
            K, V = row_keys(c, kp, vp, p, b)
            K = np.repeat(bf16_to_f32(K).astype(np.float64), rep, axis=1)  # [T][nh][D]
            V = np.repeat(bf16_to_f32(V).astype(np.float64), rep, axis=1)
            q = bf16_to_f32(c.q[row]).astype(np.float64)
            s = SCALE * np.einsum("hd,thd->ht", q, K)
            w = np.exp(s - s.max(-1, keepdims=True))
            w /= w.sum(-1, keepdims=True)
            r[row] = np.einsum("ht,thd->hd", w, V)
            floor[row] = 2.0 ** -10 * np.abs(V).max(axis=(0, 2))
    return r, floor, live


def restated_out(c, kp, vp):
    """The kernels' walk in float32: NG lane groups, group g takes positions g, g + NG, ... in increasing order with an online
    softmax (16 lanes x 8 dims per dot product, butterfly over the lanes), then the log-sum-exp merge and one bf16 rounding."""
    nh, nkv, B = c.spec["n_heads"], c.spec["n_kv"], c.spec["B"]
    rep = nh // nkv
    C = max(c.spec["chunk"], 1)
    NG = 32 if (c.spec["max_pages"] > 1 and rep <= 2) else 16
    f32 = np.float32
    out = np.zeros((C * B, nh, D), np.uint16)
    scale = f32(SCALE)
    for p in range(C):
        for b in range(B):
            if c.pos[p, b] < 0:
                continue
            row = p * B + b
            K, V = row_keys(c, kp, vp, p, b)
            T = K.shape[0]
            K = np.repeat(bf16_to_f32(K), rep, axis=1)
            V = np.repeat(bf16_to_f32(V), rep, axis=1)
            q = bf16_to_f32(c.q[row])
            m = np.full((NG, nh), -np.inf, f32)
            l = np.zeros((NG, nh), f32)
            acc = np.zeros((NG, nh, D), f32)
            with np.errstate(invalid="ignore"):
                for s0 in range(0, T, NG):
                    t = s0 + np.arange(NG)
                    ok = t < T
                    tc = np.minimum(t, T - 1)
                    prod = (q[None] * K[tc]).reshape(NG, nh, 16, 8)
                    d = np.zeros((NG, nh, 16), f32)
                    for j in range(8):
                        d = d + prod[..., j]
                    for o in (1, 2, 4, 8):
                        d = d + d[..., np.arange(16) ^ o]
                    sc = d[..., 0] * scale
                    mn = np.maximum(m, sc)
                    alpha = np.where(np.isneginf(m), f32(0), np.exp(m - mn)).astype(f32)
                    pr = np.exp(sc - mn).astype(f32)
                    l2 = l * alpha + pr
                    acc2 = acc * alpha[..., None] + pr[..., None] * V[tc]
                    okh = ok[:, None]
                    m = np.where(okh, mn, m)
                    l = np.where(okh, l2, l)
                    acc = np.where(okh[..., None], acc2, acc)
                M = m.max(0)
                w = np.where(np.isneginf(m), f32(0), np.exp(m - M[None])).astype(f32)
            num = np.zeros((nh, D), f32)
            den = np.zeros(nh, f32)
            for g in range(NG):
                num = num + acc[g] * w[g][:, None]
                den = den + l[g] * w[g]
            out[row] = f2b(num / den[:, None])
    return out


def worst_ratio(out_bits, r, floor, live):
    """max |a - r| / bar over the live rows; inf when anything is not finite."""
    a = bf16_to_f32(out_bits).astype(np.float64).reshape(r.shape)[live]
    rr, fl = r[live], floor[live]
    if a.size == 0:
        return 0.0
    if not np.isfinite(a).all():
        return float("inf")
    bar = ULP * np.maximum(np.abs(rr), fl[..., None])
    return float((np.abs(a - rr) / bar).max())


def hook_args(c, **over):
    s = c.spec
    kw = dict(n_heads=s["n_heads"], n_kv=s["n_kv"], B=s["B"], kv_len=c.kv_len, active=c.active, block_table=c.bt,
              max_pages=s["max_pages"], eps=EPS, scale=SCALE, fixed_len=c.fixed_len, identity_pages=c.identity, chunk=s["chunk"],
              chunk_n_prompt=c.n_prompt, chunk_r_base=c.r_base, nt_kv=s["nt_kv"])
    kw.update(over)
    return kw


def run_hook(m, c, kpool=None, vpool=None, **over):
    return m.debug_attention(c.qkv, c.qn_w, c.kn_w, c.cos, c.sin, c.kpool if kpool is None else kpool,
                             c.vpool if vpool is None else vpool, **hook_args(c, **over))


# ---------------------------------------------------------------------------------------------
# CPU part: the generator, the reference and the bar against the float32 restatement
# ---------------------------------------------------------------------------------------------
def test_case_matrix_reaches_every_dispatch_branch():
    seen = set()
    for s in SPECS:
        rep = s["n_heads"] // s["n_kv"]
        wide = s["max_pages"] > 1 and rep <= 2
        if s["chunk"] > 1:
            seen.add(("chunk", rep, wide, s["chunk"] > 8))
        else:
            seen.add(("one", rep, wide, bool(s["nt_kv"]) and wide and rep == 2))
    want = {("one", 1, False, False), ("one", 1, True, False), ("one", 2, False, False), ("one", 2, True, False), ("one", 2, True, True),
            ("one", 3, False, False), ("one", 4, False, False)}
    for rep in (1, 2, 3, 4):
        for wide in ((False, True) if rep <= 2 else (False,)):
            for big in (False, True):
                want.add(("chunk", rep, wide, big))
    assert want <= seen, want - seen
    assert {s["chunk"] for s in CHUNK_SPECS} == {2, 4, 8, 9, 16}
    assert {s["B"] for s in SPECS if s["chunk"] == 0} >= {1, 3, 17, 33}
    lens = {r[0] for s in SPECS if s["chunk"] == 0 and s["max_pages"] > 1 for r in s["rows"]}
    assert lens >= {0, 1, 15, 16, 31, 32, 63, 64, 65, 127, 128, 200}
    pads = [s["pad"] for s in CHUNK_SPECS if s.get("pad")]
    assert pads and all({0, 1, s["chunk"] - 1, s["chunk"]} <= set(s["pad"]) for s in CHUNK_SPECS if s.get("pad"))


def test_reference_and_bar_hold_against_the_float32_restatement():
    """The float32 lane-group walk stays inside the bar for every case, and dropping a row's peak key does not: the inputs
    are inside the bar without the kernel, and the bar bites."""
    worst, where = 0.0, None
    for s in SPECS:
        c = make_case(s)
        assert np.isfinite(bf16_to_f32(c.q)).all() and np.isfinite(bf16_to_f32(c.k)).all()
        r, floor, live = reference_out(c, c.kpool_exp, c.vpool_exp)
        assert np.isfinite(r).all()
        w = worst_ratio(restated_out(c, c.kpool_exp, c.vpool_exp), r, floor, live)
        if w > worst:
            worst, where = w, s["name"]
        assert w <= 1.0, (s["name"], w)
    print("attention block, float32 restatement: worst |a - r| / bar = %.3f (%s)" % (worst, where))


def test_a_dropped_peak_key_breaks_the_bar():
    """Rows whose score peak sits on the last cached key or on the new token: without that key the restated result is far
    outside the bar (what the edge cases rely on)."""
    for mp in (4, 1):
        s = next(x for x in SPECS if x["chunk"] == 0 and x["max_pages"] == mp and x["B"] >= 17 and "cp-" not in x["name"])
        name = s["name"]
        c = make_case(s)
        r, floor, live = reference_out(c, c.kpool_exp, c.vpool_exp)
        for b, (T, prof) in enumerate(s["rows"]):
            if prof not in ("peak_last", "peak_new") or T == 0 or (c.active is not None and not c.active[b]):
                continue
            kp = c.kpool_exp.copy()
            t = T - 1 if prof == "peak_last" else T
            kp[c.bt[b, t // PAGE], :, t % PAGE] = 0  # the key scores 0 instead of the peak
            only = np.zeros_like(live)
            only[b] = True
            assert worst_ratio(restated_out(c, kp, c.vpool_exp), r, floor, only) > 4.0, (name, b, T, prof)


# ---------------------------------------------------------------------------------------------
# GPU part
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine(ckpt_dirs):
    from qwen3tts import Qwen3TTSModel
    m = Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-a"], max_batch=1, max_frames=8, max_prompt=16)
    yield m
    m.close()


WORST = {"ratio": 0.0, "case": None}


def check_launch(c, out, kp, vp):
    """V and the untouched slots bit-exact, K equal or adjacent, out inside the bar; returns the worst ratio."""
    name = c.spec["name"]
    assert (vp == c.vpool_exp).all(), (name, "V pool: %d elements differ" % int((vp != c.vpool_exp).sum()))
    assert (kp[~c.live] == c.kpool_exp[~c.live]).all(), (name, "a K slot that is no live new position was written")
    a, e = kp[c.live], c.kpool_exp[c.live]
    if a.size:
        near = (np.abs(a.astype(np.int32) - e.astype(np.int32)) <= 1) | (bf16_to_f32(a) == bf16_to_f32(e))
        assert near.all(), (name, "appended K off by more than one bf16 step: %d elements" % int((~near).sum()))
        assert (a != e).mean() < 0.02, (name, float((a != e).mean()))
    r, floor, live = reference_out(c, kp, vp)
    w = worst_ratio(out, r, floor, live)
    print("%s: worst |a - r| / bar = %.3f" % (name, w))
    assert w <= 1.0, (name, w)
    assert (out.reshape(live.size, -1)[~live] == 0xFFFF).all(), (name, "a padded chunk element's out row was written")
    if w > WORST["ratio"]:
        WORST["ratio"], WORST["case"] = w, name
    return w


@pytest.mark.gpu
@pytest.mark.parametrize("spec", SPECS, ids=SPEC_IDS)
def test_attention_block_matches_float64(engine, spec):
    c = make_case(spec)
    out, kp, vp = run_hook(engine, c)
    check_launch(c, out, kp, vp)
    if c.active is not None:  # `active` only gates the append
        out2, kp2, vp2 = run_hook(engine, c, active=None)
        assert (out2 == out).all(), spec["name"]
        assert (vp2 != vp).any(), spec["name"]  # (and without it the same rows do append)
    print("attention block, GPU: worst |a - r| / bar so far = %.3f (%s)" % (WORST["ratio"], WORST["case"]))


@pytest.mark.gpu
@pytest.mark.parametrize("spec", CHUNK_SPECS, ids=[s["name"] for s in CHUNK_SPECS])
def test_chunk_is_bit_identical_to_one_position_at_a_time(engine, spec):
    """A chunk == its live positions fed one launch at a time (attn_decode.hip: every lane group walks its positions in the
    order the one-position kernel would): out rows and both pools, bit for bit."""
    c = make_case(spec)
    B, C = spec["B"], spec["chunk"]
    out, kp, vp = run_hook(engine, c)
    kp1, vp1 = c.kpool, c.vpool
    for i in range(C):
        p = c.p0 + i  # element of every row at this step
        on = p < C
        if not on.any():
            break
        pc = np.minimum(p, C - 1)
        qkv = c.qkv.reshape(C, B, -1)[pc, np.arange(B)]
        kv_len = np.where(on, c.kv_len + i, 0).astype(np.int32) if c.fixed_len < 0 else c.kv_len
        o1, kp1, vp1 = engine.debug_attention(qkv, c.qn_w, c.kn_w, c.cos, c.sin, kp1, vp1,
                                              **hook_args(c, chunk=0, chunk_n_prompt=None, kv_len=kv_len, active=on.astype(np.uint8),
                                                          fixed_len=(c.fixed_len + i) if c.fixed_len >= 0 else -1))
        for b in np.nonzero(on)[0]:
            assert (o1[b] == out[pc[b] * B + b]).all(), (spec["name"], "element", int(pc[b]), "row", int(b))
    assert (kp1 == kp).all() and (vp1 == vp).all(), spec["name"]


@pytest.mark.gpu
def test_chunk_query_split_changes_nothing(engine, monkeypatch):
    """gridDim.z (Q3TTS_CHUNK_QSPLIT = 1, 2, 4) only deals the queries of a chunk to workgroups: the same bits as the default."""
    from qwen3tts import _lib
    monkeypatch.delenv("Q3TTS_CHUNK_QSPLIT", raising=False)
    _lib.reload_debug_env()
    cases = [make_case(s) for s in CHUNK_SPECS]
    base = [run_hook(engine, c) for c in cases]
    try:
        for qs in ("1", "2", "4"):
            monkeypatch.setenv("Q3TTS_CHUNK_QSPLIT", qs)
            _lib.reload_debug_env()
            for c, ref in zip(cases, base):
                got = run_hook(engine, c)
                assert all((x == y).all() for x, y in zip(got, ref)), (c.spec["name"], qs)
    finally:
        monkeypatch.delenv("Q3TTS_CHUNK_QSPLIT", raising=False)
        _lib.reload_debug_env()


@pytest.mark.gpu
def test_bad_arguments_are_refused_on_the_host(engine):
    """Nothing a caller passes becomes an index on the GPU unchecked: each of these returns INVALID_INPUT (3), and a good call
    afterwards gives what it gave before."""
    from qwen3tts import Qwen3TTSError
    one = make_case(next(s for s in SPECS if s["name"].startswith("one-") and s["max_pages"] == 4 and s["B"] >= 3))
    chk = make_case(next(s for s in CHUNK_SPECS if s["name"].startswith("chunk-4x2-p4") and s["chunk"] <= 8))
    cp = make_case(next(s for s in SPECS if s["name"].startswith("cp-4x2-f16")))
    good = run_hook(engine, one)

    def bt_with(c, b, pg, v):
        t = c.bt.copy()
        t[b, pg] = v
        return t

    def lens_with(c, b, v):
        t = c.kv_len.copy()
        t[b] = v
        return t

    T0 = int(one.kv_len[0])
    bad = [
        (one, dict(block_table=bt_with(one, 0, T0 // PAGE, one.n_pages))),  # the new token's page is outside the pool
        (one, dict(block_table=bt_with(one, 0, 0, -1))),
        (one, dict(kv_len=lens_with(one, 1, 4 * PAGE))),                   # no room for the new token
        (one, dict(kv_len=lens_with(one, 1, -1))),
        (one, dict(kv_len=lens_with(one, 2, N_POS))),                      # beyond the RoPE tables (and the pages)
        (chk, dict(kv_len=lens_with(chk, 0, 4 * PAGE - chk.spec["chunk"] + 1))),  # the chunk's last position has no page
        (cp, dict(fixed_len=64)),
        (cp, dict(fixed_len=-2)),
    ]
    for c, over in bad:
        with pytest.raises(Qwen3TTSError) as e:
            run_hook(engine, c, **over)
        assert e.value.status == 3, over
    small = cp.kpool[: cp.spec["B"] - 1]
    with pytest.raises(Qwen3TTSError) as e:  # identity_pages: row b owns page b, so B pages at least
        run_hook(engine, cp, kpool=small, vpool=cp.vpool[: cp.spec["B"] - 1])
    assert e.value.status == 3
    rope_short = one.cos[: int(one.kv_len.max())]
    with pytest.raises(Qwen3TTSError) as e:  # a RoPE table shorter than the longest row
        engine.debug_attention(one.qkv, one.qn_w, one.kn_w, rope_short, one.sin[: rope_short.shape[0]], one.kpool, one.vpool,
                               **hook_args(one))
    assert e.value.status == 3
    qkv17 = np.zeros((17 * chk.spec["B"], chk.qkv.shape[1]), np.uint16)
    with pytest.raises(Qwen3TTSError) as e:  # seventeen positions per launch
        chk_args = hook_args(chk, chunk=17)
        engine.debug_attention(qkv17, chk.qn_w, chk.kn_w, chk.cos, chk.sin, chk.kpool, chk.vpool, **chk_args)
    assert e.value.status == 3
    for nh in (5 * one.spec["n_kv"], one.spec["n_kv"] + 1):  # five query heads per kv head; not a multiple
        qkv = np.zeros((one.spec["B"], (nh + 2 * one.spec["n_kv"]) * D), np.uint16)
        with pytest.raises(Qwen3TTSError) as e:
            engine.debug_attention(qkv, one.qn_w, one.kn_w, one.cos, one.sin, one.kpool, one.vpool, **hook_args(one, n_heads=nh))
        assert e.value.status == 3, nh
    again = run_hook(engine, one)
    assert all((x == y).all() for x, y in zip(good, again))
