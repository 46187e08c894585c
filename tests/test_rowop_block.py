"""Block-level parity of the non-GEMM row kernels of the codec decoder (csrc/kernels/codec_misc.hip) and of the voice-clone front
end (csrc/kernels/voice_frontend.hip) through q3tts_debug_rowop: one launch of the product's own launcher per case, on
caller-built host buffers (the slot table per op: include/q3tts.h), against references written here. 21 launchers.

References. numpy float64 of the mathematical operation, unrounded, on the exact fp32 inputs:
  rmsnorm_f32      x / sqrt(mean(x^2) + eps) * w
  dwconv_ln        y_c = b_c + sum_k x[t-6+k][c] w[c][k] over the rows t-6+k >= -hist, then LayerNorm_c(y) * ln_w + ln_b
  layernorm_f32    (x - mean) / sqrt(var + eps) * w + b, var = mean((x - mean)^2)
  silu_mul_f32     g / (1 + exp(-g)) * u
  attn_full_f32    softmax_j(q_i . k_j / 8) v_j over j < T;  attn_causal_f32: over j <= i
  enc_init_conv    bias_c + sum_k w[c][k] audio[t-(K-1)+k], zero in front of the clip
  rope_qk_f32      (x1 c - x2 s, x1 s + x2 c) on (x[d], x[d+32]) of the q and k heads
  log_mel          log(max(sum_k (re^2 + im^2) fb[k][m], 1e-10f))
  time_stats       mean_t x, sqrt(mean_t (x - mean)^2 + eps)
  scale_res        x se + res
  asp_pool         w_t = softmax_t(att), mean = sum w x, sqrt(max(sum w (x - mean)^2, eps))
The copies and the kernels that claim an order are held to == on raw bits instead: rvq_gather against fp32 adds in layer order;
rvq_encode's codes against a float32 restatement (separate multiply and add, dimensions in order, c2 - dot, lowest index on
ties, residual r - emb; a frame with no distance below +inf takes bin 0 on every layer); roll_history, roll_history_rows (the new
margin is the last `hist` frames of [old margin ++ the `take` frames written]; everything but the margins of rows with mode != 0
keeps its bits), history_state_rows, stream_take_chunk, asp_concat, mask_tail, copy2d_f32 and the v third of rope_qk_f32 against
the copy itself.

Bars. e = 2^-24, half an fp32 step. A sum of n terms in any order lies within n e sum|terms|; each further
fp32 operation adds e |value|; expf / logf / sinf / cosf one fp32 step of the result (2 e); division and sqrtf are correctly
rounded (no fast-math flag). Operand errors are carried through first-order derivatives (the square of a carried error is kept
where a clamp or a small eps makes it matter). Never a constant floor.
  rmsnorm_f32      ((C + 3) / 2 + 4) e |out|           tot = sum x^2 within (C + 1) e tot (positive terms), / C, + eps: rel (C + 3) e;
                                                        sqrt halves it, + e, 1 / . + e, two products 2 e
  LayerNorm tail   y_c known within Ey_c (dwconv_ln: (taps + 2) e (sum |x w| + |b|); layernorm_f32: 0)
                   Em  = (sum Ey + C e sum|y|) / C + e |mean|                                 the error of the mean, carried into
                   Ed  = Ey + Em + e |d|,  d = y - mean                                       (y - mean)
                   Ev  = (sum (2 |d| Ed + Ed^2 + e d^2) + C e sum d^2) / C + e var
                   Rr  = (Ev + e (var + eps)) / (2 (var + eps)) + 2 e                         relative error of 1 / sqrt(var + eps)
                   out = |w| (rstd Ed + |d rstd| (Rr + 2 e)) + e |out|
  silu_mul_f32     5 e |out|                            expf 2 e, 1 + . e (exp(-g) <= 1 + exp(-g)), / e, * e
  attentions       ds = (64 + 2) e scale sum_d |q_d k_jd|, ds_max over the query's keys;
                   (2 ds_max + (3 n + 8) e) sum_j p_j |v_jd|, n the query's keys (T; causal: i + 1)
  enc_init_conv    (K + 2) e (sum |w x| + |bias|)
  rope_qk_f32      2 e (|x1 c| + |x2 s|)   and   2 e (|x1 s| + |x2 c|)
  log_mel          compared in the log domain: (nfreq + 6) e + 2 e |log|    re^2 + im^2 rel 2 e, sqrt 2 e, squared 5 e, * fb 6 e, the sum
                                                        of nfreq non-negative terms nfreq e; d log = relative error; one logf step
                   (measured on an MI355X: logf(1e-10f) lies 3.19e-6 from the exact logarithm, 1.7 fp32 steps, against 2 e |log| =
                   2.74e-6; the all-zero frame stays inside the bar through the sum's term only, 0.94 of it at nfreq 5)
  time_stats       Em = e sum|x| + e |mean| (T terms: T e sum|x| / T);  Ed = Em + e |d|
                   Ev = (sum (2 |d| Ed + Ed^2 + e d^2) + T e sum d^2) / T + e var;  std: (Ev + e (var + eps)) / (2 std) + e std
  scale_res        e |x se| + e (|x se| + |res|)
  asp_pool         a_t = att - max (exact max): p_t rel (|a_t| + 2) e; sum rel Rs = (T + max|a| + 2) e; w_t rel Rw_t = (|a_t| + 3) e + Rs
                   Em = sum |w x| (Rw + e) + T e sum |w x|;  Ed = Em + e |d|
                   Ev = sum w ((2 |d| Ed + Ed^2 + e d^2) + d^2 (Rw + e)) + T e sum w d^2
                   std = sqrt(max(var, eps)): min(Ev / sqrt(max(var, eps)), sqrt(Ev)) + e std     (|sqrt a - sqrt b| <= sqrt|a - b|)
These constants are derived from the code, not measured. Their check is the CPU part: a float32 restatement of each kernel's
walk in the kernel's order (256-thread strides, the 64-lane xor butterfly then ((s0 + s1) + s2) + s3, the online softmax key by
key, time_stats' four time slices) against the float64 reference under the same bars, every case. No element is exempt.

Bit-exact equivalences (== on raw bits), derived from the code: per element the operation sequence depends on the row's own
length and width only, so a row of a ragged batch equals the same row alone (rmsnorm_f32, dwconv_ln, silu_mul_f32, attn_full_f32,
layernorm_f32, enc_init_conv, rvq_encode); dwconv_ln cut in two launches with hist = 6 equals one launch; attn_causal_f32 rows
[0, T') of a T-long run equal a T'-long run, and keys / values behind a query do not move its output; enc_init_conv across the
256-sample block edge equals the same samples inside a block.

Sentinels (the NaN pattern 0x7FC12345): input rows a launch must not read (behind a row's length, in front of the `hist` rows),
every output before the launch. Afterwards every element the op owns is finite and inside its bar and everything else keeps its
bits. State buffers of the copy kernels hold distinct random bits instead and are compared whole.

The CPU part (no marker) runs every job's check_only call (the case table is launchable), the restatements under the bars with
the bit-exact claims, and the host refusals; the GPU part runs the same flows through the launchers and prints WORST."""
import zlib

import numpy as np
import pytest

E = 2.0 ** -24
SENT = 0x7FC12345
WORST = {}            # op -> worst error / bar seen in this process
F32 = np.float32
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31


def rng_of(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def sent(shape, dtype=np.float32):
    a = np.empty(shape, np.uint32)
    a[...] = SENT
    return a.view(dtype)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def is_sent(a):
    return bits(a) == SENT


def noise_bits(key, n):
    """n distinct-looking finite floats: what a copy kernel moves, and what it must leave alone."""
    return rng_of("bits", key).standard_normal(n).astype(F32)


def job(op, p, f=(), ins=(), ios=(), **meta):
    return dict(op=op, p=list(p), f=list(f), ins=list(ins), ios=list(ios), **meta)


def within(op, got, ref, bar, what):
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), "%s: %s holds a non-finite value" % (op, what)
    err = np.abs(got - ref)
    bar = np.broadcast_to(bar, err.shape)
    if (err > bar).any():
        i = np.unravel_index(np.argmax(err - bar), err.shape)
        raise AssertionError("%s: %s leaves its bar at %r: error %.4g, bar %.4g" % (op, what, i, err[i], bar[i]))
    pos = bar > 0
    if pos.any():
        WORST[op] = max(WORST.get(op, 0.0), float((err[pos] / bar[pos]).max()))


def same_bits(a, b, what):
    a, b = bits(a), bits(b)
    assert a.shape == b.shape, what
    if not np.array_equal(a, b):
        i = np.flatnonzero(a.ravel() != b.ravel())
        raise AssertionError("%s: %d of %d words differ, the first at %d" % (what, i.size, a.size, i[0]))


def untouched(a, what):
    assert is_sent(a).all(), "%s: a sentinel was overwritten" % what


# ---------------------------------------------------------------------------------------------
# the kernels' reductions, restated in float32
# ---------------------------------------------------------------------------------------------
def thread_partials(v):
    """(..., n) float32 -> (..., 256): thread i adds elements i, i + 256, ... in that order, from 0."""
    n = v.shape[-1]
    k = -(-n // 256)
    pad = np.zeros(v.shape[:-1] + (k * 256,), F32)
    pad[..., :n] = v
    pad = pad.reshape(v.shape[:-1] + (k, 256))
    s = np.zeros(v.shape[:-1] + (256,), F32)
    for i in range(k):
        s = s + pad[..., i, :]
    return s


def block_sum(s):
    """block_sum_256: the xor butterfly 32, 16, ..., 1 within each wave of 64, then ((s0 + s1) + s2) + s3."""
    w = s.reshape(s.shape[:-1] + (4, 64))
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        w = w + w[..., lane ^ off]
    w = w[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def ln_restate(y, w, b, eps):
    """The LayerNorm tail of dwconv_ln_kernel / layernorm_f32_kernel on rows y (..., C)."""
    C = y.shape[-1]
    mean = (block_sum(thread_partials(y)) / F32(C))[..., None]
    d = y - mean
    var = block_sum(thread_partials(d * d)) / F32(C)
    rstd = (F32(1) / np.sqrt(var + F32(eps)))[..., None]
    return ((d * rstd) * w) + b


def ln_ref_bar(y, Ey, w, b, eps):
    """float64 LayerNorm of rows y (..., C) known within Ey, and the bar of the header."""
    C = y.shape[-1]
    w, b = w.astype(np.float64), b.astype(np.float64)
    mean = y.mean(-1, keepdims=True)
    Em = (Ey.sum(-1, keepdims=True) + C * E * np.abs(y).sum(-1, keepdims=True)) / C + E * np.abs(mean)
    d = y - mean
    Ed = Ey + Em + E * np.abs(d)
    var = (d * d).mean(-1, keepdims=True)
    Ev = ((2 * np.abs(d) * Ed + Ed * Ed + E * d * d).sum(-1, keepdims=True) + C * E * (d * d).sum(-1, keepdims=True)) / C + E * var
    eps = float(F32(eps))
    Rr = (Ev + E * (var + eps)) / (2 * (var + eps)) + 2 * E
    rstd = 1.0 / np.sqrt(var + eps)
    out = d * rstd * w + b
    bar = np.abs(w) * (rstd * Ed + np.abs(d * rstd) * (Rr + 2 * E)) + E * np.abs(out)
    return out, bar


def seq_rows(seed, C, n=64, scale=1.0):
    """Row data of sequence `seed`: the same rows whatever case asks for them."""
    return (rng_of("seq", seed, C).standard_normal((n, C)) * scale).astype(F32)


def vecf(tag, n, scale=1.0, shift=0.0):
    return (rng_of("vec", tag, n).standard_normal(n) * scale + shift).astype(F32)


# ---------------------------------------------------------------------------------------------
# codec decoder
# ---------------------------------------------------------------------------------------------
class RvqGather:
    op = "rvq_gather"
    CASES = [dict(inner=64, n_rest=1, rows=[(0, 5)], Fmax=5, csf=5, ff=None),
             dict(inner=256, n_rest=15, rows=[(0, 4)], Fmax=6, csf=6, ff=None),
             dict(inner=260, n_rest=15, rows=[(0, 5), (1, 0), (2, 3)], Fmax=6, csf=6, ff=None),
             dict(inner=260, n_rest=15, rows=[(0, 5), (1, 0), (2, 3)], Fmax=6, csf=9, ff=[2, 0, 1])]
    RF, RR = 7, 5

    def make(self, c):
        inner, n_rest, B = c["inner"], c["n_rest"], len(c["rows"])
        r = rng_of("gather", inner, n_rest)
        cbf = r.standard_normal((self.RF, inner)).astype(F32)
        gap = 8                                                       # the tables sit apart in the pool, in reverse order
        per = self.RR * inner + gap
        pool = sent(n_rest * per)
        offs = np.array([(n_rest - 1 - j) * per + 4 for j in range(n_rest)], np.int64)
        cbr = r.standard_normal((n_rest, self.RR, inner)).astype(F32)
        for j in range(n_rest):
            pool[offs[j]:offs[j] + self.RR * inner] = cbr[j].ravel()
        codes = sent((B, c["csf"], 16), np.int32)
        for b, (seed, F) in enumerate(c["rows"]):
            f0 = c["ff"][b] if c["ff"] else 0
            cr = rng_of("codes", seed).integers(0, 5, (c["csf"], 16)).astype(np.int32)
            cr[0, :4] = [-1, self.RR, INT_MAX, INT_MIN]               # clamped: -1 -> 0, rows -> rows - 1, ...
            cr[1, :4] = [self.RF, -1, INT_MIN, INT_MAX]
            cr[2, 0] = INT_MAX
            codes[b, f0:f0 + F] = cr[:F]
        frames = np.array([F for _, F in c["rows"]], np.int32)
        ff = None if c["ff"] is None else np.array(c["ff"], np.int32)
        out = sent((B, c["Fmax"], 2 * inner))
        return job(self.op, [B, c["Fmax"], c["csf"], n_rest, inner, self.RF, self.RR], [], [codes, cbf, pool, frames, ff, offs], [out],
                   c=c, cbf=cbf, cbr=cbr)

    def expect(self, j):
        """fp32 adds in layer order, on the clamped rows."""
        c, (codes, _, _, frames, ff, _) = j["c"], j["ins"]
        inner = c["inner"]
        out = j["ios"][0].copy()
        for b in range(len(frames)):
            f0 = int(ff[b]) if ff is not None else 0
            for f in range(frames[b]):
                cd = codes[b, f0 + f].astype(np.int64)
                out[b, f, :inner] = j["cbf"][np.clip(cd[0], 0, self.RF - 1)]
                q = j["cbr"][0][np.clip(cd[1], 0, self.RR - 1)]
                for k in range(1, c["n_rest"]):
                    q = q + j["cbr"][k][np.clip(cd[1 + k], 0, self.RR - 1)]
                out[b, f, inner:] = q
        return out

    def restate(self, j):
        return [self.expect(j)]

    def flow(self, run, jobs):
        for j in jobs:
            got = run(j)[0]
            same_bits(got, self.expect(j), "rvq_gather %r" % (j["c"],))                  # frames >= frames[b] keep the sentinel
            c, inner = j["c"], j["c"]["inner"]
            for b, (_, F) in enumerate(c["rows"]):                                         # and the order's error against float64
                f0 = c["ff"][b] if c["ff"] else 0
                for f in range(F):
                    cd = j["ins"][0][b, f0 + f].astype(np.int64)
                    terms = np.stack([j["cbr"][k][np.clip(cd[1 + k], 0, self.RR - 1)] for k in range(c["n_rest"])]).astype(np.float64)
                    within(self.op, got[b, f, inner:], terms.sum(0), c["n_rest"] * E * np.abs(terms).sum(0), "the acoustic sum")

    def jobs(self):
        return [self.make(c) for c in self.CASES]


def ragged_x(rows, Tmax, C, ppf, hist=0, margin=0):
    """[B][Tmax][C]: row b holds rows [start - hist, start + frames * ppf) of its sequence behind `margin - hist` sentinels."""
    x = sent((len(rows), Tmax, C))
    for b, (seed, start, F) in enumerate(rows):
        if F > 0:
            x[b, margin - hist:margin + F * ppf] = seq_rows(seed, C)[start - hist:start + F * ppf]
    return x


class RmsNorm:
    op = "rmsnorm_f32"
    EPS = 1e-5
    CASES = [dict(C=1, rows=[(1, 0, 3)]), dict(C=128, rows=[(1, 0, 3)]), dict(C=512, rows=[(1, 0, 3)]), dict(C=516, rows=[(1, 0, 3)]),
             dict(C=516, ppf=2, rows=[(1, 0, 3)], key="alone1"), dict(C=516, ppf=2, rows=[(3, 0, 2)], key="alone3"),
             dict(C=516, ppf=2, rows=[(1, 0, 3), (2, 0, 0), (3, 0, 2)], Tmax=7, key="ragged")]

    def make(self, c):
        C, ppf, rows = c["C"], c.get("ppf", 1), c["rows"]
        Tmax = c.get("Tmax", max(F for _, _, F in rows) * ppf + 1)
        x = ragged_x(rows, Tmax, C, ppf)
        w = vecf("rms-w", C, 0.5, 1.0)
        frames = np.array([F for _, _, F in rows], np.int32)
        return job(self.op, [len(rows), Tmax, ppf, C], [self.EPS], [x, w, frames], [sent((len(rows), Tmax, C))], c=c, ppf=ppf)

    def restate(self, j):
        x, w, frames = j["ins"]
        out = j["ios"][0].copy()
        for b, F in enumerate(frames):
            v = x[b, :F * j["ppf"]]
            tot = block_sum(thread_partials(v * v))
            rstd = F32(1) / np.sqrt(tot / F32(v.shape[-1]) + F32(self.EPS))
            out[b, :F * j["ppf"]] = (v * rstd[:, None]) * w
        return [out]

    def verify(self, j, got):
        x, w, frames = j["ins"]
        C = x.shape[-1]
        for b, F in enumerate(frames):
            n = F * j["ppf"]
            v = x[b, :n].astype(np.float64)
            ref = v / np.sqrt((v * v).mean(-1, keepdims=True) + float(F32(self.EPS))) * w.astype(np.float64)
            within(self.op, got[b, :n], ref, ((C + 3) / 2 + 4) * E * np.abs(ref), "out")
            untouched(got[b, n:], self.op)

    def flow(self, run, jobs):
        res = {}
        for j in jobs:
            got = run(j)[0]
            self.verify(j, got)
            res[j["c"].get("key")] = got
        same_bits(res["ragged"][0, :6], res["alone1"][0, :6], "rmsnorm_f32: row 0 of a ragged batch against the row alone")
        same_bits(res["ragged"][2, :4], res["alone3"][0, :4], "rmsnorm_f32: row 2 of a ragged batch against the row alone")

    def jobs(self):
        return [self.make(c) for c in self.CASES]


class DwconvLn:
    op = "dwconv_ln"
    EPS = 1e-6
    #            C, hist, margin, rows (seed, start, frames)
    CASES = [dict(C=128, hist=0, margin=1, rows=[(1, 0, 1)]),
             dict(C=260, hist=2, margin=3, rows=[(1, 2, 5)]),
             dict(C=1024, hist=6, margin=8, rows=[(1, 6, 6)]),
             dict(C=260, hist=0, margin=2, rows=[(1, 0, 7)]),                       # positions 0 .. 6: 1 .. 7 taps
             dict(C=128, hist=6, margin=7, rows=[(2, 6, 20)]),
             dict(C=260, hist=2, margin=4, rows=[(3, 2, 20)], bigmean=True),
             dict(C=260, hist=0, margin=1, rows=[(4, 0, 20)], key="whole"),
             dict(C=260, hist=0, margin=1, rows=[(4, 0, 9)], key="cut1"),
             dict(C=260, hist=6, margin=9, rows=[(4, 9, 11)], key="cut2"),
             dict(C=260, hist=2, margin=4, ppf=2, rows=[(5, 2, 5)], key="alone5"),
             dict(C=260, hist=2, margin=4, ppf=2, rows=[(6, 2, 3)], key="alone6"),
             dict(C=260, hist=2, margin=4, ppf=2, rows=[(5, 2, 5), (7, 2, 0), (6, 2, 3)], Tmax=17, key="ragged")]

    def make(self, c):
        C, ppf, rows, hist, margin = c["C"], c.get("ppf", 1), c["rows"], c["hist"], c["margin"]
        Tmax = c.get("Tmax", margin + max(F for _, _, F in rows) * ppf + 1)
        x = ragged_x(rows, Tmax, C, ppf, hist, margin)
        dw_w = (rng_of("dw-w", C).standard_normal((C, 7)) / np.sqrt(7)).astype(F32)
        dw_b = vecf("dw-b", C, 0.05, 50.0) if c.get("bigmean") else vecf("dw-b", C, 0.3)   # |mean| >> std across the channels
        ln_w, ln_b = vecf("ln-w", C, 0.5, 1.0), vecf("ln-b", C, 0.3)
        frames = np.array([F for _, _, F in rows], np.int32)
        return job(self.op, [len(rows), Tmax, ppf, C, hist, margin], [self.EPS], [x, dw_w, dw_b, ln_w, ln_b, frames],
                   [sent((len(rows), Tmax, C))], c=c, ppf=ppf)

    def taps(self, j, b, dtype):
        """[7][T][C] tap operands of batch row b (zero where the kernel skips a tap), and the taps' mask [7][T]."""
        x = j["ins"][0]
        hist, margin = j["c"]["hist"], j["c"]["margin"]
        T = int(j["ins"][5][b]) * j["ppf"]
        t = np.arange(T)
        xs, ms = [], []
        for k in range(7):
            ti = t - 6 + k
            ok = ti >= -hist
            row = np.where(ok, margin + ti, margin)      # (a valid row where the tap is skipped)
            xs.append(np.where(ok[:, None], x[b, row].astype(dtype), 0))
            ms.append(ok)
        return np.stack(xs), np.stack(ms)

    def restate(self, j):
        _, dw_w, dw_b, ln_w, ln_b, frames = j["ins"]
        out = j["ios"][0].copy()
        M = j["c"]["margin"]
        for b, F in enumerate(frames):
            if F == 0:
                continue
            xs, ms = self.taps(j, b, F32)
            acc = np.zeros(xs.shape[1:], F32)
            for k in range(7):
                acc = np.where(ms[k][:, None], acc + xs[k] * dw_w[:, k], acc)
            y = acc + dw_b
            out[b, M:M + F * j["ppf"]] = ln_restate(y, ln_w, ln_b, self.EPS)
        return [out]

    def verify(self, j, got):
        _, dw_w, dw_b, ln_w, ln_b, frames = j["ins"]
        M = j["c"]["margin"]
        for b, F in enumerate(frames):
            n = F * j["ppf"]
            if n:
                xs, ms = self.taps(j, b, np.float64)
                prod = xs * dw_w.astype(np.float64).T[:, None, :]
                y = prod.sum(0) + dw_b.astype(np.float64)
                S = np.abs(prod).sum(0) + np.abs(dw_b.astype(np.float64))
                Ey = (ms.sum(0)[:, None] + 2) * E * S
                ref, bar = ln_ref_bar(y, Ey, ln_w, ln_b, self.EPS)
                within(self.op, got[b, M:M + n], ref, bar, "out %r" % (j["c"],))
            untouched(got[b, :M], self.op)
            untouched(got[b, M + n:], self.op)

    def flow(self, run, jobs):
        res = {}
        for j in jobs:
            got = run(j)[0]
            self.verify(j, got)
            res[j["c"].get("key")] = got
        cut = np.concatenate([res["cut1"][0, 1:10], res["cut2"][0, 9:20]])
        same_bits(cut, res["whole"][0, 1:21], "dwconv_ln: cut in two launches with hist = 6 against one launch")
        same_bits(res["ragged"][0, 4:14], res["alone5"][0, 4:14], "dwconv_ln: row 0 of a ragged batch against the row alone")
        same_bits(res["ragged"][2, 4:10], res["alone6"][0, 4:10], "dwconv_ln: row 2 of a ragged batch against the row alone")

    def jobs(self):
        return [self.make(c) for c in self.CASES]


class SiluMul:
    op = "silu_mul_f32"
    CASES = [dict(I=256, rows=[(1, 3)]), dict(I=260, rows=[(1, 3)], cold=True), dict(I=1024, rows=[(1, 3)]),
             dict(I=260, ppf=2, rows=[(1, 3)], key="alone1"), dict(I=260, ppf=2, rows=[(3, 2)], key="alone3"),
             dict(I=260, ppf=2, rows=[(1, 3), (2, 0), (3, 2)], Tmax=7, key="ragged")]

    def make(self, c):
        I, ppf, rows = c["I"], c.get("ppf", 1), c["rows"]
        Tmax = c.get("Tmax", max(F for _, F in rows) * ppf + 1)
        gu = sent((len(rows), Tmax, 2 * I))
        for b, (seed, F) in enumerate(rows):
            r = rng_of("silu", seed, I)
            g = r.uniform(-30, 30, (8, I)).astype(F32)
            u = r.standard_normal((8, I)).astype(F32)
            u[u == 0] = 1
            if c.get("cold"):
                g[:, ::7] = -200.0                                      # expf(200) = inf: the result is exactly -0 * u
            gu[b, :F * ppf] = np.concatenate([g, u], 1)[:F * ppf]
        frames = np.array([F for _, F in rows], np.int32)
        return job(self.op, [len(rows), Tmax, ppf, I], [], [gu, frames], [sent((len(rows), Tmax, I))], c=c, ppf=ppf)

    def restate(self, j):
        gu, frames = j["ins"]
        I = j["c"]["I"]
        out = j["ios"][0].copy()
        for b, F in enumerate(frames):
            n = F * j["ppf"]
            g, u = gu[b, :n, :I], gu[b, :n, I:]
            with np.errstate(over="ignore"):
                out[b, :n] = (g / (F32(1) + np.exp(-g))) * u
        return [out]

    def verify(self, j, got):
        gu, frames = j["ins"]
        I = j["c"]["I"]
        for b, F in enumerate(frames):
            n = F * j["ppf"]
            g, u = gu[b, :n, :I].astype(np.float64), gu[b, :n, I:].astype(np.float64)
            cold = g == -200.0
            ref = np.where(cold, 0.0, g / (1 + np.exp(-np.where(cold, 0.0, g))) * u)
            within(self.op, got[b, :n], ref, np.where(cold, 0.0, 5 * E * np.abs(ref)), "out")
            assert (np.signbit(got[b, :n][cold]) == (u[cold] > 0)).all(), "silu_mul_f32: g = -200 must give -0 * u"
            untouched(got[b, n:], self.op)

    def flow(self, run, jobs):
        res = {}
        for j in jobs:
            got = run(j)[0]
            self.verify(j, got)
            res[j["c"].get("key")] = got
        same_bits(res["ragged"][0, :6], res["alone1"][0, :6], "silu_mul_f32: row 0 of a ragged batch against the row alone")
        same_bits(res["ragged"][2, :4], res["alone3"][0, :4], "silu_mul_f32: row 2 of a ragged batch against the row alone")

    def jobs(self):
        return [self.make(c) for c in self.CASES]


# ---- the two attentions ----
def attn_rows(seed, T, heads, causal):
    """qkv [T][3 heads 64] whose scores spread to |s| = 20. Query i, by i % 6: its score peak on key 0, 63, 64 or T - 1 (causal:
    clipped to the diagonal; `T - 1` is the query itself), a ramp over the keys from -20 to 20, or all scores equal. A peaked
    row hides every key but the peak, so a lost edge key only shows where the peak sits on it (tests/test_attention_block.py)."""
    r = rng_of("attn", seed, heads)
    k = r.standard_normal((130, heads, 64))[:T]
    v = r.standard_normal((130, heads, 64))[:T]
    n = 130 if causal else T                                              # (causal: a shorter run is a prefix of the longer one)
    k[:, :, 0] = (16.0 * (np.arange(T) / n - 0.5))[:, None]
    q = np.zeros((T, heads, 64))
    for i in range(T):
        kind = i % 6
        if kind < 4:
            p = min((0, 63, 64, T - 1)[kind], i if causal else T - 1)
            q[i] = k[p] * (160.0 / (k[p] * k[p]).sum(-1))[:, None]       # q . k_p / 8 = 20
        elif kind == 4:
            q[i, :, 0] = 20.0                                             # s_ij = 40 (j / n - 1 / 2)
    return np.concatenate([q.reshape(T, -1), k.reshape(T, -1), v.reshape(T, -1)], 1).astype(F32)


def attn_restate(qkv, heads, causal):
    """One query per thread, keys one after the other: s = sum_d q k in dimension order, the online softmax per key."""
    T = qkv.shape[0]
    q, k, v = (qkv[:, i * heads * 64:(i + 1) * heads * 64].reshape(T, heads, 64) for i in range(3))
    m = np.full((T, heads), -np.inf, F32)
    l = np.zeros((T, heads), F32)
    acc = np.zeros((T, heads, 64), F32)
    qi = np.arange(T)
    with np.errstate(invalid="ignore"):
        for j in range(T):
            s = np.zeros((T, heads), F32)
            for d in range(64):
                s = s + q[:, :, d] * k[j, :, d]
            s = s * F32(0.125)
            mn = np.maximum(m, s)
            alpha, p = np.exp(m - mn), np.exp(s - mn)
            l2 = l * alpha + p
            acc2 = acc * alpha[..., None] + p[..., None] * v[j]
            if causal:
                on = (j <= qi)[:, None]
                m, l, acc = np.where(on, mn, m), np.where(on, l2, l), np.where(on[..., None], acc2, acc)
            else:
                m, l, acc = mn, l2, acc2
    return (acc * (F32(1) / l)[..., None]).reshape(T, heads * 64)


def attn_ref_bar(qkv, heads, causal):
    T = qkv.shape[0]
    q, k, v = (qkv[:, i * heads * 64:(i + 1) * heads * 64].reshape(T, heads, 64).astype(np.float64) for i in range(3))
    s = np.einsum("ihd,jhd->hij", q, k) * 0.125
    sa = np.einsum("ihd,jhd->hij", np.abs(q), np.abs(k)) * 0.125
    on = np.tril(np.ones((T, T), bool)) if causal else np.ones((T, T), bool)
    s = np.where(on, s, -np.inf)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    ds = (66 * E * np.where(on, sa, 0.0)).max(-1)                          # [h][i]
    nk = (np.arange(T) + 1 if causal else np.full(T, T)).astype(np.float64)
    ref = np.einsum("hij,jhd->ihd", p, v)
    bar = (2 * ds.T + (3 * nk[:, None] + 8) * E)[..., None] * np.einsum("hij,jhd->ihd", p, np.abs(v))
    return ref.reshape(T, -1), bar.reshape(T, -1)


class AttnFull:
    op = "attn_full_f32"
    HEADS = 3
    CASES = [dict(rows=[(1, 1)]), dict(rows=[(1, 63)]), dict(rows=[(1, 64)]), dict(rows=[(2, 65)], key="alone65"),
             dict(rows=[(1, 130)], key="alone130"), dict(rows=[(1, 130), (3, 0), (2, 65)], Tmax=131, key="ragged")]

    def make(self, c):
        rows = c["rows"]
        Tmax = c.get("Tmax", max(T for _, T in rows) + 1)
        qkv = sent((len(rows), Tmax, 3 * self.HEADS * 64))
        for b, (seed, T) in enumerate(rows):
            if T:
                qkv[b, :T] = attn_rows(seed, T, self.HEADS, False)
        frames = np.array([T for _, T in rows], np.int32)
        return job(self.op, [len(rows), Tmax, self.HEADS], [], [qkv, frames], [sent((len(rows), Tmax, self.HEADS * 64))], c=c)

    def restate(self, j):
        qkv, frames = j["ins"]
        out = j["ios"][0].copy()
        for b, T in enumerate(frames):
            if T:
                out[b, :T] = attn_restate(qkv[b, :T], self.HEADS, False)
        return [out]

    def verify(self, j, got):
        qkv, frames = j["ins"]
        for b, T in enumerate(frames):
            if T:
                ref, bar = attn_ref_bar(qkv[b, :T], self.HEADS, False)
                within(self.op, got[b, :T], ref, bar, "out T=%d" % T)
            untouched(got[b, T:], self.op)

    def flow(self, run, jobs):
        res = {}
        for j in jobs:
            got = run(j)[0]
            self.verify(j, got)
            res[j["c"].get("key")] = got
        same_bits(res["ragged"][0, :130], res["alone130"][0, :130], "attn_full_f32: row 0 of a ragged batch against the row alone")
        same_bits(res["ragged"][2, :65], res["alone65"][0, :65], "attn_full_f32: row 2 of a ragged batch against the row alone")

    def jobs(self):
        return [self.make(c) for c in self.CASES]


# ---- the stream's state kernels: distinct bits everywhere, compared whole ----
class RollHistory:
    op = "roll_history"
    #        B, keep, chunk, bstride
    CASES = [(1, 4, 4, 8), (2, 4, 12, 24), (1, 65540, 65540, 131080), (2, 65540, 65544, 131088)]

    def make(self, c):
        B, keep, chunk, bs = c
        return job(self.op, [B, bs, keep, chunk], [], [], [noise_bits(c, (B - 1) * bs + keep + chunk)], c=c)

    def expect(self, j):
        B, keep, chunk, bs = j["c"]
        buf = j["ios"][0].copy()
        for b in range(B):
            row = j["ios"][0][b * bs:]
            buf[b * bs:b * bs + keep] = row[chunk:chunk + keep]       # the last `keep` floats of the chunk behind the margin
        return buf

    def restate(self, j):
        return [self.expect(j)]

    def flow(self, run, jobs):
        for j in jobs:
            same_bits(run(j)[0], self.expect(j), "roll_history %r" % (j["c"],))

    def jobs(self):
        return [self.make(c) for c in self.CASES]


def roll_pool(key, B, Tal, ffs):
    """The tensors of a RollDesc table in one pool, 4 or 5 floats apart (float4 tensors stay 16-byte aligned)."""
    offs, at = [], 4
    for ff in ffs:
        if ff % 4 == 0:
            at = -(-at // 4) * 4
        offs.append(at)
        at += B * Tal * ff + 5
    return noise_bits(key, at), offs


def align16(n):
    return -(-n // 16) * 16


class RollHistoryRows:
    op = "roll_history_rows"
    HIST = 4
    CASES = ([dict(B=4, chunk=4, ffs=[8, 6, 12], mode=[1, 0, 2, 1], take=None),
              dict(B=4, chunk=4, ffs=[8, 6, 12], mode=[1, 0, 2, 1], take=[4, 1, 1, 2]),
              dict(B=4, chunk=7, ffs=[8, 6, 12], mode=[1, 0, 2, 1], take=None)] +
             [dict(B=4, chunk=7, ffs=[8, 6, 12], mode=[1, 0, 2, 1], take=[7, 3, 3, tk]) for tk in (-3, 0, 1, 2, 3, 4, 5, 7, 12)] +
             [dict(B=1, chunk=7, ffs=[8, 6, 16392], mode=[1], take=[3]), dict(B=1, chunk=7, ffs=[8, 6, 16392], mode=[1], take=None),
              dict(B=1, chunk=7, ffs=[8, 6, 16392], mode=[2], take=None),
              dict(B=4, chunk=7, ffs=[8, 6, 12], mode=None, take=None, only_row=2)])

    def make(self, c):
        B, chunk, ffs = c["B"], c["chunk"], c["ffs"]
        Tal = self.HIST + chunk
        pool, offs = roll_pool(("rows", B, chunk, tuple(ffs)), B, Tal, ffs)
        desc = np.array([[o, ff, 0] for o, ff in zip(offs, ffs)], np.int64)
        mode = None if c["mode"] is None else np.array(c["mode"], np.int32)
        take = None if c["take"] is None else np.array(c["take"], np.int32)
        return job(self.op, [B, Tal, self.HIST, chunk, len(ffs), c.get("only_row", -1)], [], [desc, mode, take],
                   [pool, np.full(B, 7, np.int32)], c=c, offs=offs, Tal=Tal)

    def rows(self, j):
        c = j["c"]
        for b in range(c["B"]):
            m = c["mode"][b] if c["mode"] is not None else (2 if b == c["only_row"] else 0)
            tk = c["chunk"] if (c["take"] is None or m != 1) else min(max(c["take"][b], 0), c["chunk"])
            if m != 0 and tk != 0:
                yield b, m, tk

    def expect(self, j):
        """The new margin: the last `hist` frames of [old margin ++ the tk frames written] = frames [tk, tk + hist) of the row."""
        c, pool = j["c"], j["ios"][0].copy()
        for o, ff in zip(j["offs"], c["ffs"]):
            for b, m, tk in self.rows(j):
                row = o + b * j["Tal"] * ff
                old = j["ios"][0][row:row + j["Tal"] * ff]
                pool[row:row + self.HIST * ff] = 0.0 if m == 2 else old[tk * ff:(tk + self.HIST) * ff]
        nf = j["ios"][1].copy()
        if c["mode"] is None:
            nf[c["only_row"]] = 0
        return pool, nf

    def restate(self, j):
        """The kernel's walk: element i of the margin takes element i + from, front to back, in place."""
        c, pool = j["c"], j["ios"][0].copy()
        for o, ff in zip(j["offs"], c["ffs"]):
            for b, m, tk in self.rows(j):
                row = pool[o + b * j["Tal"] * ff:]
                keep, frm = self.HIST * ff, tk * ff
                if m != 1:
                    row[:keep] = 0.0
                else:
                    for s in range(0, keep, frm):                      # residue chains j, j + from, ...: blockwise the same order
                        n = min(frm, keep - s)
                        row[s:s + n] = row[s + frm:s + frm + n].copy()
        return [pool, self.expect(j)[1]]

    def flow(self, run, jobs):
        for j in jobs:
            pool, nf = run(j)
            want, wnf = self.expect(j)
            same_bits(pool, want, "roll_history_rows %r" % (j["c"],))
            assert np.array_equal(nf, wnf), "roll_history_rows: nonfinite %r, expected %r" % (nf, wnf)

    def jobs(self):
        return [self.make(c) for c in self.CASES]


class HistoryStateRows:
    op = "history_state_rows"
    B, HIST, CHUNK, FFS = 4, 3, 5, [8, 6, 10]            # 32-byte frames: the 16-byte path; 24 and 40 bytes: the 4-byte path

    def layout(self):
        offs, at = [], 16
        for ff in self.FFS:
            offs.append(at)
            at = align16(at + self.HIST * ff * 4) + 16    # padding up to 16 bytes, and a 16-byte gap
        return offs, at

    def make(self, load, src_blob=None):
        Tal = self.HIST + self.CHUNK
        pool, offs = roll_pool(("state", load), self.B, Tal, self.FFS)
        so, total = self.layout()
        desc = np.array([[o, ff, s] for o, ff, s in zip(offs, self.FFS, so)], np.int64)
        blob = sent(total // 4) if src_blob is None else src_blob
        row = 3 if load else 1
        return job(self.op, [self.B, Tal, self.HIST, len(self.FFS), row, load], [], [desc], [pool, blob, np.full(self.B, 7, np.int32)],
                   offs=offs, so=so, Tal=Tal, row=row, load=load)

    def expect(self, j):
        pool, blob, nf = (a.copy() for a in j["ios"])
        for o, ff, s in zip(j["offs"], self.FFS, j["so"]):
            m = slice(o + j["row"] * j["Tal"] * ff, o + j["row"] * j["Tal"] * ff + self.HIST * ff)
            bl = slice(s // 4, s // 4 + self.HIST * ff)
            if j["load"]:
                pool[m] = blob[bl]
            else:
                blob[bl] = pool[m]
        if j["load"]:
            nf[j["row"]] = 0
        return [pool, blob, nf]

    def restate(self, j):
        return self.expect(j)

    def flow(self, run, jobs):
        save = jobs[0]
        got = run(save)
        for a, b, what in zip(got, self.expect(save), ("pool", "blob", "nonfinite")):
            same_bits(a, b, "history_state_rows save: " + what)               # (the blob's padding keeps the sentinel)
        assert is_sent(got[1]).sum() == got[1].size - sum(self.HIST * ff for ff in self.FFS)
        load = self.make(1, got[1])
        got2 = run(load)
        for a, b, what in zip(got2, self.expect(load), ("pool", "blob", "nonfinite")):
            same_bits(a, b, "history_state_rows load: " + what)
        assert list(got2[2]) == [7, 7, 7, 0]

    def jobs(self):
        return [self.make(0), self.make(1, self.expect(self.make(0))[1])]


class StreamTakeChunk:
    op = "stream_take_chunk"
    #        latent, off, take, front frames
    CASES = [(4, [0, 2, 1], [3, 0, 2], 6), (128, [0, 2, 1], [3, 0, 2], 6), (1024, [3, 2, 0], [3, 0, 1], 6), (1024, [1], [70], 72)]

    def make(self, c):
        latent, off, take, nf = c
        B, mt = len(off), max(take)
        fbs, lat_off = nf * latent + 8, 2 * latent
        lbs = lat_off + (mt + 1) * latent
        return job(self.op, [B, fbs, lbs, latent, mt, lat_off], [],
                   [noise_bits(("front", c[0], B), B * fbs).reshape(B, fbs), np.array(off, np.int32), np.array(take, np.int32)],
                   [noise_bits(("lat", c[0], B), B * lbs).reshape(B, lbs)], c=c, lat_off=lat_off)

    def expect(self, j):
        latent, off, take, _ = j["c"]
        lat = j["ios"][0].copy()
        for b in range(len(off)):
            lat[b, j["lat_off"]:j["lat_off"] + take[b] * latent] = j["ins"][0][b, off[b] * latent:(off[b] + take[b]) * latent]
        return lat

    def restate(self, j):
        return [self.expect(j)]

    def flow(self, run, jobs):
        for j in jobs:
            same_bits(run(j)[0], self.expect(j), "stream_take_chunk %r" % (j["c"][:3],))

    def jobs(self):
        return [self.make(c) for c in self.CASES]


# ---------------------------------------------------------------------------------------------
# voice-clone front end
# ---------------------------------------------------------------------------------------------
def audio_of(seed, n=1024):
    return (rng_of("audio", seed).standard_normal(n) * 0.3).astype(F32)


class EncInitConv:
    op = "enc_init_conv"
    #    S, K, C, clips (seed, first sample)
    CASES = [dict(S=1, K=1, C=8, clips=[(1, 0)]), dict(S=255, K=7, C=64, clips=[(1, 0)]), dict(S=256, K=17, C=8, clips=[(1, 0)]),
             dict(S=257, K=7, C=8, clips=[(1, 0)]),
             dict(S=600, K=17, C=64, clips=[(1, 0), (2, 0)], key="batch"), dict(S=600, K=17, C=64, clips=[(2, 0)], key="alone"),
             dict(S=400, K=17, C=64, clips=[(2, 200)], key="shifted")]

    def make(self, c):
        S, K, C, B = c["S"], c["K"], c["C"], len(c["clips"])
        audio = np.stack([audio_of(seed)[s0:s0 + S] for seed, s0 in c["clips"]])
        w = (rng_of("enc-w", K, C).standard_normal((C, K)) / np.sqrt(K)).astype(F32)
        bias = vecf("enc-b", C, 0.3)
        obs = S * C + 8
        return job(self.op, [B, S, C, K, obs], [], [audio, w, bias], [sent((B, obs))], c=c)

    def windows(self, j, dtype):
        audio = j["ins"][0]
        B, S = audio.shape
        K = j["c"]["K"]
        pad = np.concatenate([np.zeros((B, K - 1), dtype), audio.astype(dtype)], 1)
        return np.stack([pad[:, k:k + S] for k in range(K)], -1)       # [B][S][K]: audio[t - (K - 1) + k]

    def restate(self, j):
        _, w, bias = j["ins"]
        c = j["c"]
        xs = self.windows(j, F32)
        acc = np.zeros(xs.shape[:2] + (c["C"],), F32)
        for k in range(c["K"]):
            acc = acc + w[:, k] * xs[:, :, k, None]
        out = j["ios"][0].copy()
        out[:, :c["S"] * c["C"]] = (acc + bias).reshape(xs.shape[0], -1)
        return [out]

    def verify(self, j, got):
        _, w, bias = j["ins"]
        c = j["c"]
        xs = self.windows(j, np.float64)
        prod = xs[:, :, None, :] * w.astype(np.float64)                # [B][S][C][K]
        ref = prod.sum(-1) + bias.astype(np.float64)
        bar = (c["K"] + 2) * E * (np.abs(prod).sum(-1) + np.abs(bias.astype(np.float64)))
        n = c["S"] * c["C"]
        within(self.op, got[:, :n].reshape(ref.shape), ref, bar, "out %r" % (c,))
        untouched(got[:, n:], self.op)

    def flow(self, run, jobs):
        res = {}
        for j in jobs:
            got = run(j)[0]
            self.verify(j, got)
            res[j["c"].get("key")] = got
        n = 600 * 64
        same_bits(res["batch"][1, :n], res["alone"][0, :n], "enc_init_conv: row 1 of a batch against the clip alone")
        # samples 216 .. 599 of the clip: in the 600-sample run they straddle the block edges at 256 and 512, in the shifted
        # run (the clip from sample 200 on) they sit at 16 .. 399, the edge elsewhere; behind the first K - 1 outputs both see
        # the same 17 samples
        same_bits(res["alone"][0, 216 * 64:n], res["shifted"][0, 16 * 64:400 * 64], "enc_init_conv: across the 256-sample block edge")

    def jobs(self):
        return [self.make(c) for c in self.CASES]


class LayerNorm:
    op = "layernorm_f32"
    EPS = 1e-5
    CASES = [dict(C=1), dict(C=128), dict(C=260, key="batch"), dict(C=512), dict(C=260, bigmean=True), dict(C=260, B=1, key="alone")]

    def make(self, c):
        C, B, T = c["C"], c.get("B", 2), 3
        xbs, obs = T * C + 4, T * C + 8
        x = sent((B, xbs))
        for b in range(B):
            x[b, :T * C] = (seq_rows(("ln", b), C)[:T] + F32(100.0 if c.get("bigmean") else 0.0)).ravel()   # |mean| >> std
        return job(self.op, [B, T, C, xbs, obs], [self.EPS], [x, vecf("ln-w", C, 0.5, 1.0), vecf("ln-b", C, 0.3)], [sent((B, obs))], c=c, T=T, B=B)

    def restate(self, j):
        x, w, b = j["ins"]
        C, T, B = j["c"]["C"], j["T"], j["B"]
        out = j["ios"][0].copy()
        out[:, :T * C] = ln_restate(x[:, :T * C].reshape(B, T, C), w, b, self.EPS).reshape(B, -1)
        return [out]

    def verify(self, j, got):
        x, w, b = j["ins"]
        C, T, B = j["c"]["C"], j["T"], j["B"]
        y = x[:, :T * C].reshape(B, T, C).astype(np.float64)
        ref, bar = ln_ref_bar(y, np.zeros_like(y), w, b, self.EPS)
        within(self.op, got[:, :T * C].reshape(B, T, C), ref, bar, "out %r" % (j["c"],))
        untouched(got[:, T * C:], self.op)

    def flow(self, run, jobs):
        res = {}
        for j in jobs:
            got = run(j)[0]
            self.verify(j, got)
            res[j["c"].get("key")] = got
        same_bits(res["batch"][0, :780], res["alone"][0, :780], "layernorm_f32: row 0 of a batch against the row alone")

    def jobs(self):
        return [self.make(c) for c in self.CASES]


class RopeQk:
    op = "rope_qk_f32"
    CASES = [(1, 1), (3, 5), (3, 130), (1, 130)]      # heads, T

    def make(self, c):
        heads, T = c
        ang = np.arange(T)[:, None] * (10000.0 ** (-np.arange(32) / 32.0))[None, :]
        cos_t, sin_t = np.cos(ang).astype(F32), np.sin(ang).astype(F32)
        qkv = (rng_of("rope", c).standard_normal((2, T, 3 * heads * 64))).astype(F32)
        return job(self.op, [2, T, heads], [], [cos_t, sin_t], [qkv], c=c)

    def halves(self, j, dtype):
        heads, T = j["c"]
        x = j["ios"][0][:, :, :2 * heads * 64].reshape(2, T, 2 * heads, 2, 32).astype(dtype)
        return x[:, :, :, 0], x[:, :, :, 1], j["ins"][0].astype(dtype)[None, :, None, :], j["ins"][1].astype(dtype)[None, :, None, :]

    def restate(self, j):
        heads, T = j["c"]
        x1, x2, c, s = self.halves(j, F32)
        out = j["ios"][0].copy()
        out[:, :, :2 * heads * 64] = np.stack([x1 * c - x2 * s, x1 * s + x2 * c], 3).reshape(2, T, -1)
        return [out]

    def flow(self, run, jobs):
        for j in jobs:
            heads, T = j["c"]
            got = run(j)[0]
            x1, x2, c, s = self.halves(j, np.float64)
            ref = np.stack([x1 * c - x2 * s, x1 * s + x2 * c], 3)
            bar = 2 * E * np.stack([np.abs(x1 * c) + np.abs(x2 * s), np.abs(x1 * s) + np.abs(x2 * c)], 3)
            within(self.op, got[:, :, :2 * heads * 64].reshape(ref.shape), ref, bar, "q, k %r" % (j["c"],))
            same_bits(got[:, :, 2 * heads * 64:], j["ios"][0][:, :, 2 * heads * 64:], "rope_qk_f32: the v third")

    def jobs(self):
        return [self.make(c) for c in self.CASES]


class AttnCausal:
    op = "attn_causal_f32"
    HEADS, B = 3, 2
    TS = [1, 63, 64, 65, 130]

    def make(self, T, scramble_from=None):
        qkv = np.stack([attn_rows(("causal", b), 130, self.HEADS, True)[:T] for b in range(self.B)])
        if scramble_from is not None:        # other finite keys and values at positions >= scramble_from
            n = self.HEADS * 64
            qkv[:, scramble_from:, n:] = rng_of("scramble", T).standard_normal((self.B, T - scramble_from, 2 * n)).astype(F32) * 3
        return job(self.op, [self.B, T, self.HEADS], [], [qkv], [sent((self.B, T, self.HEADS * 64))], T=T)

    def restate(self, j):
        return [np.stack([attn_restate(q, self.HEADS, True) for q in j["ins"][0]])]

    def flow(self, run, jobs):
        res = {}
        for j in jobs:
            T = j["T"]
            got = run(j)[0]
            if len(res) < len(self.TS):
                for b in range(self.B):
                    ref, bar = attn_ref_bar(j["ins"][0][b], self.HEADS, True)
                    within(self.op, got[b], ref, bar, "out T=%d" % T)
                res[T] = got
            else:                                # the scrambled runs: queries in front of the scrambled positions do not move
                assert np.isfinite(got).all()
                j0 = (T + 1) // 2
                same_bits(got[:, :j0], res[T][:, :j0], "attn_causal_f32: keys / values behind a query moved its output (T=%d)" % T)
        for T in self.TS[:-1]:
            same_bits(res[130][:, :T], res[T], "attn_causal_f32: rows [0, %d) of a 130-long run against a %d-long run" % (T, T))

    def jobs(self):
        return [self.make(T) for T in self.TS] + [self.make(T, (T + 1) // 2) for T in self.TS[1:]]


class RvqEncode:
    op = "rvq_encode"
    T = 6
    PAIRS = [(3, 259), (70, 700), (5, 1029)]   # one thread in two add chains, two waves, two 1024-bin blocks
    CASES = [dict(dim=5, bins=128, L=1, l0=0), dict(dim=8, bins=1000, L=3, l0=1), dict(dim=12, bins=1024, L=3, l0=0, wide=True),
             dict(dim=64, bins=1025, L=15, l0=1), dict(dim=256, bins=2048, L=3, l0=0, wide=True, key="batch"),
             dict(dim=256, bins=2048, L=3, l0=0, wide=True, B=1, key="alone"),
             dict(dim=64, bins=1025, L=15, l0=0, nan=True)]

    def make(self, c):
        dim, bins, L, l0, B, T = c["dim"], c["bins"], c["L"], c["l0"], c.get("B", 2), self.T
        r = rng_of("rvq", dim, bins, L)
        emb = r.standard_normal((L, bins, dim)).astype(F32)
        pairs = [(a, b) for a, b in self.PAIRS if b < bins]
        for a, b in pairs:
            emb[:, b] = emb[:, a]                                        # duplicate rows with equal c2: exact ties
        c2 = ((emb.astype(np.float64) ** 2).sum(-1).astype(F32) / F32(2)).astype(F32)
        if pairs:
            a, b = pairs[-1]                                             # behind a frame that sat on a row the residual is 0 and
            c2[1:, [a, b]] = c2[1:].min(-1, keepdims=True) - F32(1)      # the distance is c2: the tie decides the next layer too
        ldx, xcol = (2 * dim, dim) if c.get("wide") else (dim, 0)
        valid = np.array([T, T - 2][:B], np.int32)
        xbs = T * ldx + 4
        x = sent((B, xbs))
        for b in range(B):
            rows = sent((T, ldx))
            fr = rng_of("rvq-x", b, dim).standard_normal((T, dim)).astype(F32) * F32(1.5)
            for i, (a, _) in enumerate(pairs):
                fr[i + 1] = emb[0, a]                                    # a frame exactly on a duplicated row
            if c.get("nan"):
                fr[4] = np.nan                                           # (row 0 only: row 1 has four frames)
            rows[:valid[b], xcol:xcol + dim] = fr[:valid[b]]
            x[b, :T * ldx] = rows.ravel()
        n_own = (l0 + L) * valid
        code_off = np.array([3, 3 + n_own[0] + 5][:B], np.int64)         # ranges apart, with sentinels around them
        codes = sent(int(code_off[-1] + n_own[B - 1] + 4), np.int32)
        cpool, c2pool = sent(L * (bins * dim + 4) + 4), sent(L * (bins + 4) + 4)
        cb_off = np.array([4 + (L - 1 - k) * (bins * dim + 4) for k in range(L)], np.int64)
        c2_off = np.array([4 + k * (bins + 4) for k in range(L)], np.int64)
        for k in range(L):
            cpool[cb_off[k]:cb_off[k] + bins * dim] = emb[k].ravel()
            c2pool[c2_off[k]:c2_off[k] + bins] = c2[k]
        return job(self.op, [B, T, ldx, xbs, dim, bins, L, l0, xcol], [], [x, valid, code_off, cpool, c2pool, cb_off, c2_off], [codes],
                   c=c, emb=emb, c2=c2, pairs=pairs, ldx=ldx, xcol=xcol, B=B)

    def search(self, j, dtype):
        """Per batch row: codes [L][valid] and the distance table of every layer. float32: the kernel's walk -- separate multiply
        and add, dimensions in order, c2 - dot, lowest index on ties (argmin's rule; an all-NaN row gives 0), r - emb."""
        c, emb, c2 = j["c"], j["emb"].astype(dtype), j["c2"].astype(dtype)
        res = []
        for b in range(j["B"]):
            T = int(j["ins"][1][b])
            r = j["ins"][0][b, :self.T * j["ldx"]].reshape(self.T, j["ldx"])[:T, j["xcol"]:j["xcol"] + c["dim"]].astype(dtype)
            codes, dists = [], []
            with np.errstate(invalid="ignore"):
                for k in range(c["L"]):
                    dot = np.zeros((T, c["bins"]), dtype)
                    for d in range(c["dim"]):
                        dot = dot + r[:, d, None] * emb[k, :, d]
                    dist = c2[k] - dot
                    idx = np.where(np.isnan(dist).all(1), 0, np.argmin(np.where(np.isnan(dist), np.inf, dist), 1))
                    r = r - emb[k, idx]
                    codes.append(idx.astype(np.int32))
                    dists.append(dist)
            res.append((np.stack(codes), dists))
        return res

    def expect(self, j):
        codes = j["ios"][0].copy()
        for b, (cd, _) in enumerate(self.search(j, F32)):
            T, off = int(j["ins"][1][b]), int(j["ins"][2][b])
            for k in range(j["c"]["L"]):
                at = off + (j["c"]["l0"] + k) * T
                codes[at:at + T] = cd[k]
        return codes

    def restate(self, j):
        return [self.expect(j)]

    def flow(self, run, jobs):
        res = {}
        for j in jobs:
            c = j["c"]
            got = run(j)[0]
            same_bits(got, self.expect(j), "rvq_encode %r" % (c,))          # padding frames and everything outside the ranges: sentinel
            res[c.get("key")] = (j, got)
            off, T = int(j["ins"][2][0]), self.T
            first = got[off + c["l0"] * T:off + (c["l0"] + 1) * T]
            for i, (a, twin) in enumerate(j["pairs"]):
                assert first[i + 1] == a, "rvq_encode: the lower index of the tie (%d, %d) must win" % (a, twin)
            if j["pairs"] and c["L"] > 1:
                second = got[off + (c["l0"] + 1) * T:off + (c["l0"] + 2) * T]
                assert (second[1:1 + len(j["pairs"])] == j["pairs"][-1][0]).all(), "rvq_encode: the tie of the next layer"
            if c.get("nan"):
                for b in range(j["B"]):
                    Tb, ob = int(j["ins"][1][b]), int(j["ins"][2][b])
                    own = got[ob:ob + (c["l0"] + c["L"]) * Tb].reshape(-1, Tb)
                    assert Tb <= 4 or (own[:, 4] == 0).all(), "rvq_encode: a frame without a finite distance takes bin 0 on every layer"
        (jb, gb), (ja, ga) = res["batch"], res["alone"]
        ob, oa, n = int(jb["ins"][2][0]), int(ja["ins"][2][0]), 3 * self.T
        same_bits(gb[ob:ob + n], ga[oa:oa + n], "rvq_encode: row 0 of a batch against the row alone")

    def jobs(self):
        return [self.make(c) for c in self.CASES]


class LogMel:
    op = "log_mel"
    CASES = [(5, 3, 12), (513, 128, 1030), (513, 130, 1026)]       # nfreq, n_mels, ld
    FLOOR = float(F32(1e-10))

    def make(self, c):
        nfreq, n_mels, ld = c
        T = 3
        r = rng_of("mel", c)
        spec = sent((T, ld))
        spec[:, :2 * nfreq] = (r.standard_normal((T, 2 * nfreq)) * 2.0 ** r.integers(-6, 3, (T, 2 * nfreq))).astype(F32)
        spec[1, :2 * nfreq] = 0.0                                    # an all-zero frame: log(1e-10)
        fb = np.maximum(r.standard_normal((nfreq, n_mels)), 0.0).astype(F32) * F32(0.01)
        return job(self.op, [T, ld, nfreq, n_mels], [], [spec, fb], [sent((T, n_mels))], c=c)

    def restate(self, j):
        nfreq, n_mels, _ = j["c"]
        spec, fb = j["ins"]
        re, im = spec[:, :nfreq], spec[:, nfreq:2 * nfreq]
        mag = np.sqrt(re * re + im * im)
        pw = mag * mag
        acc = np.zeros((spec.shape[0], n_mels), F32)
        for k in range(nfreq):
            acc = acc + pw[:, k, None] * fb[k]
        return [np.log(np.maximum(acc, F32(1e-10)))]

    def flow(self, run, jobs):
        for j in jobs:
            nfreq, n_mels, _ = j["c"]
            spec, fb = (a.astype(np.float64) for a in j["ins"])
            pw = spec[:, :nfreq] ** 2 + spec[:, nfreq:2 * nfreq] ** 2
            ref = np.log(np.maximum(pw @ fb, self.FLOOR))
            got = run(j)[0]
            within(self.op, got, ref, (nfreq + 6) * E + 2 * E * np.abs(ref), "log-mel %r" % (j["c"],))
            assert (bits(got[1]) == bits(got[1])[0]).all()      # the all-zero frame: logf(1e-10f) in every bin, held to the bar above

    def jobs(self):
        return [self.make(c) for c in self.CASES]


class TimeStats:
    op = "time_stats"
    CASES = [(1, 1, True), (3, 64, True), (4, 65, True), (5, 384, True), (130, 65, True), (130, 384, False), (130, 384, True)]   # T, C, std

    def make(self, c):
        T, C, std = c
        ld = C + 3
        x = sent((T, ld))
        x[:, :C] = seq_rows("ts", C, 130)[:T] * vecf("ts-s", C, 1.0, 0.0) + vecf("ts-m", C, 2.0)
        eps = 1e-12 if std else 0.0
        return job(self.op, [T, C, ld], [eps], [x], [sent(C), sent(C) if std else None], c=c, eps=eps)

    def restate(self, j):
        T, C, std = j["c"]
        x = j["ins"][0][:, :C]

        def sliced(v):
            parts = []
            for p in range(4):
                s = np.zeros(C, F32)
                for t in range(p, T, 4):
                    s = s + v[t]
                parts.append(s)
            return ((parts[0] + parts[1]) + parts[2]) + parts[3]
        mu = sliced(x) / F32(T)
        if not std:
            return [mu, None]
        d = x - mu
        return [mu, np.sqrt(sliced(d * d) / F32(T) + F32(j["eps"]))]

    def flow(self, run, jobs):
        for j in jobs:
            T, C, std = j["c"]
            x = j["ins"][0][:, :C].astype(np.float64)
            got = run(j)
            mu = x.mean(0)
            Em = E * np.abs(x).sum(0) + E * np.abs(mu)
            within(self.op, got[0], mu, Em, "mean %r" % (j["c"],))
            if std:
                eps = float(F32(j["eps"]))
                d = x - mu
                Ed = Em + E * np.abs(d)
                var = (d * d).mean(0)
                Ev = ((2 * np.abs(d) * Ed + Ed * Ed + E * d * d).sum(0) + T * E * (d * d).sum(0)) / T + E * var
                sd = np.sqrt(var + eps)
                within(self.op, got[1], sd, (Ev + E * (var + eps)) / (2 * sd) + E * sd, "std %r" % (j["c"],))
            else:
                assert got[1] is None

    def jobs(self):
        return [self.make(c) for c in self.CASES]


class ScaleRes:
    op = "scale_res"
    CASES = [(3, 5), (3, 384)]

    def make(self, c):
        T, C = c
        x, res = sent((T, C + 1)), sent((T, C + 2))
        x[:, :C], res[:, :C] = seq_rows("sr-x", C)[:T], seq_rows("sr-r", C)[:T]
        return job(self.op, [T, C, C + 1, C + 2, C + 3], [], [x, vecf("sr-se", C), res], [sent((T, C + 3))], c=c)

    def restate(self, j):
        T, C = j["c"]
        x, se, res = j["ins"]
        out = j["ios"][0].copy()
        out[:, :C] = x[:, :C] * se + res[:, :C]
        return [out]

    def flow(self, run, jobs):
        for j in jobs:
            T, C = j["c"]
            x, se, res = (a.astype(np.float64) for a in j["ins"])
            got = run(j)[0]
            pr = x[:, :C] * se
            within(self.op, got[:, :C], pr + res[:, :C], E * np.abs(pr) + E * (np.abs(pr) + np.abs(res[:, :C])), "out")
            untouched(got[:, C:], self.op)

    def jobs(self):
        return [self.make(c) for c in self.CASES]


class AspConcat:
    op = "asp_concat"
    CASES = [(3, 5), (3, 384)]

    def make(self, c):
        T, C = c
        return job(self.op, [T, C], [], [seq_rows("ac", C)[:T], vecf("ac-m", C), vecf("ac-s", C)], [sent((T, 3 * C))], c=c)

    def expect(self, j):
        x, mean, std = j["ins"]
        return np.concatenate([x, np.tile(mean, (x.shape[0], 1)), np.tile(std, (x.shape[0], 1))], 1)

    def restate(self, j):
        return [self.expect(j)]

    def flow(self, run, jobs):
        for j in jobs:
            same_bits(run(j)[0], self.expect(j), "asp_concat %r" % (j["c"],))

    def jobs(self):
        return [self.make(c) for c in self.CASES]


class Copy2d:
    op = "copy2d_f32"
    CASES = [(3, 5), (3, 384)]

    def make(self, c):
        T, C = c
        src = sent((T, C + 1))
        src[:, :C] = seq_rows("cp", C)[:T]
        return job(self.op, [T, C, C + 1, C + 2], [], [src], [sent((T, C + 2))], c=c)

    def expect(self, j):
        T, C = j["c"]
        out = j["ios"][0].copy()
        out[:, :C] = j["ins"][0][:, :C]
        return out

    def restate(self, j):
        return [self.expect(j)]

    def flow(self, run, jobs):
        for j in jobs:
            same_bits(run(j)[0], self.expect(j), "copy2d_f32 %r" % (j["c"],))

    def jobs(self):
        return [self.make(c) for c in self.CASES]


class AspPool:
    op = "asp_pool"
    EPS = 1e-12
    CASES = [(1, 1), (2, 64), (130, 65), (130, 200)]

    def make(self, c):
        T, C = c
        att = rng_of("asp", c).uniform(-30, 30, (T, C)).astype(F32)
        x = seq_rows("asp-x", C, 130)[:T].copy()
        x[:, 0] = 1.5                                                  # a constant channel: the max(var, eps) clamp decides
        return job(self.op, [T, C], [self.EPS], [att, x], [sent(2 * C)], c=c)

    def restate(self, j):
        T, C = j["c"]
        att, x = j["ins"]
        a = att - att.max(0)
        s = np.zeros(C, F32)
        for t in range(T):
            s = s + np.exp(a[t])
        mean = np.zeros(C, F32)
        for t in range(T):
            mean = mean + (np.exp(a[t]) / s) * x[t]
        var = np.zeros(C, F32)
        for t in range(T):
            d = x[t] - mean
            var = var + (np.exp(a[t]) / s) * (d * d)
        return [np.concatenate([mean, np.sqrt(np.maximum(var, F32(self.EPS)))])]

    def flow(self, run, jobs):
        for j in jobs:
            T, C = j["c"]
            att, x = (v.astype(np.float64) for v in j["ins"])
            got = run(j)[0]
            a = att - att.max(0)
            w = np.exp(a)
            w /= w.sum(0)
            Rs = (T + np.abs(a).max(0) + 2) * E
            Rw = (np.abs(a) + 3) * E + Rs
            mean = (w * x).sum(0)
            Em = (np.abs(w * x) * (Rw + E)).sum(0) + T * E * np.abs(w * x).sum(0)
            within(self.op, got[:C], mean, Em, "mean %r" % (j["c"],))
            d = x - mean
            Ed = Em + E * np.abs(d)
            var = (w * d * d).sum(0)
            Ev = (w * ((2 * np.abs(d) * Ed + Ed * Ed + E * d * d) + d * d * (Rw + E))).sum(0) + T * E * var
            eps = float(F32(self.EPS))
            sd = np.sqrt(np.maximum(var, eps))
            within(self.op, got[C:], sd, np.minimum(Ev / sd, np.sqrt(Ev)) + E * sd, "std %r" % (j["c"],))

    def jobs(self):
        return [self.make(c) for c in self.CASES]


class MaskTail:
    op = "mask_tail"
    CASES = [(4, 5, 24, [4, 0, 3]), (1100, 256, 1100 * 256 + 4, [7])]    # Tpad, C, bstride, valid

    def make(self, c):
        Tpad, C, bs, valid = c
        return job(self.op, [len(valid), Tpad, C, bs], [], [np.array(valid, np.int32)], [noise_bits(("mask", Tpad), len(valid) * bs).reshape(-1, bs)], c=c)

    def expect(self, j):
        Tpad, C, bs, valid = j["c"]
        x = j["ios"][0].copy()
        for b, v in enumerate(valid):
            x[b, v * C:Tpad * C] = 0.0
        return x

    def restate(self, j):
        return [self.expect(j)]

    def flow(self, run, jobs):
        for j in jobs:
            same_bits(run(j)[0], self.expect(j), "mask_tail %r" % (j["c"][:2],))

    def jobs(self):
        return [self.make(c) for c in self.CASES]


OPS = [RvqGather(), RmsNorm(), DwconvLn(), SiluMul(), AttnFull(), RollHistory(), RollHistoryRows(), HistoryStateRows(), StreamTakeChunk(),
       EncInitConv(), LayerNorm(), RopeQk(), AttnCausal(), RvqEncode(), LogMel(), TimeStats(), ScaleRes(), AspConcat(), AspPool(), MaskTail(),
       Copy2d()]
BY_NAME = {o.op: o for o in OPS}
_JOBS = {}


def jobs_of(o):
    if o.op not in _JOBS:
        _JOBS[o.op] = o.jobs()
    return _JOBS[o.op]


def check_only(j):
    from qwen3tts import _lib
    return _lib.rowop(None, j["op"], j["p"], j["f"], j["ins"], [None if v is None else v.copy() for v in j["ios"]], check_only=True)


# ---------------------------------------------------------------------------------------------
# CPU part
# ---------------------------------------------------------------------------------------------
def test_every_launcher_has_a_flow():
    from qwen3tts import _lib
    assert {o.op for o in OPS} == set(_lib.ROWOPS) and len(_lib.ROWOPS) == len(OPS) == 21


@pytest.mark.parametrize("op", [o.op for o in OPS])
def test_case_table_is_launchable(op):
    """Every job of the table passes the hook's host checks (check_only: no model, no GPU): what the GPU part launches is what the
    launchers' conditions admit."""
    for j in jobs_of(BY_NAME[op]):
        assert check_only(j) == 0, "%s: the host checks refuse %r" % (op, j["p"])


@pytest.mark.parametrize("op", [o.op for o in OPS])
def test_restated_walk_stays_inside_the_bars(op):
    """The float32 restatement of the kernel's walk through the flow the GPU results get: the float64 reference under the same
    bars, the sentinels, the bit-exact claims."""
    o = BY_NAME[op]
    WORST.pop(op, None)
    o.flow(lambda j: o.restate(j), jobs_of(o))
    print("restatement, worst error / bar: %s %.4f" % (op, WORST.get(op, 0.0)))


def test_rvq_encode_pick_is_the_float64_minimum_within_the_order_error():
    """The restated search against float64: the distance of its pick lies within twice (dim + 2) e (sum |r emb| + |c2|) of the
    float64 minimum, layer 0 of every finite frame (behind a differing pick the residuals part ways)."""
    o = BY_NAME["rvq_encode"]
    for j in jobs_of(o):
        c = j["c"]
        emb, c2 = j["emb"][0].astype(np.float64), j["c2"][0].astype(np.float64)
        for b, (cd, _) in enumerate(o.search(j, F32)):
            T = int(j["ins"][1][b])
            r = j["ins"][0][b, :o.T * j["ldx"]].reshape(o.T, j["ldx"])[:T, j["xcol"]:j["xcol"] + c["dim"]].astype(np.float64)
            ok = np.isfinite(r).all(1)
            dist = c2 - r[ok] @ emb.T
            bar = (c["dim"] + 2) * E * (np.abs(r[ok]) @ np.abs(emb).T + np.abs(c2))
            pick = cd[0][ok]
            rows = np.arange(pick.size)
            assert (dist[rows, pick] - dist.min(1) <= bar[rows, pick] + bar[rows, dist.argmin(1)]).all()


def mutate(j, p=None, ins=None, ios=None):
    j = dict(j, p=list(j["p"]), ins=list(j["ins"]) + [None] * (8 - len(j["ins"])), ios=list(j["ios"]))
    for k, v in (p or {}).items():
        j["p"][k] = v
    for k, v in (ins or {}).items():
        j["ins"][k] = v
    for k, v in (ios or {}).items():
        j["ios"][k] = v
    return j


def i32(*v):
    return np.array(v, np.int32)


def i64(*v):
    return np.array(v, np.int64)


# name -> (op, job index, what to change): one per condition the hook states
REFUSED = {
    "size-against-counts": ("rmsnorm_f32", 1, lambda j: mutate(j, ins={0: j["ins"][0][:, :-1].copy()})),
    "size-of-an-output": ("copy2d_f32", 0, lambda j: mutate(j, ios={0: sent(3 * 7 - 1)})),
    "unnamed-slot": ("copy2d_f32", 0, lambda j: mutate(j, ins={1: sent(4)})),
    "unknown-op": ("copy2d_f32", 0, lambda j: dict(j, op=None)),
    "frames-over-Tmax": ("rmsnorm_f32", 1, lambda j: mutate(j, ins={2: i32(5)})),
    "frames-negative": ("attn_full_f32", 0, lambda j: mutate(j, ins={1: i32(-1)})),
    "dwconv-C-4097": ("dwconv_ln", 0, lambda j: mutate(j, p={3: 4097})),
    "dwconv-hist-over-margin": ("dwconv_ln", 1, lambda j: mutate(j, p={4: 4})),
    "dwconv-margin-plus-frames": ("dwconv_ln", 1, lambda j: mutate(j, ins={5: i32(7)})),
    "enc-K-18": ("enc_init_conv", 2, lambda j: mutate(j, p={3: 18})),
    "enc-out-bstride": ("enc_init_conv", 2, lambda j: mutate(j, p={4: 256 * 8 - 1})),
    "rvq-dim-4097": ("rvq_encode", 0, lambda j: mutate(j, p={4: 4097})),
    "rvq-xcol": ("rvq_encode", 0, lambda j: mutate(j, p={8: 1})),
    "rvq-valid-over-Tmax": ("rvq_encode", 0, lambda j: mutate(j, ins={1: i32(7, 4)})),
    "rvq-code-ranges-overlap": ("rvq_encode", 0, lambda j: mutate(j, ins={2: i64(3, 8)})),
    "rvq-code-range-outside": ("rvq_encode", 0, lambda j: mutate(j, ins={2: i64(3, 19)})),
    "rvq-code-off-negative": ("rvq_encode", 0, lambda j: mutate(j, ins={2: i64(-1, 14)})),
    "rvq-codebook-outside-pool": ("rvq_encode", 0, lambda j: mutate(j, ins={5: i64(9)})),
    "rvq-c2-outside-pool": ("rvq_encode", 0, lambda j: mutate(j, ins={6: i64(9)})),
    "gather-codebook-outside-pool": ("rvq_gather", 0, lambda j: mutate(j, ins={5: i64(12)})),
    "gather-first-frame": ("rvq_gather", 3, lambda j: mutate(j, ins={4: i32(5, 0, 1)})),
    "gather-n-rest-16": ("rvq_gather", 0, lambda j: mutate(j, p={3: 16})),
    "take-latent-mod4": ("stream_take_chunk", 0, lambda j: mutate(j, p={3: 6})),
    "take-lat-off-mod4": ("stream_take_chunk", 0, lambda j: mutate(j, p={5: 6})),
    "take-bstride-mod4": ("stream_take_chunk", 0, lambda j: mutate(j, p={1: 30}, ins={0: sent((3, 30))})),
    "take-outside-front": ("stream_take_chunk", 0, lambda j: mutate(j, ins={1: i32(6, 2, 1)})),
    "take-over-max-take": ("stream_take_chunk", 0, lambda j: mutate(j, p={4: 2})),
    "take-outside-lat": ("stream_take_chunk", 0, lambda j: mutate(j, p={5: 16})),
    "roll-keep-mod4": ("roll_history", 1, lambda j: mutate(j, p={2: 6}, ios={0: sent(24 + 6 + 12)})),
    "roll-chunk-mod4": ("roll_history", 1, lambda j: mutate(j, p={3: 10}, ios={0: sent(24 + 4 + 10)})),
    "roll-chunk-below-keep": ("roll_history", 1, lambda j: mutate(j, p={2: 16}, ios={0: sent(24 + 16 + 12)})),
    "roll-bstride-mod4": ("roll_history", 1, lambda j: mutate(j, p={1: 22}, ios={0: sent(22 + 4 + 12)})),
    "rows-chunk-below-hist": ("roll_history_rows", 0, lambda j: mutate(j, p={1: 7, 3: 3})),
    "rows-Tal": ("roll_history_rows", 0, lambda j: mutate(j, p={1: 9})),
    "rows-only-row": ("roll_history_rows", 15, lambda j: mutate(j, p={5: 4})),
    "rows-mode-3": ("roll_history_rows", 0, lambda j: mutate(j, ins={1: i32(1, 0, 3, 1)})),
    "rows-float4-tensor-off-16-bytes": ("roll_history_rows", 0, lambda j: mutate(j, ins={0: j["ins"][0] + i64(1, 0, 0)})),
    "rows-tensor-outside-pool": ("roll_history_rows", 0, lambda j: mutate(j, ins={0: j["ins"][0] + i64(400, 0, 0)})),
    "rows-tensors-overlap": ("roll_history_rows", 0, lambda j: mutate(j, ins={0: j["ins"][0] * i64(0, 1, 1) + i64(8, 0, 0)})),
    "state-off-mod16": ("history_state_rows", 0, lambda j: mutate(j, ins={0: j["ins"][0] + i64(0, 0, 8)})),
    "state-outside-blob": ("history_state_rows", 0, lambda j: mutate(j, ins={0: j["ins"][0] + i64(0, 0, 320)})),
    "state-row": ("history_state_rows", 0, lambda j: mutate(j, p={4: 4})),
    "mel-lds": ("log_mel", 0, lambda j: mutate(j, p={1: 40000, 2: 16385}, ins={0: sent((3, 40000)), 1: sent((16385, 3))})),
    "mel-ld": ("log_mel", 0, lambda j: mutate(j, p={1: 9}, ins={0: sent((3, 9))})),
    "head-width": ("attn_causal_f32", 0, lambda j: mutate(j, ins={0: sent((2, 1, 3 * 3 * 32))})),
    "stats-ld-below-C": ("time_stats", 1, lambda j: mutate(j, p={2: 60}, ins={0: sent((3, 60))})),
    "mask-valid-over-Tpad": ("mask_tail", 0, lambda j: mutate(j, ins={0: i32(5, 0, 3)})),
    "mask-bstride": ("mask_tail", 0, lambda j: mutate(j, p={3: 19}, ios={0: sent((3, 19))})),
    "layernorm-stride": ("layernorm_f32", 1, lambda j: mutate(j, p={3: 383}, ins={0: sent((2, 383))})),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_host_refusals(name):
    """Every refusal precedes allocation: check_only with m == NULL returns INVALID_INPUT, and the job it was made from is accepted."""
    from qwen3tts import _lib
    op, i, change = REFUSED[name]
    j = jobs_of(BY_NAME[op])[i]
    assert check_only(j) == 0
    bad = change(j)
    if bad["op"] is None:
        a = _lib.RowopDebug(op=21, check_only=1)
        assert _lib.lib().q3tts_debug_rowop(None, a) == 3
        return
    assert check_only(bad) == 3, name


# ---------------------------------------------------------------------------------------------
# GPU part
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine(ckpt_dirs):
    from qwen3tts import Qwen3TTSModel
    m = Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-a"], max_batch=1, max_frames=8, max_prompt=16)
    yield m
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("op", [o.op for o in OPS])
def test_rowop_block_matches_its_reference(engine, op):
    """Every job of the op: one launch of the product's launcher; every owned element finite and inside its bar or equal bit for
    bit, every sentinel intact, the bit-exact claims between launches."""
    o = BY_NAME[op]
    WORST.pop(op, None)
    o.flow(lambda j: engine.debug_rowop(j["op"], j["p"], j["f"], j["ins"], j["ios"]), jobs_of(o))
    print("GPU, worst error / bar: %s %.4f" % (op, WORST.get(op, 0.0)))


@pytest.mark.gpu
def test_refused_arguments_launch_nothing(engine):
    """With a live model: a refused call (status 3) leaves its output untouched, and a good call afterwards works."""
    from qwen3tts import Qwen3TTSError
    j = jobs_of(BY_NAME["dwconv_ln"])[0]
    bad = mutate(j, p={3: 4097})
    with pytest.raises(Qwen3TTSError) as e:
        engine.debug_rowop(bad["op"], bad["p"], bad["f"], bad["ins"], bad["ios"])
    assert e.value.status == 3
    o = BY_NAME["dwconv_ln"]
    o.verify(j, engine.debug_rowop(j["op"], j["p"], j["f"], j["ins"], j["ios"])[0])
