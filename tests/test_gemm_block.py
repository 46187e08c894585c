"""Block-level parity of the decode GEMMs (csrc/kernels/gemm_decode.hip, gemm_body.inc, gemm_prefill.hip, repack.hip and the
norm-row job of row_jobs.h) through q3tts_debug_gemm: one launch of the product's own launcher per case, on caller-built host
buffers, against a float64 reference written here.

The reference (numpy float64) rounds where the oracle rounds (q3tts_oracle.c o_rmsnorm_bf16, o_linear_bf16, o_qlinear_bf16,
o_silu_mul_bf16, o_add_bf16): operands are the exact bf16 values; int4 weights are bf16(q * scale + bias), multiply and add
rounded separately in fp32; the norm prologue is bf16(bf16(h * rstd) * w) with rstd in fp32 from the float64 sum of the given
partials; EPI 0 is bf16(acc + bias) [then bf16(silu(.))], EPI 2 bf16(bf16(silu(bf16(g))) * bf16(u)), EPI 3
bf16((resid ? h_old : 0) + bf16(acc + bias)). The partial sums of squares handed to the prologue are multiples of 1/16 below
2^20, so their fp32 sum is exact in ANY order and rstd (correctly rounded fp32 divide / sqrt on both sides) is the same number
in the kernel and here: the normalised operand carries no error of its own, and dropping or doubling a partial moves it grossly.

Bars. u = 2^-7 is one bf16 step relative to the value. A is the fp32 accumulation bound of one output,
  A = (32 + 4 * ceil(KC / NW) + NW + 1) * 2^-24 * (sum_k |x_k w_k| + |bias|),   KC = K / 128, NW = 4 (KC <= 4) or 8:
every product enters one 32-wide MFMA (at most 32 roundings inside it, whatever its internal order), the MFMAs of a wave form a
chain of 4 * ceil(KC / NW) fp32 additions, NW wave partials are added in order, then the bias. Both sides round a number to
bf16; two numbers at most A apart round to bf16 values at most one step + A apart, hence for a rounded GEMM term t
  d(t) = u |t| + (1 + 2u) A                                  -- never a constant floor: where t cancels, A is what is left.
  EPI 0            |a - r| <= d(r);  with act_silu: |silu'(t)| d(t) + u |r|
  EPI 3            |a - r| <= d(t) + (resid ? u |r| : 0)       (one step of the GEMM term plus one of the sum)
  EPI 2            gb = bf16(g), ub = bf16(u), sg = bf16(silu(gb)):  d(sg) = |silu'(gb)| d(gb) + u |sg|,
                   |a - r| <= d(sg) |ub| + |sg| d(ub) + u |r|   (first order)
No element is exempt. For plain EPI 0 (no bias, no activation, no prologue) fewer than 2 % of the elements may differ from the
reference at all. ss_out against the float64 sum of the 16 squares the kernel itself stored: 16 fp32 additions of positive
terms, relative 2^-20. Norm rows (rider and stand-alone): out equal or adjacent bf16, fewer than 2 % differing, ss_out as above.
Everything a launch must not write keeps its sentinel bits: rows >= M of y below and above Mpad, the ss_out slots of those
rows, the columns behind N (where the missing tile of a ragged gate/up workgroup would land).

Bit-exact equivalences. Per output element the arithmetic is fixed by K alone (wave count, chunk order per wave, four MFMAs per
chunk, LDS reduction in wave order), so every launch of a class writes, for the same row content, the same bits whatever M, the
row's position, grid.y split, row blocks per workgroup, tiles per workgroup, registers or streamed, non-temporal loads, the
diagnostic switches, y_tiled, padded allocations, rider or not, tall or skinny, norm prologue or launch_norm_rows + plain GEMM.
Rows are drawn from a pool of 64 row contents per (class, K); each launch places them by its own permutation, and the first
launch that produces a (row content, column) records its bits; every later one must match them (`==` on the raw bits).

Instantiations the launchers can dispatch (522), all reached by the case table (test_case_table_reaches_every_instantiation):
  gemm_skinny_kernel<MB, EPI, NW, CH, NORM, QUANT, NP, NTW>
    EPI {0,2,3} x NORM x QUANT x (NW,CH) {(4,1),(8,1),(8,2),(8,3),(8,6),(8,0 streamed)} x (MB 1..4, or MB 1..2 with NTW)   432
        cases "mb*": K 128/384/512 -> (4,1), 640 -> (8,1), 1024/1152/2048 -> (8,2), 3072 -> (8,3), 4096/4224 -> (8,0),
        6144 -> (8,6); MB forced with Q3TTS_GEMM_NO_ROW_SPLIT, and as the launcher splits ("nat*")
    MB 4, NORM 0, NTW 0, CH 0, NP {2,4} x EPI x QUANT  (prefill chunks)                                                     12
        cases "pf-np2" (M 64, mbw 4 reached naturally by the width), "pf-np4" (M 128: int4, bias, or the tall form switched off)
    EPI 2, MB {1,2}, CH {1,2}, NP {2,3} x NORM x QUANT x NTW  (one round of gate/up workgroups)                            64
        cases "gu-*": 2056 columns (257 tiles, NP 2, ragged), 4104 / 4112 / 4120 columns (513 / 514 / 515 tiles, NP 3)
  gemm_skinny_side_kernel<MB {1,2}, CH {1,2}, QUANT>                                                                          8
        cases "ride-*" (EPI 0 with prologue, K 640 / 1152 / 2048)
  gemm_tall_kernel<shape 2 (128 x 64) | 3 (64 x 64), EPI {0,2,3}>                                                             6
        cases "tall-*" (M 65, 100, 128, 513; EPI 3 with residual and ss_out)

The CPU part (no marker) asserts that coverage through geometry_only (host code), and runs every pool of the matrix through a
float32 restatement of the kernels' walk (chunk-interleaved wave partials of 32-wide products, wave partials added in order, the
same rounding points) against the float64 reference under the same bars, so the inputs are known to stay inside the bars
without the kernel."""
import zlib

import numpy as np
import pytest

from conftest import bf16_to_f32

ULP = 2.0 ** -7
SENT = 0x7FC1                      # a NaN: what must not be read poisons the output, what must not be written keeps these bits
SENT_F = np.uint32(0x7FC12345)     # the same for the fp32 buffers
R = 64                             # row contents per pool
EPS = 1e-6
ENV_KEYS = ("Q3TTS_GEMM_NO_ROW_SPLIT", "Q3TTS_GEMM_ONE_PAIR", "Q3TTS_NO_TALL_GEMM", "Q3TTS_TALL_SHAPE")
FORMS = [(4, 1), (8, 1), (8, 2), (8, 3), (8, 6), (8, 0)]
KS = [128, 384, 512, 640, 1024, 1152, 2048, 3072, 4096, 4224, 6144]
BIG_KS = (640, 1152)               # the only K that carry wide N (the several-tiles-per-workgroup forms)
SS_COUNTS = [1, 7, 8, 9, 64, 127, 128, 129, 192, 256]
CLASSES = [(e, n, q) for e in (0, 2, 3) for n in (0, 1) for q in (0, 1)]
CLASS_IDS = ["epi%d-%s-%s" % (e, "norm" if n else "plain", "int4" if q else "bf16") for e, n, q in CLASSES]


def f2b(x):
    from qwen3tts import synth
    return synth.f32_to_bf16_bits(np.ascontiguousarray(x, np.float32))


def rb32(x):
    return bf16_to_f32(f2b(x))


def rb64(x):
    """float64 -> nearest-even bf16 value, held in float64 (no double rounding through fp32; normal range only)."""
    b = np.ascontiguousarray(x, np.float64).view(np.uint64)
    b = (b + np.uint64(0x0FFFFFFFFFFF) + ((b >> np.uint64(45)) & np.uint64(1))) & ~np.uint64((1 << 45) - 1)
    return b.view(np.float64)


def rb(x):
    return rb32(x) if x.dtype == np.float32 else rb64(x)


def silu(x):
    return x / (1.0 + np.exp(-x))


def dsilu(x):
    s = 1.0 / (1.0 + np.exp(-x))
    return s * (1.0 + x * (1.0 - s))


def default_ss_count(K):
    return min(K // 16, 256) if K != 6144 else 129   # the engine's K / 16 where norm rows can fold it; 129: one tail partial


def nw_of(K):
    return 4 if K // 128 <= 4 else 8


def acc_depth(K):
    nw = nw_of(K)
    return 32 + 4 * -(-(K // 128) // nw) + nw + 1


# ---------------------------------------------------------------------------------------------
# weights and row pools
# ---------------------------------------------------------------------------------------------
_WEIGHTS = {}


def weights(K, quant, which):
    """The checkpoint form of one matrix with every row a case may take: bf16 [Nmax][K], or MLX int4 (uint32 [Nmax][K / 8],
    bf16 scales of both signs and biases [Nmax][K / 64]). A case takes the first N rows."""
    key = (K, quant, which)
    if key not in _WEIGHTS:
        nmax = 4192 if K in BIG_KS else 80
        rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
        if quant:
            q = rng.integers(0, 2 ** 32, (nmax, K // 8), dtype=np.uint64).astype(np.uint32)
            sc = f2b(rng.uniform(0.003, 0.009, (nmax, K // 64)) * rng.choice([-1.0, 1.0], (nmax, K // 64)))
            bi = f2b(-7.5 * bf16_to_f32(sc) * rng.uniform(0.8, 1.2, (nmax, K // 64)))
            _WEIGHTS[key] = dict(W=q, scales=sc, biases=bi)
        else:
            _WEIGHTS[key] = dict(W=f2b(rng.standard_normal((nmax, K)) * 0.03))
    return _WEIGHTS[key]


def weight_values(w, n):
    """float32 [n][K]: the values the kernel multiplies with."""
    if "scales" not in w:
        return bf16_to_f32(w["W"][:n])
    q = w["W"][:n]
    nib = ((q[:, :, None] >> (4 * np.arange(8, dtype=np.uint32))) & np.uint32(15)).reshape(n, -1).astype(np.float32)
    sc = np.repeat(bf16_to_f32(w["scales"][:n]), 64, axis=1)
    bi = np.repeat(bf16_to_f32(w["biases"][:n]), 64, axis=1)
    return rb32((nib * sc).astype(np.float32) + bi)   # multiply and add rounded separately in fp32, then bf16


def partial_sums(rng, K, ssc):
    """[R][ssc] fp32 partial sums of squares: multiples of 1/16 (exact fp32 sums in any order), deliberately NOT the rows' true
    sums; one partial holds three quarters of a row's total and sits at index 0, 7, 8, 127, 128 or ssc - 1 in turn."""
    f = rng.uniform(0.5, 2.0, R)
    rest = 0.25 * K * f[:, None] / max(ssc - 1, 1) * rng.uniform(0.5, 1.5, (R, ssc))
    p = np.maximum(np.round(rest * 16), 1.0)
    cand = [j for j in (0, 7, 8, 127, 128, ssc - 1) if j < ssc]
    for r in range(R):
        p[r, cand[r % len(cand)]] = np.round(0.75 * K * f[r] * 16)
    assert p.sum(1).max() < 2 ** 24
    return (p / 16.0).astype(np.float32)


def rstd_of(total, dim):
    """fp32, the kernel's expression: 1 / sqrt(s / dim + eps)."""
    s = np.asarray(total, np.float32)
    return (np.float32(1.0) / np.sqrt(s / np.float32(dim) + np.float32(EPS))).astype(np.float32)


def normed(h_bits, w_bits, rstd):
    return rb32(rb32(bf16_to_f32(h_bits) * rstd[:, None]) * bf16_to_f32(w_bits)[None, :])


class Pool:
    """64 row contents of one (class, K, gain, ss_count): inputs, the float64 accumulators over every column a case can take,
    and the bits the first launch of each variant recorded."""

    def __init__(self, epi, norm, quant, K, gain="lo", ssc=None, nmax=None):
        self.epi, self.norm, self.quant, self.K, self.gain = epi, norm, quant, K, gain
        self.ssc = (ssc or default_ss_count(K)) if norm else 0
        self.nmax = nmax or (4192 if K in BIG_KS else 80)
        rng = np.random.default_rng(zlib.crc32(repr((epi, norm, quant, K, gain, self.ssc)).encode()))
        self.h = f2b(rng.standard_normal((R, K)))
        self.wg, self.wu = weights(K, quant, "g"), (weights(K, quant, "u") if epi == 2 else None)
        if norm:
            g = rng.standard_normal(K)
            self.norm_w = f2b(6.0 * (1.0 + 0.5 * g) * rng.choice([-1.0, 1.0], K) if gain == "hi" else 1.0 + 0.2 * g)
            self.P = partial_sums(rng, K, self.ssc)
            self.rstd = rstd_of(self.P.astype(np.float64).sum(1), K)
            self.xv = normed(self.h, self.norm_w, self.rstd)
        else:
            self.xv = bf16_to_f32(self.h)
        self.bias = f2b(rng.standard_normal(self.nmax) * 0.5)
        x64 = self.xv.astype(np.float64)
        self.acc, self.S = [], []
        for w in (self.wg, self.wu):
            if w is not None:
                wv = weight_values(w, self.nmax).astype(np.float64)
                self.acc.append(x64 @ wv.T)
                self.S.append(np.abs(x64) @ np.abs(wv).T)
        t = rb64(self.acc[0] + bf16_to_f32(self.bias).astype(np.float64))
        if gain == "hi":   # the residual cancels the GEMM term to within a few steps
            self.h_old = f2b((-t * (1.0 + 2.0 ** -6 * rng.standard_normal(t.shape))).astype(np.float32))
        else:
            self.h_old = f2b(rng.standard_normal((R, self.nmax)))
        self.bits = {}

    def accumulate_f32(self):
        """The kernels' walk in fp32: wave w takes the 128-wide chunks w, w + NW, ... in order, four 32-wide products per chunk
        (k = 128 kc + 32 h + 8 i + j, h = 0..3, j = 0..7 for product i), then the wave partials are added in wave order."""
        K, nw = self.K, nw_of(self.K)
        KC = K // 128
        xs = self.xv.reshape(R, KC, 4, 4, 8)
        out = []
        for w in (self.wg, self.wu):
            if w is None:
                continue
            ws = weight_values(w, self.nmax).reshape(self.nmax, KC, 4, 4, 8)
            total = np.zeros((R, self.nmax), np.float32)
            for wave in range(nw):
                part = np.zeros((R, self.nmax), np.float32)
                for kc in range(wave, KC, nw):
                    for i in range(4):
                        part += xs[:, kc, :, i, :].reshape(R, 32) @ ws[:, kc, :, i, :].reshape(self.nmax, 32).T
                total += part
            out.append(total)
        return out

    def finish(self, accs, rows, N, bias=False, silu_act=False, resid=False):
        """The epilogue at the oracle's rounding points on accumulators of either precision -> values [len(rows)][N]."""
        dt = accs[0].dtype
        a = [x[rows][:, :N] for x in accs]
        if self.epi == 2:
            return rb(rb(silu(rb(a[0]))) * rb(a[1]))
        t = rb(a[0] + (bf16_to_f32(self.bias[:N]).astype(dt) if bias else 0))
        if self.epi == 0:
            return rb(silu(t)) if silu_act else t
        return rb(bf16_to_f32(self.h_old[rows][:, :N]).astype(dt) + t) if resid else t

    def bar(self, rows, N, bias=False, silu_act=False, resid=False):
        """(reference, bar) per element, float64: the derivation of the module docstring."""
        c = acc_depth(self.K) * 2.0 ** -24 * (1.0 + 2.0 * ULP)
        r = self.finish(self.acc, rows, N, bias, silu_act, resid)
        if self.epi == 2:
            gb, ub = rb64(self.acc[0][rows][:, :N]), rb64(self.acc[1][rows][:, :N])
            d_gb = ULP * np.abs(gb) + c * self.S[0][rows][:, :N]
            d_ub = ULP * np.abs(ub) + c * self.S[1][rows][:, :N]
            sg = rb64(silu(gb))
            d_sg = np.abs(dsilu(gb)) * d_gb + ULP * np.abs(sg)
            return r, d_sg * np.abs(ub) + np.abs(sg) * d_ub + ULP * np.abs(r)
        bv = np.abs(bf16_to_f32(self.bias[:N]).astype(np.float64)) if bias else 0.0
        t = rb64(self.acc[0][rows][:, :N] + (bf16_to_f32(self.bias[:N]).astype(np.float64) if bias else 0.0))
        d_t = ULP * np.abs(t) + c * (self.S[0][rows][:, :N] + bv)
        if self.epi == 0:
            return r, (np.abs(dsilu(t)) * d_t + ULP * np.abs(r)) if silu_act else d_t
        return r, d_t + (ULP * np.abs(r) if resid else 0.0)


_POOLS = {}


def pool(epi, norm, quant, K, gain="lo", ssc=None, nmax=None):
    key = (epi, norm, quant, K, gain, ssc, nmax)
    if key not in _POOLS:
        if len(_POOLS) > 64:   # wide pools are tens of megabytes
            _POOLS.clear()
        _POOLS[key] = Pool(epi, norm, quant, K, gain, ssc, nmax)
    return _POOLS[key]


# ---------------------------------------------------------------------------------------------
# the case matrix
# ---------------------------------------------------------------------------------------------
def _case(name, K, M, N, **kw):
    c = dict(name=name, K=K, M=M, N=N, env={}, nt=0, y_tiled=0, pad=True, bias=False, silu=False, resid=False, ss_out=False,
             gain="lo", ssc=None, nmax=None, rider=None, via_rows=False)
    c.update(kw)
    return c


def class_cases(epi, norm, quant):
    """Every launch of one (EPI, NORM, QUANT) class."""
    out = []
    small = 24 if epi == 2 else 32
    nosplit = {"Q3TTS_GEMM_NO_ROW_SPLIT": "1"}
    more = dict(resid=True, ss_out=True) if epi == 3 else {}
    k = 0
    # every (NW, CH) x row blocks per workgroup, forced and with non-temporal loads; ragged and full M
    for K in KS:
        for mb, Ms in ((1, (1, 15, 16)), (2, (17, 32)), (3, (33, 48)), (4, (49, 64))):
            M = Ms[k % len(Ms)]
            out.append(_case("mb%d-k%d-m%d" % (mb, K, M), K, M, small, env=nosplit, y_tiled=k % 2 if epi == 0 else 0, pad=k % 3 != 0,
                             **more))
            if mb <= 2:
                out.append(_case("mb%d-k%d-m%d-nt" % (mb, K, M), K, M, small, env=nosplit, nt=1, pad=k % 3 != 1, **more))
            k += 1
    # the rows as the launcher itself splits them (grid.y 4, 2, 3 / 1), with every M of the list
    for K in (128, 640, 1152, 4096):
        for M in (1, 15, 16, 17, 33, 48, 64):
            out.append(_case("nat-k%d-m%d" % (K, M), K, M, small, y_tiled=(M // 16) % 2 if epi == 0 else 0, pad=M % 2 == 1, **more))
    out.append(_case("nat-k640-m64-tight", 640, 64, small, pad=False, **more))
    out.append(_case("nat-k640-m64-onepair", 640, 64, small, env={"Q3TTS_GEMM_ONE_PAIR": "1"}, **more))
    # epilogue options and the second input set (large norm gains, a residual that cancels the GEMM term)
    for K in (640, 4096):
        for M, env in ((33, {}), (64, nosplit)):
            out.append(_case("hi-k%d-m%d" % (K, M), K, M, small, env=env, gain="hi", **more))
            if epi != 2:
                out.append(_case("hi-k%d-m%d-bias" % (K, M), K, M, small, env=env, gain="hi", bias=True, **more))
    if epi == 0:
        out.append(_case("silu-k384-m17", 384, 17, 48, silu=True, bias=True))
        out.append(_case("silu-k1152-m64", 1152, 64, 48, silu=True, env=nosplit))
    if epi == 3:
        out.append(_case("noresid-k640-m33", 640, 33, 32, ss_out=True))
        out.append(_case("noresid-k1152-m64-bias", 1152, 64, 32, bias=True, env=nosplit))
        out.append(_case("resid-noss-k640-m17", 640, 17, 32, resid=True))
    # more than 64 rows outside the tall form
    if norm:
        out.append(_case("rows128-k1152", 1152, 128, small, **more))
        out.append(_case("rows128-k128", 128, 128, small, **more))
    if quant or epi != 2:
        for M in (65, 128):
            b = dict(bias=True) if (not quant and epi != 2) else {}
            if quant or b:
                out.append(_case("rows%d-k640" % M, 640, M, small, **b, **more))
    # prefill-chunk forms: four row blocks and several tiles per workgroup
    if not norm:
        wide2 = 1032 if epi == 2 else 2064                 # 129 tiles: mbw 4 naturally at M 64, NP 2, ragged
        wide4 = 8 * 261 if epi == 2 else 16 * 261          # 261 tiles at split 2: NP 4, ragged
        b = dict(bias=True) if epi != 2 else {}
        out.append(_case("pf-np2-m64", 640, 64, wide2, **more))
        if b:
            out.append(_case("pf-np2-m64-bias", 640, 64, wide2, **b, **more))
        out.append(_case("pf-np2-m64-onepair", 640, 64, wide2, env={"Q3TTS_GEMM_ONE_PAIR": "1"}, **more))
        if quant or b:
            out.append(_case("pf-np4-m128", 640, 128, wide4, **(b if not quant else {}), **more))
            out.append(_case("pf-np4-m113-tight", 640, 113, wide4, pad=False, **(b if not quant else {}), **more))
        else:
            out.append(_case("pf-np4-m128", 640, 128, wide4, env={"Q3TTS_NO_TALL_GEMM": "1"}, **more))
    # gate/up: several tiles per workgroup, ragged widths
    if epi == 2:
        widths = {2: [2056], 3: [4104, 4112, 4120]}
        j = 0
        for K in BIG_KS:
            for npw in (2, 3):
                for mb, M in ((1, (1, 15, 16)), (2, (17, 32))):
                    for nt in (0, 1):
                        N = widths[npw][j % len(widths[npw])]
                        out.append(_case("gu-np%d-k%d-m%d-n%d%s" % (npw, K, M[j % len(M)], N, "-nt" if nt else ""), K, M[j % len(M)], N,
                                         nt=nt, pad=j % 3 != 0))
                        j += 1
        out.append(_case("gu-np3-k640-m16-n4120-onepair", 640, 16, 4120, env={"Q3TTS_GEMM_ONE_PAIR": "1"}))
        out.append(_case("gu-np2-k1152-m32-n2056-onepair", 1152, 32, 2056, env={"Q3TTS_GEMM_ONE_PAIR": "1"}))
    # the rider kernel, against the plain launch and against launch_norm_rows alone
    if epi == 0 and norm:
        for K in (640, 1152, 2048):
            for M in (7, 16, 32):   # (32 rows of a narrow layer stay in one workgroup only with the switch)
                out.append(_case("ride-k%d-m%d" % (K, M), K, M, 48, rider="own" if M != 16 else "ss_in", env=nosplit if M > 16 else {}))
    # the prologue against launch_norm_rows(ss_in) + the same GEMM without it, for every partial count
    if norm:
        for i, ssc in enumerate(SS_COUNTS):
            M = (33, 64, 17)[i % 3]
            out.append(_case("ssc%d-k640-m%d" % (ssc, M), 640, M, small, ssc=ssc, nmax=small, via_rows=True, **more))
        out.append(_case("ssc129-k2048-m32", 2048, 32, small, ssc=129, nmax=small, via_rows=True, **more))
    # the tall form, both shapes, against skinny
    if not norm and not quant:
        for M, K in ((65, 384), (100, 1152), (128, 640), (513, 1152)):
            for tag, env in (("auto", {}), ("s2", {"Q3TTS_TALL_SHAPE": "2"}), ("s3", {"Q3TTS_TALL_SHAPE": "3"}),
                             ("skinny", {"Q3TTS_NO_TALL_GEMM": "1"})):
                out.append(_case("tall-m%d-k%d-%s" % (M, K, tag), K, M, 80, env=env, y_tiled=M % 2 if epi == 0 else 0, **more))
    return out


def rowmap(c):
    """Which row content sits at row m of the launch: a permutation of its own per case, so that the same content meets every
    row position, row block and grid.y workgroup."""
    s = zlib.crc32(c["name"].encode())
    a, b = 2 * (s % 29) + 1, (s >> 8) % R
    return (a * np.arange(c["M"]) + b) % R


def dims(c, epi):
    Mp = -(-c["M"] // 16) * 16
    tiled = epi != 0 or c["y_tiled"]
    n128 = -(-c["N"] // 128) * 128
    if c["pad"]:
        return dict(xrows=Mp + 16, yrows=Mp + 32, ss_ld=Mp + 16, y_cols=n128 + 128 if tiled else c["N"] + 8)
    return dict(xrows=Mp, yrows=Mp, ss_ld=Mp, y_cols=n128 if tiled else c["N"])


def geometry(c, epi, norm, quant):
    from qwen3tts import _lib
    d = dims(c, epi)
    kw = dict(M=c["M"], K=c["K"], N=c["N"], xMB=d["xrows"] // 16, yMB=d["yrows"] // 16, ss_ld=d["ss_ld"], y_cols=d["y_cols"], epi=epi,
              act_silu=int(c["silu"]), resid=int(c["resid"]), nt_weights=c["nt"], y_tiled=c["y_tiled"], norm=norm, quant=quant,
              has_bias=int(c["bias"]), ss_count=(c["ssc"] or default_ss_count(c["K"])) if norm else 0, norm_dim=c["K"])
    if c["rider"]:
        kw.update(rider_M=c["M"], rider_H=c["K"], rider_MB=d["xrows"] // 16)
    return _lib.gemm_geometry(**kw)


def instantiation(g, epi, norm, quant):
    if g["tall"]:
        return ("tall", g["tall_shape"], epi)
    if g["rode"]:
        return ("side", g["mbw"], g["ch"], quant)
    return ("skinny", g["mbw"], epi, g["nw"], g["ch"], norm, quant, g["np"], g["ntw"])


def expected_instantiations():
    """What launch_q / launch_mb, launch_gemm_skinny_with_norm_rows and launch_shape can dispatch (the docstring's table)."""
    s = set()
    for epi, norm, quant in CLASSES:
        for ntw, mbs in ((0, (1, 2, 3, 4)), (1, (1, 2))):
            for mb in mbs:
                for nw, ch in FORMS:
                    s.add(("skinny", mb, epi, nw, ch, norm, quant, 1, ntw))
                if epi == 2 and mb <= 2:
                    for ch in (1, 2):
                        for npw in (2, 3):
                            s.add(("skinny", mb, 2, 8, ch, norm, quant, npw, ntw))
        if not norm:
            for npw in (2, 4):
                s.add(("skinny", 4, epi, 8, 0, 0, quant, npw, 0))
    s |= {("side", mb, ch, q) for mb in (1, 2) for ch in (1, 2) for q in (0, 1)}
    s |= {("tall", shape, epi) for shape in (2, 3) for epi in (0, 2, 3)}
    return s


class Env:
    """The launchers' diagnostic switches, re-read after every change (they are read once per model load)."""

    def __init__(self, monkeypatch):
        self.mp, self.cur = monkeypatch, None

    def set(self, env):
        from qwen3tts import _lib
        if env == self.cur:
            return
        for k in ENV_KEYS:
            if k in env:
                self.mp.setenv(k, env[k])
            else:
                self.mp.delenv(k, raising=False)
        _lib.reload_debug_env()
        self.cur = dict(env)


@pytest.fixture
def switches(monkeypatch):
    e = Env(monkeypatch)
    yield e
    e.set({})


def by_env(cases):
    return sorted(cases, key=lambda c: sorted(c["env"].items()))


# ---------------------------------------------------------------------------------------------
# CPU part
# ---------------------------------------------------------------------------------------------
def test_case_table_reaches_every_instantiation(switches):
    """Through geometry_only (skinny_geometry, gemm_tall_takes, the rider test: host code) the case table reaches exactly the
    set of kernels the launchers can dispatch: a new instantiation without a case, or a case that no longer reaches its
    kernel, fails here. Also: row splits 2 and 4, and mbw 4 without any switch."""
    reached, splits, natural4 = {}, set(), False
    for epi, norm, quant in CLASSES:
        for c in by_env(class_cases(epi, norm, quant)):
            switches.set(c["env"])
            g = geometry(c, epi, norm, quant)
            if c["rider"]:
                assert g["rode"] == 1, c["name"]
            reached.setdefault(instantiation(g, epi, norm, quant), c["name"])
            if c["rider"]:  # the plain launch of the same arguments is run too
                reached.setdefault(("skinny", g["mbw"], epi, g["nw"], g["ch"], norm, quant, g["np"], g["ntw"]), c["name"])
            if not g["tall"]:
                splits.add(g["split"])
                natural4 = natural4 or (g["mbw"] == 4 and not c["env"])
    want = expected_instantiations()
    assert len(want) == 522
    missing = sorted(want - set(reached))
    assert not missing, "%d instantiations without a case, e.g. %r" % (len(missing), missing[:8])
    extra = sorted(set(reached) - want)
    assert not extra, "cases reach kernels the table does not list: %r" % [(k, reached[k]) for k in extra[:8]]
    assert {1, 2, 4} <= splits and natural4


def variant_of(c):
    return (c["bias"], c["silu"], c["resid"])


def test_restated_walk_stays_inside_the_bars():
    """Every pool of the matrix through the float32 restatement of the kernels' walk, against the float64 reference under the
    GPU test's bars, over all 64 row contents and every column a case takes."""
    worst, where = 0.0, None
    for epi, norm, quant in CLASSES:
        seen = {}
        for c in class_cases(epi, norm, quant):
            key = (c["K"], c["gain"], c["ssc"], c["nmax"])
            seen.setdefault(key, {}).setdefault(variant_of(c), 0)
            seen[key][variant_of(c)] = max(seen[key][variant_of(c)], c["N"])
        for (K, gain, ssc, nmax), variants in seen.items():
            p = pool(epi, norm, quant, K, gain, ssc, nmax)
            acc32 = p.accumulate_f32()
            rows = np.arange(R)
            for (bias, sl, resid), N in variants.items():
                a = p.finish(acc32, rows, N, bias, sl, resid).astype(np.float64)
                r, bar = p.bar(rows, N, bias, sl, resid)
                assert np.isfinite(r).all() and (bar > 0).all()
                w = float((np.abs(a - r) / bar).max())
                assert w <= 1.0, (CLASS_IDS[CLASSES.index((epi, norm, quant))], K, gain, ssc, bias, sl, resid, w)
                if epi == 0 and not (norm or bias or sl):
                    assert (a != r).mean() < 0.02
                if w > worst:
                    worst, where = w, (epi, norm, quant, K, gain)
        _POOLS.clear()
    print("gemm block, float32 restatement: worst |a - r| / bar = %.3f %r" % (worst, where))


def test_a_dropped_or_doubled_partial_breaks_the_bar():
    """What the ss_count cases rely on: without the dominant partial of a row (or with it twice) the restated result leaves the
    bar on most of the row's elements."""
    p = pool(0, 1, 0, 640, "lo", 129, 32)
    rows = np.arange(R)
    r, bar = p.bar(rows, 32)
    for factor in (0.0, 2.0):
        P = p.P.astype(np.float64).copy()
        j = P.argmax(1)
        P[rows, j] *= factor
        xv = normed(p.h, p.norm_w, rstd_of(P.sum(1), 640)).astype(np.float64)
        a = rb64(xv @ weight_values(p.wg, 32).astype(np.float64).T)
        assert ((np.abs(a - r) > bar).mean(1) > 0.5).all(), factor


# ---------------------------------------------------------------------------------------------
# GPU part
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engines(ckpt_dirs):
    from qwen3tts import Qwen3TTSModel
    out = {"tiny-a": Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-a"], max_batch=1, max_frames=8, max_prompt=16)}
    yield out
    for m in out.values():
        m.close()


def sent_f32(shape):
    return np.full(shape, SENT_F, np.uint32).view(np.float32)


def norm_rows_reference(h_bits, w_bits, total):
    return normed(h_bits, w_bits, rstd_of(total, h_bits.shape[1]))


def check_norm_rows(name, p, rm, M, res, ss_in_used):
    """Norm rows (rider or stand-alone): out equal or adjacent bf16 with fewer than 2 % differing; ss_out against the float64
    sum of the stored squares; rows >= M untouched."""
    out, sso = res["rider_out"], res["rider_ss_out"]
    total = p.P[rm].astype(np.float64).sum(1) if ss_in_used else (bf16_to_f32(p.h[rm]).astype(np.float64) ** 2).sum(1)
    want = f2b(norm_rows_reference(p.h[rm], p.norm_w, total))
    got = out[:M]
    near = (np.abs(got.astype(np.int32) - want.astype(np.int32)) <= 1) | (bf16_to_f32(got) == bf16_to_f32(want))
    assert near.all(), (name, "norm rows off by more than one bf16 step: %d elements" % int((~near).sum()))
    assert (got != want).mean() < 0.02, (name, float((got != want).mean()))
    assert (out[M:] == SENT).all(), (name, "norm rows wrote a row >= M")
    if sso is not None:
        exact = (bf16_to_f32(got).astype(np.float64) ** 2).sum(1)
        rel = np.abs(sso[:M].astype(np.float64) - exact) / exact
        print("%s: norm rows ss_out worst relative error %.3g (bar %.3g)" % (name, rel.max(), 2.0 ** -20))
        assert (rel <= 2.0 ** -20).all(), (name, float(rel.max()))
        assert (sso[M:].view(np.uint32) == SENT_F).all(), name


def run_case(m, epi, norm, quant, c, stats):
    p = pool(epi, norm, quant, c["K"], c["gain"], c["ssc"], c["nmax"])
    d = dims(c, epi)
    M, N, K = c["M"], c["N"], c["K"]
    rm = rowmap(c)
    x = np.full((d["xrows"], K), SENT, np.uint16)
    x[:M] = p.h[rm]
    y = np.full((d["yrows"], d["y_cols"]), SENT, np.uint16)
    if c["resid"]:
        y[:M, :N] = p.h_old[rm][:, :N]
    kw = dict(x=x, y=y, M=M, epi=epi, N=N, W=p.wg["W"][:N], act_silu=int(c["silu"]), resid=int(c["resid"]), nt_weights=c["nt"],
              y_tiled=c["y_tiled"])
    if quant:
        kw.update(scales=p.wg["scales"][:N], biases=p.wg["biases"][:N])
    if epi == 2:
        kw.update(W_up=p.wu["W"][:N])
        if quant:
            kw.update(scales_up=p.wu["scales"][:N], biases_up=p.wu["biases"][:N])
    if c["bias"]:
        kw.update(bias=p.bias[:N])
    if c["ss_out"]:
        kw.update(ss_out=sent_f32((N // 16, d["ss_ld"])))
    ss_in = None
    if norm:
        ss_in = sent_f32((p.ssc, d["ss_ld"])).copy()
        ss_in[:, :M] = p.P[rm].T
        kw.update(norm_w=p.norm_w, ss_in=ss_in, norm_dim=K, norm_eps=EPS)
    res = m.debug_gemm(**kw)
    g = {f: res[f] for f in ("tall", "tall_shape", "split", "mbw", "nw", "ch", "np", "gx", "ntw")}
    name = "%s [%s]" % (c["name"], " ".join("%s=%d" % kv for kv in g.items() if kv[1]))
    variant = (c["K"], c["gain"], c["ssc"], c["nmax"]) + variant_of(c)
    check_output(name, p, c, rm, res["y"], res["ss_out"], d, variant, stats)

    if c["rider"]:
        # the same launch with riders: the GEMM's bits unchanged, the riders' rows against launch_norm_rows alone
        rider = dict(h=x, w=p.norm_w, out=np.full_like(x, SENT), M=M, eps=EPS, ss_out=sent_f32((d["xrows"],)))
        if c["rider"] == "ss_in":
            rs = sent_f32((p.ssc, d["xrows"])).copy()
            rs[:, :M] = p.P[rm].T
            rider["ss_in"] = rs
        rode = m.debug_gemm(rider=rider, **kw)
        assert rode["rode"] == 1, name
        assert (rode["y"] == res["y"]).all(), (name, "the GEMM's output differs when riders share its launch")
        check_norm_rows(name + " rider", p, rm, M, rode, c["rider"] == "ss_in")
        alone = m.debug_gemm(mode=1, rider=rider)
        assert (alone["rider_out"] == rode["rider_out"]).all(), (name, "rider rows differ from launch_norm_rows")
        assert (alone["rider_ss_out"].view(np.uint32) == rode["rider_ss_out"].view(np.uint32)).all(), name
        check_norm_rows(name + " alone", p, rm, M, alone, c["rider"] == "ss_in")
    if c["via_rows"]:
        # launch_norm_rows(ss_in) then the same GEMM without prologue: kernels.h promises the prologue's bits
        rs = sent_f32((p.ssc, d["xrows"])).copy()
        rs[:, :M] = p.P[rm].T
        rows = m.debug_gemm(mode=1, rider=dict(h=x, w=p.norm_w, out=np.full_like(x, SENT), M=M, eps=EPS, ss_in=rs))
        check_norm_rows(name + " rows", p, rm, M, rows, True)
        kw2 = dict(kw, x=rows["rider_out"], norm_w=None, ss_in=None)
        two = m.debug_gemm(**kw2)
        assert (two["y"] == res["y"]).all(), (name, "norm prologue differs from launch_norm_rows + GEMM")
        if c["ss_out"]:
            assert (two["ss_out"].view(np.uint32) == res["ss_out"].view(np.uint32)).all(), name


def check_output(name, p, c, rm, y, sso, d, variant, stats):
    M, N = c["M"], c["N"]
    got = y[:M, :N]
    assert (y[M:] == SENT).all(), (name, "a row >= M of y was written")
    assert (y[:M, N:] == SENT).all(), (name, "a column >= N of y was written (the missing tile of a ragged workgroup)")
    r, bar = p.bar(rm, N, c["bias"], c["silu"], c["resid"])
    a = bf16_to_f32(got).astype(np.float64)
    ratio = np.abs(a - r) / bar
    w = float(np.nanmax(ratio)) if np.isfinite(a).all() else float("inf")
    stats["worst"] = max(stats["worst"], w)
    assert w <= 1.0, (name, "worst |a - r| / bar = %.3f at %r" % (w, np.unravel_index(np.argmax(np.nan_to_num(ratio, nan=np.inf)), ratio.shape)))
    if p.epi == 0 and not (p.norm or c["bias"] or c["silu"]):
        assert (a != r).mean() < 0.02, (name, float((a != r).mean()))
    if sso is not None:
        exact = (a.reshape(M, N // 16, 16) ** 2).sum(2).T          # [N / 16][M] from what the kernel stored
        s = sso[:, :M].astype(np.float64)
        rel = np.abs(s - exact) / np.maximum(exact, 1e-300)
        stats["worst_ss"] = max(stats["worst_ss"], float(rel.max()))
        assert (rel <= 2.0 ** -20).all(), (name, "ss_out relative error %.3g" % rel.max())
        assert (sso[:, M:].view(np.uint32) == SENT_F).all(), (name, "an ss_out slot of a row >= M was written")
    # the same row content: the same bits as whichever launch produced it first
    base = p.bits.setdefault(variant, dict(y=np.zeros((R, p.nmax), np.uint16), ss=np.zeros((R, p.nmax // 16), np.uint32),
                                           have=np.zeros((R, p.nmax), bool), have_ss=np.zeros((R, p.nmax // 16), bool),
                                           by=np.full(R, "", object)))
    for i, row in enumerate(rm):
        h = base["have"][row, :N]
        same = got[i][h] == base["y"][row, :N][h]
        assert same.all(), (name, "row %d (content %d): %d elements differ in their bits from %s" % (i, row, int((~same).sum()), base["by"][row]))
        base["y"][row, :N][~h] = got[i][~h]
        if not h.all():
            base["by"][row] = name
        base["have"][row, :N] = True
        if sso is not None:
            t = N // 16
            hs = base["have_ss"][row, :t]
            v = sso[:, i].view(np.uint32)
            assert (v[hs] == base["ss"][row, :t][hs]).all(), (name, "row %d (content %d): ss_out bits differ from an earlier launch" % (i, row))
            base["ss"][row, :t][~hs] = v[~hs]
            base["have_ss"][row, :t] = True
    stats["compared"] += int(M * N)


@pytest.mark.gpu
@pytest.mark.parametrize("epi,norm,quant", CLASSES, ids=CLASS_IDS)
def test_gemm_block_matches_float64_and_itself(engines, switches, epi, norm, quant):
    """Every launch of the class: y and ss_out inside the bars, sentinels intact, and the bits of a row content the same in
    every launch that carries it (see the module docstring)."""
    m = engines["tiny-a"]
    stats = dict(worst=0.0, worst_ss=0.0, compared=0)
    cases = by_env(class_cases(epi, norm, quant))
    for c in cases:
        switches.set(c["env"])
        run_case(m, epi, norm, quant, c, stats)
    print("gemm block %s: %d launches, %d outputs, worst |a - r| / bar = %.3f, worst ss_out relative error = %.3g"
          % (CLASS_IDS[CLASSES.index((epi, norm, quant))], len(cases), stats["compared"], stats["worst"], stats["worst_ss"]))
    _POOLS.clear()


@pytest.mark.gpu
@pytest.mark.parametrize("H", [128, 3072, 4096])
def test_norm_rows_alone(engines, H):
    """launch_norm_rows by itself, one and two trips over the row (H above 2048), from its own sum of squares and from given
    partials (as many as its job folds: 256 at H 4096), at a ragged row count."""
    m = engines["tiny-a"]
    p = pool(0, 1, 0, H)
    for M, with_ss in ((1, False), (17, True), (33, False), (64, True)):
        c = dict(name="rows-h%d-m%d" % (H, M), M=M)
        rm = rowmap(c)
        rows = -(-M // 16) * 16 + 16
        h = np.full((rows, H), SENT, np.uint16)
        h[:M] = p.h[rm]
        rider = dict(h=h, w=p.norm_w, out=np.full_like(h, SENT), M=M, eps=EPS, ss_out=sent_f32((rows,)))
        if with_ss:
            rs = sent_f32((p.ssc, rows)).copy()
            rs[:, :M] = p.P[rm].T
            rider["ss_in"] = rs
        check_norm_rows(c["name"], p, rm, M, m.debug_gemm(mode=1, rider=rider), with_ss)
    _POOLS.clear()


@pytest.mark.gpu
def test_launched_geometry_is_the_reported_geometry(engines, switches):
    """geometry_only and a real launch report the same geometry (the coverage test's link to what runs)."""
    m = engines["tiny-a"]
    for epi, norm, quant in ((0, 1, 0), (2, 0, 1), (3, 0, 0)):
        for c in by_env(class_cases(epi, norm, quant))[::7]:
            switches.set(c["env"])
            want = geometry(dict(c, rider=None), epi, norm, quant)
            p = pool(epi, norm, quant, c["K"], c["gain"], c["ssc"], c["nmax"])
            d = dims(c, epi)
            x = np.zeros((d["xrows"], c["K"]), np.uint16)
            kw = dict(x=x, y=np.zeros((d["yrows"], d["y_cols"]), np.uint16), M=c["M"], epi=epi, N=c["N"], W=p.wg["W"][:c["N"]],
                      act_silu=int(c["silu"]), resid=int(c["resid"]), nt_weights=c["nt"], y_tiled=c["y_tiled"])
            if quant:
                kw.update(scales=p.wg["scales"][:c["N"]], biases=p.wg["biases"][:c["N"]])
            if epi == 2:
                kw.update(W_up=p.wu["W"][:c["N"]])
                if quant:
                    kw.update(scales_up=p.wu["scales"][:c["N"]], biases_up=p.wu["biases"][:c["N"]])
            if c["bias"]:
                kw.update(bias=p.bias[:c["N"]])
            if norm:
                kw.update(norm_w=p.norm_w, ss_in=np.ones((p.ssc, d["ss_ld"]), np.float32), norm_dim=c["K"], norm_eps=EPS)
            got = m.debug_gemm(**kw)
            assert {k: got[k] for k in want} == want, c["name"]
    _POOLS.clear()


@pytest.mark.gpu
def test_bad_arguments_are_refused_on_the_host(engines):
    """Nothing a caller passes becomes an index on the GPU unchecked: each of these returns INVALID_INPUT (3) before anything
    is launched -- among them 257 partial sums for launch_norm_rows, whose job folds at most 256 -- and a good call afterwards
    gives what it gave before."""
    from qwen3tts import Qwen3TTSError
    m = engines["tiny-a"]
    rng = np.random.default_rng(5)
    K, N, M = 256, 32, 20
    x, W = f2b(rng.standard_normal((32, K))), f2b(rng.standard_normal((N, K)) * 0.03)
    y = np.full((32, N), SENT, np.uint16)
    good = m.debug_gemm(x=x, W=W, y=y, M=M)["y"]
    h, w = f2b(rng.standard_normal((16, K))), f2b(np.ones(K))

    def rider(n_ss):
        return dict(h=h, w=w, out=np.zeros_like(h), M=16, ss_in=np.ones((n_ss, 16), np.float32))

    assert m.debug_gemm(mode=1, rider=rider(256))["rider_out"].shape == h.shape
    bad = [
        dict(mode=1, rider=rider(257)),
        dict(x=x, W=W, y=y, M=33),                                  # more rows than the x / y allocations hold
        dict(x=x, W=W, y=y, M=0),
        dict(x=x, W=W, y=y, M=M, epi=1),
        dict(x=x, W=W[:24], y=y, M=M),                              # N no multiple of 16
        dict(x=x[:, :192], W=W[:, :192], y=y, M=M),                 # K no multiple of 128
        dict(x=x, W=W, y=y, M=M, y_tiled=1),                        # fragment-major y needs whole 128-column chunks
        dict(x=x, W=W, y=y[:, :24], M=M),                           # y narrower than N
        dict(x=x, W=W, y=y, M=M, epi=2),                            # gate without up
        dict(x=x, W=W, y=y, M=M, norm_w=w),                         # prologue without partial sums
        dict(x=x, W=W, y=y, M=M, norm_w=w, ss_in=np.ones((4, 16), np.float32), norm_dim=K),  # ss_ld below Mpad
        dict(x=x, W=W, y=y, M=M, resid=1),                          # residual outside epi 3
        dict(x=x, W=W, y=y, M=M, rider=dict(h=h, w=w, out=np.zeros_like(h), M=17)),          # rider rows beyond its buffer
    ]
    for kw in bad:
        with pytest.raises(Qwen3TTSError) as e:
            m.debug_gemm(**kw)
        assert e.value.status == 3, sorted(kw)
    again = m.debug_gemm(x=x, W=W, y=y, M=M)["y"]
    assert (again == good).all() and (again[M:] == SENT).all()
