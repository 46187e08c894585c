"""Block-level parity of the codec decoder's convolutions (csrc/kernels/codec_conv.hip, codec_conv_h1.hip and the out-convs of
codec_misc.hip / codec_conv_h1.hip) through q3tts_debug_conv: one launch of the product's own launcher per case, on caller-built
host buffers, against a float64 reference written here:

  out = res + scale * act(bias + sum_{tap,ci} W[n][tap][ci] * A(t - (K-1-tap)*dil + shift, ci)),   out2 = SnakeBeta_post(out)

A is the input after pre-add, ELU and SnakeBeta, with zero or reflect padding or the `hist` rows of the previous chunk.

Rounding points of the reference. fp32 and fp16x2 paths: inputs are the exact fp32 values and the reference does not round.
float16 kinds (header of codec_conv_h1.hip, OracleModel._main_decoder16): fp16(acc), fp16(+ bias), fp16(res + .), SnakeBeta as
t = fp16(x ea), s = fp16(sin t), q = fp16(s s), r = fp16(ib q), y = fp16(x + r), and an fp32 input (x_f32) rounded to float16
first; float64 is rounded to float16 directly. The fused units are the same composition of two convs and two activations.

Bars (e = 2^-24 is half an fp32 step, u = 2^-11 half a float16 step, S = sum |w x| of the element, E = the
operand error carried in, sum |w| dA). Never a constant floor: where the sum cancels, the accumulation term is what is left.
  fp32 MFMA   A = (K * 32 * ceil(Cin / 32) + 3) e (S + |bias|) + E        the fmaf chain in index order (kernel comment) and
              the epilogue's three operations
  fp16x2      A = 1.25 * 2^-22 S                                           operand splitting 2^-22 worst case + the dropped
                + (3 steps + 32 + 3) e (S + |bias|)                        C xl' term (2^-12 * 2^-12); three 32-wide MFMAs per
                + 2^-38 rowmax_n sum |x| + 2^-36 sum |w| + E               (tap, chunk) step chained in fp32, at most 32 roundings
              inside one; lo planes of elements 2^-15 below the row maximum and of inputs below 2^-14 are subnormal (absolute
              2^-25 of the scaled value). The 2^-s rescale is exact.
  epilogue    t = acc + bias within A;  g = act(t): |g'(t)| A + Eact(t);  * scale: |scale| . + e |v|;  + res: + e |out|.
              Eact: GELU(erf) 0.5 |t| (2^-21 + 2^-24 + 2^-23) + 3 e |g| (erff within 4 steps, its argument's rounding times
              |z erf'(z)| <= 0.5, the addition); GELU(tanh) 0.5 |t| (2^-22 + 5 e + 2^-23) + 3 e |g|; ReLU exact; sigmoid 2^-22 |g|
              (expf one step, addition, division); tanh(ReLU) 2^-22 |g|.
  SnakeBeta   f = v + ib sin^2(ea v) in fp32 on an input within dv: with a = |ea v|,
              df = dv + |ib| (Esin + 3 e a + |ea| dv) + 4 e |ib sin^2| + e |f|        (|d sin^2 / da| <= 1; ea, ib come from expf:
              one step each, plus the product's and the quotient's roundings). Esin = 1.2e-7 for snake_sin2 (snake.h), 5 e for
              sinf squared (one step of the sine, doubled by the square, plus the square's rounding). |ea v| stays below 8, so the
              argument's own rounding, 3 e a, is below 1.5e-6 and is carried explicitly.
  ELU         v <= 0: 2^-23 + e |r| (expf one step of a value <= 1, the subtraction); x2 pre-add: e |x + x2|.
  float16     accumulation A = (steps + 32) e S + E (products exact, one MFMA per step); at every rounding point both sides round
              numbers at most A apart, so the results are at most one float16 step + A apart (as test_gemm_block.py):
              d(t) = step(t) + (1 + 4u) A, and 0 where A is 0. step(t) is the float16 spacing at the reference value, between
              u |t| (just below a power of two) and 2u |t| (just above one). (Written as u |t| + (1 + 2u) A with u = 2^-11 the
              bar is half a step for most values and correct arithmetic leaves it: the CPU restatement itself did, 3 of 34952
              elements of h1-n136-k1-t257 at 2^-9 against 1.07e-3 -- a mistake in that derivation, not in a kernel.) The sine is
              the one place where A is tiny against a step: there the allowance is one step only where a rounding boundary lies
              within 2^-22 |s| of the float64 sine, else nothing.
  Where a float16 launch writes out and out2, out2 is also held against the float16 SnakeBeta of the launch's own out: equal, but
  for a sine on a rounding boundary (fewer than 2 % of the elements).
  No element is exempt. Every float16 conv output (`out`, with or without bias and residual) may differ from the reference in
  fewer than 2 % of its elements; the inputs are chosen such that the CPU restatement stays under 1 %.
  out-convs   fp32: A = (7 C + 3) e (S + |bias|) + E, then clip (1-Lipschitz); float16: the float16 rule on fp16(acc), fp16(+ bias).

Sentinels (a NaN bit pattern): input rows >= T and whole rows of empty batch entries, input columns >= Cin, the rows in front of
the `hist` rows, all of out / out2 / pcm before the launch. After it every position < T and channel < N is finite and inside its
bar, everything else keeps its bits, and nonfinite[b] changes only for a row that holds a non-finite value.

Bit-exact equivalences (== on raw bits). The pointwise kernel against conv_gemm_h2_kernel<BN, false> (Q3TTS_CONV_NO_PW), claimed
by the kernel's comment. Derived here from the code: per output element the MFMA sequence -- (chunk, tap) steps in order, a
step's products smallest first, each MFMA the same 32 (or 4) k values -- depends only on Cin, K and the kernel family, never on
the element's place in a tile, the tile width, the batch row, the strides or the launch that computes it; rows a causal conv
finds in the `hist` margin are the rows it would have found in the tensor. So the same sequence gives the same bits as B = 1,
as a row of a ragged B = 3 batch, cut in two streamed launches and with padded strides; the first N' channels do not depend
on BN (N = 128 / 96 / 64); res aliased with out equals res apart; out2 alone equals out2 beside out. A fused unit against its
two convs as launches is compared under the bars only (attach_h2_perm / attach_h1_perm change the summation order).

Instantiations the launchers can dispatch (29), all reached by the case table (test_case_table_reaches_every_instantiation):
  conv_gemm_kernel<128 | 96 | 64>                              3      conv_pw_h2_kernel<128 | 96 | 64, 2>            3
  conv_gemm_h2_kernel<128 | 96 | 64, PRO false | true>         6      resunit_h2_kernel<2,2 | 4,2 | 6,4 | 12,2>      4
  conv_gemm_h1_kernel<128 | 96 | 64, 1 | 2 | 7, false>         9      conv_gemm_h1_kernel<128, 7, true>              1
  resunit_h1_kernel<6, 4>                                      1      out_conv_kernel, out_conv_h1_kernel            2

The CPU part (no marker) asserts that coverage through geometry_only (host code), runs every case through a float32 / float16
restatement of the kernels' walk (the loader's row shifts and two-plane split, three products smallest first per (chunk, tap)
step, the fp32 kernel's fmaf chain, the float16 epilogue roundings) against the float64 reference under the same bars and the
same differing-share cap, and checks the host refusals."""
import zlib

import numpy as np
import pytest

E24 = 2.0 ** -24
U16 = 2.0 ** -11
SENT_F = np.uint32(0x7FC12345)     # a NaN: what must not be read poisons the output, what must not be written keeps these bits
SENT_H = np.uint16(0x7E31)
ESIN2 = 1.2e-7                     # snake_sin2 (snake.h)
ESINF2 = 5 * E24                   # sinf squared
SEQ_ROWS = 2400
OFF = 64                           # a sequence's position 0 within its pool (room for the hist rows in front)
FAMILY = {0: "f32", 1: "h2", 2: "pw", 3: "unit", 4: "h1", 5: "unit_h1", 6: "out", 7: "out_h1"}
WORST = {}                         # path -> worst error / bar seen in this process (printed by the tests)


def r16(x):
    """float64 -> nearest-even float16 value, held in float64 (numpy converts directly: no double rounding through fp32)."""
    return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def ulp16(v):
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -14))) - 10)


def step16(t, A):
    """Both sides round to float16 two numbers at most A apart; t: the reference's rounded value. One float16 step at t (between
    u |t| and 2u |t|) plus A."""
    return np.where(A > 0, ulp16(t) + (1 + 4 * U16) * A, 0.0)


def near_boundary(v, A):
    """One float16 step where a rounding boundary lies within A of v, else nothing (A far below a step)."""
    ul = ulp16(np.abs(v) + A)
    frac = np.abs(v) / ul
    dist = np.abs(frac - np.floor(frac) - 0.5) * ul
    return np.where(dist <= A, ul, 0.0)


def rng_of(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ---------------------------------------------------------------------------------------------
# inputs: pools shared by every case that names the same content
# ---------------------------------------------------------------------------------------------
_POOL = {}


def pool(key, make):
    if key not in _POOL:
        _POOL[key] = make()
    return _POOL[key]


def seq(tag, h1, C, scale=1.0):
    """[SEQ_ROWS][C] activation rows; float16-exact for the float16 kinds."""
    def make():
        x = (rng_of("seq", tag, C).standard_normal((SEQ_ROWS, C)) * scale).astype(np.float32)
        return x.astype(np.float16).astype(np.float32) if h1 else x
    return pool(("seq", tag, h1, C, scale), make)


def weights(tag, h1, K, Cin, gain=1.0):
    """[192][K][Cin]: a case takes the first N rows. Row magnitudes spread over a factor 16 downwards (the loader's row shifts
    differ; outputs stay of order 1, so that every SnakeBeta argument stays below about 8)."""
    def make():
        r = rng_of("w", tag, K, Cin)
        w = r.standard_normal((192, K, Cin)) * (gain / np.sqrt(K * Cin)) * 2.0 ** r.integers(-4, 1, (192, 1, 1))
        w = w.astype(np.float32)
        return w.astype(np.float16).astype(np.float32) if h1 else w
    return pool(("w", tag, h1, K, Cin, gain), make)


def vec(tag, h1, n, scale=0.3):
    def make():
        v = (rng_of("vec", tag, n).standard_normal(n) * scale).astype(np.float32)
        return v.astype(np.float16).astype(np.float32) if h1 else v
    return pool(("vec", tag, h1, n, scale), make)


def snake_raw(tag, h1, C):
    """Raw (alpha, beta). float16 kinds: float16-exact values whose exp (and reciprocal) sit away from a float16 rounding boundary,
    so that expf's last bit cannot change the parameter the loader rounds."""
    def make():
        r = rng_of("snake", tag, C)
        al, be = r.uniform(-0.5, 0.2, C).astype(np.float32), r.uniform(-0.5, 0.5, C).astype(np.float32)
        if h1:
            al, be = al.astype(np.float16), be.astype(np.float16)
            for _ in range(8):
                ea = np.exp(al.astype(np.float64))
                bad = near_boundary(ea, 2.0 ** -20 * ea) > 0
                al = np.where(bad, np.nextafter(al, np.float16(1)), al)
                eb = np.exp(be.astype(np.float64))
                bad = (near_boundary(eb, 2.0 ** -20 * eb) > 0) | (near_boundary(1.0 / r16(eb), 2.0 ** -20) > 0)
                be = np.where(bad, np.nextafter(be, np.float16(1)), be)
            al, be = al.astype(np.float32), be.astype(np.float32)
        return al, be
    return pool(("snake", tag, h1, C), make)


def snake_f32_params(raw):
    al, be = raw[0].astype(np.float64), raw[1].astype(np.float64)
    return np.exp(al), 1.0 / (np.exp(be) + 1e-9)


def snake_f16_params(raw):
    al, be = raw[0].astype(np.float64), raw[1].astype(np.float64)
    return r16(np.exp(r16(al))), r16(1.0 / r16(np.exp(r16(be))))


# ---------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------
def case(name, kind, Cin, N, K, dil, T=None, rows=None, ppf=1, Tmax=None, **kw):
    """rows: [(sequence id, first row of the sequence, frames)] per batch entry; T: one entry with T positions."""
    c = dict(name=name, kind=kind, Cin=Cin, N=N, K=K, dil=dil, ppf=ppf, split=0, hist=0, margin=None, ldx=Cin, ldo=N, ldr=N, ldx2=Cin,
             bias=False, bias2=False, scale=False, res=False, res_is_out=False, out=True, out2=False, post_C=0, snake=False,
             act=0, pre_act=0, x2=False, shift=0, reflect=0, x_f32=0, tag="t", gain=1.0, inf_at=None, env={})
    c.update(kw)
    c["rows"] = rows if rows is not None else [(0, 0, T)]
    if c["margin"] is None:
        c["margin"] = c["hist"]
    need = max(c["margin"] + f * ppf for _, _, f in c["rows"])
    c["Tmax"] = Tmax if Tmax is not None else need + 3
    if c["out2"] and not c["post_C"]:
        c["post_C"] = N
    c["h1"] = kind in (2, 3, 5)
    return c


RAG = dict(rows=[(0, 0, 25), (1, 0, 0), (2, 0, 17)], ppf=8)
EPI = dict(bias=True, scale=True, res=True)


def conv_cases(kind, split, pre):
    """One list serves conv_gemm_kernel, the fp16x2 kernels and the float16 kernel: the N tails, Cin chunk counts and tails, (K, dil) pairs and Tmax values around the tile edges."""
    h1 = kind == 2
    c4, c132 = (8, 136) if h1 else (4, 132)
    k3 = (7, 3) if h1 else (3, 2)          # the float16 kernel takes 1, 2 or 7 taps
    kw = dict(split=split)
    epi = dict(bias=True, res=True) if h1 else EPI
    acts = [0] * 6 if h1 else ([1, 2, 3, 4, 5, 0] if not split else [1, 0, 1, 0, 1, 0])
    L = [
        case(pre + "n128-k7d9-t200", kind, 40, 128, 7, 9, T=200, act=acts[0], **epi, **kw),
        case(pre + "n96-k3-t129", kind, 32, 96, *k3, T=129, act=acts[1], out2=True, **kw),
        case(pre + "n72-k2-t65", kind, c132, 72, 2, 1, T=65, act=acts[2], bias=True, **kw),
        case(pre + "n136-k1-t257", kind, c4, 136, 1, 1, T=257, act=acts[3], **kw),
        case(pre + "n4-k7d3-t63", kind, 64, 4, 7, 3, T=63, act=acts[4], res=True, **kw),
        case(pre + "n192-k7-t127", kind, 96, 192, 7, 1, T=127, out=False, out2=True, post_C=96, **kw),
        case(pre + "n64-k2-t128", kind, 40, 64, 2, 1, T=128, bias=True, **kw),
        case(pre + "n128-k2-t130", kind, 64, 128, 2, 1, T=130, res=True, **kw),
        case(pre + "n96-k2-t64", kind, 32, 96, 2, 1, T=64, bias=True, **kw),
        case(pre + "n64-k7d9-t1", kind, 32, 64, 7, 9, T=1, **kw),
        case(pre + "n128-k1-t64", kind, 96, 128, 1, 1, T=64, bias=True, res=True, res_is_out=True, **kw),
        case(pre + "n96-k1-c40", kind, 40, 96, 1, 1, T=130, out2=True, **kw),
        case(pre + "n64-k1-c132", kind, c132, 64, 1, 1, T=129, **kw),
        case(pre + "n72-k1-c64", kind, 64, 72, 1, 1, T=127, bias=True, **kw),
        case(pre + "ragged", kind, 40, 72, 7, 1, **RAG, hist=8, margin=16, ldx=48, ldo=80, ldr=88, **epi, **kw),
        case(pre + "ragged-k1", kind, 40, 136, 1, 1, **RAG, ldx=56, ldo=144, out2=True, post_C=68, **kw),
    ]
    # the XCD-contiguous tile order at workgroup counts that are no multiple of 8 (and 1): 1, 3, 7, 9, 15, 17
    for K in (1, 2):
        for wg, g in ((1, dict(T=100)), (3, dict(T=300)), (7, dict(T=800)), (9, dict(rows=[(0, 0, 300), (1, 0, 290), (2, 0, 257)])),
                      (15, dict(rows=[(0, 0, 600), (1, 0, 513), (2, 0, 0)])), (17, dict(T=2100))):
            L.append(case(pre + "wg%d-k%d" % (wg, K), kind, 8, 8, K, 1, wg=wg, **g, **kw))
    return L


def pro_cases(split, pre):
    """The voice-clone prologues: conv_gemm_kernel, and conv_gemm_h2_kernel<*, true> through `split`."""
    kw = dict(split=split, tag="p")
    return [
        case(pre + "snake-n128", 0, 40, 128, 7, 3, T=140, snake=True, bias=True, **kw),
        case(pre + "elu-n96", 0, 32, 96, 7, 1, T=129, pre_act=1, **kw),
        case(pre + "x2-n64", 0, 64, 64, 3, 2, T=70, x2=True, ldx2=72, **kw),
        case(pre + "x2-elu-k1", 0, 40, 72, 1, 1, T=65, x2=True, pre_act=1, **kw),
        case(pre + "shift-zero", 0, 32, 64, 7, 1, T=5, shift=3, **kw),
        case(pre + "shift-reflect", 0, 32, 64, 7, 1, T=5, shift=3, reflect=1, **kw),
        case(pre + "shift-reflect-d2", 0, 36, 128, 3, 2, T=131, shift=2, reflect=1, snake=True, **kw),
        case(pre + "shift-k1pro", 0, 32, 96, 1, 1, T=64, snake=True, out2=True, **kw),
    ]


def unit_cases(kind):
    pre = "unit-" if kind == 1 else "unit16-"
    L = []
    for C, around in ((96, 256),) if kind == 3 else ((32, 128), (64, 128), (96, 256), (192, 128)):
        for i, dil in enumerate((1, 3, 9)):
            T = around + (-1, 0, 1)[i]
            L.append(case(pre + "c%d-d%d" % (C, dil), kind, C, C, 7, dil, T=T, snake=True, bias=i != 1, bias2=i != 2, out2=i != 0, tag="u"))
    L.append(case(pre + "ragged", kind, 96, 96, 7, 9, **RAG, hist=56, margin=64, snake=True, bias=True, bias2=True, out2=True, tag="u"))
    L.append(case(pre + "t1", kind, 96, 96, 7, 3, T=1, snake=True, tag="u"))
    return L


def out_cases(kind):
    pre = "out-" if kind == 4 else "out16-"
    L = [case(pre + "c%d" % C, kind, C, 4, 7, 1, T=T, snake=True, bias=True, out=False, tag="o", gain=1.6) for C, T in ((4, 63), (32, 64), (96, 65))]
    L.append(case(pre + "ragged-inf", kind, 32, 4, 7, 1, rows=[(0, 0, 9), (1, 0, 0), (2, 0, 8)], ppf=8, hist=8, margin=12, snake=True, bias=True,
                  out=False, tag="o", gain=1.6, inf_at=(2, 30, 5)))
    if kind == 5:
        L.append(case(pre + "nobias", kind, 32, 4, 7, 1, T=70, snake=True, out=False, tag="o", gain=1.6))
    return L


GROUPS = {
    "f32": conv_cases(0, 0, "f32-") + pro_cases(0, "f32-"),
    "h2": conv_cases(0, 1, "h2-") + pro_cases(1, "h2pro-"),
    "h1": conv_cases(2, 0, "h1-") + [case("h1-x32-n128", 2, 136, 128, 7, 1, T=129, x_f32=1, bias=True, out2=True),
                                     case("h1-x32-ragged", 2, 40, 128, 7, 3, **RAG, hist=24, margin=24, x_f32=1, ldx=48)],
    "unit": unit_cases(1),
    "unit_h1": unit_cases(3),
    "out": out_cases(4),
    "out_h1": out_cases(5),
}
ALL_CASES = [c for g in GROUPS.values() for c in g]


def geometry(c, env_no_pw=False):
    from qwen3tts import _lib
    outc = c["kind"] >= 4
    return _lib.conv_geometry(
        frames=[f for _, _, f in c["rows"]], kind=c["kind"], split=c["split"], B=len(c["rows"]), Tmax=c["Tmax"], ppf=c["ppf"], hist=c["hist"],
        margin=c["margin"], Cin=c["Cin"], N=c["N"], K=c["K"], dil=c["dil"], ldx=c["ldx"], ldo=0 if outc else c["ldo"],
        ldr=c["ldo"] if c["res_is_out"] else (c["ldr"] if c["res"] else 0), ldx2=c["ldx2"] if c["x2"] else 0, act=c["act"], pre_act=c["pre_act"],
        shift=c["shift"], reflect=c["reflect"], post_C=c["post_C"] if (c["out2"] and c["kind"] in (0, 2)) else 0, x_f32=c["x_f32"],
        res_is_out=int(c["res_is_out"]), x2=c["x2"], bias=c["bias"], bias2=c["bias2"], scale=c["scale"],
        snake=c["snake"], act2=c["kind"] in (1, 3), post=c["out2"], res=c["res"] and not c["res_is_out"], out=c["out"] and not outc,
        out2=c["out2"], w2=c["kind"] in (1, 3), pcm=outc, nonfinite=outc)


def instantiation(g):
    f = FAMILY[g["family"]]
    if f == "f32":
        return (f, g["BN"])
    if f == "h2":
        return (f, g["BN"], g["pro"])
    if f == "pw":
        return (f, g["BN"], g["pw_depth"])
    if f in ("unit", "unit_h1"):
        return (f, g["CT2"], g["PT"])
    if f == "h1":
        return (f, g["BN"], g["KT"], g["X32"])
    return (f,)


def dispatchable():
    s = {("f32", bn) for bn in (128, 96, 64)} | {("h2", bn, p) for bn in (128, 96, 64) for p in (0, 1)}
    s |= {("pw", bn, 2) for bn in (128, 96, 64)} | {("unit", ct, pt) for ct, pt in ((2, 2), (4, 2), (6, 4), (12, 2))}
    s |= {("h1", bn, kt, 0) for bn in (128, 96, 64) for kt in (1, 2, 7)} | {("h1", 128, 7, 1), ("unit_h1", 6, 4), ("out",), ("out_h1",)}
    return s


# ---------------------------------------------------------------------------------------------
# buffers of one case
# ---------------------------------------------------------------------------------------------
def build(c):
    """Host buffers as the launch takes them (sentinels everywhere a launch must neither read nor write) and the per-row views."""
    h1, kind, Cin, N, K = c["h1"], c["kind"], c["Cin"], c["N"], c["K"]
    B, Tmax, M, hist, ppf = len(c["rows"]), c["Tmax"], c["margin"], c["hist"], c["ppf"]
    outc = kind >= 4
    xin_f32 = not h1 or c["x_f32"]
    b = dict(frames=np.array([f for _, _, f in c["rows"]], np.int32))
    x = np.full((B, Tmax, c["ldx"]), SENT_F, np.uint32).view(np.float32) if xin_f32 else np.full((B, Tmax, c["ldx"]), SENT_H, np.uint16)
    x2 = np.full((Tmax, c["ldx2"]), SENT_F, np.uint32).view(np.float32) if c["x2"] else None
    res = None
    if c["res"] and not c["res_is_out"]:
        res = np.full((B, Tmax, c["ldr"]), SENT_H if h1 else SENT_F, np.uint16 if h1 else np.uint32)
        res = res if h1 else res.view(np.float32)
    mk_out = lambda: (np.full((B, Tmax, c["ldo"]), SENT_H, np.uint16) if h1 else np.full((B, Tmax, c["ldo"]), SENT_F, np.uint32).view(np.float32))
    out = mk_out() if (c["out"] and not outc) else None
    out2 = mk_out() if c["out2"] else None
    xs, rs, x2s = [], [], []
    for bi, (sid, s0, f) in enumerate(c["rows"]):
        T = f * ppf
        X = seq((c["tag"], sid), h1 and not c["x_f32"], Cin)
        rows = X[OFF + s0 - hist:OFF + s0 + T].copy()
        if c["inf_at"] and c["inf_at"][0] == bi:
            rows[hist + c["inf_at"][1], c["inf_at"][2]] = np.inf
        xs.append(rows)
        if T > 0:
            x[bi, M - hist:M + T, :Cin] = rows if xin_f32 else rows.astype(np.float16).view(np.uint16)
        Rr = seq((c["tag"], "res", sid), h1, N, 0.5)[OFF + s0:OFF + s0 + T] if (c["res"] or c["res_is_out"]) else None
        rs.append(Rr)
        if Rr is not None and T > 0:
            dst = out if c["res_is_out"] else res
            dst[bi, M:M + T, :N] = Rr.astype(np.float16).view(np.uint16) if h1 else Rr
        if c["x2"]:
            X2 = seq((c["tag"], "x2", sid), False, Cin)[OFF + s0 - hist:OFF + s0 + T]
            x2s.append(X2)
            x2[M - hist:M + T, :Cin] = X2
        else:
            x2s.append(None)
    nW = 1 if outc else N
    W = weights(c["tag"], h1 and not outc, K, Cin, c["gain"])[:nW]
    if outc:                                                # taps of unit norm: a waveform of order 1, which clips at +-1 here and there
        W = (W / np.sqrt((W.astype(np.float64) ** 2).sum())).astype(np.float32)
    b.update(x=x, x2=x2, res=res, out=out, out2=out2, W=W, xs=xs, rs=rs, x2s=x2s)
    b["bias"] = vec((c["tag"], "b"), h1, 192)[:nW] if c["bias"] else None
    b["bias2"] = vec((c["tag"], "b2"), h1, 192)[:N] if c["bias2"] else None
    b["scale"] = (1.0 + vec((c["tag"], "sc"), False, 192, 0.15)[:N]).astype(np.float32) if c["scale"] else None
    b["snake"] = snake_raw((c["tag"], "pre"), h1, Cin) if c["snake"] else None
    if kind in (1, 3):
        b["W2"] = weights((c["tag"], "2"), h1, 1, N)[:N, 0, :]
        b["act2"] = snake_raw((c["tag"], "a2"), h1, N)
    pc = N if kind in (1, 3) else c["post_C"]
    b["post"] = snake_raw((c["tag"], "post"), h1, pc) if c["out2"] else None
    if outc:
        b["pcm"] = np.full((B, Tmax), SENT_F, np.uint32).view(np.float32)
        b["nonfinite"] = np.array([4, 0, 2, 6][:B], np.int32)
    return b


def launch(m, c, b):
    kw = dict(frames=b["frames"], x=b["x"], w=b["W"], K=c["K"], dil=c["dil"], ppf=c["ppf"], hist=c["hist"], margin=c["margin"], split=c["split"],
              Cin=c["Cin"], N=c["N"], bias=b["bias"], bias2=b["bias2"], scale=b["scale"], snake=b["snake"], post=b["post"],
              post_C=c["post_C"] if c["kind"] in (0, 2) else 0, res=b["res"], res_is_out=int(c["res_is_out"]), out=b["out"], out2=b["out2"],
              x2=b["x2"], act=c["act"], pre_act=c["pre_act"], shift=c["shift"], reflect=c["reflect"], x_f32=c["x_f32"])
    if c["kind"] in (1, 3):
        kw.update(w2=b["W2"], act2=b["act2"])
    if c["kind"] >= 4:
        kw.update(pcm=b["pcm"], nonfinite=b["nonfinite"])
    return m.debug_conv(c["kind"], **kw)


# ---------------------------------------------------------------------------------------------
# the float64 reference and its bars
# ---------------------------------------------------------------------------------------------
def gather(T, K, dil, shift, reflect, hist):
    t = np.arange(T)[:, None] - (K - 1 - np.arange(K))[None, :] * dil + shift
    if reflect:
        t = np.where(t < 0, -t, np.where(t >= T, 2 * (T - 1) - t, t))
        return t, np.ones_like(t, bool)
    return t, (t >= -hist) & (t < T)


def conv64(A, dA, W, T, K, dil, shift=0, reflect=0, hist=0):
    """A, dA [hist + T][Cin] (row hist is position 0) -> acc, S = sum |w a|, E = sum |w| dA, SX = sum |a| over the window."""
    src, ok = gather(T, K, dil, shift, reflect, hist)
    N = W.shape[0]
    acc, S, E, SX = (np.zeros((T, N)) for _ in range(4))
    for k in range(K):
        idx = np.where(ok[:, k], src[:, k] + hist, 0)
        a = np.where(ok[:, k, None], A[idx], 0.0)
        da = np.where(ok[:, k, None], dA[idx], 0.0)
        Wk = W[:, k, :].astype(np.float64)
        acc += a @ Wk.T
        S += np.abs(a) @ np.abs(Wk).T
        E += da @ np.abs(Wk).T
        SX += np.abs(a).sum(1)[:, None]
    return acc, S, E, SX


def snake32(v, dv, par, esin):
    ea, ib = par
    u = v * ea
    assert not (np.abs(u[np.isfinite(u)]) > 10).any(), "a SnakeBeta argument beyond the range the bars are written for"
    s2 = np.sin(u) ** 2
    f = v + ib * s2
    return f, dv + np.abs(ib) * (esin + 3 * E24 * np.abs(u) + np.abs(ea) * dv) + 4 * E24 * np.abs(ib * s2) + E24 * np.abs(f)


def snake16(x, dx, par):
    ea, ib = par
    t = r16(x * ea)
    dt = step16(t, np.abs(ea) * dx)
    s64 = np.sin(t)
    s = r16(s64)
    ds = np.where(dt > 0, step16(s, np.abs(np.cos(t)) * dt + 2.0 ** -22 * np.abs(s64)), near_boundary(s64, 2.0 ** -22 * np.abs(s64)))
    q = r16(s * s)
    dq = step16(q, 2 * np.abs(s) * ds + ds * ds)
    r = r16(ib * q)
    dr = step16(r, np.abs(ib) * dq)
    y = r16(x + r)
    return y, step16(y, dx + dr)


def act64(t, act):
    from math import erf, pi, sqrt
    if act == 0:
        return t, np.ones_like(t), np.zeros_like(t)
    if act == 1:
        z = t / np.sqrt(2.0)
        Phi = 0.5 * (1 + np.vectorize(erf)(z))
        g = t * Phi
        return g, np.abs(Phi + t * np.exp(-z * z) / sqrt(2 * pi)), 0.5 * np.abs(t) * (2.0 ** -21 + 2.0 ** -24 + 2.0 ** -23) + 3 * E24 * np.abs(g)
    if act == 2:
        c = 0.7978845608
        w = c * (t + 0.044715 * t ** 3)
        th = np.tanh(w)
        g = 0.5 * t * (1 + th)
        dg = 0.5 * (1 + th) + 0.5 * t * (1 - th * th) * c * (1 + 3 * 0.044715 * t * t)
        return g, np.abs(dg), 0.5 * np.abs(t) * (2.0 ** -22 + 5 * E24 + 2.0 ** -23) + 3 * E24 * np.abs(g)
    if act == 3:
        return np.maximum(t, 0), np.ones_like(t), np.zeros_like(t)
    if act == 4:
        g = 1 / (1 + np.exp(-t))
        return g, g * (1 - g), 2.0 ** -22 * g
    g = np.tanh(np.maximum(t, 0))
    return g, np.ones_like(t), 2.0 ** -22 * g


def acc_bar(c, path, S, E, SX, W, bias):
    """The accumulation + operand bound of one conv on `path`."""
    K, Cin = W.shape[1], W.shape[2]
    steps = K * -(-Cin // 32)
    ab = 0.0 if bias is None else np.abs(bias.astype(np.float64))[None, :]
    if path == "f32":
        return (32 * steps + 3) * E24 * (S + ab) + E
    if path == "h2":
        rowmax = np.abs(W).max((1, 2)).astype(np.float64)[None, :]
        sw = np.abs(W).sum((1, 2)).astype(np.float64)[None, :]
        return 1.25 * 2.0 ** -22 * S + (3 * steps + 35) * E24 * (S + ab) + 2.0 ** -38 * rowmax * SX + 2.0 ** -36 * sw + E
    return (steps + 32) * E24 * S + E   # float16: products exact


def reference(c, b, bi):
    """Row bi of the case: dict(out, d_out, out2, d_out2, pcm, d_pcm, flag) in float64 over [T][N] (None where absent)."""
    kind, K, dil, hist, h1 = c["kind"], c["K"], c["dil"], c["hist"], c["h1"]
    T = c["rows"][bi][2] * c["ppf"]
    W = b["W"]
    x = b["xs"][bi].astype(np.float64)
    r = dict(out=None, d_out=None, out2=None, d_out2=None, pcm=None, d_pcm=None, flag=0, T=T)
    if T == 0:
        return r
    with np.errstate(all="ignore"):
        return _reference(c, b, bi, r, T)


def _reference(c, b, bi, r, T):
    kind, K, dil, hist, h1 = c["kind"], c["K"], c["dil"], c["hist"], c["h1"]
    W = b["W"]
    x = b["xs"][bi].astype(np.float64)
    path = "f32" if (kind in (0, 4) and not c["split"]) else ("h2" if kind in (0, 1) else "h1")
    esin = ESIN2 if kind in (1, 4) else ESINF2
    bias = b["bias"]
    b64 = 0.0 if bias is None else bias.astype(np.float64)[None, :]
    if kind in (0, 1, 4):                                   # ---- fp32 tensors ----
        dA = np.zeros_like(x)
        if c["x2"]:
            x = x + b["x2s"][bi].astype(np.float64)
            dA = E24 * np.abs(x)
        if c["pre_act"]:
            neg = x <= 0
            e = np.where(neg, np.expm1(np.minimum(x, 0)), x)
            dA = dA + np.where(neg | (x <= dA), 2.0 ** -23 + E24 * np.abs(e), 0.0)
            x = e
        if c["snake"]:
            x, dA = snake32(x, dA, snake_f32_params(b["snake"]), esin)
        acc, S, E, SX = conv64(x, dA, W, T, K, dil, c["shift"], c["reflect"], hist)
        A = acc_bar(c, path, S, E, SX, W, bias)
        if kind == 4:
            v = acc + b64
            A = (7 * c["Cin"] + 3) * E24 * (S + np.abs(b64)) + E
            fin = np.isfinite(v[:, 0])
            r["flag"] = int(not fin.all())
            r["pcm"], r["d_pcm"], r["fin"] = np.clip(v[:, 0], -1, 1), A[:, 0], fin
            return r
        if kind == 0:
            g, dg, eact = act64(acc + b64, c["act"])
            d = dg * A + eact
            if c["scale"]:
                sc = b["scale"].astype(np.float64)[None, :]
                g, d = g * sc, np.abs(sc) * d + E24 * np.abs(g * sc)
            if b["rs"][bi] is not None:
                g = g + b["rs"][bi].astype(np.float64)
                d = d + E24 * np.abs(g)
            out, d_out = g, d
        else:
            a2, d2 = snake32(acc + b64, A + E24 * np.abs(acc + b64), snake_f32_params(b["act2"]), ESIN2)
            W2 = b["W2"][:, None, :]
            acc2, S2, E2, SX2 = conv64(a2, d2, W2, T, 1, 1)
            bb = 0.0 if b["bias2"] is None else b["bias2"].astype(np.float64)[None, :]
            out = acc2 + bb + x0_rows(b, bi, hist)
            d_out = acc_bar(c, "h2", S2, E2, SX2, W2, b["bias2"]) + 2 * E24 * np.abs(out)
        r["out"], r["d_out"] = out, d_out
        if c["out2"]:
            ea, ib = snake_f32_params(b["post"])
            reps = c["N"] // ea.shape[0]
            r["out2"], r["d_out2"] = snake32(out, d_out, (np.tile(ea, reps)[None, :], np.tile(ib, reps)[None, :]), ESIN2)
        return r
    # ---- float16 tensors ----
    x = r16(x)                                              # (x_f32: rounded while staged)
    dA = np.zeros_like(x)
    if kind in (3, 5):
        x, dA = snake16(x, dA, snake_f16_params(b["snake"]))
    acc, S, E, SX = conv64(x, dA, W, T, K, dil, 0, 0, hist)   # (kind 5: the out-conv's taps are fp32)
    A = acc_bar(c, "h1", S, E, SX, W, None)
    if kind == 5:
        A = (7 * c["Cin"] + 3) * E24 * S + E                # fp32 products of fp32 taps: an fmaf chain per lane, two shuffles
    v = r16(acc)
    d = step16(v, A)
    if bias is not None:
        v = r16(v + b64)
        d = step16(v, d)
    if kind == 5:
        fin = np.isfinite(v[:, 0])
        r["flag"] = int(not fin.all())
        r["pcm"], r["d_pcm"], r["fin"] = np.clip(v[:, 0], -1, 1), d[:, 0], fin
        return r
    if kind == 2:
        if b["rs"][bi] is not None:
            v = r16(b["rs"][bi].astype(np.float64) + v)
            d = step16(v, d)
    else:
        a2, d2 = snake16(v, d, snake_f16_params(b["act2"]))
        W2 = b["W2"][:, None, :]
        acc2, S2, E2, SX2 = conv64(a2, d2, W2, T, 1, 1)
        v = r16(acc2)
        d = step16(v, acc_bar(c, "h1", S2, E2, SX2, W2, None))
        if b["bias2"] is not None:
            v = r16(v + b["bias2"].astype(np.float64)[None, :])
            d = step16(v, d)
        v = r16(r16(x0_rows(b, bi, hist)) + v)
        d = step16(v, d)
    r["out"], r["d_out"] = v, d
    if c["out2"]:
        ea, ib = snake_f16_params(b["post"])
        reps = c["N"] // ea.shape[0]
        r["out2"], r["d_out2"] = snake16(v, d, (np.tile(ea, reps)[None, :], np.tile(ib, reps)[None, :]))
    return r


def x0_rows(b, bi, hist):
    return b["xs"][bi][hist:].astype(np.float64)


_REF = {}


def ref_of(c, b, bi):
    key = (c["name"], bi)
    if key not in _REF:
        _REF[key] = reference(c, b, bi)
    return _REF[key]


# ---------------------------------------------------------------------------------------------
# checking one result (a launch's, or the CPU restatement's)
# ---------------------------------------------------------------------------------------------
def path_of(c):
    return {0: "h2" if c["split"] else "f32", 1: "unit", 2: "h1", 3: "unit_h1", 4: "out", 5: "out_h1"}[c["kind"]]


def to64(a, h1):
    return (a.view(np.float16) if h1 else a).astype(np.float64)


def note(path, ratio):
    WORST[path] = max(WORST.get(path, 0.0), float(ratio))


def check_values(c, b, got, shares):
    """got: dict(out, out2 [B][Tmax][ldo], pcm, nonfinite) as the launch returned them."""
    h1, M, N = c["h1"], c["margin"], c["N"]
    sent = SENT_H if h1 else SENT_F
    raw = lambda a: a if h1 else a.view(np.uint32)
    for bi in range(len(c["rows"])):
        r = ref_of(c, b, bi)
        T = r["T"]
        for name in ("out", "out2"):
            g = got.get(name)
            if g is None:
                continue
            keep = np.ones(g.shape[1:], bool)
            keep[M:M + T, :N] = False
            was = raw(b[name][bi])
            if c["res_is_out"] and name == "out":           # (the residual sat in out: it keeps ITS bits outside the valid region)
                assert np.array_equal(raw(g[bi])[keep], was[keep]), "%s: %s written outside [0, T) x [0, N), row %d" % (c["name"], name, bi)
            else:
                assert (raw(g[bi])[keep] == sent).all(), "%s: %s written outside [0, T) x [0, N), row %d" % (c["name"], name, bi)
            if T == 0:
                continue
            a = to64(g[bi, M:M + T, :N], h1)
            assert np.isfinite(a).all(), "%s: %s holds a non-finite value, row %d" % (c["name"], name, bi)
            err, bar = np.abs(a - r[name]), r["d_" + name]
            ok = err <= bar
            i = np.unravel_index(np.argmax(err - bar), err.shape)
            assert ok.all(), "%s: %s row %d [t %d][n %d] = %r, reference %r, bar %.3g (%d of %d outside)" % (
                c["name"], name, bi, i[0], i[1], a[i], r[name][i], bar[i], (~ok).sum(), ok.size)
            nz = bar > 0
            if nz.any():
                note(path_of(c) + ("" if name == "out" else "/out2"), (err[nz] / bar[nz]).max())
            if h1 and name == "out" and c["kind"] == 2:
                shares.append((c["name"], float((err > 0).mean()), err.size))
        if h1 and T > 0 and got.get("out") is not None and got.get("out2") is not None:
            # out2 is SnakeBeta of the launch's OWN out, op for op: the five float16 roundings leave no room but a sine that sits
            # on a rounding boundary (the accumulation's flips are in out already)
            own = to64(got["out"][bi, M:M + T, :N], True)
            ea, ib = snake_f16_params(b["post"])
            reps = N // ea.shape[0]
            y, dy = snake16(own, np.zeros_like(own), (np.tile(ea, reps)[None, :], np.tile(ib, reps)[None, :]))
            e2 = np.abs(to64(got["out2"][bi, M:M + T, :N], True) - y)
            assert (e2 <= dy).all(), "%s: out2 is not the float16 SnakeBeta of out, row %d: %d of %d elements, worst %.3g" % (
                c["name"], bi, (e2 > dy).sum(), e2.size, (e2 - dy).max())
            shares.append((c["name"] + "/snake", float((e2 > 0).mean()), e2.size))
        if c["kind"] >= 4:
            g = got["pcm"]
            keep = np.ones(g.shape[1], bool)
            keep[M:M + T] = False
            assert (g[bi].view(np.uint32)[keep] == SENT_F).all(), "%s: pcm written outside [0, T), row %d" % (c["name"], bi)
            want_flag = int(b["nonfinite"][bi]) | r["flag"]
            assert int(got["nonfinite"][bi]) == want_flag, "%s: nonfinite[%d] = %d, expected %d" % (c["name"], bi, got["nonfinite"][bi], want_flag)
            if T == 0:
                continue
            a = g[bi, M:M + T].astype(np.float64)
            fin = r["fin"]
            assert ((a[~fin] >= -1) & (a[~fin] <= 1)).all(), "%s: a non-finite sample must come out clipped" % c["name"]
            err, bar = np.abs(a - r["pcm"])[fin], r["d_pcm"][fin]
            assert np.isfinite(a[fin]).all() and (err <= bar).all(), "%s: pcm row %d off by %.3g (bar %.3g)" % (
                c["name"], bi, (err - bar).max(), bar[np.argmax(err - bar)])
            note(path_of(c), (err[bar > 0] / bar[bar > 0]).max() if (bar > 0).any() else 0.0)
            assert (np.abs(r["pcm"]) == 1).any() or c["name"].endswith("c4"), "%s: the case is meant to clip" % c["name"]


def check_shares(shares, cap):
    for name, share, n in shares:
        assert share < cap, "%s: %.2f %% of %d float16 outputs differ from the reference (cap %.0f %%)" % (name, 100 * share, n, 100 * cap)
    if shares:
        print("float16 conv outputs differing from the reference: worst %.3f %% (%s)" % (100 * max(s for _, s, _ in shares),
                                                                                        max(shares, key=lambda s: s[1])[0]))


# ---------------------------------------------------------------------------------------------
# CPU restatement of the kernels' walk
# ---------------------------------------------------------------------------------------------
f32 = np.float32


def fl32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def windows(c, T, K, dil, hist, shift=0, reflect=0):
    src, ok = gather(T, K, dil, shift, reflect, hist)
    return np.where(ok, src + hist, 0), ok


def walk_f32(A, W, idx, ok):
    """conv_gemm_kernel: one fmaf per (chunk, tap, channel) in index order, every accumulator on its own."""
    N, K, Cin = W.shape
    acc = np.zeros((idx.shape[0], N), np.float32)
    for c0 in range(0, Cin, 32):
        for k in range(K):
            a = np.where(ok[:, k, None], A[idx[:, k]], f32(0))
            for ci in range(c0, min(c0 + 32, Cin)):
                acc = fl32(acc.astype(np.float64) + a[:, ci, None].astype(np.float64) * W[None, :, k, ci].astype(np.float64))
    return acc


def split_x(a):
    xh = a.astype(np.float16)
    xl = ((a - xh.astype(np.float32)) * f32(2048)).astype(np.float16)
    return xh.astype(np.float64), xl.astype(np.float64)


def split_w(W):
    """The loader's row shifts (2^s brings a row's largest |w| into [2^13, 2^14)) and two-plane split."""
    mx = np.abs(W).reshape(W.shape[0], -1).max(1)
    s = np.clip(14 - np.frexp(mx)[1], -100, 100)
    ws = np.ldexp(W, s.reshape(-1, *[1] * (W.ndim - 1))).astype(np.float32)
    hi = ws.astype(np.float16)
    lo = (ws - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64), np.ldexp(np.float32(1), -s).astype(np.float32)


def walk_h2(A, W, idx, ok):
    """The fp16x2 kernels: per (chunk, tap) step three 32-wide products, smallest first, each added to the fp32 accumulator;
    the exact 2^-s rescale last."""
    N, K, Cin = W.shape
    hi, lo, sc = split_w(W)
    acc = np.zeros((idx.shape[0], N), np.float32)
    for c0 in range(0, Cin, 32):
        for k in range(K):
            a = np.where(ok[:, k, None], A[idx[:, k]], f32(0))[:, c0:c0 + 32]
            xh, xl = split_x(a)
            h, l = hi[:, k, c0:c0 + 32], lo[:, k, c0:c0 + 32]
            hs = (h.astype(np.float16) * np.float16(2.0 ** -11)).astype(np.float64)
            for p in (xl @ hs.T, xh @ l.T, xh @ h.T):
                acc = fl32(acc.astype(np.float64) + p)
    return acc * sc[None, :]


def walk_h1(A, W, idx, ok):
    N, K, Cin = W.shape
    acc = np.zeros((idx.shape[0], N), np.float32)
    W = W.astype(np.float64)
    for c0 in range(0, Cin, 32):
        for k in range(K):
            a = np.where(ok[:, k, None], A[idx[:, k]], 0.0)[:, c0:c0 + 32].astype(np.float64)
            acc = fl32(acc.astype(np.float64) + a @ W[:, k, c0:c0 + 32].T)
    return acc


def snake_w32(v, raw, libm=True):
    ea, ib = np.exp(raw[0]).astype(np.float32), (f32(1) / (np.exp(raw[1]).astype(np.float32) + f32(1e-9))).astype(np.float32)
    s = np.sin((v * ea).astype(np.float32)).astype(np.float32)
    return (v + ib * (s * s).astype(np.float32)).astype(np.float32)


def h(x):
    return np.asarray(x).astype(np.float16)


def snake_w16(x, raw):
    ea, ib = (h(v) for v in snake_f16_params(raw))
    t = x * ea
    s = h(np.sin(t.astype(np.float32)))
    q = s * s
    return x + ib * q


def act_w32(v, act):
    from math import erf
    if act == 1:
        return (f32(0.5) * v * (f32(1) + np.vectorize(erf)(v * f32(0.70710678)).astype(np.float32))).astype(np.float32)
    if act == 2:
        return (v * f32(0.5) * (f32(1) + np.tanh(f32(0.7978845608) * (v + f32(0.044715) * (v * v * v))))).astype(np.float32)
    if act == 3:
        return np.maximum(v, f32(0))
    if act == 4:
        return (f32(1) / (f32(1) + np.exp(-v))).astype(np.float32)
    return np.tanh(np.maximum(v, f32(0))).astype(np.float32)


def restate(c, b):
    """What the kernel of this case computes, restated in float32 / float16 numpy: buffers shaped like a launch's results."""
    kind, K, dil, hist, h1, M, N = c["kind"], c["K"], c["dil"], c["hist"], c["h1"], c["margin"], c["N"]
    got = dict(out=None if b["out"] is None else b["out"].copy(), out2=None if b["out2"] is None else b["out2"].copy())
    if kind >= 4:
        got.update(pcm=b["pcm"].copy(), nonfinite=b["nonfinite"].copy())
    W = b["W"]
    tile = lambda raw: (np.tile(raw[0], N // raw[0].shape[0]), np.tile(raw[1], N // raw[1].shape[0]))
    put = lambda name, bi, T, v: got[name].__setitem__((bi, slice(M, M + T), slice(0, N)), v.astype(np.float16).view(np.uint16) if h1 else v)
    with np.errstate(all="ignore"):
        for bi, (_, _, f) in enumerate(c["rows"]):
            T = f * c["ppf"]
            if T == 0:
                continue
            x = b["xs"][bi]
            idx, ok = windows(c, T, K, dil, hist, c["shift"], c["reflect"])
            if kind in (0, 1, 4):
                a = x.astype(np.float32)
                if c["x2"]:
                    a = (a + b["x2s"][bi]).astype(np.float32)
                if c["pre_act"]:
                    a = np.where(a > 0, a, (np.exp(np.minimum(a, 0)).astype(np.float32) - f32(1))).astype(np.float32)
                if c["snake"]:
                    a = snake_w32(a, b["snake"])
                if kind == 4:
                    v = walk_f32(a, W, idx, ok)[:, 0] + b["bias"][0]
                    got["pcm"][bi, M:M + T] = np.clip(np.where(np.isnan(v), f32(-1), v), -1, 1)
                    got["nonfinite"][bi] |= int(not np.isfinite(v).all())
                    continue
                acc = (walk_h2 if (c["split"] or kind == 1) else walk_f32)(a, W, idx, ok)
                v = acc if b["bias"] is None else (acc + b["bias"][None, :]).astype(np.float32)
                if kind == 0:
                    if c["act"]:
                        v = act_w32(v, c["act"])
                    if c["scale"]:
                        v = (v * b["scale"][None, :]).astype(np.float32)
                    if b["rs"][bi] is not None:
                        v = (v + b["rs"][bi]).astype(np.float32)
                else:
                    a2 = snake_w32(v, b["act2"])
                    i1, o1 = windows(c, T, 1, 1, 0)
                    v = walk_h2(a2, b["W2"][:, None, :], i1, o1)
                    if b["bias2"] is not None:
                        v = (v + b["bias2"][None, :]).astype(np.float32)
                    v = (v + x[hist:]).astype(np.float32)
                if got["out"] is not None:
                    put("out", bi, T, v)
                if c["out2"]:
                    put("out2", bi, T, snake_w32(v, tile(b["post"])))
                continue
            a = h(x)
            if kind in (3, 5):
                a = snake_w16(a, b["snake"])
            acc = walk_h1(a.astype(np.float32), W, idx, ok)
            v = h(acc)
            if b["bias"] is not None:
                v = v + h(b["bias"])[None, :]
            if kind == 5:
                p = v[:, 0].astype(np.float32)
                got["pcm"][bi, M:M + T] = np.clip(np.where(np.isnan(p), f32(-1), p), -1, 1)
                got["nonfinite"][bi] |= int(not np.isfinite(p).all())
                continue
            if kind == 2:
                if b["rs"][bi] is not None:
                    v = h(b["rs"][bi]) + v
            else:
                a2 = snake_w16(v, b["act2"])
                i1, o1 = windows(c, T, 1, 1, 0)
                v = h(walk_h1(a2.astype(np.float32), b["W2"][:, None, :], i1, o1))
                if b["bias2"] is not None:
                    v = v + h(b["bias2"])[None, :]
                v = h(x[hist:]) + v
            if got["out"] is not None:
                put("out", bi, T, v)
            if c["out2"]:
                put("out2", bi, T, snake_w16(v, tile(b["post"])))
    return got


# ---------------------------------------------------------------------------------------------
# CPU tests
# ---------------------------------------------------------------------------------------------
def test_case_table_reaches_every_instantiation():
    """Through geometry_only (host code, the dispatch functions the launchers switch on): the case table reaches exactly the
    instantiations the launchers can dispatch, the pointwise cases reach conv_gemm_h2_kernel<BN, false> under Q3TTS_CONV_NO_PW, the
    workgroup counts 1, 3, 7, 9, 15 and 17 occur on every kernel with the XCD-contiguous tile order, and wdb is as derived."""
    from qwen3tts import _lib
    _lib.reload_debug_env()
    seen, wgs = set(), {}
    for c in ALL_CASES:
        g = geometry(c)
        seen.add(instantiation(g))
        if "wg" in c:
            assert g["grid_x"] * g["grid_y"] * g["grid_z"] == c["wg"], c["name"]
            wgs.setdefault(FAMILY[g["family"]], set()).add(c["wg"])
        if c["kind"] == 1:   # conv1's weight tiles are double-buffered where (rows + 2 C) * 160 B fit 80 KiB: never at C = 192
            rows = (256 if c["N"] == 96 else 128) + 6 * c["dil"]
            assert g["wdb"] == int((rows + 2 * c["N"]) * 160 <= 80 * 1024) == int(c["N"] != 192), c["name"]
            assert g["lds_bytes"] == (rows + (2 if g["wdb"] else 1) * c["N"]) * 160
        if c["kind"] == 0 and c["N"] in (72, 136):
            assert (g["BN"], g["grid_x"]) == ((64, 2) if c["N"] == 72 else (128, 2)), c["name"]   # a masked second tile
    assert seen == dispatchable(), "not reached: %r; unexpected: %r" % (sorted(dispatchable() - seen), sorted(seen - dispatchable()))
    assert len(seen) == 29
    for fam in ("h2", "pw", "h1"):
        assert wgs[fam] == {1, 3, 7, 9, 15, 17}, (fam, wgs[fam])
    print("instantiations reached (%d): %s" % (len(seen), sorted(seen)))


def test_no_pw_switch_selects_the_general_kernel(monkeypatch):
    from qwen3tts import _lib
    monkeypatch.setenv("Q3TTS_CONV_NO_PW", "1")
    _lib.reload_debug_env()
    try:
        n = 0
        for c in GROUPS["h2"]:
            g = geometry(c)
            assert FAMILY[g["family"]] == "h2", c["name"]
            n += c["K"] == 1 and not g["pro"]
        assert n >= 10
    finally:
        monkeypatch.delenv("Q3TTS_CONV_NO_PW")
        _lib.reload_debug_env()


@pytest.mark.parametrize("group", list(GROUPS))
def test_restated_walk_stays_inside_the_bars(group):
    """The float32 / float16 restatement of each kernel's walk against the float64 reference, under the bars and the share cap the
    GPU results get (the cap here: 1 %): the inputs sit inside the bars without the kernel."""
    shares = []
    for c in GROUPS[group]:
        b = build(c)
        check_values(c, b, restate(c, b), shares)
    check_shares(shares, 0.01)
    print("restatement, worst error / bar: %s" % {k: round(v, 4) for k, v in sorted(WORST.items())})


BASE = dict(kind=0, B=1, Tmax=64, ppf=1, Cin=32, N=64, K=7, dil=1, ldx=32, ldo=64, out=True, frames=[60])
REFUSED = {
    "halo": dict(K=7, dil=10),
    "halo-h1": dict(kind=2, K=7, dil=10),
    "h1-k3": dict(kind=2, K=3),
    "cin-mod4": dict(Cin=34, ldx=36),
    "n-mod4": dict(N=66, ldo=68),
    "ldx-mod4": dict(ldx=34),
    "ldo-mod4": dict(ldo=66),
    "ldx-small": dict(ldx=28),
    "h1-cin-mod8": dict(kind=2, Cin=36, ldx=40),
    "h1-ldx-mod8": dict(kind=2, ldx=36),
    "x2-batch": dict(B=2, frames=[60, 60], x2=True, ldx2=32),
    "x2-ldx2": dict(x2=True, ldx2=34),
    "out2-without-post": dict(out2=True, post_C=64),
    "out2-post_C-0": dict(out2=True, post=True, post_C=0),
    "out2-post_C-mod4": dict(out2=True, post=True, post_C=2),
    "h1-out2-post_C": dict(kind=2, out2=True, post=True, post_C=0),
    "x32-k1": dict(kind=2, K=1, x_f32=1, N=128, ldo=128),
    "x32-bn64": dict(kind=2, x_f32=1),
    "unit-c48": dict(kind=1, Cin=48, N=48, ldx=48, ldo=48, w2=True, snake=True, act2=True),
    "unit-halo": dict(kind=1, Cin=96, N=96, ldx=96, ldo=96, dil=10, w2=True, snake=True, act2=True),
    "unit16-c192": dict(kind=3, Cin=192, N=192, ldx=192, ldo=192, w2=True, snake=True, act2=True),
    "unit16-k3": dict(kind=3, Cin=96, N=96, ldx=96, ldo=96, K=3, w2=True, snake=True, act2=True),
    "unit-ld": dict(kind=1, Cin=96, N=96, ldx=104, ldo=96, w2=True, snake=True, act2=True),
    "reflect-wide": dict(reflect=1, shift=3, frames=[3]),
    "reflect-shift": dict(reflect=1, shift=6, frames=[5]),
    "shift-range": dict(shift=7),
    "act-range": dict(act=6),
    "frames-over": dict(frames=[65]),
    "margin": dict(hist=8, margin=4),
    "prologue-on-h1": dict(kind=2, snake=True),
    "out-conv-k": dict(kind=4, K=3, N=4, ldo=0, out=False, snake=True, bias=True, pcm=True),
    "out-conv-c": dict(kind=5, Cin=2000, ldx=2000, N=4, ldo=0, out=False, snake=True, pcm=True),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_host_refusals(name):
    """Every refusal precedes allocation: geometry_only with m == NULL returns INVALID_INPUT, and the base case is accepted."""
    from qwen3tts import _lib
    assert _lib.conv_geometry(**BASE)["family"] == 0
    with pytest.raises(ValueError, match="status 3"):
        _lib.conv_geometry(**{**BASE, **REFUSED[name]})


# ---------------------------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine(ckpt_dirs):
    from qwen3tts import Qwen3TTSModel
    m = Qwen3TTSModel.from_pretrained(ckpt_dirs["tiny-a"], max_batch=1, max_frames=8, max_prompt=16)
    yield m
    m.close()


@pytest.fixture
def no_pw(monkeypatch):
    from qwen3tts import _lib

    def set_(on):
        if on:
            monkeypatch.setenv("Q3TTS_CONV_NO_PW", "1")
        else:
            monkeypatch.delenv("Q3TTS_CONV_NO_PW", raising=False)
        _lib.reload_debug_env()
    yield set_
    set_(False)


def valid(c, got, name):
    """The valid elements of a result, batch row by batch row."""
    M, N = c["margin"], c["N"]
    if name == "pcm":
        return [got["pcm"][bi, M:M + f * c["ppf"]].view(np.uint32) for bi, (_, _, f) in enumerate(c["rows"])]
    return [got[name][bi, M:M + f * c["ppf"], :N] for bi, (_, _, f) in enumerate(c["rows"])]


@pytest.mark.gpu
@pytest.mark.parametrize("group", list(GROUPS))
def test_conv_block_matches_float64(engine, no_pw, group):
    """Every case of the group: one launch, the reported geometry equal to geometry_only's, every valid element finite and inside
    its bar, every sentinel intact; float16 conv outputs differ from the reference in fewer than 2 % of the elements. The
    pointwise cases run a second time through conv_gemm_h2_kernel<BN, false> and must give the same bits."""
    from qwen3tts import _lib
    shares = []
    for c in GROUPS[group]:
        b = build(c)
        got = launch(engine, c, b)
        assert {k: got[k] for k in _lib.CONV_GEOM_FIELDS} == geometry(c), c["name"]
        check_values(c, b, got, shares)
        if FAMILY[got["family"]] == "pw":
            no_pw(True)
            alt = launch(engine, c, b)
            no_pw(False)
            assert FAMILY[alt["family"]] == "h2" and alt["pro"] == 0 and alt["BN"] == got["BN"], c["name"]
            for name in ("out", "out2"):
                if got[name] is not None:
                    assert np.array_equal(got[name].view(np.uint32), alt[name].view(np.uint32)), \
                        "%s: conv_pw_h2_kernel and conv_gemm_h2_kernel<BN, false> differ in %s" % (c["name"], name)
    check_shares(shares, 0.02)
    print("GPU, worst error / bar: %s" % {k: round(v, 4) for k, v in sorted(WORST.items())})


def settings_of(kind, split, pro):
    """One sequence in four settings: alone, as row 2 of a ragged batch with a larger Tmax, cut in two streamed launches, and with
    padded strides."""
    h1 = kind in (2, 3, 5)
    unit, outc = kind in (1, 3), kind >= 4
    C, N = (96, 96) if unit else ((32, 4) if outc else (40, 72))
    K, dil = (7, 9) if unit else ((7, 1) if outc else (7, 3))
    ppf, F = 8, 22                                            # 176 positions: two position tiles of the convs
    halo = (K - 1) * dil
    hist = -(-halo // ppf) * ppf
    kw = dict(tag="e", snake=unit or outc or pro, bias=True, bias2=unit, out2=not outc, out=not outc, split=split, gain=1.6 if outc else 1.0)
    if kind in (0, 2):
        kw.update(res=True)
    if kind == 0:
        kw.update(scale=True, act=1)
    name = "eq-%d-%d-%d-" % (kind, split, pro)
    alone = case(name + "alone", kind, C, N, K, dil, rows=[(0, 0, F)], ppf=ppf, **kw)
    ragged = case(name + "ragged", kind, C, N, K, dil, rows=[(1, 0, 30), (2, 0, 0), (0, 0, F)], ppf=ppf, **kw)
    cut1 = case(name + "cut1", kind, C, N, K, dil, rows=[(0, 0, 9)], ppf=ppf, **kw)
    cut2 = case(name + "cut2", kind, C, N, K, dil, rows=[(0, 9 * ppf, F - 9)], ppf=ppf, hist=hist, margin=hist + 8, **kw)
    L = [alone, ragged, cut1, cut2]
    if not unit and not outc:
        L.append(case(name + "padded", kind, C, N, K, dil, rows=[(0, 0, F)], ppf=ppf, ldx=C + 8, ldo=N + 12, ldr=N + 4, **kw))
    return L


EQ = [(0, 0, 0), (0, 1, 0), (0, 1, 1), (0, 0, 1), (1, 0, 0), (2, 0, 0), (3, 0, 0), (4, 0, 0), (5, 0, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,split,pro", EQ, ids=["f32", "h2", "h2pro", "f32pro", "unit", "h1", "unit_h1", "out", "out_h1"])
def test_same_sequence_same_bits_in_every_setting(engine, kind, split, pro):
    """Alone, as a row of a ragged batch, cut in two streamed launches (the second finds the first's last rows in its hist margin)
    and with padded ldx / ldo / ldr: the same bits for every valid element, and every launch inside the bars."""
    cs = settings_of(kind, split, pro)
    res = {}
    for c in cs:
        b = build(c)
        got = launch(engine, c, b)
        check_values(c, b, got, [])
        res[c["name"].split("-")[-1]] = (c, got)
    names = ["pcm"] if kind >= 4 else ["out", "out2"]
    for name in names:
        ref = valid(*res["alone"], name)[0]
        assert np.array_equal(valid(*res["ragged"], name)[2], ref), "%s differs as a row of a ragged batch" % name
        cut = np.concatenate([valid(*res["cut1"], name)[0], valid(*res["cut2"], name)[0]])
        assert np.array_equal(cut, ref), "%s differs when the sequence is cut in two streamed launches" % name
        if "padded" in res:
            assert np.array_equal(valid(*res["padded"], name)[0], ref), "%s differs with padded strides" % name


@pytest.mark.gpu
@pytest.mark.parametrize("kind,split,K", [(0, 0, 7), (0, 1, 7), (0, 1, 1), (2, 0, 7), (2, 0, 2), (2, 0, 1)],
                         ids=["f32", "h2", "pw", "h1-k7", "h1-k2", "h1-k1"])
def test_tile_width_and_aliasing_do_not_change_bits(engine, kind, split, K):
    """The same weights as N = 128, 96 and 64 rows (BN 128, 96, 64): the shared channels agree bit for bit. res aliased with out
    against res in a buffer of its own, and out2 alone against out2 beside out, likewise."""
    got = {}
    for N in (128, 96, 64):
        c = case("tw-%d-%d-%d-n%d" % (kind, split, K, N), kind, 40, N, K, 3 if K == 7 else 1, T=150, split=split, tag="w", bias=True, out2=True,
                 post_C=32)
        b = build(c)
        got[N] = (c, launch(engine, c, b))
        assert got[N][1]["BN"] == N
        check_values(c, b, got[N][1], [])
    for name in ("out", "out2"):
        a128 = valid(*got[128], name)[0]
        assert np.array_equal(valid(*got[96], name)[0], a128[:, :96]) and np.array_equal(valid(*got[64], name)[0], a128[:, :64]), \
            "%s depends on the tile width" % name
    kw = dict(split=split, tag="w", bias=True, res=True, out2=True)
    apart = case("al-%d-%d-%d-apart" % (kind, split, K), kind, 40, 72, K, 1, T=150, **kw)
    alias = case("al-%d-%d-%d-alias" % (kind, split, K), kind, 40, 72, K, 1, T=150, res_is_out=True, **kw)
    only2 = case("al-%d-%d-%d-only2" % (kind, split, K), kind, 40, 72, K, 1, T=150, out=False, **kw)
    r = {}
    for c in (apart, alias, only2):
        b = build(c)
        r[c["name"].split("-")[-1]] = (c, launch(engine, c, b))
        check_values(c, b, r[c["name"].split("-")[-1]][1], [])
    assert np.array_equal(valid(*r["alias"], "out")[0], valid(*r["apart"], "out")[0]), "res aliased with out changes out"
    assert np.array_equal(valid(*r["alias"], "out2")[0], valid(*r["apart"], "out2")[0]), "res aliased with out changes out2"
    assert np.array_equal(valid(*r["only2"], "out2")[0], valid(*r["apart"], "out2")[0]), "out2 alone differs from out2 beside out"


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [1, 3], ids=["unit", "unit_h1"])
def test_fused_unit_against_its_two_convs(engine, kind):
    """A fused unit and its two convs as separate launches (conv1 with the SnakeBeta'd input and act2 as its out2, then the
    pointwise conv2 with the residual): both under the float64 bars -- the fused kernel's k order is another summation order."""
    T, C, dil = 200, 96, 3
    u = case("fu-%d-unit" % kind, kind, C, C, 7, dil, T=T, snake=True, bias=True, bias2=True, out2=True, tag="u")
    b = build(u)
    got = launch(engine, u, b)
    check_values(u, b, got, [])
    r = ref_of(u, b, 0)
    h1 = kind == 3
    if not h1:
        c1 = engine.debug_conv(0, frames=[T], x=b["x"], w=b["W"], K=7, dil=dil, split=1, snake=b["snake"], bias=b["bias"], post=b["act2"], post_C=C,
                               out2=np.zeros((1, u["Tmax"], C), np.float32))
        c2 = engine.debug_conv(0, frames=[T], x=c1["out2"], w=b["W2"][:, None, :], K=1, split=1, bias=b["bias2"], res=b["x"],
                               out=np.zeros((1, u["Tmax"], C), np.float32))
        a = c2["out"][0, :T].astype(np.float64)
    else:
        # (the float16 conv has no prologue: act1 is the producer's out2 in the decoder; here the reference's activated input)
        a1, _ = snake16(r16(b["xs"][0].astype(np.float64)), 0.0, snake_f16_params(b["snake"]))
        xin = np.zeros((1, u["Tmax"], C), np.uint16)
        xin[0, :T] = a1.astype(np.float16).view(np.uint16)
        c1 = engine.debug_conv(2, frames=[T], x=xin, w=b["W"], K=7, dil=dil, bias=b["bias"], post=b["act2"], post_C=C,
                               out2=np.zeros((1, u["Tmax"], C), np.uint16))
        c2 = engine.debug_conv(2, frames=[T], x=c1["out2"], w=b["W2"][:, None, :], K=1, bias=b["bias2"], res=b["x"],
                               out=np.zeros((1, u["Tmax"], C), np.uint16))
        a = c2["out"][0, :T].view(np.float16).astype(np.float64)
    err = np.abs(a - r["out"])
    assert (err <= r["d_out"]).all(), "the two launches leave the unit's bars by %.3g" % (err - r["d_out"]).max()


@pytest.mark.gpu
def test_refused_arguments_launch_nothing(engine):
    """With a live model: a refused call (status 3) leaves out untouched, and a good call afterwards works."""
    from qwen3tts import Qwen3TTSError
    c = GROUPS["f32"][6]
    b = build(c)
    bad = dict(c, dil=60)
    with pytest.raises(Qwen3TTSError) as e:
        launch(engine, bad, b)
    assert e.value.status == 3
    h3 = case("bad-h1-k3", 2, 40, 64, 3, 1, T=50)
    with pytest.raises(Qwen3TTSError) as e:
        launch(engine, h3, build(h3))
    assert e.value.status == 3
    check_values(c, b, launch(engine, c, b), [])
