// gemm_body.inc -- device-side body of the skinny decode GEMM (see gemm_decode.hip for the design notes). Included inside
// namespace q3 { namespace { ... } } by gemm_decode.hip.
// Diagnostic build only (make TIMELINE=1 defines Q3TTS_GEMM_TIMELINE; the shipped library holds none of this): clock stamps
// (100 MHz wall clock, the same on every CU) of each wave of the first and the last workgroup of the talker's 32-row gate/up,
// down_proj and qkv launches, kept in registers and written by lane 0 with plain stores behind the last output store into a buffer
// nothing else reads. tools/gemm_timeline.py prints the last launch's table. Stamps: 0 wave start, 1 prologue done (rstd known),
// 2 first MFMAs issued (first weight fragments and their x landed), 3 last MFMA issued (last weight fragment landed),
// 4 every wave's partials of the last tile in LDS, 5 last tile reduced, 6 last store issued, 7 first tile reduced.
#ifdef Q3TTS_GEMM_TIMELINE
__device__ unsigned long long g_gemm_tl[4][2][8][8];  // [gate/up chunk-major | gate/up tile-major | down_proj | qkv][first | last workgroup][wave][stamp]
#define Q3_TL_BEGIN()                                                                                                       \
    constexpr int kTlForm = (EPI == 2 && MB == 2 && NW == 8 && CH == 2 && NP == 3 && NTW) ? (TM ? 1 : 0)                    \
                            : ((EPI == 3 && MB == 1 && NW == 8 && CH == 6 && !NORM && NTW) ? 2                              \
                               : ((EPI == 0 && MB == 2 && NW == 8 && CH == 2 && NORM && NP == 1 && NTW) ? 3 : -1));         \
    unsigned long long tl_[8] = {0, 0, 0, 0, 0, 0, 0, 0};                                                                   \
    Q3_TL(0)
#define Q3_TL(k)                                   \
    do {                                           \
        if constexpr (kTlForm >= 0) {              \
            __builtin_amdgcn_sched_barrier(0);     \
            tl_[k] = wall_clock64();               \
            __builtin_amdgcn_sched_barrier(0);     \
        }                                          \
    } while (0)
#define Q3_TL_END()                                                                                                         \
    do {                                                                                                                    \
        if constexpr (kTlForm >= 0) {                                                                                       \
            const bool tl_last = blockIdx.x == gridDim.x - 1 && blockIdx.y == gridDim.y - 1;                                \
            if ((tl_last || (blockIdx.x == 0 && blockIdx.y == 0)) && lane == 0) {                                           \
                _Pragma("unroll") for (int k = 0; k < 8; ++k) g_gemm_tl[kTlForm][tl_last ? 1 : 0][wave][k] = tl_[k];        \
            }                                                                                                               \
        }                                                                                                                   \
    } while (0)
#else
#define Q3_TL_BEGIN() ((void)0)
#define Q3_TL(k) ((void)0)
#define Q3_TL_END() ((void)0)
#endif

__device__ __forceinline__ f32x4 mfma16(const uint4& a, const uint4& b, f32x4 c) {
    bf16x8 av, bv;
    __builtin_memcpy(&av, &a, 16);
    __builtin_memcpy(&bv, &b, 16);
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv, c, 0, 0, 0);
}

__device__ __forceinline__ float silu_f(float v) { return v / (1.0f + __expf(-v)); }

// bf16( bf16(h * rstd) * w ) on 8 packed elements
__device__ __forceinline__ uint4 norm8(const uint4& hx, const uint4& wx, float rstd) {
    const uint32_t hw[4] = {hx.x, hx.y, hx.z, hx.w}, ww[4] = {wx.x, wx.y, wx.z, wx.w};
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float n0 = rbf(lo_bf(hw[j]) * rstd), n1 = rbf(hi_bf(hw[j]) * rstd);
        o[j] = pack_bf(n0 * lo_bf(ww[j]), n1 * hi_bf(ww[j]));
    }
    return make_uint4(o[0], o[1], o[2], o[3]);
}

// MLX affine int4, group 64 (QuantizedLinear installed by quantize(model:...) at Qwen3.swift:1412-1425):
// w = bf16(q * scale + bias). One dwordx4 per lane holds the 32 nibbles of its four A fragments of a chunk
// (8 consecutive k per uint32, little-endian nibbles), so an int4 weight tile is 1 KiB instead of 4 KiB.
__device__ __forceinline__ void dequant_chunk(const uint4& qw, uint32_t sb, uint4 (&out)[4]) {
    const float sc = lo_bf(sb), bi = hi_bf(sb);
    const uint32_t w[4] = {qw.x, qw.y, qw.z, qw.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint32_t o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float q0 = (float)((w[i] >> (8 * j)) & 15u), q1 = (float)((w[i] >> (8 * j + 4)) & 15u);
            // mul and add rounded separately like the oracle (no fma contraction)
            o[j] = pack_bf(__fadd_rn(__fmul_rn(q0, sc), bi), __fadd_rn(__fmul_rn(q1, sc), bi));
        }
        out[i] = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

// EPI: 0 = bf16 store (+bias, +optional silu), row-major or fragment-major
//      2 = gate/up tiles (rows 0..7 gate, rows 8..15 up of the same eight columns, model.cc) -> bf16(bf16(silu(g)) * u),
//          eight columns per tile, fragment-major
//      3 = hidden-state store, fragment-major, in place: h = bf16((resid ? h : 0) + bf16(acc + bias)),
//          plus ss_out[tile][m] = sum over the tile's 16 features of h^2
// NORM: RMSNorm prologue on x (x is then the raw residual stream h)
// NP: weight tiles per workgroup. Decode (EPI 2): a 6144-wide MLP is 768 gate/up tiles, three per workgroup is exactly
// one round of 256 workgroups. Prefill chunks (four row blocks per workgroup, any EPI): every workgroup reads all K of
// its 64 rows of x, so at one tile each the x operand is 0.1-0.8 GB of L2 traffic per launch (3072 workgroups x 256 KB for
// gate/up); four tiles per workgroup quarter it. Per-output arithmetic does not depend on NP.
// NTW: weight tiles are loaded non-temporally (common.h ld16).
// TM: tile-major order for a workgroup of several gate/up tiles (EPI 2, NORM, every chunk's x prefetched). A wave that
// requests everything up front (64 wave-wide loads at NP 3) stands at the issue of its loads until the memory system has
// taken the last one -- 7.8 of the 12.5 us a wave of the 1.7B talker's gate/up launch lives (profiles/talker_gemm_timeline.txt)
// -- and only then starts the prologue's VALU work (rstd, then normalising x: 1.3 us, 2.7 us for the second wave of a SIMD),
// with every MFMA and all NP epilogues behind that. Here only tile 0's weights are requested with the sums of squares and
// x; the prologue and the normalisation of x (once, into the registers it arrived in) run while those are in flight, the
// other tiles' weights are requested behind them, tile by tile (loads return in issue order), and each tile's MFMAs are
// followed at once by its reduction and store, so tile t's epilogue runs while tiles t + 1.. are still arriving. Every tile
// has LDS buffers of its own, so no barrier guards their reuse. Per output the arithmetic is the same: wave w's chunks in
// order, four MFMAs per chunk, wave partials added in wave order.
template <int MB, int EPI, int NW, int CH, bool NORM, bool QUANT, int NP = 1, bool NTW = false, bool TM = false>
__device__ __forceinline__ void gemm_skinny_body(const GemmArgs& a, const int tile, const int mb0) {
    constexpr int NT = NP;                   // weight tiles per workgroup
    constexpr int NR = 1;                    // tiles reduced per pass of the epilogue
    constexpr int NB = TM ? NT : 1;          // LDS reduction buffers
    constexpr int kDefer = TM ? NT - 1 : 0;  // tiles whose weights are requested behind the prologue
    static_assert(!TM || (EPI == 2 && NORM && !QUANT && CH > 0 && NP > 1), "tile-major order is a gate/up form");
    // EPI 2: a.N counts output columns, eight per tile; the last workgroup of a ragged width re-reads the last tile for its
    // missing ones and does not store them
    const int n_tiles = (EPI == 2) ? (a.N >> 3) : (a.N >> 4);
    __shared__ float red[NB][NW][NR][MB][4][64];
    __shared__ __attribute__((aligned(16))) uint16_t ys[NB][MB][16][16];
    __shared__ float rstd_s[NORM ? 16 * MB : 1];
    __shared__ float ssp_s[NORM ? 8 : 1][NORM ? 16 * MB : 1];

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    Q3_TL_BEGIN();
    // mb0: first 16-row block of this workgroup (launch_q splits the rows of narrow layers)
    const int KC = a.K >> 7;  // 128-wide k chunks

    f32x4 acc[NT][MB];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) acc[t][mb] = f32x4{0.f, 0.f, 0.f, 0.f};

    const uint4* Wt = reinterpret_cast<const uint4*>(a.W);
    const uint4* Xt = reinterpret_cast<const uint4*>(a.x);

    // 0. NORM: the producer's per-tile sums of squares are requested before anything else. They gate the whole prologue
    //    (rstd -> normalised x fragments), and loads return in issue order: with the sums first, the reduction and the
    //    VALU work on x run while the weight tiles are still arriving instead of after the last of them.
    constexpr int kSsIter = NORM ? (16 * MB * 8 + NW * 64 - 1) / (NW * 64) : 1;
    float sst[kSsIter][16];
    if constexpr (NORM) {
        // EVERY thread loads (threads past rows * 8 wrap onto valid slots and never use the values): a load guarded by
        // the same condition as its later use was compiled into `load; s_waitcnt vmcnt(0); add` -- a whole memory round
        // trip in front of the weight requests -- and one branch per load. Unconditional loads stay a straight line.
        const int rows = 16 * MB;
#pragma unroll
        for (int it = 0; it < kSsIter; ++it) {
            const int idx = (threadIdx.x + it * NW * 64) % (rows * 8);
            const int row = idx % rows, part = idx / rows;  // (row, part): 8 strided partial sums per row
            const float* sp = a.ss_in + 16 * mb0 + row;
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int j = part + 8 * u;
                sst[it][u] = sp[(size_t)(j < a.ss_count ? j : 0) * a.ss_ld];
            }
        }
        // keep these requests in front of the weight requests (loads return in issue order; hipcc otherwise sinks
        // them behind the sixteen-byte loads and the whole prologue then waits for the last weight tile)
        __builtin_amdgcn_sched_barrier(0);
    }

    // 1. weight loads: they depend on nothing
    constexpr int CHR = CH > 0 ? CH : 1;
    constexpr int WL = QUANT ? 1 : 4;  // dwordx4 loads per (chunk, tile): packed int4 needs one
    uint4 wf[CHR][NT][WL];
    uint32_t wsb[CHR][NT];
    auto load_w = [&](int c, int kc, int t0, int t1) {  // chunk c of tiles t0 .. t1 - 1
#pragma unroll
        for (int t = t0; t < t1; ++t) {
            const int tt = tile * NT + t;
            const size_t blk = (size_t)(tt < n_tiles ? tt : n_tiles - 1) * KC + kc;
            if constexpr (QUANT) {
                wf[c][t][0] = ld16<NTW>(Wt + blk * 64 + lane);
                wsb[c][t] = a.Wsb[blk * 64 + lane];
            } else {
                const uint4* wp = Wt + blk * 256 + lane;
#pragma unroll
                for (int i = 0; i < 4; ++i) wf[c][t][i] = ld16<NTW>(wp + i * 64);
            }
        }
    };

    // 1b. every other operand that does not depend on arithmetic is requested now as well, so that the kernel pays
    //     ONE memory round trip instead of a chain of three (sums of squares -> x fragments -> residual tile):
    //     the raw x fragments of the first XG chunks, and (EPI 3) the old hidden-state piece this thread will update.
    // chunks whose x fragments are prefetched: as many as fit next to the weight registers (16 VGPRs per fragment set)
    constexpr int kWRegs = CH * NT * (QUANT ? 5 : 16);
    // (one row block leaves room for every chunk of the widest layer, K = 6144: one round trip for the whole workgroup)
    constexpr int kRoom = (((MB == 1 && !NORM) ? 200 : 176) - kWRegs) / (MB * 16);
    constexpr int kCap = (MB == 1 && !NORM) ? 6 : 3;
    constexpr int XG0 = (CH == 0) ? 0 : (kRoom < 1 ? 1 : (kRoom > kCap ? (CH < kCap ? CH : kCap) : (kRoom < CH ? kRoom : CH)));
    // The K = 2048 norm-prologue projections (the 1.7B talker's qkv and head: two row blocks, two chunks per wave) take x one
    // chunk at a time: 128 instead of 180 VGPRs, i.e. two workgroups fit a CU. Alone that costs nothing (3.408 -> 3.403 ms per
    // frame step); beside a codec decode, which leaves the frame loop half of the CUs, the launch's 256 workgroups then run
    // together instead of in two rounds (steady pipelined step 795.0 -> 791.4 ms).
    constexpr int XG = (MB == 2 && NORM && CH == 2 && NT == 1 && EPI == 0) ? 1 : XG0;
    static_assert(!TM || XG == CH, "tile-major order keeps every chunk's x fragments in registers");
    uint4 xr[XG > 0 ? XG : 1][MB][4];
    uint4 nwr[(NORM && XG > 0) ? XG : 1][4];
    // issue order: weights then x, or (NORM) x then weights so that normalising x overlaps the weights' arrival.
    // Written as a two-trip unrolled loop instead of lambdas: capturing the fragment arrays by reference sends them to scratch.
#pragma unroll
    for (int ph = 0; ph < 2; ++ph) {
        if (ph == 1) __builtin_amdgcn_sched_barrier(0);  // issue order between the two groups as written
        if ((ph == 0) != NORM) {
    if constexpr (TM) {
#pragma unroll
            for (int t = 0; t < NT - kDefer; ++t)
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    const int kl = wave + c * NW;
                    load_w(c, kl < KC ? kl : 0, t, t + 1);
                }
    } else if constexpr (CH > 0) {
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const int kl = wave + c * NW;
                load_w(c, kl < KC ? kl : 0, 0, NT);
            }
        }
        } else {
    if constexpr (XG > 0) {
#pragma unroll
        for (int c = 0; c < XG; ++c) {
            const int kl = wave + c * NW;
            const int kc = kl < KC ? kl : 0;
            if constexpr (NORM) {
                const uint4* np = reinterpret_cast<const uint4*>(a.norm_w + kc * 128 + 32 * (lane >> 4));
#pragma unroll
                for (int i = 0; i < 4; ++i) nwr[c][i] = np[i];
            }
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) {
                const uint4* xp = Xt + ((size_t)(kc * a.xMB + mb0 + mb) * 4) * 64 + lane;
#pragma unroll
                for (int i = 0; i < 4; ++i) xr[c][mb][i] = xp[i * 64];
            }
        }
    }
        }
    }
    __builtin_amdgcn_sched_barrier(0);  // every request above is issued before any arithmetic below
    uint4 hv_pre = make_uint4(0, 0, 0, 0);
    if constexpr (EPI == 3 && NT == 1) {
        if (a.resid && threadIdx.x < 32 * MB) {
            const int o = threadIdx.x, mb = o >> 5, b = (o >> 1) & 15, p = o & 1;
            hv_pre = *reinterpret_cast<const uint4*>(a.y + act_tiled_offset(16 * (mb0 + mb) + b, tile * 16 + 8 * p, a.yMB));
        }
    }

    // 2. NORM: rstd per row from the producer's per-tile sums of squares, summed in tile order
    float rstd[MB];
    if constexpr (NORM) {
        const int rows = 16 * MB;
#pragma unroll
        for (int it = 0; it < kSsIter; ++it) {
            const int idx = threadIdx.x + it * NW * 64;
            if (idx < rows * 8) {
                const int row = idx % rows, part = idx / rows;
                float s = 0.f;
#pragma unroll
                for (int u = 0; u < 16; ++u)
                    if (part + 8 * u < a.ss_count) s += sst[it][u];
                for (int j = part + 128; j < a.ss_count; j += 8) s += a.ss_in[(size_t)j * a.ss_ld + 16 * mb0 + row];
                ssp_s[part][row] = s;
            }
        }
        __syncthreads();
        if (threadIdx.x < rows) {
            float s = 0.f;
#pragma unroll
            for (int p = 0; p < 8; ++p) s += ssp_s[p][threadIdx.x];
            rstd_s[threadIdx.x] = 1.0f / sqrtf(s / (float)a.norm_dim + a.norm_eps);
        }
        __syncthreads();
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) rstd[mb] = rstd_s[16 * mb + (lane & 15)];
    }
    Q3_TL(1);
    if constexpr (TM) {  // x normalised once, in place: every tile multiplies with the same fragments
#pragma unroll
        for (int c = 0; c < CH; ++c) {
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                for (int i = 0; i < 4; ++i) xr[c][mb][i] = norm8(xr[c][mb][i], nwr[c][i], rstd[mb]);
        }
        // only now the other tiles' weights (the barriers keep hipcc from hoisting the requests in front of the VALU work)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = NT - kDefer; t < NT; ++t)
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const int kl = wave + c * NW;
                load_w(c, kl < KC ? kl : 0, t, t + 1);
            }
        __builtin_amdgcn_sched_barrier(0);
    }

    // 3. x fragments (+ norm) and MFMAs
    auto chunk = [&](int kc, int c, const uint4 (*xpre)[4], const uint4* nwpre) {
        uint4 w[NT][4];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if constexpr (QUANT) {
                dequant_chunk(wf[c][t][0], wsb[c][t], w[t]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) w[t][i] = wf[c][t][i];
            }
        }
        uint4 nw[4];
        if constexpr (NORM) {
            if (nwpre) {
#pragma unroll
                for (int i = 0; i < 4; ++i) nw[i] = nwpre[i];
            } else {
                const uint4* np = reinterpret_cast<const uint4*>(a.norm_w + kc * 128 + 32 * (lane >> 4));
#pragma unroll
                for (int i = 0; i < 4; ++i) nw[i] = np[i];
            }
        }
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
            uint4 xf[4];
            if (xpre) {
#pragma unroll
                for (int i = 0; i < 4; ++i) xf[i] = xpre[mb][i];
            } else {
                const uint4* xp = Xt + ((size_t)(kc * a.xMB + mb0 + mb) * 4) * 64 + lane;
#pragma unroll
                for (int i = 0; i < 4; ++i) xf[i] = xp[i * 64];
            }
            if constexpr (NORM) {
#pragma unroll
                for (int i = 0; i < 4; ++i) xf[i] = norm8(xf[i], nw[i], rstd[mb]);
            }
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[t][mb] = mfma16(w[t][i], xf[i], acc[t][mb]);
        }
    };
    if constexpr (TM) {
        // the MFMAs stand in front of each tile's epilogue below
    } else if constexpr (CH > 0) {
        // chunks in groups of XG: the first group's fragments are already in flight; each later group is requested as a
        // whole (one round trip per group) into the same registers
#pragma unroll
        for (int g0 = 0; g0 < CH; g0 += XG) {
            if (g0 > 0) {
#pragma unroll
                for (int c = 0; c < XG; ++c) {
                    if (g0 + c < CH) {
                        const int kl = wave + (g0 + c) * NW;
                        const int kc = kl < KC ? kl : 0;
                        if constexpr (NORM) {
                            const uint4* np = reinterpret_cast<const uint4*>(a.norm_w + kc * 128 + 32 * (lane >> 4));
#pragma unroll
                            for (int i = 0; i < 4; ++i) nwr[c][i] = np[i];
                        }
#pragma unroll
                        for (int mb = 0; mb < MB; ++mb) {
                            const uint4* xp = Xt + ((size_t)(kc * a.xMB + mb0 + mb) * 4) * 64 + lane;
#pragma unroll
                            for (int i = 0; i < 4; ++i) xr[c][mb][i] = xp[i * 64];
                        }
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < XG; ++c) {
                if (g0 + c < CH) {
                    const int kl = wave + (g0 + c) * NW;
                    if (kl < KC) chunk(kl, g0 + c, xr[c], NORM ? nwr[c] : nullptr);  // wave-uniform
                }
                if (g0 + c == 0) Q3_TL(2);
            }
        }
    } else {
        for (int kl = wave; kl < KC; kl += NW) {
            load_w(0, kl, 0, NT);
            chunk(kl, 0, nullptr, nullptr);
        }
    }

    if constexpr (!TM) Q3_TL(3);
    // 4. cross-wave K reduction through LDS, fixed wave order; one tile (EPI 2: one gate/up pair) per pass
#pragma unroll
    for (int pr = 0; pr < NT / NR; ++pr) {
    const int rb = TM ? pr : 0;  // this pass's LDS buffers
    if constexpr (TM) {
        // tile pr's fragments are complete before those of the tiles behind it: its MFMAs, chunks in the wave's order
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            if (wave + c * NW < KC) {  // wave-uniform
#pragma unroll
                for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[pr][mb] = mfma16(wf[c][pr][i], xr[c][mb][i], acc[pr][mb]);
            }
        }
        if (pr == 0) Q3_TL(2);
        if (pr == NT - 1) Q3_TL(3);
    } else {
        if (pr > 0) __syncthreads();  // the previous pair's red / ys reads
    }
#pragma unroll
    for (int t = 0; t < NR; ++t)
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int q = 0; q < 4; ++q) red[rb][wave][t][mb][q][lane] = acc[pr * NR + t][mb][q];
    __syncthreads();
    if (pr == NT / NR - 1) Q3_TL(4);
    const int otile = tile * (NT / NR) + pr;  // 16-column output tile

    if constexpr (EPI == 2) {
        // 128*MB outputs per tile: thread -> (mb, batch row b, column f); gate = tile row f, up = tile row f + 8
        for (int o = threadIdx.x; o < 128 * MB; o += NW * 64) {
            const int mb = o >> 7, rem = o & 127;
            const int b = rem >> 3, f = rem & 7;
            const int lg = (f >> 2) * 16 + b, lu = (2 + (f >> 2)) * 16 + b, q = f & 3;
            float g = 0.f, u = 0.f;
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                g += red[rb][w][0][mb][q][lg];
                u += red[rb][w][0][mb][q][lu];
            }
            ys[rb][mb][b][f] = f2bf(rbf(silu_f(rbf(g))) * rbf(u));
        }
    } else {
    // 256*MB outputs per tile: thread -> (mb, batch row b, feature f)
    for (int o = threadIdx.x; o < 256 * MB; o += NW * 64) {
        const int mb = o >> 8, rem = o & 255;
        const int b = rem >> 4, f = rem & 15;
        const int src_lane = (f >> 2) * 16 + b, q = f & 3;
        float sum = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) sum += red[rb][w][0][mb][q][src_lane];
        const int n = otile * 16 + f;
        float y = sum;
        if (a.bias && otile < n_tiles) y += bf2f(a.bias[n]);
        uint16_t yb = f2bf(y);
        if (EPI == 0 && a.act_silu) yb = f2bf(silu_f(bf2f(yb)));
        ys[rb][mb][b][f] = yb;
    }
    }
    __syncthreads();
    if (pr == 0) Q3_TL(7);
    if (pr == NT / NR - 1) Q3_TL(5);
    if constexpr (EPI == 2) {  // one 16-byte store per (mb, row b): the tile's eight columns
        for (int o = threadIdx.x; o < 16 * MB; o += NW * 64) {
            const int mb = o >> 4, b = o & 15;
            const int m = 16 * (mb0 + mb) + b;
            if (m < a.M && otile < n_tiles)
                *reinterpret_cast<uint4*>(a.y + act_tiled_offset(m, otile * 8, a.yMB)) = *reinterpret_cast<const uint4*>(&ys[rb][mb][b][0]);
        }
    } else
    // 16-byte stores: thread -> (mb, row b, 8-feature piece p)
    for (int o = threadIdx.x; o < 32 * MB; o += NW * 64) {
        const int mb = o >> 5, b = (o >> 1) & 15, p = o & 1;
        const int m = 16 * (mb0 + mb) + b;
        uint4 v = *reinterpret_cast<const uint4*>(&ys[rb][mb][b][8 * p]);
        const int n = otile * 16 + 8 * p;
        if constexpr (EPI == 3) {
            uint16_t* hp = a.y + act_tiled_offset(m, n, a.yMB);
            float ss = 0.f;
            const uint32_t yw[4] = {v.x, v.y, v.z, v.w};
            uint32_t ow[4];
            uint4 hv = hv_pre;  // o == threadIdx.x here (32 * MB <= 128 threads, one trip)
            if constexpr (NT > 1) {
                if (a.resid && m < a.M && otile < n_tiles) hv = *reinterpret_cast<const uint4*>(hp);
            }
            const uint32_t hw[4] = {hv.x, hv.y, hv.z, hv.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float h0 = lo_bf(yw[j]), h1 = hi_bf(yw[j]);
                if (a.resid) {
                    h0 = rbf(lo_bf(hw[j]) + h0);
                    h1 = rbf(hi_bf(hw[j]) + h1);
                }
                ss += h0 * h0;
                ss += h1 * h1;
                ow[j] = pack_bf(h0, h1);
            }
            const float other = __shfl_xor(ss, 1, 64);  // the tile's second 8-feature piece of this row
            if (m < a.M && otile < n_tiles) {
                *reinterpret_cast<uint4*>(hp) = make_uint4(ow[0], ow[1], ow[2], ow[3]);
                if (p == 0 && a.ss_out) a.ss_out[(size_t)otile * a.ss_ld + m] = ss + other;
            }
        } else {
            if (m >= a.M || otile >= n_tiles) continue;
            if (a.y_tiled)
                *reinterpret_cast<uint4*>(a.y + act_tiled_offset(m, n, a.yMB)) = v;
            else
                *reinterpret_cast<uint4*>(a.y + (size_t)m * a.ldy + n) = v;
        }
    }
    }
    Q3_TL(6);
    Q3_TL_END();
}
