// 3x3 convolutions on the bf16 matrix pipe (VLG_PRECISION=bf16 of the pixel step): the implicit GEMMs of conv.hip - forward,
// data gradient and weight gradient over the same padded-NHWC tensors, halo, masks, guard rows, row tables and
// [cout_p][9][cin_p] weights - with v_mfma_f32_32x32x16_bf16 (8x the fp32 MFMA's rate per instruction) instead of
// v_mfma_f32_32x32x2_f32.
//
// Numerical contract: every tensor stays fp32 in memory.  Only the two GEMM operands are rounded to bf16 (round to nearest
// even, plain casts: v_cvt_pk_bf16_f32, NaN stays NaN) on their way into LDS; the PReLU applied on load (act_f, act_ch) is
// computed in fp32 before that rounding; the products accumulate in fp32 and every epilogue (bias, residual, PReLU, row mask,
// PReLU' with the slope-gradient partials, accumulate, the bias gradient's column sums of dOut) works on fp32 values exactly
// as in conv.hip.  The result is not bit-identical to the fp32 path (the reference's precision); see DESIGN.md.
//
// Operand images (gemm_tile16.h), BK = 32 contraction steps per tile (cin_p, cout_p are multiples of 32: a K tile never
// straddles a tap):
//   forward          A = input rows shifted by the tap (KC)          B = weights [cout][9 cin_p] (KC)
//   data gradient    A = dOut rows shifted by -tap / per-tap tables   B = weights, contraction-major [cout][tap cin_p + ci] (MC)
//   weight gradient  A = dOut [pixel][cout] (MC)                     B = act(input) [pixel + shift(tap)][ci] (MC)
// Staging: 8 fp32 values (two 16-byte loads) per slot into registers one K tile ahead, converted on the LDS write; LDS double
// buffered, one barrier per K tile.  Validation, plan (tile, split-K on the coarse 256-512 channel levels) and the finish
// kernels of split-K are conv.hip's, shared with the fp32 path; this file holds the kernel and its launcher.
#include "conv_common.h"
#include "gemm_tile16.h"

namespace {

constexpr int BK16 = 32;

// act(v) per channel of 8 consecutive channels c .. c+7 (channels >= act_ch stay linear)
__device__ __forceinline__ void act8(float4& lo, float4& hi, float a, int c, int act_ch) {
    lo = act4(lo, slope4(a, c, act_ch));
    hi = act4(hi, slope4(a, c + 4, act_ch));
}

template <int MODE, int BM, int BN, int WM>
__global__ __launch_bounds__(GEMM_THREADS, 2) void conv_bf16_kernel(const ConvArgs g) {
    constexpr int BK = BK16;
    constexpr bool A_KC = MODE != CONV_WGRAD;
    constexpr bool B_KC = MODE == CONV_FWD;
    constexpr int WN = 4 / WM;
    constexpr int TM = BM / (32 * WM), TN = BN / (32 * WN);
    static_assert(TM >= 1 && TN >= 1 && TM * 32 * WM == BM && TN * 32 * WN == BN, "tile / wave layout");
    using TA = Tile16<BM, A_KC, BK>;
    using TB = Tile16<BN, B_KC, BK>;
    constexpr int ELEMS = 2 * (TA::ELEMS + TB::ELEMS);
    // (weight gradient: the bias gradient's per-slot column sums reuse the tiles after the main loop)
    static_assert(MODE != CONV_WGRAD || TA::SLOTS * 8 * 4 <= ELEMS * 2, "column-sum scratch");
    __shared__ __attribute__((aligned(16))) bf16_t smem[ELEMS];
    __shared__ float red[GEMM_THREADS / 64];
    bf16_t* const As0 = smem;
    bf16_t* const Bs0 = smem + 2 * TA::ELEMS;

    const int ntile = g.tiles_m * g.tiles_n;
    const int split = blockIdx.x / ntile, tile = blockIdx.x - split * ntile;
    const int tm = tile / g.tiles_n, tn = tile - tm * g.tiles_n;
    const int64_t m0 = (int64_t)tm * BM;
    const int n0 = tn * BN;
    const int64_t kbeg = (int64_t)split * g.kc_per_split;
    const int64_t kend = kbeg + g.kc_per_split < g.Kc ? kbeg + g.kc_per_split : g.Kc;
    const int nk = (int)((kend - kbeg + BK - 1) / BK);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int wm = wave / WN, wn = wave - wm * WN;
    const bool act = g.prelu != nullptr;
    const float slope = act ? g.prelu[0] : 1.0f;

    // ---- per-thread constants of the gathers (slot i of this thread: idx = tid + 256 i; KC: row idx / 4, k 8 (idx % 4);
    // MC: k idx / (BR / 8), row 8 (idx % (BR / 8))).  Slots past a tile's SLOTS are never written to LDS; their
    // addresses are clamped into the operand.
    const float* pa[TA::NV];
    const float* pb[TB::NV];
    int arow[TA::NV], acol[TA::NV];                            // forward / data gradient: row of A, k offset of the slot
    int amaj[TA::NV], bmaj[TB::NV];                            // weight gradient: the k row (pixel) of each slot
    int bch[TB::NV];                                           // weight gradient: first channel of each B slot
#pragma unroll
    for (int i = 0; i < TA::NV; ++i) {
        int idx = tid + GEMM_THREADS * i;
        if (idx >= TA::SLOTS) idx = 0;
        if constexpr (MODE != CONV_WGRAD) {
            int64_t r = m0 + idx / TA::PER_ROW;
            r = r < g.M ? r : g.M - 1;                         // rows past M are computed but never stored
            arow[i] = (int)r;
            acol[i] = (idx % TA::PER_ROW) << 3;
            if (g.rowtab != nullptr && g.tab_stride == 0) r = g.rowtab[r];
            pa[i] = g.A + r * g.lda + acol[i];
        } else {
            amaj[i] = idx / TA::PER_ROW;
            pa[i] = g.A + m0 + ((idx % TA::PER_ROW) << 3);
        }
    }
#pragma unroll
    for (int i = 0; i < TB::NV; ++i) {
        int idx = tid + GEMM_THREADS * i;
        if (idx >= TB::SLOTS) idx = 0;
        if constexpr (MODE == CONV_FWD) {
            int row = n0 + idx / TB::PER_ROW;
            row = row < g.N ? row : g.N - 1;                   // output channels past cout are computed but never stored
            pb[i] = g.B + (int64_t)row * g.ldb + ((idx % TB::PER_ROW) << 3);
        } else if constexpr (MODE == CONV_DGRAD) {
            pb[i] = g.B + (int64_t)(idx / TB::PER_ROW) * g.ldb + n0 + ((idx % TB::PER_ROW) << 3);
        } else {
            int col = n0 + ((idx % TB::PER_ROW) << 3);
            if (col > g.N - 8) col = g.N - 8;                  // columns past N are computed but never stored
            const int tap = col / g.cin;
            bch[i] = col - tap * g.cin;
            bmaj[i] = idx / TB::PER_ROW;
            pb[i] = g.B + (int64_t)g.shift[tap] * g.ldb + bch[i];
        }
    }
    (void)arow; (void)acol; (void)amaj; (void)bmaj; (void)bch;

    Stage16<float, TA::NV> sa;
    Stage16<float, TB::NV> sb;
    float csum[TA::NV][8];                                     // weight gradient: column sums of the staged dOut (bias gradient)
#pragma unroll
    for (int i = 0; i < TA::NV; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) csum[i][j] = 0.f;
    int g_tap = (int)(kbeg / g.cin), g_ci = (int)(kbeg - (int64_t)g_tap * g.cin);   // (tap, channel block) of the next load
    int ach = 0;                                               // forward: channel block of the staged A tile

    auto gload = [&](int64_t k0) {
        if constexpr (MODE != CONV_WGRAD) {
            const int tap = g_tap, ci0 = g_ci;
            g_ci += BK;
            if (g_ci >= g.cin) { g_ci = 0; ++g_tap; }
            ach = ci0;
#pragma unroll
            for (int i = 0; i < TA::NV; ++i) {
                const float* src;
                if (g.tab_stride != 0) {                       // per-tap row tables (data gradient of a stride-2 conv)
                    const int64_t r = g.rowtab[(int64_t)tap * g.tab_stride + arow[i]];
                    src = g.A + r * g.lda + ci0 + acol[i];
                } else {
                    src = pa[i] + (int64_t)g.shift[tap] * g.lda + ci0;
                }
                sa.lo[i] = ld4(src);
                sa.hi[i] = ld4(src + 4);
            }
            const int64_t boff = MODE == CONV_FWD ? k0 : (int64_t)ci0 * g.ldb + (int64_t)tap * g.b_tap_stride;
#pragma unroll
            for (int i = 0; i < TB::NV; ++i) {
                sb.lo[i] = ld4(pb[i] + boff);
                sb.hi[i] = ld4(pb[i] + boff + 4);
            }
        } else {
            // contraction = pixels: rows past the split's end (kend) are zeros
#pragma unroll
            for (int i = 0; i < TA::NV; ++i) {
                const int64_t p = k0 + amaj[i];
                const bool ok = p < kend;
                const float* src = pa[i] + (ok ? p : kend - 1) * g.lda;
                const float4 lo = ld4(src), hi = ld4(src + 4);
                sa.lo[i] = ok ? lo : f4_zero();
                sa.hi[i] = ok ? hi : f4_zero();
            }
#pragma unroll
            for (int i = 0; i < TB::NV; ++i) {
                const int64_t p = k0 + bmaj[i];
                const bool ok = p < kend;
                int64_t r = ok ? p : kend - 1;
                if (g.rowtab != nullptr) r = g.rowtab[r];
                const float* src = pb[i] + r * g.ldb;
                const float4 lo = ld4(src), hi = ld4(src + 4);
                sb.lo[i] = ok ? lo : f4_zero();
                sb.hi[i] = ok ? hi : f4_zero();
            }
        }
    };
    // fp32 work on the staged values (the activation on load, the bias gradient's sums), then bf16 into LDS
    auto sstore = [&](int buf) {
        if constexpr (MODE == CONV_FWD) {
            if (act) {
#pragma unroll
                for (int i = 0; i < TA::NV; ++i) {
                    const int idx = tid + GEMM_THREADS * i;
                    act8(sa.lo[i], sa.hi[i], slope, ach + ((idx % TA::PER_ROW) << 3), g.act_ch);
                }
            }
        } else if constexpr (MODE == CONV_WGRAD) {
#pragma unroll
            for (int i = 0; i < TA::NV; ++i) {
                csum[i][0] += sa.lo[i].x; csum[i][1] += sa.lo[i].y; csum[i][2] += sa.lo[i].z; csum[i][3] += sa.lo[i].w;
                csum[i][4] += sa.hi[i].x; csum[i][5] += sa.hi[i].y; csum[i][6] += sa.hi[i].z; csum[i][7] += sa.hi[i].w;
            }
            if (act) {
#pragma unroll
                for (int i = 0; i < TB::NV; ++i) act8(sb.lo[i], sb.hi[i], slope, bch[i], g.act_ch);
            }
        }
        TA::sstore(sa, As0 + buf * TA::ELEMS, tid);
        TB::sstore(sb, Bs0 + buf * TB::ELEMS, tid);
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    if (nk > 0) {
        gload(kbeg);
        sstore(0);
    }
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        const bool more = kt + 1 < nk;
        if (more) gload(kbeg + (int64_t)(kt + 1) * BK);       // in flight behind this tile's MFMAs
        const bf16_t* as = As0 + cur * TA::ELEMS;
        const bf16_t* bs = Bs0 + cur * TB::ELEMS;
#pragma unroll
        for (int s = 0; s < BK / 16; ++s) {
            bf16x8 fa[TM], fb[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) fa[i] = TA::frag(as, (wm * TM + i) * 32, s, lane);
#pragma unroll
            for (int j = 0; j < TN; ++j) fb[j] = TB::frag(bs, (wn * TN + j) * 32, s, lane);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        // (the other buffer was last read before the previous iteration's barrier)
        if (more) sstore(cur ^ 1);
        __syncthreads();
    }

    // ---- epilogue (C/D layout: col = lane&31, row = (r&3) + 8*(r>>2) + 4*h); a split-K launch stores raw partial tiles
    // (the host passes no bias / residual / mask / epilogue flags then)
    float* const Cs = g.C + (int64_t)split * g.slab_stride;
    const int64_t row0 = m0 + wm * TM * 32 + 4 * h;
    const int col0 = n0 + wn * TN * 32 + l31;
    float da = 0.f;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int col = col0 + j * 32;
            if (col >= g.N) continue;
            const float bv = (MODE == CONV_FWD && g.bias != nullptr) ? g.bias[col] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t row = row0 + i * 32 + (r & 3) + 8 * (r >> 2);
                if (row >= g.M) continue;
                const int64_t o = row * g.ldc + col;
                float v = acc[i][j][r] + bv;
                if constexpr (MODE != CONV_WGRAD) {
                    if (g.epi & VLG_CEPI_RESID) v += g.aux_in[o];
                    if (g.epi & VLG_CEPI_PRELU) v = prelu_f(v, slope);
                    if (g.rowmask != nullptr) v *= g.rowmask[row];
                    // data gradient: appended AddCoords channels are constants - no gradient flows through them
                    if (MODE == CONV_DGRAD && col >= g.act_ch) v = 0.f;
                    if (g.epi & VLG_CEPI_DPRELU) {
                        const float x = g.aux_in[o];
                        if (col < g.act_ch) {
                            da += x > 0.f ? 0.f : v * x;
                            v *= x > 0.f ? 1.0f : slope;
                        }
                    }
                    if (g.epi & VLG_CEPI_ACCUM) v += Cs[o];
                }
                Cs[o] = v;
            }
        }
    if constexpr (MODE == CONV_WGRAD) {
        // bias gradient: slot (k row, 8 columns) sums -> LDS, then one thread per column adds its BK rows in a fixed order
        if (tn == 0) {
            float* const part = reinterpret_cast<float*>(smem);
#pragma unroll
            for (int i = 0; i < TA::NV; ++i) {
                const int idx = tid + GEMM_THREADS * i;
                if (idx < TA::SLOTS) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) part[idx * 8 + j] = csum[i][j];
                }
            }
            __syncthreads();
            if (tid < BM && m0 + tid < g.M) {
                float s = 0.f;
                for (int kr = 0; kr < BK; ++kr) s += part[(kr * TA::PER_ROW + (tid >> 3)) * 8 + (tid & 7)];
                Cs[g.colsum_off + m0 + tid] = s;
            }
        }
    }
    if constexpr (MODE == CONV_DGRAD) {
        if (g.da_slab != nullptr) {                            // slope gradient: one partial per block
            da = block_sum(da, red);
            if (tid == 0) g.da_slab[blockIdx.x] = da;
        }
    }
}

template <int MODE, int BM, int BN, int WM>
int launch_bf16(ConvArgs g, hipStream_t s) {
    g.tiles_m = (int)((g.M + BM - 1) / BM);
    g.tiles_n = (g.N + BN - 1) / BN;
    const int64_t blocks = (int64_t)g.tiles_m * g.tiles_n * g.splits;
    if (blocks < 1 || blocks > 0x7fffffff) return VLG_ERR_SHAPE;
    hipLaunchKernelGGL((conv_bf16_kernel<MODE, BM, BN, WM>), dim3((unsigned)blocks), dim3(GEMM_THREADS), 0, s, g);
    return vlg_last_error();
}
template <int MODE>
int launch_bf16_tile(int bm, int bn, const ConvArgs& g, hipStream_t s) {
    if (bn == 32) return launch_bf16<MODE, 128, 32, 4>(g, s);
    if (bn == 64) return bm == 64 ? launch_bf16<MODE, 64, 64, 2>(g, s) : launch_bf16<MODE, 128, 64, 2>(g, s);
    if (bn == 96) return launch_bf16<MODE, 128, 96, 4>(g, s);
    return bm == 64 ? launch_bf16<MODE, 64, 128, 2>(g, s) : launch_bf16<MODE, 128, 128, 2>(g, s);
}

}  // namespace

// the bf16 kernel of a tile that conv.hip's plan chose (the weight gradient: BM rows of cout_p, BN = 128)
int conv_bf16_launch(int mode, int bm, int bn, const ConvArgs& g, hipStream_t s) {
    if (mode == CONV_FWD) return launch_bf16_tile<CONV_FWD>(bm, bn, g, s);
    if (mode == CONV_DGRAD) return launch_bf16_tile<CONV_DGRAD>(bm, bn, g, s);
    switch (bm) {
        case 128: return launch_bf16<CONV_WGRAD, 128, 128, 1>(g, s);
        case 96: return launch_bf16<CONV_WGRAD, 96, 128, 1>(g, s);
        case 64: return launch_bf16<CONV_WGRAD, 64, 128, 1>(g, s);
        default: return launch_bf16<CONV_WGRAD, 32, 128, 1>(g, s);
    }
}
