// bf16-MFMA GEMMs of the bf16 mode (BASELINE.json configs[2]): v_mfma_f32_32x32x16_bf16, fp32 accumulate.
//
// Same three products as gemm.hip (forward A.W^T, data gradient dY.W, weight gradient dY^T.X split over tokens),
// same 128x128 block tile / 2x2 wave tiles / XCD-aware tile order / slab outputs, but the operand tiles live in LDS
// as bf16, 64 contraction steps deep, whatever the HBM element type (bf16 activations are copied, fp32 operands -
// weights, residual-stream gradients - are rounded once on their way to LDS):
//   KC image  [row][k]   rows of 64 bf16 + 8 pad = 36 dwords: the per-lane 16-byte fragment reads (ds_read_b128,
//                        lane = row, half-wave h picks k = 16s + 8h ..+7) hit 16 distinct 4-bank slots per 16 lanes
//   MC image  [k][row]   the operand is contraction-major in memory (W for the data gradient, dY and X for the weight
//                        gradient), so the tile is stored exactly as it arrives and read with gfx950's TRANSPOSING
//                        LDS read ds_read_b64_tr_b16: each 16-lane group fetches a 4(k) x 16(row) block and every
//                        lane receives the 4 k-values of ITS row - two reads make the 8-deep MFMA operand.  Row
//                        stride = BR*2 + 64 bytes, so the four k-rows of a block start 64 B apart modulo the 256-B
//                        bank window: conflict-free.
// Both images give lane (row = l & 31, h = l >> 5) the k-values 16s + 8h + j, j = 0..7, so A and B agree on the
// contraction order whatever their layouts.
// Algorithmic work per launch: 2*M*N*K flop; bytes = element sizes x (M*K + N*K + M*N) (+ aux operands): with
// bf16 activations the 128 x 128 x 64 tile needs 16 MFMAs (512 cycles) per 32 KB staged - the kernel is priced
// against HBM, not MFMA.
#include "common.h"
#include <type_traits>
#include "gemm_tile16.h"
#include "reduce_body.h"
#include <stdlib.h>

// LDS elements (bf16) of one block: both operand tiles, double-buffered
template <int BM, int BN, int BK16, bool A_KC, bool B_KC>
constexpr int gemm16_smem_elems() { return 2 * (Tile16<BM, A_KC, BK16>::ELEMS + Tile16<BN, B_KC, BK16>::ELEMS); }

// the kernel body as a function of (arguments, LDS, block number, block count): one problem per launch (gemm_bf16_kernel) or
// a projection's data gradient and weight gradient side by side (gemm16_pair_kernel), as in gemm.hip
template <int BM, int BN, int BK16, bool A_KC, bool B_KC, int EPI, bool COLSUM, typename EA, typename EB, typename EO>
__device__ __forceinline__ void gemm16_body(const GemmArgs& g, bf16_t* const smem, const int bid, const int nwg) {
    constexpr int DEPTH = BK16 == 64 ? 2 : 1;          // register-resident tiles in flight besides the two LDS buffers
    // (a 32-deep, DEPTH 1, 4-blocks-per-CU instantiation was measured: +4 % on forward / data gradient, -30 % on the
    // weight gradient whose column-sum registers then spill - not kept)
    constexpr int NS = BK16 / 16;                      // 16-deep MFMA steps per tile
    static_assert(!COLSUM || !A_KC, "column sums are taken from a contraction-major A tile");
    const EA* const gA = static_cast<const EA*>(g.A);
    const EB* const gB = static_cast<const EB*>(g.B);
    using W = Waves16<BM, BN>;
    constexpr int WN = W::WN, TM = W::TM, TN = W::TN;
    using TA = Tile16<BM, A_KC, BK16>;
    using TB = Tile16<BN, B_KC, BK16>;
    bf16_t* const As0 = smem;
    bf16_t* const Bs0 = smem + 2 * TA::ELEMS;

    const Place16 pl = gemm16_place<BM, BN>(g, bid, nwg);
    const int tn = pl.tn, n0 = pl.n0;
    const int64_t m0 = pl.m0, kbeg = pl.kbeg, kend = pl.kend;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int wm = wave / WN, wn = wave - wm * WN;

    f32x16 acc[TM][TN];
    float bv[TN];
    gemm16_start<EPI>(acc, bv, g, n0 + wn * TN * 32 + l31);
    float csum[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) csum[j] = 0.f;

    const int nk = (int)((kend - kbeg + BK16 - 1) / BK16);
    auto kstep = [&](const bf16_t* as, const bf16_t* bs, int s) {
        bf16x8 a[TM], b[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) a[i] = TA::frag(as, (wm * TM + i) * 32, s, lane);
#pragma unroll
        for (int j = 0; j < TN; ++j) b[j] = TB::frag(bs, (wn * TN + j) * 32, s, lane);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    };
    auto mainloop = [&](auto guard_tag) {
        constexpr bool GUARD = decltype(guard_tag)::value;
        Stage16<EA, TA::NV> sa0, sa1;
        Stage16<EB, TB::NV> sb0, sb1;
        auto load = [&](Stage16<EA, TA::NV>& xa, Stage16<EB, TB::NV>& xb, int t) {
            const int64_t k0 = kbeg + (int64_t)t * BK16;
            TA::template gload<GUARD>(xa, gA, g.lda, m0, g.M, k0, kend, tid);
            TB::template gload<GUARD>(xb, gB, g.ldb, n0, g.N, k0, kend, tid);
        };
        // one iteration: the MFMAs of the tile in LDS buffer kt&1; in the middle, tile kt+1 (in registers) goes to the other
        // buffer and its registers are refilled with tile kt+3 - two tiles are in flight between HBM and LDS at any time
        auto iter = [&](int kt, Stage16<EA, TA::NV>& xa, Stage16<EB, TB::NV>& xb) {
            const int cur = kt & 1;
            const bf16_t* as = As0 + cur * TA::ELEMS;
            const bf16_t* bs = Bs0 + cur * TB::ELEMS;
#pragma unroll
            for (int ks = 0; ks < NS / 2; ++ks) kstep(as, bs, ks);
            if (kt + 1 < nk) {
                if constexpr (COLSUM) { if (tn == 0) TA::colsum_add(csum, xa); }
                TA::sstore(xa, As0 + (cur ^ 1) * TA::ELEMS, tid);
                TB::sstore(xb, Bs0 + (cur ^ 1) * TB::ELEMS, tid);
            }
            if (kt + 1 + DEPTH < nk) load(xa, xb, kt + 1 + DEPTH);
#pragma unroll
            for (int ks = NS / 2; ks < NS; ++ks) kstep(as, bs, ks);
            __syncthreads();
        };
        if (nk > 0) {
            load(sa0, sb0, 0);
            if constexpr (COLSUM) { if (tn == 0) TA::colsum_add(csum, sa0); }
            TA::sstore(sa0, As0, tid);
            TB::sstore(sb0, Bs0, tid);
        }
        if (nk > 1) load(sa0, sb0, 1);
        if constexpr (DEPTH == 2) {
            if (nk > 2) load(sa1, sb1, 2);
        }
        __syncthreads();
        if constexpr (DEPTH == 2) {
            for (int kt = 0; kt < nk; kt += 2) {        // tile kt+1 sits in (sa0, sb0) on even, in (sa1, sb1) on odd iterations
                iter(kt, sa0, sb0);
                if (kt + 1 < nk) iter(kt + 1, sa1, sb1);
            }
        } else {
            for (int kt = 0; kt < nk; ++kt) iter(kt, sa0, sb0);
        }
    };
    if (pl.full && ((kend - kbeg) % BK16) == 0) mainloop(std::false_type{});
    else mainloop(std::true_type{});

    // ---- epilogue (gemm_tile16.h)
    const int64_t row0 = m0 + wm * TM * 32 + 4 * h;      // the lane's first element of C
    const int col0 = n0 + wn * TN * 32 + l31;
    EO* Cs = static_cast<EO*>(g.C) + (int64_t)pl.split * g.slab_stride;
    // (An LDS-staged epilogue for bf16 outputs - column pairs packed with a DPP swap, 16-byte row-contiguous stores - was
    // measured and is NOT faster than these 2-byte stores: the kernels are not bound by store requests.)
    if (pl.full) gemm16_emit<false, EPI>(g, acc, bv, Cs, row0, col0);
    else gemm16_emit<true, EPI>(g, acc, bv, Cs, row0, col0);
    if constexpr (COLSUM) {
        if (tn == 0) gemm16_colsum_store<TA, BM>(g, csum, reinterpret_cast<float*>(smem), Cs, m0, tid);
    }
}

// IO bit 0: A is bf16, bit 1: B is bf16, bit 2: C and the epilogue's auxiliary operands are bf16 (else float)
template <int BM, int BN, bool A_KC, bool B_KC, int EPI, bool COLSUM, int IO>
__global__ __launch_bounds__(GEMM_THREADS, 2) void gemm_bf16_kernel(const GemmArgs g) {
    using EA = std::conditional_t<(IO & 1) != 0, bf16_t, float>;
    using EB = std::conditional_t<(IO & 2) != 0, bf16_t, float>;
    using EO = std::conditional_t<(IO & 4) != 0, bf16_t, float>;
    __shared__ __attribute__((aligned(16))) bf16_t smem[gemm16_smem_elems<BM, BN, 64, A_KC, B_KC>()];
    gemm16_body<BM, BN, 64, A_KC, B_KC, EPI, COLSUM, EA, EB, EO>(g, smem, (int)blockIdx.x, (int)gridDim.x);
}

// A projection's data gradient (blocks [0, nd_pad): nd real, padded to a multiple of 8 for the XCD mapping of the second
// problem) and weight gradient (the rest) in ONE launch - csrc/gemm.hip, gemm_pair_kernel.  The bf16-storage step's
// combinations: dY bf16 or fp32 (A16), W / X bf16, dX (+ the multiply epilogue's operand) bf16.
// (blocks past both problems: rider rows of a slab-reduction table, as in gemm_pair_kernel)
template <int EPI_D, bool A16>
__global__ __launch_bounds__(GEMM_THREADS, 2) void gemm16_pair_kernel(const GemmArgs gd, const GemmArgs gw, const int nd, const int nd_pad,
                                                                     const int nw, const int64_t* __restrict__ rider, const int rider_bpr) {
    using EA = std::conditional_t<A16, bf16_t, float>;
    constexpr int FD = gemm16_smem_elems<128, 128, 64, true, false>(), FW = gemm16_smem_elems<128, 128, 64, false, false>();
    __shared__ __attribute__((aligned(16))) bf16_t smem[FD > FW ? FD : FW];
    const int b = (int)blockIdx.x;
    if (b < nd_pad) {
        if (b < nd) gemm16_body<128, 128, 64, true, false, EPI_D, false, EA, bf16_t, bf16_t>(gd, smem, b, nd);
    } else if (b < nd_pad + nw) {
        gemm16_body<128, 128, 64, false, false, VLG_EPI_NONE, true, EA, bf16_t, float>(gw, smem, b - nd_pad, nw);
    } else {
        const int rb = b - nd_pad - nw;
        reduce_table_row(rider, rb / rider_bpr, rb % rider_bpr, rider_bpr, reinterpret_cast<float4(*)[16]>(smem));
    }
}
// ---- host side: the instantiated kernels, one row each (gemm_tile.h); gemm_plan (gemm.hip) takes a call's kernel from here
// and gemm.hip launches it.  Everything fp32 in HBM (io 0, the "bf16_mfma" mode) and the combinations the bf16-storage
// step launches (bf16 activations AND bf16 shadow weights); the pair: W / X / dX bf16, the shared dY bf16 or fp32 (a
// residual-stream gradient).
GemmPairKernel vlg_gemm16_pair_kernel(int epi_d, bool dy_bf16) {
    if (epi_d == VLG_EPI_NONE) return dy_bf16 ? gemm16_pair_kernel<VLG_EPI_NONE, true> : gemm16_pair_kernel<VLG_EPI_NONE, false>;
    if (epi_d == VLG_EPI_MUL) return dy_bf16 ? gemm16_pair_kernel<VLG_EPI_MUL, true> : gemm16_pair_kernel<VLG_EPI_MUL, false>;
    return nullptr;
}
template <int CALL, int EPI, int IO, int BM, int BN>
constexpr GemmKernelRow bf16_row() {
    return {CALL, EPI, IO, BM, BN, 64, gemm_bf16_kernel<BM, BN, CALL != VLG_CALL_WGRAD, CALL == VLG_CALL_FWD, EPI, CALL == VLG_CALL_WGRAD, IO>};
}
#define EPI_GELU_GRAD (VLG_EPI_BIAS | VLG_EPI_GELU | VLG_EPI_GELU_GRAD)
static const GemmKernelRow gemm_bf16_kernels[] = {
    bf16_row<VLG_CALL_FWD, VLG_EPI_BIAS, 0, 128, 32>(), bf16_row<VLG_CALL_FWD, VLG_EPI_BIAS, 0, 128, 128>(),
    bf16_row<VLG_CALL_FWD, VLG_EPI_BIAS, 3, 128, 32>(), bf16_row<VLG_CALL_FWD, VLG_EPI_BIAS, 3, 128, 128>(),
    bf16_row<VLG_CALL_FWD, VLG_EPI_BIAS, 7, 128, 32>(), bf16_row<VLG_CALL_FWD, VLG_EPI_BIAS, 7, 128, 128>(),
    bf16_row<VLG_CALL_FWD, VLG_EPI_BIAS | VLG_EPI_GELU, 0, 128, 128>(), bf16_row<VLG_CALL_FWD, VLG_EPI_BIAS | VLG_EPI_GELU, 7, 128, 128>(),
    bf16_row<VLG_CALL_FWD, EPI_GELU_GRAD, 0, 128, 128>(), bf16_row<VLG_CALL_FWD, EPI_GELU_GRAD, 7, 128, 128>(),
    bf16_row<VLG_CALL_FWD, VLG_EPI_BIAS | VLG_EPI_RESID, 0, 128, 128>(), bf16_row<VLG_CALL_FWD, VLG_EPI_BIAS | VLG_EPI_RESID, 3, 128, 128>(),
    bf16_row<VLG_CALL_DGRAD, VLG_EPI_NONE, 0, 128, 128>(), bf16_row<VLG_CALL_DGRAD, VLG_EPI_NONE, 6, 128, 128>(),
    bf16_row<VLG_CALL_DGRAD, VLG_EPI_NONE, 7, 128, 128>(),
    bf16_row<VLG_CALL_DGRAD, VLG_EPI_DGELU, 0, 128, 128>(), bf16_row<VLG_CALL_DGRAD, VLG_EPI_DGELU, 6, 128, 128>(),
    bf16_row<VLG_CALL_DGRAD, VLG_EPI_MUL, 0, 128, 128>(), bf16_row<VLG_CALL_DGRAD, VLG_EPI_MUL, 6, 128, 128>(),
    bf16_row<VLG_CALL_WGRAD, VLG_EPI_NONE, 0, 32, 128>(), bf16_row<VLG_CALL_WGRAD, VLG_EPI_NONE, 0, 128, 128>(),
    bf16_row<VLG_CALL_WGRAD, VLG_EPI_NONE, 2, 32, 128>(), bf16_row<VLG_CALL_WGRAD, VLG_EPI_NONE, 2, 128, 128>(),
    bf16_row<VLG_CALL_WGRAD, VLG_EPI_NONE, 3, 32, 128>(), bf16_row<VLG_CALL_WGRAD, VLG_EPI_NONE, 3, 128, 128>(),
};
GemmKernel vlg_gemm16_kernel(const GemmProblem& p) {
    return gemm_find_kernel(gemm_bf16_kernels, sizeof(gemm_bf16_kernels) / sizeof(gemm_bf16_kernels[0]), p);
}
