// fp32 MFMA GEMMs for the dense QKV / FFN / head projections.
//
// One kernel template serves forward (A.W^T), data-gradient (dY.W) and weight-gradient
// (dY^T.X, split over the token dimension) by choosing how each operand tile sits in LDS:
//   *_KC  tile[row][k]  - operand rows are contraction-contiguous in memory; row stride 36
//                         floats, so the per-lane float4 fragment reads (ds_read_b128) are
//                         bank-conflict-free (36*i mod 64 hits 16 distinct 4-bank slots)
//   *_MC  tile[k][row]  - operand is contraction-major in memory (W for dgrad, dY and X for
//                         wgrad); fragments are 4 ds_read_b32, lanes 0..31 on consecutive banks
// MFMA: v_mfma_f32_32x32x2_f32 (exact fp32, 64 cycles/SIMD, 157 TFLOP/s chip peak).  Its two
// k-slices per instruction go to lane halves h = lane>>5; we assign k = 8*s + 4*h + j to
// MFMA j of chunk s so ONE float4 read feeds four MFMAs (A and B use the same assignment,
// the contraction order inside a chunk is free).
// Block = 256 threads = 4 waves; 128x128 tile => each wave owns 64x64 = 2x2 MFMA tiles
// (64 accumulator VGPRs).  Staging is global -> VGPR -> LDS, double-buffered in LDS and one tile
// deep in registers: tile kt+1 is loaded from global one iteration ahead, written to the idle LDS
// buffer BETWEEN the MFMAs of one chunk of tile kt (one ds_write_b128 / load behind each MFMA, pinned
// with sched_group_barrier); fragment reads are double-buffered in registers (chunk s+1's LDS reads
// are issued before chunk s's 16 MFMAs); the iteration's one barrier sits in FRONT of the last
// chunk's MFMAs and the next tile's first fragments are read behind it, under those MFMAs.
// BK (contraction depth per tile) is a template parameter: 32 -> 73.7 KB LDS, 2 blocks / CU;
// 16 -> 41 KB, 3 blocks / CU.  blockIdx is remapped so tiles sharing an A panel sit on one XCD (L2).
//
// THE ONE PIPE.  On gfx950 this MFMA and the vector ALU of a SIMD execute serially, oldest wave first
// (tools/micro/mfma_f32_valu_share.hip): every vector instruction of ANY wave on the SIMD costs 8 cycles
// of matrix time (12 for a transcendental, packed or not), memory and LDS instructions cost none, and
// s_setprio changes nothing.  So the kernel has two paths:
//   fast     (128x128 tiles whose block lies inside both operands; mainloop_fast / emit_fast): no vector
//            instruction in the steady-state iteration - buffer loads with the K advance in the scalar
//            offset, two iterations unrolled so LDS addresses are immediates, zero tiles instead of
//            peeled tails; the bias in the accumulator start; buffer stores; GELU on packed
//            instructions in lockstep over 8 row pairs; optionally a RUN of N tiles per block, the K loop
//            continuing into the next tile.  151 TFLOP/s at K = 4096 (96 %), 115-143 per shape of the step.
//   general  (edge tiles, 32-wide tiles of the head, the GELU-on-load variants; mainloop / emit): 64-bit
//            pointers, clamps and selects - ~26 vector instructions per iteration, 141 TFLOP/s at best.
// Algorithmic work per launch: 2*M*N*K flop; bytes 4*(M*K + N*K + M*N) (+ aux operands).
#include "common.h"
#include <type_traits>

#include "gemm_tile.h"
#include "reduce_body.h"

// keeps the hand-placed order "next chunk's LDS reads, then this chunk's MFMAs" (see ldfrag below); VLG_NO_SCHED_FENCE
// builds the loop without it (A/B switch for tools/kernel_bench.py)
// internal template bits on top of the public VLG_EPI_* ones: the operand named passes through GELU on its way to LDS
// (VLG_EPI_ACT_GELU: the FFN hidden activation is never stored - the second projection and its weight gradient
// recompute it from the pre-activation while they stage it, in the shadow of their own MFMAs)
#define GEMM_A_GELU (1 << 20)
#define GEMM_B_GELU (1 << 21)
__device__ __forceinline__ float4 gelu4(float4 v) { return make_float4(gelu_f(v.x), gelu_f(v.y), gelu_f(v.z), gelu_f(v.w)); }

// raw buffer descriptor over [p, p + 2 GB): base in the descriptor, offsets in a VGPR (per thread) and an SGPR (per wave)
// (loads beyond `bytes` return zeros, stores beyond it are dropped)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t vlg_rsrc(const void* p, int bytes = 0x7fffffff) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, 0x00020000);
}

// Epilogue pacing (compile-time option, OFF: measured neutral, tools/ab/gemm_ab.py).  The CU's vector-memory pipeline is one
// FIFO for all its waves and takes ~5 cycles per 128-B line (tools/micro/mfma_f32_valu_share.hip mem), so a 64 KB epilogue
// burst holds it for 1-2 us; sleeping between small groups of the epilogue's memory instructions (-DVLG_EPI_PACE=1) keeps the
// FIFO short for the co-resident block's tile loads - but that block's waves are not waiting on the FIFO: what they wait
// for is the vector ALU (oldest wave first), so nothing is gained.
#ifndef VLG_EPI_PACE
#define VLG_EPI_PACE 0          /* s_sleep argument (x 64 cycles) behind every VLG_EPI_PACE_EVERY memory instructions; 0 = off */
#endif
#ifndef VLG_EPI_PACE_EVERY
#define VLG_EPI_PACE_EVERY 2
#endif
__device__ __forceinline__ void vlg_epi_pace(int issued) {
#if VLG_EPI_PACE > 0
    if (issued % VLG_EPI_PACE_EVERY == 0) __builtin_amdgcn_s_sleep(VLG_EPI_PACE);
#endif
}

#ifdef VLG_NO_SCHED_FENCE
#define VLG_SCHED_FENCE()
#else
#define VLG_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
#endif

// LDS floats of one block: both operand tiles, double-buffered
template <int BM, int BN, int BK, bool A_KC, bool B_KC>
constexpr int gemm_smem_floats() { return 2 * (Tile<BM, A_KC, BK>::FLOATS + Tile<BN, B_KC, BK>::FLOATS); }

// The kernel body as a device function of (arguments, LDS, block number, block count): gemm_f32_kernel runs one problem per
// launch, gemm_pair_kernel two independent ones (a projection's data gradient and weight gradient) side by side.
template <int BM, int BN, int BK, bool A_KC, bool B_KC, int EPI, bool COLSUM>
__device__ __forceinline__ void gemm_f32_body(const GemmArgs& g, float* const smem, const int bid, const int nwg) {
    // Raised priority until the main loop starts.  It does NOT get this block's vector instructions past an older block's
    // MFMA stream (the vector ALU serves the oldest wave that has a matrix or vector instruction ready, whatever s_setprio
    // says: tools/micro/mfma_f32_valu_share.hip prio / two), but the prologue's loads and LDS writes are issued ahead of the
    // neighbour's: measured 3-5 % per launch.
    __builtin_amdgcn_s_setprio(3);
    using EO = float;
    const float* const gA = static_cast<const float*>(g.A);
    const float* const gB = static_cast<const float*>(g.B);
    const float* const gAuxIn = static_cast<const float*>(g.aux_in);
    float* const gAuxOut = static_cast<float*>(g.aux_out);
    // 128x128: 2 x 2 waves of 64x64; 64x64 (launches whose 128-wide tiles would leave CUs empty: small M): 2 x 2 waves of 32x32
    constexpr int WM = (BM == BN && (BM == 128 || BM == 64)) ? 2 : (BM == 128 ? 4 : 1);
    constexpr int WN = 4 / WM;
    constexpr int TM = BM / (32 * WM), TN = BN / (32 * WN);
    constexpr int NCH = BK / 8;                    // 8-deep MFMA chunks per tile
    using TA = Tile<BM, A_KC, BK>;
    using TB = Tile<BN, B_KC, BK>;
    float* const As0 = smem;                       // As[buf] = As0 + buf * TA::FLOATS
    float* const Bs0 = smem + 2 * TA::FLOATS;      // Bs[buf] = Bs0 + buf * TB::FLOATS

    // XCD-aware remap: hardware deals blocks round-robin over 8 XCDs; give each XCD a
    // contiguous run of logical tiles (bijective for any grid size)
    const int swz = xcd_swizzle(bid, nwg);
    // N tiles per block: the fast path of the BK = 32 kernels without bias-gradient sums (the host sets it); a compile-time 1
    // elsewhere, so those kernels have no loop around [main loop, epilogue]
    constexpr bool CHAIN = BM == 128 && BN == 128 && BK == 32 && !COLSUM && (EPI & ((1 << 20) | (1 << 21))) == 0;
    const int run = (CHAIN && g.run > 1) ? g.run : 1;
    const int tng = g.tiles_n / run;
    const int ntile = g.tiles_m * tng;
    const int split = swz / ntile;
    const int tile = swz - split * ntile;
    const int tm = tile / tng, tn = (tile - tm * tng) * run;
    const int64_t m0 = (int64_t)tm * BM;
    const int n0 = tn * BN;
    const int64_t kbeg = (int64_t)split * g.kc_per_split;
    int64_t kend = kbeg + g.kc_per_split;
    if (kend > g.Kc) kend = g.Kc;

    // (the mask is a no-op at 256 threads, but the range it states, tid < 256, keeps the compiled kernels shorter)
    const int tid = threadIdx.x & (GEMM_THREADS - 1), lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int wm = wave / WN, wn = wave - wm * WN;
#ifdef VLG_TIMELINE
    // diagnostic build only (tools/diag/gemm_timeline.py): 100 MHz stamps at entry / loop start / loop end / exit + placement
    const unsigned long long tl_entry = __builtin_amdgcn_s_memrealtime();
    unsigned long long tl_loop0 = 0, tl_loop1 = 0;
#endif

    f32x16 acc[TM][TN];
    // bias gradient (COLSUM): every thread sums the four dY rows 4*(tid % PER_ROW) .. +3 of the tiles it stages, straight
    // from its staging registers (no LDS reads, no serial chain on two of the four waves); combined through LDS at the end
    // (two packed adds per float4, in every block: a block-uniform branch around them would cut the hand-scheduled
    // iteration into several basic blocks; only the tn == 0 blocks write their sums out)
    v2f col_lo = v2(0.f), col_hi = v2(0.f);
    auto colsum = [&](const float4 (&xa)[TA::NV]) {
#pragma unroll
        for (int i = 0; i < TA::NV; ++i) {
            col_lo += v2f{xa[i].x, xa[i].y};
            col_hi += v2f{xa[i].z, xa[i].w};
        }
    };
    // the accumulators START from the bias (a lane's 16 accumulators of a 32x32 tile share one column): no vector
    // instruction is spent on it in the epilogue, where every one of them costs matrix time (see common.h, gelu2)
    float bv[TN];
    auto load_bias = [&](int n0v) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            bv[j] = 0.f;
            if constexpr ((EPI & VLG_EPI_BIAS) != 0) {
                const int col = n0v + (wn * TN + j) * 32 + l31;
                bv[j] = g.bias[col < g.N ? col : g.N - 1];
            }
        }
    };
    auto init_acc = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = bv[j];
    };
    load_bias(n0);
    init_acc();

#ifndef VLG_TIMELINE
    unsigned long long t0 = 0, r0 = 0;
    if (g.clock_probe) { t0 = __builtin_amdgcn_s_memtime(); r0 = __builtin_amdgcn_s_memrealtime(); }
#endif
    float4 ra[TA::NV], rb[TB::NV];
    const int nk = (int)((kend - kbeg + BK - 1) / BK);
    bool fast_tile = false;
    auto act = [&](float4 (&xa)[TA::NV], float4 (&xb)[TB::NV]) {
        if constexpr ((EPI & GEMM_A_GELU) != 0) {
#pragma unroll
            for (int i = 0; i < TA::NV; ++i) xa[i] = gelu4(xa[i]);
        }
        if constexpr ((EPI & GEMM_B_GELU) != 0) {
#pragma unroll
            for (int i = 0; i < TB::NV; ++i) xb[i] = gelu4(xb[i]);
        }
    };
    // Fragment reads are software-pipelined by hand: the reads of chunk s+1 are issued BEFORE the 16 MFMAs of chunk s, into a
    // second register set, so a wave never waits on LDS between MFMAs.  Left to itself hipcc re-reads two registers at
    // a time with an s_waitcnt lgkmcnt(0) in front of every 2-4 MFMAs: each wave then idles ~30 % of the time and the
    // two waves of a SIMD idle together often enough to cost ~10 % of the matrix pipe.
    auto ldfrag = [&](float (&a)[TM][4], float (&b)[TN][4], const float* as, const float* bs, int s) {
#pragma unroll
        for (int i = 0; i < TM; ++i) TA::frag(a[i], as, (wm * TM + i) * 32 + l31, s, h);
#pragma unroll
        for (int j = 0; j < TN; ++j) TB::frag(b[j], bs, (wn * TN + j) * 32 + l31, s, h);
    };
    auto mma = [&](const float (&a)[TM][4], const float (&b)[TN][4]) {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][kk], b[j][kk], acc[i][j], 0, 0, 0);
    };
    // One iteration: MFMAs of the tile in LDS buffer `cur`; in the middle, the register-resident tile kt+1 goes to the
    // other LDS buffer and the registers are refilled with tile kt+DEPTH (DEPTH tiles travel global -> register at once).
    auto mainloop = [&](auto guard_tag) {
        constexpr bool GUARD = decltype(guard_tag)::value;
        constexpr int DEPTH = 1;                 // tiles travelling global -> register at once
        auto load = [&](float4 (&xa)[TA::NV], float4 (&xb)[TB::NV], int t) {
            const int64_t k0 = kbeg + (int64_t)t * BK;
            TA::template gload<GUARD>(xa, gA, g.lda, m0, g.M, k0, kend, tid);
            TB::template gload<GUARD>(xb, gB, g.ldb, n0, g.N, k0, kend, tid);
        };
        // STORE / LOAD / NEXT are compile-time so the steady-state iteration is ONE basic block: the compiler can then spread
        // the staging instructions (8 ds_write_b128, 8 global_load_dwordx4, address arithmetic) between the MFMAs instead
        // of issuing them as a blob with the matrix pipe idle; the last two iterations are peeled.
        // The iteration's ONE barrier sits in front of the LAST chunk's MFMAs, not behind them: by then every wave has
        // its last fragments of this tile in registers and has finished writing the next tile (staged during chunk SS), so
        // behind the barrier the next tile's first fragments are read while the last chunk's 16 MFMAs run - a wave
        // leaves the barrier with matrix work in hand instead of an LDS round trip.
        constexpr int SS = NCH / 2 - 1;          // chunk whose MFMAs cover the staging traffic
        float fa[2][TM][4], fb[2][TN][4];        // fragment sets: chunk s lives in set s & 1 (NCH is even)
        auto iter = [&](int kt, float4 (&xa)[TA::NV], float4 (&xb)[TB::NV], auto store_tag, auto load_tag, auto next_tag) {
            constexpr bool STORE = decltype(store_tag)::value, LOAD = decltype(load_tag)::value, NEXT = decltype(next_tag)::value;
            const int cur = kt & 1;
            const float* as = As0 + cur * TA::FLOATS;
            const float* bs = Bs0 + cur * TB::FLOATS;
#pragma unroll
            for (int s = 0; s < NCH; ++s) {
                if (s + 1 < NCH) ldfrag(fa[(s + 1) & 1], fb[(s + 1) & 1], as, bs, s + 1);
                if (s == NCH - 1 && NEXT) {
                    __syncthreads();
                    ldfrag(fa[0], fb[0], As0 + (cur ^ 1) * TA::FLOATS, Bs0 + (cur ^ 1) * TB::FLOATS, 0);
                }
                VLG_SCHED_FENCE();                 // reads above, MFMAs below; the staging code may mix with the MFMAs
                if (s == SS) {
                    if constexpr (STORE) {
                        if constexpr (COLSUM) colsum(xa);
                        act(xa, xb);
                        TA::sstore(xa, As0 + (cur ^ 1) * TA::FLOATS, tid);
                        TB::sstore(xb, Bs0 + (cur ^ 1) * TB::FLOATS, tid);
                    }
                    if constexpr (LOAD) load(xa, xb, kt + 1 + DEPTH);
                }
                mma(fa[s & 1], fb[s & 1]);
                if (s == SS && (STORE || LOAD))
                    pin_staging<4 * TM * TN, (STORE ? TA::NV + TB::NV : 0), (LOAD ? TA::NV + TB::NV : 0)>();
            }
        };
        static_assert(NCH >= 2 && NCH % 2 == 0, "fragment sets alternate by chunk parity");
        if (nk > 0) {
            load(ra, rb, 0);
            if constexpr (COLSUM) colsum(ra);
            act(ra, rb);
            TA::sstore(ra, As0, tid);
            TB::sstore(rb, Bs0, tid);
        }
        if (nk > 1) load(ra, rb, 1);
        __syncthreads();
        if (nk > 0) ldfrag(fa[0], fb[0], As0, Bs0, 0);
        __builtin_amdgcn_s_setprio(0);
        int kt = 0;
        for (; kt + 2 < nk; ++kt) iter(kt, ra, rb, std::true_type{}, std::true_type{}, std::true_type{});
        if (kt + 1 < nk) { iter(kt, ra, rb, std::true_type{}, std::false_type{}, std::true_type{}); ++kt; }
        if (kt < nk) iter(kt, ra, rb, std::false_type{}, std::false_type{}, std::false_type{});
        __syncthreads();                           // the tiles are dead from here on (the COLSUM epilogue reuses the LDS)
    };
    // ---- fast path (round 2, second half): NO vector-ALU instruction in the steady-state iteration.
    // v_mfma_f32_32x32x2_f32 and the vector ALU of a SIMD execute serially (tools/micro/mfma_f32_valu_share.hip: every
    // vector instruction of any wave on the SIMD costs 8 cycles of matrix time), and the loop above spent ~26 of them per
    // iteration on addresses (64-bit global pointers, LDS addresses that depend on the buffer parity): 6-8 % of the
    // matrix pipe.  Here the global loads are buffer loads - one loop-constant byte offset per thread and operand, the K
    // advance and the float4 number in the SCALAR offset - and two iterations are unrolled so the LDS buffer is a compile-
    // time constant and every LDS address is one loop-constant register plus an instruction immediate.
    constexpr bool FAST = BM == BN && (BM == 128 || BM == 64) && (EPI & (GEMM_A_GELU | GEMM_B_GELU)) == 0;
    // A block may compute `run` consecutive N tiles of one row panel back to back (multi-round launches): the K loop
    // then simply CONTINUES into the next tile - the loads its last two iterations issue are the next tile's first two K
    // tiles, the LDS write of its last iteration is the next tile's tile 0 and the fragments read behind its last
    // barrier are the next tile's first - so only the epilogue separates the MFMA streams of two tiles.  (A block that
    // starts while an older one streams MFMAs cannot do that: the vector ALU serves the MFMA stream first - s_setprio
    // does not change it, tools/micro/mfma_f32_valu_share.hip prio - so its index arithmetic, and with it its first loads,
    // wait for the neighbour's loop end: per-CU timelines show 1.3-3.4 us of idle matrix pipe per block.)
#ifndef VLG_GEMM_DEPTH
#define VLG_GEMM_DEPTH 1     /* 2 measured: no gain (tools/ab/gemm_ab.py), +16..32 registers */
#endif
    constexpr int DEPTH = VLG_GEMM_DEPTH;
    v4f xas[DEPTH][TA::NV], xbs[DEPTH][TB::NV];      // staging registers and fragment sets live across the tiles of a run
    float ffa[2][TM][4], ffb[2][TN][4];
    // The epilogue's auxiliary operand (residual, multiplier, dGELU argument): a lane's 16 values per 32x32 sub-tile.  The
    // first AUX_EARLY sub-tiles of a tile are requested INSIDE its main loop, by its last two iterations (half each, behind
    // that iteration's staging load), so they travel under the tile's last MFMAs and the epilogue finds them in registers
    // (issued at the epilogue's start they cost one exposed memory round trip per tile, cold from HBM for the FFN's u').
    // Loads retire in order: no staging load that an iteration's LDS write waits for sits behind a request, and a tile's
    // requests are issued inside its own loop only, i.e. behind the previous tile's epilogue.  (Kernels with an auxiliary
    // operand contract over at least one K tile - forward and data gradient are never split - so the requesting pair runs.)
#ifndef VLG_AUX_EARLY
#define VLG_AUX_EARLY 4      /* sub-tiles requested in the main loop (of TM * TN); 0 = all at the epilogue's start */
#endif
    constexpr int AUX_EARLY = (FAST && BK == 32 && (EPI & (VLG_EPI_RESID | VLG_EPI_DGELU | VLG_EPI_MUL)) != 0)
                                  ? (VLG_AUX_EARLY < TM * TN ? VLG_AUX_EARLY : TM * TN) : 0;
    float aux_early[AUX_EARLY > 0 ? AUX_EARLY : 1][16];     // (a tile's values live from its second-last iteration to its epilogue)
    // (per-thread byte offset of its first element in a tile of the operand, which shares C's layout; bytes per row)
    int vc_aux = 0, rowb_aux = 0;
    if constexpr (AUX_EARLY > 0) {
        vc_aux = ((wm * TM * 32 + 4 * h) * g.ldc + wn * TN * 32 + l31) * 4;
        rowb_aux = g.ldc * 4;
    }
    auto mainloop_fast = [&](int n0v, bool first, bool has_next) __attribute__((always_inline)) {
        const float* pa = A_KC ? gA + m0 * g.lda + kbeg : gA + kbeg * g.lda + m0;
        const float* pb = B_KC ? gB + (int64_t)n0v * g.ldb + kbeg : gB + kbeg * g.ldb + n0v;
        // a contraction-major operand's descriptor ends with the K range of this block: loads beyond it return zeros
        const int ext_b = (int)(kend - kbeg);
        const __amdgpu_buffer_rsrc_t da = A_KC ? vlg_rsrc(pa) : vlg_rsrc(pa, ext_b * g.lda * 4);
        const __amdgpu_buffer_rsrc_t db = B_KC ? vlg_rsrc(pb) : vlg_rsrc(pb, ext_b * g.ldb * 4);
        const __amdgpu_buffer_rsrc_t dza = vlg_rsrc(pa, 0), dzb = vlg_rsrc(pb, 0);      // empty: every load returns zeros
        const int va = TA::voff_bytes(g.lda, tid), vb = TB::voff_bytes(g.ldb, tid);
        const int a_is = TA::ISTEP * g.lda * 4, b_is = TB::ISTEP * g.ldb * 4;              // bytes between a thread's float4
        const int a_ks = A_KC ? BK * 4 : BK * g.lda * 4, b_ks = B_KC ? BK * 4 : BK * g.ldb * 4;   // bytes per K tile
        const int b_next = B_KC ? BN * g.ldb * 4 : BN * 4;                                  // bytes to the next N tile of B
        float* const aw = smem + TA::soff(tid);
        float* const bw = smem + 2 * TA::FLOATS + TB::soff(tid);
        // one read base per 32-row group: every fragment offset of a contraction-major tile is then a multiple of 256 B below
        // 64 KB, which ds_read2st64_b32 encodes (two bases short, hipcc re-derives addresses with v_add_u32 inside the loop)
        const float* ar[TM];
        const float* br[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) ar[i] = smem + TA::roff((wm * TM + i) * 32 + l31, h);
#pragma unroll
        for (int j = 0; j < TN; ++j) br[j] = smem + 2 * TA::FLOATS + TB::roff((wn * TN + j) * 32 + l31, h);
        auto load = [&](int t, int set) __attribute__((always_inline)) {
            v4f (&xa)[TA::NV] = xas[set];
            v4f (&xb)[TB::NV] = xbs[set];
            // K tiles past the end: the NEXT tile of the run (same A panel from its start, B one N tile further), or - no next
            // tile - zeros: through the empty descriptor (K-contiguous operand) or past the end of the operand's own
            // descriptor (contraction-major operand); an odd nk runs one iteration on such a zero tile
            const bool in = t < nk, wrap = !in && has_next;
            const int tw = wrap ? t - nk : t;
            const __amdgpu_buffer_rsrc_t ua = (A_KC && !in && !wrap) ? dza : da, ub = (B_KC && !in && !wrap) ? dzb : db;
            const int oa = tw * a_ks, ob = tw * b_ks + (wrap ? b_next : 0);
#pragma unroll
            for (int i = 0; i < TA::NV; ++i) xa[i] = __builtin_amdgcn_raw_buffer_load_b128(ua, va, oa + i * a_is, 0);
#pragma unroll
            for (int i = 0; i < TB::NV; ++i) xb[i] = __builtin_amdgcn_raw_buffer_load_b128(ub, vb, ob + i * b_is, 0);
        };
        auto store = [&](int c, int set) __attribute__((always_inline)) {
            v4f (&xa)[TA::NV] = xas[set];
            v4f (&xb)[TB::NV] = xbs[set];
            if constexpr (COLSUM) {
#pragma unroll
                for (int i = 0; i < TA::NV; ++i) {
                    // (as asm: hipcc merges the two halves into one 4-wide add and then splits THAT into four v_add_f32)
                    const v2f lo = __builtin_shufflevector(xa[i], xa[i], 0, 1), hi = __builtin_shufflevector(xa[i], xa[i], 2, 3);
                    asm("v_pk_add_f32 %0, %0, %1" : "+v"(col_lo) : "v"(lo));
                    asm("v_pk_add_f32 %0, %0, %1" : "+v"(col_hi) : "v"(hi));
                }
            }
#pragma unroll
            for (int i = 0; i < TA::NV; ++i) *reinterpret_cast<v4f*>(aw + c * TA::FLOATS + i * TA::SSTEP) = xa[i];
#pragma unroll
            for (int i = 0; i < TB::NV; ++i) *reinterpret_cast<v4f*>(bw + c * TB::FLOATS + i * TB::SSTEP) = xb[i];
        };
        auto ldf = [&](float (&a)[TM][4], float (&b)[TN][4], int c, int s) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < TM; ++i) TA::frag_at(a[i], ar[i] + c * TA::FLOATS, 0, s);
#pragma unroll
            for (int j = 0; j < TN; ++j) TB::frag_at(b[j], br[j] + c * TB::FLOATS, 0, s);
        };
        constexpr int SS = NCH / 2 - 1;
        // cur is a literal at every call site (the lambda is always inlined), so cur * FLOATS folds into the immediates.
        // There are NO peeled tail iterations: the last two iterations run the same code - their loads fetch the next tile of
        // the run (or zeros), their LDS writes go to the buffer nobody reads any more (or hold the next tile's first K
        // tile) and the fragments read behind the last barrier are dropped (or are the next tile's first).  One copy of the
        // iteration per buffer parity keeps the code small and the register allocation tight (seven inlined tail copies
        // cost 60+ registers and spills).
        auto iter = [&](int kt, int cur) __attribute__((always_inline)) {
#pragma unroll
            for (int s = 0; s < NCH; ++s) {
                if (s + 1 < NCH) ldf(ffa[(s + 1) & 1], ffb[(s + 1) & 1], cur, s + 1);
                if (s == NCH - 1) {
                    __syncthreads();
                    ldf(ffa[0], ffb[0], cur ^ 1, 0);
                }
                VLG_SCHED_FENCE();
                if (s == SS) {                               // tile kt + 1 -> LDS, its registers take tile kt + 1 + DEPTH
                    const int set = DEPTH == 2 ? (cur ^ 1) : 0;
                    store(cur ^ 1, set);
                    load(kt + 1 + DEPTH, set);
                }
                mma(ffa[s & 1], ffb[s & 1]);
                if (s == SS) pin_staging<4 * TM * TN, TA::NV + TB::NV, TA::NV + TB::NV>();
            }
        };
        if (first) {
            load(0, 0);
            store(0, 0);
            // (fenced: hipcc's wait-count pass merges the prologue's load order into the loop's; loads reordered HERE make it
            // wait for the youngest tile inside the loop)
            VLG_SCHED_FENCE();
            if constexpr (DEPTH == 2) { load(1, 1); VLG_SCHED_FENCE(); load(2, 0); }
            else load(1, 0);
            VLG_SCHED_FENCE();
            __syncthreads();
            ldf(ffa[0], ffb[0], 0, 0);
        }
        __builtin_amdgcn_s_setprio(0);
        if constexpr (AUX_EARLY > 0) {
            // The copies of the iteration that also request the tile's auxiliary operand, sub-tiles [T0, T1): in the chunk behind
            // the staging one, the requests spread behind its MFMAs.  Only the last pair of a tile's iterations are these copies
            // (cur and the sub-tiles are compile-time tags), so the steady-state iteration above is untouched.  Defined HERE, in
            // the discarded branch of every other instantiation: a lambda merely defined beside `iter` changes this closure's
            // layout and, through the register allocation, the code of kernels that never call it.
            auto iter_req = [&](int kt, auto cur_tag, auto t0_tag, auto t1_tag) __attribute__((always_inline)) {
                constexpr int cur = decltype(cur_tag)::value, T0 = decltype(t0_tag)::value, T1 = decltype(t1_tag)::value;
#pragma unroll
                for (int s = 0; s < NCH; ++s) {
                    if (s + 1 < NCH) ldf(ffa[(s + 1) & 1], ffb[(s + 1) & 1], cur, s + 1);
                    if (s == NCH - 1) {
                        __syncthreads();
                        ldf(ffa[0], ffb[0], cur ^ 1, 0);
                    }
                    VLG_SCHED_FENCE();
                    if (s == SS) {
                        store(cur ^ 1, 0);
                        load(kt + 1 + DEPTH, 0);
                    }
                    if (s == SS + 1 && T1 > T0) {
                        const __amdgpu_buffer_rsrc_t dxin = vlg_rsrc(gAuxIn ? gAuxIn + (m0 * g.ldc + n0v) : gA);
#pragma unroll
                        for (int t = T0; t < T1; ++t)
#pragma unroll
                            for (int r = 0; r < 16; ++r)       // (the loads of emit_fast's fetch: sub-tile (t / TN, t % TN), row of register r)
                                aux_early[t][r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
                                    dxin, vc_aux + (t % TN) * 128, ((t / TN) * 32 + (r & 3) + 8 * (r >> 2)) * rowb_aux, 0));
                    }
                    mma(ffa[s & 1], ffb[s & 1]);
                    if (s == SS) pin_staging<4 * TM * TN, TA::NV + TB::NV, TA::NV + TB::NV>();
                    if (s == SS + 1 && T1 > T0) pin_staging<4 * TM * TN, 0, 16 * (T1 - T0)>();
                }
            };
            // The last pair of iterations is peeled (a block-uniform branch BETWEEN pairs) and carries the requests, half of the
            // sub-tiles each: a wave then never has more than 8 + 32 + 8 + 32 loads outstanding when the first half has not
            // returned yet, and 48 when it has - the in-order counter holds 63, and a wave that would exceed it stalls at the
            // ISSUE of the load, MFMAs behind it included, until the oldest one returns (all 64 requests behind one staging load
            // stall at the 56th until that staging load is back).  nk = 1, 2 run this pair alone, the requests then sit behind
            // the prologue's loads.
            static_assert(DEPTH == 1 && SS + 1 < NCH, "the requesting copies: one staging set, a chunk behind the staging chunk");
            constexpr int E0 = (AUX_EARLY + 1) / 2;
            using I0 = std::integral_constant<int, 0>;
            using I1 = std::integral_constant<int, 1>;
            int kt = 0;
            for (; kt + 2 < nk; kt += 2) { iter(kt, 0); iter(kt + 1, 1); }
            if (kt < nk) {
                iter_req(kt, I0{}, I0{}, std::integral_constant<int, E0>{});
                iter_req(kt + 1, I1{}, std::integral_constant<int, E0>{}, std::integral_constant<int, AUX_EARLY>{});
            }
        } else {
            for (int kt = 0; kt < nk; kt += 2) { iter(kt, 0); iter(kt + 1, 1); }
        }
        __builtin_amdgcn_s_setprio(2);
    };
    // interior blocks (every tile fully inside both operands) take the unguarded instantiation
    const bool interior = (m0 + BM <= g.M) && (n0 + run * BN <= g.N) && (((kend - kbeg) % BK) == 0);
#ifdef VLG_TIMELINE
    tl_loop0 = __builtin_amdgcn_s_memrealtime();
#endif
    if constexpr (FAST) {
        // byte offsets from the tile origins are 32-bit in the fast path
        const int64_t ext = kend - kbeg;
        const int64_t span_a = A_KC ? (int64_t)(BM - 1) * g.lda + ext : ext * g.lda + BM;
        const int64_t span_b = B_KC ? (int64_t)(2 * BN - 1) * g.ldb + ext : ext * g.ldb + 2 * BN;   // (+ the next N tile of a run)
        const bool fits = span_a < (1ll << 28) && span_b < (1ll << 28) && (int64_t)(BM - 1) * g.ldc + BN < (1ll << 28);
        fast_tile = interior && fits;
        if (!fast_tile) mainloop(std::true_type{});
    } else {
        if (interior) mainloop(std::false_type{});
        else mainloop(std::true_type{});
    }
#ifdef VLG_TIMELINE
    tl_loop1 = __builtin_amdgcn_s_memrealtime();
#endif

#ifndef VLG_TIMELINE
    if (g.clock_probe && tid == 0) {
        g.clock_probe[2 * bid] = __builtin_amdgcn_s_memtime() - t0;
        g.clock_probe[2 * bid + 1] = __builtin_amdgcn_s_memrealtime() - r0;
    }
#endif
    // ---- epilogue.  C/D layout of the 32x32 MFMA: col = lane&31, row = (r&3) + 8*(r>>2) + 4*h.
    // 32 lanes of a half write one 128-B row segment per store.
    // (emit below is a copy of gemm16_emit, gemm_tile16.h - kept a copy: what is defined beside the fast path moves its registers)
    EO* Cs = static_cast<EO*>(g.C) + (int64_t)split * g.slab_stride;
    const int64_t row0 = m0 + wm * TM * 32 + 4 * h;
    const int col0 = n0 + wn * TN * 32 + l31;
    const int64_t base = row0 * g.ldc + col0;
    const bool full = (m0 + BM <= g.M) && (n0 + BN <= g.N);
    auto emit = [&](auto guard_tag) {
        constexpr bool GUARD = decltype(guard_tag)::value;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                if (GUARD && col0 + j * 32 >= g.N) continue;
                float aux[16];
                if constexpr ((EPI & (VLG_EPI_RESID | VLG_EPI_DGELU | VLG_EPI_MUL)) != 0) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int ro = i * 32 + (r & 3) + 8 * (r >> 2);
                        aux[r] = (!GUARD || row0 + ro < g.M) ? ld1(gAuxIn + base + ro * g.ldc + j * 32) : 0.f;
                    }
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int ro = i * 32 + (r & 3) + 8 * (r >> 2);
                    if (GUARD && row0 + ro >= g.M) continue;
                    const int64_t o = base + ro * g.ldc + j * 32;
                    float v = acc[i][j][r];
                    if constexpr ((EPI & VLG_EPI_GELU) != 0) {
                        if constexpr ((EPI & VLG_EPI_GELU_GRAD) != 0) {
                            float c, pd;
                            gelu_parts(v, c, pd);
                            st1(gAuxOut + o, c + v * pd);
                            v *= c;
                        } else {
                            st1(gAuxOut + o, v);
                            v = gelu_f(v);
                        }
                    }
                    if constexpr ((EPI & VLG_EPI_RESID) != 0) v += aux[r];
                    if constexpr ((EPI & VLG_EPI_DGELU) != 0) v *= dgelu_f(aux[r]);
                    if constexpr ((EPI & VLG_EPI_MUL) != 0) v *= aux[r];
                    st1(Cs + o, v);
                }
            }
    };
    // fast epilogue: no address arithmetic on the vector ALU (buffer stores: one loop-constant byte offset per thread, the
    // row in the scalar offset, the 32-column group in the immediate), GELU / dGELU on packed instructions, two rows at a time
    auto emit_fast = [&](int n0v) __attribute__((always_inline)) {
        const int64_t corner = m0 * g.ldc + n0v;
        const __amdgpu_buffer_rsrc_t dc = vlg_rsrc(Cs + corner);
        const __amdgpu_buffer_rsrc_t dxin = vlg_rsrc(gAuxIn ? gAuxIn + corner : gA);
        const __amdgpu_buffer_rsrc_t dxout = vlg_rsrc(gAuxOut ? gAuxOut + corner : Cs + corner);
        const int vc = ((wm * TM * 32 + 4 * h) * g.ldc + wn * TN * 32 + l31) * 4;
        const int rowb = g.ldc * 4;
        constexpr bool AUX = (EPI & (VLG_EPI_RESID | VLG_EPI_DGELU | VLG_EPI_MUL)) != 0;
        // the auxiliary operand: what the main loop has not requested already (AUX_EARLY sub-tiles, see aux_early) is requested
        // before the first store where the registers allow (BK = 32: two blocks per CU, 256 registers) - loads and stores
        // retire through one in-order counter, so a load issued behind a tile's stores is not usable before those stores
        // have landed; with three blocks per CU (BK = 16) one tile ahead
        constexpr bool AUX_ALL = BK == 32;
        constexpr int NAUX = AUX_ALL ? TM * TN : 2;
        float auxb[NAUX][16];
        auto fetch = [&](float (&a)[16], int i, int j) __attribute__((always_inline)) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                a[r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(dxin, vc + j * 128, (i * 32 + (r & 3) + 8 * (r >> 2)) * rowb, 0));
                vlg_epi_pace(r + 1);
            }
        };
        if constexpr (AUX_EARLY > 0) {
#pragma unroll
            for (int t = 0; t < AUX_EARLY; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) auxb[t][r] = aux_early[t][r];
        }
        if constexpr (AUX) {
            if constexpr (AUX_ALL) {
#pragma unroll
                for (int t = AUX_EARLY; t < TM * TN; ++t) fetch(auxb[t], t / TN, t % TN);
            } else {
                fetch(auxb[0], 0, 0);
            }
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int tix = i * TN + j;
                float (&aux)[16] = auxb[AUX_ALL ? tix : (tix & 1)];
                if constexpr (AUX && !AUX_ALL) {
                    if (tix + 1 < TM * TN) fetch(auxb[(tix + 1) & 1], (tix + 1) / TN, (tix + 1) % TN);
                }
                const auto soff = [&](int r) { return (i * 32 + (r & 3) + 8 * (r >> 2)) * rowb; };       // row of register r
                v2f v[8];                                                // the tile's 16 registers as 8 row pairs (r, r + 1)
#pragma unroll
                for (int q = 0; q < 8; ++q) v[q] = v2f{acc[i][j][2 * q], acc[i][j][2 * q + 1]};
                if constexpr ((EPI & VLG_EPI_GELU) != 0 && (EPI & VLG_EPI_GELU_GRAD) != 0) {
                    v2f dv[8];
                    gelu_both2n<8>(v, dv);
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(dv[q].x), dxout, vc + j * 128, soff(2 * q), 0);
                        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(dv[q].y), dxout, vc + j * 128, soff(2 * q + 1), 0);
                        vlg_epi_pace(2 * q + 2);
                    }
                } else if constexpr ((EPI & VLG_EPI_GELU) != 0) {
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[q].x), dxout, vc + j * 128, soff(2 * q), 0);
                        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[q].y), dxout, vc + j * 128, soff(2 * q + 1), 0);
                        vlg_epi_pace(2 * q + 2);
                    }
                    gelu2n<8>(v);
                }
                if constexpr ((EPI & VLG_EPI_RESID) != 0) {
#pragma unroll
                    for (int q = 0; q < 8; ++q) v[q] += v2f{aux[2 * q], aux[2 * q + 1]};
                }
                if constexpr ((EPI & VLG_EPI_MUL) != 0) {
#pragma unroll
                    for (int q = 0; q < 8; ++q) v[q] *= v2f{aux[2 * q], aux[2 * q + 1]};
                }
                if constexpr ((EPI & VLG_EPI_DGELU) != 0) {
                    v2f u[8], d[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q) u[q] = v2f{aux[2 * q], aux[2 * q + 1]};
                    dgelu2n<8>(u, d);
#pragma unroll
                    for (int q = 0; q < 8; ++q) v[q] *= d[q];
                }
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[q].x), dc, vc + j * 128, soff(2 * q), 0);
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[q].y), dc, vc + j * 128, soff(2 * q + 1), 0);
                    vlg_epi_pace(2 * q + 2);
                }
            }
    };
    if (fast_tile) {
        // the tiles of the run: [main loop, epilogue] per tile; the next tile's bias is fetched ahead of the main loop
        for (int rt = 0; rt < run; ++rt) {
            const int n0v = n0 + rt * BN;
            const bool has_next = rt + 1 < run;
            mainloop_fast(n0v, rt == 0, has_next);
            if (has_next) load_bias(n0v + BN);
            emit_fast(n0v);
            if (has_next) init_acc();
        }
    } else if (full) emit(std::false_type{});
    else emit(std::true_type{});
#ifdef VLG_TIMELINE
    if (g.clock_probe) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned long long tl_exit = __builtin_amdgcn_s_memrealtime();
        if (tid == 0) {
            unsigned long long* o = g.clock_probe + 8 * (size_t)bid;
            o[0] = tl_entry; o[1] = tl_loop0; o[2] = tl_loop1; o[3] = tl_exit;
            o[4] = __builtin_amdgcn_s_getreg(4 | (31 << 11));        // HW_REG_HW_ID
            o[5] = __builtin_amdgcn_s_getreg(20 | (31 << 11));       // HW_REG_XCC_ID
            o[6] = (unsigned long long)tile; o[7] = (unsigned long long)split;
        }
    }
#endif
    if constexpr (COLSUM) {
        static_assert(!A_KC, "column sums are taken from a contraction-major A tile");
        if (tn == 0) {                                  // block-uniform; the tiles are dead (the main loop ended on a barrier)
            constexpr int PR = TA::PER_ROW, NG = GEMM_THREADS / PR;       // threads per k-row, groups sharing the same rows
            float* red = smem;
            st4(red + (tid / PR) * BM + 4 * (tid % PR), make_float4(col_lo.x, col_lo.y, col_hi.x, col_hi.y));
            __syncthreads();
            if (tid < BM && m0 + tid < g.M) {
                float s = 0.f;
#pragma unroll 8
                for (int t = 0; t < NG; ++t) s += red[t * BM + tid];
                st1(Cs + g.colsum_off + m0 + tid, s);
            }
        }
    }
}

template <int BM, int BN, int BK, bool A_KC, bool B_KC, int EPI, bool COLSUM>
__global__ __launch_bounds__(GEMM_THREADS, (BM == 64 && BN == 64) ? 4 : (BK == 16 ? 3 : 2)) void gemm_f32_kernel(const GemmArgs g) {
    __shared__ __attribute__((aligned(16))) float smem[gemm_smem_floats<BM, BN, BK, A_KC, B_KC>()];
    gemm_f32_body<BM, BN, BK, A_KC, B_KC, EPI, COLSUM>(g, smem, (int)blockIdx.x, (int)gridDim.x);
}

// A projection's data gradient dX = dY . W and weight gradient dW = dY^T . X need nothing from each other: ONE launch runs
// both (blocks [0, nd_pad) the data gradient - nd of them real, padded to a multiple of 8 so that a block's number mod 8
// still names its XCD for the second problem - the rest the weight gradient).  Each problem's blocks execute exactly the code
// of its own launch (same tiles, same split plan, same sums: bit for bit the two launches), but the chip is dealt both at
// once: launches that cannot fill 256 CUs on their own (few tokens per GPU: the strong-scaling shard) share it, and one
// launch ramp / drain is paid instead of two.
// Blocks past both problems are RIDERS: rows of a slab-reduction table (the previous gradient bucket's partial sums, complete
// since the launches that wrote them precede this one on the stream; this launch's weight gradient writes the OTHER arena).
// The reduction is pure bandwidth work on 256-thread blocks that need 4 KB of LDS: it runs in the slots the GEMM blocks leave
// towards the end of the launch instead of as a launch of its own.
template <int BT, int EPI_D>
__global__ __launch_bounds__(GEMM_THREADS, BT == 64 ? 4 : 2) void gemm_pair_kernel(const GemmArgs gd, const GemmArgs gw, const int nd, const int nd_pad,
                                                                                   const int nw, const int64_t* __restrict__ rider, const int rider_bpr) {
    constexpr int FD = gemm_smem_floats<BT, BT, 32, true, false>(), FW = gemm_smem_floats<BT, BT, 32, false, false>();
    __shared__ __attribute__((aligned(16))) float smem_all[FD > FW ? FD : FW];
    const int b = (int)blockIdx.x;
    if (b < nd_pad) {
        if (b < nd) gemm_f32_body<BT, BT, 32, true, false, EPI_D, false>(gd, smem_all, b, nd);
    } else if (b < nd_pad + nw) {
        gemm_f32_body<BT, BT, 32, false, false, VLG_EPI_NONE, true>(gw, smem_all, b - nd_pad, nw);
    } else {
        const int rb = b - nd_pad - nw;
        reduce_table_row(rider, rb / rider_bpr, rb % rider_bpr, rider_bpr, reinterpret_cast<float4(*)[16]>(smem_all));
    }
}

// ---- host side.  The library keeps NO mutable process-wide state (include/vlg_hip.h).  The development switches below
// exist only in the diagnostic build (`make diag` -> libvlg_hip_diag.so, -DVLG_DIAG; loaded by tools/diag, tools/ab through
// VLG_HIP_LIB); in the product build they are constants (VLG_TUNE, common.h) and the vlg_debug_set_* entry points do not
// exist.  They are inputs of the planner (gemm_plan) and of nothing else.
#ifdef VLG_DIAG
// a device buffer of 2 * blocks uint64 set through vlg_debug_set_clock_probe (NULL = off)
static unsigned long long* vlg_gemm_clock_probe = nullptr;
extern "C" void vlg_debug_set_clock_probe(unsigned long long* p) { vlg_gemm_clock_probe = p; }
// VLG_GEMM_BK=16|32 (or vlg_debug_set_gemm_bk) forces one contraction depth for A/B runs
static int vlg_gemm_bk_forced = -1;
extern "C" void vlg_debug_set_gemm_bk(int bk) { vlg_gemm_bk_forced = (bk == 16 || bk == 32) ? bk : 0; }
// run: 0 = never chain, -1 = the library's choice, > 0 = that many
static int vlg_gemm_run_forced = -1;
extern "C" void vlg_debug_set_gemm_run(int run) { vlg_gemm_run_forced = run < 0 ? -1 : run; }
#else
static constexpr unsigned long long* vlg_gemm_clock_probe = nullptr;
static constexpr int vlg_gemm_bk_forced = -1, vlg_gemm_run_forced = -1;
#endif
static int gemm_bk_override() { return vlg_gemm_bk_forced >= 0 ? vlg_gemm_bk_forced : VLG_TUNE("VLG_GEMM_BK", 0); }

// The instantiated native-fp32 kernels.  The call fixes the operand layouts: forward A.W^T reads both operands
// contraction-contiguous, the data gradient dY.W reads W contraction-major, the weight gradient dY^T.X reads both
// contraction-major and sums the columns of dY.  128x128 tiles come at both contraction depths.
template <int CALL, int EPI, int BM, int BN, int BK>
constexpr GemmKernelRow f32_row() {
    return {CALL, EPI, 0, BM, BN, BK, gemm_f32_kernel<BM, BN, BK, CALL != VLG_CALL_WGRAD, CALL == VLG_CALL_FWD, EPI, CALL == VLG_CALL_WGRAD>};
}
#define EPI_GELU_GRAD (VLG_EPI_BIAS | VLG_EPI_GELU | VLG_EPI_GELU_GRAD)
#define EPI_ACT_FWD (VLG_EPI_BIAS | VLG_EPI_RESID | GEMM_A_GELU)      /* A = gelu(stored pre-activation): the FFN's second projection */
static const GemmKernelRow gemm_f32_kernels[] = {
    f32_row<VLG_CALL_FWD, EPI_ACT_FWD, 128, 128, 16>(), f32_row<VLG_CALL_FWD, EPI_ACT_FWD, 128, 128, 32>(),
    f32_row<VLG_CALL_FWD, VLG_EPI_BIAS, 128, 32, 32>(), f32_row<VLG_CALL_FWD, VLG_EPI_BIAS, 64, 64, 32>(),
    f32_row<VLG_CALL_FWD, VLG_EPI_BIAS, 128, 128, 16>(), f32_row<VLG_CALL_FWD, VLG_EPI_BIAS, 128, 128, 32>(),
    f32_row<VLG_CALL_FWD, VLG_EPI_BIAS | VLG_EPI_GELU, 64, 64, 32>(),
    f32_row<VLG_CALL_FWD, VLG_EPI_BIAS | VLG_EPI_GELU, 128, 128, 16>(), f32_row<VLG_CALL_FWD, VLG_EPI_BIAS | VLG_EPI_GELU, 128, 128, 32>(),
    f32_row<VLG_CALL_FWD, EPI_GELU_GRAD, 64, 64, 32>(),
    f32_row<VLG_CALL_FWD, EPI_GELU_GRAD, 128, 128, 16>(), f32_row<VLG_CALL_FWD, EPI_GELU_GRAD, 128, 128, 32>(),
    f32_row<VLG_CALL_FWD, VLG_EPI_BIAS | VLG_EPI_RESID, 64, 64, 32>(),
    f32_row<VLG_CALL_FWD, VLG_EPI_BIAS | VLG_EPI_RESID, 128, 128, 16>(), f32_row<VLG_CALL_FWD, VLG_EPI_BIAS | VLG_EPI_RESID, 128, 128, 32>(),
    f32_row<VLG_CALL_DGRAD, VLG_EPI_NONE, 64, 64, 32>(),
    f32_row<VLG_CALL_DGRAD, VLG_EPI_NONE, 128, 128, 16>(), f32_row<VLG_CALL_DGRAD, VLG_EPI_NONE, 128, 128, 32>(),
    f32_row<VLG_CALL_DGRAD, VLG_EPI_DGELU, 64, 64, 32>(),
    f32_row<VLG_CALL_DGRAD, VLG_EPI_DGELU, 128, 128, 16>(), f32_row<VLG_CALL_DGRAD, VLG_EPI_DGELU, 128, 128, 32>(),
    f32_row<VLG_CALL_DGRAD, VLG_EPI_MUL, 64, 64, 32>(),
    f32_row<VLG_CALL_DGRAD, VLG_EPI_MUL, 128, 128, 16>(), f32_row<VLG_CALL_DGRAD, VLG_EPI_MUL, 128, 128, 32>(),
    // (X = gelu(stored pre-activation): weight gradient of the FFN's second projection)
    f32_row<VLG_CALL_WGRAD, GEMM_B_GELU, 128, 128, 16>(), f32_row<VLG_CALL_WGRAD, GEMM_B_GELU, 128, 128, 32>(),
    f32_row<VLG_CALL_WGRAD, VLG_EPI_NONE, 64, 64, 32>(), f32_row<VLG_CALL_WGRAD, VLG_EPI_NONE, 32, 128, 32>(),
    f32_row<VLG_CALL_WGRAD, VLG_EPI_NONE, 128, 128, 16>(), f32_row<VLG_CALL_WGRAD, VLG_EPI_NONE, 128, 128, 32>(),
};
static GemmPairKernel gemm_f32_pair_kernel(int bt, int epi_d) {
    if (bt == 64) return epi_d == VLG_EPI_MUL ? gemm_pair_kernel<64, VLG_EPI_MUL> : gemm_pair_kernel<64, VLG_EPI_NONE>;
    return epi_d == VLG_EPI_MUL ? gemm_pair_kernel<128, VLG_EPI_MUL> : gemm_pair_kernel<128, VLG_EPI_NONE>;
}

// ================================================================================================ the planner
// gemm_plan() is the ONE place that decides how a vlg_linear_* call runs: kernel family, tile, contraction depth, chained N
// tiles, the weight gradient's split, one fused launch or two for a pair - and whether the call has a kernel at all.  It
// is a function of the call's shape, flags and leading dimensions (and, in the diagnostic build, of the switches above):
// the entry points launch what it returns, vlg_linear_plan and the slab-count queries report it.

// storage bits of the flags word -> IO template value (bit 0 A, bit 1 B, bit 2 C + aux)
static int gemm_io_bits(int flags) {
    return ((flags & VLG_EPI_A_BF16) ? 1 : 0) | ((flags & VLG_EPI_B_BF16) ? 2 : 0) | ((flags & VLG_EPI_OUT_BF16) ? 4 : 0);
}
#define VLG_EPI_STORAGE (VLG_EPI_A_BF16 | VLG_EPI_B_BF16 | VLG_EPI_OUT_BF16)

// What the caller's buffers add to the checks of a call, so that the planner applies every check in the one order the
// entry points have always applied them.  The plan queries pass none: every buffer is taken to be fine.
struct GemmBufs {
    bool ab_ok = true;            // fwd, dgrad: both operands 16-byte aligned and the output non-NULL
    bool wg_ok = true;            // wgrad: dY and X 16-byte aligned, slabs non-NULL
    bool bias = true, aux_in = true, aux_out = true;      // present
    bool out16_ok = true;         // bf16 outputs: C (and aux_out) 16-byte aligned
    bool slabs = false;           // wgrad: the caller's slab stride and capacity, to be checked
    int64_t slab_stride = 0, slab_capacity = 0;
};

// 64x64 tiles (four 32x32 waves, four blocks per CU) for launches whose 128x128 tiles would leave CUs without a block: the
// per-GPU share of a GLOBAL batch (reference src/trainer.py:148: 32 // 8 = 4 clips, M = 4 096 tokens) gives the N = 256
// products 64 tiles for 256 CUs.  VLG_GEMM_SMALL=0 keeps 128x128 everywhere (A/B runs).
// Measured (tools/shard_bench.py, interleaved repeated runs on one box): 64x64 tiles pay while the 128x128 tiles would not fill
// the 512 block slots of the chip (2 per CU) - four resident 64x64 blocks overlap one block's prologue / epilogue with the
// others' MFMAs: B = 4: 1.75 -> 1.05 ms, B = 8: 1.79 -> 1.76, B = 16: 3.11 -> 3.05.  A launch of exactly 512 blocks (the d x d
// products of the headline step) is FASTER on 128x128 tiles (their higher arithmetic intensity: K = 4096 asymptote 150 vs 140
// TFLOP/s; the step 5.55 vs 5.63 ms with a threshold of 1 025 - a first single-run sweep had suggested the opposite).
static bool gemm_small_tiles() { return VLG_TUNE("VLG_GEMM_SMALL", 1) != 0; }
static bool gemm_wants_small(int64_t M, int N) {
    return gemm_small_tiles() && ((M + 127) / 128) * (int64_t)((N + 127) / 128) < VLG_TUNE("VLG_GEMM_SMALL_BELOW", 512);
}

// Consecutive N tiles per block (GemmArgs::run) of a 128x128, BK = 32 launch that would otherwise take several rounds of
// blocks: the largest divisor of the N tile count that still leaves one block per slot (512 = 256 CUs x 2).  Only where
// EVERY block takes the fast path (no edge tiles, an even number of K tiles, 32-bit spans): a block that does not
// computes one tile only.  A is contraction-contiguous in every launch that may chain (forward, data gradient).
// (The span test restates `fits` of gemm_f32_body for BM = BN = 128 and a contraction-contiguous A: sharing one helper
// with the kernel changed its register allocation, and the device code is to stay as it is.)
static int gemm_run(int64_t M, int N, int64_t Kc, int lda, int ldb, int ldc, bool b_kc) {
    if (M % 128 != 0 || N % 128 != 0 || Kc % 64 != 0 || vlg_gemm_run_forced == 0) return 1;
    const int64_t span_a = (int64_t)127 * lda + Kc, span_b = b_kc ? (int64_t)255 * ldb + Kc : Kc * ldb + 256;
    if (span_a >= (1ll << 28) || span_b >= (1ll << 28) || (int64_t)127 * ldc + 128 >= (1ll << 28)) return 1;
    const int64_t tiles_m = M / 128;
    const int tiles_n = N / 128;
    int best = 1;
    for (int r = 2; r <= tiles_n; ++r)
        if (tiles_n % r == 0 && tiles_m * (tiles_n / r) >= 512) best = r;
    if (vlg_gemm_run_forced > 0 && tiles_n % vlg_gemm_run_forced == 0) best = vlg_gemm_run_forced;
    return best;
}

// Split of the weight gradient over the tokens: enough blocks to fill 256 CUs x 2 blocks, each split a multiple of 64 token rows.
// small (native fp32 kernel only: flags without the bf16 / split / GELU-on-load bits): 64x64 tiles, four resident blocks per
// CU, token ranges down to 128 rows - taken when the 128x128 plan would leave CUs without a block (few tokens: the
// strong-scaling shard): under 3/4 of the 512 slots (B = 32 keeps the 128x128 plan: 504-512 blocks).
static void wgrad_split(GemmProblem& p, int64_t M, int N, int K, bool native) {
    const int bm = N <= 32 ? 32 : 128;
    int64_t tiles = ((N + bm - 1) / bm) * (int64_t)((K + 127) / 128);
    int64_t want = 512 / tiles;                      // blocks <= 512 = 256 CUs x 2 resident blocks: one full wave, no tail
    int64_t max_splits = (M + 255) / 256;
    const bool small = native && bm == 128 && gemm_small_tiles() &&
                       tiles * (want < max_splits ? (want < 1 ? 1 : want) : max_splits) < VLG_TUNE("VLG_GEMM_SMALL_BELOW_WGRAD", 385);
    if (small) {
        tiles = ((N + 63) / 64) * (int64_t)((K + 63) / 64);
        want = VLG_TUNE("VLG_WGRAD_SMALL_SLOTS", 1024) / tiles;
        max_splits = (M + 127) / 128;
    }
    if (want > max_splits) want = max_splits;
    if (want < 1) want = 1;
    if (small) {
        // equal token ranges where a slightly smaller count allows them (a ragged last range costs a whole block round)
        for (int64_t c = want; c >= 1 && 4 * c >= 3 * want; --c)
            if (M % (c * 64) == 0) { want = c; break; }
    }
    // whole K tiles, and an even number of the fp32 kernel's 32-row tiles (its loop runs them in pairs: an odd count costs
    // one iteration on zeros)
    p.per = ((M + want - 1) / want + 63) / 64 * 64;
    p.splits = (int)((M + p.per - 1) / p.per);
    p.bm = small ? 64 : bm;
    p.bn = small ? 64 : 128;
}

// Argument checks of the three single calls, up to the choice of a kernel; the pair accepts exactly what its two single calls accept.
static int check_fwd(int64_t M, int N, int K, int flags, int lda, int ldw, int ldc, const GemmBufs& b) {
    if (M < 1 || N < 1 || K < 4 || (K & 3) || lda < K || ldw < K || ldc < N) return VLG_ERR_SHAPE;
    if (!b.ab_ok || (lda & 3) || (ldw & 3)) return VLG_ERR_ALIGN;
    const bool bf16 = (flags & VLG_EPI_BF16) != 0, split3 = (flags & VLG_EPI_SPLIT3) != 0, act_gelu = (flags & VLG_EPI_ACT_GELU) != 0;
    const int io = gemm_io_bits(flags);
    const int epi = flags & ~(VLG_EPI_BF16 | VLG_EPI_STORAGE | VLG_EPI_SPLIT3);
    if (split3 && (bf16 || io != 0)) return VLG_ERR_SHAPE;
    if (((epi & VLG_EPI_BIAS) && !b.bias) || ((epi & (VLG_EPI_RESID | VLG_EPI_DGELU)) && !b.aux_in) || ((epi & VLG_EPI_GELU) && !b.aux_out))
        return VLG_ERR_SHAPE;
    if ((epi & VLG_EPI_MUL) != 0) return VLG_ERR_SHAPE;                                               // a dgrad epilogue
    if ((epi & VLG_EPI_GELU_GRAD) && (split3 || epi != EPI_GELU_GRAD)) return VLG_ERR_SHAPE;          // native fp32 and bf16 paths
    if (act_gelu && (bf16 || split3)) return VLG_ERR_SHAPE;                                           // native fp32 path only
    if (io != 0 && !bf16) return VLG_ERR_SHAPE;      // bf16 activation storage exists for the bf16 MFMA mode only
    if (((io & 1) && (lda & 7)) || ((io & 2) && (ldw & 7))) return VLG_ERR_ALIGN;
    return 0;
}
static int check_dgrad(int64_t M, int N, int K, int flags, int ldy, int ldw, int ldx, const GemmBufs& b) {
    if (M < 1 || N < 4 || (N & 3) || K < 4 || (K & 3) || ldy < N || ldw < K || ldx < K) return VLG_ERR_SHAPE;
    if (!b.ab_ok || (ldy & 3) || (ldw & 3)) return VLG_ERR_ALIGN;
    const bool bf16 = (flags & VLG_EPI_BF16) != 0, split3 = (flags & VLG_EPI_SPLIT3) != 0;
    const int io = gemm_io_bits(flags);
    const int epi = flags & ~(VLG_EPI_BF16 | VLG_EPI_STORAGE | VLG_EPI_SPLIT3);
    if (split3 && (bf16 || io != 0)) return VLG_ERR_SHAPE;
    if (io != 0 && !bf16) return VLG_ERR_SHAPE;
    if (((io & 1) && (ldy & 7)) || ((io & 2) && (ldw & 7))) return VLG_ERR_ALIGN;
    if ((epi == VLG_EPI_DGELU || epi == VLG_EPI_MUL) && !b.aux_in) return VLG_ERR_SHAPE;
    if (epi == VLG_EPI_MUL && split3) return VLG_ERR_SHAPE;                                           // native fp32 and bf16 paths
    return 0;
}
static int check_wgrad(int64_t M, int N, int K, int flags, int ldy, int ldx, const GemmBufs& b) {
    if (M < 1 || N < 4 || (N & 3) || K < 4 || (K & 3) || ldy < N || ldx < K) return VLG_ERR_SHAPE;
    if (b.slabs && b.slab_stride < (int64_t)N * K + N) return VLG_ERR_SHAPE;
    if (!b.wg_ok || (ldy & 3) || (ldx & 3)) return VLG_ERR_ALIGN;
    const int io = gemm_io_bits(flags);
    if (io != 0 && !(flags & VLG_EPI_BF16)) return VLG_ERR_SHAPE;
    if (((io & 1) && (ldy & 7)) || ((io & 2) && (ldx & 7))) return VLG_ERR_ALIGN;
    return 0;
}

// One single call's kernel: family, tile, depth, chaining, split, instantiation, grid.  Every field is filled whatever the
// result (M, N, K >= 1); the result is 0 or the refusal.  bk_forced: 0 = the library's choice.
static int gemm_problem(GemmProblem& p, int call, int64_t M, int N, int K, int flags, int lda, int ldb, int ldc, int bk_forced, const GemmBufs& b) {
    const bool fwd = call == VLG_CALL_FWD, wgrad = call == VLG_CALL_WGRAD;
    const bool act = !(call == VLG_CALL_DGRAD) && (flags & VLG_EPI_ACT_GELU) != 0, narrow = N <= 32;
    p = GemmProblem{};
    p.call = call;
    p.family = (flags & VLG_EPI_BF16) ? VLG_GEMM_BF16 : (flags & VLG_EPI_SPLIT3) ? VLG_GEMM_F32X3 : VLG_GEMM_F32;
    const bool native = p.family == VLG_GEMM_F32;
    p.io = gemm_io_bits(flags);
    // (a weight gradient has no epilogue and ignores the bits; the data gradient knows no GELU on load and finds no kernel for the bit)
    p.epi = wgrad ? (act && native ? GEMM_B_GELU : 0)
                  : (flags & ~(VLG_EPI_BF16 | VLG_EPI_STORAGE | VLG_EPI_SPLIT3 | (fwd ? VLG_EPI_ACT_GELU : 0))) | (act && native ? GEMM_A_GELU : 0);
    // the product in the kernel's terms: C[gM, gN] = A . B over gK
    const int64_t gM = wgrad ? N : M, gK = fwd ? K : wgrad ? M : N;
    const int gN = fwd ? N : K;
    p.bm = 128; p.bn = 128; p.run = 1; p.splits = 1; p.per = gK;
    p.bk = native ? 32 : p.family == VLG_GEMM_BF16 ? 64 : 16;
    // tiles.  32 wide for the narrow side of the head's products (N <= 32), where that kernel exists; the native kernels
    // without bias-gradient sums and GELU on load have 64x64 twins (the weight gradient's come with its split)
    if (wgrad) wgrad_split(p, M, N, K, native && !act);
    else if (fwd && narrow && (!native || p.epi == VLG_EPI_BIAS)) p.bn = 32;
    else if (native && !act && gemm_wants_small(gM, gN)) p.bm = p.bn = 64;
    // contraction depth and chaining of the native 128x128 kernels.  Measured on MI355X at the metric shape
    // (tools/kernel_bench.py): BK = 32 (2 blocks / CU) is 3-5 % faster for plain epilogues, BK = 16 (41 KB LDS, 3 blocks /
    // CU) is 8-11 % faster when the epilogue is heavy (GELU / dGELU: two extra 134 MB streams), because more resident
    // blocks de-synchronise the store bursts from the other blocks' MFMA phases - unless the tiles chain (run > 1).
    if (native && p.bm == 128 && p.bn == 128) {
        const bool heavy = (p.epi & (VLG_EPI_GELU | VLG_EPI_DGELU)) != 0;
        const int run32 = (wgrad || act) ? 1 : gemm_run(gM, gN, gK, lda, ldb, ldc, fwd);
        if (bk_forced == 16 || (bk_forced != 32 && heavy && run32 == 1)) p.bk = 16;
        else p.run = run32;
    }
    p.kernel = native ? gemm_find_kernel(gemm_f32_kernels, sizeof(gemm_f32_kernels) / sizeof(gemm_f32_kernels[0]), p)
                      : p.family == VLG_GEMM_BF16 ? vlg_gemm16_kernel(p) : vlg_gemm_split_kernel(p);
    p.blocks = ((gM + p.bm - 1) / p.bm) * (((gN + p.bn - 1) / p.bn) / p.run) * p.splits;

    // the caller's slab buffer must hold every slab
    if (wgrad && b.slabs && b.slab_capacity < (int64_t)p.splits * b.slab_stride) return VLG_ERR_SHAPE;
    if (!wgrad && p.family == VLG_GEMM_BF16 && (p.io & 4) && ((ldc & 7) || !b.out16_ok)) return VLG_ERR_ALIGN;
    // bf16 LDS tiles are filled in 8-element slots: every memory-contiguous extent of the two operands in whole slots
    if (!native && (fwd ? (K & 7) : ((N | K) & 7)) != 0) return VLG_ERR_SHAPE;
    if (act && (!native || narrow)) return VLG_ERR_SHAPE;
    if (!p.kernel || p.blocks < 1 || p.blocks > 0x7fffffff) return VLG_ERR_SHAPE;
    return 0;
}

// ---- data gradient + weight gradient of one projection in ONE launch (gemm_pair_kernel, gemm16_pair_kernel)
// VLG_GEMM_PAIR (diagnostic build): 0 = always two launches, 1 = one launch only where both problems take the 64x64 tiles (few
// tokens: neither fills the chip alone), 2 (default) = also on 128x128 tiles.  Measured at the metric shape (interleaved
// repeated runs, one box): 5.553 -> 5.500 ms per step (-1.0 %, three of three pairs of runs) - each launch pays one ramp
// and one drain for two problems, and the second problem's blocks fill the slots the first one's stragglers leave.
#define VLG_RIDER_BPR 128          /* blocks per table row: what vlg_reduce_slabs_table launches get from the engine */

// call: VLG_CALL_*; (M, N, K) and the leading dimensions as the entry point of that call takes them: (lda, ldb, ldc) =
// fwd (lda, ldw, ldc), dgrad (ldy, ldw, ldx), wgrad (ldy, ldx, -), pair (ldy, ldw, ldx) + ldxx.  O(N tiles) arithmetic.
static GemmPlan gemm_plan(int call, int64_t M, int N, int K, int flags, int lda, int ldb, int ldc, int ldxx = 0, const GemmBufs& b = GemmBufs{}) {
    GemmPlan r{};
    r.n = call == VLG_CALL_PAIR ? 2 : 1;
    r.err = VLG_ERR_SHAPE;
    if (call < VLG_CALL_FWD || call > VLG_CALL_PAIR || M < 1 || N < 1 || K < 1) return r;
    auto first = [](int e0, int e1) { return e0 ? e0 : e1; };
    if (call != VLG_CALL_PAIR) {
        const int e = call == VLG_CALL_FWD ? check_fwd(M, N, K, flags, lda, ldb, ldc, b)
                    : call == VLG_CALL_DGRAD ? check_dgrad(M, N, K, flags, lda, ldb, ldc, b) : check_wgrad(M, N, K, flags, lda, ldb, b);
        r.err = first(e, gemm_problem(r.p[0], call, M, N, K, flags, lda, ldb, call == VLG_CALL_WGRAD ? K : ldc, gemm_bk_override(), b));
        return r;
    }
    // the weight gradient's flags (bf16 storage: A = the shared dY, B = W of the data gradient AND X of the weight gradient)
    const int wflags = flags & (VLG_EPI_BF16 | VLG_EPI_SPLIT3 | VLG_EPI_A_BF16 | VLG_EPI_B_BF16);
    const int e = first(check_wgrad(M, N, K, wflags, lda, ldxx, b), check_dgrad(M, N, K, flags, lda, ldb, ldc, b));
    GemmProblem &d = r.p[0], &w = r.p[1];
    int ew = gemm_problem(w, VLG_CALL_WGRAD, M, N, K, wflags, lda, ldxx, K, gemm_bk_override(), b);
    int ed = gemm_problem(d, VLG_CALL_DGRAD, M, N, K, flags, lda, ldb, ldc, gemm_bk_override(), b);
    // fusable into one launch: the data gradient's epilogue is NONE or MUL and both products are wide, and
    //   native fp32: both problems on the same tiles (64x64 at few tokens, 128x128 elsewhere - VLG_GEMM_PAIR >= 2)
    //   bf16 storage (bf16 W / X / dX, dY bf16 or fp32; VLG_GEMM_PAIR >= 2): the bf16-tile pair kernel at every shape - but
    //   not MUL with a bf16 dY, which the single data gradient has no kernel for
    const int st_bits = flags & VLG_EPI_STORAGE;
    const bool a16 = (st_bits & VLG_EPI_A_BF16) != 0, mul = d.epi == VLG_EPI_MUL;
    const bool bf16_pair = (flags & VLG_EPI_BF16) && (st_bits & ~VLG_EPI_A_BF16) == (VLG_EPI_B_BF16 | VLG_EPI_OUT_BF16);
    const bool native = d.family == VLG_GEMM_F32 && w.family == VLG_GEMM_F32;
    const int mode = VLG_TUNE("VLG_GEMM_PAIR", 2);
    r.fused = (d.epi == VLG_EPI_NONE || mul) && N > 32 && K > 32 &&
              (bf16_pair ? (mode > 1 && !(mul && a16)) : (native && mode > 0 && w.bm == d.bm && (d.bm == 64 || mode > 1)));
    if (r.fused) {
        // the pair kernels are built at the families' one depth (native: BK = 32); a misaligned bf16 dX is a shape error here
        ew = gemm_problem(w, VLG_CALL_WGRAD, M, N, K, wflags, lda, ldxx, K, 32, b);
        ed = gemm_problem(d, VLG_CALL_DGRAD, M, N, K, flags, lda, ldb, ldc, 32, b) ? VLG_ERR_SHAPE : 0;
        r.pair = bf16_pair ? vlg_gemm16_pair_kernel(d.epi, a16) : gemm_f32_pair_kernel(d.bm, d.epi);
        // (the data gradient's blocks are padded to a multiple of 8: a block's number mod 8 still names its XCD for the second problem)
        if ((d.blocks + 7) / 8 * 8 + w.blocks > 0x7fffffff) ed = VLG_ERR_SHAPE;
    }
    r.err = first(e, first(ew, ed));
    return r;
}

extern "C" int vlg_linear_plan(int call, int64_t M, int N, int K, int flags, int lda, int ldb, int ldc, int ldxx, vlg_gemm_plan* out) {
    const GemmPlan r = gemm_plan(call, M, N, K, flags, lda, ldb, ldc, ldxx);
    if (!out) return VLG_ERR_ALIGN;
    *out = vlg_gemm_plan{};
    if (r.err) return r.err;
    out->family = r.p[0].family; out->problems = r.n; out->fused = r.fused ? 1 : 0; out->launches = r.n == 2 && !r.fused ? 2 : 1;
    for (int i = 0; i < r.n; ++i) {
        const GemmProblem& p = r.p[i];
        out->p[i] = vlg_gemm_problem{p.bm, p.bn, p.bk, p.run, p.splits, (int)p.blocks, p.per};
    }
    return 0;
}
// (every M >= 1, N >= 1, K >= 1: the split follows from the extents and the mode bits, also where the call itself is refused)
extern "C" int vlg_linear_wgrad_slabs_for(int64_t M, int N, int K, int flags) { return gemm_plan(VLG_CALL_WGRAD, M, N, K, flags, N, K, K).p[0].splits; }
extern "C" int vlg_linear_wgrad_slabs(int64_t M, int N, int K) { return vlg_linear_wgrad_slabs_for(M, N, K, 0); }

// ================================================================================================ the launches
// One launch of one problem, whatever the family: host-only arguments, grid and kernel come from the plan.
static int gemm_launch(GemmArgs g, const GemmProblem& p, hipStream_t s) {
    gemm_apply_plan(g, p, p.family == VLG_GEMM_F32 ? vlg_gemm_clock_probe : nullptr);
    hipLaunchKernelGGL(p.kernel, dim3((unsigned)p.blocks), dim3(GEMM_THREADS), 0, s, g);
    return vlg_last_error();
}
// A fused pair: blocks [0, nd_pad) the data gradient, [nd_pad, nd_pad + nw) the weight gradient, then the rider rows.
static int gemm_launch_pair(GemmArgs gd, GemmArgs gw, const GemmPlan& plan, const int64_t* rider, int rider_rows, hipStream_t s) {
    gemm_apply_plan(gd, plan.p[0], nullptr);
    gemm_apply_plan(gw, plan.p[1], nullptr);
    const int64_t nd = plan.p[0].blocks, nw = plan.p[1].blocks, nd_pad = (nd + 7) / 8 * 8;
    const int64_t nr = rider ? (int64_t)rider_rows * VLG_RIDER_BPR : 0;
    if (nd_pad + nw + nr > 0x7fffffff) return VLG_ERR_SHAPE;
    hipLaunchKernelGGL(plan.pair, dim3((unsigned)(nd_pad + nw + nr)), dim3(GEMM_THREADS), 0, s, gd, gw, (int)nd, (int)nd_pad, (int)nw, rider,
                       VLG_RIDER_BPR);
    return vlg_last_error();
}

// C[M,N] = A[M,K] . W[N,K]^T
static GemmArgs fwd_args(const void* A, int lda, const void* W, int ldw, const float* bias, void* C, int ldc, const void* aux_in,
                         void* aux_out, int64_t M, int N, int K) {
    GemmArgs g{};
    g.A = A; g.B = W; g.C = C; g.bias = bias; g.aux_in = aux_in; g.aux_out = aux_out;
    g.M = M; g.N = N; g.Kc = K; g.lda = lda; g.ldb = ldw; g.ldc = ldc;
    return g;
}
// dX[M,K] = dY[M,N] . W[N,K]  : contraction over N, W is contraction-major
static GemmArgs dgrad_args(const void* dY, int ldy, const void* W, int ldw, void* dX, int ldx, const void* aux_in, int64_t M, int N, int K) {
    GemmArgs g{};
    g.A = dY; g.B = W; g.C = dX; g.aux_in = aux_in;
    g.M = M; g.N = K; g.Kc = N; g.lda = ldy; g.ldb = ldw; g.ldc = ldx;
    return g;
}
// slab[s][n*K + k] = sum_{m in split s} dY[m,n] X[m,k] ;  slab[s][N*K + n] = sum_m dY[m,n]
static GemmArgs wgrad_args(const void* dY, int ldy, const void* X, int ldx, float* slabs, int64_t slab_stride, int64_t M, int N, int K) {
    GemmArgs g{};
    g.A = dY; g.B = X; g.C = slabs;
    g.M = N; g.N = K; g.Kc = M; g.lda = ldy; g.ldb = ldx; g.ldc = K;
    g.slab_stride = slab_stride; g.colsum_off = (int64_t)N * K;
    return g;
}

// Every entry point: the buffers' facts, the plan (all checks), then - only for an accepted call - the launches.
extern "C" int vlg_linear_fwd(const void* A, int lda, const void* W, int ldw, const float* bias,
                              void* C, int ldc, const void* aux_in, void* aux_out,
                              int64_t M, int N, int K, int epilogue, void* stream) {
    GemmBufs b;
    b.ab_ok = vlg_aligned16(A) && vlg_aligned16(W) && C;
    b.bias = bias; b.aux_in = aux_in; b.aux_out = aux_out;
    b.out16_ok = vlg_aligned16(C) && vlg_aligned16(aux_out);
    const GemmPlan plan = gemm_plan(VLG_CALL_FWD, M, N, K, epilogue, lda, ldw, ldc, 0, b);
    if (plan.err) return plan.err;
    return gemm_launch(fwd_args(A, lda, W, ldw, bias, C, ldc, aux_in, aux_out, M, N, K), plan.p[0], (hipStream_t)stream);
}

extern "C" int vlg_linear_dgrad(const void* dY, int ldy, const void* W, int ldw, void* dX, int ldx,
                                const void* aux_in, int64_t M, int N, int K, int epilogue, void* stream) {
    GemmBufs b;
    b.ab_ok = vlg_aligned16(dY) && vlg_aligned16(W) && dX;
    b.aux_in = aux_in;
    b.out16_ok = vlg_aligned16(dX);
    const GemmPlan plan = gemm_plan(VLG_CALL_DGRAD, M, N, K, epilogue, ldy, ldw, ldx, 0, b);
    if (plan.err) return plan.err;
    return gemm_launch(dgrad_args(dY, ldy, W, ldw, dX, ldx, aux_in, M, N, K), plan.p[0], (hipStream_t)stream);
}

extern "C" int vlg_linear_wgrad(const void* dY, int ldy, const void* X, int ldx, float* slabs,
                                int64_t slab_stride, int64_t slab_capacity, int64_t M, int N, int K, int flags, void* stream) {
    GemmBufs b;
    b.wg_ok = vlg_aligned16(dY) && vlg_aligned16(X) && slabs;
    b.slabs = true; b.slab_stride = slab_stride; b.slab_capacity = slab_capacity;
    const GemmPlan plan = gemm_plan(VLG_CALL_WGRAD, M, N, K, flags, ldy, ldx, 0, 0, b);
    if (plan.err) return plan.err;
    return gemm_launch(wgrad_args(dY, ldy, X, ldx, slabs, slab_stride, M, N, K), plan.p[0], (hipStream_t)stream);
}

extern "C" int vlg_reduce_slabs_table(const int64_t* table, int n_rows, int blocks_per_row, void* stream);

extern "C" int vlg_linear_dgrad_wgrad(const void* dY, int ldy, const void* W, int ldw, void* dX, int ldx, const void* aux_in,
                                      const void* X, int ldxx, float* slabs, int64_t slab_stride, int64_t slab_capacity,
                                      int64_t M, int N, int K, int epilogue, const int64_t* rider_table, int rider_rows,
                                      void* stream) {
    // dX[M,K] = dY[M,N] . W[N,K] (x aux_in with VLG_EPI_MUL)   and   slab[s] = dY^T . X, column sums of dY  - the results of
    // vlg_linear_wgrad followed by vlg_linear_dgrad with the same arguments, bit for bit.  rider_table (may be NULL): rows of
    // a slab-reduction table (vlg_reduce_slabs_table) over OTHER buffers than this call writes, reduced by extra blocks of the
    // same launch where the two products are fused, by a launch of their own otherwise - same sums either way.
    if (rider_table != nullptr && (rider_rows < 1 || rider_rows > 4096)) return VLG_ERR_SHAPE;
    GemmBufs b;
    b.wg_ok = vlg_aligned16(dY) && vlg_aligned16(X) && slabs;
    b.ab_ok = vlg_aligned16(dY) && vlg_aligned16(W) && dX;
    b.aux_in = aux_in;
    b.out16_ok = vlg_aligned16(dX);
    b.slabs = true; b.slab_stride = slab_stride; b.slab_capacity = slab_capacity;
    const GemmPlan plan = gemm_plan(VLG_CALL_PAIR, M, N, K, epilogue, ldy, ldw, ldx, ldxx, b);
    if (plan.err) return plan.err;
    const GemmArgs gd = dgrad_args(dY, ldy, W, ldw, dX, ldx, aux_in, M, N, K);
    const GemmArgs gw = wgrad_args(dY, ldy, X, ldxx, slabs, slab_stride, M, N, K);
    hipStream_t s = (hipStream_t)stream;
    if (plan.fused) return gemm_launch_pair(gd, gw, plan, rider_table, rider_rows, s);
    if (rider_table != nullptr) {
        if (const int rc = vlg_reduce_slabs_table(rider_table, rider_rows, VLG_RIDER_BPR, stream)) return rc;
    }
    if (const int rc = gemm_launch(gw, plan.p[1], s)) return rc;
    return gemm_launch(gd, plan.p[0], s);
}
