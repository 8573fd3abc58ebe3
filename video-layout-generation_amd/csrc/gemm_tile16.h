// bf16 operand tiles in LDS for the bf16-MFMA GEMMs (gemm_bf16.hip, gemm_split.hip): images, staging, fragment reads;
// below them the block frame those kernels share (placement, start-up, epilogue, bias-gradient reduction).
//   KC image  [row][k]   rows of BK bf16 + 8 pad: per-lane 16-byte fragment reads (ds_read_b128, lane = row, half-wave h
//                        picks k = 16s + 8h ..+7) are bank-conflict-free for BK = 64 (36-dword rows) and 16 (12-dword rows)
//   MC image  [k][row]   the operand is contraction-major in memory: stored as it arrives and read with gfx950's
//                        TRANSPOSING LDS read ds_read_b64_tr_b16 - each 16-lane group fetches a 4(k) x 16(row) block and
//                        every lane receives the 4 k-values of ITS row; two reads make the 8-deep MFMA operand.  Row stride
//                        = BR*2 + 64 bytes: the four k-rows of a block start 64 B apart modulo the 256-B bank window.
// Both images give lane (row = l & 31, h = l >> 5) the k-values 16s + 8h + j, j = 0..7.
#pragma once
#include "gemm_tile.h"
#include <type_traits>

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;


// pack 8 fp32 values (two float4) into 8 bf16 (round to nearest even)
__device__ __forceinline__ uint4 pack_bf16x8(float4 a, float4 b) {
    const bf16x8 t = {(bf16_t)a.x, (bf16_t)a.y, (bf16_t)a.z, (bf16_t)a.w, (bf16_t)b.x, (bf16_t)b.y, (bf16_t)b.z, (bf16_t)b.w};
    return __builtin_bit_cast(uint4, t);
}

// Register stage of one operand tile: raw loads, converted only when written to LDS (so the loads stay in flight).
template <typename E, int NV> struct Stage16;
template <int NV> struct Stage16<bf16_t, NV> { uint4 v[NV]; };
template <int NV> struct Stage16<float, NV> { float4 lo[NV], hi[NV]; };

template <int BR, bool KC, int BK16>
struct Tile16 {
    static constexpr int RS = KC ? BK16 + 8 : BR + 32;                   // row stride of the LDS image, elements
    static constexpr int ELEMS = KC ? BR * RS : BK16 * RS;
    static constexpr int SLOTS = BR * BK16 / 8;                          // 16-byte (8-element) slots per tile
    static constexpr int NV = (SLOTS + GEMM_THREADS - 1) / GEMM_THREADS;
    static constexpr int PER_ROW = KC ? BK16 / 8 : BR / 8;               // slots per memory row

    template <bool GUARD, typename E>
    __device__ static __forceinline__ void gload(Stage16<E, NV>& st, const E* __restrict__ P, int ld,
                                                 int64_t r0, int64_t R, int64_t k0, int64_t kend, int tid) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int idx = tid + GEMM_THREADS * i;
            const bool live = (SLOTS % GEMM_THREADS == 0) || idx < SLOTS;
            const int major = idx / PER_ROW, minor = (idx % PER_ROW) << 3;
            int64_t grow = KC ? r0 + major : k0 + major;
            int64_t gcol = KC ? k0 + minor : r0 + minor;
            bool ok = live;
            if constexpr (GUARD) {
                const int64_t rlim = KC ? R : kend, clim = KC ? kend : R;     // clim is a multiple of 8 (checked on the host)
                ok = live && grow < rlim && gcol < clim;
                grow = grow < rlim ? grow : rlim - 1;
                gcol = gcol < clim ? gcol : clim - 8;
            } else if (!live) { grow = KC ? r0 : k0; gcol = KC ? k0 : r0; }
            const E* src = P + grow * ld + gcol;
            if constexpr (std::is_same<E, float>::value) {
                const float4 a = ld4(src), b = ld4(src + 4);
                st.lo[i] = ok ? a : f4_zero();
                st.hi[i] = ok ? b : f4_zero();
            } else {
                const uint4 v = *reinterpret_cast<const uint4*>(src);
                st.v[i] = ok ? v : make_uint4(0u, 0u, 0u, 0u);
            }
        }
    }
    template <typename E>
    __device__ static __forceinline__ void sstore(const Stage16<E, NV>& st, bf16_t* S, int tid) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int idx = tid + GEMM_THREADS * i;
            if (SLOTS % GEMM_THREADS != 0 && idx >= SLOTS) continue;
            uint4 v;
            if constexpr (std::is_same<E, float>::value) v = pack_bf16x8(st.lo[i], st.hi[i]);
            else v = st.v[i];
            *reinterpret_cast<uint4*>(S + (idx / PER_ROW) * RS + ((idx % PER_ROW) << 3)) = v;
        }
    }
    // MFMA operand of the 32-row sub-tile starting at tile row rb for k16-step s: lane (l31, h) gets k = 16s + 8h + 0..7
    __device__ static __forceinline__ bf16x8 frag(const bf16_t* S, int rb, int s, int lane) {
        if constexpr (KC) {
            return *reinterpret_cast<const bf16x8*>(S + (rb + (lane & 31)) * RS + 16 * s + 8 * (lane >> 5));
        } else {
            // group g = lane>>4 covers rows rb + 16(g&1) .. +15 and k = 16s + 8(g>>1) .. +7; lane 4q+p of the group supplies
            // the address of k-row q, rows 4p..4p+3 and receives the 4 k-values of row (lane & 15)
            const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
            const bf16_t* a = S + (16 * s + 8 * (g >> 1) + q) * RS + rb + 16 * (g & 1) + 4 * p;
            const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a));
            const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a + 4 * RS));
            typedef short s16x8 __attribute__((ext_vector_type(8)));
            const s16x8 t = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            return __builtin_bit_cast(bf16x8, t);
        }
    }
    // column sums of the tile this thread staged (weight gradient: bias gradient), 8 rows per thread
    template <typename E>
    __device__ static __forceinline__ void colsum_add(float (&acc)[8], const Stage16<E, NV>& st) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            if constexpr (std::is_same<E, float>::value) {
                acc[0] += st.lo[i].x; acc[1] += st.lo[i].y; acc[2] += st.lo[i].z; acc[3] += st.lo[i].w;
                acc[4] += st.hi[i].x; acc[5] += st.hi[i].y; acc[6] += st.hi[i].z; acc[7] += st.hi[i].w;
            } else {
                const unsigned w[4] = {st.v[i].x, st.v[i].y, st.v[i].z, st.v[i].w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc[2 * j] += __uint_as_float(w[j] << 16);
                    acc[2 * j + 1] += __uint_as_float(w[j] & 0xffff0000u);
                }
            }
        }
    }
};

// ---- The block frame of the GEMM kernels on these tiles (gemm16_body in gemm_bf16.hip, gemm_split_kernel in gemm_split.hip):
// everything around the main loop, stated once.  A kernel body places its block, starts its accumulators, runs ITS main loop
// (how a tile reaches LDS, the k-step and the schedule are what the two files differ in), then emits and, for a weight
// gradient, reduces the bias-gradient column sums.  (gemm.hip's general path has the same shape; it keeps its own copy
// because its fast path's register allocation depends on what is defined beside it.)

// 4 waves: 128x128 as 2 x 2 waves of 64x64, 128x32 as 4 x 1, 32x128 as 1 x 4 waves of 32x32; TM x TN MFMA tiles per wave
template <int BM, int BN>
struct Waves16 {
    static constexpr int WM = (BM == 128 && BN == 128) ? 2 : (BM == 128 ? 4 : 1);
    static constexpr int WN = 4 / WM;
    static constexpr int TM = BM / (32 * WM), TN = BN / (32 * WN);
};

// where block bid of nwg works: K split, N tile number, first row / column of its tile, its contraction range
struct Place16 {
    int split, tn;
    int64_t m0;
    int n0;
    int64_t kbeg, kend;
    bool full;               // the tile lies inside C: no row / column guards
};
template <int BM, int BN>
__device__ __forceinline__ Place16 gemm16_place(const GemmArgs& g, int bid, int nwg) {
    const int swz = xcd_swizzle(bid, nwg);
    const int ntile = g.tiles_m * g.tiles_n;
    Place16 p;
    p.split = swz / ntile;
    const int tile = swz - p.split * ntile;
    const int tm = tile / g.tiles_n;
    p.tn = tile - tm * g.tiles_n;
    p.m0 = (int64_t)tm * BM;
    p.n0 = p.tn * BN;
    p.kbeg = (int64_t)p.split * g.kc_per_split;
    p.kend = p.kbeg + g.kc_per_split;
    if (p.kend > g.Kc) p.kend = g.Kc;
    p.full = (p.m0 + BM <= g.M) && (p.n0 + BN <= g.N);
    return p;
}

// zero accumulators; the bias of the lane's column of each of its TN tiles (col0 = the lane's column in the first: clamped, so
// a lane past N reads something valid that the epilogue never stores)
template <int EPI, int TM, int TN>
__device__ __forceinline__ void gemm16_start(f32x16 (&acc)[TM][TN], float (&bv)[TN], const GemmArgs& g, int col0) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        bv[j] = 0.f;
        if constexpr ((EPI & VLG_EPI_BIAS) != 0) {
            const int col = col0 + j * 32;
            bv[j] = g.bias[col < g.N ? col : g.N - 1];
        }
    }
}

// The general epilogue, all five VLG_EPI_* bits (C/D layout of the 32x32 MFMA: col = lane&31, row = (r&3) + 8*(r>>2) + 4*h).
// (row0, col0) = the lane's first element in C; EO = element type of C and of the auxiliary operands.
template <bool GUARD, int EPI, typename EO, int TM, int TN>
__device__ __forceinline__ void gemm16_emit(const GemmArgs& g, const f32x16 (&acc)[TM][TN], const float (&bv)[TN], EO* Cs,
                                            int64_t row0, int col0) {
    const EO* const gAuxIn = static_cast<const EO*>(g.aux_in);
    EO* const gAuxOut = static_cast<EO*>(g.aux_out);
    const int64_t base = row0 * g.ldc + col0;
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
                float v = acc[i][j][r] + bv[j];
                if constexpr ((EPI & VLG_EPI_GELU) != 0) {
                    if constexpr ((EPI & VLG_EPI_GELU_GRAD) != 0) {      // aux_out = gelu'(pre) (common.h, gelu_parts): the backward
                        float c, pd;                                     // pass then multiplies (VLG_EPI_MUL) instead of recomputing
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
}

// Bias gradient of a weight-gradient block (A = dY, contraction-major): every thread summed the 8 rows 8*(tid % PER_ROW) .. +7
// of the tiles it staged (csum); combine the threads that share a row group through LDS (red = the tiles, which are dead: the
// main loop ended on a barrier) and write the BM sums behind the block's slab
template <typename TA, int BM, typename EO>
__device__ __forceinline__ void gemm16_colsum_store(const GemmArgs& g, const float (&csum)[8], float* red, EO* Cs, int64_t m0, int tid) {
    constexpr int PR = TA::PER_ROW;
    if ((TA::SLOTS % GEMM_THREADS == 0) || tid < TA::SLOTS) {
#pragma unroll
        for (int j = 0; j < 8; ++j) red[(tid / PR) * BM + 8 * (tid % PR) + j] = csum[j];
    }
    __syncthreads();
    constexpr int NTL = (TA::SLOTS < GEMM_THREADS ? TA::SLOTS : GEMM_THREADS) / PR;     // threads per row group
    if (tid < BM && m0 + tid < g.M) {
        float s = 0.f;
#pragma unroll 4
        for (int t = 0; t < NTL; ++t) s += red[t * BM + tid];
        st1(Cs + g.colsum_off + m0 + tid, s);
    }
}

