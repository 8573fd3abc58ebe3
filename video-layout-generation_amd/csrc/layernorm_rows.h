// Row layout of the layer-norm kernels, shared by layernorm.hip and dropout.hip: one 64-lane wavefront per token row,
// the row in registers (d/64 floats per lane, float4 loads when d % 256 == 0), plus the stateless dropout mask the fused
// kernels of dropout.hip apply to such a row.
#pragma once
#include "common.h"
#include "philox.h"

#define LN_BLOCK 256
#define LN_WAVES (LN_BLOCK / 64)
#define LN_BWD_MAX_BLOCKS 512

// E = floats per lane; V4 => lane holds E/4 float4 at columns 4*lane + 256*i, else scalars at lane + 64*i
template <int E, bool V4>
struct RowIO {
    template <typename EL>
    __device__ static __forceinline__ void load(const EL* __restrict__ row, int lane, float (&v)[E]) {
        if constexpr (V4) {
#pragma unroll
            for (int i = 0; i < E / 4; ++i) {
                const float4 t = ld4(row + 4 * lane + 256 * i);
                v[4 * i] = t.x; v[4 * i + 1] = t.y; v[4 * i + 2] = t.z; v[4 * i + 3] = t.w;
            }
        } else {
#pragma unroll
            for (int i = 0; i < E; ++i) v[i] = ld1(row + lane + 64 * i);
        }
    }
    template <typename EL>
    __device__ static __forceinline__ void store(EL* __restrict__ row, int lane, const float (&v)[E]) {
        if constexpr (V4) {
#pragma unroll
            for (int i = 0; i < E / 4; ++i)
                st4(row + 4 * lane + 256 * i, make_float4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]));
        } else {
#pragma unroll
            for (int i = 0; i < E; ++i) st1(row + lane + 64 * i, v[i]);
        }
    }
    // column index of register j
    __device__ static __forceinline__ int col(int lane, int j) {
        if constexpr (V4) return 4 * lane + 256 * (j >> 2) + (j & 3);
        else return lane + 64 * j;
    }
};

// rows a wave holds in flight per loop trip: one 1-KB row per wave leaves too few bytes in flight to cover the HBM latency
// (8 192 resident waves x 1 KB = 8 MB against ~16 MB for 8 TB/s x 2 us), so short rows are processed LN_ROWS(E) at a time
#define LN_ROWS(E) ((E) <= 4 ? 4 : (E) <= 8 ? 2 : 1)

static inline int ln_fwd_blocks(int64_t rows) {
    int64_t b = (rows + LN_WAVES - 1) / LN_WAVES;
    return (int)(b > 2048 ? 2048 : (b < 1 ? 1 : b));
}
static inline int ln_bwd_blocks(int64_t rows) {
    int64_t b = (rows + LN_WAVES - 1) / LN_WAVES;
    return (int)(b > LN_BWD_MAX_BLOCKS ? LN_BWD_MAX_BLOCKS : (b < 1 ? 1 : b));
}

#define LN_DISPATCH(d, CALL)                                 \
    switch (d) {                                             \
        case 64:   { CALL(1, false) } break;                 \
        case 128:  { CALL(2, false) } break;                 \
        case 192:  { CALL(3, false) } break;                 \
        case 256:  { CALL(4, true) } break;                  \
        case 512:  { CALL(8, true) } break;                  \
        case 768:  { CALL(12, true) } break;                 \
        case 1024: { CALL(16, true) } break;                 \
        default: return VLG_ERR_SHAPE;                       \
    }
static inline bool ln_supports(int d) { return d == 64 || d == 128 || d == 192 || d == 256 || d == 512 || d == 768 || d == 1024; }

// ------------------------------------------------------------------------------------------------------ dropout mask
// Stateless mask (include/vlg_hip.h, "dropout"): element (row m, column c) of site s at step k is KEPT iff word c % 4 of
// Philox4x32-10 (philox.h), counter (m, c / 4, s, k), key (seed lo, seed hi), is >= thr.  One call serves one float4; a bit
// depends on (m, c, s, k, seed) alone, never on the launch geometry.  The third counter word is the SITE here, not a stream
// of vlg_rng_stream: the mask is kept apart from those draws by its own seed.
struct LnDrop {
    float* out;             // bwd only: dy_drop
    const int* step;        // k, read by the kernel when it runs (a captured graph advances it by replaying)
    uint32_t thr, k0, k1, site;
    float scale;
};

// keep[j] of the registers RowIO<E, V4> holds of row `row`.  V4: one Philox call per float4.  Scalar layout (d < 256): a
// lane's columns lane + 64*j lie in different float4s, so it pays one call per element and takes word c % 4 of it.
template <int E, bool V4>
__device__ __forceinline__ void drop_keep(const LnDrop& dp, uint32_t k, int64_t row, int lane, bool (&keep)[E]) {
    uint32_t x[4];
    if constexpr (V4) {
#pragma unroll
        for (int i = 0; i < E / 4; ++i) {
            philox4x32_10((uint32_t)row, (uint32_t)(lane + 64 * i), dp.site, k, dp.k0, dp.k1, x);
#pragma unroll
            for (int w = 0; w < 4; ++w) keep[4 * i + w] = x[w] >= dp.thr;
        }
    } else {
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const int c = lane + 64 * j;
            philox4x32_10((uint32_t)row, (uint32_t)(c >> 2), dp.site, k, dp.k0, dp.k1, x);
            const int w = c & 3;
            const uint32_t xw = w == 0 ? x[0] : w == 1 ? x[1] : w == 2 ? x[2] : x[3];
            keep[j] = xw >= dp.thr;
        }
    }
}

// The backward kernel lives in layernorm.hip and serves both vlg_layernorm_bwd (dp.out == nullptr) and the fused dropout
// backward of dropout.hip (dp.out = dy_drop): this launches it, arguments already checked.  VLG_ERR_SHAPE for a d outside
// LN_DISPATCH's set, before anything is enqueued.
int ln_bwd_launch(const void* dy, bool dy_bf16, const float* x, const float* mean, const float* rstd, const float* gamma,
                  const float* dres, float* dx_out, float* slabs, int64_t slab_stride, int64_t rows, int d, const LnDrop& dp,
                  hipStream_t s);
