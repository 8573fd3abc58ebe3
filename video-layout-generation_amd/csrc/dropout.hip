// Dropout fused into the layer-norm launches of the layout-token step (include/vlg_hip.h, "dropout").
//
//   fwd: x_out = (resid ? resid : 0) + select(y),  h = LN(x_out)      one launch where the step had its layer-norm forward
//   bwd: vlg_layernorm_bwd + a second output dy_drop = select(dx_out) for the site that FED this layer-norm - the SAME
//        kernel (ln_bwd_kernel, layernorm.hip) with its dropout branch taken; this file holds its host side
//
// Same row layout as layernorm.hip (layernorm_rows.h): one wavefront per row, the row in registers, LN_ROWS(E) rows in
// flight per trip, and the arithmetic of ln_fwd_kernel statement for statement.  The mask is stateless
// (Philox4x32-10 of (row, float4 index, site, step) under the seed): nothing is stored for backward, and the step
// counter is READ from device memory, so a captured graph draws a new mask at every replay.
//
// Roofline: still HBM-bound.  fwd algorithmic bytes 16*d per row (y, resid in; x_out, h out: 12*d without resid, 14*d /
// 10*d with bf16 h) against layer-norm's 8*d; bwd 20*d per row against 16*d.  Per float4 there is one Philox call: 10
// rounds x 4 = 40 quarter-rate 32-bit multiplies, 16 issue cycles each for a 64-lane wave = ~640 cycles per KB of row; over
// 1024 SIMDs at 2.4 GHz that is ~0.26 ns of chip time per row-KB against 0.5 ns of HBM time for the 4 KB the forward
// moves per row-KB at 8 TB/s (0.7-0.9 ns at the 0.55-0.73 of HBM these row kernels reach): a fraction of the memory
// time, issued while the other rows' loads are in flight.  (d < 256 uses the scalar row layout, where a lane's elements
// lie in different float4s: one call per ELEMENT, 4x the multiplies.)
// Measured alone and cold at 32768 x 256 (tools/ab/dropout_ab.py): fwd 39.2 us for 134 MB = 0.43 of 8 TB/s where
// vlg_layernorm_fwd moves its 67 MB at 0.37; bwd 46.6 us for 168 MB = 0.45 against vlg_layernorm_bwd's 0.42: the mask
// does not lower the rate these row kernels reach.
#include "layernorm_rows.h"

// x_out may be y itself: every load of a row group precedes its stores and a group belongs to one wave, so neither
// pointer carries __restrict__.  A SELECT, not a product: whatever a dropped y holds (inf, NaN) does not reach x_out.
template <int E, bool V4, typename EY = float>
__global__ __launch_bounds__(LN_BLOCK) void dropout_add_ln_fwd_kernel(
    const float* y, const float* __restrict__ resid, const float* __restrict__ gamma, const float* __restrict__ beta,
    float* x_out, EY* __restrict__ h, float* __restrict__ mean, float* __restrict__ rstd, int64_t rows, float eps,
    const LnDrop dp) {
    constexpr int d = E * 64, R = LN_ROWS(E);
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * LN_WAVES + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * LN_WAVES;
    float g[E], b[E];
    RowIO<E, V4>::load(gamma, lane, g);
    RowIO<E, V4>::load(beta, lane, b);
    const uint32_t k = (uint32_t)*dp.step;
    for (int64_t r0 = wave * R; r0 < rows; r0 += nwaves * R) {
        float v[R][E], rr[R][E];
#pragma unroll
        for (int i = 0; i < R; ++i) {                          // a short last group re-reads the last row, stores are guarded
            const int64_t r = r0 + i < rows ? r0 + i : rows - 1;
            RowIO<E, V4>::load(y + r * d, lane, v[i]);
            if (resid != nullptr) RowIO<E, V4>::load(resid + r * d, lane, rr[i]);
            else {
#pragma unroll
                for (int j = 0; j < E; ++j) rr[i][j] = 0.f;
            }
        }
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const int64_t r = r0 + i < rows ? r0 + i : rows - 1;
            bool keep[E];
            drop_keep<E, V4>(dp, k, r, lane, keep);
#pragma unroll
            for (int j = 0; j < E; ++j) v[i][j] = rr[i][j] + (keep[j] ? v[i][j] * dp.scale : 0.f);
            if (r0 + i < rows) RowIO<E, V4>::store(x_out + (r0 + i) * d, lane, v[i]);
        }
#pragma unroll
        for (int i = 0; i < R; ++i) {                          // ln_fwd_kernel's arithmetic on the row just formed
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < E; ++j) s += v[i][j];
            const float mu = wave_sum(s) * (1.0f / d);
            float q = 0.f;
#pragma unroll
            for (int j = 0; j < E; ++j) { const float t = v[i][j] - mu; q += t * t; }
            const float rs = 1.0f / sqrtf(wave_sum(q) * (1.0f / d) + eps);
#pragma unroll
            for (int j = 0; j < E; ++j) v[i][j] = (v[i][j] - mu) * rs * g[j] + b[j];
            if (r0 + i < rows) {
                RowIO<E, V4>::store(h + (r0 + i) * d, lane, v[i]);
                if (lane == 0) { mean[r0 + i] = mu; rstd[r0 + i] = rs; }
            }
        }
    }
}

__global__ void dropout_step_advance_kernel(int* step) { *step += 1; }

// --------------------------------------------------------------------------------------------------------------- host
extern "C" int vlg_dropout_plan(double p, uint32_t* thr_host, float* scale_host) {
    if (!(p >= 0.0 && p < 1.0) || thr_host == nullptr || scale_host == nullptr) return VLG_ERR_SHAPE;
    const double two32 = 4294967296.0;
    double t = __builtin_floor(p * two32 + 0.5);
    if (t > two32 - 1.0) t = two32 - 1.0;
    *thr_host = (uint32_t)t;
    *scale_host = (float)(1.0 / (1.0 - t / two32));
    return 0;
}

static inline bool mask_ok(int64_t rows, int d, float scale, int site, const int* step) {
    return rows >= 1 && rows < ((int64_t)1 << 32) && ln_supports(d) && scale >= 1.0f && scale <= 4294967296.0f && site >= 0 &&
           step != nullptr;
}
static inline LnDrop make_drop(float* out, uint32_t thr, float scale, uint64_t seed, int site, const int* step) {
    const PhiloxKey key = philox_key(seed);
    return LnDrop{out, step, thr, key.k0, key.k1, (uint32_t)site, scale};
}

template <typename EY>
static int dropout_add_ln_fwd(const float* y, const float* resid, const float* gamma, const float* beta, float* x_out, EY* h,
                              float* mean, float* rstd, int64_t rows, int d, float eps, uint32_t thr, float scale,
                              uint64_t seed, int site, const int* step, hipStream_t s) {
    if (!mask_ok(rows, d, scale, site, step)) return VLG_ERR_SHAPE;
    if (!y || !gamma || !beta || !x_out || !h || !mean || !rstd) return VLG_ERR_ALIGN;
    if (!vlg_aligned16(y) || !vlg_aligned16(x_out) || !vlg_aligned16(gamma) || !vlg_aligned16(beta) ||
        !(sizeof(EY) == 4 ? vlg_aligned16(h) : vlg_aligned8(h)) || (resid && !vlg_aligned16(resid)) || !vlg_aligned4(mean) ||
        !vlg_aligned4(rstd) || !vlg_aligned4(step)) return VLG_ERR_ALIGN;
    const int64_t nb = rows * d * 4, nh = rows * d * (int64_t)sizeof(EY);
    if ((x_out != y && vlg_overlap(x_out, nb, y, nb)) || vlg_overlap(h, nh, y, nb) || vlg_overlap(h, nh, x_out, nb) ||
        vlg_overlap(resid, nb, x_out, nb) || vlg_overlap(resid, nb, y, nb) || vlg_overlap(resid, nb, h, nh))
        return VLG_ERR_SHAPE;                                      // (a NULL resid or dres overlaps nothing)
    const dim3 grid(ln_fwd_blocks(rows)), block(LN_BLOCK);
    const LnDrop dp = make_drop(nullptr, thr, scale, seed, site, step);
#define CALL(E, V4) hipLaunchKernelGGL((dropout_add_ln_fwd_kernel<E, V4, EY>), grid, block, 0, s, y, resid, gamma, beta, x_out, h, mean, rstd, rows, eps, dp);
    LN_DISPATCH(d, CALL)
#undef CALL
    return vlg_last_error();
}

extern "C" int vlg_dropout_add_layernorm_fwd(const float* y, const float* resid, const float* gamma, const float* beta,
                                             float* x_out, float* h, float* mean, float* rstd, int64_t rows, int d, float eps,
                                             uint32_t thr, float scale, uint64_t seed, int site, const int* step, void* stream) {
    return dropout_add_ln_fwd<float>(y, resid, gamma, beta, x_out, h, mean, rstd, rows, d, eps, thr, scale, seed, site, step,
                                     (hipStream_t)stream);
}

extern "C" int vlg_dropout_add_layernorm_fwd_bf16(const float* y, const float* resid, const float* gamma, const float* beta,
                                                  float* x_out, vlg_bf16* h, float* mean, float* rstd, int64_t rows, int d,
                                                  float eps, uint32_t thr, float scale, uint64_t seed, int site,
                                                  const int* step, void* stream) {
    return dropout_add_ln_fwd<bf16_t>(y, resid, gamma, beta, x_out, reinterpret_cast<bf16_t*>(h), mean, rstd, rows, d, eps, thr,
                                      scale, seed, site, step, (hipStream_t)stream);
}

template <typename EY>
static int ln_bwd_dropout(const EY* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                          const float* dres, float* dx_out, float* dy_drop, float* slabs, int64_t slab_stride,
                          int64_t slab_capacity, int64_t rows, int d, uint32_t thr, float scale, uint64_t seed, int site,
                          const int* step, hipStream_t s) {
    if (!mask_ok(rows, d, scale, site, step) || slab_stride < 2 * (int64_t)d) return VLG_ERR_SHAPE;
    if (slab_capacity < (int64_t)ln_bwd_blocks(rows) * slab_stride) return VLG_ERR_SHAPE;   // every block writes one slab
    if (!dy || !x || !mean || !rstd || !gamma || !dx_out || !dy_drop || !slabs) return VLG_ERR_ALIGN;
    if (!(sizeof(EY) == 4 ? vlg_aligned16(dy) : vlg_aligned8(dy)) || !vlg_aligned16(x) || !vlg_aligned16(gamma) ||
        !vlg_aligned16(dx_out) || !vlg_aligned16(dy_drop) || (dres && !vlg_aligned16(dres)) || !vlg_aligned4(mean) ||
        !vlg_aligned4(rstd) || !vlg_aligned4(slabs) || !vlg_aligned4(step)) return VLG_ERR_ALIGN;
    const int64_t nb = rows * d * 4, ny = rows * d * (int64_t)sizeof(EY);
    if (vlg_overlap(dy_drop, nb, dx_out, nb) || vlg_overlap(dy_drop, nb, dy, ny) || vlg_overlap(dy_drop, nb, x, nb) ||
        vlg_overlap(dy_drop, nb, dres, nb) || vlg_overlap(dx_out, nb, dy, ny) || vlg_overlap(dx_out, nb, x, nb) ||
        (dres != dx_out && vlg_overlap(dres, nb, dx_out, nb))) return VLG_ERR_SHAPE;
    return ln_bwd_launch(dy, sizeof(EY) == 2, x, mean, rstd, gamma, dres, dx_out, slabs, slab_stride, rows, d,
                         make_drop(dy_drop, thr, scale, seed, site, step), s);      // the one backward kernel (layernorm.hip)
}

extern "C" int vlg_layernorm_bwd_dropout(const float* dy, const float* x, const float* mean, const float* rstd,
                                         const float* gamma, const float* dres, float* dx_out, float* dy_drop, float* slabs,
                                         int64_t slab_stride, int64_t slab_capacity, int64_t rows, int d, uint32_t thr,
                                         float scale, uint64_t seed, int site, const int* step, void* stream) {
    return ln_bwd_dropout<float>(dy, x, mean, rstd, gamma, dres, dx_out, dy_drop, slabs, slab_stride, slab_capacity, rows, d, thr,
                                 scale, seed, site, step, (hipStream_t)stream);
}

extern "C" int vlg_layernorm_bwd_dropout_bf16(const vlg_bf16* dy, const float* x, const float* mean, const float* rstd,
                                              const float* gamma, const float* dres, float* dx_out, float* dy_drop,
                                              float* slabs, int64_t slab_stride, int64_t slab_capacity, int64_t rows, int d,
                                              uint32_t thr, float scale, uint64_t seed, int site, const int* step,
                                              void* stream) {
    return ln_bwd_dropout<bf16_t>(reinterpret_cast<const bf16_t*>(dy), x, mean, rstd, gamma, dres, dx_out, dy_drop, slabs,
                                  slab_stride, slab_capacity, rows, d, thr, scale, seed, site, step, (hipStream_t)stream);
}

extern "C" int vlg_dropout_step_advance(int* step, void* stream) {
    if (step == nullptr || !vlg_aligned4(step)) return VLG_ERR_ALIGN;
    hipLaunchKernelGGL(dropout_step_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, step);
    return vlg_last_error();
}
