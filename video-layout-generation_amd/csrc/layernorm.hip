// Layer-norm forward / backward, one 64-lane wavefront per token row (HBM-bound).
//
// A row of d floats lives in registers (d/64 per lane, float4 loads when d % 256 == 0),
// mean/variance/gradient sums are wavefront-shuffle reductions - no LDS in the row path.
// fwd algorithmic bytes: 8*d per row (+8 for the saved mean / rstd).
// bwd algorithmic bytes: 16*d per row (dy, x, dres in; dx out); per-channel dgamma/dbeta
// sums stay in registers across the grid-stride loop, are combined across the block's 4
// waves through LDS and leave as one [dgamma | dbeta] slab per block (reduced by
// vlg_reduce_slabs: reproducible, no atomics).
// The backward kernel also serves the fused dropout backward of dropout.hip: with dp.out set it writes a second output,
// select(dx_out), behind a wave-uniform branch.  ONE kernel for both, so that vlg_layernorm_bwd_dropout's dx_out and
// slabs are vlg_layernorm_bwd's bit for bit by construction: two kernels compiled from the same statements are not (the
// compiler contracts a - s1 with the 1/d product or not depending on the code around it).
#include "layernorm_rows.h"      // RowIO, LN_ROWS, the block counts and LN_DISPATCH (shared with dropout.hip)

template <int E, bool V4, typename EY = float>
__global__ __launch_bounds__(LN_BLOCK) void ln_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
    EY* __restrict__ y, float* __restrict__ mean, float* __restrict__ rstd, int64_t rows, float eps) {
    constexpr int d = E * 64, R = LN_ROWS(E);
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * LN_WAVES + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * LN_WAVES;
    float g[E], b[E];
    RowIO<E, V4>::load(gamma, lane, g);
    RowIO<E, V4>::load(beta, lane, b);
    for (int64_t r0 = wave * R; r0 < rows; r0 += nwaves * R) {
        float v[R][E];
#pragma unroll
        for (int i = 0; i < R; ++i) {                          // a short last group re-reads the last row, stores are guarded
            const int64_t r = r0 + i < rows ? r0 + i : rows - 1;
            RowIO<E, V4>::load(x + r * d, lane, v[i]);
        }
#pragma unroll
        for (int i = 0; i < R; ++i) {
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
                RowIO<E, V4>::store(y + (r0 + i) * d, lane, v[i]);
                if (lane == 0) { mean[r0 + i] = mu; rstd[r0 + i] = rs; }
            }
        }
    }
}

template <int E, bool V4, typename EY = float>
__global__ __launch_bounds__(LN_BLOCK) void ln_bwd_kernel(
    const EY* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ mean,
    const float* __restrict__ rstd, const float* __restrict__ gamma, const float* __restrict__ dres,
    float* __restrict__ dx_out, float* __restrict__ slabs, int64_t slab_stride, int64_t rows, const LnDrop dp) {
    constexpr int d = E * 64, R = LN_ROWS(E);
    __shared__ float red[LN_WAVES][2 * d];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t wave = (int64_t)blockIdx.x * LN_WAVES + w;
    const int64_t nwaves = (int64_t)gridDim.x * LN_WAVES;
    float g[E], dg[E], db[E];
    RowIO<E, V4>::load(gamma, lane, g);
#pragma unroll
    for (int j = 0; j < E; ++j) { dg[j] = 0.f; db[j] = 0.f; }
    for (int64_t r0 = wave * R; r0 < rows; r0 += nwaves * R) {
        float gy[R][E], xv[R][E], o[R][E], mu[R], rs[R];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const int64_t r = r0 + i < rows ? r0 + i : rows - 1;
            RowIO<E, V4>::load(dy + r * d, lane, gy[i]);
            RowIO<E, V4>::load(x + r * d, lane, xv[i]);
            if (dres != nullptr) RowIO<E, V4>::load(dres + r * d, lane, o[i]);
            else {
#pragma unroll
                for (int j = 0; j < E; ++j) o[i][j] = 0.f;
            }
            mu[i] = mean[r];
            rs[i] = rstd[r];
        }
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const float live = r0 + i < rows ? 1.f : 0.f;      // rows past the end add nothing to dgamma / dbeta
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const float xh = (xv[i][j] - mu[i]) * rs[i];
                const float gl = gy[i][j] * live;
                const float a = gy[i][j] * g[j];
                dg[j] += gl * xh;
                db[j] += gl;
                s1 += a;
                s2 += a * xh;
                xv[i][j] = xh;
                gy[i][j] = a;
            }
            s1 = wave_sum(s1) * (1.0f / d);
            s2 = wave_sum(s2) * (1.0f / d);
#pragma unroll
            for (int j = 0; j < E; ++j) o[i][j] += rs[i] * (gy[i][j] - s1 - xv[i][j] * s2);
            if (r0 + i < rows) {
                RowIO<E, V4>::store(dx_out + (r0 + i) * d, lane, o[i]);
                if (dp.out != nullptr) {       // fused dropout (dropout.hip): kept ? dx_out * scale : 0 under the feeding site's mask
                    bool keep[E];
                    drop_keep<E, V4>(dp, (uint32_t)*dp.step, r0 + i, lane, keep);
#pragma unroll
                    for (int j = 0; j < E; ++j) o[i][j] = keep[j] ? o[i][j] * dp.scale : 0.f;
                    RowIO<E, V4>::store(dp.out + (r0 + i) * d, lane, o[i]);
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const int c = RowIO<E, V4>::col(lane, j);
        red[w][c] = dg[j];
        red[w][d + c] = db[j];
    }
    __syncthreads();
    float* slab = slabs + (int64_t)blockIdx.x * slab_stride;
    for (int c = threadIdx.x; c < 2 * d; c += LN_BLOCK) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < LN_WAVES; ++k) s += red[k][c];
        slab[c] = s;
    }
}

extern "C" int vlg_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y,
                                 float* mean, float* rstd, int64_t rows, int d, float eps, void* stream) {
    if (rows < 1) return VLG_ERR_SHAPE;
    if (!vlg_aligned16(x) || !vlg_aligned16(y) || !vlg_aligned16(gamma) || !vlg_aligned16(beta)) return VLG_ERR_ALIGN;
    const dim3 grid(ln_fwd_blocks(rows)), block(LN_BLOCK);
    hipStream_t s = (hipStream_t)stream;
#define CALL(E, V4) hipLaunchKernelGGL((ln_fwd_kernel<E, V4>), grid, block, 0, s, x, gamma, beta, y, mean, rstd, rows, eps);
    LN_DISPATCH(d, CALL)
#undef CALL
    return vlg_last_error();
}

extern "C" int vlg_layernorm_bwd_slabs(int64_t rows) { return ln_bwd_blocks(rows); }

// launch of the one backward kernel, arguments already checked (declared in layernorm_rows.h; dropout.hip calls it with dp.out set)
int ln_bwd_launch(const void* dy, bool dy_bf16, const float* x, const float* mean, const float* rstd, const float* gamma,
                  const float* dres, float* dx_out, float* slabs, int64_t slab_stride, int64_t rows, int d, const LnDrop& dp,
                  hipStream_t s) {
    const dim3 grid(ln_bwd_blocks(rows)), block(LN_BLOCK);
    if (dy_bf16) {
        const bf16_t* dyb = static_cast<const bf16_t*>(dy);
#define CALL(E, V4) hipLaunchKernelGGL((ln_bwd_kernel<E, V4, bf16_t>), grid, block, 0, s, dyb, x, mean, rstd, gamma, dres, dx_out, slabs, slab_stride, rows, dp);
        LN_DISPATCH(d, CALL)
#undef CALL
    } else {
        const float* dyf = static_cast<const float*>(dy);
#define CALL(E, V4) hipLaunchKernelGGL((ln_bwd_kernel<E, V4>), grid, block, 0, s, dyf, x, mean, rstd, gamma, dres, dx_out, slabs, slab_stride, rows, dp);
        LN_DISPATCH(d, CALL)
#undef CALL
    }
    return vlg_last_error();
}

extern "C" int vlg_layernorm_bwd(const float* dy, const float* x, const float* mean, const float* rstd,
                                 const float* gamma, const float* dres, float* dx_out, float* slabs,
                                 int64_t slab_stride, int64_t slab_capacity, int64_t rows, int d, void* stream) {
    if (rows < 1 || slab_stride < 2 * (int64_t)d) return VLG_ERR_SHAPE;
    if (slab_capacity < (int64_t)ln_bwd_blocks(rows) * slab_stride) return VLG_ERR_SHAPE;   // every block writes one slab
    if (!vlg_aligned16(dy) || !vlg_aligned16(x) || !vlg_aligned16(gamma) || !vlg_aligned16(dx_out) ||
        (dres && !vlg_aligned16(dres))) return VLG_ERR_ALIGN;
    return ln_bwd_launch(dy, false, x, mean, rstd, gamma, dres, dx_out, slabs, slab_stride, rows, d, LnDrop{}, (hipStream_t)stream);
}

extern "C" int vlg_layernorm_fwd_bf16(const float* x, const float* gamma, const float* beta, vlg_bf16* y,
                                      float* mean, float* rstd, int64_t rows, int d, float eps, void* stream) {
    if (rows < 1) return VLG_ERR_SHAPE;
    if (!vlg_aligned16(x) || !vlg_aligned8(y) || !vlg_aligned16(gamma) || !vlg_aligned16(beta)) return VLG_ERR_ALIGN;
    const dim3 grid(ln_fwd_blocks(rows)), block(LN_BLOCK);
    hipStream_t s = (hipStream_t)stream;
    bf16_t* yb = reinterpret_cast<bf16_t*>(y);
#define CALL(E, V4) hipLaunchKernelGGL((ln_fwd_kernel<E, V4, bf16_t>), grid, block, 0, s, x, gamma, beta, yb, mean, rstd, rows, eps);
    LN_DISPATCH(d, CALL)
#undef CALL
    return vlg_last_error();
}

extern "C" int vlg_layernorm_bwd_bf16(const vlg_bf16* dy, const float* x, const float* mean, const float* rstd,
                                      const float* gamma, const float* dres, float* dx_out, float* slabs,
                                      int64_t slab_stride, int64_t slab_capacity, int64_t rows, int d, void* stream) {
    if (rows < 1 || slab_stride < 2 * (int64_t)d) return VLG_ERR_SHAPE;
    if (slab_capacity < (int64_t)ln_bwd_blocks(rows) * slab_stride) return VLG_ERR_SHAPE;   // every block writes one slab
    if (!vlg_aligned8(dy) || !vlg_aligned16(x) || !vlg_aligned16(gamma) || !vlg_aligned16(dx_out) ||
        (dres && !vlg_aligned16(dres))) return VLG_ERR_ALIGN;
    return ln_bwd_launch(dy, true, x, mean, rstd, gamma, dres, dx_out, slabs, slab_stride, rows, d, LnDrop{}, (hipStream_t)stream);
}
