// Slab reduction and fused Adam on the flat parameter buffer (both HBM-bound, float4 streams).
//
// vlg_reduce_slabs : dst[e] = sum_s slabs[s*stride + e].  Every partial-sum producer in this
//                    library (weight gradients split over tokens, layer-norm gain/bias sums,
//                    embedding-table sums) writes slabs and leaves the final sum to this kernel,
//                    so gradients are bitwise reproducible run to run (no float atomics).
//                    Algorithmic bytes: 4*len*(n_slabs + 1).
// vlg_adam_step    : torch.optim.Adam arithmetic on ONE flat fp32 buffer holding every
//                    parameter (reference src/trainer.py:83,258 - Adam(lr, betas=(beta1,0.999)),
//                    no weight decay, no amsgrad).  One launch per step instead of one per tensor.
//                    Algorithmic bytes: 16 B read + 12 B written per parameter.
// The guarded step (global-norm clipping, skip of a non-finite gradient, learning rate in device memory) is three
// launches around one 16-float device record `ctl` (layout: include/vlg_hip.h), so it needs no host synchronisation and
// survives hipGraph replay:
// vlg_grad_sumsq   : per-block partial sums of grad[i]^2, accumulated in fp64 per lane (the kernel is HBM-bound: four
//                    fp64 FMAs per 16 bytes are far below the vector rate) and combined in a fixed order - bitwise
//                    reproducible; inf / NaN pass through.  Algorithmic bytes: 4 B read per parameter.
// vlg_optim_control: one block sums the partials in double and decides the step: norm, clip coefficient, apply flag,
//                    step counter and bias-correction factors (as adam_state_kernel computes them).
// vlg_adam_step_ctl: adam_kernel's arithmetic with {step_size, sqrt_bc2, gradient multiplier} read from ctl; when the
//                    apply flag is 0 every block returns before it touches memory.
// The training recipe on top of it (decoupled weight decay on marked float4s, linear warm-up counted in applied steps, an
// exponential moving average of the weights) is the same three launches with a second 16-float record `ext` (VLG_EXT_*):
// vlg_optim_control_ext : vlg_optim_control's decision from the same code, plus this step's effective learning rate,
//                    decay multiplier and EMA weight, written to ext.
// vlg_adamw_ema_step_ctl: vlg_adam_step_ctl plus, per float4, p *= DECAY_MULT where a byte mask marks it (before Adam's
//                    update: torch.optim.AdamW's order) and e += EMA_OMD * (p_new - e) on an fp32 average (+ its bf16
//                    copy).  Algorithmic bytes on top of the parent's: 4 B read + 4 B written (+ 2 B) per parameter with
//                    the average, 0.25 B read with the mask.
#include "common.h"
#include "reduce_body.h"
#include <math.h>

__global__ __launch_bounds__(256) void reduce_slabs_kernel(const float* __restrict__ slabs, int64_t stride,
                                                           int n_slabs, float* __restrict__ dst, int64_t len4) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < len4; e += (int64_t)gridDim.x * blockDim.x) {
        float4 acc = f4_zero();
        const float* p = slabs + e * 4;
        int s = 0;
        for (; s + 4 <= n_slabs; s += 4) {       // 4 independent loads in flight per lane
            const float4 a = ld4(p), b = ld4(p + stride), c = ld4(p + 2 * stride), d = ld4(p + 3 * stride);
            acc = f4_add(acc, f4_add(f4_add(a, b), f4_add(c, d)));
            p += 4 * stride;
        }
        for (; s < n_slabs; ++s) { acc = f4_add(acc, ld4(p)); p += stride; }
        st4(dst + e * 4, acc);
    }
}

// Many slabs, short vectors (layer-norm gain/bias: 512 slabs x 2d floats; embedding tables): the flat
// kernel above would leave one block walking hundreds of slabs serially.  Here a block owns 16 float4
// columns and its 256 threads split the slabs 16 ways, then combine through LDS in a fixed order
// (still bitwise reproducible).
__global__ __launch_bounds__(256) void reduce_slabs_tall_kernel(const float* __restrict__ slabs, int64_t stride,
                                                                int n_slabs, float* __restrict__ dst, int64_t len4) {
    __shared__ float4 part[16][16];
    const int c = threadIdx.x & 15, sg = threadIdx.x >> 4;
    const int64_t col = (int64_t)blockIdx.x * 16 + c;
    float4 acc = f4_zero();
    if (col < len4) {
        const float* p = slabs + col * 4;
        int s = sg;
        for (; s + 48 < n_slabs; s += 64) {       // 4 independent loads in flight per lane
            const float4 a = ld4(p + s * stride), b = ld4(p + (s + 16) * stride);
            const float4 c2 = ld4(p + (s + 32) * stride), d = ld4(p + (s + 48) * stride);
            acc = f4_add(acc, f4_add(f4_add(a, b), f4_add(c2, d)));
        }
        for (; s < n_slabs; s += 16) acc = f4_add(acc, ld4(p + s * stride));
    }
    part[sg][c] = acc;
    __syncthreads();
    if (sg == 0 && col < len4) {
        float4 t = part[0][c];
#pragma unroll
        for (int k = 1; k < 16; ++k) t = f4_add(t, part[k][c]);
        st4(dst + col * 4, t);
    }
}

// The update of four consecutive parameters: the one statement of Adam's arithmetic, shared by every Adam kernel here
// (so the guarded step is bitwise the plain one whenever its gradient multiplier equals grad_scale).  On registers:
// adam_update4 wraps it in the loads and stores, the recipe kernel adds its own around it.
__device__ __forceinline__ void adam_math4(float4& p, const float4& g, float4& mm, float4& vv, float omb1, float beta2,
                                           float omb2, float eps, float step_size, float sqrt_bc2, float grad_scale) {
    float* pp = &p.x; const float* gp = &g.x; float* mp = &mm.x; float* vp = &vv.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float gk = gp[k] * grad_scale;
        mp[k] = mp[k] + omb1 * (gk - mp[k]);            // exp_avg.lerp_(grad, 1-beta1)
        vp[k] = vp[k] * beta2 + omb2 * gk * gk;
        const float denom = sqrtf(vp[k]) / sqrt_bc2 + eps;
        pp[k] -= step_size * (mp[k] / denom);
    }
}

__device__ __forceinline__ void adam_update4(float* __restrict__ param, const float* __restrict__ grad, float* __restrict__ m,
                                             float* __restrict__ v, bf16_t* __restrict__ shadow, int64_t e, float omb1,
                                             float beta2, float omb2, float eps, float step_size, float sqrt_bc2,
                                             float grad_scale) {
    float4 p = ld4(param + e * 4), g = ld4(grad + e * 4), mm = ld4(m + e * 4), vv = ld4(v + e * 4);
    adam_math4(p, g, mm, vv, omb1, beta2, omb2, eps, step_size, sqrt_bc2, grad_scale);
    st4(param + e * 4, p); st4(m + e * 4, mm); st4(v + e * 4, vv);
    if (shadow != nullptr) st4(shadow + e * 4, p);         // bf16 copy of the updated weights for the bf16-MFMA projections
}

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ param, const float* __restrict__ grad,
                                                   float* __restrict__ m, float* __restrict__ v, int64_t n4,
                                                   float beta1, float beta2, float eps, float step_size,
                                                   float sqrt_bc2, float grad_scale, bf16_t* __restrict__ shadow,
                                                   const float* __restrict__ coef_dev) {
    // captured-graph mode: the bias-correction factors of THIS step live in device memory (adam_state_kernel), because a
    // replayed launch cannot take new by-value arguments
    if (coef_dev != nullptr) { step_size = coef_dev[0]; sqrt_bc2 = coef_dev[1]; }
    const float omb1 = 1.f - beta1, omb2 = 1.f - beta2;
    (void)beta1;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n4; e += (int64_t)gridDim.x * blockDim.x) {
        adam_update4(param, grad, m, v, shadow, e, omb1, beta2, omb2, eps, step_size, sqrt_bc2, grad_scale);
    }
}

static unsigned stream_blocks(int64_t n4) {
    int64_t b = (n4 + 255) / 256;
    if (b > 2048) b = 2048;
    if (b < 1) b = 1;
    return (unsigned)b;
}

// Many independent reductions in ONE launch (blockIdx.y = table row): the backward of the reference's GridNet leaves one
// slab set per convolution (61) - each a few microseconds of work behind its own launch.  table[i] = {slabs pointer,
// slab stride, slab count, destination pointer, length}, int64 each, in DEVICE memory (built once: the tape is static).
// Every row is reduced exactly as vlg_reduce_slabs would reduce it (same summation order).
__global__ __launch_bounds__(256) void reduce_slabs_table_kernel(const int64_t* __restrict__ table) {
    __shared__ float4 part[16][16];
    reduce_table_row(table, (int)blockIdx.y, (int)blockIdx.x, (int)gridDim.x, part);          // csrc/reduce_body.h
}

extern "C" int vlg_reduce_slabs_table(const int64_t* table, int n_rows, int blocks_per_row, void* stream) {
    if (!table || n_rows < 1 || n_rows > 65535 || blocks_per_row < 1 || blocks_per_row > 4096) return VLG_ERR_SHAPE;
    hipLaunchKernelGGL(reduce_slabs_table_kernel, dim3((unsigned)blocks_per_row, (unsigned)n_rows), dim3(256), 0,
                       (hipStream_t)stream, table);
    return vlg_last_error();
}

// table[i] = {partials pointer, count, destination pointer}: dst[0] = sum of the partials (as vlg_sum_partials, accumulate = 0)
__global__ __launch_bounds__(256) void sum_partials_table_kernel(const int64_t* __restrict__ table) {
    __shared__ float red[4];
    const int64_t* t = table + 3 * (int64_t)blockIdx.x;
    const float* __restrict__ part = reinterpret_cast<const float*>(t[0]);
    const int n = (int)t[1];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += part[i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) reinterpret_cast<float*>(t[2])[0] = s;
}

extern "C" int vlg_sum_partials_table(const int64_t* table, int n_rows, void* stream) {
    if (!table || n_rows < 1) return VLG_ERR_SHAPE;
    hipLaunchKernelGGL(sum_partials_table_kernel, dim3((unsigned)n_rows), dim3(256), 0, (hipStream_t)stream, table);
    return vlg_last_error();
}

extern "C" int vlg_reduce_slabs(const float* slabs, int64_t slab_stride, int n_slabs, float* dst, int64_t len,
                                void* stream) {
    if (n_slabs < 1 || len < 4 || (len & 3) || (slab_stride & 3) || slab_stride < len) return VLG_ERR_SHAPE;
    if (!vlg_aligned16(slabs) || !vlg_aligned16(dst)) return VLG_ERR_ALIGN;
    const int64_t len4 = len / 4;
    if (len4 < 32768 && n_slabs >= 16)         // fewer than 128 flat blocks: split the slabs across threads instead
        hipLaunchKernelGGL(reduce_slabs_tall_kernel, dim3((unsigned)((len4 + 15) / 16)), dim3(256), 0,
                           (hipStream_t)stream, slabs, slab_stride, n_slabs, dst, len4);
    else
        hipLaunchKernelGGL(reduce_slabs_kernel, dim3(stream_blocks(len4)), dim3(256), 0, (hipStream_t)stream, slabs,
                           slab_stride, n_slabs, dst, len4);
    return vlg_last_error();
}

static int adam_launch(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, bf16_t* shadow, int64_t n,
                       int step, float lr, float beta1, float beta2, float eps, float grad_scale, void* stream) {
    if (n < 4 || (n & 3) || step < 1) return VLG_ERR_SHAPE;
    if (!vlg_aligned16(param) || !vlg_aligned16(grad) || !vlg_aligned16(exp_avg) || !vlg_aligned16(exp_avg_sq) ||
        (shadow && !vlg_aligned8(shadow))) return VLG_ERR_ALIGN;
    // bias corrections in double, as torch.optim.Adam computes them on the host
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    const float step_size = (float)((double)lr / bc1);
    const float sqrt_bc2 = (float)sqrt(bc2);
    hipLaunchKernelGGL(adam_kernel, dim3(stream_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, param, grad,
                       exp_avg, exp_avg_sq, n / 4, beta1, beta2, eps, step_size, sqrt_bc2, grad_scale, shadow, (const float*)nullptr);
    return vlg_last_error();
}

extern "C" int vlg_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                             int step, float lr, float beta1, float beta2, float eps, float grad_scale,
                             void* stream) {
    return adam_launch(param, grad, exp_avg, exp_avg_sq, nullptr, n, step, lr, beta1, beta2, eps, grad_scale, stream);
}

extern "C" int vlg_adam_step_bf16(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                                  vlg_bf16* shadow, int64_t n, int step, float lr, float beta1, float beta2,
                                  float eps, float grad_scale, void* stream) {
    if (!shadow) return VLG_ERR_SHAPE;
    return adam_launch(param, grad, exp_avg, exp_avg_sq, reinterpret_cast<bf16_t*>(shadow), n, step, lr, beta1, beta2, eps,
                       grad_scale, stream);
}

// ---- Adam with its step counter on the device (hipGraph replay: vlg/engine.py capture_train_step)
// state = {float step_size, float sqrt_bc2, int step, int pad}: one thread advances the counter and recomputes the two
// factors in double, exactly as adam_launch does on the host.
__global__ void adam_state_kernel(float* state, float lr, float beta1, float beta2, int advance) {
    int* istate = reinterpret_cast<int*>(state);
    const int step = istate[2] + (advance ? 1 : 0);
    istate[2] = step;
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    state[0] = (float)((double)lr / bc1);
    state[1] = (float)sqrt(bc2);
}

extern "C" int vlg_adam_step_graph(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, vlg_bf16* shadow,
                                   int64_t n, float* state, int advance, float lr, float beta1, float beta2, float eps,
                                   float grad_scale, void* stream) {
    if (n < 4 || (n & 3) || !state) return VLG_ERR_SHAPE;
    if (!vlg_aligned16(param) || !vlg_aligned16(grad) || !vlg_aligned16(exp_avg) || !vlg_aligned16(exp_avg_sq) ||
        !vlg_aligned16(state) || (shadow && !vlg_aligned8(shadow))) return VLG_ERR_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(adam_state_kernel, dim3(1), dim3(1), 0, s, state, lr, beta1, beta2, advance);
    hipLaunchKernelGGL(adam_kernel, dim3(stream_blocks(n / 4)), dim3(256), 0, s, param, grad, exp_avg, exp_avg_sq, n / 4,
                       beta1, beta2, eps, 0.f, 1.f, grad_scale, reinterpret_cast<bf16_t*>(shadow), (const float*)state);
    return vlg_last_error();
}

// ---- guarded step: gradient norm, control record, Adam driven by the record
#define VLG_SUMSQ_MAX_BLOCKS 2048

extern "C" int vlg_grad_sumsq_blocks(int64_t n) {
    int64_t b = (n / 4 + 255) / 256;
    if (b > VLG_SUMSQ_MAX_BLOCKS) b = VLG_SUMSQ_MAX_BLOCKS;
    if (b < 1) b = 1;
    return (int)b;
}

__device__ __forceinline__ double sumsq4(double acc, float4 g) {
    const double x = g.x, y = g.y, z = g.z, w = g.w;         // squares of fp32 values are exact in fp64
    return acc + ((x * x + y * y) + (z * z + w * w));
}

// sum over the block in a fixed order (lane tree, then the waves in order); result valid in thread 0
__device__ __forceinline__ double block_sum_f64(double v, double* smem) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63, nw = (blockDim.x + 63) >> 6;
    if (l == 0) smem[w] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0)
        for (int i = 0; i < nw; ++i) r += smem[i];
    return r;
}

__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ grad, int64_t n4,
                                                         float* __restrict__ partials) {
    __shared__ double red[4];
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double a0 = 0.0, a1 = 0.0;
    for (; e + stride < n4; e += 2 * stride) {               // 2 independent loads in flight per lane
        const float4 g0 = ld4(grad + e * 4), g1 = ld4(grad + (e + stride) * 4);
        a0 = sumsq4(a0, g0);
        a1 = sumsq4(a1, g1);
    }
    if (e < n4) a0 = sumsq4(a0, ld4(grad + e * 4));
    const double s = block_sum_f64(a0 + a1, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = (float)s;   // beyond fp32 range -> inf: the step is skipped, not wrong
}

extern "C" int vlg_grad_sumsq(const float* grad, int64_t n, float* partials, void* stream) {
    if (n < 4 || (n & 3) || !partials) return VLG_ERR_SHAPE;
    if (!vlg_aligned16(grad) || !vlg_aligned16(partials)) return VLG_ERR_ALIGN;
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)vlg_grad_sumsq_blocks(n)), dim3(256), 0, (hipStream_t)stream,
                       grad, n / 4, partials);
    return vlg_last_error();
}

// ctl: the record include/vlg_hip.h documents (VLG_CTL_*).  One block; thread 0 decides.  `ext` (VLG_EXT_*, or NULL: the
// plain guarded step) adds the recipe: the learning rate of THIS step under warm-up, and from it the decay multiplier, and
// the EMA weight.  With ext == NULL, or warm-up off, every ctl slot gets the bits it always got ((double)LR * 1 is LR).
__device__ __forceinline__ void optim_control_decide(float* __restrict__ ctl, float* __restrict__ ext,
                                                     const float* __restrict__ partials, int n_partials, float grad_scale,
                                                     float max_norm, float beta1, float beta2, double* red) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < n_partials; i += 256) acc += (double)partials[i];
    const double sum = block_sum_f64(acc, red);
    if (threadIdx.x != 0) return;
    int* ictl = reinterpret_cast<int*>(ctl);
    const double norm = (double)grad_scale * sqrt(sum);
    const float norm_f = (float)norm;
    ctl[VLG_CTL_GRAD_NORM] = norm_f;
    if (!isfinite(norm_f)) {                                 // inf or NaN anywhere in the gradient: leave the state alone
        ictl[VLG_CTL_APPLY] = 0;
        ictl[VLG_CTL_SKIPPED] = ictl[VLG_CTL_SKIPPED] + 1;
        return;
    }
    const int step = ictl[VLG_CTL_STEP] + 1;
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    double coef = 1.0;
    if (max_norm > 0.f) coef = fmin(1.0, (double)max_norm / (norm + 1e-6));     // torch.nn.utils.clip_grad_norm_
    double lr_eff = (double)ctl[VLG_CTL_LR];
    if (ext != nullptr) {
        const int* iext = reinterpret_cast<const int*>(ext);
        const int warmup = iext[VLG_EXT_WARMUP_STEPS];
        if (warmup > 0) lr_eff = __dmul_rn(lr_eff, fmin(1.0, (double)step / (double)warmup));
        double d_t = (double)ext[VLG_EXT_EMA_DECAY];
        if (iext[VLG_EXT_EMA_WARMUP] != 0) d_t = fmin(d_t, (1.0 + (double)step) / (10.0 + (double)step));
        ext[VLG_EXT_LR_EFF] = (float)lr_eff;
        // (products rounded on their own: a fused multiply-add would differ from 1 - lr * wd in the last bit of the double)
        ext[VLG_EXT_DECAY_MULT] = (float)(1.0 - __dmul_rn(lr_eff, (double)ext[VLG_EXT_WEIGHT_DECAY]));
        ext[VLG_EXT_EMA_OMD] = (float)(1.0 - d_t);
    }
    ctl[VLG_CTL_STEP_SIZE] = (float)(lr_eff / bc1);
    ctl[VLG_CTL_SQRT_BC2] = (float)sqrt(bc2);
    ictl[VLG_CTL_STEP] = step;
    ictl[VLG_CTL_APPLY] = 1;
    ctl[VLG_CTL_GRAD_MULT] = max_norm > 0.f ? (float)((double)grad_scale * coef) : grad_scale;
    ctl[VLG_CTL_CLIP_COEF] = (float)coef;
}

__global__ __launch_bounds__(256) void optim_control_kernel(float* __restrict__ ctl, const float* __restrict__ partials,
                                                            int n_partials, float grad_scale, float max_norm,
                                                            float beta1, float beta2) {
    __shared__ double red[4];
    optim_control_decide(ctl, nullptr, partials, n_partials, grad_scale, max_norm, beta1, beta2, red);
}

__global__ __launch_bounds__(256) void optim_control_ext_kernel(float* __restrict__ ctl, float* __restrict__ ext,
                                                                const float* __restrict__ partials, int n_partials,
                                                                float grad_scale, float max_norm, float beta1, float beta2) {
    __shared__ double red[4];
    optim_control_decide(ctl, ext, partials, n_partials, grad_scale, max_norm, beta1, beta2, red);
}

extern "C" int vlg_optim_control(float* ctl, const float* partials, int n_partials, float grad_scale, float max_norm,
                                 float beta1, float beta2, void* stream) {
    if (!ctl || !partials || n_partials < 1 || n_partials > VLG_SUMSQ_MAX_BLOCKS) return VLG_ERR_SHAPE;
    if (!vlg_aligned16(ctl)) return VLG_ERR_ALIGN;
    hipLaunchKernelGGL(optim_control_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, ctl, partials, n_partials,
                       grad_scale, max_norm, beta1, beta2);
    return vlg_last_error();
}

extern "C" int vlg_optim_control_ext(float* ctl, float* ext, const float* partials, int n_partials, float grad_scale,
                                     float max_norm, float beta1, float beta2, void* stream) {
    if (!ctl || !ext || !partials || n_partials < 1 || n_partials > VLG_SUMSQ_MAX_BLOCKS) return VLG_ERR_SHAPE;
    if (!vlg_aligned16(ctl) || !vlg_aligned16(ext)) return VLG_ERR_ALIGN;
    hipLaunchKernelGGL(optim_control_ext_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, ctl, ext, partials,
                       n_partials, grad_scale, max_norm, beta1, beta2);
    return vlg_last_error();
}

__global__ __launch_bounds__(256) void adam_ctl_kernel(float* __restrict__ param, const float* __restrict__ grad,
                                                       float* __restrict__ m, float* __restrict__ v, int64_t n4,
                                                       float beta1, float beta2, float eps, bf16_t* __restrict__ shadow,
                                                       const float* __restrict__ ctl) {
    // a branch, not a multiplication by zero: 0 * inf would write NaN into the moments
    if (reinterpret_cast<const int*>(ctl)[VLG_CTL_APPLY] == 0) return;
    const float step_size = ctl[VLG_CTL_STEP_SIZE], sqrt_bc2 = ctl[VLG_CTL_SQRT_BC2], grad_mult = ctl[VLG_CTL_GRAD_MULT];
    const float omb1 = 1.f - beta1, omb2 = 1.f - beta2;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n4; e += (int64_t)gridDim.x * blockDim.x)
        adam_update4(param, grad, m, v, shadow, e, omb1, beta2, omb2, eps, step_size, sqrt_bc2, grad_mult);
}

extern "C" int vlg_adam_step_ctl(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, vlg_bf16* shadow,
                                 int64_t n, const float* ctl, float beta1, float beta2, float eps, void* stream) {
    if (n < 4 || (n & 3) || !ctl) return VLG_ERR_SHAPE;
    if (!vlg_aligned16(param) || !vlg_aligned16(grad) || !vlg_aligned16(exp_avg) || !vlg_aligned16(exp_avg_sq) ||
        !vlg_aligned16(ctl) || (shadow && !vlg_aligned8(shadow))) return VLG_ERR_ALIGN;
    hipLaunchKernelGGL(adam_ctl_kernel, dim3(stream_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, param, grad,
                       exp_avg, exp_avg_sq, n / 4, beta1, beta2, eps, reinterpret_cast<bf16_t*>(shadow), ctl);
    return vlg_last_error();
}

// ---- the recipe step: decoupled weight decay under a float4 mask, and the weights' moving average
// One float4 per lane and trip, like adam_ctl_kernel: the mask is a byte per lane (one 64-byte line per wave, 0.25 B per
// parameter), the average one more float4 stream in and out.  MASK / EMA are compile-time so that the plain shape of the
// loop (neither) is adam_ctl_kernel's, instruction for instruction.
template <bool MASK, bool EMA>
__global__ __launch_bounds__(256) void adamw_ema_ctl_kernel(float* __restrict__ param, const float* __restrict__ grad,
                                                            float* __restrict__ m, float* __restrict__ v, int64_t n4,
                                                            float beta1, float beta2, float eps, bf16_t* __restrict__ shadow,
                                                            float* __restrict__ ema, bf16_t* __restrict__ ema_shadow,
                                                            const unsigned char* __restrict__ mask,
                                                            const float* __restrict__ ctl, const float* __restrict__ ext) {
    // a branch, not a multiplication by zero: 0 * inf would write NaN into the moments
    if (reinterpret_cast<const int*>(ctl)[VLG_CTL_APPLY] == 0) return;
    const float step_size = ctl[VLG_CTL_STEP_SIZE], sqrt_bc2 = ctl[VLG_CTL_SQRT_BC2], grad_mult = ctl[VLG_CTL_GRAD_MULT];
    const float decay_mult = ext[VLG_EXT_DECAY_MULT], omd = ext[VLG_EXT_EMA_OMD];
    const float omb1 = 1.f - beta1, omb2 = 1.f - beta2;
    (void)decay_mult; (void)omd;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n4; e += (int64_t)gridDim.x * blockDim.x) {
        float4 p = ld4(param + e * 4), g = ld4(grad + e * 4), mm = ld4(m + e * 4), vv = ld4(v + e * 4);
        float4 ev = f4_zero();
        if (EMA) ev = ld4(ema + e * 4);
        if (MASK) {
            if (mask[e] != 0) {       // p.mul_(1 - lr * wd) BEFORE the update, rounded on its own (not fused into it)
                p.x = __fmul_rn(p.x, decay_mult); p.y = __fmul_rn(p.y, decay_mult);
                p.z = __fmul_rn(p.z, decay_mult); p.w = __fmul_rn(p.w, decay_mult);
            }
        }
        adam_math4(p, g, mm, vv, omb1, beta2, omb2, eps, step_size, sqrt_bc2, grad_mult);
        st4(param + e * 4, p); st4(m + e * 4, mm); st4(v + e * 4, vv);
        if (shadow != nullptr) st4(shadow + e * 4, p);
        if (EMA) {
            ev.x = ev.x + omd * (p.x - ev.x); ev.y = ev.y + omd * (p.y - ev.y);
            ev.z = ev.z + omd * (p.z - ev.z); ev.w = ev.w + omd * (p.w - ev.w);
            st4(ema + e * 4, ev);
            if (ema_shadow != nullptr) st4(ema_shadow + e * 4, ev);
        }
    }
}

extern "C" int vlg_adamw_ema_step_ctl(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, vlg_bf16* shadow,
                                      float* ema, vlg_bf16* ema_shadow, const uint8_t* decay_mask, int64_t n,
                                      const float* ctl, const float* ext, float beta1, float beta2, float eps, void* stream) {
    if (n < 4 || (n & 3) || !ctl || !ext || (ema_shadow && !ema)) return VLG_ERR_SHAPE;
    if (!vlg_aligned16(param) || !vlg_aligned16(grad) || !vlg_aligned16(exp_avg) || !vlg_aligned16(exp_avg_sq) ||
        !vlg_aligned16(ctl) || !vlg_aligned16(ext) || (shadow && !vlg_aligned8(shadow)) || (ema && !vlg_aligned16(ema)) ||
        (ema_shadow && !vlg_aligned8(ema_shadow)) || !vlg_aligned4(decay_mask)) return VLG_ERR_ALIGN;
    const dim3 grid(stream_blocks(n / 4)), block(256);
    hipStream_t s = (hipStream_t)stream;
    bf16_t* sh = reinterpret_cast<bf16_t*>(shadow);
    bf16_t* esh = reinterpret_cast<bf16_t*>(ema_shadow);
#define VLG_RECIPE_LAUNCH(MASK, EMA)                                                                                       \
    hipLaunchKernelGGL((adamw_ema_ctl_kernel<MASK, EMA>), grid, block, 0, s, param, grad, exp_avg, exp_avg_sq, n / 4, beta1, \
                       beta2, eps, sh, ema, esh, decay_mask, ctl, ext)
    if (decay_mask && ema) VLG_RECIPE_LAUNCH(true, true);
    else if (decay_mask) VLG_RECIPE_LAUNCH(true, false);
    else if (ema) VLG_RECIPE_LAUNCH(false, true);
    else VLG_RECIPE_LAUNCH(false, false);
#undef VLG_RECIPE_LAUNCH
    return vlg_last_error();
}
