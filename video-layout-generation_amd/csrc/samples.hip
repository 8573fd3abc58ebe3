// Sampled futures: score K generated futures of every clip against the frames that really followed, measure how much the K
// differ, and select the best one - three launches, no host wait (include/vlg_hip.h, "sampled futures"; tests/samples_ref.py
// restates them in fp64; DESIGN.md, "Sampled futures").
//
// gen_cls (K,B,S,N) int64 / gen_box (K,B,S,N,4) fp32 are the samples; the truth is read in place from clip_class (B,tgt_T,N) /
// clip_box (B,tgt_T,N,4), frame t0 + s for generated frame s.  A token is SCORED when its truth class is in [0, n_classes).
// Per scored token, in fp32 (this file is compiled with floating-point contraction off, so every operation below is one
// rounding and the values can be restated exactly):
//   iou   IoU of the (cx,cy,w,h) boxes, the formula and iou_eps of csrc/loss.hip; 0 when the generated class is >= n_classes
//   disp  sqrtf(dx*dx + dy*dy) of the two centres
//   hit   generated class == truth class
// min / max are fminf / fmaxf: a NaN coordinate is ignored by them, a NaN size makes the union and so the IoU NaN.
// Sums are doubles added in a fixed order: thread i of a block adds its tokens i, i + 256, ... in that order, the 256 thread sums
// are added by a halving tree in LDS.  No floating-point atomics, no scratch: the same call gives the same bits.
//
// vlg_layout_sample_scores     one block per (sample, clip): S*N tokens, 8 floats out.  Launch-bound.
// vlg_layout_sample_diversity  one block per clip: every pair j < k of samples on every scored token (K(K-1)/2 * S*N IoUs of
//     boxes the first pair pulled into the cache), 2 floats out.
// vlg_layout_sample_select     ONE block: thread b walks clip b's K scores (the first sample that is not NaN and strictly
//     better than every earlier one; 0 if all are NaN), adds the clip's terms to 16 doubles, the block adds those to the
//     record; then all threads copy the selected samples (24 bytes per token).
#include "common.h"

#define SMP_BLOCK 256
#define SMP_MAX_C 28                 /* decode's limit on n_classes (n_classes + 4 <= 32) */
#define SMP_SCORE_COLS 4             /* IOU, ADE, FDE, ACC: the columns a criterion may name */

// the block's sum of v, in a fixed order, to every thread (sh: SMP_BLOCK doubles; safe to call back to back)
__device__ __forceinline__ double smp_block_sum(double v, double* sh) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
#pragma unroll
    for (int o = SMP_BLOCK / 2; o > 0; o >>= 1) {
        if (tid < o) sh[tid] += sh[tid + o];
        __syncthreads();
    }
    const double tot = sh[0];
    __syncthreads();
    return tot;
}

// IoU of two (cx, cy, w, h) boxes: csrc/loss.hip's formula
__device__ __forceinline__ float smp_iou(float4 a, float4 b, float eps) {
    const float ax1 = a.x - 0.5f * a.z, ax2 = a.x + 0.5f * a.z;
    const float ay1 = a.y - 0.5f * a.w, ay2 = a.y + 0.5f * a.w;
    const float bx1 = b.x - 0.5f * b.z, bx2 = b.x + 0.5f * b.z;
    const float by1 = b.y - 0.5f * b.w, by2 = b.y + 0.5f * b.w;
    const float iw = fmaxf(fminf(ax2, bx2) - fmaxf(ax1, bx1), 0.f);
    const float ih = fmaxf(fminf(ay2, by2) - fmaxf(ay1, by1), 0.f);
    const float inter = iw * ih;
    const float uni = a.z * a.w + b.z * b.w - inter;
    return inter / (uni + eps);
}

__global__ __launch_bounds__(SMP_BLOCK) void sample_scores_kernel(
    const int64_t* __restrict__ gen_cls, const float* __restrict__ gen_box, const int64_t* __restrict__ clip_class,
    const float* __restrict__ clip_box, float* __restrict__ scores, int B, int S, int N, int tgt_T, int t0, int C, float iou_eps) {
    __shared__ double sh[SMP_BLOCK];
    const int tid = threadIdx.x, SN = S * N;
    const int64_t kb = blockIdx.x;                         // k*B + b
    const int64_t b = kb % B;
    double s_iou = 0.0, s_disp = 0.0, s_last = 0.0, s_hit = 0.0, n_sc = 0.0, n_last = 0.0;
    for (int i = tid; i < SN; i += SMP_BLOCK) {
        const int s = i / N, n = i - s * N;
        const int64_t src = (b * tgt_T + t0 + s) * N + n, g = kb * SN + i;
        const int64_t tc = clip_class[src];
        if (tc < 0 || tc >= C) continue;
        const int64_t gc = gen_cls[g];
        const float4 gb = ld4(gen_box + 4 * g), tb = ld4(clip_box + 4 * src);
        const float iou = gc >= C ? 0.f : smp_iou(gb, tb, iou_eps);
        const float dx = gb.x - tb.x, dy = gb.y - tb.y;
        const float disp = sqrtf(dx * dx + dy * dy);
        s_iou += (double)iou;
        s_disp += (double)disp;
        s_hit += gc == tc ? 1.0 : 0.0;
        n_sc += 1.0;
        if (s == S - 1) { s_last += (double)disp; n_last += 1.0; }
    }
    s_iou = smp_block_sum(s_iou, sh);
    s_disp = smp_block_sum(s_disp, sh);
    s_last = smp_block_sum(s_last, sh);
    s_hit = smp_block_sum(s_hit, sh);
    n_sc = smp_block_sum(n_sc, sh);                        // counts <= 2^24: exact in double and in the float they leave as
    n_last = smp_block_sum(n_last, sh);
    if (tid == 0) {
        float* row = scores + kb * VLG_SMP_COLS;
        st4(row, make_float4(n_sc > 0.0 ? (float)(s_iou / n_sc) : 0.f, n_sc > 0.0 ? (float)(s_disp / n_sc) : 0.f,
                             n_last > 0.0 ? (float)(s_last / n_last) : 0.f, n_sc > 0.0 ? (float)(s_hit / n_sc) : 0.f));
        st4(row + 4, make_float4((float)n_sc, (float)n_last, 0.f, 0.f));
    }
}

__global__ __launch_bounds__(SMP_BLOCK) void sample_diversity_kernel(
    const int64_t* __restrict__ gen_cls, const float* __restrict__ gen_box, const int64_t* __restrict__ clip_class,
    float* __restrict__ div, int K, int B, int S, int N, int tgt_T, int t0, int C, float iou_eps) {
    __shared__ double sh[SMP_BLOCK];
    const int tid = threadIdx.x, SN = S * N;
    const int64_t b = blockIdx.x, stride = (int64_t)B * SN;    // from one sample of a token to the next
    double s_box = 0.0, s_cls = 0.0, n_sc = 0.0;
    for (int i = tid; i < SN; i += SMP_BLOCK) {
        const int s = i / N, n = i - s * N;
        const int64_t tc = clip_class[(b * tgt_T + t0 + s) * N + n];
        if (tc < 0 || tc >= C) continue;
        n_sc += 1.0;
        const int64_t g0 = b * SN + i;
        for (int j = 0; j + 1 < K; ++j) {
            const float4 bj = ld4(gen_box + 4 * (g0 + j * stride));
            const int64_t cj = gen_cls[g0 + j * stride];
            for (int k = j + 1; k < K; ++k) {
                const float d = 1.0f - smp_iou(bj, ld4(gen_box + 4 * (g0 + k * stride)), iou_eps);
                s_box += (double)d;
                s_cls += cj != gen_cls[g0 + k * stride] ? 1.0 : 0.0;
            }
        }
    }
    s_box = smp_block_sum(s_box, sh);
    s_cls = smp_block_sum(s_cls, sh);
    n_sc = smp_block_sum(n_sc, sh);
    if (tid == 0) {
        const double terms = n_sc * (0.5 * (double)K * (double)(K - 1));
        div[2 * b] = terms > 0.0 ? (float)(s_box / terms) : 0.f;
        div[2 * b + 1] = terms > 0.0 ? (float)(s_cls / terms) : 0.f;
    }
}

// is a better than b under the column's sense (IOU, ACC: larger; ADE, FDE: smaller)?  false when either is NaN
__device__ __forceinline__ bool smp_better(float a, float b, int col) {
    return (col == VLG_SMP_ADE || col == VLG_SMP_FDE) ? a < b : a > b;
}
// the column's choice among a clip's K scores: the first sample that is not NaN and strictly better than every earlier one
__device__ __forceinline__ int smp_choose(const float* __restrict__ scores, int64_t b, int K, int B, int col) {
    int pick = -1;
    float best = 0.f;
    for (int k = 0; k < K; ++k) {
        const float v = scores[((int64_t)k * B + b) * VLG_SMP_COLS + col];
        if (v != v) continue;
        if (pick < 0 || smp_better(v, best, col)) { pick = k; best = v; }
    }
    return pick < 0 ? 0 : pick;
}

__global__ __launch_bounds__(SMP_BLOCK) void sample_select_kernel(
    const float* __restrict__ scores, const float* __restrict__ div, const int64_t* __restrict__ gen_cls,
    const float* __restrict__ gen_box, int* __restrict__ best, int64_t* __restrict__ best_cls, float* __restrict__ best_box,
    double* __restrict__ record, int K, int B, int S, int N, int criterion) {
    __shared__ double sh[SMP_BLOCK];
    const int tid = threadIdx.x;
    double acc[VLG_SMP_REC_SLOTS];
#pragma unroll
    for (int i = 0; i < VLG_SMP_REC_SLOTS; ++i) acc[i] = 0.0;
    for (int64_t b = tid; b < B; b += SMP_BLOCK) {
        const int sel = smp_choose(scores, b, K, B, criterion);
        best[b] = sel;
        const float* row0 = scores + b * VLG_SMP_COLS;
        if (!(row0[VLG_SMP_N_SCORED] > 0.f)) continue;                     // (the counts are the truth's: the same for every sample)
        const bool last = row0[VLG_SMP_N_SCORED_LAST] > 0.f;
#pragma unroll
        for (int col = 0; col < SMP_SCORE_COLS; ++col) {
            if (col == VLG_SMP_FDE && !last) continue;
            const int own = smp_choose(scores, b, K, B, col);
            double mean = 0.0;
            for (int k = 0; k < K; ++k) mean += (double)scores[((int64_t)k * B + b) * VLG_SMP_COLS + col];
            acc[VLG_SMP_REC_BEST + col] += (double)scores[((int64_t)own * B + b) * VLG_SMP_COLS + col];
            acc[VLG_SMP_REC_MEAN + col] += mean / (double)K;
            acc[VLG_SMP_REC_SELECTED + col] += (double)scores[((int64_t)sel * B + b) * VLG_SMP_COLS + col];
        }
        acc[VLG_SMP_REC_DIV_BOX] += (double)div[2 * b];
        acc[VLG_SMP_REC_DIV_CLASS] += (double)div[2 * b + 1];
        acc[VLG_SMP_REC_CLIPS] += 1.0;
        acc[VLG_SMP_REC_CLIPS_FDE] += last ? 1.0 : 0.0;
    }
#pragma unroll
    for (int i = 0; i < VLG_SMP_REC_SLOTS; ++i) {
        const double tot = smp_block_sum(acc[i], sh);                       // (its barriers also publish best[] to the block)
        if (tid == i) record[i] += tot;
    }
    // the selected samples
    const int64_t SN = (int64_t)S * N, total = (int64_t)B * SN;
    for (int64_t i = tid; i < total; i += SMP_BLOCK) {
        const int64_t b = i / SN, g = ((int64_t)best[b] * B) * SN + i;
        best_cls[i] = gen_cls[g];
        st4(best_box + 4 * i, ld4(gen_box + 4 * g));
    }
}

extern "C" int vlg_layout_sample_record_slots(void) { return VLG_SMP_REC_SLOTS; }

// the refusals the three entries share; sizes of the sample and truth buffers in tokens
static int samples_checks(int K, int B, int S, int N, int tgt_T, int t0, int n_classes) {
    if (K < 1 || B < 1 || S < 1 || N < 1 || t0 < 0 || (int64_t)t0 + S > tgt_T) return VLG_ERR_SHAPE;
    if (n_classes < 1 || n_classes > SMP_MAX_C) return VLG_ERR_SHAPE;
    if ((int64_t)S * N > (1LL << 24)) return VLG_ERR_SHAPE;                 // a clip's counts leave as floats
    if ((int64_t)K * B > 0x7fffffffLL) return VLG_ERR_SHAPE;                // one block per (sample, clip)
    return 0;
}

extern "C" int vlg_layout_sample_scores(const int64_t* gen_cls, const float* gen_box, const int64_t* clip_class,
                                        const float* clip_box, float* scores, int K, int B, int S, int N, int tgt_T, int t0,
                                        int n_classes, float iou_eps, void* stream) {
    const int err = samples_checks(K, B, S, N, tgt_T, t0, n_classes);
    if (err != 0) return err;
    if (!gen_cls || !gen_box || !clip_class || !clip_box || !scores) return VLG_ERR_ALIGN;
    if (!vlg_aligned8(gen_cls) || !vlg_aligned16(gen_box) || !vlg_aligned8(clip_class) || !vlg_aligned16(clip_box) ||
        !vlg_aligned16(scores)) return VLG_ERR_ALIGN;
    const int64_t G = (int64_t)K * B * S * N, Tk = (int64_t)B * tgt_T * N, out_n = (int64_t)K * B * VLG_SMP_COLS * 4;
    if (vlg_overlap(scores, out_n, gen_cls, G * 8) || vlg_overlap(scores, out_n, gen_box, G * 16) ||
        vlg_overlap(scores, out_n, clip_class, Tk * 8) || vlg_overlap(scores, out_n, clip_box, Tk * 16)) return VLG_ERR_SHAPE;
    hipLaunchKernelGGL(sample_scores_kernel, dim3((unsigned)((int64_t)K * B)), dim3(SMP_BLOCK), 0, (hipStream_t)stream, gen_cls,
                       gen_box, clip_class, clip_box, scores, B, S, N, tgt_T, t0, n_classes, iou_eps);
    return vlg_last_error();
}

extern "C" int vlg_layout_sample_diversity(const int64_t* gen_cls, const float* gen_box, const int64_t* clip_class, float* div,
                                           int K, int B, int S, int N, int tgt_T, int t0, int n_classes, float iou_eps,
                                           void* stream) {
    const int err = samples_checks(K, B, S, N, tgt_T, t0, n_classes);
    if (err != 0) return err;
    if (!gen_cls || !gen_box || !clip_class || !div) return VLG_ERR_ALIGN;
    if (!vlg_aligned8(gen_cls) || !vlg_aligned16(gen_box) || !vlg_aligned8(clip_class) || !vlg_aligned8(div)) return VLG_ERR_ALIGN;
    const int64_t G = (int64_t)K * B * S * N, Tk = (int64_t)B * tgt_T * N, out_n = (int64_t)B * 2 * 4;
    if (vlg_overlap(div, out_n, gen_cls, G * 8) || vlg_overlap(div, out_n, gen_box, G * 16) ||
        vlg_overlap(div, out_n, clip_class, Tk * 8)) return VLG_ERR_SHAPE;
    hipLaunchKernelGGL(sample_diversity_kernel, dim3((unsigned)B), dim3(SMP_BLOCK), 0, (hipStream_t)stream, gen_cls, gen_box,
                       clip_class, div, K, B, S, N, tgt_T, t0, n_classes, iou_eps);
    return vlg_last_error();
}

extern "C" int vlg_layout_sample_select(const float* scores, const float* div, const int64_t* gen_cls, const float* gen_box,
                                        int* best, int64_t* best_cls, float* best_box, double* record, int K, int B, int S, int N,
                                        int criterion, void* stream) {
    if (K < 1 || B < 1 || S < 1 || N < 1 || (int64_t)S * N > (1LL << 24) || (int64_t)K * B > 0x7fffffffLL) return VLG_ERR_SHAPE;
    if (criterion != VLG_SMP_IOU && criterion != VLG_SMP_ADE && criterion != VLG_SMP_FDE && criterion != VLG_SMP_ACC)
        return VLG_ERR_SHAPE;
    if (!scores || !div || !gen_cls || !gen_box || !best || !best_cls || !best_box || !record) return VLG_ERR_ALIGN;
    if (!vlg_aligned16(scores) || !vlg_aligned8(div) || !vlg_aligned8(gen_cls) || !vlg_aligned16(gen_box) || !vlg_aligned4(best) ||
        !vlg_aligned8(best_cls) || !vlg_aligned16(best_box) || !vlg_aligned8(record)) return VLG_ERR_ALIGN;
    const int64_t BSN = (int64_t)B * S * N, G = BSN * K;
    const void* in_p[4] = {scores, div, gen_cls, gen_box};
    const int64_t in_n[4] = {(int64_t)K * B * VLG_SMP_COLS * 4, (int64_t)B * 8, G * 8, G * 16};
    const void* out_p[4] = {best, best_cls, best_box, record};
    const int64_t out_n[4] = {(int64_t)B * 4, BSN * 8, BSN * 16, VLG_SMP_REC_SLOTS * 8};
    for (int j = 0; j < 4; ++j) {
        for (int i = 0; i < 4; ++i)
            if (vlg_overlap(in_p[i], in_n[i], out_p[j], out_n[j])) return VLG_ERR_SHAPE;
        for (int i = j + 1; i < 4; ++i)
            if (vlg_overlap(out_p[i], out_n[i], out_p[j], out_n[j])) return VLG_ERR_SHAPE;
    }
    hipLaunchKernelGGL(sample_select_kernel, dim3(1), dim3(SMP_BLOCK), 0, (hipStream_t)stream, scores, div, gen_cls, gen_box, best,
                       best_cls, best_box, record, K, B, S, N, criterion);
    return vlg_last_error();
}
