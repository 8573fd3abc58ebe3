// Gaussian box head: the negative log-likelihood of the target box under N(mu, sigma^2) per coordinate, its gradient with
// respect to the raw SCALE outputs, and the coverage statistic - one pass over 32 bytes of each head-output row
// (include/vlg_hip.h, "Gaussian box head"; DESIGN.md, "Gaussian box head"; fp64 restatement: tests/boxhead_ref.py).
//
//   mu_k = sigmoid(out[m, C+k])  (a constant here: no gradient reaches the mean),  g_k = sigmoid(out[m, C+4+k]),
//   s_k = s_min + (s_max - s_min) g_k,  e_k = (tgt_k - mu_k) exp(-s_k),  nll_m = 1/4 sum_k (e_k^2 / 2 + s_k + ln(2 pi) / 2)
//
// One thread per token: the 32-byte run out[m, C .. C+8) starts 80 B into a row whose stride is a multiple of 16 B, so it is
// two 16-B loads per lane, beside one 16-B load of the target box; the gradient leaves as two 16-B stores per lane
// (dout[m, C+4 .. C+8) and the exact zeros of the padding columns C+8 .. C+11).  Nothing else of out or dout is touched.
// 52 B in and 32 B out per token - 2.8 MB at the metric shape - so the launch is bound by its latency, not by bytes.
// Every block counts the valid slots ITSELF, as layout_loss_kernel does (the mean's denominator scales every gradient; a
// sum of 0/1 flags is exact in fp32 in any order), with its first pass's loads already in flight.  The last block to
// finish (an integer ticket in scratch[1], which it resets) folds the per-block partials in a fixed order into loss_io
// (vlg_ticket_draw / vlg_ticket_last / vlg_fold_partials, common.h): no float atomics, the same bits from launch to launch.
#include "common.h"

#define BNLL_BLOCK 256
#define BNLL_MAX_BLOCKS 128          /* 32 768 tokens per grid pass; more tokens take the grid-stride loop */
#define BNLL_NCLS 20
// scratch layout (floats): [1] = ticket counter (int, zero between launches); [4 .. 4 + 4*BNLL_MAX_BLOCKS) = per-block partials
#define BNLL_SCRATCH (4 + 4 * BNLL_MAX_BLOCKS)

__global__ __launch_bounds__(BNLL_BLOCK) void layout_box_nll_kernel(
    const float* __restrict__ out, int ld, const float* __restrict__ tgt_box, const float* __restrict__ valid,
    float* __restrict__ dout, float* __restrict__ scratch, float* __restrict__ loss_io, int B, int T, int N, float s_min,
    float s_max, float w_nll) {
    __shared__ float red[BNLL_BLOCK / 64];
    __shared__ float cnt_sh;
    __shared__ int last_sh;
    const int64_t M = (int64_t)B * T * N;
    const int tid = threadIdx.x;
    const float range = s_max - s_min;
    float inv_cnt = 0.f;
    float s_nll = 0.f, s_cov = 0.f;
    const int64_t first = (int64_t)blockIdx.x * BNLL_BLOCK;
    for (int64_t m0 = first; m0 < M; m0 += (int64_t)gridDim.x * BNLL_BLOCK) {
        // ---- this pass's row and targets: requested first, consumed after the count
        const int64_t m = m0 + tid;
        const bool mine = m < M;
        float w = 0.f;
        float4 mr = f4_zero(), sr = f4_zero(), tb = f4_zero();
        if (mine) {
            const int t = (int)(m % T);
            const int64_t bn = m / T;
            const int n = (int)(bn % N);
            const int64_t b = bn / N;
            const int64_t src = (b * T + t) * N + n;
            mr = ld4(out + m * ld + BNLL_NCLS);
            sr = ld4(out + m * ld + BNLL_NCLS + 4);
            w = valid[src];
            tb = ld4(tgt_box + src * 4);
        }
        if (m0 == first) {
            // 1 / max(#valid, 1): sums of 0/1 flags are exact in fp32 in any order, so every block gets the same value
            float c = 0.f;
            const int64_t n4 = M >> 2;
            int64_t i = tid;
            for (; i + 7 * BNLL_BLOCK < n4; i += 8 * BNLL_BLOCK) {
                float4 v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = ld4(valid + 4 * (i + u * BNLL_BLOCK));
#pragma unroll
                for (int u = 0; u < 8; ++u) c += (v[u].x + v[u].y) + (v[u].z + v[u].w);
            }
            for (; i < n4; i += BNLL_BLOCK) {
                const float4 v = ld4(valid + 4 * i);
                c += (v.x + v.y) + (v.z + v.w);
            }
            for (int64_t j = 4 * n4 + tid; j < M; j += BNLL_BLOCK) c += valid[j];
            c = block_sum(c, red);
            if (tid == 0) cnt_sh = 1.0f / fmaxf(c, 1.0f);
            __syncthreads();
            inv_cnt = cnt_sh;
        }
        if (mine) {
            const float raw_mu[4] = {mr.x, mr.y, mr.z, mr.w}, raw_s[4] = {sr.x, sr.y, sr.z, sr.w};
            const float tg[4] = {tb.x, tb.y, tb.z, tb.w};
            const float scale = w_nll * w * inv_cnt * 0.25f;       // an invalid token: multiplication by valid, as the loss kernel
            float g4[4];
            float nll = 0.f, cov = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float mu = 1.0f / (1.0f + expf(-raw_mu[k]));
                // g = sigmoid(x) and g (1 - g) from q = exp(-|x|): g (1 - g) = q / (1 + q)^2 keeps its relative precision
                // where 1 - g would cancel
                const float q = expf(-fabsf(raw_s[k]));
                const float r = 1.0f / (1.0f + q);
                const float g = raw_s[k] >= 0.f ? r : q * r;       // (a NaN raw scale: q, and with it g, is NaN)
                const float s = s_min + range * g;
                const float df = tg[k] - mu;
                const float e = df * expf(-s);
                const float e2 = e * e;
                nll += 0.5f * e2 + s + 0.91893853320467274f;       // ln(2 pi) / 2
                cov += fabsf(df) <= expf(s) ? 1.f : 0.f;
                g4[k] = scale * (1.0f - e2) * range * (q * r * r);
            }
            float* drow = dout + m * ld + BNLL_NCLS + 4;
            st4(drow, make_float4(g4[0], g4[1], g4[2], g4[3]));
            st4(drow + 4, f4_zero());                              // the padding columns: exact zeros, so their weights never move
            s_nll += w * (nll * 0.25f);
            s_cov += w * (cov * 0.25f);
        }
    }
    s_nll = block_sum(s_nll, red);
    s_cov = block_sum(s_cov, red);
    unsigned int* ticket = reinterpret_cast<unsigned int*>(scratch) + 1;
    if (tid == 0) {
        float* part = scratch + 4 + 4 * blockIdx.x;
        part[0] = s_nll * inv_cnt; part[1] = s_cov * inv_cnt; part[2] = 0.f; part[3] = 0.f;
        vlg_ticket_draw(ticket, &last_sh);
    }
    if (vlg_ticket_last(&last_sh) && tid < 64) {
        float acc[2];                                               // nll, coverage
        vlg_fold_partials<2>(scratch + 4, (int)gridDim.x, tid, acc);
        if (tid == 0) {
            loss_io[0] = loss_io[0] + w_nll * acc[0];               // once: the total the loss launch before this one wrote
            loss_io[4] = acc[0]; loss_io[5] = acc[1]; loss_io[6] = 0.f; loss_io[7] = 0.f;
            *ticket = 0u;                                           // ready for the next launch
        }
    }
}

extern "C" int vlg_layout_box_nll_scratch(void) { return BNLL_SCRATCH; }

extern "C" int vlg_layout_box_nll(const float* out, int ld, const float* tgt_box, const float* valid, float* dout,
                                  float* loss_io, float* scratch, int B, int T, int N, int n_classes, float s_min, float s_max,
                                  float w_nll, void* stream) {
    if (n_classes != BNLL_NCLS || B < 1 || T < 1 || N < 1 || ld < BNLL_NCLS + 12 || (ld & 3)) return VLG_ERR_SHAPE;
    if (!(s_min < s_max) || !(s_min >= -3.0e38f) || !(s_max <= 3.0e38f)) return VLG_ERR_SHAPE;      // (NaN fails the first)
    if (!(w_nll >= 0.f) || !(w_nll <= 3.0e38f)) return VLG_ERR_SHAPE;                               // negative, inf or NaN
    if (!out || !dout || !tgt_box || !valid) return VLG_ERR_ALIGN;
    if (!vlg_aligned16(out) || !vlg_aligned16(dout) || !vlg_aligned16(tgt_box) || !vlg_aligned16(valid)) return VLG_ERR_ALIGN;
    if (!loss_io || !vlg_aligned4(loss_io) || !scratch || !vlg_aligned16(scratch)) return VLG_ERR_ALIGN;
    const int64_t M = (int64_t)B * T * N;
    int64_t blocks = (M + BNLL_BLOCK - 1) / BNLL_BLOCK;
    if (blocks > BNLL_MAX_BLOCKS) blocks = BNLL_MAX_BLOCKS;
    hipLaunchKernelGGL(layout_box_nll_kernel, dim3((unsigned)blocks), dim3(BNLL_BLOCK), 0, (hipStream_t)stream, out, ld, tgt_box,
                       valid, dout, scratch, loss_io, B, T, N, s_min, s_max, w_nll);
    return vlg_last_error();
}
