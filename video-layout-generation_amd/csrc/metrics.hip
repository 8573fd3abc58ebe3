// Validation metrics of the layout-token model: one pass over head outputs that ADDS class accuracy, top-k accuracy, the
// confusion matrix, IoU statistics and the NLL / IoU / box-L1 sums of its tokens to a running record in device memory
// (HBM-bound: one ld-float row + 28-32 bytes of targets per token in, nothing per token out).  The host reads the record
// once per validation pass or rollout (vlg/metrics.py).
//
// Definition (include/vlg_hip.h repeats it; tests/metrics_ref.py restates it in fp64).  Token m = (b*N + n)*T + t of `out`
// is scored against src = (b*tgt_T + t0 + t)*N + n of the targets:
//   scored      (valid == NULL or valid[src] != 0) and 0 <= tgt_class[src] < C; anything else: UNSCORED += 1 and the
//               token's outputs are not examined (a padded slot may hold NaN)
//   non-finite  a scored token with inf or NaN among its C + 4 outputs: NONFINITE += 1, nothing else
//   otherwise   SCORED += 1;  pred = first maximum of the logits (vlg_layout_decode at temperature 0);
//               TOP1 += (pred == tgt);  CONF[tgt*C + pred] += 1;
//               rank = #{c: l[c] > l[tgt]} + #{c < tgt: l[c] == l[tgt]} (decode's tie order);  TOPK += (rank < top_k);
//               p = sigmoid(raw);  iou = IoU(p, tgt_box) in fp32, the formula and iou_eps of csrc/loss.hip;
//               IOU_HIT += (iou >= iou_thr);  BOTH_HIT += (pred == tgt and iou >= iou_thr);
//               sums (fp32 per token, accumulated in double):  NLL += logf(sum exp(l - max)) + max - l[tgt];
//               IOU += iou;  BOX_L1 += mean_k |p_k - tgt_k|;  IOU_BY_CLASS[tgt] += iou
//
// A block of 256 threads owns 128 tokens at a time (csrc/loss.hip's shape): their rows are staged through LDS with
// coalesced 16-B loads of the ceil((C+4)/4) float4 that hold data, lane t < 128 then scores token t from its LDS row.
// C is a run-time value, so the row stride is too: 4 * (F4 | 1) floats, an ODD number of 16-B slots, so the 16 lanes of a
// ds_read_b128 group (banks (a/4) % 64 = 16 slots) hit 16 distinct slots for every C (28 floats at C = 20, as loss.hip).
// Counts: the confusion matrix is a per-block LDS histogram (integer LDS atomics), the seven scalar counts are summed per
// wavefront by shuffles and per block by LDS atomics; non-zero bins leave as 64-bit integer atomics.  Integer addition
// commutes: every count is exact whatever the schedule.
// Sums: no floating-point atomics.  Thread (slot s = tid % 32, group g = tid / 32) adds, in token order, the values of
// slot s of tokens 16g .. 16g+15 of every pass to ONE double; the 8 groups are added in group order, and the block's 32
// sums leave as one partial row of scratch.  The LAST block to finish (an integer ticket in scratch, which it resets, as
// loss.hip) adds the partial rows in the same (group = block % 8, then group order) pattern and adds the totals to `sums`.
// The block count follows from B*T*N alone, so the same call on the same record gives the same bits.
#include "common.h"
#include <float.h>

#define MET_BLOCK 256
#define MET_TOK 128                  /* tokens per block pass */
#define MET_MAX_BLOCKS 256           /* nothing is written per token: one block per CU keeps the partial fold short */
#define MET_MAX_OUT 32               /* decode's limit on C + 4 */
#define MET_MAX_C (MET_MAX_OUT - 4)
#define MET_MAX_F4 (MET_MAX_OUT / 4)
#define MET_ROWF (4 * (MET_MAX_F4 | 1))                /* largest LDS row stride, floats */
#define MET_NV (MET_TOK * MET_MAX_F4 / MET_BLOCK)      /* staged float4 per thread, at most */
#define MET_SLOTS 32                 /* double sums per block: VLG_MET_IOU_BY_CLASS + C <= 32 */
#define MET_GROUPS (MET_BLOCK / MET_SLOTS)
#define MET_GTOK (MET_TOK / MET_GROUPS)
#define MET_FOLD (MET_MAX_BLOCKS / MET_GROUPS)         /* = 32: partial rows a thread of the last block has in flight */
#define MET_NCNT 7                  /* scalar counts: VLG_MET_SCORED .. VLG_MET_UNSCORED */

// scratch layout (8-byte slots): [0] = ticket (low 4 bytes, zero between launches); [2 + 32*b + s] = sum s of block b
#define MET_SCRATCH (2 + MET_SLOTS * MET_MAX_BLOCKS)

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the 8 group sums of slot s, added in group order by the first 32 threads; result valid in threads < MET_SLOTS
__device__ __forceinline__ double met_fold(double acc, double (*dred)[MET_SLOTS], int tid) {
    dred[tid / MET_SLOTS][tid % MET_SLOTS] = acc;
    __syncthreads();
    double tot = 0.0;
    if (tid < MET_SLOTS)
        for (int g = 0; g < MET_GROUPS; ++g) tot += dred[g][tid];
    __syncthreads();
    return tot;
}

__global__ __launch_bounds__(MET_BLOCK) void layout_metrics_kernel(
    const float* __restrict__ out, int ld, const int64_t* __restrict__ tgt_class, const float* __restrict__ tgt_box,
    const float* __restrict__ valid, int tgt_T, int t0, unsigned long long* __restrict__ counts,
    double* __restrict__ sums, double* __restrict__ partials, unsigned int* __restrict__ ticket, int B, int T, int N,
    int C, int top_k, float iou_thr, float iou_eps) {
    __shared__ __attribute__((aligned(16))) float rows[MET_TOK * MET_ROWF];
    __shared__ int hist[MET_MAX_C * MET_MAX_C];
    __shared__ int cnt_sh[8];
    __shared__ int tok_cls[MET_TOK];                 // target class of a token that reached the sums, else -1
    __shared__ float tok_val[3][MET_TOK];            // its NLL, IoU, box L1
    __shared__ double dred[MET_GROUPS][MET_SLOTS];
    __shared__ int last_sh;
    const int64_t M = (int64_t)B * T * N;
    const int tid = threadIdx.x;
    const int n_out = C + 4, F4 = (n_out + 3) >> 2, C4 = (C + 3) >> 2, stride = 4 * (F4 | 1), nf4 = MET_TOK * F4;
    for (int i = tid; i < C * C; i += MET_BLOCK) hist[i] = 0;
    if (tid < 8) cnt_sh[tid] = 0;
    int cnt[MET_NCNT] = {0, 0, 0, 0, 0, 0, 0};
    double acc = 0.0;
    const int slot = tid % MET_SLOTS, grp = tid / MET_SLOTS;
    for (int64_t m0 = (int64_t)blockIdx.x * MET_TOK; m0 < M; m0 += (int64_t)gridDim.x * MET_TOK) {
        // ---- this pass's rows and targets, all requested before the first use
        float4 stage[MET_NV];
#pragma unroll
        for (int i = 0; i < MET_NV; ++i) {
            const int f = tid + i * MET_BLOCK, tok = f / F4, c = f - tok * F4;
            stage[i] = (f < nf4 && m0 + tok < M) ? ld4(out + (m0 + tok) * ld + 4 * c) : f4_zero();
        }
        const int64_t m = m0 + tid;
        const bool mine = tid < MET_TOK && m < M;
        bool scored = false;
        int tgt = 0;
        float4 tb = f4_zero();
        if (mine) {
            const int t = (int)(m % T);
            const int64_t bn = m / T;
            const int n = (int)(bn % N);
            const int64_t b = bn / N;
            const int64_t src = (b * tgt_T + t0 + t) * N + n;
            const float w = valid != nullptr ? valid[src] : 1.0f;
            const int64_t cls = tgt_class[src];
            tb = ld4(tgt_box + src * 4);
            scored = w != 0.f && cls >= 0 && cls < C;
            tgt = scored ? (int)cls : 0;
        }
#pragma unroll
        for (int i = 0; i < MET_NV; ++i) {
            const int f = tid + i * MET_BLOCK, tok = f / F4, c = f - tok * F4;
            if (f < nf4) st4(rows + tok * stride + 4 * c, stage[i]);
        }
        if (tid < MET_TOK) tok_cls[tid] = -1;
        __syncthreads();
        if (mine && !scored) ++cnt[VLG_MET_UNSCORED];
        if (mine && scored) {
            const float* row = rows + tid * stride;
            bool fin = true;
            float mx = 0.f;
            int pred = 0;
            for (int c4 = 0; c4 < F4; ++c4) {
                const float4 q = ld4(row + 4 * c4);
                const float e[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c = 4 * c4 + j;
                    if (c < n_out) fin = fin && fabsf(e[j]) <= FLT_MAX;
                    if (c < C && (c == 0 || e[j] > mx)) { mx = e[j]; pred = c; }     // first maximum
                }
            }
            if (!fin) {
                ++cnt[VLG_MET_NONFINITE];
            } else {
                const float lt = row[tgt];
                float se = 0.f;
                int rank = 0;
                for (int c4 = 0; c4 < C4; ++c4) {
                    const float4 q = ld4(row + 4 * c4);
                    const float e[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int c = 4 * c4 + j;
                        if (c < C) {
                            se += expf(e[j] - mx);
                            rank += (e[j] > lt || (e[j] == lt && c < tgt)) ? 1 : 0;
                        }
                    }
                }
                const float nll = logf(se) + mx - lt;
                // boxes: p = sigmoid(raw) as (cx, cy, w, h); IoU of axis-aligned boxes as csrc/loss.hip
                const float tg[4] = {tb.x, tb.y, tb.z, tb.w};
                float p[4], l1 = 0.f;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    p[k] = 1.0f / (1.0f + expf(-row[C + k]));
                    l1 += fabsf(p[k] - tg[k]);
                }
                l1 *= 0.25f;
                const float ax1 = p[0] - 0.5f * p[2], ax2 = p[0] + 0.5f * p[2];
                const float ay1 = p[1] - 0.5f * p[3], ay2 = p[1] + 0.5f * p[3];
                const float bx1 = tg[0] - 0.5f * tg[2], bx2 = tg[0] + 0.5f * tg[2];
                const float by1 = tg[1] - 0.5f * tg[3], by2 = tg[1] + 0.5f * tg[3];
                const float iw = fmaxf(fminf(ax2, bx2) - fmaxf(ax1, bx1), 0.f);
                const float ih = fmaxf(fminf(ay2, by2) - fmaxf(ay1, by1), 0.f);
                const float inter = iw * ih;
                const float uni = p[2] * p[3] + tg[2] * tg[3] - inter;
                const float iou = inter / (uni + iou_eps);
                const bool top1 = pred == tgt, hit = iou >= iou_thr;
                ++cnt[VLG_MET_SCORED];
                cnt[VLG_MET_TOP1] += top1 ? 1 : 0;
                cnt[VLG_MET_TOPK] += rank < top_k ? 1 : 0;
                cnt[VLG_MET_IOU_HIT] += hit ? 1 : 0;
                cnt[VLG_MET_BOTH_HIT] += (top1 && hit) ? 1 : 0;
                atomicAdd(&hist[tgt * C + pred], 1);
                tok_cls[tid] = tgt;
                tok_val[0][tid] = nll; tok_val[1][tid] = iou; tok_val[2][tid] = l1;
            }
        }
        __syncthreads();
        // ---- slot `slot` of this group's 16 tokens, in token order
        for (int i = grp * MET_GTOK; i < (grp + 1) * MET_GTOK; ++i) {
            const int c = tok_cls[i];
            if (c >= 0) {
                const float v = slot < 3 ? tok_val[slot][i] : (slot - VLG_MET_IOU_BY_CLASS == c ? tok_val[1][i] : 0.f);
                acc += (double)v;
            }
        }
        __syncthreads();                          // rows and token values are free for the next pass
    }
    // ---- counts: wavefront, block (LDS atomics), record (64-bit atomics; zeros add nothing)
#pragma unroll
    for (int k = 0; k < MET_NCNT; ++k) {
        const int v = wave_sum_i(cnt[k]);
        if ((tid & 63) == 0 && v != 0) atomicAdd(&cnt_sh[k], v);
    }
    const double tot = met_fold(acc, dred, tid);     // (its barriers also order cnt_sh)
    // ---- sums: publish the block's partial row (agent scope), take a ticket; the last block sees every row (the protocol:
    // vlg_ticket_draw / vlg_ticket_last, common.h).  This comes BEFORE the count atomics: the fence then waits for one
    // store, and the atomics drain while the last block folds
    if (tid < MET_SLOTS) {
        partials[(int64_t)blockIdx.x * MET_SLOTS + tid] = tot;
        __threadfence();
    }
    __syncthreads();
    if (tid == 0) vlg_ticket_draw(ticket, &last_sh);
    if (tid < MET_NCNT && cnt_sh[tid] != 0) atomicAdd(counts + tid, (unsigned long long)cnt_sh[tid]);
    for (int i = tid; i < C * C; i += MET_BLOCK)
        if (hist[i] != 0) atomicAdd(counts + VLG_MET_CONF + i, (unsigned long long)hist[i]);
    if (vlg_ticket_last(&last_sh)) {
        // group g adds rows g, g + 8, ... in increasing order; the record's own value and all the rows a thread adds at
        // up to 256 blocks are requested before the first add (one trip to memory instead of one per row)
        const bool own = tid < VLG_MET_IOU_BY_CLASS + C;
        const double before = own ? sums[tid] : 0.0;
        double a = 0.0;
        const int nb = (int)gridDim.x;
        for (int b0 = grp; b0 < nb; b0 += MET_GROUPS * MET_FOLD) {
            double v[MET_FOLD];
#pragma unroll
            for (int u = 0; u < MET_FOLD; ++u) {
                const int b = b0 + u * MET_GROUPS;
                v[u] = b < nb ? partials[(int64_t)b * MET_SLOTS + slot] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < MET_FOLD; ++u) a += v[u];
        }
        const double all = met_fold(a, dred, tid);
        if (own) sums[tid] = before + all;
        if (tid == 0) *ticket = 0u;                                    // ready for the next launch
    }
}

extern "C" int vlg_layout_metrics_counts(int n_classes) { return VLG_MET_CONF + n_classes * n_classes; }
extern "C" int vlg_layout_metrics_sums(int n_classes) { return VLG_MET_IOU_BY_CLASS + n_classes; }
extern "C" int vlg_layout_metrics_scratch(void) { return MET_SCRATCH; }

extern "C" int vlg_layout_metrics(const float* out, int ld, const int64_t* tgt_class, const float* tgt_box,
                                  const float* valid, int tgt_T, int t0, int64_t* counts, double* sums, void* scratch,
                                  int B, int T, int N, int n_classes, int top_k, float iou_thr, float iou_eps,
                                  void* stream) {
    if (n_classes < 1 || n_classes + 4 > MET_MAX_OUT || top_k < 1 || top_k > n_classes) return VLG_ERR_SHAPE;
    if (!(fabsf(iou_thr) <= FLT_MAX)) return VLG_ERR_SHAPE;                             // inf or NaN
    if (B < 1 || T < 1 || N < 1 || t0 < 0 || (int64_t)t0 + T > tgt_T) return VLG_ERR_SHAPE;
    if (ld < n_classes + 4 || (ld & 3)) return VLG_ERR_SHAPE;
    const int64_t M = (int64_t)B * T * N;
    if (M > (1LL << 38)) return VLG_ERR_SHAPE;                                          // a block's counts are 32-bit
    if (!out || !tgt_box || !scratch || !sums || !tgt_class || !counts) return VLG_ERR_ALIGN;
    if (!vlg_aligned16(out) || !vlg_aligned16(tgt_box) || !vlg_aligned16(scratch) || !vlg_aligned8(sums) ||
        !vlg_aligned8(tgt_class) || !vlg_aligned8(counts) || !vlg_aligned4(valid)) return VLG_ERR_ALIGN;
    int64_t blocks = (M + MET_TOK - 1) / MET_TOK;
    if (blocks > MET_MAX_BLOCKS) blocks = MET_MAX_BLOCKS;
    double* partials = reinterpret_cast<double*>(scratch) + 2;
    hipLaunchKernelGGL(layout_metrics_kernel, dim3((unsigned)blocks), dim3(MET_BLOCK), 0, (hipStream_t)stream, out, ld,
                       tgt_class, tgt_box, valid, tgt_T, t0, reinterpret_cast<unsigned long long*>(counts), sums, partials,
                       reinterpret_cast<unsigned int*>(scratch), B, T, N, n_classes, top_k, iou_thr, iou_eps);
    return vlg_last_error();
}
