// Per-clip temporal encoder core (option attention = "clip"): block-causal softmax attention over ALL T*N tokens of a
// clip, per (clip, head) - token (t, n) attends to every slot of frames <= t; padded slots (valid == 0) are never keys,
// except for themselves.  SELF-ORACLE (the CPU specification clip_attention under oracle/): the reference has no attention at all; this is
// the "LDS-staged per-clip tiles" reading of BASELINE.json's temporal encoder, next to the per-slot default (attention.hip).
//
// Flash-style, exact fp32 on v_mfma_f32_32x32x2_f32, nothing quadratic ever leaves the chip.
//   token order   inside a clip the kernels walk tokens FRAME-major, s = t*N + n (memory row of s: (b*N + n)*T + t), so the
//                 causal structure is block-lower-triangular in s and whole 32-key tiles are either visible, hidden or (on the
//                 frame boundary / with padded slots) masked element-wise
//   forward       a block = 4 waves x 32 queries; 32-key tiles of K (row-major) and V (transposed) are staged through LDS once
//                 per block (register-prefetched one tile ahead); per tile and wave:
//                     S^T = K . Q^T          32 MFMAs   A = K rows from LDS, B = the wave's Q fragment (registers, pre-scaled by
//                                                       log2(e) / sqrt(64)); C layout: lane = query, registers = keys, so the
//                                                       online-softmax row statistics are IN-LANE reductions (+ one lane-xor-32)
//                     O  += P . V            32 MFMAs   the probability tile in C layout IS the A operand (lane = query row,
//                                                       k-slot = the register's key), B = V^T from LDS
//                 the running maximum's rescale factor lives per query LANE but scales O's query ROWS (registers): it is turned
//                 through a 128-B wave-private LDS line (1 write + 4 broadcast reads)
//   backward      two kernels, so that every gradient element has ONE owner and a fixed summation order (no atomics):
//                     dQ  (query owner)   S^T, dP^T = V . dO^T, dS^T = P (dP - delta) / 8, dQ += dS . K        96 MFMAs / tile
//                     dKV (key owner)     S, dP = dO . V^T, dV += P^T . dO, dK += dS^T . Q                      128 MFMAs / tile
//                 P is recomputed from the saved log-sum-exp (one float per query and head); delta = <dO, O> per query.
// Algorithmic work per (clip, head): N^2 T (T + 1) / 2 visible (query, key) pairs x 4 * 64 flop forward, x 2.5 that backward
// (5 products; the two-kernel backward executes 7).  Measured at (32, 16, 64), d = 256 (tools/clip_attn_bench.py, box to box
// +-4 %): forward 195-204 us = 90-94 TFLOP/s = 0.57-0.59 of the fp32 MFMA peak, backward 600-620 us = 74-76 TFLOP/s algorithmic
// (0.47-0.48; 0.66 counting the executed products); (8, 32, 64), d = 512: 0.63 / 0.52.
// Dealing the longest blocks first took the forward from 314 to 210 us and the backward from 1 076 to 647 us (a 32-tile block
// dealt last runs alone for 80 us); occupancy did the rest: the key-owner kernel held to 256 registers (two waves per SIMD
// instead of one: 647 -> 599 us), the forward to 168 (three waves per SIMD, 8 registers spilled: 210 -> 195 us).  A lazily
// updated reference maximum (rescale O only when the maximum moves by > 2^6) was measured: 213 us - the rescale is not what
// the matrix pipe waits for; not kept.
//
// bf16 storage (precision "bf16": vlg_attention_clip_{fwd,bwd}_bf16) - the same walk, classification and dealing order on
// v_mfma_f32_32x32x16_bf16, fp32 accumulation.  Precision contract:
//   inputs / outputs  qkv, out, dout, dqkv bf16; valid, lse, delta fp32 in the fp32 kernels' layouts (lse log2 domain, one value
//                     per (clip, head, query))
//   scores            S accumulated in fp32 from the bf16 q and k; the log2(e) / sqrt(64) scale applied in fp32 (Q is never
//                     pre-scaled and rounded back)
//   softmax           running max, row sum, lse and delta = <dO, O> fp32; masked keys are set to -inf BEFORE the row max, so
//                     they contribute exactly zero
//   rounding points   P rounded to bf16 (nearest even) only as the operand of P.V and P^T.dO; dS only as the operand of dS.K
//                     and dS^T.Q; O, dQ, dK, dV accumulated in fp32 and rounded once, on store
//   ownership         every gradient element has one owner, no atomics: bitwise reproducible
// Measured at (32, 16, 64), d = 256 (tools/clip_attn_bench.py --bf16, alternated with the fp32 kernels): forward 54 us = 336
// TFLOP/s, backward 155 us = 295 TFLOP/s algorithmic (0.13 / 0.12 of the 2.5 PF bf16 peak; fp32 in the same run 185 / 643 us).
#include "common.h"
#include "gemm_tile.h"

#define CHD 64          /* head dim */
#define CKT 32          /* tokens per LDS tile */
#define CQB 128         /* owner tokens per block: 4 waves x 32 */
#define CLDR 68         /* row stride of a row-major [32][64] tile (floats) */
#define CLDT 36         /* row stride of a transposed [64][32] tile */
#define CINVALID 0x10000
#define MFMA32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

__device__ __forceinline__ int64_t clip_row(int64_t b, int s, int T, int N) {
    const int t = s / N, n = s - t * N;
    return (b * N + n) * (int64_t)T + t;
}
// a key's frame, + CINVALID when it is a padded slot (valid may be NULL: none is).  A query of frame tq sees a key of frame
// code fr iff fr <= tq or the key is the query itself: s_reg = the token of the tile register, s_own = the lane's token
__device__ __forceinline__ int clip_frame_code(const float* __restrict__ valid, int64_t b, int s, int T, int N) {
    const int t = s / N, n = s - t * N;
    return t + ((valid != nullptr && valid[(b * T + t) * N + n] <= 0.f) ? CINVALID : 0);
}
// (macros, not functions: an inlined bool function compiles the || differently, and the fp32 kernels' code stays as tuned)
#define CLIP_VISIBLE(fr, tq, s_reg, s_own) ((fr) <= (tq) || (s_reg) == (s_own))
// register r of a 32x32 C/D tile, lane half h  ->  its row
__device__ __forceinline__ int clip_crow(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// Blocks are dealt in order of blockIdx.x, then .y: (clip, head) runs fastest and the LONGEST blocks come first, so a launch
// ends on short blocks instead of one 32-tile straggler.  Query owners: the last frames (they see every key) are the longest;
// key owners: the first frames (every later query sees them).
struct ClipBlock { int hh; int64_t b; };
__device__ __forceinline__ ClipBlock clip_block(int heads) { return {(int)(blockIdx.x % heads), (int64_t)(blockIdx.x / heads)}; }
__device__ __forceinline__ int clip_query_block0() { return ((int)gridDim.y - 1 - (int)blockIdx.y) * CQB; }
__device__ __forceinline__ int clip_key_block0() { return blockIdx.y * CQB; }
// query owner: the key tiles of frames <= the block's last query frame
__device__ __forceinline__ int clip_key_tiles(int q0, int nq, int N, int S) {
    const int kend = ((q0 + nq - 1) / N + 1) * N;
    return ((kend < S ? kend : S) + CKT - 1) / CKT;
}
// key owner: the first query tile holding a frame >= the block's first key frame
__device__ __forceinline__ int clip_first_query_tile(int kb0, int N) { return ((kb0 / N) * N) / CKT; }
// Tile classification of a wave's 32 queries (frames tq_min .. tq_max) against the 32-key tile at k0: HIDDEN (every key lies
// in a later frame: skipped), else VISIBLE (whole tile seen) unless ELEMENT-WISE (frame boundary inside, or padded slots)
#define CLIP_TILE_HIDDEN(k0, N, tq_max) ((k0) / (N) > (tq_max))
#define CLIP_TILE_ELEMENTWISE(valid, k0, N, tq_min) ((valid) != nullptr || ((k0) + CKT - 1) / (N) > (tq_min))
// ... and of a wave's 32 keys (first frame tk_min) against the 32-query tile at q0: hidden if every query is in an earlier frame
#define CLIP_QUERY_TILE_HIDDEN(q0, N, tk_min) (((q0) + CKT - 1) / (N) < (tk_min))
// register r of a 32x32 C/D tile, lane half h  ->  row (r & 3) + 8 (r >> 2) + 4 h: the four registers 4g .. 4g+3 are rows
// 8g + 4h .. + 3, i.e. ONE float4 at offset 8g + 4h of a 32-entry per-row table
__device__ __forceinline__ void rows16(float (&v)[16], const float* tab, int h) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 t = ld4(tab + 8 * g + 4 * h);
        v[4 * g] = t.x; v[4 * g + 1] = t.y; v[4 * g + 2] = t.z; v[4 * g + 3] = t.w;
    }
}
__device__ __forceinline__ void rows16i(int (&v)[16], const int* tab, int h) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int4 t = *reinterpret_cast<const int4*>(tab + 8 * g + 4 * h);
        v[4 * g] = t.x; v[4 * g + 1] = t.y; v[4 * g + 2] = t.z; v[4 * g + 3] = t.w;
    }
}
// one thread's share of a staged [32 tokens][64 dims] tile: token tid >> 3, float4 columns (tid & 7) and (tid & 7) + 8
struct ClipStage { float4 a, b; };
__device__ __forceinline__ ClipStage stage_load(const float* __restrict__ p, int c4) {
    ClipStage v;
    v.a = ld4(p + 4 * c4);
    v.b = ld4(p + 4 * (c4 + 8));
    return v;
}
__device__ __forceinline__ void stage_rows(float* Xs, int tok, int c4, const ClipStage& v) {
    st4(Xs + tok * CLDR + 4 * c4, v.a);
    st4(Xs + tok * CLDR + 4 * (c4 + 8), v.b);
}
__device__ __forceinline__ void stage_transposed(float* Xt, int tok, int c4, const ClipStage& v) {
    float* p = Xt + (4 * c4) * CLDT + tok;
    p[0] = v.a.x; p[CLDT] = v.a.y; p[2 * CLDT] = v.a.z; p[3 * CLDT] = v.a.w;
    p += 32 * CLDT;
    p[0] = v.b.x; p[CLDT] = v.b.y; p[2 * CLDT] = v.b.z; p[3 * CLDT] = v.b.w;
}
// D[row][col] = sum over the 64 dims of A[row][dim] B[col][dim], both operands as "X[l31][32 h + i]", i = 0 .. 31 (MFMA step i of
// lane (l31, h)): B = a register fragment, A = read from the row-major LDS tile as it is consumed (four values per ds_read_b128)
__device__ __forceinline__ f32x16 dot64_rows(const float* Xs, int l31, int h, const float (&b)[32]) {
    f32x16 c;
#pragma unroll
    for (int r = 0; r < 16; ++r) c[r] = 0.f;
    const float* p = Xs + l31 * CLDR + 32 * h;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const float4 t = ld4(p + 4 * q);
        c = MFMA32(t.x, b[4 * q], c);
        c = MFMA32(t.y, b[4 * q + 1], c);
        c = MFMA32(t.z, b[4 * q + 2], c);
        c = MFMA32(t.w, b[4 * q + 3], c);
    }
    return c;
}
// acc[dt] (rows = the A operand's rows, cols = dims 32 dt + l31) += sum over the tile's 32 tokens of a[token] Xt[dim][token]
__device__ __forceinline__ void contract32(f32x16 (&acc)[2], const float (&a)[16], const float* Xt, int l31, int h) {
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 t = ld4(Xt + (l31 + 32 * dt) * CLDT + 8 * g + 4 * h);
            acc[dt] = MFMA32(a[4 * g], t.x, acc[dt]);
            acc[dt] = MFMA32(a[4 * g + 1], t.y, acc[dt]);
            acc[dt] = MFMA32(a[4 * g + 2], t.z, acc[dt]);
            acc[dt] = MFMA32(a[4 * g + 3], t.w, acc[dt]);
        }
}
// store a C-layout tile pair (rows = 32 tokens of this wave, cols = 64 dims) to rows rowtab[0..31] of a [rows, ld] matrix
__device__ __forceinline__ void store_rows(float* __restrict__ dst, int64_t ld, const int* rowtab, int h, int l31,
                                           const f32x16 (&acc)[2]) {
    int rows[16];
    rows16i(rows, rowtab, h);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float* p = dst + rows[r] * ld + l31;
        p[0] = acc[0][r];
        p[32] = acc[1][r];
    }
}

#define CLIP_SCALE_LOG2 0.18033688011112042f    /* log2(e) / sqrt(64) */
#define CLIP_SCALE 0.125f

// ---------------------------------------------------------------------------------------------------------- forward
__global__ __launch_bounds__(256, 3) void attn_clip_fwd_kernel(const float* __restrict__ qkv, const float* __restrict__ valid,
                                                            float* __restrict__ out, float* __restrict__ lse, int T, int N, int d) {
    __shared__ __attribute__((aligned(16))) float Ks[CKT * CLDR];
    __shared__ __attribute__((aligned(16))) float Vt[CHD * CLDT];
    __shared__ __attribute__((aligned(16))) int kfr[CKT];
    __shared__ __attribute__((aligned(16))) float tr[4][32];
    __shared__ __attribute__((aligned(16))) int qrow[CQB];
    const int S = T * N, heads = d / CHD;
    const ClipBlock blk = clip_block(heads);
    const int hh = blk.hh;
    const int64_t b = blk.b;
    const int q0 = clip_query_block0();
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int nq = S - q0 < CQB ? S - q0 : CQB;
    const int64_t ld = 3 * (int64_t)d;
    if (tid < CQB) qrow[tid] = tid < nq ? (int)clip_row(b, q0 + tid, T, N) : 0;
    const bool wact = 32 * w < nq;                                   // wave-uniform (S is a multiple of 32)
    const int sq = q0 + 32 * w + l31;
    const int tq = wact ? sq / N : 0;
    const int tq_min = (q0 + 32 * w) / N, tq_max = wact ? (q0 + 32 * w + 31) / N : -1;
    float qf[32];
    if (wact) {
        const float* qp = qkv + clip_row(b, sq, T, N) * ld + hh * CHD + 32 * h;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float4 t = ld4(qp + 4 * c);
            qf[4 * c] = t.x * CLIP_SCALE_LOG2; qf[4 * c + 1] = t.y * CLIP_SCALE_LOG2;
            qf[4 * c + 2] = t.z * CLIP_SCALE_LOG2; qf[4 * c + 3] = t.w * CLIP_SCALE_LOG2;
        }
    }
    const int ntiles = clip_key_tiles(q0, nq, N, S);
    const int tok = tid >> 3, c4 = tid & 7;
    auto tile_load = [&](int j, ClipStage& kn, ClipStage& vn, int& fr) __attribute__((always_inline)) {
        const int sk = j * CKT + tok;
        const float* p = qkv + clip_row(b, sk, T, N) * ld + hh * CHD;
        kn = stage_load(p + d, c4);
        vn = stage_load(p + 2 * d, c4);
        fr = clip_frame_code(valid, b, sk, T, N);
    };
    ClipStage kn, vn;
    int frn;
    tile_load(0, kn, vn, frn);
    float m_run = -INFINITY, l_run = 0.f;
    f32x16 o[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { o[0][r] = 0.f; o[1][r] = 0.f; }
    for (int j = 0; j < ntiles; ++j) {
        __syncthreads();                                             // the previous tile is consumed
        stage_rows(Ks, tok, c4, kn);
        stage_transposed(Vt, tok, c4, vn);
        if (c4 == 0) kfr[tok] = frn;
        __syncthreads();
        if (j + 1 < ntiles) tile_load(j + 1, kn, vn, frn);           // in flight under this tile's MFMAs
        const int k0 = j * CKT;
        if (!wact || CLIP_TILE_HIDDEN(k0, N, tq_max)) continue;
        f32x16 st = dot64_rows(Ks, l31, h, qf);                      // S^T[key (r, h)][query l31], log2 domain
        if (CLIP_TILE_ELEMENTWISE(valid, k0, N, tq_min)) {
            int fr[16];
            rows16i(fr, kfr, h);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                st[r] = CLIP_VISIBLE(fr[r], tq, k0 + clip_crow(r, h), sq) ? st[r] : -INFINITY;
            }
        }
        float tmax = st[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) tmax = fmaxf(tmax, st[r]);
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
        const float m_new = fmaxf(m_run, tmax);
        const float m_use = m_new == -INFINITY ? 0.f : m_new;
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);
        float p[16], rs = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) { p[r] = __builtin_amdgcn_exp2f(st[r] - m_use); rs += p[r]; }
        rs += __shfl_xor(rs, 32);
        l_run = l_run * alpha + rs;
        m_run = m_new;
        if (__any(alpha != 1.0f)) {                                  // rescale the O rows by their query's factor
            if (h == 0) tr[w][l31] = alpha;
            __builtin_amdgcn_wave_barrier();
            float ar[16];
            rows16(ar, tr[w], h);
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int r = 0; r < 16; ++r) { o[0][r] *= ar[r]; o[1][r] *= ar[r]; }
        }
        contract32(o, p, Vt, l31, h);                                // O[query][dim] += P[query][key] V[key][dim]
    }
    if (!wact) return;
    if (h == 0) {
        tr[w][l31] = 1.0f / l_run;
        lse[((b * heads + hh) * (int64_t)S) + sq] = m_run + __builtin_amdgcn_logf(l_run);       // log2 domain
    }
    __builtin_amdgcn_wave_barrier();
    float li[16];
    rows16(li, tr[w], h);
#pragma unroll
    for (int r = 0; r < 16; ++r) { o[0][r] *= li[r]; o[1][r] *= li[r]; }
    store_rows(out + hh * CHD, d, qrow + 32 * w, h, l31, o);
}

// ------------------------------------------------------------------------------------------- backward, query owner (dQ)
__global__ __launch_bounds__(256) void attn_clip_dq_kernel(const float* __restrict__ qkv, const float* __restrict__ valid,
                                                           const float* __restrict__ out, const float* __restrict__ dout,
                                                           const float* __restrict__ lse, float* __restrict__ delta,
                                                           float* __restrict__ dqkv, int T, int N, int d) {
    __shared__ __attribute__((aligned(16))) float Ks[CKT * CLDR];
    __shared__ __attribute__((aligned(16))) float Vs[CKT * CLDR];
    __shared__ __attribute__((aligned(16))) float Kt[CHD * CLDT];
    __shared__ __attribute__((aligned(16))) int kfr[CKT];
    __shared__ __attribute__((aligned(16))) int qrow[CQB];
    const int S = T * N, heads = d / CHD;
    const ClipBlock blk = clip_block(heads);
    const int hh = blk.hh;
    const int64_t b = blk.b;
    const int q0 = clip_query_block0();
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int nq = S - q0 < CQB ? S - q0 : CQB;
    const int64_t ld = 3 * (int64_t)d;
    if (tid < CQB) qrow[tid] = tid < nq ? (int)clip_row(b, q0 + tid, T, N) : 0;
    const bool wact = 32 * w < nq;
    const int sq = q0 + 32 * w + l31;
    const int tq = wact ? sq / N : 0;
    const int tq_min = (q0 + 32 * w) / N, tq_max = wact ? (q0 + 32 * w + 31) / N : -1;
    float qf[32], dof[32];
    float lse_q = 0.f, del_q = 0.f;
    if (wact) {
        const int64_t row = clip_row(b, sq, T, N);
        const float* qp = qkv + row * ld + hh * CHD + 32 * h;
        const float* gp = dout + row * d + hh * CHD + 32 * h;
        const float* op = out + row * d + hh * CHD + 32 * h;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float4 t = ld4(qp + 4 * c), g = ld4(gp + 4 * c), y = ld4(op + 4 * c);
            qf[4 * c] = t.x * CLIP_SCALE_LOG2; qf[4 * c + 1] = t.y * CLIP_SCALE_LOG2;
            qf[4 * c + 2] = t.z * CLIP_SCALE_LOG2; qf[4 * c + 3] = t.w * CLIP_SCALE_LOG2;
            dof[4 * c] = g.x; dof[4 * c + 1] = g.y; dof[4 * c + 2] = g.z; dof[4 * c + 3] = g.w;
            del_q += g.x * y.x + g.y * y.y + g.z * y.z + g.w * y.w;
        }
        del_q += __shfl_xor(del_q, 32);                              // <dO, O> over the 64 dims of the head
        const int64_t li = (b * heads + hh) * (int64_t)S + sq;
        lse_q = lse[li];
        if (h == 0) delta[li] = del_q;                               // the key-owner kernel reads it
    }
    const int ntiles = clip_key_tiles(q0, nq, N, S);
    const int tok = tid >> 3, c4 = tid & 7;
    auto tile_load = [&](int j, ClipStage& kn, ClipStage& vn, int& fr) __attribute__((always_inline)) {
        const int sk = j * CKT + tok;
        const float* p = qkv + clip_row(b, sk, T, N) * ld + hh * CHD;
        kn = stage_load(p + d, c4);
        vn = stage_load(p + 2 * d, c4);
        fr = clip_frame_code(valid, b, sk, T, N);
    };
    ClipStage kn, vn;
    int frn;
    tile_load(0, kn, vn, frn);
    f32x16 dq[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { dq[0][r] = 0.f; dq[1][r] = 0.f; }
    for (int j = 0; j < ntiles; ++j) {
        __syncthreads();
        stage_rows(Ks, tok, c4, kn);
        stage_transposed(Kt, tok, c4, kn);
        stage_rows(Vs, tok, c4, vn);
        if (c4 == 0) kfr[tok] = frn;
        __syncthreads();
        if (j + 1 < ntiles) tile_load(j + 1, kn, vn, frn);
        const int k0 = j * CKT;
        if (!wact || CLIP_TILE_HIDDEN(k0, N, tq_max)) continue;
        float ds[16];
        {
            const f32x16 st = dot64_rows(Ks, l31, h, qf);            // S^T, log2 domain
#pragma unroll
            for (int r = 0; r < 16; ++r) ds[r] = __builtin_amdgcn_exp2f(st[r] - lse_q);      // P^T
        }
        if (CLIP_TILE_ELEMENTWISE(valid, k0, N, tq_min)) {
            int fr[16];
            rows16i(fr, kfr, h);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                ds[r] = CLIP_VISIBLE(fr[r], tq, k0 + clip_crow(r, h), sq) ? ds[r] : 0.f;
            }
        }
        {
            const f32x16 dpt = dot64_rows(Vs, l31, h, dof);          // dP^T[key][query] = <V[key], dO[query]>
#pragma unroll
            for (int r = 0; r < 16; ++r) ds[r] = ds[r] * (dpt[r] - del_q) * CLIP_SCALE;       // dS^T
        }
        contract32(dq, ds, Kt, l31, h);                              // dQ[query][dim] += dS[query][key] K[key][dim]
    }
    if (!wact) return;
    store_rows(dqkv + hh * CHD, ld, qrow + 32 * w, h, l31, dq);
}

// --------------------------------------------------------------------------------------- backward, key owner (dK, dV)
__global__ __launch_bounds__(256, 2) void attn_clip_dkv_kernel(const float* __restrict__ qkv, const float* __restrict__ valid,
                                                            const float* __restrict__ dout, const float* __restrict__ lse,
                                                            const float* __restrict__ delta, float* __restrict__ dqkv,
                                                            int T, int N, int d) {
    __shared__ __attribute__((aligned(16))) float Qs[CKT * CLDR];
    __shared__ __attribute__((aligned(16))) float Gs[CKT * CLDR];
    __shared__ __attribute__((aligned(16))) float Qt[CHD * CLDT];
    __shared__ __attribute__((aligned(16))) float Gt[CHD * CLDT];
    __shared__ __attribute__((aligned(16))) float qlse[CKT];
    __shared__ __attribute__((aligned(16))) float qdel[CKT];
    __shared__ __attribute__((aligned(16))) int qfr[CKT];
    __shared__ __attribute__((aligned(16))) int krow[CQB];
    const int S = T * N, heads = d / CHD;
    const ClipBlock blk = clip_block(heads);
    const int hh = blk.hh;
    const int64_t b = blk.b;
    const int kb0 = clip_key_block0();
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int nk = S - kb0 < CQB ? S - kb0 : CQB;
    const int64_t ld = 3 * (int64_t)d;
    if (tid < CQB) krow[tid] = tid < nk ? (int)clip_row(b, kb0 + tid, T, N) : 0;
    const bool wact = 32 * w < nk;
    const int sk = kb0 + 32 * w + l31;
    int kfr_own = 0;                                                 // this lane's key: frame (+ CINVALID if padded)
    const int tk_min = (kb0 + 32 * w) / N;
    float kf[32], vf[32];
    if (wact) {
        kfr_own = clip_frame_code(valid, b, sk, T, N);
        const float* kp = qkv + clip_row(b, sk, T, N) * ld + hh * CHD + 32 * h;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float4 t = ld4(kp + d + 4 * c), u = ld4(kp + 2 * d + 4 * c);
            kf[4 * c] = t.x * CLIP_SCALE_LOG2; kf[4 * c + 1] = t.y * CLIP_SCALE_LOG2;
            kf[4 * c + 2] = t.z * CLIP_SCALE_LOG2; kf[4 * c + 3] = t.w * CLIP_SCALE_LOG2;
            vf[4 * c] = u.x; vf[4 * c + 1] = u.y; vf[4 * c + 2] = u.z; vf[4 * c + 3] = u.w;
        }
    }
    const int jfirst = clip_first_query_tile(kb0, N);
    const int ntiles = S / CKT;
    const int tok = tid >> 3, c4 = tid & 7;
    const int64_t lbase = (b * heads + hh) * (int64_t)S;
    auto tile_load = [&](int j, ClipStage& qn, ClipStage& gn, float& ls, float& dl, int& fr) __attribute__((always_inline)) {
        const int sq = j * CKT + tok;
        const int tq = sq / N, nq_ = sq - tq * N;
        const int64_t row = (b * N + nq_) * (int64_t)T + tq;
        qn = stage_load(qkv + row * ld + hh * CHD, c4);
        gn = stage_load(dout + row * d + hh * CHD, c4);
        ls = lse[lbase + sq];
        dl = delta[lbase + sq];
        fr = tq;
    };
    ClipStage qn, gn;
    float lsn, dln;
    int frn;
    tile_load(jfirst, qn, gn, lsn, dln, frn);
    f32x16 dk[2], dv[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { dk[0][r] = 0.f; dk[1][r] = 0.f; dv[0][r] = 0.f; dv[1][r] = 0.f; }
    for (int j = jfirst; j < ntiles; ++j) {
        __syncthreads();
        stage_rows(Qs, tok, c4, qn);
        stage_transposed(Qt, tok, c4, qn);
        stage_rows(Gs, tok, c4, gn);
        stage_transposed(Gt, tok, c4, gn);
        if (c4 == 0) { qlse[tok] = lsn; qdel[tok] = dln; qfr[tok] = frn; }
        __syncthreads();
        if (j + 1 < ntiles) tile_load(j + 1, qn, gn, lsn, dln, frn);
        const int q0 = j * CKT;
        if (!wact || CLIP_QUERY_TILE_HIDDEN(q0, N, tk_min)) continue;
        float p[16], ds[16];
        {
            const f32x16 s = dot64_rows(Qs, l31, h, kf);             // S[query (r, h)][key l31], log2 domain
            float ls[16];
            rows16(ls, qlse, h);
            int fr[16];
            rows16i(fr, qfr, h);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int query = q0 + clip_crow(r, h);
                const bool ok = CLIP_VISIBLE(kfr_own, fr[r], query, sk);
                p[r] = ok ? __builtin_amdgcn_exp2f(s[r] - ls[r]) : 0.f;
            }
        }
        {
            const f32x16 dp = dot64_rows(Gs, l31, h, vf);            // dP[query][key] = <dO[query], V[key]>
            float dl[16];
            rows16(dl, qdel, h);
#pragma unroll
            for (int r = 0; r < 16; ++r) ds[r] = p[r] * (dp[r] - dl[r]) * CLIP_SCALE;
        }
        contract32(dv, p, Gt, l31, h);                               // dV[key][dim] += P[query][key] dO[query][dim]
        contract32(dk, ds, Qt, l31, h);                              // dK[key][dim] += dS[query][key] Q[query][dim]
    }
    if (!wact) return;
    store_rows(dqkv + d + hh * CHD, ld, krow + 32 * w, h, l31, dk);
    store_rows(dqkv + 2 * d + hh * CHD, ld, krow + 32 * w, h, l31, dv);
}

// ============================================================================== bf16 storage (precision = "bf16")
// The same walk, tiles, classification and dealing order on v_mfma_f32_32x32x16_bf16.  k-step s of lane (l31, h) carries
// the dims 32 h + 8 s .. + 7 of a 64-dim row, for both operands of a product over the head dim (one 16-byte LDS read).  A
// product over the 32 tokens of a tile takes the fp32 C-layout tile of the previous product as its B operand (registers
// 8s .. 8s+7 = k-step s, rounded to bf16 here and nowhere else): the A operand is then the transposed LDS image whose
// token order inside each 16-token k-slice is the C layout's row order (clip_kslice_pos), one 16-byte read per k-step.
#define CLDR16 72       /* row stride of a row-major bf16 [32][64] tile (elements): 36 dwords, conflict-free b128 rows */
#define CLDT16 40       /* row stride of a transposed bf16 [64][32] tile (elements) */
#define MFMA_BF16(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16((a), (b), (c), 0, 0, 0)

// tile token 16 s + 8 a + 4 h + c (C-layout row of register 8 s + 4 a + c, lane half h) -> position 16 s + 8 h + 4 a + c
__device__ __forceinline__ int clip_kslice_pos(int tok) { return (tok & ~12) | ((tok & 4) << 1) | ((tok & 8) >> 1); }
// one thread's share of a staged bf16 [32 tokens][64 dims] tile: token tid >> 3, dims 8 (tid & 7) .. + 7
__device__ __forceinline__ uint4 stage16_load(const bf16_t* __restrict__ p, int c8) {
    return *reinterpret_cast<const uint4*>(p + 8 * c8);
}
__device__ __forceinline__ void stage16_rows(bf16_t* Xs, int tok, int c8, uint4 v) {
    *reinterpret_cast<uint4*>(Xs + tok * CLDR16 + 8 * c8) = v;
}
__device__ __forceinline__ void stage16_transposed(bf16_t* Xt, int tok, int c8, uint4 v) {
    unsigned short* p = reinterpret_cast<unsigned short*>(Xt) + (8 * c8) * CLDT16 + clip_kslice_pos(tok);
    const unsigned u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        p[(2 * i) * CLDT16] = (unsigned short)(u[i] & 0xffffu);
        p[(2 * i + 1) * CLDT16] = (unsigned short)(u[i] >> 16);
    }
}
// a lane's 32 dims 32 h .. 32 h + 31 of one bf16 row as the four k-step fragments
__device__ __forceinline__ void frag16_load(bf16x8 (&f)[4], const bf16_t* __restrict__ p) {
#pragma unroll
    for (int s = 0; s < 4; ++s) f[s] = *reinterpret_cast<const bf16x8*>(p + 8 * s);
}
// D[row][col] = sum over the 64 dims of A[row][dim] B[col][dim]: A = row l31 of the row-major LDS tile, B = a fragment
__device__ __forceinline__ f32x16 dot64_rows16(const bf16_t* Xs, int l31, int h, const bf16x8 (&b)[4]) {
    f32x16 c;
#pragma unroll
    for (int r = 0; r < 16; ++r) c[r] = 0.f;
    const bf16_t* p = Xs + l31 * CLDR16 + 32 * h;
#pragma unroll
    for (int s = 0; s < 4; ++s) c = MFMA_BF16(*reinterpret_cast<const bf16x8*>(p + 8 * s), b[s], c);
    return c;
}
// acc[dt] (rows = dims 32 dt + crow, cols = x's lane) += sum over the tile's 32 tokens of Xt[dim][token] x[token]: x is an fp32
// C-layout tile with the tokens on its rows
__device__ __forceinline__ void contract32_16(f32x16 (&acc)[2], const float (&x)[16], const bf16_t* Xt, int l31, int h) {
    bf16x8 xb[2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) xb[s][j] = (bf16_t)x[8 * s + j];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int s = 0; s < 2; ++s)
            acc[dt] = MFMA_BF16(*reinterpret_cast<const bf16x8*>(Xt + (32 * dt + l31) * CLDT16 + 16 * s + 8 * h), xb[s], acc[dt]);
}
// store a transposed C-layout pair (lane = the token, registers = dims 32 dt + crow) to the token's row, rounded to bf16
__device__ __forceinline__ void store_cols16(bf16_t* __restrict__ dst, int h, const f32x16 (&acc)[2], float scale) {
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g)
            st4(dst + 32 * dt + 8 * g + 4 * h, make_float4(acc[dt][4 * g] * scale, acc[dt][4 * g + 1] * scale,
                                                          acc[dt][4 * g + 2] * scale, acc[dt][4 * g + 3] * scale));
}

// ----------------------------------------------------------------------------------------------------- forward, bf16
// S^T = K . Q^T (lane = query, registers = keys: row statistics in-lane), O^T += V^T . P^T (lane = query again, so the
// rescale and the final 1 / l are per-lane multiplies)
__global__ __launch_bounds__(256, 3) void attn_clip_fwd_bf16_kernel(const bf16_t* __restrict__ qkv, const float* __restrict__ valid,
                                                                 bf16_t* __restrict__ out, float* __restrict__ lse, int T, int N, int d) {
    __shared__ __attribute__((aligned(16))) bf16_t Ks[CKT * CLDR16];
    __shared__ __attribute__((aligned(16))) bf16_t Vt[CHD * CLDT16];
    __shared__ __attribute__((aligned(16))) int kfr[CKT];
    const int S = T * N, heads = d / CHD;
    const ClipBlock blk = clip_block(heads);
    const int hh = blk.hh;
    const int64_t b = blk.b;
    const int q0 = clip_query_block0();
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int nq = S - q0 < CQB ? S - q0 : CQB;
    const int64_t ld = 3 * (int64_t)d;
    const bool wact = 32 * w < nq;                                   // wave-uniform (S is a multiple of 32)
    const int sq = q0 + 32 * w + l31;
    const int tq = wact ? sq / N : 0;
    const int tq_min = (q0 + 32 * w) / N, tq_max = wact ? (q0 + 32 * w + 31) / N : -1;
    const int64_t qrow = wact ? clip_row(b, sq, T, N) : 0;
    bf16x8 qf[4];                                                    // Q as it is stored: the scale is applied to S in fp32
    if (wact) frag16_load(qf, qkv + qrow * ld + hh * CHD + 32 * h);
    const int ntiles = clip_key_tiles(q0, nq, N, S);
    const int tok = tid >> 3, c8 = tid & 7;
    auto tile_load = [&](int j, uint4& kn, uint4& vn, int& fr) __attribute__((always_inline)) {
        const int sk = j * CKT + tok;
        const bf16_t* p = qkv + clip_row(b, sk, T, N) * ld + hh * CHD;
        kn = stage16_load(p + d, c8);
        vn = stage16_load(p + 2 * d, c8);
        fr = clip_frame_code(valid, b, sk, T, N);
    };
    uint4 kn, vn;
    int frn;
    tile_load(0, kn, vn, frn);
    float m_run = -INFINITY, l_run = 0.f;
    f32x16 o[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { o[0][r] = 0.f; o[1][r] = 0.f; }
    for (int j = 0; j < ntiles; ++j) {
        __syncthreads();                                             // the previous tile is consumed
        stage16_rows(Ks, tok, c8, kn);
        stage16_transposed(Vt, tok, c8, vn);
        if (c8 == 0) kfr[tok] = frn;
        __syncthreads();
        if (j + 1 < ntiles) tile_load(j + 1, kn, vn, frn);           // in flight under this tile's MFMAs
        const int k0 = j * CKT;
        if (!wact || CLIP_TILE_HIDDEN(k0, N, tq_max)) continue;
        f32x16 st = dot64_rows16(Ks, l31, h, qf);                    // S^T[key (r, h)][query l31]
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] *= CLIP_SCALE_LOG2;       // log2 domain, fp32
        if (CLIP_TILE_ELEMENTWISE(valid, k0, N, tq_min)) {
            int fr[16];
            rows16i(fr, kfr, h);
#pragma unroll
            for (int r = 0; r < 16; ++r) st[r] = CLIP_VISIBLE(fr[r], tq, k0 + clip_crow(r, h), sq) ? st[r] : -INFINITY;
        }
        float tmax = st[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) tmax = fmaxf(tmax, st[r]);
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
        const float m_new = fmaxf(m_run, tmax);
        const float m_use = m_new == -INFINITY ? 0.f : m_new;
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);
        float p[16], rs = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) { p[r] = __builtin_amdgcn_exp2f(st[r] - m_use); rs += p[r]; }
        rs += __shfl_xor(rs, 32);
        l_run = l_run * alpha + rs;
        m_run = m_new;
        if (__any(alpha != 1.0f)) {
#pragma unroll
            for (int r = 0; r < 16; ++r) { o[0][r] *= alpha; o[1][r] *= alpha; }
        }
        contract32_16(o, p, Vt, l31, h);                             // O^T[dim][query] += V^T[dim][key] P^T[key][query]
    }
    if (!wact) return;
    if (h == 0) lse[((b * heads + hh) * (int64_t)S) + sq] = m_run + __builtin_amdgcn_logf(l_run);       // log2 domain
    store_cols16(out + qrow * d + hh * CHD, h, o, 1.0f / l_run);
}

// ------------------------------------------------------------------------------------- backward, query owner (dQ), bf16
__global__ __launch_bounds__(256, 3) void attn_clip_dq_bf16_kernel(const bf16_t* __restrict__ qkv, const float* __restrict__ valid,
                                                                const bf16_t* __restrict__ out, const bf16_t* __restrict__ dout,
                                                                const float* __restrict__ lse, float* __restrict__ delta,
                                                                bf16_t* __restrict__ dqkv, int T, int N, int d) {
    __shared__ __attribute__((aligned(16))) bf16_t Ks[CKT * CLDR16];
    __shared__ __attribute__((aligned(16))) bf16_t Vs[CKT * CLDR16];
    __shared__ __attribute__((aligned(16))) bf16_t Kt[CHD * CLDT16];
    __shared__ __attribute__((aligned(16))) int kfr[CKT];
    const int S = T * N, heads = d / CHD;
    const ClipBlock blk = clip_block(heads);
    const int hh = blk.hh;
    const int64_t b = blk.b;
    const int q0 = clip_query_block0();
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int nq = S - q0 < CQB ? S - q0 : CQB;
    const int64_t ld = 3 * (int64_t)d;
    const bool wact = 32 * w < nq;
    const int sq = q0 + 32 * w + l31;
    const int tq = wact ? sq / N : 0;
    const int tq_min = (q0 + 32 * w) / N, tq_max = wact ? (q0 + 32 * w + 31) / N : -1;
    const int64_t qrow = wact ? clip_row(b, sq, T, N) : 0;
    bf16x8 qf[4], dof[4];
    float lse_q = 0.f, del_q = 0.f;
    if (wact) {
        frag16_load(qf, qkv + qrow * ld + hh * CHD + 32 * h);
        frag16_load(dof, dout + qrow * d + hh * CHD + 32 * h);
        const bf16_t* op = out + qrow * d + hh * CHD + 32 * h;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float4 y = ld4(op + 4 * c);
            del_q += (float)dof[c >> 1][4 * (c & 1)] * y.x + (float)dof[c >> 1][4 * (c & 1) + 1] * y.y +
                     (float)dof[c >> 1][4 * (c & 1) + 2] * y.z + (float)dof[c >> 1][4 * (c & 1) + 3] * y.w;
        }
        del_q += __shfl_xor(del_q, 32);                              // <dO, O> over the 64 dims of the head, fp32
        const int64_t li = (b * heads + hh) * (int64_t)S + sq;
        lse_q = lse[li];
        if (h == 0) delta[li] = del_q;                               // the key-owner kernel reads it
    }
    const int ntiles = clip_key_tiles(q0, nq, N, S);
    const int tok = tid >> 3, c8 = tid & 7;
    auto tile_load = [&](int j, uint4& kn, uint4& vn, int& fr) __attribute__((always_inline)) {
        const int sk = j * CKT + tok;
        const bf16_t* p = qkv + clip_row(b, sk, T, N) * ld + hh * CHD;
        kn = stage16_load(p + d, c8);
        vn = stage16_load(p + 2 * d, c8);
        fr = clip_frame_code(valid, b, sk, T, N);
    };
    uint4 kn, vn;
    int frn;
    tile_load(0, kn, vn, frn);
    f32x16 dq[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { dq[0][r] = 0.f; dq[1][r] = 0.f; }
    for (int j = 0; j < ntiles; ++j) {
        __syncthreads();
        stage16_rows(Ks, tok, c8, kn);
        stage16_transposed(Kt, tok, c8, kn);
        stage16_rows(Vs, tok, c8, vn);
        if (c8 == 0) kfr[tok] = frn;
        __syncthreads();
        if (j + 1 < ntiles) tile_load(j + 1, kn, vn, frn);
        const int k0 = j * CKT;
        if (!wact || CLIP_TILE_HIDDEN(k0, N, tq_max)) continue;
        float ds[16];
        {
            const f32x16 st = dot64_rows16(Ks, l31, h, qf);          // S^T
#pragma unroll
            for (int r = 0; r < 16; ++r) ds[r] = __builtin_amdgcn_exp2f(st[r] * CLIP_SCALE_LOG2 - lse_q);      // P^T
        }
        if (CLIP_TILE_ELEMENTWISE(valid, k0, N, tq_min)) {
            int fr[16];
            rows16i(fr, kfr, h);
#pragma unroll
            for (int r = 0; r < 16; ++r) ds[r] = CLIP_VISIBLE(fr[r], tq, k0 + clip_crow(r, h), sq) ? ds[r] : 0.f;
        }
        {
            const f32x16 dpt = dot64_rows16(Vs, l31, h, dof);        // dP^T[key][query] = <V[key], dO[query]>
#pragma unroll
            for (int r = 0; r < 16; ++r) ds[r] = ds[r] * (dpt[r] - del_q) * CLIP_SCALE;       // dS^T
        }
        contract32_16(dq, ds, Kt, l31, h);                           // dQ^T[dim][query] += K^T[dim][key] dS^T[key][query]
    }
    if (!wact) return;
    store_cols16(dqkv + qrow * ld + hh * CHD, h, dq, 1.0f);
}

// --------------------------------------------------------------------------------- backward, key owner (dK, dV), bf16
// S = Q . K^T and dP = dO . V^T with the key on the lane; dV^T += dO^T . P and dK^T += Q^T . dS keep it there
__global__ __launch_bounds__(256, 2) void attn_clip_dkv_bf16_kernel(const bf16_t* __restrict__ qkv, const float* __restrict__ valid,
                                                                 const bf16_t* __restrict__ dout, const float* __restrict__ lse,
                                                                 const float* __restrict__ delta, bf16_t* __restrict__ dqkv,
                                                                 int T, int N, int d) {
    __shared__ __attribute__((aligned(16))) bf16_t Qs[CKT * CLDR16];
    __shared__ __attribute__((aligned(16))) bf16_t Gs[CKT * CLDR16];
    __shared__ __attribute__((aligned(16))) bf16_t Qt[CHD * CLDT16];
    __shared__ __attribute__((aligned(16))) bf16_t Gt[CHD * CLDT16];
    __shared__ __attribute__((aligned(16))) float qlse[CKT];
    __shared__ __attribute__((aligned(16))) float qdel[CKT];
    __shared__ __attribute__((aligned(16))) int qfr[CKT];
    const int S = T * N, heads = d / CHD;
    const ClipBlock blk = clip_block(heads);
    const int hh = blk.hh;
    const int64_t b = blk.b;
    const int kb0 = clip_key_block0();
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int nk = S - kb0 < CQB ? S - kb0 : CQB;
    const int64_t ld = 3 * (int64_t)d;
    const bool wact = 32 * w < nk;
    const int sk = kb0 + 32 * w + l31;
    const int tk_min = (kb0 + 32 * w) / N;
    const int64_t krow = wact ? clip_row(b, sk, T, N) : 0;
    int kfr_own = 0;                                                 // this lane's key: frame (+ CINVALID if padded)
    bf16x8 kf[4], vf[4];
    if (wact) {
        kfr_own = clip_frame_code(valid, b, sk, T, N);
        frag16_load(kf, qkv + krow * ld + d + hh * CHD + 32 * h);
        frag16_load(vf, qkv + krow * ld + 2 * d + hh * CHD + 32 * h);
    }
    const int jfirst = clip_first_query_tile(kb0, N);
    const int ntiles = S / CKT;
    const int tok = tid >> 3, c8 = tid & 7;
    const int64_t lbase = (b * heads + hh) * (int64_t)S;
    auto tile_load = [&](int j, uint4& qn, uint4& gn, float& ls, float& dl, int& fr) __attribute__((always_inline)) {
        const int sq = j * CKT + tok;
        const int64_t row = clip_row(b, sq, T, N);
        qn = stage16_load(qkv + row * ld + hh * CHD, c8);
        gn = stage16_load(dout + row * d + hh * CHD, c8);
        ls = lse[lbase + sq];
        dl = delta[lbase + sq];
        fr = sq / N;
    };
    uint4 qn, gn;
    float lsn, dln;
    int frn;
    tile_load(jfirst, qn, gn, lsn, dln, frn);
    f32x16 dk[2], dv[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { dk[0][r] = 0.f; dk[1][r] = 0.f; dv[0][r] = 0.f; dv[1][r] = 0.f; }
    for (int j = jfirst; j < ntiles; ++j) {
        __syncthreads();
        stage16_rows(Qs, tok, c8, qn);
        stage16_transposed(Qt, tok, c8, qn);
        stage16_rows(Gs, tok, c8, gn);
        stage16_transposed(Gt, tok, c8, gn);
        if (c8 == 0) { qlse[tok] = lsn; qdel[tok] = dln; qfr[tok] = frn; }
        __syncthreads();
        if (j + 1 < ntiles) tile_load(j + 1, qn, gn, lsn, dln, frn);
        const int q0 = j * CKT;
        if (!wact || CLIP_QUERY_TILE_HIDDEN(q0, N, tk_min)) continue;
        float p[16], ds[16];
        {
            const f32x16 s = dot64_rows16(Qs, l31, h, kf);           // S[query (r, h)][key l31]
            float ls[16];
            rows16(ls, qlse, h);
            int fr[16];
            rows16i(fr, qfr, h);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int query = q0 + clip_crow(r, h);
                const bool ok = CLIP_VISIBLE(kfr_own, fr[r], query, sk);
                p[r] = ok ? __builtin_amdgcn_exp2f(s[r] * CLIP_SCALE_LOG2 - ls[r]) : 0.f;
            }
        }
        {
            const f32x16 dp = dot64_rows16(Gs, l31, h, vf);          // dP[query][key] = <dO[query], V[key]>
            float dl[16];
            rows16(dl, qdel, h);
#pragma unroll
            for (int r = 0; r < 16; ++r) ds[r] = p[r] * (dp[r] - dl[r]) * CLIP_SCALE;
        }
        contract32_16(dv, p, Gt, l31, h);                            // dV^T[dim][key] += dO^T[dim][query] P[query][key]
        contract32_16(dk, ds, Qt, l31, h);                           // dK^T[dim][key] += Q^T[dim][query] dS[query][key]
    }
    if (!wact) return;
    store_cols16(dqkv + krow * ld + d + hh * CHD, h, dk, 1.0f);
    store_cols16(dqkv + krow * ld + 2 * d + hh * CHD, h, dv, 1.0f);
}

// ---------------------------------------------------------------------------------------------------------- C ABI
static int clip_check(int64_t B, int T, int N, int d) {
    if (B < 1 || T < 1 || N < 1 || d < CHD || (d % CHD) != 0) return VLG_ERR_SHAPE;
    const int64_t S = (int64_t)T * N;
    if ((S % CKT) != 0 || S > (1 << 20) || B * (d / CHD) >= (1ll << 31)) return VLG_ERR_SHAPE;
    if (B * S >= (1ll << 31)) return VLG_ERR_SHAPE;                  // row numbers are ints
    return 0;
}
// one block per (clip, head) x 128 owner tokens
static dim3 clip_grid(int64_t B, int T, int N, int d) {
    return dim3((unsigned)(B * (d / CHD)), (unsigned)((T * N + CQB - 1) / CQB));
}

extern "C" int vlg_attention_clip_fwd(const float* qkv, const float* valid, float* out, float* lse, int64_t B, int T, int N,
                                      int d, void* stream) {
    if (const int rc = clip_check(B, T, N, d)) return rc;
    if (!vlg_aligned16(qkv) || !vlg_aligned16(out) || !lse) return VLG_ERR_ALIGN;
    const int S = T * N;
    const dim3 grid((unsigned)(B * (d / CHD)), (unsigned)((S + CQB - 1) / CQB));
    hipLaunchKernelGGL(attn_clip_fwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, qkv, valid, out, lse, T, N, d);
    return vlg_last_error();
}

extern "C" int vlg_attention_clip_bwd(const float* qkv, const float* valid, const float* out, const float* dout,
                                      const float* lse, float* delta, float* dqkv, int64_t B, int T, int N, int d, void* stream) {
    if (const int rc = clip_check(B, T, N, d)) return rc;
    if (!vlg_aligned16(qkv) || !vlg_aligned16(out) || !vlg_aligned16(dout) || !vlg_aligned16(dqkv) || !lse || !delta) return VLG_ERR_ALIGN;
    const int S = T * N;
    const dim3 grid((unsigned)(B * (d / CHD)), (unsigned)((S + CQB - 1) / CQB));
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(attn_clip_dq_kernel, grid, dim3(256), 0, s, qkv, valid, out, dout, lse, delta, dqkv, T, N, d);
    hipLaunchKernelGGL(attn_clip_dkv_kernel, grid, dim3(256), 0, s, qkv, valid, dout, lse, delta, dqkv, T, N, d);
    return vlg_last_error();
}

extern "C" int vlg_attention_clip_fwd_bf16(const vlg_bf16* qkv_, const float* valid, vlg_bf16* out_, float* lse, int64_t B, int T,
                                           int N, int d, void* stream) {
    if (const int rc = clip_check(B, T, N, d)) return rc;
    if (!qkv_ || !out_ || !vlg_aligned16(qkv_) || !vlg_aligned16(out_) || !lse) return VLG_ERR_ALIGN;
    const bf16_t* qkv = reinterpret_cast<const bf16_t*>(qkv_);
    bf16_t* out = reinterpret_cast<bf16_t*>(out_);
    hipLaunchKernelGGL(attn_clip_fwd_bf16_kernel, clip_grid(B, T, N, d), dim3(256), 0, (hipStream_t)stream, qkv, valid, out, lse,
                       T, N, d);
    return vlg_last_error();
}

extern "C" int vlg_attention_clip_bwd_bf16(const vlg_bf16* qkv_, const float* valid, const vlg_bf16* out_, const vlg_bf16* dout_,
                                           const float* lse, float* delta, vlg_bf16* dqkv_, int64_t B, int T, int N, int d,
                                           void* stream) {
    if (const int rc = clip_check(B, T, N, d)) return rc;
    if (!qkv_ || !out_ || !dout_ || !dqkv_ || !vlg_aligned16(qkv_) || !vlg_aligned16(out_) || !vlg_aligned16(dout_) ||
        !vlg_aligned16(dqkv_) || !lse || !delta) return VLG_ERR_ALIGN;
    const bf16_t* qkv = reinterpret_cast<const bf16_t*>(qkv_);
    const bf16_t* out = reinterpret_cast<const bf16_t*>(out_);
    const bf16_t* dout = reinterpret_cast<const bf16_t*>(dout_);
    bf16_t* dqkv = reinterpret_cast<bf16_t*>(dqkv_);
    const dim3 grid = clip_grid(B, T, N, d);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(attn_clip_dq_bf16_kernel, grid, dim3(256), 0, s, qkv, valid, out, dout, lse, delta, dqkv, T, N, d);
    hipLaunchKernelGGL(attn_clip_dkv_bf16_kernel, grid, dim3(256), 0, s, qkv, valid, dout, lse, delta, dqkv, T, N, d);
    return vlg_last_error();
}
