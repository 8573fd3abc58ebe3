// Per-clip temporal encoder core (option attention = "clip"): block-causal softmax attention over ALL T*N tokens of a
// clip, per (clip, head) - token (t, n) attends to every slot of frames <= t; padded slots (valid == 0) are never keys,
// except for themselves.  SELF-ORACLE (the CPU specification clip_attention under oracle/): the reference has no attention at all; this is
// the "LDS-staged per-clip tiles" reading of BASELINE.json's temporal encoder, next to the per-slot default (attention.hip).
//
// Flash-style, nothing quadratic ever leaves the chip.  THE WALK is written once, as three kernel templates over a storage
// policy (ClipF32: exact fp32 on v_mfma_f32_32x32x2_f32; ClipBf16: bf16 storage on v_mfma_f32_32x32x16_bf16, fp32 accumulation):
//   token order   inside a clip the kernels walk tokens FRAME-major, s = t*N + n (memory row of s: (b*N + n)*T + t), so the
//                 causal structure is block-lower-triangular in s and whole 32-key tiles are either visible, hidden or (on the
//                 frame boundary / with padded slots) masked element-wise
//   forward       a block = 4 waves x 32 queries; 32-key tiles of K (row-major) and V (transposed) are staged through LDS once
//                 per block (register-prefetched one tile ahead); per tile and wave:
//                     S^T = K . Q^T          A = K rows from LDS, B = the wave's Q fragment (registers); C layout: lane = query,
//                                            registers = keys, so the online-softmax row statistics are IN-LANE reductions (+ one
//                                            lane-xor-32)
//                     O  += P . V            the probability tile in C layout is an operand as it stands, the other is V^T from LDS
//   backward      two kernels, so that every gradient element has ONE owner and a fixed summation order (no atomics, bitwise
//                 reproducible):
//                     dQ  (query owner)   S^T, dP^T = V . dO^T, dS^T = P (dP - delta) / 8, dQ += dS . K        3 products / tile
//                     dKV (key owner)     S, dP = dO . V^T, dV += P^T . dO, dK += dS^T . Q                      4 products / tile
//                 P is recomputed from the saved log-sum-exp (one float per query and head, log2 domain); delta = <dO, O> per
//                 query.  valid, lse and delta are fp32 in both storages, in the same layouts.
//   step          generation against a K/V cache, a fourth template: the forward's tile body (CLIP_FWD_TILE) for the N queries
//                 of one frame, the KEY tiles split among a block's four waves and merged in a fixed order (see the kernel)
//
// WHAT A STORAGE POLICY DECIDES (everything else - dealing order, wave activity, tile classification, the prefetch / two-barrier
// staging loop, the online softmax, lse / delta - is the templates' and exists once):
//                          ClipF32                                          ClipBf16
//   tile image in LDS      floats, row stride 68 / transposed 36            bf16, row stride 72 / transposed 40; the transposed image
//                                                                           holds each 16-token k-slice in the C layout's row order
//                                                                           (clip_kslice_pos), one 16-byte read per k-step
//   operand fragment       32 floats; 32 MFMAs per product                  4 x bf16x8: k-step s of lane (l31, h) carries the dims
//                                                                           32 h + 8 s .. + 7 (one 16-byte LDS read); 4 MFMAs per product
//   log2(e) / sqrt(64)     folded into Q in all three kernels (the query    applied to S in fp32 (Q is never pre-scaled and rounded
//                          owners' Q fragment as it is loaded, the key      back)
//                          owner's Q rows as they are staged): a score
//                          recomputed in the backward is bitwise the
//                          forward's, so P = exp2(s - lse) of a token that
//                          sees only itself is exactly 1
//   rounding points        none                                             P only as the operand of P.V and P^T.dO, dS only as the
//                                                                           operand of dS.K and dS^T.Q (nearest even, in contract32);
//                                                                           O, dQ, dK, dV accumulated in fp32, rounded once on store
//   accumulator tile       owner tokens on REGISTERS (rows), dims on        owner token on the LANE, dims on registers: the products
//                          lanes: a per-query factor lives per lane but     over the tile's tokens take the fp32 C-layout tile of the
//                          scales rows, so it is turned through a 128-B     previous product as their B operand, the factor is a
//                          wave-private LDS line (Turn: 1 write + 4         per-lane multiply and each lane stores its own row
//                          broadcast reads) and the store goes by a row
//                          table in LDS (Rows)
//   masked keys            set to -inf BEFORE the row max in both: they contribute exactly zero
//
// Algorithmic work per (clip, head): N^2 T (T + 1) / 2 visible (query, key) pairs x 4 * 64 flop forward, x 2.5 that backward
// (5 products; the two-kernel backward executes 7).
// fp32, measured at (32, 16, 64), d = 256 (tools/clip_attn_bench.py, box to box
// +-4 %): forward 195-204 us = 90-94 TFLOP/s = 0.57-0.59 of the fp32 MFMA peak, backward 600-620 us = 74-76 TFLOP/s algorithmic
// (0.47-0.48; 0.66 counting the executed products); (8, 32, 64), d = 512: 0.63 / 0.52.
// Dealing the longest blocks first took the forward from 314 to 210 us and the backward from 1 076 to 647 us (a 32-tile block
// dealt last runs alone for 80 us); occupancy did the rest: the key-owner kernel held to 256 registers (two waves per SIMD
// instead of one: 647 -> 599 us), the forward to 168 (three waves per SIMD, 8 registers spilled: 210 -> 195 us).  A lazily
// updated reference maximum (rescale O only when the maximum moves by > 2^6) was measured: 213 us - the rescale is not what
// the matrix pipe waits for; not kept.
// bf16, measured at (32, 16, 64), d = 256 (tools/clip_attn_bench.py --bf16, alternated with the fp32 kernels): forward 54 us = 336
// TFLOP/s, backward 155 us = 295 TFLOP/s algorithmic (0.13 / 0.12 of the 2.5 PF bf16 peak; fp32 in the same run 185 / 643 us).
//
// FRAME-LOCAL INSTANTIATIONS (option attention = "factored", its odd layers; vlg_attention_frame_*): the four templates take a
// compile-time flag FRAME.  false is the block-causal code above, unchanged.  true is attention INSIDE a frame - the same
// walk, the same policies, lse / delta layouts and rounding points, with three rules exchanged (stated once in Python and
// checked by brute force: tests/frame_walk.py, tests/test_frame_walk_cpu.py):
//   visibility      FRAME_VISIBLE: the key's frame code EQUALS the query's frame, or the key is the query itself.  A padded
//                   slot's code carries CINVALID as before, so it equals no frame: never a key except its own.
//   tile ranges     from the frames alone.  A query-owner block walks the key tiles from the one holding the first token of
//                   its first frame (frame_first_tile) to the one holding the last token of its last frame (clip_key_tiles,
//                   as before); a key-owner block walks the query tiles of exactly that range of ITS frames; the step walks
//                   the tiles of frame p and stages zeros for whatever they hold of other frames - it loads no row and no
//                   valid entry of another position, earlier ones included.
//   classification  FRAME_TILE_HIDDEN: none of the tile's frames is among the wave's; FRAME_TILE_ELEMENTWISE: valid is given,
//                   or the tile or the wave's own 32 tokens hold a frame boundary; whole otherwise (then both are one frame).
// Work per (clip, head): N^2 T pairs.  Every block of a frame-local launch walks the tiles of its own one or two frames, so
// there is no longest block to deal first: the launch keeps the grid and the block -> token map of the block-causal one
// ((clip, head) fastest, so the blocks resident together read neighbouring rows), and that order decides nothing.
// Measured at (32, 16, 64), d = 256 (tools/clip_attn_bench.py --frame --bf16): forward 46 us fp32 / 17 us bf16, backward 158 /
// 57 us, step 19 / 5.4 us at every p.  At N^2 T pairs these are bandwidth kernels with a short matrix body (the forward's
// ideal is 14 us of fp32 MFMA, 21 us of HBM): a block stages four tiles and each wave computes two, too short a walk for the
// prefetch to hide anything - the forward moves its bytes at 2.9 TB/s (DESIGN.md "Factored space-time attention").
#include <initializer_list>
#include "common.h"
#include "gemm_tile.h"

#define CHD 64          /* head dim */
#define CKT 32          /* tokens per LDS tile */
#define CQB 128         /* owner tokens per block: 4 waves x 32 */
#define CINVALID 0x10000
#define CLIP_SCALE_LOG2 0.18033688011112042f    /* log2(e) / sqrt(64) */
#define CLIP_SCALE 0.125f
#define MFMA32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)
#define MFMA_BF16(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16((a), (b), (c), 0, 0, 0)

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
// frame-local: the key's frame code IS the query's frame (tests/frame_walk.py: visible).  FRAME is a template constant
#define FRAME_VISIBLE(fr, tq, s_reg, s_own) ((fr) == (tq) || (s_reg) == (s_own))
#define CLIP_SEES(FRAME, fr, tq, s_reg, s_own) ((FRAME) ? FRAME_VISIBLE(fr, tq, s_reg, s_own) : CLIP_VISIBLE(fr, tq, s_reg, s_own))
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
// Frame-local (tests/frame_walk.py: first_tile, end_tile, classify).  The first tile of an owner block's walk - query owners'
// key tiles and key owners' query tiles alike - holds the first token of the block's first frame; the walk ends with
// clip_key_tiles.  A 32-token tile at k0 against a wave whose 32 owner tokens lie in frames t_min .. t_max:
__device__ __forceinline__ int frame_first_tile(int s0, int N) { return ((s0 / N) * N) / CKT; }
#define FRAME_TILE_HIDDEN(k0, N, t_min, t_max) (((k0) + CKT - 1) / (N) < (t_min) || (k0) / (N) > (t_max))
#define FRAME_TILE_ELEMENTWISE(valid, k0, N, t_min, t_max)                                                                \
    ((valid) != nullptr || (k0) / (N) != ((k0) + CKT - 1) / (N) || (t_min) != (t_max))
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

// ------------------------------------------------------------------------------------------------- storage policies
// Common vocabulary: a thread stages token tok = tid >> 3, column group c = tid & 7 of a [32 tokens][64 dims] tile; a lane
// (l31, h) of a wave holds the dims 32 h .. 32 h + 31 of its owner token as a fragment.
//   dot64       D[row][col] = sum over the 64 dims of A[row][dim] B[col][dim]: A = row l31 of a row-major LDS tile, read as it is
//               consumed, B = a fragment.  The result has the TILE's tokens on registers and the owner token on the lane.
//   contract32  acc += the product over the tile's 32 tokens of a C-layout tile x (as dot64 returns it) with a transposed LDS tile
struct ClipF32 {
    typedef float elem;
    struct Stage { float4 a, b; };                                   // float4 columns c and c + 8
    typedef float Frag[32];
    static constexpr int LDR = 68, LDT = 36;                         // row strides of the row-major / transposed tile (floats)
    static constexpr int DQ_WAVES = 1;                               // the query-owner backward's waves-per-SIMD bound (202 + 32 registers)
    struct Turn { float f[4][32]; };                                 // per wave: a per-query factor on its way from lanes to rows
    struct Rows { int row[CQB]; };                                   // the block's owner tokens -> memory rows

    __device__ static __forceinline__ void own_rows(Rows& R, int64_t b, int s0, int n, int T, int N) {
        const int tid = threadIdx.x;
        if (tid < CQB) R.row[tid] = tid < n ? (int)clip_row(b, s0 + tid, T, N) : 0;
    }
    __device__ static __forceinline__ Stage stage_load(const float* __restrict__ p, int c) {
        Stage v;
        v.a = ld4(p + 4 * c);
        v.b = ld4(p + 4 * (c + 8));
        return v;
    }
    __device__ static __forceinline__ void stage_rows(float* Xs, int tok, int c, const Stage& v) {
        st4(Xs + tok * LDR + 4 * c, v.a);
        st4(Xs + tok * LDR + 4 * (c + 8), v.b);
    }
    // ... carrying the score scale, rounded as frag_load_scored rounds it: the key owner's S = (Q scale) . K^T is then the
    // forward's S^T = K . (Q scale)^T product for product, so P = exp2(S - lse) is recomputed from the bits lse was made of
    __device__ static __forceinline__ void stage_rows_scored(float* Xs, int tok, int c, const Stage& v) {
        st4(Xs + tok * LDR + 4 * c, make_float4(v.a.x * CLIP_SCALE_LOG2, v.a.y * CLIP_SCALE_LOG2, v.a.z * CLIP_SCALE_LOG2,
                                                v.a.w * CLIP_SCALE_LOG2));
        st4(Xs + tok * LDR + 4 * (c + 8), make_float4(v.b.x * CLIP_SCALE_LOG2, v.b.y * CLIP_SCALE_LOG2, v.b.z * CLIP_SCALE_LOG2,
                                                      v.b.w * CLIP_SCALE_LOG2));
    }
    __device__ static __forceinline__ void stage_transposed(float* Xt, int tok, int c, const Stage& v) {
        float* p = Xt + (4 * c) * LDT + tok;
        p[0] = v.a.x; p[LDT] = v.a.y; p[2 * LDT] = v.a.z; p[3 * LDT] = v.a.w;
        p += 32 * LDT;
        p[0] = v.b.x; p[LDT] = v.b.y; p[2 * LDT] = v.b.z; p[3 * LDT] = v.b.w;
    }
    __device__ static __forceinline__ void frag_load(Frag& f, const float* __restrict__ p) {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float4 t = ld4(p + 4 * c);
            f[4 * c] = t.x; f[4 * c + 1] = t.y; f[4 * c + 2] = t.z; f[4 * c + 3] = t.w;
        }
    }
    // the fragment of a score product carries the scale, so a raw score IS the log2-domain score
    __device__ static __forceinline__ void frag_load_scored(Frag& f, const float* __restrict__ p) {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float4 t = ld4(p + 4 * c);
            f[4 * c] = t.x * CLIP_SCALE_LOG2; f[4 * c + 1] = t.y * CLIP_SCALE_LOG2;
            f[4 * c + 2] = t.z * CLIP_SCALE_LOG2; f[4 * c + 3] = t.w * CLIP_SCALE_LOG2;
        }
    }
    __device__ static __forceinline__ float log2_score(float s) { return s; }
    __device__ static __forceinline__ float frag_elem(const Frag& f, int i) { return f[i]; }
    // both operands as "X[l31][32 h + i]", i = 0 .. 31 (MFMA step i of lane (l31, h)); four values per ds_read_b128
    __device__ static __forceinline__ f32x16 dot64(const float* Xs, int l31, int h, const Frag& b) {
        f32x16 c;
#pragma unroll
        for (int r = 0; r < 16; ++r) c[r] = 0.f;
        const float* p = Xs + l31 * LDR + 32 * h;
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
    // x = the A operand as it stands (lane = its row, k-slot = the register's token): acc[dt] has x's lane token on ROWS,
    // the dims 32 dt + l31 on lanes
    __device__ static __forceinline__ void contract32(f32x16 (&acc)[2], const float (&x)[16], const float* Xt, int l31, int h) {
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 t = ld4(Xt + (l31 + 32 * dt) * LDT + 8 * g + 4 * h);
                acc[dt] = MFMA32(x[4 * g], t.x, acc[dt]);
                acc[dt] = MFMA32(x[4 * g + 1], t.y, acc[dt]);
                acc[dt] = MFMA32(x[4 * g + 2], t.z, acc[dt]);
                acc[dt] = MFMA32(x[4 * g + 3], t.w, acc[dt]);
            }
    }
    // acc's rows *= their owner token's factor f (one per lane l31, both halves alike)
    __device__ static __forceinline__ void rescale(Turn& U, f32x16 (&acc)[2], float f, int w, int l31, int h) {
        if (h == 0) U.f[w][l31] = f;
        __builtin_amdgcn_wave_barrier();
        float fr[16];
        rows16(fr, U.f[w], h);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[0][r] *= fr[r]; acc[1][r] *= fr[r]; }
    }
    // the wave's 32 owner tokens x 64 dims to their rows of a [rows, ld] matrix (the lane's own row is not what it holds)
    __device__ static __forceinline__ void store(const Rows& R, float* __restrict__ dst, int64_t ld, int64_t, const f32x16 (&acc)[2],
                                                 int w, int l31, int h) {
        int rows[16];
        rows16i(rows, R.row + 32 * w, h);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float* p = dst + rows[r] * ld + l31;
            p[0] = acc[0][r];
            p[32] = acc[1][r];
        }
    }
    // the generation step: a tile of 32 owner tokens on CONSECUTIVE rows from row0 of which the first n are real - the rest
    // are not stored - and a staged token that is not loaded
    __device__ static __forceinline__ void store_rows(float* __restrict__ dst, int64_t ld, int64_t row0, int n, const f32x16 (&acc)[2],
                                                      int l31, int h) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = clip_crow(r, h);
            if (row < n) {
                float* p = dst + (row0 + row) * ld + l31;
                p[0] = acc[0][r];
                p[32] = acc[1][r];
            }
        }
    }
    __device__ static __forceinline__ Stage stage_zero() {
        Stage v;
        v.a = v.b = make_float4(0.f, 0.f, 0.f, 0.f);
        return v;
    }
    // The generation step's scores.  dot64 is one chain of 64 fp32 FMAs per score: at |s| ~ 100 (peaked softmax rows) it is
    // off by a few ulp of 7.6e-6, which shows against fp64 in the few rows a step computes (as it did in vlg_attention_step,
    // which accumulates in fp64 for that reason).  So the step forms its scores on the vector unit in fp64 - the product of
    // two fp32 values is exact there - from the UNSCALED query rows Qs (row-major like Ks, the block's 32 queries) and
    // returns each as the fp32 value st nearest to it and the remainder lo: exp2(st - m) (1 + ln2 lo) is the probability of
    // the unrounded score, whatever m the online softmax subtracts.  Lane (l31, h): query l31, keys clip_crow(r, h).
    static constexpr bool STEP_EXACT = true;
    __device__ static __forceinline__ void step_scores(f32x16& st, float (&lo)[16], const float* Ks, const float* Qs, int l31, int h,
                                                       const Frag&) {
        double acc[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0;
#pragma unroll 1
        for (int c = 0; c < 8; ++c) {                                // 8 dims at a time
            const float4 qa = ld4(Qs + l31 * LDR + 8 * c), qb = ld4(Qs + l31 * LDR + 8 * c + 4);
            const double q[8] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float* kp = Ks + clip_crow(r, h) * LDR + 8 * c;
                const float4 ka = ld4(kp), kb = ld4(kp + 4);
                const double k[8] = {ka.x, ka.y, ka.z, ka.w, kb.x, kb.y, kb.z, kb.w};
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[r] = fma(k[i], q[i], acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const double s = acc[r] * 0.18033688011112042;           // log2(e) / sqrt(64)
            st[r] = (float)s;
            lo[r] = (float)(s - (double)st[r]);
        }
    }
    // ... and the remainder of a query's score with ITSELF as a key (always visible), by the same operations in the same order,
    // so it is bitwise the lo that step_scores finds for that key.  The step subtracts it from every lo of the query - a factor
    // common to all keys of a softmax row changes nothing - so that a token that sees only itself still has P exactly 1.
    __device__ static __forceinline__ float step_self_lo(const float* __restrict__ qrow, const float* __restrict__ krow) {
        double acc = 0.0;
#pragma unroll 1
        for (int c = 0; c < 8; ++c) {
            const float4 qa = ld4(qrow + 8 * c), qb = ld4(qrow + 8 * c + 4), ka = ld4(krow + 8 * c), kb = ld4(krow + 8 * c + 4);
            const double q[8] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
            const double k[8] = {ka.x, ka.y, ka.z, ka.w, kb.x, kb.y, kb.z, kb.w};
#pragma unroll
            for (int i = 0; i < 8; ++i) acc = fma(k[i], q[i], acc);
        }
        const double s = acc * 0.18033688011112042;
        return (float)(s - (double)(float)s);
    }
};

struct ClipBf16 {
    typedef bf16_t elem;
    typedef uint4 Stage;                                             // dims 8 c .. + 7
    typedef bf16x8 Frag[4];
    static constexpr int LDR = 72, LDT = 40;                         // elements; 36 dwords: conflict-free b128 rows
    static constexpr int DQ_WAVES = 3;
    struct Turn {};                                                  // the owner token is on the lane: nothing to turn, no table
    struct Rows {};

    __device__ static __forceinline__ void own_rows(Rows&, int64_t, int, int, int, int) {}
    __device__ static __forceinline__ Stage stage_load(const bf16_t* __restrict__ p, int c) {
        return *reinterpret_cast<const uint4*>(p + 8 * c);
    }
    __device__ static __forceinline__ void stage_rows(bf16_t* Xs, int tok, int c, Stage v) {
        *reinterpret_cast<uint4*>(Xs + tok * LDR + 8 * c) = v;
    }
    __device__ static __forceinline__ void stage_rows_scored(bf16_t* Xs, int tok, int c, Stage v) { stage_rows(Xs, tok, c, v); }
    // tile token 16 s + 8 a + 4 h + c (C-layout row of register 8 s + 4 a + c, lane half h) -> position 16 s + 8 h + 4 a + c
    __device__ static __forceinline__ int clip_kslice_pos(int tok) { return (tok & ~12) | ((tok & 4) << 1) | ((tok & 8) >> 1); }
    __device__ static __forceinline__ void stage_transposed(bf16_t* Xt, int tok, int c, Stage v) {
        unsigned short* p = reinterpret_cast<unsigned short*>(Xt) + (8 * c) * LDT + clip_kslice_pos(tok);
        const unsigned u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            p[(2 * i) * LDT] = (unsigned short)(u[i] & 0xffffu);
            p[(2 * i + 1) * LDT] = (unsigned short)(u[i] >> 16);
        }
    }
    __device__ static __forceinline__ void frag_load(Frag& f, const bf16_t* __restrict__ p) {
#pragma unroll
        for (int s = 0; s < 4; ++s) f[s] = *reinterpret_cast<const bf16x8*>(p + 8 * s);
    }
    // the fragment stays as stored; the scale is applied to the fp32 score
    __device__ static __forceinline__ void frag_load_scored(Frag& f, const bf16_t* __restrict__ p) { frag_load(f, p); }
    __device__ static __forceinline__ float log2_score(float s) { return s * CLIP_SCALE_LOG2; }
    __device__ static __forceinline__ float frag_elem(const Frag& f, int i) { return (float)f[i >> 3][i & 7]; }
    __device__ static __forceinline__ f32x16 dot64(const bf16_t* Xs, int l31, int h, const Frag& b) {
        f32x16 c;
#pragma unroll
        for (int r = 0; r < 16; ++r) c[r] = 0.f;
        const bf16_t* p = Xs + l31 * LDR + 32 * h;
#pragma unroll
        for (int s = 0; s < 4; ++s) c = MFMA_BF16(*reinterpret_cast<const bf16x8*>(p + 8 * s), b[s], c);
        return c;
    }
    // x = the B operand, rounded to bf16 here and nowhere else (registers 8 s .. 8 s + 7 = k-step s): acc[dt] has the dims
    // 32 dt + crow on ROWS, x's lane token on the lane
    __device__ static __forceinline__ void contract32(f32x16 (&acc)[2], const float (&x)[16], const bf16_t* Xt, int l31, int h) {
        bf16x8 xb[2];
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int j = 0; j < 8; ++j) xb[s][j] = (bf16_t)x[8 * s + j];
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int s = 0; s < 2; ++s)
                acc[dt] = MFMA_BF16(*reinterpret_cast<const bf16x8*>(Xt + (32 * dt + l31) * LDT + 16 * s + 8 * h), xb[s], acc[dt]);
    }
    __device__ static __forceinline__ void rescale(Turn&, f32x16 (&acc)[2], float f, int, int, int) {
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[0][r] *= f; acc[1][r] *= f; }
    }
    // the lane's token to its own row, rounded to bf16
    __device__ static __forceinline__ void store(const Rows&, bf16_t* __restrict__ dst, int64_t ld, int64_t row, const f32x16 (&acc)[2],
                                                 int, int, int h) {
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                st4(dst + row * ld + 32 * dt + 8 * g + 4 * h,
                    make_float4(acc[dt][4 * g], acc[dt][4 * g + 1], acc[dt][4 * g + 2], acc[dt][4 * g + 3]));
    }
    __device__ static __forceinline__ void store_rows(bf16_t* __restrict__ dst, int64_t ld, int64_t row0, int n, const f32x16 (&acc)[2],
                                                      int l31, int h) {
        if (l31 < n) store(Rows(), dst, ld, row0 + l31, acc, 0, l31, h);
    }
    __device__ static __forceinline__ Stage stage_zero() { return make_uint4(0u, 0u, 0u, 0u); }
    // the generation step's scores: the forward's (bf16 products are exact in fp32; the storage's error is far above fp32 sums)
    static constexpr bool STEP_EXACT = false;
    __device__ static __forceinline__ void step_scores(f32x16& st, float (&lo)[16], const bf16_t* Ks, const bf16_t*, int l31, int h,
                                                       const Frag& qf) {
        st = dot64(Ks, l31, h, qf);
#pragma unroll
        for (int r = 0; r < 16; ++r) { st[r] = log2_score(st[r]); lo[r] = 0.f; }
    }
    __device__ static __forceinline__ float step_self_lo(const bf16_t*, const bf16_t*) { return 0.f; }
};

// ---------------------------------------------------------------------------------------------------------- forward
// One key tile of a query owner's walk, staged as Ks (row-major K), Vt (transposed V) and kfr (the keys' frame codes): the
// scores, the mask, the online softmax and O += P . V.  The forward and the generation step share it.  It reads the walk's
// names from the scope it stands in: qf (the wave's scored Q fragment), valid, k0 (the tile's first key token), N, the
// lane's query token sq and its frame tq, the wave's first and last query frame tq_min / tq_max and the template's FRAME
// (tq_max is read by the frame-local classification alone), the running m_run / l_run / o, turn, w, l31, h.
// (a macro for the reason CLIP_VISIBLE is one: the forward's code stays as tuned)
// SCORES declares and fills st, the tile's log2-domain scores; PFIX is appended to every probability exp2(st - m): the forward
// takes the MFMA scores and no fix, the fp32 generation step exact scores with their rounding remainder (ClipF32::step_scores).
#define CLIP_SCORES_MFMA(P, Ks)                                                                                          \
        f32x16 st = P::dot64(Ks, l31, h, qf);                        /* S^T[key (r, h)][query l31] */                    \
        _Pragma("unroll") for (int r = 0; r < 16; ++r) st[r] = P::log2_score(st[r]);
#define CLIP_FWD_TILE(P, Ks, Vt, kfr, SCORES, PFIX)                                                                      \
    {                                                                                                                    \
        SCORES                                                                                                           \
        if (FRAME ? FRAME_TILE_ELEMENTWISE(valid, k0, N, tq_min, tq_max) : CLIP_TILE_ELEMENTWISE(valid, k0, N, tq_min)) {  \
            int fr[16];                                                                                                  \
            rows16i(fr, kfr, h);                                                                                         \
            _Pragma("unroll") for (int r = 0; r < 16; ++r) {                                                             \
                st[r] = CLIP_SEES(FRAME, fr[r], tq, k0 + clip_crow(r, h), sq) ? st[r] : -INFINITY;                       \
            }                                                                                                            \
        }                                                                                                                \
        float tmax = st[0];                                                                                              \
        _Pragma("unroll") for (int r = 1; r < 16; ++r) tmax = fmaxf(tmax, st[r]);                                        \
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32));                                                                        \
        const float m_new = fmaxf(m_run, tmax);                                                                          \
        const float m_use = m_new == -INFINITY ? 0.f : m_new;                                                            \
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);                                                       \
        float p[16], rs = 0.f;                                                                                           \
        _Pragma("unroll") for (int r = 0; r < 16; ++r) { p[r] = __builtin_amdgcn_exp2f(st[r] - m_use) PFIX; rs += p[r]; } \
        rs += __shfl_xor(rs, 32);                                                                                        \
        l_run = l_run * alpha + rs;                                                                                      \
        m_run = m_new;                                                                                                   \
        if (__any(alpha != 1.0f)) P::rescale(turn, o, alpha, w, l31, h);      /* O by its query's factor */              \
        P::contract32(o, p, Vt, l31, h);                             /* O[query][dim] += P[query][key] V[key][dim] */    \
    }
template <typename P, bool FRAME>
__global__ __launch_bounds__(256, 3) void attn_clip_fwd_kernel(const typename P::elem* __restrict__ qkv, const float* __restrict__ valid,
                                                            typename P::elem* __restrict__ out, float* __restrict__ lse, int T, int N, int d) {
    __shared__ __attribute__((aligned(16))) typename P::elem Ks[CKT * P::LDR];
    __shared__ __attribute__((aligned(16))) typename P::elem Vt[CHD * P::LDT];
    __shared__ __attribute__((aligned(16))) int kfr[CKT];
    __shared__ __attribute__((aligned(16))) typename P::Turn turn;
    __shared__ __attribute__((aligned(16))) typename P::Rows rows;
    const int S = T * N, heads = d / CHD;
    const ClipBlock blk = clip_block(heads);
    const int hh = blk.hh;
    const int64_t b = blk.b;
    const int q0 = clip_query_block0();
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int nq = S - q0 < CQB ? S - q0 : CQB;
    const int64_t ld = 3 * (int64_t)d;
    P::own_rows(rows, b, q0, nq, T, N);
    const bool wact = 32 * w < nq;                                   // wave-uniform (S is a multiple of 32)
    const int sq = q0 + 32 * w + l31;
    const int tq = wact ? sq / N : 0;
    const int tq_min = (q0 + 32 * w) / N, tq_max = wact ? (q0 + 32 * w + 31) / N : -1;
    const int64_t qrow = wact ? clip_row(b, sq, T, N) : 0;
    typename P::Frag qf;
    if (wact) P::frag_load_scored(qf, qkv + qrow * ld + hh * CHD + 32 * h);
    const int jfirst = FRAME ? frame_first_tile(q0, N) : 0;          // frame-local: from the block's first frame on
    const int ntiles = clip_key_tiles(q0, nq, N, S);
    const int tok = tid >> 3, c = tid & 7;
    auto tile_load = [&](int j, typename P::Stage& kn, typename P::Stage& vn, int& fr) __attribute__((always_inline)) {
        const int sk = j * CKT + tok;
        const typename P::elem* p = qkv + clip_row(b, sk, T, N) * ld + hh * CHD;
        kn = P::stage_load(p + d, c);
        vn = P::stage_load(p + 2 * d, c);
        fr = clip_frame_code(valid, b, sk, T, N);
    };
    typename P::Stage kn, vn;
    int frn;
    tile_load(jfirst, kn, vn, frn);
    float m_run = -INFINITY, l_run = 0.f;
    f32x16 o[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { o[0][r] = 0.f; o[1][r] = 0.f; }
    for (int j = jfirst; j < ntiles; ++j) {
        __syncthreads();                                             // the previous tile is consumed
        P::stage_rows(Ks, tok, c, kn);
        P::stage_transposed(Vt, tok, c, vn);
        if (c == 0) kfr[tok] = frn;
        __syncthreads();
        if (j + 1 < ntiles) tile_load(j + 1, kn, vn, frn);           // in flight under this tile's MFMAs
        const int k0 = j * CKT;
        if (!wact || (FRAME ? FRAME_TILE_HIDDEN(k0, N, tq_min, tq_max) : CLIP_TILE_HIDDEN(k0, N, tq_max))) continue;
        CLIP_FWD_TILE(P, Ks, Vt, kfr, CLIP_SCORES_MFMA(P, Ks), )
    }
    if (!wact) return;
    if (h == 0) lse[((b * heads + hh) * (int64_t)S) + sq] = m_run + __builtin_amdgcn_logf(l_run);       // log2 domain
    P::rescale(turn, o, 1.0f / l_run, w, l31, h);
    P::store(rows, out + hh * CHD, d, qrow, o, w, l31, h);
}

// ------------------------------------------------------------------------------------------- generation step (forward)
// The forward restricted to the N queries of frame pos, against the keys of frames <= pos (the K/V cache): out is compact,
// row b*N + n.  The forward's decomposition does not fit - N queries are a fraction of a 128-query block, and its one wave
// per 32 queries would walk every key tile alone - so the KEYS are split: a block = one 32-query tile of (clip, head), all
// four waves hold the same 32 queries (lanes past N repeat query N-1 and do not store) and each walks a contiguous quarter
// of the visible key tiles through tile images of its own.  The partial (m, l, O) meet in LDS: every wave forms the merged
// maximum and sum from the four (m, l) pairs in wave order, scales its O by exp2(m_w - m) / l, and wave 0 adds the four O
// in wave order and stores.  No atomics; the order is fixed by the shape, so the bits are too.
// Scores: P::step_scores - bf16 the forward's MFMA product; fp32 exact (fp64 on the vector unit, from an LDS image Qs of the
// block's unscaled queries), handed to the shared softmax as the nearest fp32 value and a remainder that corrects P.
// Tokens from (pos + 1) N on - the tail of the last key tile - belong to later frames: their rows and their valid are NOT
// read (they may hold NaN); the images get zeros and a frame code no query sees, so P = 0 meets V = 0.
// Frame-local (FRAME): the keys are the tokens of frame pos alone, kbeg <= s < kend - the walk starts at the tile holding
// kbeg, and what the first and last tile hold of OTHER frames, earlier ones included, is treated as the tail above is.
template <typename P>
struct ClipStepTiles {
    typename P::elem Ks[CKT * P::LDR];
    typename P::elem Vt[CHD * P::LDT];
    int kfr[CKT];
};
template <typename P, bool FRAME>
__global__ __launch_bounds__(256, P::STEP_EXACT ? 1 : 2) void attn_clip_step_kernel(const typename P::elem* __restrict__ qkv, const float* __restrict__ valid,
                                                             typename P::elem* __restrict__ out, int T, int N, int d, int pos,
                                                             int64_t ldo) {
    __shared__ __attribute__((aligned(16))) ClipStepTiles<P> tiles[4];
    __shared__ __attribute__((aligned(16))) float part_m[4][32];
    __shared__ __attribute__((aligned(16))) float part_l[4][32];
    __shared__ __attribute__((aligned(16))) typename P::Turn turn;
    __shared__ __attribute__((aligned(16))) typename P::elem Qs[P::STEP_EXACT ? CKT * P::LDR : 8];      // the block's unscaled queries
    static_assert(sizeof(ClipStepTiles<P>) % 16 == 0 && sizeof(tiles) >= 3 * 64 * 32 * sizeof(float), "the merge reuses the tile images");
    const int heads = d / CHD;
    const ClipBlock blk = clip_block(heads);
    const int hh = blk.hh;
    const int64_t b = blk.b;
    const int n0 = blockIdx.y * CKT;                                 // the block's first query slot
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int nlive = N - n0 < CKT ? N - n0 : CKT;
    const int64_t ld = 3 * (int64_t)d;
    const int tq = pos, tq_min = pos, tq_max = pos;
    const int sq = pos * N + n0 + (l31 < nlive ? l31 : nlive - 1);
    typename P::Frag qf;
    P::frag_load_scored(qf, qkv + clip_row(b, sq, T, N) * ld + hh * CHD + 32 * h);
    const float lo_self = P::step_self_lo(qkv + clip_row(b, sq, T, N) * ld + hh * CHD, qkv + clip_row(b, sq, T, N) * ld + d + hh * CHD);
    if (P::STEP_EXACT) {                                             // (the first barrier of the tile loop orders it; there is a tile)
        const int qt = tid >> 3;                                     // 8 threads per query row
        const int sr = pos * N + n0 + (qt < nlive ? qt : nlive - 1);
        P::stage_rows(Qs, qt, tid & 7, P::stage_load(qkv + clip_row(b, sr, T, N) * ld + hh * CHD, tid & 7));
    }
    const int kend = (pos + 1) * N;                                  // the keys: tokens s < kend
    const int kbeg = FRAME ? pos * N : 0;                            // ... frame-local: kbeg <= s
    const int jt0 = FRAME ? kbeg / CKT : 0;                          // the first tile that holds a key
    const int ntiles = (kend + CKT - 1) / CKT - jt0;
    const int jlo = jt0 + (w * ntiles) / 4, jhi = jt0 + ((w + 1) * ntiles) / 4;  // this wave's tiles; at most (ntiles + 3) / 4 of them
    typename P::elem* Ks = tiles[w].Ks;
    typename P::elem* Vt = tiles[w].Vt;
    int* kfr = tiles[w].kfr;
    const int tok = lane >> 3, c = lane & 7;                         // a lane stages the tokens tok + 8 i, column group c
    typename P::Stage kn[4], vn[4];
    int frn[4];
    auto tile_load = [&](int j) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int sk = j * CKT + tok + 8 * i;
            kn[i] = P::stage_zero();
            vn[i] = P::stage_zero();
            frn[i] = CINVALID + T;
            if (sk < kend && (!FRAME || sk >= kbeg)) {
                const typename P::elem* p = qkv + clip_row(b, sk, T, N) * ld + hh * CHD;
                kn[i] = P::stage_load(p + d, c);
                vn[i] = P::stage_load(p + 2 * d, c);
                frn[i] = clip_frame_code(valid, b, sk, T, N);
            }
        }
    };
    tile_load(jlo < jhi ? jlo : jt0 + ntiles);                       // (no tile: zeros, never staged)
    float m_run = -INFINITY, l_run = 0.f;
    f32x16 o[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { o[0][r] = 0.f; o[1][r] = 0.f; }
    const int nit = (ntiles + 3) / 4;
    for (int it = 0; it < nit; ++it) {
        const int j = jlo + it;
        __syncthreads();                                             // the previous tile is consumed
        if (j < jhi) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                P::stage_rows(Ks, tok + 8 * i, c, kn[i]);
                P::stage_transposed(Vt, tok + 8 * i, c, vn[i]);
                if (c == 0) kfr[tok + 8 * i] = frn[i];
            }
        }
        __syncthreads();
        if (j >= jhi) continue;                                      // wave-uniform
        if (j + 1 < jhi) tile_load(j + 1);                           // in flight under this tile's MFMAs
        const int k0 = j * CKT;
        CLIP_FWD_TILE(P, Ks, Vt, kfr, f32x16 st; float lo[16]; P::step_scores(st, lo, Ks, Qs, l31, h, qf);,
                      * (1.0f + 0.69314718f * (lo[r] - lo_self)))
    }
    if (h == 0) { part_m[w][l31] = m_run; part_l[w][l31] = l_run; }
    __syncthreads();                                                 // every wave is past its last tile: the images are free
    float m_all = part_m[0][l31];
#pragma unroll
    for (int v = 1; v < 4; ++v) m_all = fmaxf(m_all, part_m[v][l31]);
    const float m_use = m_all == -INFINITY ? 0.f : m_all;
    float l_all = 0.f;
#pragma unroll
    for (int v = 0; v < 4; ++v) l_all += part_l[v][l31] * __builtin_amdgcn_exp2f(part_m[v][l31] - m_use);
    P::rescale(turn, o, __builtin_amdgcn_exp2f(m_run - m_use) / l_all, w, l31, h);
    float* part_o = reinterpret_cast<float*>(tiles);                 // [3 waves][32 registers][64 lanes]
    if (w > 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            part_o[((w - 1) * 32 + r) * 64 + lane] = o[0][r];
            part_o[((w - 1) * 32 + 16 + r) * 64 + lane] = o[1][r];
        }
    }
    __syncthreads();
    if (w > 0) return;
#pragma unroll
    for (int v = 0; v < 3; ++v)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            o[0][r] += part_o[(v * 32 + r) * 64 + lane];
            o[1][r] += part_o[(v * 32 + 16 + r) * 64 + lane];
        }
    P::store_rows(out + hh * CHD, ldo, b * N + n0, nlive, o, l31, h);
}

// ------------------------------------------------------------------------------------------- backward, query owner (dQ)
template <typename P, bool FRAME>
__global__ __launch_bounds__(256, P::DQ_WAVES) void attn_clip_dq_kernel(const typename P::elem* __restrict__ qkv,
                                                                        const float* __restrict__ valid,
                                                                        const typename P::elem* __restrict__ out,
                                                                        const typename P::elem* __restrict__ dout,
                                                                        const float* __restrict__ lse, float* __restrict__ delta,
                                                                        typename P::elem* __restrict__ dqkv, int T, int N, int d) {
    __shared__ __attribute__((aligned(16))) typename P::elem Ks[CKT * P::LDR];
    __shared__ __attribute__((aligned(16))) typename P::elem Vs[CKT * P::LDR];
    __shared__ __attribute__((aligned(16))) typename P::elem Kt[CHD * P::LDT];
    __shared__ __attribute__((aligned(16))) int kfr[CKT];
    __shared__ __attribute__((aligned(16))) typename P::Rows rows;
    const int S = T * N, heads = d / CHD;
    const ClipBlock blk = clip_block(heads);
    const int hh = blk.hh;
    const int64_t b = blk.b;
    const int q0 = clip_query_block0();
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int nq = S - q0 < CQB ? S - q0 : CQB;
    const int64_t ld = 3 * (int64_t)d;
    P::own_rows(rows, b, q0, nq, T, N);
    const bool wact = 32 * w < nq;
    const int sq = q0 + 32 * w + l31;
    const int tq = wact ? sq / N : 0;
    const int tq_min = (q0 + 32 * w) / N, tq_max = wact ? (q0 + 32 * w + 31) / N : -1;
    const int64_t qrow = wact ? clip_row(b, sq, T, N) : 0;
    typename P::Frag qf, dof;
    float lse_q = 0.f, del_q = 0.f;
    if (wact) {
        P::frag_load_scored(qf, qkv + qrow * ld + hh * CHD + 32 * h);
        P::frag_load(dof, dout + qrow * d + hh * CHD + 32 * h);
        const typename P::elem* op = out + qrow * d + hh * CHD + 32 * h;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float4 y = ld4(op + 4 * i);
            del_q += P::frag_elem(dof, 4 * i) * y.x + P::frag_elem(dof, 4 * i + 1) * y.y + P::frag_elem(dof, 4 * i + 2) * y.z +
                     P::frag_elem(dof, 4 * i + 3) * y.w;
        }
        del_q += __shfl_xor(del_q, 32);                              // <dO, O> over the 64 dims of the head, fp32
        const int64_t li = (b * heads + hh) * (int64_t)S + sq;
        lse_q = lse[li];
        if (h == 0) delta[li] = del_q;                               // the key-owner kernel reads it
    }
    const int jfirst = FRAME ? frame_first_tile(q0, N) : 0;
    const int ntiles = clip_key_tiles(q0, nq, N, S);
    const int tok = tid >> 3, c = tid & 7;
    auto tile_load = [&](int j, typename P::Stage& kn, typename P::Stage& vn, int& fr) __attribute__((always_inline)) {
        const int sk = j * CKT + tok;
        const typename P::elem* p = qkv + clip_row(b, sk, T, N) * ld + hh * CHD;
        kn = P::stage_load(p + d, c);
        vn = P::stage_load(p + 2 * d, c);
        fr = clip_frame_code(valid, b, sk, T, N);
    };
    typename P::Stage kn, vn;
    int frn;
    tile_load(jfirst, kn, vn, frn);
    f32x16 dq[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { dq[0][r] = 0.f; dq[1][r] = 0.f; }
    for (int j = jfirst; j < ntiles; ++j) {
        __syncthreads();
        P::stage_rows(Ks, tok, c, kn);
        P::stage_transposed(Kt, tok, c, kn);
        P::stage_rows(Vs, tok, c, vn);
        if (c == 0) kfr[tok] = frn;
        __syncthreads();
        if (j + 1 < ntiles) tile_load(j + 1, kn, vn, frn);
        const int k0 = j * CKT;
        if (!wact || (FRAME ? FRAME_TILE_HIDDEN(k0, N, tq_min, tq_max) : CLIP_TILE_HIDDEN(k0, N, tq_max))) continue;
        float ds[16];
        {
            const f32x16 st = P::dot64(Ks, l31, h, qf);              // S^T
#pragma unroll
            for (int r = 0; r < 16; ++r) ds[r] = __builtin_amdgcn_exp2f(P::log2_score(st[r]) - lse_q);      // P^T
        }
        if (FRAME ? FRAME_TILE_ELEMENTWISE(valid, k0, N, tq_min, tq_max) : CLIP_TILE_ELEMENTWISE(valid, k0, N, tq_min)) {
            int fr[16];
            rows16i(fr, kfr, h);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                ds[r] = CLIP_SEES(FRAME, fr[r], tq, k0 + clip_crow(r, h), sq) ? ds[r] : 0.f;
            }
        }
        {
            const f32x16 dpt = P::dot64(Vs, l31, h, dof);            // dP^T[key][query] = <V[key], dO[query]>
#pragma unroll
            for (int r = 0; r < 16; ++r) ds[r] = ds[r] * (dpt[r] - del_q) * CLIP_SCALE;       // dS^T
        }
        P::contract32(dq, ds, Kt, l31, h);                           // dQ[query][dim] += dS[query][key] K[key][dim]
    }
    if (!wact) return;
    P::store(rows, dqkv + hh * CHD, ld, qrow, dq, w, l31, h);
}

// --------------------------------------------------------------------------------------- backward, key owner (dK, dV)
// S = Q . K^T and dP = dO . V^T with the key on the lane and the tile's queries on registers: lse, delta and the frame of a
// query come from 32-entry tables staged with the tile
template <typename P, bool FRAME>
__global__ __launch_bounds__(256, 2) void attn_clip_dkv_kernel(const typename P::elem* __restrict__ qkv, const float* __restrict__ valid,
                                                            const typename P::elem* __restrict__ dout, const float* __restrict__ lse,
                                                            const float* __restrict__ delta, typename P::elem* __restrict__ dqkv,
                                                            int T, int N, int d) {
    __shared__ __attribute__((aligned(16))) typename P::elem Qs[CKT * P::LDR];
    __shared__ __attribute__((aligned(16))) typename P::elem Gs[CKT * P::LDR];
    __shared__ __attribute__((aligned(16))) typename P::elem Qt[CHD * P::LDT];
    __shared__ __attribute__((aligned(16))) typename P::elem Gt[CHD * P::LDT];
    __shared__ __attribute__((aligned(16))) float qlse[CKT];
    __shared__ __attribute__((aligned(16))) float qdel[CKT];
    __shared__ __attribute__((aligned(16))) int qfr[CKT];
    __shared__ __attribute__((aligned(16))) typename P::Rows rows;
    const int S = T * N, heads = d / CHD;
    const ClipBlock blk = clip_block(heads);
    const int hh = blk.hh;
    const int64_t b = blk.b;
    const int kb0 = clip_key_block0();
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int nk = S - kb0 < CQB ? S - kb0 : CQB;
    const int64_t ld = 3 * (int64_t)d;
    P::own_rows(rows, b, kb0, nk, T, N);
    const bool wact = 32 * w < nk;
    const int sk = kb0 + 32 * w + l31;
    const int tk_min = (kb0 + 32 * w) / N, tk_max = wact ? (kb0 + 32 * w + 31) / N : -1;    // (tk_max: frame-local alone)
    const int64_t krow = wact ? clip_row(b, sk, T, N) : 0;
    int kfr_own = 0;                                                 // this lane's key: frame (+ CINVALID if padded)
    typename P::Frag kf, vf;
    if (wact) {
        kfr_own = clip_frame_code(valid, b, sk, T, N);
        P::frag_load(kf, qkv + krow * ld + d + hh * CHD + 32 * h);   // the scale rides on the Q rows (stage_rows_scored)
        P::frag_load(vf, qkv + krow * ld + 2 * d + hh * CHD + 32 * h);
    }
    const int jfirst = clip_first_query_tile(kb0, N);                // (= frame_first_tile: the block's first frame, either way)
    const int ntiles = FRAME ? clip_key_tiles(kb0, nk, N, S) : S / CKT;     // frame-local: through the block's last frame
    const int tok = tid >> 3, c = tid & 7;
    const int64_t lbase = (b * heads + hh) * (int64_t)S;
    auto tile_load = [&](int j, typename P::Stage& qn, typename P::Stage& gn, float& ls, float& dl, int& fr)
                         __attribute__((always_inline)) {
        const int sq = j * CKT + tok;
        const int64_t row = clip_row(b, sq, T, N);
        qn = P::stage_load(qkv + row * ld + hh * CHD, c);
        gn = P::stage_load(dout + row * d + hh * CHD, c);
        ls = lse[lbase + sq];
        dl = delta[lbase + sq];
        fr = sq / N;
    };
    typename P::Stage qn, gn;
    float lsn, dln;
    int frn;
    tile_load(jfirst, qn, gn, lsn, dln, frn);
    f32x16 dk[2], dv[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { dk[0][r] = 0.f; dk[1][r] = 0.f; dv[0][r] = 0.f; dv[1][r] = 0.f; }
    for (int j = jfirst; j < ntiles; ++j) {
        __syncthreads();
        P::stage_rows_scored(Qs, tok, c, qn);
        P::stage_transposed(Qt, tok, c, qn);
        P::stage_rows(Gs, tok, c, gn);
        P::stage_transposed(Gt, tok, c, gn);
        if (c == 0) { qlse[tok] = lsn; qdel[tok] = dln; qfr[tok] = frn; }
        __syncthreads();
        if (j + 1 < ntiles) tile_load(j + 1, qn, gn, lsn, dln, frn);
        const int q0 = j * CKT;
        if (!wact || (FRAME ? FRAME_TILE_HIDDEN(q0, N, tk_min, tk_max) : CLIP_QUERY_TILE_HIDDEN(q0, N, tk_min))) continue;
        float p[16], ds[16];
        {
            const f32x16 s = P::dot64(Qs, l31, h, kf);               // S[query (r, h)][key l31]
            float ls[16];
            rows16(ls, qlse, h);
            int fr[16];
            rows16i(fr, qfr, h);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int query = q0 + clip_crow(r, h);
                const bool ok = CLIP_SEES(FRAME, kfr_own, fr[r], query, sk);
                p[r] = ok ? __builtin_amdgcn_exp2f(P::log2_score(s[r]) - ls[r]) : 0.f;
            }
        }
        {
            const f32x16 dp = P::dot64(Gs, l31, h, vf);              // dP[query][key] = <dO[query], V[key]>
            float dl[16];
            rows16(dl, qdel, h);
#pragma unroll
            for (int r = 0; r < 16; ++r) ds[r] = p[r] * (dp[r] - dl[r]) * CLIP_SCALE;
        }
        P::contract32(dv, p, Gt, l31, h);                            // dV[key][dim] += P[query][key] dO[query][dim]
        P::contract32(dk, ds, Qt, l31, h);                           // dK[key][dim] += dS[query][key] Q[query][dim]
    }
    if (!wact) return;
    P::store(rows, dqkv + d + hh * CHD, ld, krow, dk, w, l31, h);
    P::store(rows, dqkv + 2 * d + hh * CHD, ld, krow, dv, w, l31, h);
}

// ---------------------------------------------------------------------------------------------------------- C ABI
static int clip_check(int64_t B, int T, int N, int d) {
    if (B < 1 || T < 1 || N < 1 || d < CHD || (d % CHD) != 0) return VLG_ERR_SHAPE;
    const int64_t S = (int64_t)T * N;
    if ((S % CKT) != 0 || S > (1 << 20) || B * (d / CHD) >= (1ll << 31)) return VLG_ERR_SHAPE;
    if (B * S >= (1ll << 31)) return VLG_ERR_SHAPE;                  // row numbers are ints
    return 0;
}
// the shape, then the pointers: every tensor is required (valid alone may be null, and is not passed here), and the token
// tensors are read and written 16 bytes at a time.  Nothing is enqueued on a refusal.
static int clip_args(int64_t B, int T, int N, int d, std::initializer_list<const void*> tensors,
                     std::initializer_list<const void*> stats) {
    if (const int rc = clip_check(B, T, N, d)) return rc;
    for (const void* p : tensors)
        if (p == nullptr || !vlg_aligned16(p)) return VLG_ERR_ALIGN;
    for (const void* p : stats)
        if (p == nullptr) return VLG_ERR_ALIGN;
    return 0;
}
// one block per (clip, head) x 128 owner tokens
static dim3 clip_grid(int64_t B, int T, int N, int d) {
    return dim3((unsigned)(B * (d / CHD)), (unsigned)((T * N + CQB - 1) / CQB));
}

template <typename P, bool FRAME>
static int clip_fwd(const typename P::elem* qkv, const float* valid, typename P::elem* out, float* lse, int64_t B, int T, int N,
                    int d, void* stream) {
    if (const int rc = clip_args(B, T, N, d, {qkv, out}, {lse})) return rc;
    hipLaunchKernelGGL((attn_clip_fwd_kernel<P, FRAME>), clip_grid(B, T, N, d), dim3(256), 0, (hipStream_t)stream, qkv, valid, out, lse,
                       T, N, d);
    return vlg_last_error();
}
template <typename P, bool FRAME>
static int clip_bwd(const typename P::elem* qkv, const float* valid, const typename P::elem* out, const typename P::elem* dout,
                    const float* lse, float* delta, typename P::elem* dqkv, int64_t B, int T, int N, int d, void* stream) {
    if (const int rc = clip_args(B, T, N, d, {qkv, out, dout, dqkv}, {lse, delta})) return rc;
    const dim3 grid = clip_grid(B, T, N, d);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL((attn_clip_dq_kernel<P, FRAME>), grid, dim3(256), 0, s, qkv, valid, out, dout, lse, delta, dqkv, T, N, d);
    hipLaunchKernelGGL((attn_clip_dkv_kernel<P, FRAME>), grid, dim3(256), 0, s, qkv, valid, dout, lse, delta, dqkv, T, N, d);
    return vlg_last_error();
}

// one block per (clip, head) x 32 queries of frame p.  The pointers: 16 bytes fp32, 8 bytes bf16 (its stores are 8 bytes wide,
// so its rows must keep that: ldo a multiple of 4 elements)
template <typename P, bool FRAME>
static int clip_step(const typename P::elem* qkv, const float* valid, typename P::elem* o, int64_t B, int T, int N, int d, int p,
                     int64_t ldo, void* stream) {
    if (const int rc = clip_check(B, T, N, d)) return rc;
    if (p < 0 || p >= T || ldo < d) return VLG_ERR_SHAPE;
    const bool wide = sizeof(typename P::elem) == 4;
    for (const void* t : {(const void*)qkv, (const void*)o})
        if (t == nullptr || !(wide ? vlg_aligned16(t) : vlg_aligned8(t))) return VLG_ERR_ALIGN;
    if (!wide && (ldo % 4) != 0) return VLG_ERR_ALIGN;
    hipLaunchKernelGGL((attn_clip_step_kernel<P, FRAME>), dim3((unsigned)(B * (d / CHD)), (unsigned)((N + CKT - 1) / CKT)), dim3(256), 0,
                       (hipStream_t)stream, qkv, valid, o, T, N, d, p, ldo);
    return vlg_last_error();
}

// This file is compiled twice: as itself it instantiates the block-causal kernels, and through attention_frame.hip
// (VLG_ATTENTION_FRAME_TU) the frame-local ones.  Two translation units, because the instantiations of one unit share the
// module-wide lowering of their LDS variables: with the frame-local key-owner kernel beside it, the block-causal one came
// out with a different prologue.  Apart, the block-causal code objects are instruction for instruction what they were.
#ifndef VLG_ATTENTION_FRAME_TU
extern "C" int vlg_attention_clip_step(const float* qkv, const float* valid, float* o, int64_t B, int T, int N, int d, int p,
                                       int64_t ldo, void* stream) {
    return clip_step<ClipF32, false>(qkv, valid, o, B, T, N, d, p, ldo, stream);
}
extern "C" int vlg_attention_clip_step_bf16(const vlg_bf16* qkv, const float* valid, vlg_bf16* o, int64_t B, int T, int N, int d,
                                            int p, int64_t ldo, void* stream) {
    return clip_step<ClipBf16, false>(reinterpret_cast<const bf16_t*>(qkv), valid, reinterpret_cast<bf16_t*>(o), B, T, N, d, p, ldo, stream);
}
extern "C" int vlg_attention_clip_fwd(const float* qkv, const float* valid, float* out, float* lse, int64_t B, int T, int N,
                                      int d, void* stream) {
    return clip_fwd<ClipF32, false>(qkv, valid, out, lse, B, T, N, d, stream);
}
extern "C" int vlg_attention_clip_bwd(const float* qkv, const float* valid, const float* out, const float* dout,
                                      const float* lse, float* delta, float* dqkv, int64_t B, int T, int N, int d, void* stream) {
    return clip_bwd<ClipF32, false>(qkv, valid, out, dout, lse, delta, dqkv, B, T, N, d, stream);
}
extern "C" int vlg_attention_clip_fwd_bf16(const vlg_bf16* qkv, const float* valid, vlg_bf16* out, float* lse, int64_t B, int T,
                                           int N, int d, void* stream) {
    return clip_fwd<ClipBf16, false>(reinterpret_cast<const bf16_t*>(qkv), valid, reinterpret_cast<bf16_t*>(out), lse, B, T, N, d, stream);
}
extern "C" int vlg_attention_clip_bwd_bf16(const vlg_bf16* qkv, const float* valid, const vlg_bf16* out, const vlg_bf16* dout,
                                           const float* lse, float* delta, vlg_bf16* dqkv, int64_t B, int T, int N, int d,
                                           void* stream) {
    return clip_bwd<ClipBf16, false>(reinterpret_cast<const bf16_t*>(qkv), valid, reinterpret_cast<const bf16_t*>(out),
                              reinterpret_cast<const bf16_t*>(dout), lse, delta, reinterpret_cast<bf16_t*>(dqkv), B, T, N, d, stream);
}
#else
// frame-local attention (attention = "factored", odd layers): the argument lists and the host front end of the entries above
extern "C" int vlg_attention_frame_step(const float* qkv, const float* valid, float* o, int64_t B, int T, int N, int d, int p,
                                       int64_t ldo, void* stream) {
    return clip_step<ClipF32, true>(qkv, valid, o, B, T, N, d, p, ldo, stream);
}
extern "C" int vlg_attention_frame_step_bf16(const vlg_bf16* qkv, const float* valid, vlg_bf16* o, int64_t B, int T, int N, int d,
                                            int p, int64_t ldo, void* stream) {
    return clip_step<ClipBf16, true>(reinterpret_cast<const bf16_t*>(qkv), valid, reinterpret_cast<bf16_t*>(o), B, T, N, d, p, ldo, stream);
}
extern "C" int vlg_attention_frame_fwd(const float* qkv, const float* valid, float* out, float* lse, int64_t B, int T, int N,
                                      int d, void* stream) {
    return clip_fwd<ClipF32, true>(qkv, valid, out, lse, B, T, N, d, stream);
}
extern "C" int vlg_attention_frame_bwd(const float* qkv, const float* valid, const float* out, const float* dout,
                                      const float* lse, float* delta, float* dqkv, int64_t B, int T, int N, int d, void* stream) {
    return clip_bwd<ClipF32, true>(qkv, valid, out, dout, lse, delta, dqkv, B, T, N, d, stream);
}
extern "C" int vlg_attention_frame_fwd_bf16(const vlg_bf16* qkv, const float* valid, vlg_bf16* out, float* lse, int64_t B, int T,
                                           int N, int d, void* stream) {
    return clip_fwd<ClipBf16, true>(reinterpret_cast<const bf16_t*>(qkv), valid, reinterpret_cast<bf16_t*>(out), lse, B, T, N, d, stream);
}
extern "C" int vlg_attention_frame_bwd_bf16(const vlg_bf16* qkv, const float* valid, const vlg_bf16* out, const vlg_bf16* dout,
                                           const float* lse, float* delta, vlg_bf16* dqkv, int64_t B, int T, int N, int d,
                                           void* stream) {
    return clip_bwd<ClipBf16, true>(reinterpret_cast<const bf16_t*>(qkv), valid, reinterpret_cast<const bf16_t*>(out),
                              reinterpret_cast<const bf16_t*>(dout), lse, delta, reinterpret_cast<bf16_t*>(dqkv), B, T, N, d, stream);
}
#endif
