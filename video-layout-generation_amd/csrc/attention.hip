// Temporal encoder core: causal softmax attention along T per (clip, slot, head).
//
// Rows are in the internal order m = (b*N + n)*T + t, so the T frames of one slot are T consecutive rows of qkv [rows, 3d],
// and one wavefront owns one (slot, head): the T x 64 tiles q, k, v of that head.  Algorithmic bytes per (slot, head):
// fwd 4*T*64*4 (q,k,v in, o out); bwd 7*T*64*4 (q,k,v,do in; dq,dk,dv out).  4*T*T*64 flop per head is little next to the
// 1 KB/row streamed, so the kernels are meant to be HBM-bound.  Nothing is saved for backward: P is recomputed from q, k
// (cheaper than 4*T*T bytes of traffic).  Three schemes, each written once over the storage type EL (fp32 or bf16;
// the arithmetic is fp32 in both):
//   T = 4, 8      attn_fwd_kernel<T> / attn_bwd_kernel<T>: the tiles are staged in LDS (row stride 68 floats: 16-B aligned
//                 and float4-conflict-free), the T x T scores are computed with lanes laid out (row i, column group), each
//                 softmax row is reduced with wavefront shuffles over the LPR lanes that share it.  All fp32 VALU work.
//   T = 16, 32    attn_mfma_fwd_body<NB> / attn_mfma_bwd_body<NB>: NB = T / 16 query blocks against 16 x 16 score tiles
//                 on the fp32 matrix cores, operands in registers (below).
//   one query     attn_step_kernel<T>: generation against the cache (at the end of the file).
#include <initializer_list>
#include <type_traits>

#include "common.h"

#define HD 64
#define LDT 68     // LDS row stride of a T x 64 tile

template <int T>
struct AttnGeom {
    static constexpr int LPR = (T >= 8) ? 64 / T : T;   // lanes sharing one score row
    static constexpr int JPL = T / LPR;                 // score columns per lane
    static constexpr int ACTIVE = T * LPR;              // lanes that own a row (T=4: 16)
    static constexpr int CPL = HD / LPR;                // output channels per lane
};

// stage a T x 64 tile whose rows are `ld` floats apart into LDS
template <int T, typename EL>
__device__ __forceinline__ void stage_tile(float* S, const EL* __restrict__ src, int64_t ld, int lane) {
#pragma unroll
    for (int r = 0; r < (T * 16 + 63) / 64; ++r) {
        const int idx = r * 64 + lane;
        if (idx < T * 16) {
            const int row = idx >> 4, c4 = idx & 15;
            st4(S + row * LDT + c4 * 4, ld4(src + row * ld + c4 * 4));
        }
    }
}

// s[jj] = scale * <A[i,:], Bm[j,:]> for j = jg*JPL + jj, causal (j <= i) else -inf
template <int T>
__device__ __forceinline__ void score_rows(const float* A, const float* Bm, int i, int jg, float scale,
                                           float (&s)[AttnGeom<T>::JPL]) {
    constexpr int JPL = AttnGeom<T>::JPL;
#pragma unroll
    for (int jj = 0; jj < JPL; ++jj) s[jj] = 0.f;
#pragma unroll
    for (int c4 = 0; c4 < 16; ++c4) {
        const float4 a = ld4(A + i * LDT + c4 * 4);
#pragma unroll
        for (int jj = 0; jj < JPL; ++jj) {
            const float4 b = ld4(Bm + (jg * JPL + jj) * LDT + c4 * 4);
            s[jj] += a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
        }
    }
#pragma unroll
    for (int jj = 0; jj < JPL; ++jj) s[jj] = (jg * JPL + jj <= i) ? s[jj] * scale : -INFINITY;
}

template <int T>
__device__ __forceinline__ void softmax_rows(float (&s)[AttnGeom<T>::JPL]) {
    constexpr int JPL = AttnGeom<T>::JPL, LPR = AttnGeom<T>::LPR;
    float mx = -INFINITY;
#pragma unroll
    for (int jj = 0; jj < JPL; ++jj) mx = fmaxf(mx, s[jj]);
    mx = group_max<LPR>(mx);
    float sum = 0.f;
#pragma unroll
    for (int jj = 0; jj < JPL; ++jj) { s[jj] = expf(s[jj] - mx); sum += s[jj]; }
    sum = group_sum<LPR>(sum);
    const float inv = 1.0f / sum;
#pragma unroll
    for (int jj = 0; jj < JPL; ++jj) s[jj] *= inv;
}

template <int T, typename EL = float>
__global__ __launch_bounds__(64) void attn_fwd_kernel(const EL* __restrict__ qkv, EL* __restrict__ o,
                                                      int d, int n_heads) {
    using G = AttnGeom<T>;
    __shared__ __attribute__((aligned(16))) float sm[3 * T * LDT + T * (T + 1)];
    float* Qs = sm; float* Ks = sm + T * LDT; float* Vs = sm + 2 * T * LDT; float* Ps = sm + 3 * T * LDT;
    const int lane = threadIdx.x;
    const int64_t seq = blockIdx.x / n_heads;
    const int hh = blockIdx.x - (int)(seq * n_heads);
    const int64_t ld = 3 * (int64_t)d;
    const EL* base = qkv + seq * T * ld + hh * HD;
    stage_tile<T>(Qs, base, ld, lane);
    stage_tile<T>(Ks, base + d, ld, lane);
    stage_tile<T>(Vs, base + 2 * d, ld, lane);
    __syncthreads();
    const bool active = lane < G::ACTIVE;
    const int i = active ? lane / G::LPR : 0, jg = lane % G::LPR;
    float s[G::JPL];
    score_rows<T>(Qs, Ks, i, jg, 0.125f, s);          // 1/sqrt(64)
    softmax_rows<T>(s);
    if (active) {
#pragma unroll
        for (int jj = 0; jj < G::JPL; ++jj) Ps[i * (T + 1) + jg * G::JPL + jj] = s[jj];
    }
    __syncthreads();
    if (active) {
        float4 acc[G::CPL / 4];
#pragma unroll
        for (int c = 0; c < G::CPL / 4; ++c) acc[c] = f4_zero();
        for (int j = 0; j <= i; ++j) {
            const float p = Ps[i * (T + 1) + j];
#pragma unroll
            for (int c = 0; c < G::CPL / 4; ++c) {
                const float4 v = ld4(Vs + j * LDT + jg * G::CPL + c * 4);
                acc[c].x += p * v.x; acc[c].y += p * v.y; acc[c].z += p * v.z; acc[c].w += p * v.w;
            }
        }
        EL* dst = o + (seq * T + i) * (int64_t)d + hh * HD + jg * G::CPL;
#pragma unroll
        for (int c = 0; c < G::CPL / 4; ++c) st4(dst + c * 4, acc[c]);
    }
}

template <int T, typename EL = float>
__global__ __launch_bounds__(64) void attn_bwd_kernel(const EL* __restrict__ qkv, const EL* __restrict__ dout,
                                                      EL* __restrict__ dqkv, int d, int n_heads) {
    using G = AttnGeom<T>;
    __shared__ __attribute__((aligned(16))) float sm[4 * T * LDT + 2 * T * (T + 1)];
    float* Qs = sm; float* Ks = sm + T * LDT; float* Vs = sm + 2 * T * LDT; float* Os = sm + 3 * T * LDT;
    float* Ps = sm + 4 * T * LDT; float* Ds = Ps + T * (T + 1);
    const int lane = threadIdx.x;
    const int64_t seq = blockIdx.x / n_heads;
    const int hh = blockIdx.x - (int)(seq * n_heads);
    const int64_t ld = 3 * (int64_t)d;
    const EL* base = qkv + seq * T * ld + hh * HD;
    stage_tile<T>(Qs, base, ld, lane);
    stage_tile<T>(Ks, base + d, ld, lane);
    stage_tile<T>(Vs, base + 2 * d, ld, lane);
    stage_tile<T>(Os, dout + seq * T * (int64_t)d + hh * HD, d, lane);
    __syncthreads();
    const bool active = lane < G::ACTIVE;
    const int i = active ? lane / G::LPR : 0, jg = lane % G::LPR;
    const float scale = 0.125f;
    float p[G::JPL], dp[G::JPL];
    score_rows<T>(Qs, Ks, i, jg, scale, p);
    softmax_rows<T>(p);
    score_rows<T>(Os, Vs, i, jg, 1.0f, dp);           // dP = dO . V^T (masked entries are -inf: unused)
    float delta = 0.f;
#pragma unroll
    for (int jj = 0; jj < G::JPL; ++jj) {
        const bool in = jg * G::JPL + jj <= i;
        dp[jj] = in ? dp[jj] : 0.f;
        delta += p[jj] * dp[jj];
    }
    delta = group_sum<G::LPR>(delta);
    if (active) {
#pragma unroll
        for (int jj = 0; jj < G::JPL; ++jj) {
            const int j = jg * G::JPL + jj;
            Ps[i * (T + 1) + j] = p[jj];
            Ds[i * (T + 1) + j] = p[jj] * (dp[jj] - delta) * scale;   // dS, pre-scaled
        }
    }
    __syncthreads();
    if (active) {
        // lane (row r = i, channel group jg): dQ[r] = sum_{j<=r} dS[r,j] K[j];
        // dK[r] = sum_{i>=r} dS[i,r] Q[i];  dV[r] = sum_{i>=r} P[i,r] dO[i]
        const int r = i, c0 = jg * G::CPL;
        float4 aq[G::CPL / 4], ak[G::CPL / 4], av[G::CPL / 4];
#pragma unroll
        for (int c = 0; c < G::CPL / 4; ++c) { aq[c] = f4_zero(); ak[c] = f4_zero(); av[c] = f4_zero(); }
        for (int j = 0; j <= r; ++j) {
            const float ds = Ds[r * (T + 1) + j];
#pragma unroll
            for (int c = 0; c < G::CPL / 4; ++c) {
                const float4 k = ld4(Ks + j * LDT + c0 + c * 4);
                aq[c].x += ds * k.x; aq[c].y += ds * k.y; aq[c].z += ds * k.z; aq[c].w += ds * k.w;
            }
        }
        for (int ii = r; ii < T; ++ii) {
            const float ds = Ds[ii * (T + 1) + r];
            const float pp = Ps[ii * (T + 1) + r];
#pragma unroll
            for (int c = 0; c < G::CPL / 4; ++c) {
                const float4 q = ld4(Qs + ii * LDT + c0 + c * 4);
                const float4 g = ld4(Os + ii * LDT + c0 + c * 4);
                ak[c].x += ds * q.x; ak[c].y += ds * q.y; ak[c].z += ds * q.z; ak[c].w += ds * q.w;
                av[c].x += pp * g.x; av[c].y += pp * g.y; av[c].z += pp * g.z; av[c].w += pp * g.w;
            }
        }
        EL* dst = dqkv + (seq * T + r) * ld + hh * HD + c0;
#pragma unroll
        for (int c = 0; c < G::CPL / 4; ++c) {
            st4(dst + c * 4, aq[c]);
            st4(dst + d + c * 4, ak[c]);
            st4(dst + 2 * d + c * 4, av[c]);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// T = 16 * NB: the MFMA scheme.  A 16 x 16 score tile is exactly one v_mfma_f32_16x16x4_f32 tile, so the T x T scores are an
// NB x NB grid of such tiles, of which the causal mask leaves query block qb the key tiles 0 .. qb; the last of them, the
// diagonal one, is masked element-wise and the others are whole.  One wavefront keeps q, k, v (and dO) of all T frames of
// its (slot, head) in registers, one set per block of 16 frames, loaded straight from HBM in the MFMA operand layouts, and
// every product is an exact-fp32 MFMA chain (at T = 32 the 4 T T 64 flop per head are no longer negligible on the vector
// ALU: the LDS-tile kernels above ran at 0.23 / 0.14 of the HBM roofline there):
//   row-style load   lane (r = l&15, g = l>>4) holds X[r][16f + 4g + e]   (f = float4 index, e = element)
//                    -> as operand A it is X[row r][k], as operand B it is X[col r][k]: the SAME
//                    registers give  S^T = K.Q^T  (A = K, B = Q)  and  S = Q.K^T  (A = Q, B = K)
//   k-style load     lane (c = l&15, g = l>>4) holds X[4g + rho][4c + e], rho = 0..3
//                    -> operand A of the products that contract over the 16 frames of a block
//   C/D layout       col = l&15, row = 4*(l>>4) + reg.  A score tile in this layout is ALREADY the B
//                    operand of the next product (k-slot g <-> frame 4g + reg at MFMA step reg), so P
//                    never moves between lanes (guide: "an accumulator tile as the next MFMA's operand").
// With output-channel mapping  row c' of tile ct  <->  channel 4c' + ct, a lane ends up owning 16
// consecutive channels of one frame: four float4 stores, 256 B contiguous per frame.
// The softmax of a query row spans the key tiles of its block; its statistics are shuffle reductions (over lane groups
// for a transposed tile, over the 16 lanes of a group for a plain tile).  The only LDS is one 16 x 68-float tile per
// wave, through which tiles are turned between the layouts on their way to a product or to memory.
// NB = 1 (T = 16, the metric shape) and NB = 2 (T = 32) are the instances; every loop over blocks and tiles is unrolled
// at compile time, so tiles stay in registers (NB = 2 backward: nine p / dS / dS^T tiles, no scratch).
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// f(I) for I = 0 .. N-1 in order, I an integral constant: a loop whose index can size an array or bound an inner loop
template <int N, int I = 0, typename F>
__device__ __forceinline__ void unrolled(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        unrolled<N, I + 1>(f);
    }
}

template <typename EL>
__device__ __forceinline__ void load_rows16(float4 (&x)[4], const EL* __restrict__ base, int64_t ld, int r, int g) {
#pragma unroll
    for (int f = 0; f < 4; ++f) x[f] = ld4(base + r * ld + 16 * f + 4 * g);
}
template <typename EL>
__device__ __forceinline__ void load_kmajor16(float4 (&x)[4], const EL* __restrict__ base, int64_t ld, int c, int g) {
#pragma unroll
    for (int rho = 0; rho < 4; ++rho) x[rho] = ld4(base + (4 * g + rho) * ld + 4 * c);
}
// D = sum_c A[.][c] * B[.][c] over the 64 channels held row-style (two chains to halve the latency)
__device__ __forceinline__ f32x4 dot_rows16(const float4 (&a)[4], const float4 (&b)[4]) {
    f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int f = 0; f < 4; ++f) {
        c0 = MFMA16(a[f].x, b[f].x, c0);
        c1 = MFMA16(a[f].y, b[f].y, c1);
        c0 = MFMA16(a[f].z, b[f].z, c0);
        c1 = MFMA16(a[f].w, b[f].w, c1);
    }
    return c0 + c1;
}
// out[ct] (tile of 16 channels 4c'+ct x 16 columns) += sum_rho A_k[rho][ct] * Bt[rho]
__device__ __forceinline__ void contract_frames16(f32x4 (&out)[4], const float4 (&ak)[4], const f32x4& bt) {
#pragma unroll
    for (int rho = 0; rho < 4; ++rho) {
        out[0] = MFMA16(ak[rho].x, bt[rho], out[0]);
        out[1] = MFMA16(ak[rho].y, bt[rho], out[1]);
        out[2] = MFMA16(ak[rho].z, bt[rho], out[2]);
        out[3] = MFMA16(ak[rho].w, bt[rho], out[3]);
    }
}
__device__ __forceinline__ void zero_tiles16(f32x4 (&o)[4]) {
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) o[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
}
// An output tile (lane (col, g) owns the 16 consecutive channels 16g .. 16g+15 of row `col`), stored through the wave's LDS
// tile: the MFMA layout hands a lane 16 channels of one frame in four 16-B pieces 64 B apart, i.e. every direct store
// instruction writes 64 scattered 16-B pieces; turned through LDS (4 ds_write_b128 + 4 ds_read_b128, conflict-free at the
// 68-float stride) each store instruction writes four full 256-B rows.  `rows0` = first of the 16 rows (row stride ld
// elements), column base already applied.
template <typename EL>
__device__ __forceinline__ void store_tiles16_rows(float* __restrict__ Tl, EL* __restrict__ rows0, int64_t ld, int lane,
                                                   const f32x4 (&o)[4]) {
    const int r = lane & 15, g = lane >> 4;
#pragma unroll
    for (int rho = 0; rho < 4; ++rho) st4(Tl + r * LDT + 16 * g + 4 * rho, make_float4(o[0][rho], o[1][rho], o[2][rho], o[3][rho]));
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int row = 4 * k + g;
        st4(rows0 + row * ld + 4 * r, ld4(Tl + row * LDT + 4 * r));
    }
    __builtin_amdgcn_wave_barrier();
}

// Softmax of one query block over its NT key tiles, the LAST of which is the diagonal one.
// TRANSPOSED tiles: lane (i, g) holds, for query i of the block, keys 4g + reg of key tile t
template <int NT>
__device__ __forceinline__ void softmax_t16n(f32x4* s, int i, int g, float scale) {
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool ok = t + 1 < NT || 4 * g + r <= i;
            s[t][r] = ok ? s[t][r] * scale : -INFINITY;
            mx = fmaxf(mx, s[t][r]);
        }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) { s[t][r] = expf(s[t][r] - mx); sum += s[t][r]; }
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
    const float inv = 1.0f / sum;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) s[t][r] *= inv;
}
// PLAIN tiles: lane (j, g) holds key j of key tile t for queries 4g + reg.  The probabilities are v / sum, a division per
// tile and not a shared reciprocal: it is the rule the T = 16 kernel has always had, so NB = 1 keeps its bits and query
// block 0 of a longer sequence computes what T = 16 computes on the same frames.
template <int NT>
__device__ __forceinline__ void softmax_p16n(f32x4* s, int j, int g, float scale) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float v[NT], mx, sum;                 // both start from tile 0, not from -inf and 0: NT = 1 is then one max and one sum
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            v[t] = (t + 1 < NT || j <= 4 * g + r) ? s[t][r] * scale : -INFINITY;
            const float m = group_max<16>(v[t]);
            mx = t ? fmaxf(mx, m) : m;
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            v[t] = expf(v[t] - mx);
            const float a = group_sum<16>(v[t]);
            sum = t ? sum + a : a;
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) s[t][r] = v[t] / sum;
    }
}

template <int NB, typename EL>
__device__ __forceinline__ void attn_mfma_fwd_body(const EL* __restrict__ qkv, EL* __restrict__ o, int d, int n_heads, int64_t n_items) {
    __shared__ __attribute__((aligned(16))) float out_tile[4][16 * LDT];
    const int lane = threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);     // four waves per block, one (slot, head) each
    if (item >= n_items) return;                                          // wave-uniform
    const int64_t seq = item / n_heads;
    const int hh = (int)(item - seq * n_heads);
    const int r = lane & 15, g = lane >> 4;
    const int64_t ld = 3 * (int64_t)d;
    const EL* base = qkv + seq * (16 * NB) * ld + hh * HD;
    float4 qf[NB][4], kf[NB][4], vk[NB][4];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        load_rows16(qf[b], base + b * 16 * ld, ld, r, g);
        load_rows16(kf[b], base + b * 16 * ld + d, ld, r, g);
        load_kmajor16(vk[b], base + b * 16 * ld + 2 * d, ld, r, g);
    }
    float* const Tl = out_tile[threadIdx.x >> 6];
    EL* const obase = o + seq * (16 * NB) * (int64_t)d + hh * HD;
    unrolled<NB>([&](auto qb) {
        constexpr int NT = qb + 1;
        f32x4 pt[NT], acc[4];
#pragma unroll
        for (int t = 0; t < NT; ++t) pt[t] = dot_rows16(kf[t], qf[qb]);       // S^T[j = 4g+reg of tile t][i = r]
        softmax_t16n<NT>(pt, r, g, 0.125f);                                   // 1/sqrt(64)
        zero_tiles16(acc);
#pragma unroll
        for (int t = 0; t < NT; ++t) contract_frames16(acc, vk[t], pt[t]);    // O^T[c][i] = sum_j V[j][c] P^T[j][i]
        store_tiles16_rows(Tl, obase + qb * 16 * (int64_t)d, (int64_t)d, lane, acc);
    });
}

// probabilities and score gradients of one query block against its NT key tiles, in both layouts:
//   p[t], ds[t]  plain (lane (j, g): key j, queries 4g + reg)        dst[t]  transposed (lane (i, g): query i, keys 4g + reg)
template <int NT>
__device__ __forceinline__ void attn_block_grads(const float4 (&q)[4], const float4 (&gq)[4], const float4 (*k)[4], const float4 (*v)[4],
                                                 int r, int g, float scale, f32x4* p, f32x4* ds, f32x4* dst) {
    f32x4 pt[NT], dp[NT], dpt[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        pt[t] = dot_rows16(k[t], q);                          // S^T : lane (i, g), keys 4g + reg of tile t
        p[t] = dot_rows16(q, k[t]);                           // S   : lane (j, g), queries 4g + reg
        dpt[t] = dot_rows16(v[t], gq);                        // dP^T[j][i] = sum_c V[j][c] dO[i][c]
        dp[t] = dot_rows16(gq, v[t]);                         // dP  [i][j]
    }
    softmax_t16n<NT>(pt, r, g, scale);
    softmax_p16n<NT>(p, r, g, scale);
    float dl = 0.f;                                           // delta_i = sum_j P[i][j] dP[i][j]  (masked entries have P = 0)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) dl += pt[t][kk] * dpt[t][kk];
    dl += __shfl_xor(dl, 16);
    dl += __shfl_xor(dl, 32);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        float dk;                                             // the same delta for query 4g + kk, summed over the key lanes
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const float a = group_sum<16>(p[t][kk] * dp[t][kk]);
            dk = t ? dk + a : a;
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            dst[t][kk] = pt[t][kk] * (dpt[t][kk] - dl) * scale;
            ds[t][kk] = p[t][kk] * (dp[t][kk] - dk) * scale;
        }
    }
}

template <int NB, typename EL>
__device__ __forceinline__ void attn_mfma_bwd_body(const EL* __restrict__ qkv, const EL* __restrict__ dout, EL* __restrict__ dqkv,
                                                   int d, int n_heads, int64_t n_items) {
    __shared__ __attribute__((aligned(16))) float turn_tile[4][16 * LDT];
    const int lane = threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);     // four waves per block, one (slot, head) each
    if (item >= n_items) return;                                          // wave-uniform
    const int64_t seq = item / n_heads;
    const int hh = (int)(item - seq * n_heads);
    const int r = lane & 15, g = lane >> 4;
    const int64_t ld = 3 * (int64_t)d;
    const EL* base = qkv + seq * (16 * NB) * ld + hh * HD;
    const EL* gbase = dout + seq * (16 * NB) * (int64_t)d + hh * HD;
    float* const T = turn_tile[threadIdx.x >> 6];
    float4 qf[NB][4], kf[NB][4], gf[NB][4];
    f32x4 p[NB][NB], ds[NB][NB], dst[NB][NB];                  // [query block qb][key tile t <= qb]
    {
        float4 vf[NB][4];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            load_rows16(qf[b], base + b * 16 * ld, ld, r, g);
            load_rows16(kf[b], base + b * 16 * ld + d, ld, r, g);
            load_rows16(vf[b], base + b * 16 * ld + 2 * d, ld, r, g);
            load_rows16(gf[b], gbase + b * 16 * (int64_t)d, (int64_t)d, r, g);
        }
        unrolled<NB>([&](auto qb) { attn_block_grads<qb + 1>(qf[qb], gf[qb], kf, vf, r, g, 0.125f, p[qb], ds[qb], dst[qb]); });
    }
    EL* const obase = dqkv + seq * (16 * NB) * ld + hh * HD;
    f32x4 acc[NB][4];                                          // one output tile per block of 16 frames
    float4 xk[4];
    // The three products below contract over the frames of a block, so they need dO, Q, K frame-major ("k-style").  Loading
    // them from HBM a second time in that layout costs 1.35x the algorithmic bytes (PMC), so the row-style registers are
    // turned through the wave's 4 KB LDS tile, each block once for all its contractions: 4 ds_write_b128 + 4 ds_read_b128
    // per tile, both conflict-free at the 68-float row stride.  One wave owns the tile and DS operations of a wave execute
    // in order, so no barrier is needed - only the compiler must not reorder the accesses (wave_barrier).
    auto turn = [&](const float4 (&rows)[4]) {
#pragma unroll
        for (int f = 0; f < 4; ++f) st4(T + r * LDT + 16 * f + 4 * g, rows[f]);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int rho = 0; rho < 4; ++rho) xk[rho] = ld4(T + (4 * g + rho) * LDT + 4 * r);
        __builtin_amdgcn_wave_barrier();
    };
    auto zero = [&] {
#pragma unroll
        for (int b = 0; b < NB; ++b) zero_tiles16(acc[b]);
    };
    auto store = [&](EL* rows0) {
#pragma unroll
        for (int b = 0; b < NB; ++b) store_tiles16_rows(T, rows0 + b * 16 * ld, ld, lane, acc[b]);
    };
    // dV[j][c] = sum_i P[i][j] dO[i][c] and dK[j][c] = sum_i dS[i][j] Q[i][c]: the accumulator of key tile t takes query blocks
    // t .. NB-1 in rising order.  The two are written out: folded into one lambda over (rows, weights) the same products were
    // scheduled differently and the T = 16 backward took 41.7 - 42.3 us against 40.7 - 40.9 us in this form (parent 40.6 - 41.1).
    zero();
    unrolled<NB>([&](auto qb) {
        turn(gf[qb]);
#pragma unroll
        for (int t = 0; t <= qb; ++t) contract_frames16(acc[t], xk, p[qb][t]);
    });
    store(obase + 2 * d);
    zero();
    unrolled<NB>([&](auto qb) {
        turn(qf[qb]);
#pragma unroll
        for (int t = 0; t <= qb; ++t) contract_frames16(acc[t], xk, ds[qb][t]);
    });
    store(obase + d);
    // dQ[i][c] = sum_j dS^T[j][i] K[j][c]: key tile t reaches the query blocks t .. NB-1
    zero();
    unrolled<NB>([&](auto t) {
        turn(kf[t]);
#pragma unroll
        for (int qb = t; qb < NB; ++qb) contract_frames16(acc[qb], xk, dst[qb][t]);
    });
    store(obase);
}

// The kernels keep one name per (T, storage): the benchmark and the profiling tools find them by name.
template <int T, typename EL> struct AttnMfma;
#define ATTN_MFMA_KERNELS(T, SFX, EL)                                                                                              \
    __global__ __launch_bounds__(256) void attn##T##_fwd##SFX##_kernel(const EL* __restrict__ qkv, EL* __restrict__ o, int d,      \
                                                                       int n_heads, int64_t n_items) {                             \
        attn_mfma_fwd_body<T / 16>(qkv, o, d, n_heads, n_items);                                                                   \
    }                                                                                                                              \
    __global__ __launch_bounds__(256) void attn##T##_bwd##SFX##_kernel(const EL* __restrict__ qkv, const EL* __restrict__ dout,    \
                                                                       EL* __restrict__ dqkv, int d, int n_heads, int64_t n_items) { \
        attn_mfma_bwd_body<T / 16>(qkv, dout, dqkv, d, n_heads, n_items);                                                          \
    }                                                                                                                              \
    template <> struct AttnMfma<T, EL> {                                                                                           \
        static constexpr auto fwd = attn##T##_fwd##SFX##_kernel;                                                                   \
        static constexpr auto bwd = attn##T##_bwd##SFX##_kernel;                                                                   \
    };
ATTN_MFMA_KERNELS(16, , float)
ATTN_MFMA_KERNELS(16, _bf16, bf16_t)
ATTN_MFMA_KERNELS(32, , float)
ATTN_MFMA_KERNELS(32, _bf16, bf16_t)

// ------------------------------------------------------------------------------------------------
// One query position against the cache (generation while the history grows): query row r*T + p, keys and values of rows
// r*T + j, j <= p; rows j > p are never read.  One wavefront per (sequence, head), lane = channel: a key or value row of
// a head is one coalesced 64-element load, a score is one wavefront reduction, and the softmax is the max-subtracted expf
// one of the kernels above.  Every load of the wave is issued before the first reduction.  Bytes per (sequence, head):
// 2*(p+1)*64 elements in, 64 out; at B*N sequences the launch is latency-bound, not bandwidth-bound.
// The score reduction runs in fp64 (a product of two fp32 values is exact there, so the score is rounded once): a
// shuffle tree cannot accumulate by FMA the way the tile kernels' dot products do, and with |score| ~ 60-90 the rounding
// of 64 fp32 products showed against the fp64 reference.  6 x 2 more shuffles per key in a kernel that waits on launches.
__device__ __forceinline__ double wave_sum64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
template <int T, typename EL>
__global__ __launch_bounds__(256) void attn_step_kernel(const EL* __restrict__ qkv, EL* __restrict__ o, int d, int n_heads,
                                                        int64_t n_items, int p, int64_t ldo) {
    const int lane = threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= n_items) return;                             // wave-uniform
    const int64_t seq = item / n_heads;
    const int hh = (int)(item - seq * n_heads);
    const int64_t ld = 3 * (int64_t)d;
    const EL* base = qkv + seq * T * ld + hh * HD + lane;
    const double q = (double)ld1(base + p * ld);
    float k[T], v[T], s[T];
#pragma unroll
    for (int j = 0; j < T; ++j) {
        k[j] = v[j] = 0.f;
        if (j <= p) {                                         // wave-uniform
            k[j] = ld1(base + j * ld + d);
            v[j] = ld1(base + j * ld + 2 * d);
        }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < T; ++j) {
        s[j] = -INFINITY;
        if (j <= p) {
            s[j] = (float)wave_sum64(q * (double)k[j]) * 0.125f;      // 1/sqrt(64)
            mx = fmaxf(mx, s[j]);
        }
    }
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < T; ++j) {
        s[j] = j <= p ? expf(s[j] - mx) : 0.f;
        sum += s[j];
    }
    const float inv = 1.0f / sum;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < T; ++j)
        if (j <= p) acc += (s[j] * inv) * v[j];
    st1(o + seq * ldo + hh * HD + lane, acc);
}

// ------------------------------------------------------------------------------------------------
// Host side.  Every rule of the entry points' arguments, stated once; the shape is decided before the alignment.  The tile
// kernels move four elements per access, so their pointers need align = 4 * sizeof(EL): 16 B in fp32 storage, 8 B in bf16.
static int attn_check(std::initializer_list<const void*> ptrs, size_t align, int64_t n_seq, int T, int d) {
    if (n_seq < 1 || d < HD || (d % HD) != 0) return VLG_ERR_SHAPE;
    if (T != 4 && T != 8 && T != 16 && T != 32) return VLG_ERR_SHAPE;
    if (n_seq * (d / HD) > 0x7fffffff) return VLG_ERR_SHAPE;          // one block (T = 4, 8) or wave per item
    for (const void* p : ptrs)
        if ((reinterpret_cast<uintptr_t>(p) & (align - 1)) != 0) return VLG_ERR_ALIGN;
    return 0;
}

template <typename EL>
static int attn_fwd_launch(const EL* qkv, EL* o, int64_t n_seq, int T, int d, void* stream) {
    if (int e = attn_check({qkv, o}, 4 * sizeof(EL), n_seq, T, d)) return e;
    const int H = d / HD;
    const int64_t items = n_seq * H;
    const dim3 grid1((unsigned)items), block1(64), grid4((unsigned)((items + 3) / 4)), block4(256);
    hipStream_t s = (hipStream_t)stream;
    switch (T) {
        case 4:  hipLaunchKernelGGL((attn_fwd_kernel<4, EL>), grid1, block1, 0, s, qkv, o, d, H); break;
        case 8:  hipLaunchKernelGGL((attn_fwd_kernel<8, EL>), grid1, block1, 0, s, qkv, o, d, H); break;
        case 16: hipLaunchKernelGGL((AttnMfma<16, EL>::fwd), grid4, block4, 0, s, qkv, o, d, H, items); break;
        default: hipLaunchKernelGGL((AttnMfma<32, EL>::fwd), grid4, block4, 0, s, qkv, o, d, H, items); break;
    }
    return vlg_last_error();
}

template <typename EL>
static int attn_bwd_launch(const EL* qkv, const EL* dout, EL* dqkv, int64_t n_seq, int T, int d, void* stream) {
    if (int e = attn_check({qkv, dout, dqkv}, 4 * sizeof(EL), n_seq, T, d)) return e;
    const int H = d / HD;
    const int64_t items = n_seq * H;
    const dim3 grid1((unsigned)items), block1(64), grid4((unsigned)((items + 3) / 4)), block4(256);
    hipStream_t s = (hipStream_t)stream;
    switch (T) {
        case 4:  hipLaunchKernelGGL((attn_bwd_kernel<4, EL>), grid1, block1, 0, s, qkv, dout, dqkv, d, H); break;
        case 8:  hipLaunchKernelGGL((attn_bwd_kernel<8, EL>), grid1, block1, 0, s, qkv, dout, dqkv, d, H); break;
        case 16: hipLaunchKernelGGL((AttnMfma<16, EL>::bwd), grid4, block4, 0, s, qkv, dout, dqkv, d, H, items); break;
        default: hipLaunchKernelGGL((AttnMfma<32, EL>::bwd), grid4, block4, 0, s, qkv, dout, dqkv, d, H, items); break;
    }
    return vlg_last_error();
}

// The step kernel loads single elements.  Its entry points keep the order of their checks: the 8-B rule for both storages,
// then p and ldo, then null pointers, then (fp32) 16 B.
template <typename EL>
static int attn_step_launch(const EL* qkv, EL* o, int64_t n_seq, int T, int d, int p, int64_t ldo, void* stream) {
    if (int e = attn_check({qkv, o}, 8, n_seq, T, d)) return e;
    if (p < 0 || p >= T || ldo < d) return VLG_ERR_SHAPE;
    if (!qkv || !o) return VLG_ERR_ALIGN;
    if (int e = attn_check({qkv, o}, 4 * sizeof(EL), n_seq, T, d)) return e;
    const int H = d / HD;
    const int64_t items = n_seq * H;
    const dim3 grid((unsigned)((items + 3) / 4)), block(256);
    hipStream_t s = (hipStream_t)stream;
    switch (T) {
        case 4:  hipLaunchKernelGGL((attn_step_kernel<4, EL>),  grid, block, 0, s, qkv, o, d, H, items, p, ldo); break;
        case 8:  hipLaunchKernelGGL((attn_step_kernel<8, EL>),  grid, block, 0, s, qkv, o, d, H, items, p, ldo); break;
        case 16: hipLaunchKernelGGL((attn_step_kernel<16, EL>), grid, block, 0, s, qkv, o, d, H, items, p, ldo); break;
        default: hipLaunchKernelGGL((attn_step_kernel<32, EL>), grid, block, 0, s, qkv, o, d, H, items, p, ldo); break;
    }
    return vlg_last_error();
}

static const bf16_t* bf(const vlg_bf16* p) { return reinterpret_cast<const bf16_t*>(p); }
static bf16_t* bf(vlg_bf16* p) { return reinterpret_cast<bf16_t*>(p); }

extern "C" int vlg_attention_fwd(const float* qkv, float* o, int64_t n_seq, int T, int d, void* stream) {
    return attn_fwd_launch(qkv, o, n_seq, T, d, stream);
}
extern "C" int vlg_attention_fwd_bf16(const vlg_bf16* qkv, vlg_bf16* o, int64_t n_seq, int T, int d, void* stream) {
    return attn_fwd_launch(bf(qkv), bf(o), n_seq, T, d, stream);
}
extern "C" int vlg_attention_bwd(const float* qkv, const float* dout, float* dqkv, int64_t n_seq, int T, int d,
                                 void* stream) {
    return attn_bwd_launch(qkv, dout, dqkv, n_seq, T, d, stream);
}
extern "C" int vlg_attention_bwd_bf16(const vlg_bf16* qkv, const vlg_bf16* dout, vlg_bf16* dqkv, int64_t n_seq, int T, int d,
                                      void* stream) {
    return attn_bwd_launch(bf(qkv), bf(dout), bf(dqkv), n_seq, T, d, stream);
}
extern "C" int vlg_attention_step(const float* qkv, float* o, int64_t n_seq, int T, int d, int p, int64_t ldo, void* stream) {
    return attn_step_launch(qkv, o, n_seq, T, d, p, ldo, stream);
}
extern "C" int vlg_attention_step_bf16(const vlg_bf16* qkv, vlg_bf16* o, int64_t n_seq, int T, int d, int p, int64_t ldo,
                                       void* stream) {
    return attn_step_launch(bf(qkv), bf(o), n_seq, T, d, p, ldo, stream);
}
