// Augmentation of a layout batch on the device (rule: include/vlg_hip.h, "augmentation"; DESIGN.md "Augmentation").
//
// vlg_augment_plan    host only: probability -> the 24-bit coin threshold (philox_coin_threshold, philox.h)
// vlg_layout_augment  per clip flip / zoom / shift, per input token jitter, per track drop: one launch, the caller's batch
//                     only read, four engine-owned buffers written
//
// One thread per token i = (b*T + t)*N + n: a wave's lanes sit on consecutive n, so the 8-byte class, the two 16-byte box
// and the 4-byte valid accesses are all coalesced.  The clip draw is recomputed by every thread of the clip and the track
// draw by the T threads of the track (an integer-only Philox call each, no LDS, no second launch).  Launch-bound: 88 bytes
// per token, 2.9 MB at (32,16,64).  Three compile-time variants: AUG_COPY (flip / drop only: a box that is not flipped is
// moved as the four words it is), AUG_GEO (zoom / shift) and AUG_JIT (+ the third Philox call of the token draw).
#include "common.h"
#include "philox.h"

#define AUG_BLOCK 256
enum { AUG_COPY = 0, AUG_GEO = 1, AUG_JIT = 2 };

// One axis of the crop to the image.  max / min of the rule are the comparisons written here, so a NaN becomes the constant.
__device__ __forceinline__ void aug_crop(float& c, float& w) {
#pragma clang fp contract(off)
    const float half = 0.5f * w;
    const float lo = c - half, hi = c + half;
    const float x0 = lo > 0.f ? lo : 0.f, x1 = hi < 1.f ? hi : 1.f;
    const float d = x1 - x0, m = 0.5f * (x0 + x1);
    w = d > 0.0009765625f ? d : 0.0009765625f;
    const float m0 = m > 0.f ? m : 0.f;
    c = m0 < 1.f ? m0 : 1.f;
}

// The box map.  Every operation is one rounded fp32 operation: contraction is off in this function (and for the whole
// file, csrc/Makefile), because tests/augment_ref.py restates it operation by operation and the outputs are compared by bits.
template <int MODE, bool JIT>
__device__ __forceinline__ float4 aug_map(float4 b, bool flip, float s, float tx, float ty, float jx, float jy, float jw, float jh) {
#pragma clang fp contract(off)
    if (flip) b.x = 1.0f - b.x;
    if constexpr (MODE != AUG_COPY) {
        b.x = ((b.x - 0.5f) * s + 0.5f) + tx;
        b.y = ((b.y - 0.5f) * s + 0.5f) + ty;
        b.z = b.z * s;
        b.w = b.w * s;
        if constexpr (JIT) {
            b.x = b.x + jx;
            b.y = b.y + jy;
            b.z = b.z * jw;
            b.w = b.w * jh;
        }
        aug_crop(b.x, b.z);
        aug_crop(b.y, b.w);
    }
    return b;
}

template <int MODE>
__global__ __launch_bounds__(AUG_BLOCK) void layout_augment_kernel(
    const int64_t* __restrict__ cls, const float* __restrict__ box, const float* __restrict__ tgt_box,
    const float* __restrict__ valid, int64_t* __restrict__ aug_cls, float* __restrict__ aug_box,
    float* __restrict__ aug_tgt_box, float* __restrict__ aug_valid, const int* __restrict__ step_ptr, int M, int T, int N,
    int C, uint32_t thr_flip, uint32_t thr_drop, float zoom, float shift, float jitter, uint32_t k0, uint32_t k1) {
#pragma clang fp contract(off)
    const int64_t gi = (int64_t)blockIdx.x * AUG_BLOCK + threadIdx.x;
    if (gi >= M) return;
    const int i = (int)gi, TN = T * N;
    const int b = i / TN, rem = i - b * TN, n = rem % N;
    const uint32_t k = (uint32_t)*step_ptr;
    int64_t c = cls[i];
    float4 bx = ld4(box + 4 * (int64_t)i), tb = ld4(tgt_box + 4 * (int64_t)i);
    float v = valid[i];

    uint32_t x[4];
    bool flip = false, drop = false;
    float s = 1.f, tx = 0.f, ty = 0.f, jx = 0.f, jy = 0.f, jw = 1.f, jh = 1.f;
    if (MODE != AUG_COPY || thr_flip != 0u) {                      // (a zero threshold never wins: the draw is not needed)
        philox4x32_10((uint32_t)b, k, VLG_RNG_CLIP_DRAW, 0u, k0, k1, x);
        flip = philox_coin(x[0], thr_flip);
        if constexpr (MODE != AUG_COPY) {
            s = 1.0f + zoom * philox_signed(x[1]);
            tx = shift * philox_signed(x[2]);
            ty = shift * philox_signed(x[3]);
        }
    }
    if (thr_drop != 0u) {
        philox4x32_10((uint32_t)(b * N + n), k, VLG_RNG_TRACK_DROP, 0u, k0, k1, x);
        drop = philox_coin(x[0], thr_drop);
    }
    if constexpr (MODE == AUG_JIT) {
        philox4x32_10((uint32_t)i, k, VLG_RNG_TOKEN_JITTER, 0u, k0, k1, x);
        jx = jitter * philox_signed(x[0]);
        jy = jitter * philox_signed(x[1]);
        jw = 1.0f + jitter * philox_signed(x[2]);
        jh = 1.0f + jitter * philox_signed(x[3]);
    }

    if (drop) {                                                    // the whole track, in every frame: reserved class, zero box
        c = C;
        bx = f4_zero();
    } else if (c < C) {                                            // (a padded token keeps its id and its box)
        if (MODE != AUG_COPY || flip) bx = aug_map<MODE, MODE == AUG_JIT>(bx, flip, s, tx, ty, jx, jy, jw, jh);
    }
    if (v > 0.f && (MODE != AUG_COPY || flip)) tb = aug_map<MODE, false>(tb, flip, s, tx, ty, 0.f, 0.f, 1.f, 1.f);
    if (drop) v = 0.f;
    aug_cls[i] = c;
    st4(aug_box + 4 * (int64_t)i, bx);
    st4(aug_tgt_box + 4 * (int64_t)i, tb);
    aug_valid[i] = v;
}

extern "C" int vlg_augment_plan(double p, uint32_t* thr_host) {
    if (!(p >= 0.0 && p <= 1.0) || thr_host == nullptr) return VLG_ERR_SHAPE;
    *thr_host = philox_coin_threshold(p);
    return 0;
}

static inline bool aug_knob_ok(float x, float bound) { return x >= 0.f && x <= bound; }      // (refuses NaN and inf)

extern "C" int vlg_layout_augment(const int64_t* cls, const float* box, const float* tgt_box, const float* valid,
                                  int64_t* aug_cls, float* aug_box, float* aug_tgt_box, float* aug_valid, const int* step,
                                  int B, int T, int N, int n_classes, uint32_t thr_flip, uint32_t thr_drop, float zoom,
                                  float shift, float jitter, uint64_t seed, void* stream) {
    if (B < 1 || T < 1 || N < 1 || n_classes < 1) return VLG_ERR_SHAPE;
    const int64_t M = (int64_t)B * T * N;
    if (!philox_index_fits(M)) return VLG_ERR_SHAPE;                                    // the Philox counter word is the token index
    if (thr_flip > (1u << 24) || thr_drop > (1u << 24)) return VLG_ERR_SHAPE;
    if (!aug_knob_ok(zoom, 0.5f) || !aug_knob_ok(shift, 0.5f) || !aug_knob_ok(jitter, 0.25f)) return VLG_ERR_SHAPE;
    if (!cls || !box || !tgt_box || !valid || !aug_cls || !aug_box || !aug_tgt_box || !aug_valid || !step) return VLG_ERR_SHAPE;
    // inputs are only read and outputs only written: an output overlapping any other buffer is refused
    const void* p[9] = {aug_cls, aug_box, aug_tgt_box, aug_valid, cls, box, tgt_box, valid, step};
    const int64_t nb[9] = {M * 8, M * 16, M * 16, M * 4, M * 8, M * 16, M * 16, M * 4, 4};
    for (int o = 0; o < 4; ++o)
        for (int j = o + 1; j < 9; ++j)
            if (vlg_overlap(p[o], nb[o], p[j], nb[j])) return VLG_ERR_SHAPE;
    if (!vlg_aligned16(box) || !vlg_aligned16(tgt_box) || !vlg_aligned16(aug_box) || !vlg_aligned16(aug_tgt_box) ||
        !vlg_aligned8(cls) || !vlg_aligned8(aug_cls) || !vlg_aligned4(valid) || !vlg_aligned4(aug_valid) || !vlg_aligned4(step))
        return VLG_ERR_ALIGN;
    const dim3 grid((unsigned)((M + AUG_BLOCK - 1) / AUG_BLOCK)), block(AUG_BLOCK);
    const PhiloxKey key = philox_key(seed);
#define AUG_LAUNCH(MODE)                                                                                                       \
    hipLaunchKernelGGL(layout_augment_kernel<MODE>, grid, block, 0, (hipStream_t)stream, cls, box, tgt_box, valid, aug_cls,   \
                       aug_box, aug_tgt_box, aug_valid, step, (int)M, T, N, n_classes, thr_flip, thr_drop, zoom, shift, jitter, \
                       key.k0, key.k1)
    if (jitter > 0.f) AUG_LAUNCH(AUG_JIT);                         // one decision for the whole launch
    else if (zoom > 0.f || shift > 0.f) AUG_LAUNCH(AUG_GEO);
    else AUG_LAUNCH(AUG_COPY);
#undef AUG_LAUNCH
    return vlg_last_error();
}
