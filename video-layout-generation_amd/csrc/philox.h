// The device's random numbers, stated once ("Random draws"): Philox4x32-10 (Salmon et al., Random123) as a
// stateless function of a 4-word counter and a 2-word key, the three ways a kernel turns an output word into a number, and
// the host rules that go with them.  A counter is (index, step, stream, sample) under the key of the call's 64-bit seed; `stream`
// is an entry of vlg_rng_stream (include/vlg_hip.h), the one table of them; `sample` is the sample index of the K-sample decoding
// entries (vlg_layout_decode_samples) and 0 for every other draw.  The dropout mask (layernorm_rows.h) is the
// exception: its counter is (row, float4 index, site, step), under a seed of its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/vlg_hip.h"

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t (&x)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    x[0] = c0; x[1] = c1; x[2] = c2; x[3] = c3;
}

// word 0 of counter (c0, c1, stream, c3): the same call - the compiler drops what only the other three words need
__device__ __forceinline__ uint32_t philox_word0(uint32_t c0, uint32_t c1, uint32_t stream, uint32_t c3, uint32_t k0, uint32_t k1) {
    uint32_t x[4];
    philox4x32_10(c0, c1, stream, c3, k0, k1, x);
    return x[0];
}

// ---- one output word -> a number: the upper 24 bits, so (float)(x >> 8) is exact.  Both products below are exact too, so
// each function gives the same bits with floating-point contraction on or off (augment.hip compiles with it off).
// uniform in (0, 1], as the class draw forms it: (x >> 8) * 2^-24 + 2^-25 in fp32 - the sum rounds above 2^23 and may give 1.0
__device__ __forceinline__ float philox_unit(uint32_t x) {
    return (float)(x >> 8) * 5.9604644775390625e-08f + 2.98023223876953125e-08f;
}
// signed value in [-1, 1): (x >> 8) * 2^-23 - 1, every step exact in fp32
__device__ __forceinline__ float philox_signed(uint32_t x) { return (float)(x >> 8) * 1.1920928955078125e-7f - 1.0f; }
// coin that wins with probability thr / 2^24: thr = 0 never wins, 2^24 always does
__device__ __forceinline__ bool philox_coin(uint32_t x, uint32_t thr) { return (x >> 8) < thr; }

// ---- host side
struct PhiloxKey { uint32_t k0, k1; };
static inline PhiloxKey philox_key(uint64_t seed) { return PhiloxKey{(uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32)}; }
// probability in [0, 1] (the caller refuses anything else) -> philox_coin's threshold, round(p * 2^24)
static inline uint32_t philox_coin_threshold(double p) { return (uint32_t)__builtin_floor(p * 16777216.0 + 0.5); }
// an index that is a counter word of these draws: `count` of them must fit 31 bits (the kernels hold it in an int)
static inline bool philox_index_fits(int64_t count) { return count <= 0x7fffffffLL; }
