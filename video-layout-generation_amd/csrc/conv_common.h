// Shared by the fp32 (conv.hip) and bf16-MFMA (conv_bf16.hip) 3x3 convolutions: the launch arguments, the activation
// applied on load, and the bf16 launcher that conv.hip's entry points call with their plan's tile.
#pragma once
#include "gemm_tile.h"

#define CONV_FWD 0
#define CONV_DGRAD 1
#define CONV_WGRAD 2

struct ConvArgs {
    const float* A; const float* B; float* C;
    const float* bias; const float* aux_in; const float* rowmask; const float* prelu; float* da_slab;
    const int* rowtab; int64_t tab_stride;
    int64_t M;               // rows of C
    int N;                   // cols of C that are stored
    int64_t Kc;              // contraction extent
    int lda, ldb, ldc;
    int cin;                 // channels per tap of the gathered operand (multiple of 32)
    int b_tap_stride;        // dgrad: column offset of one tap inside a weight row
    int shift[9];
    int wp, sign;            // shift[tap] = sign * ((tap / 3 - 1) * wp + tap % 3 - 1) (0 / 0 with per-tap row tables)
    int tiles_m, tiles_n, splits;
    int64_t kc_per_split, slab_stride, colsum_off;
    int epi;
    int act_ch;              // PReLU applies to channels < act_ch only (AddCoords channels stay linear)
    // tail of the tile order cut along K ("data-parallel + split-K remainder"): the last tail_tiles tiles (whole row tiles)
    // are computed by tail_splits blocks each, which store raw partial tiles to tail_ws[split][row - tail_row0][ldc];
    // conv_finish_* sums them and applies the epilogue.  0 = every tile by one block.
    int tail_tiles, tail_splits;
    int64_t tail_kc, tail_row0, tail_stride;
    float* tail_ws;
    unsigned long long* probe;   // diagnostic build only (-DVLG_TIMELINE, tools/diag/conv_timeline.py)
};

__device__ __forceinline__ float prelu_f(float v, float a) { return v > 0.f ? v : a * v; }
// branch-free and exact: max(v,0) + a*min(v,0) is v for v > 0 and the singly-rounded a*v otherwise; a = 1 is the identity,
// a = 0 is ReLU.  med3 keeps the compiler from inserting NaN-canonicalising moves around max/min.
__device__ __forceinline__ float act_f(float v, float a) {
    return __builtin_fmaf(a, __builtin_amdgcn_fmed3f(v, -__builtin_inff(), 0.f), __builtin_amdgcn_fmed3f(v, 0.f, __builtin_inff()));
}
__device__ __forceinline__ float4 act4(float4 v, float4 a) { return make_float4(act_f(v.x, a.x), act_f(v.y, a.y), act_f(v.z, a.z), act_f(v.w, a.w)); }
// slopes of channels c .. c+3: channels >= act_ch (the AddCoords pair, padding) stay linear
__device__ __forceinline__ float4 slope4(float a, int c, int act_ch) {
    return make_float4(c < act_ch ? a : 1.f, c + 1 < act_ch ? a : 1.f, c + 2 < act_ch ? a : 1.f, c + 3 < act_ch ? a : 1.f);
}

// launch conv_bf16_kernel (conv_bf16.hip) for mode CONV_* on a BM x BN tile of the plan; g as conv.hip fills it
int conv_bf16_launch(int mode, int bm, int bn, const ConvArgs& g, hipStream_t s);
