/*
 * vlg_hip.h - C ABI of libvlg_hip.so, the MI355X (gfx950) kernels behind the
 * per-clip layout-generation training step.
 *
 * The reference (gongaa/video-layout-generation) has no native code and no FFI:
 * every device op is a stock torch.nn call made from src/trainer.py.  Each entry
 * point below therefore cites the torch call site in the reference it replaces
 * (file:line under /root/reference), or says SELF-ORACLE where BASELINE.json
 * names an op the reference does not contain.
 *
 * Conventions
 *   - plain pointers and sizes only; all pointers are DEVICE pointers unless
 *     the name ends in _host; the caller (PyTorch) owns every buffer
 *   - `stream` is a hipStream_t passed as void*; kernels are stream-ordered on it,
 *     never allocate, never synchronise, keep no global state
 *   - return value: 0 on success, otherwise a hipError_t (launch/config error) or
 *     VLG_ERR_* below; the Python side raises RuntimeError on non-zero
 *   - token-major activations use the INTERNAL row order  m = (b*N + n)*T + t
 *     (all frames of one slot contiguous: one T x d tile per (clip, slot));
 *     inputs/targets keep the public (B,T,N) order and are re-indexed in-kernel
 *
 * Grammar (ENFORCED: the Python binding is derived from this file - vlg/cabi.py reads it at import, types every entry
 * point from its prototype, finds arguments by their parameter names and takes every constant from its #define - and
 * the reader refuses, quoting the text, whatever is not listed here)
 *   - comments are of this kind only, never the double-slash kind
 *   - preprocessor lines: the include guard, the stdint.h include, #ifdef __cplusplus and #ifdef VLG_DIAG with their
 *     #endif, and `#define VLG_NAME <number>`, the number one integer or one `(x.yf)` float.  No function-like macro, no
 *     expression as a value, no #if / #elif / #else
 *   - a prototype returns int, int64_t, void or const char*, and NAMES every parameter; a name is declared once
 *   - scalar parameters are int, int64_t, uint32_t, uint64_t, float or double (no long, no unsigned, no size_t); every
 *     other parameter is a pointer, to one of those, to void, char, uint8_t, uint16_t, unsigned long long, or to a type
 *     this file typedefs.  No struct or typedef by value, no array, function pointer or variadic parameter
 *   - `stream` is the last parameter wherever it occurs
 *   - `typedef struct {...} name;` and `typedef <integer type> name;` only make `name` a legal pointer target
 *   - an enum gives every member its value (`NAME = n`)
 *   - prototypes between #ifdef VLG_DIAG and its #endif are the diagnostic build's: typed only when the library has them
 */
#ifndef VLG_HIP_H
#define VLG_HIP_H

#include <stdint.h>

/* Every entry point that writes per-block partial sums ("slabs") takes slab_capacity = the number of floats available at
 * `slabs`; it is checked against slab count x slab_stride on the host BEFORE the launch (VLG_ERR_SHAPE), so a short buffer
 * can never become an out-of-bounds device write. */
typedef uint16_t vlg_bf16;    /* bfloat16 bit pattern (activation storage of the bf16 mode) */

#ifdef __cplusplus
extern "C" {
#endif

#define VLG_ERR_SHAPE   1001   /* unsupported or inconsistent shape argument */
#define VLG_ERR_ALIGN   1002   /* pointer or leading dimension not 16-byte aligned */

/* library / build identification */
int         vlg_abi_version(void);
const char* vlg_build_arch(void);          /* "gfx950" */

/* DIAGNOSTIC BUILD ONLY (`make -C csrc diag` -> libvlg_hip_diag.so, compiled with -DVLG_DIAG; the product library does
 * NOT export these, keeps no mutable process-wide state and reads no environment: every kernel and slab plan follows from
 * the call's arguments).  That build also honours the development tuning variables (VLG_TUNE in csrc/common.h, read once).
 * Development tools load it through VLG_HIP_LIB (tools/diag, tools/ab). */
#ifdef VLG_DIAG
/* when set to a device buffer of 2*blocks uint64, every block of the next GEMM launches records {shader-clock ticks,
 * 100 MHz ticks} of its main loop; NULL switches it off (tools/diag/gemm_shader_clock.py) */
void vlg_debug_set_clock_probe(unsigned long long* buf);
void vlg_debug_set_conv_probe(unsigned long long* buf);
/* force the contraction depth per LDS tile of the 128x128 fp32 GEMM kernels (16 | 32; 0 = the library's own choice per
 * epilogue; the VLG_GEMM_BK environment variable sets the initial value) (tools/ab/gemm_ab.py) */
void vlg_debug_set_gemm_bk(int bk);
/* consecutive N tiles per block of the chained fp32 GEMM path (0 = never chain, -1 = the library's choice) */
void vlg_debug_set_gemm_run(int run);
#endif

/* ------------------------------------------------------------------ embedding
 * Object-slot embedding.  SELF-ORACLE; lookup semantics = nn.Embedding row gather
 * (reference src/models/simple.py:23,41).
 *   x[m,:] = cls_emb[slot_class[b,t,n]] + box_w @ slot_box[b,t,n] + box_b + time_emb[t]
 * bwd writes per-block partial slabs laid out [cls_emb | box_w | box_b | time_emb]
 * (the first tensors of the flat gradient buffer); vlg_reduce_slabs sums them. */
int vlg_embed_fwd(const int64_t* slot_class, const float* slot_box,
                  const float* cls_emb, const float* box_w, const float* box_b,
                  const float* time_emb, float* x,
                  int B, int T, int N, int d, int vocab, void* stream);
int vlg_embed_bwd_slabs(void);             /* upper bound of the number of slabs any vlg_embed_bwd launch writes */
int vlg_embed_bwd_slabs_for(int B, int T, int N, int d, int vocab);   /* slabs THIS shape's launch writes (<= the bound): reduce exactly these */
int vlg_embed_bwd(const float* dx, const int64_t* slot_class, const float* slot_box,
                  float* slabs, int64_t slab_stride, int64_t slab_capacity,
                  int B, int T, int N, int d, int vocab, void* stream);

/* ------------------------------------------------------------------ layer-norm
 * SELF-ORACLE (F.layer_norm arithmetic, biased variance, eps inside the sqrt).
 * bwd: dx_out = (dres ? dres : 0) + LN'(dy); partial [dgamma | dbeta] slabs. */
int vlg_layernorm_fwd(const float* x, const float* gamma, const float* beta,
                      float* y, float* mean, float* rstd,
                      int64_t rows, int d, float eps, void* stream);
/* same, y written as bf16 (the normalised activation only feeds a projection in the bf16 mode) */
int vlg_layernorm_fwd_bf16(const float* x, const float* gamma, const float* beta,
                           vlg_bf16* y, float* mean, float* rstd,
                           int64_t rows, int d, float eps, void* stream);
int vlg_layernorm_bwd_slabs(int64_t rows);
int vlg_layernorm_bwd(const float* dy, const float* x, const float* mean, const float* rstd,
                      const float* gamma, const float* dres, float* dx_out,
                      float* slabs, int64_t slab_stride, int64_t slab_capacity,
                      int64_t rows, int d, void* stream);
/* same, dy read as bf16 (it comes out of a projection's data gradient); x, dres, dx stay fp32 */
int vlg_layernorm_bwd_bf16(const vlg_bf16* dy, const float* x, const float* mean, const float* rstd,
                           const float* gamma, const float* dres, float* dx_out,
                           float* slabs, int64_t slab_stride, int64_t slab_capacity,
                           int64_t rows, int d, void* stream);

/* --------------------------------------------------------------------- dropout
 * SELF-ORACLE (tests/dropout_ref.py restates it): inverted dropout on a (rows, d) activation, fused into the layer-norm
 * launch that follows it (forward) or precedes it (backward).  Sites of the layout-token model, 2L + 1 of them:
 *   site 0        x0      = drop(embed(...))
 *   site 1 + 2l   xmid_l  = x_l    + drop(proj(att_l) + proj_b)
 *   site 2 + 2l   x_{l+1} = xmid_l + drop(ff2(gelu(...)) + ff2_b)          (the bias is inside the dropout)
 * Mask: thr = min(floor(p * 2^32 + 0.5), 2^32 - 1), scale = fp32(1 / (1 - thr / 2^32)) computed in double
 * (vlg_dropout_plan is the one place this rule lives).  Element (row m, column c) of site s at step k under the 64-bit
 * seed is KEPT iff x_w >= thr, x_w = word w = c % 4 of Philox4x32-10 with counter (m, c / 4, s, k) and key
 * (seed & 0xffffffff, seed >> 32); m is the internal row index.  One Philox call serves one float4; a mask bit is a
 * function of (m, c, s, k, seed) alone, never of the launch geometry; thr = 0 keeps everything with scale 1.
 * Values are chosen by SELECT, not by a product: select(v) = kept ? v * scale : 0, exactly 0 whatever a dropped v holds
 * (inf, NaN).  k is an int32 in DEVICE memory that the kernels read when they run, so a captured graph advances it by
 * replaying vlg_dropout_step_advance.  Nothing is stored for backward: it recomputes the mask.
 *
 * vlg_dropout_plan (host only; thr_host / scale_host are HOST pointers): VLG_ERR_SHAPE unless 0 <= p < 1.
 *
 * vlg_dropout_add_layernorm_fwd:  x_out = (resid ? resid : 0) + select(y);  h = LN(x_out), mean / rstd saved, with
 * vlg_layernorm_fwd's arithmetic, d set, row grouping and wave-per-row layout.  resid may be NULL (site 0).  x_out may
 * BE y (in place); every other overlap among y, resid, x_out, h is refused.  _bf16: h stored as bf16, as
 * vlg_layernorm_fwd_bf16 does.  Algorithmic bytes per row: (8 + 4 [resid] + 4 | 2 [h]) * d.
 *
 * vlg_layernorm_bwd_dropout:  exactly vlg_layernorm_bwd - dx_out and every slab bit for bit: it is the same kernel with
 * its second output switched on - plus dy_drop = select(dx_out) under the mask of the site that FEEDS this layer-norm (the gradient of that site's y).  dres
 * may BE dx_out, as in vlg_layernorm_bwd; dy_drop overlaps none of dy, x, dres, dx_out; dx_out overlaps neither dy nor x.
 * _bf16: dy read as bf16.  One more 4 * d bytes per row than vlg_layernorm_bwd, no extra launch.
 *
 * Refusals, all before anything is enqueued.  VLG_ERR_SHAPE: rows < 1 or rows >= 2^32 (the row is a 32-bit counter
 * word), d outside vlg_layernorm_fwd's set, site < 0, scale outside [1, 2^32], step NULL, a short slab buffer, a
 * forbidden overlap.  VLG_ERR_ALIGN: a NULL pointer (resid and dres excepted) or y, resid, x_out, gamma, beta, fp32 h,
 * dy, x, dres, dx_out, dy_drop not 16-byte aligned (bf16 h / dy: 8), mean, rstd, slabs, step not 4.
 *
 * vlg_dropout_step_advance: a one-thread launch, *step += 1. */
int vlg_dropout_plan(double p, uint32_t* thr_host, float* scale_host);
int vlg_dropout_add_layernorm_fwd(const float* y, const float* resid, const float* gamma, const float* beta,
                                  float* x_out, float* h, float* mean, float* rstd,
                                  int64_t rows, int d, float eps,
                                  uint32_t thr, float scale, uint64_t seed, int site, const int* step, void* stream);
int vlg_dropout_add_layernorm_fwd_bf16(const float* y, const float* resid, const float* gamma, const float* beta,
                                       float* x_out, vlg_bf16* h, float* mean, float* rstd,
                                       int64_t rows, int d, float eps,
                                       uint32_t thr, float scale, uint64_t seed, int site, const int* step, void* stream);
int vlg_layernorm_bwd_dropout(const float* dy, const float* x, const float* mean, const float* rstd,
                              const float* gamma, const float* dres, float* dx_out, float* dy_drop,
                              float* slabs, int64_t slab_stride, int64_t slab_capacity,
                              int64_t rows, int d,
                              uint32_t thr, float scale, uint64_t seed, int site, const int* step, void* stream);
int vlg_layernorm_bwd_dropout_bf16(const vlg_bf16* dy, const float* x, const float* mean, const float* rstd,
                                   const float* gamma, const float* dres, float* dx_out, float* dy_drop,
                                   float* slabs, int64_t slab_stride, int64_t slab_capacity,
                                   int64_t rows, int d,
                                   uint32_t thr, float scale, uint64_t seed, int site, const int* step, void* stream);
int vlg_dropout_step_advance(int* step, void* stream);

/* ------------------------------------------------------------------------ GEMM
 * fp32 MFMA (v_mfma_f32_32x32x2_f32) GEMMs for the dense QKV/FFN/head projections.
 * SELF-ORACLE (F.linear arithmetic); the reference's dense contraction is conv only.
 *
 * vlg_linear_fwd : C[M,N] = A[M,K] . W[N,K]^T + bias      (epilogue selects extras)
 * vlg_linear_dgrad: C[M,K] = A[M,N] . W[N,K]              (epilogue selects extras)
 * vlg_linear_wgrad: slabs[s][N*K + N] = partial ( dY[M,N]^T . X[M,K] | colsum dY )
 */
#define VLG_EPI_NONE   0
#define VLG_EPI_BIAS   1   /* + bias[col]                                            */
#define VLG_EPI_GELU   2   /* aux_out = pre-activation, C = gelu(pre)   (needs BIAS) */
#define VLG_EPI_RESID  4   /* C = acc (+bias) + aux_in[row,col]                      */
#define VLG_EPI_DGELU  8   /* C = acc * gelu'(aux_in[row,col])                       */
#define VLG_EPI_BF16   16  /* v_mfma_f32_32x32x16_bf16 with fp32 accumulate (BASELINE.json configs[2]); fp32 operands are rounded
                              to bf16 on their way to LDS, bf16 ones (storage bits below) are copied; default is native
                              fp32 MFMA */
#define VLG_EPI_SPLIT3 256  /* fp32 tensors, fp32-grade result on the bf16 matrix cores: each operand is split exactly into
                              three bf16 terms and a product block is six v_mfma_f32_32x32x16_bf16 (a1b1 + a1b2 + a2b1 +
                              a1b3 + a2b2 + a3b1, fp32 accumulate; the dropped terms are <= 3 * 2^-24 |a||b|)          */
#define VLG_EPI_ACT_GELU 512 /* native fp32 path: the activation operand (A of vlg_linear_fwd with BIAS | RESID, X of
                              vlg_linear_wgrad) holds PRE-activations and passes through GELU on its way to LDS - the
                              FFN hidden activation gelu(u) is then never written to HBM: the first projection stores
                              u only (plain BIAS epilogue), the second projection and its weight gradient recompute    */
#define VLG_EPI_GELU_GRAD 1024 /* native fp32 and bf16 paths, with BIAS | GELU: aux_out = gelu'(pre) instead of the pre-activation itself.
                              The epilogue has exp(-pre^2/2) and the tail polynomial in registers anyway, and the backward
                              pass needs the pre-activation for nothing but this derivative: the data gradient of the
                              second projection then takes VLG_EPI_MUL instead of VLG_EPI_DGELU (one multiply per
                              element instead of ~20 vector instructions - which the fp32 MFMA kernels pay for in matrix
                              time, see csrc/common.h)                                                                  */
#define VLG_EPI_MUL    2048 /* native fp32 and bf16 paths, vlg_linear_dgrad: C = acc * aux_in[row,col]                            */
/* bf16 ACTIVATION STORAGE (with VLG_EPI_BF16 only): the activation operands named below are vlg_bf16 arrays in
 * HBM instead of float - half the bytes of a mode that is HBM-bound.  Biases, gradient slabs, master weights and
 * the residual stream stay fp32; leading dimensions count elements.                                             */
#define VLG_EPI_A_BF16   32   /* first operand (A of fwd, dY of dgrad / wgrad) is bf16                          */
#define VLG_EPI_B_BF16   64   /* second operand is bf16: X of wgrad, W of fwd / dgrad (the shadow vlg_adam_step_bf16 keeps) */
#define VLG_EPI_OUT_BF16 128  /* C and the epilogue's auxiliary operands (aux_in, aux_out) are bf16             */
int vlg_linear_fwd(const void* A, int lda, const void* W, int ldw, const float* bias,
                   void* C, int ldc, const void* aux_in, void* aux_out,
                   int64_t M, int N, int K, int epilogue, void* stream);
int vlg_linear_dgrad(const void* dY, int ldy, const void* W, int ldw,
                     void* dX, int ldx, const void* aux_in,
                     int64_t M, int N, int K, int epilogue, void* stream);
int vlg_linear_wgrad_slabs(int64_t M, int N, int K);                 /* slab count of a flags = 0 launch */
int vlg_linear_wgrad_slabs_for(int64_t M, int N, int K, int flags);  /* slab count of a launch with these flags */
int vlg_linear_wgrad(const void* dY, int ldy, const void* X, int ldx,
                     float* slabs, int64_t slab_stride, int64_t slab_capacity,
                     int64_t M, int N, int K, int flags /* VLG_EPI_BF16 | storage bits */, void* stream);
/* vlg_linear_wgrad and vlg_linear_dgrad of ONE projection (same dY) as one call: accepts exactly what the two calls accept
 * (the weight gradient takes the mode and the dY / X storage bits of `epilogue`), and results are bit for bit those of the
 * two calls.  Native fp32 tensors and the bf16-storage step (bf16 W / X / dX) with epilogue VLG_EPI_NONE | VLG_EPI_MUL can
 * run as ONE launch whose blocks are dealt both problems at once; everything else runs as the two launches.  Which it is,
 * and on which tiles, is part of the call's plan (gemm_plan in csrc/gemm.hip, a function of shape, flags and leading
 * dimensions alone; vlg_linear_plan below reports it).  Like every vlg_linear_* call it is checked and planned completely
 * before its first launch: a call that is refused - for either product - has enqueued nothing, riders included.
 * Replaces the two autograd nodes of one nn.Linear backward. */
int vlg_linear_dgrad_wgrad(const void* dY, int ldy, const void* W, int ldw, void* dX, int ldx, const void* aux_in,
                           const void* X, int ldxx, float* slabs, int64_t slab_stride, int64_t slab_capacity,
                           int64_t M, int N, int K, int epilogue,
                           const int64_t* rider_table /* NULL, or a vlg_reduce_slabs_table table over OTHER buffers (a finished
                              gradient bucket's partial sums): reduced by extra blocks of the same launch where the products are
                              fused, by its own launch otherwise; rows as vlg_reduce_slabs_table requires, 1 <= rider_rows
                              <= 4096 */, int rider_rows, void* stream);
/* The plan of a vlg_linear_* call: a pure host-side planner like the slab-count queries (no GPU, no launch, no state), and
 * the same function the entry points launch from.  (M, N, K, flags) as the call takes them; the leading dimensions in the
 * call's own order: fwd (lda, ldw, ldc), dgrad (ldy, ldw, ldx), wgrad (ldy, ldx, unused), pair (ldy, ldw, ldx) and ldxx
 * (unused by the others).  Returns 0 and fills *plan, or the error the call returns on shape, flag and leading-dimension
 * grounds (pointers, slab stride and capacity are taken to be fine; *plan is zeroed). */
#define VLG_CALL_FWD   0
#define VLG_CALL_DGRAD 1
#define VLG_CALL_WGRAD 2
#define VLG_CALL_PAIR  3   /* vlg_linear_dgrad_wgrad: p[0] = the data gradient, p[1] = the weight gradient */
#define VLG_GEMM_F32   0   /* kernel family: native fp32 MFMA (csrc/gemm.hip) */
#define VLG_GEMM_BF16  1   /* bf16 MFMA (csrc/gemm_bf16.hip) */
#define VLG_GEMM_F32X3 2   /* fp32 as three bf16 terms (csrc/gemm_split.hip) */
typedef struct vlg_gemm_problem {
    int bm, bn, bk;            /* block tile of the output and contraction depth per LDS tile */
    int run;                   /* consecutive N tiles one block computes */
    int splits;                /* ranges of the contraction extent = slabs of a weight gradient */
    int blocks;                /* blocks of the launch that work on this problem */
    int64_t rows_per_split;    /* contraction rows per range */
} vlg_gemm_problem;
typedef struct vlg_gemm_plan {
    int family;                /* VLG_GEMM_* */
    int launches;              /* GEMM launches: 1, or 2 for a pair that runs as its two single calls (weight gradient first) */
    int problems;              /* entries of p: 1, or 2 for VLG_CALL_PAIR */
    int fused;                 /* 1 = a pair as one launch of the pair kernel, on the tiles p names */
    vlg_gemm_problem p[2];
} vlg_gemm_plan;
int vlg_linear_plan(int call, int64_t M, int N, int K, int flags, int lda, int ldb, int ldc, int ldxx, vlg_gemm_plan* plan);


/* ------------------------------------------------------------------- attention
 * Temporal encoder core: causal softmax attention along T for each (clip, slot,
 * head); one wavefront owns one T x 64 tile staged in LDS.  SELF-ORACLE.
 * qkv is [rows, 3d] = [q | k | v]; head h owns columns h*64..h*64+63 of each. */
int vlg_attention_fwd(const float* qkv, float* o, int64_t n_seq, int T, int d, void* stream);
int vlg_attention_bwd(const float* qkv, const float* dout, float* dqkv,
                      int64_t n_seq, int T, int d, void* stream);
/* same with every tensor stored as bf16 (arithmetic stays fp32) */
int vlg_attention_fwd_bf16(const vlg_bf16* qkv, vlg_bf16* o, int64_t n_seq, int T, int d, void* stream);
int vlg_attention_bwd_bf16(const vlg_bf16* qkv, const vlg_bf16* dout, vlg_bf16* dqkv,
                           int64_t n_seq, int T, int d, void* stream);
/* The same attention for ONE query position p against a K/V cache (generation while the history is shorter than the
 * window; DESIGN.md, "Generation").  qkv is the [n_seq*T, 3d] buffer above; for sequence r and head h the query is row
 * r*T + p, keys and values are rows r*T + j, j <= p.  Rows j > p are never read (they may hold anything, NaN included).
 * o is [n_seq, d] with leading dimension ldo >= d elements: o[r, :] is written and nothing else.  Scale 1/8 and the
 * max-subtracted expf softmax of vlg_attention_fwd: p = T-1 agrees with row T-1 of that entry to rounding.
 * VLG_ERR_SHAPE, nothing enqueued: T outside {4, 8, 16, 32}, p outside [0, T), d % 64 != 0, ldo < d, n_seq < 1.
 * VLG_ERR_ALIGN: qkv or o NULL or misaligned (16 bytes fp32, 8 bytes bf16). */
int vlg_attention_step(const float* qkv, float* o, int64_t n_seq, int T, int d, int p, int64_t ldo, void* stream);
int vlg_attention_step_bf16(const vlg_bf16* qkv, vlg_bf16* o, int64_t n_seq, int T, int d, int p, int64_t ldo, void* stream);

/* ---------------------------------------------------------------------- losses
 * Fused softmax-cross-entropy + smooth-L1 + IoU, forward and backward in one pass.
 *   CE    : nn.CrossEntropyLoss(reduction='mean')   reference src/trainer.py:124,250
 *   weights 40 / 20 / 10                            reference src/trainer.py:248-250
 *   smooth-L1, IoU : SELF-ORACLE
 * out/dout are [rows, ld] with columns [0,C) = logits, [C,C+4) = raw box.
 * loss_out[4] = {total, smooth_l1, iou, ce}.  scratch holds >= vlg_layout_loss_scratch()
 * floats, 16-byte aligned, ZERO-INITIALISED ONCE by the caller: scratch[1] is the integer ticket by which the last
 * block of the (single) launch folds the per-block partials into loss_out; that block leaves it zero again. */
int vlg_layout_loss_scratch(void);
int vlg_layout_loss(const float* out, int ld, const int64_t* tgt_class, const float* tgt_box,
                    const float* valid, float* dout, float* loss_out, float* scratch,
                    int B, int T, int N, int n_classes, float beta, float iou_eps,
                    float w_reg, float w_iou, float w_ce, void* stream);
/* The same launch with the options of the classification and overlap terms ("Loss options"; definition in
 * fp64: tests/loss_ext_ref.py).  One kernel body serves both entries; the options are its compile-time parameters and
 * vlg_layout_loss is the all-off instantiation, so class_weight = NULL, label_smoothing = 0, flags = 0 gives its bits.
 *   class_weight     NULL, or n_classes floats >= 0 ON THE DEVICE: F.cross_entropy(weight=) - token i counts w[y_i]
 *                    times, and the CE mean divides by W = sum_i valid_i w[y_i] instead of the valid count.  W == 0 (every
 *                    valid target has weight 0): the CE term and its gradient are exactly 0 (torch: NaN).  Every block
 *                    forms W by the same operations in the same order, so a launch is reproducible bit for bit; that
 *                    loop reads tgt_class as well (8 B per token).  The box terms keep the valid count.
 *   label_smoothing  eps in [0, 1): F.cross_entropy(label_smoothing=) - the target distribution of token i is
 *                    q_i[c] = (eps/C) w[c] + (1-eps) w[y_i] [c == y_i]  (w = 1 without weights);
 *                    CE = (1/W) sum_i valid_i sum_c q_i[c] (-log p_i[c]),  dCE/dz_i[k] = valid_i/W (Q_i p_i[k] - q_i[k]),
 *                    Q_i = sum_c q_i[c]
 *   flags            VLG_LOSS_GIOU: the overlap term is mean_valid(1 - giou) in [0, 2],
 *                    giou = inter/(uni + iou_eps) - (ac - uni)/(ac + iou_eps), ac = the area of the smallest box
 *                    enclosing both; min / max split 0.5 / 0.5 at a tie and clamp passes the gradient at 0, as torch's.
 *                    loss_out[2] is then that term.  Unlike 1 - IoU it has a gradient for boxes that do not touch.
 * Layout, scratch contract (ticket reset), ld rule and alignment checks are vlg_layout_loss's.  VLG_ERR_SHAPE, nothing
 * enqueued: label_smoothing outside [0, 1) or NaN, a flag bit other than VLG_LOSS_GIOU, and every refusal of the plain entry. */
#define VLG_LOSS_GIOU 1
int vlg_layout_loss_ext(const float* out, int ld, const int64_t* tgt_class, const float* tgt_box,
                        const float* valid, const float* class_weight, float* dout, float* loss_out, float* scratch,
                        int B, int T, int N, int n_classes, float beta, float iou_eps,
                        float w_reg, float w_iou, float w_ce, float label_smoothing, int flags, void* stream);

/* ------------------------------------------------------------------ Gaussian box head (csrc/box_nll.hip)
 * SELF-ORACLE (tests/boxhead_ref.py restates it in fp64); DESIGN.md, "Gaussian box head".  With the option
 * LayoutConfig(box_head="gaussian") a head-output row holds [0,C) logits | [C,C+4) raw mean | [C+4,C+8) raw scale |
 * [C+8,C+12) padding.  For token row m = (b*N + n)*T + t, targets at src = (b*T + t)*N + n as the loss kernel reads them:
 *   mu_k    = sigmoid(out[m, C+k])                  a CONSTANT here: no gradient reaches the mean, which the smooth-L1
 *                                                   and IoU terms keep training exactly as they did
 *   g_k     = sigmoid(out[m, C+4+k]),  s_k = s_min + (s_max - s_min) g_k,  sigma_k = exp(s_k)
 *   e_k     = (tgt_k - mu_k) exp(-s_k)
 *   nll_m   = 1/4 sum_k (e_k^2 / 2 + s_k + ln(2 pi) / 2)
 *   cover_m = 1/4 sum_k [ |tgt_k - mu_k| <= sigma_k ]          (a calibrated head reads 0.683)
 *   cnt = max(sum valid, 1),  box_nll = 1/cnt sum_m valid_m nll_m,  box_cover = 1/cnt sum_m valid_m cover_m
 *   dout[m, C+4+k] = w_nll valid_m/cnt 1/4 (1 - e_k^2) (s_max - s_min) g_k (1 - g_k),   dout[m, C+8 .. C+11] = 0
 * out / dout are [rows, ld], ld >= C+12 and a multiple of 4.  READ: out[m, C .. C+8), tgt_box, valid - nothing else (the
 * logits and the padding columns may hold anything, NaN included).  WRITTEN: dout[m, C+4 .. C+12) and nothing else of
 * dout - the loss launch wrote [0, C+4) - with plain vector stores.
 * loss_io is 8 floats.  The launch writes [4] = box_nll, [5] = box_cover, [6] = [7] = 0 and [0] = [0] + w_nll * box_nll,
 * once.  THE RULE: call it once, in stream order, after the vlg_layout_loss[_ext] launch that wrote [0..3].
 * An invalid token is multiplied by its valid flag, as in the loss kernel: a finite row with valid == 0 contributes
 * exact zeros; a NON-FINITE mean, scale or target of an invalid token still makes its gradient row and both sums NaN.
 * scratch: >= vlg_layout_box_nll_scratch() floats of its OWN (not the loss launch's), 16-byte aligned, zeroed once by the
 * caller; scratch[1] is the ticket by which the last block folds the per-block partials in block order, and is left zero.
 * No float atomics: two launches on the same inputs agree bit for bit.  Every block forms the valid count itself.
 * VLG_ERR_SHAPE, nothing enqueued: n_classes != 20, B, T or N < 1, ld < C+12 or not a multiple of 4, !(s_min < s_max) or
 * either not finite, w_nll negative or not finite.  VLG_ERR_ALIGN: out, dout, tgt_box, valid or scratch NULL or not
 * 16-byte aligned, loss_io NULL.  52 B in and 32 B out per token: bound by the launch, not by bytes. */
#define VLG_BOX_S_MIN (-7.0f)   /* the bounds the DECODING entries below use for log sigma; vlg.spec.BOX_S_MIN / BOX_S_MAX */
#define VLG_BOX_S_MAX (0.0f)
int vlg_layout_box_nll_scratch(void);
int vlg_layout_box_nll(const float* out, int ld, const float* tgt_box, const float* valid, float* dout, float* loss_io,
                       float* scratch, int B, int T, int N, int n_classes, float s_min, float s_max, float w_nll,
                       void* stream);

/* ------------------------------------------------------------------ per-clip attention (option attention = "clip")
 * Block-causal softmax attention over ALL T*N tokens of a clip, per (clip, head): token (t, n) attends to every slot of
 * frames <= t; slots with valid == 0 (valid may be NULL: none) are never keys, except for themselves.  SELF-ORACLE
 * (oracle/layout_spec.py:clip_attention) - the reference has no attention; this is the "per-clip tile" reading of
 * BASELINE.json's temporal encoder next to the per-slot default (vlg_attention_fwd / _bwd).  fp32, head dim 64, T*N a multiple
 * of 32.  qkv [B*N*T, 3d] / out, dout [B*N*T, d] in the internal row order; valid (B,T,N) floats in the public order;
 * lse and delta: B * (d/64) * T*N floats each (log-sum-exp in the log2 domain, written by fwd; <dO, O>, scratch of bwd).
 * valid values: a slot is visible as a key iff its value is > 0 (any positive float, not only 1; -0.0, 0 and every negative
 * value pad it), as the specification has it.  NaN is outside the contract: the kernels test `<= 0` and would see such a
 * slot, the specification tests `> 0` and would not.  A clip may be padded anywhere - whole leading frames, every slot.
 * bwd = two launches (query owner: dQ; key owner: dK, dV): every gradient element has one owner, no atomics.
 * Refusals, before anything is enqueued: VLG_ERR_SHAPE for a shape outside the above; VLG_ERR_ALIGN if qkv, out (fwd) or qkv,
 * out, dout, dqkv (bwd) is NULL or not 16-byte aligned, or if lse (fwd, bwd) or delta (bwd) is NULL.  Only valid may be NULL. */
int vlg_attention_clip_fwd(const float* qkv, const float* valid, float* out, float* lse,
                           int64_t B, int T, int N, int d, void* stream);
int vlg_attention_clip_bwd(const float* qkv, const float* valid, const float* out, const float* dout, const float* lse,
                           float* delta, float* dqkv, int64_t B, int T, int N, int d, void* stream);
/* bf16 storage (precision "bf16"): qkv, out, dout and dqkv bf16; valid, lse and delta fp32 in the layouts above.  Products
 * on bf16 MFMA with fp32 accumulation; scores, softmax statistics, lse and delta fp32; P and dS rounded to bf16 only as
 * MFMA operands; O, dQ, dK, dV rounded once on store.  Same shape contract, refusals (a NULL or misaligned tensor included)
 * and return codes as the fp32 entries: one host front end serves both. */
int vlg_attention_clip_fwd_bf16(const vlg_bf16* qkv, const float* valid, vlg_bf16* out, float* lse,
                                int64_t B, int T, int N, int d, void* stream);
int vlg_attention_clip_bwd_bf16(const vlg_bf16* qkv, const float* valid, const vlg_bf16* out, const vlg_bf16* dout,
                                const float* lse, float* delta, vlg_bf16* dqkv,
                                int64_t B, int T, int N, int d, void* stream);
/* The same attention for the N queries of ONE frame p against a K/V cache (generation while the history is shorter than the
 * window, LayoutEngine(clip_cache=True); DESIGN.md, "Generation").  qkv and valid are the buffers above.  Per clip b and head
 * h the queries are the tokens (p, n): query n is row (b*N + n)*T + p of qkv, columns h*64 .. + 63.  Query (p, n) sees key
 * (j, n') iff j <= p and (valid == NULL or valid[(b*T + j)*N + n'] > 0 or (j, n') == (p, n)) - vlg_attention_clip_fwd
 * restricted to the query tokens s = p*N + n of its frame-major walk over the key tokens s < (p + 1)*N, with its scale,
 * its max-subtracted softmax (masked keys are -inf before the row maximum) and, in bf16, its rounding points.
 * o is [B*N, d] with leading dimension ldo >= d elements: o[b*N + n, h*64 .. + 63] is written and nothing else; no lse
 * (generation has no backward).  NEVER READ: rows of qkv at positions j > p and valid[:, j > p] - they may hold anything,
 * NaN included; what the last 32-key tile holds past (p + 1)*N reaches neither a load nor the P.V product.
 * The fp32 entry accumulates its scores in fp64 (a step computes few rows, and at |score| ~ 100 one chain of fp32 sums shows
 * against fp64, as in vlg_attention_step); softmax and P.V are the forward's.  The bf16 entry is the forward's arithmetic throughout.
 * One block per (clip, head, 32 queries); its four waves split the key tiles and merge in a fixed order: no atomics, the
 * same bits from run to run and for a clip alone or inside a larger batch.
 * VLG_ERR_SHAPE, nothing enqueued: the shape contract of vlg_attention_clip_fwd, p outside [0, T), ldo < d.
 * VLG_ERR_ALIGN: qkv or o NULL or misaligned (16 bytes fp32, 8 bytes bf16; bf16: ldo not a multiple of 4).  Only valid may
 * be NULL. */
int vlg_attention_clip_step(const float* qkv, const float* valid, float* o,
                            int64_t B, int T, int N, int d, int p, int64_t ldo, void* stream);
int vlg_attention_clip_step_bf16(const vlg_bf16* qkv, const float* valid, vlg_bf16* o,
                                 int64_t B, int T, int N, int d, int p, int64_t ldo, void* stream);

/* ------------------------------------------------------------------ frame attention (option attention = "factored")
 * Softmax attention INSIDE a frame, per (clip, head): token (t, n) attends to the tokens (t, m) of its own frame with
 * valid[(b*T + t)*N + m] > 0 (valid may be NULL: all), and to itself - the per-clip rule for padded slots, unchanged: a
 * padded slot is never a key except its own.  Not causal in n; nothing crosses frames.  SELF-ORACLE: clip_attention of the
 * CPU specification on the B*T one-frame clips.  The odd layers of attention = "factored" (even layers: vlg_attention_fwd /
 * _bwd / _step, causal along time per slot), so all mixing along time stays causal.
 * The entries are the per-clip ones with that visibility rule: the same buffers, row order, scale, head layout, lse and
 * delta layouts (log2 domain), fp64 score path of the fp32 step, bf16 rounding points, one owner per gradient element (no
 * atomics; a clip's bits depend neither on B nor on the run), shape contract (T*N a multiple of 32) and refusals - the
 * argument lists and the host front end are shared, and a refused call enqueues nothing.  A token that sees only itself
 * returns its V row bit for bit.
 * What the frame-local walk reads: a query-owner block the key tiles from the first token of its first frame to the last
 * token of its last frame, a key-owner block the query tiles of its own frames.  vlg_attention_frame_step reads the rows of
 * position p ALONE - q, k and v of the N tokens (p, n) - and valid[:, p]: rows of every other position, EARLIER ones
 * included, and their valid entries may hold anything, NaN included.  It needs no cache: generation calls it on the q k v
 * rows the projection just wrote at position p. */
int vlg_attention_frame_fwd(const float* qkv, const float* valid, float* out, float* lse,
                            int64_t B, int T, int N, int d, void* stream);
int vlg_attention_frame_bwd(const float* qkv, const float* valid, const float* out, const float* dout, const float* lse,
                            float* delta, float* dqkv, int64_t B, int T, int N, int d, void* stream);
int vlg_attention_frame_fwd_bf16(const vlg_bf16* qkv, const float* valid, vlg_bf16* out, float* lse,
                                 int64_t B, int T, int N, int d, void* stream);
int vlg_attention_frame_bwd_bf16(const vlg_bf16* qkv, const float* valid, const vlg_bf16* out, const vlg_bf16* dout,
                                 const float* lse, float* delta, vlg_bf16* dqkv,
                                 int64_t B, int T, int N, int d, void* stream);
int vlg_attention_frame_step(const float* qkv, const float* valid, float* o,
                             int64_t B, int T, int N, int d, int p, int64_t ldo, void* stream);
int vlg_attention_frame_step_bf16(const vlg_bf16* qkv, const float* valid, vlg_bf16* o,
                                  int64_t B, int T, int N, int d, int p, int64_t ldo, void* stream);

/* ------------------------------------------------------------------ random draws (csrc/philox.h)
 * Every draw of generation, scheduled sampling, augmentation and the Gaussian box head below is a word of Philox4x32-10 on
 * counter (index, step, stream, 0) under key (seed & 0xffffffff, seed >> 32).  `stream` keeps the draws of one (index, step)
 * apart; this is the one table of them, and a new kind of draw takes a new entry.  The rules below name them by number.
 * The counter rule, word by word:  word 0: the index (token, track or clip);  word 1: the step;  word 2: the stream;
 * word 3: the sample index, 0 for every other draw - only vlg_layout_decode_samples / vlg_layout_decode_append_samples set it.
 * The dropout mask above is not in it: its third counter word is its SITE, and its own seed keeps it apart from these. */
enum vlg_rng_stream {
    VLG_RNG_CLASS_DRAW   = 0,   /* u of a sampled class: vlg_layout_decode*, and a replaced token of vlg_layout_mix_inputs */
    VLG_RNG_SCHED_COIN   = 1,   /* scheduled sampling: truth or prediction */
    VLG_RNG_CLIP_DRAW    = 2,   /* augmentation, per clip: flip, zoom, shift */
    VLG_RNG_TRACK_DROP   = 3,   /* augmentation, per track: drop */
    VLG_RNG_TOKEN_JITTER = 4,   /* augmentation, per input token: jitter */
    VLG_RNG_BOX_NORMAL   = 5    /* the sampled box of vlg_layout_decode*_ext */
};

/* ------------------------------------------------------------------ generation (csrc/decode.hip)
 * The forward-only tail of an autoregressive rollout (reference src/trainer.py:453-476 rolls its pixel model out the same
 * way: predict, argmax, append, slide).  SELF-ORACLE (tests/decode_ref.py); rule and rooflines: DESIGN.md, "Generation".
 *
 * Final layer-norm + head on the LAST frame's rows only (generation needs no other row).
 * x: residual stream [B*N*T, d] fp32 in the internal row order m = (b*N + n)*T + t; only rows m = r*T + (T-1),
 * r = b*N + n, are read.  out_last[r, :] = head_w[n_out, d] . LN(x[m, :]; gamma, beta, eps) + head_b,  [B*N, n_out] fp32.
 * F.layer_norm arithmetic as vlg_layernorm_fwd (biased variance, eps inside the sqrt); fp32 throughout, fp32 MASTER weights
 * in every precision mode.  d % 64 == 0, d <= 1024, 1 <= n_out <= 32, else VLG_ERR_SHAPE; 16-byte-aligned pointers, else
 * VLG_ERR_ALIGN. */
int vlg_head_last_frame(const float* x, const float* gamma, const float* beta, const float* head_w, const float* head_b,
                        float* out_last, int B, int T, int N, int d, int n_out, float eps, void* stream);
/* The same on frame t_read, 0 <= t_read < T (else VLG_ERR_SHAPE): rows m = r*T + t_read are read and no other.  One kernel,
 * one arithmetic: vlg_head_last_frame IS the t_read = T-1 call and gives bit-identical results.  A rollout whose history is
 * still shorter than the window reads the newest real frame with it; T = 1 serves a compact [B*N, d] residual stream. */
int vlg_head_frame(const float* x, const float* gamma, const float* beta, const float* head_w, const float* head_b,
                   float* out_last, int B, int T, int N, int d, int n_out, int t_read, float eps, void* stream);
/* One decoding step: choose the next frame from out_last ([B*N, n_classes + 4]: logits | raw box), write it to
 * gen_cls[b, step, n] / gen_box[b, step, n, :] ((B, steps, N) int64 / (B, steps, N, 4) fp32; other step indices are not
 * touched) and write the NEXT window: cls_out[:, t] = cls_in[:, t + 1] for t < T - 1, cls_out[:, T - 1] = the new frame
 * (boxes likewise); valid_out (may be NULL) = 1.0f where cls_out < n_classes else 0.0f.  (B, T, N) public order.
 * cls_in / box_in are only read; in and out must not alias (VLG_ERR_SHAPE).
 *   box    sigmoid(raw)
 *   class  temperature == 0: the first maximum of the logits (torch.argmax).  temperature > 0: kept set = every class
 *          (top_k == 0) or the top_k largest RAW logits (equal values: lower index first); z = logit / temperature,
 *          p = expf(z - max kept z) on the kept set, 0 elsewhere; cum = running sum of p in class order, S its last value
 *          (fp32); the class is the first kept c with cum_c >= u * S (the last kept one if rounding leaves none)
 *   u      (x0 >> 8) * 2^-24 + 2^-25, x0 = first word of Philox4x32-10 on counter (b*N + n, step, 0, 0) under key
 *          (seed & 0xffffffff, seed >> 32): a draw depends on token, step and seed alone, never on the launch geometry
 *   keep_padded != 0: a slot whose class in frame T-1 of cls_in is >= n_classes keeps that class id and its box
 * VLG_ERR_SHAPE before anything is enqueued: temperature < 0 or not finite, top_k < 0 or > n_classes, n_classes < 1 or
 * n_classes + 4 > 32, step outside [0, steps), B, T or N < 1.  Box pointers and out_last 16-byte, class pointers 8-byte
 * aligned, else VLG_ERR_ALIGN. */
int vlg_layout_decode(const float* out_last, const int64_t* cls_in, const float* box_in,
                      int64_t* cls_out, float* box_out, float* valid_out, int64_t* gen_cls, float* gen_box,
                      int B, int T, int N, int n_classes, int steps, int step,
                      float temperature, int top_k, uint64_t seed, int keep_padded, void* stream);
/* The same step while the history holds pos < T frames: nothing slides, the window (cls, box, valid; (B, T, N) public
 * order) is updated IN PLACE.  The newest frame pos-1 is read (keep_padded looks at it), the frame drawn from out_last by
 * the rule above (one device function serves both entries; Philox counter (b*N + n, step, 0, 0)) is written to frame pos
 * of cls / box, with valid[:, pos] (valid may be NULL) = 1.0f where the class is < n_classes else 0.0f, to
 * gen_cls[:, step] / gen_box[:, step], and to the compact copy frame_cls (B, N) int64 / frame_box (B, N, 4) fp32 that the
 * next step's embedding reads (vlg_embed_fwd with T = 1).  No other element of any buffer is touched; plain vector stores.
 * Refusals as vlg_layout_decode, plus VLG_ERR_SHAPE for pos outside [1, T), a NULL frame_cls / frame_box, or any two of
 * the eight buffers overlapping. */
int vlg_layout_decode_append(const float* out_last, int64_t* cls, float* box, float* valid,
                             int64_t* gen_cls, float* gen_box, int64_t* frame_cls, float* frame_box,
                             int B, int T, int N, int n_classes, int pos, int steps, int step,
                             float temperature, int top_k, uint64_t seed, int keep_padded, void* stream);
/* The two steps above with a row stride and a SAMPLED box (the Gaussian box head): the argument lists of vlg_layout_decode /
 * vlg_layout_decode_append plus `ld` after out_last - the row stride of out_last in floats, ld >= n_classes + 4 and a
 * multiple of 4 - and `box_temperature` after top_k.  One front end and one kernel body serve both pairs; box sampling is a
 * compile-time parameter of it, and the plain entries are the ld = n_classes + 4, box_temperature = 0 calls.
 *   box    box_temperature == 0: sigmoid(raw), exactly as above (the kernel instantiation of the plain entries).
 *          box_temperature = tau > 0 (needs ld >= n_classes + 8 and n_classes + 8 <= 32, else VLG_ERR_SHAPE): out_last rows
 *          are [logits | raw mean | raw scale | ...];  (x0, x1, x2, x3) = all four words of Philox4x32-10 on counter
 *          (b*N + n, step, 5, 0) under the call's key (stream VLG_RNG_BOX_NORMAL of enum vlg_rng_stream above);
 *          u_i = (x_i >> 8) * 2^-24 + 2^-25 evaluated in fp32 as the class draw's u (so u may round to 1.0, which gives z = 0);  z0 = sqrt(-2 ln u0) cos(2 pi u1), z1 = sqrt(-2 ln u0) sin(2 pi u1), z2, z3 likewise
 *          from u2, u3;  mu_k = sigmoid(raw mean_k), sigma_k = exp(VLG_BOX_S_MIN + (VLG_BOX_S_MAX - VLG_BOX_S_MIN)
 *          sigmoid(raw scale_k));  box_k = min(max(mu_k + tau sigma_k z_k, 0), 1).
 *   class  untouched: the same counter (b*N + n, step, 0, 0), the same rule.
 *   A slot kept by keep_padded keeps its box.  Columns >= n_classes + 8 (tau == 0: >= n_classes + 4) are never read.  A draw
 *   is a function of (token, step, seed) alone.
 * Refusals as the plain entries, plus VLG_ERR_SHAPE for a bad ld and for box_temperature negative, NaN or infinite. */
int vlg_layout_decode_ext(const float* out_last, int ld, const int64_t* cls_in, const float* box_in,
                          int64_t* cls_out, float* box_out, float* valid_out, int64_t* gen_cls, float* gen_box,
                          int B, int T, int N, int n_classes, int steps, int step,
                          float temperature, int top_k, float box_temperature, uint64_t seed, int keep_padded, void* stream);
int vlg_layout_decode_append_ext(const float* out_last, int ld, int64_t* cls, float* box, float* valid,
                                 int64_t* gen_cls, float* gen_box, int64_t* frame_cls, float* frame_box,
                                 int B, int T, int N, int n_classes, int pos, int steps, int step,
                                 float temperature, int top_k, float box_temperature, uint64_t seed, int keep_padded,
                                 void* stream);
/* K futures per clip in one launch: the two _ext steps above - their argument lists plus `clips` and `sample0` before stream -
 * on a batch whose B clips are B / clips SAMPLES of `clips` prompts, sample-major: batch clip b is prompt b % clips, sample
 * k = sample0 + b / clips.  Token (b, n) draws with counter (r0, step, stream, k), r0 = (b % clips)*N + n, for the class draw
 * (stream 0) and the box normal (stream 5) alike, under the call's key; everything else is the rule above, the same device
 * function.  So a future is a function of (prompt token, step, sample, seed) alone: sample 0 draws what the _ext entries
 * draw, a launch of sample k alone (B = clips, sample0 = k) gives slice k of the batched launch bit for bit, and
 * clips = B, sample0 = 0 IS the _ext call.
 * Refusals as the _ext entries, plus VLG_ERR_SHAPE for clips < 1, B % clips != 0, sample0 < 0, or sample0 + B / clips not
 * fitting 31 bits. */
int vlg_layout_decode_samples(const float* out_last, int ld, const int64_t* cls_in, const float* box_in,
                              int64_t* cls_out, float* box_out, float* valid_out, int64_t* gen_cls, float* gen_box,
                              int B, int T, int N, int n_classes, int steps, int step,
                              float temperature, int top_k, float box_temperature, uint64_t seed, int keep_padded,
                              int clips, int sample0, void* stream);
int vlg_layout_decode_append_samples(const float* out_last, int ld, int64_t* cls, float* box, float* valid,
                                     int64_t* gen_cls, float* gen_box, int64_t* frame_cls, float* frame_box,
                                     int B, int T, int N, int n_classes, int pos, int steps, int step,
                                     float temperature, int top_k, float box_temperature, uint64_t seed, int keep_padded,
                                     int clips, int sample0, void* stream);

/* ------------------------------------------------------------------ scheduled sampling (csrc/decode.hip)
 * SELF-ORACLE (tests/sched_ref.py restates it); DESIGN.md, "Scheduled sampling".  Builds the inputs of a training step's
 * second pass from the true inputs and the first pass's outputs: every input token is either the truth or the model's own
 * decoded prediction of it.
 *   out       [B*N*T, ld] fp32: logits | raw box of an evaluation forward on the true inputs, INTERNAL row order
 *             m = (b*N + n)*T + t; row m predicts frame t + 1.  Rows with t = T-1 feed nothing and are NOT read.
 *   cls, box  the true inputs, (B,T,N) int64 / (B,T,N,4) fp32, public order, only read
 *   mix_cls, mix_box  the mixed inputs, same shapes; every element is written, each by exactly one thread (plain stores)
 *   step      int32 in DEVICE memory: the step counter k, read when the kernel runs (a captured graph advances it by
 *             replaying vlg_dropout_step_advance on it)
 * Input token i = (b*T + t)*N + n keeps the truth when t == 0 or cls[i] >= n_classes (a padded slot: id and box stay).
 * Every other token is replaced iff (x >> 8) < thr(k), x = first word of Philox4x32-10 on counter (i, k, 1, 0) under key
 * (seed & 0xffffffff, seed >> 32);  thr(k) = thr_max when ramp_steps == 0, else
 * (uint64)thr_max * min(k + 1, ramp_steps) / ramp_steps (integer division).  thr_max = round(eps_max * 2^24)
 * (vlg_sched_plan is the one place this rule lives): 0 never replaces, 2^24 always does.
 * A replaced token takes, from row (b*N + n)*T + (t-1) of out: class = vlg_layout_decode's rule for a slot that is not
 * padded (one device function serves all three entries), its u drawn from counter (i, k, 0, 0); box = sigmoid(raw).
 *
 * vlg_sched_plan (host only; thr_host is a HOST pointer): VLG_ERR_SHAPE unless 0 <= eps_max <= 1 (NaN refused).
 * vlg_layout_mix_inputs refuses before anything is enqueued.  VLG_ERR_SHAPE: B, T or N < 1, B*T*N >= 2^31 (the token is
 * a 32-bit counter word), n_classes < 1 or n_classes + 4 > 32, ld < n_classes + 4, thr_max > 2^24, ramp_steps < 0,
 * temperature < 0 or not finite, top_k < 0 or > n_classes, a NULL pointer, or mix_cls / mix_box overlapping each other
 * or any of out, cls, box, step.  VLG_ERR_ALIGN: out, box, mix_box not 16-byte, cls, mix_cls not 8-byte, step not 4-byte
 * aligned.  Algorithmic bytes: 4 * (n_classes + 4) * B*N*(T-1) read of out, 2 * 24 * B*T*N of tokens. */
int vlg_sched_plan(double eps_max, uint32_t* thr_host);
int vlg_layout_mix_inputs(const float* out, int ld, const int64_t* cls, const float* box,
                          int64_t* mix_cls, float* mix_box, const int* step,
                          int B, int T, int N, int n_classes, uint32_t thr_max, int ramp_steps,
                          float temperature, int top_k, uint64_t seed, void* stream);

/* ------------------------------------------------------------------ augmentation (csrc/augment.hip)
 * SELF-ORACLE (tests/augment_ref.py restates it); DESIGN.md, "Augmentation".  Builds the batch a training step runs on
 * from the caller's batch: per clip a horizontal flip, a zoom about the image centre and a shift, per input token a
 * jitter, per track (one slot of one clip, all its frames) a drop.  One launch.
 *   cls, box        the inputs slot_class (B,T,N) int64 / slot_box (B,T,N,4) fp32 (cx, cy, w, h), public order, only read
 *   tgt_box, valid  the targets' boxes (B,T,N,4) fp32 and valid (B,T,N) fp32, only read.  tgt_class has no part in it:
 *                   the step keeps reading the caller's
 *   aug_cls, aug_box, aug_tgt_box, aug_valid   the augmented batch, same shapes; every element is written, each by exactly
 *                   one thread (plain vector stores)
 *   step            int32 in DEVICE memory: the step counter k, read when the kernel runs (a captured graph advances it by
 *                   replaying vlg_dropout_step_advance on it)
 * Token i = (b*T + t)*N + n, track r = b*N + n.  W(c0,c1,c2,c3) = the four words of Philox4x32-10 on that counter under key
 * (seed & 0xffffffff, seed >> 32);  v(x) = (float)(x >> 8) * 2^-23 - 1, in [-1, 1) and exact in fp32;
 * coin(x, thr) = (x >> 8) < thr with thr = round(p * 2^24) (vlg_augment_plan is the one place this rounding lives): 0 never
 * wins, 2^24 always does.  Counter word c2 names the stream: 2, 3, 4 here (enum vlg_rng_stream above, the one table).
 *   clip draw   (x0..x3) = W(b, k, 2, 0):  flip = coin(x0, thr_flip), s = 1 + zoom * v(x1), tx = shift * v(x2), ty = shift * v(x3)
 *   track draw  drop = coin(first word of W(r, k, 3, 0), thr_drop)
 *   token draw  (inputs only, only when jitter > 0)  (y0..y3) = W(i, k, 4, 0):  jx = jitter * v(y0), jy = jitter * v(y1),
 *               jw = 1 + jitter * v(y2), jh = 1 + jitter * v(y3)
 * The box map on (cx, cy, w, h).  EVERY operation is rounded to fp32 and nothing is fused: the device code of this function
 * is compiled with floating-point contraction off.  max(a, c) below means a > c ? a : c and min(a, c) means a < c ? a : c
 * (c the constant), so a NaN coordinate becomes the constant.
 *   1. flip: cx = 1 - cx
 *   2. the geometric stage, only if zoom > 0 || shift > 0 || jitter > 0 (ONE decision for the whole launch):
 *        cx = ((cx - 0.5) * s + 0.5) + tx;  cy = ((cy - 0.5) * s + 0.5) + ty;  w = w * s;  h = h * s
 *        an input box with jitter > 0:  cx = cx + jx;  cy = cy + jy;  w = w * jw;  h = h * jh
 *        crop to the image, x axis:  x0 = max(cx - 0.5 * w, 0);  x1 = min(cx + 0.5 * w, 1);  w = max(x1 - x0, 2^-10);
 *        cx = min(max(0.5 * (x0 + x1), 0), 1);  the y axis likewise with cy, h.  A box pushed wholly outside becomes a
 *        sliver on the border, never NaN or a negative size
 *   3. geometric stage off: a box that is not flipped is copied bit for bit, also where the data's own boxes stick out
 * Per token:
 *   input, dropped track   class n_classes and a zero box in all T frames (whatever the tokens held), aug_valid = 0 in all T
 *   input, padded token    (cls[i] >= n_classes, track kept) class and box copied untouched - the convention of rollout
 *                          and scheduled sampling
 *   input, otherwise       class copied, box = the map with jitter
 *   target                 aug_tgt_box[i] = the map WITHOUT jitter when valid[i] > 0, else a bit copy
 *   aug_valid[i]           drop ? 0 : valid[i].  valid[b,t,n] is both the key mask of input token (t,n) in the per-clip
 *                          attention kinds and the loss mask of the target of (t,n): only whole tracks are ever invalidated
 *
 * vlg_augment_plan (host only; thr_host is a HOST pointer): VLG_ERR_SHAPE unless 0 <= p <= 1 (NaN refused).
 * vlg_layout_augment refuses before anything is enqueued.  VLG_ERR_SHAPE: B, T or N < 1, B*T*N >= 2^31 (the token is a
 * 32-bit counter word), n_classes < 1, thr_flip or thr_drop > 2^24, zoom or shift outside [0, 0.5] or jitter outside
 * [0, 0.25] (NaN and inf refused), a NULL pointer, or one of the four outputs overlapping any other buffer.  VLG_ERR_ALIGN:
 * a box pointer not 16-byte, a class pointer not 8-byte, valid, aug_valid or step not 4-byte aligned.
 * Algorithmic bytes: 88 per token (8 + 16 + 16 + 4 read, the same written): a launch-bound pass, 2.9 MB at (32,16,64). */
int vlg_augment_plan(double p, uint32_t* thr_host);
int vlg_layout_augment(const int64_t* cls, const float* box, const float* tgt_box, const float* valid,
                       int64_t* aug_cls, float* aug_box, float* aug_tgt_box, float* aug_valid, const int* step,
                       int B, int T, int N, int n_classes, uint32_t thr_flip, uint32_t thr_drop,
                       float zoom, float shift, float jitter, uint64_t seed, void* stream);

/* ------------------------------------------------------------------ validation metrics (csrc/metrics.hip)
 * Scores head outputs against targets and ADDS the result to a running record in device memory: `counts` (int64 slots,
 * vlg_layout_metrics_counts(n_classes) of them) and `sums` (double slots, vlg_layout_metrics_sums(n_classes)).  One launch,
 * no host wait, nothing written per token; the caller zeroes a record to start one and reads it whenever it likes.
 * SELF-ORACLE (tests/metrics_ref.py); DESIGN.md, "Validation metrics".
 *   out       [rows, ld] fp32: logits | raw box, INTERNAL row order m = (b*N + n)*T + t.  T = 1 makes it the [B*N, n_out]
 *             buffer vlg_head_last_frame writes, so one kernel serves training-shaped outputs and rollout steps
 *   targets   tgt_class (B,tgt_T,N) int64, tgt_box (B,tgt_T,N,4) fp32, valid (B,tgt_T,N) fp32 or NULL, public order;
 *             frame t of `out` is scored against frame t0 + t: src = (b*tgt_T + t0 + t)*N + n (no slice is ever copied)
 * Per token:
 *   scored      (valid == NULL or valid[src] != 0) and 0 <= tgt_class[src] < n_classes.  Anything else: UNSCORED += 1 and
 *               the token's outputs are not examined (a padded slot may hold NaN there)
 *   non-finite  a scored token with inf or NaN among its n_classes + 4 outputs: NONFINITE += 1 and nothing else
 *   otherwise   SCORED += 1, and with l = logits, tgt = tgt_class[src]:
 *               pred = the first maximum of l (vlg_layout_decode at temperature 0);  TOP1 += (pred == tgt);
 *               CONF[tgt*n_classes + pred] += 1;
 *               rank = #{c: l[c] > l[tgt]} + #{c < tgt: l[c] == l[tgt]} (decode's tie order);  TOPK += (rank < top_k);
 *               p = sigmoid(raw);  iou = IoU of the (cx,cy,w,h) boxes p and tgt_box in fp32, formula and iou_eps of
 *               vlg_layout_loss;  IOU_HIT += (iou >= iou_thr);  BOTH_HIT += (pred == tgt and iou >= iou_thr);
 *               sums, each value computed in fp32 and accumulated in double:
 *               NLL += logf(sum_c expf(l[c] - max)) + max - l[tgt];  IOU += iou;  BOX_L1 += mean_k |p[k] - tgt_box[k]|;
 *               IOU_BY_CLASS[tgt] += iou
 * Per launch SCORED + NONFINITE + UNSCORED grows by exactly B*T*N.  Counts are integer atomics: exact in any schedule.
 * Sums use no floating-point atomics: per-block partials in `scratch`, added in block order by the last block (an integer
 * ticket in scratch, which that block resets), so the same call on the same record gives the same bits.
 * scratch: >= vlg_layout_metrics_scratch() 8-byte slots, 16-byte aligned, ZERO-INITIALISED ONCE by the caller; launches
 * that share it must be ordered on one stream.
 * Refusals, all before anything is enqueued.  VLG_ERR_SHAPE: n_classes < 1 or n_classes + 4 > 32; top_k outside
 * [1, n_classes]; iou_thr not finite; B, T or N < 1; t0 < 0 or t0 + T > tgt_T; ld < n_classes + 4 or ld % 4 != 0;
 * B*T*N > 2^38.  VLG_ERR_ALIGN: out, tgt_box, scratch (16 bytes), sums, tgt_class, counts (8 bytes) NULL or misaligned;
 * valid non-NULL and not 4-byte aligned. */
#define VLG_MET_SCORED     0   /* counts: tokens that reached the statistics                          */
#define VLG_MET_TOP1       1
#define VLG_MET_TOPK       2
#define VLG_MET_IOU_HIT    3
#define VLG_MET_BOTH_HIT   4
#define VLG_MET_NONFINITE  5
#define VLG_MET_UNSCORED   6
#define VLG_MET_CONF       8   /* counts[VLG_MET_CONF + tgt*n_classes + pred]                          */
#define VLG_MET_NLL        0   /* sums                                                                 */
#define VLG_MET_IOU        1
#define VLG_MET_BOX_L1     2
#define VLG_MET_IOU_BY_CLASS 4 /* sums[VLG_MET_IOU_BY_CLASS + tgt]                                     */
int vlg_layout_metrics_counts(int n_classes);   /* int64 slots of a record: VLG_MET_CONF + n_classes^2 */
int vlg_layout_metrics_sums(int n_classes);     /* double slots: VLG_MET_IOU_BY_CLASS + n_classes */
int vlg_layout_metrics_scratch(void);           /* 8-byte slots of scratch */
int vlg_layout_metrics(const float* out, int ld, const int64_t* tgt_class, const float* tgt_box, const float* valid,
                       int tgt_T, int t0, int64_t* counts, double* sums, void* scratch,
                       int B, int T, int N, int n_classes, int top_k, float iou_thr, float iou_eps, void* stream);

/* ------------------------------------------------------------------ sampled futures (csrc/samples.hip)
 * Score K sampled futures of every clip against the frames that really followed, measure how much the K differ, select the
 * best one: three launches, no host wait.  SELF-ORACLE (tests/samples_ref.py restates them in fp64); DESIGN.md, "Sampled
 * futures".
 *   gen_cls (K,B,S,N) int64, gen_box (K,B,S,N,4) fp32   the samples (what K stacked rollouts return), only read
 *   clip_class (B,tgt_T,N) int64, clip_box (B,tgt_T,N,4) fp32   the truth, read in place as vlg_layout_metrics reads it:
 *             generated frame s is scored against frame t0 + s
 * A token is SCORED when 0 <= clip_class < n_classes.  Per scored token, every operation one fp32 rounding (the file is
 * compiled with floating-point contraction off):
 *   iou   IoU of the (cx,cy,w,h) boxes gen_box and clip_box, formula and iou_eps of vlg_layout_loss, min / max = fminf /
 *         fmaxf (a NaN coordinate is ignored by them, a NaN size makes the IoU NaN); 0 when the generated class is >= n_classes
 *   disp  sqrtf(dx*dx + dy*dy), (dx, dy) the difference of the two centres
 *   hit   generated class == truth class
 * Sums are doubles added in a fixed order - no floating-point atomics, no scratch, the same bits on every call.
 *
 * vlg_layout_sample_scores: scores (K,B,VLG_SMP_COLS) fp32, per sample and clip.  IOU, ADE, ACC: the mean of iou, disp, hit
 * over the clip's scored tokens; FDE: the mean of disp over the scored tokens of frame S-1; N_SCORED, N_SCORED_LAST: the two
 * token counts, as floats (S*N <= 2^24, else VLG_ERR_SHAPE); two columns of zero.  A mean over no token is 0.
 * vlg_layout_sample_diversity: div (B,2) fp32, per clip, over all sample pairs j < k and the clip's scored tokens:
 * [0] the mean of 1 - IoU(gen_box_j, gen_box_k) (the formula above, whatever the classes), [1] the share of terms with
 * gen_cls_j != gen_cls_k.  Both 0 for K = 1 or a clip with no scored token.
 * vlg_layout_sample_select: criterion = VLG_SMP_IOU | ADE | FDE | ACC names a score column; IOU and ACC are maximised, ADE
 * and FDE minimised.  best[b] (int32) = the first sample whose score is not NaN and strictly better than every earlier
 * one's; 0 if all K are NaN - so of equal samples the lowest index wins.  best_cls (B,S,N) / best_box (B,S,N,4) = that sample
 * of every clip, bit for bit.  It ADDS to `record` (VLG_SMP_REC_SLOTS doubles; the caller zeroes it to start one), summed
 * over the COUNTED clips, those with N_SCORED > 0:  REC_BEST + c: column c's own optimum over the K samples, chosen by the
 * rule above;  REC_MEAN + c: its mean over all K (a NaN score makes it NaN);  REC_SELECTED + c: its value at best[b]
 * (c = IOU, ADE, FDE, ACC);  REC_DIV_BOX, REC_DIV_CLASS: the clip's div;  REC_CLIPS: 1.  The three FDE terms are added only
 * for a clip with N_SCORED_LAST > 0, counted in REC_CLIPS_FDE.
 * Cost: all three are launch-bound at every shape the project uses (DESIGN.md gives the bytes): one block per (sample, clip),
 * one per clip, one block in all.
 * Refusals, before anything is enqueued.  VLG_ERR_SHAPE: K, B, S or N < 1; S*N > 2^24; K*B >= 2^31; t0 < 0 or t0 + S > tgt_T;
 * n_classes outside [1, 28]; a criterion that is none of the four; an output overlapping an input or another output.
 * VLG_ERR_ALIGN: a NULL pointer; a box pointer or scores not 16-byte, a class pointer, div or record not 8-byte, best not
 * 4-byte aligned. */
#define VLG_SMP_COLS          8   /* floats per (sample, clip) row of scores                              */
#define VLG_SMP_IOU           0
#define VLG_SMP_ADE           1
#define VLG_SMP_FDE           2
#define VLG_SMP_ACC           3
#define VLG_SMP_N_SCORED      4
#define VLG_SMP_N_SCORED_LAST 5
#define VLG_SMP_REC_BEST      0   /* record[VLG_SMP_REC_BEST + column], column = IOU, ADE, FDE, ACC        */
#define VLG_SMP_REC_MEAN      4
#define VLG_SMP_REC_SELECTED  8
#define VLG_SMP_REC_DIV_BOX   12
#define VLG_SMP_REC_DIV_CLASS 13
#define VLG_SMP_REC_CLIPS     14
#define VLG_SMP_REC_CLIPS_FDE 15
#define VLG_SMP_REC_SLOTS     16
int vlg_layout_sample_record_slots(void);       /* double slots of a record: VLG_SMP_REC_SLOTS */
int vlg_layout_sample_scores(const int64_t* gen_cls, const float* gen_box, const int64_t* clip_class, const float* clip_box,
                             float* scores, int K, int B, int S, int N, int tgt_T, int t0, int n_classes, float iou_eps,
                             void* stream);
int vlg_layout_sample_diversity(const int64_t* gen_cls, const float* gen_box, const int64_t* clip_class, float* div,
                                int K, int B, int S, int N, int tgt_T, int t0, int n_classes, float iou_eps, void* stream);
int vlg_layout_sample_select(const float* scores, const float* div, const int64_t* gen_cls, const float* gen_box,
                             int* best, int64_t* best_cls, float* best_box, double* record,
                             int K, int B, int S, int N, int criterion, void* stream);

/* ------------------------------------------------------------------ rasterised layouts (csrc/raster.hip)
 * Draws layouts - the slots of a frame as (class, cx, cy, w, h) - into label maps, and counts a confusion matrix of two
 * label maps.  SELF-ORACLE (tests/raster_ref.py restates the definition in fp32 numpy; every quantity below is ONE
 * correctly rounded fp32 operation, so the device matches it exactly); DESIGN.md, "Rasterised layouts".
 *
 * vlg_layout_rasterize
 *   inputs    cls (B,T_buf,N) int64, box (B,T_buf,N,4) fp32 cxcywh, valid (B,T_buf,N) fp32 or NULL, public order.  Frames
 *             t0 .. t0+T-1 of every clip are drawn into labels (B,T,H,W); the clip is read in place, as vlg_layout_metrics
 *             reads its targets
 *   drawn     a slot is drawn iff (valid == NULL or valid != 0) and 0 <= cls < n_classes and all four box values are
 *             finite and w > 0 and h > 0
 *   edges     in pixel units, one rounded fp32 operation per step:  hw = 0.5f*w;  X0 = (cx - hw) * (float)W;
 *             X1 = (cx + hw) * (float)W;  Y0, Y1 likewise from cy, h, H.  (Contracting cx - 0.5f*w into an fma changes
 *             nothing: 0.5f*w is exact.  No other step has the fma shape.)
 *   coverage  pixel (y,x) is covered iff X0 <= x + 0.5f < X1 and Y0 <= y + 0.5f < Y1: centres decide, left/top edges are
 *             inclusive, right/bottom exclusive.  Nothing is clamped: a box that hangs over the border is clipped by the
 *             image, a box thinner than a pixel may cover no centre
 *   winner    of a pixel: the covering drawn slot with the smallest (area, n), area = w*h one rounded multiplication; the
 *             lower slot index wins equal areas; small objects lie on top
 *   label     what = VLG_RASTER_CLASS: the winner's class; VLG_RASTER_SLOT: its slot index n; no winner: `background`
 *   out_kind  VLG_LABEL_U8 (1 B per pixel, what vlg_label_confusion reads), VLG_LABEL_I64 (the dtype of a cross-entropy
 *             target), VLG_LABEL_F32 (the dtype of the pixel model's segmentation input)
 * Worked example (H = 8, W = 16, background 20): slot 0 = class 3, box (.5,.5,.5,.5); slot 1 = class 5, box
 * (.5,.5,.25,.25); slot 2 = class 7, box (.25,.5,.25,.25).  Rows 2 and 5 are 20 x4, 3 x8, 20 x4; rows 3 and 4 are
 * 20 20 7 7 7 7 5 5 5 5 3 3 20 20 20 20; every other row is background.
 * Refusals, all before anything is enqueued.  VLG_ERR_SHAPE: B, T, N or H < 1; t0 < 0 or t0 + T > T_buf; N > 1024;
 * n_classes < 1 or > 255; W < 16 or W % 16 != 0; H or W > 16384; background outside [0, 255]; an unknown out_kind or what;
 * what = SLOT with U8 and N > 255; a NULL cls, box or labels; labels overlapping an input.  VLG_ERR_ALIGN: box or labels
 * not 16-byte aligned, cls not 8-byte aligned, valid not 4-byte aligned.
 * Writes: every element of labels exactly once, by one thread, with plain vector stores; nothing else.  No atomics, no
 * scratch, no block waits for another.
 *
 * vlg_label_confusion
 *   pred, truth  (B,T,hw) uint8 label maps.  counts: per_frame ? T : 1 rows of n_labels*n_labels + 1 int64, ADDED TO
 *   pixel (b,t,i) goes to row t (row 0 without per_frame) and adds 1 to [truth*n_labels + pred] - the orientation of
 *   VLG_MET_CONF - or, if either label is >= n_labels, to the row's last slot (IGNORED).  Per launch the rows grow by
 *   exactly B*T*hw in total.  Per-block LDS histogram; non-zero bins leave as 64-bit integer atomics, as vlg_layout_metrics'
 *   counts do: exact whatever the schedule, no scratch.
 * VLG_ERR_SHAPE: n_labels outside [1, 32]; hw < 16 or hw % 16 != 0; B*T*hw >= 2^31; B or T < 1; a NULL pointer; per_frame
 * with T > 65535 (the frame is a grid dimension).
 * VLG_ERR_ALIGN: the maps not 16-byte aligned or counts not 8-byte aligned.  A refused call enqueues nothing. */
#define VLG_LABEL_U8     0
#define VLG_LABEL_I64    1
#define VLG_LABEL_F32    2
#define VLG_RASTER_CLASS 0
#define VLG_RASTER_SLOT  1
int vlg_layout_rasterize(const int64_t* cls, const float* box, const float* valid, void* labels,
                         int B, int T_buf, int t0, int T, int N, int n_classes, int H, int W,
                         int out_kind, int what, int background, void* stream);
int vlg_label_confusion(const uint8_t* pred, const uint8_t* truth, int64_t* counts,
                        int B, int T, int64_t hw, int n_labels, int per_frame, void* stream);

/* ------------------------------------------------------------------ reductions */
int vlg_reduce_slabs(const float* slabs, int64_t slab_stride, int n_slabs,
                     float* dst, int64_t len, void* stream);

/* Adam whose step counter lives on the device, for a step captured in a hipGraph (a replayed launch cannot take new
 * by-value arguments): state = {float step_size, float sqrt_bc2, int step, int pad}, 16-byte aligned; the call advances
 * the counter (advance != 0), recomputes the two bias-correction factors in double as vlg_adam_step does on the host,
 * then updates.  shadow may be NULL. */
int vlg_adam_step_graph(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, vlg_bf16* shadow,
                        int64_t n, float* state, int advance, float lr, float beta1, float beta2, float eps,
                        float grad_scale, void* stream);

/* Many reductions in one launch, driven by a DEVICE table (static graphs: the reference GridNet's 61 convolutions).
 * vlg_reduce_slabs_table: row i = {slabs pointer, slab stride, slab count, destination pointer, length} (int64 each);
 * every row is reduced exactly as vlg_reduce_slabs would.  The table lives in device memory, so the host checks
 * vlg_reduce_slabs makes cannot be made on its rows: the CALLER guarantees, per row, length >= 4 and slab stride multiples of 4,
 * slab stride >= length, slab count >= 1, and 16-byte-aligned slabs and destination pointers (a length that is not a
 * multiple of 4 loses its tail silently).  The same holds for the rider_table of vlg_linear_dgrad_wgrad.
 * vlg_sum_partials_table: row i = {partials pointer, count, destination pointer}: dst[0] = sum (vlg_sum_partials with accumulate = 0). */
int vlg_reduce_slabs_table(const int64_t* table, int n_rows, int blocks_per_row, void* stream);
int vlg_sum_partials_table(const int64_t* table, int n_rows, void* stream);

/* ------------------------------------------------------------------- optimiser
 * torch.optim.Adam(lr, betas=(beta1, 0.999)) on one flat fp32 buffer
 * (reference src/trainer.py:83,258; src/main.py:139-141).  `step` is 1-based.
 * grad_scale multiplies the gradient first (1/world_size turns an all-reduce SUM
 * into DDP's mean, reference src/trainer.py:113). */
int vlg_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                  int64_t n, int step, float lr, float beta1, float beta2, float eps,
                  float grad_scale, void* stream);
/* same, and shadow[i] = bf16(param[i]) after the update: the weight operand of the bf16-MFMA projections */
int vlg_adam_step_bf16(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, vlg_bf16* shadow,
                       int64_t n, int step, float lr, float beta1, float beta2, float eps,
                       float grad_scale, void* stream);

/* The guarded step: global-norm gradient clipping, a step that is skipped when the gradient holds inf or NaN, and a
 * learning rate that lives in device memory - all decided on the device by three stream-ordered launches, so the step
 * needs no host synchronisation and a captured graph replays it unchanged:
 *     vlg_grad_sumsq -> vlg_optim_control -> vlg_adam_step_ctl
 * They share `ctl`, a 16-float, 16-byte-aligned device record (ints are stored in the same 4-byte slots): */
#define VLG_CTL_STEP_SIZE  0   /* float  lr / (1 - beta1^step) of the step about to be applied          */
#define VLG_CTL_SQRT_BC2   1   /* float  sqrt(1 - beta2^step)                                            */
#define VLG_CTL_STEP       2   /* int    steps applied so far (slots 0-2 = the state of vlg_adam_step_graph) */
#define VLG_CTL_APPLY      3   /* int    1: this step updates; 0: the gradient was not finite, nothing is touched */
#define VLG_CTL_GRAD_MULT  4   /* float  what Adam multiplies the gradient by: grad_scale * clip coefficient */
#define VLG_CTL_GRAD_NORM  5   /* float  grad_scale * ||grad||_2 (the norm of the mean gradient under data parallelism) */
#define VLG_CTL_LR         6   /* float  learning rate: an INPUT, written by the host, only read by the kernels */
#define VLG_CTL_SKIPPED    7   /* int    running count of skipped steps                                  */
#define VLG_CTL_CLIP_COEF  8   /* float  min(1, max_norm / (norm + 1e-6)); 1 without clipping           */
#define VLG_CTL_FLOATS     16  /* slots 9-15 are reserved and stay as the host left them                 */
/* partials[b] = sum of grad[i]^2 over the elements block b visits, b < vlg_grad_sumsq_blocks(n) (a pure host planner,
 * 1 <= blocks <= 2048, non-decreasing in n); later elements of `partials` are not written.  fp64 accumulation, fixed
 * summation order (bitwise reproducible), no atomics; an inf or NaN element gives an inf or NaN partial.
 * n >= 4, n % 4 == 0 (VLG_ERR_SHAPE); 16-byte-aligned pointers (VLG_ERR_ALIGN). */
int vlg_grad_sumsq_blocks(int64_t n);
int vlg_grad_sumsq(const float* grad, int64_t n, float* partials, void* stream);
/* One block: norm = grad_scale * sqrt(sum of the partials, in double, fixed order) -> VLG_CTL_GRAD_NORM.  Finite norm:
 * APPLY = 1, STEP += 1, the two bias-correction factors from STEP and VLG_CTL_LR in double (as vlg_adam_step computes
 * them on the host), GRAD_MULT = grad_scale * min(1, max_norm / (norm + 1e-6)) - torch.nn.utils.clip_grad_norm_'s rule;
 * max_norm <= 0 = no clipping, GRAD_MULT = grad_scale exactly.  Otherwise APPLY = 0, SKIPPED += 1 and STEP, the factors,
 * GRAD_MULT and CLIP_COEF keep their values.  1 <= n_partials <= 2048. */
int vlg_optim_control(float* ctl, const float* partials, int n_partials, float grad_scale, float max_norm,
                      float beta1, float beta2, void* stream);
/* vlg_adam_step / vlg_adam_step_bf16 (shadow may be NULL) with step_size, sqrt_bc2 and the gradient multiplier read
 * from ctl: bitwise their result when GRAD_MULT == grad_scale.  With APPLY == 0 no element of param, the moments or
 * the shadow is read or written.  May be called on slices of the buffers, like the other Adam entry points. */
int vlg_adam_step_ctl(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, vlg_bf16* shadow,
                      int64_t n, const float* ctl, float beta1, float beta2, float eps, void* stream);

/* The training recipe on the guarded step: decoupled weight decay (torch.optim.AdamW) on marked float4s, a linear
 * learning-rate warm-up counted in APPLIED steps, and an exponential moving average (EMA) of the weights - decided and
 * applied on the device, so a captured graph replays them:
 *     vlg_grad_sumsq -> vlg_optim_control_ext -> vlg_adamw_ema_step_ctl
 * They share `ctl` (above, same contract) and `ext`, a second 16-float, 16-byte-aligned device record: */
#define VLG_EXT_WEIGHT_DECAY 0   /* float  INPUT  the decay wd (0 = none)                                              */
#define VLG_EXT_WARMUP_STEPS 1   /* int    INPUT  warm-up length W in applied steps; 0 = off                           */
#define VLG_EXT_EMA_DECAY    2   /* float  INPUT  the EMA decay d                                                      */
#define VLG_EXT_EMA_WARMUP   3   /* int    INPUT  0 or 1: d_t = min(d, (1 + step) / (10 + step))                       */
#define VLG_EXT_LR_EFF       4   /* float  OUTPUT effective learning rate of this step                                 */
#define VLG_EXT_DECAY_MULT   5   /* float  OUTPUT 1 - LR_EFF * wd: what a marked parameter is multiplied by            */
#define VLG_EXT_EMA_OMD      6   /* float  OUTPUT 1 - d_t: the weight of the new parameters in the average             */
#define VLG_EXT_FLOATS       16  /* inputs are written by the host and only read by the kernels; slots 7-15 are reserved
                                    and stay as the host left them */
/* vlg_optim_control, from the same code (same ctl slots, same bits whenever WARMUP_STEPS == 0), plus the outputs of ext.
 * `step` = the 1-based count of the step being applied (STEP after its increment; skipped steps do not advance it).  In
 * double, each output rounded to float once:
 *     lr_eff = LR                                   WARMUP_STEPS == 0 (bit for bit)
 *            = LR * min(1, step / WARMUP_STEPS)     otherwise
 *     STEP_SIZE = lr_eff / (1 - beta1^step)         DECAY_MULT = 1 - lr_eff * wd
 *     d_t = EMA_DECAY, or min(EMA_DECAY, (1 + step) / (10 + step)) with EMA_WARMUP;   EMA_OMD = 1 - d_t
 * On a skipped step (non-finite norm) no output slot of ext changes.  ext non-NULL and 16-byte aligned. */
int vlg_optim_control_ext(float* ctl, float* ext, const float* partials, int n_partials, float grad_scale, float max_norm,
                          float beta1, float beta2, void* stream);
/* vlg_adam_step_ctl plus two optional parts per float4 (group of 4 consecutive parameters; tensors start at multiples of 4
 * floats, so a float4 never straddles two):
 *   decay_mask  uint8[n/4] or NULL, one byte per float4.  Non-zero: p = p * DECAY_MULT (one rounded multiplication) BEFORE
 *               Adam's update - torch.optim.AdamW's order.  Zero, or NULL: no multiplication is issued, the float4 is
 *               bitwise vlg_adam_step_ctl's.
 *   ema         fp32[n] or NULL.  After the update e = e + EMA_OMD * (p_new - e).  ema_shadow: bf16[n] or NULL, only with
 *               ema (else VLG_ERR_SHAPE): bf16(e), round to nearest even, stored as `shadow` is.
 * With decay_mask, ema NULL, wd = 0 and WARMUP_STEPS = 0 the pair is bitwise vlg_optim_control + vlg_adam_step_ctl.  With
 * APPLY == 0 no element of any buffer is read or written, the average included.
 * Algorithmic bytes on top of vlg_adam_step_ctl's 16 B read + 12 B written (+ 2 B shadow) per parameter: 4 + 4 (+ 2) B with
 * ema, 0.25 B with the mask.  n >= 4, n % 4 == 0, ctl and ext non-NULL (VLG_ERR_SHAPE); param, grad, the moments, ema, ctl,
 * ext 16-byte aligned, the shadows 8, decay_mask 4 (VLG_ERR_ALIGN).  A refused call enqueues nothing. */
int vlg_adamw_ema_step_ctl(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, vlg_bf16* shadow,
                           float* ema, vlg_bf16* ema_shadow, const uint8_t* decay_mask, int64_t n, const float* ctl,
                           const float* ext, float beta1, float beta2, float eps, void* stream);

/* ---------------------------------------------------- reference-real image ops
 * Pixel-space ops of the reference step that exist verbatim in the reference.
 *   vlg_ce_nchw        nn.CrossEntropyLoss('mean') on (b,C,H,W) logits / (b,H,W) int64
 *                      targets; writes loss[0] and dlogits = grad_scale * dCE
 *                                                     reference src/trainer.py:124,250
 *   vlg_l1_mean        nn.L1Loss()                    reference src/trainer.py:130,248
 *   vlg_gradient_loss  GradientLoss.forward           reference src/loss.py:20-25
 *   vlg_ssim_loss      SsimLoss.SSIM/forward          reference src/loss.py:68-91
 *   vlg_prep_input     normalise + concat + flip      reference src/trainer.py:193-206
 * Each loss writes value to loss[0] and, when grad != NULL, d(loss)/d(first arg) *
 * grad_scale.  scratch >= vlg_image_loss_scratch() floats. */
int vlg_image_loss_scratch(void);
int vlg_ce_nchw(const float* logits, const int64_t* target, float* dlogits, float* loss,
                float* scratch, int b, int C, int64_t hw, float grad_scale, void* stream);
int vlg_l1_mean(const float* a, const float* b, float* da, float* loss, float* scratch,
                int64_t n, float grad_scale, void* stream);
int vlg_gradient_loss(const float* a, const float* b, float* da, float* loss, float* scratch,
                      int planes, int H, int W, float grad_scale, void* stream);
int vlg_ssim_loss(const float* x, const float* y, float* dx, float* loss, float* scratch,
                  int b, int C, int H, int W, float grad_scale, void* stream);
/* dst = (src - shift[c]) * scale[c] on (b,C,H,W), C <= 4; shift/scale are HOST arrays of C floats.
 * img = (img - mean_arr) / std_arr, reference src/trainer.py:120-121,212 (and its transpose in backward). */
int vlg_affine_nchw(const float* src, float* dst, int b, int C, int64_t hw, const float* shift_host,
                    const float* scale_host, void* stream);
int vlg_prep_input(const float* e1, const float* seg1, const float* frame1,
                   const float* frame2, const float* seg2, const float* e2,
                   const float* frame3, const int64_t* seg3,
                   float* x10, float* frame3_out, int64_t* seg3_out,
                   int b, int H, int W, int flip, void* stream);

/* Autoregressive rollout, reference src/trainer.py:453-476 (8 steps from two frames + two segmentation maps).
 *   vlg_argmax_nchw    out[b,1,hw] = float(argmax over C of logits[b,C,hw]), first maximum wins     trainer.py:467
 *   vlg_rollout_input  x10 = cat[e_a, seg_a, img_a, img_b, seg_b, e_b] (frames already normalised): trainer.py:461 with
 *                      the two edge channels the 10-channel net was trained with (trainer.py:197) */
int vlg_argmax_nchw(const float* logits, float* out, int b, int C, int64_t hw, void* stream);
int vlg_rollout_input(const float* e_a, const float* seg_a, const float* img_a, const float* img_b,
                      const float* seg_b, const float* e_b, float* x10, int b, int64_t hw, void* stream);

/* ------------------------------------------------- GridNet convolution path (reference-real)
 * The reference's trainable model (CoordGridNet / GridNet, reference src/models/gridnet.py:7-114) is built
 * from three blocks (reference src/models/modules.py:5-58): PReLU -> conv3x3 -> PReLU -> conv3x3, the first
 * conv stride 2 in down blocks, a bilinear x2 (align_corners=True) in front of up blocks.  These entry
 * points replace nn.Conv2d(k=3, padding=1[, stride=2]) + nn.PReLU() + nn.Upsample at modules.py:12-17,
 * 34-39, 49-55 and AddCoords at modules.py:65-96, forward and backward.
 *
 * Tensors are "padded NHWC": rows p = (n*(H+2) + y')*(W+2) + x' of Cp floats (Cp = channels rounded up to
 * 32, extras zero), zero one-pixel halo, zero guard rows before/after (csrc/conv.hip header).  Weights are
 * [cout_p][9][cin_p] (tap = ky*3+kx), bias [cout_p].  rowmask[p] = 1 on interior pixels, 0 on the halo.
 * rowtab (stride 2 forward / weight gradient): output row -> input row of the window centre.
 * tap_tables (stride 2 data gradient): [9][tab_stride] input row -> output row through that tap, or a
 * guard row.  prelu_slope: device pointer to the single shared slope (NULL = no activation); the
 * activation is applied to channels < act_ch only, so appended AddCoords channels stay linear. */
#define VLG_CEPI_BIAS   1   /* (fwd always adds bias when bias != NULL)                          */
#define VLG_CEPI_RESID  2   /* out += resid[row, col]   (sum with the other grid branch)         */
#define VLG_CEPI_PRELU  4   /* out = prelu(out)         (activation applied by the producer)     */
#define VLG_CEPI_DPRELU 8   /* dgrad: din = acc * prelu'(x_in); slope-gradient partials -> da    */
#define VLG_CEPI_ACCUM  16  /* C += result              (tensor consumed by several blocks)      */
#define VLG_CEPI_CIN4   32  /* fwd: only input channels 0..3 carry data (the image layers of the frozen trunks, 3 channels in a
                               32-channel padded tensor): contract over (tap, 4 channels) - same result, 1/6 of the products.
                               Stride 1, no activation on load, no residual / PReLU epilogue (else VLG_ERR_SHAPE). */
int vlg_conv3x3_fwd(const float* in, const float* w, const float* bias, float* out, const float* resid,
                    const float* rowmask, const float* prelu_slope, const int* rowtab, int64_t rows_out,
                    int cin_p, int cout, int cout_p, int wp_in, int act_ch, int epilogue,
                    float* workspace /* NULL, or >= vlg_conv3x3_fwd_workspace() floats: enables split-K (all tiles at the coarse
                                        levels; elsewhere the tiles beyond the last full round of 256, see csrc/conv.hip) */,
                    int64_t workspace_capacity /* floats available at workspace (checked; too small for the tail plan = no tail
                                                  split, too small for the coarse-level split = VLG_ERR_SHAPE) */, void* stream);
/* K ranges the forward uses for EVERY tile when given a workspace (1 = no such split): coarse levels of the 256-512 channel trunks */
int vlg_conv3x3_fwd_splits(int64_t rows_out, int cin_p, int cout, int cout_p);
/* floats of workspace the forward can use for this shape (0 = none): splits * rows_out * cout_p, or the tail plan's partial tiles */
int64_t vlg_conv3x3_fwd_workspace(int64_t rows_out, int cin_p, int cout, int cout_p);
int vlg_conv3x3_dgrad_slabs(int64_t rows_in, int cin_p);   /* length of the slope-gradient partial vector */
int vlg_conv3x3_dgrad(const float* dout, const float* w, float* din, const float* x_in,
                      const float* rowmask_in, const float* prelu_slope, float* da_slab,
                      const int* tap_tables, int64_t tab_stride, int64_t rows_in, int cin_p, int cout_p,
                      int wp, int act_ch, int epilogue,
                      float* workspace /* NULL, or >= vlg_conv3x3_dgrad_workspace() floats (split-K as in the forward; used only
                                          when da_slab and tap_tables are NULL, i.e. by the frozen trunks) */,
                      int64_t workspace_capacity /* floats available at workspace (checked) */,
                      int da_capacity /* floats available at da_slab, >= vlg_conv3x3_dgrad_slabs() (checked) */, void* stream);
int vlg_conv3x3_dgrad_splits(int64_t rows_in, int cin_p, int cout_p);
int64_t vlg_conv3x3_dgrad_workspace(int64_t rows_in, int cin_p, int cout_p);
int vlg_conv3x3_wgrad_slabs(int64_t rows, int cin_p, int cout_p);
int vlg_conv3x3_wgrad(const float* dout, const float* in, float* slabs, int64_t slab_stride, int64_t slab_capacity,
                      const int* rowtab, const float* prelu_slope, int64_t rows, int cin_p, int cout_p,
                      int wp_in, int act_ch, void* stream);
/* bf16-MFMA twins of the three convolutions (csrc/conv_bf16.hip; VLG_PRECISION=bf16 of the pixel step).  Same arguments,
 * layouts, validation and return codes as the fp32 entry points; every tensor stays fp32, only the two GEMM operands are
 * rounded to bf16 (RNE, after the activation on load) and multiplied on v_mfma_f32_32x32x16_bf16 with fp32 accumulation.
 * Their tile plan is their own: size workspaces, slope partials and slabs from the _bf16 queries.  VLG_CEPI_CIN4 is
 * accepted and served by the general path over the 32 padded channels. */
int vlg_conv3x3_fwd_bf16(const float* in, const float* w, const float* bias, float* out, const float* resid,
                         const float* rowmask, const float* prelu_slope, const int* rowtab, int64_t rows_out,
                         int cin_p, int cout, int cout_p, int wp_in, int act_ch, int epilogue, float* workspace,
                         int64_t workspace_capacity, void* stream);
int vlg_conv3x3_fwd_bf16_splits(int64_t rows_out, int cin_p, int cout, int cout_p);
int64_t vlg_conv3x3_fwd_bf16_workspace(int64_t rows_out, int cin_p, int cout, int cout_p);
int vlg_conv3x3_dgrad_bf16_slabs(int64_t rows_in, int cin_p);
int vlg_conv3x3_dgrad_bf16(const float* dout, const float* w, float* din, const float* x_in,
                           const float* rowmask_in, const float* prelu_slope, float* da_slab,
                           const int* tap_tables, int64_t tab_stride, int64_t rows_in, int cin_p, int cout_p,
                           int wp, int act_ch, int epilogue, float* workspace, int64_t workspace_capacity,
                           int da_capacity, void* stream);
int vlg_conv3x3_dgrad_bf16_splits(int64_t rows_in, int cin_p, int cout_p);
int64_t vlg_conv3x3_dgrad_bf16_workspace(int64_t rows_in, int cin_p, int cout_p);
int vlg_conv3x3_wgrad_bf16_slabs(int64_t rows, int cin_p, int cout_p);
int vlg_conv3x3_wgrad_bf16(const float* dout, const float* in, float* slabs, int64_t slab_stride, int64_t slab_capacity,
                           const int* rowtab, const float* prelu_slope, int64_t rows, int cin_p, int cout_p,
                           int wp_in, int act_ch, void* stream);
/* (b,C,H,W) <-> padded NHWC; to_padded can append AddCoords' two channels (modules.py:65-96) at c0, c0+1 */
int vlg_nchw_to_padded(const float* src, float* dst, int b, int C, int H, int W, int cp, int coord_c0, void* stream);
int vlg_padded_to_nchw(const float* src, float* dst, int b, int C, int H, int W, int cp, void* stream);
int vlg_fill_coords(float* dst, int b, int H, int W, int cp, int coord_c0, void* stream);
/* nn.Upsample(scale_factor=2, mode='bilinear', align_corners=True), modules.py:50, on padded NHWC */
int vlg_upsample2x_fwd(const float* in, float* out, int b, int h, int w, int cp, void* stream);
int vlg_upsample2x_bwd(const float* dout, float* din, int b, int h, int w, int cp, int accumulate, void* stream);
/* Frozen HED edge detector, forward only (reference src/models/hned.py:9-105; used at trainer.py:190-192,216).
 * 3x3 convs reuse vlg_conv3x3_fwd with prelu_slope pointing at 0.0 (ReLU, applied by the consumer on load). */
int vlg_maxpool2x2(const float* in, float* out, int b, int h, int w, int cp, void* stream);            /* hned.py:20,28,38,48 */
int vlg_score1x1_relu(const float* in, const float* w, const float* bias, float* out, int b, int H, int W,
                      int C, int cp, void* stream);                                                    /* hned.py:60-64,90-94 */
int vlg_hed_head(const float* s0, const float* s1, const float* s2, const float* s3, const float* s4,
                 const float* combine_w, const float* combine_b, float* out /* (6,b,H,W) */, int b, int H, int W,
                 void* stream);                                                                        /* hned.py:96-105 */
/* VggLoss (reference src/loss.py:29-49): frozen VGG19 features[:27] on both images, L1 mean of the relu4_4 features.
 * The trunk reuses vlg_conv3x3_fwd / _dgrad (ReLU = slope 0) and vlg_maxpool2x2; these two close the loop. */
int vlg_maxpool2x2_bwd(const float* in, const float* dout, float* din, int b, int h, int w, int cp, void* stream);
int vlg_l1_relu_padded(const float* a, const float* b, float* da, float* loss, float* scratch /* >= 4096 */,
                       int64_t rows, int cp, int64_t count, float grad_scale, void* stream);
/* dst = src (+ dst): gradient hand-over along the residual sums of gridnet.py:51-56 */
int vlg_add_rows(float* dst, const float* src, int64_t n, int accumulate, void* stream);
/* sums a vector of per-block partials into dst[0] (PReLU slope gradients); accumulate != 0 adds to dst */
int vlg_sum_partials(const float* partials, int n, float* dst, int accumulate, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VLG_HIP_H */
