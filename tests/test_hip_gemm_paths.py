"""Every kernel path the projection-GEMM dispatcher (csrc/gemm.hip) can pick, against fp64.

The dispatcher chooses tile size, contraction depth (BK), chained N tiles, the fast or guarded main loop per block, the
paired launch and its rider blocks from the call's shape alone, so a path is reached by choosing a shape.  CASES names
the path each shape is meant to reach; `mirror_plan` below restates the planner (gemm_plan) in Python, function by
function, and test_mirror_names_the_path / test_mirror_matches_the_library_plan keep the table and the mirror honest on
the host: the second compares every field the library's own plan query reports with the mirror's.  The GPU tests then run each case with every output inside a larger buffer filled with a sentinel
bit pattern (leading dimension >= N + 4, spare rows below the last one, slab padding and spare slab capacity), compare
the results with an fp64 CPU reference computed from the same fp32 (or bf16-representable) inputs, and assert that no
padding bit changed and that every output element was written (the sentinel is a NaN, which conftest.assert_close
would let through: check_close refuses any non-finite value first).  Bars: 1e-4 for fp32 and fp32x3 outputs,
test_hip_ops.BF_OUT (one bf16 rounding) for bf16 outputs; native fp32 products must also stay within 4x of torch-CPU
fp32's own error against fp64.
"""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from helpers import check_close
from test_hip_ops import BF_OUT
from vlg import hip

EPI_NONE, EPI_BIAS, EPI_GELU, EPI_RESID, EPI_DGELU, EPI_BF16 = 0, 1, 2, 4, 8, 16
EPI_A_BF16, EPI_B_BF16, EPI_OUT_BF16, EPI_SPLIT3 = 32, 64, 128, 256
EPI_ACT_GELU, EPI_GELU_GRAD, EPI_MUL = 512, 1024, 2048
ERR_SHAPE = 1001

BF = torch.bfloat16
SENT32, SENT16 = 0x7FA5A5A5, 0x7FA5           # NaN payloads no kernel computes
SPARE_ROWS = 136                              # more than one 128-row tile below the last output row


def _cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ dispatch mirror
# An independent restatement of gemm_plan (csrc/gemm.hip) and its helpers, named by the function each piece mirrors.
# mirror_plan returns exactly the fields vlg_linear_plan reports; describe() turns such fields - the mirror's or the
# library's - into the path label the case table uses.
F32, BF16_MFMA, F32X3 = 0, 1, 2                          # VLG_GEMM_*
CALLS = {"fwd": hip.CALL_FWD, "dgrad": hip.CALL_DGRAD, "wgrad": hip.CALL_WGRAD, "pair": hip.CALL_PAIR}    # VLG_CALL_*
STORAGE = EPI_A_BF16 | EPI_B_BF16 | EPI_OUT_BF16


def wants_small(M, N):
    """gemm_wants_small - 64x64 tiles while the 128x128 grid has fewer than 512 blocks."""
    return _cdiv(M, 128) * _cdiv(N, 128) < 512


def gemm_run(M, N, Kc, lda, ldb, ldc, b_kc, slots=512):
    """gemm_run (BM = BN = 128, BK = 32, A contraction-contiguous): N tiles chained per block when every block takes
    the fast path."""
    if M % 128 or N % 128 or Kc % 64:
        return 1
    span_a = 127 * lda + Kc
    span_b = 255 * ldb + Kc if b_kc else Kc * ldb + 256
    if span_a >= 1 << 28 or span_b >= 1 << 28 or 127 * ldc + 128 >= 1 << 28:
        return 1
    tm, tn = M // 128, N // 128
    best = 1
    for r in range(2, tn + 1):
        if tn % r == 0 and tm * (tn // r) >= slots:
            best = r
    return best


def wgrad_plan(M, N, K, flags):
    """wgrad_split -> (splits, rows per split, small)."""
    native = (flags & (EPI_BF16 | EPI_SPLIT3 | EPI_ACT_GELU)) == 0
    bm = 32 if N <= 32 else 128
    tiles = _cdiv(N, bm) * _cdiv(K, 128)
    want = 512 // tiles
    max_splits = _cdiv(M, 256)
    small = False
    eff = max(want, 1) if want < max_splits else max_splits
    if native and bm == 128 and tiles * eff < 385:
        small = True
        tiles = _cdiv(N, 64) * _cdiv(K, 64)
        want = 1024 // tiles
        max_splits = _cdiv(M, 128)
    want = max(min(want, max_splits), 1)
    if small:
        c, w0 = want, want
        while c >= 1 and 4 * c >= 3 * w0:
            if M % (c * 64) == 0:
                want = c
                break
            c -= 1
    p = _cdiv(_cdiv(M, want), 64) * 64
    return _cdiv(M, p), p, small


def body_kinds(BM, BN, BK, fast_kernel, M, N, Kc, lda, ldb, ldc, a_kc, b_kc, splits=1, per=None, run=1):
    """gemm_f32_body: tile and K range of a block, `interior`, `fits`, fast or guarded main loop.
    Returns the set of main loops the blocks take: fast / guarded (fast-path kernels), general / guarded (the others),
    plus "unfit" when some block misses the fast path only for its 32-bit byte offsets."""
    per = Kc if per is None else per
    m_in = {tm * BM + BM <= M for tm in range(_cdiv(M, BM))}
    n_in = {tn * BN + run * BN <= N for tn in range(0, _cdiv(N, BN), run)}
    k_in = set()
    for s in range(splits):
        ext = min(s * per + per, Kc) - s * per
        span_a = (BM - 1) * lda + ext if a_kc else ext * lda + BM
        span_b = (2 * BN - 1) * ldb + ext if b_kc else ext * ldb + 2 * BN
        fits = span_a < 1 << 28 and span_b < 1 << 28 and (BM - 1) * ldc + BN < 1 << 28
        k_in.add((ext % BK == 0, fits))
    kinds = set()
    for mi in m_in:
        for ni in n_in:
            for ki, fits in k_in:
                interior = mi and ni and ki
                if fast_kernel:
                    kinds.add("fast" if interior and fits else "guarded")
                    if interior and not fits:
                        kinds.add("unfit")
                else:
                    kinds.add("general" if interior else "guarded")
    return "+".join(k for k in ("fast", "general", "guarded", "unfit") if k in kinds)


def _family(flags):
    return BF16_MFMA if flags & EPI_BF16 else F32X3 if flags & EPI_SPLIT3 else F32


def _terms(call, M, N, K, ldc):
    """The product in the kernel's terms (fwd_args, dgrad_args, wgrad_args): C[gM, gN] over gK, leading dimension of C."""
    return {"fwd": (M, N, K, ldc), "dgrad": (M, K, N, ldc), "wgrad": (N, K, M, K)}[call]


def mirror_problem(call, M, N, K, flags, lda, ldb, ldc):
    """gemm_problem -> (bm, bn, bk, run, splits, blocks, rows per split) of one single call."""
    fwd, wgrad = call == "fwd", call == "wgrad"
    native = _family(flags) == F32
    act = call != "dgrad" and bool(flags & EPI_ACT_GELU)         # GELU on load: no small tiles, no chaining, no fast path
    epi = 0 if wgrad else flags & (EPI_BIAS | EPI_GELU | EPI_RESID | EPI_DGELU | EPI_GELU_GRAD | EPI_MUL)
    gM, gN, gK, gldc = _terms(call, M, N, K, ldc)
    bm = bn = 128
    bk = {F32: 32, BF16_MFMA: 64, F32X3: 16}[_family(flags)]
    run, splits, per = 1, 1, gK
    if wgrad:
        splits, per, small = wgrad_plan(M, N, K, flags)
        bm, bn = (64, 64) if small else (32 if N <= 32 else 128, 128)
    elif fwd and N <= 32 and (not native or (epi == EPI_BIAS and not act)):
        bn = 32
    elif native and not act and wants_small(gM, gN):
        bm = bn = 64
    if native and bm == 128 and bn == 128:
        run32 = 1 if wgrad or act else gemm_run(gM, gN, gK, lda, ldb, gldc, fwd)
        if epi & (EPI_GELU | EPI_DGELU) and run32 == 1:          # heavy epilogue: three blocks per CU, unless the tiles chain
            bk = 16
        else:
            run = run32
    return (bm, bn, bk, run, splits, _cdiv(gM, bm) * (_cdiv(gN, bn) // run) * splits, per)


def mirror_plan(call, M, N, K, flags, lda, ldb, ldc, ldxx=0):
    """gemm_plan -> (family, launches, problems, fused, problem[, problem]) as vlg_linear_plan reports them."""
    if call != "pair":
        return (_family(flags), 1, 1, 0, mirror_problem(call, M, N, K, flags, lda, ldb, ldc))
    st = flags & STORAGE
    epi = flags & ~(EPI_BF16 | STORAGE)
    wflags = flags & (EPI_BF16 | EPI_SPLIT3 | EPI_A_BF16 | EPI_B_BF16)
    small = wgrad_plan(M, N, K, wflags)[2]
    mul = epi == EPI_MUL
    bf16_pair = bool(flags & EPI_BF16) and (st & ~EPI_A_BF16) == (EPI_B_BF16 | EPI_OUT_BF16)
    native = not (flags & EPI_BF16) and st == 0
    small_d = wants_small(M, K)
    fused = (epi == EPI_NONE or mul) and N > 32 and K > 32 and \
        ((not (mul and st & EPI_A_BF16)) if bf16_pair else (native and small == small_d))
    d = mirror_problem("dgrad", M, N, K, flags, lda, ldb, ldc)
    w = mirror_problem("wgrad", M, N, K, wflags, lda, ldxx, K)
    return (_family(flags), 1 if fused else 2, 2, int(fused), d, w)


def _describe_problem(call, family, prob, M, N, K, flags, lda, ldb, ldc):
    bm, bn, bk, run, splits, _, per = prob
    sp = " splits%d" % splits if splits > 1 else ""
    if family != F32:
        return "%s %dx%d%s" % ("gemm_bf16_kernel" if family == BF16_MFMA else "gemm_split_kernel", bm, bn, sp)
    gM, gN, gK, gldc = _terms(call, M, N, K, ldc)
    fast = bm == bn and bm in (64, 128) and not (call != "dgrad" and flags & EPI_ACT_GELU)
    kinds = body_kinds(bm, bn, bk, fast, gM, gN, gK, lda, ldb, gldc, call != "wgrad", call == "fwd", splits, per, run)
    return "gemm_f32_kernel %dx%d BK%d%s%s %s" % (bm, bn, bk, " run%d" % run if run > 1 else "", sp, kinds)


def describe(fields, call, M, N, K, flags, lda, ldb, ldc, ldxx=0):
    """The path label of a plan (the mirror's or the library's fields): kernel, tile, depth, chaining, splits, and the
    main loops its blocks take."""
    family, launches, problems, fused = fields[:4]
    if call != "pair":
        return _describe_problem(call, family, fields[4], M, N, K, flags, lda, ldb, ldc)
    wflags = flags & (EPI_BF16 | EPI_SPLIT3 | EPI_A_BF16 | EPI_B_BF16)
    d, w = fields[4], fields[5]
    if not fused:
        return "two calls | w %s | d %s" % (_describe_problem("wgrad", family, w, M, N, K, wflags, lda, ldxx, K),
                                            _describe_problem("dgrad", family, d, M, N, K, flags, lda, ldb, ldc))
    if family == BF16_MFMA:
        return "gemm16_pair_kernel splits%d" % w[4]
    bt = d[0]
    assert (d[0], d[1], d[2], w[0], w[1], w[2], w[3]) == (bt, bt, 32, bt, bt, 32, 1)
    dk = body_kinds(bt, bt, 32, True, M, K, N, lda, ldb, ldc, True, False, run=d[3])
    wk = body_kinds(bt, bt, 32, True, N, K, M, lda, ldxx, K, False, False, w[4], w[6])
    return "gemm_pair_kernel %d | d%s %s | w splits%d %s" % (bt, " run%d" % d[3] if d[3] > 1 else "", dk, w[4], wk)


def _ld(n):
    return _cdiv(n + 4, 8) * 8                 # >= n + 4 and a multiple of 8 (bf16 outputs need it)


def launch_lds(call, N, K):
    """Leading dimensions the GPU tests launch a case with, in vlg_linear_plan's order (lda, ldb, ldc, ldxx)."""
    return {"fwd": (K, K, _ld(N), 0), "dgrad": (N, K, _ld(K), 0), "wgrad": (N, K, 0, 0), "pair": (N, K, _ld(K), K)}[call]


def plan(call, M, N, K, flags):
    """The mirror's name of the path a case reaches, with the leading dimensions the GPU tests use."""
    lds = launch_lds(call, N, K)
    return describe(mirror_plan(call, M, N, K, flags, *lds), call, M, N, K, flags, *lds)


class _Problem(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("bm", "bn", "bk", "run", "splits", "blocks")] + [("rows_per_split", ctypes.c_int64)]


class _Plan(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("family", "launches", "problems", "fused")] + [("p", _Problem * 2)]


def library_plan(lib, call, M, N, K, flags, lda, ldb, ldc, ldxx=0):
    """vlg_linear_plan -> (return code, fields in mirror_plan's layout)."""
    out = _Plan()
    rc = lib.vlg_linear_plan(CALLS[call], M, N, K, flags, lda, ldb, ldc, ldxx, ctypes.byref(out))
    probs = tuple((p.bm, p.bn, p.bk, p.run, p.splits, p.blocks, p.rows_per_split) for p in out.p[:out.problems])
    return rc, (out.family, out.launches, out.problems, out.fused) + probs


def library_path(lib, call, M, N, K, flags):
    """The path the LIBRARY's plan names for the leading dimensions the GPU tests launch with."""
    lds = launch_lds(call, N, K)
    rc, fields = library_plan(lib, call, M, N, K, flags, *lds)
    assert rc == 0, (call, M, N, K, flags, rc)
    return describe(fields, call, M, N, K, flags, *lds)


# ------------------------------------------------------------------------------------------------ the case table
B16 = EPI_BF16 | EPI_B_BF16                    # bf16 MFMA with the bf16 weight shadow / bf16 X
CASES = [
    # id, call, M, N, K, flags, path the mirror must name
    ("fwd bias 128 BK32 interior+edge", "fwd", 33000, 520, 256, EPI_BIAS, "gemm_f32_kernel 128x128 BK32 fast+guarded"),
    ("fwd bias+resid 128 BK32 interior+edge", "fwd", 33000, 520, 256, EPI_BIAS | EPI_RESID,
     "gemm_f32_kernel 128x128 BK32 fast+guarded"),
    ("fwd gelu 128 BK16 interior+edge", "fwd", 33000, 520, 256, EPI_BIAS | EPI_GELU, "gemm_f32_kernel 128x128 BK16 fast+guarded"),
    ("fwd gelu+grad 128 BK16 interior+edge", "fwd", 33000, 520, 256, EPI_BIAS | EPI_GELU | EPI_GELU_GRAD,
     "gemm_f32_kernel 128x128 BK16 fast+guarded"),
    ("fwd bias 128 BK32 guarded-K", "fwd", 33000, 520, 196, EPI_BIAS, "gemm_f32_kernel 128x128 BK32 guarded"),
    ("fwd gelu+grad 128 BK16 guarded-K", "fwd", 33000, 520, 196, EPI_BIAS | EPI_GELU | EPI_GELU_GRAD,
     "gemm_f32_kernel 128x128 BK16 guarded"),
    ("fwd resid 128 chained", "fwd", 16384, 1536, 192, EPI_BIAS | EPI_RESID, "gemm_f32_kernel 128x128 BK32 run3 fast"),
    ("fwd gelu 128 chained", "fwd", 16384, 1536, 192, EPI_BIAS | EPI_GELU, "gemm_f32_kernel 128x128 BK32 run3 fast"),
    ("fwd act-gelu 128 ragged", "fwd", 33000, 520, 256, EPI_BIAS | EPI_RESID | EPI_ACT_GELU,
     "gemm_f32_kernel 128x128 BK32 general+guarded"),
    ("fwd narrow 128x32 large M", "fwd", 33000, 32, 256, EPI_BIAS, "gemm_f32_kernel 128x32 BK32 general+guarded"),
    ("fwd narrow N=21", "fwd", 33000, 21, 256, EPI_BIAS, "gemm_f32_kernel 128x32 BK32 guarded"),
    ("fwd N=130", "fwd", 33000, 130, 256, EPI_BIAS, "gemm_f32_kernel 128x128 BK32 fast+guarded"),
    ("dgrad none 128 guarded-K", "dgrad", 33000, 520, 264, EPI_NONE, "gemm_f32_kernel 128x128 BK32 guarded"),
    ("dgrad none 128 interior+edge", "dgrad", 33000, 512, 264, EPI_NONE, "gemm_f32_kernel 128x128 BK32 fast+guarded"),
    ("dgrad dgelu 128 BK16 guarded-K", "dgrad", 33000, 520, 264, EPI_DGELU, "gemm_f32_kernel 128x128 BK16 guarded"),
    ("dgrad dgelu 128 BK16 interior+edge", "dgrad", 33000, 512, 264, EPI_DGELU, "gemm_f32_kernel 128x128 BK16 fast+guarded"),
    ("dgrad mul 128 guarded-K", "dgrad", 33000, 520, 264, EPI_MUL, "gemm_f32_kernel 128x128 BK32 guarded"),
    ("dgrad mul 128 interior+edge", "dgrad", 33000, 512, 264, EPI_MUL, "gemm_f32_kernel 128x128 BK32 fast+guarded"),
    ("dgrad none 128 chained", "dgrad", 16384, 192, 1536, EPI_NONE, "gemm_f32_kernel 128x128 BK32 run3 fast"),
    ("dgrad dgelu 128 chained", "dgrad", 16384, 192, 1536, EPI_DGELU, "gemm_f32_kernel 128x128 BK32 run3 fast"),
    ("wgrad 128 split ragged last range", "wgrad", 33000, 520, 264, 0, "gemm_f32_kernel 128x128 BK32 splits33 fast+guarded"),
    ("wgrad narrow 32x128 large M", "wgrad", 33000, 24, 256, 0, "gemm_f32_kernel 32x128 BK32 splits129 guarded"),
    ("wgrad act-gelu large M", "wgrad", 33000, 520, 264, EPI_ACT_GELU, "gemm_f32_kernel 128x128 BK32 splits33 general+guarded"),
    ("pair none 128 ragged", "pair", 33000, 520, 264, EPI_NONE,
     "gemm_pair_kernel 128 | d guarded | w splits33 fast+guarded"),
    ("pair mul 128 ragged", "pair", 33000, 520, 264, EPI_MUL, "gemm_pair_kernel 128 | d guarded | w splits33 fast+guarded"),
    ("pair mul 128 interior+edge", "pair", 33000, 512, 264, EPI_MUL,
     "gemm_pair_kernel 128 | d fast+guarded | w splits40 fast+guarded"),
    ("pair none 128 chained dgrad", "pair", 32768, 256, 768, EPI_NONE, "gemm_pair_kernel 128 | d run3 fast | w splits40 fast"),
    ("pair none 64 ragged", "pair", 4000, 192, 136, EPI_NONE, "gemm_pair_kernel 64 | d fast+guarded | w splits32 fast+guarded"),
    ("pair mul 64 ragged", "pair", 4000, 192, 136, EPI_MUL, "gemm_pair_kernel 64 | d fast+guarded | w splits32 fast+guarded"),
    ("pair not fusable N<=32", "pair", 5000, 24, 256, EPI_NONE,
     "two calls | w gemm_f32_kernel 32x128 BK32 splits20 guarded | d gemm_f32_kernel 64x64 BK32 guarded"),
    ("bf16 pair none fp32 dY", "pair", 33000, 520, 264, B16 | EPI_OUT_BF16, "gemm16_pair_kernel splits33"),
    ("bf16 pair none bf16 dY", "pair", 33000, 520, 264, B16 | EPI_A_BF16 | EPI_OUT_BF16, "gemm16_pair_kernel splits33"),
    ("bf16 pair mul fp32 dY", "pair", 33000, 520, 264, EPI_MUL | B16 | EPI_OUT_BF16, "gemm16_pair_kernel splits33"),
    ("bf16 dgrad mul io6", "dgrad", 33000, 520, 264, EPI_MUL | B16 | EPI_OUT_BF16, "gemm_bf16_kernel 128x128"),
    ("bf16 fwd narrow", "fwd", 33000, 24, 256, EPI_BIAS | B16 | EPI_A_BF16 | EPI_OUT_BF16, "gemm_bf16_kernel 128x32"),
    ("bf16 wgrad narrow", "wgrad", 33000, 24, 256, B16 | EPI_A_BF16, "gemm_bf16_kernel 32x128 splits129"),
    # kernel rows of gemm_bf16.hip no other case reaches with an edge tile (ragged rows and columns, K = one 64-deep tile + 8)
    ("bf16 io0 fwd bias ragged", "fwd", 200, 136, 72, EPI_BIAS | EPI_BF16, "gemm_bf16_kernel 128x128"),
    ("bf16 io0 fwd gelu ragged", "fwd", 200, 136, 72, EPI_BIAS | EPI_GELU | EPI_BF16, "gemm_bf16_kernel 128x128"),
    ("bf16 io0 fwd resid ragged", "fwd", 200, 136, 72, EPI_BIAS | EPI_RESID | EPI_BF16, "gemm_bf16_kernel 128x128"),
    ("bf16 io3 fwd bias ragged", "fwd", 200, 136, 72, EPI_BIAS | B16 | EPI_A_BF16, "gemm_bf16_kernel 128x128"),
    ("bf16 io7 fwd gelu+grad ragged", "fwd", 200, 136, 72, EPI_BIAS | EPI_GELU | EPI_GELU_GRAD | B16 | EPI_A_BF16 | EPI_OUT_BF16,
     "gemm_bf16_kernel 128x128"),
    ("bf16 io0 dgrad none ragged", "dgrad", 200, 72, 136, EPI_BF16, "gemm_bf16_kernel 128x128"),
    ("bf16 io0 dgrad dgelu ragged", "dgrad", 200, 72, 136, EPI_DGELU | EPI_BF16, "gemm_bf16_kernel 128x128"),
    ("bf16 io0 wgrad ragged", "wgrad", 200, 136, 72, EPI_BF16, "gemm_bf16_kernel 128x128"),
    ("fp32x3 fwd 128 ragged", "fwd", 33000, 520, 264, EPI_BIAS | EPI_SPLIT3, "gemm_split_kernel 128x128"),
    ("fp32x3 dgrad 128 ragged", "dgrad", 33000, 520, 264, EPI_SPLIT3, "gemm_split_kernel 128x128"),
    ("fp32x3 wgrad 128 ragged", "wgrad", 33000, 520, 264, EPI_SPLIT3, "gemm_split_kernel 128x128 splits33"),
]
FALLBACK = ("wgrad 32-bit-offset fallback", "wgrad", 65536, 4096, 4096, 0, "gemm_f32_kernel 128x128 BK32 guarded+unfit")
ALL_CASES = CASES + [FALLBACK]


@pytest.mark.parametrize("case", ALL_CASES, ids=[c[0] for c in ALL_CASES])
def test_mirror_names_the_path(case):
    """Host only: each shape reaches the path its case names, under the mirrored dispatch rules."""
    _, call, M, N, K, flags, path = case
    assert plan(call, M, N, K, flags) == path


# Sweep of test_mirror_matches_the_library_plan.  Extents are multiples of 8 (the bf16 and fp32x3 kernels' slots).  M crosses:
# 512 blocks of gemm_wants_small at N or K = 256 (32 640 / 32 768 / 32 896), the weight-gradient rule's 385 at N = K = 256
# (24 576 / 24 832), M % 128 (1 000, 4 000, 33 000), and the `tiles_m * tiles_n / r >= 512` steps of gemm_run (16 256 /
# 16 384 x 1 536, 32 768 x 768 | 1 024, 65 536).  N crosses N <= 32 and N % 128, K crosses Kc % 64.
SWEEP_M = (128, 1000, 4000, 4096, 8192, 16256, 16384, 24576, 24832, 32640, 32768, 32896, 33000, 65536)
SWEEP_N = (24, 32, 40, 200, 256, 520, 768, 1024, 1536)
SWEEP_K = (64, 136, 192, 256, 264, 768)
IO3, IO6, IO7 = EPI_A_BF16 | EPI_B_BF16, EPI_B_BF16 | EPI_OUT_BF16, STORAGE
GG = EPI_BIAS | EPI_GELU | EPI_GELU_GRAD
SWEEP_FLAGS = {        # plain and heavy epilogues; native fp32, fp32x3, bf16 with io 0 and the storage combinations the step uses
    "fwd": [EPI_BIAS, EPI_BIAS | EPI_GELU, GG, EPI_BIAS | EPI_RESID, EPI_BIAS | EPI_RESID | EPI_ACT_GELU,
            EPI_SPLIT3 | EPI_BIAS, EPI_SPLIT3 | EPI_BIAS | EPI_GELU, EPI_SPLIT3 | EPI_BIAS | EPI_RESID,
            EPI_BF16 | EPI_BIAS, EPI_BF16 | EPI_BIAS | EPI_GELU, EPI_BF16 | GG, EPI_BF16 | EPI_BIAS | EPI_RESID,
            EPI_BF16 | IO3 | EPI_BIAS, EPI_BF16 | IO7 | EPI_BIAS, EPI_BF16 | IO7 | EPI_BIAS | EPI_GELU, EPI_BF16 | IO7 | GG,
            EPI_BF16 | IO3 | EPI_BIAS | EPI_RESID],
    "dgrad": [EPI_NONE, EPI_DGELU, EPI_MUL, EPI_SPLIT3, EPI_SPLIT3 | EPI_DGELU, EPI_BF16, EPI_BF16 | EPI_DGELU,
              EPI_BF16 | EPI_MUL, EPI_BF16 | IO6, EPI_BF16 | IO6 | EPI_DGELU, EPI_BF16 | IO6 | EPI_MUL, EPI_BF16 | IO7],
    "wgrad": [0, EPI_ACT_GELU, EPI_SPLIT3, EPI_BF16, EPI_BF16 | EPI_B_BF16, EPI_BF16 | IO3],
    "pair": [EPI_NONE, EPI_MUL, EPI_DGELU, EPI_SPLIT3, EPI_BF16, EPI_BF16 | IO6, EPI_BF16 | IO7, EPI_BF16 | IO6 | EPI_MUL],
}
# leading dimensions on both sides of the 2^28-element spans of gemm_run: 127 * lda + Kc, 255 * ldb + Kc (forward) or
# Kc * ldb + 256 (data gradient), 127 * ldc + 128
LD_A = (2113648, 2113672)            # 127 * ld + 768 < 2^28 <= 127 * ld + 64
LD_C = (2113656, 2113664)            # 127 * ld + 128 < 2^28 <= ...


def _sweep_lds(call, M, N, K):
    """Leading-dimension sets of one shape: tight, padded, and - where the shape could chain - around each 2^28 span."""
    a, bb, c, xx = launch_lds(call, N, K)
    tight = {"fwd": (K, K, N, 0), "dgrad": (N, K, K, 0), "wgrad": (N, K, 0, 0), "pair": (N, K, K, K)}[call]
    out = [tight, (a + 8, bb + 8, c, xx + 8 if xx else 0)]
    if call != "wgrad" and M % 128 == 0 and M >= 16384:
        gK = K if call == "fwd" else N
        ld_b = ((1 << 28) // 255 // 8 * 8 - 8, (1 << 28) // 255 // 8 * 8 + 8) if call == "fwd" else \
            (((1 << 28) - 256) // gK // 8 * 8 - 8, ((1 << 28) - 256) // gK // 8 * 8 + 8)
        out += [(v, bb, c, xx) for v in LD_A] + [(a, v, c, xx) for v in ld_b] + [(a, bb, v, xx) for v in LD_C]
    return out


def _accepted(call, N, flags):
    """Combinations with a kernel (the table of gemm_plan): the narrow forward exists with the BIAS epilogue only outside the
    native family, GELU on load needs wide products."""
    epi = flags & ~(EPI_BF16 | EPI_SPLIT3 | STORAGE)
    if flags & EPI_ACT_GELU and N <= 32:
        return False
    return not (call == "fwd" and N <= 32 and flags & (EPI_BF16 | EPI_SPLIT3) and epi != EPI_BIAS)


def test_mirror_matches_the_library_plan():
    """Host only (no launch): every field vlg_linear_plan reports - family, launches, fused, and per problem tile, BK, run,
    splits, blocks, rows per split - is the mirror's, for every case of the tables at the leading dimensions it launches
    with and over a sweep that crosses each threshold of the planner, so neither the mirror nor a case's path can drift
    from csrc/gemm.hip silently.  The slab-count queries read the same plan."""
    from vlg import hip
    lib = hip.load()
    n = 0
    todo = [(c[1], c[2], c[3], c[4], c[5], launch_lds(c[1], c[3], c[4])) for c in ALL_CASES]
    todo += [("pair", M, N, K, fl, launch_lds("pair", N, K)) for _, M, N, K, fl, _ in RIDER_CALLS]
    for call, flag_list in SWEEP_FLAGS.items():
        for M in SWEEP_M:
            for N in SWEEP_N:
                for K in SWEEP_K:
                    for lds in _sweep_lds(call, M, N, K):
                        todo += [(call, M, N, K, fl, lds) for fl in flag_list if _accepted(call, N, fl)]
    for call, M, N, K, fl, lds in todo:
        rc, got = library_plan(lib, call, M, N, K, fl, *lds)
        assert rc == 0, (call, M, N, K, fl, lds, rc)
        assert got == mirror_plan(call, M, N, K, fl, *lds), (call, M, N, K, fl, lds)
        w = got[-1] if call in ("wgrad", "pair") else None
        if w is not None:
            wfl = fl & (EPI_BF16 | EPI_SPLIT3 | EPI_A_BF16 | EPI_B_BF16) if call == "pair" else fl
            assert lib.vlg_linear_wgrad_slabs_for(M, N, K, wfl) == w[4], (call, M, N, K, fl)
            if wfl == 0:
                assert lib.vlg_linear_wgrad_slabs(M, N, K) == w[4]
        n += 1
    assert n > SWEEP_MIN_PLANS, n
    # every threshold was crossed: both sides appear among the compared plans
    seen = {(call, lib_fields[4][:4]) for call, lib_fields in
            ((c, library_plan(lib, c, M, N, K, fl, *lds)[1]) for c, M, N, K, fl, lds in todo)}
    for want in (("fwd", (64, 64, 32, 1)), ("fwd", (128, 128, 32, 1)), ("fwd", (128, 128, 16, 1)), ("fwd", (128, 32, 32, 1)),
                 ("fwd", (128, 128, 32, 3)), ("fwd", (128, 128, 32, 4)), ("fwd", (128, 128, 32, 12)), ("dgrad", (128, 128, 16, 1)),
                 ("dgrad", (128, 128, 32, 2)), ("wgrad", (64, 64, 32, 1)), ("wgrad", (32, 128, 32, 1)), ("wgrad", (128, 128, 32, 1)),
                 ("fwd", (128, 128, 64, 1)), ("fwd", (128, 128, 16, 1)), ("pair", (64, 64, 32, 1)), ("pair", (128, 128, 32, 3))):
        assert want in seen, want


# compared plans of the sweep above (a count of the table, asserted so that a shrinking sweep is noticed)
SWEEP_MIN_PLANS = 100000


# A chained shape on both sides of each 32-bit span: run > 1 just under 2^28 elements, 1 at or above
@pytest.mark.parametrize("call,which", [("fwd", 0), ("fwd", 1), ("fwd", 2), ("dgrad", 0), ("dgrad", 1), ("dgrad", 2)])
def test_chaining_stops_at_the_32_bit_spans(call, which):
    from vlg import hip
    lib = hip.load()
    M, N, K = (16384, 1536, 192) if call == "fwd" else (16384, 192, 1536)
    lds = [lst for lst in _sweep_lds(call, M, N, K)[2:]]
    under, over = lds[2 * which], lds[2 * which + 1]
    for ld, run in ((under, 3), (over, 1)):
        rc, got = library_plan(lib, call, M, N, K, EPI_BIAS if call == "fwd" else EPI_NONE, *ld)
        assert rc == 0 and got[4][3] == run, (ld, got)
        assert got == mirror_plan(call, M, N, K, EPI_BIAS if call == "fwd" else EPI_NONE, *ld)


# ------------------------------------------------------------------------------------------------ GPU helpers
def _stream():
    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """A rows x cols output inside a sentinel-filled buffer: leading dimension ld >= cols + 4, SPARE_ROWS spare rows."""

    def __init__(self, rows, cols, dev, dtype=torch.float32, ld=None, spare=SPARE_ROWS):
        self.rows, self.cols, self.ld, self.spare = rows, cols, ld or _ld(cols), spare
        self.itype, self.sent = (torch.int32, SENT32) if dtype == torch.float32 else (torch.int16, SENT16)
        self.raw = torch.full(((rows + spare) * self.ld,), self.sent, dtype=self.itype, device=dev)
        self.t = self.raw.view(dtype)[:rows * self.ld].view(rows, self.ld)[:, :cols]

    def ptr(self):
        return self.t.data_ptr()

    def check(self, what):
        r = self.raw.view(self.rows + self.spare, self.ld)
        unwritten = int((r[:self.rows, :self.cols] == self.sent).sum())
        assert unwritten == 0, "%s: %d output elements never written" % (what, unwritten)
        assert bool((r[:self.rows, self.cols:] == self.sent).all()), "%s: write into the padding columns" % what
        assert bool((r[self.rows:] == self.sent).all()), "%s: write below the last row" % what


class GuardedSlabs:
    """Weight-gradient slabs: stride > N*K + N (padded), capacity splits x stride + spare, all sentinel."""

    def __init__(self, splits, N, K, dev, extra=4096):
        self.splits, self.L = splits, N * K + N
        self.stride = self.L + 36
        self.raw = torch.full((splits * self.stride + extra,), SENT32, dtype=torch.int32, device=dev)
        self.f = self.raw.view(torch.float32)

    def check(self, what):
        body = self.raw[:self.splits * self.stride].view(self.splits, self.stride)
        unwritten = int((body[:, :self.L] == SENT32).sum())
        assert unwritten == 0, "%s: %d slab entries (dW or bias-gradient sums) never written" % (what, unwritten)
        assert bool((body[:, self.L:] == SENT32).all()), "%s: write into the slab padding" % what
        assert bool((self.raw[self.splits * self.stride:] == SENT32).all()), "%s: write beyond splits x stride" % what


def _reduce(H, gs, dev):
    dst = torch.empty(gs.L, device=dev)
    H.call("vlg_reduce_slabs", gs.f.data_ptr(), gs.stride, gs.splits, dst.data_ptr(), gs.L, _stream())
    return dst.cpu()


def _dgelu(u):
    return 0.5 * (1 + torch.erf(u / math.sqrt(2))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi)


def _vs_cpu_fp32(got, want64, cpu32, what):
    """Native fp32: error against fp64 at most 4x torch-CPU fp32's (the test_linear_split3_is_fp32_grade rule)."""
    e_gpu = float((got.detach().cpu().double() - want64).abs().max())
    e_cpu = float((cpu32.double() - want64).abs().max())
    floor = 1e-7 * max(1.0, float(want64.abs().max()))
    assert e_gpu <= 4 * e_cpu + floor, "%s: |err| vs fp64 %.3e > 4 x torch-CPU fp32's %.3e" % (what, e_gpu, e_cpu)


def _dev_copy(t, dev, dtype):
    return t.to(dev).to(dtype) if dtype != torch.float32 else t.to(dev)


def test_checks_refuse_unwritten_outputs():
    """Host only: an output element left at the sentinel fails both the buffer check and the value comparison, a
    stray write into the padding fails the buffer check, a fully written buffer passes."""
    g = Guarded(5, 6, torch.device("cpu"))
    want = torch.randn(5, 6, dtype=torch.float64)
    g.t[:4] = want[:4].float()                                   # last row never written
    with pytest.raises(AssertionError, match="never written"):
        g.check("C")
    with pytest.raises(AssertionError, match="not finite"):
        check_close(g.t, want, what="C")
    g.t[4] = want[4].float()
    g.check("C")
    check_close(g.t, want, what="C")
    g.raw.view(5 + SPARE_ROWS, g.ld)[2, 6] = 0
    with pytest.raises(AssertionError, match="padding columns"):
        g.check("C")
    s = GuardedSlabs(2, 4, 4, torch.device("cpu"))
    s.f[:s.L] = 1.0
    s.f[s.stride:s.stride + 4 * 4] = 1.0                         # second slab's bias-gradient sums never written
    with pytest.raises(AssertionError, match="never written"):
        s.check("slabs")


@pytest.fixture(scope="module")
def H():
    from vlg import hip
    hip.load()
    return hip


# ------------------------------------------------------------------------------------------------ forward
def run_fwd(H, dev, M, N, K, flags):
    torch.manual_seed(M + N + K + flags)
    bf16 = bool(flags & EPI_BF16)
    a = torch.randn(M, K) * (1.5 if flags & EPI_ACT_GELU else 1.0)
    w, b = torch.randn(N, K) / math.sqrt(K), torch.randn(N)
    if bf16:
        a, w = a.to(BF).float(), w.to(BF).float()
    ad = _dev_copy(a, dev, BF if flags & EPI_A_BF16 else torch.float32)
    wd = _dev_copy(w, dev, BF if flags & EPI_B_BF16 else torch.float32)
    bd = b.to(dev)
    out_t = BF if flags & EPI_OUT_BF16 else torch.float32
    c = Guarded(M, N, dev, out_t)
    aux_out = Guarded(M, N, dev, out_t, ld=c.ld) if flags & EPI_GELU else None
    r = None
    if flags & EPI_RESID:
        r = torch.randn(M, c.ld)
        rd = r.to(dev)
        r = r[:, :N]
    H.call("vlg_linear_fwd", ad.data_ptr(), K, wd.data_ptr(), K, bd.data_ptr(), c.ptr(), c.ld, rd.data_ptr() if r is not None else 0,
           aux_out.ptr() if aux_out is not None else 0, M, N, K, flags, _stream())
    torch.cuda.synchronize()
    c.check("C")
    if aux_out is not None:
        aux_out.check("aux_out")
    a64 = F.gelu(a.double()) if flags & EPI_ACT_GELU else a.double()
    pre = a64 @ w.double().t() + b.double()
    tol = BF_OUT if bf16 and out_t == BF else dict(rtol=1e-4, atol=1e-5)
    native = not (flags & (EPI_BF16 | EPI_SPLIT3))
    if flags & EPI_GELU:
        if flags & EPI_GELU_GRAD:
            check_close(aux_out.t, _dgelu(pre), what="saved gelu'", **tol)
        else:
            check_close(aux_out.t, pre, what="pre-activation", **tol)
            if native:
                _vs_cpu_fp32(aux_out.t, pre, F.linear(a, w, b), "pre-activation")
        check_close(c.t, F.gelu(pre), what="gelu output", **tol)
        return
    want = pre + r.double() if r is not None else pre
    check_close(c.t.float() if bf16 else c.t, want, what="C", **tol)
    if native and not flags & EPI_ACT_GELU:
        _vs_cpu_fp32(c.t, want, F.linear(a, w, b) + r if r is not None else F.linear(a, w, b), "C")


# ------------------------------------------------------------------------------------------------ data gradient
def run_dgrad(H, dev, M, N, K, flags):
    torch.manual_seed(M + 3 * N + K + flags)
    bf16 = bool(flags & EPI_BF16)
    dy, w = torch.randn(M, N), torch.randn(N, K) / math.sqrt(N)
    if bf16:
        dy, w = dy.to(BF).float(), w.to(BF).float()
    out_t = BF if flags & EPI_OUT_BF16 else torch.float32
    c = Guarded(M, K, dev, out_t)
    aux = None
    if flags & (EPI_DGELU | EPI_MUL):
        aux = torch.randn(M, c.ld) * 1.5
        if out_t == BF:
            aux = aux.to(BF).float()
        auxd = _dev_copy(aux, dev, out_t)
        aux = aux[:, :K]
    dyd = _dev_copy(dy, dev, BF if flags & EPI_A_BF16 else torch.float32)
    wd = _dev_copy(w, dev, BF if flags & EPI_B_BF16 else torch.float32)
    H.call("vlg_linear_dgrad", dyd.data_ptr(), N, wd.data_ptr(), K, c.ptr(), c.ld, auxd.data_ptr() if aux is not None else 0,
           M, N, K, flags, _stream())
    torch.cuda.synchronize()
    c.check("dX")
    prod = dy.double() @ w.double()
    want = prod
    if flags & EPI_DGELU:
        want = prod * _dgelu(aux.double())
    elif flags & EPI_MUL:
        want = prod * aux.double()
    tol = BF_OUT if out_t == BF else dict(rtol=1e-4, atol=1e-5)
    check_close(c.t.float(), want, what="dX", **tol)
    if not flags & (EPI_BF16 | EPI_SPLIT3 | EPI_DGELU | EPI_MUL):
        _vs_cpu_fp32(c.t, want, dy @ w, "dX")


# ------------------------------------------------------------------------------------------------ weight gradient
def check_wgrad(g, dy, x, M, N, K, what, native):
    sc = math.sqrt(M)
    want = dy.double().t() @ x
    check_close(g[:N * K].view(N, K) / sc, want / sc, rtol=1e-4, atol=1e-5, what=what + " dW")
    check_close(g[N * K:] / sc, dy.double().sum(0) / sc, rtol=1e-4, atol=1e-5, what=what + " bias gradient")
    if native:
        _vs_cpu_fp32(g[:N * K].view(N, K), want, dy.t() @ x.float(), what + " dW")


def run_wgrad(H, dev, M, N, K, flags):
    lib = H.load()
    torch.manual_seed(M + 5 * N + K + flags)
    bf16 = bool(flags & EPI_BF16)
    dy, x = torch.randn(M, N), torch.randn(M, K) * (1.5 if flags & EPI_ACT_GELU else 1.0)
    if bf16:
        dy, x = dy.to(BF).float(), x.to(BF).float()
    dyd = _dev_copy(dy, dev, BF if flags & EPI_A_BF16 else torch.float32)
    xd = _dev_copy(x, dev, BF if flags & EPI_B_BF16 else torch.float32)
    ns = lib.vlg_linear_wgrad_slabs_for(M, N, K, flags)
    gs = GuardedSlabs(ns, N, K, dev)
    H.call("vlg_linear_wgrad", dyd.data_ptr(), N, xd.data_ptr(), K, gs.f.data_ptr(), gs.stride, gs.raw.numel(), M, N, K, flags,
           _stream())
    torch.cuda.synchronize()
    gs.check("slabs")
    x64 = F.gelu(x.double()) if flags & EPI_ACT_GELU else x.double()
    check_wgrad(_reduce(H, gs, dev), dy, x64, M, N, K, "wgrad", not flags & (EPI_BF16 | EPI_SPLIT3 | EPI_ACT_GELU))


# ------------------------------------------------------------------------------------------------ paired call
def pair_inputs(M, N, K, flags, dev, seed):
    torch.manual_seed(seed)
    bf16 = bool(flags & EPI_BF16)
    dy, w, x = torch.randn(M, N), torch.randn(N, K) / math.sqrt(N), torch.randn(M, K)
    aux = torch.randn(M, _ld(K)) if flags & EPI_MUL else None
    if bf16:
        dy, w, x = dy.to(BF).float(), w.to(BF).float(), x.to(BF).float()
        aux = aux.to(BF).float() if aux is not None else None
    out_t = BF if flags & EPI_OUT_BF16 else torch.float32
    d = dict(dy=_dev_copy(dy, dev, BF if flags & EPI_A_BF16 else torch.float32),
             w=_dev_copy(w, dev, BF if flags & EPI_B_BF16 else torch.float32),
             x=_dev_copy(x, dev, BF if flags & EPI_B_BF16 else torch.float32),
             aux=_dev_copy(aux, dev, out_t) if aux is not None else None)
    return (dy, w, x, aux[:, :K] if aux is not None else None), d, out_t


def call_pair(H, dev, d, M, N, K, flags, out_t, fused, rider=None, rider_rows=0):
    wflags = flags & (EPI_BF16 | EPI_SPLIT3 | EPI_A_BF16 | EPI_B_BF16)
    ns = H.load().vlg_linear_wgrad_slabs_for(M, N, K, wflags)
    gs = GuardedSlabs(ns, N, K, dev)
    dx = Guarded(M, K, dev, out_t)
    aux = H.ptr(d["aux"])
    if fused:
        H.call("vlg_linear_dgrad_wgrad", d["dy"].data_ptr(), N, d["w"].data_ptr(), K, dx.ptr(), dx.ld, aux, d["x"].data_ptr(), K,
               gs.f.data_ptr(), gs.stride, gs.raw.numel(), M, N, K, flags, H.ptr(rider), rider_rows, _stream())
    else:
        H.call("vlg_linear_wgrad", d["dy"].data_ptr(), N, d["x"].data_ptr(), K, gs.f.data_ptr(), gs.stride, gs.raw.numel(), M, N, K,
               wflags, _stream())
        H.call("vlg_linear_dgrad", d["dy"].data_ptr(), N, d["w"].data_ptr(), K, dx.ptr(), dx.ld, aux, M, N, K, flags, _stream())
    torch.cuda.synchronize()
    dx.check("paired dX")
    gs.check("paired slabs")
    return dx, gs


def run_pair(H, dev, M, N, K, flags):
    (dy, w, x, aux), d, out_t = pair_inputs(M, N, K, flags, dev, M + 7 * N + K + flags)
    dx1, gs1 = call_pair(H, dev, d, M, N, K, flags, out_t, fused=False)
    dx2, gs2 = call_pair(H, dev, d, M, N, K, flags, out_t, fused=True)
    assert torch.equal(dx1.raw, dx2.raw), "paired dX differs from the single call"
    assert torch.equal(gs1.raw, gs2.raw), "paired slabs differ from the single call"
    want = dy.double() @ w.double()
    if aux is not None:
        want = want * aux.double()
    tol = BF_OUT if out_t == BF else dict(rtol=1e-4, atol=1e-5)
    check_close(dx2.t.float(), want, what="paired dX", **tol)
    native = not flags & (EPI_BF16 | EPI_SPLIT3)
    if native and aux is None:
        _vs_cpu_fp32(dx2.t, want, dy @ w, "paired dX")
    check_wgrad(_reduce(H, gs2, dev), dy, x.double(), M, N, K, "paired", native)


RUNNERS = {"fwd": run_fwd, "dgrad": run_dgrad, "wgrad": run_wgrad, "pair": run_pair}


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_gemm_path_against_fp64(H, dev, case):
    _, call, M, N, K, flags, path = case
    assert plan(call, M, N, K, flags) == path
    assert library_path(H.load(), call, M, N, K, flags) == path
    RUNNERS[call](H, dev, M, N, K, flags)


@pytest.mark.gpu
def test_wgrad_32bit_offset_fallback(H, dev):
    """M x ld >= 2^28: the 128x128 weight-gradient kernel's byte offsets no longer fit 32 bits, so every block takes the
    guarded 64-bit main loop (one split).  About 2 GB of operands: compared with fp64 on a seeded 64 x 64 sample of the
    output (last row and last column included) and on the bias-gradient sums of the sampled columns."""
    _, _, M, N, K, flags, path = FALLBACK
    assert plan("wgrad", M, N, K, flags) == path
    lib = H.load()
    assert library_path(lib, "wgrad", M, N, K, flags) == path
    ns = lib.vlg_linear_wgrad_slabs_for(M, N, K, 0)
    assert ns == 1
    gen = torch.Generator(device=dev)
    gen.manual_seed(77)
    dyd = torch.randn(M, N, device=dev, generator=gen)
    xd = torch.randn(M, K, device=dev, generator=gen)
    gs = GuardedSlabs(ns, N, K, dev)
    H.call("vlg_linear_wgrad", dyd.data_ptr(), N, xd.data_ptr(), K, gs.f.data_ptr(), gs.stride, gs.raw.numel(), M, N, K, 0, _stream())
    torch.cuda.synchronize()
    gs.check("slabs (32-bit-offset fallback)")
    g = torch.Generator()
    g.manual_seed(78)
    rows = torch.cat([torch.randperm(N - 1, generator=g)[:63], torch.tensor([N - 1])])
    cols = torch.cat([torch.randperm(K - 1, generator=g)[:63], torch.tensor([K - 1])])
    dys = dyd[:, rows.to(dev)].cpu().double()
    xs = xd[:, cols.to(dev)].cpu().double()
    del dyd, xd
    slab = gs.f[:N * K].view(N, K)
    got = slab[rows.to(dev)][:, cols.to(dev)].cpu()
    sc = math.sqrt(M)
    check_close(got / sc, (dys.t() @ xs) / sc, rtol=1e-4, atol=1e-5, what="dW sample (fallback)")
    check_close(gs.f[N * K:N * K + N][rows.to(dev)].cpu() / sc, dys.sum(0) / sc, rtol=1e-4, atol=1e-5,
                 what="bias gradient sample (fallback)")


# ------------------------------------------------------------------------------------------------ rider reductions
# (slab count, length, stride): the "tall" branch of reduce_table_row (len4 < 32768 and n_slabs >= 16) and the flat one, slab
# counts that are not multiples of 4, 16 or 64, lengths on both sides of len4 = 32768
RIDER_ROWS = [(67, 1000, 1012), (130, 4096, 4100), (19, 131068, 131072), (17, 131076, 131076), (7, 200000, 200004),
              (5, 64, 68), (1, 8, 8), (3, 100, 104)]
RIDER_CALLS = [("fused 128 pair", 33000, 520, 264, EPI_MUL, "gemm_pair_kernel 128"),
               ("fused 64 pair", 4000, 192, 136, EPI_NONE, "gemm_pair_kernel 64"),
               ("not fusable", 5000, 24, 256, EPI_NONE, "two calls")]


def _rider_table(dev, seed=31):
    torch.manual_seed(seed)
    slabs = [torch.randn(n * stride).to(dev) for n, _, stride in RIDER_ROWS]
    gap = 36
    offs, o = [], gap
    for _, length, _ in RIDER_ROWS:
        offs.append(o)
        o += length + gap
    dst = torch.full((o,), SENT32, dtype=torch.int32, device=dev)
    df = dst.view(torch.float32)
    rows = [[s.data_ptr(), stride, n, df[off:].data_ptr(), length] for s, (n, length, stride), off in zip(slabs, RIDER_ROWS, offs)]
    table = torch.tensor(rows, dtype=torch.int64, device=dev)
    return slabs, dst, offs, table


@pytest.mark.gpu
@pytest.mark.parametrize("rc", RIDER_CALLS, ids=[r[0] for r in RIDER_CALLS])
def test_rider_reductions(H, dev, rc):
    """vlg_linear_dgrad_wgrad with a slab-reduction table: every destination is bit for bit what vlg_reduce_slabs gives for
    the same row and right against fp64, nothing outside the destinations is written, and the GEMM results are bit for bit
    those of the same call without riders."""
    _, M, N, K, flags, kind = rc
    assert plan("pair", M, N, K, flags).startswith(kind)
    assert library_path(H.load(), "pair", M, N, K, flags).startswith(kind)
    slabs, dst, offs, table = _rider_table(dev)
    (dy, w, x, aux), d, out_t = pair_inputs(M, N, K, flags, dev, 41)
    dx0, gs0 = call_pair(H, dev, d, M, N, K, flags, out_t, fused=True)
    dx1, gs1 = call_pair(H, dev, d, M, N, K, flags, out_t, fused=True, rider=table, rider_rows=len(RIDER_ROWS))
    assert torch.equal(dx0.raw, dx1.raw) and torch.equal(gs0.raw, gs1.raw), "riders changed the GEMM results"
    df = dst.view(torch.float32)
    mask = torch.ones(dst.numel(), dtype=torch.bool, device=dev)
    for s, (n, length, stride), off in zip(slabs, RIDER_ROWS, offs):
        mask[off:off + length] = False
        got = df[off:off + length]
        single = torch.empty(length, device=dev)
        H.call("vlg_reduce_slabs", s.data_ptr(), stride, n, single.data_ptr(), length, _stream())
        torch.cuda.synchronize()
        assert torch.equal(got, single), "rider row (%d slabs, length %d) differs from vlg_reduce_slabs" % (n, length)
        want = s.view(n, stride)[:, :length].cpu().double().sum(0)
        check_close(got, want, rtol=1e-5, atol=1e-5, what="rider row (%d slabs, length %d)" % (n, length))
    assert bool((dst[mask] == SENT32).all()), "a rider wrote outside its destination"
    lib = H.load()
    for bad in (0, 4097):
        assert lib.vlg_linear_dgrad_wgrad(d["dy"].data_ptr(), N, d["w"].data_ptr(), K, dx1.ptr(), dx1.ld, H.ptr(d["aux"]),
                                          d["x"].data_ptr(), K, gs1.f.data_ptr(), gs1.stride, gs1.raw.numel(), M, N, K, flags,
                                          table.data_ptr(), bad, _stream()) == ERR_SHAPE
