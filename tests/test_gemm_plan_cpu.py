"""CPU: the projection GEMMs (csrc/gemm.hip) check and plan a call completely before their first launch, so a call the plan
refuses returns its VLG_ERR_* on a machine without a GPU - where anything enqueued first would have surfaced as a HIP
error instead - and vlg_linear_plan, the host query of the same plan, returns the same code.  None of these calls is made
on a GPU: every one is refused on the host.  (Accepted calls are launches: tests/test_hip_gemm_paths.py.)"""
import ctypes

import pytest

from test_hip_gemm_paths import (CALLS, EPI_A_BF16, EPI_ACT_GELU, EPI_B_BF16, EPI_BF16, EPI_BIAS, EPI_DGELU, EPI_GELU,
                                 EPI_GELU_GRAD, EPI_MUL, EPI_NONE, EPI_OUT_BF16, EPI_RESID, EPI_SPLIT3, _Plan)

VLG_ERR_SHAPE, VLG_ERR_ALIGN = 1001, 1002
# stand-in device pointers: 16-byte aligned, never dereferenced - every call below is refused on the host
FAKE = 1 << 40
M, N, K = 4096, 256, 256
STRIDE = N * K + N


def _lib():
    from vlg import hip
    return hip.load()


def _query(lib, call, flags, lda, ldb, ldc, ldxx=0, n=N):
    return lib.vlg_linear_plan(CALLS[call], M, n, K, flags, lda, ldb, ldc, ldxx, ctypes.byref(_Plan()))


def _pair(lib, flags, rider, dx=FAKE, ldx=K, aux=FAKE, capacity=10 ** 12):
    return lib.vlg_linear_dgrad_wgrad(FAKE, N, FAKE, K, dx, ldx, aux, FAKE, K, FAKE, STRIDE, capacity, M, N, K, flags,
                                      FAKE if rider else 0, 3 if rider else 0, None)


@pytest.mark.parametrize("rider", [False, True], ids=["no riders", "rider table"])
@pytest.mark.parametrize("flags,why", [
    (EPI_BF16 | EPI_A_BF16 | EPI_B_BF16, "bf16 dY / W / X without a bf16 dX: the weight gradient has a kernel, the data gradient none"),
    (EPI_BF16 | EPI_A_BF16 | EPI_B_BF16 | EPI_OUT_BF16 | EPI_MUL, "MUL with a bf16 dY: neither fused nor as a single data gradient"),
    (EPI_SPLIT3 | EPI_MUL, "MUL is a native fp32 / bf16 epilogue"),
    (EPI_ACT_GELU, "GELU on load is no data-gradient option"),
    (EPI_DGELU | EPI_MUL, "two data-gradient epilogues at once"),
])
def test_pair_is_refused_before_anything_is_enqueued(flags, why, rider):
    lib = _lib()
    assert _pair(lib, flags, rider) == VLG_ERR_SHAPE, why
    assert _query(lib, "pair", flags, N, K, K, K) == VLG_ERR_SHAPE, why


def test_pair_refusals_keep_their_precedence():
    """Slab capacity (shape) comes before the data gradient's output alignment (align), which comes before its kernel table."""
    lib = _lib()
    io7 = EPI_BF16 | EPI_A_BF16 | EPI_B_BF16 | EPI_OUT_BF16
    assert _pair(lib, EPI_BF16, False, capacity=STRIDE) == VLG_ERR_SHAPE                       # one slab's room for 32
    # not fused (fp32 W and X): a bf16 dX on an odd leading dimension or 8-byte pointer is an alignment error ...
    assert _pair(lib, EPI_BF16 | EPI_OUT_BF16, False, ldx=K + 4) == VLG_ERR_ALIGN
    assert _pair(lib, EPI_BF16 | EPI_OUT_BF16, True, dx=FAKE + 8) == VLG_ERR_ALIGN
    assert _pair(lib, EPI_BF16 | EPI_OUT_BF16, False, ldx=K + 4, capacity=STRIDE) == VLG_ERR_SHAPE
    # ... fused (the bf16-storage pair kernel) the same defect has always been a shape error
    assert _pair(lib, io7, False, ldx=K + 4) == VLG_ERR_SHAPE
    assert _pair(lib, io7, True, dx=FAKE + 8) == VLG_ERR_SHAPE
    assert _pair(lib, EPI_NONE, False, dx=0) == VLG_ERR_ALIGN
    assert _pair(lib, EPI_MUL, False, aux=0) == VLG_ERR_SHAPE
    assert lib.vlg_linear_dgrad_wgrad(FAKE, N, FAKE, K, FAKE, K, 0, FAKE, K, FAKE, STRIDE, 10 ** 12, M, N, K, 0, FAKE, 4097,
                                      None) == VLG_ERR_SHAPE


def test_single_calls_are_refused_by_the_plan():
    lib = _lib()
    gg = EPI_BIAS | EPI_GELU | EPI_GELU_GRAD

    def fwd(flags, a=FAKE, n=N, bias=FAKE, aux_in=FAKE, aux_out=FAKE, lda=K):
        return lib.vlg_linear_fwd(a, lda, FAKE, K, bias, FAKE, n + 8, aux_in, aux_out, M, n, K, flags, None)

    for flags in (gg | EPI_RESID, gg | EPI_SPLIT3, gg | EPI_ACT_GELU, EPI_BIAS | EPI_MUL, EPI_GELU, EPI_SPLIT3 | EPI_BF16 | EPI_BIAS,
                  EPI_BIAS | EPI_A_BF16, EPI_BF16 | EPI_BIAS | EPI_ACT_GELU, EPI_BF16 | EPI_BIAS | EPI_A_BF16):
        assert fwd(flags) == VLG_ERR_SHAPE, flags
        assert _query(lib, "fwd", flags, K, K, N + 8) == VLG_ERR_SHAPE, flags
    for flags in (EPI_BF16 | EPI_BIAS | EPI_GELU, EPI_SPLIT3 | EPI_BIAS | EPI_RESID, EPI_BIAS | EPI_RESID | EPI_ACT_GELU):
        assert fwd(flags, n=24) == VLG_ERR_SHAPE, flags                                         # narrow: BIAS only
        assert _query(lib, "fwd", flags, K, K, 32, n=24) == VLG_ERR_SHAPE, flags
    assert fwd(EPI_BIAS, bias=0) == VLG_ERR_SHAPE and fwd(gg, aux_out=0) == VLG_ERR_SHAPE
    # precedence: operand alignment, then flags, then the 8-element leading dimensions of bf16 operands
    assert fwd(EPI_BIAS | EPI_MUL, a=FAKE + 4) == VLG_ERR_ALIGN
    assert fwd(EPI_BIAS | EPI_MUL, lda=K + 2) == VLG_ERR_ALIGN
    assert fwd(EPI_BF16 | EPI_A_BF16 | EPI_BIAS | EPI_MUL, lda=K + 4) == VLG_ERR_SHAPE
    assert fwd(EPI_BF16 | EPI_A_BF16 | EPI_BIAS, lda=K + 4) == VLG_ERR_ALIGN
    assert _query(lib, "fwd", EPI_BF16 | EPI_A_BF16 | EPI_BIAS, K + 4, K, N) == VLG_ERR_ALIGN

    def dgrad(flags, ldx=K, aux=FAKE):
        return lib.vlg_linear_dgrad(FAKE, N, FAKE, K, FAKE, ldx, aux, M, N, K, flags, None)

    for flags in (EPI_SPLIT3 | EPI_MUL, EPI_BIAS, EPI_ACT_GELU, EPI_BF16 | EPI_A_BF16 | EPI_B_BF16, EPI_BF16 | EPI_OUT_BF16 | EPI_DGELU,
                  EPI_BF16 | EPI_A_BF16 | EPI_B_BF16 | EPI_OUT_BF16 | EPI_MUL, EPI_OUT_BF16):
        assert dgrad(flags) == VLG_ERR_SHAPE, flags
        assert _query(lib, "dgrad", flags, N, K, K) == VLG_ERR_SHAPE, flags
    assert dgrad(EPI_DGELU, aux=0) == VLG_ERR_SHAPE
    assert dgrad(EPI_BF16 | EPI_B_BF16 | EPI_OUT_BF16, ldx=K + 4) == VLG_ERR_ALIGN
    assert _query(lib, "dgrad", EPI_BF16 | EPI_B_BF16 | EPI_OUT_BF16, N, K, K + 4) == VLG_ERR_ALIGN

    def wgrad(flags, stride=STRIDE, capacity=10 ** 12, n=N):
        return lib.vlg_linear_wgrad(FAKE, n, FAKE, K, FAKE, stride, capacity, M, n, K, flags, None)

    for flags, n in ((EPI_BF16 | EPI_ACT_GELU, N), (EPI_SPLIT3 | EPI_ACT_GELU, N), (EPI_BF16 | EPI_OUT_BF16, N), (EPI_B_BF16, N),
                     (EPI_ACT_GELU, 24), (EPI_BF16, 268), (EPI_SPLIT3, 268)):
        assert wgrad(flags, n=n, stride=n * K + n) == VLG_ERR_SHAPE, flags
        assert _query(lib, "wgrad", flags, n, K, 0, n=n) == VLG_ERR_SHAPE, flags
    assert wgrad(0, stride=STRIDE - 4) == VLG_ERR_SHAPE
    slabs = lib.vlg_linear_wgrad_slabs_for(M, N, K, 0)
    assert slabs > 1 and wgrad(0, capacity=slabs * STRIDE - 1) == VLG_ERR_SHAPE


def test_plan_query_refuses_what_is_no_call():
    lib = _lib()
    out = _Plan()
    out.family = 7
    assert lib.vlg_linear_plan(4, M, N, K, 0, K, K, N, 0, ctypes.byref(out)) == VLG_ERR_SHAPE
    assert (out.family, out.launches, out.problems, out.p[0].bm) == (0, 0, 0, 0)               # zeroed on refusal
    assert lib.vlg_linear_plan(0, 0, N, K, EPI_BIAS, K, K, N, 0, ctypes.byref(out)) == VLG_ERR_SHAPE
    assert lib.vlg_linear_plan(0, M, N, K, EPI_BIAS, K - 4, K, N, 0, ctypes.byref(out)) == VLG_ERR_SHAPE
    assert lib.vlg_linear_plan(0, M, N, K, EPI_BIAS, K, K, N, 0, ctypes.byref(out)) == 0 and out.problems == 1
