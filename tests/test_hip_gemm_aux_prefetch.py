"""The fast GEMM path's auxiliary operand (residual, multiplier, dGELU argument) is requested inside the main loop, under the
last two iterations of a tile (csrc/gemm.hip: aux_early, iter_req), instead of at the epilogue's start.  The shapes below are
the smallest that reach each form of that loop: 64x64 and 128x128 fast tiles, one, two, three (an odd count: one iteration on
a zero tile) and eight K tiles, one tile per block and chained tiles (the next tile's requests must not pass this tile's
epilogue), guarded tiles beside fast ones.  Every result is compared with fp64 (1e-4, and helpers.vs_cpu32: at most 4x
torch-CPU fp32's own error), inside sentinel-filled buffers; the paired call must equal its two single calls bit for bit.

Shapes are in the kernel's terms, C[M, N] summed over K: a forward call is (M, N, K), a data gradient is the call
(M, N = K-of-the-shape, K = N-of-the-shape).
"""
import math

import pytest
import torch
import torch.nn.functional as F

from helpers import check_close, vs_cpu32
from test_hip_gemm_paths import (EPI_BIAS, EPI_DGELU, EPI_MUL, EPI_RESID, Guarded, _dgelu, _reduce, _stream, call_pair,
                                 check_wgrad, launch_lds, library_plan, pair_inputs)

# (M, N, K), tile, run, the paired call is one launch
SHAPES = [
    ((256, 128, 64), 64, 1, True),          # 64x64 fast tiles, two K tiles: the peeled pair alone
    ((256, 128, 32), 64, 1, False),         # one K tile: the pair's second half runs on zeros (pair: K <= 32 is not fused)
    ((8192, 1024, 64), 128, 1, False),      # 128x128 fast tiles, run = 1, two K tiles
    ((8192, 1024, 96), 128, 1, False),      # three: a steady pair, then the peeled pair with its zero tile
    ((8192, 1024, 256), 128, 1, True),      # eight
    ((16384, 1024, 128), 128, 2, True),     # chained tiles
    ((8200, 1032, 72), 128, 1, False),      # ragged in M, N and K: guarded tiles
    ((8200, 1032, 64), 128, 1, False),      # ragged in M and N only: guarded edge tiles beside fast ones
]
IDS = ["%dx%dx%d" % s[0] for s in SHAPES]


@pytest.fixture(scope="module")
def H():
    from vlg import hip
    hip.load()
    return hip


def _problem(H, call, M, N, K, flags):
    rc, fields = library_plan(H.load(), call, M, N, K, flags, *launch_lds(call, N, K))
    assert rc == 0, (call, M, N, K, flags, rc)
    return fields


def _bk(tile, run, heavy):
    """The planner's depth: 16 for a heavy epilogue on unchained 128x128 tiles, 32 elsewhere."""
    return 16 if heavy and tile == 128 and run == 1 else 32


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_plans(H, shape):
    """Host only: every shape gets the tile, depth and run it was written for, in each call the GPU tests make."""
    (M, N, K), tile, run, fused = shape
    assert _problem(H, "fwd", M, N, K, EPI_BIAS | EPI_RESID)[4][:4] == (tile, tile, 32, run)
    assert _problem(H, "dgrad", M, K, N, EPI_MUL)[4][:4] == (tile, tile, 32, run)
    assert _problem(H, "dgrad", M, K, N, EPI_DGELU)[4][:4] == (tile, tile, _bk(tile, run, True), run)
    p = _problem(H, "pair", M, K, N, EPI_MUL)
    assert p[3] == int(fused) and p[4][:4] == (tile, tile, 32, run)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_forward_bias_residual(H, dev, shape):
    (M, N, K), tile, run, _ = shape
    assert _problem(H, "fwd", M, N, K, EPI_BIAS | EPI_RESID)[4][:4] == (tile, tile, 32, run)
    torch.manual_seed(M + N + K)
    a, w, b = torch.randn(M, K), torch.randn(N, K) / math.sqrt(K), torch.randn(N)
    c = Guarded(M, N, dev)
    r = torch.randn(M, c.ld)
    ad, wd, bd, rd = a.to(dev), w.to(dev), b.to(dev), r.to(dev)
    H.call("vlg_linear_fwd", ad.data_ptr(), K, wd.data_ptr(), K, bd.data_ptr(), c.ptr(), c.ld, rd.data_ptr(), 0, M, N, K,
           EPI_BIAS | EPI_RESID, _stream())
    torch.cuda.synchronize()
    c.check("C")
    r = r[:, :N]
    want = a.double() @ w.double().t() + b.double() + r.double()
    check_close(c.t, want, what="C")
    vs_cpu32(c.t, want, F.linear(a, w, b) + r, "C")


@pytest.mark.gpu
@pytest.mark.parametrize("epi", [EPI_MUL, EPI_DGELU], ids=["mul", "dgelu"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_data_gradient(H, dev, shape, epi):
    (M, N, K), tile, run, _ = shape
    assert _problem(H, "dgrad", M, K, N, epi)[4][:4] == (tile, tile, _bk(tile, run, epi == EPI_DGELU), run)
    torch.manual_seed(M + 3 * N + K + epi)
    dy, w = torch.randn(M, K), torch.randn(K, N) / math.sqrt(K)
    c = Guarded(M, N, dev)
    aux = torch.randn(M, c.ld) * 1.5
    dyd, wd, auxd = dy.to(dev), w.to(dev), aux.to(dev)
    H.call("vlg_linear_dgrad", dyd.data_ptr(), K, wd.data_ptr(), N, c.ptr(), c.ld, auxd.data_ptr(), M, K, N, epi, _stream())
    torch.cuda.synchronize()
    c.check("dX")
    aux = aux[:, :N]
    f64 = _dgelu(aux.double()) if epi == EPI_DGELU else aux.double()
    f32 = _dgelu(aux) if epi == EPI_DGELU else aux
    want = (dy.double() @ w.double()) * f64
    check_close(c.t, want, what="dX")
    vs_cpu32(c.t, want, (dy @ w) * f32, "dX")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_pair_multiply(H, dev, shape):
    """vlg_linear_dgrad_wgrad with the multiply epilogue: bit for bit its two single calls, and right against fp64."""
    (M, N, K), tile, run, fused = shape
    p = _problem(H, "pair", M, K, N, EPI_MUL)
    assert p[3] == int(fused) and p[4][:4] == (tile, tile, 32, run)
    (dy, w, x, aux), d, out_t = pair_inputs(M, K, N, EPI_MUL, dev, M + 7 * N + K)
    dx1, gs1 = call_pair(H, dev, d, M, K, N, EPI_MUL, out_t, fused=False)
    dx2, gs2 = call_pair(H, dev, d, M, K, N, EPI_MUL, out_t, fused=True)
    assert torch.equal(dx1.raw, dx2.raw), "paired dX differs from the single call"
    assert torch.equal(gs1.raw, gs2.raw), "paired slabs differ from the single call"
    want = (dy.double() @ w.double()) * aux.double()
    check_close(dx2.t, want, what="paired dX")
    vs_cpu32(dx2.t, want, (dy @ w) * aux, "paired dX")
    check_wgrad(_reduce(H, gs2, dev), dy, x.double(), M, K, N, "paired", True)
