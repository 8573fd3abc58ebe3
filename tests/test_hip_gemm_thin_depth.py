"""The 32-wide tiles of the head's projections (128x32 forward, 32x128 weight gradient) in the general main loop of
csrc/gemm.hip, at the loop lengths where its prologue, steady iterations and peeled tail meet: contraction ranges of 1, 2 and
3 K tiles (prologue and tail only), 8 (steady iterations) and 6 + 4 (a ragged last range of the weight gradient's split), row
counts below one tile, ragged and many blocks.  Written with a deeper K-tile prefetch for these tiles (measured and not
kept: DESIGN.md, GEMM note); the cases are the ones any change to that loop's staging depth has to pass.  Every result
against fp64 (1e-4, and helpers.vs_cpu32: at most 4x torch-CPU fp32's own error; check_wgrad's bar for the weight
gradient) inside sentinel-filled buffers.  The data gradient with a contraction of 24 - the head's third product - runs
64x64 tiles and one K tile.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from helpers import check_close, vs_cpu32
from test_hip_gemm_paths import (EPI_BIAS, EPI_NONE, Guarded, GuardedSlabs, _reduce, _stream, check_wgrad, launch_lds,
                                 library_plan)

N_OUT = 24


@pytest.fixture(scope="module")
def H():
    from vlg import hip
    hip.load()
    return hip


def _problem(H, call, M, N, K, flags):
    rc, fields = library_plan(H.load(), call, M, N, K, flags, *launch_lds(call, N, K))
    assert rc == 0, (call, M, N, K, flags, rc)
    return fields[4]


# rows -> (splits, rows per split) of the weight gradient: 8 K tiles; 2; ranges of 6 and 4; 16 ranges of 8
WGRAD = {256: (1, 256), 64: (1, 64), 320: (2, 192), 4096: (16, 256)}


@pytest.mark.parametrize("M", sorted(WGRAD))
def test_weight_gradient_plan(H, M):
    """Host only: the 32x128 tile and the split each case was written for."""
    assert _problem(H, "wgrad", M, N_OUT, 256, 0) == (32, 128, 32, 1, WGRAD[M][0], 2 * WGRAD[M][0], WGRAD[M][1])


@pytest.mark.gpu
@pytest.mark.parametrize("K", [32, 64, 96, 256])
@pytest.mark.parametrize("M", [128, 300, 4096])
def test_forward(H, dev, M, K):
    assert _problem(H, "fwd", M, N_OUT, K, EPI_BIAS)[:4] == (128, 32, 32, 1)
    torch.manual_seed(M + K)
    a, w, b = torch.randn(M, K), torch.randn(N_OUT, K) / math.sqrt(K), torch.randn(N_OUT)
    ad, wd, bd = a.to(dev), w.to(dev), b.to(dev)
    c = Guarded(M, N_OUT, dev)
    H.call("vlg_linear_fwd", ad.data_ptr(), K, wd.data_ptr(), K, bd.data_ptr(), c.ptr(), c.ld, 0, 0, M, N_OUT, K, EPI_BIAS, _stream())
    torch.cuda.synchronize()
    c.check("C")
    want = a.double() @ w.double().t() + b.double()
    check_close(c.t, want, what="C")
    vs_cpu32(c.t, want, F.linear(a, w, b), "C")


@pytest.mark.gpu
@pytest.mark.parametrize("M", sorted(WGRAD))
def test_weight_gradient(H, dev, M):
    K = 256
    splits, per = WGRAD[M]
    assert _problem(H, "wgrad", M, N_OUT, K, 0) == (32, 128, 32, 1, splits, 2 * splits, per)
    torch.manual_seed(M + 5 * N_OUT + K)
    dy, x = torch.randn(M, N_OUT), torch.randn(M, K)
    dyd, xd = dy.to(dev), x.to(dev)
    gs = GuardedSlabs(splits, N_OUT, K, dev)
    H.call("vlg_linear_wgrad", dyd.data_ptr(), N_OUT, xd.data_ptr(), K, gs.f.data_ptr(), gs.stride, gs.raw.numel(), M, N_OUT, K, 0,
           _stream())
    torch.cuda.synchronize()
    gs.check("slabs")
    check_wgrad(_reduce(H, gs, dev), dy, x.double(), M, N_OUT, K, "wgrad", True)


@pytest.mark.gpu
@pytest.mark.parametrize("M", [300, 4096])
def test_data_gradient_contraction_24(H, dev, M):
    K = 256
    assert _problem(H, "dgrad", M, N_OUT, K, EPI_NONE)[:4] == (64, 64, 32, 1)
    torch.manual_seed(M + 3 * N_OUT + K)
    dy, w = torch.randn(M, N_OUT), torch.randn(N_OUT, K) / math.sqrt(N_OUT)
    dyd, wd = dy.to(dev), w.to(dev)
    c = Guarded(M, K, dev)
    H.call("vlg_linear_dgrad", dyd.data_ptr(), N_OUT, wd.data_ptr(), K, c.ptr(), c.ld, 0, M, N_OUT, K, EPI_NONE, _stream())
    torch.cuda.synchronize()
    c.check("dX")
    want = dy.double() @ w.double()
    check_close(c.t, want, what="dX")
    vs_cpu32(c.t, want, dy @ w, "dX")
