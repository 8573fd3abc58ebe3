"""GPU: vlg_attention_step / _bf16 - per-slot causal attention of ONE query position against the K/V cache - against
oracle.temporal_attention in fp64 on rows 0 .. p.  Every qkv row after p holds NaN (it must not be read), the output has
a leading dimension larger than d and starts as NaN sentinels (the pad columns must stay that way)."""
import pytest
import torch

from helpers import vs_cpu32
from oracle import layout_spec as O

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
NAN = float("nan")
ERR_SHAPE, ERR_ALIGN = 1001, 1002
PAD = 8                                   # extra columns of the output's leading dimension


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _qkv(T, d, n_seq, seed, bf16):
    """[n_seq*T, 3d] in the internal row order; q and k of every other sequence x5: scaled scores of |s| ~ 60-90, softmax
    rows near one-hot, so that the max subtraction matters"""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(n_seq, T, 3 * d, generator=g)
    qkv[0::2, :, :2 * d] *= 5.0
    return qkv.to(BF).float() if bf16 else qkv


def _ref(qkv, p, dt):
    """oracle attention on frames 0 .. p alone -> its row p, (n_seq, d)"""
    n_seq, T, d3 = qkv.shape
    x = qkv[:, :p + 1].to(dt).permute(1, 0, 2)[None]                  # (1, p+1, n_seq, 3d)
    return O.temporal_attention(x, d3 // 192)[0, p]


def _run(dev, qkv, p, bf16, poison=True):
    from vlg import hip
    n_seq, T, d3 = qkv.shape
    d, dt = d3 // 3, BF if bf16 else torch.float32
    q = qkv.clone()
    if poison:
        q[:, p + 1:] = NAN
    qd = q.view(n_seq * T, d3).to(dev).to(dt)
    o = torch.full((n_seq, d + PAD), NAN, device=dev, dtype=dt)
    hip.call("vlg_attention_step" + ("_bf16" if bf16 else ""), qd.data_ptr(), o.data_ptr(), n_seq, T, d, p, d + PAD, _stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(o[:, d:]).all()), "the pad columns of o were written"
    return o[:, :d].float().cpu()


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n_seq", [1, 5, 67])
@pytest.mark.parametrize("d", [64, 192])
@pytest.mark.parametrize("T", [4, 8, 16, 32])
def test_attention_step_vs_fp64(dev, T, d, n_seq, bf16):
    """Bar (helpers.vs_cpu32): 4x torch-CPU fp32's own error against fp64 plus 2^-20 of the largest value; a bf16 output one
    bf16 rounding more.  n_seq * d/64 = 1, 3, 5, 15, 67, 201 items: the last 4-wave block holds 1, 3, 1, 3, 3, 1 of them."""
    qkv = _qkv(T, d, n_seq, seed=T * 1000 + d + n_seq, bf16=bf16)
    for p in sorted({0, 1, T // 2, T - 1}):
        got = _run(dev, qkv, p, bf16)
        w64, w32 = _ref(qkv, p, torch.float64), _ref(qkv, p, torch.float32)
        print("T=%d d=%d n_seq=%d p=%d %s: |err| vs fp64 %.3e, torch-CPU fp32's %.3e, max |fp64| %.3e" % (
            T, d, n_seq, p, "bf16" if bf16 else "fp32", float((got.double() - w64).abs().max()),
            float((w32.double() - w64).abs().max()), float(w64.abs().max())))
        vs_cpu32(got, w64, w32, "attention step T=%d p=%d" % (T, p), bf16=bf16)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("T,d,n_seq", [(4, 64, 5), (8, 192, 5), (16, 64, 67), (32, 192, 5)])
def test_last_position_agrees_with_the_full_kernel(dev, T, d, n_seq, bf16):
    """p = T-1 against row T-1 of vlg_attention_fwd: both under the same bar against fp64 (they sum in different orders, so
    they need not be bit-equal)"""
    from vlg import hip
    qkv = _qkv(T, d, n_seq, seed=T + d + n_seq, bf16=bf16)
    dt = BF if bf16 else torch.float32
    qd = qkv.view(n_seq * T, 3 * d).to(dev).to(dt)
    full = torch.full((n_seq * T, d), NAN, device=dev, dtype=dt)
    hip.call("vlg_attention_fwd" + ("_bf16" if bf16 else ""), qd.data_ptr(), full.data_ptr(), n_seq, T, d, _stream())
    full = full.float().cpu().view(n_seq, T, d)[:, T - 1]
    step = _run(dev, qkv, T - 1, bf16, poison=False)
    w64, w32 = _ref(qkv, T - 1, torch.float64), _ref(qkv, T - 1, torch.float32)
    vs_cpu32(step, w64, w32, "attention step at p = T-1", bf16=bf16)
    vs_cpu32(full, w64, w32, "attention fwd, row T-1", bf16=bf16)
    # and against each other under that bar; two bf16 outputs are each one rounding (2^-8, relative) from their fp32 value
    err = (step.double() - full.double()).abs() - (2.0 ** -7 * w64.abs() if bf16 else 0.0)
    bar = 4 * float((w32.double() - w64).abs().max()) + 2.0 ** -20 * float(w64.abs().max())
    assert float(err.max()) <= bar, "step vs fwd: %.3e > %.3e" % (float(err.max()), bar)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_refusals_enqueue_nothing(dev, bf16):
    from vlg import hip
    n_seq, T, d = 5, 8, 64
    dt = BF if bf16 else torch.float32
    f = getattr(hip.load(), "vlg_attention_step" + ("_bf16" if bf16 else ""))
    qd = torch.randn(n_seq * 32, 3 * 128, device=dev).to(dt)           # room for every shape tried below
    o = torch.full((n_seq, 128 + PAD), NAN, device=dev, dtype=dt)
    q, op, s = qd.data_ptr(), o.data_ptr(), _stream()
    bad = [((q, op, n_seq, 5, d, 0, d), ERR_SHAPE), ((q, op, n_seq, 64, d, 0, d), ERR_SHAPE), ((q, op, n_seq, T, d, -1, d), ERR_SHAPE),
           ((q, op, n_seq, T, d, T, d), ERR_SHAPE), ((q, op, n_seq, T, 96, 0, 96), ERR_SHAPE), ((q, op, n_seq, T, 0, 0, 64), ERR_SHAPE),
           ((q, op, n_seq, T, d, 0, d - 1), ERR_SHAPE), ((q, op, 0, T, d, 0, d), ERR_SHAPE),
           ((0, op, n_seq, T, d, 0, d), ERR_ALIGN), ((q, 0, n_seq, T, d, 0, d), ERR_ALIGN),
           ((q + 4, op, n_seq, T, d, 0, d), ERR_ALIGN), ((q, op + 4, n_seq, T, d, 0, d + PAD), ERR_ALIGN)]
    for args, want in bad:
        assert f(*args, s) == want, args
        torch.cuda.synchronize()
        assert bool(torch.isnan(o).all()), args
    assert f(q, op, n_seq, T, d, T - 1, 128 + PAD, s) == 0               # and the same buffers are accepted as they are
    torch.cuda.synchronize()
    assert bool(torch.isfinite(o[:, :d]).all()) and bool(torch.isnan(o[:, d:]).all())
