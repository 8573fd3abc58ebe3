"""GPU: the bf16-storage per-clip attention (vlg_attention_clip_fwd_bf16 / _bwd_bf16, csrc/attention_clip.hip) through the C ABI.

Inputs are bf16-representable; the reference is the CPU specification oracle.layout_spec.clip_attention (with autograd) in
fp64 on the same values.  The bars follow the kernels' precision contract: scores, softmax statistics and lse are fp32 (lse is
held tightly), P and dS are rounded to bf16 only as MFMA operands, O / dQ / dK / dV once on store."""
import math

import pytest
import torch

from oracle import layout_spec as O

pytestmark = pytest.mark.gpu

SHAPES = [(2, 4, 8, 64, False), (2, 4, 8, 64, True), (3, 8, 16, 128, True), (2, 16, 24, 64, True),
          (1, 16, 64, 256, False), (2, 32, 5, 64, True), (1, 4, 40, 64, False),
          (1, 32, 64, 128, True),                       # 2 048 tokens, 16 query blocks
          (1, 8, 32, 512, True)]                        # d = 512: 8 heads


@pytest.fixture(scope="module")
def H():
    from vlg import hip
    hip.load()
    return hip


def stream():
    return torch.cuda.current_stream().cuda_stream


def to_rows(t):
    """(B,T,N,C) -> the internal row order (b, n, t)"""
    B, T, N, C = t.shape
    return t.permute(0, 2, 1, 3).contiguous().view(B * N * T, C)


def from_rows(t, B, T, N):
    return t.view(B, N, T, -1).permute(0, 2, 1, 3)


def run(H, qkv, gy, valid, B, T, N, d):
    """fwd + bwd on bf16 device copies of qkv (B,T,N,3d) and gy (B,T,N,d); every output prefilled with NaN"""
    dev = torch.device("cuda:0")
    heads, M, S = d // 64, B * T * N, T * N
    qd = to_rows(qkv).to(dev, torch.bfloat16)
    gd = to_rows(gy).to(dev, torch.bfloat16)
    vd = valid.to(dev) if valid is not None else None
    out = torch.full((M, d), float("nan"), device=dev, dtype=torch.bfloat16)
    lse = torch.full((B * heads * S,), float("nan"), device=dev)
    H.call("vlg_attention_clip_fwd_bf16", qd.data_ptr(), H.ptr(vd), out.data_ptr(), lse.data_ptr(), B, T, N, d, stream())
    dqkv = torch.full((M, 3 * d), float("nan"), device=dev, dtype=torch.bfloat16)
    delta = torch.full((B * heads * S,), float("nan"), device=dev)
    H.call("vlg_attention_clip_bwd_bf16", qd.data_ptr(), H.ptr(vd), out.data_ptr(), gd.data_ptr(), lse.data_ptr(),
           delta.data_ptr(), dqkv.data_ptr(), B, T, N, d, stream())
    torch.cuda.synchronize()
    return {"out": from_rows(out, B, T, N).float().cpu(), "lse": lse.cpu(), "delta": delta.cpu(),
            "dqkv": from_rows(dqkv, B, T, N).float().cpu(), "out_rows": out.float().cpu(), "gd": gd.float().cpu()}


def inputs(B, T, N, d, masked, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(B, T, N, 3 * d, generator=g) * 0.7).bfloat16().float()
    gy = torch.randn(B, T, N, d, generator=g).bfloat16().float()
    valid = (torch.rand(B, T, N, generator=g) > 0.3).float() if masked else None
    return qkv, gy, valid


def lse_want(qkv, valid, heads):
    """fp64 log2-sum-exp of the visible scaled scores, laid out (b, head, frame-major token)"""
    B, T, N, _ = qkv.shape
    d, S = heads * 64, T * N
    x = qkv.double().reshape(B, S, 3 * d)
    q = x[..., :d].reshape(B, S, heads, 64).transpose(1, 2)
    k = x[..., d:2 * d].reshape(B, S, heads, 64).transpose(1, 2)
    s = q @ k.transpose(-1, -2) / 8.0                                         # (B, heads, S, S)
    fr = torch.arange(S) // N
    vis = (fr[None, :] <= fr[:, None])[None].expand(B, S, S).clone()
    if valid is not None:
        vis &= (valid.reshape(B, S) > 0)[:, None, :]
    vis |= torch.eye(S, dtype=torch.bool)[None]
    s = s.masked_fill(~vis[:, None], float("-inf"))
    return (torch.logsumexp(s, dim=-1) / math.log(2.0)).reshape(-1)


def rel_l2(got, want):
    return float((got.double() - want.double()).norm() / want.double().norm())


@pytest.mark.parametrize("B,T,N,d,masked", SHAPES)
def test_clip_attention_bf16_against_fp64(H, B, T, N, d, masked):
    heads = d // 64
    qkv, gy, valid = inputs(B, T, N, d, masked, seed=B * 1000 + T * N + d)
    q = qkv.double().requires_grad_(True)
    want = O.clip_attention(q, heads, valid.double() if valid is not None else None)
    want.backward(gy.double())
    got = run(H, qkv, gy, valid, B, T, N, d)
    for k in ("out", "lse", "delta", "dqkv"):
        assert bool(torch.isfinite(got[k]).all()), k + " not fully written"
    # lse: fp32 scores from exact bf16 products - the sharp check on masks and scaling
    lw = lse_want(qkv, valid, heads)
    assert torch.allclose(got["lse"].double(), lw, rtol=1e-5, atol=1e-5), float((got["lse"].double() - lw).abs().max())
    w = want.detach()
    e = rel_l2(got["out"], w)
    assert e <= 1e-2, ("out rel L2", e)
    worst = float((got["out"].double() - w).abs().max())
    assert worst <= 2.0 ** -6 * float(w.abs().max()), ("out max err", worst)
    # delta = <dO, O> on the stored bf16 values, fp32
    dw = (got["gd"].double() * got["out_rows"].double()).view(B, N, T, heads, 64).sum(-1)     # (b, n, t, head)
    dw = dw.permute(0, 3, 2, 1).reshape(-1)                                                    # (b, head, t, n)
    assert torch.allclose(got["delta"].double(), dw, rtol=1e-4, atol=1e-4 * float(dw.abs().max()))
    for i, name in enumerate(("dq", "dk", "dv")):
        g, r = got["dqkv"][..., i * d:(i + 1) * d], q.grad[..., i * d:(i + 1) * d]
        e = rel_l2(g, r)
        assert e <= 2e-2, (name, "rel L2", e)
        worst = float((g.double() - r).abs().max())
        assert worst <= 6e-2 * float(r.abs().max()), (name, "max err", worst)


@pytest.mark.parametrize("B,T,N,d", [(2, 16, 24, 64), (1, 32, 64, 128), (2, 8, 16, 512)])
def test_clip_attention_bf16_masks_are_exact(H, B, T, N, d):
    """No tolerance: padded slots and later frames contribute exactly nothing, and two identical calls agree bit for bit."""
    qkv, gy, valid = inputs(B, T, N, d, True, seed=77 + N)
    base = run(H, qkv, gy, valid, B, T, N, d)
    again = run(H, qkv, gy, valid, B, T, N, d)
    for k in ("out", "lse", "delta", "dqkv"):
        assert torch.equal(base[k], again[k]), k + " is not reproducible"
    # padded slots' q, k, v changed: every other row of out and dq unchanged
    pad = valid == 0
    assert bool(pad.any())
    q2 = qkv.clone()
    q2[pad] = (torch.randn(int(pad.sum()), 3 * d) * 3.0).bfloat16().float()
    got = run(H, q2, gy, valid, B, T, N, d)
    keep = ~pad
    assert torch.equal(got["out"][keep], base["out"][keep])
    assert torch.equal(got["dqkv"][..., :d][keep], base["dqkv"][..., :d][keep])
    # the tokens of frame t changed: every row of frames < t unchanged
    t = T // 2
    q3 = qkv.clone()
    q3[:, t] = (torch.randn(B, N, 3 * d) * 0.7).bfloat16().float()
    got = run(H, q3, gy, valid, B, T, N, d)
    assert torch.equal(got["out"][:, :t], base["out"][:, :t])
    assert torch.equal(got["dqkv"][:, :t, :, :d], base["dqkv"][:, :t, :, :d])
    assert not torch.equal(got["out"][:, t:], base["out"][:, t:])


def test_clip_attention_bf16_refuses_what_fp32_refuses(H):
    lib = H.load()
    dev = torch.device("cuda:0")
    q32 = torch.zeros(64 * 3 * 128, device=dev)
    o32 = torch.zeros(64 * 128, device=dev)
    q16 = torch.zeros(64 * 3 * 128, device=dev, dtype=torch.bfloat16)
    o16 = torch.zeros(64 * 128, device=dev, dtype=torch.bfloat16)
    lse = torch.zeros(1024, device=dev)
    delta = torch.zeros(1024, device=dev)
    s = stream()
    cases = [(0, 0, 1, 3, 5, 64), (0, 0, 1, 4, 8, 96), (4, 2, 1, 4, 8, 64)]   # T*N = 15; d = 96; misaligned qkv
    for off32, off16, B, T, N, d in cases:
        f = lib.vlg_attention_clip_fwd(q32.data_ptr() + off32, 0, o32.data_ptr(), lse.data_ptr(), B, T, N, d, s)
        g = lib.vlg_attention_clip_fwd_bf16(q16.data_ptr() + off16, 0, o16.data_ptr(), lse.data_ptr(), B, T, N, d, s)
        assert f == g != 0, (f, g, (B, T, N, d))
        f = lib.vlg_attention_clip_bwd(q32.data_ptr() + off32, 0, o32.data_ptr(), o32.data_ptr(), lse.data_ptr(),
                                       delta.data_ptr(), q32.data_ptr(), B, T, N, d, s)
        g = lib.vlg_attention_clip_bwd_bf16(q16.data_ptr() + off16, 0, o16.data_ptr(), o16.data_ptr(), lse.data_ptr(),
                                            delta.data_ptr(), q16.data_ptr(), B, T, N, d, s)
        assert f == g != 0, (f, g, (B, T, N, d))
    assert lib.vlg_attention_clip_fwd_bf16(q16.data_ptr(), 0, o16.data_ptr(), lse.data_ptr(), 1, 3, 5, 64, s) == 1001
    assert lib.vlg_attention_clip_fwd_bf16(q16.data_ptr() + 2, 0, o16.data_ptr(), lse.data_ptr(), 1, 4, 8, 64, s) == 1002
    # every tensor but valid is required: a null one is refused by all four entries before anything is enqueued
    B, T, N, d = 1, 4, 8, 64
    for sfx, dt in (("", torch.float32), ("_bf16", torch.bfloat16)):
        fwd, bwd = getattr(lib, "vlg_attention_clip_fwd" + sfx), getattr(lib, "vlg_attention_clip_bwd" + sfx)
        qkv, dout = torch.randn(32, 192, device=dev).to(dt), torch.randn(32, 64, device=dev).to(dt)
        out, dqkv = torch.full((32, 64), 3.0, device=dev, dtype=dt), torch.full((32, 192), 5.0, device=dev, dtype=dt)
        lse, delta = torch.full((32,), 7.0, device=dev), torch.full((32,), 9.0, device=dev)
        written = (out, dqkv, lse, delta)
        before = [t.clone() for t in written]
        for entry, tensors in ((fwd, (qkv, out, lse)), (bwd, (qkv, out, dout, lse, delta, dqkv))):
            for i in range(len(tensors)):
                p = [0 if j == i else t.data_ptr() for j, t in enumerate(tensors)]
                assert entry(p[0], 0, *p[1:], B, T, N, d, s) == 1002, (sfx, len(tensors), i)
        torch.cuda.synchronize()
        for t, keep in zip(written, before):
            assert torch.equal(t, keep), sfx
