"""GPU: attention inside a frame (vlg_attention_frame_fwd / _bwd and their bf16 forms; the FRAME instantiations of
csrc/attention_clip.hip, the odd layers of attention = "factored") through the C ABI, against tests/factored_ref.py:
oracle.clip_attention on the B*T one-frame clips, with autograd, in fp64.

Every output buffer starts as a NaN sentinel with a guard behind it (the conventions of test_hip_layout_ops.py).  Bars are the
project's own: fp32 by helpers.vs_cpu32 (4x torch-CPU fp32's error + 2^-20 of the largest value) and lse within
1e-5 (1 + |lse|); bf16 on bf16-representable inputs at out rel-L2 1e-2 / 2^-6 of the largest value, gradients 2e-2 / 6e-2,
lse 1e-5.  The exact checks have no tolerance.

Shapes: (2,4,8) four frames inside one 32-token tile; (3,8,4) eight frames inside one tile; (1,4,40) frame boundaries inside
tiles; (2,4,72) a frame over three tiles and a 128-token block over two frames; (1,16,64) the production alignment, two whole
tiles per frame; (1,1,32) T = 1."""
import math

import pytest
import torch

import factored_ref as R
from helpers import vs_cpu32
from test_hip_clip_attention_bf16 import from_rows, lse_want, rel_l2, to_rows
from test_hip_layout_ops import _buf, _guard
from test_hip_pixel_ops import within

pytestmark = pytest.mark.gpu

SHAPES = [(2, 4, 8, 64), (3, 8, 4, 64), (1, 4, 40, 128), (2, 4, 72, 64), (1, 16, 64, 256), (1, 1, 32, 64)]
MASKS = ("null", "random", "prefix")
BF = torch.bfloat16


@pytest.fixture(scope="module")
def H():
    from vlg import hip
    hip.load()
    return hip


def S():
    return torch.cuda.current_stream().cuda_stream


def make_valid(kind, B, T, N, g):
    if kind == "null":
        return None
    if kind == "random":
        return (torch.rand(B, T, N, generator=g) > 0.3).float()
    nv = torch.randint(1, N + 1, (B, T), generator=g)              # prefix: the first nv slots of every frame are real
    return (torch.arange(N)[None, None] < nv[..., None]).float()


def inputs(B, T, N, d, kind, bf16, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, T, N, 3 * d, generator=g) * (0.7 if bf16 else 1.5)
    gy = torch.randn(B, T, N, d, generator=g)
    if bf16:
        qkv, gy = qkv.bfloat16().float(), gy.bfloat16().float()
    return qkv, gy, make_valid(kind, B, T, N, g)


def frame_run(H, dev, qkv, gy, valid, bf16):
    """fwd + bwd on device copies in the internal row order; every output a sentinel-prefilled buffer with a guard"""
    B, T, N, d3 = qkv.shape
    d = d3 // 3
    M, nl = B * T * N, B * (d // 64) * T * N
    sfx, dt = ("_bf16", BF) if bf16 else ("", torch.float32)
    qd, gd = to_rows(qkv).to(dev, dt), to_rows(gy).to(dev, dt)
    vd = valid.to(dev) if valid is not None else None
    oraw, out = _buf(M * d, dev, bf16)
    lraw, lse = _buf(nl, dev)
    H.call("vlg_attention_frame_fwd" + sfx, qd.data_ptr(), H.ptr(vd), out.data_ptr(), lse.data_ptr(), B, T, N, d, S())
    draw, dqkv = _buf(M * 3 * d, dev, bf16)
    eraw, delta = _buf(nl, dev)
    H.call("vlg_attention_frame_bwd" + sfx, qd.data_ptr(), H.ptr(vd), out.data_ptr(), gd.data_ptr(), lse.data_ptr(),
           delta.data_ptr(), dqkv.data_ptr(), B, T, N, d, S())
    torch.cuda.synchronize()
    for raw, n, what in ((oraw, M * d, "out"), (lraw, nl, "lse"), (draw, M * 3 * d, "dqkv"), (eraw, nl, "delta")):
        _guard(raw, n, "frame attention " + what)
    got = {"out": from_rows(out.view(M, d).float().cpu(), B, T, N), "lse": lse.cpu(), "delta": delta.cpu(),
           "dqkv": from_rows(dqkv.view(M, 3 * d).float().cpu(), B, T, N)}
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), k + " not fully written"
    return got


def frame_lse_want(qkv, valid, heads):
    """fp64 log2-sum-exp of the visible scores in the kernels' layout (b, head, frame-major token)"""
    B, T, N, d3 = qkv.shape
    v = None if valid is None else valid.reshape(B * T, 1, N)
    lw = lse_want(qkv.reshape(B * T, 1, N, d3), v, heads)               # (b, t, head, n)
    return lw.reshape(B, T, heads, N).permute(0, 2, 1, 3).reshape(-1)


_REF = {}


def reference(B, T, N, d, kind, bf16):
    """the inputs of a case and their fp64 / torch-CPU fp32 results, computed once and shared"""
    key = (B, T, N, d, kind, bf16)
    if key not in _REF:
        qkv, gy, valid = inputs(B, T, N, d, kind, bf16, seed=B * 1000 + T * N + d + MASKS.index(kind))
        ref = {}
        for dt in (torch.float64, torch.float32):
            q = qkv.detach().to(dt, copy=True).requires_grad_(True)
            o = R.frame_attention(q, d // 64, valid.to(dt) if valid is not None else None)
            o.backward(gy.to(dt))
            ref[dt] = (o.detach(), q.grad)
        _REF[key] = (qkv, gy, valid, ref, frame_lse_want(qkv, valid, d // 64))
    return _REF[key]


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("B,T,N,d", SHAPES)
def test_frame_attention_fp32_against_fp64(H, dev, B, T, N, d, kind):
    qkv, gy, valid, ref, lw = reference(B, T, N, d, kind, False)
    got = frame_run(H, dev, qkv, gy, valid, False)
    vs_cpu32(got["out"], ref[torch.float64][0], ref[torch.float32][0], "frame out")
    for i, name in enumerate(("dq", "dk", "dv")):
        sl = slice(i * d, (i + 1) * d)
        vs_cpu32(got["dqkv"][..., sl], ref[torch.float64][1][..., sl], ref[torch.float32][1][..., sl], "frame " + name)
    within(got["lse"], lw, 1e-5 * (1 + lw.abs()), "frame lse")


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("B,T,N,d", SHAPES)
def test_frame_attention_bf16_against_fp64(H, dev, B, T, N, d, kind):
    qkv, gy, valid, ref, lw = reference(B, T, N, d, kind, True)
    got = frame_run(H, dev, qkv, gy, valid, True)
    assert torch.allclose(got["lse"].double(), lw, rtol=1e-5, atol=1e-5), float((got["lse"].double() - lw).abs().max())
    w, gw = ref[torch.float64]
    e = rel_l2(got["out"], w)
    worst = float((got["out"].double() - w).abs().max())
    print("\nbf16 %s %s: out rel L2 %.2e, max err %.2e of %.2e" % ((B, T, N, d), kind, e, worst, float(w.abs().max())))
    assert e <= 1e-2, ("out rel L2", e)
    assert worst <= 2.0 ** -6 * float(w.abs().max()), ("out max err", worst)
    for i, name in enumerate(("dq", "dk", "dv")):
        g, r = got["dqkv"][..., i * d:(i + 1) * d], gw[..., i * d:(i + 1) * d]
        e = rel_l2(g, r)
        worst = float((g.double() - r).abs().max())
        print("  %s rel L2 %.2e, max err %.2e of %.2e" % (name, e, worst, float(r.abs().max())))
        assert e <= 2e-2, (name, "rel L2", e)
        assert worst <= 6e-2 * float(r.abs().max()), (name, "max err", worst)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,T,N,d", SHAPES)
def test_frame_attention_exact_properties(H, dev, B, T, N, d, bf16):
    """No tolerance.  Two calls agree bit for bit; a clip alone equals the same clip inside a batch; with every slot padded
    out == v and dv == dout; what the OTHER frames hold - q, k, v and dout - reaches nothing of a frame; a padded slot's
    q, k, v reach no valid token's out or dq (its query still attends, so dk and dv of the valid keys are held fixed only
    where its dout is zero - then they are bit-identical too)."""
    g = torch.Generator().manual_seed(99 + N)
    rnd = (lambda *s: (torch.randn(*s, generator=g) * 0.9).bfloat16().float()) if bf16 else (lambda *s: torch.randn(*s, generator=g) * 0.9)
    qkv, gy, valid = inputs(B, T, N, d, "random", bf16, seed=77 + N)
    base = frame_run(H, dev, qkv, gy, valid, bf16)
    again = frame_run(H, dev, qkv, gy, valid, bf16)
    for k in ("out", "lse", "delta", "dqkv"):
        assert torch.equal(base[k], again[k]), k + " is not reproducible"
    # a clip alone and inside a batch, behind another clip
    one = frame_run(H, dev, qkv[:1], gy[:1], valid[:1], bf16)
    q2, g2, v2 = (torch.cat([rnd(1, *t.shape[1:]), t[:1]]) for t in (qkv, gy, valid))
    two = frame_run(H, dev, q2, g2, (v2 > 0).float(), bf16)
    for k in ("out", "dqkv"):
        assert torch.equal(two[k][1], one[k][0]), k + " of a clip depends on the batch around it"
    # every slot padded: each token sees itself alone
    none = frame_run(H, dev, qkv, gy, torch.zeros(B, T, N), bf16)
    assert torch.equal(none["out"], qkv[..., 2 * d:]), "a token that sees only itself must return its V row"
    assert torch.equal(none["dqkv"][..., 2 * d:], gy), "dv of a token that sees only itself must be its dout"
    # the other frames
    if T > 1:
        t = T // 2
        other = torch.ones(T, dtype=torch.bool)
        other[t] = False
        q3, g3 = qkv.clone(), gy.clone()
        q3[:, other] = rnd(B, T - 1, N, 3 * d)
        g3[:, other] = rnd(B, T - 1, N, d)
        got = frame_run(H, dev, q3, g3, valid, bf16)
        assert torch.equal(got["out"][:, t], base["out"][:, t]), "another frame reached a frame's output"
        assert torch.equal(got["dqkv"][:, t], base["dqkv"][:, t]), "another frame reached a frame's dq, dk or dv"
        assert not torch.equal(got["out"][:, other], base["out"][:, other])
    # padded slots
    pad = valid == 0
    assert bool(pad.any()) and bool((~pad).any())
    q4 = qkv.clone()
    q4[pad] = rnd(int(pad.sum()), 3 * d) * 3.0
    got = frame_run(H, dev, q4, gy, valid, bf16)
    assert torch.equal(got["out"][~pad], base["out"][~pad]), "a padded slot's q, k, v reached another token's output"
    assert torch.equal(got["dqkv"][..., :d][~pad], base["dqkv"][..., :d][~pad]), "a padded slot's q, k, v reached another token's dq"
    g5 = gy.clone()
    g5[pad] = 0.0
    a, b = frame_run(H, dev, qkv, g5, valid, bf16), frame_run(H, dev, q4, g5, valid, bf16)
    assert torch.equal(a["dqkv"][~pad], b["dqkv"][~pad]), "a padded slot with no dout reached a valid token's dq, dk or dv"


def test_frame_entries_refuse_what_the_clip_entries_refuse(H, dev):
    lib = H.load()
    q = torch.zeros(64 * 3 * 128, device=dev)
    o = torch.full((64 * 128,), float("nan"), device=dev)
    lse = torch.full((64 * 2,), float("nan"), device=dev)
    s = S()
    for sfx in ("", "_bf16"):
        fwd, bwd = getattr(lib, "vlg_attention_frame_fwd" + sfx), getattr(lib, "vlg_attention_frame_bwd" + sfx)
        assert fwd(q.data_ptr(), 0, o.data_ptr(), lse.data_ptr(), 1, 3, 5, 64, s) == 1001            # T*N not a multiple of 32
        assert fwd(q.data_ptr() + 2, 0, o.data_ptr(), lse.data_ptr(), 1, 4, 8, 64, s) == 1002
        assert fwd(q.data_ptr(), 0, o.data_ptr(), 0, 1, 4, 8, 64, s) == 1002
        assert bwd(q.data_ptr(), 0, o.data_ptr(), o.data_ptr(), lse.data_ptr(), 0, q.data_ptr(), 1, 4, 8, 64, s) == 1002
        assert bwd(q.data_ptr(), 0, o.data_ptr(), o.data_ptr(), lse.data_ptr(), lse.data_ptr(), q.data_ptr(), 1, 4, 8, 96, s) == 1001
    torch.cuda.synchronize()
    assert bool(torch.isnan(o).all()) and bool(torch.isnan(lse).all()), "a refused call wrote something"
