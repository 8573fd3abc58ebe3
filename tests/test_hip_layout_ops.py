"""The layout-token step's kernels outside the GEMMs - temporal attention (csrc/attention.hip), per-clip attention in fp32
(csrc/attention_clip.hip), layer-norm (csrc/layernorm.hip), the embedding (csrc/embed.hip), the fused layout loss
(csrc/loss.hip), slab reduction and Adam (csrc/optim.hip) - one C-ABI entry point at a time, against
oracle/layout_spec.py, F.layer_norm and Adam arithmetic run in float64 on the same fp32 (or bf16-representable) inputs.

Conventions of test_hip_pixel_ops.py: every output buffer starts as a NaN sentinel and has a guard after it, every element
a kernel owns must be written and finite, padding columns, slab padding and guards keep their sentinel bits.  Bars: gathers
and selects bitwise; elsewhere at most 4x the error of torch-CPU fp32 against fp64 on the same inputs plus a stated floor
(the test_hip_gemm_paths rule), or a first-order bound c EPS sum|terms| derived from the operation (EPS = 2^-24); a bf16
output adds one bf16 rounding (2^-8 of the value).

The `prod` cases run each grid-stride loop more than once and end on a ragged tail: layer-norm above 2048 blocks x 4 waves
x LN_ROWS rows forward and 512 x 4 x LN_ROWS backward, the embedding backward above 256 blocks x G groups of sequences,
the loss above 1024 blocks x 128 tokens, Adam and the flat slab reduction above 2048 blocks x 1024 floats; the temporal
attention runs at the metric shape (2048 sequences, T = 16, d = 256).
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import vs_cpu32
from oracle import layout_spec as O
from test_hip_clip_attention_bf16 import lse_want
from test_hip_pixel_ops import EPS, SENT, SENT16, f32, sentinel, untouched, within

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
NAN = float("nan")
GUARD = 64


@pytest.fixture(scope="module")
def H():
    from vlg import hip
    hip.load()
    return hip


def S():
    return torch.cuda.current_stream().cuda_stream


def _buf(n, dev, bf16=False):
    """n elements and a guard of GUARD more, every bit the sentinel: (raw integer tensor, value view of the n)."""
    if bf16:
        raw = torch.full((n + GUARD,), SENT16, dtype=torch.int16, device=dev)
        return raw, raw.view(BF)[:n]
    raw = sentinel(n + GUARD, dev)
    return raw, f32(raw)[:n]


def _guard(raw, n, what):
    sent = SENT16 if raw.dtype == torch.int16 else SENT
    assert bool((raw[n:] == sent).all()), "%s wrote past its %d elements" % (what, n)


# ------------------------------------------------------------------------------------------------ temporal attention
def _rows(t):
    """(1, T, n_seq, C) -> the internal row order (seq, frame)"""
    return t[0].permute(1, 0, 2).contiguous().view(-1, t.shape[-1])


def _attn_inputs(T, d, n_seq, seed, bf16):
    """qkv (1, T, n_seq, 3d) and dout: q and k of every other sequence x5, so that its scaled scores reach |s| ~ 60-90 and
    its softmax rows are near one-hot (the max subtraction matters); the other sequences plain randn."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(1, T, n_seq, 3 * d, generator=g)
    qkv[:, :, 0::2, :2 * d] *= 5.0
    do = torch.randn(1, T, n_seq, d, generator=g)
    if bf16:
        qkv, do = qkv.to(BF).float(), do.to(BF).float()
    return qkv, do


def _attn_ref(qkv, do, dt):
    q = qkv.detach().to(dt, copy=True).requires_grad_(True)
    o = O.temporal_attention(q, q.shape[-1] // 192)
    o.backward(do.to(dt))
    return _rows(o.detach()), _rows(q.grad)


def _attn_run(H, dev, qkv, do, bf16):
    """vlg_attention_fwd / _bwd (or the _bf16 pair) -> (out (rows, d), dqkv (rows, 3d)) as fp32 CPU tensors."""
    T, n_seq, d = qkv.shape[1], qkv.shape[2], qkv.shape[3] // 3
    rows = n_seq * T
    dt = BF if bf16 else torch.float32
    sfx = "_bf16" if bf16 else ""
    qd, gd = _rows(qkv).to(dev).to(dt), _rows(do).to(dev).to(dt)
    oraw, o = _buf(rows * d, dev, bf16)
    H.call("vlg_attention_fwd" + sfx, qd.data_ptr(), o.data_ptr(), n_seq, T, d, S())
    draw, dq = _buf(rows * 3 * d, dev, bf16)
    H.call("vlg_attention_bwd" + sfx, qd.data_ptr(), gd.data_ptr(), dq.data_ptr(), n_seq, T, d, S())
    torch.cuda.synchronize()
    _guard(oraw, rows * d, "attention fwd")
    _guard(draw, rows * 3 * d, "attention bwd")
    return o.float().view(rows, d).cpu(), dq.float().view(rows, 3 * d).cpu()


# T x d grid; n_seq d/64 = 7 (d = 64) and 18 (d = 192) leave 3 and 2 items in the last 4-wave block of the T = 16 / 32
# kernels, the extra rows 5, 15 and 21 (1, 3, 1 mod 4)
_NSEQ = {64: 7, 192: 6, 256: 5, 512: 3}
ATTN = [(T, d, _NSEQ[d]) for T in (4, 8, 16, 32) for d in (64, 192, 256, 512)]
ATTN += [(16, 64, 5), (32, 64, 5), (16, 192, 5), (32, 192, 7), pytest.param(16, 256, 2048, id="prod")]


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("T,d,n_seq", ATTN)
def test_temporal_attention(H, dev, T, d, n_seq, bf16):
    """vlg_attention_fwd / _bwd (fp32 and bf16 storage) against oracle.temporal_attention and its autograd in fp64 on the
    same inputs.  Bar: 4x torch-CPU fp32's error plus 2^-20 of the largest value; bf16 outputs one bf16 rounding more
    (the kernels compute in fp32 from the bf16 values).  Unwritten tail items of the last block stay NaN and fail."""
    qkv, do = _attn_inputs(T, d, n_seq, seed=T * 1000 + d + n_seq, bf16=bf16)
    o64, dq64 = _attn_ref(qkv, do, torch.float64)
    o32, dq32 = _attn_ref(qkv, do, torch.float32)
    o, dq = _attn_run(H, dev, qkv, do, bf16)
    vs_cpu32(o, o64, o32, "attention out", bf16=bf16)
    for i, name in enumerate(("dq", "dk", "dv")):
        sl = slice(i * d, (i + 1) * d)
        vs_cpu32(dq[:, sl], dq64[:, sl], dq32[:, sl], "attention " + name, bf16=bf16)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("T,d,n_seq", [(4, 128, 5), (8, 64, 7), (16, 192, 5), (32, 128, 3)])
def test_temporal_attention_exact(H, dev, T, d, n_seq, bf16):
    """Bit for bit: (1) other values of q, k, v in frames > t leave the outputs of frames <= t unchanged; (2) dout = 0 on
    frames > t gives dq, dk, dv = 0 exactly there; (3) a NaN in the q row of frame i of one (slot, head) leaves every
    other (slot, head) unchanged; inside it the output and dq are NaN exactly where torch's fp64 result is (row i) and
    every other row is unchanged, and dk, dv of frames <= i are NaN (as torch's).  dk, dv of frames > i differ from torch
    between the kernels and are not pinned (layout step NaN contract)."""
    qkv, do = _attn_inputs(T, d, n_seq, seed=T + d + n_seq, bf16=bf16)
    rd = (lambda t: t.to(BF).float()) if bf16 else (lambda t: t)
    o, dq = _attn_run(H, dev, qkv, do, bf16)
    t = T // 2 - 1
    g = torch.Generator().manual_seed(T * d)
    q2 = qkv.clone()
    q2[:, t + 1:] = rd(torch.randn(1, T - t - 1, n_seq, 3 * d, generator=g) * 3)
    o2, _ = _attn_run(H, dev, q2, do, bf16)
    fr = lambda x: x.view(n_seq, T, -1)
    assert torch.equal(fr(o2)[:, :t + 1], fr(o)[:, :t + 1]), "later frames changed the output of earlier ones"
    assert not torch.equal(fr(o2)[:, t + 1:], fr(o)[:, t + 1:])
    do3 = do.clone()
    do3[:, t + 1:] = 0
    _, dq3 = _attn_run(H, dev, qkv, do3, bf16)
    assert bool((fr(dq3)[:, t + 1:] == 0).all()), "dq / dk / dv of frames without an upstream gradient are not 0"
    nh, s, h, i = d // 64, n_seq // 2, d // 64 - 1, T // 2
    q4 = qkv.clone()
    q4[0, i, s, h * 64 + 5] = NAN
    o4, dq4 = _attn_run(H, dev, q4, do, bf16)
    heads = lambda x, k: x.view(n_seq, T, k, nh, 64).permute(0, 3, 1, 2, 4)      # (seq, head, frame, k, 64)
    other = torch.ones(n_seq, nh, dtype=torch.bool)
    other[s, h] = False
    assert torch.equal(heads(o4, 1)[other], heads(o, 1)[other]), "a NaN leaked into another (slot, head)'s output"
    assert torch.equal(heads(dq4, 3)[other], heads(dq, 3)[other]), "a NaN leaked into another (slot, head)'s gradient"
    o64, dq64 = _attn_ref(q4, do, torch.float64)
    assert torch.equal(torch.isnan(o4), torch.isnan(o64)), "output NaN positions differ from torch's"
    assert torch.equal(torch.isnan(dq4[:, :d]), torch.isnan(dq64[:, :d])), "dq NaN positions differ from torch's"
    keep = ~torch.isnan(o64)
    assert torch.equal(o4[keep], o[keep]), "rows torch leaves finite changed"
    keep = ~torch.isnan(dq64[:, :d])
    assert torch.equal(dq4[:, :d][keep], dq[:, :d][keep])
    assert bool(torch.isnan(heads(dq4, 3)[s, h, :i + 1, 1:]).all()), "dk / dv of frames <= the poisoned one not all NaN"


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("d,n_seq", [(64, 5), (192, 3)])
def test_temporal_attention_first_block_is_t16(H, dev, d, n_seq, bf16):
    """Bit for bit: the MFMA scheme is one body over T / 16 query blocks, so frames 0..15 of a T = 32 sequence get what the
    T = 16 kernel computes on those frames alone - the output, and with dout = 0 on frames 16..31 (the later query block
    then adds exact zeros to dk, dv of the first key tile) also dq, dk, dv."""
    qkv, do = _attn_inputs(32, d, n_seq, seed=32 + d + n_seq, bf16=bf16)
    do[:, 16:] = 0
    o32, dq32 = _attn_run(H, dev, qkv, do, bf16)
    o16, dq16 = _attn_run(H, dev, qkv[:, :16], do[:, :16], bf16)
    first = lambda x: x.view(n_seq, 32, -1)[:, :16].reshape(n_seq * 16, -1)
    assert torch.equal(first(o32), o16), "output of frames 0..15 at T = 32 differs from T = 16"
    for i, name in enumerate(("dq", "dk", "dv")):
        sl = slice(i * d, (i + 1) * d)
        assert torch.equal(first(dq32)[:, sl], dq16[:, sl]), "%s of frames 0..15 at T = 32 differs from T = 16" % name


# ------------------------------------------------------------------------------------------------ per-clip attention fp32
def _to_rows(t):
    """(B,T,N,C) -> the internal row order (b, n, t)"""
    B, T, N, C = t.shape
    return t.permute(0, 2, 1, 3).contiguous().view(B * N * T, C)


def _from_rows(t, B, T, N):
    return t.view(B, N, T, -1).permute(0, 2, 1, 3)


def _clip_run(H, dev, qkv, gy, valid):
    B, T, N, d3 = qkv.shape
    d = d3 // 3
    M, nl = B * T * N, B * (d // 64) * T * N
    qd, gd = _to_rows(qkv).to(dev), _to_rows(gy).to(dev)
    vd = valid.to(dev) if valid is not None else None
    oraw, out = _buf(M * d, dev)
    lraw, lse = _buf(nl, dev)
    H.call("vlg_attention_clip_fwd", qd.data_ptr(), H.ptr(vd), out.data_ptr(), lse.data_ptr(), B, T, N, d, S())
    draw, dqkv = _buf(M * 3 * d, dev)
    eraw, delta = _buf(nl, dev)
    H.call("vlg_attention_clip_bwd", qd.data_ptr(), H.ptr(vd), out.data_ptr(), gd.data_ptr(), lse.data_ptr(), delta.data_ptr(),
           dqkv.data_ptr(), B, T, N, d, S())
    torch.cuda.synchronize()
    for raw, n, what in ((oraw, M * d, "out"), (lraw, nl, "lse"), (draw, M * 3 * d, "dqkv"), (eraw, nl, "delta")):
        _guard(raw, n, "clip attention " + what)
    return {"out": _from_rows(out.cpu(), B, T, N), "lse": lse.cpu(), "delta": delta.cpu(),
            "dqkv": _from_rows(dqkv.cpu(), B, T, N)}


CLIP = [(2, 4, 8, 64), (1, 8, 24, 128), (2, 32, 5, 64), pytest.param(2, 16, 64, 256, id="prod")]


@pytest.mark.parametrize("mode", ["null", "ones", "masked"])
@pytest.mark.parametrize("B,T,N,d", CLIP)
def test_clip_attention_fp32(H, dev, B, T, N, d, mode):
    """vlg_attention_clip_fwd / _bwd against oracle.clip_attention and its autograd in fp64.  valid = NULL and valid = all
    ones take different tile paths (CLIP_TILE_ELEMENTWISE) and must both meet the bar: 4x torch-CPU fp32's error plus 2^-20
    of the largest value.  lse (log2 domain) within 1e-5 of fp64, as the bf16 test holds it."""
    g = torch.Generator().manual_seed(B * 100 + T * N + d)
    qkv = torch.randn(B, T, N, 3 * d, generator=g) * 1.5
    gy = torch.randn(B, T, N, d, generator=g)
    valid = {"null": None, "ones": torch.ones(B, T, N), "masked": (torch.rand(B, T, N, generator=g) > 0.3).float()}[mode]
    ref = {}
    for dt in (torch.float64, torch.float32):
        q = qkv.detach().to(dt, copy=True).requires_grad_(True)
        o = O.clip_attention(q, d // 64, valid.to(dt) if valid is not None else None)
        o.backward(gy.to(dt))
        ref[dt] = (o.detach(), q.grad)
    got = _clip_run(H, dev, qkv, gy, valid)
    vs_cpu32(got["out"], ref[torch.float64][0], ref[torch.float32][0], "clip out")
    for i, name in enumerate(("dq", "dk", "dv")):
        sl = slice(i * d, (i + 1) * d)
        vs_cpu32(got["dqkv"][..., sl], ref[torch.float64][1][..., sl], ref[torch.float32][1][..., sl], "clip " + name)
    lw = lse_want(qkv, valid, d // 64)
    within(got["lse"], lw, 1e-5 * (1 + lw.abs()), "clip lse")


@pytest.mark.parametrize("B,T,N,d", [(2, 16, 24, 64), (1, 32, 64, 128), (2, 8, 16, 512)])
def test_clip_attention_fp32_masks_are_exact(H, dev, B, T, N, d):
    """No tolerance (the fp32 counterpart of test_clip_attention_bf16_masks_are_exact): two identical calls agree bit for
    bit, padded slots contribute exactly nothing, and neither do the tokens of later frames."""
    g = torch.Generator().manual_seed(77 + N)
    qkv = torch.randn(B, T, N, 3 * d, generator=g) * 0.7
    gy = torch.randn(B, T, N, d, generator=g)
    valid = (torch.rand(B, T, N, generator=g) > 0.3).float()
    base = _clip_run(H, dev, qkv, gy, valid)
    again = _clip_run(H, dev, qkv, gy, valid)
    for k in ("out", "lse", "delta", "dqkv"):
        assert bool(torch.isfinite(base[k]).all()), k + " not fully written"
        assert torch.equal(base[k], again[k]), k + " is not reproducible"
    pad = valid == 0
    assert bool(pad.any())
    q2 = qkv.clone()
    q2[pad] = torch.randn(int(pad.sum()), 3 * d, generator=g) * 3.0
    got = _clip_run(H, dev, q2, gy, valid)
    keep = ~pad
    assert torch.equal(got["out"][keep], base["out"][keep]), "a padded slot's q, k, v reached another token's output"
    assert torch.equal(got["dqkv"][..., :d][keep], base["dqkv"][..., :d][keep])
    t = T // 2
    q3 = qkv.clone()
    q3[:, t] = torch.randn(B, N, 3 * d, generator=g) * 0.7
    got = _clip_run(H, dev, q3, gy, valid)
    assert torch.equal(got["out"][:, :t], base["out"][:, :t]), "a later frame reached an earlier frame's output"
    assert torch.equal(got["dqkv"][:, :t, :, :d], base["dqkv"][:, :t, :, :d])
    assert not torch.equal(got["out"][:, t:], base["out"][:, t:])


# ------------------------------------------------------------------------------------------------ layer-norm
def _ln_R(d):
    E = d // 64
    return 4 if E <= 4 else 2 if E <= 8 else 1                 # LN_ROWS(E), csrc/layernorm.hip


LN = []
for _d in (64, 128, 192, 256, 512, 768, 1024):
    _R = _ln_R(_d)
    LN += [pytest.param(_d, 5 * _R + r, id="d%d-r%d" % (_d, 5 * _R + r)) for r in range(1, _R)] or [pytest.param(_d, 7, id="d%d-r7" % _d)]
    # above one backward trip (512 blocks x 4 waves x R rows), and above one forward trip (2048 x 4 x R); 1003 rows more:
    # a short last row group in the last trip
    LN += [pytest.param(_d, 512 * 4 * _R + 1003, id="prod-bwd-d%d" % _d), pytest.param(_d, 2048 * 4 * _R + 1003, id="prod-fwd-d%d" % _d)]


def _ln_inputs(rows, d, seed):
    """randn x 2 + 0.5 rows, every 7th row offset by 1e3, every 11th row constant (a value of the same randn x 2 + 0.5);
    dy bf16-representable (the bf16 backward reads the same values)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, d, generator=g) * 2 + 0.5
    x[3::7] += 1e3
    const = x[5::11]
    const.copy_((torch.randn(const.shape[0], 1, generator=g) * 2 + 0.5).expand_as(const))
    gam = torch.rand(d, generator=g) + 0.5
    bet = torch.randn(d, generator=g)
    dy = torch.randn(rows, d, generator=g).to(BF).float()
    res = torch.randn(rows, d, generator=g)
    return x, gam, bet, dy, res


def _ln_ref(x, gam, bet, dy, dt):
    xx, gg, bb = (t.detach().to(dt, copy=True).requires_grad_(True) for t in (x, gam, bet))
    y = F.layer_norm(xx, (x.shape[1],), gg, bb, O.LN_EPS)
    y.backward(dy.to(dt))
    return y.detach(), xx.grad, gg.grad, bb.grad


def _ln_bars(x, gam, bet, dy):
    """First-order bounds of the kernels' fp32 arithmetic (csrc/layernorm.hip), elementwise, constants doubled: the row
    sums are E = d/64 serial adds per lane, a 6-level shuffle tree and the 1/d scale (c = 2 (E + 8) roundings of the sum
    of |terms|); the mean's error moves x - mu, the variance and rstd; dx adds the two row sums of the backward (with the
    product of the x-hat and s2 errors, which rstd can make large)."""
    d = x.shape[1]
    c = 2 * (d // 64 + 8)
    xd, g, b, gy = x.double(), gam.double(), bet.double(), dy.double()
    mu = xd.mean(-1, keepdim=True)
    xc = xd - mu
    var = (xc * xc).mean(-1, keepdim=True)
    rs = 1.0 / torch.sqrt(var + O.LN_EPS)
    xh = xc * rs
    d_mu = c * EPS * xd.abs().mean(-1, keepdim=True)
    d_var = 2 * xc.abs().mean(-1, keepdim=True) * d_mu + d_mu * d_mu + (c + 4) * EPS * var
    d_rs = 0.5 * d_var / (var + O.LN_EPS) + 4 * EPS                         # relative
    d_xh = rs * (d_mu + 2 * EPS * xc.abs()) + xh.abs() * d_rs
    y = g.abs() * d_xh + 4 * EPS * ((g * xh).abs() + b.abs())
    a = gy * g
    s1, s2 = a.mean(-1, keepdim=True), (a * xh).mean(-1, keepdim=True)
    d_s1 = c * EPS * a.abs().mean(-1, keepdim=True)
    d_s2 = c * EPS * (a * xh).abs().mean(-1, keepdim=True) + (a.abs() * d_xh).mean(-1, keepdim=True)
    core = rs * (a - s1 - xh * s2)
    dx = core.abs() * d_rs + rs * (d_s1 + (xh.abs() + d_xh) * (s2.abs() + d_s2) - xh.abs() * s2.abs() +
                                   4 * EPS * (a.abs() + s1.abs() + (xh * s2).abs())) + 2 * EPS * core.abs()
    return {"y": y, "mean": (d_mu + 2 * EPS * mu.abs()).squeeze(-1), "rstd": (rs * d_rs).squeeze(-1), "dx": dx,
            "dg_terms": (gy * xh).abs().sum(0), "dg_xh": (gy.abs() * d_xh).sum(0), "db_terms": gy.abs().sum(0)}


@pytest.mark.parametrize("d,rows", LN)
def test_layernorm(H, dev, d, rows):
    """vlg_layernorm_fwd / _bwd and their bf16 variants against F.layer_norm and its autograd in fp64.  y, mean, rstd, dx:
    the bounds of _ln_bars (bf16 y one rounding more).  dgamma / dbeta, summed over vlg_layernorm_bwd_slabs(rows) slabs by
    vlg_reduce_slabs: 4x torch-CPU fp32's error plus (rows per lane + 4 waves + the slab reduction) EPS sum |terms| (and
    for dgamma the x-hat bound of each row times |dy|).  The fp32 backward adds into dres in place, the bf16 one runs with
    dres = NULL."""
    lib = H.load()
    x, gam, bet, dy, res = _ln_inputs(rows, d, seed=rows + d)
    y64, dx64, dg64, db64 = _ln_ref(x, gam, bet, dy, torch.float64)
    _, _, dg32, db32 = _ln_ref(x, gam, bet, dy, torch.float32)
    bar = _ln_bars(x, gam, bet, dy)
    xd, gd, bd = x.to(dev), gam.to(dev), bet.to(dev)
    n = rows * d
    ns = lib.vlg_layernorm_bwd_slabs(rows)
    cr = -(-rows // (ns * 4 * _ln_R(d))) * _ln_R(d) + 4 + -(-ns // 16) + 16
    dg_bar = 4 * float((dg32.double() - dg64).abs().max()) + cr * EPS * bar["dg_terms"] + bar["dg_xh"]
    db_bar = 4 * float((db32.double() - db64).abs().max()) + cr * EPS * bar["db_terms"]
    x64 = x.double()
    for bf16 in (False, True):
        tag = "bf16 " if bf16 else ""
        sfx = "_bf16" if bf16 else ""
        yraw, y = _buf(n, dev, bf16)
        mraw, mean = _buf(rows, dev)
        rraw, rstd = _buf(rows, dev)
        H.call("vlg_layernorm_fwd" + sfx, xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), y.data_ptr(), mean.data_ptr(),
               rstd.data_ptr(), rows, d, O.LN_EPS, S())
        torch.cuda.synchronize()
        for raw, k, what in ((yraw, n, "y"), (mraw, rows, "mean"), (rraw, rows, "rstd")):
            _guard(raw, k, tag + "ln fwd " + what)
        yb = bar["y"] + (2.0 ** -8 * y64.abs() if bf16 else 0)
        within(y.float().view(rows, d), y64, yb, tag + "ln y")
        within(mean, x64.mean(-1), bar["mean"], tag + "ln mean")
        within(rstd, 1.0 / torch.sqrt(x64.var(-1, unbiased=False) + O.LN_EPS), bar["rstd"], tag + "ln rstd")
        # backward: slabs of 2d floats at a stride of 2d + 4 (the padding keeps its sentinel)
        stride = 2 * d + 4
        sraw, slabs = _buf(ns * stride, dev)
        dyd = dy.to(dev).to(BF if bf16 else torch.float32)
        if bf16:
            dxraw, dx = _buf(n, dev)
            dres, want_dx, dxb = None, dx64, bar["dx"]
        else:
            dxraw = sentinel(n + GUARD, dev)
            f32(dxraw)[:n] = res.to(dev).view(-1)
            dx = f32(dxraw)[:n]
            dres, want_dx, dxb = dx, dx64 + res.double(), bar["dx"] + 2 * EPS * (res.double().abs() + dx64.abs())
        H.call("vlg_layernorm_bwd" + sfx, dyd.data_ptr(), xd.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gd.data_ptr(),
               H.ptr(dres), dx.data_ptr(), slabs.data_ptr(), stride, ns * stride, rows, d, S())
        torch.cuda.synchronize()
        _guard(dxraw, n, tag + "ln dx")
        owned = torch.zeros(ns * stride + GUARD, dtype=torch.bool, device=dev)
        owned[:ns * stride].view(ns, stride)[:, :2 * d] = True
        untouched(sraw, owned, tag + "ln bwd slabs")
        within(dx.view(rows, d), want_dx, dxb, tag + "ln dx" + ("" if bf16 else " (+ dres, in place)"))
        gb = torch.empty(2 * d, device=dev)
        H.call("vlg_reduce_slabs", slabs.data_ptr(), stride, ns, gb.data_ptr(), 2 * d, S())
        torch.cuda.synchronize()
        within(gb[:d], dg64, dg_bar, tag + "ln dgamma")
        within(gb[d:], db64, db_bar, tag + "ln dbeta")


# ------------------------------------------------------------------------------------------------ embedding
def _embed_groups(T, d, vocab):
    """csrc/embed.hip embed_bwd_groups"""
    rows, G = max(vocab, T + 5), 1024 // d
    while G > 1 and G * rows * d * 4 > 96 * 1024:
        G //= 2
    return G


# (3,4,7,64) / (3,8,5,64): forward blocks hold spb = 4 / 2 sequences, n_seq = 21 / 15 leaves a short last block;
# (3,16,7,192) / (2,32,5,64): the backward loads ids per row (no lane shuffles).  prod: B N above 256 blocks x G groups,
# so every backward block walks several groups of sequences and the last trip is ragged
EMB = [(3, 4, 7, 64), (3, 8, 5, 64), (3, 16, 7, 192), (2, 32, 5, 64),
       pytest.param(17, 16, 61, 256, id="prod-d256"), pytest.param(7, 8, 331, 64, id="prod-d64"),
       pytest.param(3, 4, 97, 1024, id="prod-d1024"), pytest.param(5, 32, 211, 128, id="prod-d128")]


@pytest.mark.parametrize("B,T,N,d", EMB)
def test_embedding(H, dev, B, T, N, d):
    """vlg_embed_fwd / _bwd with vocab 30 (the reserved id 29 in every frame) against oracle.embed in fp64.  Forward: the
    class-table gather alone (other tables zero) bitwise; the full sum within 8 EPS of the sum of |terms|.  Backward: two
    launches give the same slab bits, every slab's L floats are written and its stride padding is not; after
    vlg_reduce_slabs each table gradient is within (sequences per group x T + G + slabs + 1) EPS sum |terms| of fp64."""
    lib = H.load()
    vocab = 30
    g = torch.Generator().manual_seed(B * T * N + d)
    p = {"cls_emb": torch.randn(vocab, d, generator=g), "box_w": torch.randn(d, 4, generator=g) * 0.5,
         "box_b": torch.randn(d, generator=g) * 0.1, "time_emb": torch.randn(T, d, generator=g)}
    cls = torch.randint(0, vocab, (B, T, N), generator=g)
    cls[:, :, 0] = vocab - 1
    box = torch.rand(B, T, N, 4, generator=g)
    M = B * T * N
    pd = {k: v.to(dev) for k, v in p.items()}
    clsd, boxd = cls.to(dev), box.to(dev)
    xraw, x = _buf(M * d, dev)
    H.call("vlg_embed_fwd", clsd.data_ptr(), boxd.data_ptr(), pd["cls_emb"].data_ptr(), pd["box_w"].data_ptr(),
           pd["box_b"].data_ptr(), pd["time_emb"].data_ptr(), x.data_ptr(), B, T, N, d, vocab, S())
    zeros = torch.zeros(d * 4 + d + T * d, device=dev)
    graw, xg = _buf(M * d, dev)
    H.call("vlg_embed_fwd", clsd.data_ptr(), boxd.data_ptr(), pd["cls_emb"].data_ptr(), zeros.data_ptr(),
           zeros[d * 4:].data_ptr(), zeros[d * 5:].data_ptr(), xg.data_ptr(), B, T, N, d, vocab, S())
    torch.cuda.synchronize()
    _guard(xraw, M * d, "embed fwd")
    _guard(graw, M * d, "embed fwd (gather)")
    assert torch.equal(_from_rows(xg.cpu(), B, T, N), p["cls_emb"][cls]), "class-table gather is not exact"
    want = O.embed({k: v.double() for k, v in p.items()}, cls, box.double())
    terms = (p["cls_emb"][cls].double().abs() + box.double().abs() @ p["box_w"].double().abs().t() +
             p["box_b"].double().abs() + p["time_emb"].double().abs()[None, :, None, :])
    within(_from_rows(x.cpu(), B, T, N), want, 8 * EPS * terms, "embed fwd")

    dx = torch.randn(B, T, N, d, generator=g)
    dxd = _to_rows(dx).to(dev)
    L = vocab * d + d * 4 + d + T * d
    stride = L + 4
    ns = lib.vlg_embed_bwd_slabs_for(B, T, N, d, vocab)
    runs = []
    for _ in range(2):
        sraw, slabs = _buf(ns * stride, dev)
        H.call("vlg_embed_bwd", dxd.data_ptr(), clsd.data_ptr(), boxd.data_ptr(), slabs.data_ptr(), stride, ns * stride,
               B, T, N, d, vocab, S())
        torch.cuda.synchronize()
        runs.append(sraw)
    assert torch.equal(runs[0], runs[1]), "two backward launches differ"
    owned = torch.zeros(ns * stride + GUARD, dtype=torch.bool, device=dev)
    owned[:ns * stride].view(ns, stride)[:, :L] = True
    untouched(runs[0], owned, "embed bwd slabs")
    gt = torch.empty(L, device=dev)
    H.call("vlg_reduce_slabs", f32(runs[0]).data_ptr(), stride, ns, gt.data_ptr(), L, S())
    torch.cuda.synchronize()
    gt = gt.cpu()
    d2 = dx.double().reshape(-1, d)
    bx = box.double().reshape(-1, 4)
    ids = cls.reshape(-1)
    want = {"cls_emb": torch.zeros(vocab, d, dtype=torch.float64).index_add_(0, ids, d2), "box_w": d2.t() @ bx,
            "box_b": d2.sum(0), "time_emb": dx.double().sum((0, 2))}
    mag = {"cls_emb": torch.zeros(vocab, d, dtype=torch.float64).index_add_(0, ids, d2.abs()), "box_w": d2.abs().t() @ bx.abs(),
           "box_b": d2.abs().sum(0), "time_emb": dx.double().abs().sum((0, 2))}
    G = _embed_groups(T, d, vocab)
    cr = -(-(B * N) // (ns * G)) * T + G + ns + 1
    o = 0
    for name in ("cls_emb", "box_w", "box_b", "time_emb"):
        k = want[name].numel()
        within(gt[o:o + k].view(want[name].shape), want[name], cr * EPS * mag[name], "embed d" + name)
        o += k


# ------------------------------------------------------------------------------------------------ layout loss
def _loss_rows(t):
    B, T, N, C = t.shape
    return t.permute(0, 2, 1, 3).contiguous().view(B * T * N, C)


def _loss_run(H, dev, logits, raw, batch, ld, scratch, beta):
    """vlg_layout_loss on head outputs with a row stride ld (padding columns hold the sentinel); returns the four loss
    values, dout's 24 owned columns and dout's raw bits, after checking that nothing else was written."""
    B, T, N = logits.shape[:3]
    M = B * T * N
    oraw = sentinel(M * ld + GUARD, dev)
    f32(oraw)[:M * ld].view(M, ld)[:, :24] = torch.cat([_loss_rows(logits), _loss_rows(raw)], 1).to(dev)
    draw = sentinel(M * ld + GUARD, dev)
    lraw = sentinel(4 + GUARD, dev)
    tc, tb, va = batch["tgt_class"].to(dev), batch["tgt_box"].to(dev), batch["valid"].to(dev)
    H.call("vlg_layout_loss", f32(oraw).data_ptr(), ld, tc.data_ptr(), tb.data_ptr(), va.data_ptr(), f32(draw).data_ptr(),
           f32(lraw).data_ptr(), f32(scratch).data_ptr(), B, T, N, 20, beta, O.IOU_EPS, O.W_REG, O.W_IOU, O.W_CE, S())
    torch.cuda.synchronize()
    owned = torch.zeros(M * ld + GUARD, dtype=torch.bool, device=dev)
    owned[:M * ld].view(M, ld)[:, :24] = True
    untouched(draw, owned, "loss dout")
    _guard(lraw, 4, "loss values")
    _guard(scratch, H.load().vlg_layout_loss_scratch(), "loss scratch")
    assert int(scratch[1]) == 0, "the ticket counter was not reset for the next launch"
    return f32(lraw)[:4].cpu(), f32(draw)[:M * ld].view(M, ld)[:, :24].cpu(), draw


def _scratch(H, dev):
    n = H.load().vlg_layout_loss_scratch()
    s = sentinel(n + GUARD, dev)
    s[:n] = 0
    return s


def _loss_check(loss, dout, logits, raw, batch):
    """Gradients: per block of columns (class logits, box outputs), 4x torch-CPU fp32's error plus 2^-20 of the largest
    value.  Values: 4x torch-CPU fp32's error plus 64 EPS of the summed magnitudes / count (per token |term| + 1, and the
    largest |logit| for the cross entropy, which log-sum-exp subtracts and adds back)."""
    ref = {}
    for dt in (torch.float64, torch.float32):
        lg, rw = (t.detach().to(dt, copy=True).requires_grad_(True) for t in (logits, raw))
        parts = O.losses(lg, rw, batch["tgt_class"], batch["tgt_box"].to(dt), batch["valid"].to(dt))
        parts[0].backward()
        ref[dt] = (torch.stack([t.detach() for t in parts]), torch.cat([_loss_rows(lg.grad), _loss_rows(rw.grad)], 1))
    (v64, g64), (v32, g32) = ref[torch.float64], ref[torch.float32]
    vs_cpu32(dout[:, :20], g64[:, :20], g32[:, :20], "loss d logits")
    vs_cpu32(dout[:, 20:], g64[:, 20:], g32[:, 20:], "loss d box")
    lg, tb, va = logits.double(), batch["tgt_box"].double(), batch["valid"].double()
    box = torch.sigmoid(raw.double())
    reg = F.smooth_l1_loss(box, tb, beta=O.SMOOTH_L1_BETA, reduction="none").sum(-1) / 4
    iou = 1 - O.box_iou_cxcywh(box, tb)
    ce = F.cross_entropy(lg.reshape(-1, 20), batch["tgt_class"].reshape(-1), reduction="none").view(va.shape)
    cnt = float(va.sum().clamp(min=1))
    fl = [64 * EPS * float(((t.abs() + 1 + extra) * va).sum()) / cnt
          for t, extra in ((reg, 0), (iou, 0), (ce, lg.abs().amax(-1)))]
    floors = torch.tensor([O.W_REG * fl[0] + O.W_IOU * fl[1] + O.W_CE * fl[2]] + fl, dtype=torch.float64)
    within(loss, v64, 4 * (v32.double() - v64).abs() + floors, "loss values (total, smooth-L1, IoU, CE)")


@pytest.mark.parametrize("B,T,N", [pytest.param(5, 32, 821, id="prod")])
def test_layout_loss_prod(H, dev, B, T, N):
    """M = 131 360 tokens: above 1024 blocks x 128 tokens (a second pass for 2 blocks, 32 tokens in the last group), row
    stride ld = 28 with the padding columns of out and dout holding the sentinel, variable-N validity; a second launch on
    the same scratch buffer gives the same bits (the last block resets the ticket)."""
    batch = O.synthetic_batch(B, T, N, seed=5, variable_n=True, min_valid=100)
    g = torch.Generator().manual_seed(55)
    logits = torch.randn(B, T, N, 20, generator=g) * 3
    raw = torch.randn(B, T, N, 4, generator=g) * 2
    sc = _scratch(H, dev)
    loss, dout, bits = _loss_run(H, dev, logits, raw, batch, 28, sc, O.SMOOTH_L1_BETA)
    loss2, _, bits2 = _loss_run(H, dev, logits, raw, batch, 28, sc, O.SMOOTH_L1_BETA)
    assert torch.equal(bits, bits2) and torch.equal(loss, loss2), "a second launch on the same scratch differs"
    _loss_check(loss, dout, logits, raw, batch)


def _edge_batch(B, T, N, seed):
    g = torch.Generator().manual_seed(seed)
    batch = O.synthetic_batch(B, T, N, seed=seed)
    logits = torch.randn(B, T, N, 20, generator=g) * 2
    raw = torch.randn(B, T, N, 4, generator=g)
    logits[:, :, 0] = torch.where(torch.rand(B, T, 20, generator=g) > 0.5, 80.0, -80.0)    # logits at +-80
    logits[:, :, 1] = 7.0                                                                  # all logits equal
    raw[:, :, 2] = torch.tensor([30.0, -30.0, 30.0, -30.0])                                # saturated sigmoid
    # raw = 0: p = (0.5, 0.5, 0.5, 0.5) exactly in fp32 and fp64, the box [0.25, 0.75]^2; targets of exact binary fractions
    raw[:, :, 3:10] = 0.0
    tb = batch["tgt_box"]
    tb[:, :, 3] = torch.tensor([0.5, 0.5, 0.5, 0.5])          # prediction = target: every min / max of the IoU ties
    tb[:, :, 4] = torch.tensor([1.0, 0.5, 0.5, 0.5])          # touching in x (bx1 = ax2 = 0.75): iw_raw = 0
    tb[:, :, 5] = torch.tensor([0.5, 0.0, 0.5, 0.5])          # touching in y (by2 = ay1 = 0.25): ih_raw = 0
    tb[:, :, 6] = torch.tensor([0.875, 0.875, 0.125, 0.125])  # disjoint
    tb[:, :, 7] = torch.tensor([0.375, 0.625, 0.5, 0.375])    # |p - t| = beta (0.125) in cx, cy, h; w ties
    tb[:, :, 8] = torch.tensor([0.625, 0.5, 0.25, 0.5])       # right edges tie, y edges tie
    tb[:, :, 9] = torch.tensor([0.5, 0.5, 0.75, 0.25])        # overlapping, no edge ties
    return logits, raw, batch


def test_layout_loss_edges(H, dev, monkeypatch):
    """Logits at +-80 and all equal, raw = +-30, and (with raw = 0, so p = 0.5 exactly) a prediction equal to its target
    (the 0.5 split of the min / max subgradients), touching boxes (clamp at iw_raw = 0 passes the gradient, as torch's),
    disjoint boxes and |p - t| exactly at the smooth-L1 switch.  beta = 0.125 here (passed to the kernel and set in the
    oracle) so that the switch point is exact in both precisions."""
    monkeypatch.setattr(O, "SMOOTH_L1_BETA", 0.125)
    logits, raw, batch = _edge_batch(3, 4, 12, seed=9)
    loss, dout, _ = _loss_run(H, dev, logits, raw, batch, 24, _scratch(H, dev), 0.125)
    _loss_check(loss, dout, logits, raw, batch)


def test_layout_loss_single_valid_slot(H, dev, monkeypatch):
    """One valid slot (a tied box, raw = 0): the mean is that slot's terms, every other gradient row exactly 0."""
    monkeypatch.setattr(O, "SMOOTH_L1_BETA", 0.125)
    logits, raw, batch = _edge_batch(2, 8, 12, seed=10)
    batch["valid"].zero_()
    batch["valid"][1, 5, 8] = 1.0
    loss, dout, _ = _loss_run(H, dev, logits, raw, batch, 24, _scratch(H, dev), 0.125)
    _loss_check(loss, dout, logits, raw, batch)
    live = torch.zeros(2, 8, 12, 1, dtype=torch.bool)
    live[1, 5, 8] = True
    assert bool((dout[~_loss_rows(live)[:, 0]] == 0).all()), "a masked slot has a gradient"


# ------------------------------------------------------------------------------------------------ reduce and Adam
@pytest.mark.parametrize("n_slabs", [16, 47, 48, 49, 64, 512])
def test_reduce_slabs_tall(H, dev, n_slabs):
    """The tall path (fewer than 32 768 float4 columns, >= 16 slabs): 16 slab groups per column, 4 loads per lane while
    s + 48 < n_slabs, then the rest one at a time.  341 float4 columns (a ragged last block of 16), a stride with NaN
    padding the kernel must not read.  Bar: (ceil(n / 16) + 16) EPS sum |terms| (the serial adds, then the 16-way sum)."""
    length = 4 * (16 * 21 + 5)
    stride = length + 12
    g = torch.Generator().manual_seed(n_slabs)
    s = torch.randn(n_slabs, stride, generator=g)
    s[:, length:] = NAN
    sd = s.to(dev)
    raw, dst = _buf(length, dev)
    H.call("vlg_reduce_slabs", sd.data_ptr(), stride, n_slabs, dst.data_ptr(), length, S())
    torch.cuda.synchronize()
    _guard(raw, length, "reduce_slabs (tall)")
    v = s[:, :length].double()
    within(dst, v.sum(0), (-(-n_slabs // 16) + 16) * EPS * v.abs().sum(0), "tall reduction of %d slabs" % n_slabs)


@pytest.mark.parametrize("length,n_slabs", [pytest.param(2097152 + 4 * 37, 5, id="prod")])
def test_reduce_slabs_flat(H, dev, length, n_slabs):
    """The flat path above its 2048-block cap (2 097 152 floats per trip): a second trip with 37 float4 of it.  Bar:
    (n_slabs + 1) EPS sum |terms|."""
    stride = length + 8
    g = torch.Generator().manual_seed(3)
    s = torch.randn(n_slabs, stride, generator=g)
    s[:, length:] = NAN
    sd = s.to(dev)
    raw, dst = _buf(length, dev)
    H.call("vlg_reduce_slabs", sd.data_ptr(), stride, n_slabs, dst.data_ptr(), length, S())
    torch.cuda.synchronize()
    _guard(raw, length, "reduce_slabs (flat)")
    v = s[:, :length].double()
    within(dst, v.sum(0), (n_slabs + 1) * EPS * v.abs().sum(0), "flat reduction")


@pytest.mark.parametrize("step", [pytest.param(1, id="prod-step1"), pytest.param(1000, id="prod-step1000")])
def test_adam_prod(H, dev, step):
    """vlg_adam_step and vlg_adam_step_bf16 on n = 2 101 156 parameters (above the 2048-block cap of 2 097 152) with
    grad_scale 0.3, against Adam in fp64 (oracle.adam_step) on the same fp32 state with the fp32 hyper-parameters the
    kernel receives.  Bars, first order with doubled constants: m within 8 EPS (|m| + |g|), v within 16 EPS (|v| + (1 -
    beta2) g^2), params within 2 (step_size dm / denom + 12 EPS |update| + EPS |p|).  The bf16 variant leaves p, m, v
    bitwise those of vlg_adam_step, and its shadow is the round-to-nearest-even bf16 of the new p; nothing past n."""
    n = 2097152 + 4 * 1001
    lr, b1, b2, eps, gs = (float(np.float32(v)) for v in (2e-4, 0.5, 0.999, 1e-8, 0.3))
    g = torch.Generator().manual_seed(step)
    p = torch.randn(n, generator=g)
    grad = torch.randn(n, generator=g) * torch.pow(10.0, torch.rand(n, generator=g) * 4 - 3)
    grad[::97] = 0
    if step == 1:
        m, v = torch.zeros(n), torch.zeros(n)
    else:
        m, v = torch.randn(n, generator=g) * 0.1, torch.rand(n, generator=g) * 0.01
    outs = []
    for name in ("vlg_adam_step", "vlg_adam_step_bf16"):
        bufs = []
        for t in (p, m, v):
            raw = sentinel(n + GUARD, dev)
            f32(raw)[:n] = t.to(dev)
            bufs.append(raw)
        gd = grad.to(dev)
        sh = torch.full((n + GUARD,), SENT16, dtype=torch.int16, device=dev)
        ptrs = [f32(b).data_ptr() for b in bufs]
        args = [ptrs[0], gd.data_ptr(), ptrs[1], ptrs[2]] + ([sh.data_ptr()] if name.endswith("bf16") else [])
        H.call(name, *args, n, step, lr, b1, b2, eps, gs, S())
        torch.cuda.synchronize()
        for b, what in zip(bufs, ("p", "m", "v")):
            _guard(b, n, name + " " + what)
        outs.append(([f32(b)[:n].cpu() for b in bufs], sh))
    (p1, m1, v1), _ = outs[0]
    (p2, m2, v2), sh = outs[1]
    assert torch.equal(p1, p2) and torch.equal(m1, m2) and torch.equal(v1, v2), "the bf16 variant changed the fp32 update"
    assert torch.equal(sh[:n].cpu(), p1.to(BF).view(torch.int16)), "bf16 shadow is not the RNE of the new parameter"
    _guard(sh, n, "vlg_adam_step_bf16 shadow")
    p64, m64, v64 = p.double(), m.double(), v.double()
    gk = grad.double() * gs
    O.adam_step(p64, gk, m64, v64, step, lr=lr, beta1=b1, beta2=b2, eps=eps)
    within(m1, m64, 8 * EPS * (m.double().abs() + gk.abs()), "adam m")
    within(v1, v64, 16 * EPS * (v.double().abs() + (1 - b2) * gk * gk), "adam v")
    step_size = lr / (1 - b1 ** step)
    denom = v64.sqrt() / math.sqrt(1 - b2 ** step) + eps
    upd = step_size * m64 / denom
    dm = 8 * EPS * (m.double().abs() + gk.abs())
    within(p1, p64, 2 * (step_size * dm / denom + 12 * EPS * upd.abs() + EPS * p64.abs()), "adam params")
