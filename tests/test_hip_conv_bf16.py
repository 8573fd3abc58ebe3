"""GPU: the bf16-MFMA convolutions vlg_conv3x3_{fwd,dgrad,wgrad}_bf16 (csrc/conv_bf16.hip) one at a time through the C ABI.

The contract they implement: fp32 tensors; act(x) (PReLU on channels < act_ch) computed in fp32, then the two GEMM operands
rounded to bf16 (RNE); fp32 accumulation; the epilogues of the fp32 path on the fp32 accumulator.  So the reference here is
fp64 torch on the bf16-ROUNDED operands (x -> act in fp32 -> bf16, W -> bf16, dOut -> bf16), followed by the fp32 path's
epilogue (bias, residual, mask, PReLU' and the slope gradient on the fp32 input, the bias gradient from the fp32 dOut).
Against it the kernels agree to 1e-5 of each tensor's scale (fp32 accumulation order is all that remains).  Against the
UNROUNDED fp64 result the error is at least 10x larger: the operands really are rounded to bf16, to nearest even (a
truncating conversion would agree with neither).  Every output lives in a NaN-sentinel buffer: each element the kernel
owns is written and finite, halo rows are zero, guard rows, padding lanes and slab tails come back untouched."""
import pytest
import torch
import torch.nn.functional as F

from test_hip_conv_ops import CASES, _away_from_kink, _Harness

pytestmark = pytest.mark.gpu

TOL = 1e-5
DISCRIMINATE = 10.0
NAN = float("nan")


def _bf(t):
    return t.float().to(torch.bfloat16).double()


def _ref(x, w, bias, slope, act, stride, resid, r, rounded):
    """fp64 on (rounded or unrounded) operands + the fp32 path's epilogues: y, dx, slope gradient, its scale, dW, db."""
    x32 = x.float()
    xa32 = x32 if slope is None else torch.cat([F.prelu(x32[:, :act], torch.tensor([slope], dtype=torch.float32)),
                                                x32[:, act:]], dim=1)
    q = _bf if rounded else (lambda t: t.double())
    xa, wq, rq = q(xa32), q(w), q(r)
    y = F.conv2d(xa, wq, bias.double(), stride=stride, padding=1)
    if resid is not None:
        y = y + resid.double()
    dxa = torch.nn.grad.conv2d_input(tuple(x.shape), wq, rq, stride=stride, padding=1)
    dx = dxa.clone()
    dx[:, act:] = 0                                            # constant (AddCoords) channels pass no gradient on
    da = da_scale = None
    if slope is not None:
        xd = x32.double()[:, :act]
        neg = ~(xd > 0)
        s32 = float(torch.tensor(slope, dtype=torch.float32))
        dx[:, :act] = torch.where(neg, dxa[:, :act] * s32, dxa[:, :act])
        terms = dxa[:, :act] * xd
        da = float(terms[neg].sum())
        da_scale = float(terms.abs()[neg].sum())
    dw = torch.nn.grad.conv2d_weight(xa, tuple(w.shape), rq, stride=stride, padding=1)
    db = r.double().sum((0, 2, 3))
    return y, dx, da, da_scale, dw, db


def _err(got, want):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-12)


def _check(what, got, want_rounded, want_plain, tol=TOL):
    e = _err(got, want_rounded)
    e_plain = _err(got, want_plain)
    print("BF16ERR %-10s rounded %.3e  unrounded %.3e" % (what, e, e_plain))
    assert e <= tol, "%s: %.3e of scale against the bf16-operand reference (bar %.0e)" % (what, e, tol)
    assert e_plain >= DISCRIMINATE * max(e, 1e-9), "%s: %.3e vs unrounded is not >> %.3e: operands not rounded to bf16?" % (
        what, e_plain, e)


def _padded_view(h, pt, geo):
    """(b, H+2, W+2, cp) view of the rows of pt, and the guard bands before / after them"""
    n0, n1 = geo.guard * pt.cp, (geo.guard + geo.rows) * pt.cp
    return pt.buf[n0:n1].view(geo.b, geo.H + 2, geo.W + 2, pt.cp), pt.buf[:n0], pt.buf[n1:]


def _sentinel_checks(what, h, pt, geo, C, pad_untouched):
    v, g0, g1 = _padded_view(h, pt, geo)
    v = v.cpu()
    assert bool(torch.isnan(g0).all()) and bool(torch.isnan(g1).all()), what + ": guard rows were written"
    assert bool(torch.isfinite(v[:, 1:-1, 1:-1, :C]).all()), what + ": an interior element is unwritten or not finite"
    for halo in (v[:, 0, :, :C], v[:, -1, :, :C], v[:, :, 0, :C], v[:, :, -1, :C]):
        assert float(halo.abs().max()) == 0.0, what + ": halo rows are not zero"
    if pad_untouched and C < pt.cp:
        assert bool(torch.isnan(v[..., C:]).all()), what + ": padding lanes were written"


def _run_case(dev, b, H, W, cin, cout, stride, act_ch, resid, slope, ws_fwd=False, ws_dgrad=False, accumulate=False):
    from vlg import hip
    from vlg.hip import CEPI_ACCUM, CEPI_DPRELU, CEPI_RESID
    lib = hip.load()
    g = torch.Generator().manual_seed(1000 * cin + 10 * cout + stride + 7)
    h = _Harness(dev, b, H, W, cin, cout, stride)
    act = cin if act_ch is None else act_ch
    x = _away_from_kink((b, cin, H, W), g)
    w = (torch.rand(cout, cin, 3, 3, generator=g) * 2 - 1) / (cin * 9) ** 0.5
    bias = (torch.rand(cout, generator=g) * 2 - 1) * 0.1
    Ho, Wo = H // stride, W // stride
    r = torch.randn(b, cout, Ho, Wo, generator=g)
    rs = torch.randn(b, cout, Ho, Wo, generator=g) if resid else None
    prior = torch.randn(b, cin, H, W, generator=g) if accumulate else None
    want = _ref(x, w, bias, slope, act, stride, rs, r, True)
    plain = _ref(x, w, bias, slope, act, stride, rs, r, False)
    S = h.S
    h.put(x, h.x, cin, h.gi)
    h.put(r, h.dy, cout, h.go)
    if resid:
        h.put(rs, h.res, cout, h.go)
    wdev = h.pack_weight(w)
    bdev = torch.zeros(h.cout_p, device=dev)
    bdev[:cout] = bias.to(dev)
    sl = None if slope is None else torch.tensor([slope, 0, 0, 0], dtype=torch.float32, device=dev)
    slp = 0 if sl is None else sl.data_ptr()
    act_arg = h.cin_p if act_ch is None else act_ch
    rowtab = h.gi.down_rowtab.data_ptr() if stride == 2 else 0
    # ---- forward, into a NaN-sentinel output
    wsn = lib.vlg_conv3x3_fwd_bf16_workspace(h.go.rows, h.cin_p, cout, h.cout_p) if ws_fwd else 0
    ws = torch.full((wsn,), NAN, device=dev) if wsn else None
    h.y.buf.fill_(NAN)
    hip.call("vlg_conv3x3_fwd_bf16", h.x.ptr, wdev.data_ptr(), bdev.data_ptr(), h.y.ptr, h.res.ptr if resid else 0,
             h.go.mask.data_ptr(), slp, rowtab, h.go.rows, h.cin_p, cout, h.cout_p, h.gi.wp, act_arg,
             CEPI_RESID if resid else 0, hip.ptr(ws), wsn, S)
    torch.cuda.synchronize()
    _sentinel_checks("forward", h, h.y, h.go, cout, True)
    _check("forward", h.get(h.y, cout, h.go), want[0], plain[0])
    # ---- data gradient (+ PReLU' and the slope-gradient partials; or split-K through a workspace)
    split = ws_dgrad
    n_da = lib.vlg_conv3x3_dgrad_bf16_slabs(h.gi.rows, h.cin_p)
    use_da = sl is not None and not split
    da_part = torch.zeros(n_da + 8, device=dev)
    dwsn = lib.vlg_conv3x3_dgrad_bf16_workspace(h.gi.rows, h.cin_p, h.cout_p) if split else 0
    dws = torch.full((dwsn,), NAN, device=dev) if dwsn else None
    taps = h.gi.down_taptabs.data_ptr() if stride == 2 else 0
    if accumulate:
        h.put(prior, h.dx, cin, h.gi)
    else:
        h.dx.buf.fill_(NAN)
    epi = (CEPI_DPRELU if sl is not None else 0) | (CEPI_ACCUM if accumulate else 0)
    hip.call("vlg_conv3x3_dgrad_bf16", h.dy.ptr, wdev.data_ptr(), h.dx.ptr, h.x.ptr, h.gi.mask.data_ptr(), slp,
             da_part.data_ptr() if use_da else 0, taps, h.gi.rows if stride == 2 else 0, h.gi.rows, h.cin_p,
             h.cout_p, h.gi.wp, act_arg, epi, hip.ptr(dws), dwsn, n_da, S)
    torch.cuda.synchronize()
    if not accumulate:
        _sentinel_checks("dx", h, h.dx, h.gi, cin, False)
    add = prior.double() if accumulate else 0
    _check("dx", h.get(h.dx, cin, h.gi), want[1] + add, plain[1] + add)
    if use_da:
        da = torch.zeros(4, device=dev)
        hip.call("vlg_sum_partials", da_part.data_ptr(), n_da, da.data_ptr(), 0, S)
        e = abs(float(da[0]) - want[2]) / max(want[3], 1e-12)
        print("BF16ERR %-10s rounded %.3e  unrounded %.3e" % ("slope", e, abs(float(da[0]) - plain[2]) / max(plain[3], 1e-12)))
        assert e <= TOL, ("slope gradient", float(da[0]), want[2], want[3])
    # ---- weight + bias gradient, into NaN-sentinel slabs with a tail behind each slab and a spare slab
    n_slabs = lib.vlg_conv3x3_wgrad_bf16_slabs(h.go.rows, h.cin_p, h.cout_p)
    need = h.cout_p * 9 * h.cin_p + h.cout_p
    stride_f = need + 4
    slabs = torch.full(((n_slabs + 1) * stride_f,), NAN, device=dev)
    hip.call("vlg_conv3x3_wgrad_bf16", h.dy.ptr, h.x.ptr, slabs.data_ptr(), stride_f, n_slabs * stride_f, rowtab, slp,
             h.go.rows, h.cin_p, h.cout_p, h.gi.wp, act_arg, S)
    torch.cuda.synchronize()
    sv = slabs.cpu().view(n_slabs + 1, stride_f)
    assert bool(torch.isfinite(sv[:n_slabs, :need]).all()), "wgrad: a slab element is unwritten or not finite"
    assert bool(torch.isnan(sv[:n_slabs, need:]).all()) and bool(torch.isnan(sv[n_slabs]).all()), "wgrad wrote past its slabs"
    gw = torch.empty(stride_f, device=dev)
    hip.call("vlg_reduce_slabs", slabs.data_ptr(), stride_f, n_slabs, gw.data_ptr(), stride_f, S)
    torch.cuda.synchronize()
    _check("dW", h.unpack_weight(gw), want[4], plain[4])
    db = gw.cpu()[h.cout_p * 9 * h.cin_p:][:cout]
    e = _err(db, want[5])                                      # (from the fp32 dOut: no rounding to discriminate)
    print("BF16ERR %-10s rounded %.3e" % ("db", e))
    assert e <= TOL, ("db", e)
    full = gw.cpu()[:h.cout_p * 9 * h.cin_p].view(h.cout_p, 9, h.cin_p)
    assert float(full[cout:].abs().max() if cout < h.cout_p else 0.0) == 0.0
    return n_slabs


@pytest.mark.parametrize("b,H,W,cin,cout,stride,act_ch,resid,slope", CASES)
def test_conv3x3_bf16_fwd_dgrad_wgrad(dev, b, H, W, cin, cout, stride, act_ch, resid, slope):
    n_slabs = _run_case(dev, b, H, W, cin, cout, stride, act_ch, resid, slope)
    if (b, H, W) == (2, 40, 44):
        assert n_slabs > 1, "this case is meant to split the weight gradient over row ranges"


def test_conv3x3_bf16_dgrad_accumulates(dev):
    _run_case(dev, 2, 12, 16, 32, 64, 1, None, False, 0.25, accumulate=True)


@pytest.mark.parametrize("b,H,W,cin,cout", [(1, 16, 16, 128, 128), (2, 8, 8, 256, 256), (1, 16, 16, 128, 256),
                                           (1, 8, 8, 512, 512), (2, 4, 4, 512, 512)])
def test_conv3x3_bf16_split_k_trunks(dev, b, H, W, cin, cout):
    """Coarse levels of the frozen trunks: ReLU -> conv with the contraction cut into K ranges (forward, and the ReLU'
    data gradient the VGG term back-propagates), summed by conv.hip's finish kernels."""
    from vlg import hip
    lib = hip.load()
    h = _Harness(dev, b, H, W, cin, cout, 1)
    assert lib.vlg_conv3x3_fwd_bf16_splits(h.go.rows, h.cin_p, cout, h.cout_p) > 1
    assert lib.vlg_conv3x3_dgrad_bf16_splits(h.gi.rows, h.cin_p, h.cout_p) > 1
    _run_case(dev, b, H, W, cin, cout, 1, None, False, 0.0, ws_fwd=True, ws_dgrad=True)


@pytest.mark.parametrize("b,H,W,cin,cout,resid", [(2, 128, 128, 128, 128, False), (2, 128, 128, 64, 128, True)])
def test_conv3x3_bf16_tail_split_shapes(dev, b, H, W, cin, cout, resid):
    """The shapes the fp32 path cuts into a tail split (265 / 529 row tiles), given a workspace as the trunks do."""
    _run_case(dev, b, H, W, cin, cout, 1, None, resid, 0.0, ws_fwd=True, ws_dgrad=True, accumulate=True)


@pytest.mark.parametrize("b,H,W,cin,cout", [(1, 16, 16, 3, 64), (2, 40, 44, 3, 64), (1, 24, 28, 4, 20)])
def test_conv3x3_bf16_image_layer_cin4(dev, b, H, W, cin, cout):
    """VLG_CEPI_CIN4 (the trunks' image layers) is accepted and computed over the 32 padded channels."""
    from vlg import hip
    from vlg.hip import CEPI_CIN4
    lib = hip.load()
    g = torch.Generator().manual_seed(31 * cin + cout + H)
    h = _Harness(dev, b, H, W, cin, cout, 1)
    x = torch.randn(b, cin, H, W, generator=g)
    w = (torch.rand(cout, cin, 3, 3, generator=g) * 2 - 1) / (cin * 9) ** 0.5
    bias = (torch.rand(cout, generator=g) * 2 - 1) * 0.1
    want = F.conv2d(_bf(x), _bf(w), bias.double(), padding=1)
    plain = F.conv2d(x.double(), w.double(), bias.double(), padding=1)
    h.put(x, h.x, cin, h.gi)
    wdev = h.pack_weight(w)
    bdev = torch.zeros(h.cout_p, device=dev)
    bdev[:cout] = bias.to(dev)
    h.y.buf.fill_(NAN)
    hip.call("vlg_conv3x3_fwd_bf16", h.x.ptr, wdev.data_ptr(), bdev.data_ptr(), h.y.ptr, 0, h.go.mask.data_ptr(), 0, 0,
             h.go.rows, h.cin_p, cout, h.cout_p, h.gi.wp, h.cin_p, CEPI_CIN4, 0, 0, h.S)
    torch.cuda.synchronize()
    _sentinel_checks("cin4", h, h.y, h.go, cout, True)
    _check("cin4", h.get(h.y, cout, h.go), want, plain)
    zero = torch.zeros(4, device=dev)                          # the fp32 entry point's refusals hold here too
    rc = lib.vlg_conv3x3_fwd_bf16(h.x.ptr, wdev.data_ptr(), bdev.data_ptr(), h.y.ptr, 0, h.go.mask.data_ptr(),
                                  zero.data_ptr(), 0, h.go.rows, h.cin_p, cout, h.cout_p, h.gi.wp, h.cin_p, CEPI_CIN4, 0, 0, h.S)
    assert rc == 1001


def test_conv3x3_bf16_nan_propagates(dev):
    """A NaN operand gives NaN in the outputs it feeds (the plain bf16 cast keeps NaN), finite values elsewhere."""
    from vlg import hip
    lib = hip.load()
    b, H, W, cin, cout = 1, 12, 16, 32, 64
    g = torch.Generator().manual_seed(5)
    h = _Harness(dev, b, H, W, cin, cout, 1)
    x = _away_from_kink((b, cin, H, W), g)
    w = (torch.rand(cout, cin, 3, 3, generator=g) * 2 - 1) / (cin * 9) ** 0.5
    w[5, 3, 1, 1] = NAN                                        # output channel 5
    r = torch.randn(b, cout, H, W, generator=g)
    r[0, 7, 6, 8] = NAN                                        # dOut at one pixel, channel 7
    h.put(x, h.x, cin, h.gi)
    h.put(r, h.dy, cout, h.go)
    wdev = h.pack_weight(w)
    S = h.S
    hip.call("vlg_conv3x3_fwd_bf16", h.x.ptr, wdev.data_ptr(), 0, h.y.ptr, 0, h.go.mask.data_ptr(), 0, 0, h.go.rows,
             h.cin_p, cout, h.cout_p, h.gi.wp, h.cin_p, 0, 0, 0, S)
    y = h.get(h.y, cout, h.go)
    assert bool(torch.isnan(y[:, 5]).all()) and bool(torch.isfinite(torch.cat([y[:, :5], y[:, 6:]], 1)).all())
    w[5, 3, 1, 1] = 0.0
    wdev = h.pack_weight(w)
    hip.call("vlg_conv3x3_dgrad_bf16", h.dy.ptr, wdev.data_ptr(), h.dx.ptr, h.x.ptr, h.gi.mask.data_ptr(), 0, 0, 0, 0,
             h.gi.rows, h.cin_p, h.cout_p, h.gi.wp, h.cin_p, 0, 0, 0, 0, S)
    dx = h.get(h.dx, cin, h.gi)
    assert bool(torch.isnan(dx[0, :, 5:8, 7:10]).all())      # the 3x3 input window behind that output pixel
    assert bool(torch.isfinite(dx[0, :, :4]).all()) and bool(torch.isfinite(dx[0, :, 9:]).all())
    n_slabs = lib.vlg_conv3x3_wgrad_bf16_slabs(h.go.rows, h.cin_p, h.cout_p)
    stride_f = h.cout_p * 9 * h.cin_p + h.cout_p
    slabs = torch.empty(n_slabs * stride_f, device=dev)
    hip.call("vlg_conv3x3_wgrad_bf16", h.dy.ptr, h.x.ptr, slabs.data_ptr(), stride_f, slabs.numel(), 0, 0, h.go.rows,
             h.cin_p, h.cout_p, h.gi.wp, h.cin_p, S)
    gw = torch.empty(stride_f, device=dev)
    hip.call("vlg_reduce_slabs", slabs.data_ptr(), stride_f, n_slabs, gw.data_ptr(), stride_f, S)
    dw = h.unpack_weight(gw)
    db = gw.cpu()[h.cout_p * 9 * h.cin_p:][:cout]
    assert bool(torch.isnan(dw[7]).all()) and bool(torch.isnan(db[7]))
    assert bool(torch.isfinite(dw[:7]).all()) and bool(torch.isfinite(db[:7]).all())


def test_conv3x3_bf16_exact_capacities_are_accepted(dev):
    """The queried workspace, slope-partial count and slab count are exactly enough: launches given exactly that run."""
    from vlg import hip
    lib = hip.load()
    b, H, W, cin, cout = 2, 8, 8, 256, 256
    h = _Harness(dev, b, H, W, cin, cout, 1)
    wdev = torch.zeros(h.cout_p * 9 * h.cin_p, device=dev)
    zero = torch.zeros(4, device=dev)
    need = lib.vlg_conv3x3_fwd_bf16_workspace(h.go.rows, h.cin_p, cout, h.cout_p)
    assert need > 0
    ws = torch.empty(need, device=dev)
    hip.call("vlg_conv3x3_fwd_bf16", h.x.ptr, wdev.data_ptr(), 0, h.y.ptr, 0, h.go.mask.data_ptr(), zero.data_ptr(), 0,
             h.go.rows, h.cin_p, cout, h.cout_p, h.gi.wp, h.cin_p, 0, ws.data_ptr(), need, h.S)
    dneed = lib.vlg_conv3x3_dgrad_bf16_workspace(h.gi.rows, h.cin_p, h.cout_p)
    dws = torch.empty(dneed, device=dev)
    hip.call("vlg_conv3x3_dgrad_bf16", h.dy.ptr, wdev.data_ptr(), h.dx.ptr, h.x.ptr, h.gi.mask.data_ptr(), zero.data_ptr(),
             0, 0, 0, h.gi.rows, h.cin_p, h.cout_p, h.gi.wp, h.cin_p, 0, dws.data_ptr(), dneed, 0, h.S)
    n_da = lib.vlg_conv3x3_dgrad_bf16_slabs(h.gi.rows, h.cin_p)
    da = torch.empty(n_da, device=dev)
    hip.call("vlg_conv3x3_dgrad_bf16", h.dy.ptr, wdev.data_ptr(), h.dx.ptr, h.x.ptr, h.gi.mask.data_ptr(), zero.data_ptr(),
             da.data_ptr(), 0, 0, h.gi.rows, h.cin_p, h.cout_p, h.gi.wp, h.cin_p, 8, 0, 0, n_da, h.S)
    n_slabs = lib.vlg_conv3x3_wgrad_bf16_slabs(h.go.rows, h.cin_p, h.cout_p)
    stride_f = h.cout_p * 9 * h.cin_p + h.cout_p
    slabs = torch.empty(n_slabs * stride_f, device=dev)
    hip.call("vlg_conv3x3_wgrad_bf16", h.dy.ptr, h.x.ptr, slabs.data_ptr(), stride_f, n_slabs * stride_f, 0, zero.data_ptr(),
             h.go.rows, h.cin_p, h.cout_p, h.gi.wp, h.cin_p, h.S)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(da).all()) and bool(torch.isfinite(slabs).all())
