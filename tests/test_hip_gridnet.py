"""GPU: the reference's trainable model (GridNet / CoordGridNet, reference src/models/gridnet.py,
src/models/modules.py) on the implicit-GEMM convolution kernels - TRUE parity: expected values were
produced by the reference modules themselves (tests/golden/gridnet_*.npz, coordgridnet_256.npz, written
by oracle/make_golden.py); the CPU restatement oracle/gridnet_spec.py (bit-identical to the reference on
those fixtures, tests/test_oracle_golden.py) covers extra shapes.  fp32, tolerance 1e-4."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN
from helpers import check_close
from oracle import gridnet_spec as G

pytestmark = pytest.mark.gpu


def rel_close(got, want, tol=1e-4, what=""):
    scale = max(float(want.abs().max()), 1e-12)
    check_close(got.cpu() / scale, want / scale, rtol=tol, atol=tol * 0.2, what=what)


def kink_tolerant(got, want, what):
    """Gradients of a PReLU network with REAL slopes: a pre-activation inside the fp32 rounding band of its kink
    flips the local derivative between 1 and the slope, which moves downstream gradient sums by ~1e-3 of
    their scale (oracle.gridnet_spec.test_params docstring).  Bound: 2e-2 of the tensor's max, 5e-3 in L2."""
    got, want = got.detach().cpu().double(), want.double()
    scale = max(float(want.abs().max()), 1e-12)
    assert float((got - want).abs().max()) <= 2e-2 * scale, what
    assert float((got - want).norm()) <= 5e-3 * max(float(want.norm()), 1e-12), what


def branch_pattern(net, p, x, coord, band=1e-5):
    """The PReLU branch pattern of the HIP forward ({key: x > 0}), checked against the CPU restatement's own: the two
    may disagree ONLY on elements whose pre-activation lies within `band` x (tensor scale) of the kink, i.e. inside the
    forward pass's fp32 rounding band - anything else is a forward error.  Returns (pattern, number of disagreements)."""
    positive = {k: (v > 0).cpu() for k, v in net.prelu_inputs().items()}
    rec = {}
    with torch.no_grad():
        G.forward(p, x, coord, branches=G.Branches(record=rec))
    assert set(rec) == set(positive)
    flips = 0
    for k, v in rec.items():
        diff = (v > 0) != positive[k]
        if bool(diff.any()):
            worst = float(v[diff].abs().max())
            assert worst <= band * float(v.abs().max()), ("branch of %s differs %.3e away from the kink" % (k, worst))
            flips += int(diff.sum())
    return positive, flips


def strict_given_branches(net, dx, p, x, r_seg, r_img, coord, tol=1e-4):
    """REAL slopes, strict bound: the backward pass of a PReLU network is smooth once every element's branch is fixed,
    so with the CPU restatement evaluated (in fp64) on the branch pattern the HIP forward actually took, every
    gradient - dx, every weight / bias tensor, every slope gradient - must agree to `tol`; the pattern itself is held
    to the restatement's by branch_pattern().  Together with the 1e-4 forward check this is parity with no
    kink allowance: a sign, indexing or slope-selection slip in the dPReLU epilogue, the act_ch cut-off or the slope
    partials fails here."""
    positive, flips = branch_pattern(net, p, x, coord)
    p64 = {k: v.double() for k, v in p.items()}
    _, _, grads_w, dx_w = G.forward_backward(p64, x.double(), r_seg.double(), r_img.double(), coord,
                                             branches=G.Branches(positive=positive))
    rel_close(dx, dx_w, tol=tol, what="dx (branches pinned)")
    check_grads(net.named_grads(), grads_w, True, tol=tol)
    return flips


def check_grads(grads, want, linear, tol=1e-4):
    """All parameter gradients.  Tensors: rel_close (smooth net) / kink_tolerant (real slopes).  PReLU-slope
    gradients are single numbers - cancelling sums over every activation of a layer - so they are compared on
    the scale of the largest slope gradient in the network, not each on its own magnitude."""
    smax = max(float(w.abs().max()) for w in want.values() if w.numel() == 1)
    for k, w in want.items():
        if w.numel() == 1:
            bound = (tol if linear else 2e-2) * max(abs(float(w)), 0.05 * smax)
            assert abs(float(grads[k]) - float(w)) <= bound, ("slope grad " + k, float(grads[k]), float(w))
        elif linear:
            rel_close(grads[k], w, tol=tol, what="grad " + k)
        else:
            kink_tolerant(grads[k], w, what="grad " + k)


def run_case(dev, z, filters, b, H, W, seed, x, coord, tag, linear):
    from vlg.gridnet import GridNetHIP
    net = GridNetHIP(10, b, H, W, dev, coord=coord, filters=filters, need_input_grad=True)
    shapes = G.param_shapes(10, filters, coord=coord)
    ref_shapes = net.reference_shapes()
    assert set(shapes) == set(ref_shapes) and all(tuple(ref_shapes[k]) == tuple(v) for k, v in shapes.items())
    p = G.test_params(shapes, seed=seed, linear=linear)
    net.load_state_dict(p)
    back = net.state_dict()                                   # layout conversion round-trips exactly
    assert all(torch.equal(back[k], p[k]) for k in p)
    seg, img = net.forward(x.to(dev))
    return net, seg, img


@pytest.mark.parametrize("linear", [False, True])
def test_gridnet_small_matches_reference_everywhere(dev, linear):
    z = np.load(os.path.join(GOLDEN, "gridnet_small.npz"))
    tag = "lin_" if linear else ""
    net, seg, img = run_case(dev, z, (8, 16, 24), 2, 32, 48, 1, torch.from_numpy(z["x"]), False, tag, linear)
    rel_close(seg, torch.from_numpy(z[tag + "seg"]), what="seg")
    rel_close(img, torch.from_numpy(z[tag + "img"]), what="img")
    dx = net.backward(torch.from_numpy(z["r_seg"]).to(dev), torch.from_numpy(z["r_img"]).to(dev))
    check = rel_close if linear else kink_tolerant
    check(dx, torch.from_numpy(z[tag + "dx"]), what="dx")
    grads = net.named_grads()
    assert set(tag + "grad:" + k for k in grads) == set(k for k in z.files if k.startswith(tag + "grad:"))
    check_grads(grads, {k: torch.from_numpy(z[tag + "grad:" + k]) for k in grads}, linear)
    if not linear:
        p = G.test_params(G.param_shapes(10, (8, 16, 24)), seed=1)
        strict_given_branches(net, dx, p, torch.from_numpy(z["x"]), torch.from_numpy(z["r_seg"]), torch.from_numpy(z["r_img"]), False)


@pytest.mark.parametrize("linear", [False, True])
def test_gridnet_real_widths_64(dev, linear):
    z = np.load(os.path.join(GOLDEN, "gridnet_full64.npz"))
    tag = "lin_" if linear else ""
    x = torch.randn(1, 10, 64, 64, generator=torch.Generator().manual_seed(4))
    net, seg, img = run_case(dev, z, (32, 64, 96), 1, 64, 64, 2, x, False, tag, linear)
    rel_close(seg, torch.from_numpy(z[tag + "seg"]), what="seg")
    rel_close(img, torch.from_numpy(z[tag + "img"]), what="img")
    g = torch.Generator().manual_seed(2 + 77)
    r_seg, r_img = torch.randn(seg.shape, generator=g), torch.randn(img.shape, generator=g)
    dx = net.backward(r_seg.to(dev), r_img.to(dev))
    check = rel_close if linear else kink_tolerant
    check(dx, torch.from_numpy(z[tag + "dx"]), what="dx")
    grads = net.named_grads()
    want = {f[len(tag) + 5:]: torch.from_numpy(z[f]) for f in z.files if f.startswith(tag + "grad:")}
    want.update({str(n): torch.tensor([float(v)]) for n, v in zip(z["prelu_names"], z[tag + "prelu_grads"])})
    check_grads(grads, want, linear)
    if not linear:
        strict_given_branches(net, dx, G.test_params(G.param_shapes(10), seed=2), x, r_seg, r_img, False)
    order = list(G.param_shapes(10).keys())
    for k, w in zip(order, z[tag + "grad_abs_sums"]):
        if grads[k].numel() > 1:                                  # every other tensor: |grad| sum (slopes: above)
            got = float(grads[k].double().abs().sum())
            assert abs(got - w) <= (2e-4 if linear else 1e-2) * w + 1e-9, (k, got, w)


@pytest.mark.parametrize("linear", [False, True])
def test_coordgridnet_256(dev, linear):
    z = np.load(os.path.join(GOLDEN, "coordgridnet_256.npz"))
    tag = "lin_" if linear else ""
    x = torch.randn(1, 10, 256, 256, generator=torch.Generator().manual_seed(5))
    net, seg, img = run_case(dev, z, (8, 16, 24), 1, 256, 256, 3, x, True, tag, linear)
    rel_close(img[:, :, 100:164, 100:164], torch.from_numpy(z[tag + "img_crop"]), what="img crop")
    rel_close(seg[:, :, :24, :24], torch.from_numpy(z[tag + "seg_crop"]), what="seg crop")
    for name, t in (("seg", seg), ("img", img)):
        s1, s2 = float(t.double().sum()), float((t.double() ** 2).sum())
        assert abs(s1 - float(z[tag + name + "_sum"])) <= 1e-4 * abs(float(z[tag + name + "_sum"])) + 1e-4 * s2 ** 0.5
        assert abs(s2 - float(z[tag + name + "_sq"])) <= 1e-4 * float(z[tag + name + "_sq"])
    g = torch.Generator().manual_seed(3 + 77)
    r_seg, r_img = torch.randn(seg.shape, generator=g), torch.randn(img.shape, generator=g)
    dx = net.backward(r_seg.to(dev), r_img.to(dev))
    check = (lambda a, w, what: rel_close(a, w, tol=2e-4, what=what)) if linear else kink_tolerant
    check(dx[:, :, -16:, -16:], torch.from_numpy(z[tag + "dx_crop"]), what="dx crop")
    check_grads(net.named_grads(), {f[len(tag) + 5:]: torch.from_numpy(z[f]) for f in z.files if f.startswith(tag + "grad:")},
                linear, tol=2e-4)
    if not linear:
        strict_given_branches(net, dx, G.test_params(G.param_shapes(10, (8, 16, 24), coord=True), seed=3), x, r_seg, r_img,
                              True, tol=2e-4)


@pytest.mark.parametrize("linear", [False, True])
@pytest.mark.parametrize("b,H,W,filters", [(3, 16, 20, (8, 16, 24)), (1, 128, 128, (32, 64, 96))])
def test_against_cpu_restatement_other_shapes(dev, b, H, W, filters, linear):
    """Shapes without a stored fixture: ragged width / batch 3, and 128x128 at the real widths."""
    from vlg.gridnet import GridNetHIP
    net = GridNetHIP(10, b, H, W, dev, filters=filters, need_input_grad=True)
    p = G.test_params(G.param_shapes(10, filters), seed=9, linear=linear)
    net.load_state_dict(p)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(b, 10, H, W, generator=g)
    r_seg, r_img = torch.randn(b, 20, H, W, generator=g), torch.randn(b, 3, H, W, generator=g)
    seg_w, img_w, grads_w, dx_w = G.forward_backward(p, x, r_seg, r_img)
    seg, img = net.forward(x.to(dev))
    rel_close(seg, seg_w, what="seg")
    rel_close(img, img_w, what="img")
    dx = net.backward(r_seg.to(dev), r_img.to(dev))
    check = (lambda a, w, what: rel_close(a, w, tol=2e-4, what=what)) if linear else kink_tolerant
    check(dx, dx_w, what="dx")
    check_grads(net.named_grads(), grads_w, linear, tol=2e-4)
    if not linear:
        strict_given_branches(net, dx, p, x, r_seg, r_img, False, tol=2e-4)
    # halo stays exactly zero after forward + backward (the convolutions rely on it)
    for t in net.tensors:
        v = t.buf[t.geo.guard * t.cp:(t.geo.guard + t.geo.rows) * t.cp].view(t.geo.b, t.geo.H + 2, t.geo.W + 2, t.cp)
        c = t.C
        assert float(v[:, 0, :, :c].abs().max()) == 0 and float(v[:, :, 0, :c].abs().max()) == 0
        assert float(v[:, -1, :, :c].abs().max()) == 0 and float(v[:, :, -1, :c].abs().max()) == 0


def test_upsample_matches_torch(dev):
    from vlg import hip
    from vlg.gridnet import _Geo, _PT
    torch.manual_seed(0)
    b, h, w, C = 2, 6, 10, 5
    x = torch.randn(b, C, h, w, requires_grad=True)
    y = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)       # reference modules.py:50
    r = torch.randn_like(y)
    y.backward(r)
    S = torch.cuda.current_stream().cuda_stream
    gi, go = _Geo(b, h, w, dev), _Geo(b, 2 * h, 2 * w, dev)
    ti, to, tg, tgi = _PT(gi, C, dev), _PT(go, C, dev), _PT(go, C, dev), _PT(gi, C, dev)
    xd, rd = x.detach().to(dev), r.to(dev)
    hip.call("vlg_nchw_to_padded", xd.data_ptr(), ti.ptr, b, C, h, w, ti.cp, -1, S)
    hip.call("vlg_upsample2x_fwd", ti.ptr, to.ptr, b, h, w, ti.cp, S)
    out = torch.empty(b, C, 2 * h, 2 * w, device=dev)
    hip.call("vlg_padded_to_nchw", to.ptr, out.data_ptr(), b, C, 2 * h, 2 * w, to.cp, S)
    check_close(out, y.detach(), rtol=1e-5, atol=1e-6, what="upsample fwd")
    hip.call("vlg_nchw_to_padded", rd.data_ptr(), tg.ptr, b, C, 2 * h, 2 * w, tg.cp, -1, S)
    hip.call("vlg_upsample2x_bwd", tg.ptr, tgi.ptr, b, h, w, tgi.cp, 0, S)
    dxo = torch.empty(b, C, h, w, device=dev)
    hip.call("vlg_padded_to_nchw", tgi.ptr, dxo.data_ptr(), b, C, h, w, tgi.cp, S)
    check_close(dxo, x.grad, rtol=1e-5, atol=1e-5, what="upsample bwd")


def test_fill_coords_matches_reference_addcoords(dev):
    """The two constant channels vlg_fill_coords writes into a padded tensor are, bit for bit, what the reference's own
    AddCoords module appends (tests/golden/addcoords.npz, captured by oracle/make_golden_addcoords.py from
    models.modules.AddCoords, reference src/models/modules.py:65-96): first channel varies along H, second along W."""
    import numpy as np
    from conftest import GOLDEN
    from vlg import hip
    from vlg.gridnet import _Geo, _PT
    want = torch.from_numpy(np.load(GOLDEN + "/addcoords.npz")["coord_channels"])       # (2, 256, 256)
    b, H, W, C = 2, 256, 256, 5
    geo = _Geo(b, H, W, dev)
    t = _PT(geo, C, dev, coord=True)
    S = torch.cuda.current_stream().cuda_stream
    hip.call("vlg_fill_coords", t.ptr, b, H, W, t.cp, t.coord_c0, S)
    out = torch.empty(b, C + 2, H, W, device=dev)
    hip.call("vlg_padded_to_nchw", t.ptr, out.data_ptr(), b, C + 2, H, W, t.cp, S)
    got = out.cpu()
    for n in range(b):
        assert torch.equal(got[n, C:], want), "coordinate channels differ from the reference module's"
    assert float(got[:, :C].abs().max()) == 0.0
