"""The pixel step's layout, resampling, pooling, HED / VGG head and helper kernels (csrc/gridnet_ops.hip, the helper half of
csrc/image_ops.hip, the table launches of csrc/optim.hip), one C-ABI entry point at a time, against torch on the CPU in
float64 run on the same fp32 inputs.

Padded channels-last tensors are built on the host as vlg/gridnet.py builds them ((H+2) x (W+2) halo, cp lanes, guard rows
before and after), except that the halo, the guard rows and the lanes >= C hold a NaN sentinel wherever the kernel must not
read them, and every output buffer starts as that sentinel.  Each case asserts that every element the kernel owns was
written (and is finite, outside the NaN cases), that no other bit changed, and that the error is within a stated bar:
bitwise where the arithmetic is the same, otherwise a bound derived from the operation (EPS = 2^-24, the fp32 unit
roundoff).  The `prod` cases run every gridnet_ops.hip kernel above its 4096-block grid cap, so the grid-stride loops
iterate as they do at the benchmark shape, and the image losses at (32,3,256,256) against the plain-C oracle.

NaN cases follow torch's own CPU result: max-pool and ReLU keep a NaN, the max-pool gradient goes to the window's last
NaN in row-major order, argmax picks the first NaN, and the SSIM loss is NaN (torch.clamp keeps it).
"""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import check_close
from oracle import image_ref as R
from test_hip_gemm_paths import RIDER_ROWS, _rider_table

pytestmark = pytest.mark.gpu

SENT, SENT16 = 0x7FA5A5A5, 0x7FA5            # NaN payloads no kernel computes
EPS = 2.0 ** -24
ERR_SHAPE, ERR_ALIGN = 1001, 1002
NAN = float("nan")


@pytest.fixture(scope="module")
def H():
    from vlg import hip
    hip.load()
    return hip


def S():
    return torch.cuda.current_stream().cuda_stream


def _ceil(v, m):
    return -(-v // m) * m


def sentinel(n, dev):
    return torch.full((n,), SENT, dtype=torch.int32, device=dev)


def f32(raw):
    return raw.view(torch.float32)


class Padded:
    """(b, H+2, W+2, cp) channels-last rows between guard rows (vlg/gridnet.py _Geo / _PT); every bit is the sentinel
    until set."""

    def __init__(self, b, H, W, cp, dev):
        self.b, self.H, self.W, self.cp = b, H, W, cp
        self.guard = W + 2 + 40
        self.rows = b * (H + 2) * (W + 2)
        self.raw = sentinel((self.rows + 2 * self.guard) * cp, dev)
        self.ptr = f32(self.raw).data_ptr() + 4 * self.guard * cp

    def grid(self, t=None):
        t = f32(self.raw) if t is None else t
        return t[self.guard * self.cp:(self.guard + self.rows) * self.cp].view(self.b, self.H + 2, self.W + 2, self.cp)

    def set(self, x, c0=0):
        """x (b, C, H, W) -> interior lanes [c0, c0 + C)."""
        self.grid()[:, 1:self.H + 1, 1:self.W + 1, c0:c0 + x.shape[1]] = x.permute(0, 2, 3, 1).to(self.raw.device)

    def get(self, C=None, c0=0):
        """Interior lanes [c0, c0 + C) as (b, C, H, W) on the CPU."""
        C = self.cp - c0 if C is None else C
        return self.grid()[:, 1:self.H + 1, 1:self.W + 1, c0:c0 + C].permute(0, 3, 1, 2).cpu()

    def interior(self, C=None, c0=0):
        m = torch.zeros(self.raw.numel(), dtype=torch.bool, device=self.raw.device)
        self.grid(m)[:, 1:self.H + 1, 1:self.W + 1, c0:c0 + (self.cp - c0 if C is None else C)] = True
        return m


def untouched(raw, owned, what, before=None):
    """No bit outside `owned` differs from `before` (default: the sentinel)."""
    keep = ~owned
    ref = SENT if before is None else before[keep]
    same = raw[keep] == ref
    assert bool(same.all()), "%s: %d elements outside the owned region changed" % (what, int((~same).sum()))


def within(got, want, bound, what):
    """Every element finite and |got - want| <= bound (elementwise, fp64)."""
    got = got.detach().cpu()
    bad = ~torch.isfinite(got)
    assert not bool(bad.any()), "%s: %d/%d elements not finite" % (what, int(bad.sum()), bad.numel())
    err = (got.double() - want.double()).abs() - bound
    if bool((err > 0).any()):
        i = int(torch.argmax(err))
        raise AssertionError("%s: %d/%d outside the bound; worst at flat index %d: got %.9g want %.9g bound %.3g" % (
            what, int((err > 0).sum()), err.numel(), i, float(got.flatten()[i]), float(want.flatten()[i]),
            float(bound.flatten()[i] if torch.is_tensor(bound) else bound)))


def same_with_nan(got, want, what):
    """NaN at exactly the positions torch has one, equal values elsewhere (the NaN cases' comparison)."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert bool(wn.any()), "%s: the reference holds no NaN - the case tests nothing" % what
    assert torch.equal(gn, wn), "%s: NaN at %d positions, torch at %d (%d disagree)" % (
        what, int(gn.sum()), int(wn.sum()), int((gn != wn).sum()))
    assert torch.equal(got[~wn], want[~wn]), "%s: values differ outside the NaN positions" % what


# ------------------------------------------------------------------------------------------------ layout
LAYOUT = [(3, 1, 2, 2), (3, 3, 5, 7), (1, 5, 2, 9), (3, 33, 7, 3), pytest.param(32, 1, 256, 256, id="prod")]


@pytest.mark.parametrize("coord", [False, True], ids=["plain", "coord"])
@pytest.mark.parametrize("b,C,h,w", LAYOUT)
def test_layout_round_trip(H, dev, b, C, h, w, coord):
    """vlg_nchw_to_padded (with and without the AddCoords lanes) and vlg_padded_to_nchw: exact, only the owned lanes."""
    nc = C + (2 if coord else 0)
    cp = _ceil(nc, 4) + 4                               # lanes no kernel owns
    torch.manual_seed(C * 1000 + h + w)
    x = torch.randn(b, C, h, w)
    t = Padded(b, h, w, cp, dev)
    H.call("vlg_nchw_to_padded", x.to(dev).data_ptr(), t.ptr, b, C, h, w, cp, C if coord else -1, S())
    torch.cuda.synchronize()
    assert torch.equal(t.get(C), x)
    untouched(t.raw, t.interior(nc), "nchw_to_padded")
    if coord:
        yy = (torch.arange(h, dtype=torch.float64) / (h - 1) * 2 - 1).view(h, 1).expand(h, w)
        xx = (torch.arange(w, dtype=torch.float64) / (w - 1) * 2 - 1).view(1, w).expand(h, w)
        # fp32 quotient (<= EPS/2 of a value <= 1, doubled) then - 1: at most 2 EPS absolute
        within(t.get(2, c0=C), torch.stack([yy, xx]).expand(b, 2, h, w), 2 * EPS, "AddCoords lanes")
    n = b * C * h * w
    out = sentinel(n + 64, dev)
    H.call("vlg_padded_to_nchw", t.ptr, out.data_ptr(), b, C, h, w, cp, S())
    torch.cuda.synchronize()
    assert torch.equal(f32(out)[:n].view(b, C, h, w).cpu(), x)
    assert bool((out[n:] == SENT).all()), "padded_to_nchw wrote past its output"


# ------------------------------------------------------------------------------------------------ bilinear x2 upsample
UPS = [(2, 2, 3, 32), (1, 3, 7, 96), (2, 7, 2, 32), (1, 64, 128, 32), (1, 128, 64, 32),
       pytest.param(32, 128, 128, 12, id="prod")]


def _up(x):
    return F.interpolate(x, size=(2 * x.shape[2], 2 * x.shape[3]), mode="bilinear", align_corners=True)


def _up_t(g, h, w):
    """Uᵀ g in fp64 (autograd of _up)."""
    x = torch.zeros(g.shape[0], g.shape[1], h, w, dtype=torch.float64, requires_grad=True)
    _up(x).backward(g)
    return x.grad


@pytest.mark.parametrize("b,h,w,cp", UPS)
def test_upsample2x(H, dev, b, h, w, cp):
    """vlg_upsample2x_fwd / _bwd against F.interpolate(bilinear, align_corners=True) and its autograd; accumulate = 1 is
    bitwise the fresh result plus the prior contents; <Ux, g> = <x, Uᵀg> in fp64.  Bars: the source coordinate
    scale * o is formed in fp32, which moves each axis weight by up to k = 2 max(h, w) EPS (two taps of |x| <= max|x|
    each), plus the blend's own roundings; the transpose sums at most 16 such terms of |g| <= max|g|."""
    torch.manual_seed(h * 1000 + w + cp)
    x = torch.randn(b, cp, h, w)
    ti = Padded(b, h, w, cp, dev)
    ti.set(x)
    to = Padded(b, 2 * h, 2 * w, cp, dev)
    H.call("vlg_upsample2x_fwd", ti.ptr, to.ptr, b, h, w, cp, S())
    torch.cuda.synchronize()
    k = 2 * max(h, w)
    y = to.get()
    fwd_bar = (4 * k + 8) * EPS * float(x.abs().max())
    within(y, _up(x.double()), fwd_bar, "upsample fwd")
    untouched(to.raw, to.interior(), "upsample fwd")

    g = torch.randn(b, cp, 2 * h, 2 * w)
    tg = Padded(b, 2 * h, 2 * w, cp, dev)
    tg.set(g)
    di = Padded(b, h, w, cp, dev)
    H.call("vlg_upsample2x_bwd", tg.ptr, di.ptr, b, h, w, cp, 0, S())
    torch.cuda.synchronize()
    gx = di.get()
    bwd_bar = 16 * (2 * k + 8) * EPS * float(g.abs().max())
    within(gx, _up_t(g.double(), h, w), bwd_bar, "upsample bwd")
    untouched(di.raw, di.interior(), "upsample bwd")

    prior = torch.randn(b, cp, h, w)
    da = Padded(b, h, w, cp, dev)
    da.set(prior)
    H.call("vlg_upsample2x_bwd", tg.ptr, da.ptr, b, h, w, cp, 1, S())
    torch.cuda.synchronize()
    assert torch.equal(da.get(), gx + prior), "accumulate = 1 is not the fresh result plus the prior contents"
    untouched(da.raw, da.interior(), "upsample bwd (accumulate)")

    lhs = float((y.double() * g.double()).sum())
    rhs = float((x.double() * gx.double()).sum())
    tol = fwd_bar * float(g.double().abs().sum()) + bwd_bar * float(x.double().abs().sum())
    assert abs(lhs - rhs) <= tol, "<Ux, g> = %.12g but <x, U^T g> = %.12g (bar %.3g)" % (lhs, rhs, tol)


# ------------------------------------------------------------------------------------------------ 2x2 max-pool
POOL = [(2, 3, 5, 8), (1, 8, 8, 32), (3, 7, 2, 4), pytest.param(32, 128, 128, 12, id="prod")]
TIES = torch.tensor([-2.0, -1.0, -0.0, 0.0, 1.0, 2.0])


def _pool(H, dev, x, gy):
    """Runs vlg_maxpool2x2 and vlg_maxpool2x2_bwd on x (b, cp, 2h, 2w) and gy (b, cp, h, w); returns (y, dx) as
    (b, cp, ...) CPU tensors after checking that nothing outside the interiors was written."""
    b, cp, h, w = x.shape[0], x.shape[1], x.shape[2] // 2, x.shape[3] // 2
    ti, to = Padded(b, 2 * h, 2 * w, cp, dev), Padded(b, h, w, cp, dev)
    ti.set(x)
    H.call("vlg_maxpool2x2", ti.ptr, to.ptr, b, h, w, cp, S())
    tg, di = Padded(b, h, w, cp, dev), Padded(b, 2 * h, 2 * w, cp, dev)
    tg.set(gy)
    H.call("vlg_maxpool2x2_bwd", ti.ptr, tg.ptr, di.ptr, b, h, w, cp, S())
    torch.cuda.synchronize()
    untouched(to.raw, to.interior(), "maxpool fwd")
    untouched(di.raw, di.interior(), "maxpool bwd")
    return to.get(), di.get()


def _pool_ref(x, gy):
    xd = x.double().requires_grad_(True)
    y = F.max_pool2d(xd, 2)
    y.backward(gy.double())
    return y.detach(), xd.grad


@pytest.mark.parametrize("b,h,w,cp", POOL)
def test_maxpool2x2(H, dev, b, h, w, cp):
    """Values from a 6-element set with ±0, so most windows tie: the value is torch's, and the backward writes the
    gradient at torch's index (the first maximum in row-major order) and zeros at the three other positions."""
    gen = torch.Generator().manual_seed(h * 100 + w)
    x = TIES[torch.randint(0, len(TIES), (b, cp, 2 * h, 2 * w), generator=gen)]
    gy = torch.randn(b, cp, h, w, generator=gen)
    win = x.double().unfold(2, 2, 2).unfold(3, 2, 2).reshape(b, cp, h, w, 4)
    assert bool(((win == win.max(-1, keepdim=True).values).sum(-1) > 1).any()), "no tied window"
    y, dx = _pool(H, dev, x, gy)
    want_y, want_dx = _pool_ref(x, gy)
    assert torch.equal(y.double(), want_y), "max-pool value"
    assert torch.equal(dx.double(), want_dx), "max-pool gradient routing"


def test_maxpool2x2_nan(H, dev):
    """torch's max_pool2d returns NaN for a window holding one, and its gradient goes to the window's LAST NaN."""
    b, h, w, cp = 2, 4, 5, 8
    gen = torch.Generator().manual_seed(7)
    x = TIES[torch.randint(0, len(TIES), (b, cp, 2 * h, 2 * w), generator=gen)]
    x[0, 0, 0, 1] = x[0, 0, 1, 0] = NAN                   # two NaNs in one window
    x[0, 1, 0, 2] = NAN                                    # NaN first in its window
    x[1, 5, 3, 3] = NAN                                    # NaN last in its window
    x[1, 2][torch.rand(2 * h, 2 * w, generator=gen) < 0.1] = NAN
    gy = torch.randn(b, cp, h, w, generator=gen)
    y, dx = _pool(H, dev, x, gy)
    want_y, want_dx = _pool_ref(x, gy)
    same_with_nan(y, want_y, "max-pool value with NaN")
    assert torch.equal(dx.double(), want_dx), "max-pool gradient routing with NaN"


# ------------------------------------------------------------------------------------------------ HED score + head
def _score(H, dev, x, w, bias, cp):
    """vlg_score1x1_relu on x (b, C, H, W) in a padded tensor with NaN lanes >= C and NaN halos -> (b, H, W)."""
    b, C, h, ww = x.shape
    t = Padded(b, h, ww, cp, dev)
    t.set(x)
    prm = torch.cat([w, bias]).to(dev)
    n = b * h * ww
    out = sentinel(n + 64, dev)
    H.call("vlg_score1x1_relu", t.ptr, prm.data_ptr(), prm.data_ptr() + 4 * C, f32(out).data_ptr(), b, h, ww, C, cp, S())
    torch.cuda.synchronize()
    assert bool((out[n:] == SENT).all()), "score1x1 wrote past its output"
    return f32(out)[:n].view(b, h, ww).cpu()


SCORE = [(2, 1, 5, 7, 32), (2, 3, 5, 7, 32), (2, 63, 5, 7, 64), (2, 64, 5, 7, 96), (2, 65, 5, 7, 96),
         (1, 512, 4, 6, 544), pytest.param(32, 3, 256, 256, 4, id="prod")]


@pytest.mark.parametrize("b,C,h,w,cp", SCORE)
def test_score1x1_relu(H, dev, b, C, h, w, cp):
    """relu(x) . w + b over the C real lanes; the NaN in lanes >= C and in the halos must not leak.  Bar: C + 2
    roundings (products, the per-lane sums and the shuffle tree, the bias) relative to sum |terms| + |b|."""
    torch.manual_seed(C)
    x, wt, bias = torch.randn(b, C, h, w), torch.randn(C), torch.randn(1)
    got = _score(H, dev, x, wt, bias, cp)
    terms = F.relu(x.double()) * wt.double().view(1, C, 1, 1)
    bound = (C + 2) * EPS * (terms.abs().sum(1) + bias.double().abs())
    within(got, terms.sum(1) + bias.double(), bound, "score1x1")


def _hed_ref(s, cw, cb, Hh, Ww):
    """(6, b, H, W): sigmoid of each level's score upsampled with F.interpolate(bilinear, align_corners=False), and the
    sigmoid of the 1x1 fuse over the five (oracle/hned_spec.py forward), in fp64; plus the same upsampling of |score|."""
    up = [F.interpolate(t.double().unsqueeze(1), size=(Hh, Ww), mode="bilinear", align_corners=False).squeeze(1) for t in s]
    up_abs = [F.interpolate(t.double().abs().unsqueeze(1), size=(Hh, Ww), mode="bilinear", align_corners=False).squeeze(1)
              for t in s]
    f = cb.double() + sum(float(cw[k]) * up[k] for k in range(5))
    return torch.stack([torch.sigmoid(u) for u in up] + [torch.sigmoid(f)]), up_abs


def _hed_head(H, dev, s, cw, cb, b, Hh, Ww):
    ds = [t.contiguous().to(dev) for t in s]
    prm = torch.cat([cw, cb]).to(dev)
    n = 6 * b * Hh * Ww
    out = sentinel(n + 64, dev)
    H.call("vlg_hed_head", *[t.data_ptr() for t in ds], prm.data_ptr(), prm.data_ptr() + 20, f32(out).data_ptr(), b, Hh, Ww, S())
    torch.cuda.synchronize()
    assert bool((out[n:] == SENT).all()), "hed_head wrote past its output"
    return f32(out)[:n].view(6, b, Hh, Ww).cpu()


@pytest.mark.parametrize("b,Hh,Ww", [(1, 16, 16), (2, 48, 80), (3, 256, 256), pytest.param(32, 256, 256, id="prod")])
def test_hed_head(H, dev, b, Hh, Ww):
    """Five score maps (level k at H >> k; at 16x16 level 4 is 1x1) with a tenth of the scores at up to ±100
    (saturated sigmoids).  Absolute bars: fp32 flushes to 0 what fp64 keeps near 0.  The interpolation weights are
    exact in fp32 here (powers of two), so a level's blend is off by <= 6 EPS sum |terms| and its sigmoid by 1/4 of
    that plus the sigmoid's own rounding; the fuse adds 7 roundings of cb + sum_k cw_k v_k."""
    gen = torch.Generator().manual_seed(Hh + Ww + b)
    s = []
    for k in range(5):
        t = torch.randn(b, Hh >> k, Ww >> k, generator=gen) * 3
        big = torch.rand(t.shape, generator=gen) < 0.1
        t[big] = (torch.rand(t.shape, generator=gen)[big] * 200 - 100)
        s.append(t)
    cw, cb = torch.randn(5, generator=gen) * 0.5, torch.randn(1, generator=gen)
    got = _hed_head(H, dev, s, cw, cb, b, Hh, Ww)
    want, up_abs = _hed_ref(s, cw, cb, Hh, Ww)
    sig = 4e-7
    for k in range(5):
        within(got[k], want[k], sig + 0.25 * 6 * EPS * up_abs[k], "d%d" % (k + 1))
    arg = sum(abs(float(cw[k])) * up_abs[k] for k in range(5))
    within(got[5], want[5], sig + 0.25 * (6 * EPS * arg + 7 * EPS * (arg + abs(float(cb)))), "fuse")


def test_score1x1_then_hed_head_nan(H, dev):
    """A NaN feature lane below C gives a NaN score (torch's relu keeps it), and the HED head carries it into d1 and the
    fuse at that pixel only; the other pixels stay finite and right."""
    b, C, Hh, Ww, cp = 2, 65, 16, 32, 96
    torch.manual_seed(3)
    x, wt, bias = torch.randn(b, C, Hh, Ww), torch.randn(C) * 0.1, torch.randn(1)
    x[0, 7, 3, 5] = NAN
    x[1, 64, 10, 0] = NAN
    s0 = _score(H, dev, x, wt, bias, cp)
    want0 = (F.relu(x.double()) * wt.double().view(1, C, 1, 1)).sum(1) + bias.double()
    assert bool(torch.isnan(want0).sum() == 2)
    assert torch.equal(torch.isnan(s0), torch.isnan(want0)), "score1x1: NaN positions differ from torch"
    fin = ~torch.isnan(want0)
    check_close(s0[fin], want0[fin], rtol=1e-5, atol=1e-5, what="score1x1 (finite pixels)")
    gen = torch.Generator().manual_seed(4)
    s = [s0] + [torch.randn(b, Hh >> k, Ww >> k, generator=gen) for k in range(1, 5)]
    cw, cb = torch.randn(5, generator=gen), torch.randn(1, generator=gen)
    got = _hed_head(H, dev, s, cw, cb, b, Hh, Ww)
    want, _ = _hed_ref([s0.double()] + s[1:], cw, cb, Hh, Ww)
    for k in range(6):
        gn, wn = torch.isnan(got[k]), torch.isnan(want[k])
        assert torch.equal(gn, wn), "hed_head output %d: NaN positions differ from torch" % k
        check_close(got[k][~wn], want[k][~wn], rtol=0, atol=1e-6, what="hed_head output %d (finite pixels)" % k)


# ------------------------------------------------------------------------------------------------ VGG L1 of ReLU
def _l1_relu(H, dev, xa, xb, cp, gscale, want_grad=True):
    """vlg_l1_relu_padded over two padded tensors with zero halos and zero lanes >= C (as the VGG trunk leaves them);
    returns (loss, da padded) after checking the guard rows and the scratch tail."""
    b, C, h, w = xa.shape
    ta, tb = Padded(b, h, w, cp, dev), Padded(b, h, w, cp, dev)
    for t, x in ((ta, xa), (tb, xb)):
        t.grid().zero_()
        t.set(x)
    da = Padded(b, h, w, cp, dev)
    scratch = sentinel(4096 + 64, dev)
    loss = sentinel(4, dev)
    H.call("vlg_l1_relu_padded", ta.ptr, tb.ptr, da.ptr if want_grad else 0, f32(loss).data_ptr(), f32(scratch).data_ptr(),
           ta.rows, cp, b * C * h * w, gscale, S())
    torch.cuda.synchronize()
    assert bool((scratch[4096:] == SENT).all()), "l1_relu_padded wrote past its 4096-float scratch"
    assert bool((loss[1:] == SENT).all())
    rows = torch.zeros(da.raw.numel(), dtype=torch.bool, device=dev)
    da.grid(rows).fill_(True)
    untouched(da.raw, rows if want_grad else torch.zeros_like(rows), "l1_relu_padded gradient")
    return f32(loss)[:1].cpu(), da


def _l1_relu_ref(xa, xb, gscale):
    a = xa.double().requires_grad_(True)
    v = F.l1_loss(F.relu(a), F.relu(xb.double()), reduction="sum") / xa.numel()
    (gscale * v).backward()
    return v.detach(), a.grad


@pytest.mark.parametrize("b,C,h,w,cp", [(2, 5, 6, 7, 8), pytest.param(4, 13, 256, 256, 16, id="prod")])
def test_l1_relu_padded(H, dev, b, C, h, w, cp):
    """mean |relu(a) - relu(b)| over count = b C H W and its gradient times grad_scale; with da = NULL the value is bitwise
    the same.  The prod case has more than 4096 x 256 float4, so the 4096 block partials fill the scratch exactly.  Value
    bar: each thread sums 4 k elements serially, then two block trees and the 1/count scale: (4 k + 40) EPS relative."""
    torch.manual_seed(b + C)
    xa, xb = torch.randn(b, C, h, w), torch.randn(b, C, h, w)
    gscale = 0.75
    loss, da = _l1_relu(H, dev, xa, xb, cp, gscale)
    loss0, _ = _l1_relu(H, dev, xa, xb, cp, gscale, want_grad=False)
    assert torch.equal(loss, loss0), "the value changes when no gradient is asked for"
    v, g = _l1_relu_ref(xa, xb, gscale)
    rows = b * (h + 2) * (w + 2)
    n4 = rows * cp // 4
    k = -(-n4 // (min(4096, -(-n4 // 256)) * 256))
    within(loss, v.view(1), (4 * k + 40) * EPS * v.abs(), "L1-of-ReLU value")
    within(da.get(C), g, 2 * EPS * g.abs(), "L1-of-ReLU gradient")
    rest = da.grid()[:, :, :, :].clone()
    rest[:, 1:h + 1, 1:w + 1, :C] = 0
    assert bool((rest == 0).all()), "gradient not zero in the halo / lanes >= C"


def test_l1_relu_padded_nan(H, dev):
    """A NaN in the generator's features: torch's value is NaN, its gradient 0 at the NaN lane and unchanged elsewhere."""
    b, C, h, w, cp = 2, 5, 6, 7, 8
    torch.manual_seed(9)
    xa, xb = torch.randn(b, C, h, w), torch.randn(b, C, h, w)
    xa[1, 2, 3, 4] = NAN
    loss, da = _l1_relu(H, dev, xa, xb, cp, 1.0)
    v, g = _l1_relu_ref(xa, xb, 1.0)
    assert math.isnan(float(v))
    assert math.isnan(float(loss)), "L1-of-ReLU value is %r where torch's is NaN" % float(loss)
    check_close(da.get(C), g, rtol=1e-6, atol=0, what="L1-of-ReLU gradient with a NaN lane")


# ------------------------------------------------------------------------------------------------ add_rows
@pytest.mark.parametrize("n", [4, pytest.param(8 * 4096 * 256 + 12, id="prod")])
def test_add_rows(H, dev, n):
    """dst = src (accumulate 0) and dst += src (accumulate 1), bitwise; nothing past n."""
    torch.manual_seed(n % 1000)
    src = torch.randn(n, device=dev)
    prior = torch.randn(n, device=dev)
    for acc in (0, 1):
        dst = sentinel(n + 64, dev)
        if acc:
            f32(dst)[:n] = prior
        H.call("vlg_add_rows", f32(dst).data_ptr(), src.data_ptr(), n, acc, S())
        torch.cuda.synchronize()
        want = prior + src if acc else src
        assert torch.equal(f32(dst)[:n], want), "add_rows accumulate=%d" % acc
        assert bool((dst[n:] == SENT).all()), "add_rows wrote past n"


# ------------------------------------------------------------------------------------------------ image helpers
@pytest.mark.parametrize("b,hw", [(2, 185), pytest.param(32, 65536, id="prod")])
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_affine_nchw(H, dev, b, C, hw):
    """(x - shift[c]) * scale[c], bitwise torch fp32."""
    torch.manual_seed(C * 10 + b)
    x = torch.randn(b, C, hw)
    sh, sc = torch.randn(C), torch.rand(C) + 0.5
    arr = ctypes.c_float * C
    out = sentinel(x.numel() + 64, dev)
    H.call("vlg_affine_nchw", x.to(dev).data_ptr(), f32(out).data_ptr(), b, C, hw, arr(*sh.tolist()), arr(*sc.tolist()), S())
    torch.cuda.synchronize()
    assert torch.equal(f32(out)[:x.numel()].view(b, C, hw).cpu(), (x - sh.view(1, C, 1)) * sc.view(1, C, 1))
    assert bool((out[x.numel():] == SENT).all())


def test_rollout_input(H, dev):
    """cat[e_a, seg_a, img_a, img_b, seg_b, e_b] (vlg/image_engine.py rollout order), bitwise."""
    b, hw = 3, 7 * 9
    torch.manual_seed(11)
    one = [torch.randn(b, 1, hw) for _ in range(4)]
    img = [torch.randn(b, 3, hw) for _ in range(2)]
    parts = [one[0], one[1], img[0], img[1], one[2], one[3]]
    dp = [t.to(dev) for t in parts]
    n = b * 10 * hw
    out = sentinel(n + 64, dev)
    H.call("vlg_rollout_input", *[t.data_ptr() for t in dp], f32(out).data_ptr(), b, hw, S())
    torch.cuda.synchronize()
    assert torch.equal(f32(out)[:n].view(b, 10, hw).cpu(), torch.cat(parts, 1))
    assert bool((out[n:] == SENT).all())


def _argmax(H, dev, x):
    b, C, hw = x.shape
    out = sentinel(b * hw + 64, dev)
    H.call("vlg_argmax_nchw", x.to(dev).data_ptr(), f32(out).data_ptr(), b, C, hw, S())
    torch.cuda.synchronize()
    assert bool((out[b * hw:] == SENT).all())
    return f32(out)[:b * hw].view(b, hw).cpu()


@pytest.mark.parametrize("b,C,hw", [(3, 5, 63), (2, 1, 35), (2, 20, 1001)])
def test_argmax_nchw(H, dev, b, C, hw):
    """torch.argmax(dim=1) on logits from a small integer set (ties everywhere): the first maximum wins."""
    gen = torch.Generator().manual_seed(C * hw)
    x = torch.randint(-2, 3, (b, C, hw), generator=gen).float()
    assert torch.equal(_argmax(H, dev, x), torch.argmax(x.double(), dim=1).float())


def test_argmax_nchw_nan(H, dev):
    """torch.argmax returns the first NaN of a pixel's classes."""
    b, C, hw = 2, 6, 45
    gen = torch.Generator().manual_seed(12)
    x = torch.randint(-2, 3, (b, C, hw), generator=gen).float()
    x[0, 3, 0] = NAN
    x[0, 1, 1] = x[0, 4, 1] = NAN
    x[1, 0, 2] = NAN
    x[1, 5, 3] = NAN
    want = torch.argmax(x.double(), dim=1).float()
    assert int(want[0, 1]) == 1 and int(want[1, 3]) == 5
    assert torch.equal(_argmax(H, dev, x), want), "argmax with NaN"


# ------------------------------------------------------------------------------------------------ partial sums, tables
PARTS = [1, 255, 257, 5000]


@pytest.mark.parametrize("n", PARTS)
def test_sum_partials(H, dev, n):
    """vlg_sum_partials against the fp64 sum (bar: ceil(n / 256) serial adds plus an 8-level tree, relative to
    sum |p|); accumulate = 1 is bitwise the prior value plus the fresh sum."""
    torch.manual_seed(n)
    p = torch.randn(n, device=dev)
    dst = sentinel(4, dev)
    H.call("vlg_sum_partials", p.data_ptr(), n, f32(dst).data_ptr(), 0, S())
    torch.cuda.synchronize()
    fresh = f32(dst)[:1].cpu()
    pd = p.cpu().double()
    within(fresh, pd.sum().view(1), (-(-n // 256) + 10) * EPS * pd.abs().sum(), "sum_partials")
    assert bool((dst[1:] == SENT).all())
    f32(dst)[0] = 0.625
    H.call("vlg_sum_partials", p.data_ptr(), n, f32(dst).data_ptr(), 1, S())
    torch.cuda.synchronize()
    assert torch.equal(f32(dst)[:1].cpu(), torch.tensor([0.625]) + fresh), "accumulate = 1"


def test_sum_partials_table(H, dev):
    """Each table row {partials, count, destination} is bitwise vlg_sum_partials of the same partials; nothing else in
    the destination buffer is written."""
    torch.manual_seed(21)
    parts = [torch.randn(n, device=dev) for n in PARTS]
    dst = sentinel(64, dev)
    offs = [3, 17, 18, 40]
    table = torch.tensor([[p.data_ptr(), p.numel(), f32(dst).data_ptr() + 4 * o] for p, o in zip(parts, offs)],
                         dtype=torch.int64, device=dev)
    H.call("vlg_sum_partials_table", table.data_ptr(), len(parts), S())
    single = sentinel(4, dev)
    mask = torch.zeros(64, dtype=torch.bool, device=dev)
    for p, o in zip(parts, offs):
        H.call("vlg_sum_partials", p.data_ptr(), p.numel(), f32(single).data_ptr(), 0, S())
        torch.cuda.synchronize()
        assert torch.equal(dst[o:o + 1], single[:1]), "table row of %d partials" % p.numel()
        mask[o] = True
    untouched(dst, mask, "sum_partials_table")


def test_reduce_slabs_table_standalone(H, dev):
    """vlg_reduce_slabs_table as its own launch at GridNet's 64 blocks per row (vlg/gridnet.py), over the rider rows of
    test_hip_gemm_paths (tall and flat branches): each row bitwise vlg_reduce_slabs, nothing outside the rows written."""
    slabs, dst, offs, table = _rider_table(dev, seed=33)
    H.call("vlg_reduce_slabs_table", table.data_ptr(), len(RIDER_ROWS), 64, S())
    torch.cuda.synchronize()
    df = f32(dst)
    mask = torch.zeros(dst.numel(), dtype=torch.bool, device=dev)
    for s, (n, length, stride), off in zip(slabs, RIDER_ROWS, offs):
        mask[off:off + length] = True
        single = torch.empty(length, device=dev)
        H.call("vlg_reduce_slabs", s.data_ptr(), stride, n, single.data_ptr(), length, S())
        torch.cuda.synchronize()
        assert torch.equal(df[off:off + length], single), "table row (%d slabs, length %d)" % (n, length)
    untouched(dst, mask, "reduce_slabs_table")


def test_adam_step_graph(H, dev):
    """K = 50 steps of vlg_adam_step_graph (step counter and bias-correction factors on the device) against vlg_adam_step
    at the same step from the same state: params, m and v bitwise, the bf16 shadow = params.to(bfloat16); advance = 0
    repeats the step without moving the counter.  The device computes the factors with its own pow: a step where one
    differs from the host's (torch.optim.Adam's double arithmetic) by one ulp is reported and bounded there instead."""
    n, K = 4100, 50
    lr, b1, b2, eps, gs = 2e-4, 0.5, 0.999, 1e-8, 0.5
    lrf, b1f, b2f = (float(np.float32(v)) for v in (lr, b1, b2))
    torch.manual_seed(50)
    p = torch.randn(n, device=dev)
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    pg, mg, vg = p.clone(), m.clone(), v.clone()
    state = torch.zeros(4, device=dev)
    shadow = torch.full((n + 8,), SENT16, dtype=torch.int16, device=dev)
    off_by_one = []

    def graph_step(g, advance):
        H.call("vlg_adam_step_graph", pg.data_ptr(), g.data_ptr(), mg.data_ptr(), vg.data_ptr(), shadow.data_ptr(), n,
               state.data_ptr(), advance, lr, b1, b2, eps, gs, S())

    for k, advance in [(k, 1) for k in range(1, K + 1)] + [(K, 0)]:
        g = torch.randn(n, device=dev)
        pg.copy_(p), mg.copy_(m), vg.copy_(v)               # same state on both sides: no difference carries over
        p_before = p.clone()
        H.call("vlg_adam_step", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, k, lr, b1, b2, eps, gs, S())
        graph_step(g, advance)
        torch.cuda.synchronize()
        st = state.cpu()
        assert int(st.view(torch.int32)[2]) == k, "step counter %d after step %d (advance=%d)" % (
            int(st.view(torch.int32)[2]), k, advance)
        host = np.array([lrf / (1.0 - b1f ** k), math.sqrt(1.0 - b2f ** k)], dtype=np.float32)
        ulps = np.abs(st[:2].numpy().view(np.int32).astype(np.int64) - host.view(np.int32).astype(np.int64))
        assert torch.equal(mg, m) and torch.equal(vg, v), "m / v differ at step %d" % k
        if ulps.max() == 0:
            assert torch.equal(pg, p), "params differ at step %d (same factors)" % k
        else:
            assert ulps.max() <= 1, "device factors %d ulp from the host's at step %d" % (int(ulps.max()), k)
            off_by_one.append(k)
            bound = 4 * EPS * (p - p_before).abs() + 2 * EPS * p.abs()
            assert bool(((pg - p).abs() <= bound).all()), "params beyond the one-ulp bar at step %d" % k
        assert torch.equal(shadow[:n], pg.to(torch.bfloat16).view(torch.int16)), "bf16 shadow at step %d" % k
        assert bool((shadow[n:] == SENT16).all()), "shadow written past n"
    if off_by_one:
        print("vlg_adam_step_graph: a device factor is one ulp from the host's at steps %s" % off_by_one)


# ------------------------------------------------------------------------------------------------ image losses, prod
def _loss(H, dev, name, a, b, *dims, target=None):
    ad, bd = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev) if target is None else torch.from_numpy(target).to(dev)
    g = torch.full_like(ad, NAN)
    loss = torch.full((1,), NAN, device=dev)
    scratch = torch.zeros(H.load().vlg_image_loss_scratch(), device=dev)
    H.call(name, ad.data_ptr(), bd.data_ptr(), g.data_ptr(), loss.data_ptr(), scratch.data_ptr(), *dims, 1.0, S())
    torch.cuda.synchronize()
    return float(loss.item()), g.cpu()


def test_image_losses_prod(H, dev):
    """vlg_l1_mean, vlg_gradient_loss, vlg_ssim_loss and vlg_ce_nchw (with ignore_index pixels) at the benchmark's
    (32,3,256,256), above the 1024-block cap of the image kernels, against the plain-C oracle (bars of
    test_hip_image_ops.test_losses_match_c_oracle; every gradient element written and finite)."""
    b, C, Hh, Ww = 32, 3, 256, 256
    rng = np.random.default_rng(32)
    x = rng.random((b, C, Hh, Ww), dtype=np.float32)
    y = (x + 0.2 * rng.standard_normal(x.shape).astype(np.float32)).clip(0, 1).astype(np.float32)
    for fn, ref, dims in (("vlg_l1_mean", R.l1_mean, (x.size,)), ("vlg_gradient_loss", R.gradient_loss, (b * C, Hh, Ww)),
                          ("vlg_ssim_loss", R.ssim_loss, (b, C, Hh, Ww))):
        v, g = _loss(H, dev, fn, x, y, *dims)
        rv, rg = ref(x, y)
        assert abs(v - rv) <= 1e-4 * abs(rv), "%s: %r vs %r" % (fn, v, rv)
        check_close(g, torch.from_numpy(rg), rtol=1e-4, atol=1e-5 * float(np.abs(rg).max()), what=fn)
    logits = (rng.standard_normal((b, C, Hh, Ww)) * 3).astype(np.float32)
    target = rng.integers(0, C, (b, Hh, Ww))
    target[rng.random(target.shape) < 0.05] = -100
    v, g = _loss(H, dev, "vlg_ce_nchw", logits, None, b, C, Hh * Ww, target=target)
    rv, rg = R.ce_nchw(logits, target)
    assert abs(v - rv) <= 1e-4 * abs(rv), "ce: %r vs %r" % (v, rv)
    check_close(g, torch.from_numpy(rg), rtol=1e-4, atol=1e-9, what="ce gradient")


def test_ssim_tile_cap(H, dev):
    """One partial per 32x32 tile: exactly IMG_MAX_TILES (65536) tiles are accepted and right, one plane more is refused."""
    rng = np.random.default_rng(65536)
    x = rng.random((16384, 4, 3, 3), dtype=np.float32)
    y = rng.random((16384, 4, 3, 3), dtype=np.float32)
    v, g = _loss(H, dev, "vlg_ssim_loss", x, y, 16384, 4, 3, 3)
    rv, rg = R.ssim_loss(x, y)
    assert abs(v - rv) <= 1e-4 * abs(rv), "ssim at 65536 tiles: %r vs %r" % (v, rv)
    check_close(g, torch.from_numpy(rg), rtol=1e-4, atol=2e-7, what="ssim gradient at 65536 tiles")
    z = torch.zeros(65537 * 9, device=dev)
    scratch = torch.zeros(H.load().vlg_image_loss_scratch(), device=dev)
    assert H.load().vlg_ssim_loss(z.data_ptr(), z.data_ptr(), z.data_ptr(), scratch.data_ptr(), scratch.data_ptr(),
                                  65537, 1, 3, 3, 1.0, S()) == ERR_SHAPE


def _ssim_ref(x, y):
    """reference src/loss.py:68-91 restated in torch fp64: 3x3 mean windows without padding, clamp((1 - SSIM) / 2, 0, 1),
    mean over (b, H-2, W-2) per channel, summed over channels."""
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    mu_x, mu_y = F.avg_pool2d(x, 3, 1), F.avg_pool2d(y, 3, 1)
    sx = F.avg_pool2d(x * x, 3, 1) - mu_x ** 2
    sy = F.avg_pool2d(y * y, 3, 1) - mu_y ** 2
    sxy = F.avg_pool2d(x * y, 3, 1) - mu_x * mu_y
    s = ((2 * mu_x * mu_y + C1) * (2 * sxy + C2)) / ((mu_x ** 2 + mu_y ** 2 + C1) * (sx + sy + C2))
    return torch.clamp((1 - s) / 2, 0, 1).mean(dim=(0, 2, 3)).sum()


def test_ssim_nan(H, dev):
    """One NaN pixel in the generator output: torch's SSIM loss is NaN (torch.clamp keeps it), so the kernel's must be."""
    rng = np.random.default_rng(5)
    x = rng.random((2, 3, 40, 40), dtype=np.float32)
    y = rng.random((2, 3, 40, 40), dtype=np.float32)
    x[1, 2, 20, 33] = np.nan
    want = _ssim_ref(torch.from_numpy(x).double(), torch.from_numpy(y).double())
    assert math.isnan(float(want))
    v, _ = _loss(H, dev, "vlg_ssim_loss", x, y, 2, 3, 40, 40)
    assert math.isnan(v), "SSIM loss is %r where torch's is NaN" % v


# ------------------------------------------------------------------------------------------------ argument checks
def test_bad_arguments_are_refused(H, dev):
    """Shape and alignment errors come back as VLG_ERR_SHAPE / VLG_ERR_ALIGN before anything is launched."""
    lib = H.load()
    buf = torch.zeros(4096, device=dev)
    p, q, r = buf.data_ptr(), buf.data_ptr() + 4096, buf.data_ptr() + 8192
    s = S()
    shape = [
        ("maxpool cp % 4", lib.vlg_maxpool2x2(p, q, 1, 2, 2, 6, s)),
        ("maxpool_bwd cp % 4", lib.vlg_maxpool2x2_bwd(p, q, r, 1, 2, 2, 6, s)),
        ("upsample fwd cp % 4", lib.vlg_upsample2x_fwd(p, q, 1, 2, 2, 6, s)),
        ("upsample bwd cp % 4", lib.vlg_upsample2x_bwd(p, q, 1, 2, 2, 6, 0, s)),
        ("l1_relu_padded cp % 4", lib.vlg_l1_relu_padded(p, q, r, r, r, 4, 6, 4, 1.0, s)),
        ("nchw_to_padded cp % 4", lib.vlg_nchw_to_padded(p, q, 1, 3, 2, 2, 6, -1, s)),
        ("hed_head H % 16", lib.vlg_hed_head(p, p, p, p, p, q, q, r, 1, 24, 16, s)),
        ("hed_head W % 16", lib.vlg_hed_head(p, p, p, p, p, q, q, r, 1, 16, 40, s)),
        ("add_rows n % 4", lib.vlg_add_rows(p, q, 6, 0, s)),
        ("score1x1 C > cp", lib.vlg_score1x1_relu(p, q, q, r, 1, 2, 2, 9, 8, s)),
    ]
    align = [
        ("maxpool in + 4", lib.vlg_maxpool2x2(p + 4, q, 1, 2, 2, 8, s)),
        ("maxpool_bwd din + 4", lib.vlg_maxpool2x2_bwd(p, q, r + 4, 1, 2, 2, 8, s)),
        ("upsample fwd out + 4", lib.vlg_upsample2x_fwd(p, q + 4, 1, 2, 2, 8, s)),
        ("upsample bwd dout + 4", lib.vlg_upsample2x_bwd(p + 4, q, 1, 2, 2, 8, 0, s)),
        ("l1_relu_padded a + 4", lib.vlg_l1_relu_padded(p + 4, q, r, r, r, 4, 8, 4, 1.0, s)),
        ("add_rows src + 4", lib.vlg_add_rows(p, q + 4, 8, 0, s)),
    ]
    torch.cuda.synchronize()
    for what, rc in shape:
        assert rc == ERR_SHAPE, "%s returned %d" % (what, rc)
    for what, rc in align:
        assert rc == ERR_ALIGN, "%s returned %d" % (what, rc)
