"""Dropout on the GPU (csrc/dropout.hip, vlg/engine.py): the two fused kernels against the CPU restatement of the mask
(tests/dropout_ref.py) and fp64 arithmetic - also past one trip of their row loops ("prod") -, their refusals, and the
engine with the knob on - against dropout_ref's fp64 model with the masks of the counter value the step read - the step
counter, capture, checkpoints, evaluation entry points and the knob-off engine."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import dropout_ref as R
import step_stages as SS
from helpers import check_close
from oracle import layout_spec as O
from test_hip_layout_ops import GUARD, H, S, _buf, _guard, _ln_bars, _ln_inputs, _ln_R  # noqa: F401  (H is a fixture)
from test_hip_pixel_ops import ERR_ALIGN, ERR_SHAPE, SENT, f32, sentinel, untouched, within

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SEED = (0x9E3779B9 << 32) | 1024          # both key words in use
ROWS = (1, 5, 259)                        # fewer rows than a row group, a ragged last group, several rows per wave
DS = (64, 192, 256, 512, 1024)
PS = (0.0, 0.1, 0.5)


def _step_buf(dev, k):
    return torch.full((1,), k, dtype=torch.int32, device=dev)


def _fwd_inputs(rows, d, seed):
    """|y| >= 0.1 (a kept element never equals its residual); resid has y's sign, so resid + y * scale does not cancel
    and the two fp32 roundings of the kernel (product, sum: 2 x 2^-24 relative) stay inside rtol = 1e-6."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(rows, d, generator=g)
    y = torch.where(y >= 0, 0.1 + y, -0.1 + y)
    resid = torch.randn(rows, d, generator=g).abs() * torch.sign(y)
    gam = torch.rand(d, generator=g) + 0.5
    bet = torch.randn(d, generator=g)
    return y, resid, gam, bet


def _run_fwd(H, dev, y, resid, gam, bet, thr, scale, site, k, bf16=False, in_place=False):
    """-> x_out, h, mean, rstd (device views; guards checked)"""
    rows, d = y.shape
    n = rows * d
    xraw, xo = _buf(n, dev)
    yd = y.to(dev).contiguous()
    if in_place:
        xo.copy_(yd.view(-1))
        yd = xo
    hraw, h = _buf(n, dev, bf16)
    mraw, mean = _buf(rows, dev)
    rraw, rstd = _buf(rows, dev)
    rd = None if resid is None else resid.to(dev).contiguous()
    gd, bd, step = gam.to(dev), bet.to(dev), _step_buf(dev, k)          # (held until the launch has run)
    H.call("vlg_dropout_add_layernorm_fwd" + ("_bf16" if bf16 else ""), yd.data_ptr(), H.ptr(rd), gd.data_ptr(),
           bd.data_ptr(), xo.data_ptr(), h.data_ptr(), mean.data_ptr(), rstd.data_ptr(), rows, d, O.LN_EPS, thr, scale,
           SEED, site, step.data_ptr(), S())
    torch.cuda.synchronize()
    for raw, m, what in ((xraw, n, "x_out"), (hraw, n, "h"), (mraw, rows, "mean"), (rraw, rows, "rstd")):
        _guard(raw, m, "dropout fwd " + what)
    return xo.view(rows, d), h.view(rows, d), mean, rstd


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("d", DS)
def test_forward_kernel(H, dev, d, p):
    """vlg_dropout_add_layernorm_fwd, rows 1 / 5 / 259, with and without resid, site 3, step 6: the dropped set
    (x_out == resid bitwise) is EXACTLY the reference's; kept values within rtol 1e-6 of resid + y * scale (fp64);
    h, mean, rstd of the x_out the kernel formed within test_hip_layout_ops' layer-norm bounds; in place == out of place;
    the bf16 entry's h == the fp32 entry's rounded to nearest even; rows 0..4 of the 259-row launch == the 5-row launch."""
    _forward_rows(H, dev, d, p, ROWS)


def _forward_rows(H, dev, d, p, row_counts):
    """test_forward_kernel's checks at every row count of `row_counts` (ascending, 5 among them; the last one is the launch
    whose rows 0..4 are compared with the 5-row launch)"""
    thr, scale = R.plan(p)
    site, k = 3, 6
    y, resid, gam, bet = _fwd_inputs(row_counts[-1], d, seed=d + int(p * 100))
    small = {}
    for rows in row_counts:
        keep = torch.from_numpy(R.keep_mask(rows, d, site, k, SEED, thr))
        assert bool(keep.all()) == (p == 0.0)
        for with_resid in (True, False):
            yy, rr = y[:rows], (resid[:rows] if with_resid else None)
            base = rr if with_resid else torch.zeros(rows, d)
            xo, h, mean, rstd = _run_fwd(H, dev, yy, rr, gam, bet, thr, scale, site, k)
            xc = xo.cpu()
            tag = "d=%d p=%g rows=%d resid=%s: " % (d, p, rows, with_resid)
            dropped = _bits(xc) == _bits(base)
            assert torch.equal(dropped, ~keep), tag + "dropped set differs from the reference in %d elements" % int((dropped != ~keep).sum())
            want = base.double() + torch.where(keep, yy.double() * scale, torch.zeros((), dtype=torch.float64))
            check_close(xc, want, rtol=1e-6, atol=0.0, what=tag + "x_out")
            bar = _ln_bars(xc, gam, bet, torch.zeros(rows, d))
            x64 = xc.double()
            within(h, F.layer_norm(x64, (d,), gam.double(), bet.double(), O.LN_EPS), bar["y"], tag + "h")
            within(mean, x64.mean(-1), bar["mean"], tag + "mean")
            within(rstd, 1.0 / torch.sqrt(x64.var(-1, unbiased=False) + O.LN_EPS), bar["rstd"], tag + "rstd")
            got = (xo.clone(), h.clone(), mean.clone(), rstd.clone())
            again = _run_fwd(H, dev, yy, rr, gam, bet, thr, scale, site, k, in_place=True)
            for a, b, what in zip(got, again, ("x_out", "h", "mean", "rstd")):
                assert torch.equal(_bits(a), _bits(b)), tag + "in place differs: " + what
            xb, hb, mb, rb = _run_fwd(H, dev, yy, rr, gam, bet, thr, scale, site, k, bf16=True)
            assert torch.equal(_bits(xb), _bits(got[0])) and torch.equal(_bits(mb), _bits(got[2])) and torch.equal(_bits(rb), _bits(got[3]))
            assert torch.equal(hb.view(torch.int16), got[1].to(BF).view(torch.int16)), tag + "bf16 h != fp32 h rounded to nearest even"
            if rows == 5:
                small[with_resid] = got
            if rows == row_counts[-1]:
                for a, b, what in zip(small[with_resid], got, ("x_out", "h", "mean", "rstd")):
                    assert torch.equal(_bits(a), _bits(b[:5])), tag + "rows 0..4 depend on the launch geometry: " + what


PROD_DS = (64, 256, 512, 1024)            # both mask layouts (scalar below 256), LN_ROWS = 4 / 4 / 2 / 1


@pytest.mark.parametrize("d", PROD_DS)
def test_forward_kernel_prod(H, dev, d):
    """Past one trip of the row loop, as test_hip_layout_ops' "prod" cases of the plain layer-norm: 2048 blocks x 4 waves x
    LN_ROWS rows + 1003 (a second trip that ends on a short row group), p = 0.25.  Every check of test_forward_kernel;
    the point is the first: the dropped set over ALL rows is the reference's, so the Philox row counter is the global row
    in every trip (a launch-local index would pass every single-trip case)."""
    _forward_rows(H, dev, d, 0.25, (5, 2048 * 4 * _ln_R(d) + 1003))


@pytest.mark.parametrize("d", DS)
def test_forward_kernel_selects(H, dev, d):
    """inf and NaN at dropped positions of y leave x_out and h finite - and unchanged, bit for bit"""
    thr, scale = R.plan(0.5)
    y, resid, gam, bet = _fwd_inputs(259, d, seed=d)
    keep = torch.from_numpy(R.keep_mask(259, d, 1, 2, SEED, thr))
    clean = [t.clone() for t in _run_fwd(H, dev, y, resid, gam, bet, thr, scale, 1, 2)]
    poison = torch.where(torch.arange(259 * d).view(259, d) % 2 == 0, torch.tensor(float("inf")), torch.tensor(float("nan")))
    bad = torch.where(keep, y, poison)
    for in_place in (False, True):
        got = _run_fwd(H, dev, bad, resid, gam, bet, thr, scale, 1, 2, in_place=in_place)
        assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all())
        for a, b in zip(clean, got):
            assert torch.equal(_bits(a), _bits(b))


def _ulp_neighbours(t):
    return torch.nextafter(t, torch.full_like(t, -float("inf"))), torch.nextafter(t, torch.full_like(t, float("inf")))


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("d", DS)
def test_backward_kernel(H, dev, d, p):
    """vlg_layernorm_bwd_dropout (in place on dres, as the engine runs it) and its bf16-dy entry (dres = NULL): dx_out and
    every slab BITWISE equal to vlg_layernorm_bwd / _bf16 on the same inputs; dy_drop exactly 0 on the reference's
    dropped set and within 1 ulp of fp32(dx_out * scale) elsewhere."""
    _backward_rows(H, dev, d, p, [_ln_inputs(rows, d, seed=rows + d) for rows in ROWS])


def _backward_rows(H, dev, d, p, cases):
    """test_backward_kernel's checks on every (x, gamma, beta, dy, res) of `cases` -> per case {bf16 entry?: (dx_out, dy_drop)
    of the fused launch, on the CPU}"""
    lib = H.load()
    thr, scale = R.plan(p)
    site, k = 4, 9
    results = []
    for x, gam, bet, dy, res in cases:
        rows = x.shape[0]
        results.append({})
        keep = torch.from_numpy(R.keep_mask(rows, d, site, k, SEED, thr))
        n = rows * d
        xd, gd, bd = x.to(dev), gam.to(dev), bet.to(dev)
        yv, mean, rstd = torch.empty(n, device=dev), torch.empty(rows, device=dev), torch.empty(rows, device=dev)
        H.call("vlg_layernorm_fwd", xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), yv.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
               rows, d, O.LN_EPS, S())
        ns = lib.vlg_layernorm_bwd_slabs(rows)
        stride = 2 * d + 4
        step = _step_buf(dev, k)
        for bf16 in (False, True):
            tag = "d=%d p=%g rows=%d%s: " % (d, p, rows, " bf16" if bf16 else "")
            sfx = "_bf16" if bf16 else ""
            dyd = dy.to(dev).to(BF if bf16 else torch.float32)
            outs = []
            for fused in (False, True):
                sraw, slabs = _buf(ns * stride, dev)
                dxraw, dx = _buf(n, dev)
                dres = None
                if not bf16:
                    dx.copy_(res.to(dev).view(-1))
                    dres = dx
                args = [dyd.data_ptr(), xd.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gd.data_ptr(), H.ptr(dres), dx.data_ptr()]
                if fused:
                    draw, dd = _buf(n, dev)
                    H.call("vlg_layernorm_bwd_dropout" + sfx, *args, dd.data_ptr(), slabs.data_ptr(), stride, ns * stride, rows, d,
                           thr, scale, SEED, site, step.data_ptr(), S())
                else:
                    H.call("vlg_layernorm_bwd" + sfx, *args, slabs.data_ptr(), stride, ns * stride, rows, d, S())
                torch.cuda.synchronize()
                _guard(dxraw, n, tag + "dx")
                owned = torch.zeros(ns * stride + GUARD, dtype=torch.bool, device=dev)
                owned[:ns * stride].view(ns, stride)[:, :2 * d] = True
                untouched(sraw, owned, tag + "slabs")
                outs.append((dx.clone(), sraw.clone()))
            assert bool(torch.isfinite(outs[0][0]).all())
            assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0])), tag + "dx_out differs from vlg_layernorm_bwd"
            assert torch.equal(outs[0][1], outs[1][1]), tag + "slabs differ from vlg_layernorm_bwd"
            _guard(draw, n, tag + "dy_drop")
            got, dxc = dd.view(rows, d).cpu(), outs[1][0].view(rows, d).cpu()
            assert bool((_bits(got)[~keep] == 0).all()), tag + "dy_drop not exactly 0 on the dropped set"
            lo, hi = _ulp_neighbours(dxc * torch.tensor(scale, dtype=torch.float32))
            ok = (got >= lo) & (got <= hi)
            assert bool(ok[keep].all()), tag + "dy_drop off by more than 1 ulp from dx_out * scale in %d elements" % int((~ok[keep]).sum())
            results[-1][bf16] = (dxc, got)
    return results


@pytest.mark.parametrize("d", PROD_DS)
def test_backward_kernel_prod(H, dev, d):
    """Past one trip of the backward's row loop: 512 blocks (LN_BWD_MAX_BLOCKS) x 4 waves x LN_ROWS rows + 1003, p = 0.25.
    Every check of test_backward_kernel - dy_drop exactly 0 on the reference's dropped set over ALL rows, so the mask's row
    counter is the global row in every trip - and rows 0..4 of dx_out and dy_drop bitwise those of the 5-row launch on the
    same rows."""
    rows = 512 * 4 * _ln_R(d) + 1003
    assert H.load().vlg_layernorm_bwd_slabs(rows) == 512
    x, gam, bet, dy, res = _ln_inputs(rows, d, seed=rows + d)
    small, big = _backward_rows(H, dev, d, 0.25, [(x[:5], gam, bet, dy[:5], res[:5]), (x, gam, bet, dy, res)])
    for bf16 in (False, True):
        for a, b, what in zip(small[bf16], big[bf16], ("dx_out", "dy_drop")):
            assert torch.equal(_bits(a), _bits(b[:5])), "d=%d%s: rows 0..4 depend on the launch geometry: %s" % (d, " bf16" if bf16 else "", what)


def test_kernel_refusals(H, dev):
    """p out of range, rows < 1 or >= 2^32, bad d, a misaligned or NULL pointer, forbidden aliasing, a short slab buffer:
    refused with the documented code, and nothing is enqueued (every output keeps its sentinel)."""
    lib = H.load()
    thr_, scale_ = ctypes.c_uint32(), ctypes.c_float()
    for bad in (-0.5, 1.0, float("nan")):
        assert lib.vlg_dropout_plan(bad, ctypes.byref(thr_), ctypes.byref(scale_)) == ERR_SHAPE
    thr, scale = R.plan(0.25)
    rows, d = 8, 256
    n = rows * d
    bufs = {k: sentinel(n + 8, dev) for k in ("y", "resid", "x_out", "h", "dy", "x", "dres", "dx", "dd")}
    small = {k: sentinel(rows, dev) for k in ("mean", "rstd")}
    vec = {k: sentinel(d, dev) for k in ("gamma", "beta")}
    ns = lib.vlg_layernorm_bwd_slabs(rows)
    slabs = sentinel(ns * 2 * d, dev)
    step = _step_buf(dev, 0)
    P = {k: v.data_ptr() for k, v in {**bufs, **small, **vec}.items()}
    P.update(slabs=slabs.data_ptr(), step=step.data_ptr())

    def fwd(name="vlg_dropout_add_layernorm_fwd", rows=rows, d=d, scale=scale, site=0, **over):
        q = dict(P, **over)
        return getattr(lib, name)(q["y"], q["resid"], q["gamma"], q["beta"], q["x_out"], q["h"], q["mean"], q["rstd"], rows, d,
                                  O.LN_EPS, thr, scale, SEED, site, q["step"], S())

    def bwd(name="vlg_layernorm_bwd_dropout", rows=rows, d=d, cap=ns * 2 * d, site=0, **over):
        q = dict(P, **over)
        return getattr(lib, name)(q["dy"], q["x"], q["mean"], q["rstd"], q["gamma"], q["dres"], q["dx"], q["dd"], q["slabs"], 2 * d,
                                  cap, rows, d, thr, scale, SEED, site, q["step"], S())

    for name in ("vlg_dropout_add_layernorm_fwd", "vlg_dropout_add_layernorm_fwd_bf16"):
        assert fwd(name, rows=0) == ERR_SHAPE and fwd(name, rows=2 ** 32) == ERR_SHAPE
        assert fwd(name, d=100) == ERR_SHAPE and fwd(name, d=320) == ERR_SHAPE
        assert fwd(name, site=-1) == ERR_SHAPE and fwd(name, scale=0.5) == ERR_SHAPE and fwd(name, scale=float("nan")) == ERR_SHAPE
        assert fwd(name, step=0) == ERR_SHAPE
        for k in ("y", "gamma", "beta", "x_out", "h", "mean", "rstd"):
            assert fwd(name, **{k: 0}) == ERR_ALIGN, k
        for k in ("y", "resid", "gamma", "beta", "x_out", "h"):
            assert fwd(name, **{k: P[k] + 4}) == ERR_ALIGN, k
        assert fwd(name, x_out=P["resid"]) == ERR_SHAPE                  # only y may be written in place
        assert fwd(name, h=P["y"]) == ERR_SHAPE and fwd(name, h=P["x_out"]) == ERR_SHAPE and fwd(name, h=P["resid"]) == ERR_SHAPE
        assert fwd(name, resid=P["y"]) == ERR_SHAPE
        assert fwd(name, x_out=P["y"] + 16) == ERR_SHAPE                 # a partial overlap is not "in place"
    for name in ("vlg_layernorm_bwd_dropout", "vlg_layernorm_bwd_dropout_bf16"):
        assert bwd(name, rows=0) == ERR_SHAPE and bwd(name, rows=2 ** 32) == ERR_SHAPE and bwd(name, d=100) == ERR_SHAPE
        assert bwd(name, cap=ns * 2 * d - 1) == ERR_SHAPE and bwd(name, site=-1) == ERR_SHAPE and bwd(name, step=0) == ERR_SHAPE
        for k in ("dy", "x", "mean", "rstd", "gamma", "dx", "dd", "slabs"):
            assert bwd(name, **{k: 0}) == ERR_ALIGN, k
        for k in ("dy", "x", "gamma", "dres", "dx", "dd"):
            assert bwd(name, **{k: P[k] + 4}) == ERR_ALIGN, k
        for k in ("dx", "dy", "x", "dres"):
            assert bwd(name, dd=P[k]) == ERR_SHAPE, k                    # dy_drop overlaps nothing
        assert bwd(name, dx=P["x"]) == ERR_SHAPE and bwd(name, dres=P["dx"] + 16) == ERR_SHAPE
    assert lib.vlg_dropout_step_advance(0, S()) == ERR_ALIGN
    torch.cuda.synchronize()
    for k, v in {**bufs, **small, **vec, "slabs": slabs}.items():
        assert bool((v == SENT).all()), "a refused call wrote " + k
    assert int(step.item()) == 0
    # and the calls the refusals were derived from are accepted
    f32(vec["gamma"]).fill_(1.0)
    for k in ("y", "resid", "dy", "x", "dres", "beta", "mean", "rstd"):
        f32({**bufs, **small, **vec}[k]).zero_()
    assert fwd() == 0 and fwd(x_out=P["y"]) == 0 and fwd(resid=0) == 0 and bwd() == 0 and bwd(dres=P["dx"]) == 0 and bwd(dres=0) == 0
    assert lib.vlg_dropout_step_advance(P["step"], S()) == 0
    torch.cuda.synchronize()
    assert int(step.item()) == 1


# ---------------------------------------------------------------------------------------------------------------- engine
KW = dict(B=2, T=16, N=16, d=256, n_layers=2)
PROB, ENG_SEED = 0.25, 77


def _cfg(attention="slot"):
    from vlg.spec import LayoutConfig
    return LayoutConfig(attention=attention, **KW)


def _engine(dev, precision="fp32", attention="slot", variable_n=False, **kw):
    from vlg.engine import LayoutEngine
    return LayoutEngine(_cfg(attention), dev, seed=1024, precision=precision, padded_slots=variable_n, **kw)


def _batch(variable_n=False, seed=7):
    return O.synthetic_batch(KW["B"], KW["T"], KW["N"], seed=seed, variable_n=variable_n, min_valid=3)


def to_dev(batch, dev):
    return {k: v.to(dev) for k, v in batch.items()}


@functools.lru_cache(maxsize=None)
def _reference(attention, variable_n, k):
    """dropout_ref's fp64 model at dropout step k: (loss parts, grads, logits, raw boxes), computed once per case"""
    from vlg.spec import param_shapes
    p = O.init_params(param_shapes(_cfg(attention)), seed=1024)
    return R.loss_and_grads(R.to64(p), R.to64(_batch(variable_n)), KW["n_layers"], PROB, k, ENG_SEED, attention=attention)


def _step_vs_reference_fp32(dev, precision, attention, variable_n, k=3):
    eng = _engine(dev, precision, attention, variable_n, dropout=PROB, dropout_seed=ENG_SEED)
    eng.set_dropout_step(k)
    parts, grads, logits, box_raw = _reference(attention, variable_n, k)
    loss = eng.forward_backward(to_dev(_batch(variable_n), dev))
    assert eng.dropout_step == k + 1
    check_close(loss, torch.tensor(parts), rtol=1e-4, atol=1e-6, what="loss parts")
    gl, gb = eng.outputs_btn()
    check_close(gl, logits, rtol=1e-4, atol=1e-4, what="logits")
    check_close(gb, box_raw, rtol=1e-4, atol=1e-4, what="box outputs")
    for name, g in eng.named_grads().items():
        scale = max(float(grads[name].abs().max()), 1e-6)
        check_close(g / scale, grads[name] / scale, rtol=1e-4, atol=2e-5, what="grad " + name)


@pytest.mark.parametrize("attention,variable_n", [("slot", False), ("clip", True)])
def test_engine_fp32_matches_reference(dev, attention, variable_n):
    """p = 0.25: loss parts, logits, box outputs and every gradient against dropout_ref's fp64 model with the masks of the
    counter value the step read, at test_step_matches_oracle's bars (1e-4, gradients scaled by their maximum)."""
    _step_vs_reference_fp32(dev, "fp32", attention, variable_n)


def test_engine_fp32x3_matches_reference(dev):
    """the same bars for fp32x3, which also runs the plain one-stream backward (no paired launches)"""
    _step_vs_reference_fp32(dev, "fp32x3", "slot", False)


def test_engine_plain_backward_equals_paired(dev, monkeypatch):
    """VLG_PAIR_BACKWARD=0 (separate weight- and data-gradient launches) gives the paired backward's gradients bit for bit"""
    b = to_dev(_batch(), dev)
    eng = _engine(dev, dropout=PROB, dropout_seed=ENG_SEED)
    eng.forward_backward(b)
    want = eng.grads.clone()
    monkeypatch.setenv("VLG_PAIR_BACKWARD", "0")
    plain = _engine(dev, dropout=PROB, dropout_seed=ENG_SEED)
    assert not plain.pair_backward
    plain.forward_backward(b)
    assert torch.equal(plain.grads, want)


K_MODES = 0      # the dropout step of the reduced-precision cases (a fresh engine's); see test_engine_bf16_matches_reference


@pytest.mark.parametrize("precision,attention,variable_n", [("bf16", "slot", False), ("bf16", "clip", True), ("bf16_mfma", "slot", False)])
def test_engine_bf16_matches_reference(dev, precision, attention, variable_n):
    """The bf16 modes against the same fp64 reference, at step_stages.end_to_end_bars for this shape and mode (loss
    relative, gradient tensors relative L2, as test_bf16_projection_mode applies them): dropout adds one fp32 select and one
    multiply, and no new rounding of stored tensors.
    Those bars are 4 x the mode's distance measured WITHOUT dropout.  Under dropout the MODE ITSELF - dropout_ref's CPU
    emulation of its roundings, no kernel involved - is bimodal in the masks: with 512 tokens, at most steps every tensor
    lies near 0.3 of its bar, and at the others one min / max branch of the loss goes the other way under the mode's
    rounding and every tensor moves by about 1e-2 (CPU, slot attention, p = 0.25, seed 77, worst tensor / bar at steps
    0..7: bf16 0.31 0.30 0.38 1.76 0.29 0.29 0.29 2.91; bf16_mfma 0.33 1.55 0.29 1.15 0.29 4.05 0.29 1.96).  At such a step
    no kernel can meet the bar (the engine measured 1.78 and 1.16 at step 3, the emulation's 1.76 and 1.15).  The issue
    leaves step and seed to the test, so the case is the step a fresh engine reads, 0, and the test first asserts ON THE
    CPU that the mode's own distance under these masks is within half of every bar: the bars then measure the kernels.
    (Per-clip attention under "bf16" also rounds P and dS, which the emulation does not model: no such precondition there.)"""
    k = K_MODES
    from vlg.spec import param_shapes
    bar_loss, bar_grad, _ = SS.end_to_end_bars(KW, precision, attention, variable_n, seed=7)
    if attention == "slot":
        p = O.init_params(param_shapes(_cfg(attention)), seed=1024)
        own = R.mode_distance(R.to64(p), R.to64(_batch(variable_n)), KW["n_layers"], PROB, k, ENG_SEED, precision, attention)
        worst = max(bar_grad, key=lambda n: own[n] / bar_grad[n])
        assert own[worst] <= 0.5 * bar_grad[worst], "the mode itself is at %.2f of %s's bar under these masks" % (own[worst] / bar_grad[worst], worst)
    eng = _engine(dev, precision, attention, variable_n, dropout=PROB, dropout_seed=ENG_SEED)
    eng.set_dropout_step(k)
    parts, grads, _, _ = _reference(attention, variable_n, k)
    loss = eng.forward_backward(to_dev(_batch(variable_n), dev)).cpu()
    errs = {n: float((g.cpu().double() - grads[n]).norm() / grads[n].norm()) for n, g in eng.named_grads().items() if n in bar_grad}
    print("\n%s %s dropout: loss off by %.2e (bar %.2e); gradients (rel L2 / bar): %s" % (
        precision, attention, abs(float(loss[0]) - parts[0]) / abs(parts[0]), bar_loss,
        ", ".join("%s %.1e/%.1e" % (n, e, bar_grad[n]) for n, e in errs.items())))
    assert bool(torch.isfinite(eng.grads).all())
    assert abs(float(loss[0]) - parts[0]) <= bar_loss * abs(parts[0]), (float(loss[0]), parts[0], bar_loss)
    assert len(errs) >= len(grads) - 2 * KW["n_layers"]
    for name, err in errs.items():
        assert err <= bar_grad[name], (name, err, bar_grad[name])


@pytest.mark.parametrize("precision", ["bf16", "bf16_mfma"])
def test_engine_computes_the_mode_where_the_mode_misses_the_bar(dev, precision):
    """Step 3 of the same case is one where the mode itself lies OUTSIDE the no-dropout bars (docstring above).  There the
    engine must still compute the mode: every gradient within the bar of dropout_ref's CPU emulation of the mode under
    the same masks: the engine against its own mode, which no branch of the loss separates."""
    from vlg.spec import param_shapes
    k = 3
    _, bar_grad, _ = SS.end_to_end_bars(KW, precision, "slot", False, seed=7)
    p = R.to64(O.init_params(param_shapes(_cfg()), seed=1024))
    _, emu, _, _ = R.loss_and_grads(p, R.to64(_batch()), KW["n_layers"], PROB, k, ENG_SEED, mode=precision)
    _, exact, _, _ = _reference("slot", False, k)
    own = float((emu["head_b"] - exact["head_b"]).norm() / exact["head_b"].norm())
    assert own > bar_grad["head_b"], "step %d is no longer a step at which the mode itself misses head_b's bar" % k
    eng = _engine(dev, precision, dropout=PROB, dropout_seed=ENG_SEED)
    eng.set_dropout_step(k)
    eng.forward_backward(to_dev(_batch(), dev))
    got = {n: g.cpu().double() for n, g in eng.named_grads().items()}
    for n in bar_grad:
        err = float((got[n] - emu[n]).norm() / emu[n].norm())
        assert err <= bar_grad[n], (n, err, bar_grad[n])


def _x0_dropped(eng, M):
    return (eng.x[0][:M] == 0).cpu()


def test_counter_advances_and_reproduces(dev):
    """two consecutive training steps read k and k + 1 (their x[0] dropped sets are the reference's for those steps, and
    differ); set_dropout_step(k) on the same parameters reproduces a step bitwise; the counter also advances when the
    guarded optimiser skips the step."""
    b = to_dev(_batch(), dev)
    M, d = KW["B"] * KW["T"] * KW["N"], KW["d"]
    thr, _ = R.plan(PROB)
    eng = _engine(dev, dropout=PROB, dropout_seed=ENG_SEED)
    assert eng.dropout_step == 0
    sets = []
    for k in (0, 1):
        eng.forward_backward(b)
        assert eng.dropout_step == k + 1
        sets.append(_x0_dropped(eng, M))
        assert torch.equal(sets[-1], torch.from_numpy(~R.keep_mask(M, d, 0, k, ENG_SEED, thr))), "x[0] dropped set at step %d" % k
    assert not torch.equal(sets[0], sets[1])
    g1, l1 = eng.grads.clone(), eng.loss_out.clone()
    eng.set_dropout_step(1)
    eng.forward_backward(b)
    assert torch.equal(eng.grads, g1) and torch.equal(eng.loss_out, l1)
    with pytest.raises(ValueError):
        eng.set_dropout_step(-1)
    guarded = _engine(dev, dropout=PROB, dropout_seed=ENG_SEED, skip_nonfinite=True)
    before = guarded.params.clone()
    bad = dict(b, slot_box=torch.full_like(b["slot_box"], float("nan")))
    guarded.train_step(bad)
    assert torch.equal(guarded.params, before) and guarded.dropout_step == 1


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_captured_step_replays_like_eager_steps(dev, precision):
    """a captured step replayed 3 times == 3 eager steps, bitwise: parameters, loss and the counter"""
    b = to_dev(_batch(), dev)
    eager = _engine(dev, precision, dropout=PROB, dropout_seed=ENG_SEED)
    for _ in range(3):
        eager.train_step(b)
    want_loss = eager.loss_out.clone()
    graph = _engine(dev, precision, dropout=PROB, dropout_seed=ENG_SEED)
    run = graph.capture_train_step(b)
    assert graph.dropout_step == 0                                   # capture does not move the trajectory
    for _ in range(3):
        run(b)
    torch.cuda.synchronize()
    assert graph.dropout_step == 3 == eager.dropout_step
    assert torch.equal(graph.params, eager.params) and torch.equal(graph.loss_out, want_loss)
    assert torch.equal(graph.exp_avg, eager.exp_avg)


def test_state_dict_carries_the_counter(dev):
    b = to_dev(_batch(), dev)
    eng = _engine(dev, dropout=PROB, dropout_seed=ENG_SEED)
    for _ in range(2):
        eng.train_step(b)
    sd = eng.state_dict()
    assert sd["dropout_step"] == 2
    other = _engine(dev, dropout=PROB, dropout_seed=ENG_SEED)
    other.load_state_dict(sd)
    assert other.dropout_step == 2
    eng.train_step(b)
    other.train_step(b)
    assert torch.equal(other.params, eng.params) and torch.equal(other.loss_out, eng.loss_out)
    off = _engine(dev)
    assert "dropout_step" not in off.state_dict() and set(off.state_dict()) == set(sd) - {"dropout_step"}
    with pytest.raises(RuntimeError):
        off.dropout_step


def test_evaluation_is_untouched(dev):
    """a bare forward(), rollout() and accumulate_metrics() on an engine with dropout = 0.25 equal an engine built with
    dropout = 0 on the same parameters, bit for bit, and do not move the counter"""
    b = to_dev(_batch(), dev)
    on, off = _engine(dev, dropout=PROB, dropout_seed=ENG_SEED), _engine(dev)
    assert torch.equal(on.params, off.params)
    assert torch.equal(on.forward(b), off.forward(b)) and torch.equal(on.out, off.out)
    recs = []
    for e in (on, off):
        rec = e.metrics_record()
        e.accumulate_metrics(b, rec)
        recs.append(rec)
    assert torch.equal(recs[0].counts, recs[1].counts) and torch.equal(recs[0].sums, recs[1].sums)
    ga, gb = on.rollout(b["slot_class"], b["slot_box"], steps=2), off.rollout(b["slot_class"], b["slot_box"], steps=2)
    assert torch.equal(ga[0], gb[0]) and torch.equal(ga[1], gb[1])
    assert on.dropout_step == 0
    on.forward_backward(b)                                           # and the training entry point does drop
    off.forward_backward(b)
    assert not torch.equal(on.out, off.out) and on.dropout_step == 1


def test_knob_off_is_the_engine_without_the_argument(dev):
    b = to_dev(_batch(), dev)
    a, c = _engine(dev, dropout=0.0), _engine(dev)
    for e in (a, c):
        for _ in range(2):
            e.train_step(b)
    assert torch.equal(a.params, c.params) and torch.equal(a.loss_out, c.loss_out) and torch.equal(a.exp_avg_sq, c.exp_avg_sq)
    assert a.drop_step is None and not hasattr(a, "ybranch") and not hasattr(a, "ddrop")      # nothing new allocated


def test_engine_refusals(dev, monkeypatch):
    for bad in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="dropout"):
            _engine(dev, dropout=bad)
    monkeypatch.setenv("VLG_OVERLAP_WGRAD", "1")
    with pytest.raises(ValueError, match="VLG_OVERLAP_WGRAD.*dropout"):
        _engine(dev, dropout=0.1)
    _engine(dev)                                                     # the option alone is still accepted
