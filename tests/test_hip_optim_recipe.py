"""GPU: the training recipe on the guarded optimiser step - vlg_optim_control_ext and vlg_adamw_ema_step_ctl
(csrc/optim.hip: decoupled weight decay under a float4 mask, warm-up in applied steps, the weights' moving average) bit for
bit against the guarded pair where the header claims it and against the fp64 restatement (optim_recipe_ref.py, pinned to
torch.optim.AdamW by test_optim_recipe_cpu.py) everywhere else; then the engines' and the Trainer's use of them.

Tolerances against fp64 are those of test_hip_optim_guard.test_adam_ctl_clipped_matches_torch (rtol 1e-6, atol 1e-7): the
recipe adds one rounded multiplication before Adam's update and three fp32 operations for the average, each 2^-24 relative."""
import contextlib
import math
import os
import socket
import sys
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import optim_recipe_ref as R
from conftest import PKG, ROOT
from helpers import check_close, reference_args
from oracle import layout_spec as O
# slots of the records (VLG_CTL_* / VLG_EXT_* in include/vlg_hip.h)
from vlg.optim import APPLY, CLIP_COEF, GRAD_MULT, GRAD_NORM, LR as LR_SLOT, SKIPPED, SQRT_BC2, STEP, STEP_SIZE
from vlg.optim import (EXT_DECAY_MULT as X_DECAY_MULT, EXT_EMA_DECAY as X_EMA, EXT_EMA_OMD as X_EMA_OMD,
                       EXT_EMA_WARMUP as X_EMA_WARMUP, EXT_LR_EFF as X_LR_EFF, EXT_WARMUP_STEPS as X_WARMUP,
                       EXT_WEIGHT_DECAY as X_WD)

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
f32 = lambda x: float(np.float32(x))
LR, B1, B2, EPS = f32(2e-4), 0.5, f32(0.999), f32(1e-8)            # as the kernels see them: floats widened to double
WD, WARMUP, EMA_D = f32(0.1), 5, 0.5
RTOL, ATOL = 1e-6, 1e-7
CTL_MARK, EXT_MARK, OUT_MARK = -9.0, -3.0, -5.0                      # reserved slots / not-yet-written outputs
FULL = dict(weight_decay=WD, warmup_steps=WARMUP, ema_decay=EMA_D, ema_warmup=True)


@pytest.fixture(scope="module")
def H():
    from vlg import hip
    hip.load()
    return hip


def stream():
    return torch.cuda.current_stream().cuda_stream


def to_dev(batch, dev):
    return {k: v.to(dev) for k, v in batch.items()}


def new_ctl(dev, lr=LR, step=0, skipped=0):
    host = torch.zeros(16)
    host[9:] = CTL_MARK
    host[LR_SLOT] = lr
    host[CLIP_COEF] = 1.0
    host.view(torch.int32)[STEP] = step
    host.view(torch.int32)[SKIPPED] = skipped
    return host.to(dev)


def new_ext(dev, wd=0.0, warmup=0, ema=0.0, ema_warmup=0):
    host = torch.full((16,), EXT_MARK)
    host[X_LR_EFF:X_EMA_OMD + 1] = OUT_MARK
    host[X_WD], host[X_EMA] = wd, ema
    host.view(torch.int32)[X_WARMUP] = warmup
    host.view(torch.int32)[X_EMA_WARMUP] = ema_warmup
    return host.to(dev)


def dptr(t, off=0):
    return 0 if t is None else t.data_ptr() + off


def sumsq(H, g):
    n = g.numel()
    P = H.load().vlg_grad_sumsq_blocks(n)
    part = torch.zeros(P, device=g.device)
    H.call("vlg_grad_sumsq", g.data_ptr(), n, part.data_ptr(), stream())
    return part, P


def guarded_step(H, p, g, m, v, sh, ctl, grad_scale=1.0, max_norm=0.0):
    """the parent pair: vlg_optim_control + vlg_adam_step_ctl"""
    part, P = sumsq(H, g)
    H.call("vlg_optim_control", ctl.data_ptr(), part.data_ptr(), P, grad_scale, max_norm, B1, B2, stream())
    H.call("vlg_adam_step_ctl", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), dptr(sh), p.numel(), ctl.data_ptr(),
           B1, B2, EPS, stream())


def recipe_step(H, p, g, m, v, sh, ema, esh, mask, ctl, ext, grad_scale=1.0, max_norm=0.0):
    """the new pair: vlg_optim_control_ext + vlg_adamw_ema_step_ctl"""
    part, P = sumsq(H, g)
    H.call("vlg_optim_control_ext", ctl.data_ptr(), ext.data_ptr(), part.data_ptr(), P, grad_scale, max_norm, B1, B2, stream())
    H.call("vlg_adamw_ema_step_ctl", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), dptr(sh), dptr(ema), dptr(esh),
           dptr(mask), p.numel(), ctl.data_ptr(), ext.data_ptr(), B1, B2, EPS, stream())


def two_trip_n(H):
    """test_hip_optim_guard.two_trip_n's kind: every block of the largest grid (2048 blocks of 256 lanes, the cap the Adam
    kernels share with vlg_grad_sumsq) makes more than one grid-stride trip, and the last trip is partial"""
    lib = H.load()
    p_max = lib.vlg_grad_sumsq_blocks(1 << 40)
    assert p_max == 2048
    n = 4 * (2 * p_max * 256 + 259)
    assert lib.vlg_grad_sumsq_blocks(n) == p_max
    return n


def size_of(H, n):
    return two_trip_n(H) if n == "two_trips" else n


TRIP = 2048 * 256                                                   # float4 index at which the second grid-stride trip starts


def make_mask(kind, n4, seed=0):
    idx = torch.arange(n4)
    if kind == "zero":
        return torch.zeros(n4, dtype=torch.uint8)
    if kind == "one":
        return torch.ones(n4, dtype=torch.uint8)
    if kind == "alternating":
        return (idx % 2).to(torch.uint8)
    if kind == "random":                                            # non-zero bytes of any value mark a float4
        g = torch.Generator().manual_seed(seed)
        return (torch.randint(0, 2, (n4,), generator=g) * torch.randint(1, 256, (n4,), generator=g)).to(torch.uint8)
    # runs that change at the wave edge 63|64, the block edge 255|256 and the first | second trip edge
    runs = ((idx < 64) | ((idx >= 256) & (idx < TRIP))).to(torch.uint8)
    return runs if kind == "runs" else 1 - runs


def fresh_state(n, dev, seed, bf16=True):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g).to(dev)
    m = (torch.randn(n, generator=g) * 0.1).to(dev)
    v = (torch.rand(n, generator=g) * 0.01).to(dev)
    grad = torch.randn(n, generator=g).to(dev)
    return p, m, v, (p.to(BF) if bf16 else None), grad


# ------------------------------------------------------------------------------------------------- bit for bit
@pytest.mark.parametrize("max_norm", [0.0, 1.0], ids=["noclip", "clip"])
@pytest.mark.parametrize("n", [4, 4 * 257, "two_trips"])
def test_new_pair_with_everything_off_is_bitwise_the_guarded_pair(H, dev, n, max_norm):
    """decay_mask NULL, ema NULL, WARMUP_STEPS 0, wd 0: param, both moments, shadow and every ctl slot equal those of
    vlg_optim_control + vlg_adam_step_ctl over two steps; the reserved slots of both records stay as the host left them"""
    n = size_of(H, n)
    p, m, v, sh, g = fresh_state(n, dev, 1)
    ours = [t.clone() for t in (p, m, v, sh)]
    ctl_a, ctl_b, ext = new_ctl(dev), new_ctl(dev), new_ext(dev)
    for step in (1, 2):
        guarded_step(H, p, g, m, v, sh, ctl_a, 0.5, max_norm)
        recipe_step(H, ours[0], g, *ours[1:], None, None, None, ctl_b, ext, 0.5, max_norm)
        for a, b in zip((p, m, v, sh), ours):
            assert torch.equal(a, b), step
        assert torch.equal(ctl_a.view(torch.int32), ctl_b.view(torch.int32)), step
    assert torch.equal(ctl_b[9:].cpu(), torch.full((7,), CTL_MARK))
    e = ext.cpu()
    assert torch.equal(e[7:], torch.full((9,), EXT_MARK))
    assert e[X_LR_EFF].numpy() == np.float32(LR) and float(e[X_DECAY_MULT]) == 1.0 and float(e[X_EMA_OMD]) == 1.0
    if max_norm > 0.0 and n > 4:
        assert float(ctl_b[CLIP_COEF]) < 1.0


@pytest.mark.parametrize("n,kind", [(4, "zero"), (4, "one"), (4 * 257, "alternating"), (4 * 257, "random"), (4 * 257, "runs"),
                                    ("two_trips", "zero"), ("two_trips", "one"), ("two_trips", "alternating"),
                                    ("two_trips", "random"), ("two_trips", "runs"), ("two_trips", "runs_inverted")])
def test_mask_and_average_touch_only_what_they_should(H, dev, n, kind):
    """One step with the mask, the average and both shadows against a twin run through the parent pair.  Unmarked float4s are
    bitwise the no-decay result; marked ones are bitwise the parent's result on p * DECAY_MULT (one rounded multiplication
    before the update); the moments do not depend on the mask; the average changes no bit of param, moments or shadow."""
    n = size_of(H, n)
    p, m, v, sh, g = fresh_state(n, dev, 2)
    mask4 = make_mask(kind, n // 4)
    mask = mask4.to(dev)
    marked = torch.repeat_interleave(mask4 != 0, 4).to(dev)
    plain = [t.clone() for t in (p, m, v, sh)]
    ctl_a, ctl_b, ext = new_ctl(dev), new_ctl(dev), new_ext(dev, wd=WD, ema=EMA_D)
    # an average near the weights, as training keeps it: p - e is rounded to 2^-24 |p - e|, so the bars below (atol 1e-7)
    # presuppose |p - e| well under 1; an average unrelated to the weights would need atol ~ 2^-24 max |p - e| = 5e-7
    ema = p + (0.01 * torch.randn(n, generator=torch.Generator().manual_seed(3))).to(dev)
    esh = torch.zeros(n, device=dev, dtype=BF)
    ema0 = ema.clone()
    recipe_step(H, p, g, m, v, sh, ema, esh, mask, ctl_b, ext, 1.0, 1.0)
    guarded_step(H, *plain[:1], g, *plain[1:], ctl_a, 1.0, 1.0)
    dm = ext[X_DECAY_MULT:X_DECAY_MULT + 1].clone()
    assert dm.cpu().numpy()[0] == np.float32(1.0 - LR * WD)
    assert torch.equal(m, plain[1]) and torch.equal(v, plain[2])
    assert torch.equal(p[~marked], plain[0][~marked]) and torch.equal(sh[~marked], plain[3][~marked])
    # the decayed twin: the same state with p * DECAY_MULT written by torch in fp32, stepped by the parent Adam kernel
    twin = fresh_state(n, dev, 2)
    twin[0].mul_(dm)
    ctl_c = new_ctl(dev)
    guarded_step(H, twin[0], g, twin[1], twin[2], twin[3], ctl_c, 1.0, 1.0)
    assert torch.equal(p[marked], twin[0][marked]) and torch.equal(sh[marked], twin[3][marked])
    if bool(marked.any()):
        assert not torch.equal(p[marked], plain[0][marked])
    assert torch.equal(sh, p.to(BF)) and torch.equal(esh, ema.to(BF))
    want = ema0.double() + 0.5 * (p.double() - ema0.double())
    check_close(ema, want.float(), rtol=RTOL, atol=ATOL, what="average")


# ------------------------------------------------------------------------------------ against the fp64 restatement
@pytest.mark.parametrize("n", [4, 4 * 257, "two_trips"])
def test_ten_steps_match_the_fp64_restatement(H, dev, n):
    """wd 0.1, clipping on, warm-up 5, EMA 0.5 with warm-up, random mask: each of 10 steps is checked from the device's own
    state before it.  The three output slots of ext equal the restatement's doubles rounded to float."""
    n = size_of(H, n)
    p, m, v, sh, _ = fresh_state(n, dev, 4)
    m.zero_()
    v.zero_()
    mask4 = make_mask("random", n // 4, seed=9)
    if n // 4 > TRIP:
        mask4[TRIP - 1], mask4[TRIP] = 1, 0                         # a run boundary at the trip edge
    mask = mask4.to(dev)
    ema, esh = p.clone(), p.to(BF)
    ctl, ext = new_ctl(dev), new_ext(dev, WD, WARMUP, EMA_D, 1)
    state = {"step": 0, "skipped": 0}
    gen = torch.Generator().manual_seed(10)
    max_norm = 0.5 * math.sqrt(n)                                  # about half the norm of a unit-variance gradient
    kw = dict(lr=LR, beta1=B1, beta2=B2, eps=EPS, max_norm=max_norm, weight_decay=WD, warmup_steps=WARMUP, ema_decay=EMA_D,
              ema_warmup=True, mask4=mask4.numpy())
    clipped = 0
    for step in range(1, 11):
        g = torch.randn(n, generator=gen) * (10.0 ** (step % 3 - 1))
        before = [t.cpu().numpy() for t in (p, m, v, ema)]
        recipe_step(H, p, g.to(dev), m, v, sh, ema, esh, mask, ctl, ext, 1.0, max_norm)
        wp, wm, wv, we, state, info = R.recipe_step(before[0], g.numpy(), before[1], before[2], before[3], state, **kw)
        e, c = ext.cpu(), ctl.cpu()
        assert int(c.view(torch.int32)[STEP]) == step == state["step"]
        for slot, key in ((X_LR_EFF, "lr_eff"), (X_DECAY_MULT, "decay_mult"), (X_EMA_OMD, "ema_omd")):
            assert e[slot].numpy() == np.float32(info[key]), (step, key, float(e[slot]), info[key])
        assert c[STEP_SIZE].numpy() == np.float32(info["step_size"]), step
        assert abs(float(c[CLIP_COEF]) - info["clip_coef"]) <= 1e-5 * info["clip_coef"]
        clipped += info["clip_coef"] < 1.0
        for got, want, what in ((p, wp, "param"), (m, wm, "exp_avg"), (v, wv, "exp_avg_sq"), (ema, we, "average")):
            check_close(got, torch.from_numpy(want).float(), rtol=RTOL, atol=ATOL, what="%s, step %d" % (what, step))
        assert torch.equal(sh, p.to(BF)) and torch.equal(esh, ema.to(BF)), step
    assert clipped >= 1
    assert float(ext[X_LR_EFF]) == LR and float(ext[X_EMA_OMD]) == 0.5      # past the warm-up of both


# ------------------------------------------------------------------------------------------------------- skip
@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_skip_touches_nothing_and_does_not_advance_the_warmup(H, dev, bad):
    n = 4 * 257
    p, m, v, sh, g = fresh_state(n, dev, 5)
    ema, esh = torch.randn(n, device=dev), torch.randn(n, device=dev).to(BF)
    mask = make_mask("alternating", n // 4).to(dev)
    ctl, ext = new_ctl(dev), new_ext(dev, WD, WARMUP, EMA_D, 1)
    keep = [t.clone() for t in (p, m, v, sh, ema, esh, ext)]
    gb = g.clone()
    gb[n // 2] = bad
    recipe_step(H, p, gb, m, v, sh, ema, esh, mask, ctl, ext, 1.0, 1.0)
    for a, b in zip((p, m, v, sh, ema, esh), keep):
        assert torch.equal(a.view(torch.int16) if a.dtype == BF else a, b.view(torch.int16) if b.dtype == BF else b)
    assert torch.equal(ext.view(torch.int32), keep[6].view(torch.int32))          # outputs still hold their sentinels
    i = ctl.cpu().view(torch.int32)
    assert (int(i[STEP]), int(i[APPLY]), int(i[SKIPPED])) == (0, 0, 1)
    recipe_step(H, p, g, m, v, sh, ema, esh, mask, ctl, ext, 1.0, 1.0)             # the next finite step is warm-up step 1
    e, i = ext.cpu(), ctl.cpu().view(torch.int32)
    assert (int(i[STEP]), int(i[APPLY]), int(i[SKIPPED])) == (1, 1, 1)
    s = R.scalars(1, LR, B1, B2, WD, WARMUP, EMA_D, True)
    assert e[X_LR_EFF].numpy() == np.float32(s["lr_eff"]) and abs(float(e[X_LR_EFF]) - LR / WARMUP) < 1e-9
    assert e[X_EMA_OMD].numpy() == np.float32(1.0 - 2.0 / 11.0) and e[X_DECAY_MULT].numpy() == np.float32(s["decay_mult"])
    out = [t.clone() for t in (p, ema, ext)]
    recipe_step(H, p, gb, m, v, sh, ema, esh, mask, ctl, ext, 1.0, 1.0)            # skipped again, after an applied step
    assert torch.equal(p, out[0]) and torch.equal(ema, out[1]) and torch.equal(ext.view(torch.int32), out[2].view(torch.int32))
    assert int(ctl.cpu().view(torch.int32)[SKIPPED]) == 2


# ----------------------------------------------------------------------------------------------- bad arguments
def test_bad_arguments_are_refused_and_enqueue_nothing(H, dev):
    n = 64
    bufs = [torch.full((n,), 7.0, device=dev) for _ in range(5)]               # param, grad, moments, ema
    p, g, m, v, ema = bufs
    sh, esh = torch.full((n,), 7.0, device=dev, dtype=BF), torch.full((n,), 7.0, device=dev, dtype=BF)
    mask = torch.ones(n // 4 + 4, dtype=torch.uint8, device=dev)
    ctl, ext = new_ctl(dev), new_ext(dev, WD, 0, EMA_D, 0)
    ctl.view(torch.int32)[APPLY] = 1                                         # a launch that got through WOULD write
    ctl[STEP_SIZE], ctl[SQRT_BC2], ctl[GRAD_MULT] = 0.1, 1.0, 1.0
    part = torch.ones(4, device=dev)

    def adamw(pp=0, gg=0, mm=0, vv=0, s=0, e=0, es=0, mk=0, nn=n, c=0, x=0, no_ema=False, no_ctl=False, no_ext=False):
        H.call("vlg_adamw_ema_step_ctl", p.data_ptr() + pp, g.data_ptr() + gg, m.data_ptr() + mm, v.data_ptr() + vv,
               sh.data_ptr() + s, 0 if no_ema else ema.data_ptr() + e, esh.data_ptr() + es, mask.data_ptr() + mk, nn,
               0 if no_ctl else ctl.data_ptr() + c, 0 if no_ext else ext.data_ptr() + x, B1, B2, EPS, stream())

    for kw in (dict(nn=0), dict(nn=6), dict(nn=-4), dict(no_ema=True), dict(no_ctl=True), dict(no_ext=True)):
        with pytest.raises(H.HipError, match="VLG_ERR_SHAPE"):
            adamw(**kw)
    for kw in (dict(pp=4), dict(gg=4), dict(mm=4), dict(vv=4), dict(e=4), dict(c=4), dict(x=4), dict(s=2), dict(es=2), dict(mk=1)):
        with pytest.raises(H.HipError, match="VLG_ERR_ALIGN"):
            adamw(nn=8, **kw)
    for nparts in (0, 2049):
        with pytest.raises(H.HipError, match="VLG_ERR_SHAPE"):
            H.call("vlg_optim_control_ext", ctl.data_ptr(), ext.data_ptr(), part.data_ptr(), nparts, 1.0, 0.0, B1, B2, stream())
    with pytest.raises(H.HipError, match="VLG_ERR_SHAPE"):
        H.call("vlg_optim_control_ext", ctl.data_ptr(), 0, part.data_ptr(), 4, 1.0, 0.0, B1, B2, stream())
    for c, x in ((4, 0), (0, 4)):
        with pytest.raises(H.HipError, match="VLG_ERR_ALIGN"):
            H.call("vlg_optim_control_ext", ctl.data_ptr() + c, ext.data_ptr() + x, part.data_ptr(), 4, 1.0, 0.0, B1, B2, stream())
    torch.cuda.synchronize()
    for t in bufs:
        assert torch.equal(t, torch.full((n,), 7.0, device=dev))
    assert torch.equal(sh, torch.full((n,), 7.0, device=dev, dtype=BF)) and torch.equal(esh, sh)
    assert torch.equal(ext.cpu()[X_LR_EFF:], new_ext(dev).cpu()[X_LR_EFF:])    # no control kernel ran either
    adamw(mk=4)                                                              # a mask at a 4-byte offset is accepted
    torch.cuda.synchronize()
    assert bool((p != 7.0).all()) and bool((ema != 7.0).all())


# -------------------------------------------------------------------------------------------------- layout engine
SMALL = dict(B=2, T=4, N=3, d=64, n_layers=1)                    # test_hip_optim_guard's engine configuration


def small_engine(dev, precision="fp32", **kw):
    from vlg.engine import LayoutEngine
    from vlg.spec import LayoutConfig
    return LayoutEngine(LayoutConfig(**SMALL), dev, seed=1024, precision=precision, **kw)


def small_batch(dev, seed):
    return to_dev(O.synthetic_batch(SMALL["B"], SMALL["T"], SMALL["N"], seed=seed), dev)


def restate(params, grads, exp_avg, exp_avg_sq, ema, mask, state, clip, lr=LR):
    """the fp64 restatement on an engine's flat device buffers as they were before the step"""
    return R.recipe_step(params.cpu().numpy(), grads.cpu().numpy(), exp_avg.cpu().numpy(), exp_avg_sq.cpu().numpy(),
                         ema.cpu().numpy(), state, lr=lr, beta1=B1, beta2=B2, eps=EPS, max_norm=clip, weight_decay=WD,
                         warmup_steps=WARMUP, ema_decay=EMA_D, ema_warmup=True, mask4=mask.cpu().numpy())


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_layout_engine_full_recipe_matches_the_restatement(dev, precision):
    plain = small_engine(dev, precision)
    assert plain.optim.guard is None and plain.optim.ema is None and plain.ema is None and not plain.optim.recipe
    with pytest.raises(RuntimeError):
        plain.ema_weights().__enter__()
    eng = small_engine(dev, precision, clip_grad=1.0, **FULL)
    assert eng.guarded and torch.equal(eng.ema, eng.params) and (eng.ema_shadow is not None) == (precision == "bf16")
    from vlg.optim import build_decay_mask, decays_matrix
    assert torch.equal(eng.optim.decay_mask.cpu(), build_decay_mask(eng.layout, eng.n_params, decays_matrix))
    state = {"step": 0, "skipped": 0}
    for i in range(3):
        before = [t.clone() for t in (eng.params, eng.exp_avg, eng.exp_avg_sq, eng.ema)]
        eng.train_step(small_batch(dev, 70 + i))
        wp, wm, wv, we, state, info = restate(before[0], eng.grads, before[1], before[2], before[3], eng.optim.decay_mask,
                                              state, 1.0)
        check_close(eng.params, torch.from_numpy(wp).float(), rtol=RTOL, atol=ATOL, what="parameters, step %d" % (i + 1))
        check_close(eng.ema, torch.from_numpy(we).float(), rtol=RTOL, atol=ATOL, what="average, step %d" % (i + 1))
        st = eng.optimizer_stats()
        assert st["applied_steps"] == i + 1 and st["lr_eff"] == f32(info["lr_eff"])
        assert abs(st["ema_decay_t"] - info["ema_decay_t"]) < 1e-6
        if precision == "bf16":
            assert torch.equal(eng.params_bf16, eng.params.to(BF)) and torch.equal(eng.ema_shadow, eng.ema.to(BF))
    assert not torch.equal(eng.ema, eng.params) and not torch.equal(eng.ema, before[3])


@pytest.fixture(scope="module")
def trained(dev):
    """precision -> an engine two full-recipe steps in (the average differs from the live weights), shared and left unchanged"""
    made = {}

    def get(precision):
        if precision not in made:
            eng = small_engine(dev, precision, clip_grad=1.0, **FULL)
            eng.set_lr(0.05)                                       # far enough for the two models to differ visibly
            for i in range(2):
                eng.train_step(small_batch(dev, 80 + i))
            made[precision] = eng
        return made[precision]
    return get


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_ema_weights_block_runs_the_averaged_model(dev, trained, precision):
    eng = trained(precision)
    batch = small_batch(dev, 90)
    live = eng.forward(batch).clone()
    other = small_engine(dev, precision)
    other.load_params(eng.ema_named_params())
    want = other.forward(batch).clone()
    prompt_c, prompt_b = batch["slot_class"], batch["slot_box"]
    want_c, want_b = (t.clone() for t in other.rollout(prompt_c, prompt_b, steps=3, temperature=0.0))
    with eng.ema_weights() as inside:
        assert inside is eng
        got = eng.forward(batch).clone()
        rec = eng.metrics_record()
        eng.accumulate_metrics(batch, rec)
        got_c, got_b = (t.clone() for t in eng.rollout(prompt_c, prompt_b, steps=3, temperature=0.0))
        for name, fn in (("train_step", lambda: eng.train_step(batch)), ("backward", lambda: eng.backward(batch)),
                         ("adam_step", eng.adam_step), ("optimizer_update", eng.optimizer_update),
                         ("capture_train_step", lambda: eng.capture_train_step(batch)),
                         ("load_params", lambda: eng.load_params(other.named_params()))):
            with pytest.raises(RuntimeError, match=name):
                fn()
    assert torch.equal(got, want) and not torch.equal(got, live)
    assert torch.equal(got_c, want_c) and torch.equal(got_b, want_b)
    assert torch.equal(eng.forward(batch), live)
    assert eng.optimizer_stats()["applied_steps"] == 2
    with pytest.raises(RuntimeError):                              # the live weights come back when the block raises
        with eng.ema_weights():
            raise RuntimeError("inside")
    assert torch.equal(eng.forward(batch), live)


def test_captured_full_recipe_step_replays_bitwise(dev):
    """four replays = four eager steps of a twin (a set_lr between them included) in parameters, moments, average and ctl;
    the capture itself moves neither the average nor ext"""
    eager, graphed = (small_engine(dev, clip_grad=1.0, **FULL) for _ in range(2))
    batches = [small_batch(dev, 100 + i) for i in range(4)]
    ema0, ext0 = graphed.ema.clone(), graphed.guard.ext.clone()
    run = graphed.capture_train_step(batches[0])
    assert torch.equal(graphed.ema, ema0) and torch.equal(graphed.guard.ext.view(torch.int32), ext0.view(torch.int32))
    assert torch.equal(graphed.params, eager.params) and graphed.optimizer_stats()["applied_steps"] == 0
    for i, b in enumerate(batches):
        if i == 2:
            for e in (eager, graphed):
                e.set_lr(10 * LR)
        le = eager.train_step(b).clone()
        lg = run(b).clone()
        assert torch.equal(le, lg), i
    for a, b in ((eager.params, graphed.params), (eager.exp_avg, graphed.exp_avg), (eager.exp_avg_sq, graphed.exp_avg_sq),
                 (eager.ema, graphed.ema), (eager.guard.ctl.view(torch.int32), graphed.guard.ctl.view(torch.int32)),
                 (eager.guard.ext.view(torch.int32), graphed.guard.ext.view(torch.int32))):
        assert torch.equal(a, b)
    st = graphed.optimizer_stats()
    assert st["applied_steps"] == 4 and st["lr_eff"] == f32(f32(10 * LR) * min(1.0, 4 / WARMUP)) and not torch.equal(graphed.ema, ema0)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_resume_continues_bitwise_and_an_older_state_seeds_the_average(dev, precision):
    batches = [small_batch(dev, 110 + i) for i in range(4)]
    make = lambda: small_engine(dev, precision, clip_grad=1.0, **FULL)
    whole, first = make(), make()
    for b in batches:
        whole.train_step(b)
    for b in batches[:2]:
        first.train_step(b)
    st = first.optimizer_state()
    assert {"ema", "weight_decay", "warmup_steps", "ema_decay", "ema_warmup"} <= set(st)
    resumed = make()
    resumed.load_params(first.named_params())
    assert torch.equal(resumed.ema, first.params)                  # re-seeded from the loaded parameters ...
    resumed.load_optimizer(st)
    assert torch.equal(resumed.ema, first.ema)                     # ... until the checkpoint brings the average
    for b in batches[2:]:
        resumed.train_step(b)
    for a, b in ((whole.params, resumed.params), (whole.exp_avg, resumed.exp_avg), (whole.exp_avg_sq, resumed.exp_avg_sq),
                 (whole.ema, resumed.ema)):
        assert torch.equal(a, b)
    if precision == "bf16":
        assert torch.equal(whole.ema_shadow, resumed.ema_shadow) and torch.equal(resumed.ema_shadow, resumed.ema.to(BF))
    assert resumed.optimizer_stats()["applied_steps"] == 4
    old = {k: v for k, v in st.items() if k not in ("ema", "weight_decay", "warmup_steps", "ema_decay", "ema_warmup")}
    third = make()
    third.load_params(first.named_params())
    third.load_optimizer(old)
    assert torch.equal(third.ema, first.params) and torch.equal(third.exp_avg, first.exp_avg)
    assert third.optimizer_stats()["applied_steps"] == 2
    sd = first.state_dict()                                        # the flat form: carries the average; stripped, it is re-seeded
    fourth, fifth = make(), make()
    fourth.load_state_dict(sd)
    fifth.load_state_dict({k: v for k, v in sd.items() if k != "ema"})
    assert torch.equal(fourth.ema, first.ema) and torch.equal(fifth.ema, first.params)


# --------------------------------------------------------------------------------------------------- image engine
def test_image_engine_decays_convolution_weights_only(dev):
    from oracle import gridnet_spec as G
    from vlg.image_engine import ImageEngine, synthetic_frames
    filt = (8, 16, 24)

    def make(wd):
        eng = ImageEngine(1, 32, 32, dev, arch="CoordGridNet", filters=filt, clip_grad=1.0, weight_decay=wd, ema_decay=EMA_D)
        eng.load_state_dict(G.test_params(G.param_shapes(10, filt, coord=True), seed=1))
        return eng

    eng, twin = make(WD), make(0.0)
    assert torch.equal(eng.ema, eng.net.params) and twin.optim.decay_mask is None
    batch = {k: v.to(dev) for k, v in synthetic_frames(1, 32, 32, seed=3).items()}
    before = [t.clone() for t in (eng.net.params, eng.exp_avg, eng.exp_avg_sq, eng.ema)]
    eng.train_step(batch)
    twin.train_step(batch)
    mask4 = eng.optim.decay_mask.cpu()
    wp, _, _, we, _, info = R.recipe_step(before[0].cpu().numpy(), eng.net.grads.cpu().numpy(), before[1].cpu().numpy(),
                                          before[2].cpu().numpy(), before[3].cpu().numpy(), {"step": 0, "skipped": 0}, lr=LR,
                                          beta1=B1, beta2=B2, eps=EPS, max_norm=1.0, weight_decay=WD, ema_decay=EMA_D,
                                          mask4=mask4.numpy())
    assert info["clip_coef"] < 1.0
    check_close(eng.net.params, torch.from_numpy(wp).float(), rtol=RTOL, atol=ATOL, what="pixel model parameters")
    check_close(eng.ema, torch.from_numpy(we).float(), rtol=RTOL, atol=ATOL, what="pixel model average")
    # the mask is exactly the convolution weights: biases and PReLU slopes are bitwise those of the wd = 0 twin
    marked = torch.repeat_interleave(mask4 != 0, 4)
    want = torch.zeros_like(marked)
    for lo, hi in eng.net.weight_ranges():
        want[lo:hi] = True
    assert torch.equal(marked, want) and bool(marked.any()) and not bool(marked.all())
    got, ref = eng.net.params.cpu(), twin.net.params.cpu()
    assert torch.equal(got[~marked], ref[~marked])
    a, b = eng.state_dict(), twin.state_dict()
    for k in a:
        if k.endswith(".bias") or a[k].shape == (1,):
            assert torch.equal(a[k], b[k]), k
        else:
            assert not torch.equal(a[k], b[k]), k
    ema_sd = eng.ema_state_dict()
    assert set(ema_sd) == set(a) and all(ema_sd[k].shape == a[k].shape for k in a)
    st = eng.optimizer_state()
    assert st["ema_decay"] == EMA_D and st["ema"].numel() == eng.net.params.numel()
    fresh = make(WD)
    fresh.load_state_dict(eng.state_dict())
    fresh.load_optimizer(st)
    assert torch.equal(fresh.ema, eng.ema) and torch.equal(fresh.exp_avg, eng.exp_avg)


# ------------------------------------------------------------------------------------- two ranks on one device
DP_CFG = dict(B=2, T=4, N=4, d=64, n_layers=1)


def _dp_worker(rank, world, port, out):
    for p in (ROOT, PKG, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, world_size=world, rank=rank)
    from vlg.dp import GradReducer, bucket_ranges
    from vlg.engine import LayoutEngine
    from vlg.spec import LayoutConfig
    dev = torch.device("cuda:0")
    cfg = LayoutConfig(**DP_CFG)
    eng = LayoutEngine(cfg, dev, seed=1024, clip_grad=1.0, **FULL)
    red = GradReducer(eng.grads_ext, bucket_ranges(eng.layout, eng.n_params, cfg.n_layers))
    for step in range(2):
        full = O.synthetic_batch(cfg.B * world, cfg.T, cfg.N, seed=120 + step)
        eng.train_step({k: v[rank::world].contiguous().to(dev) for k, v in full.items()}, red)
    torch.save({"params": eng.params.cpu(), "ema": eng.ema.cpu(), "stats": eng.optimizer_stats()}, "%s.%d" % (out, rank))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_hold_bit_equal_parameters_and_average(dev, tmp_path):
    world, out = 2, str(tmp_path / "dp.pt")
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.spawn(_dp_worker, args=(world, port, out), nprocs=world, join=False)
    deadline = time.time() + 120                                # the ranks' own time limit: a stuck child is ended
    while not ctx.join(timeout=5):
        if time.time() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("data-parallel ranks did not finish in 120 s")
    got = [torch.load("%s.%d" % (out, r), weights_only=True) for r in range(world)]
    assert got[0]["stats"] == got[1]["stats"] and got[0]["stats"]["applied_steps"] == 2
    assert got[0]["stats"]["lr_eff"] == f32(LR * min(1.0, 2 / WARMUP))
    assert torch.equal(got[0]["params"], got[1]["params"]) and torch.equal(got[0]["ema"], got[1]["ema"])
    assert not torch.equal(got[0]["ema"], got[0]["params"])


# -------------------------------------------------------------------------------------------------------- Trainer
TRAINER = dict(batch_size=4, epochs=1, print_freq=1, n_frames=4, n_slots=8, d_model=64, n_layers=1, train_clips=8, val_clips=8)
RECIPE_ENV = ("VLG_WEIGHT_DECAY", "VLG_WARMUP_STEPS", "VLG_EMA_DECAY", "VLG_EMA_WARMUP", "VLG_EMA_EVAL", "VLG_CLIP_GRAD",
              "VLG_SKIP_NONFINITE", "VLG_LR_DECAY", "VLG_MODEL", "VLG_PRECISION", "VLG_VAL_METRICS")


def test_trainer_evaluates_and_checkpoints_the_average(tmp_path, monkeypatch):
    from trainer import Trainer
    from vlg.data import to_device
    (tmp_path / "src").mkdir()
    monkeypatch.chdir(tmp_path / "src")
    for k in RECIPE_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in (("VLG_EMA_DECAY", "0.5"), ("VLG_WEIGHT_DECAY", "0.1"), ("VLG_WARMUP_STEPS", "2")):
        monkeypatch.setenv(k, v)
    tr = Trainer(reference_args(tmp_path / "exp", lr=0.05, **TRAINER))
    eng = tr.engine
    assert eng.optim.recipe and eng.ema is not None and tr.guarded and tr.optim["ema_eval"] is True
    tr.set_epoch(0)
    tr.train()
    assert eng.optimizer_stats()["applied_steps"] == 2 and not torch.equal(eng.ema, eng.params)

    def engine_loss(on_ema):
        total, count = 0.0, 0
        for batch in tr.val_loader:
            with (eng.ema_weights() if on_ema else contextlib.nullcontext()):
                loss = float(eng.forward(to_device(batch, tr.device))[0].item())
            size = batch["slot_class"].shape[0]
            total, count = total + loss * size, count + size
        return total / count

    on_ema, on_live = engine_loss(True), engine_loss(False)
    assert on_ema != on_live
    got = tr.validate()["loss"]
    assert got == pytest.approx(on_ema, rel=1e-6) and abs(got - on_live) > 1e-6 * abs(on_live)
    batch = to_device(next(iter(tr.val_loader)), tr.device)
    c, b = tr.generate_sequence(batch["slot_class"], batch["slot_box"], steps=2)
    with eng.ema_weights():
        wc, wb = eng.rollout(batch["slot_class"], batch["slot_box"], steps=2)
    assert torch.equal(c, wc.cpu()) and torch.equal(b, wb.cpu())
    tr.save_checkpoint({"loss": got})
    ckpt = torch.load(tmp_path / "checkpoint" / "latest.pth", weights_only=True)
    assert set(ckpt["gridnet_ema"]) == set(ckpt["gridnet"]) and "ema" in ckpt["optimizer"]
    assert torch.equal(ckpt["gridnet_ema"]["head_w"], eng.ema_named_params()["head_w"].cpu())
    # VLG_EMA_EVAL=0: the live weights
    monkeypatch.setenv("VLG_EMA_EVAL", "0")
    live_tr = Trainer(reference_args(tmp_path / "live", resume="../checkpoint/latest.pth", lr=0.05, **TRAINER))
    assert torch.equal(live_tr.engine.ema, eng.ema) and torch.equal(live_tr.engine.params, eng.params)
    assert live_tr.validate()["loss"] == pytest.approx(on_live, rel=1e-6)
    # the averaged model as a model: --ckpt of {'gridnet': gridnet_ema}, every recipe knob off
    for k in RECIPE_ENV:
        monkeypatch.delenv(k, raising=False)
    torch.save({"gridnet": ckpt["gridnet_ema"]}, tmp_path / "ema_model.pth")
    as_model = Trainer(reference_args(tmp_path / "model", ckpt=str(tmp_path / "ema_model.pth"), **TRAINER))
    assert as_model.engine.ema is None and as_model.engine.optim.guard is None
    assert as_model.validate()["loss"] == pytest.approx(got, rel=1e-6)
