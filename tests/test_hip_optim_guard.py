"""GPU: the guarded optimiser step - vlg_grad_sumsq, vlg_optim_control, vlg_adam_step_ctl (csrc/optim.hip) against fp64
restatements and, where the header claims it, bit for bit against the plain Adam entry points; then the engines' use
of them: norm, clipping, the skipped step, set_lr across graph replays, and two ranks on one device."""
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

from conftest import PKG, ROOT
from helpers import check_close
from oracle import layout_spec as O
# slots of the control record (VLG_CTL_* in include/vlg_hip.h)
from vlg.optim import APPLY, CLIP_COEF, GRAD_MULT, GRAD_NORM, LR as LR_SLOT, SKIPPED, SQRT_BC2, STEP, STEP_SIZE

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
LR, B1, B2, EPS = 2e-4, 0.5, 0.999, 1e-8


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
    host[LR_SLOT] = lr
    host[CLIP_COEF] = 1.0
    host.view(torch.int32)[STEP] = step
    host.view(torch.int32)[SKIPPED] = skipped
    return host.to(dev)


def read_ctl(ctl):
    h = ctl.cpu()
    return h, h.view(torch.int32)


def host_factors(lr, step):
    """step_size and sqrt_bc2 as the host code of vlg_adam_step computes them: float arguments widened to double, the
    bias corrections in double, one rounding to float."""
    lr, b1, b2 = (float(np.float32(x)) for x in (lr, B1, B2))
    return np.float32(lr / (1.0 - b1 ** step)), np.float32(math.sqrt(1.0 - b2 ** step))


def sumsq(H, g, sentinel=-7.0):
    n = g.numel()
    P = H.load().vlg_grad_sumsq_blocks(n)
    part = torch.full((P + 4,), sentinel, device=g.device)
    H.call("vlg_grad_sumsq", g.data_ptr(), n, part.data_ptr(), stream())
    return part, P


def control(H, ctl, partials, P, grad_scale=1.0, max_norm=0.0):
    H.call("vlg_optim_control", ctl.data_ptr(), partials.data_ptr(), P, grad_scale, max_norm, B1, B2, stream())


def adam_ctl(H, p, g, m, v, sh, ctl, lo=0, hi=None):
    hi = p.numel() if hi is None else hi
    H.call("vlg_adam_step_ctl", p.data_ptr() + 4 * lo, g.data_ptr() + 4 * lo, m.data_ptr() + 4 * lo, v.data_ptr() + 4 * lo,
           0 if sh is None else sh.data_ptr() + 2 * lo, hi - lo, ctl.data_ptr(), B1, B2, EPS, stream())


# ------------------------------------------------------------------------------------------------ vlg_grad_sumsq
def two_trip_n(H):
    """smallest kind of n at which EVERY block makes more than one grid-stride trip: twice the lanes of the largest grid"""
    lib = H.load()
    p_max = lib.vlg_grad_sumsq_blocks(1 << 40)
    n = 4 * (2 * p_max * 256 + 259)
    assert lib.vlg_grad_sumsq_blocks(n) == p_max
    return n


@pytest.mark.parametrize("n", [4, 1028, 4104, 1_000_004, "two_trips"])
def test_sumsq_matches_fp64(H, dev, n):
    """sqrt(sum of the partials) vs the fp64 sum of the same fp32 values: 1e-5 relative (fp32 chains of at most 64 terms
    would be bounded by 65 * 2^-24 = 4e-6; the kernel accumulates in fp64 and rounds each partial once)."""
    n = two_trip_n(H) if n == "two_trips" else n
    g = torch.Generator().manual_seed(n % 1000)
    x = torch.randn(n, generator=g)
    x[torch.randint(0, n, (5,), generator=g)] *= 1e3
    want = math.sqrt(float(x.double().pow(2).sum()))
    xd = x.to(dev)
    part, P = sumsq(H, xd)
    assert 1 <= P <= 2048
    host = part.cpu()
    assert torch.equal(host[P:], torch.full((4,), -7.0)), "elements at or beyond P must not be written"
    got = math.sqrt(float(host[:P].double().sum()))
    print("n=%d P=%d rel err %.3e" % (n, P, abs(got - want) / want))
    assert math.isfinite(got) and abs(got - want) <= 1e-5 * want, (got, want)
    again, _ = sumsq(H, xd)
    assert torch.equal(again.cpu(), host), "two runs must be bitwise equal"
    for bad, test in ((float("inf"), math.isinf), (float("nan"), math.isnan)):
        y = xd.clone()
        y[n // 2] = bad
        part, P = sumsq(H, y)
        assert test(float(part[:P].double().sum())), bad


def test_sumsq_bad_arguments(H, dev):
    x, part = torch.zeros(64, device=dev), torch.zeros(8, device=dev)
    for n in (0, 3, 6):
        with pytest.raises(H.HipError, match="VLG_ERR_SHAPE"):
            H.call("vlg_grad_sumsq", x.data_ptr(), n, part.data_ptr(), stream())
    with pytest.raises(H.HipError, match="VLG_ERR_ALIGN"):
        H.call("vlg_grad_sumsq", x.data_ptr() + 4, 8, part.data_ptr(), stream())
    with pytest.raises(H.HipError, match="VLG_ERR_ALIGN"):
        H.call("vlg_grad_sumsq", x.data_ptr(), 8, part.data_ptr() + 4, stream())


# --------------------------------------------------------------------------------------------- vlg_optim_control
def test_control_clips_like_torch_and_counts_steps(H, dev):
    partials = torch.tensor([1.5, 2.25, 0.25, 5.0], device=dev)           # sum 9: norm 3 at grad_scale 1
    ctl = new_ctl(dev)
    for step, (scale, max_norm) in enumerate([(1.0, 6.0), (1.0, 3.0), (0.5, 1.0)], start=1):   # below, at, above
        control(H, ctl, partials, 4, scale, max_norm)
        f, i = read_ctl(ctl)
        norm = scale * 3.0
        coef = min(1.0, max_norm / (norm + 1e-6))
        assert abs(float(f[GRAD_NORM]) - norm) <= 1e-6 * norm
        assert abs(float(f[CLIP_COEF]) - coef) <= 1e-6 * coef
        assert abs(float(f[GRAD_MULT]) - scale * coef) <= 1e-6 * scale * coef
        assert (int(i[STEP]), int(i[APPLY]), int(i[SKIPPED])) == (step, 1, 0)
        ss, bc = host_factors(LR, step)
        assert f[STEP_SIZE].numpy() == ss and f[SQRT_BC2].numpy() == bc, (step, f[:2], ss, bc)
    assert float(f[CLIP_COEF]) < 1.0 and float(f[LR_SLOT]) == float(np.float32(LR))


def test_control_without_clipping_keeps_grad_scale_bitwise(H, dev):
    partials = torch.tensor([1e6, 3.0], device=dev)
    for scale in (1.0, 0.25, 1.0 / 3.0):
        for max_norm in (0.0, -1.0):
            ctl = new_ctl(dev)
            control(H, ctl, partials, 2, scale, max_norm)
            f, i = read_ctl(ctl)
            assert f[GRAD_MULT].numpy() == np.float32(scale) and float(f[CLIP_COEF]) == 1.0 and int(i[APPLY]) == 1


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_control_skips_a_non_finite_norm(H, dev, bad):
    ctl = new_ctl(dev)
    good = torch.tensor([4.0, 5.0], device=dev)
    control(H, ctl, good, 2, 1.0, 1.0)
    before, _ = read_ctl(ctl)
    control(H, ctl, torch.tensor([4.0, bad], device=dev), 2, 1.0, 1.0)
    f, i = read_ctl(ctl)
    assert (int(i[STEP]), int(i[APPLY]), int(i[SKIPPED])) == (1, 0, 1)
    assert not math.isfinite(float(f[GRAD_NORM]))
    for slot in (STEP_SIZE, SQRT_BC2, GRAD_MULT, CLIP_COEF, LR_SLOT):
        assert f[slot].numpy() == before[slot].numpy(), slot
    control(H, ctl, good, 2, 1.0, 1.0)                                     # the next finite step is step 2, not 3
    f, i = read_ctl(ctl)
    assert (int(i[STEP]), int(i[APPLY]), int(i[SKIPPED])) == (2, 1, 1)
    assert f[STEP_SIZE].numpy() == host_factors(LR, 2)[0]


def test_control_reads_the_learning_rate_from_the_record(H, dev):
    ctl = new_ctl(dev)
    partials = torch.tensor([1.0], device=dev)
    control(H, ctl, partials, 1)
    assert read_ctl(ctl)[0][STEP_SIZE].numpy() == host_factors(LR, 1)[0]
    ctl[LR_SLOT] = 5e-5
    control(H, ctl, partials, 1)
    assert read_ctl(ctl)[0][STEP_SIZE].numpy() == host_factors(5e-5, 2)[0]


def test_control_bad_arguments(H, dev):
    ctl, part = new_ctl(dev), torch.zeros(4, device=dev)
    for n in (0, 2049):
        with pytest.raises(H.HipError, match="VLG_ERR_SHAPE"):
            H.call("vlg_optim_control", ctl.data_ptr(), part.data_ptr(), n, 1.0, 0.0, B1, B2, stream())
    with pytest.raises(H.HipError, match="VLG_ERR_ALIGN"):
        H.call("vlg_optim_control", ctl.data_ptr() + 4, part.data_ptr(), 4, 1.0, 0.0, B1, B2, stream())


# --------------------------------------------------------------------------------------------- vlg_adam_step_ctl
def guarded_step(H, p, g, m, v, sh, ctl, grad_scale=1.0, max_norm=0.0, split=None):
    part, P = sumsq(H, g)
    control(H, ctl, part, P, grad_scale, max_norm)
    if split is None:
        adam_ctl(H, p, g, m, v, sh, ctl)
    else:
        adam_ctl(H, p, g, m, v, sh, ctl, 0, split)
        adam_ctl(H, p, g, m, v, sh, ctl, split, p.numel())


def test_adam_ctl_is_bitwise_the_plain_adam(H, dev):
    """clipping off: three steps equal vlg_adam_step (inputs of test_adam_matches_torch_optim: gradient x4, grad_scale
    0.25) and vlg_adam_step_bf16 with its shadow (inputs of test_adam_keeps_the_bf16_shadow); slices equal one call."""
    torch.manual_seed(8)
    n = 4096 + 8
    p0 = torch.randn(n)
    grads = [(torch.randn(n) * (10.0 ** (step - 2)) * 4).to(dev) for step in range(1, 4)]
    plain = [p0.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)]
    ours = [t.clone() for t in plain]
    sliced = [t.clone() for t in plain]
    ctl, ctl2 = new_ctl(dev), new_ctl(dev)
    for step, gd in enumerate(grads, start=1):
        H.call("vlg_adam_step", plain[0].data_ptr(), gd.data_ptr(), plain[1].data_ptr(), plain[2].data_ptr(), n, step, LR, B1, B2,
               EPS, 0.25, stream())
        guarded_step(H, ours[0], gd, ours[1], ours[2], None, ctl, grad_scale=0.25)
        guarded_step(H, sliced[0], gd, sliced[1], sliced[2], None, ctl2, grad_scale=0.25, split=1028)
        for a, b, c in zip(plain, ours, sliced):
            assert torch.equal(a, b) and torch.equal(a, c), step
    torch.manual_seed(14)
    p0, g = torch.randn(n), torch.randn(n).to(dev)
    plain = [p0.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev, dtype=BF)]
    ours = [t.clone() for t in plain]
    ctl = new_ctl(dev)
    for step in (1, 2, 3):
        H.call("vlg_adam_step_bf16", plain[0].data_ptr(), g.data_ptr(), plain[1].data_ptr(), plain[2].data_ptr(),
               plain[3].data_ptr(), n, step, LR, B1, B2, EPS, 1.0, stream())
        guarded_step(H, ours[0], g, ours[1], ours[2], ours[3], ctl)
        for a, b in zip(plain, ours):
            assert torch.equal(a, b), step
    assert torch.equal(ours[3], ours[0].to(BF))


def test_adam_ctl_clipped_matches_torch(H, dev):
    """max_norm = half the observed norm: torch.nn.utils.clip_grad_norm_ + torch.optim.Adam in fp64, at the existing
    Adam test's tolerances."""
    torch.manual_seed(8)
    n = 4096 + 8
    p0 = torch.randn(n)
    ref = p0.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=LR, betas=(B1, B2), eps=EPS)
    p, m, v, ctl = p0.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev), new_ctl(dev)
    for step in range(1, 4):
        g = torch.randn(n) * (10.0 ** (step - 2))
        max_norm = 0.5 * float(g.double().norm())
        ref.grad = g.double().clone()
        total = torch.nn.utils.clip_grad_norm_([ref], max_norm)
        opt.step()
        guarded_step(H, p, g.to(dev), m, v, None, ctl, max_norm=max_norm)
        f, _ = read_ctl(ctl)
        assert abs(float(f[GRAD_NORM]) - float(total)) <= 1e-5 * float(total)
        assert abs(float(f[CLIP_COEF]) - 0.5) < 1e-5
        check_close(p, ref.detach().float(), rtol=1e-6, atol=1e-7, what="clipped adam step %d" % step)


def test_adam_ctl_skip_touches_nothing(H, dev):
    torch.manual_seed(3)
    n = 4096 + 8
    p, m, v = torch.randn(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    sh = p.to(BF)
    g = torch.randn(n, device=dev)
    twin = [t.clone() for t in (p, m, v, sh)]
    ctl, ctl_twin = new_ctl(dev), new_ctl(dev)
    guarded_step(H, p, g, m, v, sh, ctl)                                   # step 1
    guarded_step(H, *twin[:1], g, *twin[1:], ctl_twin)
    keep = [t.clone() for t in (p, m, v, sh)]
    bad = g.clone()
    bad[17] = float("inf")
    guarded_step(H, p, bad, m, v, sh, ctl)                                 # skipped
    for a, b in zip((p, m, v, sh), keep):
        assert torch.equal(a, b)
    _, i = read_ctl(ctl)
    assert (int(i[STEP]), int(i[APPLY]), int(i[SKIPPED])) == (1, 0, 1)
    guarded_step(H, p, g, m, v, sh, ctl)                                   # step 2 - the twin never saw the bad gradient
    guarded_step(H, *twin[:1], g, *twin[1:], ctl_twin)
    for a, b in zip((p, m, v, sh), twin):
        assert torch.equal(a, b), "the step after a skip must use the bias correction of step k+1"
    assert int(read_ctl(ctl)[1][STEP]) == 2


def test_adam_ctl_bad_arguments(H, dev):
    n = 64
    p, g, m, v = (torch.zeros(n, device=dev) for _ in range(4))
    ctl = new_ctl(dev)
    for bad_n in (0, 6):
        with pytest.raises(H.HipError, match="VLG_ERR_SHAPE"):
            H.call("vlg_adam_step_ctl", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 0, bad_n, ctl.data_ptr(),
                   B1, B2, EPS, stream())
    with pytest.raises(H.HipError, match="VLG_ERR_SHAPE"):
        H.call("vlg_adam_step_ctl", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 0, n, 0, B1, B2, EPS, stream())
    with pytest.raises(H.HipError, match="VLG_ERR_ALIGN"):
        H.call("vlg_adam_step_ctl", p.data_ptr() + 4, g.data_ptr(), m.data_ptr(), v.data_ptr(), 0, 8, ctl.data_ptr(),
               B1, B2, EPS, stream())
    with pytest.raises(H.HipError, match="VLG_ERR_ALIGN"):
        H.call("vlg_adam_step_ctl", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 0, 8, ctl.data_ptr() + 4,
               B1, B2, EPS, stream())


# -------------------------------------------------------------------------------------------------- layout engine
SMALL = dict(B=2, T=4, N=3, d=64, n_layers=1)


def small_engine(dev, precision="fp32", **kw):
    from vlg.engine import LayoutEngine
    from vlg.spec import LayoutConfig
    return LayoutEngine(LayoutConfig(**SMALL), dev, seed=1024, precision=precision, **kw)


def small_batch(dev, seed):
    return to_dev(O.synthetic_batch(SMALL["B"], SMALL["T"], SMALL["N"], seed=seed), dev)


def adam_fp64(p, g, m, v, step, lr, mult):
    g = g.double() * mult
    m = m.double() + (1 - B1) * (g - m.double())
    v = v.double() * B2 + (1 - B2) * g * g
    denom = v.sqrt() / math.sqrt(1 - B2 ** step) + EPS
    return p.double() - lr / (1 - B1 ** step) * (m / denom)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_layout_engine_norm_clip_and_skip(dev, precision):
    eng = small_engine(dev, precision, clip_grad=1.0, skip_nonfinite=True)
    assert eng.guarded
    eng.forward_backward(small_batch(dev, 11))
    p0 = eng.params.cpu()
    eng.optimizer_update()
    st = eng.optimizer_stats()
    want = math.sqrt(sum(float(g.double().pow(2).sum()) for g in eng.named_grads().values()))
    assert abs(st["grad_norm"] - want) <= 1e-5 * want, (st, want)
    coef = min(1.0, 1.0 / (want + 1e-6))
    assert coef < 1.0 and abs(st["clip_coef"] - coef) <= 1e-5 * coef
    assert (st["applied_steps"], st["skipped_steps"]) == (1, 0) and eng.step_count == 1
    zero = torch.zeros_like(p0)
    check_close(eng.params, adam_fp64(p0, eng.grads.cpu(), zero, zero, 1, LR, coef).float(), rtol=1e-6, atol=1e-7,
                what="parameters after the clipped step")
    # a non-finite gradient: nothing moves
    eng.forward_backward(small_batch(dev, 12))
    keep = [t.clone() for t in (eng.params, eng.exp_avg, eng.exp_avg_sq)] + ([eng.params_bf16.clone()] if eng.params_bf16 is not None else [])
    eng.grads[eng.n_params // 2] = float("inf")
    eng.optimizer_update()
    now = [eng.params, eng.exp_avg, eng.exp_avg_sq] + ([eng.params_bf16] if eng.params_bf16 is not None else [])
    assert all(torch.equal(a, b) for a, b in zip(now, keep))
    st = eng.optimizer_stats()
    assert (st["applied_steps"], st["skipped_steps"]) == (1, 1) and not math.isfinite(st["grad_norm"])
    assert eng.state_dict()["step"] == 1 and eng.optimizer_state()["step"] == 1 and eng.optimizer_state()["skipped"] == 1
    eng.train_step(small_batch(dev, 13))
    st = eng.optimizer_stats()
    assert (st["applied_steps"], st["skipped_steps"]) == (2, 1) and math.isfinite(st["grad_norm"])
    assert not torch.equal(eng.params, keep[0])
    if eng.params_bf16 is not None:
        assert torch.equal(eng.params_bf16, eng.params.to(BF))


def test_layout_engine_skip_then_first_step(dev):
    """a skipped step before any applied one: the following clean step applies as step 1"""
    eng, twin = small_engine(dev, skip_nonfinite=True), small_engine(dev, skip_nonfinite=True)
    eng.forward_backward(small_batch(dev, 21))
    eng.grads[3] = float("nan")
    eng.optimizer_update()
    assert eng.optimizer_stats()["skipped_steps"] == 1 and eng.optimizer_stats()["applied_steps"] == 0
    assert torch.equal(eng.params, twin.params) and not bool(eng.exp_avg.any())
    b = small_batch(dev, 22)
    eng.train_step(b)
    twin.train_step(b)
    assert eng.optimizer_stats()["applied_steps"] == 1 and torch.equal(eng.params, twin.params)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_options_off_equals_guard_on_finite_gradients(dev, precision):
    plain, guarded = small_engine(dev, precision), small_engine(dev, precision, skip_nonfinite=True)
    assert not plain.guarded and plain.guard is None
    for i in range(3):
        b = small_batch(dev, 30 + i)
        plain.train_step(b)
        guarded.train_step(b)
    assert torch.equal(plain.params, guarded.params) and torch.equal(plain.exp_avg_sq, guarded.exp_avg_sq)
    assert plain.step_count == 3 and guarded.optimizer_stats()["applied_steps"] == 3
    if plain.params_bf16 is not None:
        assert torch.equal(plain.params_bf16, guarded.params_bf16)


def test_captured_guarded_step_replays_and_takes_a_new_lr(dev):
    """three replays = three eager guarded steps (clipping active), and set_lr between replays reaches the captured
    step without a recapture (it would not if the learning rate were a launch argument)"""
    eager, graphed = small_engine(dev, clip_grad=1.0), small_engine(dev, clip_grad=1.0)
    batches = [small_batch(dev, 40 + i) for i in range(5)]
    run = graphed.capture_train_step(batches[0])
    assert torch.equal(graphed.params, eager.params) and graphed.optimizer_stats()["applied_steps"] == 0
    for b in batches[:3]:
        le = eager.train_step(b).clone()
        lg = run(b).clone()
        assert torch.equal(le, lg)
    assert torch.equal(graphed.params, eager.params)
    assert graphed.optimizer_stats()["clip_coef"] < 1.0 and graphed.optimizer_stats()["applied_steps"] == 3
    before = graphed.params.clone()
    for e in (eager, graphed):
        e.set_lr(10 * LR)
    for b in batches[3:]:
        eager.train_step(b)
        run(b)
    assert torch.equal(graphed.params, eager.params) and torch.equal(graphed.exp_avg, eager.exp_avg)
    st = graphed.optimizer_stats()
    assert st["applied_steps"] == 5 and st["lr"] == float(np.float32(10 * LR))
    assert not torch.equal(graphed.params, before)


# --------------------------------------------------------------------------------------------------- image engine
def test_image_engine_norm_is_that_of_the_tensors_and_skips(dev):
    from oracle import gridnet_spec as G
    from vlg.image_engine import ImageEngine, synthetic_frames
    filt = (8, 16, 24)
    eng = ImageEngine(2, 32, 32, dev, arch="CoordGridNet", filters=filt, clip_grad=1.0, skip_nonfinite=True)
    eng.load_state_dict(G.test_params(G.param_shapes(10, filt, coord=True), seed=1))
    batch = {k: v.to(dev) for k, v in synthetic_frames(2, 32, 32, seed=3).items()}
    eng.forward(batch)
    eng.backward()
    eng.optimizer_update()
    st = eng.optimizer_stats()
    want = math.sqrt(sum(float(g.double().pow(2).sum()) for g in eng.net.unpack(eng.net.grads).values()))
    print("image grad norm %.6g, over the tensors %.6g" % (st["grad_norm"], want))
    assert abs(st["grad_norm"] - want) <= 1e-5 * want, (st, want)
    assert st["clip_coef"] < 1.0 and (st["applied_steps"], st["skipped_steps"]) == (1, 0)
    eng.forward(batch)
    eng.backward()
    keep = [t.clone() for t in (eng.net.params, eng.exp_avg, eng.exp_avg_sq)]
    eng.net.grads[eng.net.grads.numel() // 3] = float("inf")
    eng.optimizer_update()
    assert all(torch.equal(a, b) for a, b in zip((eng.net.params, eng.exp_avg, eng.exp_avg_sq), keep))
    st = eng.optimizer_stats()
    assert (st["applied_steps"], st["skipped_steps"]) == (1, 1)
    assert eng.optimizer_state()["skipped"] == 1 and int(eng.optimizer_state()["state"][0]["step"]) == 1
    eng.train_step(batch)
    assert eng.optimizer_stats()["applied_steps"] == 2 and not torch.equal(eng.net.params, keep[0])


# ------------------------------------------------------------- one optimiser object: three forms, both engines, resumed
RESUME_CFG = dict(B=1, T=16, N=9, d=64, n_layers=2)          # the smallest two-layer config of test_hip_step's edge shapes
RESUME_LR = 7e-5


class _LayoutCase:
    def __init__(self, dev):
        self.dev = dev
        self.batches = [to_dev(O.synthetic_batch(RESUME_CFG["B"], RESUME_CFG["T"], RESUME_CFG["N"], seed=50 + i), dev) for i in range(3)]

    def engine(self, **kw):
        from vlg.engine import LayoutEngine
        from vlg.spec import LayoutConfig
        return LayoutEngine(LayoutConfig(**RESUME_CFG), self.dev, seed=1024, **kw)

    params = staticmethod(lambda eng: eng.params)
    copy_params = staticmethod(lambda src, dst: dst.load_params(src.named_params()))
    recorded_lr = staticmethod(lambda st: st["lr"])


class _ImageCase:
    FILT = (8, 16, 24)

    def __init__(self, dev):
        from vlg.image_engine import synthetic_frames
        self.dev = dev
        self.batches = [{k: v.to(dev) for k, v in synthetic_frames(1, 32, 32, seed=60 + i).items()} for i in range(3)]

    def engine(self, **kw):
        from oracle import gridnet_spec as G
        from vlg.image_engine import ImageEngine
        eng = ImageEngine(1, 32, 32, self.dev, arch="CoordGridNet", filters=self.FILT, **kw)
        eng.load_state_dict(G.test_params(G.param_shapes(10, self.FILT, coord=True), seed=1))
        return eng

    params = staticmethod(lambda eng: eng.net.params)
    copy_params = staticmethod(lambda src, dst: dst.load_state_dict(src.state_dict()))
    recorded_lr = staticmethod(lambda st: st["param_groups"][0]["lr"])


@pytest.mark.parametrize("mode", ["plain", "device_counter", "guarded"])
@pytest.mark.parametrize("case", [_LayoutCase, _ImageCase], ids=["layout", "image"])
def test_resumed_optimiser_continues_bitwise_in_every_form(dev, case, mode):
    """two steps, optimizer_state() + parameters into a fresh engine of the same form, one more step on both: parameters,
    both moments and the step count are bitwise those of the uninterrupted engine; a guarded engine takes the recorded lr"""
    c = case(dev)

    def make():
        eng = c.engine(**(dict(clip_grad=1.0) if mode == "guarded" else {}))
        if mode == "device_counter":
            eng.use_device_step_counter()
        assert eng.guarded == (mode == "guarded") and (eng.adam_state is not None) == (mode == "device_counter")
        return eng

    def steps(eng):
        counts = [eng.optimizer_stats()["applied_steps"]] if eng.guarded else [eng.step_count]
        if eng.adam_state is not None:
            counts.append(int(eng.adam_state.view(torch.int32)[2]))
        return counts

    whole = make()
    for b in c.batches[:2]:
        whole.train_step(b)
    if mode == "guarded":
        whole.set_lr(RESUME_LR)                       # the fresh engine is built with the default: it must take the recorded one
    st = whole.optimizer_state()
    assert steps(whole) == [2] * len(steps(whole))
    resumed = make()
    c.copy_params(whole, resumed)
    resumed.load_optimizer(st)
    assert steps(resumed) == steps(whole) and torch.equal(resumed.exp_avg_sq, whole.exp_avg_sq)
    if mode == "guarded":
        assert c.recorded_lr(st) == RESUME_LR
        assert resumed.optimizer_stats()["lr"] == float(np.float32(RESUME_LR)) and resumed.lr == RESUME_LR
    for eng in (whole, resumed):
        eng.train_step(c.batches[2])
    assert steps(resumed) == steps(whole) == [3] * len(steps(whole))
    assert torch.equal(c.params(resumed), c.params(whole)) and bool(torch.isfinite(c.params(whole)).all())
    assert torch.equal(resumed.exp_avg, whole.exp_avg) and torch.equal(resumed.exp_avg_sq, whole.exp_avg_sq)
    assert bool(whole.exp_avg.any()) and not torch.equal(c.params(whole), c.params(make()))


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
    eng = LayoutEngine(cfg, dev, seed=1024, clip_grad=1.0)
    red = GradReducer(eng.grads_ext, bucket_ranges(eng.layout, eng.n_params, cfg.n_layers))
    full = O.synthetic_batch(cfg.B * world, cfg.T, cfg.N, seed=60)
    mine = {k: v[rank::world].contiguous().to(dev) for k, v in full.items()}
    eng.forward_backward(mine)                                  # the local gradient, kept for the parent's check
    local = eng.grads.cpu().clone()
    eng.train_step(mine, red)
    st = eng.optimizer_stats()
    torch.save({"local": local, "params": eng.params.cpu(), "stats": st}, "%s.%d" % (out, rank))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_clip_on_the_norm_of_the_mean_gradient(dev, tmp_path):
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
    a, b = got[0]["stats"], got[1]["stats"]
    assert a["grad_norm"] == b["grad_norm"] and a["clip_coef"] == b["clip_coef"] and a["applied_steps"] == b["applied_steps"] == 1
    want = float(((got[0]["local"].double() + got[1]["local"].double()) / world).norm())
    assert abs(a["grad_norm"] - want) <= 1e-5 * want, (a, want)
    assert a["clip_coef"] < 1.0
    assert torch.equal(got[0]["params"], got[1]["params"])
