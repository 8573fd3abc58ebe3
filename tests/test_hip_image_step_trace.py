"""GPU: every launch of one ImageEngine.forward + backward against fp64 evaluated on the tensors that launch read.

The end-to-end statements of the pixel step cannot be tight: tests/test_hip_image_step_bf16.py compares the bf16 step with the
fp32 one under bars read off the GPU, and the fp32 step needs kink allowances (two forwards that differ in the last bits take
different PReLU / ReLU / max-pool / L1 branches on a few elements).  So the engine's COMPOSITION - which buffer feeds which
launch, which slope, which act_ch, which residual branch, which epilogue flags, which arena region - is checked here one launch
at a time: image_trace.trace records the launches of one step, image_trace.check holds each of them to image_stages' schedule and
to the project's per-kernel bars against fp64 on the bits that launch read, so every branch decision is the kernel's own and
nothing amplifies.  No bar is new or read off a GPU result (image_trace's docstring lists them).  tests/test_image_trace_cpu.py
shows that these bars catch a missing ACCUM, a wrong slope, an activated AddCoords lane, a wrong residual, a missing or spurious
bf16 rounding, a wrong stride-2 window, overlapping arena regions and dirty halo rows / padded lanes at the stage where it happens.

Every case runs one UNTRACED forward + backward first, so that every gradient buffer holds stale values and a missing overwrite
shows, then traces a second one and asserts that its losses and gradients are bitwise the untraced run's.  Shapes are the
smallest that take each path (see CASES); real, distinct PReLU slopes throughout."""
import pytest
import torch

import image_stages as IS
import image_trace
from helpers import check_close, vs_cpu32
from oracle import gridnet_spec as GS
from oracle import hned_spec as HS
from oracle import vgg_spec as VS

pytestmark = pytest.mark.gpu

SMALL = (8, 16, 24)
CASES = [
    # ragged width 40 / 20 / 10 at the three levels; plain input block: its shortcut conv reads the network input without a PReLU
    # and gets no data gradient, while lateral_in.conv.1's data gradient into d.g:x runs only because of its PReLU (the slope)
    ("GridNet", (2, 32, 40), SMALL, False, 0), ("GridNet", (2, 32, 40), SMALL, False, 1),
    # AddCoords lanes on two tensors, act_ch < cp; both convolutions on the network input are without a PReLU, so nothing
    # writes d.g:x, and the block's PReLU sits on a coord tensor inside it
    ("CoordGridNet", (2, 32, 40), SMALL, False, 0),
    # 32 / 64 / 96 lanes: more than one K tile, cout_p above 32; HED (H, W % 16) and VGG (% 8), whose 256 / 512-channel levels run
    # at 8x8 and 4x4 where every tile takes the workspace split
    ("CoordGridNet", (1, 32, 32), (32, 64, 96), True, 0),
]
IDS = ["%s-%dx%dx%d%s%s" % (a, s[0], s[1], s[2], "-hed-vgg" if x else "", "-flip" if f else "") for a, s, _, x, f in CASES]


def _engine(dev, arch, shape, filters, extras, precision, **kw):
    from vlg.image_engine import ImageEngine, synthetic_frames
    eng = ImageEngine(*shape, dev, arch=arch, filters=filters, with_hed=extras, with_vgg=extras, precision=precision, **kw)
    eng.load_state_dict(GS.test_params(GS.param_shapes(10, filters, coord=arch == "CoordGridNet"), linear=False))
    if extras:
        eng.hed.load_state_dict(HS.test_params())
        eng.vgg.load_state_dict(VS.test_params())
    batch = synthetic_frames(*shape, seed=11)
    if extras:                                            # the edge maps come from the HED trunk
        del batch["e1"], batch["e2"]
    return eng, batch


def _summary(log):
    worst = {}
    for stage, n, e_gpu, e_cpu in log:
        key = "%s %s" % (stage, n.split()[-1]) if n in ("loss value", "loss grad", "value", "grad") else n
        if e_gpu >= worst.get(key, (-1.0, 0.0))[0]:
            worst[key] = (e_gpu, e_cpu)
    return ", ".join("%s %.1e (cpu32 %.1e)" % (k, a, b) for k, (a, b) in sorted(worst.items()))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("arch,shape,filters,extras,flip", CASES, ids=IDS)
def test_every_launch_matches_fp64_on_its_inputs(dev, arch, shape, filters, extras, flip, precision):
    eng, batch = _engine(dev, arch, shape, filters, extras, precision)
    c = IS.Contract(arch, filters, extras, extras, precision)
    b = {k: v.to(dev) for k, v in batch.items()}
    eng.forward(b, bool(flip))
    eng.backward()
    torch.cuda.synchronize()
    grads0 = eng.net.grads_ext.clone()
    records, state = image_trace.trace(eng, b, bool(flip))
    assert torch.equal(eng.net.grads_ext, grads0), "the traced run's losses / gradients are not bitwise the untraced run's"
    log = []
    try:
        image_trace.check(records, state, c, batch, log=log)
    finally:
        print("\n%s %s %s%s: worst |err| vs fp64 per launch kind: %s" % (precision, arch, shape, " flip" if flip else "", _summary(log)))


@pytest.mark.parametrize("arch", ["GridNet", "CoordGridNet"])
def test_launch_counts_follow_the_reference_parameters(dev, arch):
    """one 3x3 forward launch and one weight-gradient launch per 4-d .weight of the reference's state_dict"""
    eng, batch = _engine(dev, arch, (2, 32, 40), SMALL, False, "fp32")
    b = {k: v.to(dev) for k, v in batch.items()}
    eng.forward(b)
    eng.backward()
    records, _ = image_trace.trace(eng, b, False)
    n3x3 = sum(1 for k, s in GS.param_shapes(10, SMALL, coord=arch == "CoordGridNet").items() if k.endswith(".weight") and len(s) == 4)
    names = [r["name"] for r in records]
    assert names.count("vlg_conv3x3_fwd") == n3x3 == names.count("vlg_conv3x3_wgrad"), (n3x3, names.count("vlg_conv3x3_fwd"))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_padded_lanes_stay_zero_through_adam(dev, precision):
    """ImageEngine.optimizer_update: the padded lanes of the flat layout 'stay zero'.  The gradient norm and Adam run over the
    flat buffer and rely on it: after three plain steps, and after two guarded ones with clipping, every padded lane of the
    parameters and of both Adam moments is exactly 0.0 (lane map: image_stages.Contract.padded_lanes)."""
    from vlg.spec import ADAM_BETA2, ADAM_EPS
    arch, shape = "CoordGridNet", (2, 32, 40)
    pad = IS.Contract(arch, SMALL, precision=precision).padded_lanes().to(dev)
    for guarded in (False, True):
        eng, batch = _engine(dev, arch, shape, SMALL, False, precision, **(dict(clip_grad=1.0) if guarded else {}))
        assert eng.net.params.numel() == pad.numel()
        b = {k: v.to(dev) for k, v in batch.items()}
        for step in range(2 if guarded else 3):
            if guarded:
                eng.forward(b, bool(step % 2))
                eng.backward()
                eng.optimizer_update()
            else:
                before = [t.cpu().clone() for t in (eng.net.params, eng.exp_avg, eng.exp_avg_sq)]
                eng.train_step(b, bool(step % 2))
                # the Adam launch on what it read - the hyperparameters are float arguments of vlg_adam_step, so the reference
                # takes them as the fp32 values the launch got (1 - fp32(0.999) is 1.3e-5 off 1e-3, and exp_avg_sq shows it):
                # test_hip_image_ops.test_adam_matches_reference_golden's bar for the parameters, helpers.vs_cpu32 for the moments
                hyper = [IS._f32(h) for h in (eng.lr, eng.beta1, ADAM_BETA2, ADAM_EPS)]
                args = (eng.net.grads.cpu(), before[1], before[2], step + 1, *hyper)
                want, cpu = IS.adam_step(before[0], *args), IS.adam_step(before[0], *args, dt=torch.float32)
                check_close(eng.net.params, want[0], rtol=1e-6, atol=1e-7, what="params after Adam step %d" % (step + 1))
                vs_cpu32(eng.exp_avg, want[1], cpu[1], "exp_avg")
                vs_cpu32(eng.exp_avg_sq, want[2], cpu[2], "exp_avg_sq")
        torch.cuda.synchronize()
        steps = eng.optimizer_stats()["applied_steps"] if guarded else eng.step_count
        assert steps == (2 if guarded else 3)
        for name, t in (("grads", eng.net.grads), ("params", eng.net.params), ("exp_avg", eng.exp_avg), ("exp_avg_sq", eng.exp_avg_sq)):
            bad = pad & (t != 0)
            assert not bool(bad.any()), "%s: %d padded lanes are not 0.0 after %d %s steps" % (
                name, int(bad.sum()), 2 if guarded else 3, "guarded" if guarded else "plain")
        assert bool((eng.exp_avg_sq[~pad] > 0).any()), "Adam did not run"
