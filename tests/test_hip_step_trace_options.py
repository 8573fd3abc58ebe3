"""GPU: test_hip_step_trace.py's per-launch check on the attention kind and the training options that file does not reach -
attention = "factored", the Gaussian box head, the loss options, scheduled sampling, augmentation, and all of them at once
beside dropout.  Same drivers, same rule: the traced run is bitwise the untraced one, every launch is held by name to the
schedule of step_stages.schedule (entry point, family, flags, the buffer behind every pointer, scalar arguments, the value
of every step counter after it) and by value to fp64 on the tensors it read.  No bar here is new: step_trace.check names the
kernel test each comparison is taken from.  tests/test_step_trace_options_cpu.py shows on a synthetic trace that each
wiring mistake these cases are about - the caller's tensor where the engine's belongs, the wrong lse row, another option's
counter - fails at its own stage.

Factored shapes, the smallest that reach each path of the frame kernels (tests/frame_walk.py): F1 (2,16,12) d=256 L=3 - a
12-token frame straddles the 32-token tiles (element-wise classification), M = 384, one frame layer at lse row 0; F2
(2,4,64) d=64 L=4 - a frame is two whole tiles ("whole" without `valid`), frame layers 1 and 3 at lse rows 0 and 1, the
smallest T; F3 (1,32,8) d=128 L=2 - the T = 32 per-slot kernels beside a frame layer, four frames per tile.
Option cases run at test_hip_step_trace's S1 with padded slots (variable N).  The three counters read 3 / 1 / 2 and the three
seeds differ and have high bits set, so a launch that reads another option's counter or seed fails by value as well as by name."""
import pytest
import torch

import augment_ref
import step_stages as SS
import step_trace
from test_hip_step_trace import S1, _batch, _summary

pytestmark = pytest.mark.gpu

F1 = dict(B=2, T=16, N=12, d=256, n_layers=3)
F2 = dict(B=2, T=4, N=64, d=64, n_layers=4)
F3 = dict(B=1, T=32, N=8, d=128, n_layers=2)
_IDS = {id(F1): "2x16x12-d256-L3", id(F2): "2x4x64-d64-L4", id(F3): "1x32x8-d128-L2"}

DROPOUT = (0.25, (0x9E3779B9 << 32) | 1024, 3)                      # (p, seed, k): test_hip_step_trace's DROP_SEED / DROP_K
SCHED = (0.5, 4, 0.0, 0, (0xC0FFEE12 << 32) | 345, 1)               # eps_max, ramp (k + 1 = 2 of 4: the integer rule is live), argmax
# temperature 0.7, top_k 5; the seed: tests/test_step_trace_options_cpu.py asserts that the float32 emulation of this case
# leaves no draw within the restatement's margin of a cumulative boundary
SCHED_SAMPLED = (0.5, 4, 0.7, 5, (0xC0FFEE12 << 32) | 345, 1)
AUGMENT = (augment_ref.ALL_ON, 0xC0FFEE1234567, 2)                   # (knobs, seed, k)
WEIGHTS = [0.5 + 0.125 * i for i in range(20)]
WEIGHTS[5] = 0.0                                                    # a class that does not count: out of the CE normaliser
LOSS = (WEIGHTS, 0.1, "giou")
W_NLL = 0.5


def _engine(dev, kw, c, gaussian=False):
    """the engine of a contract: every option of `c` as the constructor takes it, the counters at the contract's k"""
    from vlg.engine import LayoutEngine
    from vlg.spec import LayoutConfig
    cfg = LayoutConfig(attention=c.attention, **kw, **(dict(box_head="gaussian") if gaussian else {}))
    opts = {}
    if c.dropout is not None:
        opts.update(dropout=c.dropout[0], dropout_seed=c.dropout[1])
    if c.sched is not None:
        opts.update(zip(("sched_sampling", "sched_ramp_steps", "sched_temperature", "sched_top_k", "sched_seed"), c.sched[:5]))
    if c.augment is not None:
        opts.update({"aug_" + k: v for k, v in c.augment[0].items()}, aug_seed=c.augment[1])
    if c.loss is not None:
        opts.update(class_weights=c.loss[0], label_smoothing=c.loss[1], box_overlap=c.loss[2])
    if gaussian:
        opts.update(box_nll_weight=c.box_nll_weight)
    eng = LayoutEngine(cfg, dev, precision=c.precision, padded_slots=c.masked or c.attention == "slot", **opts)
    if gaussian:        # the scale rows start at zero (sigma at its midpoint, no gradient path through them yet): give them values
        p = {k: v.cpu().clone() for k, v in eng.named_params().items()}
        g = torch.Generator().manual_seed(5)
        nc = cfg.n_classes
        p["head_w"][nc + 4:nc + 8] = (torch.rand(4, cfg.d, generator=g) * 2 - 1) * cfg.d ** -0.5
        p["head_b"][nc + 4:nc + 8] = torch.rand(4, generator=g) * 2 - 1
        eng.load_params(p)
    assert eng.gelu_grad_saved == c.gelu_grad_saved and eng.pair_backward == c.paired and eng.bf16_store == c.store_bf16
    return cfg, eng


def _set_counters(eng, c):
    for name, setter in (("drop_step", eng.set_dropout_step), ("sched_step", eng.set_sched_step), ("aug_step", eng.set_augment_step)):
        if name in c.counters():
            setter(c.counters()[name])


def _traced(dev, cfg, eng, c, batch, what):
    """test_hip_step_trace's driver: an untraced step, the same step traced (bitwise the same), the per-launch check with the
    worst error per launch kind printed -> the records"""
    b = {k: v.to(dev) for k, v in batch.items()}
    _set_counters(eng, c)
    loss0 = eng.forward_backward(b).clone()
    grads0 = eng.grads.clone()
    for name, read in (("drop_step", "dropout_step"), ("sched_step", "sched_step"), ("aug_step", "augment_step")):
        if name in c.counters():
            assert getattr(eng, read) == c.counters()[name] + 1
    _set_counters(eng, c)
    records, state = step_trace.trace(eng, b)
    assert torch.equal(eng.loss_out, loss0) and torch.equal(eng.grads, grads0), "the traced run is not bitwise the untraced one"
    log = []
    try:
        step_trace.check(records, state, cfg, c, batch, log=log)
    finally:
        print("\n%s: worst |err| vs fp64 per launch kind: %s" % (what, _summary(log)))
    return records


FACTORED = [pytest.param(_p, _s, False, None, id="%s-%s" % (_p, _IDS[id(_s)])) for _s in (F1, F2, F3) for _p in SS.PRECISIONS]
for _p in ("fp32", "bf16"):
    FACTORED += [pytest.param(_p, F1, True, None, id="%s-%s-variable-n" % (_p, _IDS[id(F1)])),
                 # clip 0: 20 valid of 64 slots - the second tile of each of its frames is wholly padded
                 pytest.param(_p, F2, "prefix", None, id="%s-%s-prefix-valid" % (_p, _IDS[id(F2)])),
                 pytest.param(_p, F1, True, DROPOUT, id="%s-%s-variable-n-dropout" % (_p, _IDS[id(F1)]))]


@pytest.mark.parametrize("precision,kw,variable_n,dropout", FACTORED)
def test_every_launch_of_the_factored_step_matches_fp64_on_its_inputs(dev, precision, kw, variable_n, dropout):
    c = SS.Contract(precision, "factored", masked=bool(variable_n), dropout=dropout)
    cfg, eng = _engine(dev, kw, c)
    batch = _batch(cfg, variable_n)
    if variable_n:
        assert bool((batch["valid"] == 0).any())
    records = _traced(dev, cfg, eng, c, batch, "%s factored %s variable_n=%s dropout=%s" % (precision, kw, variable_n, dropout is not None))
    L = cfg.n_layers
    assert tuple(eng.lse.shape)[0] == L // 2                # log-sum-exp rows for the odd layers alone
    names = [r["name"] for r in records]
    assert not any(n.startswith("vlg_attention_clip") for n in names)
    sfx = "_bf16" if precision == "bf16" else ""
    assert names.count("vlg_attention_frame_fwd" + sfx) == names.count("vlg_attention_frame_bwd" + sfx) == L // 2
    assert names.count("vlg_attention_fwd" + sfx) == names.count("vlg_attention_bwd" + sfx) == L - L // 2


EVERYTHING = dict(attention="factored", box_nll_weight=W_NLL, loss=LOSS, sched=SCHED, augment=AUGMENT, dropout=DROPOUT)
OPTIONS = []
for _p in ("fp32", "bf16"):
    OPTIONS += [pytest.param(_p, S1, dict(box_nll_weight=W_NLL), id="%s-gaussian-head" % _p),
                pytest.param(_p, S1, dict(loss=LOSS), id="%s-loss-options" % _p),
                pytest.param(_p, S1, dict(sched=SCHED), id="%s-sched-argmax-ramp" % _p),
                pytest.param(_p, S1, dict(attention="clip", augment=AUGMENT), id="%s-augment-clip" % _p),
                pytest.param(_p, F1, EVERYTHING, id="%s-everything-factored" % _p)]
OPTIONS.insert(3, pytest.param("fp32", S1, dict(sched=SCHED_SAMPLED), id="fp32-sched-sampled-top5"))


@pytest.mark.parametrize("precision,kw,options", OPTIONS)
def test_every_launch_of_a_step_with_options_matches_fp64_on_its_inputs(dev, precision, kw, options):
    c = SS.Contract(precision, masked=True, **options)
    cfg, eng = _engine(dev, kw, c, gaussian="box_nll_weight" in options)
    batch = _batch(cfg, True)
    assert bool((batch["valid"] == 0).any())
    records = _traced(dev, cfg, eng, c, batch, "%s %s %s" % (precision, kw, sorted(options)))
    names = [r["name"] for r in records]
    assert names.count("vlg_dropout_step_advance") == len(c.counters())
    assert names.count("vlg_layout_loss_ext" if c.loss is not None else "vlg_layout_loss") == 1
    assert names.count("vlg_layout_box_nll") == int(cfg.gaussian_box)
    assert names.count("vlg_layout_mix_inputs") == int(c.sched is not None) and names.count("vlg_embed_fwd") == 1 + int(c.sched is not None)
    assert names.count("vlg_layout_augment") == int(c.augment is not None) and (c.augment is None or names[0] == "vlg_layout_augment")
    if c.augment is not None:      # the drop coin fell for some track: the masks and the loss have something to get wrong
        aug = eng.augmented_batch()
        assert float(aug["valid"].sum()) < float(batch["valid"].sum())
