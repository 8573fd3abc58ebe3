"""GPU: augmentation in LayoutEngine - the training step at (2,4,3), d = 64 (per-clip attention kinds: (2,4,8)) runs on
the batch the CPU restatement of the rule (tests/augment_ref.py) gives at the engine's counter, through the same kernels as
a plain engine handed that batch: loss and gradients bit for bit."""
import pytest
import torch

import augment_ref as A
from oracle import layout_spec as O

pytestmark = pytest.mark.gpu

NC = A.NC
KW = dict(B=2, T=4, N=3, d=64)
CLIP_N = 8              # per-clip attention needs T*N % 32 == 0 (LayoutConfig.validate): those cases run at (2,4,8), the smallest
KEYS = ("slot_class", "slot_box", "tgt_box", "valid")
ALL = dict(aug_flip=0.5, aug_zoom=0.3, aug_shift=0.2, aug_jitter=0.1, aug_drop=0.3)
ZERO = dict(aug_flip=0.0, aug_zoom=0.0, aug_shift=0.0, aug_jitter=0.0, aug_drop=0.0)


def _n(attention):
    return KW["N"] if attention == "slot" else CLIP_N


def _engine(dev, n_layers=2, attention="slot", precision="fp32", padded=False, **kw):
    from vlg.engine import LayoutEngine
    from vlg.spec import LayoutConfig
    cfg = LayoutConfig(attention=attention, n_layers=n_layers, **dict(KW, N=_n(attention)))
    return LayoutEngine(cfg, dev, seed=1024, precision=precision, padded_slots=padded, **kw)


def _batch(padded=False, seed=7, N=KW["N"]):
    b = O.synthetic_batch(KW["B"], KW["T"], N, seed=seed)
    if padded:                                          # the last slot of clip 1 is padded in every frame (the generator's convention)
        b["slot_class"][1, :, N - 1] = NC
        b["valid"][1, :, N - 1] = 0.0
    return b


def to_dev(batch, dev):
    return {k: v.to(dev) for k, v in batch.items()}


def _want(batch, k, seed=0, **aug):
    """the restatement for the engine's keywords"""
    return A.augment(batch, k, seed, **{name[4:]: v for name, v in aug.items()})


def _same_batch(eng, want, what=""):
    got = eng.augmented_batch()
    assert set(got) == set(KEYS)
    for key in KEYS:
        g = got[key].cpu()
        assert tuple(g.shape) == tuple(want[key].shape), key
        assert torch.equal(g, want[key]) if key == "slot_class" else torch.equal(A.bits(g), A.bits(want[key])), what + key


def _launches(eng, b):
    from vlg import hip
    names = []
    previous, hip.tracer = hip.tracer, lambda name, args: names.append(name)
    try:
        eng.train_step(b)
        torch.cuda.synchronize()
    finally:
        hip.tracer = previous
    return names


def test_all_knobs_zero_is_the_engine_without_the_option(dev):
    """every knob 0.0 turns the option on and changes nothing: the step reads a copy of the batch through the same kernels"""
    b = to_dev(_batch(), dev)
    on, off = _engine(dev, **ZERO), _engine(dev)
    for e in (on, off):
        for _ in range(3):
            e.train_step(b)
    assert torch.equal(on.params, off.params) and torch.equal(on.loss_out, off.loss_out)
    assert torch.equal(on.exp_avg, off.exp_avg) and torch.equal(on.exp_avg_sq, off.exp_avg_sq)
    for key, t in on.augmented_batch().items():
        assert torch.equal(t, b[key]), key
    assert on.augment_step == 3 and on.state_dict()["augment_step"] == 3
    # off: nothing allocated, no counter, nothing in the checkpoint, the accessors refuse, no launch of the option's
    assert off.aug_counter is None and not hasattr(off, "aug_cls") and not hasattr(off, "aug_valid")
    assert "augment_step" not in off.state_dict() and set(off.state_dict()) == set(on.state_dict()) - {"augment_step"}
    for f in (lambda: off.augment_step, lambda: off.set_augment_step(0), off.augmented_batch):
        with pytest.raises(RuntimeError):
            f()
    one = _engine(dev, aug_jitter=0.0)                                  # any knob given turns it on
    assert one.aug_counter is not None
    with pytest.raises(RuntimeError):
        one.augmented_batch()                                           # (there has been no training step yet)
    plain, with_option = _launches(off, b), _launches(on, b)
    assert "vlg_layout_augment" not in plain and plain.count("vlg_dropout_step_advance") == 0
    assert len(with_option) == len(plain) + 2                           # the augment kernel in front, its counter's advance behind
    assert with_option[0] == "vlg_layout_augment" and with_option[1:].count("vlg_dropout_step_advance") == 1
    rest = list(with_option[1:])
    rest.remove("vlg_dropout_step_advance")
    assert rest == plain


@pytest.mark.parametrize("n_layers,attention,precision", [(2, "slot", "fp32"), (1, "slot", "fp32"), (2, "clip", "fp32"),
                                                          (2, "factored", "fp32"), (2, "slot", "bf16")])
def test_all_knobs_on_runs_the_restatement_batch(dev, n_layers, attention, precision):
    """augmented_batch() is the restatement at the engine's counter; loss and every gradient are a plain engine's on the
    uploaded restatement, bit for bit.  The per-clip kinds hold a padded slot and drop tracks."""
    per_clip = attention != "slot"
    batch = _batch(per_clip, N=_n(attention))
    b = to_dev(batch, dev)
    eng = _engine(dev, n_layers, attention, precision, padded=per_clip, aug_seed=77, **ALL)
    plain = _engine(dev, n_layers, attention, precision, padded=per_clip)
    eng.set_augment_step(5)
    loss = eng.forward_backward(b)
    want = _want(batch, 5, 77, **ALL)
    _same_batch(eng, want)
    assert bool(want["drop"].any()) and not bool(want["drop"].all())
    assert not torch.equal(want["slot_box"], batch["slot_box"]) and not torch.equal(want["tgt_box"], batch["tgt_box"])
    if per_clip:
        assert bool((want["slot_class"][1, :, -1] == NC).all())
    loss_plain = plain.forward_backward(to_dev(dict(batch, **{k: want[k] for k in KEYS}), dev))
    assert torch.equal(loss, loss_plain)
    assert bool(torch.isfinite(eng.grads).all()) and torch.equal(eng.grads, plain.grads)
    for name, g in eng.named_grads().items():
        assert torch.equal(g, plain.named_grads()[name]), name
    # the caller's batch was read, not modified; the plain engine on the caller's batch computes something else
    for k in batch:
        assert torch.equal(b[k].cpu(), batch[k]), k
    assert not torch.equal(plain.forward_backward(b), loss)


def test_counter_advances_round_trips_and_reproduces(dev):
    batch = _batch()
    b = to_dev(batch, dev)
    knobs = dict(ALL, aug_seed=0xC0FFEE1234567)
    eng = _engine(dev, **knobs)
    assert eng.augment_step == 0
    seen = []
    for k in (0, 1):
        eng.forward_backward(b)                         # (no optimiser: both steps run on the same weights)
        assert eng.augment_step == k + 1
        _same_batch(eng, _want(batch, k, knobs["aug_seed"], **ALL), "step %d " % k)
        seen.append({key: t.clone() for key, t in eng.augmented_batch().items()})
    assert not torch.equal(seen[0]["slot_box"], seen[1]["slot_box"])
    g1, l1 = eng.grads.clone(), eng.loss_out.clone()
    eng.set_augment_step(1)                             # the same step again, bit for bit
    eng.forward_backward(b)
    for key, t in eng.augmented_batch().items():
        assert torch.equal(A.bits(t) if t.is_floating_point() else t, A.bits(seen[1][key]) if t.is_floating_point() else seen[1][key])
    assert torch.equal(eng.grads, g1) and torch.equal(eng.loss_out, l1) and eng.augment_step == 2
    for bad in (-1, 2 ** 31):
        with pytest.raises(ValueError):
            eng.set_augment_step(bad)
    eng.set_augment_step(2 ** 31 - 1)                   # the last legal value reaches the kernel as it is
    eng.forward_backward(b)
    _same_batch(eng, _want(batch, 2 ** 31 - 1, knobs["aug_seed"], **ALL), "step 2^31 - 1 ")
    eng.set_augment_step(2)
    # the checkpoint carries the counter
    eng.train_step(b)
    sd = eng.state_dict()
    assert sd["augment_step"] == 3
    other = _engine(dev, **knobs)
    other.load_state_dict(sd)
    assert other.augment_step == 3
    eng.train_step(b)
    other.train_step(b)
    assert torch.equal(other.params, eng.params) and torch.equal(other.augmented_batch()["slot_box"], eng.augmented_batch()["slot_box"])
    _same_batch(other, _want(batch, 3, knobs["aug_seed"], **ALL), "after the checkpoint ")


def test_captured_step_replays_like_eager_steps(dev):
    """three replays of the captured step == three eager steps of a twin engine, bit for bit; each replay reads the counter
    the one before advanced, and capture itself does not move it"""
    batch = _batch()
    b = to_dev(batch, dev)
    knobs = dict(ALL, aug_seed=3)
    eager = _engine(dev, **knobs)
    for _ in range(3):
        eager.train_step(b)
    graph = _engine(dev, **knobs)
    run = graph.capture_train_step(b)
    assert graph.augment_step == 0
    boxes = []
    for k in range(3):
        run(b)
        _same_batch(graph, _want(batch, k, 3, **ALL), "replay %d " % k)
        boxes.append(graph.augmented_batch()["slot_box"].clone())
    torch.cuda.synchronize()
    assert graph.augment_step == 3 == eager.augment_step
    assert torch.equal(graph.params, eager.params) and torch.equal(graph.loss_out, eager.loss_out)
    assert torch.equal(graph.exp_avg, eager.exp_avg) and not torch.equal(boxes[0], boxes[1])


def test_scheduled_sampling_runs_on_the_augmented_batch(dev):
    """sched_sampling = 1.0 as well: both passes read the augmented batch - frame 0 and the padded tokens of sched_inputs()
    are the augmented inputs - and the loss is taken against aug_tgt_box / aug_valid: the step is a scheduled-sampling
    engine's on the uploaded restatement, bit for bit"""
    batch = _batch(True)
    b = to_dev(batch, dev)
    eng = _engine(dev, padded=True, sched_sampling=1.0, aug_seed=4, **ALL)
    twin = _engine(dev, padded=True, sched_sampling=1.0)
    loss = eng.forward_backward(b)
    want = _want(batch, 0, 4, **ALL)
    _same_batch(eng, want)
    mc, mb = (t.cpu() for t in eng.sched_inputs())
    assert torch.equal(mc[:, 0], want["slot_class"][:, 0]) and torch.equal(A.bits(mb[:, 0]), A.bits(want["slot_box"][:, 0]))
    pad = want["slot_class"] >= NC
    assert bool(pad[:, 1:].any()) and torch.equal(mc[pad], want["slot_class"][pad]) and torch.equal(A.bits(mb[pad]), A.bits(want["slot_box"][pad]))
    live = ~pad
    live[:, 0] = False
    assert bool((mb[live] != want["slot_box"][live]).any())               # the rest was replaced by the model's own predictions
    loss_twin = twin.forward_backward(to_dev(dict(batch, **{k: want[k] for k in KEYS}), dev))
    assert torch.equal(loss, loss_twin) and torch.equal(eng.grads, twin.grads)
    assert torch.equal(eng.sched_inputs()[1], twin.sched_inputs()[1])
    assert eng.sched_step == 1 and eng.augment_step == 1


def test_dropout_and_augmentation_count_separately(dev):
    b = to_dev(_batch(), dev)
    eng = _engine(dev, dropout=0.25, dropout_seed=9, **ALL)
    eng.forward_backward(b)
    assert eng.dropout_step == 1 and eng.augment_step == 1
    eng.set_augment_step(5)
    assert eng.dropout_step == 1
    eng.forward_backward(b)
    assert eng.dropout_step == 2 and eng.augment_step == 6
    eng.set_dropout_step(0)
    assert eng.augment_step == 6
    sd = eng.state_dict()
    assert sd["dropout_step"] == 0 and sd["augment_step"] == 6


def test_evaluation_is_untouched(dev):
    """a bare forward(), rollout() and accumulate_metrics() of an augmenting engine equal a plain engine's, bit for bit, and
    do not move the counter"""
    b = to_dev(_batch(), dev)
    on, off = _engine(dev, **ALL), _engine(dev)
    assert torch.equal(on.forward(b), off.forward(b)) and torch.equal(on.out, off.out)
    recs = []
    for e in (on, off):
        rec = e.metrics_record()
        e.accumulate_metrics(b, rec)
        recs.append(rec)
    assert torch.equal(recs[0].counts, recs[1].counts) and torch.equal(recs[0].sums, recs[1].sums)
    ga, gb = on.rollout(b["slot_class"], b["slot_box"], steps=2), off.rollout(b["slot_class"], b["slot_box"], steps=2)
    assert torch.equal(ga[0], gb[0]) and torch.equal(ga[1], gb[1])
    assert on.augment_step == 0
    on.forward_backward(b)                                              # and the training entry point does augment
    off.forward_backward(b)
    assert not torch.equal(on.out, off.out) and on.augment_step == 1


def test_refusals(dev):
    for kw in (dict(aug_flip=1.5), dict(aug_flip=-0.1), dict(aug_flip=float("nan")), dict(aug_zoom=0.6), dict(aug_shift=0.51),
               dict(aug_jitter=0.3), dict(aug_jitter=float("nan")), dict(aug_drop=1.0), dict(aug_drop=-0.5)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            _engine(dev, **kw)
    for attention in ("clip", "factored"):                              # the unmasked per-clip kernels would attend to dropped slots
        with pytest.raises(ValueError, match="padded_slots"):
            _engine(dev, attention=attention, padded=False, aug_drop=0.1)
        _engine(dev, attention=attention, padded=True, aug_drop=0.1)
        _engine(dev, attention=attention, padded=False, aug_drop=0.0, aug_flip=0.5)
    _engine(dev, padded=False, aug_drop=0.1)                            # per-slot attention never looks across slots
    eng = _engine(dev, ema_decay=0.9, **ALL)
    b = to_dev(_batch(), dev)
    with eng.ema_weights():
        for f in (eng.train_step, eng.forward_backward):
            with pytest.raises(RuntimeError, match="ema_weights"):
                f(b)
        eng.forward(b)                                  # evaluation on the averaged weights is untouched
    assert eng.augment_step == 0
