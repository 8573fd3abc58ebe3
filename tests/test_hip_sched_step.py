"""GPU: scheduled sampling in LayoutEngine - the two-pass training step at (2,4,3), d = 64, one or two layers, against the
CPU restatement of the rule (tests/sched_ref.py) on the engine's own first-pass outputs and the CPU specification's
gradients on the mixed batch with the true targets."""
import pytest
import torch

import sched_ref as S
import step_stages as SS
from helpers import check_close, vs_cpu32
from oracle import layout_spec as O

pytestmark = pytest.mark.gpu

NC = S.NC
KW = dict(B=2, T=4, N=3, d=64)


CLIP_N = 8              # per-clip attention needs T*N % 32 == 0 (LayoutConfig.validate): its case runs at (2,4,8), the smallest


def _cfg(n_layers=2, attention="slot"):
    from vlg.spec import LayoutConfig
    return LayoutConfig(attention=attention, n_layers=n_layers, **dict(KW, N=CLIP_N if attention == "clip" else KW["N"]))


def _engine(dev, n_layers=2, attention="slot", precision="fp32", padded=False, **kw):
    from vlg.engine import LayoutEngine
    return LayoutEngine(_cfg(n_layers, attention), dev, seed=1024, precision=precision, padded_slots=padded, **kw)


def _batch(padded=False, seed=7, N=KW["N"]):
    b = O.synthetic_batch(KW["B"], KW["T"], N, seed=seed)
    if padded:                                          # the last slot of clip 1 is padded in every frame (the generator's convention)
        b["slot_class"][1, :, N - 1] = NC
        b["valid"][1, :, N - 1] = 0.0
    return b


def to_dev(batch, dev):
    return {k: v.to(dev) for k, v in batch.items()}


def _expected(eng, batch, dev, k=0, eps=1.0, **kw):
    """the mixed inputs the rule gives on the engine's own evaluation outputs for this batch"""
    eng.forward(to_dev(batch, dev))
    M = batch["slot_class"].numel()
    out = eng.out[:M].cpu()
    return S.mix_inputs(out, batch["slot_class"], batch["slot_box"], NC, k, S.thr_max(eps), **kw) + (out,)


def _check_inputs(eng, batch, want_c, want_b, rep, out):
    got_c, got_b = (t.cpu() for t in eng.sched_inputs())
    assert tuple(got_c.shape) == tuple(batch["slot_class"].shape) and tuple(got_b.shape) == tuple(batch["slot_box"].shape)
    assert torch.equal(got_c, want_c)
    assert torch.equal(got_b[~rep], batch["slot_box"][~rep])
    B, T, N = got_c.shape
    b, t, n = torch.meshgrid(torch.arange(B), torch.arange(T), torch.arange(N), indexing="ij")
    rows = ((b * N + n) * T + (t - 1))[rep]
    vs_cpu32(got_b[rep], want_b[rep], torch.sigmoid(out[:, NC:NC + 4])[rows], "boxes of replaced tokens")


def test_zero_probability_is_the_engine_without_the_option(dev):
    """sched_sampling = 0.0: the second pass reads a copy of the truth through the same kernels - parameters and loss scalars
    after three steps are those of an engine built without the argument, bit for bit"""
    b = to_dev(_batch(), dev)
    on, off = _engine(dev, sched_sampling=0.0), _engine(dev)
    for e in (on, off):
        for _ in range(3):
            e.train_step(b)
    assert torch.equal(on.params, off.params) and torch.equal(on.loss_out, off.loss_out) and torch.equal(on.exp_avg_sq, off.exp_avg_sq)
    c, bx = on.sched_inputs()
    assert torch.equal(c, b["slot_class"]) and torch.equal(bx, b["slot_box"]) and on.sched_step == 3
    # off: nothing allocated, nothing in the checkpoint, the accessors refuse
    assert off.sched_counter is None and not hasattr(off, "mix_cls") and "sched_step" not in off.state_dict()
    for f in (lambda: off.sched_step, lambda: off.set_sched_step(0), off.sched_inputs):
        with pytest.raises(RuntimeError):
            f()


@pytest.mark.parametrize("n_layers,attention,padded", [(2, "slot", False), (1, "slot", False), (2, "clip", True)])
def test_full_replacement_step_matches_the_specification(dev, n_layers, attention, padded):
    """sched_sampling = 1.0, temperature 0: sched_inputs() is the restatement on forward()'s outputs, and the gradients are the
    CPU specification's on that mixed batch with the TRUE targets, at the step tests' 1e-4 bars.  The per-clip case holds a
    padded slot and runs at (2,4,8): the configuration refuses attention="clip" unless T*N is a multiple of 32."""
    from vlg.spec import param_shapes
    batch = _batch(padded, N=CLIP_N if attention == "clip" else KW["N"])
    eng = _engine(dev, n_layers, attention, padded=padded, sched_sampling=1.0)
    want_c, want_b, rep, _, out = _expected(eng, batch, dev)
    assert torch.equal(rep, S.eligible(batch["slot_class"], NC)) and bool(rep.any())
    assert not torch.equal(want_c, batch["slot_class"])
    b = to_dev(batch, dev)
    loss = eng.forward_backward(b)
    _check_inputs(eng, batch, want_c, want_b, rep, out)
    if padded:
        assert bool((want_c[1, :, -1] == NC).all()) and torch.equal(eng.sched_inputs()[1][1, :, -1].cpu(), batch["slot_box"][1, :, -1])
    mixed = dict(batch, slot_class=want_c, slot_box=want_b.float())
    p = O.init_params(param_shapes(_cfg(n_layers, attention)), seed=1024)
    parts, grads = O.loss_and_grads(p, mixed, n_layers, attention=attention)
    check_close(loss, torch.tensor(parts), rtol=1e-4, atol=1e-6, what="pass 2 loss parts")
    for name, g in eng.named_grads().items():
        scale = max(float(grads[name].abs().max()), 1e-6)
        check_close(g / scale, grads[name] / scale, rtol=1e-4, atol=2e-5, what="grad " + name)
    # the true batch gives other gradients: the second pass did read the mixed inputs, embedding backward included
    _, plain = O.loss_and_grads(p, batch, n_layers, attention=attention)
    assert float((plain["cls_emb"] - grads["cls_emb"]).abs().max()) > 1e-3 * float(grads["cls_emb"].abs().max())
    for k in ("tgt_class", "tgt_box", "valid", "slot_class", "slot_box"):       # the caller's batch is only read
        assert torch.equal(b[k].cpu(), batch[k])


def test_full_replacement_step_bf16(dev):
    """precision = "bf16": the mixed inputs are the rule on that mode's own outputs; loss and gradients against the emulated
    bf16 oracle of tests/step_stages.py on the mixed batch, at the mode's end-to-end bars for this shape"""
    from vlg.spec import param_shapes
    kw = dict(n_layers=2, **KW)
    batch = _batch()
    eng = _engine(dev, precision="bf16", sched_sampling=1.0)
    want_c, want_b, rep, _, out = _expected(eng, batch, dev)
    loss = eng.forward_backward(to_dev(batch, dev)).cpu()
    _check_inputs(eng, batch, want_c, want_b, rep, out)
    mixed = dict(batch, slot_class=want_c, slot_box=want_b.float())
    p = O.init_params(param_shapes(_cfg()), seed=1024)
    l_ref, g_ref = SS.emulated_oracle(_cfg(), "bf16", p, mixed, "slot", masked=False)
    bar_loss, bar_grad, _ = SS.end_to_end_bars(kw, "bf16", seed=7)
    errs = {n: float((g.cpu().double() - g_ref[n]).norm() / g_ref[n].norm()) for n, g in eng.named_grads().items() if n in bar_grad}
    print("\nbf16 scheduled sampling: loss off by %.2e (bar %.2e); gradients (rel L2 / bar): %s" % (
        abs(float(loss[0]) - float(l_ref[0])) / abs(float(l_ref[0])), bar_loss,
        ", ".join("%s %.1e/%.1e" % (n, e, bar_grad[n]) for n, e in errs.items())))
    assert bool(torch.isfinite(eng.grads).all())
    assert abs(float(loss[0]) - float(l_ref[0])) <= bar_loss * abs(float(l_ref[0]))
    assert len(errs) >= len(g_ref) - 2 * kw["n_layers"]
    for name, err in errs.items():
        assert err <= bar_grad[name], (name, err, bar_grad[name])


def test_counter_advances_round_trips_and_reproduces(dev):
    batch = _batch()
    b = to_dev(batch, dev)
    knobs = dict(sched_sampling=0.5, sched_temperature=0.8, sched_top_k=5, sched_seed=77)
    eng = _engine(dev, **knobs)
    assert eng.sched_step == 0
    seen = []
    for k in (0, 1):
        eng.forward_backward(b)                         # (no optimiser: both steps run on the same weights)
        assert eng.sched_step == k + 1
        seen.append(tuple(t.clone() for t in eng.sched_inputs()))
        rep = S.replaced(batch["slot_class"], NC, k, S.thr_max(0.5), 0, 77)
        assert torch.equal((seen[-1][1].cpu() != batch["slot_box"]).any(-1), rep), "replaced set at step %d" % k
    assert not torch.equal(seen[0][1], seen[1][1])
    g1, l1 = eng.grads.clone(), eng.loss_out.clone()
    eng.set_sched_step(1)                               # the same step again, bit for bit
    eng.forward_backward(b)
    assert torch.equal(eng.sched_inputs()[0], seen[1][0]) and torch.equal(eng.sched_inputs()[1], seen[1][1])
    assert torch.equal(eng.grads, g1) and torch.equal(eng.loss_out, l1) and eng.sched_step == 2
    with pytest.raises(ValueError):
        eng.set_sched_step(-1)
    # the checkpoint carries the counter
    eng.train_step(b)
    sd = eng.state_dict()
    assert sd["sched_step"] == 3
    other = _engine(dev, **knobs)
    other.load_state_dict(sd)
    assert other.sched_step == 3
    eng.train_step(b)
    other.train_step(b)
    assert torch.equal(other.params, eng.params) and torch.equal(other.sched_inputs()[1], eng.sched_inputs()[1])
    # a step the guarded optimiser skips still advances it
    guarded = _engine(dev, skip_nonfinite=True, **knobs)
    before = guarded.params.clone()
    guarded.train_step(dict(b, slot_box=torch.full_like(b["slot_box"], float("nan"))))
    assert torch.equal(guarded.params, before) and guarded.sched_step == 1


def test_ramp_reaches_the_engine(dev):
    """sched_ramp_steps = 4 at eps_max = 1: step 0 replaces about a quarter of the eligible tokens as the restatement says,
    step 3 all of them"""
    batch = _batch()
    b = to_dev(batch, dev)
    eng = _engine(dev, sched_sampling=1.0, sched_ramp_steps=4, sched_seed=5)
    for k in (0, 3):
        eng.set_sched_step(k)
        eng.forward_backward(b)
        rep = S.replaced(batch["slot_class"], NC, k, S.TWO24, 4, 5)
        assert torch.equal((eng.sched_inputs()[1].cpu() != batch["slot_box"]).any(-1), rep), k
    assert torch.equal(rep, S.eligible(batch["slot_class"], NC))


def test_captured_step_replays_like_eager_steps(dev):
    """three replays of the captured two-pass step == three eager steps of a twin engine, bit for bit; each replay reads
    the counter the one before advanced"""
    b = to_dev(_batch(), dev)
    knobs = dict(sched_sampling=0.5, sched_seed=3)
    eager = _engine(dev, **knobs)
    for _ in range(3):
        eager.train_step(b)
    graph = _engine(dev, **knobs)
    run = graph.capture_train_step(b)
    assert graph.sched_step == 0                        # capture does not move the trajectory
    mixes = []
    for _ in range(3):
        run(b)
        mixes.append(graph.sched_inputs()[1].clone())
    torch.cuda.synchronize()
    assert graph.sched_step == 3 == eager.sched_step
    assert torch.equal(graph.params, eager.params) and torch.equal(graph.loss_out, eager.loss_out)
    assert torch.equal(graph.exp_avg, eager.exp_avg) and torch.equal(mixes[2], eager.sched_inputs()[1])
    assert not torch.equal(mixes[0], mixes[1])


def test_first_pass_is_evaluation_under_dropout(dev):
    """with dropout on as well: the mixed inputs are the prediction from forward()'s logits, not from a dropped forward; the
    second pass does drop"""
    batch = _batch()
    eng = _engine(dev, sched_sampling=1.0, dropout=0.25, dropout_seed=9)
    want_c, want_b, rep, _, out = _expected(eng, batch, dev)
    eng.forward_backward(to_dev(batch, dev))
    _check_inputs(eng, batch, want_c, want_b, rep, out)
    assert eng.dropout_step == 1 and eng.sched_step == 1
    assert not torch.equal(eng.out[:out.shape[0]].cpu(), out)           # pass 2 ran on other inputs, dropped


def test_refusals(dev):
    for bad in (1.5, -0.1, float("nan")):
        with pytest.raises(ValueError, match="sched_sampling"):
            _engine(dev, sched_sampling=bad)
    for kw in (dict(sched_top_k=NC + 1), dict(sched_top_k=-1), dict(sched_temperature=-1.0), dict(sched_temperature=float("inf")),
               dict(sched_ramp_steps=-1)):
        with pytest.raises(ValueError, match="sched_"):
            _engine(dev, sched_sampling=0.5, **kw)
    eng = _engine(dev, sched_sampling=0.5, ema_decay=0.9)
    b = to_dev(_batch(), dev)
    with eng.ema_weights():
        for f in (eng.train_step, eng.forward_backward):
            with pytest.raises(RuntimeError, match="ema_weights"):
                f(b)
        eng.forward(b)                                  # evaluation on the averaged weights is untouched
    assert eng.sched_step == 0


@pytest.mark.parametrize("precision,attention", [("fp32x3", "slot"), ("bf16_mfma", "slot"), ("fp32", "clip"), ("bf16", "clip")])
def test_other_modes_mix_their_own_outputs(dev, precision, attention):
    """the remaining precision modes, and per-clip attention without validity masks: the mixed inputs are the rule on that
    mode's own forward() outputs, and the step's gradients are finite"""
    batch = _batch(N=CLIP_N if attention == "clip" else KW["N"])
    eng = _engine(dev, attention=attention, precision=precision, sched_sampling=1.0)
    want_c, want_b, rep, _, out = _expected(eng, batch, dev)
    eng.train_step(to_dev(batch, dev))
    _check_inputs(eng, batch, want_c, want_b, rep, out)
    assert bool(torch.isfinite(eng.grads).all()) and bool(torch.isfinite(eng.loss_out).all())


class _Reducer:
    """what LayoutEngine.train_step asks of a gradient reducer, recording the buckets it is told about"""
    grad_scale = 1.0

    def __init__(self):
        self.tags = []

    def ready(self, tag):
        self.tags.append(tag)

    def wait(self, keep=()):
        pass


def test_reducer_sees_the_second_pass_only(dev):
    """with a data-parallel reducer attached the option tells it about each gradient bucket once, as the step without it does,
    and the parameters are those of the step without a reducer"""
    b = to_dev(_batch(), dev)
    knobs = dict(sched_sampling=0.5, sched_seed=3)
    with_r, without, plain = _engine(dev, **knobs), _engine(dev, **knobs), _engine(dev)
    r, r0 = _Reducer(), _Reducer()
    with_r.train_step(b, r)
    without.train_step(b)
    plain.train_step(b, r0)
    assert r.tags == r0.tags == ["head", "l1", "l0", "embed"]
    assert torch.equal(with_r.params, without.params) and with_r.sched_step == 1
