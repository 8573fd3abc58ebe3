"""LayoutEngine(class_weights=, label_smoothing=, box_overlap=) at (2,4,8), d = 64, 2 layers: one training step against the
float64 specification's encoder with tests/loss_ext_ref.py on top, which entry the step launches, graph capture, and the
loss validate() reports.  Bars: test_hip_step.py's (test_step_matches_oracle for fp32 - loss parts rtol 1e-4 / atol 1e-6,
every gradient scaled by its largest value rtol 1e-4 / atol 2e-5 - and test_bf16_projection_mode's for bf16: 4 x the
mode's distance from the specification, step_stages.end_to_end_bars)."""
import pytest
import torch

import loss_ext_ref as R
import step_stages as SS
from helpers import check_close, reference_args
from oracle import layout_spec as O

pytestmark = pytest.mark.gpu

KW = dict(B=2, T=4, N=8, d=64, n_layers=2)
WEIGHTS = [round(0.25 + 0.15 * ((7 * c) % 20), 4) for c in range(20)]
WEIGHTS[3] = 0.0
ALL = dict(class_weights=WEIGHTS, label_smoothing=0.1, box_overlap="giou")


def engine(dev, precision="fp32", **kw):
    from vlg.engine import LayoutEngine
    from vlg.spec import LayoutConfig
    return LayoutEngine(LayoutConfig(**KW), dev, seed=1024, precision=precision, **kw)


def to_dev(batch, dev):
    return {k: v.to(dev) for k, v in batch.items()}


@pytest.fixture(scope="module")
def spec64():
    """(batch, loss parts, gradients) of one step with every option on: the specification's encoder in float64"""
    from vlg.spec import LayoutConfig, param_shapes
    cfg = LayoutConfig(**KW)
    p = {k: v.double() for k, v in O.init_params(param_shapes(cfg), seed=1024).items()}
    batch = O.synthetic_batch(cfg.B, cfg.T, cfg.N, seed=7, variable_n=True, min_valid=3)
    parts, grads = R.loss_and_grads(p, batch, cfg.n_layers, torch.tensor(WEIGHTS, dtype=torch.float64), 0.1, "giou")
    return batch, parts, grads


def test_step_with_every_option_matches_fp64(dev, spec64):
    batch, parts, grads = spec64
    eng = engine(dev, **ALL)
    loss = eng.forward_backward(to_dev(batch, dev))
    print("\nloss parts gpu %s fp64 %s" % (loss.tolist(), list(parts)))
    check_close(loss, torch.tensor(parts, dtype=torch.float64), rtol=1e-4, atol=1e-6, what="loss parts")
    for name, g in eng.named_grads().items():
        scale = max(float(grads[name].abs().max()), 1e-6)
        check_close(g / scale, grads[name] / scale, rtol=1e-4, atol=2e-5, what="grad " + name)


def test_bf16_step_with_every_option(dev, spec64):
    batch, parts, grads = spec64
    bar_loss, bar_grad, _ = SS.end_to_end_bars(KW, "bf16", variable_n=True, seed=7)
    assert bar_loss < 2e-2 and max(bar_grad.values()) <= 5e-2
    eng = engine(dev, "bf16", **ALL)
    loss = eng.forward_backward(to_dev(batch, dev)).cpu()
    errs = {n: float((g.cpu().double() - grads[n]).norm() / grads[n].norm()) for n, g in eng.named_grads().items() if n in bar_grad}
    print("\nbf16: loss off by %.2e (bar %.2e); gradients (rel L2 / bar): %s" % (
        abs(float(loss[0]) - parts[0]) / abs(parts[0]), bar_loss,
        ", ".join("%s %.1e/%.1e" % (n, e, bar_grad[n]) for n, e in errs.items())))
    assert bool(torch.isfinite(loss).all())
    assert abs(float(loss[0]) - parts[0]) <= bar_loss * abs(parts[0]), (float(loss[0]), parts[0], bar_loss)
    assert len(errs) >= len(grads) - 2 * KW["n_layers"]
    for name, err in errs.items():
        assert err <= bar_grad[name], (name, err, bar_grad[name])


def _call_names(dev, monkeypatch, batch, **kw):
    import vlg.engine as E
    eng = engine(dev, **kw)
    names = []
    real = E.call
    monkeypatch.setattr(E, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    eng.train_step(batch)
    torch.cuda.synchronize()
    monkeypatch.setattr(E, "call", real)
    return names


@pytest.mark.parametrize("kw", [dict(class_weights=WEIGHTS), dict(label_smoothing=0.1), dict(box_overlap="giou"), ALL],
                         ids=["weights", "eps", "giou", "all"])
def test_the_step_launches_one_loss_kernel_either_way(dev, monkeypatch, spec64, kw):
    """options off: vlg_layout_loss once and never vlg_layout_loss_ext; any option on: the reverse; as many calls"""
    batch = to_dev(spec64[0], dev)
    off = _call_names(dev, monkeypatch, batch)
    assert off.count("vlg_layout_loss") == 1 and "vlg_layout_loss_ext" not in off
    on = _call_names(dev, monkeypatch, batch, **kw)
    assert on.count("vlg_layout_loss_ext") == 1 and "vlg_layout_loss" not in on
    assert len(on) == len(off)
    assert [n for n in on if n != "vlg_layout_loss_ext"] == [n for n in off if n != "vlg_layout_loss"]


def test_neutral_keywords_are_options_off(dev, monkeypatch, spec64):
    batch = to_dev(spec64[0], dev)
    names = _call_names(dev, monkeypatch, batch, class_weights=None, label_smoothing=0.0, box_overlap="iou")
    assert names.count("vlg_layout_loss") == 1 and "vlg_layout_loss_ext" not in names


def test_engine_refusals(dev):
    for kw in (dict(class_weights=[1.0] * 19), dict(class_weights=[0.0] * 20), dict(class_weights=[1.0] * 19 + [-1.0]),
               dict(class_weights=[1.0] * 19 + [float("inf")]), dict(class_weights=[1.0] * 19 + [float("nan")]),
               dict(label_smoothing=1.0), dict(label_smoothing=-0.1), dict(label_smoothing=float("nan")),
               dict(box_overlap="diou")):
        with pytest.raises(ValueError):
            engine(dev, **kw)


def test_captured_step_replays_like_eager_steps(dev, spec64):
    """a captured step replayed 3 times == 3 eager steps, bitwise: parameters, moments and loss"""
    b = to_dev(spec64[0], dev)
    eager = engine(dev, **ALL)
    for _ in range(3):
        eager.train_step(b)
    want_loss = eager.loss_out.clone()
    graph = engine(dev, **ALL)
    run = graph.capture_train_step(b)
    for _ in range(3):
        run(b)
    torch.cuda.synchronize()
    assert torch.equal(graph.params, eager.params) and torch.equal(graph.loss_out, want_loss)
    assert torch.equal(graph.exp_avg, eager.exp_avg)


def test_validate_reports_the_configured_objective(dev, tmp_path, monkeypatch):
    """Trainer.validate() on an options engine: the loss is the configured objective (float64 specification, size-weighted
    over the batches); the metrics' NLL stays the plain, unweighted and unsmoothed one."""
    from trainer import Trainer
    src = tmp_path / "src"
    src.mkdir()
    monkeypatch.chdir(src)
    args = reference_args(tmp_path / "exp", batch_size=2, epochs=1, print_freq=1, n_frames=4, n_slots=8, d_model=64,
                          n_layers=2, train_clips=4, val_clips=6, val_metrics=1,
                          class_weights=",".join("%g" % w for w in WEIGHTS), label_smoothing=0.1, box_overlap="giou")
    tr = Trainer(args)
    assert tr.engine.box_overlap == "giou" and tr.engine.label_smoothing == pytest.approx(0.1)
    assert tr.engine.class_weights.cpu().tolist() == pytest.approx(WEIGHTS)
    got = tr.validate()
    p = {k: v.cpu().double() for k, v in tr.engine.named_params().items()}
    w = torch.tensor(WEIGHTS, dtype=torch.float64)
    total = clips = nll = scored = 0.0
    for batch in tr.val_loader:
        batch = {k: v.cpu() for k, v in batch.items()}
        logits, raw = O.forward(p, batch["slot_class"], batch["slot_box"].double(), tr.cfg.n_layers)
        va = batch["valid"].double()
        parts = R.losses(logits, raw, batch["tgt_class"], batch["tgt_box"].double(), va, w, 0.1, "giou")
        n = batch["slot_class"].shape[0]
        total += float(parts[0]) * n
        clips += n
        nll += float(R.cross_entropy(logits, batch["tgt_class"], va)) * float(va.sum())
        scored += float(va.sum())
    print("\nvalidate loss %.8g fp64 %.8g; nll %.8g plain fp64 %.8g" % (got["loss"], total / clips, got["nll"], nll / scored))
    check_close(torch.tensor([got["loss"]]), torch.tensor([total / clips]), rtol=1e-4, atol=1e-6, what="validation loss")
    assert got["scored"] == scored
    check_close(torch.tensor([got["nll"]]), torch.tensor([nll / scored]), rtol=1e-4, atol=1e-6, what="plain NLL of the metrics")
