"""GPU: the layout step with the per-clip attention option in the bf16 mode (precision = "bf16", attention = "clip"), through
the engine and the Trainer.  Bars: the rule of test_hip_step.py::test_bf16_projection_mode - 4 x the CPU-measured distance
between the fp32 specification and the float64 emulation of the mode (step_stages.mode_distance; DESIGN.md, "Layout
step: storage contract of the reduced-precision modes"), per quantity, never above the 2e-2 (loss) / 5e-2 (gradient tensor, relative L2) it replaces -
plus the exact properties (reproducible, masked, equivariant)."""
import random

import pytest
import torch

import step_stages as SS
from helpers import check_close, reference_args
from oracle import layout_spec as O

pytestmark = pytest.mark.gpu


def to_dev(batch, dev):
    return {k: v.to(dev) for k, v in batch.items()}


SMALL = dict(B=2, T=16, N=16, d=256, n_layers=2)


def check_grads(got, want, bars):
    """bars: {tensor name or, for a deeper model, its base name: relative-L2 bar}"""
    gmax = max(float(v.norm()) for v in want.values())
    errs = {}
    for name, g in got.items():
        w = want[name].to(g.device)
        if float(w.norm()) < 1e-6 * gmax:
            continue                                     # analytically zero gradients (key bias)
        errs[name] = float((g - w).norm() / w.norm())
    bar = lambda n: bars[n] if n in bars else bars[n.split(".")[-1]]
    print("\ngradients (rel L2 / bar): %s" % ", ".join("%s %.1e/%.1e" % (n, e, bar(n)) for n, e in errs.items()))
    for name, err in errs.items():
        assert err <= bar(name) <= 5e-2, (name, err, bar(name))
    assert max(errs.values()) > 1e-5, "bf16 + clip produced fp32-exact gradients: the mode is not reaching the kernels"


@pytest.mark.parametrize("variable_n", [False, True])
def test_bf16_clip_step_matches_oracle(dev, variable_n):
    """Measured on the CPU (fp32 specification against the float64 emulation of bf16 + clip at this shape): loss 3.1e-5 (fixed
    N) / 3.9e-5 (variable N) -> bars 1.2e-4 / 1.6e-4 (before: 2e-2); gradient tensors 7.3e-3 (box_w) .. 1.4e-2 (l1.ln2_g) / 9.3e-3
    .. 1.5e-2 (head_w) -> 4 x is 2.9e-2 .. 5.8e-2, capped at the 5e-2 it replaces (box_w 2.9e-2, the qkv and proj weights
    3.4e-2 .. 4.2e-2; the tensors above 1.25e-2 keep 5e-2)."""
    from vlg.engine import LayoutEngine
    from vlg.spec import LayoutConfig, param_shapes
    cfg = LayoutConfig(B=2, T=16, N=16, d=256, n_layers=2, attention="clip")
    eng = LayoutEngine(cfg, dev, precision="bf16", padded_slots=variable_n)
    p = O.init_params(param_shapes(cfg), seed=1024)
    batch = O.synthetic_batch(cfg.B, cfg.T, cfg.N, seed=11, variable_n=variable_n, min_valid=3)
    parts, grads = O.loss_and_grads(p, batch, cfg.n_layers, attention="clip")
    loss = eng.forward_backward(to_dev(batch, dev)).cpu()
    bar_loss, bar_grad, _ = SS.end_to_end_bars(SMALL, "bf16", "clip", variable_n, seed=11)
    print("\nbf16 + clip: loss off by %.2e (bar %.2e)" % (abs(float(loss[0]) - parts[0]) / abs(parts[0]), bar_loss))
    assert bar_loss < 2e-2 and abs(float(loss[0]) - parts[0]) <= bar_loss * abs(parts[0]), (float(loss[0]), parts[0], bar_loss)
    check_grads(eng.named_grads(), grads, bar_grad)
    first = float(loss[0])
    b = to_dev(batch, dev)
    for _ in range(20):
        eng.train_step(b)
    assert float(eng.forward(b)[0]) < first


def test_bf16_clip_step_at_metric_shape(dev):
    """(32,16,64), d = 256, 4 layers against the native fp32 per-clip HIP step on the same batch, at the bars of the small
    shape of test_bf16_clip_step_matches_oracle (fixed N): loss 1.2e-4 (before: 2e-2), gradient tensors per kind the largest
    bar over that shape's layers, 2.9e-2 (box_w) .. 5e-2."""
    from vlg.data import synthetic_clips, to_device
    from vlg.engine import LayoutEngine
    from vlg.spec import LayoutConfig
    cfg = LayoutConfig(B=32, T=16, N=64, d=256, n_layers=4, attention="clip")
    batch = to_device(synthetic_clips(cfg.B, cfg.T, cfg.N, seed=3), dev)
    ref = LayoutEngine(cfg, dev)
    l_ref = ref.forward_backward(batch).clone()
    g_ref = {k: v.clone() for k, v in ref.named_grads().items()}
    del ref
    eng = LayoutEngine(cfg, dev, precision="bf16")
    l0 = eng.forward_backward(batch).clone()
    g0 = eng.grads.clone()
    out0 = eng.out.clone()
    bar_loss, _, bar_base = SS.end_to_end_bars(SMALL, "bf16", "clip", False, seed=11)
    print("\nbf16 + clip at the metric shape: loss off by %.2e (bar %.2e)" % (abs(float(l0[0]) - float(l_ref[0])) / abs(float(l_ref[0])), bar_loss))
    assert abs(float(l0[0]) - float(l_ref[0])) <= bar_loss * abs(float(l_ref[0])), (float(l0[0]), float(l_ref[0]), bar_loss)
    check_grads(eng.named_grads(), g_ref, bar_base)
    l1 = eng.forward_backward(batch).clone()
    assert torch.equal(l0, l1) and torch.equal(g0, eng.grads), "bf16 + clip step is not bitwise reproducible"
    perm = torch.randperm(cfg.B)
    pb = {k: v[perm.to(dev)].contiguous() for k, v in batch.items()}
    eng.forward_backward(pb)
    o2 = eng.out.view(cfg.B, -1)[torch.argsort(perm).to(dev)]
    check_close(o2, out0.view(cfg.B, -1), rtol=0, atol=0, what="per-clip outputs under permutation (bf16 + clip)")
    first = float(l0[0])
    for _ in range(10):
        eng.train_step(batch)
        assert torch.equal(eng.params_bf16, eng.params.to(torch.bfloat16))
    assert float(eng.forward(batch)[0]) < first


def test_bf16_clip_captured_step_replays_bitwise(dev):
    from vlg.engine import LayoutEngine
    from vlg.spec import LayoutConfig
    cfg = LayoutConfig(B=2, T=16, N=12, d=256, n_layers=2, attention="clip")
    batches = [to_dev(O.synthetic_batch(cfg.B, cfg.T, cfg.N, seed=90 + i), dev) for i in range(4)]
    eager = LayoutEngine(cfg, dev, precision="bf16")
    eager.use_device_step_counter()
    graphed = LayoutEngine(cfg, dev, precision="bf16")
    run = graphed.capture_train_step(batches[0])
    assert torch.equal(graphed.params, eager.params) and graphed.step_count == 0, "capturing must not take a step"
    for b in batches:
        le = eager.train_step(b).clone()
        lg = run(b).clone()
        assert torch.equal(le, lg), (le, lg)
    assert torch.equal(graphed.params, eager.params) and torch.equal(graphed.exp_avg_sq, eager.exp_avg_sq)
    assert torch.equal(graphed.params_bf16, graphed.params.to(torch.bfloat16))


def test_trainer_bf16_clip_trains_and_rolls_out(tmp_path, monkeypatch, dev):
    """VLG_PRECISION=bf16 with VLG_ATTENTION=clip: one small epoch, validation, then a rollout over a window that holds the
    reserved (padding) class id - checked against the CPU specification at the bf16 bars, and a padded slot's box must not
    reach any other slot's prediction."""
    (tmp_path / "src").mkdir()
    monkeypatch.chdir(tmp_path / "src")
    monkeypatch.delenv("VLG_MODEL", raising=False)
    monkeypatch.setenv("VLG_ATTENTION", "clip")
    monkeypatch.setenv("VLG_PRECISION", "bf16")
    from trainer import Trainer
    random.seed(1024)
    cfgk = dict(batch_size=4, epochs=1, print_freq=1, n_frames=8, n_slots=16, d_model=64, n_layers=2, train_clips=16,
                val_clips=4, variable_n=1)          # variable N: the engine masks padded slots (padded_slots)
    tr = Trainer(reference_args(tmp_path / "exp", **cfgk))
    assert tr.cfg.attention == "clip" and tr.engine.precision == "bf16" and tr.engine.padded_slots
    tr.set_epoch(0)
    tr.train()
    m = tr.validate()
    assert m["loss"] > 0 and m["loss"] == m["loss"]
    batch = next(iter(tr.val_loader))
    cls, box = batch["slot_class"].cpu().clone(), batch["slot_box"].cpu().clone()
    nc = tr.cfg.n_classes
    cls[:, 2, 3] = nc                                     # padded slots (reserved id) inside the window
    cls[:, 5, 7] = nc
    out_c, out_b = tr.generate_sequence(cls, box, steps=1)
    params = {k: v.cpu() for k, v in tr.engine.named_params().items()}
    with torch.no_grad():
        logits, raw = O.forward(params, cls, box, tr.cfg.n_layers, attention="clip", valid=(cls < nc).float())
    want_b = torch.sigmoid(raw[:, -1])
    e = float((out_b[:, 0] - want_b).norm() / want_b.norm())
    assert e <= 5e-2, e
    last = logits[:, -1]
    top2 = last.topk(2, dim=-1).values
    clear = (top2[..., 0] - top2[..., 1]) > 5e-2 * float(last.abs().max())
    assert bool((out_c[:, 0][clear] == last.argmax(-1)[clear]).all())
    # a padded slot's box changes: every other slot's prediction is bitwise unchanged
    box2 = box.clone()
    box2[:, 5, 7] = torch.rand(box.shape[0], 4)
    c2, b2 = tr.generate_sequence(cls, box2, steps=1)
    others = torch.ones(cls.shape[2], dtype=torch.bool)
    others[7] = False
    assert torch.equal(b2[:, 0, others], out_b[:, 0, others])
    assert torch.equal(c2[:, 0, others], out_c[:, 0, others])
