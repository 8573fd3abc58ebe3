"""GPU: the reference's pixel step (CoordGridNet + frozen HED + VGG19 term + Adam) with precision="bf16" - every 3x3
convolution on the bf16-MFMA kernels (csrc/conv_bf16.hip) - against the same step in fp32 from the same parameters and
batch, and the VLG_PRECISION=bf16 knob behind the Trainer surface (VLG_MODEL=gridnet).

bf16 mode is not reference parity: the bars below are set at a few times the differences measured on an MI355X
("bf16-MFMA convolutions")."""
import random

import pytest
import torch

from helpers import reference_args
from oracle import gridnet_spec as G, hned_spec as HS, vgg_spec as V

pytestmark = pytest.mark.gpu

LOSS_REL = 3e-3          # per loss part, relative; measured worst 2.6e-4 (64x64) and 5.9e-4 (256x256), both the VGG term
# Gradients, per parameter tensor r_k = ||g_bf16 - g_fp32|| / ||g_fp32||, and over the whole gradient vector.  The median
# and the whole-vector error are bounded; single tensors with a small, cancelling gradient (sums of many terms of both
# signs, each carrying ~2^-9 of bf16 rounding) reach r_k ~ 2-7 and are only reported.  Bars ~3x the measured:
# b=2 64x64: whole 8.1e-3, median 2.9e-2;  b=4 256x256: whole 2.0e-2, median 0.15.


def _engines(dev, b, H, W, filt=(32, 64, 96)):
    from vlg.image_engine import ImageEngine, synthetic_frames
    p = G.test_params(G.param_shapes(10, filt, coord=True), seed=4)
    hp, vp = HS.test_params(3), V.test_params(3)
    engs = {}
    for prec in ("fp32", "bf16"):
        e = ImageEngine(b, H, W, dev, arch="CoordGridNet", filters=filt, with_hed=True, with_vgg=True, precision=prec)
        e.load_state_dict(p)
        e.hed.load_state_dict(hp)
        e.vgg.load_state_dict(vp)
        engs[prec] = e
    batch = {k: v.to(dev) for k, v in synthetic_frames(b, H, W, seed=9).items() if k not in ("e1", "e2")}
    return engs, batch


def _compare(engs, batch, what, grad_global, grad_median):
    out = {}
    for prec, e in engs.items():
        losses = e.forward(batch).clone()
        e.backward()
        torch.cuda.synchronize()
        out[prec] = (losses.cpu()[:5].double(), e.net.unpack(e.net.grads), float(e.total()))
    (l32, g32, t32), (l16, g16, t16) = out["fp32"], out["bf16"]
    assert all(bool(torch.isfinite(g).all()) for g in g16.values()) and bool(torch.isfinite(l16).all()), what
    rel_l = [abs(float(a - b)) / max(abs(float(b)), 1e-12) for a, b in zip(l16, l32)]
    errs = []
    for k, g in g32.items():
        n = float(g.double().norm())
        if n == 0.0:
            assert float(g16[k].abs().max()) == 0.0, k
            continue
        errs.append((float((g16[k].double() - g.double()).norm()) / n, k))
    errs.sort()
    median, (worst, worst_k) = errs[len(errs) // 2][0], errs[-1]
    flat32 = torch.cat([g.double().flatten() for g in g32.values()])
    flat16 = torch.cat([g16[k].double().flatten() for k in g32])
    glob = float((flat16 - flat32).norm()) / float(flat32.norm())
    print("BF16STEP %s loss parts rel %s  total %.6g vs %.6g  grad rel L2: whole %.3e  median %.3e  worst %.3e (%s)" % (
        what, ["%.2e" % v for v in rel_l], t16, t32, glob, median, worst, worst_k))
    for name, v in zip(("l1", "gradient", "ssim", "ce", "vgg"), rel_l):
        assert v <= LOSS_REL, (what, name, v)
    assert median <= grad_median and glob <= grad_global, (what, median, glob)


def test_bf16_step_tracks_fp32(dev):
    engs, batch = _engines(dev, 2, 64, 64)
    assert engs["bf16"].net.precision == "bf16" and engs["bf16"].hed.precision == "bf16" and engs["bf16"].vgg.precision == "bf16"
    _compare(engs, batch, "b=2 64x64", grad_global=0.03, grad_median=0.1)


def test_bf16_full_size_step_tracks_fp32(dev):
    engs, batch = _engines(dev, 4, 256, 256)
    _compare(engs, batch, "b=4 256x256", grad_global=0.06, grad_median=0.5)


def test_bf16_adam_steps_reduce_the_loss(dev):
    from vlg.image_engine import ImageEngine, synthetic_frames
    eng = ImageEngine(2, 32, 32, dev, arch="CoordGridNet", filters=(8, 16, 24), lr=2e-3, precision="bf16")
    eng.load_state_dict(G.test_params(G.param_shapes(10, (8, 16, 24), coord=True), seed=1))
    batch = {k: v.to(dev) for k, v in synthetic_frames(2, 32, 32, seed=3).items()}
    first = float(eng.train_step(batch))
    for _ in range(20):
        last = float(eng.train_step(batch))
    assert last < 0.95 * first, (first, last)


def test_trainer_bf16_reference_model_and_checkpoints(tmp_path, monkeypatch):
    """VLG_MODEL=gridnet VLG_PRECISION=bf16: the Trainer trains and validates on the bf16 convolutions, its checkpoints
    resume in an fp32 Trainer and the other way round (one schema: every tensor is fp32), and the pixel rollout runs."""
    (tmp_path / "src").mkdir()
    monkeypatch.chdir(tmp_path / "src")
    monkeypatch.setenv("VLG_MODEL", "gridnet")
    monkeypatch.setenv("VLG_IMG_SIZE", "32")
    monkeypatch.setenv("VLG_PRECISION", "bf16")
    from trainer import Trainer
    random.seed(1024)
    small = dict(batch_size=2, epochs=2, print_freq=1, train_clips=8, val_clips=4)
    tr = Trainer(reference_args(tmp_path / "exp", lr=2e-3, **small))
    assert tr.image_mode and tr.engine.engine.precision == "bf16" and tr.engine.engine.net.precision == "bf16"
    vals = []
    for epoch in range(2):
        tr.set_epoch(epoch)
        tr.train()
        vals.append(tr.validate()["loss"])
    assert vals[1] < vals[0] and all(v == v for v in vals)
    tr.save_checkpoint({"loss": vals[-1]})
    monkeypatch.setenv("VLG_PRECISION", "fp32")
    again = Trainer(reference_args(tmp_path / "again", resume="../checkpoint/latest.pth", **small))
    assert again.engine.engine.precision == "fp32"
    assert torch.equal(again.engine.engine.net.params, tr.engine.engine.net.params)
    assert torch.equal(again.engine.engine.exp_avg, tr.engine.engine.exp_avg)
    again.set_epoch(0)
    again.train()
    again.save_checkpoint({"loss": 0.0})
    monkeypatch.setenv("VLG_PRECISION", "bf16")
    back = Trainer(reference_args(tmp_path / "back", resume="../checkpoint/latest.pth", **small))
    assert back.engine.engine.precision == "bf16"
    assert torch.equal(back.engine.engine.net.params, again.engine.engine.net.params)
    g = torch.Generator().manual_seed(2)
    img1, img2 = torch.randn(2, 3, 32, 32, generator=g), torch.randn(2, 3, 32, 32, generator=g)
    seg1 = torch.randint(0, 20, (2, 1, 32, 32), generator=g).float()
    seg2 = torch.randint(0, 20, (2, 1, 32, 32), generator=g).float()
    p, q = back.generate_sequence(img1.to(tr.device), img2.to(tr.device), seg1.to(tr.device), seg2.to(tr.device), steps=2)
    assert p.shape == (2, 12, 32, 32) and q.shape == (2, 4, 32, 32)
    import numpy as np
    assert bool(np.isfinite(p).all()) and bool(np.isfinite(q).all())
    ro = next(iter(back.engine._rollouts.values()))
    assert ro.net.precision == "bf16" and ro.hed.precision == "bf16"


def test_trainer_fp32x3_runs_fp32_convs_and_warns(tmp_path, monkeypatch, caplog):
    (tmp_path / "src").mkdir()
    monkeypatch.chdir(tmp_path / "src")
    monkeypatch.setenv("VLG_MODEL", "gridnet")
    monkeypatch.setenv("VLG_IMG_SIZE", "32")
    monkeypatch.setenv("VLG_PRECISION", "fp32x3")
    from trainer import Trainer
    with caplog.at_level("WARNING"):
        tr = Trainer(reference_args(tmp_path / "exp", batch_size=2, epochs=1, print_freq=1, train_clips=4, val_clips=4))
    assert tr.engine.engine.precision == "fp32"
    assert any("fp32x3" in r.getMessage() for r in caplog.records)
