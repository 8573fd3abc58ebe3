"""CPU: the definition of the loss options (tests/loss_ext_ref.py) against torch and against the specification it extends,
the balanced-weights helper of vlg.metrics, and the trainer's loss_knobs."""
import argparse
import math

import pytest
import torch
import torch.nn.functional as F

import loss_ext_ref as R
from oracle import layout_spec as O

F64 = torch.float64
KNOB_ENV = ("VLG_CLASS_WEIGHTS", "VLG_LABEL_SMOOTHING", "VLG_BOX_OVERLAP")


def _inputs(seed=3, B=2, T=4, N=5):
    batch = O.synthetic_batch(B, T, N, seed=seed, variable_n=True, min_valid=2)
    g = torch.Generator().manual_seed(seed + 100)
    logits = torch.randn(B, T, N, 20, generator=g, dtype=F64) * 3
    raw = torch.randn(B, T, N, 4, generator=g, dtype=F64)
    w = torch.rand(20, generator=g, dtype=F64) * 3
    w[int(batch["tgt_class"][0, 0, 0])] = 0.0              # a zero weight on a class that occurs among the valid targets
    return batch, logits, raw, w


@pytest.mark.parametrize("weighted,eps", [(True, 0.0), (False, 0.1), (True, 0.1), (True, 0.9)])
def test_cross_entropy_is_torchs(weighted, eps):
    batch, logits, _, w = _inputs()
    w = w if weighted else None
    valid = batch["valid"].double()
    z = logits.clone().requires_grad_(True)
    ce = R.cross_entropy(z, batch["tgt_class"], valid, w, eps)
    ce.backward()
    m = batch["valid"] > 0
    z2 = logits.clone().requires_grad_(True)
    want = F.cross_entropy(z2[m], batch["tgt_class"][m], weight=w, label_smoothing=eps, reduction="mean")
    want.backward()
    assert abs(float(ce.detach() - want.detach())) <= 1e-12
    assert float((z.grad - z2.grad).abs().max()) <= 1e-12
    assert bool((z.grad[~m] == 0).all())
    # the closed form of the gradient that the kernel implements: v/W (Q p - q)
    ww = torch.ones(20, dtype=F64) if w is None else w
    y = batch["tgt_class"]
    q = (eps / 20) * ww.expand(logits.shape).clone()
    q.scatter_add_(-1, y.unsqueeze(-1), ((1 - eps) * ww[y]).unsqueeze(-1))
    W = (valid * ww[y]).sum()
    closed = valid.unsqueeze(-1) / W * (q.sum(-1, keepdim=True) * torch.softmax(logits, -1) - q)
    assert float((closed - z.grad).abs().max()) <= 1e-12


def test_zero_total_weight_gives_zero_not_nan():
    batch, logits, _, _ = _inputs()
    w = torch.ones(20, dtype=F64)
    w[batch["tgt_class"][batch["valid"] > 0].unique()] = 0.0
    z = logits.clone().requires_grad_(True)
    ce = R.cross_entropy(z, batch["tgt_class"], batch["valid"].double(), w, 0.1)
    ce.backward()
    assert float(ce.detach()) == 0.0 and bool((z.grad == 0).all())


def test_neutral_options_are_the_specification():
    batch, logits, raw, _ = _inputs()
    a = R.losses(logits, raw, batch["tgt_class"], batch["tgt_box"].double(), batch["valid"].double())
    b = O.losses(logits, raw, batch["tgt_class"], batch["tgt_box"].double(), batch["valid"].double())
    for x, y in zip(a, b):
        assert float(x) == float(y)
    with pytest.raises(ValueError):
        R.losses(logits, raw, batch["tgt_class"], batch["tgt_box"].double(), batch["valid"].double(), box_overlap="diou")


def test_giou_properties():
    g = torch.Generator().manual_seed(5)
    a = torch.rand(256, 4, generator=g, dtype=F64) * 0.9 + 0.05
    b = torch.rand(256, 4, generator=g, dtype=F64) * 0.9 + 0.05
    same = 1 - R.box_giou_cxcywh(a, a)                                        # identical boxes: 0, up to iou_eps / area
    assert bool((same >= 0).all()) and bool((same <= O.IOU_EPS / (a[:, 2] * a[:, 3])).all())
    t = 1 - R.box_giou_cxcywh(a, b)
    assert float(t.min()) >= 0.0 and float(t.max()) <= 2.0
    assert float((R.box_giou_cxcywh(a, b) - O.box_iou_cxcywh(a, b)).max()) <= 1e-12    # giou <= iou (float64 rounding of the areas)
    # the enclosing box IS the union: same y extent, x extents that overlap or touch
    c = torch.tensor([[0.3, 0.5, 0.4, 0.2], [0.25, 0.5, 0.5, 0.5]], dtype=F64)
    d = torch.tensor([[0.6, 0.5, 0.4, 0.2], [0.75, 0.5, 0.5, 0.5]], dtype=F64)
    assert float((R.box_giou_cxcywh(c, d) - O.box_iou_cxcywh(c, d)).abs().max()) <= 1e-12
    # disjoint boxes: IoU has no gradient, GIoU has one
    p = torch.tensor([[0.5, 0.5, 0.5, 0.5]], dtype=F64, requires_grad=True)
    far = torch.tensor([[0.875, 0.875, 0.125, 0.125]], dtype=F64)
    O.box_iou_cxcywh(p, far).sum().backward()
    assert bool((p.grad == 0).all())
    p.grad = None
    R.box_giou_cxcywh(p, far).sum().backward()
    assert bool((p.grad != 0).all()) and float(p.grad[0, 0]) > 0            # moving right closes the gap


def test_balanced_class_weights():
    from vlg.metrics import MetricsRecord, CONF, balanced_class_weights
    n = [400.0, 0.0, 25.0, 100.0, 1.0, 0.0, 25.0]
    for power in (0.0, 0.5, 1.0):
        w = balanced_class_weights(n, power)
        assert math.isclose(sum(c * x for c, x in zip(n, w)), sum(n), rel_tol=1e-12)
        present = sorted((c, x) for c, x in zip(n, w) if c > 0)
        assert all(a[1] >= b[1] for a, b in zip(present, present[1:])), "not monotone in the count"
        assert w[1] == w[5] == max(x for c, x in zip(n, w) if c > 0)          # absent classes: the largest present weight
        assert w[2] == w[6]
    assert balanced_class_weights(n, 0.0) == pytest.approx([1.0] * 7)
    w = balanced_class_weights(n)                                              # power 0.5: w ~ 1 / sqrt(n)
    assert w[3] / w[0] == pytest.approx(2.0) and w[4] / w[3] == pytest.approx(10.0)
    # a record, and a row of its summary
    rec = MetricsRecord(3, rows=2)
    conf = torch.tensor([[5, 1, 0], [0, 0, 0], [2, 2, 20]])
    rec.counts[1, CONF:CONF + 9] = conf.flatten()
    want = balanced_class_weights([6, 0, 24])
    assert balanced_class_weights(rec.summary()[1]) == want and balanced_class_weights(rec, row=1) == want
    for bad in ([], [0, 0], [1, -1], [1, float("nan")]):
        with pytest.raises(ValueError):
            balanced_class_weights(bad)
    with pytest.raises(ValueError):
        balanced_class_weights([1, 2], power=-1.0)
    with pytest.raises(ValueError):
        balanced_class_weights(rec)                                            # row 0 scored nothing


def _args(**kw):
    return argparse.Namespace(**kw)


def test_loss_knobs(monkeypatch):
    from trainer import loss_knobs
    for name in KNOB_ENV:
        monkeypatch.delenv(name, raising=False)
    assert loss_knobs(_args()) == {}
    assert loss_knobs(_args(class_weights=None, label_smoothing=0.0, box_overlap="iou")) == {}
    ws = [0.5 * c for c in range(20)]
    text = ",".join("%g" % w for w in ws)
    assert loss_knobs(_args(class_weights=text)) == {"class_weights": ws}
    assert loss_knobs(_args(class_weights=ws, label_smoothing=0.1, box_overlap="giou")) == {
        "class_weights": ws, "label_smoothing": 0.1, "box_overlap": "giou"}
    assert loss_knobs(_args(label_smoothing="0.25")) == {"label_smoothing": 0.25}
    monkeypatch.setenv("VLG_CLASS_WEIGHTS", text)
    monkeypatch.setenv("VLG_LABEL_SMOOTHING", "0.05")
    monkeypatch.setenv("VLG_BOX_OVERLAP", "GIoU")
    assert loss_knobs(_args()) == {"class_weights": ws, "label_smoothing": 0.05, "box_overlap": "giou"}
    assert loss_knobs(_args(label_smoothing=0.2, box_overlap="iou")) == {"class_weights": ws, "label_smoothing": 0.2}   # args win


@pytest.mark.parametrize("kw", [
    dict(class_weights="1,2,3"), dict(class_weights=",".join(["1"] * 21)), dict(class_weights=",".join(["0"] * 20)),
    dict(class_weights=",".join(["1"] * 19 + ["-1"])), dict(class_weights=",".join(["1"] * 19 + ["inf"])),
    dict(class_weights=",".join(["1"] * 19 + ["nan"])), dict(class_weights=",".join(["1"] * 19 + ["x"])),
    dict(class_weights=[1.0] * 19), dict(label_smoothing=1.0), dict(label_smoothing=-0.1),
    dict(label_smoothing=float("nan")), dict(label_smoothing="much"), dict(box_overlap="diou")])
def test_loss_knobs_refusals(monkeypatch, kw):
    """the engine's refusals (vlg.spec.loss_options), from args and from the environment"""
    from trainer import loss_knobs
    from vlg.spec import loss_options
    for name in KNOB_ENV:
        monkeypatch.delenv(name, raising=False)
    with pytest.raises(ValueError):
        loss_knobs(_args(**kw))
    (key, value), = kw.items()
    if isinstance(value, str):
        monkeypatch.setenv("VLG_" + key.upper(), value)
        with pytest.raises(ValueError):
            loss_knobs(_args())
        value = value.split(",") if key == "class_weights" else value
    with pytest.raises(ValueError):
        loss_options(**{key: value})


def test_engine_factories_without_the_keywords_are_never_handed_one(monkeypatch, tmp_path):
    """get_layout_engine passes loss_knobs(args) to LayoutEngine only: an engine factory keeps its (cfg, args) call"""
    from helpers import oracle_factory, reference_args
    from trainer import get_layout_engine
    for name in KNOB_ENV:
        monkeypatch.delenv(name, raising=False)
    eng = get_layout_engine(reference_args(tmp_path, batch_size=2, n_frames=4, n_slots=4, d_model=64, n_layers=1),
                            engine_factory=oracle_factory)
    assert type(eng).__name__ == "OracleEngine"
