"""CPU: the dropout definition (tests/dropout_ref.py) - threshold rule, drop rate, independence of sites and steps, the
fp64 reference model and its gradient - and the trainer's dropout knobs."""
import ctypes
import math

import numpy as np
import pytest
import torch

import dropout_ref as R
from helpers import oracle_factory, reference_args
from oracle import layout_spec as O

TWO32 = 2 ** 32


def test_threshold_rule():
    assert R.plan(0.0) == (0, 1.0)
    assert R.keep_mask(7, 64, 3, 5, 1024, 0).all()                       # thr = 0 keeps everything
    for p, thr in ((0.1, 429496730), (0.25, 1 << 30), (0.5, 1 << 31)):   # floor(p * 2^32 + 0.5)
        t, s = R.plan(p)
        assert t == thr
        assert s == float(np.float32(1.0 / (1.0 - thr / TWO32)))
    assert R.plan(0.25)[1] == float(np.float32(4.0 / 3.0)) and R.plan(0.5)[1] == 2.0
    below_one = math.nextafter(1.0, 0.0)
    t, s = R.plan(below_one)                                             # p * 2^32 + 0.5 rounds to 2^32: the clamp
    assert t == TWO32 - 1 and s == float(np.float32(TWO32))
    assert R.plan(1.0 - 2.0 ** -33)[0] == TWO32 - 1                      # floor(2^32 - 0.5 + 0.5) = 2^32, clamped
    assert R.plan(1.0 - 2.0 ** -31)[0] == TWO32 - 2
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError):
            R.plan(bad)


def test_library_plan_is_the_same_rule():
    """vlg_dropout_plan is host only: the one place the product keeps the threshold rule"""
    from vlg import hip
    lib = hip.load()
    for p in (0.0, 0.1, 0.25, 0.5, 0.9, math.nextafter(1.0, 0.0), 1.0 - 2.0 ** -31, 1e-12):
        thr, scale = ctypes.c_uint32(), ctypes.c_float()
        assert lib.vlg_dropout_plan(p, ctypes.byref(thr), ctypes.byref(scale)) == 0
        assert (thr.value, scale.value) == R.plan(p), p
    for bad in (-1e-9, 1.0, 2.0, float("nan")):
        thr, scale = ctypes.c_uint32(), ctypes.c_float()
        assert lib.vlg_dropout_plan(bad, ctypes.byref(thr), ctypes.byref(scale)) == 1001


@pytest.mark.parametrize("p", [0.1, 0.25, 0.5])
def test_drop_rate(p):
    """259 x 1024 elements: the drop rate lies within 4 standard deviations of thr / 2^32 for every site and step"""
    thr, _ = R.plan(p)
    q = thr / TWO32
    n = 259 * 1024
    sd = math.sqrt(q * (1 - q) / n)
    for site in (0, 1, 2, 8):
        for step in (0, 1, 7):
            rate = 1.0 - R.keep_mask(259, 1024, site, step, 1024, thr).mean()
            assert abs(rate - q) <= 4 * sd, (site, step, (rate - q) / sd)


def test_masks_of_sites_and_steps_are_independent():
    thr, _ = R.plan(0.5)
    base = R.keep_mask(64, 256, 1, 0, 1024, thr)
    for other in (R.keep_mask(64, 256, 2, 0, 1024, thr), R.keep_mask(64, 256, 1, 1, 1024, thr)):
        assert abs((base == other).mean() - 0.5) <= 0.02


def test_mask_bit_depends_on_the_element_alone():
    """rows 3..7 of a long mask = a mask asked for those rows; a narrower d is a prefix of the columns"""
    thr, _ = R.plan(0.25)
    full = R.keep_mask(259, 256, 4, 9, 77, thr)
    assert np.array_equal(full[3:8], R.keep_mask(5, 256, 4, 9, 77, thr, row0=3))
    assert np.array_equal(full[:, :64], R.keep_mask(259, 64, 4, 9, 77, thr))


SHAPE = dict(B=2, T=4, N=3, d=64, n_layers=2)


def _setup(seed=3):
    from vlg.spec import LayoutConfig, param_shapes
    cfg = LayoutConfig(**SHAPE)
    p = O.init_params(param_shapes(cfg), seed=seed)
    batch = O.synthetic_batch(cfg.B, cfg.T, cfg.N, seed=seed)
    return cfg, p, batch


@pytest.mark.parametrize("attention", ["slot", "clip"])
def test_reference_model_without_dropout_is_the_oracle(attention):
    cfg, p, batch = _setup()
    want_parts, want_grads = O.loss_and_grads(p, batch, cfg.n_layers, attention=attention)
    parts, grads, _, _ = R.loss_and_grads(p, batch, cfg.n_layers, 0.0, 5, 1024, attention=attention)
    assert parts == want_parts
    for k in want_grads:
        assert torch.equal(grads[k], want_grads[k]), k


def test_reference_model_gradient_by_finite_differences():
    """fp64, p = 0.25: autograd against central differences on three parameters (one before every site, one between
    the sites of a layer, one after the last).  With h = 1e-6 the truncation error is O(h^2) and the rounding error
    ~ 1e-16 * |loss| / h ~ 1e-8, so 1e-6 absolute + 1e-5 relative is met with margin."""
    cfg, p, batch = _setup()
    p64, b64 = R.to64(p), R.to64(batch)
    parts, grads, _, _ = R.loss_and_grads(p64, b64, cfg.n_layers, 0.25, 2, 1024)
    assert parts != O.loss_and_grads(p64, b64, cfg.n_layers)[0]          # the masks do something

    def total(q):
        lg, bx = R.forward(q, b64["slot_class"], b64["slot_box"], cfg.n_layers, 0.25, 2, 1024)
        return float(O.losses(lg, bx, b64["tgt_class"], b64["tgt_box"], b64["valid"])[0])

    h = 1e-6
    for name, idx in (("box_w", (5, 2)), ("l0.ff1_w", (7, 11)), ("l1.ff2_b", (9,))):
        q = {k: v.clone() for k, v in p64.items()}
        q[name][idx] += h
        up = total(q)
        q[name][idx] -= 2 * h
        fd = (up - total(q)) / (2 * h)
        g = float(grads[name][idx])
        assert abs(fd - g) <= 1e-6 + 1e-5 * abs(g), (name, fd, g)


@pytest.mark.parametrize("mode", ["bf16", "bf16_mfma"])
def test_mode_emulation_without_dropout_is_step_stages_emulation(mode):
    """dropout_ref's restatement of a reduced-precision mode (autograd with the mode's roundings) against the project's
    own, step_stages.emulate (one stage function per launch): the same roundings at the same places, so with p = 0 the
    gradients agree to fp64 reassociation - 1e-12 relative L2 is four orders above that and nine below a bf16 rounding."""
    import step_stages as SS
    cfg, p, batch = _setup()
    _, want = SS.emulated_oracle(cfg, mode, p, batch, "slot", masked=False)
    _, got, _, _ = R.loss_and_grads(R.to64(p), R.to64(batch), cfg.n_layers, 0.0, 0, 0, mode=mode)
    for n, w in want.items():
        if float(w.norm()) > 0:
            assert float((got[n] - w.double()).norm() / w.double().norm()) <= 1e-12, n


def test_mode_emulation_is_off_the_exact_model_by_a_bf16_rounding():
    cfg, p, batch = _setup()
    dist = R.mode_distance(R.to64(p), R.to64(batch), cfg.n_layers, 0.25, 1, 1024, "bf16")
    assert 1e-5 < max(dist.values()) < 5e-2


# ------------------------------------------------------------------------------------------------------ trainer knobs
SMALL = dict(batch_size=4, epochs=1, print_freq=1, n_frames=4, n_slots=8, d_model=64, n_layers=1, train_clips=8, val_clips=4)


@pytest.fixture
def workdir(tmp_path, monkeypatch):
    src = tmp_path / "src"
    src.mkdir()
    monkeypatch.chdir(src)
    for k in ("VLG_DROPOUT", "VLG_DROPOUT_SEED", "VLG_MODEL"):
        monkeypatch.delenv(k, raising=False)
    return tmp_path


def test_knobs_parse_and_offset_the_seed_by_rank(workdir, monkeypatch):
    import trainer
    assert trainer.dropout_knobs(reference_args(workdir / "e")) == {}                       # off: nothing to hand over
    assert trainer.dropout_knobs(reference_args(workdir / "e", dropout=0.1)) == {"dropout": 0.1, "dropout_seed": 1024}
    assert trainer.dropout_knobs(reference_args(workdir / "e", rank=3, gpus=4, dropout=0.1, seed=7)) == {"dropout": 0.1, "dropout_seed": 10}
    monkeypatch.setenv("VLG_DROPOUT", "0.25")
    monkeypatch.setenv("VLG_DROPOUT_SEED", "99")
    assert trainer.dropout_knobs(reference_args(workdir / "e", rank=1, gpus=2)) == {"dropout": 0.25, "dropout_seed": 100}
    assert trainer.dropout_knobs(reference_args(workdir / "e", dropout=0.0)) == {}          # args win over the environment
    for bad in ("1.0", "-0.1", "nan"):
        monkeypatch.setenv("VLG_DROPOUT", bad)
        with pytest.raises(ValueError, match="VLG_DROPOUT"):
            trainer.dropout_knobs(reference_args(workdir / "e"))
    monkeypatch.setenv("VLG_DROPOUT", "0.1")
    monkeypatch.setenv("VLG_DROPOUT_SEED", "-1")
    with pytest.raises(ValueError, match="VLG_DROPOUT_SEED"):
        trainer.dropout_knobs(reference_args(workdir / "e"))


def test_dropout_rule_is_stated_once_and_names_its_caller():
    """vlg.spec.dropout_options: what LayoutEngine (keyword) and trainer.dropout_knobs (environment variable) both call"""
    from vlg.spec import dropout_options
    assert dropout_options(0) == 0.0 and dropout_options(0.1) == 0.1 and dropout_options("0.25", "VLG_DROPOUT") == 0.25
    assert dropout_options(math.nextafter(1.0, 0.0)) < 1.0
    for bad in (-0.1, 1.0, 1.5, float("nan"), -1e-9):
        with pytest.raises(ValueError, match=r"^dropout must be in \[0, 1\)"):
            dropout_options(bad)
        with pytest.raises(ValueError, match=r"^VLG_DROPOUT must be in \[0, 1\)"):
            dropout_options(bad, "VLG_DROPOUT")


def test_trainer_refuses_out_of_range_dropout_at_construction(workdir):
    from trainer import Trainer
    with pytest.raises(ValueError, match="VLG_DROPOUT"):
        Trainer(reference_args(workdir / "exp", dropout=1.0, **SMALL), engine_factory=oracle_factory)
    tr = Trainer(reference_args(workdir / "exp", **SMALL), engine_factory=oracle_factory)
    assert tr.dropout == {}
    tr = Trainer(reference_args(workdir / "exp", dropout=0.2, dropout_seed=5, **SMALL), engine_factory=oracle_factory)
    assert tr.dropout == {"dropout": 0.2, "dropout_seed": 5}


def test_engine_is_handed_the_knobs_only_when_dropout_is_on(workdir, monkeypatch):
    import trainer
    import vlg.engine
    seen = []

    class Recorder:
        def __init__(self, cfg, device, **kw):
            seen.append(kw)

    monkeypatch.setattr(vlg.engine, "LayoutEngine", Recorder)
    trainer.get_layout_engine(reference_args(workdir / "e", **SMALL))
    assert "dropout" not in seen[-1] and "dropout_seed" not in seen[-1]
    trainer.get_layout_engine(reference_args(workdir / "e", rank=1, gpus=2, dropout=0.1, **SMALL))
    assert seen[-1]["dropout"] == 0.1 and seen[-1]["dropout_seed"] == 1025
