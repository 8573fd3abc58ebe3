"""CPU: the restatement of the augmentation rule (tests/augment_ref.py) does what include/vlg_hip.h says, the host-only
planner agrees with its threshold, and the option rules (vlg.spec.augment_options, trainer.augment_knobs) refuse what they
must.  No GPU."""
import argparse
import ctypes

import numpy as np
import pytest
import torch

import augment_ref as A
from helpers import reference_args

NC = A.NC
KEYS = ("slot_class", "slot_box", "tgt_box", "valid")


def _same(a, b):
    return torch.equal(a, b) if a.dtype == torch.int64 else torch.equal(A.bits(a), A.bits(b))


def test_the_generated_batches_hold_what_the_tests_need():
    b = A.kernel_case(3, 4, 5, seed=1)
    box = b["slot_box"]
    assert bool((b["slot_class"] == NC).any()) and bool(((b["valid"] == 0) & (b["slot_class"] < NC)).any())
    assert bool((box[..., 0] - 0.5 * box[..., 2] < 0).any()) and bool((box[..., 0] + 0.5 * box[..., 2] > 1).any())      # sticking out
    small = (box[..., 2] < 0.03) & ((box[..., 0] < 0.03) | (box[..., 0] > 0.97))
    assert bool(small.any())                                            # a shift of 0.5 moves some of these wholly outside
    plain = A.kernel_case(3, 4, 5, seed=1, padded=False)
    assert bool((plain["slot_class"] < NC).all())


@pytest.mark.parametrize("shape", A.SHAPES)
def test_all_knobs_zero_is_the_identity(shape):
    b = A.kernel_case(*shape, seed=2)
    for k in (0, 5):
        got = A.augment(b, k, seed=9)
        for key in KEYS:
            assert _same(got[key], b[key]), key
        assert not bool(got["flip"].any()) and not bool(got["drop"].any())


def test_flip_one_flips_every_clip_and_twice_restores():
    b = A.kernel_case(3, 4, 5, seed=3, padded=False)
    b["valid"] = torch.ones_like(b["valid"])
    once = A.augment(b, 0, seed=1, flip=1.0)
    assert bool(once["flip"].all())
    for key in ("slot_box", "tgt_box"):
        assert torch.equal(once[key][..., 0], 1.0 - b[key][..., 0]) and _same(once[key][..., 1:], b[key][..., 1:])
    twice = A.augment(dict(b, slot_box=once["slot_box"], tgt_box=once["tgt_box"]), 0, seed=1, flip=1.0)
    cx, back = b["slot_box"][..., 0], twice["slot_box"][..., 0]
    inside = (cx >= 0) & (cx <= 1)
    # 1 - cx rounds once, to a number in [0, 1] on a grid no finer than 2^-24 near 1: off by at most 2^-25.  Where that number is
    # in [0.5, 1] the second subtraction is exact (Sterbenz), and where cx itself is there the first one is too
    assert float((back - cx)[inside].abs().max()) <= 2.0 ** -25
    assert torch.equal(back[inside & (cx >= 0.5)], cx[inside & (cx >= 0.5)])
    assert _same(once["valid"], b["valid"]) and torch.equal(once["slot_class"], b["slot_class"])


@pytest.mark.parametrize("knobs", [dict(zoom=0.5), dict(shift=0.5), dict(jitter=0.25), dict(zoom=0.5, shift=0.5, jitter=0.25, flip=0.5)])
def test_geometric_outputs_stay_in_the_image(knobs):
    b = A.kernel_case(2, 16, 64, seed=4)
    for k in (0, 1):
        got = A.augment(b, k, seed=5, **knobs)
        live = b["slot_class"] < NC
        for box, mask in ((got["slot_box"], live), (got["tgt_box"], b["valid"] > 0)):
            m = box[mask]
            assert bool(torch.isfinite(m).all())
            assert float(m[:, :2].min()) >= 0.0 and float(m[:, :2].max()) <= 1.0
            assert float(m[:, 2:].min()) >= 2.0 ** -10 and float(m[:, 2:].max()) <= 1.0
        # what the map does not touch is a bit copy
        assert _same(got["slot_box"][~live], b["slot_box"][~live]) and _same(got["tgt_box"][b["valid"] <= 0], b["tgt_box"][b["valid"] <= 0])
    # a small box near the border, shifted wholly outside, is a sliver on the border
    tiny = A.kernel_case(64, 1, 2, seed=4, padded=False)
    tiny["slot_box"] = torch.tensor([0.01, 0.5, 0.01, 0.01]).repeat(64, 1, 2, 1)
    out = A.augment(tiny, 0, seed=5, shift=0.5)["slot_box"]
    gone = out[..., 2] == 2.0 ** -10
    assert 8 <= int(gone.sum()) <= 2 * 56 and bool((out[..., 0][gone] <= 2.0 ** -10).all()) and bool((out[..., 0][gone] == 0).any())


def test_a_dropped_track_is_padded_in_every_frame_and_nothing_else_moves():
    b = A.kernel_case(3, 4, 5, seed=6)
    got = A.augment(b, 2, seed=7, drop=0.4)
    drop = got["drop"]                                                  # (B, N)
    assert bool(drop.any()) and not bool(drop.all())
    d = drop[:, None, :].expand(3, 4, 5)
    assert bool((got["slot_class"][d] == NC).all()) and bool((got["slot_box"][d] == 0).all()) and bool((got["valid"][d] == 0).all())
    assert _same(got["valid"][~d], b["valid"][~d]) and torch.equal(got["slot_class"][~d], b["slot_class"][~d])
    assert _same(got["slot_box"][~d], b["slot_box"][~d]) and _same(got["tgt_box"], b["tgt_box"])
    # the draw is per track: the same in every frame by construction, and another one at another step
    assert not torch.equal(A.augment(b, 3, seed=7, drop=0.4)["drop"], drop)
    every = A.augment(b, 0, seed=7, thr_drop=A.TWO24)
    assert bool(every["drop"].all()) and bool((every["valid"] == 0).all())


def test_targets_never_see_jitter():
    b = A.kernel_case(2, 16, 64, seed=8, padded=False)
    with_j = A.augment(b, 1, seed=3, flip=0.5, zoom=0.3, shift=0.2, jitter=0.25)
    without = A.augment(b, 1, seed=3, flip=0.5, zoom=0.3, shift=0.2)
    assert _same(with_j["tgt_box"], without["tgt_box"])
    assert not torch.equal(with_j["slot_box"], without["slot_box"])
    only = A.augment(b, 1, seed=3, jitter=0.25)                        # jitter alone turns the stage on: targets are cropped, not moved
    inside = ((b["tgt_box"][..., :2] - 0.5 * b["tgt_box"][..., 2:] >= 0) & (b["tgt_box"][..., :2] + 0.5 * b["tgt_box"][..., 2:] <= 1)).all(-1)
    inside &= b["valid"] > 0
    assert float((only["tgt_box"][inside] - b["tgt_box"][inside]).abs().max()) <= 2.0 ** -22


def test_flip_share_at_one_half():
    """4096 clips at p = 0.5: the flips number 2048 +- 5 binomial standard deviations (5 * sqrt(4096 / 4) = 160)"""
    flip, _, _, _ = A.clip_draw(4096, 0, A.COIN_SEED, A.threshold(0.5), 0.0, 0.0)
    assert abs(int(flip.sum()) - 2048) <= 160, int(flip.sum())
    other, _, _, _ = A.clip_draw(4096, 1, A.COIN_SEED, A.threshold(0.5), 0.0, 0.0)
    assert abs(int(other.sum()) - 2048) <= 160 and not np.array_equal(flip, other)


def test_v_is_exact_and_in_range():
    x = np.array([0, 255, 256, 2 ** 31, 2 ** 32 - 1], dtype=np.uint64)
    got = A.v(x)
    assert got.dtype == np.float32 and got[0] == -1.0 and got[1] == -1.0 and got[3] == 0.0 and got[4] == np.float32(1.0 - 2.0 ** -23)
    assert got[2] == np.float32(-1.0 + 2.0 ** -23)


def test_planner_is_the_restatements_threshold():
    from vlg import hip
    lib = hip.load()
    t = ctypes.c_uint32()
    for p in (0.0, 2.0 ** -24, 0.1, 0.5, 1.0):
        assert lib.vlg_augment_plan(p, ctypes.byref(t)) == 0 and t.value == A.threshold(p) == int(round(p * 2 ** 24)), p
    for bad in (-1e-9, 1.0000001, float("nan")):
        assert lib.vlg_augment_plan(bad, ctypes.byref(t)) == 1001
        with pytest.raises(ValueError):
            A.threshold(bad)
    assert lib.vlg_augment_plan(0.5, None) == 1001


def test_augment_options():
    from vlg.spec import augment_options
    assert augment_options() == (0.0, 0.0, 0.0, 0.0, 0.0)
    assert augment_options(1, 0.5, "0.5", 0.25, 0.999) == (1.0, 0.5, 0.5, 0.25, 0.999)
    assert augment_options(drop=0.25) == (0.0, 0.0, 0.0, 0.0, 0.25)
    for kw, name in ((dict(flip=1.5), "aug_flip"), (dict(flip=-0.1), "aug_flip"), (dict(flip=float("nan")), "aug_flip"),
                     (dict(zoom=0.6), "aug_zoom"), (dict(zoom=-0.1), "aug_zoom"), (dict(zoom=float("nan")), "aug_zoom"),
                     (dict(shift=0.51), "aug_shift"), (dict(shift=-1), "aug_shift"), (dict(shift=float("nan")), "aug_shift"),
                     (dict(jitter=0.26), "aug_jitter"), (dict(jitter=-0.01), "aug_jitter"), (dict(jitter=float("inf")), "aug_jitter"),
                     (dict(jitter=float("nan")), "aug_jitter"), (dict(drop=1.0), "aug_drop"), (dict(drop=-0.1), "aug_drop"),
                     (dict(drop=float("nan")), "aug_drop"), (dict(flip="x"), "aug_flip")):
        with pytest.raises(ValueError, match=name):
            augment_options(**kw)
    with pytest.raises(ValueError, match="VLG_AUG_ZOOM"):               # the message names what the caller calls it
        augment_options(zoom=2, names=("VLG_AUG_FLIP", "VLG_AUG_ZOOM", "VLG_AUG_SHIFT", "VLG_AUG_JITTER", "VLG_AUG_DROP"))


AUG_ENV = ("VLG_AUG_FLIP", "VLG_AUG_ZOOM", "VLG_AUG_SHIFT", "VLG_AUG_JITTER", "VLG_AUG_DROP", "VLG_AUG_SEED")


def _args(**kw):
    return argparse.Namespace(seed=1024, rank=0, **kw)


def test_augment_knobs(monkeypatch):
    from trainer import augment_knobs, device_flip
    for k in AUG_ENV:
        monkeypatch.delenv(k, raising=False)
    assert augment_knobs(_args()) == {} and not device_flip(_args())
    monkeypatch.setenv("VLG_AUG_SEED", "5")                             # the seed alone does not turn it on
    assert augment_knobs(_args()) == {}
    monkeypatch.delenv("VLG_AUG_SEED")
    monkeypatch.setenv("VLG_AUG_ZOOM", "0.25")
    assert augment_knobs(_args()) == dict(aug_flip=0.0, aug_zoom=0.25, aug_shift=0.0, aug_jitter=0.0, aug_drop=0.0, aug_seed=1024)
    assert not device_flip(_args())                                     # the host's flip stands down for VLG_AUG_FLIP alone
    a = _args()
    a.rank = 3
    assert augment_knobs(a)["aug_seed"] == 1027                         # ranks draw differently
    monkeypatch.setenv("VLG_AUG_SEED", "7")
    monkeypatch.setenv("VLG_AUG_FLIP", "0.5")
    monkeypatch.setenv("VLG_AUG_DROP", "0.1")
    got = augment_knobs(a)
    assert got["aug_seed"] == 10 and got["aug_flip"] == 0.5 and got["aug_drop"] == 0.1 and device_flip(a)
    assert augment_knobs(_args(aug_flip=0.0))["aug_flip"] == 0.0        # 0 is ON; args win
    for k in AUG_ENV:
        monkeypatch.delenv(k, raising=False)
    assert augment_knobs(_args(aug_jitter=0.0)) == dict(aug_flip=0.0, aug_zoom=0.0, aug_shift=0.0, aug_jitter=0.0, aug_drop=0.0,
                                                        aug_seed=1024)
    assert device_flip(_args(aug_flip=0.0)) and not device_flip(_args(aug_jitter=0.1))
    for env, bad in (("VLG_AUG_FLIP", "1.5"), ("VLG_AUG_FLIP", "nan"), ("VLG_AUG_ZOOM", "0.6"), ("VLG_AUG_SHIFT", "-0.1"),
                     ("VLG_AUG_JITTER", "0.3"), ("VLG_AUG_DROP", "1"), ("VLG_AUG_DROP", "nan"), ("VLG_AUG_ZOOM", "much")):
        with monkeypatch.context() as m:
            m.setenv(env, bad)
            with pytest.raises(ValueError, match=env):
                augment_knobs(_args())
    with monkeypatch.context() as m:
        m.setenv("VLG_AUG_FLIP", "0.5")
        m.setenv("VLG_AUG_SEED", "-1")
        with pytest.raises(ValueError, match="VLG_AUG_SEED"):
            augment_knobs(_args())


def test_the_pixel_step_refuses_the_knobs(tmp_path, monkeypatch):
    (tmp_path / "src").mkdir()
    monkeypatch.chdir(tmp_path / "src")
    for k in AUG_ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("VLG_MODEL", "gridnet")
    monkeypatch.setenv("VLG_AUG_FLIP", "0.5")
    from trainer import Trainer
    with pytest.raises(ValueError, match="VLG_AUG"):
        Trainer(reference_args(tmp_path / "exp", batch_size=2, epochs=1, print_freq=1, train_clips=4, val_clips=2))


def test_the_host_flip_runs_unless_the_device_flips(tmp_path, monkeypatch):
    """with VLG_AUG_FLIP unset the trainer does what it always did: train() draws the host's per-batch coin"""
    from helpers import oracle_factory
    import trainer as TR
    (tmp_path / "src").mkdir()
    monkeypatch.chdir(tmp_path / "src")
    for k in AUG_ENV + ("VLG_MODEL",):
        monkeypatch.delenv(k, raising=False)
    small = dict(batch_size=4, epochs=1, print_freq=1, n_frames=4, n_slots=8, d_model=64, n_layers=1, train_clips=8, val_clips=4)
    tr = TR.Trainer(reference_args(tmp_path / "exp", **small), engine_factory=oracle_factory)
    calls = []
    monkeypatch.setattr(TR.Trainer, "_flip", lambda self, batch: calls.append(1) or batch)
    tr.set_epoch(0)
    tr.train()
    assert not tr.device_flip and len(calls) == len(tr.train_loader) == 2
