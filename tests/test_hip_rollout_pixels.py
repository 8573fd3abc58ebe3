"""GPU: the pixel score of rollouts - LayoutEngine.evaluate_rollout(pixel_record=, pixel_size=), the Trainer's pixel knob
and render_layout - on a tiny engine, against the reference rasters (tests/raster_ref.py) of the frames the call itself
returns: the counts are integers and the rasters exact, so everything is compared with equality."""
import numpy as np
import pytest
import torch

import raster_ref as R
from helpers import reference_args

pytestmark = pytest.mark.gpu

SIZE = (16, 32)
S = 3


def _clip(cfg, frames, seed=9):
    g = torch.Generator().manual_seed(seed)
    B, N, C = cfg.B, cfg.N, cfg.n_classes
    cls = torch.randint(0, C, (B, frames, N), generator=g)
    cls[1, frames - 2, 5] = C                                            # one padded truth slot: not drawn
    box = torch.cat([0.2 + 0.6 * torch.rand(B, frames, N, 2, generator=g), 0.1 + 0.4 * torch.rand(B, frames, N, 2, generator=g)], -1)
    return cls, box.contiguous()


@pytest.mark.parametrize("P", [2, 4])
@pytest.mark.parametrize("attention", ["slot", "clip"])
def test_engine_pixel_record(dev, attention, P):
    from vlg.engine import LayoutEngine
    from vlg.raster import PixelRecord
    from vlg.spec import LayoutConfig
    cfg = LayoutConfig(B=2, T=4, N=8, d=64, n_layers=1, attention=attention)
    eng = LayoutEngine(cfg, dev, seed=11)
    C = cfg.n_classes
    clip_class, clip_box = _clip(cfg, P + S)
    cc, cb = clip_class.to(dev), clip_box.to(dev)
    knobs = dict(top_k=5, iou_thr=0.3, return_logits=True, temperature=0.8, sample_top_k=6, seed=1234, prompt_frames=P)
    plain, gen_c0, gen_b0, logits0 = eng.evaluate_rollout(cc, cb, **knobs)
    pix = eng.pixel_record(S)
    rec, gen_c, gen_b, logits = eng.evaluate_rollout(cc, cb, pixel_record=pix, pixel_size=SIZE, **knobs)
    # the token side is bit for bit what it is without the pixel record
    assert torch.equal(gen_c, gen_c0) and torch.equal(gen_b, gen_b0) and torch.equal(logits, logits0)
    assert torch.equal(rec.counts, plain.counts) and torch.equal(rec.sums, plain.sums)
    # the pixel side: the decoded frames against frames P .. P+S-1 of the clip, horizon step i in row i
    drawn = R.raster_ref(gen_c.cpu().numpy(), gen_b.cpu().numpy(), None, SIZE, C, C)
    truth = R.raster_ref(clip_class.numpy(), clip_box.numpy(), None, SIZE, C, C, frames=(P, S))
    want = R.confusion_ref(drawn, truth, C + 1, True)
    got = pix.counts.cpu().numpy()
    print("\n%s P %d: background %.1f %% drawn, %.1f %% true; agreeing pixels per step %s" % (
        attention, P, 100 * float((drawn == C).mean()), 100 * float((truth == C).mean()),
        [int(np.trace(w[:-1].reshape(C + 1, C + 1))) for w in want]))
    assert np.array_equal(got, want)
    assert int(got.sum()) == cfg.B * S * SIZE[0] * SIZE[1] and int(got[:, -1].sum()) == 0
    assert 0.02 < float((truth == C).mean()) < 0.9 and len(np.unique(truth)) > 5      # the truth is a picture, not a blank
    for s in pix.summary():
        assert s["pixels"] == cfg.B * SIZE[0] * SIZE[1] and 0.0 <= s["pixel_accuracy"] <= 1.0 and len(s["per_class_iou"]) == C
    # a given record is added to; the label buffers are kept
    maps = eng._pixel_maps.data_ptr()
    eng.evaluate_rollout(cc, cb, pixel_record=pix, pixel_size=SIZE, **knobs)
    assert np.array_equal(pix.counts.cpu().numpy(), 2 * want) and eng._pixel_maps.data_ptr() == maps
    # refusals come before the rollout: the token record is not added to
    before = rec.counts.clone()
    for bad in (dict(pixel_record=pix), dict(pixel_record=pix, pixel_size=(16, 40)), dict(pixel_record=PixelRecord(C, S), pixel_size=SIZE),
                dict(pixel_record=eng.pixel_record(S - 1), pixel_size=SIZE), dict(pixel_record=eng.metrics_record(S), pixel_size=SIZE)):
        with pytest.raises(ValueError):
            eng.evaluate_rollout(cc, cb, record=rec, **dict(knobs, **bad))
    assert torch.equal(rec.counts, before)


LAYOUT_CFG = dict(batch_size=2, epochs=1, print_freq=1, n_frames=4, n_slots=8, d_model=64, n_layers=1, train_clips=4, val_clips=6)
PIXEL_KEYS = {"pixel_miou", "pixel_accuracy", "pixel_per_class_iou", "pixel_background_iou"}


def test_trainer_pixel_keys_and_render_layout(tmp_path, monkeypatch, dev):
    (tmp_path / "src").mkdir()
    monkeypatch.chdir(tmp_path / "src")
    for k in ("VLG_MODEL", "VLG_VARIABLE_N", "VLG_VAL_METRICS", "VLG_VAL_TOPK", "VLG_VAL_IOU_THR", "VLG_GEN_TEMPERATURE", "VLG_GEN_TOP_K",
              "VLG_GEN_SEED", "VLG_GEN_KEEP_PADDED", "VLG_ATTENTION", "VLG_PRECISION", "VLG_VAL_PIXELS"):
        monkeypatch.delenv(k, raising=False)
    from trainer import Trainer
    tr = Trainer(reference_args(tmp_path / "exp", **LAYOUT_CFG))
    clip_class, clip_box = _clip(tr.cfg, tr.cfg.T + S)
    off = tr.evaluate_rollout(clip_class, clip_box)
    assert len(off) == S and not any(PIXEL_KEYS & set(s) for s in off)
    monkeypatch.setenv("VLG_VAL_PIXELS", "16x32")
    on = tr.evaluate_rollout(clip_class, clip_box)
    assert len(on) == S
    for a, b in zip(off, on):
        assert set(b) == set(a) | PIXEL_KEYS and all(b[k] == a[k] or (b[k] != b[k] and a[k] != a[k]) for k in a)
        assert 0.0 <= b["pixel_accuracy"] <= 1.0 and len(b["pixel_per_class_iou"]) == tr.cfg.n_classes
        assert b["pixel_miou"] is None or 0.0 <= b["pixel_miou"] <= 1.0
        assert b["pixel_background_iou"] is None or 0.0 <= b["pixel_background_iou"] <= 1.0
    # the same figures from the engine's own record
    gen_c, gen_b = tr.generate_sequence(clip_class[:, :tr.cfg.T], clip_box[:, :tr.cfg.T], steps=S)
    C = tr.cfg.n_classes
    want = R.confusion_ref(R.raster_ref(gen_c.numpy(), gen_b.numpy(), None, SIZE, C, C),
                           R.raster_ref(clip_class.numpy(), clip_box.numpy(), None, SIZE, C, C, frames=(tr.cfg.T, S)), C + 1, True)
    for i, b in enumerate(on):
        conf = want[i, :-1].reshape(C + 1, C + 1)
        assert b["pixel_accuracy"] == np.trace(conf) / conf.sum()
    # render_layout: the knob's size, CPU tensors in and out, the float maps the pixel model takes
    seg = tr.render_layout(clip_class, clip_box)
    assert seg.dtype == torch.float32 and not seg.is_cuda and tuple(seg.shape) == (2, tr.cfg.T + S, 16, 32)
    direct = tr.engine.rasterize(clip_class.to(dev), clip_box.to(dev), SIZE, dtype=torch.float32).cpu()
    assert torch.equal(seg, direct)
    assert np.array_equal(seg.numpy().astype(np.int64), R.raster_ref(clip_class.numpy(), clip_box.numpy(), None, SIZE, C, C))
    assert tuple(seg[:, 1:2].shape) == (2, 1, 16, 32)                    # a seg argument of the gridnet generate_sequence
    valid = (torch.arange(8) % 2).float().expand(2, tr.cfg.T + S, 8)
    slots = tr.render_layout(clip_class, clip_box, size=(8, 16), valid=valid, what="slot", dtype=torch.int64)
    assert np.array_equal(slots.numpy(), R.raster_ref(clip_class.numpy(), clip_box.numpy(), valid.numpy(), (8, 16), C, 8, "slot"))
    monkeypatch.delenv("VLG_VAL_PIXELS")
    assert tr.evaluate_rollout(clip_class, clip_box)[0].keys() == off[0].keys()
    with pytest.raises(ValueError):
        tr.render_layout(clip_class, clip_box)                            # no size and no knob
