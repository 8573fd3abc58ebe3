"""CPU: the rasteriser's definition on its reference (tests/raster_ref.py) - the worked example of include/vlg_hip.h and
every rule a device test later relies on - and the host side of vlg/raster.py: PixelRecord.summary(), raster_options,
trainer.pixel_knobs."""
import types

import numpy as np
import pytest
import torch

import raster_ref as R

NAN, INF = float("nan"), float("inf")
BG = 20


def _draw(slots, size=(8, 16), valid=None, what="class", n_classes=20, background=BG):
    """slots: list of (class, cx, cy, w, h) of one frame -> its (H,W) label map"""
    cls = np.array([[[s[0] for s in slots]]], dtype=np.int64)
    box = np.array([[[s[1:] for s in slots]]], dtype=np.float32)
    v = None if valid is None else np.array([[valid]], dtype=np.float32)
    return R.raster_ref(cls, box, v, size, n_classes, background, what)[0, 0]


def test_worked_example():
    got = _draw([(3, .5, .5, .5, .5), (5, .5, .5, .25, .25), (7, .25, .5, .25, .25)])
    wide = [BG] * 4 + [3] * 8 + [BG] * 4
    mid = [BG, BG, 7, 7, 7, 7, 5, 5, 5, 5, 3, 3, BG, BG, BG, BG]
    want = np.array([[BG] * 16] * 2 + [wide, mid, mid, wide] + [[BG] * 16] * 2)
    assert np.array_equal(got, want)
    # slot mode: the same picture in slot indices, background N unless told otherwise
    slots = _draw([(3, .5, .5, .5, .5), (5, .5, .5, .25, .25), (7, .25, .5, .25, .25)], what="slot", background=3)
    assert np.array_equal(slots, np.select([want == 3, want == 5, want == 7], [0, 1, 2], 3))


def test_equal_areas_lower_index_wins_and_small_lies_on_top():
    a = _draw([(1, .5, .5, .5, .5), (2, .5, .5, .5, .5)])
    assert set(np.unique(a)) == {1, BG}
    # the same area from another shape (w*h = .25 both): still slot 0 where they overlap
    b = _draw([(1, .5, .5, .5, .5), (2, .5, .5, 1.0, .25)])
    assert b[3, 8] == 1 and b[3, 0] == 2
    # a smaller slot wins whatever its index
    c = _draw([(1, .5, .5, .25, .25), (2, .5, .5, .5, .5)])
    assert c[3, 8] == 1 and c[2, 8] == 2


def test_edges_on_pixel_centres_left_inclusive_right_exclusive():
    # W = 16: X0 = (0.28125 - 0.125) * 16 = 2.5 and X1 = 6.5, both exactly on centres: pixels 2 .. 5
    row = _draw([(4, 0.28125, .5, .25, 1.0)])[0]
    assert row.tolist() == [BG, BG, 4, 4, 4, 4] + [BG] * 10
    # H = 8: Y0 = (0.4375 - 0.125) * 8 = 2.5, Y1 = 4.5: rows 2 and 3
    col = _draw([(4, .5, 0.4375, 1.0, .25)])[:, 0]
    assert col.tolist() == [BG, BG, 4, 4, BG, BG, BG, BG]
    # thinner than a pixel, between two centres: covers nothing; across one centre: covers it
    assert (_draw([(4, 0.5, .5, 0.03, 1.0)]) == BG).all()               # X in (7.76, 8.24): no centre
    assert _draw([(4, 0.53125, .5, 0.03, 1.0)])[0].tolist() == [BG] * 8 + [4] + [BG] * 7      # around 8.5


def test_slots_that_are_not_drawn():
    big = (.5, .5, 1.0, 1.0)
    for cls in (20, 21, -1, 255, -2 ** 40, 2 ** 40):
        assert (_draw([(cls,) + big]) == BG).all(), cls
    assert (_draw([(3,) + big], valid=[0.0]) == BG).all()
    assert (_draw([(3,) + big], valid=[0.5]) == 3).all()                # any non-zero value is valid
    for bad in ((NAN, .5, 1, 1), (.5, INF, 1, 1), (.5, .5, NAN, 1), (.5, .5, 1, INF), (.5, -INF, 1, 1),
                (.5, .5, 0.0, 1), (.5, .5, 1, 0.0), (.5, .5, -1.0, 1), (.5, .5, 1, -0.5)):
        assert (_draw([(3,) + bad]) == BG).all(), bad
    # a slot that is not drawn hides nothing
    assert (_draw([(3,) + big, (20, .5, .5, .1, .1), (4, .5, .5, NAN, .1)]) == 3).all()


def test_boxes_outside_and_over_the_border():
    for out in ((-3.0, .5, 1, 1), (4.0, .5, 1, 1), (.5, -3.0, 1, 1), (.5, 4.0, 1, 1), (1e30, .5, 1, 1), (-1e30, .5, 1, 1),
                (.5, 1e30, 1e10, 1e10)):
        assert (_draw([(3,) + out]) == BG).all(), out
    over = _draw([(3, 0.0, 0.0, .5, .5)])                                # X in [-4, 4), Y in [-2, 2)
    assert (over[:2, :4] == 3).all() and (over[2:] == BG).all() and (over[:, 4:] == BG).all()
    assert (_draw([(3, .5, .5, 1e30, 1e30)]) == 3).all()                 # larger than everything (area overflows to inf)
    assert (_draw([(3, .5, .5, 1e30, 1e30), (4, .5, .5, 3.0, 3.0)]) == 4).all()


def test_frames_and_confusion_ref():
    g = np.random.default_rng(0)
    cls = g.integers(0, 21, (2, 3, 5))
    box = g.random((2, 3, 5, 4)).astype(np.float32)
    full = R.raster_ref(cls, box, None, (7, 16), 20, BG)
    assert np.array_equal(R.raster_ref(cls, box, None, (7, 16), 20, BG, frames=(1, 2)), full[:, 1:])
    pred, truth = g.integers(0, 5, (2, 3, 16)), g.integers(0, 5, (2, 3, 16))
    one, per = R.confusion_ref(pred, truth, 4, False), R.confusion_ref(pred, truth, 4, True)
    assert one.shape == (1, 17) and per.shape == (3, 17) and np.array_equal(per.sum(0), one[0]) and one.sum() == 96
    assert one[0, 16] == int(((pred == 4) | (truth == 4)).sum())
    assert one[0, 2 * 4 + 1] == int(((truth == 2) & (pred == 1)).sum())


# ------------------------------------------------------------------------------------------------ vlg/raster.py
def test_pixel_record_summary_on_a_planted_confusion():
    from vlg.raster import PixelRecord
    rec = PixelRecord(3, rows=2)
    assert rec.counts.shape == (2, 17) and rec.counts.dtype == torch.int64 and rec.n_labels == 4
    empty = rec.summary()
    assert empty[0]["pixels"] == 0 and empty[0]["pixel_accuracy"] is None and empty[0]["miou"] is None
    assert empty[0]["per_class_iou"] == [None] * 3 and empty[0]["background_iou"] is None
    # truth rows x pred columns, labels 0 1 2 and background 3; class 2 never occurs on either side
    conf = [[6, 2, 0, 0],
            [1, 3, 0, 4],
            [0, 0, 0, 0],
            [3, 0, 0, 13]]
    rec.counts[1, :16] = torch.tensor(conf).flatten()
    rec.counts[1, 16] = 5
    s = rec.summary()[1]
    assert s["pixels"] == 32 and s["ignored"] == 5 and s["confusion"] == conf
    assert s["pixel_accuracy"] == 22 / 32
    assert s["per_class_iou"] == [6 / (8 + 10 - 6), 3 / (8 + 5 - 3), None]
    assert s["miou"] == (6 / 12 + 3 / 10) / 2
    assert s["background_iou"] == 13 / (16 + 17 - 13)
    assert rec.summary()[0]["pixels"] == 0
    # all_reduce hands the counts to the callable; reset() zeroes
    seen = []
    rec.all_reduce(lambda ts: seen.extend(ts))
    assert len(seen) == 1 and seen[0] is rec.counts
    rec.reset()
    assert not bool(rec.counts.any())
    for bad in (dict(n_classes=0), dict(n_classes=32), dict(n_classes=3, rows=0)):
        with pytest.raises(ValueError):
            PixelRecord(**bad)


def test_raster_options():
    from vlg.raster import parse_size, raster_options
    assert raster_options((64, 128)) == ((64, 128), 20)
    assert raster_options([1, 16], 0, 5) == ((1, 16), 0)
    assert raster_options((16384, 16384), 255, 255) == ((16384, 16384), 255)
    assert raster_options((7, 48), None, 7) == ((7, 48), 7)
    for size in ((0, 16), (8, 0), (8, 8), (8, 24), (8, 17), (16385, 16), (8, 16400), (8,), 8, None, "8x16", (8.5, 16), (8, 16, 3)):
        with pytest.raises(ValueError):
            raster_options(size)
    for kw in (dict(background=-1), dict(background=256), dict(background=1.5), dict(n_classes=0), dict(n_classes=256)):
        with pytest.raises(ValueError):
            raster_options((8, 16), **kw)
    assert parse_size("64x128") == (64, 128) and parse_size("8X16") == (8, 16)
    for text in ("64", "64x", "x", "64x128x3", "a x b", "", "64,128"):
        with pytest.raises(ValueError):
            parse_size(text)


def test_pixel_knobs(monkeypatch):
    from trainer import pixel_knobs
    monkeypatch.delenv("VLG_VAL_PIXELS", raising=False)
    none = types.SimpleNamespace()
    assert pixel_knobs(none) == {}
    monkeypatch.setenv("VLG_VAL_PIXELS", "64x128")
    assert pixel_knobs(none) == {"size": (64, 128)}
    assert pixel_knobs(types.SimpleNamespace(val_pixels="16x32")) == {"size": (16, 32)}        # args win
    assert pixel_knobs(types.SimpleNamespace(val_pixels=(8, 16))) == {"size": (8, 16)}
    assert pixel_knobs(types.SimpleNamespace(val_pixels="")) == {}
    for bad in ("64x100", "0x16", "64", "64x128x2", "big"):
        monkeypatch.setenv("VLG_VAL_PIXELS", bad)
        with pytest.raises(ValueError):
            pixel_knobs(none)
    monkeypatch.setenv("VLG_VAL_PIXELS", "0")
    assert pixel_knobs(none) == {}
