"""GPU: vlg_label_confusion against numpy's bincount (tests/raster_ref.py confusion_ref), exactly: the counts are integers.

Maps are piecewise constant like rasters (runs of random length, so that the in-register merge, the whole-wavefront merge and
the plain path all occur), fully random, or one single bin (every add of the launch lands on one LDS word).  Records start
from non-zero sentinels: the kernel must ADD."""
import functools

import numpy as np
import pytest
import torch

import raster_ref as R

pytestmark = pytest.mark.gpu

ERR_SHAPE, ERR_ALIGN = 1001, 1002


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _maps(B, T, hw, top, style, seed=0):
    """two (B,T,hw) uint8 maps with labels in [0, top)"""
    g = np.random.default_rng(1000 * seed + 31 * B + 7 * T + hw + top)
    n = B * T * hw
    if style == "random":
        pred, truth = g.integers(0, top, n), g.integers(0, top, n)
    elif style == "one":
        pred, truth = np.full(n, top - 1), np.full(n, top - 1)
    else:                                   # runs: lengths 1 .. 4096, log-uniform; the two maps break at different places
        def runs():
            lens = np.exp(g.uniform(0, np.log(4096), n // 8 + 16)).astype(np.int64) + 1
            lens = lens[:int(np.searchsorted(np.cumsum(lens), n)) + 1]               # the first runs that fill the map
            return np.repeat(g.integers(0, top, len(lens)), lens)[:n]
        pred, truth = runs(), runs()
        assert len(pred) == n and len(truth) == n
    return (torch.from_numpy(pred.astype(np.uint8)).view(B, T, hw), torch.from_numpy(truth.astype(np.uint8)).view(B, T, hw))


def _record(dev, rows, L):
    start = (1000 + 7 * torch.arange(rows * (L * L + 1))).view(rows, L * L + 1)
    return start, start.to(dev)


def _launch(dev, maps, rec, L, per_frame):
    from vlg import hip
    pred, truth = (m.to(dev) for m in maps)
    B, T, hw = pred.shape
    hip.call("vlg_label_confusion", pred.data_ptr(), truth.data_ptr(), rec.data_ptr(), B, T, hw, L, int(per_frame), _stream())
    torch.cuda.synchronize()


CASES = [  # (B, T, hw), n_labels, labels drawn from [0, top), style
    ((1, 1, 16), 21, 21, "random"), ((1, 1, 16), 1, 1, "one"), ((1, 1, 16), 1, 3, "random"),
    ((2, 3, 33 * 64), 21, 21, "runs"), ((2, 3, 33 * 64), 21, 21, "random"), ((2, 3, 33 * 64), 21, 21, "one"),
    ((2, 3, 33 * 64), 32, 32, "runs"), ((2, 3, 33 * 64), 32, 256, "random"), ((2, 3, 33 * 64), 21, 24, "runs"),
    ((2, 3, 33 * 64), 1, 2, "runs"), ((3, 5, 16), 21, 23, "random"),
    ((3, 2, 1 << 20), 21, 22, "runs"),                             # 6.3 M pixels: more vectors than one pass of the capped grid holds
    ((4, 7, 128 * 128), 32, 32, "one"),
]


@pytest.mark.parametrize("per_frame", [False, True])
@pytest.mark.parametrize("shape,L,top,style", CASES)
def test_equals_bincount(dev, shape, L, top, style, per_frame):
    maps = _maps(*shape, top, style)
    rows = shape[1] if per_frame else 1
    start, rec = _record(dev, rows + 1, L)                              # one row more than the launch may touch
    _launch(dev, maps, rec, L, per_frame)
    got = (rec.cpu() - start).numpy()
    want = R.confusion_ref(maps[0].numpy(), maps[1].numpy(), L, per_frame)
    print("\n%s L %d %s per_frame %d: ignored %d of %d" % (shape, L, style, per_frame, int(want[:, -1].sum()), int(want.sum())))
    assert np.array_equal(got[:rows], want)
    assert not got[rows].any()
    assert int(got.sum()) == shape[0] * shape[1] * shape[2]              # conservation
    if top > L:
        assert int(want[:, -1].sum()) > 0


def test_two_launches_double_a_record(dev):
    maps = _maps(2, 3, 33 * 64, 21, "runs")
    start, rec = _record(dev, 3, 21)
    _launch(dev, maps, rec, 21, True)
    once = rec.cpu() - start
    _launch(dev, maps, rec, 21, True)
    assert torch.equal(rec.cpu() - start, 2 * once) and int(once.sum()) == 2 * 3 * 33 * 64


def test_refusals(dev):
    from vlg import hip
    f = hip.load().vlg_label_confusion
    pred, truth = (m.to(dev) for m in _maps(2, 3, 33 * 64, 21, "runs"))
    start, rec = _record(dev, 3, 21)
    ok = dict(pred=pred.data_ptr(), truth=truth.data_ptr(), counts=rec.data_ptr(), B=2, T=3, hw=33 * 64, n_labels=21, per_frame=1)
    shape_bad = [dict(n_labels=0), dict(n_labels=33), dict(hw=0), dict(hw=8), dict(hw=33 * 64 + 8), dict(B=0), dict(T=0),
                 dict(B=1 << 15, T=1 << 10, hw=64), dict(hw=1 << 31), dict(pred=0), dict(truth=0), dict(counts=0)]
    align_bad = [dict(pred=pred.data_ptr() + 8), dict(truth=truth.data_ptr() + 1), dict(counts=rec.data_ptr() + 4)]
    for want, overs in ((ERR_SHAPE, shape_bad), (ERR_ALIGN, align_bad)):
        for over in overs:
            assert f(*dict(ok, **over).values(), _stream()) == want, over
    torch.cuda.synchronize()
    assert torch.equal(rec.cpu(), start)
    assert f(*ok.values(), _stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal((rec.cpu() - start).numpy(), R.confusion_ref(pred.cpu().numpy(), truth.cpu().numpy(), 21, True))
