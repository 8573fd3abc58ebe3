"""GPU: vlg_layout_augment through the C ABI against the CPU restatement of the rule (tests/augment_ref.py): all four
outputs bit for bit.  Every output buffer starts as -1 / NaN sentinels."""
import itertools

import pytest
import torch

import augment_ref as A

pytestmark = pytest.mark.gpu

NC = A.NC
ERR_SHAPE, ERR_ALIGN = 1001, 1002
NAN = float("nan")
KEYS = ("slot_class", "slot_box", "tgt_box", "valid")


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Aug:
    """buffers of one vlg_layout_augment call, outputs pre-filled with sentinels"""

    def __init__(self, dev, batch, counter=0):
        self.shape = tuple(batch["slot_class"].shape)
        B, T, N = self.shape
        self.inp = {k: batch[k].to(dev).contiguous() for k in KEYS}
        self.out = {"slot_class": torch.full((B, T, N), -1, dtype=torch.int64, device=dev),
                    "slot_box": torch.full((B, T, N, 4), NAN, device=dev), "tgt_box": torch.full((B, T, N, 4), NAN, device=dev),
                    "valid": torch.full((B, T, N), NAN, device=dev)}
        self.step = torch.full((1,), counter, dtype=torch.int32, device=dev)

    def args(self, thr_flip=0, thr_drop=0, zoom=0.0, shift=0.0, jitter=0.0, seed=0, n_classes=NC, **over):
        B, T, N = self.shape
        a = dict(cls=self.inp["slot_class"].data_ptr(), box=self.inp["slot_box"].data_ptr(), tgt_box=self.inp["tgt_box"].data_ptr(),
                 valid=self.inp["valid"].data_ptr(), aug_cls=self.out["slot_class"].data_ptr(), aug_box=self.out["slot_box"].data_ptr(),
                 aug_tgt_box=self.out["tgt_box"].data_ptr(), aug_valid=self.out["valid"].data_ptr(), step=self.step.data_ptr(),
                 B=B, T=T, N=N, n_classes=n_classes, thr_flip=thr_flip, thr_drop=thr_drop, zoom=zoom, shift=shift, jitter=jitter,
                 seed=seed)
        a.update(over)
        return list(a.values()) + [_stream()]

    def run(self, **kw):
        from vlg import hip
        hip.call("vlg_layout_augment", *self.args(**kw))
        return {k: t.cpu() for k, t in self.out.items()}

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.out["slot_class"] == -1).all()) and all(bool(torch.isnan(self.out[k]).all()) for k in KEYS[1:])


def _check(dev, batch, k, seed, what, thr_flip=None, thr_drop=None, **knobs):
    """one launch against the restatement: classes equal, the three float outputs bit for bit, the caller's tensors and the
    counter unchanged -> the restatement's dict"""
    want = A.augment(batch, k, seed, thr_flip=thr_flip, thr_drop=thr_drop, **knobs)
    m = Aug(dev, batch, counter=k)
    got = m.run(thr_flip=A.threshold(knobs.get("flip", 0.0)) if thr_flip is None else thr_flip,
                thr_drop=A.threshold(knobs.get("drop", 0.0)) if thr_drop is None else thr_drop,
                zoom=knobs.get("zoom", 0.0), shift=knobs.get("shift", 0.0), jitter=knobs.get("jitter", 0.0), seed=seed)
    assert torch.equal(got["slot_class"], want["slot_class"]), what + ": classes"
    for key in KEYS[1:]:
        assert torch.equal(A.bits(got[key]), A.bits(want[key])), what + ": " + key
    for key in KEYS:
        mine, theirs = m.inp[key].cpu(), batch[key]
        assert torch.equal(mine, theirs) if key == "slot_class" else torch.equal(A.bits(mine), A.bits(theirs)), what + ": the caller's " + key
    assert torch.equal(m.step.cpu(), torch.tensor([k], dtype=torch.int32))
    return want


@pytest.mark.parametrize("B,T,N", A.SHAPES)
def test_kernel_matches_the_restatement(dev, B, T, N):
    """padded inputs and valid == 0 targets whose class is real in one batch; each knob alone at one (step, seed), all of
    them together at every step x seed"""
    batch = A.kernel_case(B, T, N, seed=B * 100 + N)
    assert bool((batch["slot_class"] == NC).any()) and bool(((batch["valid"] == 0) & (batch["slot_class"] < NC)).any())
    for knobs in A.KNOBS[:-1]:
        _check(dev, batch, 1, A.SEEDS[1], "(%d,%d,%d) %r" % (B, T, N, knobs), **knobs)
    flips, drops, boxes = [], [], []
    for k, seed in itertools.product(A.STEPS, A.SEEDS):
        want = _check(dev, batch, k, seed, "(%d,%d,%d) all on, step %d seed %#x" % (B, T, N, k, seed), **A.ALL_ON)
        flips.append(want["flip"]), drops.append(want["drop"]), boxes.append(want["slot_box"])
    assert len({tuple(b.flatten().tolist()) for b in boxes}) == len(boxes)      # every (step, seed) draws anew
    if B * N >= 64:
        assert any(bool(d.any()) for d in drops) and any(bool(f.any()) for f in flips)


def test_a_batch_without_padding_and_all_knobs_zero(dev):
    batch = A.kernel_case(3, 4, 5, seed=12, padded=False)
    want = _check(dev, batch, 7, 5, "identity")
    for key in KEYS:
        assert torch.equal(want[key], batch[key])
    _check(dev, batch, 7, 5, "no padding, all on", **A.ALL_ON)


def test_extreme_thresholds(dev):
    """flip = 1 flips every clip; a drop threshold of 2^24 - 1, the largest a probability below 1 can give, drops (nearly)
    every track and one of 2^24 drops them all"""
    batch = A.kernel_case(2, 16, 64, seed=31)
    want = _check(dev, batch, 0, 3, "flip = 1", flip=1.0)
    assert bool(want["flip"].all())
    live = (batch["slot_class"] < NC)
    assert torch.equal(want["slot_box"][live][:, 0], 1.0 - batch["slot_box"][live][:, 0])
    want = _check(dev, batch, 0, 3, "drop thr 2^24 - 1", thr_drop=A.TWO24 - 1)
    assert int(want["drop"].sum()) >= 2 * 64 - 1 and float(want["valid"].sum()) <= 16
    want = _check(dev, batch, 0, 3, "drop thr 2^24", thr_drop=A.TWO24, zoom=0.2)
    assert bool(want["drop"].all()) and bool((want["slot_class"] == NC).all()) and not bool(want["slot_box"].any())
    assert not bool(want["valid"].any())


def test_flip_and_drop_alone_copy_boxes_bit_for_bit(dev):
    """the geometric stage off: the boxes of kept, unflipped tokens are the caller's bits - boxes that stick out of the image,
    a negative zero and a NaN payload included"""
    batch = A.kernel_case(2, 16, 64, seed=41)
    odd = torch.tensor([0x80000000 - 2 ** 32, 0x7FC01234, 0x00000001, 0xFF800000 - 2 ** 32], dtype=torch.int32).view(torch.float32)
    batch["slot_box"][:, 3, 5] = odd
    batch["slot_class"][:, 3, 5] = 1
    want = _check(dev, batch, 2, 99, "flip / drop only", flip=0.5, drop=0.3)     # (step 2 under seed 99 flips one clip of the two)
    flip, drop = want["flip"], want["drop"]
    assert bool(flip.any()) and not bool(flip.all()) and bool(drop.any())
    keep = (~flip)[:, None, None] & (~drop)[:, None, :] & torch.ones(2, 16, 64, dtype=torch.bool)
    assert torch.equal(A.bits(want["slot_box"])[keep], A.bits(batch["slot_box"])[keep])
    sticks = (batch["slot_box"][..., 0] - 0.5 * batch["slot_box"][..., 2] < 0) & keep
    assert bool(sticks.any())
    assert torch.equal(A.bits(want["tgt_box"])[~flip], A.bits(batch["tgt_box"])[~flip])


def test_the_counter_is_read_on_the_device(dev):
    batch = A.kernel_case(1, 32, 33, seed=51)
    m = Aug(dev, batch, counter=0)
    first = m.run(thr_flip=A.threshold(0.5), jitter=0.1, seed=8)
    m.step.fill_(1)                                                     # same arguments, another counter value
    second = m.run(thr_flip=A.threshold(0.5), jitter=0.1, seed=8)
    assert not torch.equal(first["slot_box"], second["slot_box"])
    assert torch.equal(second["slot_box"], A.augment(batch, 1, 8, flip=0.5, jitter=0.1)["slot_box"])


def test_refusals_enqueue_nothing(dev):
    from vlg import hip
    B, T, N = 2, 4, 6
    batch = A.kernel_case(B, T, N, seed=8)
    m = Aug(dev, batch)
    f = hip.load().vlg_layout_augment
    inp, out = m.inp, m.out
    shape = [dict(B=0), dict(T=0), dict(N=0), dict(B=2 ** 16, T=2 ** 15, N=1), dict(n_classes=0),
             dict(thr_flip=A.TWO24 + 1), dict(thr_drop=A.TWO24 + 1),
             dict(zoom=-0.1), dict(zoom=0.51), dict(zoom=NAN), dict(zoom=float("inf")),
             dict(shift=-0.1), dict(shift=0.51), dict(shift=NAN), dict(jitter=-0.01), dict(jitter=0.26), dict(jitter=NAN),
             dict(jitter=float("inf")),
             dict(cls=0), dict(box=0), dict(tgt_box=0), dict(valid=0), dict(aug_cls=0), dict(aug_box=0), dict(aug_tgt_box=0),
             dict(aug_valid=0), dict(step=0),
             dict(aug_cls=inp["slot_class"].data_ptr()), dict(aug_box=inp["slot_box"].data_ptr()),          # in == out
             dict(aug_tgt_box=inp["tgt_box"].data_ptr()), dict(aug_valid=inp["valid"].data_ptr()),
             dict(aug_box=inp["tgt_box"].data_ptr()), dict(aug_valid=m.step.data_ptr()),
             dict(aug_cls=inp["slot_class"].data_ptr() + 8 * N), dict(aug_box=inp["slot_box"].data_ptr() + 16),   # partial overlap
             dict(aug_tgt_box=out["slot_box"].data_ptr()), dict(aug_cls=out["slot_box"].data_ptr()),        # two outputs
             dict(aug_valid=out["tgt_box"].data_ptr() + 16)]
    for over in shape:
        assert f(*m.args(**over)) == ERR_SHAPE, over
        assert m.untouched(), over
    for over in (dict(aug_box=out["slot_box"].data_ptr() + 4), dict(aug_tgt_box=out["tgt_box"].data_ptr() + 8),
                 dict(box=inp["slot_box"].data_ptr() + 8), dict(tgt_box=inp["tgt_box"].data_ptr() + 4),
                 dict(cls=inp["slot_class"].data_ptr() + 4), dict(aug_cls=out["slot_class"].data_ptr() + 4),
                 dict(valid=inp["valid"].data_ptr() + 2), dict(aug_valid=out["valid"].data_ptr() + 2), dict(step=m.step.data_ptr() + 2)):
        assert f(*m.args(**over)) == ERR_ALIGN, over
        assert m.untouched(), over
    for key in KEYS:
        assert torch.equal(inp[key].cpu(), batch[key])
    assert f(*m.args(zoom=0.5, shift=0.5, jitter=0.25, thr_flip=A.TWO24, thr_drop=A.TWO24)) == 0     # the bounds themselves are legal
    torch.cuda.synchronize()
    assert not m.untouched()
