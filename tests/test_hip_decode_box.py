"""GPU: vlg_layout_decode_ext / vlg_layout_decode_append_ext (csrc/decode.hip) - the decoding step with a row stride and a
box DRAWN from the Gaussian box head - against the plain entries (bit for bit where nothing is drawn) and against
tests/boxhead_ref.py.  Every output buffer starts as NaN / -1 sentinels.

Bar of a sampled box: boxhead_ref.box_bar = 1e-5 * max(1, tau) (fp32 Box-Muller against fp64 on the same u differs by at
most 1.9e-6; sigma <= 1; the clamp is continuous: no draw is excluded)."""
import pytest
import torch

import boxhead_ref as R

pytestmark = pytest.mark.gpu

NC = 20
ERR_SHAPE = 1001
NAN = float("nan")
B, T, N, STEPS = 3, 4, 23, 3          # 69 tokens: one full and one partial 64-token block
KINDS = ("slide", "append")
POS = 2                               # the appending entry writes frame POS from frame POS - 1


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _inputs(seed=1):
    """(rows (B*N, 32) = logits | raw mean | raw scale | NaN, cls (B,T,N), box (B,T,N,4)): raw means at +-8 in places, so that
    a drawn box reaches both clamps; padded slots in the newest frame of both entries"""
    g = torch.Generator().manual_seed(seed)
    rows = torch.randn(B * N, 32, generator=g) * 3
    rows[:, NC + 4:NC + 8] = torch.randn(B * N, 4, generator=g) * 4          # sigma from e^-7 to 1
    rows[::5, NC:NC + 4] = 8.0
    rows[2::5, NC:NC + 4] = -8.0
    rows[::5, NC + 4:NC + 8] = 9.0                                            # ... with sigma = 1 there
    rows[2::5, NC + 4:NC + 8] = 9.0
    rows[:, NC + 8:] = NAN                                                    # never read
    cls = torch.randint(0, NC, (B, T, N), generator=g)
    box = torch.rand(B, T, N, 4, generator=g)
    cls[0, T - 1, 3] = cls[2, T - 1, 20] = cls[1, POS - 1, 7] = cls[0, POS - 1, 22] = NC
    return rows, cls, box


class Call:
    """buffers of one decoding call of either kind, outputs pre-filled with sentinels"""

    def __init__(self, dev, kind, rows, cls, box, shape=(B, T, N)):
        b, t, n = shape
        self.kind, self.shape = kind, shape
        self.rows = rows.to(dev).contiguous()
        self.cls_in, self.box_in = cls.view(b, t, n).to(dev).contiguous(), box.view(b, t, n, 4).to(dev).contiguous()
        self.gen_cls = torch.full((b, STEPS, n), -1, dtype=torch.int64, device=dev)
        self.gen_box = torch.full((b, STEPS, n, 4), NAN, device=dev)
        if kind == "slide":
            self.cls_out = torch.full((b, t, n), -1, dtype=torch.int64, device=dev)
            self.box_out = torch.full((b, t, n, 4), NAN, device=dev)
            self.valid = torch.full((b, t, n), NAN, device=dev)
        else:                             # in place: the window itself, and the compact frame
            self.valid = torch.full((b, t, n), NAN, device=dev)
            self.frame_cls = torch.full((b, n), -1, dtype=torch.int64, device=dev)
            self.frame_box = torch.full((b, n, 4), NAN, device=dev)

    def run(self, step, ext, ld=None, temperature=0.0, top_k=0, tau=0.0, seed=0, keep_padded=0, expect=0):
        from vlg import hip
        b, t, n = self.shape
        p = lambda x: x.data_ptr()
        head = (p(self.rows),) + ((ld,) if ext else ())
        knobs = (temperature, top_k) + ((tau,) if ext else ()) + (seed, keep_padded, _stream())
        if self.kind == "slide":
            name = "vlg_layout_decode" + ("_ext" if ext else "")
            args = head + (p(self.cls_in), p(self.box_in), p(self.cls_out), p(self.box_out), p(self.valid), p(self.gen_cls),
                           p(self.gen_box), b, t, n, NC, STEPS, step) + knobs
        else:
            name = "vlg_layout_decode_append" + ("_ext" if ext else "")
            args = head + (p(self.cls_in), p(self.box_in), p(self.valid), p(self.gen_cls), p(self.gen_box), p(self.frame_cls),
                           p(self.frame_box), b, t, n, NC, POS, STEPS, step) + knobs
        code = getattr(hip.load(), name)(*args)
        torch.cuda.synchronize()
        assert code == expect, "%s returned %d, expected %d" % (name, code, expect)
        return self

    def outputs(self):
        names = ("cls_out", "box_out", "valid", "gen_cls", "gen_box") if self.kind == "slide" else \
            ("cls_in", "box_in", "valid", "gen_cls", "gen_box", "frame_cls", "frame_box")
        return [getattr(self, k).cpu() for k in names]

    def newest(self):
        """the history's newest frame as (1-frame window) the restatement's keep_padded looks at"""
        t = self.shape[1] - 1 if self.kind == "slide" else POS - 1
        return t


def _same(a, b):
    return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in zip(a.outputs(), b.outputs()))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("temperature,top_k,keep", [(0.0, 0, 0), (0.9, 5, 1)])
def test_ext_without_a_box_draw_is_the_plain_entry(dev, kind, temperature, top_k, keep):
    rows, cls, box = _inputs()
    dense = rows[:, :NC + 4].contiguous()
    kw = dict(temperature=temperature, top_k=top_k, seed=77, keep_padded=keep)
    old = Call(dev, kind, dense, cls, box).run(1, False, **kw)
    # ld = C + 4, tau = 0: every output bit for bit
    assert _same(old, Call(dev, kind, dense, cls, box).run(1, True, ld=NC + 4, tau=0.0, **kw))
    # ld = 32, tau = 0 on the repacked rows (scale columns and NaN padding behind the 24 it reads)
    wide = Call(dev, kind, rows, cls, box).run(1, True, ld=32, tau=0.0, **kw)
    assert _same(old, wide)
    assert bool(torch.isfinite(wide.gen_box[:, 1]).all()) and bool((wide.gen_cls[:, [0, 2]] == -1).all())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("tau", [0.5, 2.0])
def test_sampled_boxes_match_the_restatement(dev, kind, tau):
    rows, cls, box = _inputs()
    step, seed = 2, 0xB0C5F00D1234
    kw = dict(temperature=0.9, top_k=5, seed=seed, keep_padded=1)
    old = Call(dev, kind, rows[:, :NC + 4].contiguous(), cls, box).run(step, False, **kw)
    got = Call(dev, kind, rows, cls, box).run(step, True, ld=32, tau=tau, **kw)
    # the box stream does not disturb the class stream
    assert torch.equal(got.gen_cls.cpu(), old.gen_cls.cpu())
    gb = got.gen_box[:, step].cpu()
    t_new = got.newest()
    want_cls, want_box, _ = R.next_frame(rows[:, :NC + 8], cls[:, :t_new + 1], box[:, :t_new + 1], NC, step, 0.9, 5, seed,
                                         keep_padded=True, box_temperature=tau)
    err = (gb.double() - want_box).abs()
    print("\n%s tau %g: largest |box - reference| %.3g (bar %.3g)" % (kind, tau, float(err.max()), R.box_bar(tau)))
    assert float(err.max()) <= R.box_bar(tau)
    assert bool(((gb >= 0) & (gb <= 1)).all()) and bool((gb == 0).any()) and bool((gb == 1).any()), "both clamps must be reached"
    # kept slots keep class and box, bit for bit
    pad = cls[:, t_new] >= NC
    assert int(pad.sum()) == 2 and torch.equal(gb[pad], box[:, t_new][pad]) and bool((got.gen_cls[:, step].cpu()[pad] == NC).all())
    # the drawn frame is what every output holds
    if kind == "slide":
        assert torch.equal(got.box_out[:, -1].cpu(), gb) and torch.equal(got.box_out[:, :-1].cpu(), box[:, 1:])
    else:
        assert torch.equal(got.box_in[:, POS].cpu(), gb) and torch.equal(got.frame_box.cpu(), gb)
        assert torch.equal(got.box_in[:, :POS].cpu(), box[:, :POS]) and torch.equal(got.box_in[:, POS + 1:].cpu(), box[:, POS + 1:])
    # it differs from the mean box where nothing clamps or pads, and another seed or step draws differently
    assert not torch.equal(gb, old.gen_box[:, step].cpu())
    again = Call(dev, kind, rows, cls, box).run(step, True, ld=32, tau=tau, **kw)
    assert _same(got, again)
    other = Call(dev, kind, rows, cls, box).run(step, True, ld=32, tau=tau, **dict(kw, seed=seed + 1))
    assert not torch.equal(other.gen_box[:, step].cpu(), gb)
    # columns >= C + 8 hold NaN above; finite ones change nothing
    clean = rows.clone()
    clean[:, NC + 8:] = 0.25
    assert _same(got, Call(dev, kind, clean, cls, box).run(step, True, ld=32, tau=tau, **kw))
    # the same flattened tokens as one clip of 69 slots: the counter is the token index, not the launch geometry
    flat = Call(dev, kind, rows, cls.permute(1, 0, 2).reshape(1, T, B * N), box.permute(1, 0, 2, 3).reshape(1, T, B * N, 4),
                shape=(1, T, B * N)).run(step, True, ld=32, tau=tau, **kw)
    assert torch.equal(flat.gen_box[0, step].cpu().view(B, N, 4), gb)
    assert torch.equal(flat.gen_cls[0, step].cpu().view(B, N), got.gen_cls[:, step].cpu())


@pytest.mark.parametrize("kind", KINDS)
def test_ext_refusals_write_nothing(dev, kind):
    rows, cls, box = _inputs()
    for bad in (dict(tau=-0.5), dict(tau=NAN), dict(tau=float("inf")), dict(tau=1.0, ld=NC + 4), dict(tau=0.0, ld=NC),
                dict(tau=0.0, ld=26), dict(tau=1.0, ld=30)):
        kw = dict(dict(ld=32), **bad)
        c = Call(dev, kind, rows, cls, box)
        before = c.outputs()
        c.run(1, True, expect=ERR_SHAPE, **kw)
        after = c.outputs()
        for x, y in zip(before, after):
            assert torch.equal(torch.nan_to_num(x.double(), nan=-7.0), torch.nan_to_num(y.double(), nan=-7.0)), bad
