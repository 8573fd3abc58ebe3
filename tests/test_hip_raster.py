"""GPU: vlg_layout_rasterize against the fp32 numpy restatement (tests/raster_ref.py), with EQUALITY: every quantity of the
definition (include/vlg_hip.h) is one correctly rounded fp32 operation.

Inputs (_case): centres uniform in [0, 1), sizes u^3 (never below 2^-20, so that no area is denormal), classes in
0 .. n_classes (the last is the reserved id).  About a quarter of the slots are then replaced by planted ones: duplicates
of another slot of the frame; boxes whose edges lie exactly on pixel centres; sizes below one pixel and (rarely: such a slot fills its frame) above the image;
centres at -3, 4 and +-1e30; NaN / inf values; and valid holds zeros.  test_inputs_cover_the_cases checks on the REFERENCE
that such inputs leave between 2 % and 50 % background and that every label occurs.
Each output sits inside a sentinel-filled buffer whose bytes before and after it must not change."""
import functools

import numpy as np
import pytest
import torch

import raster_ref as R

gpu = pytest.mark.gpu                   # test_inputs_cover_the_cases needs no device

ERR_SHAPE, ERR_ALIGN = 1001, 1002
U8, I64, F32 = 0, 1, 2
DTYPES = {U8: torch.uint8, I64: torch.int64, F32: torch.float32}
SENTINEL = {U8: 0xA5, I64: -77, F32: -77.0}
C = 20
PAD = 16                                # elements around the output: a multiple of 16 bytes for every kind
NAN, INF = float("nan"), float("inf")
SHAPES = [(1, 1, 0, 1, 1, 1, 16), (2, 3, 1, 2, 5, 7, 48), (3, 4, 0, 4, 64, 33, 64), (1, 2, 1, 1, 65, 9, 32),
          (1, 1, 0, 1, 300, 40, 16)]   # (B, T_buf, t0, T, N, H, W); the last: staging loop, more slots than threads, 2 bands


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _case(B, Tb, N, H, W, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 131 * B + 17 * Tb + N + 7 * H + W)
    cls = torch.randint(0, C + 1, (B, Tb, N), generator=g)
    box = torch.cat([torch.rand(B, Tb, N, 2, generator=g), (torch.rand(B, Tb, N, 2, generator=g) ** 3).clamp_(min=2.0 ** -20)], -1)
    kind = torch.randint(0, 30, (B, Tb, N), generator=g)
    k = torch.randint(0, 1 << 20, (B, Tb, N), generator=g)
    for b, t, n in (kind < 10).nonzero().tolist():
        q, r = int(kind[b, t, n]), int(k[b, t, n])
        if q == 0:                      # a duplicate of another slot of the frame, class included: equal areas, the lower index wins
            cls[b, t, n], box[b, t, n] = cls[b, t, r % N], box[b, t, r % N]
        elif q == 1:                    # all four edges exactly on pixel centres (i + 0.5) / W: dyadic, so exact in fp32 for W = 16, 32, 64
            x0, y0 = r % W, (r >> 8) % H
            x1, y1 = x0 + 1 + (r >> 4) % (W - x0), y0 + 1 + (r >> 12) % (H - y0)
            box[b, t, n] = torch.tensor([(x0 + x1 + 1) / (2 * W), (y0 + y1 + 1) / (2 * H), (x1 - x0) / W, (y1 - y0) / H])
        elif q == 2:                    # below one pixel
            box[b, t, n, 2:] = torch.tensor([0.3 / W, 0.7 / H])
        elif q == 3 and r % 16 == 0:    # above the image (rare: one such slot leaves its frame no background)
            box[b, t, n, 2:] = torch.tensor([3.0, 1.5])
        elif q == 4:
            box[b, t, n, r % 2] = (-3.0, 4.0, 1e30, -1e30)[(r >> 1) % 4]
        elif q == 5:
            box[b, t, n, r % 4] = (NAN, INF, -INF)[(r >> 2) % 3]
        elif q == 6 and r % 16 == 1:    # huge sizes (as rare): the area overflows to inf, the slot is still drawn, under everything
            box[b, t, n, 2:] = 1e30
        elif q == 7:                    # left / top edge on a centre, right / bottom edge between centres
            box[b, t, n, :2] = torch.tensor([((r % W) + 0.5) / W, (((r >> 8) % H) + 0.5) / H]) + 0.5 * box[b, t, n, 2:]
        elif q == 8:
            cls[b, t, n] = (-1, C + 5, 255, -2 ** 40)[r % 4]
        # q == 9: zeros in valid, below
    valid = (kind != 9).float() * (1.0 + (k % 3).float())                 # valid values 1, 2, 3 and zeros
    return cls.contiguous(), box.contiguous(), valid.contiguous()


_DEV = {}


def _on(dev, case):
    if id(case) not in _DEV:
        _DEV[id(case)] = tuple(t.to(dev) for t in case)
    return _DEV[id(case)]


def _out(dev, kind, shape):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), SENTINEL[kind], dtype=DTYPES[kind], device=dev)
    return buf, buf[PAD:PAD + n].view(shape)


def _intact(buf, kind, inner=False):
    s = torch.full((), SENTINEL[kind], dtype=DTYPES[kind])
    part = buf.cpu() if inner else torch.cat([buf[:PAD].cpu(), buf[-PAD:].cpu()])
    return bool((part == s).all())


def _args(d, out, shape, kind_, what_, bg_, use_valid=True, **over):
    B, Tb, t0, T, N, H, W = shape
    a = dict(cls=d[0].data_ptr(), box=d[1].data_ptr(), valid=d[2].data_ptr() if use_valid else 0, labels=out.data_ptr(), B=B, T_buf=Tb,
             t0=t0, T=T, N=N, n_classes=C, H=H, W=W, out_kind=kind_, what=what_, background=bg_)
    a.update(over)
    return list(a.values()) + [_stream()]


def _draw(dev, shape, kind, what, use_valid=True, bg=None):
    from vlg import hip
    B, Tb, t0, T, N, H, W = shape
    bg = (C if what == 0 else min(N, 255)) if bg is None else bg
    d = _on(dev, _case(B, Tb, N, H, W))
    buf, out = _out(dev, kind, (B, T, H, W))
    hip.call("vlg_layout_rasterize", *_args(d, out, shape, kind, what, bg, use_valid))
    torch.cuda.synchronize()
    return buf, out, bg


@functools.lru_cache(maxsize=None)
def _ref(shape, what, use_valid=True, bg=None):
    B, Tb, t0, T, N, H, W = shape
    bg = (C if what == 0 else min(N, 255)) if bg is None else bg
    cls, box, valid = _case(B, Tb, N, H, W)
    return R.raster_ref(cls.numpy(), box.numpy(), valid.numpy() if use_valid else None, (H, W), C, bg, ("class", "slot")[what], (t0, T))


@gpu
@pytest.mark.parametrize("what", [0, 1])
@pytest.mark.parametrize("kind", [U8, I64, F32])
@pytest.mark.parametrize("shape", SHAPES)
def test_equals_the_reference(dev, shape, kind, what):
    if what == 1 and kind == U8 and shape[4] > 255:
        from vlg import hip
        d = _on(dev, _case(shape[0], shape[1], shape[4], shape[5], shape[6]))
        buf, out = _out(dev, kind, (shape[0], shape[3], shape[5], shape[6]))
        assert hip.load().vlg_layout_rasterize(*_args(d, out, shape, kind, what, 255)) == ERR_SHAPE     # slot indices do not fit a byte
        torch.cuda.synchronize()
        assert _intact(buf, kind, inner=True)
        return
    buf, out, bg = _draw(dev, shape, kind, what)
    want = _ref(shape, what)
    got = out.cpu().numpy()
    bad = got.astype(np.int64) != want
    print("\n%s kind %d what %d: %d of %d pixels differ, background %.1f %%" % (shape, kind, what, int(bad.sum()), bad.size,
                                                                           100.0 * float((want == bg).mean())))
    assert got.dtype == {U8: np.uint8, I64: np.int64, F32: np.float32}[kind]
    assert not bad.any(), "first difference at %s: got %s want %s" % (np.argwhere(bad)[0], got[bad][0], want[bad][0])
    assert _intact(buf, kind)


@gpu
def test_without_valid_and_other_backgrounds(dev):
    shape = (2, 3, 1, 2, 5, 7, 48)
    for kind in (U8, I64, F32):
        buf, out, _ = _draw(dev, shape, kind, 0, use_valid=False, bg=0)
        assert np.array_equal(out.cpu().numpy().astype(np.int64), _ref(shape, 0, False, 0)) and _intact(buf, kind)
    buf, out, _ = _draw(dev, shape, I64, 1, bg=255)
    assert np.array_equal(out.cpu().numpy(), _ref(shape, 1, True, 255))


def test_inputs_cover_the_cases():
    """on the reference alone: the recipe leaves some background, not only background, and every label occurs"""
    shape = (3, 4, 0, 4, 64, 33, 64)
    want = _ref(shape, 0)
    share = float((want == C).mean())
    print("\nbackground %.1f %% of %d pixels, labels %s" % (100 * share, want.size, np.unique(want).tolist()))
    assert 0.02 < share < 0.50
    assert np.unique(want).tolist() == list(range(C + 1))
    cls, box, valid = _case(3, 4, 64, 33, 64)
    assert bool((valid == 0).any()) and bool(box.isnan().any()) and bool(box.isinf().any()) and float(box[..., :2][box[..., :2].isfinite()].abs().max()) == float(torch.tensor(1e30))
    assert float(box[..., 2:][box[..., 2:].isfinite()].min()) >= 2.0 ** -20
    slots = _ref(shape, 1)
    assert len(np.unique(slots)) > 40                                   # most slots are on top somewhere


@gpu
def test_same_call_same_bits_and_one_frame_alone(dev):
    shape = (3, 4, 0, 4, 64, 33, 64)
    for kind in (U8, I64, F32):
        _, a, _ = _draw(dev, shape, kind, 0)
        _, b, _ = _draw(dev, shape, kind, 0)
        assert torch.equal(a, b)
        for t in (0, 2, 3):                                             # frames = (t, 1) of the same clip, read in place
            buf, one, _ = _draw(dev, (3, 4, t, 1, 64, 33, 64), kind, 0)
            assert torch.equal(one[:, 0], a[:, t]) and _intact(buf, kind)


@gpu
def test_engine_rasterize(dev):
    from vlg.engine import LayoutEngine
    from vlg.spec import LayoutConfig
    eng = LayoutEngine(LayoutConfig(B=2, T=4, N=8, d=64, n_layers=1), dev, seed=3)
    shape = (2, 3, 0, 3, 5, 7, 48)
    cls, box, valid = _on(dev, _case(2, 3, 5, 7, 48))
    full = eng.rasterize(cls, box, (7, 48), valid=valid)
    assert full.dtype == torch.int64 and tuple(full.shape) == (2, 3, 7, 48)
    assert np.array_equal(full.cpu().numpy(), _ref(shape, 0))
    part = eng.rasterize(cls, box, (7, 48), valid=valid, frames=(1, 2), dtype=torch.float32)
    assert part.dtype == torch.float32 and torch.equal(part, full[:, 1:].float())
    slots = eng.rasterize(cls, box, (7, 48), valid=valid, what="slot", dtype=torch.uint8)
    assert np.array_equal(slots.cpu().numpy().astype(np.int64), _ref(shape, 1))            # background None -> N = 5
    out = torch.empty(2, 3, 7, 48, dtype=torch.uint8, device=dev)
    assert eng.rasterize(cls, box, (7, 48), dtype=torch.uint8, background=9, out=out) is out
    assert np.array_equal(out.cpu().numpy().astype(np.int64), _ref(shape, 0, False, 9))
    for bad in (dict(size=(7, 40)), dict(size=(7, 48), what="area"), dict(size=(7, 48), dtype=torch.int32), dict(size=(7, 48), frames=(2, 2)),
                dict(size=(7, 48), background=256), dict(size=(7, 48), out=out), dict(size=(7, 48), valid=valid[:, :2])):
        with pytest.raises(ValueError):
            eng.rasterize(cls, box, **bad)
    with pytest.raises(ValueError):
        eng.rasterize(cls.cpu(), box.cpu(), (7, 48))
    rec = eng.pixel_record(3)
    assert rec.counts.is_cuda and tuple(rec.counts.shape) == (3, 21 * 21 + 1) and not bool(rec.counts.any())


@gpu
def test_refusals_leave_the_output_untouched(dev):
    from vlg import hip
    f = hip.load().vlg_layout_rasterize
    shape = (2, 3, 1, 2, 5, 7, 48)
    d = _on(dev, _case(2, 3, 5, 7, 48))
    big = _on(dev, _case(1, 1, 300, 40, 16))
    for kind in (U8, I64, F32):
        buf, out = _out(dev, kind, (2, 2, 7, 48))
        esz = out.element_size()
        shape_bad = [dict(B=0), dict(T=0), dict(N=0), dict(H=0), dict(t0=-1), dict(t0=2), dict(T_buf=2), dict(N=1025), dict(n_classes=0),
                     dict(n_classes=256), dict(W=0), dict(W=8), dict(W=40), dict(W=16400), dict(H=16385), dict(background=-1),
                     dict(background=256), dict(out_kind=3), dict(out_kind=-1), dict(what=2), dict(what=-1), dict(cls=0), dict(box=0),
                     dict(labels=0),
                     # labels overlapping an input: the output range starts inside the boxes / ends inside the classes / is valid itself
                     dict(box=out.data_ptr() + 16 * esz), dict(cls=out.data_ptr() + out.numel() * esz - 8), dict(valid=out.data_ptr())]
        align_bad = [dict(box=d[1].data_ptr() + 4), dict(box=d[1].data_ptr() + 8), dict(labels=out.data_ptr() + 8),
                     dict(labels=out.data_ptr() + 1) if kind == U8 else dict(labels=out.data_ptr() + 4), dict(cls=d[0].data_ptr() + 4),
                     dict(valid=d[2].data_ptr() + 2)]
        for want, overs in ((ERR_SHAPE, shape_bad), (ERR_ALIGN, align_bad)):
            for over in overs:
                assert f(*_args(d, out, shape, kind, 0, C, **over)) == want, (kind, over)
        if kind == U8:                                                   # slot indices of 300 slots do not fit a byte; classes do
            assert f(*_args(big, out, (1, 1, 0, 1, 300, 7, 48), kind, 1, 255)) == ERR_SHAPE
        torch.cuda.synchronize()
        assert _intact(buf, kind, inner=True), kind
        assert f(*_args(d, out, shape, kind, 0, C)) == 0                 # the same buffers are accepted as they are
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().astype(np.int64), _ref(shape, 0)) and _intact(buf, kind)
