"""vlg_layout_box_nll (csrc/box_nll.hip) through the C ABI, against tests/boxhead_ref.py in float64 on the same fp32 inputs.

Conventions of test_hip_layout_loss_ext.py: every output buffer starts as a NaN sentinel with a guard after it, what the
launch does not own keeps its bits, the ticket in scratch is zero again after a launch.  Bars: boxhead_ref.check_nll -
the gradient relative to the conditioning of 1 - e^2 (e^2 reaches ~10^6 at sigma = e^-7), not absolute."""
import functools

import pytest
import torch

import boxhead_ref as R
from test_hip_pixel_ops import ERR_ALIGN, ERR_SHAPE, SENT, f32, sentinel, untouched

pytestmark = pytest.mark.gpu

C, GUARD = 20, 64
NAN = float("nan")
SMALL = (3, 4, 23)                  # 276 tokens: no multiple of any block tile
# more tokens than one grid pass covers (128 blocks x 256 threads = 32 768): the grid-stride loop and the 128-block fold
LARGE = (5, 8, 1000)                # 40 000 tokens


@pytest.fixture(scope="module")
def H():
    from vlg import hip
    hip.load()
    return hip


def S():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def inputs(shape, valid_kind):
    """(raw (M, 8) = raw mean | raw scale, tgt_box (B,T,N,4), valid (B,T,N)); built once, never modified.  Raw values scaled so
    that g = sigmoid(raw scale) reaches both ends (sigma = e^-7 and 1) and the mean both ends of [0, 1]."""
    B, T, N = shape
    M = B * T * N
    g = torch.Generator().manual_seed(31 + M)
    raw = torch.randn(M, 8, generator=g) * torch.tensor([3.0] * 4 + [8.0] * 4)
    raw[::7, 4:] = 40.0                                   # g = 1 to the last bit: sigma = 1, g (1 - g) = e^-40
    raw[3::7, 4:] = -40.0                                 # g = 0: sigma = e^-7
    tgt = torch.rand(B, T, N, 4, generator=g)
    valid = {"mixed": (torch.rand(B, T, N, generator=g) > 0.35).float(), "ones": torch.ones(B, T, N),
             "zeros": torch.zeros(B, T, N)}[valid_kind]
    return raw, tgt, valid


def scratch_of(H, dev):
    n = H.load().vlg_layout_box_nll_scratch()
    s = sentinel(n + GUARD, dev)
    s[:n] = 0
    return s


def launch(H, dev, shape, valid_kind, ld, w_nll=1.0, scratch=None, total0=3.25, fill=NAN, s_min=R.S_MIN, s_max=R.S_MAX,
           expect=0, **over):
    """One launch: out rows hold `fill` outside columns [C, C+8), dout and loss_io start as the sentinel (loss_io[0] =
    total0, what the loss launch would have left).  Returns (loss_io (8,), dout's columns [C+4, C+12), raw bits of dout,
    loss_io and scratch) after checking that nothing outside the owned region was written."""
    B, T, N = shape
    M = B * T * N
    raw, tgt, valid = inputs(shape, valid_kind)
    scratch = scratch_of(H, dev) if scratch is None else scratch
    oraw = sentinel(M * ld + GUARD, dev)
    out = f32(oraw)[:M * ld].view(M, ld)
    out[:] = fill
    out[:, C:C + 8] = raw.to(dev)
    draw = sentinel(M * ld + GUARD, dev)
    lraw = sentinel(8 + GUARD, dev)
    f32(lraw)[0] = total0
    tb, va = tgt.to(dev), valid.to(dev)
    args = dict(out=out.data_ptr(), ld=ld, tgt_box=tb.data_ptr(), valid=va.data_ptr(), dout=f32(draw).data_ptr(),
                loss_io=f32(lraw).data_ptr(), scratch=f32(scratch).data_ptr(), B=B, T=T, N=N, C=C, s_min=s_min, s_max=s_max,
                w_nll=w_nll, stream=S())
    for key in ("ld", "scratch"):                          # call_ld / call_scratch: what the CALL names (the buffers keep theirs)
        if "call_" + key in over:
            args[key] = over.pop("call_" + key)
    args.update(over)
    before = (draw.clone(), lraw.clone(), scratch.clone())
    code = H.load().vlg_layout_box_nll(*args.values())
    torch.cuda.synchronize()
    assert code == expect, "vlg_layout_box_nll returned %d, expected %d" % (code, expect)
    if expect != 0:                                        # a refusal enqueues nothing: every bit stays
        assert torch.equal(draw, before[0]) and torch.equal(lraw, before[1]) and torch.equal(scratch, before[2])
        return None
    owned = torch.zeros(M * ld + GUARD, dtype=torch.bool, device=dev)
    owned[:M * ld].view(M, ld)[:, C + 4:C + 12] = True
    untouched(draw, owned, "box_nll dout")                 # [0, C+4), the columns past C+12 and the guard keep the sentinel
    assert bool((lraw[8:] == SENT).all()), "box_nll wrote past loss_io's 8 floats"
    assert torch.equal(lraw[1:4], before[1][1:4]), "box_nll touched loss_io[1..3]"
    n = H.load().vlg_layout_box_nll_scratch()
    assert bool((scratch[n:] == SENT).all()), "box_nll wrote past its scratch"
    assert int(scratch[1]) == 0, "the ticket counter was not reset for the next launch"
    return f32(lraw)[:8].cpu(), f32(draw)[:M * ld].view(M, ld)[:, C + 4:C + 12].cpu(), draw, lraw


def reference(shape, valid_kind, w_nll=1.0, s_min=R.S_MIN, s_max=R.S_MAX):
    B, T, N = shape
    raw, tgt, valid = inputs(shape, valid_kind)
    out = torch.zeros(B * T * N, 32, dtype=torch.float64)
    out[:, C:C + 8] = raw.double()
    return R.box_nll_closed(out, tgt, valid, B, T, N, C, w_nll, s_min, s_max)


@pytest.mark.parametrize("ld", [32, 36])
@pytest.mark.parametrize("valid_kind", ["mixed", "ones", "zeros"])
def test_box_nll_matches_fp64(H, dev, ld, valid_kind):
    w_nll, total0 = 0.75, 3.25
    loss, dcols, _, _ = launch(H, dev, SMALL, valid_kind, ld, w_nll=w_nll, total0=total0)
    ref = reference(SMALL, valid_kind, w_nll)
    assert bool((dcols[:, 4:] == 0).all()), "the padding columns' gradient is not exactly 0"
    R.check_nll(dcols[:, :4], loss[4], loss[5], ref, "ld=%d valid=%s" % (ld, valid_kind))
    assert float(loss[6]) == 0.0 and float(loss[7]) == 0.0
    # loss_io[0] = its previous value + w_nll * box_nll, in fp32 from the launch's own box_nll
    want0 = torch.tensor(total0) + torch.tensor(w_nll) * loss[4]
    assert abs(float(loss[0]) - float(want0)) <= 2.0 ** -23 * abs(float(want0)), (float(loss[0]), float(want0))
    if valid_kind == "zeros":                              # cnt clamps to 1 and every output is exactly 0
        assert bool((dcols == 0).all()) and float(loss[4]) == 0.0 and float(loss[5]) == 0.0 and float(loss[0]) == total0
    else:
        assert float(ref["cover"]) > 0.05 and bool((ref["dscale"] != 0).any())


def test_box_nll_reads_only_its_columns_and_repeats_bit_for_bit(H, dev):
    """NaN in the logits and in every column from C+8 on changes nothing; a second launch on the same inputs and the same
    scratch gives the same bits"""
    scratch = scratch_of(H, dev)
    a = launch(H, dev, SMALL, "mixed", 36, scratch=scratch, fill=NAN)
    b = launch(H, dev, SMALL, "mixed", 36, scratch=scratch, fill=0.5)
    c = launch(H, dev, SMALL, "mixed", 36, scratch=scratch, fill=NAN)
    for other in (b, c):
        assert torch.equal(a[2], other[2]) and torch.equal(a[3], other[3])
    assert bool(torch.isfinite(a[0][[0, 4, 5, 6, 7]]).all()) and bool(torch.isfinite(a[1]).all())      # ([1..3] keep the sentinel)


def test_box_nll_grid_stride_and_multi_block_fold(H, dev):
    scratch = scratch_of(H, dev)
    loss, dcols, draw, lraw = launch(H, dev, LARGE, "mixed", 32, w_nll=1.0, scratch=scratch)
    R.check_nll(dcols[:, :4], loss[4], loss[5], reference(LARGE, "mixed"), "40 000 tokens")
    assert bool((dcols[:, 4:] == 0).all())
    again = launch(H, dev, LARGE, "mixed", 32, w_nll=1.0, scratch=scratch)
    assert torch.equal(draw, again[2]) and torch.equal(lraw, again[3]), "two launches differ"


def test_box_nll_other_bounds_and_zero_weight(H, dev):
    loss, dcols, _, _ = launch(H, dev, SMALL, "mixed", 32, w_nll=0.0, total0=1.5)
    assert bool((dcols == 0).all()) and float(loss[0]) == 1.5 and float(loss[4]) > 0
    loss, dcols, _, _ = launch(H, dev, SMALL, "ones", 32, w_nll=2.0, s_min=-3.0, s_max=-1.0)
    R.check_nll(dcols[:, :4], loss[4], loss[5], reference(SMALL, "ones", 2.0, -3.0, -1.0), "s in [-3, -1]")


def test_box_nll_refusals_write_nothing(H, dev):
    inf = float("inf")
    for over in (dict(C=19), dict(C=21), dict(B=0), dict(T=0), dict(N=0), dict(call_ld=28), dict(call_ld=31), dict(call_ld=34),
                 dict(s_min=0.0, s_max=0.0), dict(s_min=1.0, s_max=-1.0), dict(s_min=NAN), dict(s_max=NAN), dict(s_min=-inf),
                 dict(w_nll=-1.0), dict(w_nll=NAN), dict(w_nll=inf)):
        launch(H, dev, SMALL, "mixed", 36, expect=ERR_SHAPE, **over)
    probe = torch.zeros(64, device=dev)
    for name in ("out", "dout", "tgt_box", "valid", "call_scratch"):
        launch(H, dev, SMALL, "mixed", 36, expect=ERR_ALIGN, **{name: probe.data_ptr() + 4})
        launch(H, dev, SMALL, "mixed", 36, expect=ERR_ALIGN, **{name: 0})
    launch(H, dev, SMALL, "mixed", 36, expect=ERR_ALIGN, loss_io=0)
