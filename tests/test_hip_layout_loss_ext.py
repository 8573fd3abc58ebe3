"""vlg_layout_loss_ext (csrc/loss.hip) through the C ABI: class weights, label smoothing and the GIoU overlap term, against
tests/loss_ext_ref.py run in float64 on the same fp32 inputs.

Conventions of test_hip_layout_ops.py: every output buffer starts as a NaN sentinel with a guard after it, padding columns
and guards keep their bits, the ticket in scratch is zero again after a launch.  Bars (restated from that file's
_loss_check, with the options' terms in place of the plain ones):
  gradients  helpers.vs_cpu32 per block of columns (class logits, box outputs): 4x torch-CPU fp32's error against fp64
             plus 2^-20 of the largest value;
  values     4x torch-CPU fp32's error plus 64 EPS of the summed magnitudes over the denominator: per token |term| + 1
             for the box terms over the valid count, and for the cross entropy |sum_c q[c] (-log p[c])| + Q (1 + the
             largest |logit|, which log-sum-exp subtracts and adds back) over W - with q, Q of the definition; neutral
             options make that _loss_check's floor.
"""
import functools

import pytest
import torch

import loss_ext_ref as R
from helpers import vs_cpu32
from oracle import layout_spec as O
from test_hip_layout_ops import GUARD, _edge_batch, _guard, _loss_rows, _scratch
from test_hip_pixel_ops import EPS, ERR_ALIGN, ERR_SHAPE, SENT, f32, sentinel, untouched, within

pytestmark = pytest.mark.gpu

GIOU = 1
WEIGHTS = torch.rand(20, generator=torch.Generator().manual_seed(77)) * 3
WEIGHTS[5] = 0.0
# name -> (class weights, label smoothing, flags)
OPTIONS = {"weights": (WEIGHTS, 0.0, 0), "eps": (None, 0.1, 0), "giou": (None, 0.0, GIOU),
           "weights+eps": (WEIGHTS, 0.1, 0), "all": (WEIGHTS, 0.1, GIOU), "none": (None, 0.0, 0)}
LOSS_W = (O.W_REG, O.W_IOU, O.W_CE)


@pytest.fixture(scope="module")
def H():
    from vlg import hip
    hip.load()
    return hip


def S():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(logits, raw, batch, ld, beta) of a named input set; built once, never modified"""
    if name == "edges":                                   # test_layout_loss_edges' batch
        return _edge_batch(3, 4, 12, seed=9) + (24, 0.125)
    if name == "single":                                  # test_layout_loss_single_valid_slot's
        logits, raw, batch = _edge_batch(2, 8, 12, seed=10)
        batch["valid"].zero_()
        batch["valid"][1, 5, 8] = 1.0
        return logits, raw, batch, 24, 0.125
    B, T, N, seed = {"odd": (3, 5, 7, 21), "prod": (5, 32, 821, 5), "tail": (1, 1, 3, 3)}[name]
    batch = O.synthetic_batch(B, T, N, seed=seed, variable_n=name != "tail", min_valid=100 if name == "prod" else 3)
    g = torch.Generator().manual_seed(11 * seed)
    return (torch.randn(B, T, N, 20, generator=g) * 3, torch.randn(B, T, N, 4, generator=g) * 2, batch,
            24 if name == "tail" else 28, O.SMOOTH_L1_BETA)


def run(H, dev, name, weight, eps, flags, scratch=None, entry="vlg_layout_loss_ext", loss_w=LOSS_W, batch=None):
    """One launch on the named inputs (row stride ld, padding columns hold the sentinel); returns the four loss values,
    dout's 24 owned columns and dout's raw bits, after checking that nothing else was written."""
    logits, raw, b0, ld, beta = inputs(name)
    batch = b0 if batch is None else batch
    B, T, N = logits.shape[:3]
    M = B * T * N
    scratch = _scratch(H, dev) if scratch is None else scratch
    oraw = sentinel(M * ld + GUARD, dev)
    f32(oraw)[:M * ld].view(M, ld)[:, :24] = torch.cat([_loss_rows(logits), _loss_rows(raw)], 1).to(dev)
    draw = sentinel(M * ld + GUARD, dev)
    lraw = sentinel(4 + GUARD, dev)
    tc, tb, va = batch["tgt_class"].to(dev), batch["tgt_box"].to(dev), batch["valid"].to(dev)
    wd = None if weight is None else weight.to(dev)
    head = (f32(oraw).data_ptr(), ld, tc.data_ptr(), tb.data_ptr(), va.data_ptr())
    outs = (f32(draw).data_ptr(), f32(lraw).data_ptr(), f32(scratch).data_ptr(), B, T, N, 20, beta, O.IOU_EPS) + tuple(loss_w)
    if entry == "vlg_layout_loss":
        H.call(entry, *head, *outs, S())
    else:
        H.call(entry, *head, H.ptr(wd), *outs, eps, flags, S())
    torch.cuda.synchronize()
    owned = torch.zeros(M * ld + GUARD, dtype=torch.bool, device=dev)
    owned[:M * ld].view(M, ld)[:, :24] = True
    untouched(draw, owned, "loss dout")
    _guard(lraw, 4, "loss values")
    _guard(scratch, H.load().vlg_layout_loss_scratch(), "loss scratch")
    assert int(scratch[1]) == 0, "the ticket counter was not reset for the next launch"
    return f32(lraw)[:4].cpu(), f32(draw)[:M * ld].view(M, ld)[:, :24].cpu(), draw


def reference(name, weight, eps, flags, loss_w=LOSS_W, batch=None):
    """{dtype: (values (4,), d out (M, 24))} in float64 and float32, and the value floors"""
    logits, raw, b0, _, beta = inputs(name)
    return reference_on(logits, raw, b0 if batch is None else batch, beta, weight, eps, flags, loss_w)


def reference_on(logits, raw, batch, beta, weight, eps, flags, loss_w=LOSS_W):
    """`reference` on given tensors: logits (B,T,N,20), raw (B,T,N,4), batch = {tgt_class, tgt_box, valid} (step_trace.check
    holds the step's loss launch to the same comparison)"""
    ref = {}
    for dt in (torch.float64, torch.float32):
        lg, rw = (t.detach().to(dt, copy=True).requires_grad_(True) for t in (logits, raw))
        parts = R.losses(lg, rw, batch["tgt_class"], batch["tgt_box"].to(dt), batch["valid"].to(dt),
                         None if weight is None else weight.to(dt), eps, "giou" if flags & GIOU else "iou", beta=beta)
        total = loss_w[0] * parts[1] + loss_w[1] * parts[2] + loss_w[2] * parts[3]
        total.backward()
        ref[dt] = (torch.stack([total.detach()] + [t.detach() for t in parts[1:]]),
                   torch.cat([_loss_rows(lg.grad), _loss_rows(rw.grad)], 1))
    # floors of the values (module docstring), in float64
    lg, tb, va = logits.double(), batch["tgt_box"].double(), batch["valid"].double()
    box = torch.sigmoid(raw.double())
    reg = torch.nn.functional.smooth_l1_loss(box, tb, beta=beta, reduction="none").sum(-1) / 4
    ov = 1 - (R.box_giou_cxcywh(box, tb) if flags & GIOU else O.box_iou_cxcywh(box, tb))
    w = torch.ones(20, dtype=torch.float64) if weight is None else weight.double()
    y = batch["tgt_class"].clamp(0, 19)
    q = (eps / 20) * w.expand(lg.shape).clone()
    q.scatter_add_(-1, y.unsqueeze(-1), ((1 - eps) * w[y]).unsqueeze(-1))
    term = (q * -torch.log_softmax(lg, -1)).sum(-1)
    Q = q.sum(-1)
    cnt = float(va.sum().clamp(min=1))
    W = float((va * w[y]).sum())
    fl = [64 * EPS * float(((t.abs() + 1) * va).sum()) / cnt for t in (reg, ov)]
    fl.append(64 * EPS * float(((term.abs() + Q * (1 + lg.abs().amax(-1))) * va).sum()) / W if W > 0 else 0.0)
    floors = torch.tensor([loss_w[0] * fl[0] + loss_w[1] * fl[1] + loss_w[2] * fl[2]] + fl, dtype=torch.float64)
    return ref, floors


@functools.lru_cache(maxsize=None)
def named_reference(name, opt):
    return reference(name, *OPTIONS[opt])


def check(loss, dout, ref, floors, what):
    (v64, g64), (v32, g32) = ref[torch.float64], ref[torch.float32]
    print("%s: values gpu %s fp64 %s cpu32-err %s floors %s" % (
        what, loss.tolist(), v64.tolist(), (v32.double() - v64).abs().tolist(), floors.tolist()))
    for lo, hi, col in ((0, 20, "d logits"), (20, 24, "d box")):
        print("%s %s: max |err| %.3e, cpu32's %.3e, max |fp64| %.3e" % (
            what, col, float((dout[:, lo:hi].double() - g64[:, lo:hi]).abs().max()),
            float((g32[:, lo:hi].double() - g64[:, lo:hi]).abs().max()), float(g64[:, lo:hi].abs().max())))
        vs_cpu32(dout[:, lo:hi], g64[:, lo:hi], g32[:, lo:hi], "%s: loss %s" % (what, col))
    within(loss, v64, 4 * (v32.double() - v64).abs() + floors, "%s: loss values (total, smooth-L1, overlap, CE)" % what)


@pytest.mark.parametrize("name", ["edges", "odd"])
@pytest.mark.parametrize("opt", ["weights", "eps", "giou", "weights+eps", "all"])
def test_options_match_fp64(H, dev, opt, name):
    """Each option set on the edge batch of test_layout_loss_edges ((3,4,12), beta = 0.125: logits at +-80 and all equal,
    saturated sigmoid, tied, touching and disjoint boxes) and on (3,5,7) with ld = 28 and variable-N validity (M = 105);
    the weights hold a zero entry."""
    loss, dout, _ = run(H, dev, name, *OPTIONS[opt])
    check(loss, dout, *named_reference(name, opt), "%s/%s" % (name, opt))


def test_multipass_grid_all_options(H, dev):
    """M = 131 360 tokens: above 1024 blocks x 128 tokens, so two blocks make a second pass (where a per-block W or a
    pass-local row index would go wrong), and the W loop runs its 8-deep body and its 16-byte remainder (the (3,5,7) case
    ends it on a single token); a second launch on the same scratch gives the same bits."""
    sc = _scratch(H, dev)
    loss, dout, bits = run(H, dev, "prod", *OPTIONS["all"], scratch=sc)
    loss2, _, bits2 = run(H, dev, "prod", *OPTIONS["all"], scratch=sc)
    assert torch.equal(bits, bits2) and torch.equal(loss.view(torch.int32), loss2.view(torch.int32)), \
        "a second launch on the same scratch differs"
    check(loss, dout, *named_reference("prod", "all"), "prod/all")


@pytest.mark.parametrize("name", ["edges", "tail"])
def test_neutral_options_give_the_plain_entry_bits(H, dev, name):
    """class_weight = NULL, label_smoothing = 0, flags = 0: dout and loss_out bit for bit those of vlg_layout_loss, at
    (3,4,12) and at (1,1,3) (M = 3: the count loop is its scalar tail alone)."""
    loss, _, bits = run(H, dev, name, *OPTIONS["none"])
    loss0, _, bits0 = run(H, dev, name, None, 0.0, 0, entry="vlg_layout_loss")
    assert torch.equal(bits, bits0), "dout differs from the plain entry's"
    assert torch.equal(loss.view(torch.int32), loss0.view(torch.int32)), "loss_out differs from the plain entry's"


def test_zero_total_weight(H, dev):
    """W == 0 with eps = 0.1: the slots whose target class is below 10 are the valid ones and exactly those classes have
    weight 0 (the others keep 1, so the smoothing sum is not 0 and torch gives inf or NaN).  CE exactly 0, every logit
    gradient exactly 0, the box gradients those of the plain entry bit for bit."""
    batch = dict(inputs("edges")[2])
    batch["valid"] = (batch["tgt_class"] < 10).float()
    assert 0 < int(batch["valid"].sum()) < batch["valid"].numel()
    w = torch.ones(20)
    w[:10] = 0.0
    loss, dout, _ = run(H, dev, "edges", w, 0.1, 0, batch=batch)
    loss0, dout0, _ = run(H, dev, "edges", None, 0.0, 0, entry="vlg_layout_loss", batch=batch)
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dout).all())
    assert float(loss[3]) == 0.0, "CE with W == 0 is %r" % float(loss[3])
    assert bool((dout[:, :20] == 0).all()), "a logit gradient with W == 0"
    assert torch.equal(dout[:, 20:].view(torch.int32), dout0[:, 20:].view(torch.int32)), "box gradients changed"
    assert torch.equal(loss[1:3].view(torch.int32), loss0[1:3].view(torch.int32)), "box terms changed"
    want = O.W_REG * loss0[1].double() + O.W_IOU * loss0[2].double()
    within(loss[:1], want.reshape(1), 4 * EPS * want.abs(), "total = the box terms")


def test_out_of_range_classes_are_clamped(H, dev):
    """Target classes outside [0, 19] count as 0 or 19 - in the W loop as in the per-token part, also where only the high
    half of the int64 says so (2^32 + 3 is 19, not 3; -2^40 + 5 is 0, not 5)."""
    batch = dict(inputs("odd")[2])
    tc = batch["tgt_class"].clone()
    flat = tc.view(-1)
    odd = torch.tensor([-1, 25, 2 ** 32 + 3, -2 ** 40 + 5, 2 ** 63 - 1, -2 ** 63, 20, 2 ** 31], dtype=torch.int64)
    flat[:odd.numel()] = odd                              # (slots 0..6 of clip 0, frame 0 and one more: valid ones)
    batch["tgt_class"] = tc
    assert float(batch["valid"].view(-1)[:odd.numel()].sum()) >= 3
    loss, dout, _ = run(H, dev, "odd", *OPTIONS["all"], batch=batch)
    check(loss, dout, *reference("odd", *OPTIONS["all"], batch=batch), "odd/all, classes out of range")


def test_single_valid_slot(H, dev):
    """One valid slot, every option on: each masked row of dout exactly 0, the values that slot's terms."""
    loss, dout, _ = run(H, dev, "single", *OPTIONS["all"])
    ref, floors = named_reference("single", "all")
    check(loss, dout, ref, floors, "single/all")
    live = torch.zeros(2, 8, 12, 1, dtype=torch.bool)
    live[1, 5, 8] = True
    assert bool((dout[~_loss_rows(live)[:, 0]] == 0).all()), "a masked slot has a gradient"
    logits, raw, batch, _, beta = inputs("single")
    one = R.losses(logits[1:2, 5:6, 8:9].double(), raw[1:2, 5:6, 8:9].double(), batch["tgt_class"][1:2, 5:6, 8:9],
                   batch["tgt_box"][1:2, 5:6, 8:9].double(), torch.ones(1, 1, 1, dtype=torch.float64), WEIGHTS.double(), 0.1,
                   "giou", beta=beta)
    within(loss, torch.stack(one), 4 * (ref[torch.float32][0].double() - ref[torch.float64][0]).abs() + floors,
           "the values are the one slot's terms")


def test_giou_teaches_disjoint_boxes(H, dev):
    """The rows of the edge batch whose prediction ([0.25, 0.75]^2) does not touch its target: with the overlap term alone
    (w_reg = w_ce = 0) the iou entry's box gradient is exactly 0 there, the giou entry's is not and matches fp64."""
    only = (0.0, O.W_IOU, 0.0)
    rows = torch.zeros(3, 4, 12, 1, dtype=torch.bool)
    rows[:, :, 6] = True
    rows = _loss_rows(rows)[:, 0]
    _, d_iou, _ = run(H, dev, "edges", None, 0.0, 0, entry="vlg_layout_loss", loss_w=only)
    _, d_giou, _ = run(H, dev, "edges", None, 0.0, GIOU, loss_w=only)
    assert bool((d_iou[rows, 20:] == 0).all()), "1 - IoU has a gradient for disjoint boxes"
    ref, _ = reference("edges", None, 0.0, GIOU, loss_w=only)
    g64, g32 = ref[torch.float64][1], ref[torch.float32][1]
    assert bool((g64[rows, 20:].abs().amax(1) > 0).all()), "the reference has no gradient either"
    assert bool((d_giou[rows, 20:].abs().amax(1) > 0).all()), "1 - GIoU has no gradient for disjoint boxes"
    vs_cpu32(d_giou[rows, 20:], g64[rows, 20:], g32[rows, 20:], "giou d box on the disjoint rows")
    vs_cpu32(d_giou[:, 20:], g64[:, 20:], g32[:, 20:], "giou d box")


@pytest.mark.parametrize("case", ["eps=1", "eps<0", "eps=nan", "flag", "classes", "align"])
def test_refusals_enqueue_nothing(H, dev, case):
    """label_smoothing = 1.0, -0.1 or NaN, an unknown flag bit, n_classes = 19, a misaligned `out`: the error code, and
    dout, loss_out and scratch keep every bit."""
    B, T, N, ld = 2, 2, 3, 24
    M = B * T * N
    oraw, draw, lraw = sentinel(M * ld + GUARD, dev), sentinel(M * ld + GUARD, dev), sentinel(4 + GUARD, dev)
    f32(oraw)[:M * ld] = 0.0
    scratch = _scratch(H, dev)
    before = scratch.clone()
    batch = O.synthetic_batch(B, T, N, seed=1)
    tc, tb, va = batch["tgt_class"].to(dev), batch["tgt_box"].to(dev), batch["valid"].to(dev)
    eps = {"eps=1": 1.0, "eps<0": -0.1, "eps=nan": float("nan")}.get(case, 0.1)
    flags = 2 if case == "flag" else GIOU
    code = H.load().vlg_layout_loss_ext(
        f32(oraw).data_ptr() + (4 if case == "align" else 0), ld, tc.data_ptr(), tb.data_ptr(), va.data_ptr(),
        WEIGHTS.to(dev).data_ptr(), f32(draw).data_ptr(), f32(lraw).data_ptr(), f32(scratch).data_ptr(), B, T, N,
        19 if case == "classes" else 20, O.SMOOTH_L1_BETA, O.IOU_EPS, O.W_REG, O.W_IOU, O.W_CE, eps, flags, S())
    torch.cuda.synchronize()
    assert code == (ERR_ALIGN if case == "align" else ERR_SHAPE), code
    assert bool((draw == SENT).all()) and bool((lraw == SENT).all()), "a refused call wrote an output"
    assert torch.equal(scratch, before), "a refused call touched the scratch"
