"""The launch-by-launch checker of the pixel step (image_trace.check) on a synthetic trace: the stage functions of
image_stages.py chained in float32 under the bf16 contract, in the record format image_trace.trace writes on the GPU.  The clean
trace passes; each mutation below - one launch done wrong, everything after it computed from what that launch left behind - fails,
and the checker names the mutated stage.  This is the evidence that the per-launch bars discriminate; no GPU is needed.

Shape: CoordGridNet, b=2, 32x40, filters (8,16,24) - the second case of tests/test_hip_image_step_trace.py.

Tried, and NOT caught at this shape (therefore not in the list): a bias gradient summed over the halo rows as well.  The halo rows
of every dOut are exactly 0.0 - an invariant the checker asserts at the launch that wrote that dOut - so the longer sum adds
nothing and the result is the same bit for bit.  What the invariant does catch is the other end of that defect, a launch that
leaves something in a halo row (the upsample and the bias-on-halo mutations of the list)."""
import copy
import re

import pytest
import torch

import image_stages as IS
import image_trace
import test_hip_conv_bf16 as CB
from oracle import gridnet_spec as GS
from oracle import image_step_spec as STEP

F32, F64 = torch.float32, torch.float64
ARCH, FILTERS, SHAPE = "CoordGridNet", (8, 16, 24), (2, 32, 40)


def synthetic_frames(n, H, W, seed=1024):
    """vlg.image_engine.synthetic_frames' distributions (frames and edges U[0,1), seg ids U{0..19})"""
    g = torch.Generator().manual_seed(seed)
    out = {k: torch.rand(n, 3, H, W, generator=g) for k in ("frame1", "frame2", "frame3")}
    for k in ("seg1", "seg2"):
        out[k] = torch.randint(0, 20, (n, 1, H, W), generator=g).float()
    out["seg3"] = torch.randint(0, 20, (n, H, W), generator=g)
    for k in ("e1", "e2"):
        out[k] = torch.rand(n, 1, H, W, generator=g)
    return out


@pytest.fixture(scope="module")
def setup():
    params = GS.test_params(GS.param_shapes(filters=FILTERS, coord=True), linear=False)
    return IS.Shape(*SHAPE), params, synthetic_frames(*SHAPE, seed=5)


@pytest.fixture(scope="module")
def contracts():
    return {p: IS.Contract(ARCH, FILTERS, precision=p) for p in ("fp32", "bf16")}


def test_clean_synthetic_trace_passes(setup, contracts):
    sh, params, batch = setup
    for prec, c in contracts.items():
        records, state = IS.emulate(c, sh, params, batch, F32, flip=1)
        assert len(records) == len(c.schedule)
        log = []
        image_trace.check(records, state, c, batch, log=log)
        logged = {stage for stage, *_ in log}                # the bitwise kinds log nothing; every kind compared by value must
        valued = [e["stage"] for e in c.schedule if e["kind"] in ("conv_fwd", "conv_dgrad", "conv_wgrad", "up_fwd", "up_bwd", "loss")]
        assert len(valued) == len(set(valued)) > 150 and set(valued) <= logged
        assert all(r["name"].endswith("_bf16") == (prec == "bf16") for r in records if "conv3x3" in r["name"])
        assert not any(r["name"].endswith("_bf16") for r in records if "conv3x3" not in r["name"])


def test_clean_synthetic_trace_with_the_frozen_trunks_passes():
    """HED edges and the VGG term (the third GPU case's schedule) at the smallest shape HED takes, both precisions"""
    from oracle import hned_spec, vgg_spec
    sh, batch = IS.Shape(1, 16, 16), synthetic_frames(1, 16, 16, seed=2)
    params = GS.test_params(GS.param_shapes(filters=FILTERS, coord=True), linear=False)
    trunks = {"hed": hned_spec.test_params(), "vgg": vgg_spec.test_params()}
    for prec in ("fp32", "bf16"):
        c = IS.Contract(ARCH, FILTERS, True, True, prec)
        records, state = IS.emulate(c, sh, params, {k: v for k, v in batch.items() if k not in ("e1", "e2")}, F32, trunk_params=trunks)
        image_trace.check(records, state, c, batch)
        assert float(state["final"]["grads_ext"][c.n_params_padded + 4]) > 0          # the VGG term's slot


def test_schedule_counts_and_flags():
    """what the graph alone fixes: one forward and one weight-gradient launch per 3x3 weight of the reference, ACCUM exactly on
    the second writer of a gradient tensor, no data gradient into the network input without a PReLU"""
    for arch in ("GridNet", "CoordGridNet"):
        S = IS.schedule(arch, FILTERS, False, False, "fp32")
        n3x3 = sum(1 for k, s in GS.param_shapes(filters=FILTERS, coord=arch == "CoordGridNet").items() if k.endswith(".weight") and len(s) == 4)
        assert sum(e["kind"] == "conv_fwd" for e in S) == n3x3 == sum(e["kind"] == "conv_wgrad" for e in S)
        seen = set()
        for e in S:
            if e["kind"] == "conv_dgrad":
                assert bool(e["flags"] & IS.CEPI_ACCUM) == (e["ops"][2] in seen), e["stage"]
                assert bool(e["flags"] & IS.CEPI_DPRELU) == (e["conv"].slope is not None), e["stage"]
            if e["kind"] in ("conv_dgrad", "up_bwd", "add_rows_padded"):
                seen.add(e["ops"][2] if e["kind"] == "conv_dgrad" else e["ops"][1] if e["kind"] == "up_bwd" else e["ops"][0])
            if e["entry"] == "vlg_nchw_to_padded" and e["ops"][1].startswith("d."):
                seen.add(e["ops"][1])
        into_x = [e for e in S if e["kind"] == "conv_dgrad" and e["ops"][2] == "d.g:x"]
        assert len(into_x) == (0 if arch == "CoordGridNet" else 1)      # GridNet: lateral_in.conv.1, for its PReLU's slope
        assert [e["entry"] for e in S[-2:]] == ["vlg_reduce_slabs_table", "vlg_sum_partials_table"]
    S = IS.schedule("CoordGridNet", (32, 64, 96), True, True, "bf16")
    cin4 = [e["stage"] for e in S if e["kind"] == "conv_fwd" and e["flags"] & IS.CEPI_CIN4]
    assert cin4 == ["(e1) moduleVggOne.0", "(e2) moduleVggOne.0", "(target) features.0", "(output) features.0"]
    assert all(e["entry"].endswith("_bf16") == e["kind"].startswith("conv_") for e in S)


def test_conv_parts_restates_the_kernel_tests_reference():
    """image_stages.conv_parts in pure float64 against test_hip_conv_bf16._ref: the same numbers up to _ref's fp32 activation"""
    g = torch.Generator().manual_seed(3)
    x, w, bias = torch.randn(2, 10, 8, 12, generator=g), torch.randn(6, 10, 3, 3, generator=g) * 0.1, torch.randn(6, generator=g)
    for stride, slope, act, resid in ((1, None, 10, False), (2, 0.3, 10, False), (1, 0.2, 8, True), (1, 0.0, 10, False)):
        r = torch.randn(2, 6, 8 // stride, 12 // stride, generator=g)
        rs = torch.randn(r.shape, generator=g) if resid else None
        for rounded in (False, True):
            a = IS.conv_parts(x, w, bias, slope, act, stride, rs, r, rounded, F64, pure=True)
            b = CB._ref(x, w, bias, slope, act, stride, rs, r, rounded)
            tol = 1e-12 if slope is None else 3e-3 if rounded else 1e-6    # (an fp32 product can cross a bf16 rounding boundary)
            for u, v in zip(a, b):
                if u is not None:
                    u, v = torch.as_tensor(u, dtype=F64), torch.as_tensor(v, dtype=F64)
                    assert float((u - v).abs().max()) <= tol * max(float(v.abs().max()), 1e-3), (stride, slope, rounded)


def test_loss_stage_functions_are_the_c_oracle():
    g = torch.Generator().manual_seed(4)
    a, b = torch.rand(2, 3, 12, 16, generator=g), torch.rand(2, 3, 12, 16, generator=g)
    logits, tgt = torch.randn(2, 20, 12, 16, generator=g), torch.randint(0, 20, (2, 12, 16), generator=g)
    for kind, p, q in (("l1", a, b), ("gd", a, b), ("ssim", a, b), ("ce", logits, tgt)):
        v, gr = IS.image_loss(kind, p, q, 3.0, F64)
        rv, rg = IS.image_loss_c(kind, p, q)
        assert abs(float(v) - rv) <= 1e-6 * abs(rv), kind
        assert float((gr - 3.0 * rg.double()).abs().max()) <= 1e-5 * float(rg.abs().max()) * 3.0, kind


def test_adam_stage_function_is_torch_optim_adam():
    torch.manual_seed(6)
    p0 = torch.randn(100, dtype=F64)
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=2e-4, betas=(0.5, 0.999))
    p, m, v = p0, torch.zeros(100), torch.zeros(100)
    for step in range(1, 4):
        g = torch.randn(100, dtype=F64)
        ref.grad = g.clone()
        opt.step()
        p, m, v = IS.adam_step(p, g, m, v, step, 2e-4, 0.5, 0.999, 1e-8)
        assert torch.allclose(p, ref.detach(), rtol=1e-12, atol=1e-15)


def test_fp64_chain_is_the_oracle(setup, contracts):
    """With no rounding anywhere the float64 chain of stage functions under the schedule is oracle/image_step_spec's autograd
    to fp64 rounding - losses and every parameter gradient, with the PReLU branches fixed to the chain's own pattern: the
    schedule and the stage functions together ARE the step."""
    sh, params, batch = setup
    c = contracts["fp32"]
    for flip in (0, 1):
        _, state = IS.emulate(c, sh, params, batch, F64, flip=flip, pure=True)
        cur = state["final"]
        positive = {conv.slope: conv.x.nchw(cur[conv.x.name], sh, conv.x.C) > 0 for conv in c.convs if conv.slope}
        p64 = {k: v.double() for k, v in params.items()}
        b64 = {k: v.double() if v.is_floating_point() else v for k, v in batch.items()}
        parts, grads = STEP.loss_and_grads(p64, b64, True, flip=bool(flip), branches=GS.Branches(positive=positive))
        g = cur["grads_ext"]
        got = g[c.n_params_padded:c.n_params_padded + 4]
        assert torch.allclose(got, torch.tensor(parts[:4], dtype=F64), rtol=1e-12, atol=0), (got, parts)
        seen = set()
        for conv in c.convs:
            dw, db, _ = IS.conv_params(c, g, conv)
            named = [(conv.key + ".weight", dw), (conv.key + ".bias", db)]
            if conv.slope:
                named.append((conv.slope, g[c.off[conv.sname]].view(1)))
            for n, t in named:
                seen.add(n)
                assert float((t - grads[n]).norm()) <= 1e-12 * max(float(grads[n].norm()), 1e-3), n
        assert seen == set(grads)
        assert not bool((g[:c.n_params_padded][c.padded_lanes()] != 0).any())


# ------------------------------------------------------------------------------------------------ mutations
def _first(c, pred):
    return next(e for e in c.schedule if pred(e))


def _recompute(c, sh, e, cur, **over):
    """the launch's outputs once more, in float32, with a changed entry / convolution / input"""
    e2 = dict(e)
    get = cur.__getitem__
    if "conv" in over:
        e2["conv"] = over["conv"]
    if "flags" in over:
        e2["flags"] = over["flags"]
    if "get" in over:
        get = over["get"]
    return IS.run(e2, c, sh, get, F32, over.get("rounded", c.bf16))


def _no_accum(c, sh, e, cur, out, rec):
    t = e["conv"].x.grad()
    out[t.name] = t.pack(_recompute(c, sh, e, cur, flags=e["flags"] & ~IS.CEPI_ACCUM)["dx"], sh)


def _no_accum_flag_dropped(c, sh, e, cur, out, rec):
    _no_accum(c, sh, e, cur, out, rec)
    rec["flags"] = e["flags"] & ~IS.CEPI_ACCUM


def _neighbour_slope(c, sh, e, cur, out, rec):
    conv = e["conv"]
    other = next(k for k in c.convs if k.slope and k.slope != conv.slope)
    p = cur["g.params"].clone()
    p[c.off[conv.sname]] = p[c.off[other.sname]]
    get = lambda n: p if n == "g.params" else cur[n]
    out[conv.out.name] = conv.out.pack(_recompute(c, sh, e, cur, get=get)["y"], sh, cur[conv.out.name])


def _act_all_lanes(c, sh, e, cur, out, rec):
    conv = copy.copy(e["conv"])
    conv.act = conv.x.cin                                     # the AddCoords lanes go through the PReLU too
    out[conv.out.name] = conv.out.pack(_recompute(c, sh, e, cur, conv=conv)["y"], sh, cur[conv.out.name])


def _other_residual(c, sh, e, cur, out, rec):
    conv = copy.copy(e["conv"])
    block_in = next(k for k in c.convs if k.out is conv.x).x     # the lateral block's own input: same level, same channels
    assert (block_in.level, block_in.C) == (conv.resid.level, conv.resid.C) and block_in is not conv.resid
    conv.resid = block_in
    out[conv.out.name] = conv.out.pack(_recompute(c, sh, e, cur, conv=conv)["y"], sh)


def _other_rounding(c, sh, e, cur, out, rec):
    conv = e["conv"]
    out[conv.out.name] = conv.out.pack(_recompute(c, sh, e, cur, rounded=not c.bf16)["y"], sh, cur[conv.out.name])


def _stride1_window(c, sh, e, cur, out, rec):
    conv = e["conv"]
    w, bias, slope = IS.conv_params(c, cur["g.params"], conv)
    x = conv.x.nchw(cur[conv.x.name], sh)
    y = IS.conv_parts(x, w, bias, slope, conv.act, 1, None, torch.zeros(x.shape[0], conv.cout, x.shape[2], x.shape[3]), c.bf16, F32)[0]
    out[conv.out.name] = conv.out.pack(y[:, :, 1::2, 1::2].contiguous(), sh)      # the window centred one pixel off


def _region_overlap(c, sh, e, cur, out, rec):
    off, n, stride = rec["region"]
    rec["region"] = (off + stride // 2, n, stride)            # runs into the next convolution's region, written earlier


def _halo_after_upsample(c, sh, e, cur, out, rec):
    t = e["dst"]
    buf = out[t.name].clone()
    t.grid(buf, sh)[0, 0, 3, 1] = 0.5
    out[t.name] = buf


def _bias_on_halo(c, sh, e, cur, out, rec):
    conv = e["conv"]
    buf = out[conv.out.name].clone()
    conv.out.grid(buf, sh)[:, 0, :, :conv.cout] = IS.conv_params(c, cur["g.params"], conv)[1]
    out[conv.out.name] = buf


def _padded_wgrad_lane(c, sh, e, cur, out, rec):
    conv = e["conv"]
    buf = out["slab:" + conv.key].clone()
    buf.view(-1, conv.slab_stride)[0, conv.cin] = 1e-3       # row 0, tap 0, the first lane beyond cin
    assert conv.cin < conv.x.cp
    out["slab:" + conv.key] = buf


def _slope_partial_off(c, sh, e, cur, out, rec):
    conv = e["conv"]
    part = out["da:" + conv.key].clone()
    part[1] = 3e-5 * _recompute(c, sh, e, cur)["da_scale"]   # a stray partial worth 3e-5 of sum |terms|
    out["da:" + conv.key] = part


_dgrad_accum = lambda e: e["kind"] == "conv_dgrad" and e["flags"] & IS.CEPI_ACCUM
_fwd = lambda key: (lambda e: e["kind"] == "conv_fwd" and e["conv"].key == key)
MUTATIONS = [
    ("a data gradient without ACCUM on a tensor with two consumers, the flag still claimed", "bf16", _dgrad_accum, _no_accum),
    ("the same with the flag dropped", "bf16", _dgrad_accum, _no_accum_flag_dropped),
    ("the slope of the neighbouring PReLU", "bf16", _fwd("lateral_00.conv.3"), _neighbour_slope),
    ("act_ch = cp on a coord tensor", "bf16", _fwd("lateral_in.conv.2.conv"), _act_all_lanes),
    ("the residual from the other branch", "bf16", _fwd("lateral_10.conv.3"), _other_residual),
    ("a bf16 convolution with unrounded operands", "bf16", _fwd("down_00.conv.3"), _other_rounding),
    ("an fp32 convolution with rounded operands", "fp32", _fwd("down_00.conv.3"), _other_rounding),
    ("a stride-2 forward reading the stride-1 window", "bf16", _fwd("down_10.conv.1"), _stride1_window),
    ("a weight-gradient region overlapping the next convolution's", "bf16",
     lambda e: e["kind"] == "conv_wgrad" and e["conv"].key == "lateral_04.conv.1", _region_overlap),
    ("a nonzero halo row left by an upsample", "bf16", lambda e: e["kind"] == "up_fwd", _halo_after_upsample),
    ("the bias added on a halo row", "bf16", _fwd("lateral_01.conv.1"), _bias_on_halo),
    ("an fp32 slope gradient off by 3e-5 of its scale", "fp32", lambda e: e["kind"] == "conv_dgrad" and e["with_da"], _slope_partial_off),
    ("a nonzero padded weight-gradient lane", "bf16", lambda e: e["kind"] == "conv_wgrad" and e["conv"].key == "up_14.up.2",
     _padded_wgrad_lane),
]


@pytest.mark.parametrize("what,prec,pick,fn", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_mutation_is_caught_at_its_stage(setup, contracts, what, prec, pick, fn):
    sh, params, batch = setup
    c = contracts[prec]
    stage = _first(c, pick)["stage"]
    hit = []

    def mutate(e, cur, out, rec):
        if e["stage"] == stage:
            hit.append(stage)
            fn(c, sh, e, cur, out, rec)

    records, state = IS.emulate(c, sh, params, batch, F32, mutate)
    assert hit == [stage]
    with pytest.raises(AssertionError, match=re.escape("[%s]" % stage)):
        image_trace.check(records, state, c, batch)
