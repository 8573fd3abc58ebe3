"""The launch-by-launch checker (step_trace.check) on a synthetic trace: the stage functions of step_stages.py chained in
float32 under the "bf16" storage contract ("Layout step: storage contract of the reduced-precision
modes"), in the record format step_trace.trace writes on the GPU.  The clean trace passes; each mutation below - one
launch of the chain done wrong, everything after it computed from what that launch left behind - fails, and the checker
names the mutated stage.  This is the evidence that the per-launch bars discriminate; no GPU is needed.  The last three
mutations each drop one rounding point of the contract.

Shape: B=2, T=4, N=8 (one 32-token tile per clip), d=64, two layers, per-clip attention with padded-slot masks; clip 0
has three padded slots, clip 1 none (so the last token row carries a gradient).

Tried, and NOT caught numerically at this shape (therefore not in the list): the fp32 master weight handed to a
projection in place of its bf16 shadow.  The bf16 kernels round an fp32 operand on its way to the matrix cores, and
round-to-nearest-even of the master IS the shadow, so the product is the same bit for bit; what differs is the operand's
name and the B_BF16 storage bit, and that is how the mutation below is caught (by the contract, not by a bar)."""
import re

import pytest
import torch

import step_stages as SS
import step_trace
from oracle import layout_spec as O


def _setup():
    from vlg.spec import LayoutConfig, param_shapes
    cfg = LayoutConfig(B=2, T=4, N=8, d=64, n_layers=2, attention="clip")
    batch = O.synthetic_batch(cfg.B, cfg.T, cfg.N, seed=3)
    batch["valid"][0, :, 5:] = 0.0
    batch["slot_class"][0, :, 5:] = cfg.n_classes
    return cfg, SS.Contract("bf16", "clip", masked=True), O.init_params(param_shapes(cfg), seed=1024), batch


@pytest.fixture(scope="module")
def setup():
    return _setup()


def test_clean_synthetic_trace_passes(setup):
    cfg, c, params, batch = setup
    records, state = SS.emulate(cfg, c, params, batch, torch.float32)
    assert len(records) == len(SS.schedule(cfg, c)) and set(state["grads"]) == set(params)
    log = []
    step_trace.check(records, state, cfg, c, batch, log=log)
    assert len(log) > len(records)                       # every output and every parameter gradient was compared


def test_fp64_chain_is_the_oracle_when_nothing_rounds(setup):
    """With no rounding anywhere (the fp32 contract) the float64 chain is oracle.layout_spec's autograd, to fp64 rounding:
    the stage functions and the schedule together ARE the step."""
    cfg, _, params, batch = setup
    p64 = {k: v.double() for k, v in params.items()}
    b64 = {k: v.double() if v.is_floating_point() else v for k, v in batch.items()}
    parts, grads = O.loss_and_grads(p64, b64, cfg.n_layers, attention="clip")
    loss, g = SS.emulated_oracle(cfg, "fp32", params, batch, "clip")
    assert torch.allclose(loss, torch.tensor(parts, dtype=torch.float64), rtol=1e-12, atol=0)
    for n, w in grads.items():
        assert float((g[n] - w).norm()) <= 1e-12 * max(float(w.norm()), 1e-3), n


def _stale_h1(e, val, o, g, rec):
    o["qkv[1]"] = SS.linear_fwd(val("h1[0]"), val("pb:l1.qkv_w"), val("p:l1.qkv_b"), SS.bf)[0]


def _master_weight(e, val, o, g, rec):
    rec["ops"] = tuple("p:l0.qkv_w" if n == "pb:l0.qkv_w" else n for n in rec["ops"])
    rec["flags"] &= ~SS.EPI_B_BF16


def _no_bias(e, val, o, g, rec):
    o["xmid[0]"] = SS.linear_fwd(val("att[0]"), val("pb:l0.proj_w"), torch.zeros(64), SS.bf, resid=val("x[0]"))[0]


def _no_residual(e, val, o, g, rec):
    o["x[2]"] = SS.linear_fwd(val("gl[1]"), val("pb:l1.ff2_w"), val("p:l1.ff2_b"), SS.bf)[0]


def _gelu_grad_of_gl(e, val, o, g, rec):
    o["du"] = SS.linear_dgrad(val("dx"), val("pb:l1.ff2_w"), SS.bf, val("gl[1]"), "dgelu")


def _du_unrounded(e, val, o, g, rec):
    o["du"] = SS.Raw(o["du"])


def _mask_ignored(e, val, o, g, rec):
    cfg, c, params, batch = _setup()
    valid = batch["valid"].clone()
    valid[0, :, 6] = 1.0                                  # one padded slot attended to
    o["att[0]"], o["lse[0]"] = SS.clip_attention_fwd(val("qkv[0]"), valid, 2, 4, 8, SS.bf)


def _ln_bwd_overwrites(e, val, o, g, rec):
    o["dx"] = SS.ln_bwd(val("dh"), val("xmid[1]"), val("stats[3].mean"), val("stats[3].rstd"), val("p:l1.ln2_g"))[0]


def _bias_grad_short(e, val, o, g, rec):
    g["l0.qkv_b"] = val("dqkv")[:-1].sum(0)


def _clip_bwd_unrounded(e, val, o, g, rec):
    valid = _setup()[3]["valid"]
    o["dqkv"], o["delta"] = SS.clip_attention_bwd(val("qkv[1]"), val("dh"), val("att[1]"), val("lse[1]"), valid, 2, 4, 8)


def _clip_fwd_unrounded(e, val, o, g, rec):
    o["att[0]"], o["lse[0]"] = SS.clip_attention_fwd(val("qkv[0]"), _setup()[3]["valid"], 2, 4, 8)


def _qkv_unrounded(e, val, o, g, rec):
    o["qkv[0]"] = SS.linear_fwd(val("h1[0]"), val("p:l0.qkv_w"), val("p:l0.qkv_b"))[0]


MUTATIONS = [
    ("a projection fed the previous layer's h1", "l1.qkv", _stale_h1),
    ("the master weight in place of the bf16 shadow", "l0.qkv", _master_weight),
    ("a dropped bias", "l0.proj", _no_bias),
    ("a dropped residual", "l1.ff2", _no_residual),
    ("gelu' of the stored gelu output instead of the saved tensor", "l1.ff2 dgrad+wgrad", _gelu_grad_of_gl),
    ("du left unrounded", "l1.ff2 dgrad+wgrad", _du_unrounded),
    ("the key mask ignored for one padded slot", "l0.attention", _mask_ignored),
    ("the layer-norm backward not accumulating into dx", "l1.ln2 bwd", _ln_bwd_overwrites),
    ("a bias gradient missing its last token row", "l0.qkv dgrad+wgrad", _bias_grad_short),
    # missing rounding points; the two on-chip ones show that step_stages.flip_step's slack does not hide them
    ("the qkv weight read unrounded", "l0.qkv", _qkv_unrounded),
    ("P unrounded in the per-clip attention forward", "l0.attention", _clip_fwd_unrounded),
    ("P and dS unrounded in the per-clip attention backward", "l1.attention bwd", _clip_bwd_unrounded),
]


@pytest.mark.parametrize("what,stage,fn", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_mutation_is_caught_at_its_stage(setup, what, stage, fn):
    cfg, c, params, batch = setup
    hit = []

    def mutate(e, val, o, g, rec):
        if e["stage"] == stage:
            hit.append(stage)
            fn(e, val, o, g, rec)

    records, state = SS.emulate(cfg, c, params, batch, torch.float32, mutate)
    assert hit == [stage]
    with pytest.raises(AssertionError, match=re.escape("[%s]" % stage)):
        step_trace.check(records, state, cfg, c, batch)
