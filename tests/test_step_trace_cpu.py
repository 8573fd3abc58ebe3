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
name and the B_BF16 storage bit, and that is how the mutation below is caught (by the contract, not by a bar).

Second half: the same with dropout in the contract (p = 0.25, counter 3).  The clean trace passes, the float64 chain IS
dropout_ref's model, and eleven mutations of the dropout step fail at their stage.  Every mutation tried at this shape
was caught; the two wrong-mask ones and the bias outside the dropout are caught by the EXACT dropped-set rule, which
does not depend on how far the mistake moves a value."""
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


# ------------------------------------------------------------------------------------------------------------ dropout
# The same setup with dropout in the contract: p = 0.25, a seed with both 32-bit halves in use, the counter at 3.
DROPOUT = (0.25, (0x9E3779B9 << 32) | 1024, 3)
M, D = 2 * 4 * 8, 64


@pytest.fixture(scope="module")
def dsetup():
    cfg, _, params, batch = _setup()
    return cfg, SS.Contract("bf16", "clip", masked=True, dropout=DROPOUT), params, batch


def test_schedule_without_dropout_has_no_dropout_launch(setup):
    cfg, c, _, _ = setup
    assert c.dropout is None and c.snapshots == SS.BACKWARD_BUFFERS
    assert not any("drop" in e["entry"] or "ddrop" in e["ops"] or "ybranch" in e["ops"] for e in SS.schedule(cfg, c))


def test_dropout_schedule_is_the_plain_one_plus_the_advance(setup, dsetup):
    """launch for launch the same families in the same places, every layer-norm launch fused, one advance at the end"""
    cfg, c, _, _ = setup
    plain, drop = SS.schedule(cfg, c), SS.schedule(cfg, dsetup[1])
    L = cfg.n_layers
    assert len(drop) == len(plain) + 1 and [e["family"] for e in drop[:-1]] == [e["family"] for e in plain]
    assert drop[-1]["entry"] == "vlg_dropout_step_advance"
    assert [e["site"] for e in drop if e["kind"] == "drop_ln_fwd"] == list(range(2 * L + 1))
    assert [e["site"] for e in drop if e["kind"] == "ln_bwd_drop"] == [2 * L] + [s for l in reversed(range(L)) for s in (1 + 2 * l, 2 * l)]
    assert not any(e["entry"].startswith(("vlg_layernorm_fwd", "vlg_layernorm_bwd_bf16")) or e["entry"] == "vlg_layernorm_bwd" for e in drop)
    first = next(e for e in drop if e["kind"] == "drop_ln_fwd")
    assert first["y"] == first["x_out"] == "x[0]" and first["resid"] is None
    assert [e["h"] for e in drop if e["kind"] == "drop_ln_fwd"][-1] == "xf"
    for e in drop:
        if e["kind"] == "linear_fwd" and e["w"].endswith(("proj_w", "ff2_w")):
            assert e["c"] == "ybranch" and e["epi"] == SS.EPI_BIAS and e["aux_in"] is None and not e["flags"] & SS.EPI_RESID
        if e["kind"] == "pair" and e["w"].endswith(("proj_w", "ff2_w")):
            assert e["dy"] == "ddrop"


def test_clean_synthetic_dropout_trace_passes(dsetup):
    cfg, c, params, batch = dsetup
    records, state = SS.emulate(cfg, c, params, batch, torch.float32)
    assert len(records) == len(SS.schedule(cfg, c)) and set(state["grads"]) == set(params)
    log = []
    step_trace.check(records, state, cfg, c, batch, log=log)
    assert len(log) > len(records)
    assert {"ln1 x", "ln2 xmid", "ln2 bwd ddrop", "lnf bwd ddrop"} <= {s.split(".")[-1] + " " + n.split("[")[0] for s, n, _, _ in log}


def test_fp64_dropout_chain_is_dropout_ref_when_nothing_rounds(dsetup):
    """test_fp64_chain_is_the_oracle_when_nothing_rounds' rule under dropout: with the fp32 contract the float64 chain along
    the dropout schedule is dropout_ref's autograd model with the masks of step k, to fp64 rounding."""
    import dropout_ref as R
    cfg, _, params, batch = dsetup
    p, seed, k = DROPOUT
    parts, grads, _, _ = R.loss_and_grads(R.to64(params), R.to64(batch), cfg.n_layers, p, k, seed, attention="clip")
    loss, g = SS.emulated_oracle(cfg, "fp32", params, batch, "clip", dropout=DROPOUT)
    assert torch.allclose(loss, torch.tensor(parts, dtype=torch.float64), rtol=1e-12, atol=0)
    for n, w in grads.items():
        assert float((g[n] - w).norm()) <= 1e-12 * max(float(w.norm()), 1e-3), n


def _mask(site, k=None):
    return SS.site_mask(SS.Contract("bf16", "clip", dropout=DROPOUT), M, D, site, k)


def _bwd_mask_next_step(e, val, o, g, rec):
    keep, scale = _mask(4, k=DROPOUT[2] + 1)
    o["ddrop"] = torch.where(keep, o["dx"] * scale, torch.zeros(()))


def _bwd_mask_of_site_2l(e, val, o, g, rec):
    keep, scale = _mask(0)
    o["ddrop"] = torch.where(keep, o["dx"] * scale, torch.zeros(()))


def _fwd_mask_in_public_order(e, val, o, g, rec):
    keep, scale = _mask(0)
    keep = SS.to_rows(keep.view(2, 4, 8, D))                 # row counter (b*T + t)*N + n instead of (b*N + n)*T + t
    o["x[0]"], o["h1[0]"], o["stats[0].mean"], o["stats[0].rstd"] = SS.drop_ln_fwd(
        val("x[0]"), None, val("p:l0.ln1_g"), val("p:l0.ln1_b"), keep, scale)


def _kept_not_scaled(e, val, o, g, rec):
    keep, _ = _mask(1)
    o["xmid[0]"] = val("x[0]") + val("ybranch") * keep
    o["h2[0]"], o["stats[1].mean"], o["stats[1].rstd"] = SS.ln_fwd(o["xmid[0]"], val("p:l0.ln2_g"), val("p:l0.ln2_b"))


def _proj_bwd_reads_dx(e, val, o, g, rec):
    rec["ops"] = tuple("dx" if n == "ddrop" else n for n in rec["ops"])
    o["dh"] = SS.linear_dgrad(val("dx"), val("pb:l1.proj_w"), SS.bf)
    g["l1.proj_w"], g["l1.proj_b"] = SS.linear_wgrad(val("dx"), val("att[1]"), SS.bf)


def _embed_bwd_reads_dx(e, val, o, g, rec):
    rec["ops"] = ("dx",) + rec["ops"][1:]
    _embed_bwd_values_of_dx(e, val, o, g, rec)


def _embed_bwd_values_of_dx(e, val, o, g, rec):
    batch = _setup()[3]
    g.update(SS.embed_bwd(val("dx"), batch["slot_class"], batch["slot_box"], g["cls_emb"].shape[0], 2, 4, 8))


def _proj_keeps_residual_epilogue(e, val, o, g, rec):
    rec["flags"] |= SS.EPI_RESID
    rec["ops"] = rec["ops"][:4] + ("x[0]",) + rec["ops"][5:]
    _proj_adds_residual(e, val, o, g, rec)


def _proj_adds_residual(e, val, o, g, rec):
    o["ybranch"] = SS.linear_fwd(val("att[0]"), val("pb:l0.proj_w"), val("p:l0.proj_b"), SS.bf, resid=val("x[0]"))[0]


def _bias_after_dropout(e, val, o, g, rec):
    keep, scale = _mask(1)
    b = val("p:l0.proj_b")
    o["xmid[0]"] = val("x[0]") + torch.where(keep, (val("ybranch") - b) * scale, torch.zeros(())) + b
    o["h2[0]"], o["stats[1].mean"], o["stats[1].rstd"] = SS.ln_fwd(o["xmid[0]"], val("p:l0.ln2_g"), val("p:l0.ln2_b"))


def _fused_h_unrounded(e, val, o, g, rec):
    o["h1[1]"] = SS.Raw(o["h1[1]"])


DROPOUT_MUTATIONS = [
    ("the backward mask drawn at k + 1 (counter advanced before the backward)", "lnf bwd", _bwd_mask_next_step),
    ("l0.ln2 bwd masked with site 2l instead of 1 + 2l", "l0.ln2 bwd", _bwd_mask_of_site_2l),
    ("the forward mask taken in public (b,t,n) row order", "l0.ln1", _fwd_mask_in_public_order),
    ("kept values not scaled: a 0/1 product instead of the select", "l0.ln2", _kept_not_scaled),
    ("proj backward reads dx instead of ddrop", "l1.proj dgrad+wgrad", _proj_bwd_reads_dx),
    ("the embedding backward reads dx (by name)", "embedding bwd", _embed_bwd_reads_dx),
    ("the embedding backward reads dx (by the cls_emb / box_w gradients)", "embedding bwd", _embed_bwd_values_of_dx),
    ("proj keeps its residual epilogue (by the flags word)", "l0.proj", _proj_keeps_residual_epilogue),
    ("proj adds the residual the fused launch adds again", "l0.proj", _proj_adds_residual),
    ("the bias added after the dropout instead of inside it", "l0.ln2", _bias_after_dropout),
    ("h of a fused launch left unrounded", "l1.ln1", _fused_h_unrounded),
]


@pytest.mark.parametrize("what,stage,fn", DROPOUT_MUTATIONS, ids=[m[0] for m in DROPOUT_MUTATIONS])
def test_dropout_mutation_is_caught_at_its_stage(dsetup, what, stage, fn):
    cfg, c, params, batch = dsetup
    hit = []

    def mutate(e, val, o, g, rec):
        if e["stage"] == stage:
            hit.append(stage)
            fn(e, val, o, g, rec)

    records, state = SS.emulate(cfg, c, params, batch, torch.float32, mutate)
    assert hit == [stage]
    with pytest.raises(AssertionError, match=re.escape("[%s]" % stage)):
        step_trace.check(records, state, cfg, c, batch)
