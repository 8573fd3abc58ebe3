"""test_step_trace_cpu.py's evidence for the contracts that file does not reach: attention = "factored", the Gaussian box
head, the loss options, scheduled sampling, augmentation, and all of them beside dropout.  Per contract: the float32
emulation is a clean trace that passes step_trace.check; the float64 chain with nothing rounding IS the specification
(factored_ref, loss_ext_ref, boxhead_ref's totals, the oracle on sched_ref.mix_inputs' / augment_ref.augment's batch) to fp64
rounding; the schedule is the plain one plus what the option adds.  Then the mutations: one launch of the synthetic trace
wired or computed wrongly - the caller's tensor where the engine's belongs, the other frame layer's lse row, another
option's counter, an option dropped - and step_trace.check names the mutated stage.  No GPU is needed.

Shape: B=2, T=4, N=8, d=64 (test_step_trace_cpu's); clip 0 has three padded slots.  Factored runs four layers, so that two
frame layers save into lse rows 0 and 1.  The Gaussian head's scale rows, zero at initialisation, are given values: with
zero rows the scale columns of `out` are 0 whatever the head launch does.  Contracts are "bf16" unless a case says so.

Last: the float32 emulation of the GPU suite's sampled scheduled-sampling case (test_hip_step_trace_options.SCHED_SAMPLED)
leaves no draw within the restatement's margin of a cumulative boundary - the seed was chosen for that."""
import re

import pytest
import torch

import augment_ref
import boxhead_ref
import factored_ref
import loss_ext_ref
import sched_ref
import step_stages as SS
import step_trace
from oracle import layout_spec as O

B, T, N, D, NC = 2, 4, 8, 64, 20
DROPOUT = (0.25, (0x9E3779B9 << 32) | 1024, 3)
SCHED = (0.5, 4, 0.0, 0, (0xC0FFEE12 << 32) | 345, 1)
AUGMENT = (augment_ref.ALL_ON, 0xC0FFEE1234567, 2)
WEIGHTS = [0.5 + 0.125 * i for i in range(NC)]
WEIGHTS[5] = 0.0
LOSS = (WEIGHTS, 0.1, "giou")
W_NLL = 0.5


def _setup(attention="slot", n_layers=2, gaussian=False):
    from vlg.spec import LayoutConfig, param_shapes
    cfg = LayoutConfig(B=B, T=T, N=N, d=D, n_layers=n_layers, attention=attention, **(dict(box_head="gaussian") if gaussian else {}))
    batch = O.synthetic_batch(B, T, N, seed=3)
    batch["valid"][0, :, 5:] = 0.0
    batch["slot_class"][0, :, 5:] = NC
    params = O.init_params(param_shapes(cfg), seed=1024)
    if gaussian:
        g = torch.Generator().manual_seed(5)
        params["head_w"][NC + 4:] = 0.0
        params["head_b"][NC + 4:] = 0.0
        params["head_w"][NC + 4:NC + 8] = (torch.rand(4, D, generator=g) * 2 - 1) * D ** -0.5
        params["head_b"][NC + 4:NC + 8] = torch.rand(4, generator=g) * 2 - 1
    return cfg, params, batch


# name -> (what _setup takes, what Contract takes beside the precision)
CONTRACTS = {
    "factored": (dict(attention="factored", n_layers=4), dict(attention="factored")),
    "gaussian": (dict(gaussian=True), dict(box_nll_weight=W_NLL)),
    "loss": (dict(), dict(loss=LOSS)),
    "sched": (dict(), dict(sched=SCHED, dropout=DROPOUT)),
    "augment": (dict(attention="clip"), dict(attention="clip", augment=AUGMENT)),
    "everything": (dict(attention="factored", n_layers=3, gaussian=True),
                   dict(attention="factored", box_nll_weight=W_NLL, loss=LOSS, sched=SCHED, augment=AUGMENT, dropout=DROPOUT)),
}
_CASES = {}


def case(name, precision="bf16"):
    """(cfg, contract, params, batch) of a named contract; built once"""
    if (name, precision) not in _CASES:
        skw, ckw = CONTRACTS[name]
        cfg, params, batch = _setup(**skw)
        _CASES[name, precision] = (cfg, SS.Contract(precision, masked=True, **ckw), params, batch)
    return _CASES[name, precision]


def to64(d):
    return {k: v.double() if v.is_floating_point() else v for k, v in d.items()}


# ------------------------------------------------------------------------------------------------ clean traces
@pytest.mark.parametrize("name", list(CONTRACTS))
def test_clean_synthetic_trace_passes(name):
    cfg, c, params, batch = case(name)
    records, state = SS.emulate(cfg, c, params, batch, torch.float32)
    assert len(records) == len(SS.schedule(cfg, c)) and set(state["grads"]) == set(params)
    log = []
    step_trace.check(records, state, cfg, c, batch, log=log)
    assert len(log) > len(records) - 3 * (c.sched is not None)
    if c.augment is not None:      # a track was dropped: the masks and the loss have the caller's `valid` to get wrong
        assert float(state["aug_valid"].sum()) < float(batch["valid"].sum())
    if c.sched is not None:
        assert [n for s, n, _, _ in log if s == "sched mix"] == ["draws left out"]
    st64 = SS.emulate(cfg, c, params, batch, torch.float64)[1]                      # the mode's emulated oracle runs too
    assert st64["loss"].dtype == torch.float64 and bool(torch.isfinite(st64["loss"]).all()) and set(st64["grads"]) == set(params)
    assert all(g.dtype == torch.float64 and bool(torch.isfinite(g).all()) for g in st64["grads"].values())


def test_the_three_counters_and_seeds_differ():
    c = case("everything")[1]
    assert len(set(c.counters().values())) == 3 and len({c.dropout[1], c.sched[4], c.augment[1]}) == 3
    assert all(s >> 32 for s in (c.dropout[1], c.sched[4], c.augment[1]))
    kinds = [e["kind"] for e in SS.schedule(case("everything")[0], c)]
    assert kinds[0] == "augment" and kinds[-3:] == ["advance"] * 3
    assert [e["counter"] for e in SS.schedule(case("everything")[0], c)[-3:]] == list(SS.COUNTERS)


# ------------------------------------------------------------------------------------------------ chain identities
def _same(loss, g, parts, grads):
    assert torch.allclose(loss[:len(parts)], torch.tensor(parts, dtype=torch.float64), rtol=1e-12, atol=0)
    assert set(g) == set(grads)
    for n, w in grads.items():
        assert float((g[n] - w).norm()) <= 1e-12 * max(float(w.norm()), 1e-3), n


def test_fp64_factored_chain_is_factored_ref_when_nothing_rounds():
    cfg, _, params, batch = case("factored")
    parts, grads = factored_ref.loss_and_grads(to64(params), to64(batch), cfg.n_layers)
    _same(*SS.emulated_oracle(cfg, "fp32", params, batch, "factored"), parts, grads)


def test_fp64_loss_option_chain_is_loss_ext_ref_when_nothing_rounds():
    cfg, _, params, batch = case("loss")
    parts, grads = loss_ext_ref.loss_and_grads(to64(params), to64(batch), cfg.n_layers, torch.tensor(WEIGHTS, dtype=torch.float64),
                                               LOSS[1], LOSS[2])
    _same(*SS.emulated_oracle(cfg, "fp32", params, batch, loss=LOSS), parts, grads)


def test_fp64_gaussian_chain_gives_boxhead_ref_totals_when_nothing_rounds():
    """the specification: the oracle's encoder with the 32-row head, oracle.losses on the class and mean columns, +
    box_nll_weight * boxhead_ref.box_nll (whose autograd IS the definition's gradient: the mean is detached there)"""
    cfg, _, params, batch = case("gaussian")
    q = {k: v.double().requires_grad_(True) for k, v in params.items()}
    b = to64(batch)
    logits, rest = O.forward(q, b["slot_class"], b["slot_box"], cfg.n_layers, NC)
    parts = O.losses(logits, rest[..., :4], b["tgt_class"], b["tgt_box"], b["valid"])
    nll, cover = boxhead_ref.box_nll(SS.to_rows(torch.cat([logits, rest], -1)), b["tgt_box"], b["valid"], B, T, N, NC)
    (parts[0] + W_NLL * nll).backward()
    want = [float(x.detach()) for x in (parts[0] + W_NLL * nll,) + tuple(parts[1:]) + (nll, cover)] + [0.0, 0.0]
    loss, g = SS.emulated_oracle(cfg, "fp32", params, batch, box_nll_weight=W_NLL)
    assert float(nll.detach()) != 0.0 and float(q["head_w"].grad[NC + 4:NC + 8].abs().max()) > 0
    _same(loss, g, want, {k: v.grad for k, v in q.items()})


def test_fp64_sched_chain_is_the_specification_on_mix_inputs_batch():
    """pass 1 = the oracle's forward on the true inputs; the step = the oracle on sched_ref.mix_inputs' batch, true targets"""
    cfg, _, params, batch = case("sched")
    sched = SCHED
    p64, b64 = to64(params), to64(batch)
    with torch.no_grad():
        out = SS.to_rows(torch.cat(O.forward(p64, b64["slot_class"], b64["slot_box"], cfg.n_layers, NC), -1))
    mc, mb, rep, near = sched_ref.mix_inputs(out, batch["slot_class"], batch["slot_box"], NC, sched[5], sched_ref.thr_max(sched[0]),
                                             sched[1], sched[2], sched[3], sched[4])
    assert 0 < int(rep.sum()) < int(sched_ref.eligible(batch["slot_class"], NC).sum()) and not bool(near.any())
    parts, grads = O.loss_and_grads(p64, dict(b64, slot_class=mc, slot_box=mb), cfg.n_layers)
    _same(*SS.emulated_oracle(cfg, "fp32", params, batch, sched=SCHED), parts, grads)


def test_fp64_augment_chain_is_the_specification_on_augment_refs_batch():
    cfg, _, params, batch = case("augment")
    knobs, seed, k = AUGMENT
    a = augment_ref.augment(batch, k, seed, n_classes=NC, **knobs)
    assert bool(a["drop"].any()) and not bool(a["drop"].all())
    b = to64(dict(batch, **{n: a[n] for n in SS.AUG_NAMES}))
    parts, grads = O.loss_and_grads(to64(params), b, cfg.n_layers, attention="clip")
    _same(*SS.emulated_oracle(cfg, "fp32", params, batch, "clip", augment=AUGMENT), parts, grads)


# ------------------------------------------------------------------------------------------------ schedule identities
LAYER_FWD = ["vlg_layernorm_fwd", "vlg_linear_fwd", "vlg_attention_fwd", "vlg_linear_fwd", "vlg_layernorm_fwd", "vlg_linear_fwd",
             "vlg_linear_fwd"]
LAYER_BWD = ["vlg_linear_dgrad_wgrad", "vlg_linear_dgrad_wgrad", "vlg_layernorm_bwd", "vlg_linear_dgrad_wgrad", "vlg_attention_bwd",
             "vlg_linear_dgrad_wgrad", "vlg_layernorm_bwd"]


def test_schedule_with_the_options_off_is_the_plain_one():
    """the launch list an engine without options makes (tests/test_hip_boxhead_step.py's POINT_STEP, up to the reduction and
    Adam); nothing of an option in any operand list"""
    cfg = case("loss")[0]
    plain = SS.schedule(cfg, SS.Contract("fp32", masked=True))
    assert [e["entry"] for e in plain] == (["vlg_embed_fwd"] + LAYER_FWD * 2 + ["vlg_layernorm_fwd", "vlg_linear_fwd", "vlg_layout_loss"] +
                                           ["vlg_linear_wgrad", "vlg_linear_dgrad", "vlg_layernorm_bwd"] + LAYER_BWD * 2 + ["vlg_embed_bwd"])
    names = {n for e in plain for n in e["ops"] if n}
    assert not any(n.startswith(("aug_", "mix_", "lse", "class_weights", "box_nll")) or n in SS.COUNTERS for n in names)
    assert {n for n in names if n.startswith("batch:")} == {"batch:" + k for k in ("slot_class", "slot_box", "tgt_class", "tgt_box", "valid")}


def test_factored_schedule_differs_from_slot_in_the_odd_layers_attention_alone():
    cfg = case("factored")[0]
    for precision in ("fp32", "bf16"):
        slot = SS.schedule(cfg, SS.Contract(precision, "slot", masked=True))
        fact = SS.schedule(cfg, SS.Contract(precision, "factored", masked=True))
        differ = [f["stage"] for s, f in zip(slot, fact) if s != f]
        assert len(slot) == len(fact) and differ == ["l1.attention", "l3.attention", "l3.attention bwd", "l1.attention bwd"]
        sfx = "_bf16" if precision == "bf16" else ""
        by_stage = {e["stage"]: e for e in fact}
        for l, row in ((1, 0), (3, 1)):
            f, b = by_stage["l%d.attention" % l], by_stage["l%d.attention bwd" % l]
            assert (f["entry"], f["family"]) == ("vlg_attention_frame_fwd" + sfx, "attn_frame_fwd")
            assert (b["entry"], b["family"]) == ("vlg_attention_frame_bwd" + sfx, "attn_frame_bwd")
            assert f["ops"] == ("qkv[%d]" % l, "batch:valid", "att[%d]" % l, "lse[%d]" % row)
            assert b["ops"] == ("qkv[%d]" % l, "batch:valid", "att[%d]" % l, "dh", "lse[%d]" % row, "delta", "dqkv")
    unmasked = SS.schedule(cfg, SS.Contract("fp32", "factored", masked=False))
    assert all(e["ops"][1] is None for e in unmasked if e["kind"].startswith("frame"))


def test_sched_schedule_is_pass_1_the_mix_the_plain_step_and_one_advance():
    cfg = case("loss")[0]
    for dropout in (None, DROPOUT):
        plain = SS.schedule(cfg, SS.Contract("bf16", masked=True, dropout=dropout))
        sched = SS.schedule(cfg, SS.Contract("bf16", masked=True, dropout=dropout, sched=SCHED))
        fwd = [e for e in SS.schedule(cfg, SS.Contract("bf16", masked=True)) if e["stage"] != "loss"][:len(LAYER_FWD) * 2 + 3]
        assert fwd[-1]["stage"] == "head" and len(sched) == len(fwd) + 1 + len(plain) + 1
        assert sched[:len(fwd)] == [dict(e, stage="pass1 " + e["stage"]) for e in fwd]      # no dropout, no loss launch
        mix = sched[len(fwd)]
        assert mix["entry"] == "vlg_layout_mix_inputs" and mix["ops"] == ("out", "batch:slot_class", "batch:slot_box", "mix_cls", "mix_box", "sched_step")
        ren = lambda n: {"batch:slot_class": "mix_cls", "batch:slot_box": "mix_box"}.get(n, n)
        rest = sched[len(fwd) + 1:]
        n_adv = int(dropout is not None)
        body = plain[:len(plain) - n_adv]
        want = [dict(e, cls=ren(e["cls"]), box=ren(e["box"]), ops=tuple(ren(n) for n in e["ops"])) if e["kind"].startswith("embed") else e for e in body]
        assert rest[:len(body)] == want
        assert [e["counter"] for e in rest[len(body):]] == ["drop_step", "sched_step"][1 - n_adv:]


def test_augment_schedule_renames_four_batch_tensors_everywhere():
    cfg = case("augment")[0]
    plain = SS.schedule(cfg, SS.Contract("bf16", "clip", masked=True))
    aug = SS.schedule(cfg, SS.Contract("bf16", "clip", masked=True, augment=AUGMENT))
    assert aug[0]["entry"] == "vlg_layout_augment" and aug[-1]["counter"] == "aug_step" and len(aug) == len(plain) + 2
    ren = lambda n: "aug_" + {"slot_class": "cls", "slot_box": "box", "tgt_box": "tgt_box", "valid": "valid"}[n[6:]] \
        if n is not None and n.startswith("batch:") and n != "batch:tgt_class" else n
    assert [e["ops"] for e in aug[1:-1]] == [tuple(ren(n) for n in e["ops"]) for e in plain]
    later = {n for e in aug[1:] for n in e["ops"] if n and n.startswith("batch:")}
    assert later == {"batch:tgt_class"}


# ------------------------------------------------------------------------------------------------ mutations
def _frame_block_causal(e, val, o, g, rec):
    o["att[1]"], o["lse[0]"] = SS.clip_attention_fwd(val("qkv[1]"), val("batch:valid"), B, T, N, SS.bf)


def _frame_ignores_valid(e, val, o, g, rec):
    o["att[1]"], o["lse[0]"] = SS.clip_attention_fwd(val("qkv[1]"), None, B, T, N, SS.bf, frame_only=True)


def _frame_bwd_other_lse_row(e, val, o, g, rec):
    o["dqkv"], o["delta"] = SS.clip_attention_bwd(val("qkv[3]"), val("dh"), val("att[3]"), val("lse[0]"), val("batch:valid"), B, T, N,
                                                  SS.bf, frame_only=True)


def _frame_p_unrounded(e, val, o, g, rec):
    o["att[1]"], o["lse[0]"] = SS.clip_attention_fwd(val("qkv[1]"), val("batch:valid"), B, T, N, frame_only=True)


def _embed(val, cls, box):
    return SS.embed_fwd(val("p:cls_emb"), val("p:box_w"), val("p:box_b"), val("p:time_emb"), val(cls), val(box))


def _pass2_embeds_the_truth(e, val, o, g, rec):
    o["x[0]"] = _embed(val, "batch:slot_class", "batch:slot_box")


def _embed_bwd_on_the_truth(e, val, o, g, rec):
    g.update(SS.embed_bwd(val(e["ops"][0]), val("batch:slot_class"), val("batch:slot_box"), g["cls_emb"].shape[0], B, T, N))


def _pass1_with_dropout(e, val, o, g, rec):
    keep, scale = SS.site_mask(case("sched")[1], B * T * N, D, 0)
    _, o["h1[0]"], o["stats[0].mean"], o["stats[0].rstd"] = SS.drop_ln_fwd(val("x[0]"), None, val("p:l0.ln1_g"), val("p:l0.ln1_b"), keep, scale)


def _mix_reads_stale_out(e, val, o, g, rec):
    """`out` as the previous step's pass 2 left it (the same batch: this step's own pass 2 output)"""
    cfg, c, params, batch = case("sched")
    stale = SS.emulate(cfg, c, params, batch, torch.float32)[1]["out"]
    o["mix_cls"], o["mix_box"], _, _ = SS.sched_mix_stage(c, stale, val("batch:slot_class"), val("batch:slot_box"), NC)


def _coins_at_the_next_step(e, val, o, g, rec):
    c = case("sched")[1]
    o["mix_cls"], o["mix_box"], _, _ = SS.sched_mix_stage(c, val("out"), val("batch:slot_class"), val("batch:slot_box"), NC, k=SCHED[5] + 1)


def _mix_handed_the_dropout_counter(e, val, o, g, rec):
    c = case("sched")[1]
    rec["ops"] = tuple("drop_step" if n == "sched_step" else n for n in rec["ops"])
    o["mix_cls"], o["mix_box"], _, _ = SS.sched_mix_stage(c, val("out"), val("batch:slot_class"), val("batch:slot_box"), NC, k=DROPOUT[2])


def _mix_draws_at_the_dropout_counters_value(e, val, o, g, rec):
    c = case("sched")[1]
    o["mix_cls"], o["mix_box"], _, _ = SS.sched_mix_stage(c, val("out"), val("batch:slot_class"), val("batch:slot_box"), NC, k=DROPOUT[2])


def _no_advance(e, val, o, g, rec):
    rec["counters"] = dict(rec["counters"], sched_step=SCHED[5])


def _two_advances(e, val, o, g, rec):
    rec["counters"] = dict(rec["counters"], sched_step=SCHED[5] + 2)


def _loss(val, tgt_box="aug_tgt_box", valid="aug_valid", options=None):
    return SS.loss_fwd(val("out"), val("batch:tgt_class"), val(tgt_box), val(valid), B, T, N, NC, options)


def _loss_on_callers_valid(e, val, o, g, rec):
    o["loss_out"], o["dout"] = _loss(val, valid="batch:valid")


def _loss_on_callers_tgt_box(e, val, o, g, rec):
    o["loss_out"], o["dout"] = _loss(val, tgt_box="batch:tgt_box")


def _mask_on_callers_valid(e, val, o, g, rec):
    o["att[0]"], o["lse[0]"] = SS.clip_attention_fwd(val("qkv[0]"), val("batch:valid"), B, T, N, SS.bf)


def _dropped_track_keeps_a_gradient(e, val, o, g, rec):
    dropped = SS.to_rows(((val("aug_valid") == 0) & (val("batch:valid") > 0))[..., None])[:, 0]
    assert bool(dropped.any())
    o["dout"] = o["dout"].clone()
    o["dout"][dropped] = 1e-30


def _ext(val, weights=True, eps=LOSS[1], overlap=LOSS[2]):
    return SS.loss_fwd(val("out"), val("batch:tgt_class"), val("batch:tgt_box"), val("batch:valid"), B, T, N, NC,
                       (val("class_weights") if weights else None, eps, overlap))


def _no_label_smoothing(e, val, o, g, rec):
    o["loss_out"], o["dout"] = _ext(val, eps=0.0)


def _iou_for_giou(e, val, o, g, rec):
    o["loss_out"], o["dout"] = _ext(val, overlap="iou")


def _weights_not_in_the_normaliser(e, val, o, g, rec):
    """CE = (1 / count) sum ... in place of (1 / W) sum ...: the weighted numerator over the plain count"""
    out = SS.from_rows(val("out"), B, T, N).detach().clone().requires_grad_(True)
    w, valid, y = val("class_weights"), val("batch:valid"), val("batch:tgt_class")
    parts = loss_ext_ref.losses(out[..., :NC], out[..., NC:], y, val("batch:tgt_box"), valid, w, LOSS[1], LOSS[2])
    ce = parts[3] * (valid * w[y.clamp(0, NC - 1)]).sum() / valid.sum()
    total = O.W_REG * parts[1] + O.W_IOU * parts[2] + O.W_CE * ce
    total.backward()
    o["loss_out"], o["dout"] = torch.stack([total.detach(), parts[1].detach(), parts[2].detach(), ce.detach()]), SS.to_rows(out.grad)


def _nll_reaches_the_mean(e, val, o, g, rec):
    o["dout"] = o["dout"].clone()
    o["dout"][:, NC:NC + 4] += o["dout"][:, NC + 4:NC + 8]


def _padding_columns_written(e, val, o, g, rec):
    o["dout"] = o["dout"].clone()
    o["dout"][:, NC + 8:] = 1e-30


def _nll_weight_missing(e, val, o, g, rec):
    o["loss_out"] = o["loss_out"].clone()
    o["loss_out"][0] = val("loss_out")[0] + o["loss_out"][4]


def _head_at_24_columns(e, val, o, g, rec):
    o["out"] = o["out"].clone()
    o["out"][:, NC + 4:] = 0.0


MUTATIONS = [
    ("factored", "a frame layer computed with the block-causal visibility", "l1.attention", _frame_block_causal),
    ("factored", "a frame layer that ignores valid", "l1.attention", _frame_ignores_valid),
    ("factored", "a frame backward reading the other frame layer's lse row", "l3.attention bwd", _frame_bwd_other_lse_row),
    ("factored", "frame-layer P left unrounded under bf16", "l1.attention", _frame_p_unrounded),
    ("sched", "pass-2 embedding reading the true inputs", "embedding", _pass2_embeds_the_truth),
    ("sched", "embed_bwd reading the true inputs", "embedding bwd", _embed_bwd_on_the_truth),
    ("sched", "pass 1 run with dropout", "pass1 l0.ln1", _pass1_with_dropout),
    ("sched", "the mix reading pass 2's stale out", "sched mix", _mix_reads_stale_out),
    ("sched", "coins drawn at counter k + 1", "sched mix", _coins_at_the_next_step),
    ("sched", "the sched launch handed the dropout counter (by name)", "sched mix", _mix_handed_the_dropout_counter),
    ("sched", "the sched launch reading the dropout counter's value", "sched mix", _mix_draws_at_the_dropout_counters_value),
    ("sched", "a missing advance", "sched step", _no_advance),
    ("sched", "a doubled advance", "sched step", _two_advances),
    ("augment", "loss reading batch:valid in place of aug_valid", "loss", _loss_on_callers_valid),
    ("augment", "loss reading batch:tgt_box in place of aug_tgt_box", "loss", _loss_on_callers_tgt_box),
    ("augment", "attention masks on batch:valid", "l0.attention", _mask_on_callers_valid),
    ("augment", "a dropped track's dout rows non-zero", "loss", _dropped_track_keeps_a_gradient),
    ("loss", "label smoothing dropped", "loss", _no_label_smoothing),
    ("loss", "class weights not in the CE normaliser", "loss", _weights_not_in_the_normaliser),
    ("loss", "IoU where GIoU was configured", "loss", _iou_for_giou),
    ("gaussian", "NLL gradient leaking into the mean columns", "box nll", _nll_reaches_the_mean),
    ("gaussian", "non-zero padding columns", "box nll", _padding_columns_written),
    ("gaussian", "box_nll_weight missing from the total", "box nll", _nll_weight_missing),
    ("gaussian", "head run at 24 columns", "head", _head_at_24_columns),
]


@pytest.mark.parametrize("name,what,stage,fn", MUTATIONS, ids=[m[1] for m in MUTATIONS])
def test_mutation_is_caught_at_its_stage(name, what, stage, fn):
    cfg, c, params, batch = case(name)
    hit = []

    def mutate(e, val, o, g, rec):
        if e["stage"] == stage:
            hit.append(stage)
            fn(e, val, o, g, rec)

    records, state = SS.emulate(cfg, c, params, batch, torch.float32, mutate)
    assert hit == [stage]
    with pytest.raises(AssertionError, match=re.escape("[%s]" % stage)):
        step_trace.check(records, state, cfg, c, batch)


# ------------------------------------------------------------------------------------------------ the sampled case
def test_the_sampled_gpu_case_flags_no_draw_in_its_float32_emulation():
    """the case of test_hip_step_trace_options at its own shape, parameters and batch: with SCHED_SAMPLED's seed the
    restatement decides every draw (none within its margin of a cumulative boundary), so the GPU case leaves nothing out
    unless the device's pass 1 differs from torch-CPU fp32's by more than the margin somewhere"""
    from test_hip_step_trace import S1, _batch
    from test_hip_step_trace_options import SCHED_SAMPLED
    from vlg.spec import LayoutConfig, param_shapes
    cfg = LayoutConfig(**S1)
    c = SS.Contract("fp32", masked=True, sched=SCHED_SAMPLED)
    flagged = []

    def mutate(e, val, o, g, rec):
        if e["kind"] == "sched_mix":
            _, _, rep, near = SS.sched_mix_stage(c, val("out"), val("batch:slot_class"), val("batch:slot_box"), cfg.n_classes)
            flagged.append((int(near.sum()), int(rep.sum())))

    SS.emulate(cfg, c, O.init_params(param_shapes(cfg), seed=1024), _batch(cfg, True), torch.float32, mutate)
    assert len(flagged) == 1 and flagged[0][0] == 0 and flagged[0][1] >= 30, flagged
