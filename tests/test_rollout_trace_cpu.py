"""CPU: the per-launch check of generation discriminates.  (1) rollout_stages.rollout_schedule against vlg.engine.grow_schedule.
(2) The stage functions chained in fp64 (rollout_stages.emulate_rollout) give, at every generated frame, the logits of the
existing references on the history alone - oracle.layout_spec's forward for "slot" and "clip", factored_ref.forward for
"factored", read at position h-1 of the h frames - to 1e-12, cached and re-encoded: the cached schedule IS the specification.
(3) A float32 emulation under each contract passes rollout_trace.check.  (4) Twenty wiring mistakes each fail it at their own
stage.  (5) The tie-cap rehearsal of tests/test_hip_rollout_trace.py: for every GPU case the fp64 reference rolled out alone and
the float32 emulation under the case's contract keep the tokens inside decode_ref's exclusion width within the 1 % that
rollout_trace.check asserts (measured: 0 tokens in every case, both ways)."""
import numpy as np
import pytest
import torch

import boxhead_ref
import factored_ref
import philox_ref
import rollout_stages as RS
import rollout_trace as RT
import step_stages as SS
import test_hip_rollout_trace as G
from oracle import layout_spec as O
from vlg.engine import grow_schedule, init_params
from vlg.samples import sample_passes
from vlg.spec import LayoutConfig

T, NC = G.T, G.NC
GEN = G.GEN
_MODEL = {}


def model(attention, kw=G.A, gaussian=False):
    key = (attention, id(kw), gaussian)
    if key not in _MODEL:
        cfg = LayoutConfig(attention=attention, box_head="gaussian" if gaussian else "point", **kw)
        _MODEL[key] = (cfg, init_params(cfg, seed=1024))
    return _MODEL[key]


def prompt(kw, P, variable_n=False):
    cls, box = G.prompt(kw, variable_n)
    return cls[:, :P].contiguous(), box[:, :P].contiguous()


# ---------------------------------------------------------------------------------------------------------- the schedule
@pytest.mark.parametrize("attention,clip_cache", [("slot", False), ("clip", False), ("clip", True), ("factored", False)])
def test_schedule_identities(attention, clip_cache):
    cfg, _ = model(attention)
    L = cfg.n_layers
    per = 1 + 7 * L + 2
    for P in (1, 2, T - 1, T):
        for cache in (None, False):
            c = RS.GenContract("fp32", attention, clip_cache=clip_cache, cache=cache, **GEN)
            steps = T - P + 2
            sched = RS.rollout_schedule(cfg, c, P, steps)
            cached = P < T and cache is None and (attention != "clip" or clip_cache)
            grow = grow_schedule(P, T, steps, cached)
            assert len(sched) == per * steps
            for i, (enc, t_read, pos) in enumerate(grow):       # a grown frame and a window frame: 1 + 7 L + 2 launches each
                frame = [e for e in sched if e["frame"] == i]
                assert len(frame) == per and {e["encoder"] for e in frame} == {enc}
                steps_in = [e["entry"] for e in frame if "_step" in e["entry"]]
                assert len(steps_in) == (L if enc == "step" else 0)
                if enc == "step" and attention == "factored":   # alternates by layer parity
                    assert steps_in == ["vlg_attention_step" if l % 2 == 0 else "vlg_attention_frame_step" for l in range(L)]
                head, dec = frame[-2], frame[-1]
                assert head["entry"] == ("vlg_head_frame" if enc == "window" and t_read < T - 1 else "vlg_head_last_frame")
                assert dec["entry"] == ("vlg_layout_decode_append" if pos is not None else "vlg_layout_decode")
                assert dec["scalars"]["step"] == i and dec["scalars"].get("pos") == pos
            n_step_frames = sum(enc == "step" for enc, _, _ in grow)
            assert n_step_frames == sum(e["kind"] == "embed_step" for e in sched)
            if P == T or cache is False or (attention == "clip" and not clip_cache):
                assert not any("_step" in e["entry"] for e in sched)        # no step entry: full prompt, cache=False, clip without the option
            wins = [e["win"] for e in sched if e["kind"].startswith("decode")]
            slid = [e["kind"] == "decode_slide" for e in sched if e["kind"].startswith("decode")]
            for a, b, s in zip(wins, wins[1:], slid):           # the window buffers ping-pong by name at every slide, and only there
                assert (a != b) == s


# --------------------------------------------------------------------------------------------------- fp64 chain identities
@pytest.mark.parametrize("cache", [None, False], ids=["cached", "reencode"])
@pytest.mark.parametrize("P", [1, 2, T - 1, T])
@pytest.mark.parametrize("attention", ["slot", "clip", "factored"])
def test_fp64_chain_is_the_specification_on_the_history_alone(attention, P, cache):
    cfg, params = model(attention)
    variable_n = attention != "slot"
    c = RS.GenContract("fp32", attention, masked=variable_n, clip_cache=True, cache=cache, **dict(GEN, keep_padded=variable_n))
    pc, pb = prompt(G.A, P, variable_n)
    steps = T - P + 2
    _, st = RS.emulate_rollout(cfg, c, params, (pc, pb), steps, torch.float64)
    ps = st["passes"][0]
    p64 = {k: v.double() for k, v in params.items()}
    hist_c, hist_b = pc.clone(), pb.double()
    for i in range(steps):
        wc, wb = hist_c[:, -T:], hist_b[:, -T:]
        with torch.no_grad():
            if attention == "factored":
                wl, wr = factored_ref.forward(p64, wc, wb, cfg.n_layers, valid=(wc < NC).double())
            else:
                wl, wr = O.forward(p64, wc, wb, cfg.n_layers, attention=attention, valid=(wc < NC).double())
        want = torch.cat([wl[:, -1], wr[:, -1]], dim=-1).reshape(-1, cfg.n_out)
        err = float((ps["logits"][i] - want).abs().max())
        assert err <= 1e-12 * float(want.abs().max()), (attention, P, cache, i, err)
        hist_c = torch.cat([hist_c, ps["gen_cls"][:, i:i + 1]], 1)
        hist_b = torch.cat([hist_b, ps["gen_box"][:, i:i + 1]], 1)


# --------------------------------------------------------------------------------------------------------- clean traces
def _emulate(attention, precision, P=2, variable_n=False, gaussian=False, samples=None, mutate=None, kw=G.A, **opts):
    cfg, params = model(attention, kw, gaussian)
    knobs = dict(GEN, keep_padded=variable_n)
    knobs.update({k: opts.pop(k) for k in list(opts) if k in RS.KNOBS})
    c = RS.GenContract(precision, attention, masked=variable_n, gaussian=gaussian, **opts, **knobs)
    pr = prompt(kw, P, variable_n)
    steps = T - P + 2
    if samples is None:
        records, state = RS.emulate_rollout(cfg, c, params, pr, steps, torch.float32, mutate)
        return records, state, cfg, c, pr, None
    passes = sample_passes(samples[0], samples[1], pr[0].shape[0] * T * pr[0].shape[2], 2 * pr[0].shape[0] * T * pr[0].shape[2])
    records, state = RS.emulate_samples(cfg, c, params, pr, steps, torch.float32, passes, mutate)
    return records, state, cfg, c, pr, passes


def _check(records, state, cfg, c, pr, passes):
    return RT.check(records, state, cfg, c, pr, passes=passes)


@pytest.mark.parametrize("precision", SS.PRECISIONS)
@pytest.mark.parametrize("attention", ["slot", "clip", "factored"])
def test_clean_synthetic_traces_pass(attention, precision):
    for P, variable_n in ((2, False), (1, attention != "slot")):
        near, tokens = _check(*_emulate(attention, precision, P, variable_n, clip_cache=True))
        assert near == 0 and tokens == (T - P + 2) * 16
    if attention == "clip":                                   # without the option the grown frames re-encode
        _check(*_emulate(attention, precision, 2))


def test_clean_gaussian_and_sampled_traces_pass():
    for precision in ("fp32", "bf16"):
        _check(*_emulate("slot", precision, gaussian=True, box_temperature=0.7))
        out = _emulate("slot", precision, samples=(G.K, G.SAMPLE0))
        assert out[-1] == [(1, 2), (3, 1)]
        _check(*out)
    _check(*_emulate("slot", "fp32", P=1, temperature=0.0, top_k=0))


# ------------------------------------------------------------------------------------------------------------ mutations
def _at(e, frame, stage, kind=None):
    return e["frame"] == frame and e["stage"].endswith(" " + stage) and (kind is None or e["kind"] == kind)


def _rename(rec, old, new):
    rec["ops"] = tuple(new if n == old else n for n in rec["ops"])


def _m_time_emb(e, val, o, rec, run):
    if _at(e, 1, "embedding", "embed_step"):
        o.update(run(dict(e, p=e["p"] - 1)))


def _m_qkv_position(e, val, o, rec, run):
    if _at(e, 1, "l0.qkv", "linear_step"):
        return {"scatter": e["scatter"] - 1}


def _m_qkv_ldc(e, val, o, rec, run):
    if _at(e, 1, "l1.qkv", "linear_step"):
        return {"ld": 3 * 64}


def _m_newest_key(e, val, o, rec, run):
    if _at(e, 1, "l0.attention", "slot_step"):
        o["grow.att"] = RS.slot_step(val("qkv[0]"), e["p"], 2, T, 8, newest=False)


def _m_frame_in_even_layer(e, val, o, rec, run):
    if _at(e, 1, "l0.attention", "slot_step"):
        rec["name"], rec["family"], rec["ops"] = "vlg_attention_frame_step", "attn_frame_step", ("qkv[0]", None, "grow.att")
        o.update(run(dict(e, kind="frame_step", valid=None)))


def _m_slot_in_odd_layer(e, val, o, rec, run):
    if _at(e, 1, "l1.attention", "frame_step"):
        rec["name"], rec["family"], rec["ops"] = "vlg_attention_step", "attn_step", ("qkv[1]", "grow.att")
        o.update(run(dict(e, kind="slot_step")))


def _m_clip_unmasked(e, val, o, rec, run):
    if _at(e, 1, "l0.attention", "clip_step"):
        o.update(run(dict(e, valid=None)))


def _m_other_windows_valid(e, val, o, rec, run):
    if _at(e, 1, "l0.attention", "clip_step"):
        _rename(rec, "win0.valid", "win1.valid")
        o.update(run(dict(e, valid="win1.valid")))


def _m_head_reads_next_frame(e, val, o, rec, run):
    if _at(e, 0, "head"):
        o.update(run(dict(e, t_read=e["t_read"] + 1)))


def _m_head_on_shadow_weights(e, val, o, rec, run):
    if _at(e, 1, "head"):
        o["logits[1]"] = RS.head_frame(val(e["x"]), val("pb:lnf_g"), val("pb:lnf_b"), val("pb:head_w"), val("pb:head_b"), 16, e["T"], e["t_read"])


def _m_master_weight_in_projection(e, val, o, rec, run):
    if _at(e, 1, "l0.proj", "linear_step"):
        _rename(rec, "pb:l0.proj_w", "p:l0.proj_w")


def _m_no_out_bf16(e, val, o, rec, run):
    if _at(e, 1, "l0.qkv", "linear_step"):
        rec["flags"] &= ~SS.EPI_OUT_BF16


def _m_residual_from_xa(e, val, o, rec, run):
    if _at(e, 1, "l0.ff2", "linear_step"):
        o.update(run(dict(e, aux_in="grow.xa")))


def _decode_again(e, val, o, c, cfg, **over):
    h = T if e["pos"] is None else e["pos"]
    step = over.pop("step", e["i"])
    o["cls"], o["box"], o["near"] = RS.decode_frame(cfg, c, val("logits")[e["i"]], val(e["win"] + ".cls")[:, :h], val(e["win"] + ".box")[:, :h],
                                                    step, **over)


def _decode_mutation(frame, pass_index=0, **over):
    def mutate(e, val, o, rec, run):
        if e["kind"].startswith("decode") and e["frame"] == frame and rec["pass"] == pass_index:
            _decode_again(e, val, o, run.c, run.cfg, **over)
    return mutate


def _m_stale_compact_frame(e, val, o, rec, run):
    if e["kind"] == "decode_append" and e["frame"] == 1:
        return {"skip": ("grow.cls", "grow.box")}


def _m_append_before(e, val, o, rec, run):
    if e["kind"] == "decode_append" and e["frame"] == 0:
        return {"pos": e["pos"] - 1}


def _m_slide_in_place(e, val, o, rec, run):
    if e["kind"] == "decode_slide" and e["frame"] == 2:
        return {"slide_from": 0}


def _m_box_from_class_stream(e, val, o, rec, run):
    if e["kind"].startswith("decode") and e["frame"] == 1:
        out = val("logits")[1].double()
        mu = torch.sigmoid(out[:, NC:NC + 4])
        sigma = torch.exp(boxhead_ref.S_MIN + (boxhead_ref.S_MAX - boxhead_ref.S_MIN) * torch.sigmoid(out[:, NC + 4:NC + 8]))
        z = torch.from_numpy(boxhead_ref.normals_of_words(philox_ref.words(np.arange(16), 1, philox_ref.CLASS_DRAW, GEN["seed"])))
        o["box"] = (mu + float(np.float32(0.7)) * sigma * z).clamp(0.0, 1.0).view(2, 8, 4)


# (id, mutation, the stage it must fail at, the case: arguments of _emulate)
MUTATIONS = [
    ("time_emb row p-1 in the cached embedding", _m_time_emb, "pass 0 frame 1 embedding", dict(attention="slot", precision="fp32")),
    ("q k v written at position p-1", _m_qkv_position, "pass 0 frame 1 l0.qkv", dict(attention="slot", precision="fp32")),
    ("q k v with ldc = 3d: a neighbour row changes", _m_qkv_ldc, "pass 0 frame 1 l1.qkv", dict(attention="slot", precision="bf16")),
    ("the per-slot step omits the newest key", _m_newest_key, "pass 0 frame 1 l0.attention", dict(attention="slot", precision="fp32")),
    ("frame step in an even layer", _m_frame_in_even_layer, "pass 0 frame 1 l0.attention", dict(attention="factored", precision="fp32")),
    ("slot step in an odd layer", _m_slot_in_odd_layer, "pass 0 frame 1 l1.attention", dict(attention="factored", precision="fp32")),
    ("the clip step unmasked where _masked", _m_clip_unmasked, "pass 0 frame 1 l0.attention",
     dict(attention="clip", precision="fp32", variable_n=True, clip_cache=True)),
    ("valid of the other window buffer", _m_other_windows_valid, "pass 0 frame 1 l0.attention",
     dict(attention="clip", precision="bf16", variable_n=True, clip_cache=True)),
    ("the head reads t_read + 1 while growing", _m_head_reads_next_frame, "pass 0 frame 0 head", dict(attention="slot", precision="fp32")),
    ("bf16 shadow weights in the head", _m_head_on_shadow_weights, "pass 0 frame 1 head", dict(attention="slot", precision="bf16")),
    ("master weight in a bf16 projection", _m_master_weight_in_projection, "pass 0 frame 1 l0.proj", dict(attention="slot", precision="bf16")),
    ("missing OUT_BF16 on the cache store", _m_no_out_bf16, "pass 0 frame 1 l0.qkv", dict(attention="slot", precision="bf16")),
    ("residual aux xa where xmid belongs", _m_residual_from_xa, "pass 0 frame 1 l0.ff2", dict(attention="slot", precision="fp32")),
    ("decode with step i-1 in the counter", _decode_mutation(1, step=0), "pass 0 frame 1 decode", dict(attention="slot", precision="fp32")),
    ("the second pass's sample0 left at 0", _decode_mutation(0, pass_index=1, sample0=0), "pass 1 frame 0 decode",
     dict(attention="slot", precision="fp32", samples=(G.K, G.SAMPLE0))),
    ("compact grow.cls not refreshed", _m_stale_compact_frame, "pass 0 frame 1 decode", dict(attention="slot", precision="fp32", P=1)),
    ("append at pos - 1", _m_append_before, "pass 0 frame 0 decode", dict(attention="slot", precision="fp32")),
    ("the slide copies frames 0 .. T-2", _m_slide_in_place, "pass 0 frame 2 decode", dict(attention="slot", precision="fp32")),
    ("keep_padded ignored", _decode_mutation(1, keep_padded=False), "pass 0 frame 1 decode",
     dict(attention="factored", precision="fp32", variable_n=True)),
    ("box draw taken from the class stream", _m_box_from_class_stream, "pass 0 frame 1 decode",
     dict(attention="slot", precision="fp32", gaussian=True, box_temperature=0.7)),
]


@pytest.mark.parametrize("what,mutate,stage,kw", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_a_mutation_fails_at_its_own_stage(what, mutate, stage, kw):
    kw = dict(kw)
    clean = _emulate(**kw)
    _check(*clean)                                            # the case passes before the mutation ...
    out = _emulate(mutate=mutate, **kw)
    with pytest.raises(AssertionError) as err:                # ... and fails at the stage of the mistake after it
        _check(*out)
    assert str(err.value).startswith("[%s]" % stage), "%s: failed as %s" % (what, str(err.value)[:200])


# ---------------------------------------------------------------------------------------------------- tie-cap rehearsal
def test_tie_cap_rehearsal():
    """for every GPU case: the fp64 reference alone (the chain in float64, no storage rounding) and the float32 emulation under
    the case's contract, free-running from the case's prompt - tokens inside the exclusion width <= 1 % of the decoded ones"""
    lines = []
    for cases, samples in ((G.CASES, None), (G.SAMPLE_CASES, (G.K, G.SAMPLE0))):
        for c in cases:
            cfg, params = model(c["attention"], c["kw"], bool(c["opts"].get("gaussian")))
            pc, pb = prompt(c["kw"], c["P"], c["variable_n"])
            steps = T - c["P"] + 2
            counts = []
            for precision, dtype in (("fp32", torch.float64), (c["precision"], torch.float32)):
                gc = RS.GenContract(precision, c["attention"], masked=c["variable_n"], **c["opts"], **c["knobs"])
                if samples is None:
                    _, st = RS.emulate_rollout(cfg, gc, params, (pc, pb), steps, dtype)
                    tokens = steps * pc.shape[0] * pc.shape[2]
                else:
                    clip = pc.shape[0] * T * pc.shape[2]
                    _, st = RS.emulate_samples(cfg, gc, params, (pc, pb), steps, dtype, sample_passes(samples[0], samples[1], clip, 2 * clip))
                    tokens = samples[0] * steps * pc.shape[0] * pc.shape[2]
                assert st["near"] <= 0.01 * tokens, (G._id(c), precision, st["near"], tokens)
                counts.append(st["near"])
            lines.append("%s%s: fp64 %d, float32 emulation %d of %d tokens" % (G._id(c), "" if samples is None else "-samples", counts[0], counts[1], tokens))
    print("\n" + "\n".join(lines))
