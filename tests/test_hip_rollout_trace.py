"""GPU: every launch of one LayoutEngine.rollout / rollout_samples call against fp64 evaluated on the values that launch read.

The end-to-end rollout tests hold bf16 logits to a relative Frobenius error of 5e-2 per step and roll out nothing under
precision="bf16_mfma"; a stale cache row, a master weight where the bf16 shadow belongs, a missing storage bit on the strided
q k v store, a wrong time_emb row or the other ping-pong window's mask all pass them.  Here the COMPOSITION of generation - the
prompt pass, the three cached grow steps (per-slot, opt-in per-clip, factored) with their K/V cache, the re-encoded grow step,
the hand-over to the sliding window and the slides, the _ext and _samples decode entries - is checked one launch at a time:
rollout_trace.trace records the launches, rollout_trace.check holds each to the contract by name and to the per-kernel bar
that entry point's own test uses (its docstring has the table).  No bar here is new.  tests/test_rollout_trace_cpu.py shows that
these checks catch twenty wiring mistakes at the stage where they happen.

Shapes, L = 2, steps = T - P + 2 (the prompt pass, every grown frame, the hand-over, one or two slides):
  A  (2,4,8), d = 64: the shape of the existing rollout tests
  B  (3,4,23), d = 128: two heads; B*N = 69 tokens cross the 64-token decode block and are an odd row count for the head's
     two-rows-per-wave path.  attention = "slot" alone: T*N = 92 is no multiple of the 32-token tile, and LayoutConfig refuses
     per-clip kinds there (asserted below)
  B' (3,4,24), d = 128: what the per-clip and factored cases take in B's place - B*N = 72 tokens still cross the decode block,
     N = 24 is ragged for the 32-key tiles (frame boundaries inside every tile)

Tie counts (decoded tokens whose fp64 decision lies within decode_ref's exclusion width, 1e-5 of the kept mass): computed on
the CPU for every case below by tests/test_rollout_trace_cpu.py::test_tie_cap_rehearsal - the fp64 reference rolled out alone
and the float32 emulation under the case's contract: 0 of every case's tokens in both (32 to 360 tokens a case), under the
1 % that rollout_trace.check asserts."""
import time

import pytest
import torch

import rollout_stages as RS
import rollout_trace
from oracle import layout_spec as O
from test_hip_layout_decode import GEN

pytestmark = pytest.mark.gpu

A = dict(B=2, T=4, N=8, d=64, n_layers=2)
B_ = dict(B=3, T=4, N=23, d=128, n_layers=2)
B2 = dict(B=3, T=4, N=24, d=128, n_layers=2)
T, NC = 4, 20
_IDS = {id(A): "A", id(B_): "B", id(B2): "B'"}


def prompt(kw, variable_n=False):
    """test_hip_rollout_factored.prompt at the case's shape: seed 21; variable_n: the last three eighths of the slots padded in
    every frame, and one slot of one clip in its first frame only"""
    b = O.synthetic_batch(kw["B"], kw["T"], kw["N"], seed=21)
    cls, box = b["slot_class"].clone(), b["slot_box"].clone()
    if variable_n:
        cls[:, :, kw["N"] * 5 // 8:] = NC
        cls[1, :1, 1] = NC
    return cls, box


def case(precision, attention, kw, P, variable_n=False, **opts):
    """one rollout case: opts are GenContract's (cache, clip_cache, gaussian, samples-free knobs override GEN)"""
    knobs = dict(GEN, keep_padded=variable_n)
    knobs.update({k: opts.pop(k) for k in list(opts) if k in RS.KNOBS})
    return dict(precision=precision, attention=attention, kw=kw, P=P, variable_n=variable_n, knobs=knobs, opts=opts)


def _id(c):
    extra = "".join("-%s" % {"cache": "reencode"}.get(k, k) for k in sorted(c["opts"])) + ("-variable-n" if c["variable_n"] else "")
    if c["knobs"]["temperature"] == 0:
        extra += "-argmax"
    return "%s-%s-%s-P%d%s" % (c["precision"], c["attention"], _IDS[id(c["kw"])], c["P"], extra)


CASES = [case(p, "slot", A, P) for p in RS.SS.PRECISIONS for P in (1, 2, T - 1, T)]
CASES += [case(p, "slot", B_, 2) for p in RS.SS.PRECISIONS]
CASES += [case(p, "slot", A, 2, cache=False) for p in ("fp32", "bf16")]
for _cc in (False, True):           # per-clip attention: re-encoded without the option, the cached step with it
    _o = dict(clip_cache=True) if _cc else {}
    CASES += [case(p, "clip", A, P, **_o) for p in ("fp32", "bf16") for P in (1, T - 1)]
    CASES += [case(p, "clip", B2, P, variable_n=True, **_o) for p in ("fp32", "bf16") for P in (1, T - 1)]
CASES += [case(p, "factored", A, 2) for p in RS.SS.PRECISIONS]
CASES += [case(p, "factored", B2, 2, variable_n=True) for p in ("fp32", "bf16")]
CASES += [case(p, "slot", A, 2, gaussian=True, box_temperature=0.7) for p in ("fp32", "bf16")]
CASES += [case("fp32", "slot", A, 1, temperature=0.0, top_k=0)]
SAMPLE_CASES = [case("fp32", "slot", A, 2), case("bf16", "slot", A, 2), case("fp32", "factored", A, 2)]
K, SAMPLE0 = 3, 1


def build(dev, c, B=None):
    from vlg.engine import LayoutEngine
    from vlg.spec import LayoutConfig
    kw = dict(c["kw"], B=c["kw"]["B"] if B is None else B)
    cfg = LayoutConfig(attention=c["attention"], box_head="gaussian" if c["opts"].get("gaussian") else "point", **kw)
    eng = LayoutEngine(cfg, dev, seed=1024, precision=c["precision"], padded_slots=False, clip_cache=bool(c["opts"].get("clip_cache")))
    return cfg, eng


def contract(c, masked):
    return RS.GenContract(c["precision"], c["attention"], masked=masked, **c["opts"], **c["knobs"])


def run_case(dev, c, samples=None):
    t0 = time.time()
    cfg, eng = build(dev, c, B=None if samples is None else 2 * c["kw"]["B"])       # samples: room for exactly two samples' tokens
    cls0, box0 = prompt(c["kw"], c["variable_n"])
    P = c["P"]
    steps = T - P + 2
    pc, pb = cls0[:, :P].contiguous(), box0[:, :P].contiguous()
    kw = dict(steps=steps, cache=c["opts"].get("cache"), **c["knobs"])
    call = eng.rollout if samples is None else (lambda *a, **k: eng.rollout_samples(*a, samples=samples[0], sample0=samples[1], **k))
    plain = [t.clone() for t in call(pc.to(dev), pb.to(dev), return_logits=True, **kw)]
    records, state = rollout_trace.trace(eng, pc.to(dev), pb.to(dev), samples=None if samples is None else samples[0],
                                         sample0=0 if samples is None else samples[1], **kw)
    for a, b in zip(state["result"], plain):
        assert torch.equal(a, b), "the traced run is not bitwise the untraced one"
    if c["variable_n"]:
        assert eng._masked, "reserved ids in the prompt must switch the per-clip masks on"
    passes = None
    if samples is not None:
        from vlg.samples import sample_passes
        passes = sample_passes(samples[0], samples[1], pc.shape[0] * T * pc.shape[2], eng.capacity)
    log = []
    try:
        near, tokens = rollout_trace.check(records, state, cfg, contract(c, eng._masked), (pc, pb), passes=passes, log=log)
        print("\n%s: %d launches, %d of %d tokens inside the exclusion width" % (_id(c), len(records), near, tokens))
    finally:
        print("%s: worst error as a fraction of its bar, per launch kind: %s\n%s: %.2f s" % (
            _id(c), rollout_trace.summary(log), _id(c), time.time() - t0))
    return records, state, passes


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_every_launch_of_a_rollout_matches_fp64_on_its_inputs(dev, c):
    records, state, _ = run_case(dev, c)
    names = [r["name"] for r in records]
    L, P = c["kw"]["n_layers"], c["P"]
    assert len(records) == (1 + 7 * L + 2) * (T - P + 2)
    cached = P < T and c["opts"].get("cache") is not False and (c["attention"] != "clip" or c["opts"].get("clip_cache"))
    n_step = sum("_step" in n for n in names)
    assert n_step == (L * (T - P) if cached else 0), names
    sfx = "_ext" if c["opts"].get("gaussian") else ""
    assert names.count("vlg_layout_decode_append" + sfx) == T - P and names.count("vlg_layout_decode" + sfx) == 2
    for r in records:                       # the bf16 entry points only under bf16 storage (bf16_mfma: the fp32 kernels)
        if r["family"].startswith(("attn", "ln_")):
            assert r["name"].endswith("_bf16") == (c["precision"] == "bf16"), r["name"]


@pytest.mark.parametrize("c", SAMPLE_CASES, ids=_id)
def test_every_launch_of_a_sampled_rollout_matches_fp64_on_its_inputs(dev, c):
    """K = 3 futures from sample0 = 1 on an engine with room for two samples: passes (1, 2) and (3, 1), both through the _samples
    entries; check holds clips and sample0 of every decode launch to the pass and every frame to samples_ref on the logits it read"""
    records, state, passes = run_case(dev, c, samples=(K, SAMPLE0))
    assert passes == [(1, 2), (3, 1)] and [p["B"] for p in state["passes"]] == [2 * c["kw"]["B"], c["kw"]["B"]]
    dec = [r for r in records if r["family"] == "decode"]
    assert all(r["name"].endswith("_samples") and r["scalars"]["clips"] == c["kw"]["B"] for r in dec)
    assert {(r["pass"], r["scalars"]["sample0"]) for r in dec} == {(0, 1), (1, 3)}
    gen_c = state["result"][0]
    assert tuple(gen_c.shape) == (K, c["kw"]["B"], T - c["P"] + 2, c["kw"]["N"])
    for j, ps in enumerate(state["passes"]):             # the call's result is the concatenation of its passes, sample-major
        first = passes[j][0] - SAMPLE0
        assert torch.equal(gen_c[first:first + passes[j][1]].cpu().reshape(ps["gen_cls"].shape), ps["gen_cls"])


def test_per_clip_kinds_refuse_shape_b():
    """(3,4,23): T*N = 92 tokens per clip is no multiple of the 32-token tile; per-clip and factored configurations are refused,
    not run - their cases take (3,4,24)"""
    from vlg.spec import LayoutConfig
    for attention in ("clip", "factored"):
        with pytest.raises(ValueError, match="multiple of 32"):
            LayoutConfig(attention=attention, **B_).validate()
