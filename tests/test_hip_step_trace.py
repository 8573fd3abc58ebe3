"""GPU: every launch of one LayoutEngine.forward_backward against fp64 evaluated on the tensors that launch read.

The end-to-end bars of the reduced-precision modes cannot be tight (layer-norm gain gradients amplify one-ulp flips to
the size of the mode's whole effect), so the engine's COMPOSITION - which buffer feeds which launch, which weight copy,
which epilogue and storage flags, which saved tensor the backward reads - is checked here one launch at a time instead:
step_trace.trace records the launches of one step, step_trace.check holds each of them to the storage contract
("Layout step: storage contract of the reduced-precision modes") and to the project's per-kernel bars;
nothing amplifies.  No bar here is new or read off a GPU result: helpers.vs_cpu32, bitwise,
test_hip_layout_ops._loss_check and test_hip_gemm_paths.check_wgrad's bar.  One thing fp64 cannot decide is stated in
step_stages.flip_step: the on-chip bf16 rounding of a P / dS element of the bf16 per-clip attention that fp32 noise puts
on a rounding boundary.  Measured on the (2,16,12) fixed-N case before that was modelled: dq of layer 0 off by 1.7e-8
(largest |dq| 4.3e-4) where torch-CPU fp32, which drew no such element there, was off by 8.0e-10 - and by 2.2e-8 in
layer 1, where it drew some; all of the GPU's differences sit on the ~120 of 295 000 elements flip_step names.  tests/test_step_trace_cpu.py shows that these bars catch a stale buffer, a
missing rounding, a dropped bias / residual / mask and a short bias gradient at the stage where it happens.

Shapes are the smallest that take each path: (2,16,12) x d=256 x 2 layers - M = 384 is no multiple of 128, and a layer's
slab bucket rides in the next layer's paired launch; (1,32,8) x d=128 - the T = 32 attention kernels; (3,8,5) x d=64 -
the generic-T kernel, ragged everything (T*N = 40 is no multiple of 32, so the per-clip attention refuses this one:
asserted below).  The dropout step has cases of its own at the same shapes (DROP_CASES); attention = "factored" and the
other training options have theirs in tests/test_hip_step_trace_options.py.  VLG_OVERLAP_WGRAD=1 is not
traced: the synchronising wrapper would serialise it, and test_stream_options_do_not_change_results holds it bitwise to
the default."""
import pytest
import torch

import step_stages as SS
import step_trace
from oracle import layout_spec as O

pytestmark = pytest.mark.gpu

S1 = dict(B=2, T=16, N=12, d=256, n_layers=2)
S2 = dict(B=1, T=32, N=8, d=128, n_layers=1)
S3 = dict(B=3, T=8, N=5, d=64, n_layers=1)
_IDS = {id(S1): "2x16x12-d256-L2", id(S2): "1x32x8-d128-L1", id(S3): "3x8x5-d64-L1"}

CASES = []
for _prec in SS.PRECISIONS:
    for _att, _shapes in (("slot", (S1, S2, S3)), ("clip", (S1, S2))):
        CASES += [pytest.param(_prec, _att, _s, False, None, id="%s-%s-%s" % (_prec, _att, _IDS[id(_s)])) for _s in _shapes]
for _prec in ("fp32", "bf16"):        # padded slots (variable N, at least 3 valid): masks in the loss and, per clip, on the keys
    CASES += [pytest.param(_prec, _att, S1, True, None, id="%s-%s-variable-n" % (_prec, _att)) for _att in ("slot", "clip")]
CASES.append(pytest.param("bf16", "slot", S1, False, "0", id="bf16-slot-VLG_GELU_GRAD_SAVED-0"))
# per-clip attention on whole masked key tiles (tests/test_clip_walk_cpu.py has what each reaches): the production padding
# pattern - N = 64 with a prefix of <= 32 valid slots, the second half-frame tile all padded - and a clip whose first 32
# tokens (four leading frames) are padded, so that its queries meet a fully masked tile before they have seen a key
S4 = dict(B=2, T=4, N=64, d=64, n_layers=1)       # the smallest T a LayoutConfig takes
S5 = dict(B=2, T=8, N=8, d=64, n_layers=1)
for _prec in ("fp32", "bf16"):
    CASES += [pytest.param(_prec, "clip", S4, "prefix", None, id="%s-clip-2x4x64-prefix-valid" % _prec),
              pytest.param(_prec, "clip", S5, "lead-empty", None, id="%s-clip-2x8x8-lead-empty" % _prec)]


def _batch(cfg, variable_n):
    """variable_n False / True: oracle.synthetic_batch; "prefix": n_valid = 20 and 64 slots valid per clip; "lead-empty":
    frames 0-3 of clip 0 without objects.  Padded slots as synthetic_clips writes them: valid = 0, the reserved class id."""
    if not isinstance(variable_n, str):
        return O.synthetic_batch(cfg.B, cfg.T, cfg.N, seed=7, variable_n=variable_n, min_valid=3)
    batch = O.synthetic_batch(cfg.B, cfg.T, cfg.N, seed=7)
    valid = torch.ones(cfg.B, cfg.T, cfg.N)
    if variable_n == "prefix":
        valid[0, :, 20:] = 0.0
    else:
        valid[0, :4] = 0.0
    batch["valid"] = valid
    batch["slot_class"][valid == 0] = cfg.n_classes
    return batch


def _summary(log):
    worst = {}
    for stage, n, e_gpu, e_cpu in log:
        key = stage.split(".")[-1] + " " + n.split("[")[0].split(".")[-1]
        if e_gpu >= worst.get(key, (-1.0, 0.0))[0]:
            worst[key] = (e_gpu, e_cpu)
    return ", ".join("%s %.1e (cpu32 %.1e)" % (k, a, b) for k, (a, b) in sorted(worst.items()))


@pytest.mark.parametrize("precision,attention,kw,variable_n,gelu_saved", CASES)
def test_every_launch_matches_fp64_on_its_inputs(dev, monkeypatch, precision, attention, kw, variable_n, gelu_saved):
    from vlg.engine import LayoutEngine
    from vlg.spec import LayoutConfig
    if gelu_saved is not None:
        monkeypatch.setenv("VLG_GELU_GRAD_SAVED", gelu_saved)
    cfg = LayoutConfig(attention=attention, **kw)
    # fixed-N batches run the per-clip kernels without key masks (valid = NULL), variable-N ones with them
    eng = LayoutEngine(cfg, dev, precision=precision, padded_slots=bool(variable_n))
    c = SS.Contract(precision, attention, masked=bool(variable_n), gelu_grad_saved=None if gelu_saved is None else gelu_saved != "0")
    assert eng.gelu_grad_saved == c.gelu_grad_saved and eng.pair_backward == c.paired and eng.bf16_store == c.store_bf16
    batch = _batch(cfg, variable_n)
    if variable_n:
        assert bool((batch["valid"] == 0).any())
    b = {k: v.to(dev) for k, v in batch.items()}
    loss0 = eng.forward_backward(b).clone()
    grads0 = eng.grads.clone()
    records, state = step_trace.trace(eng, b)
    assert torch.equal(eng.loss_out, loss0) and torch.equal(eng.grads, grads0), "the traced run is not bitwise the untraced one"
    fams = [r["family"] for r in records]
    L = cfg.n_layers
    if precision in ("fp32", "bf16"):       # the paired backward; the head (N = 24) is never paired
        assert fams.count("gemm_pair") == 4 * L and fams.count("gemm_wgrad") == 0 and fams.count("gemm_dgrad") == 1, fams
    else:
        assert fams.count("gemm_pair") == 0 and fams.count("gemm_wgrad") == 4 * L and fams.count("gemm_dgrad") == 4 * L + 1, fams
    for r in records:                       # the bf16 entry points only under bf16 storage (bf16_mfma + clip: the fp32 kernels)
        if r["family"].startswith(("attn", "ln_")):
            assert r["name"].endswith("_bf16") == (precision == "bf16"), r["name"]
    log = []
    try:
        step_trace.check(records, state, cfg, c, batch, log=log)
    finally:
        print("\n%s %s %s: worst |err| vs fp64 per launch kind: %s" % (precision, attention, kw, _summary(log)))


# The dropout step (LayoutEngine._encode with drop and the `_dropped` backward; schedule: step_stages' module docstring) at
# p = 0.25 and counter k = 3 - a step at which test_hip_dropout documents the bf16 modes of its shape OUTSIDE the
# end-to-end bars; the per-launch bars hold regardless, nothing amplifies between launches.  Beyond the precisions: masks
# and dropout together (variable N), the plain backward (VLG_PAIR_BACKWARD=0 and fp32x3), the T = 32 attention with
# d = 128 and the generic-T attention with d = 64, where the mask takes the scalar row layout (one Philox call per element).
DROP_SEED = (0x9E3779B9 << 32) | 1024          # both key words in use
DROP_K = 3
DROP_CASES = [
    pytest.param("fp32", "slot", S1, False, 0.25, None, id="fp32-slot"),
    pytest.param("fp32", "clip", S1, True, 0.25, None, id="fp32-clip-variable-n"),
    pytest.param("fp32", "slot", S1, False, 0.5, "0", id="fp32-slot-p0.5-VLG_PAIR_BACKWARD-0"),
    pytest.param("fp32x3", "slot", S3, False, 0.25, None, id="fp32x3-slot-3x8x5-d64"),
    pytest.param("bf16", "slot", S1, False, 0.25, None, id="bf16-slot"),
    pytest.param("bf16", "slot", S2, False, 0.25, None, id="bf16-slot-1x32x8-d128"),
    pytest.param("bf16", "clip", S1, True, 0.25, None, id="bf16-clip-variable-n"),
    pytest.param("bf16_mfma", "slot", S1, False, 0.25, None, id="bf16_mfma-slot"),
]


@pytest.mark.parametrize("precision,attention,kw,variable_n,p,pair_env", DROP_CASES)
def test_every_launch_of_the_dropout_step_matches_fp64_on_its_inputs(dev, monkeypatch, precision, attention, kw, variable_n, p, pair_env):
    """As test_every_launch_matches_fp64_on_its_inputs, with dropout in the engine and in the contract: step_trace.check
    also holds every fused launch to the mask arguments and the counter value by name, to the reference's dropped set
    exactly, and x_out, h, mean, rstd / dx, ddrop to the bars of the plain layer-norm stages."""
    from vlg.engine import LayoutEngine
    from vlg.spec import LayoutConfig
    if pair_env is not None:
        monkeypatch.setenv("VLG_PAIR_BACKWARD", pair_env)
    cfg = LayoutConfig(attention=attention, **kw)
    eng = LayoutEngine(cfg, dev, precision=precision, padded_slots=bool(variable_n), dropout=p, dropout_seed=DROP_SEED)
    c = SS.Contract(precision, attention, masked=bool(variable_n), paired=None if pair_env is None else pair_env != "0",
                    dropout=(p, DROP_SEED, DROP_K))
    assert eng.gelu_grad_saved == c.gelu_grad_saved and eng.pair_backward == c.paired and eng.bf16_store == c.store_bf16
    batch = _batch(cfg, variable_n)
    if variable_n:
        assert bool((batch["valid"] == 0).any())
    b = {k: v.to(dev) for k, v in batch.items()}
    eng.set_dropout_step(DROP_K)
    loss0 = eng.forward_backward(b).clone()
    grads0 = eng.grads.clone()
    assert eng.dropout_step == DROP_K + 1
    eng.set_dropout_step(DROP_K)
    records, state = step_trace.trace(eng, b)
    assert torch.equal(eng.loss_out, loss0) and torch.equal(eng.grads, grads0), "the traced run is not bitwise the untraced one"
    names, fams = [r["name"] for r in records], [r["family"] for r in records]
    L = cfg.n_layers
    assert names.count("vlg_dropout_add_layernorm_fwd" + c.sfx) == 2 * L + 1 and not any(n.startswith("vlg_layernorm_fwd") for n in names)
    assert names.count("vlg_layernorm_bwd_dropout" + c.sfx) == 2 * L + 1
    assert "vlg_layernorm_bwd" not in names and "vlg_layernorm_bwd_bf16" not in names
    assert names.count("vlg_dropout_step_advance") == 1 and names[-1] == "vlg_dropout_step_advance"
    assert len(records) == len(SS.schedule(cfg, SS.Contract(precision, attention, masked=bool(variable_n), paired=c.paired))) + 1
    if c.paired:
        assert fams.count("gemm_pair") == 4 * L and fams.count("gemm_wgrad") == 0 and fams.count("gemm_dgrad") == 1, fams
    else:
        assert fams.count("gemm_pair") == 0 and fams.count("gemm_wgrad") == 4 * L and fams.count("gemm_dgrad") == 4 * L + 1, fams
    log = []
    try:
        step_trace.check(records, state, cfg, c, batch, log=log)
    finally:
        print("\n%s %s %s dropout p=%g k=%d: worst |err| vs fp64 per launch kind: %s" % (precision, attention, kw, p, DROP_K, _summary(log)))


def test_per_clip_attention_refuses_the_ragged_shape():
    """(3,8,5): T*N = 40 tokens per clip is no multiple of the 32-token tile; the configuration is refused, not run."""
    from vlg.spec import LayoutConfig
    with pytest.raises(ValueError, match="multiple of 32"):
        LayoutConfig(attention="clip", **S3).validate()
