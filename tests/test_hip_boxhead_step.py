"""GPU: the Gaussian box head in LayoutEngine at (2,4,8), d = 64, 2 layers - the step's NLL launch against
tests/boxhead_ref.py on the engine's own head outputs, the scale rows' weight gradient, the padding rows that never move,
the captured step, a short training run, the point-head engine beside it (same parameters and launches as ever), and
rollout() with drawn boxes."""
import pytest
import torch

import boxhead_ref as R
from helpers import check_close
from oracle import layout_spec as O

pytestmark = pytest.mark.gpu

C = 20
KW = dict(B=2, T=4, N=8, d=64, n_layers=2)
PRECISIONS = ("fp32", "fp32x3", "bf16", "bf16_mfma")
W_NLL = 0.5

# what one default train_step of the point-head engine at KW launches, in order (fp32): the list the engine had before the
# option existed.  forward: embedding, per layer  norm qkv attention proj norm ff1 ff2, final norm, head, loss;  backward: the
# head's weight and data gradient, final norm, per layer four paired projections with the attention and two norms between
# them (a finished bucket's reduction rides in the next paired launch), the embedding, the last table-driven reduction; Adam.
LAYER_FWD = ["vlg_layernorm_fwd", "vlg_linear_fwd", "vlg_attention_fwd", "vlg_linear_fwd", "vlg_layernorm_fwd", "vlg_linear_fwd",
             "vlg_linear_fwd"]
LAYER_BWD = ["vlg_linear_dgrad_wgrad", "vlg_linear_dgrad_wgrad", "vlg_layernorm_bwd", "vlg_linear_dgrad_wgrad", "vlg_attention_bwd",
             "vlg_linear_dgrad_wgrad", "vlg_layernorm_bwd"]
POINT_STEP = (["vlg_embed_fwd"] + LAYER_FWD * 2 + ["vlg_layernorm_fwd", "vlg_linear_fwd", "vlg_layout_loss"] +
              ["vlg_linear_wgrad", "vlg_linear_dgrad", "vlg_layernorm_bwd"] + LAYER_BWD * 2 +
              ["vlg_embed_bwd", "vlg_reduce_slabs_table", "vlg_adam_step"])


def engine(dev, box_head="gaussian", precision="fp32", **kw):
    from vlg.engine import LayoutEngine
    from vlg.spec import LayoutConfig
    return LayoutEngine(LayoutConfig(box_head=box_head, **KW), dev, seed=1024, precision=precision, **kw)


def batch_on(dev, seed=7):
    b = O.synthetic_batch(KW["B"], KW["T"], KW["N"], seed=seed, variable_n=True, min_valid=3)
    return b, {k: v.to(dev) for k, v in b.items()}


def launches(fn):
    from vlg import hip
    names = []
    previous, hip.tracer = hip.tracer, lambda name, args: names.append(name)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        hip.tracer = previous
    return names


@pytest.mark.parametrize("precision", PRECISIONS)
def test_forward_scalars_dout_and_scale_gradient(dev, precision):
    batch, b = batch_on(dev)
    eng = engine(dev, precision=precision, box_nll_weight=W_NLL)
    B, T, N = KW["B"], KW["T"], KW["N"]
    M = B * T * N
    assert eng.cfg.n_out == 32 and eng.grads_ext.numel() == eng.n_params + 8
    loss = eng.forward(b)
    assert tuple(loss.shape) == (8,)
    loss, out, dout = loss.cpu(), eng.out[:M].cpu(), eng.dout[:M].cpu()
    assert bool(torch.isfinite(loss).all()) and float(loss[6]) == 0.0 and float(loss[7]) == 0.0
    # the NLL launch against the restatement on the engine's OWN head outputs
    ref = R.box_nll_closed(out, batch["tgt_box"], batch["valid"], B, T, N, C, W_NLL)
    R.check_nll(dout[:, C + 4:C + 8], loss[4], loss[5], ref, "engine %s" % precision)
    assert bool((dout[:, C + 8:] == 0).all()) and bool(torch.isfinite(dout).all())
    total = O.W_REG * loss[1].double() + O.W_IOU * loss[2].double() + O.W_CE * loss[3].double() + W_NLL * loss[4].double()
    assert abs(float(loss[0]) - float(total)) <= 4 * 2.0 ** -23 * abs(float(total))
    assert 0.0 <= float(loss[5]) <= 1.0
    # the scale rows' weight gradient = dout[:, C+4:C+8]^T . xf - on the operands as the precision mode's products read them
    eng.backward(b)
    torch.cuda.synchronize()
    xf, dy = eng.xf[:M].float().cpu(), dout[:, C + 4:C + 8]
    if precision in ("bf16", "bf16_mfma"):
        xf, dy = xf.to(torch.bfloat16).float(), dy.to(torch.bfloat16).float()
    want = dy.double().t() @ xf.double()
    got = eng.named_grads()["head_w"][C + 4:C + 8].cpu()
    scale = max(float(want.abs().max()), 1e-30)             # (test_hip_gemm_paths.check_wgrad's bar, on values of order 1)
    check_close(got / scale, want / scale, rtol=1e-4, atol=1e-5, what="head_w scale rows, %s" % precision)
    # the bias gradient is the column sum of dout: of the fp32 values or, in the bf16 modes, possibly of the rounded operand
    # (each element within 2^-9 of itself)
    full = dout[:, C + 4:C + 8].double()
    slack = 2.0 ** -8 * float(full.abs().sum(0).max()) / scale if precision in ("bf16", "bf16_mfma") else 0.0
    check_close(eng.named_grads()["head_b"][C + 4:C + 8].cpu() / scale, full.sum(0) / scale, rtol=1e-4, atol=1e-5 + slack,
                what="head_b scale rows, %s" % precision)
    assert bool((eng.named_grads()["head_w"][C + 8:] == 0).all()) and bool((eng.named_grads()["head_b"][C + 8:] == 0).all())
    assert bool((got != 0).any())


@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_padding_rows_never_move(dev, precision, weight_decay):
    _, b = batch_on(dev)
    eng = engine(dev, precision=precision, weight_decay=weight_decay)
    first = eng.named_params()["head_w"][C + 4:C + 8].clone()
    assert bool((first == 0).all())
    for _ in range(5):
        eng.train_step(b)
    torch.cuda.synchronize()
    for t in (eng.named_params(), eng.named_grads()):
        assert bool((t["head_w"][C + 8:] == 0).all()) and bool((t["head_b"][C + 8:] == 0).all())
    assert bool((eng.named_params()["head_w"][C + 4:C + 8] != 0).any()), "the scale rows did not train"
    assert bool(torch.isfinite(eng.params).all())


def test_captured_step_replays_like_eager_steps(dev):
    """a captured step replayed 3 times == 3 eager steps, bitwise: parameters, moments and the 8 loss scalars"""
    _, b = batch_on(dev)
    eager = engine(dev)
    for _ in range(3):
        eager.train_step(b)
    want_loss = eager.loss_out.clone()
    graph = engine(dev)
    run = graph.capture_train_step(b)
    for _ in range(3):
        run(b)
    torch.cuda.synchronize()
    assert torch.equal(graph.params, eager.params) and torch.equal(graph.loss_out, want_loss) and want_loss.numel() == 8
    assert torch.equal(graph.exp_avg, eager.exp_avg) and float(want_loss[4]) != 0.0


def test_forty_steps_lower_the_nll(dev):
    _, b = batch_on(dev)
    eng = engine(dev, lr=1e-3)
    seen = []
    for _ in range(40):
        seen.append(eng.train_step(b)[4:6].clone())
    torch.cuda.synchronize()
    first, last = seen[0].cpu(), seen[-1].cpu()
    print("\nbox_nll %.4f -> %.4f, box_cover %.3f -> %.3f over 40 steps" % (float(first[0]), float(last[0]), float(first[1]), float(last[1])))
    assert float(last[0]) < float(first[0])


def test_point_head_engine_is_the_engine_it_was(dev):
    from vlg.spec import LayoutConfig, param_layout
    _, b = batch_on(dev)
    point, gauss = engine(dev, "point"), engine(dev)
    assert point.n_params == param_layout(LayoutConfig(**KW))[1] and point.cfg.n_out == 24 and point.grads_ext.numel() == point.n_params + 4
    assert gauss.n_params == point.n_params + 8 * KW["d"] + 8
    assert not hasattr(point, "box_nll_scratch") and tuple(point.forward(b).shape) == (4,)
    names = launches(lambda: point.train_step(b))
    assert names == POINT_STEP, names
    on = launches(lambda: gauss.train_step(b))
    assert on.count("vlg_layout_box_nll") == 1 and on[on.index("vlg_layout_loss") + 1] == "vlg_layout_box_nll"
    assert [n for n in on if n != "vlg_layout_box_nll"] == POINT_STEP
    # every tensor but the head's scale and padding rows starts as the point model's; a point checkpoint grows into it
    for name, t in point.named_params().items():
        g = gauss.named_params()[name]
        assert torch.equal(g[:t.shape[0]] if name.startswith("head_") else g, t), name
    with pytest.raises(ValueError, match="grow_box_head"):
        gauss.load_params({k: v.cpu() for k, v in point.named_params().items()})
    with pytest.raises(ValueError, match="grow_box_head"):
        gauss.load_state_dict(point.state_dict())
    from vlg.spec import grow_box_head
    gauss.load_params(grow_box_head({k: v.cpu() for k, v in point.named_params().items()}, gauss.cfg))
    with pytest.raises(ValueError):
        engine(dev, "point", box_nll_weight=0.5)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            engine(dev, box_nll_weight=bad)


def test_scheduled_sampling_pass_two_carries_the_nll(dev):
    _, b = batch_on(dev)
    eng = engine(dev, sched_sampling=1.0)
    names = launches(lambda: eng.train_step(b))
    assert names.count("vlg_layout_box_nll") == 1 and names.count("vlg_layout_mix_inputs") == 1
    assert names.index("vlg_layout_mix_inputs") < names.index("vlg_layout_box_nll")
    assert bool(torch.isfinite(eng.loss_out).all()) and bool(torch.isfinite(eng.grads).all()) and float(eng.loss_out[4]) != 0.0


def test_trainer_knobs_reach_the_engine_and_validate_reports_the_head(dev, tmp_path, monkeypatch):
    from helpers import reference_args
    from trainer import Trainer
    src = tmp_path / "src"
    src.mkdir()
    monkeypatch.chdir(src)
    for k in ("VLG_BOX_HEAD", "VLG_BOX_NLL_WEIGHT", "VLG_GEN_BOX_TEMPERATURE"):
        monkeypatch.delenv(k, raising=False)
    small = dict(batch_size=2, epochs=1, print_freq=1, n_frames=4, n_slots=8, d_model=64, n_layers=2, train_clips=4, val_clips=6)
    tr = Trainer(reference_args(tmp_path / "exp", box_head="gaussian", box_nll_weight=0.25, gen_box_temperature=1.0, **small))
    assert tr.cfg.box_head == "gaussian" and tr.engine.cfg.n_out == 32 and tr.engine.box_nll_weight == 0.25
    got = tr.validate()
    # the restatement on the engine's own outputs, size-weighted over the batches as validate() weights them
    nll = cover = clips = 0.0
    for batch in tr.val_loader:
        b = {k: v.to(dev) for k, v in batch.items()}
        batch = {k: v.cpu() for k, v in batch.items()}
        tr.engine.forward(b)
        B, T, N = batch["slot_class"].shape
        want = R.box_nll(tr.engine.out[:B * T * N].cpu(), batch["tgt_box"], batch["valid"], B, T, N, C)
        nll, cover, clips = nll + float(want[0]) * B, cover + float(want[1]) * B, clips + B
    assert got["box_nll"] == pytest.approx(nll / clips, rel=1e-5) and got["box_cover"] == pytest.approx(cover / clips, abs=1e-6)
    assert "loss" in got
    prompt = next(iter(tr.val_loader))
    a = tr.generate_sequence(prompt["slot_class"], prompt["slot_box"], steps=2)
    b = tr.generate_sequence(prompt["slot_class"], prompt["slot_box"], steps=2)
    assert torch.equal(a[1], b[1])
    tr.args.gen_box_temperature = 0.0
    assert not torch.equal(tr.generate_sequence(prompt["slot_class"], prompt["slot_box"], steps=2)[1], a[1])
    # without the knobs: the trainer and the engine they always were
    plain = Trainer(reference_args(tmp_path / "exp2", **small))
    assert plain.cfg.box_head == "point" and set(plain.validate()) == {"loss"}
    with pytest.raises(ValueError):
        Trainer(reference_args(tmp_path / "exp3", box_nll_weight=0.25, **small))


# --------------------------------------------------------------------------------------------------------------- rollout
def _prompt(dev, P, seed=3):
    g = torch.Generator().manual_seed(seed)
    cls = torch.randint(0, C, (KW["B"], P, KW["N"]), generator=g)
    return cls.to(dev), torch.rand(KW["B"], P, KW["N"], 4, generator=g).to(dev)


def test_rollout_draws_boxes(dev):
    eng, point = engine(dev), engine(dev, "point")
    T, steps = KW["T"], 3
    cls, box = _prompt(dev, T)
    names = launches(lambda: eng.rollout(cls, box, steps=steps))
    assert names.count("vlg_layout_decode_ext") == steps and "vlg_layout_decode" not in names
    pnames = launches(lambda: point.rollout(cls, box, steps=steps))
    assert pnames.count("vlg_layout_decode") == steps and not any(n.endswith("_ext") for n in pnames)
    # box_temperature = 0: the mean boxes
    c0, b0, logits = eng.rollout(cls, box, steps=steps, return_logits=True)
    assert tuple(logits.shape) == (steps, KW["B"] * KW["N"], 32)
    mean = torch.sigmoid(logits[:, :, C:C + 4].double()).view(steps, KW["B"], KW["N"], 4).permute(1, 0, 2, 3)
    check_close(b0, mean, rtol=0, atol=1e-6, what="mean boxes")
    # the same seed twice: equal bits; two seeds: other boxes and, at temperature 0, the same first-frame classes
    c1, b1, l1 = eng.rollout(cls, box, steps=steps, seed=5, box_temperature=1.0, return_logits=True)
    c2, b2 = eng.rollout(cls, box, steps=steps, seed=5, box_temperature=1.0)
    c3, b3 = eng.rollout(cls, box, steps=steps, seed=6, box_temperature=1.0)
    assert torch.equal(c1, c2) and torch.equal(b1, b2)
    assert not torch.equal(b1, b3) and not torch.equal(b1[:, 0], b3[:, 0])
    assert torch.equal(c1[:, 0], c3[:, 0]) and torch.equal(c1[:, 0], c0[:, 0])
    assert bool(((b1 >= 0) & (b1 <= 1)).all()) and not torch.equal(b1[:, 0], b0[:, 0])
    # the first frame against the restatement on the step's own rows
    want = R.sampled_boxes(l1[0].cpu(), C, 0, 1.0, 5).view(KW["B"], KW["N"], 4)
    err = float((b1[:, 0].cpu().double() - want).abs().max())
    print("\nrollout first frame: largest |box - reference| %.3g" % err)
    assert err <= R.box_bar(1.0)
    # a short prompt: cached and re-encoded grown steps give the same first frame bit for bit, and both draw
    cs, bs = _prompt(dev, 2)
    names = launches(lambda: eng.rollout(cs, bs, steps=4, seed=9, box_temperature=0.7))
    assert names.count("vlg_layout_decode_append_ext") == 2 and names.count("vlg_layout_decode_ext") == 2
    ca, ba = eng.rollout(cs, bs, steps=4, seed=9, box_temperature=0.7)
    cb, bb = eng.rollout(cs, bs, steps=4, seed=9, box_temperature=0.7, cache=False)
    assert torch.equal(ca[:, 0], cb[:, 0]) and torch.equal(ba[:, 0], bb[:, 0])
    _, bm = eng.rollout(cs, bs, steps=4, seed=9)
    assert not torch.equal(ba[:, 1], bm[:, 1])
    # refusals, before anything runs
    with pytest.raises(ValueError):
        point.rollout(cls, box, steps=steps, box_temperature=0.5)
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            eng.rollout(cls, box, steps=steps, box_temperature=bad)
    # evaluate_rollout passes it through
    g = torch.Generator().manual_seed(4)
    clip_c = torch.randint(0, C, (KW["B"], T + 2, KW["N"]), generator=g).to(dev)
    clip_b = torch.rand(KW["B"], T + 2, KW["N"], 4, generator=g).to(dev)
    _, _, gb_a, _ = eng.evaluate_rollout(clip_c, clip_b, return_logits=True, seed=5, box_temperature=1.0)
    _, _, gb_b, _ = eng.evaluate_rollout(clip_c, clip_b, return_logits=True, seed=5)
    assert not torch.equal(gb_a, gb_b)
    with pytest.raises(ValueError):
        point.evaluate_rollout(clip_c, clip_b, box_temperature=1.0)
