"""CPU: the training recipe on the guarded optimiser step - decoupled weight decay, warm-up in applied steps, the
weights' moving average.  The fp64 restatement the GPU tests compare the kernels with (optim_recipe_ref.py) is pinned to
torch.optim.AdamW here; then the decay-mask builder, knob parsing, and FlatAdam's host side driven through a stub in place
of the library (no kernel runs, nothing is loaded)."""
import contextlib
import math

import numpy as np
import pytest
import torch

import optim_recipe_ref as R
from helpers import OracleEngine, reference_args
from vlg import hip
from vlg.spec import LayoutConfig, param_layout

LR, B1, B2, EPS = 2e-4, 0.5, 0.999, 1e-8
WD, WARMUP, EMA_D, MAX_NORM = 0.1, 5, 0.5, 1.0
RECIPE_ENV = ("VLG_WEIGHT_DECAY", "VLG_WARMUP_STEPS", "VLG_EMA_DECAY", "VLG_EMA_WARMUP", "VLG_EMA_EVAL",
              "VLG_CLIP_GRAD", "VLG_SKIP_NONFINITE", "VLG_LR_DECAY")


# --------------------------------------------------------------------------------- the restatement against torch
def test_restatement_equals_torch_adamw_with_clip_warmup_and_ema():
    """10 applied steps (+ one with an inf gradient, at which nothing moves): torch.optim.AdamW in fp64 over two parameter
    groups (decay 0.1 / 0), clip_grad_norm_, warm-up by setting the groups' lr, and an EMA loop beside it.  Warm-up 5 leaves
    its ramp at step 5 and min(0.5, (1 + t) / (10 + t)) changes branch at step 8, both inside the 10 steps."""
    gen = torch.Generator().manual_seed(5)
    n_dec, n_no = 40, 24                                  # float4 multiples: the mask is per float4
    n = n_dec + n_no
    p0 = torch.randn(n, generator=gen, dtype=torch.float64)
    a = p0[:n_dec].clone().requires_grad_(True)
    b = p0[n_dec:].clone().requires_grad_(True)
    opt = torch.optim.AdamW([{"params": [a], "weight_decay": WD}, {"params": [b], "weight_decay": 0.0}], lr=LR,
                            betas=(B1, B2), eps=EPS)
    ema_t = p0.clone()
    mask4 = np.array([1] * (n_dec // 4) + [0] * (n_no // 4), dtype=np.uint8)
    p, m, v, ema = p0.numpy().copy(), np.zeros(n), np.zeros(n), p0.numpy().copy()
    state = {"step": 0, "skipped": 0}
    kw = dict(lr=LR, beta1=B1, beta2=B2, eps=EPS, max_norm=MAX_NORM, weight_decay=WD, warmup_steps=WARMUP, ema_decay=EMA_D,
              ema_warmup=True, mask4=mask4)
    branches, clipped = set(), set()
    t = 0
    for it in range(11):
        g = torch.randn(n, generator=gen, dtype=torch.float64) * (10.0 ** (it % 3 - 1))
        if it == 6:                                       # the skipped step: torch's side does nothing at all
            g[3] = float("inf")
            before = [x.copy() for x in (p, m, v, ema)]
            p, m, v, ema, state, info = R.recipe_step(p, g.numpy(), m, v, ema, state, **kw)
            assert not info["applied"] and state == {"step": t, "skipped": 1}
            assert all(np.array_equal(x, y) for x, y in zip((p, m, v, ema), before))
            continue
        t += 1
        a.grad, b.grad = g[:n_dec].clone(), g[n_dec:].clone()
        torch.nn.utils.clip_grad_norm_([a, b], MAX_NORM)
        for group in opt.param_groups:
            group["lr"] = LR * min(1.0, t / WARMUP)
        opt.step()
        d_t = min(EMA_D, (1 + t) / (10 + t))
        branches.add(d_t == EMA_D)
        now = torch.cat([a.detach(), b.detach()])
        ema_t = ema_t + (1 - d_t) * (now - ema_t)
        p, m, v, ema, state, info = R.recipe_step(p, g.numpy(), m, v, ema, state, **kw)
        clipped.add(info["clip_coef"] < 1.0)
        assert info["applied"] and state["step"] == t and info["lr_eff"] == LR * min(1.0, t / WARMUP)
        assert info["ema_decay_t"] == d_t
        np.testing.assert_allclose(p, now.numpy(), rtol=1e-12, atol=0.0, err_msg="parameters, step %d" % t)
        np.testing.assert_allclose(ema, ema_t.numpy(), rtol=1e-12, atol=0.0, err_msg="EMA, step %d" % t)
        np.testing.assert_allclose(m[:n_dec], opt.state[a]["exp_avg"].numpy(), rtol=1e-12, atol=0.0)
        np.testing.assert_allclose(v[n_dec:], opt.state[b]["exp_avg_sq"].numpy(), rtol=1e-12, atol=0.0)
    assert t == 10 and state == {"step": 10, "skipped": 1}
    assert branches == {True, False} and clipped == {True, False}
    assert (1 + 7) / (10 + 7) < EMA_D == (1 + 8) / (10 + 8)             # the branch changes at step 8


def test_restatement_without_the_recipe_is_plain_adam():
    gen = torch.Generator().manual_seed(6)
    n = 16
    p0 = torch.randn(n, generator=gen, dtype=torch.float64)
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=LR, betas=(B1, B2), eps=EPS)
    p, m, v, state = p0.numpy().copy(), np.zeros(n), np.zeros(n), {"step": 0, "skipped": 0}
    for _ in range(3):
        g = torch.randn(n, generator=gen, dtype=torch.float64)
        ref.grad = g.clone()
        opt.step()
        p, m, v, ema, state, info = R.recipe_step(p, g.numpy(), m, v, None, state, lr=LR, beta1=B1, beta2=B2, eps=EPS)
        assert ema is None and info["lr_eff"] == LR and info["decay_mult"] == 1.0
        np.testing.assert_allclose(p, ref.detach().numpy(), rtol=1e-12, atol=0.0)


# ------------------------------------------------------------------------------------------------ the decay mask
@pytest.mark.parametrize("d", [64, 256])
def test_layout_decay_mask_marks_exactly_the_weight_matrices(d):
    from vlg.optim import build_decay_mask, decays_matrix
    cfg = LayoutConfig(B=2, T=4, N=3, d=d, n_layers=2)
    layout, n = param_layout(cfg)
    mask = build_decay_mask(layout, n, decays_matrix)
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == (n // 4,) and n % 4 == 0
    want = torch.zeros(n // 4, dtype=torch.uint8)
    marked, unmarked = set(), set()
    for name, (off, shape) in layout.items():
        assert off % 4 == 0, name
        size = math.prod(shape)
        lo, hi = off // 4, (off + size + 3) // 4            # up to the tensor's 16-byte padding
        if name.endswith("_w"):
            want[lo:hi] = 1
            marked.add(name.split(".")[-1])
            assert bool(mask[lo:hi].all()), name
        else:
            unmarked.add(name.split(".")[-1])
            assert not bool(mask[lo:hi].any()), name
    assert torch.equal(mask, want)
    assert marked == {"qkv_w", "proj_w", "ff1_w", "ff2_w", "head_w", "box_w"}
    assert {"cls_emb", "time_emb", "qkv_b", "proj_b", "ff1_b", "ff2_b", "head_b", "box_b", "ln1_g", "ln1_b", "ln2_g", "ln2_b",
            "lnf_g", "lnf_b"} <= unmarked


def test_mask_builder_rounds_up_and_refuses_a_straddling_start():
    from vlg.optim import build_decay_mask, decay_mask_ranges
    layout = {"a_w": (0, (3, 2)), "a_b": (8, (3,)), "c_w": (12, (4,))}          # a_w: 6 floats, padded to 8
    assert build_decay_mask(layout, 16, lambda name: name.endswith("_w")).tolist() == [1, 1, 0, 1]
    assert decay_mask_ranges(16, []).tolist() == [0, 0, 0, 0]
    with pytest.raises(ValueError):
        decay_mask_ranges(16, [(2, 8)])
    with pytest.raises(ValueError):
        decay_mask_ranges(18, [])


# ------------------------------------------------------------------------------------------------------- knobs
@pytest.fixture
def workdir(tmp_path, monkeypatch):
    src = tmp_path / "src"
    src.mkdir()
    monkeypatch.chdir(src)
    for name in RECIPE_ENV:
        monkeypatch.delenv(name, raising=False)
    return tmp_path


def test_recipe_knobs_from_args_and_environment(workdir, monkeypatch):
    from trainer import optim_knobs, recipe_kwargs
    a = reference_args(workdir / "exp")
    off = optim_knobs(a)
    assert off == {"clip_grad": 0.0, "skip_nonfinite": False, "lr_decay": False} and recipe_kwargs(off) == {}
    monkeypatch.setenv("VLG_EMA_EVAL", "0")                 # not read while the average is off
    monkeypatch.setenv("VLG_EMA_WARMUP", "1")
    assert optim_knobs(a) == off
    monkeypatch.setenv("VLG_WEIGHT_DECAY", "0.1")
    monkeypatch.setenv("VLG_WARMUP_STEPS", "500")
    monkeypatch.setenv("VLG_EMA_DECAY", "0.999")
    k = optim_knobs(a)
    assert (k["weight_decay"], k["warmup_steps"], k["ema_decay"], k["ema_warmup"], k["ema_eval"]) == (0.1, 500, 0.999, True, False)
    assert recipe_kwargs(k) == {"weight_decay": 0.1, "warmup_steps": 500, "ema_decay": 0.999, "ema_warmup": True}
    monkeypatch.delenv("VLG_EMA_EVAL")
    monkeypatch.delenv("VLG_EMA_WARMUP")
    k = optim_knobs(a)
    assert k["ema_eval"] is True and k["ema_warmup"] is False
    b = reference_args(workdir / "exp", weight_decay=0.0, warmup_steps=7, ema_decay=0.5, ema_eval=0)   # args win
    k = optim_knobs(b)
    assert "weight_decay" not in k and k["warmup_steps"] == 7 and k["ema_decay"] == 0.5 and k["ema_eval"] is False
    for bad in (dict(ema_decay=1.0), dict(ema_decay=-0.1), dict(weight_decay=-1.0), dict(warmup_steps=-1)):
        with pytest.raises(ValueError):
            optim_knobs(reference_args(workdir / "exp", **bad))


def test_recipe_rule_is_stated_once_and_names_its_caller():
    """vlg.spec.recipe_options: what FlatAdam (keywords) and trainer.optim_knobs (environment variables) both call"""
    from vlg.spec import recipe_options
    assert recipe_options() == (0.0, 0, 0.0) and recipe_options(0.1, 500, 0.999) == (0.1, 500, 0.999)
    env = ("VLG_WEIGHT_DECAY", "VLG_WARMUP_STEPS", "VLG_EMA_DECAY")
    for bad in (dict(ema_decay=1.0), dict(ema_decay=-0.1), dict(ema_decay=float("nan")), dict(weight_decay=-1.0), dict(warmup_steps=-1)):
        with pytest.raises(ValueError, match="weight_decay and warmup_steps must be >= 0, ema_decay in"):
            recipe_options(**bad)
        with pytest.raises(ValueError, match="VLG_WEIGHT_DECAY and VLG_WARMUP_STEPS must be >= 0, VLG_EMA_DECAY in"):
            recipe_options(names=env, **bad)


# ----------------------------------------------------------------------------- FlatAdam's host side, on a stub
class _StubLib:
    def vlg_grad_sumsq_blocks(self, n):
        return 3


@pytest.fixture
def stub(monkeypatch):
    """vlg.optim with the library replaced: load() hands out a planner stub, call() records instead of launching"""
    from vlg import optim
    calls = []
    monkeypatch.setattr(optim.hip, "load", lambda: _StubLib())
    monkeypatch.setattr(optim, "call", lambda name, *a: calls.append((name, a)))
    return optim, calls


def test_flat_adam_with_every_knob_off_allocates_and_calls_nothing_new(stub):
    optim, calls = stub
    opt = optim.FlatAdam(16, torch.device("cpu"), LR, B1)
    assert opt.guard is None and opt.ema is None and opt.ema_shadow is None and opt.decay_mask is None and not opt.recipe
    guarded = optim.FlatAdam(16, torch.device("cpu"), LR, B1, clip_grad=1.0)
    assert guarded.guard is not None and guarded.guard.ext is None and guarded.ema is None and not guarded.recipe
    p, g = torch.zeros(16), torch.zeros(16)
    guarded.update_guarded(p, g, 1.0, 0)
    assert [c[0] for c in calls] == ["vlg_grad_sumsq", "vlg_optim_control", "vlg_adam_step_ctl"]
    assert guarded.adam_bytes() == 28.0 * 16
    opt.seed_ema(p)                                      # no average: nothing to seed, nothing raised
    for setter, arg in ((opt.set_weight_decay, 0.1), (opt.set_ema_decay, 0.9)):
        with pytest.raises(RuntimeError):
            setter(arg)


@pytest.mark.parametrize("knob", [dict(weight_decay=0.1), dict(warmup_steps=5), dict(ema_decay=0.5)])
def test_any_recipe_knob_turns_the_guard_on_and_routes_through_the_new_entry_points(stub, knob):
    optim, calls = stub
    mask = torch.ones(4, dtype=torch.uint8) if "weight_decay" in knob else None
    opt = optim.FlatAdam(16, torch.device("cpu"), LR, B1, decay_mask=mask, **knob)
    assert opt.guard is not None and opt.recipe and tuple(opt.guard.ext.shape) == (16,)
    assert (opt.ema is not None) == ("ema_decay" in knob) and (opt.decay_mask is not None) == ("weight_decay" in knob)
    opt.update_guarded(torch.zeros(16), torch.zeros(16), 1.0, 0)
    assert [c[0] for c in calls] == ["vlg_grad_sumsq", "vlg_optim_control_ext", "vlg_adamw_ema_step_ctl"]
    args = calls[-1][1]
    ema, ema_shadow, decay_mask = (args[hip.param_index("vlg_adamw_ema_step_ctl", p)] for p in ("ema", "ema_shadow", "decay_mask"))
    assert len(args) == 15 and (ema != 0) == ("ema_decay" in knob) and ema_shadow == 0 and (decay_mask != 0) == ("weight_decay" in knob)
    assert opt.adam_bytes() == 16 * (28.0 + (8.0 if "ema_decay" in knob else 0.0) + (0.25 if "weight_decay" in knob else 0.0))


def test_weight_decay_needs_a_mask_of_the_right_size(stub):
    optim, _ = stub
    for mask in (None, torch.ones(3, dtype=torch.uint8), torch.ones(4, dtype=torch.float32)):
        with pytest.raises(ValueError):
            optim.FlatAdam(16, torch.device("cpu"), LR, B1, weight_decay=0.1, decay_mask=mask)
    with pytest.raises(ValueError):
        optim.FlatAdam(16, torch.device("cpu"), LR, B1, ema_decay=1.0)


def test_ext_record_holds_the_inputs_and_the_setters_write_them(stub):
    optim, _ = stub
    opt = optim.FlatAdam(16, torch.device("cpu"), LR, B1, weight_decay=0.1, warmup_steps=5, ema_decay=0.5, ema_warmup=True,
                         decay_mask=torch.ones(4, dtype=torch.uint8), shadow=torch.zeros(16, dtype=torch.bfloat16), ema_shadow=True)
    ext, iext = opt.guard.ext, opt.guard.ext.view(torch.int32)
    assert float(ext[optim.EXT_WEIGHT_DECAY]) == float(np.float32(0.1)) and int(iext[optim.EXT_WARMUP_STEPS]) == 5
    assert float(ext[optim.EXT_EMA_DECAY]) == 0.5 and int(iext[optim.EXT_EMA_WARMUP]) == 1
    assert opt.ema_shadow is not None and opt.ema_shadow.dtype == torch.bfloat16
    assert opt.adam_bytes(4) == 4 * 40.25                # 30 B + 10 B with the average and its shadow + 0.25 B of mask
    opt.set_weight_decay(0.05)
    opt.set_warmup(9)
    opt.set_ema_decay(0.75, ema_warmup=False)
    assert float(ext[optim.EXT_WEIGHT_DECAY]) == float(np.float32(0.05)) and int(iext[optim.EXT_WARMUP_STEPS]) == 9
    assert float(ext[optim.EXT_EMA_DECAY]) == 0.75 and int(iext[optim.EXT_EMA_WARMUP]) == 0
    assert bool((ext[7:] == 0).all())                    # reserved slots stay as they were
    st = opt.stats()                                     # before any applied step: the inputs themselves
    assert st["lr_eff"] == st["lr"] and st["ema_decay_t"] == 0.75 and st["applied_steps"] == 0


def test_flat_state_carries_the_recipe_and_an_older_checkpoint_loads(stub):
    optim, _ = stub
    kw = dict(weight_decay=0.1, warmup_steps=5, ema_decay=0.5, ema_warmup=True, decay_mask=torch.ones(4, dtype=torch.uint8))
    opt = optim.FlatAdam(16, torch.device("cpu"), LR, B1, **kw)
    params = torch.arange(16, dtype=torch.float32)
    opt.seed_ema(params)
    opt.ema[3] = -1.0                                    # an average that has moved away from the parameters
    opt.exp_avg.fill_(0.25)
    opt.set_step(4, 1)
    st = opt.flat_state()
    assert {"exp_avg", "exp_avg_sq", "step", "lr", "beta1", "skipped", "ema", "weight_decay", "warmup_steps", "ema_decay",
            "ema_warmup"} == set(st)
    assert (st["weight_decay"], st["warmup_steps"], st["ema_decay"], st["ema_warmup"], st["step"], st["skipped"]) == (0.1, 5, 0.5, True, 4, 1)
    fresh = optim.FlatAdam(16, torch.device("cpu"), LR, B1, weight_decay=0.2, warmup_steps=1, ema_decay=0.9,
                           decay_mask=torch.ones(4, dtype=torch.uint8))
    fresh.seed_ema(params)
    fresh.load_flat_state(st)
    assert torch.equal(fresh.ema, opt.ema) and torch.equal(fresh.exp_avg, opt.exp_avg)
    assert (fresh.weight_decay, fresh.warmup_steps, fresh.ema_decay, fresh.ema_warmup) == (0.1, 5, 0.5, True)
    assert torch.equal(fresh.guard.ext[:4], opt.guard.ext[:4])
    # a checkpoint from before the recipe: loads, the average stays what the engine seeded it with, the knobs the engine's own
    old = {k: st[k] for k in ("exp_avg", "exp_avg_sq", "step", "lr", "beta1")}
    third = optim.FlatAdam(16, torch.device("cpu"), LR, B1, **kw)
    third.seed_ema(params)
    third.load_flat_state(old)
    assert torch.equal(third.ema, params) and torch.equal(third.exp_avg, opt.exp_avg) and third.step_count == 4
    assert (third.weight_decay, third.warmup_steps, third.ema_decay) == (0.1, 5, 0.5)
    # and an optimiser without the recipe ignores the new keys of a newer checkpoint
    plain = optim.FlatAdam(16, torch.device("cpu"), LR, B1)
    plain.load_flat_state(st)
    assert plain.ema is None and plain.guard is None and plain.step_count == 4


# ------------------------------------------------------------------------------- Trainer: where evaluation runs
SMALL = dict(batch_size=4, epochs=1, print_freq=1, n_frames=4, n_slots=8, d_model=64, n_layers=1, train_clips=8, val_clips=8)


class EmaOracleEngine(OracleEngine):
    """OracleEngine with the surface Trainer uses of the moving average: ema_weights() swaps the weights forward() reads."""

    def __init__(self, cfg, args):
        super().__init__(cfg, seed=int(args.seed), lr=float(args.lr), beta1=float(args.beta1))
        self.ema_flat = self.params * 0.5                # any weights that are not the live ones
        self.entered = 0

    @contextlib.contextmanager
    def ema_weights(self):
        live, self.params = self.params, self.ema_flat
        self.entered += 1
        try:
            yield self
        finally:
            self.params = live

    def ema_named_params(self):
        return {n: self._view(self.ema_flat, n) for n in self.layout}

    set_lr = staticmethod(lambda lr: None)

    def optimizer_stats(self):
        return {"grad_norm": 0.0, "clip_coef": 1.0, "applied_steps": 0, "skipped_steps": 0, "lr": self.lr}


def test_trainer_validates_on_the_average_unless_told_otherwise(workdir, monkeypatch):
    from trainer import Trainer
    losses = {}
    for name, env in (("off", {}), ("ema", {"VLG_EMA_DECAY": "0.9"}), ("live", {"VLG_EMA_DECAY": "0.9", "VLG_EMA_EVAL": "0"})):
        for k in RECIPE_ENV:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        tr = Trainer(reference_args(workdir / name, **SMALL), engine_factory=EmaOracleEngine)
        losses[name] = tr.validate()["loss"]
        assert tr.engine.entered == (1 if name == "ema" else 0)
        monkeypatch.chdir(workdir / "src")
        tr.save_checkpoint({"loss": losses[name]})
        ckpt = torch.load(workdir / "checkpoint" / "latest.pth", weights_only=True)
        assert ("gridnet_ema" in ckpt) == (name != "off")
        if name != "off":
            assert set(ckpt["gridnet_ema"]) == set(ckpt["gridnet"])
            assert torch.equal(ckpt["gridnet_ema"]["head_w"], ckpt["gridnet"]["head_w"] * 0.5)
    assert losses["off"] == losses["live"] != losses["ema"]
