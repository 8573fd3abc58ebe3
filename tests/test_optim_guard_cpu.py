"""CPU: the host side of the guarded optimiser step (global-norm clipping, non-finite skip, learning-rate decay): the
partial-sum planner, the decay formula, knob parsing, and the Trainer's use of set_lr / optimizer_stats / checkpoints,
driven with an oracle-backed double that restates the device record's rules (include/vlg_hip.h, VLG_CTL_*)."""
import logging
import math
import os

import pytest
import torch

from helpers import OracleEngine, reference_args
from oracle import layout_spec as O
from vlg.spec import ADAM_BETA2, ADAM_EPS

SMALL = dict(batch_size=4, epochs=2, print_freq=1, n_frames=4, n_slots=8, d_model=64, n_layers=1,
             train_clips=12, val_clips=8)


class GuardedOracleEngine(OracleEngine):
    """OracleEngine with LayoutEngine's guarded-step surface; `ctl` restates what vlg_optim_control keeps on the device."""

    def __init__(self, cfg, seed=1024, lr=2e-4, beta1=0.5, clip_grad=0.0, skip_nonfinite=False):
        super().__init__(cfg, seed=seed, lr=lr, beta1=beta1)
        self.clip_grad, self.ctl, self.lr_calls = float(clip_grad), None, []
        if clip_grad > 0 or skip_nonfinite:
            self._enable_guard()

    @property
    def guarded(self):
        return self.ctl is not None

    def _enable_guard(self):
        if self.ctl is None:
            self.ctl = {"step": self.step_count, "skipped": 0, "lr": self.lr, "grad_norm": 0.0, "clip_coef": 1.0}

    def set_lr(self, lr):
        self.lr = float(lr)
        self.lr_calls.append(self.lr)
        self._enable_guard()
        self.ctl["lr"] = self.lr

    def optimizer_stats(self):
        c = self.ctl
        self.step_count = c["step"]
        return {"grad_norm": c["grad_norm"], "clip_coef": c["clip_coef"], "applied_steps": c["step"],
                "skipped_steps": c["skipped"], "lr": c["lr"]}

    def optimizer_update(self, grad_scale=1.0):
        self._enable_guard()
        c = self.ctl
        norm = grad_scale * math.sqrt(float(self.grads.double().pow(2).sum()))
        c["grad_norm"] = norm
        if not math.isfinite(norm):
            c["skipped"] += 1
            return
        c["step"] += 1
        c["clip_coef"] = min(1.0, self.clip_grad / (norm + 1e-6)) if self.clip_grad > 0 else 1.0
        O.adam_step(self.params, self.grads * (grad_scale * c["clip_coef"]), self.exp_avg, self.exp_avg_sq, c["step"],
                    lr=c["lr"], beta1=self.beta1, beta2=ADAM_BETA2, eps=ADAM_EPS)
        self.step_count = c["step"]

    def train_step(self, batch, reducer=None):
        if self.ctl is None:
            return super().train_step(batch, reducer)
        loss = self.forward_backward(batch, reducer)
        if reducer is not None:
            reducer.wait()
        self.optimizer_update(reducer.grad_scale if reducer is not None else 1.0)
        return loss

    def optimizer_state(self):
        st = super().optimizer_state()
        st["skipped"] = self.ctl["skipped"] if self.ctl is not None else 0
        return st

    def load_optimizer(self, st):
        super().load_optimizer(st)
        if self.ctl is not None:
            self.ctl["step"], self.ctl["skipped"] = self.step_count, int(st.get("skipped", 0))
            if st.get("lr") is not None:
                self.set_lr(float(st["lr"]))


def guarded_factory(cfg, args):
    from trainer import optim_knobs
    k = optim_knobs(args)
    return GuardedOracleEngine(cfg, seed=int(args.seed), lr=float(args.lr), beta1=float(args.beta1),
                               clip_grad=k["clip_grad"], skip_nonfinite=k["skip_nonfinite"])


@pytest.fixture
def workdir(tmp_path, monkeypatch):
    src = tmp_path / "src"
    src.mkdir()
    monkeypatch.chdir(src)
    for name in ("VLG_CLIP_GRAD", "VLG_SKIP_NONFINITE", "VLG_LR_DECAY"):
        monkeypatch.delenv(name, raising=False)
    return tmp_path


def test_sumsq_planner_is_bounded_and_monotone():
    from vlg import hip
    lib = hip.load()
    ns = [4, 8, 1024, 1028, 4104, 1_000_004, 2_097_152, 2_097_156, 4_194_304, 1 << 28, (1 << 33) + 4]
    ps = [lib.vlg_grad_sumsq_blocks(n) for n in ns]
    assert all(1 <= p <= 2048 for p in ps), ps
    assert ps == sorted(ps) and ps[0] == 1 and ps[-1] == 2048, ps
    prev = 0
    for n in range(4, 3_000_000, 4 * 997):
        p = lib.vlg_grad_sumsq_blocks(n)
        assert 1 <= p <= 2048 and p >= prev, (n, p, prev)
        prev = p


def test_binding_lists_the_guarded_entry_points():
    from vlg import hip
    for name in ("vlg_grad_sumsq_blocks", "vlg_grad_sumsq", "vlg_optim_control", "vlg_adam_step_ctl"):
        assert name in hip.SIGNATURES
    assert hip.load().vlg_abi_version() == 1


def test_lr_decay_formula(workdir):
    from trainer import epoch_lr
    from vlg.optim_guard import decayed_lr
    args = reference_args(workdir / "exp", lr=2e-4, lr_decay_step=5, lr_decay_gamma=0.1)
    want = {0: 2e-4, 4: 2e-4, 5: 2e-5, 9: 2e-5, 10: 2e-6}
    for epoch, lr in want.items():
        assert epoch_lr(args, epoch) == pytest.approx(lr, rel=1e-12), epoch
        assert decayed_lr(2e-4, epoch, 5, 0.1) == epoch_lr(args, epoch)
    with pytest.raises(ValueError):
        decayed_lr(2e-4, 3, 0, 0.1)


def test_knobs_from_args_and_environment(workdir, monkeypatch):
    from trainer import optim_knobs
    a = reference_args(workdir / "exp")
    assert optim_knobs(a) == {"clip_grad": 0.0, "skip_nonfinite": False, "lr_decay": False}
    monkeypatch.setenv("VLG_CLIP_GRAD", "0.5")
    monkeypatch.setenv("VLG_SKIP_NONFINITE", "1")
    monkeypatch.setenv("VLG_LR_DECAY", "1")
    assert optim_knobs(a) == {"clip_grad": 0.5, "skip_nonfinite": True, "lr_decay": True}
    b = reference_args(workdir / "exp", clip_grad=2.5, skip_nonfinite=0)          # args win over the environment
    assert optim_knobs(b) == {"clip_grad": 2.5, "skip_nonfinite": False, "lr_decay": True}
    monkeypatch.setenv("VLG_LR_DECAY", "0")
    assert optim_knobs(b)["lr_decay"] is False


def test_trainer_sets_lr_per_epoch_only_with_decay(workdir, monkeypatch):
    from trainer import Trainer
    kw = dict(SMALL, lr_decay_step=1, lr_decay_gamma=0.5)
    tr = Trainer(reference_args(workdir / "exp", **kw), engine_factory=guarded_factory)
    for epoch in range(3):
        tr.set_epoch(epoch)
    assert tr.engine.lr_calls == [] and not tr.engine.guarded and not tr.guarded
    monkeypatch.setenv("VLG_LR_DECAY", "1")
    tr = Trainer(reference_args(workdir / "exp2", **kw), engine_factory=guarded_factory)
    assert tr.engine.guarded and tr.guarded
    for epoch in range(3):
        tr.set_epoch(epoch)
    assert tr.engine.lr_calls[-3:] == pytest.approx([2e-4, 1e-4, 5e-5], rel=1e-12)
    tr.train()
    assert tr.engine.optimizer_stats()["lr"] == pytest.approx(5e-5, rel=1e-12)


def test_log_line_and_scalars_gain_the_norm_only_when_guarded(workdir, caplog):
    from trainer import Trainer
    args = reference_args(workdir / "plain", **SMALL)
    tr = Trainer(args, engine_factory=guarded_factory)
    with caplog.at_level(logging.INFO):
        tr.set_epoch(0)
        tr.train()
    assert not any("grad_norm" in r.message for r in caplog.records)
    rows = open(os.path.join(args.path, "scalars.tsv")).read().splitlines()
    assert all(r.startswith("train/gen loss GAN") for r in rows) and len(rows) == 3
    caplog.clear()
    args = reference_args(workdir / "guarded", clip_grad=0.5, **SMALL)
    tr = Trainer(args, engine_factory=guarded_factory)
    with caplog.at_level(logging.INFO):
        tr.set_epoch(0)
        tr.train()
    lines = [r.message for r in caplog.records if "loss [" in r.message]
    assert len(lines) == 3 and all("grad_norm [" in m and "skipped [0]" in m for m in lines)
    rows = open(os.path.join(args.path, "scalars.tsv")).read().splitlines()
    assert sum(r.startswith("train/grad_norm") for r in rows) == 3 and sum(r.startswith("train/lr") for r in rows) == 3
    assert tr.engine.optimizer_stats()["clip_coef"] < 1.0          # loss weights 40/20/10: the first norms are far above 0.5


def test_checkpoint_resumes_lr_applied_steps_and_skips(workdir):
    from trainer import Trainer
    tr = Trainer(reference_args(workdir / "exp", skip_nonfinite=1, **SMALL), engine_factory=guarded_factory)
    tr.set_epoch(0)
    tr.train()                                               # 3 applied steps
    tr.engine.grads[5] = float("inf")
    keep = tr.engine.params.clone()
    tr.engine.optimizer_update()                             # skipped: nothing moves
    assert torch.equal(tr.engine.params, keep)
    tr.engine.set_lr(7e-5)
    st = tr.engine.optimizer_stats()
    assert (st["applied_steps"], st["skipped_steps"]) == (3, 1) and not math.isfinite(st["grad_norm"])
    tr.save_checkpoint({"loss": 1.0})
    ck = torch.load("../checkpoint/latest.pth", weights_only=True)
    assert ck["optimizer"]["step"] == 3 and ck["optimizer"]["skipped"] == 1 and ck["optimizer"]["lr"] == 7e-5
    tr2 = Trainer(reference_args(workdir / "exp2", skip_nonfinite=1, resume="../checkpoint/latest.pth", **SMALL),
                  engine_factory=guarded_factory)
    st2 = tr2.engine.optimizer_stats()
    assert (st2["applied_steps"], st2["skipped_steps"], st2["lr"]) == (3, 1, 7e-5)
    batch = next(iter(tr.train_loader))
    tr.engine.train_step(batch)
    tr2.engine.train_step(batch)
    assert torch.equal(tr2.engine.params, tr.engine.params)
    # an entry written before these fields existed still loads: the counts start from its step, the lr stays the engine's
    old = {k: v for k, v in ck["optimizer"].items() if k not in ("lr", "skipped")}
    torch.save(dict(ck, optimizer=old), "../checkpoint/old.pth")
    tr3 = Trainer(reference_args(workdir / "exp3", skip_nonfinite=1, resume="../checkpoint/old.pth", **SMALL),
                  engine_factory=guarded_factory)
    st3 = tr3.engine.optimizer_stats()
    assert (st3["applied_steps"], st3["skipped_steps"], st3["lr"]) == (3, 0, 2e-4)
    # ... and an unguarded run ignores the new fields, as before
    tr4 = Trainer(reference_args(workdir / "exp4", resume="../checkpoint/latest.pth", lr=1e-3, **SMALL),
                  engine_factory=guarded_factory)
    assert tr4.engine.step_count == 3 and tr4.engine.lr == 1e-3 and not tr4.engine.guarded
