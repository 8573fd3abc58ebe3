"""Adam over one flat fp32 buffer, for both engines (`FlatAdam`), and its guarded form (`OptimControl`): global-norm
gradient clipping, a step that is skipped when the gradient holds inf or NaN, and a learning rate that can change between
steps - decided on the device.

The guarded step is three stream-ordered launches around one 16-float device record (`ctl`, layout in include/vlg_hip.h):

    vlg_grad_sumsq     partial sums of grad^2 (one more read of the gradient buffer: 4 B / parameter)
    vlg_optim_control  one block: norm, clip coefficient, apply flag, step counter, bias-correction factors
    vlg_adam_step_ctl  Adam's arithmetic with its scalars read from ctl; returns at once when the step is skipped

Nothing is read back, so the step costs no host synchronisation and a captured hipGraph replays it unchanged; the
learning rate is an input slot of the record, so `set_lr` needs no recapture.  The host learns what happened only when it
asks (`read`, one 64-byte copy).  A non-finite norm ALWAYS skips the step here: whoever runs this path gets the guard.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import hip
from .hip import call, ptr
from .spec import ADAM_BETA2, ADAM_EPS

# slots of ctl (VLG_CTL_* in include/vlg_hip.h)
STEP_SIZE, SQRT_BC2, STEP, APPLY, GRAD_MULT, GRAD_NORM, LR, SKIPPED, CLIP_COEF, CTL_FLOATS = 0, 1, 2, 3, 4, 5, 6, 7, 8, 16


def decayed_lr(base_lr: float, epoch: int, decay_step: int, gamma: float) -> float:
    """Step decay: base_lr * gamma ** (epoch // decay_step), `epoch` 0-based (what the reference's --lr_decay_step /
    --lr_decay_gamma describe, src/main.py:142-145; its adjust_learning_rate was never called)."""
    if decay_step < 1:
        raise ValueError("lr_decay_step must be at least 1 epoch")
    return float(base_lr) * float(gamma) ** (int(epoch) // int(decay_step))


class OptimControl:
    """ctl and the partial-sum buffer for one flat gradient buffer of `n` floats (n % 4 == 0)."""

    def __init__(self, n: int, device: torch.device, lr: float, beta1: float, max_norm: float = 0.0, step: int = 0):
        lib = hip.load()
        self.n, self.beta1, self.max_norm = int(n), float(beta1), float(max_norm)
        self.n_partials = int(lib.vlg_grad_sumsq_blocks(self.n))
        self.partials = torch.zeros(self.n_partials, dtype=torch.float32, device=device)
        self.ctl = torch.zeros(CTL_FLOATS, dtype=torch.float32, device=device)
        self._ictl = self.ctl.view(torch.int32)
        self.ctl[CLIP_COEF] = 1.0
        self.set_lr(lr)
        self.set_counts(step, 0)

    def set_lr(self, lr: float) -> None:
        """One 4-byte host-to-device write, ordered on the current stream: legal between graph replays."""
        self.lr = float(lr)
        self.ctl[LR:LR + 1].copy_(torch.tensor([self.lr], dtype=torch.float32))

    def set_counts(self, step: int, skipped: Optional[int] = None) -> None:
        self._ictl[STEP:STEP + 1].copy_(torch.tensor([int(step)], dtype=torch.int32))
        if skipped is not None:
            self._ictl[SKIPPED:SKIPPED + 1].copy_(torch.tensor([int(skipped)], dtype=torch.int32))

    def read(self) -> Dict[str, float]:
        """One device-to-host copy of ctl (synchronises the stream)."""
        host = self.ctl.cpu()
        ints = host.view(torch.int32)
        return {"grad_norm": float(host[GRAD_NORM]), "clip_coef": float(host[CLIP_COEF]),
                "applied_steps": int(ints[STEP]), "skipped_steps": int(ints[SKIPPED]), "lr": float(host[LR])}

    def update(self, params: torch.Tensor, grads: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor,
               shadow: Optional[torch.Tensor], grad_scale: float, stream: int) -> None:
        """sumsq -> control -> Adam over the whole buffer."""
        if not (params.numel() == grads.numel() == exp_avg.numel() == exp_avg_sq.numel() == self.n):
            raise ValueError("guarded step was built for %d parameters" % self.n)
        call("vlg_grad_sumsq", ptr(grads), self.n, ptr(self.partials), stream)
        call("vlg_optim_control", ptr(self.ctl), ptr(self.partials), self.n_partials, float(grad_scale), self.max_norm,
             self.beta1, ADAM_BETA2, stream)
        call("vlg_adam_step_ctl", ptr(params), ptr(grads), ptr(exp_avg), ptr(exp_avg_sq), ptr(shadow), self.n,
             ptr(self.ctl), self.beta1, ADAM_BETA2, ADAM_EPS, stream)


class FlatAdam:
    """torch.optim.Adam(lr, betas=(beta1, 0.999)) over a flat buffer of `n` floats: the moments, and the one place that knows where
    the step count lives: the host (`step_count`), a 4-float device record (`adam_state`: {step_size, sqrt_bc2, step}, what a captured
    plain step needs), or GUARDED `guard.ctl`; a later form stays on.  `shadow`: the parameters' bf16 copy, refreshed by every update."""

    def __init__(self, n: int, device: torch.device, lr: float, beta1: float, clip_grad: float = 0.0,
                 skip_nonfinite: bool = False, shadow: Optional[torch.Tensor] = None):
        self.n, self.device, self.shadow = int(n), device, shadow
        self.lr, self.beta1 = float(lr), float(beta1)
        self.clip_grad, self.skip_nonfinite = max(float(clip_grad), 0.0), bool(skip_nonfinite)
        self.exp_avg = torch.zeros(self.n, dtype=torch.float32, device=device)
        self.exp_avg_sq = torch.zeros(self.n, dtype=torch.float32, device=device)
        self.step_count = 0
        self.adam_state: Optional[torch.Tensor] = None
        self.guard: Optional[OptimControl] = None    # guarded step: the optimiser's scalars live in its device record
        self.captured_plain = False                  # a captured graph holds the plain Adam launches (lr by value)
        if self.clip_grad > 0.0 or self.skip_nonfinite:
            self.enable_guard()

    @property
    def guarded(self) -> bool:
        return self.guard is not None

    def enable_guard(self) -> None:
        if self.guard is None:
            if self.captured_plain:
                raise RuntimeError("a step was captured with the plain optimiser (learning rate by value): build the engine "
                                   "with clip_grad / skip_nonfinite, or call set_lr, BEFORE capture_train_step")
            self.guard = OptimControl(self.n, self.device, self.lr, self.beta1, self.clip_grad, self.step_count)

    def use_device_counter(self) -> None:
        """Move the step counter (and its bias-correction factors) to device memory; the host count keeps mirroring it."""
        if self.adam_state is None:
            self.adam_state = torch.zeros(4, dtype=torch.float32, device=self.device)
            self.adam_state.view(torch.int32)[2] = int(self.step_count)

    def begin_capture(self) -> torch.Tensor:
        """The device tensor holding the optimiser's scalars in a captured step, to snapshot around the capture passes.  An
        unguarded optimiser moves its counter there and is latched plain: its captured launches carry lr by value."""
        if self.guard is not None:
            return self.guard.ctl
        self.use_device_counter()
        self.captured_plain = True
        return self.adam_state

    def set_lr(self, lr: float) -> None:
        """One 4-byte write into the device record the guarded step reads (no recapture needed).  Turns the guarded step on."""
        self.lr = float(lr)
        self.enable_guard()
        self.guard.set_lr(self.lr)

    def stats(self) -> Dict[str, float]:
        """{grad_norm, clip_coef, applied_steps, skipped_steps, lr}: one 64-byte copy that waits for the stream."""
        if self.guard is None:
            raise RuntimeError("optimizer_stats() needs the guarded step (clip_grad, skip_nonfinite or set_lr)")
        st = self.guard.read()
        self.step_count = st["applied_steps"]        # the device count is the authority: skipped steps do not advance it
        return st

    def applied_steps(self) -> int:
        return self.stats()["applied_steps"] if self.guard is not None else int(self.step_count)

    def set_step(self, step: int, skipped: Optional[int] = None) -> None:
        """the step count, wherever it lives (and, guarded, the skip count where given)"""
        self.step_count = int(step)
        if self.adam_state is not None:
            self.adam_state.view(torch.int32)[2] = self.step_count
        if self.guard is not None:
            self.guard.set_counts(self.step_count, skipped)

    def update_guarded(self, params: torch.Tensor, grads: torch.Tensor, grad_scale: float, stream: int) -> None:
        """Norm of grad_scale * grads (1 / world: of the MEAN gradient) -> control record -> Adam.  Turns the guard on."""
        self.enable_guard()
        self.guard.update(params, grads, self.exp_avg, self.exp_avg_sq, self.shadow, grad_scale, stream)

    def step(self, params: torch.Tensor, grads: torch.Tensor, grad_scale: float = 1.0, lo: int = 0, hi: Optional[int] = None,
             advance: bool = True, stream: int = 0, launch=None) -> None:
        """On the buffer or its [lo, hi) slice (multiples of 4); advance=False keeps the count (second slice of one step).
        `launch` (default hip.call) issues the plain fp32 launch: an engine with a kernel timer passes its bracketing caller."""
        hi = self.n if hi is None else hi
        if self.guard is not None:
            if lo != 0 or hi != self.n or not advance:
                raise ValueError("the guarded step updates the whole buffer at once (its norm needs every gradient)")
            self.update_guarded(params, grads, grad_scale, stream)
            return
        self.step_count += int(advance)
        o = 4 * lo
        p, g, m, v = params.data_ptr() + o, grads.data_ptr() + o, self.exp_avg.data_ptr() + o, self.exp_avg_sq.data_ptr() + o
        shadow = self.shadow.data_ptr() + o // 2 if self.shadow is not None else 0
        if self.adam_state is not None:          # captured / capturable step: the counter and its factors live on the device
            call("vlg_adam_step_graph", p, g, m, v, shadow, hi - lo, ptr(self.adam_state), 1 if advance else 0, self.lr,
                 self.beta1, ADAM_BETA2, ADAM_EPS, grad_scale, stream)
        elif self.shadow is not None:
            call("vlg_adam_step_bf16", p, g, m, v, shadow, hi - lo, self.step_count, self.lr, self.beta1, ADAM_BETA2,
                 ADAM_EPS, grad_scale, stream)
        else:
            (launch or call)("vlg_adam_step", p, g, m, v, hi - lo, self.step_count, self.lr, self.beta1, ADAM_BETA2,
                             ADAM_EPS, grad_scale, stream)

    def flat_state(self) -> Dict[str, object]:
        """Adam state as flat CPU tensors: {exp_avg, exp_avg_sq, step, lr, beta1, skipped}."""
        skipped = self.stats()["skipped_steps"] if self.guard is not None else 0     # (refreshes step_count)
        return {"exp_avg": self.exp_avg.cpu().clone(), "exp_avg_sq": self.exp_avg_sq.cpu().clone(),
                "step": int(self.step_count), "lr": self.lr, "beta1": self.beta1, "skipped": skipped}

    def load_flat_state(self, st: Dict[str, object]) -> None:
        """Guarded, also resumes lr and the skip count where recorded (older entries lack them); unguarded, keeps its own lr."""
        if st["exp_avg"].numel() != self.n or st["exp_avg_sq"].numel() != self.n:
            raise ValueError("optimizer state has %d elements, model has %d" % (st["exp_avg"].numel(), self.n))
        self.exp_avg.copy_(st["exp_avg"])
        self.exp_avg_sq.copy_(st["exp_avg_sq"])
        self.set_step(int(st["step"]), int(st.get("skipped", 0)))
        if self.guard is not None and st.get("lr") is not None:
            self.set_lr(float(st["lr"]))


def _passed(name: str) -> property:
    """engine attribute that IS its FlatAdam's (`engine.optim`): read and assigned through, never copied"""
    return property(lambda eng: getattr(eng.optim, name), lambda eng, value: setattr(eng.optim, name, value))


class AdamSurface:
    """What an engine that holds a FlatAdam as `self.optim` shows of it."""
    exp_avg, exp_avg_sq, step_count, lr, beta1, guard, adam_state, clip_grad, skip_nonfinite = (_passed(k) for k in (
        "exp_avg", "exp_avg_sq", "step_count", "lr", "beta1", "guard", "adam_state", "clip_grad", "skip_nonfinite"))
    guarded = property(lambda eng: eng.optim.guard is not None)

    def set_lr(self, lr: float) -> None:
        """New learning rate from the next step on, legal between replays of a captured step; turns the guarded step on."""
        self.optim.set_lr(lr)

    def optimizer_stats(self) -> Dict[str, float]:
        """{grad_norm, clip_coef, applied_steps, skipped_steps, lr} of the guarded step (waits for the stream)."""
        return self.optim.stats()

    def use_device_step_counter(self) -> None:
        """Move Adam's step counter to device memory, the form a captured step needs; `step_count` keeps mirroring it."""
        self.optim.use_device_counter()
