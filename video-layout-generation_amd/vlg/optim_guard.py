"""The guarded optimiser step of both engines: global-norm gradient clipping, a step that is skipped when the gradient
holds inf or NaN, and a learning rate that can change between steps - decided on the device.

Three stream-ordered launches around one 16-float device record (`ctl`, layout in include/vlg_hip.h):

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
