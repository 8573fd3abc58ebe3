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

The training recipe rides on the same three launches (`weight_decay`, `warmup_steps`, `ema_decay` of FlatAdam; all off by
default, and off nothing below is allocated or called): a second 16-float record `ext` (VLG_EXT_*) holds the decay, the
warm-up length and the EMA decay as inputs; vlg_optim_control_ext writes this step's effective learning rate, decay
multiplier and EMA weight into it, and vlg_adamw_ema_step_ctl applies decoupled weight decay (torch.optim.AdamW's order) to
the float4s a byte mask marks and keeps an exponential moving average of the weights (+ its bf16 copy).
"""
from __future__ import annotations

from typing import Callable, Dict, Mapping, Optional, Sequence, Tuple

import torch

from . import cabi, hip
from .hip import call, ptr
from .spec import ADAM_BETA2, ADAM_EPS, recipe_options

# slots of ctl (VLG_CTL_* in include/vlg_hip.h)
STEP_SIZE, SQRT_BC2, STEP, APPLY, GRAD_MULT, GRAD_NORM, LR, SKIPPED, CLIP_COEF, CTL_FLOATS = cabi.values(
    "VLG_CTL_", "STEP_SIZE", "SQRT_BC2", "STEP", "APPLY", "GRAD_MULT", "GRAD_NORM", "LR", "SKIPPED", "CLIP_COEF", "FLOATS")
# slots of ext (VLG_EXT_* in include/vlg_hip.h)
EXT_WEIGHT_DECAY, EXT_WARMUP_STEPS, EXT_EMA_DECAY, EXT_EMA_WARMUP, EXT_LR_EFF, EXT_DECAY_MULT, EXT_EMA_OMD, EXT_FLOATS = cabi.values(
    "VLG_EXT_", "WEIGHT_DECAY", "WARMUP_STEPS", "EMA_DECAY", "EMA_WARMUP", "LR_EFF", "DECAY_MULT", "EMA_OMD", "FLOATS")


def decay_mask_ranges(n: int, ranges: Sequence[Tuple[int, int]]) -> torch.Tensor:
    """uint8[n / 4] on the CPU, one byte per float4 of a flat buffer of `n` floats: 1 on every float4 that [lo, hi) of
    `ranges` touches (a range that ends inside a float4 marks it: the rest of it is the tensor's padding)."""
    if n % 4:
        raise ValueError("the flat buffer must hold a multiple of 4 floats")
    mask = torch.zeros(n // 4, dtype=torch.uint8)
    for lo, hi in ranges:
        if lo % 4 or not 0 <= lo <= hi <= n:
            raise ValueError("range [%d, %d) must start on a float4 inside the buffer of %d floats" % (lo, hi, n))
        mask[lo // 4:(hi + 3) // 4] = 1
    return mask


def build_decay_mask(layout: Mapping[str, Tuple[int, Sequence[int]]], n: int, decays: Callable[[str], bool]) -> torch.Tensor:
    """The decay mask of a name -> (offset, shape) layout: the float4s of every tensor `decays(name)` accepts.  Offsets are
    multiples of 4 floats, so no float4 belongs to two tensors.  Pure Python: needs neither the library nor a device."""
    ranges = []
    for name, (off, shape) in layout.items():
        if decays(name):
            size = 1
            for s in shape:
                size *= int(s)
            ranges.append((int(off), int(off) + size))
    return decay_mask_ranges(n, ranges)


def decays_matrix(name: str) -> bool:
    """LayoutEngine's rule: the weight matrices (names ending in _w), not biases, layer-norm gains or embedding tables"""
    return name.endswith("_w")


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
        self.ext: Optional[torch.Tensor] = None      # the recipe's record: enable_ext

    def enable_ext(self, weight_decay: float = 0.0, warmup_steps: int = 0, ema_decay: float = 0.0, ema_warmup: bool = False) -> None:
        """Allocate `ext` and route update() through vlg_optim_control_ext / vlg_adamw_ema_step_ctl."""
        if self.ext is None:
            self.ext = torch.zeros(EXT_FLOATS, dtype=torch.float32, device=self.ctl.device)
            self._iext = self.ext.view(torch.int32)
            self.ext[EXT_DECAY_MULT] = 1.0
            self.ext[EXT_EMA_OMD] = 1.0
        self.set_ext(weight_decay, warmup_steps, ema_decay, ema_warmup)

    def set_ext(self, weight_decay: Optional[float] = None, warmup_steps: Optional[int] = None, ema_decay: Optional[float] = None,
                ema_warmup: Optional[bool] = None) -> None:
        """4-byte host-to-device writes into the input slots of ext, ordered on the current stream: legal between replays."""
        if weight_decay is not None:
            self.weight_decay = float(weight_decay)
            self.ext[EXT_WEIGHT_DECAY:EXT_WEIGHT_DECAY + 1].copy_(torch.tensor([self.weight_decay], dtype=torch.float32))
        if warmup_steps is not None:
            self.warmup_steps = int(warmup_steps)
            self._iext[EXT_WARMUP_STEPS:EXT_WARMUP_STEPS + 1].copy_(torch.tensor([self.warmup_steps], dtype=torch.int32))
        if ema_decay is not None:
            self.ema_decay = float(ema_decay)
            self.ext[EXT_EMA_DECAY:EXT_EMA_DECAY + 1].copy_(torch.tensor([self.ema_decay], dtype=torch.float32))
        if ema_warmup is not None:
            self.ema_warmup = bool(ema_warmup)
            self._iext[EXT_EMA_WARMUP:EXT_EMA_WARMUP + 1].copy_(torch.tensor([int(self.ema_warmup)], dtype=torch.int32))

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
        out = {"grad_norm": float(host[GRAD_NORM]), "clip_coef": float(host[CLIP_COEF]),
               "applied_steps": int(ints[STEP]), "skipped_steps": int(ints[SKIPPED]), "lr": float(host[LR])}
        if self.ext is not None:                     # (a second 64-byte copy; before the first applied step: lr and the decay itself)
            ext = self.ext.cpu()
            applied = out["applied_steps"] > 0
            out["lr_eff"] = float(ext[EXT_LR_EFF]) if applied else out["lr"]
            out["ema_decay_t"] = 1.0 - float(ext[EXT_EMA_OMD]) if applied else float(ext[EXT_EMA_DECAY])
        return out

    def update(self, params: torch.Tensor, grads: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor,
               shadow: Optional[torch.Tensor], grad_scale: float, stream: int, ema: Optional[torch.Tensor] = None,
               ema_shadow: Optional[torch.Tensor] = None, decay_mask: Optional[torch.Tensor] = None, launch=None) -> None:
        """sumsq -> control -> Adam over the whole buffer; with `ext`, the recipe's two entry points instead of the last two.
        `launch` (default hip.call) issues the Adam launch: an engine with a kernel timer passes its bracketing caller."""
        if not (params.numel() == grads.numel() == exp_avg.numel() == exp_avg_sq.numel() == self.n):
            raise ValueError("guarded step was built for %d parameters" % self.n)
        call("vlg_grad_sumsq", ptr(grads), self.n, ptr(self.partials), stream)
        if self.ext is not None:
            call("vlg_optim_control_ext", ptr(self.ctl), ptr(self.ext), ptr(self.partials), self.n_partials, float(grad_scale),
                 self.max_norm, self.beta1, ADAM_BETA2, stream)
            (launch or call)("vlg_adamw_ema_step_ctl", ptr(params), ptr(grads), ptr(exp_avg), ptr(exp_avg_sq), ptr(shadow), ptr(ema),
                             ptr(ema_shadow), ptr(decay_mask), self.n, ptr(self.ctl), ptr(self.ext), self.beta1, ADAM_BETA2,
                             ADAM_EPS, stream)
            return
        call("vlg_optim_control", ptr(self.ctl), ptr(self.partials), self.n_partials, float(grad_scale), self.max_norm,
             self.beta1, ADAM_BETA2, stream)
        (launch or call)("vlg_adam_step_ctl", ptr(params), ptr(grads), ptr(exp_avg), ptr(exp_avg_sq), ptr(shadow), self.n,
                         ptr(self.ctl), self.beta1, ADAM_BETA2, ADAM_EPS, stream)


class FlatAdam:
    """torch.optim.Adam(lr, betas=(beta1, 0.999)) over a flat buffer of `n` floats: the moments, and the one place that knows where
    the step count lives: the host (`step_count`), a 4-float device record (`adam_state`: {step_size, sqrt_bc2, step}, what a captured
    plain step needs), or GUARDED `guard.ctl`; a later form stays on.  `shadow`: the parameters' bf16 copy, refreshed by every update.
    The recipe (module docstring): weight_decay on the float4s `decay_mask` (uint8[n / 4], CPU or device) marks, warmup_steps of
    linear warm-up in applied steps, ema_decay > 0 keeps `ema` (fp32, and `ema_shadow` in bf16 where asked) - any of the three
    non-zero turns the guarded step on and routes it through the recipe's entry points; all off, nothing of it exists.  The
    average starts from the parameters: whoever fills them calls `seed_ema` (the engines do, in their load methods)."""

    def __init__(self, n: int, device: torch.device, lr: float, beta1: float, clip_grad: float = 0.0,
                 skip_nonfinite: bool = False, shadow: Optional[torch.Tensor] = None, weight_decay: float = 0.0,
                 warmup_steps: int = 0, ema_decay: float = 0.0, ema_warmup: bool = False,
                 decay_mask: Optional[torch.Tensor] = None, ema_shadow: bool = False):
        self.n, self.device, self.shadow = int(n), device, shadow
        self.weight_decay, self.warmup_steps, self.ema_decay = recipe_options(weight_decay, warmup_steps, ema_decay)
        self.ema_warmup = bool(ema_warmup)
        self.ema: Optional[torch.Tensor] = None
        self.ema_shadow: Optional[torch.Tensor] = None
        self.decay_mask: Optional[torch.Tensor] = None
        self._want_ema_shadow = bool(ema_shadow)
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
        if self.weight_decay > 0.0 or self.warmup_steps > 0 or self.ema_decay > 0.0:
            if self.weight_decay > 0.0:
                if decay_mask is None or decay_mask.numel() != self.n // 4 or decay_mask.dtype != torch.uint8:
                    raise ValueError("weight_decay needs decay_mask: uint8[%d], one byte per float4" % (self.n // 4))
                self.decay_mask = decay_mask.to(device).contiguous()
            self.enable_recipe()

    @property
    def guarded(self) -> bool:
        return self.guard is not None

    @property
    def recipe(self) -> bool:
        return self.guard is not None and self.guard.ext is not None

    def enable_recipe(self) -> None:
        """Turn the guarded step on and give it `ext`; with an EMA decay, allocate the average (zero until seed_ema)."""
        self.enable_guard()
        if self.guard.ext is None:
            self.guard.enable_ext(self.weight_decay, self.warmup_steps, self.ema_decay, self.ema_warmup)
        if self.ema_decay > 0.0 and self.ema is None:
            self.ema = torch.zeros(self.n, dtype=torch.float32, device=self.device)
            if self._want_ema_shadow:
                self.ema_shadow = torch.zeros(self.n, dtype=torch.bfloat16, device=self.device)

    def seed_ema(self, params: torch.Tensor) -> None:
        """the average (and its bf16 copy, rounded to nearest even as the kernel rounds) := the parameters"""
        if self.ema is not None:
            self.ema.copy_(params)
            if self.ema_shadow is not None:
                self.ema_shadow.copy_(self.ema)

    def set_weight_decay(self, weight_decay: float) -> None:
        """One 4-byte write into ext, legal between graph replays (the mask is fixed at construction)."""
        if self.decay_mask is None and float(weight_decay) != 0.0:
            raise RuntimeError("build the optimiser with weight_decay > 0 (it owns the decay mask) before changing the decay")
        self.weight_decay = float(weight_decay)
        self.enable_recipe()
        self.guard.set_ext(weight_decay=self.weight_decay)

    def set_warmup(self, warmup_steps: int) -> None:
        """One 4-byte write into ext, legal between graph replays; turns the recipe's step on."""
        self.warmup_steps = int(warmup_steps)
        self.enable_recipe()
        self.guard.set_ext(warmup_steps=self.warmup_steps)

    def set_ema_decay(self, ema_decay: float, ema_warmup: Optional[bool] = None) -> None:
        """4-byte writes into ext, legal between graph replays.  The average must exist (ema_decay > 0 at construction)."""
        if self.ema is None:
            raise RuntimeError("build the optimiser with ema_decay > 0 (it owns the average) before changing the decay")
        self.ema_decay = float(ema_decay)
        self.ema_warmup = self.ema_warmup if ema_warmup is None else bool(ema_warmup)
        self.guard.set_ext(ema_decay=self.ema_decay, ema_warmup=self.ema_warmup)

    def enable_guard(self) -> None:
        if self.guard is None:
            if self.captured_plain:
                raise RuntimeError("a step was captured with the plain optimiser (learning rate by value): build the engine "
                                   "with clip_grad / skip_nonfinite, or call set_lr, BEFORE capture_train_step")
            self.guard = OptimControl(self.n, self.device, self.lr, self.beta1, self.clip_grad, self.step_count)

    def adam_bytes(self, n: Optional[int] = None) -> float:
        """Algorithmic bytes of the Adam launch over `n` parameters: 16 B read + 12 B written (+ 2 B shadow), + 4 + 4 (+ 2) B
        with the average, + 0.25 B with the decay mask."""
        per = 28.0 + (2.0 if self.shadow is not None else 0.0)
        if self.ema is not None:
            per += 8.0 + (2.0 if self.ema_shadow is not None else 0.0)
        if self.decay_mask is not None:
            per += 0.25
        return per * (self.n if n is None else n)

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
        """{grad_norm, clip_coef, applied_steps, skipped_steps, lr} (+ lr_eff, ema_decay_t of the last applied step with the
        recipe on): one 64-byte copy per record that waits for the stream."""
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

    def update_guarded(self, params: torch.Tensor, grads: torch.Tensor, grad_scale: float, stream: int, launch=None) -> None:
        """Norm of grad_scale * grads (1 / world: of the MEAN gradient) -> control record -> Adam.  Turns the guard on."""
        self.enable_guard()
        self.guard.update(params, grads, self.exp_avg, self.exp_avg_sq, self.shadow, grad_scale, stream, self.ema,
                          self.ema_shadow, self.decay_mask, launch)

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
        """Adam state as flat CPU tensors: {exp_avg, exp_avg_sq, step, lr, beta1, skipped}; with the recipe on also
        {weight_decay, warmup_steps, ema_decay, ema_warmup} and, where there is an average, `ema`."""
        skipped = self.stats()["skipped_steps"] if self.guard is not None else 0     # (refreshes step_count)
        st = {"exp_avg": self.exp_avg.cpu().clone(), "exp_avg_sq": self.exp_avg_sq.cpu().clone(),
              "step": int(self.step_count), "lr": self.lr, "beta1": self.beta1, "skipped": skipped}
        if self.recipe:
            st.update(weight_decay=self.weight_decay, warmup_steps=self.warmup_steps, ema_decay=self.ema_decay,
                      ema_warmup=self.ema_warmup)
            if self.ema is not None:
                st["ema"] = self.ema.cpu().clone()
        return st

    def load_flat_state(self, st: Dict[str, object]) -> None:
        """Guarded, also resumes lr and the skip count where recorded (older entries lack them); unguarded, keeps its own lr.
        With the recipe on, takes the recorded decay, warm-up and EMA scalars and the average; an entry without an average
        leaves it as the engine seeded it (from the loaded parameters)."""
        if st["exp_avg"].numel() != self.n or st["exp_avg_sq"].numel() != self.n:
            raise ValueError("optimizer state has %d elements, model has %d" % (st["exp_avg"].numel(), self.n))
        self.exp_avg.copy_(st["exp_avg"])
        self.exp_avg_sq.copy_(st["exp_avg_sq"])
        self.set_step(int(st["step"]), int(st.get("skipped", 0)))
        if self.guard is not None and st.get("lr") is not None:
            self.set_lr(float(st["lr"]))
        if self.recipe:
            if st.get("weight_decay") is not None and (self.decay_mask is not None or float(st["weight_decay"]) == 0.0):
                self.set_weight_decay(float(st["weight_decay"]))
            if st.get("warmup_steps") is not None:
                self.set_warmup(int(st["warmup_steps"]))
            if self.ema is not None:
                if st.get("ema_decay"):
                    self.set_ema_decay(float(st["ema_decay"]), st.get("ema_warmup"))
                if st.get("ema") is not None:
                    if st["ema"].numel() != self.n:
                        raise ValueError("optimizer state's average has %d elements, model has %d" % (st["ema"].numel(), self.n))
                    self.ema.copy_(st["ema"])
                    if self.ema_shadow is not None:
                        self.ema_shadow.copy_(self.ema)


def _passed(name: str) -> property:
    """engine attribute that IS its FlatAdam's (`engine.optim`): read and assigned through, never copied"""
    return property(lambda eng: getattr(eng.optim, name), lambda eng, value: setattr(eng.optim, name, value))


class AdamSurface:
    """What an engine that holds a FlatAdam as `self.optim` shows of it."""
    exp_avg, exp_avg_sq, step_count, lr, beta1, guard, adam_state, clip_grad, skip_nonfinite = (_passed(k) for k in (
        "exp_avg", "exp_avg_sq", "step_count", "lr", "beta1", "guard", "adam_state", "clip_grad", "skip_nonfinite"))
    guarded = property(lambda eng: eng.optim.guard is not None)
    ema = property(lambda eng: eng.optim.ema)
    ema_shadow = property(lambda eng: eng.optim.ema_shadow)

    def set_lr(self, lr: float) -> None:
        """New learning rate from the next step on, legal between replays of a captured step; turns the guarded step on."""
        self.optim.set_lr(lr)

    def set_weight_decay(self, weight_decay: float) -> None:
        self.optim.set_weight_decay(weight_decay)

    def set_warmup(self, warmup_steps: int) -> None:
        self.optim.set_warmup(warmup_steps)

    def set_ema_decay(self, ema_decay: float, ema_warmup: Optional[bool] = None) -> None:
        self.optim.set_ema_decay(ema_decay, ema_warmup)

    def optimizer_stats(self) -> Dict[str, float]:
        """{grad_norm, clip_coef, applied_steps, skipped_steps, lr} of the guarded step, + {lr_eff, ema_decay_t} with the
        recipe on (waits for the stream)."""
        return self.optim.stats()

    def use_device_step_counter(self) -> None:
        """Move Adam's step counter to device memory, the form a captured step needs; `step_count` keeps mirroring it."""
        self.optim.use_device_counter()
