"""fp64 restatement of one optimiser step with the training recipe (include/vlg_hip.h, VLG_EXT_*; vlg/optim.py):

    norm -> clip -> skip -> warm-up -> decay on masked elements -> Adam -> EMA

Arrays in, arrays out; no device, no library.  test_optim_recipe_cpu.py pins it to torch.optim.AdamW in fp64, the GPU tests
compare the kernels with it.  `state` is a dict {step, skipped}; nothing given is modified."""
import math

import numpy as np


def expand_mask(mask4, n):
    """one byte per float4 -> one bool per element"""
    mask4 = np.asarray(mask4)
    assert mask4.shape == (n // 4,) and n % 4 == 0
    return np.repeat(mask4 != 0, 4)


def scalars(step, lr, beta1, beta2, weight_decay=0.0, warmup_steps=0, ema_decay=0.0, ema_warmup=False):
    """The step's scalars, `step` = the 1-based count of the step being applied: {lr_eff, decay_mult, ema_decay_t, ema_omd,
    step_size, sqrt_bc2}, all Python doubles."""
    lr_eff = lr if warmup_steps == 0 else lr * min(1.0, step / warmup_steps)
    d_t = min(ema_decay, (1.0 + step) / (10.0 + step)) if ema_warmup else ema_decay
    return {"lr_eff": lr_eff, "decay_mult": 1.0 - lr_eff * weight_decay, "ema_decay_t": d_t, "ema_omd": 1.0 - d_t,
            "step_size": lr_eff / (1.0 - beta1 ** step), "sqrt_bc2": math.sqrt(1.0 - beta2 ** step)}


def recipe_step(p, g, m, v, ema, state, lr, beta1, beta2, eps, grad_scale=1.0, max_norm=0.0, weight_decay=0.0,
                warmup_steps=0, ema_decay=0.0, ema_warmup=False, mask4=None):
    """One step.  p, g, m, v: arrays of n values (read as fp64); ema: array or None; mask4: uint8[n / 4] or None.
    Returns (p, m, v, ema, state, info): new fp64 arrays, the new {step, skipped}, and info = {applied, grad_norm, clip_coef,
    grad_mult} plus, on an applied step, scalars()'s entries.  A non-finite norm returns the inputs' values unchanged, counts
    a skipped step and does not advance `step`."""
    p, g, m, v = (np.asarray(x, dtype=np.float64) for x in (p, g, m, v))
    ema = None if ema is None else np.asarray(ema, dtype=np.float64)
    norm = grad_scale * math.sqrt(float(np.sum(g * g)))
    if not math.isfinite(norm):
        return (p.copy(), m.copy(), v.copy(), None if ema is None else ema.copy(),
                {"step": state["step"], "skipped": state["skipped"] + 1}, {"applied": False, "grad_norm": norm})
    step = state["step"] + 1
    coef = min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0.0 else 1.0
    s = scalars(step, lr, beta1, beta2, weight_decay, warmup_steps, ema_decay, ema_warmup)
    gk = g * (grad_scale * coef)
    if mask4 is not None:
        p = np.where(expand_mask(mask4, p.size), p * s["decay_mult"], p)
    m = m + (1.0 - beta1) * (gk - m)
    v = v * beta2 + (1.0 - beta2) * gk * gk
    p = p - s["step_size"] * (m / (np.sqrt(v) / s["sqrt_bc2"] + eps))
    if ema is not None:
        ema = ema + s["ema_omd"] * (p - ema)
    info = dict(s, applied=True, grad_norm=norm, clip_coef=coef, grad_mult=grad_scale * coef)
    return p, m, v, ema, {"step": step, "skipped": state["skipped"]}, info
