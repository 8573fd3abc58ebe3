"""Hand-scheduled training step of the layout-token model on one MI355X.

No autograd, no tracing compiler: forward and backward are explicit sequences of
launches of the gfx950 kernels in libvlg_hip.so on the caller's HIP stream, over
buffers allocated once (parameters, gradients and Adam moments are single flat
fp32 buffers; activations live in a preallocated workspace sized for the largest
batch).  PyTorch supplies device memory and streams only.

Step order mirrors the reference's Trainer.train() body (reference
src/trainer.py:209-258): forward -> weighted loss (40/20/10) -> backward ->
[gradient all-reduce by the caller] -> Adam.  Gradients are overwritten every
step, i.e. the zero_grad() the reference forgot is implied.

A transformer layer is written once per direction.  Forward: LayoutEngine._encode, the walk that forward(), the training
forward with dropout and the cached generation step all take - they differ in the buffer set, the attention launch and
whether the residual sums form in a GEMM epilogue or in the fused dropout norm.  Backward: the loop in backward(), whose
projection step is one paired call or a weight gradient (on the side stream, with VLG_OVERLAP_WGRAD=1) and a data gradient.

Row order of every (M, .) activation is the internal  m = (b*N + n)*T + t.
"""
from __future__ import annotations

import contextlib
import ctypes
import dataclasses
import functools
import math
import os
import types
from typing import Dict, Optional

import torch

from . import hip
from .attention import MODES, cached_by_default, layer_kinds, lse_rows
from .metrics import MetricsRecord
from .raster import MAX_SLOTS, WHATS, PixelRecord, raster_options
from .samples import COLS as SMP_COLS, CRITERIA, SampleRecord, sample_passes, samples_options, select_option
from .optim import AdamSurface, FlatAdam, build_decay_mask, decays_matrix
from .slabs import SlabBuckets
from .hip import (EPI_A_BF16, EPI_B_BF16, EPI_BIAS, EPI_DGELU, EPI_GELU, EPI_NONE, EPI_OUT_BF16, EPI_RESID,
                  call, ptr)
from .spec import (ADAM_BETA1, ADAM_BETA2, ADAM_EPS, ADAM_LR, BOX_DIM, IOU_EPS, LN_EPS, LOSS_W_CE,
                   LOSS_W_REG, LOSS_W_STRUCT, SMOOTH_L1_BETA, LayoutConfig, decode_options, dropout_options, loss_options,
                   augment_options, param_layout, sched_options, BOX_HEAD_EXTRA, BOX_S_MAX, BOX_S_MIN, box_options,
                   box_temperature_options)

# the int32 device step counters: checkpoint key (= the advance launch's timer family, = the property that reads it) -> the
# option an engine needs to have one
STEP_COUNTERS = {"dropout_step": "dropout > 0", "sched_step": "sched_sampling", "augment_step": "an aug_* option"}


def init_params(cfg: LayoutConfig, seed: int) -> Dict[str, torch.Tensor]:
    """Deterministic CPU initialisation (one generator, tensors in flat-buffer order).

    Embedding tables ~ N(0,1) (nn.Embedding default, reference src/models/simple.py:23),
    projections ~ U(+-1/sqrt(fan_in)) for weight and bias (nn.Linear default),
    layer-norm gain 1 / bias 0.  Every rank uses the same seed, as the reference does
    (src/main.py:57-60), so replicas start identical without a broadcast.
    """
    layout, _ = param_layout(cfg)
    g = torch.Generator().manual_seed(seed)
    fan_in = {name[:-2] + "_b": shape[1] for name, (_, shape) in layout.items() if name.endswith("_w")}
    out: Dict[str, torch.Tensor] = {}
    for name, (_, shape) in layout.items():
        base = name.split(".")[-1]
        grown = cfg.gaussian_box and name in ("head_w", "head_b")
        if grown:                                        # draw the point head's rows, in its order and shapes; append below
            shape = (shape[0] - BOX_HEAD_EXTRA,) + tuple(shape[1:])
        if base in ("cls_emb", "time_emb"):
            t = torch.randn(shape, generator=g, dtype=torch.float32)
        elif base.endswith("_g"):
            t = torch.ones(shape)
        elif base.startswith("ln") and base.endswith("_b"):
            t = torch.zeros(shape)
        elif base.endswith("_w"):
            t = (torch.rand(shape, generator=g, dtype=torch.float32) * 2 - 1) * (1.0 / math.sqrt(shape[1]))
        else:
            t = (torch.rand(shape, generator=g, dtype=torch.float32) * 2 - 1) * (1.0 / math.sqrt(fan_in[name]))
        if grown:       # the scale and padding rows start at zero: sigma = exp((BOX_S_MIN + BOX_S_MAX) / 2); the padding rows stay there
            t = torch.cat([t, t.new_zeros((BOX_HEAD_EXTRA,) + tuple(shape[1:]))], dim=0)
        out[name] = t
    return out


def grow_schedule(P: int, T: int, steps: int, cached: bool) -> list:
    """What each of a rollout's `steps` generated frames does, from a prompt of P frames in a T-frame window: a list of
    (encoder, t_read, pos).  encoder: "window" = the encoder on all T frames of the window buffer, "step" = the cached step
    on the newest frame's rows alone; t_read: the window position whose output predicts the frame (the newest real frame);
    pos: the position the new frame is appended at in place, or None once the window is full and slides instead.
    The history grows while P + i < T; the step at P + i == T reads position T-1 and is the first to slide."""
    if not 1 <= P <= T or steps < 1:
        raise ValueError("grow_schedule takes 1 <= P <= T and steps >= 1")
    out = []
    for i in range(steps):
        h = min(P + i, T)                                # frames of history the step predicts from
        out.append(("step" if cached and 0 < i and P + i <= T else "window", h - 1, h if h < T else None))
    return out


class LayoutEngine(AdamSurface):
    """Owns parameters, optimiser state and workspace; runs forward/backward/Adam."""

    def __init__(self, cfg: LayoutConfig, device: torch.device, seed: int = 1024,
                 lr: float = ADAM_LR, beta1: float = ADAM_BETA1, precision: str = "fp32", padded_slots: bool = True,
                 clip_grad: float = 0.0, skip_nonfinite: bool = False, weight_decay: float = 0.0, warmup_steps: int = 0,
                 ema_decay: float = 0.0, ema_warmup: bool = False, dropout: float = 0.0, dropout_seed: int = 0,
                 clip_cache: bool = False, class_weights=None, label_smoothing: float = 0.0, box_overlap: str = "iou",
                 sched_sampling: Optional[float] = None, sched_ramp_steps: int = 0, sched_temperature: float = 0.0,
                 sched_top_k: int = 0, sched_seed: int = 0, aug_flip: Optional[float] = None, aug_zoom: Optional[float] = None,
                 aug_shift: Optional[float] = None, aug_jitter: Optional[float] = None, aug_drop: Optional[float] = None,
                 aug_seed: int = 0, box_nll_weight: float = 1.0):
        """clip_grad > 0 clips the gradient to that global L2 norm (torch.nn.utils.clip_grad_norm_'s rule); skip_nonfinite
        leaves parameters, moments and step count untouched when the gradient holds inf or NaN.  Either one - or a call
        of set_lr - turns on the GUARDED optimiser step (vlg/optim.py), eager and captured alike; with both off and
        set_lr never called, the step's launches are exactly those of an engine without these options.
        The recipe (FlatAdam in vlg/optim.py says what each does, vlg.spec.recipe_options what is legal; each off at 0, any of
        them turns the guarded step on): weight_decay falls on the weight matrices - every tensor whose name ends in _w; not
        biases, layer-norm gains and biases, cls_emb or time_emb; warmup_steps; ema_decay / ema_warmup, the weights' moving
        average (in the bf16 mode with its own bf16 copy): `with engine.ema_weights():` evaluates and generates on it.
        precision:
        "fp32"      exact-fp32 MFMA projections, every tensor fp32 (parity 1e-4);
        "bf16"      BASELINE.json configs[2]: bf16 MFMA projections (fp32 accumulate) AND the activations that only
                    feed projections / attention (normalised inputs, q k v, attention output, FFN hidden and their
                    gradients) stored as bf16 in HBM - the mode is HBM-bound, so the bytes are what count;
        "bf16_mfma" bf16 MFMA projections with every tensor still fp32 in HBM (operands rounded on their way to LDS);
        "fp32x3"    fp32 tensors and fp32-grade projections on the bf16 matrix cores: every operand split exactly into
                    three bf16 terms, six bf16 MFMAs per product block (csrc/gemm_split.hip).
        The residual stream and its gradient, layer-norm statistics, softmax, losses, weight gradients, Adam and the
        master weights are fp32 in all three.  Every attention kind (vlg/attention.py) follows the storage: its bf16 entry
        points under "bf16" (per clip: bf16 MFMA, fp32 scores and softmax statistics), the fp32 kernels otherwise (bf16_mfma
        included); cfg.attention changes the per-layer attention launch and nothing else in the step.
        dropout = p in [0, 1) (0 = off: nothing allocated, no launch changed): inverted dropout on the embedding and on
        the two residual branches of every layer (2L + 1 sites; rule and sites: include/vlg_hip.h, "dropout"), fused into
        the step's layer-norm launches.  Only forward_backward / train_step / capture_train_step apply it; a bare
        forward(), rollout(), evaluate_rollout(), accumulate_metrics() and everything under ema_weights() stay
        evaluation.  The mask is a stateless Philox function of (row, column, site, step) under dropout_seed; the step is a
        device counter (dropout_step / set_dropout_step) advanced once per training forward+backward, whether or not the
        guarded optimiser then skips.  Not combined with VLG_OVERLAP_WGRAD=1.
        clip_cache = True (off by default; it matters with attention = "clip" alone): rollout()'s grown frames take the
        K/V-cached step with per-clip attention too (rollout's docstring).
        Loss options (DESIGN.md "Loss options"; legal values: vlg.spec.loss_options; all off by default, and then the step
        launches vlg_layout_loss as ever; with any of them on, vlg_layout_loss_ext in its place - one launch either way):
        class_weights = the weight= of F.cross_entropy (uploaded once; the CE mean then divides by the summed weight of the
        valid targets, per rank under data parallelism); label_smoothing = its label_smoothing=; box_overlap = "giou" makes
        the overlap term mean(1 - GIoU), which has a gradient for boxes that do not touch.
        Fixed at construction; checkpoints do not carry them.  forward() - validation included - returns this configured
        objective; accumulate_metrics / evaluate_rollout keep reporting the plain NLL and IoU.
        Scheduled sampling (DESIGN.md "Scheduled sampling"; rule: include/vlg_hip.h; legal values: vlg.spec.sched_options):
        sched_sampling = None is off - nothing allocated, no launch changed; a float eps_max turns it on.  forward_backward /
        train_step / capture_train_step then run PASS 1 and the mix (_mix_inputs), which replaces each input token of a frame
        t >= 1 that is not padded with the model's own decoded prediction of it (class by the decoding rule of rollout()
        under sched_temperature / sched_top_k, box = sigmoid(raw)) with probability eps_max - ramped linearly over the first
        sched_ramp_steps training steps when that is > 0 - and PASS 2, the training step as ever on the mixed inputs and the
        TRUE targets; no gradient flows through the replaced inputs.  Coins and draws are stateless Philox functions of
        (token, step) under sched_seed; the step is a device counter of its own (sched_step / set_sched_step), advanced as
        dropout's is.  sched_inputs() shows the last training step's mixed inputs.  Whatever evaluates is untouched.
        Augmentation (DESIGN.md "Augmentation"; rule: include/vlg_hip.h; legal values: vlg.spec.augment_options): with aug_flip,
        aug_zoom, aug_shift, aug_jitter and aug_drop all None it is off - nothing allocated, no launch changed; any of them
        given, 0.0 included, turns it on and the missing ones count as 0.  forward_backward / train_step / capture_train_step
        then FIRST build the batch they train on in engine-owned buffers (_augment, one launch; the caller's tensors are only
        read): per clip a flip with probability aug_flip, a zoom about the centre by 1 +- aug_zoom and a shift by +- aug_shift
        of the image, per input token a box jitter of +- aug_jitter, per track a drop with probability aug_drop, which pads the
        track's inputs and takes its targets out of the loss.  Scheduled sampling then runs both passes on that batch.  Draws
        are stateless Philox functions of (clip | track | token, step) under aug_seed; the step is a device counter of its own
        (augment_step / set_augment_step).  augmented_batch() shows the last training step's batch.  Whatever evaluates is
        untouched.  aug_drop > 0 needs padded_slots = True with a per-clip attention kind: their unmasked kernels would
        attend to the dropped slots.
        Gaussian box head (DESIGN.md "Gaussian box head"; rule: include/vlg_hip.h; legal values: vlg.spec.box_options): it is the
        MODEL's option, LayoutConfig(box_head="gaussian") - with "point" nothing is allocated and no launch changes.  The head
        then predicts four per-coordinate scales beside the four means (n_out = n_classes + 12), one vlg_layout_box_nll launch
        follows the loss launch of every forward - training, validation, captured, scheduled sampling's pass 2 - and adds
        box_nll_weight times the Gaussian negative log-likelihood of the target box to the total; its gradient reaches the scale
        outputs only (the mean is detached).  forward() then returns 8 scalars {total, smooth_l1, iou, ce, box_nll, box_cover,
        0, 0}, and rollout() / evaluate_rollout() take box_temperature to DRAW boxes.  box_nll_weight other than 1.0 is legal only
        with that head."""
        cfg.validate()
        self.box_nll_weight = box_options(cfg.box_head, box_nll_weight)[1]
        given = (aug_flip, aug_zoom, aug_shift, aug_jitter, aug_drop)
        self._aug = None if all(v is None for v in given) else augment_options(*given) + (int(aug_seed) & 0xFFFFFFFFFFFFFFFF,)
        self._sched = None if sched_sampling is None else sched_options(    # (the option rules: vlg/spec.py, the trainer's *_knobs call them too)
            sched_sampling, sched_ramp_steps, sched_temperature, sched_top_k, cfg.n_classes) + (int(sched_seed) & 0xFFFFFFFFFFFFFFFF,)
        weights, self.label_smoothing, self.box_overlap = loss_options(class_weights, label_smoothing, box_overlap, cfg.n_classes)
        self.clip_cache = bool(clip_cache)
        self.dropout = dropout_options(dropout)
        # vlg/attention.py: every layer's attention kind and lse row; of the mode as a whole, whether a layer takes `valid` and
        # whether a short prompt's grown frames have a cached step
        self.attn = layer_kinds(cfg.attention, cfg.n_layers)
        self._lse_row, self._per_clip = lse_rows(self.attn), any(k.per_clip for k in MODES[cfg.attention])
        self._cacheable = self.clip_cache or cached_by_default(cfg.attention)
        if self.dropout > 0.0 and os.environ.get("VLG_OVERLAP_WGRAD", "0") == "1":
            raise ValueError("VLG_OVERLAP_WGRAD=1 together with dropout=%g is not supported: the side stream's hazard "
                             "tracking does not cover the dropout gradient buffer" % self.dropout)
        if precision not in ("fp32", "bf16", "bf16_mfma", "fp32x3"):
            raise ValueError("precision must be fp32, fp32x3, bf16 or bf16_mfma")
        # attention = "clip": padded slots (batch['valid'] == 0) must not be attended to; padded_slots = False tells the engine
        # that its batches never hold any (fixed-N feeds), so the kernels skip the per-key validity masks
        self.padded_slots = bool(padded_slots)
        self._masked = self.padded_slots             # this forward's choice; its backward follows it
        if self._aug is not None and self._aug[4] > 0.0 and self._per_clip and not self.padded_slots:
            raise ValueError("aug_drop=%g with attention=%r needs padded_slots=True: the unmasked per-clip kernels would attend "
                             "to the dropped slots" % (self._aug[4], cfg.attention))
        self.precision = precision
        self.gemm_flags = {"fp32": 0, "fp32x3": hip.EPI_SPLIT3}.get(precision, hip.EPI_BF16)
        self.bf16_store = precision == "bf16"
        # native fp32 and the bf16 modes: the FFN's first projection stores gelu'(u) in the pre-activation buffer instead of u (VLG_EPI_GELU_GRAD;
        # nothing else reads u) and the second projection's data gradient multiplies by it (VLG_EPI_MUL): ~20 vector
        # instructions per element less in a kernel that pays for each of them in matrix time (csrc/common.h)
        self.gelu_grad_saved = precision in ("fp32", "bf16", "bf16_mfma") and os.environ.get("VLG_GELU_GRAD_SAVED", "1") != "0"
        self._epi_ff1 = EPI_BIAS | EPI_GELU | (hip.EPI_GELU_GRAD if self.gelu_grad_saved else 0)
        self._epi_dff2 = hip.EPI_MUL if self.gelu_grad_saved else EPI_DGELU
        self._sfx = "_bf16" if self.bf16_store else ""
        hip.load()                                   # fail loudly before touching the GPU
        if device.type != "cuda":
            raise hip.HipError("LayoutEngine needs a HIP device (got %s); there is no CPU path" % device)
        self.cfg, self.device = cfg, device
        self._counters: Dict[str, torch.Tensor] = {}     # STEP_COUNTERS key -> the counter, for the options that are on
        # dropout: (thr, scale, seed) for the kernels + the device step counter, or None with the knob off
        self._drop, self._dropped = None, False
        if self.dropout > 0.0:
            thr, scale = ctypes.c_uint32(), ctypes.c_float()
            hip.check(hip.load().vlg_dropout_plan(self.dropout, ctypes.byref(thr), ctypes.byref(scale)), "vlg_dropout_plan")
            self._drop = (thr.value, scale.value, int(dropout_seed) & 0xFFFFFFFFFFFFFFFF)
            self._counters["dropout_step"] = torch.zeros(1, dtype=torch.int32, device=device)
        # scheduled sampling: (thr_max, ramp_steps, temperature, top_k, seed) for the mix kernel + its own device step counter
        if self._sched is not None:
            thr = ctypes.c_uint32()
            hip.check(hip.load().vlg_sched_plan(self._sched[0], ctypes.byref(thr)), "vlg_sched_plan")
            self._sched = (thr.value,) + self._sched[1:]
            self._counters["sched_step"] = torch.zeros(1, dtype=torch.int32, device=device)
        # augmentation: (thr_flip, zoom, shift, jitter, thr_drop, seed) for the augment kernel + its own device step counter
        if self._aug is not None:
            thr = [ctypes.c_uint32(), ctypes.c_uint32()]
            for t, p in zip(thr, (self._aug[0], self._aug[4])):
                hip.check(hip.load().vlg_augment_plan(p, ctypes.byref(t)), "vlg_augment_plan")
            self._aug = (thr[0].value,) + self._aug[1:4] + (thr[1].value, self._aug[5])
            self._counters["augment_step"] = torch.zeros(1, dtype=torch.int32, device=device)
        self.drop_step, self.sched_counter = self._counters.get("dropout_step"), self._counters.get("sched_step")
        self.aug_counter = self._counters.get("augment_step")
        self.layout, self.n_params = param_layout(cfg)
        f32 = dict(dtype=torch.float32, device=device)
        self.class_weights = None if weights is None else torch.tensor(weights, **f32)
        self._loss_ext = weights is not None or self.label_smoothing > 0.0 or self.box_overlap != "iou"
        self.params = torch.zeros(self.n_params, **f32)
        # cfg.loss_tail (4; 8 with the Gaussian box head) extra floats after the last parameter hold the loss scalars, so they
        # travel inside the first gradient bucket of the data-parallel all-reduce (vlg.dp.bucket_ranges(tail_extra=cfg.loss_tail))
        self.grads_ext = torch.zeros(self.n_params + cfg.loss_tail, **f32)
        self.grads = self.grads_ext[:self.n_params]
        # bf16 mode: a bf16 copy of the weights feeds the projections (the Adam kernel refreshes it with every update)
        self.params_bf16 = torch.zeros(self.n_params, dtype=torch.bfloat16, device=device) if self.bf16_store else None
        self._w32, self._w16, self._on_ema = self.params, self.params_bf16, False    # what p() / pw() resolve to (ema_weights)
        mask = build_decay_mask(self.layout, self.n_params, decays_matrix) if weight_decay > 0.0 else None
        self.optim = FlatAdam(self.n_params, device, lr, beta1, clip_grad, skip_nonfinite, shadow=self.params_bf16,
                              weight_decay=weight_decay, warmup_steps=warmup_steps, ema_decay=ema_decay, ema_warmup=ema_warmup,
                              decay_mask=mask, ema_shadow=self.bf16_store)
        self.load_params(init_params(cfg, seed))
        self._wgrad_plans: Dict[tuple, tuple] = {}
        self._alloc_workspace(cfg.tokens)
        self.loss_out = self.grads_ext[self.n_params:]   # {total, smooth_l1, iou, ce}; Gaussian box head: + {box_nll, box_cover, 0, 0}
        self.timer = None                            # optional KernelTimer (bench.py roofline leg)

    # ------------------------------------------------------------------ parameters
    def view(self, flat: torch.Tensor, name: str) -> torch.Tensor:
        off, shape = self.layout[name]
        return flat[off:off + math.prod(shape)].view(shape)

    def p(self, name: str) -> torch.Tensor:
        """a parameter as the kernels read it: the live fp32 master - inside ema_weights(), its moving average"""
        return self.view(self._w32, name)

    def pw(self, name: str) -> torch.Tensor:
        """weight operand of a projection: the fp32 master, or its bf16 shadow in the bf16 mode (inside ema_weights(): the
        average, or the average's bf16 shadow)"""
        return self.view(self._w16 if self.bf16_store else self._w32, name)

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the block p() / pw() resolve to the weights' moving average (and its bf16 shadow): forward, rollout,
        accumulate_metrics and evaluate_rollout run on the averaged model.  Nothing is copied.  Whatever would train or
        overwrite weights raises inside it; leaving the block restores the live weights."""
        if self.optim.ema is None:
            raise RuntimeError("ema_weights() needs an engine built with ema_decay > 0")
        self._not_on_ema("ema_weights")
        self._w32, self._w16, self._on_ema = self.optim.ema, self.optim.ema_shadow, True
        try:
            yield self
        finally:
            self._w32, self._w16, self._on_ema = self.params, self.params_bf16, False

    def _not_on_ema(self, what: str) -> None:
        if self._on_ema:
            raise RuntimeError("%s inside ema_weights(): the block evaluates on the averaged weights, it cannot train on or "
                               "replace them" % what)

    def ema_named_params(self) -> Dict[str, torch.Tensor]:
        """name -> view of the moving average, the form named_params() / load_params() use"""
        if self.optim.ema is None:
            raise RuntimeError("ema_named_params() needs an engine built with ema_decay > 0")
        return {n: self.view(self.optim.ema, n) for n in self.layout}

    def _refresh_shadow(self) -> None:
        if self.params_bf16 is not None:
            self.params_bf16.copy_(self.params)          # round to nearest even, as the Adam kernel does

    def g(self, name: str) -> torch.Tensor:
        return self.view(self.grads, name)

    def load_params(self, tensors: Dict[str, torch.Tensor]) -> None:
        """(the moving average, where there is one, restarts from the loaded parameters)"""
        self._not_on_ema("load_params")
        for name in self.layout:
            if self.cfg.gaussian_box and name in ("head_w", "head_b") and tensors[name].shape[0] == self.cfg.n_out - BOX_HEAD_EXTRA:
                raise ValueError("%s has %d rows, a point head's; this engine's Gaussian box head has %d - "
                                 "vlg.spec.grow_box_head(tensors, cfg) pads a point-head checkpoint with the zero rows"
                                 % (name, tensors[name].shape[0], self.cfg.n_out))
            self.view(self.params, name).copy_(tensors[name].to(torch.float32))
        self._refresh_shadow()
        self.optim.seed_ema(self.params)

    def named_params(self) -> Dict[str, torch.Tensor]:
        return {n: self.view(self.params, n) for n in self.layout}

    def named_grads(self) -> Dict[str, torch.Tensor]:
        return {n: self.g(n) for n in self.layout}

    def state_dict(self) -> Dict[str, object]:
        sd = {"params": self.params.detach().cpu().clone(), "exp_avg": self.exp_avg.cpu().clone(),
              "exp_avg_sq": self.exp_avg_sq.cpu().clone(), "step": self.optim.applied_steps(),
              "layout": {k: (o, tuple(s)) for k, (o, s) in self.layout.items()}}
        if self.optim.ema is not None:
            sd["ema"] = self.optim.ema.cpu().clone()
        sd.update((key, self._read_step(key)) for key in self._counters)    # (option off: no key, the checkpoint it always was)
        return sd

    def load_state_dict(self, sd: Dict[str, object]) -> None:
        if tuple(sd["params"].shape) != (self.n_params,):
            hint = ""
            if self.cfg.gaussian_box and sd["params"].numel() == param_layout(dataclasses.replace(self.cfg, box_head="point"))[1]:
                hint = (" (a point-head checkpoint: load its named parameters through vlg.spec.grow_box_head(tensors, cfg) "
                        "and load_params)")
            raise ValueError("checkpoint has %d parameters, model has %d%s" % (sd["params"].numel(), self.n_params, hint))
        self._not_on_ema("load_state_dict")
        self.params.copy_(sd["params"])
        self._refresh_shadow()
        # the moving average: the checkpoint's where it brings one, else it restarts from the loaded parameters
        self.optim.seed_ema(sd["ema"].to(self.device) if sd.get("ema") is not None else self.params)
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self.optim.set_step(int(sd["step"]))
        for key in self._counters:
            if sd.get(key) is not None:
                self._set_step(key, int(sd[key]))

    def _step_counter(self, key: str, who: str) -> torch.Tensor:
        if key not in self._counters:
            raise RuntimeError("%s needs an engine built with %s" % (who, STEP_COUNTERS[key]))
        return self._counters[key]

    def _read_step(self, key: str) -> int:
        """the step k the next training step will read from that counter (a host read: it waits for the device)"""
        return int(self._step_counter(key, key).item())

    def _set_step(self, key: str, k: int) -> None:
        counter = self._step_counter(key, "set_" + key)
        if not 0 <= int(k) < 2 ** 31:
            raise ValueError("%s must be in [0, 2^31), got %r" % (key, k))
        counter.fill_(int(k))

    def _advance_step(self, key: str, stream: int) -> None:
        """the next training step draws anew (a captured graph advances by replaying this launch)"""
        self._timed(key, 0.0, "vlg_dropout_step_advance", ptr(self._counters[key]), stream, nbytes=8.0)

    sched_step = property(lambda self: self._read_step("sched_step"), doc="the scheduled-sampling counter: _read_step")
    dropout_step = property(lambda self: self._read_step("dropout_step"), doc="the dropout counter: _read_step")
    augment_step = property(lambda self: self._read_step("augment_step"), doc="the augmentation counter: _read_step")
    set_sched_step = functools.partialmethod(_set_step, "sched_step")
    set_augment_step = functools.partialmethod(_set_step, "augment_step")
    set_dropout_step = functools.partialmethod(_set_step, "dropout_step")

    def sched_inputs(self) -> tuple:
        """(slot_class (B,T,N) int64, slot_box (B,T,N,4) fp32): views of the mixed inputs the last training step's second pass read"""
        if self._sched is None:
            raise RuntimeError("sched_inputs needs an engine built with sched_sampling")
        if getattr(self, "_mixed_shape", None) is None:
            raise RuntimeError("sched_inputs shows the last training step: there has been none")
        B, T, N = self._mixed_shape
        M = B * T * N
        return self.mix_cls[:M].view(B, T, N), self.mix_box[:M].view(B, T, N, BOX_DIM)

    def augmented_batch(self) -> Dict[str, torch.Tensor]:
        """{slot_class (B,T,N) int64, slot_box (B,T,N,4), tgt_box (B,T,N,4), valid (B,T,N) fp32}: views of the batch the last
        training step ran on (before scheduled sampling mixed its inputs; tgt_class is the caller's own)"""
        if self._aug is None:
            raise RuntimeError("augmented_batch needs an engine built with an aug_* option")
        if getattr(self, "_aug_shape", None) is None:
            raise RuntimeError("augmented_batch shows the last training step: there has been none")
        B, T, N = self._aug_shape
        M = B * T * N
        return {"slot_class": self.aug_cls[:M].view(B, T, N), "slot_box": self.aug_box[:M].view(B, T, N, BOX_DIM),
                "tgt_box": self.aug_tgt_box[:M].view(B, T, N, BOX_DIM), "valid": self.aug_valid[:M].view(B, T, N)}

    def optimizer_state(self) -> Dict[str, object]:
        """Adam state for the checkpoint's 'optimizer' entry (flat tensors, CPU)."""
        return self.optim.flat_state()

    def load_optimizer(self, st: Dict[str, object]) -> None:
        self.optim.load_flat_state(st)

    # ------------------------------------------------------------------- workspace
    def _alloc_workspace(self, tokens: int) -> None:
        cfg, d, ff = self.cfg, self.cfg.d, self.cfg.d_ff
        f32 = dict(dtype=torch.float32, device=self.device)
        M = self.capacity = tokens
        L = cfg.n_layers
        lib = hip.load()
        act = dict(dtype=torch.bfloat16 if self.bf16_store else torch.float32, device=self.device)
        self.x = torch.empty(L + 1, M, d, **f32)          # residual stream entering each layer (+ final)
        self.h1 = torch.empty(L, M, d, **act)
        self.qkv = torch.empty(L, M, 3 * d, **act)
        self.att = torch.empty(L, M, d, **act)
        self.xmid = torch.empty(L, M, d, **f32)
        self.h2 = torch.empty(L, M, d, **act)
        self.u = torch.empty(L, M, ff, **act)             # FFN pre-activation
        self.gl = torch.empty(L, M, ff, **act)            # gelu(u)
        self.stats = torch.empty(2 * L + 1, 2, M, **f32)  # mean / rstd of every layer-norm
        self.xf = torch.empty(M, d, **act)
        self.out = torch.empty(M, cfg.n_out, **f32)
        self.dout = torch.empty(M, cfg.n_out, **f32)
        self.dx = torch.empty(M, d, **f32)                # gradient of the residual stream
        self.dh = torch.empty(M, d, **act)
        self.du = torch.empty(M, ff, **act)
        self.dqkv = torch.empty(M, 3 * d, **act)
        if self._drop is not None:
            if M >= 2 ** 32:
                raise ValueError("dropout: %d rows do not fit the mask's 32-bit row counter" % M)
            self.ybranch = torch.empty(M, d, **f32)       # proj / ff2 output (+ bias) on its way into a dropout site
            self.ddrop = torch.empty(M, d, **f32)         # gradient of that output: select(dx) of the site's layer-norm backward
        if self._sched is not None:
            if M >= 2 ** 31:
                raise ValueError("scheduled sampling: %d tokens do not fit the coin's 32-bit token counter" % M)
            self.mix_cls = torch.empty(M, dtype=torch.int64, device=self.device)      # the second pass's inputs
            self.mix_box = torch.empty(M, BOX_DIM, **f32)
            self._mixed_shape = None
        if self._aug is not None:
            if M >= 2 ** 31:
                raise ValueError("augmentation: %d tokens do not fit the draws' 32-bit token counter" % M)
            self.aug_cls = torch.empty(M, dtype=torch.int64, device=self.device)      # the batch a training step runs on
            self.aug_box, self.aug_tgt_box = torch.empty(M, BOX_DIM, **f32), torch.empty(M, BOX_DIM, **f32)
            self.aug_valid = torch.empty(M, **f32)
            self._aug_shape = None
        self.loss_scratch = torch.zeros(lib.vlg_layout_loss_scratch(), **f32)
        if cfg.gaussian_box:                              # the NLL launch's own partials and ticket, zero between launches
            self.box_nll_scratch = torch.zeros(lib.vlg_layout_box_nll_scratch(), **f32)
        # validation metrics (vlg_layout_metrics): per-block partial sums and the ticket, zero between launches
        self.metrics_scratch = torch.zeros(lib.vlg_layout_metrics_scratch(), dtype=torch.float64, device=self.device)
        n_clip = sum(k.per_clip for k in self.attn)
        if n_clip:      # per query and head: log-sum-exp of every per-clip layer (saved for backward; row: _lse), <dO, O> scratch once
            self.lse = torch.empty(n_clip, cfg.n_heads * M, **f32)
            self.delta = torch.empty(cfg.n_heads * M, **f32)
        # partial-sum ("slab") arenas: floats needed by the embedding, a layer-norm, and each weight-gradient shape
        emb_len = self.layout["l0.ln1_g"][0]
        need = [lib.vlg_embed_bwd_slabs() * emb_len, lib.vlg_layernorm_bwd_slabs(M) * 2 * d]
        for (dy, x, n, k) in ((self.dqkv, self.h1, 3 * d, d), (self.dx, self.att, d, d), (self.du, self.h2, ff, d),
                              (self.dx, self.gl, d, ff), (self.dout, self.xf, cfg.n_out, d)):      # as backward launches them
            need.append(self._wgrad_plan(dy, x, M, n, k)[1] * (n * k + n))
        # two streams (see backward): -1.7 % step time at the metric shape; OFF: sharing the chip, a kernel's duration says nothing
        self.side = torch.cuda.Stream(device=self.device)
        self.overlap_wgrad = os.environ.get("VLG_OVERLAP_WGRAD", "0") == "1"
        self.group_reduce = not self.overlap_wgrad       # 27 reduction launches of ~5.5 us -> 6 per step
        self.pair_backward = (not self.overlap_wgrad and self.precision in ("fp32", "bf16")
                              and os.environ.get("VLG_PAIR_BACKWARD", "1") == "1")
        # a finished bucket's table may be reduced by rider blocks of the NEXT paired launch instead of by a launch of its own
        self.ride_reduces = self.group_reduce and self.pair_backward and os.environ.get("VLG_RIDE_REDUCE", "1") == "1"
        if self.group_reduce:       # buckets (vlg/slabs.py): a layer, the head, the embeddings
            self.buckets = self.wbuckets = SlabBuckets([need[2:6] + [need[1]] * 2, [need[6], need[1]], [need[0]]], self.device, True,
                                                       self.ride_reduces)
        else:   # one arena per producer family, each reduced right behind its producer (before the next one writes)
            self.buckets = SlabBuckets([need[:2]], self.device, False, False)       # layer-norm, embedding (main stream)
            self.wbuckets = SlabBuckets([need[2:]], self.device, False, False)      # weight gradients (the side stream)

    # --------------------------------------------------------------------- helpers
    @staticmethod
    def _stream() -> int:
        return torch.cuda.current_stream().cuda_stream

    def _wgrad_plan(self, dy, x, M: int, N: int, K: int) -> tuple:
        """(flags word, partial sums written) of the weight gradient dy^T . x, alone or as the weight-gradient half of a paired call"""
        key = (M, N, K, dy.dtype, x.dtype)
        plan = self._wgrad_plans.get(key)             # (the library's plan depends on these alone; asked once per shape)
        if plan is None:
            flags = self.gemm_flags | self._storage_bits(dy, x)
            plan = self._wgrad_plans[key] = (flags, hip.load().vlg_linear_wgrad_slabs_for(M, N, K, flags))
        return plan

    def _timed(self, family: str, flops: float, name: str, *args, nbytes: float = 0.0) -> None:
        """Launch through the C ABI; when a timer is attached, bracket the launch with events on
        the launch stream (torch's current stream IS the stream handed to the kernel)."""
        if self.timer is None or (self.timer.only is not None and family not in self.timer.only):
            call(name, *args)
        else:
            with self.timer.section(family, flops, nbytes):
                call(name, *args)

    @staticmethod
    def _storage_bits(a=None, b=None, out=None) -> int:
        """storage flags of a projection call from the dtypes of its activation operands"""
        bf = torch.bfloat16
        return ((EPI_A_BF16 if a is not None and a.dtype == bf else 0) | (EPI_B_BF16 if b is not None and b.dtype == bf else 0) |
                (EPI_OUT_BF16 if out is not None and out.dtype == bf else 0))

    def _linear(self, a, w, b, c, M, N, K, epi, aux_in=None, aux_out=None, ldc=None):
        """ldc: leading dimension of c in elements (None = N, a dense output; the cached generation step writes one
        position's q k v rows straight into the [rows, 3d] cache with ldc = T*3d)"""
        nb = (a.element_size() * M * K + w.element_size() * N * K +
              c.element_size() * M * N * (1 + (aux_in is not None) + (aux_out is not None)))
        flags = epi | self.gemm_flags | self._storage_bits(a, w, c)
        self._timed("gemm_fwd" if N > 32 else "gemm_head", 2.0 * M * N * K, "vlg_linear_fwd", ptr(a), K, ptr(w), K,
                    ptr(b), ptr(c), N if ldc is None else ldc, ptr(aux_in), ptr(aux_out), M, N, K, flags, self._stream(), nbytes=nb)

    def _dgrad(self, dy, w, dx, M, N, K, epi=EPI_NONE, aux_in=None):
        nb = dy.element_size() * M * N + w.element_size() * N * K + dx.element_size() * M * K * (1 + (aux_in is not None))
        flags = epi | self.gemm_flags | self._storage_bits(dy, w, dx)
        self._timed("gemm_dgrad", 2.0 * M * N * K, "vlg_linear_dgrad", ptr(dy), N, ptr(w), K, ptr(dx), K,
                    ptr(aux_in), M, N, K, flags, self._stream(), nbytes=nb)

    def _wgrad(self, dy, x, wname, M, N, K):
        """grad[w | b] = (dy^T . x | colsum dy): split partials -> slab arena -> flat gradient, on the CURRENT stream."""
        stride = N * K + N
        flags, n_slabs = self._wgrad_plan(dy, x, M, N, K)
        arena = self.wbuckets.reserve(n_slabs * stride)
        s = self._stream()
        self._timed("gemm_wgrad" if N > 32 else "gemm_head", 2.0 * M * N * K, "vlg_linear_wgrad", ptr(dy), N, ptr(x),
                    K, ptr(arena), stride, arena.numel(), M, N, K, flags, s,
                    nbytes=dy.element_size() * M * N + x.element_size() * M * K + 4.0 * n_slabs * stride)
        self.wbuckets.add(arena, stride, n_slabs, self.grads.data_ptr() + 4 * self.layout[wname][0], stride, s)

    def _dgrad_wgrad(self, dy, w, dx, x, wname, M, N, K, epi=EPI_NONE, aux_in=None):
        """backward of one projection y = x W^T + b given dy: grad[w | b] (slab partials -> flat gradient) AND dx = dy . W
        (x aux_in with EPI_MUL) through ONE C-ABI call, which the library runs as one launch where neither product fills
        the chip alone (few tokens per GPU; vlg_linear_dgrad_wgrad).  Same results, bit for bit, as _wgrad then _dgrad."""
        stride = N * K + N
        n_slabs = self._wgrad_plan(dy, x, M, N, K)[1]
        arena = self.wbuckets.reserve(n_slabs * stride)
        nb = (dy.element_size() * M * N * 2 + w.element_size() * N * K + dx.element_size() * M * K * (1 + (aux_in is not None)) +
              x.element_size() * M * K + 4.0 * n_slabs * stride)
        bits = self._storage_bits(dy, w, dx)       # bf16 mode: A = the shared dY, B = W (data gradient) AND X (weight gradient), OUT = dX
        if (x.dtype == torch.bfloat16) != (w.dtype == torch.bfloat16):
            raise ValueError("paired backward: X and W must have the same storage type")
        rider, rider_rows, then, rider_bytes = self.buckets.take_rider()    # a finished bucket's reduction rides in this launch
        s = self._stream()
        self._timed("gemm_pair", 4.0 * M * N * K, "vlg_linear_dgrad_wgrad", ptr(dy), N, ptr(w), K, ptr(dx), K, ptr(aux_in),
                    ptr(x), K, ptr(arena), stride, arena.numel(), M, N, K, epi | self.gemm_flags | bits, rider, rider_rows,
                    s, nbytes=nb + rider_bytes)
        if then is not None:
            then()
        self.wbuckets.add(arena, stride, n_slabs, self.grads.data_ptr() + 4 * self.layout[wname][0], stride, s)

    def _lse(self, l: int) -> torch.Tensor:
        return self.lse[self._lse_row[l]]

    def _attn_fwd(self, l: int, batch, B, T, N, M) -> None:
        """the attention launch of layer l, by its kind (vlg/attention.py): per slot along time, per clip, or inside a frame"""
        k, d, s = self.attn[l], self.cfg.d, self._stream()
        nb = 4.0 * self.qkv.element_size() * M * d          # qkv read, out written; the fp32 lse is negligible
        if k.per_clip:      # flops: visible (query, key) pairs x 2 products x 2 x head dim, all heads
            self._timed(k.family + "_fwd", 4.0 * B * d * k.pairs(T, N), k.stem + "_fwd" + self._sfx, ptr(self.qkv[l]),
                        ptr(batch["valid"]) if self._masked else 0, ptr(self.att[l]), ptr(self._lse(l)), B, T, N, d, s, nbytes=nb)
        else:
            self._timed(k.family + "_fwd", 0.0, k.stem + "_fwd" + self._sfx, ptr(self.qkv[l]), ptr(self.att[l]), B * N, T, d, s, nbytes=nb)

    def _attn_bwd(self, l: int, batch, B, T, N, M) -> None:
        k, d, s = self.attn[l], self.cfg.d, self._stream()
        nb = 7.0 * self.qkv.element_size() * M * d          # qkv, out, dout read, dqkv written (+ qkv, dout again)
        if k.per_clip:      # ALGORITHMIC flops: 5 products against the forward's 2 (the two-kernel backward recomputes S and dP: 7 are executed)
            self._timed(k.family + "_bwd", 2.5 * 4.0 * B * d * k.pairs(T, N), k.stem + "_bwd" + self._sfx, ptr(self.qkv[l]),
                        ptr(batch["valid"]) if self._masked else 0, ptr(self.att[l]), ptr(self.dh), ptr(self._lse(l)),
                        ptr(self.delta), ptr(self.dqkv), B, T, N, d, s, nbytes=nb)
        else:
            self._timed(k.family + "_bwd", 0.0, k.stem + "_bwd" + self._sfx, ptr(self.qkv[l]), ptr(self.dh), ptr(self.dqkv), B * N, T, d, s,
                        nbytes=nb)

    def _ln_fwd(self, x, gname, y, stat, M):
        d = self.cfg.d
        self._timed("ln_fwd", 0.0, "vlg_layernorm_fwd_bf16" if y.dtype == torch.bfloat16 else "vlg_layernorm_fwd", ptr(x), ptr(self.p(gname)),
                    ptr(self.p(gname[:-1] + "b")), ptr(y), ptr(stat[0]), ptr(stat[1]), M, d, LN_EPS, self._stream(),
                    nbytes=(4.0 + y.element_size()) * M * d)

    def _drop_ln_fwd(self, y, resid, x_out, gname, h, stat, site, M):
        """x_out = resid + drop_site(y), h = LN(x_out): the fused launch that stands where a training forward had _ln_fwd"""
        d = self.cfg.d
        thr, scale, seed = self._drop
        self._timed("ln_fwd", 0.0, "vlg_dropout_add_layernorm_fwd" + ("_bf16" if h.dtype == torch.bfloat16 else ""), ptr(y), ptr(resid),
                    ptr(self.p(gname)), ptr(self.p(gname[:-1] + "b")), ptr(x_out), ptr(h), ptr(stat[0]), ptr(stat[1]), M, d,
                    LN_EPS, thr, scale, seed, site, ptr(self.drop_step), self._stream(),
                    nbytes=(8.0 + (4.0 if resid is not None else 0.0) + h.element_size()) * M * d)

    def _ln_bwd(self, dy, x, stat, gname, dres, dx_out, M, site=None):
        """site: the dropout site that produced x.  After a training forward with dropout the fused variant also leaves
        select(dx_out) under that site's mask in self.ddrop"""
        d = self.cfg.d
        n_slabs = hip.load().vlg_layernorm_bwd_slabs(M)
        arena = self.buckets.reserve(n_slabs * 2 * d)
        s = self._stream()
        # the fused variant: + the ddrop output behind dx_out, + (thr, scale, seed, site, step) before the stream, + 4 bytes per element
        name, out2, mask = "vlg_layernorm_bwd", (), ()
        if self._dropped:
            name, out2, mask = name + "_dropout", (ptr(self.ddrop),), self._drop + (site, ptr(self.drop_step))
        self._timed("ln_bwd", 0.0, name + ("_bf16" if dy.dtype == torch.bfloat16 else ""), ptr(dy), ptr(x), ptr(stat[0]), ptr(stat[1]),
                    ptr(self.p(gname)), ptr(dres), ptr(dx_out), *out2, ptr(arena), 2 * d, arena.numel(), M, d, *mask, s,
                    nbytes=(dy.element_size() + 4.0 + 4.0 + 4.0 * len(out2) + (4.0 if dres is not None else 0.0)) * M * d)
        self.buckets.add(arena, 2 * d, n_slabs, self.grads.data_ptr() + 4 * self.layout[gname][0], 2 * d, s)

    def _check_batch(self, batch) -> tuple:
        sc = batch["slot_class"]
        B, T, N = sc.shape
        if T != self.cfg.T:
            raise ValueError("batch has T=%d, engine was built for T=%d" % (T, self.cfg.T))
        M = B * T * N
        if M > self.capacity:
            raise ValueError("batch of %d tokens exceeds workspace capacity %d" % (M, self.capacity))
        for k, dt in (("slot_class", torch.int64), ("slot_box", torch.float32), ("tgt_class", torch.int64),
                      ("tgt_box", torch.float32), ("valid", torch.float32)):
            t = batch[k]
            if t.dtype != dt or not t.is_cuda or not t.is_contiguous():
                raise ValueError("batch[%r] must be a contiguous %s HIP tensor" % (k, dt))
        return B, T, N, M

    # --------------------------------------------------------------------- forward
    def forward(self, batch: Dict[str, torch.Tensor], padded_slots: Optional[bool] = None) -> torch.Tensor:
        """Forward + fused loss (the loss kernel also leaves d(total)/d(out) in self.dout).
        Returns the device tensor {total, smooth_l1, iou, ce} - with the Gaussian box head 8 floats, + {box_nll, box_cover, 0, 0},
        and the total includes box_nll_weight * box_nll.  padded_slots overrides the engine's setting for this
        forward and the backward that follows it: a rollout window can hold padded slots where training batches never do."""
        return self._forward(batch, padded_slots, False)

    def _predict(self, batch: Dict[str, torch.Tensor], padded_slots: Optional[bool], train: bool) -> tuple:
        """the forward's launches up to the loss: the window through the final norm, then the head into self.out"""
        B, T, N, M = self._check_batch(batch)
        self._masked = self.padded_slots if padded_slots is None else bool(padded_slots)
        self._shape = (B, T, N, M)
        self._dropped = bool(train) and self._drop is not None and not self._on_ema    # this forward's choice; its backward follows it
        self._encode_window(batch, B, T, N, drop=self._dropped, final=True)
        self._linear(self.xf, self.pw("head_w"), self.p("head_b"), self.out, M, self.cfg.n_out, self.cfg.d, EPI_BIAS)
        return B, T, N, M

    def _augment(self, batch: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """Augmentation: vlg_layout_augment builds the batch this training step runs on from the caller's, which is only read.
        Returns it: slot_class / slot_box / tgt_box / valid are the engine's buffers, tgt_class the caller's."""
        self._not_on_ema("an augmenting training step")
        B, T, N, M = self._check_batch(batch)
        thr_flip, zoom, shift, jitter, thr_drop, seed = self._aug
        self._timed("augment", 0.0, "vlg_layout_augment", ptr(batch["slot_class"]), ptr(batch["slot_box"]), ptr(batch["tgt_box"]),
                    ptr(batch["valid"]), ptr(self.aug_cls), ptr(self.aug_box), ptr(self.aug_tgt_box), ptr(self.aug_valid),
                    ptr(self.aug_counter), B, T, N, self.cfg.n_classes, thr_flip, thr_drop, zoom, shift, jitter, seed,
                    self._stream(), nbytes=88.0 * M)
        self._aug_shape = (B, T, N)
        return dict(batch, **self.augmented_batch())

    def _mix_inputs(self, batch: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """Scheduled sampling, pass 1 and the mix: the evaluation forward on the true inputs (no dropout, no loss launch), then
        vlg_layout_mix_inputs builds the second pass's inputs from self.out.  Returns the batch the training pass runs on:
        slot_class / slot_box are the engine's mixed buffers, targets and valid the caller's."""
        self._not_on_ema("a scheduled-sampling training step")
        cfg = self.cfg
        B, T, N, M = self._predict(batch, None, False)
        thr_max, ramp, temperature, top_k, seed = self._sched
        self._timed("sched_mix", 0.0, "vlg_layout_mix_inputs", ptr(self.out), cfg.n_out, ptr(batch["slot_class"]), ptr(batch["slot_box"]),
                    ptr(self.mix_cls), ptr(self.mix_box), ptr(self.sched_counter), B, T, N, cfg.n_classes, thr_max, ramp,
                    temperature, top_k, seed, self._stream(), nbytes=4.0 * cfg.n_out * B * N * (T - 1) + 2.0 * 24 * M)
        self._mixed_shape = (B, T, N)
        mixed = dict(batch)
        mixed["slot_class"], mixed["slot_box"] = self.mix_cls[:M].view(B, T, N), self.mix_box[:M].view(B, T, N, BOX_DIM)
        return mixed

    def _forward(self, batch: Dict[str, torch.Tensor], padded_slots: Optional[bool], train: bool) -> torch.Tensor:
        cfg = self.cfg
        B, T, N, M = self._predict(batch, padded_slots, train)
        s = self._stream()
        targets = (ptr(self.out), cfg.n_out, ptr(batch["tgt_class"]), ptr(batch["tgt_box"]), ptr(batch["valid"]))
        outs = (ptr(self.dout), ptr(self.loss_out), ptr(self.loss_scratch), B, T, N, cfg.n_classes, SMOOTH_L1_BETA, IOU_EPS,
                LOSS_W_REG, LOSS_W_STRUCT, LOSS_W_CE)
        nbytes = (2.0 * 4 * cfg.n_out + 8 + 16 + 4) * M
        if self._loss_ext:                            # any option on: the same kernel body with the options compiled in
            self._timed("loss", 0.0, "vlg_layout_loss_ext", *targets, ptr(self.class_weights), *outs, self.label_smoothing,
                        hip.LOSS_GIOU if self.box_overlap == "giou" else 0, s,
                        nbytes=nbytes + (12.0 * M if self.class_weights is not None else 0.0))
        else:
            self._timed("loss", 0.0, "vlg_layout_loss", *targets, *outs, s, nbytes=nbytes)
        if cfg.gaussian_box:        # the scale columns' gradient, the padding columns' zeros, loss_out[4..7], and the total's NLL share
            self._timed("box_nll", 0.0, "vlg_layout_box_nll", ptr(self.out), cfg.n_out, ptr(batch["tgt_box"]), ptr(batch["valid"]),
                        ptr(self.dout), ptr(self.loss_out), ptr(self.box_nll_scratch), B, T, N, cfg.n_classes, BOX_S_MIN,
                        BOX_S_MAX, self.box_nll_weight, s, nbytes=(52.0 + 32.0) * M)
        return self.loss_out

    def _encode(self, cls, box, time_emb, w, attn, B: int, T: int, N: int, drop: bool = False, final: bool = False, ldc=None) -> None:
        """THE forward walk: the launches from the embedding through the last layer's second FFN projection - with `final`,
        through the final norm into self.xf.  A layer reads  norm -> qkv -> attention -> proj -> norm -> ff1 -> ff2  and every
        norm is a RESIDUAL norm: x_out = resid + branch, h = LN(x_out).
        drop False: the projection that ends a branch forms x_out in its EPI_BIAS | EPI_RESID epilogue; the norm is _ln_fwd.
        drop True (a training forward with dropout): that projection writes branch + bias into self.ybranch and the norm is the
        fused _drop_ln_fwd, which forms x_out under its site's mask on the way (site 0: the embedding, in place, no residual).
        As many launches either way.
        cls, box, time_emb: what the embedding reads, B*T*N rows of it.  w: the buffer set, indexed by layer - x (L + 1), h1,
        qkv (what the qkv projection WRITES, leading dimension ldc), att, xmid, h2, u, gl (L each), stats (2L, + 1 with final):
        the engine itself for the window, _encode_step's compact set.  attn(l): the attention launch of layer l."""
        cfg, d, ff, L = self.cfg, self.cfg.d, self.cfg.d_ff, self.cfg.n_layers
        M = B * T * N

        def linear(a, wname, c, n, k, epi, **kw):
            self._linear(a, self.pw(wname), self.p(wname[:-1] + "b"), c, M, n, k, epi, **kw)

        def branch_out(a, wname, k, resid, x_out):
            if drop:
                linear(a, wname, self.ybranch, d, k, EPI_BIAS)
            else:
                linear(a, wname, x_out, d, k, EPI_BIAS | EPI_RESID, aux_in=resid)

        def resid_norm(resid, x_out, gname, h, site):
            if drop:
                self._drop_ln_fwd(self.ybranch if site else x_out, resid, x_out, gname, h, w.stats[site], site, M)
            else:
                self._ln_fwd(x_out, gname, h, w.stats[site], M)

        self._timed("embed_fwd", 0.0, "vlg_embed_fwd", ptr(cls), ptr(box), ptr(self.p("cls_emb")), ptr(self.p("box_w")),
                    ptr(self.p("box_b")), ptr(time_emb), ptr(w.x[0]), B, T, N, d, cfg.vocab, self._stream(),
                    nbytes=4.0 * M * d + 24.0 * M)
        for l in range(L):
            pre = "l%d." % l
            resid_norm(w.xmid[l - 1] if l else None, w.x[l], pre + "ln1_g", w.h1[l], 2 * l)
            linear(w.h1[l], pre + "qkv_w", w.qkv[l], 3 * d, d, EPI_BIAS, ldc=ldc)
            attn(l)
            branch_out(w.att[l], pre + "proj_w", d, w.x[l], w.xmid[l])
            resid_norm(w.x[l], w.xmid[l], pre + "ln2_g", w.h2[l], 2 * l + 1)
            linear(w.h2[l], pre + "ff1_w", w.gl[l], ff, d, self._epi_ff1, aux_out=w.u[l])
            branch_out(w.gl[l], pre + "ff2_w", ff, w.xmid[l], w.x[l + 1])
        if final:
            resid_norm(w.xmid[L - 1], w.x[L], "lnf_g", self.xf, 2 * L)

    def _encode_window(self, batch: Dict[str, torch.Tensor], B: int, T: int, N: int, drop: bool = False, final: bool = False) -> None:
        """_encode on all T frames, in the workspace's per-layer buffers: leaves the residual stream in self.x[n_layers] (final:
        and its norm in self.xf).  forward() and rollout(); reads slot_class, slot_box and - per-clip attention with
        self._masked - valid of `batch`."""
        self._encode(batch["slot_class"], batch["slot_box"], self.p("time_emb"), self,
                     lambda l: self._attn_fwd(l, batch, B, T, N, B * T * N), B, T, N, drop, final)

    # -------------------------------------------------------------------- backward
    def backward(self, batch: Dict[str, torch.Tensor], reducer=None) -> None:
        """Fills self.grads (every element overwritten) from the state forward() left.  `reducer`
        (vlg.dp.GradReducer) is told as soon as each contiguous gradient bucket is complete so its
        all-reduce overlaps the rest of backward.

        One walk: head, final norm, then per layer  ff2, ff1, norm, proj, attention, qkv, norm  and the close of the layer's
        bucket, then the embedding.  Its modes differ in two steps only, proj_bwd (a projection's backward) and close.
        Default: ONE stream.  Each projection's data and weight gradient go through one paired call (`pair_backward`), one
        table-driven launch reduces the partial sums of a bucket - the head, a layer, the embeddings (`group_reduce`) - and a
        finished bucket's reduction rides in the next paired launch instead (`ride_reduces`, vlg/slabs.py).
        After a training forward with dropout every layer-norm backward is the fused variant: it also writes select(dx) under the
        mask of the site that fed it into self.ddrop, which - not self.dx - is the dY of the next proj / ff2 backward and what the
        embedding backward reads; self.dx keeps carrying the residual gradient.  One counter advance ends the backward.
        Not paired (fp32x3, bf16_mfma, VLG_PAIR_BACKWARD=0, two streams): a projection's backward is a weight-gradient launch,
        then a data-gradient launch; a bucket is reduced when it closes, or (two streams) each producer right behind itself.
        Option, VLG_OVERLAP_WGRAD=1: two HIP streams.  The data-gradient chain stays on the caller's stream; every weight gradient
        (+ its slab reduction) is launched on `self.side` as soon as its dY exists and runs CONCURRENTLY with the chain, filling the
        gaps its launches leave in the matrix pipes.  Ordering is by events: a side kernel waits for the producer of its dY, and the
        chain waits before it overwrites a buffer a side kernel still reads (du, dqkv, dx) and before a bucket goes to the reducer."""
        self._not_on_ema("backward")
        cfg, d, ff = self.cfg, self.cfg.d, self.cfg.d_ff
        B, T, N, M = self._shape
        main = torch.cuda.current_stream(self.device)
        side = self.side if self.overlap_wgrad else main
        s = main.cuda_stream
        L = cfg.n_layers
        dxy = self.ddrop if self._dropped else self.dx      # gradient of a residual BRANCH's output (= the stream's without dropout)
        last_read: Dict[str, torch.cuda.Event] = {}

        def on_side(reads, fn):
            """launch fn on the side stream once everything enqueued on the main stream so far is done; remember when the
            buffers it reads become free again"""
            if side is main:
                fn()
                return
            e = torch.cuda.Event()
            e.record(main)
            side.wait_event(e)
            with torch.cuda.stream(side):
                fn()
                done = torch.cuda.Event()
                done.record(side)
            for name in reads:
                last_read[name] = done

        def before_write(*names):
            for name in names:
                e = last_read.pop(name, None)
                if e is not None:
                    main.wait_event(e)

        def join():
            if side is not main:
                e = torch.cuda.Event()
                e.record(side)
                main.wait_event(e)
                last_read.clear()

        def proj_bwd(dy, wname, dx, x, N, K, reads, writes=(), epi=EPI_NONE, aux_in=None):
            """backward of the projection y = x W^T + b given dy: grad[w | b], and dx = dy . W.  reads: what the weight gradient
            reads of the buffers the chain reuses; writes: those of them the data gradient overwrites"""
            if self.pair_backward:
                self._dgrad_wgrad(dy, self.pw(wname), dx, x, wname, M, N, K, epi, aux_in)
                return
            on_side(reads, lambda: self._wgrad(dy, x, wname, M, N, K))       # (enqueued first: it waits for dy alone)
            before_write(*writes)
            self._dgrad(dy, self.pw(wname), dx, M, N, K, epi, aux_in)

        ready = (lambda tag: (lambda: reducer.ready(tag))) if reducer is not None else (lambda tag: None)

        def close(tag):
            """the open bucket - the head's, a layer's - is complete.  Paired: it rides in the next paired launch (the head's in
            the last layer's first, layer 0's in the embedding bucket's table) and ready(tag) follows that launch.  Two streams
            without a reducer: nothing to do, and no join - the chain must not wait for the side stream once per layer."""
            if reducer is not None or self.group_reduce:
                join()
                self.buckets.close(s, defer=self.pair_backward, then=ready(tag))

        self.buckets.reset()         # a backward that raised half way leaves nothing behind for this one
        on_side(("dout",), lambda: self._wgrad(self.dout, self.xf, "head_w", M, cfg.n_out, d))
        self._dgrad(self.dout, self.pw("head_w"), self.dh, M, cfg.n_out, d)
        self._ln_bwd(self.dh, self.x[L], self.stats[2 * L], "lnf_g", None, self.dx, M, site=2 * L)
        close("head")
        for l in reversed(range(L)):
            pre = "l%d." % l
            # FFN:  x_out = xmid + W2 gelu(W1 h2 + b1) + b2
            proj_bwd(dxy, pre + "ff2_w", self.du, self.gl[l], d, ff, ("dx",), ("du",), self._epi_dff2, self.u[l])
            proj_bwd(self.du, pre + "ff1_w", self.dh, self.h2[l], ff, d, ("du",))
            before_write("dx")
            self._ln_bwd(self.dh, self.xmid[l], self.stats[2 * l + 1], pre + "ln2_g", self.dx, self.dx, M, site=1 + 2 * l)
            # attention:  xmid = x + Wo attn(Wqkv h1 + b) + bo
            proj_bwd(dxy, pre + "proj_w", self.dh, self.att[l], d, d, ("dx",))
            before_write("dqkv")
            self._attn_bwd(l, batch, B, T, N, M)
            proj_bwd(self.dqkv, pre + "qkv_w", self.dh, self.h1[l], 3 * d, d, ("dqkv",))
            before_write("dx")
            self._ln_bwd(self.dh, self.x[l], self.stats[2 * l], pre + "ln1_g", self.dx, self.dx, M, site=2 * l)
            close("l%d" % l)
        join()
        self._backward_tail(batch, B, T, N, M, reducer)
        if self._dropped:            # the next training step draws new masks
            self._advance_step("dropout_step", s)

    def _backward_tail(self, batch, B, T, N, M, reducer) -> None:
        cfg, d = self.cfg, self.cfg.d
        s = self._stream()
        emb_len = self.layout["l0.ln1_g"][0]
        n_slabs = hip.load().vlg_embed_bwd_slabs_for(B, T, N, d, cfg.vocab)          # by shape: few clips write (and reduce) few slabs
        arena = self.buckets.reserve(n_slabs * emb_len)
        self._timed("embed_bwd", 0.0, "vlg_embed_bwd", ptr(self.ddrop if self._dropped else self.dx), ptr(batch["slot_class"]), ptr(batch["slot_box"]), ptr(arena),
                    emb_len, arena.numel(), B, T, N, d, cfg.vocab, s, nbytes=4.0 * M * d + 24.0 * M)
        self.buckets.add(arena, emb_len, n_slabs, self.grads.data_ptr(), emb_len, s)
        # (flushes a bucket still waiting for a ride in the same table: the gradient buffer is complete for whoever runs next)
        self.buckets.close(s, then=(lambda: reducer.ready("embed")) if reducer is not None else None)

    def forward_backward(self, batch: Dict[str, torch.Tensor], reducer=None) -> torch.Tensor:
        if self._aug is not None:                     # augmentation first: everything below runs on the augmented batch
            batch = self._augment(batch)
        if self._sched is not None:                   # scheduled sampling: pass 1 + the mix; the step below is pass 2
            batch = self._mix_inputs(batch)
        loss = self._forward(batch, None, True)       # (a training forward: the one place dropout is applied)
        self.backward(batch, reducer)
        if self._sched is not None:                   # the next training step flips new coins
            self._advance_step("sched_step", self._stream())
        if self._aug is not None:                     # the next training step draws anew
            self._advance_step("augment_step", self._stream())
        return loss

    def train_step(self, batch: Dict[str, torch.Tensor], reducer=None) -> torch.Tensor:
        """forward -> loss -> backward (+ overlapped gradient all-reduce) -> Adam, as one call.
        Returns the loss scalars (summed over ranks when a reducer is attached).
        Guarded step: the norm needs every gradient, so with a reducer it waits for ALL buckets and then runs one
        squared-norm pass and one Adam over the whole buffer - the split Adam below, which updates everything but the
        embeddings while their bucket is still in flight, is given up in that mode (and only there)."""
        self._not_on_ema("train_step")
        loss = self.forward_backward(batch, reducer)
        if self.optim.guard is not None:
            if reducer is not None:
                reducer.wait()
            self.optimizer_update(reducer.grad_scale if reducer is not None else 1.0)
        elif reducer is not None:
            # the embedding bucket is the last to be produced, so its all-reduce would be fully exposed: update
            # everything else while it is in flight, then the embedding range
            split = self.layout["l0.ln1_g"][0]
            reducer.wait(keep=("embed",))
            self.adam_step(reducer.grad_scale, lo=split, hi=self.n_params)
            reducer.wait()
            self.adam_step(reducer.grad_scale, lo=0, hi=split, advance=False)
        else:
            self.adam_step()
        return loss

    # ------------------------------------------------------------------- optimiser
    def adam_step(self, grad_scale: float = 1.0, lo: int = 0, hi: Optional[int] = None, advance: bool = True) -> None:
        """torch.optim.Adam(lr, betas=(beta1, 0.999)) on the flat buffer (reference src/trainer.py:83,258), or on its
        [lo, hi) slice (both multiples of 4); `advance` = False keeps the step count (second slice of one step)."""
        self._not_on_ema("adam_step")
        if self.optim.guard is not None:             # (whole buffer or an error: FlatAdam.step)
            self.optim.step(self.params, self.grads, grad_scale, lo, hi, advance, self._stream())
            return
        launch = call if self.timer is None else (
            lambda name, *a: self._timed("adam", 0.0, name, *a, nbytes=28.0 * ((self.n_params if hi is None else hi) - lo)))
        self.optim.step(self.params, self.grads, grad_scale, lo, hi, advance, self._stream(), launch)

    def optimizer_update(self, grad_scale: float = 1.0) -> None:
        """The guarded stage after backward and every gradient bucket; the 4 loss floats behind the parameters are not in the norm."""
        self._not_on_ema("optimizer_update")
        launch = None if self.timer is None else (        # bytes of the guarded Adam launch: FlatAdam.adam_bytes
            lambda name, *a: self._timed("adam", 0.0, name, *a, nbytes=self.optim.adam_bytes()))
        self.optim.update_guarded(self.params, self.grads, grad_scale, self._stream(), launch)

    # ------------------------------------------------------------------- hipGraph
    def capture_train_step(self, example_batch: Dict[str, torch.Tensor]):
        """Capture forward -> loss -> backward -> Adam for this batch SHAPE in one hipGraph (single process: the
        data-parallel hooks are not captured) and return `run(batch) -> loss scalars`: it copies the batch into the
        graph's static input buffers and replays ~110 kernel launches with one host call.  Everything the step
        touches is preallocated and no launch argument changes between steps (the Adam step counter moves to the
        device), so replay is bitwise identical to the eager step.  A guarded engine captures its guarded step: clipping,
        the skip and set_lr keep working across replays."""
        self._not_on_ema("capture_train_step")
        self._check_batch(example_batch)
        counter = self.optim.begin_capture()     # the optimiser's device-side scalars
        static = {k: example_batch[k].clone() for k in ("slot_class", "slot_box", "tgt_class", "tgt_box", "valid")}
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        # what the two capture passes move: parameters, moments, the optimiser's scalars, the recipe's state (the average, its
        # bf16 copy, the outputs of ext) and the options' step counters
        moved = [t for t in (self.params, self.exp_avg, self.exp_avg_sq, counter, self.optim.ema, self.optim.ema_shadow,
                             self.optim.guard.ext if self.optim.guard is not None else None, *self._counters.values()) if t is not None]
        kept, kept_steps = [t.clone() for t in moved], self.step_count
        def restore():
            for t, k in zip(moved, kept):
                t.copy_(k)
            self.step_count = kept_steps
            self._refresh_shadow()

        with torch.cuda.stream(side):            # warm-up on a side stream, as stream capture requires
            self.train_step(static)
        torch.cuda.current_stream(self.device).wait_stream(side)
        torch.cuda.synchronize(self.device)
        # undo the warm-up step: capture must not change the training trajectory
        restore()
        timer, self.timer = self.timer, None     # events are not capturable work
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            self.train_step(static)
        self.timer = timer
        restore()

        def run(batch: Dict[str, torch.Tensor]) -> torch.Tensor:
            for k, t in static.items():
                if batch[k] is not t:
                    t.copy_(batch[k], non_blocking=True)
            graph.replay()
            if self.guard is None:                   # (guarded: the device record counts, optimizer_stats() reads it)
                self.step_count += 1
            return self.loss_out
        run.graph, run.static_batch = graph, static
        return run

    # ------------------------------------------------------------------ generation
    def _windows(self) -> tuple:
        """The two (class, box, valid) window buffers a rollout ping-pongs between, sized for the workspace capacity"""
        if getattr(self, "_win", None) is None:
            M = self.capacity
            self._win = tuple((torch.empty(M, dtype=torch.int64, device=self.device),
                               torch.empty(M, BOX_DIM, dtype=torch.float32, device=self.device),
                               torch.empty(M, dtype=torch.float32, device=self.device)) for _ in range(2))
        return self._win

    def _grow_buffers(self) -> dict:
        """Compact buffers of the cached grow step: one frame's B*N rows of every activation an encoder layer passes on,
        capacity / T rows each, allocated on first use like _windows"""
        if getattr(self, "_grow", None) is None:
            cfg, R = self.cfg, -(-self.capacity // self.cfg.T)
            f32 = dict(dtype=torch.float32, device=self.device)
            act = dict(dtype=torch.bfloat16 if self.bf16_store else torch.float32, device=self.device)
            self._grow = dict(cls=torch.empty(R, dtype=torch.int64, device=self.device), box=torch.empty(R, BOX_DIM, **f32),
                              xa=torch.empty(R, cfg.d, **f32), xb=torch.empty(R, cfg.d, **f32), xmid=torch.empty(R, cfg.d, **f32),
                              h=torch.empty(R, cfg.d, **act), att=torch.empty(R, cfg.d, **act), u=torch.empty(R, cfg.d_ff, **act),
                              gl=torch.empty(R, cfg.d_ff, **act), stat=torch.empty(2, R, **f32))
        return self._grow

    def _encode_step(self, p: int, B: int, N: int, valid: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The encoder on the B*N rows of position p alone, against the K/V cache that self.qkv[l] holds for positions < p:
        embeds the compact frame vlg_layout_decode_append left, writes that position's q k v rows
        into the cache and returns the compact residual stream [B*N, d] leaving the last layer.  _encode with T = 1 and
        time_emb[p] on the compact set: the residual stream ping-pongs between xa and xb, one h and one stat serve every norm,
        and the qkv projection writes its rows into the cache with ldc = T*3d.  As many launches as on the window (1 + 7 per
        layer), on 1/T of its rows.  Attention is the _step entry point of the layer's kind (vlg/attention.py): the queries of
        frame p against the keys of the frames the kind sees (FRAME: the rows the projection just wrote, no cache behind it);
        a per-clip kind is masked by the window's `valid` when self._masked - its frame p is what the previous
        vlg_layout_decode_append wrote."""
        d, T, L = self.cfg.d, self.cfg.T, self.cfg.n_layers
        g, BN, s = self._grow_buffers(), B * N, self._stream()
        h, one = [g["h"]] * L, lambda name: [g[name]] * L
        w = types.SimpleNamespace(x=[g["xa"], g["xb"]] * L, h1=h, h2=h, qkv=[self.qkv[l].view(-1)[p * 3 * d:] for l in range(L)],
                                  att=one("att"), xmid=one("xmid"), u=one("u"), gl=one("gl"), stats=[g["stat"]] * (2 * L))

        def attn(l):
            k = self.attn[l]
            frames = k.step_frames(p)           # q and o rows of frame p, k and v of the frames behind it (FRAME: its own alone)
            nb = self.qkv.element_size() * BN * d * (2.0 * frames + 2.0)
            if k.per_clip:
                self._timed(k.family + "_step", 4.0 * B * d * k.step_pairs(N, p), k.stem + "_step" + self._sfx, ptr(self.qkv[l]),
                            ptr(valid) if self._masked else 0, ptr(g["att"]), B, T, N, d, p, d, s,
                            nbytes=nb + (4.0 * BN * frames if self._masked else 0.0))
            else:
                self._timed(k.family + "_step", 0.0, k.stem + "_step" + self._sfx, ptr(self.qkv[l]), ptr(g["att"]), BN, T, d, p, d, s,
                            nbytes=nb)

        self._encode(g["cls"], g["box"], self.p("time_emb")[p], w, attn, B, 1, N, ldc=T * 3 * d)
        return w.x[L]

    def rollout(self, slot_class: torch.Tensor, slot_box: torch.Tensor, steps: int = 8, temperature: float = 0.0,
                top_k: int = 0, seed: int = 0, keep_padded: bool = False, return_logits: bool = False,
                cache: Optional[bool] = None, box_temperature: float = 0.0) -> tuple:
        """Autoregressive generation on the device from a prompt of P frames, 1 <= P <= T: slot_class (B,P,N) int64 and
        slot_box (B,P,N,4) fp32 are device tensors and are not modified.  Returns DEVICE tensors gen_cls (B,steps,N) int64,
        gen_box (B,steps,N,4) fp32 and, with return_logits, the (steps, B*N, n_out) buffer of each step's [logits | raw box].
        P == T: `steps` times predict the frame after the T-frame window, append it and slide the window.  Per step: the
        encoder launches of forward(), vlg_head_last_frame on the B*N rows of the last frame (fp32 master weights in every
        precision mode) and vlg_layout_decode, which draws the frame (temperature 0 = argmax; else temperature / top-k
        sampling, Philox counter = token and step under `seed`; keep_padded carries a reserved class id and its box
        forward), records it and writes the next window into the other of two engine-owned buffers.
        P < T: the history GROWS until it fills the window, and the frame after an h-frame history is the model's output
        at position h-1 of those h frames alone (all mixing along time is causal).  The window buffer holds T frames
        throughout - the reserved class id, zero boxes and valid = 0 after the history; causality hides them.  The prompt
        pass encodes that window once, reads frame P-1 (vlg_head_frame) and appends in place (vlg_layout_decode_append).
        Each further frame until the window is full is a CACHED step (cache None or True): the encoder runs on the newest
        frame's B*N rows only, against the keys and values self.qkv[l] already holds for the earlier positions
        (_encode_step).  Which modes are cached by default: vlg/attention.py - per-clip attention only in an engine built with
        clip_cache=True: without the option it re-encodes the window per grown frame and cache=True raises.  cache=False
        always re-encodes.  Once the window is full the steps are the sliding ones above, from the same buffers.
        No loss, no targets, no host wait inside the loop (one before it with per-clip attention: the mask decision).
        box_temperature (the Gaussian box head; ValueError when > 0 on a point-head engine): 0 keeps the mean box sigmoid(raw);
        tau > 0 DRAWS every generated box, box_k = clamp(mu_k + tau sigma_k z_k, 0, 1), z a stateless Philox normal of (token,
        step) under `seed` on a stream of its own - the class draw is what it is without it.  A Gaussian-head engine decodes
        through vlg_layout_decode_ext / vlg_layout_decode_append_ext (row stride n_out) in every step kind, sliding, cached and
        re-encoded alike; a point-head engine's launches are what they always were."""
        return self._rollout(slot_class, slot_box, steps, temperature, top_k, seed, keep_padded, return_logits, cache,
                             box_temperature)

    def _rollout(self, slot_class, slot_box, steps, temperature, top_k, seed, keep_padded, return_logits, cache, box_temperature,
                 smp: Optional[tuple] = None) -> tuple:
        """rollout()'s loop.  smp = (clips, sample0), from rollout_samples alone: the batch holds B / clips samples of `clips`
        prompts, sample-major, and every frame is decoded by the _samples entries (the _ext argument lists plus clips and
        sample0) - nothing else in the loop knows.  None launches what rollout() always launched."""
        cfg, d = self.cfg, self.cfg.d
        box_tau = box_temperature_options(box_temperature, cfg.box_head)
        if slot_class.dim() != 3 or tuple(slot_box.shape) != tuple(slot_class.shape) + (BOX_DIM,):
            raise ValueError("rollout takes slot_class (B,P,N) and slot_box (B,P,N,4)")
        B, P, N = slot_class.shape
        T = cfg.T
        M, BN = B * T * N, B * N
        if not 1 <= P <= T:
            raise ValueError("prompt has %d frames, the engine's window takes 1 to T=%d" % (P, T))
        if cache and not self._cacheable:
            raise ValueError("cache=True: the cached step of per-clip attention is an option, LayoutEngine(clip_cache=True) / "
                             "VLG_GEN_CLIP_CACHE=1 (without it cache=None re-encodes the window)")
        if M > self.capacity:
            raise ValueError("window of %d tokens exceeds workspace capacity %d" % (M, self.capacity))
        for t, dt, what in ((slot_class, torch.int64, "slot_class"), (slot_box, torch.float32, "slot_box")):
            if t.dtype != dt or not t.is_cuda:
                raise ValueError("%s must be a %s HIP tensor" % (what, dt))
        steps, top_k = int(steps), int(top_k)
        if steps < 1:
            raise ValueError("steps must be >= 1")
        decode_options(temperature, top_k, cfg.n_classes)
        cached = P < T and self._cacheable and (cache is None or bool(cache))
        win = [(c[:M].view(B, T, N), b[:M].view(B, T, N, BOX_DIM), v[:M].view(B, T, N)) for c, b, v in self._windows()]
        if P == T:
            win[0][0].copy_(slot_class)
            win[0][1].copy_(slot_box)
            torch.lt(slot_class, cfg.n_classes, out=win[0][2])      # the first window's validity comes from the prompt
        else:                                                       # frames after the history: reserved id, zero boxes, valid 0
            win[0][0][:, :P].copy_(slot_class)
            win[0][0][:, P:].fill_(cfg.n_classes)
            win[0][1][:, :P].copy_(slot_box)
            win[0][1][:, P:].zero_()
            torch.lt(win[0][0], cfg.n_classes, out=win[0][2])
        # per-clip attention: masks are decided ONCE, here (the only host wait of the call), on the prompt's real frames.  Later
        # frames are masked by the decode kernels' valid; they never gain a padded slot the prompt did not have
        self._masked = self._per_clip and (self.padded_slots or bool((win[0][2][:, :P] == 0).any()))
        gen_cls = torch.empty(B, steps, N, dtype=torch.int64, device=self.device)
        gen_box = torch.empty(B, steps, N, BOX_DIM, dtype=torch.float32, device=self.device)
        logits = torch.empty(steps, BN, cfg.n_out, dtype=torch.float32, device=self.device)
        L, s = cfg.n_layers, self._stream()
        grow = self._grow_buffers() if P < T else None
        head = (ptr(self.p("lnf_g")), ptr(self.p("lnf_b")), ptr(self.p("head_w")), ptr(self.p("head_b")))
        head_kw = dict(nbytes=4.0 * BN * (d + cfg.n_out) + 4.0 * cfg.n_out * d)
        knobs = (float(temperature), top_k, int(seed) & 0xFFFFFFFFFFFFFFFF, int(bool(keep_padded)), s)
        # the Gaussian head's rows are [logits | raw mean | raw scale | padding]: the _ext entries take the stride and the box draw
        ext, dec_ld, dec_tau = ("_ext", (cfg.n_out,), (box_tau,)) if cfg.gaussian_box else ("", (), ())
        if smp is not None:                                         # K futures per prompt: the sample is the counter's last word
            ext, dec_ld, dec_tau = "_samples", (cfg.n_out,), (box_tau,)
            knobs = knobs[:4] + (int(smp[0]), int(smp[1]), s)
        cur = 0                                                    # the window buffer that holds the history
        for i, (encoder, t_read, pos) in enumerate(grow_schedule(P, T, steps, cached)):
            (cls, box, valid), (ncls, nbox, nvalid) = win[cur], win[cur ^ 1]
            if encoder == "step":                                   # the newest frame alone, against the cache: its rows are the last
                x, Tx, frame = self._encode_step(t_read, B, N, valid), 1, ()
            else:                                                   # the window: the last frame, or - still growing - frame t_read
                self._encode_window({"slot_class": cls, "slot_box": box, "valid": valid}, B, T, N)
                x, Tx, frame = self.x[L], T, (t_read,) if t_read < T - 1 else ()
            self._timed("head_last", 2.0 * BN * cfg.n_out * d, "vlg_head_frame" if frame else "vlg_head_last_frame", ptr(x), *head,
                        ptr(logits[i]), B, Tx, N, d, cfg.n_out, *frame, LN_EPS, s, **head_kw)
            if pos is not None:                                     # append in place; the window does not move
                self._timed("decode", 0.0, "vlg_layout_decode_append" + ext, ptr(logits[i]), *dec_ld, ptr(cls), ptr(box), ptr(valid),
                            ptr(gen_cls), ptr(gen_box), ptr(grow["cls"]), ptr(grow["box"]), B, T, N, cfg.n_classes, pos, steps, i,
                            *knobs[:2], *dec_tau, *knobs[2:], nbytes=4.0 * BN * cfg.n_out + 3.0 * 28 * BN)
                continue
            self._timed("decode", 0.0, "vlg_layout_decode" + ext, ptr(logits[i]), *dec_ld, ptr(cls), ptr(box), ptr(ncls), ptr(nbox),
                        ptr(nvalid), ptr(gen_cls), ptr(gen_box), B, T, N, cfg.n_classes, steps, i, *knobs[:2], *dec_tau, *knobs[2:],
                        nbytes=4.0 * BN * cfg.n_out + 2.0 * 28 * M)
            cur ^= 1
        return (gen_cls, gen_box, logits) if return_logits else (gen_cls, gen_box)

    # ------------------------------------------------------------- sampled futures
    def rollout_samples(self, slot_class: torch.Tensor, slot_box: torch.Tensor, steps: int = 8, samples: int = 1, sample0: int = 0,
                        temperature: float = 0.0, top_k: int = 0, seed: int = 0, keep_padded: bool = False,
                        return_logits: bool = False, cache: Optional[bool] = None, box_temperature: float = 0.0) -> tuple:
        """K = `samples` futures of every prompt from ONE seed, in one rollout (DESIGN.md "Sampled futures"): the prompt
        slot_class (B,P,N) / slot_box (B,P,N,4) and every other argument are rollout()'s.  Returns DEVICE tensors gen_cls
        (K,B,steps,N) int64, gen_box (K,B,steps,N,4) fp32 and, with return_logits, logits (K,steps,B*N,n_out).
        The prompt is replicated sample-major into a batch of K*B clips and rollout()'s own loop runs on it - every attention
        mode, the cached and the re-encoded grow steps and the slide - with the _samples decode entries: the token of prompt b,
        slot n draws with Philox counter (b*N + n, step, stream, sample0 + k) under `seed`.  So sample k is a function of (prompt,
        weights, seed, sample0 + k) alone - not of K, of the other prompts' place in the batch or of how the samples were split
        into passes - and sample 0 draws the random numbers rollout() draws.  When K*B*T*N exceeds the workspace capacity the
        call runs ceil(K / k_fit) passes of k_fit = capacity // (B*T*N) samples, each with its own first sample index
        (vlg.samples.sample_passes); ValueError if not even one sample fits.  samples > 1 with temperature 0 and box_temperature
        0 is refused: all samples would be equal.  samples = 1 with sample0 = 0 IS rollout(): the same launches."""
        K, k0 = samples_options(samples, sample0)
        if slot_class.dim() != 3 or tuple(slot_box.shape) != tuple(slot_class.shape) + (BOX_DIM,):
            raise ValueError("rollout_samples takes slot_class (B,P,N) and slot_box (B,P,N,4)")
        B, P, N = slot_class.shape
        box_tau = box_temperature_options(box_temperature, self.cfg.box_head)
        decode_options(temperature, int(top_k), self.cfg.n_classes)
        if K > 1 and float(temperature) == 0.0 and box_tau == 0.0:
            raise ValueError("samples=%d with temperature 0 and box_temperature 0: every sample would be the argmax rollout" % K)
        if B < 1 or N < 1:
            raise ValueError("rollout_samples needs at least one clip and one slot")
        passes = sample_passes(K, k0, B * self.cfg.T * N, self.capacity)
        steps, outs = int(steps), []
        for first, k in passes:
            if k == 1 and first == 0:
                out = self._rollout(slot_class, slot_box, steps, temperature, top_k, seed, keep_padded, return_logits, cache,
                                    box_temperature)
            else:
                out = self._rollout(slot_class.repeat(k, 1, 1), slot_box.repeat(k, 1, 1, 1), steps, temperature, top_k, seed,
                                    keep_padded, return_logits, cache, box_temperature, smp=(B, first))
            out = [out[0].view(k, B, steps, N), out[1].view(k, B, steps, N, BOX_DIM)] + (
                [out[2].view(steps, k, B * N, self.cfg.n_out).transpose(0, 1)] if return_logits else [])
            outs.append(out)
        return tuple(o[0] if len(outs) == 1 else torch.cat(o, dim=0) for o in zip(*outs))

    def sample_record(self) -> SampleRecord:
        """A zeroed SampleRecord (vlg/samples.py) on the engine's device."""
        return SampleRecord(self.device)

    def evaluate_samples(self, clip_class: torch.Tensor, clip_box: torch.Tensor, samples: int = 1, select: str = "iou",
                         record: Optional[SampleRecord] = None, prompt_frames: Optional[int] = None, sample0: int = 0,
                         temperature: float = 0.0, sample_top_k: int = 0, seed: int = 0, keep_padded: bool = False,
                         cache: Optional[bool] = None, box_temperature: float = 0.0, return_samples: bool = False):
        """Best-of-K score of a stochastic model.  clip_class (B,P+S,N) int64 / clip_box (B,P+S,N,4) fp32 as evaluate_rollout
        takes them: the first P = prompt_frames frames (None: T) prompt rollout_samples(..., steps=S, samples=K) under the
        sampling knobs, and the K futures are scored against frames P .. P+S-1 of the clip, read in place, by three launches
        (definitions: include/vlg_hip.h, "sampled futures"): vlg_layout_sample_scores - per sample and clip the mean IoU, the
        mean and the final-frame displacement of the box centres (ADE / FDE) and the class accuracy of the DRAWN frames over
        the tokens whose truth is a real class; vlg_layout_sample_diversity - how much a clip's samples differ pairwise;
        vlg_layout_sample_select - the best sample of every clip by `select` (iou | ade | fde | acc), gathered, and the sums
        ADDED to `record` (a fresh SampleRecord if None).  No host wait; record.summary() makes the one host read.
        Returns the record, or with return_samples (record, dict(best (B,) int32, best_cls (B,S,N), best_box (B,S,N,4),
        gen_cls (K,B,S,N), gen_box (K,B,S,N,4), scores (K,B,VLG_SMP_COLS), div (B,2)))."""
        cfg = self.cfg
        criterion = CRITERIA[select_option(select)]
        if clip_class.dim() != 3 or tuple(clip_box.shape) != tuple(clip_class.shape) + (BOX_DIM,):
            raise ValueError("evaluate_samples takes clip_class (B,P+S,N) and clip_box (B,P+S,N,4)")
        B, TS, N = clip_class.shape
        P = cfg.T if prompt_frames is None else int(prompt_frames)
        if not 1 <= P <= cfg.T:
            raise ValueError("prompt_frames must be in [1, T=%d], got %r" % (cfg.T, prompt_frames))
        S = TS - P
        if S < 1:
            raise ValueError("the clip has %d frames: the %d-frame prompt and at least one frame to score" % (TS, P))
        for t, dt, what in ((clip_class, torch.int64, "clip_class"), (clip_box, torch.float32, "clip_box")):
            if t.dtype != dt or not t.is_cuda or not t.is_contiguous():
                raise ValueError("%s must be a contiguous %s HIP tensor" % (what, dt))
        if record is None:
            record = self.sample_record()
        elif not isinstance(record, SampleRecord) or not record.sums.is_cuda:
            raise ValueError("record must be a SampleRecord on %s (engine.sample_record())" % self.device)
        gen_cls, gen_box = self.rollout_samples(clip_class[:, :P], clip_box[:, :P], steps=S, samples=samples, sample0=sample0,
                                                temperature=temperature, top_k=sample_top_k, seed=seed, keep_padded=keep_padded,
                                                cache=cache, box_temperature=box_temperature)
        gen_cls, gen_box = gen_cls.contiguous(), gen_box.contiguous()
        K, C, s = gen_cls.shape[0], cfg.n_classes, self._stream()
        f32 = dict(dtype=torch.float32, device=self.device)
        scores, div = torch.empty(K, B, SMP_COLS, **f32), torch.empty(B, 2, **f32)
        best = torch.empty(B, dtype=torch.int32, device=self.device)
        best_cls, best_box = torch.empty_like(gen_cls[0]), torch.empty_like(gen_box[0])
        G = float(K * B * S * N)
        self._timed("samples", 0.0, "vlg_layout_sample_scores", ptr(gen_cls), ptr(gen_box), ptr(clip_class), ptr(clip_box),
                    ptr(scores), K, B, S, N, TS, P, C, IOU_EPS, s, nbytes=48.0 * G + 4.0 * SMP_COLS * K * B)
        self._timed("samples", 0.0, "vlg_layout_sample_diversity", ptr(gen_cls), ptr(gen_box), ptr(clip_class), ptr(div),
                    K, B, S, N, TS, P, C, IOU_EPS, s, nbytes=24.0 * G + 8.0 * B * S * N + 8.0 * B)
        self._timed("samples", 0.0, "vlg_layout_sample_select", ptr(scores), ptr(div), ptr(gen_cls), ptr(gen_box), ptr(best),
                    ptr(best_cls), ptr(best_box), ptr(record.sums), K, B, S, N, criterion, s,
                    nbytes=4.0 * SMP_COLS * K * B + 48.0 * B * S * N + 12.0 * B)
        if not return_samples:
            return record
        return record, dict(best=best, best_cls=best_cls, best_box=best_box, gen_cls=gen_cls, gen_box=gen_box, scores=scores, div=div)

    # --------------------------------------------------------------------- metrics
    def metrics_record(self, rows: int = 1) -> MetricsRecord:
        """A zeroed MetricsRecord (vlg/metrics.py) on the engine's device, `rows` independent rows."""
        return MetricsRecord(self.cfg.n_classes, rows, self.device)

    def _metrics(self, out, ld, tgt_class, tgt_box, valid, tgt_T, t0, record, row, B, T, N, top_k, iou_thr) -> None:
        C = self.cfg.n_classes
        if not isinstance(record, MetricsRecord) or record.n_classes != C or not record.counts.is_cuda:
            raise ValueError("record must be a MetricsRecord of %d classes on %s (engine.metrics_record())" % (C, self.device))
        if not 0 <= int(row) < record.rows:
            raise ValueError("row %d outside the record's %d rows" % (row, record.rows))
        if not 1 <= int(top_k) <= C or not math.isfinite(iou_thr):
            raise ValueError("top_k must be in [1, %d] and iou_thr finite" % C)
        M = B * T * N
        self._timed("metrics", 0.0, "vlg_layout_metrics", ptr(out), ld, ptr(tgt_class), ptr(tgt_box), ptr(valid), tgt_T, t0,
                    ptr(record.counts[row]), ptr(record.sums[row]), ptr(self.metrics_scratch), B, T, N, C, int(top_k),
                    float(iou_thr), IOU_EPS, self._stream(), nbytes=(4.0 * ld + 8 + 16 + (4 if valid is not None else 0)) * M)

    def accumulate_metrics(self, batch: Dict[str, torch.Tensor], record: MetricsRecord, row: int = 0, top_k: int = 5,
                           iou_thr: float = 0.5) -> None:
        """Score self.out of the last forward() against that batch's tgt_class / tgt_box / valid and ADD the result to
        row `row` of `record`: one launch of vlg_layout_metrics (definition: include/vlg_hip.h), no host wait.  `batch`
        must be the batch that forward() was given."""
        B, T, N, M = self._check_batch(batch)
        if getattr(self, "_shape", None) != (B, T, N, M):
            raise ValueError("accumulate_metrics scores the last forward(): call it with that forward's batch")
        self._metrics(self.out, self.cfg.n_out, batch["tgt_class"], batch["tgt_box"], batch["valid"], T, 0, record, row,
                      B, T, N, top_k, iou_thr)

    def evaluate_rollout(self, clip_class: torch.Tensor, clip_box: torch.Tensor, record: Optional[MetricsRecord] = None,
                         top_k: int = 5, iou_thr: float = 0.5, return_logits: bool = False, temperature: float = 0.0,
                         sample_top_k: int = 0, seed: int = 0, keep_padded: bool = False, prompt_frames: Optional[int] = None,
                         cache: Optional[bool] = None, pixel_record: Optional[PixelRecord] = None, pixel_size=None,
                         box_temperature: float = 0.0):
        """Score a rollout against the frames that really followed.  clip_class (B,P+S,N) int64 and clip_box (B,P+S,N,4)
        fp32 are device tensors: the first P = prompt_frames frames (None: T; 1 <= P <= T; `cache` as rollout takes it) are
        the prompt, rollout(..., steps=S) generates S frames under the sampling knobs (temperature, sample_top_k =
        rollout's top_k, seed, keep_padded, and box_temperature - the Gaussian box head's box draw), and step i's [logits | raw box]
        are scored against frame P+i of the clip into row i of `record` (a fresh S-row record if None; a given one is
        added to): S launches of vlg_layout_metrics reading the clip in place, no host wait.  top_k and iou_thr are the
        METRIC's (top-k accuracy, IoU hit).  A truth slot with the reserved class id is unscored.
        A step is scored on the model's DISTRIBUTION at that step - arg-max, rank and NLL of its logits, box =
        sigmoid(raw) - not on the class that was drawn: with temperature > 0 the history the model conditions on is
        sampled, the score is still that of the logits.
        pixel_record (engine.pixel_record(S)) with pixel_size = (H, W) adds the score of the frames that were actually
        DRAWN and fed back: the decoded gen_cls / gen_box and frames P .. P+S-1 of the clip (read in place) are rasterised
        as uint8 class maps into two engine-owned buffers, and one vlg_label_confusion launch adds horizon step i to row i
        of the pixel record - three more launches, no host wait; the token record and the return value are what they are
        without it.
        Returns the record, or (record, gen_cls, gen_box, logits) with return_logits."""
        cfg = self.cfg
        if clip_class.dim() != 3 or tuple(clip_box.shape) != tuple(clip_class.shape) + (BOX_DIM,):
            raise ValueError("evaluate_rollout takes clip_class (B,P+S,N) and clip_box (B,P+S,N,4)")
        B, TS, N = clip_class.shape
        P = cfg.T if prompt_frames is None else int(prompt_frames)
        if not 1 <= P <= cfg.T:
            raise ValueError("prompt_frames must be in [1, T=%d], got %r" % (cfg.T, prompt_frames))
        S = TS - P
        if S < 1:
            raise ValueError("the clip has %d frames: the %d-frame prompt and at least one frame to score" % (TS, P))
        for t, dt, what in ((clip_class, torch.int64, "clip_class"), (clip_box, torch.float32, "clip_box")):
            if t.dtype != dt or not t.is_cuda or not t.is_contiguous():
                raise ValueError("%s must be a contiguous %s HIP tensor" % (what, dt))
        if record is None:
            record = self.metrics_record(S)
        elif record.rows < S:
            raise ValueError("the record has %d rows, the rollout %d steps" % (record.rows, S))
        size = self._check_pixels(pixel_record, S, pixel_size) if pixel_record is not None else None
        gen_cls, gen_box, logits = self.rollout(clip_class[:, :P], clip_box[:, :P], steps=S, temperature=temperature,
                                                top_k=sample_top_k, seed=seed, keep_padded=keep_padded, return_logits=True,
                                                cache=cache, box_temperature=box_temperature)
        for i in range(S):
            self._metrics(logits[i], cfg.n_out, clip_class, clip_box, None, TS, P + i, record, i, B, 1, N, top_k, iou_thr)
        if pixel_record is not None:
            self._score_pixels(gen_cls, gen_box, clip_class, clip_box, P, pixel_record, size)
        return (record, gen_cls, gen_box, logits) if return_logits else record

    # --------------------------------------------------------------------- rasterised layouts
    _LABEL_KINDS = {torch.uint8: hip.LABEL_U8, torch.int64: hip.LABEL_I64, torch.float32: hip.LABEL_F32}

    def pixel_record(self, rows: int = 1) -> PixelRecord:
        """A zeroed PixelRecord (vlg/raster.py) on the engine's device, `rows` independent rows."""
        return PixelRecord(self.cfg.n_classes, rows, self.device)

    def rasterize(self, slot_class: torch.Tensor, slot_box: torch.Tensor, size, valid: Optional[torch.Tensor] = None,
                  frames: Optional[tuple] = None, dtype: torch.dtype = torch.int64, what: str = "class",
                  background: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Draw layouts into label maps on the device: one launch of vlg_layout_rasterize (definition: include/vlg_hip.h),
        no host wait.  slot_class (B,T,N) int64, slot_box (B,T,N,4) fp32 and valid (B,T,N) fp32 or None are contiguous
        device tensors and are read in place; frames = (t0, T') draws frames t0 .. t0+T'-1 only.  Returns (B,T',H,W) of
        `dtype` - uint8 (what the pixel score reads), int64 (a cross-entropy target) or float32 (the pixel model's
        segmentation input) - holding per pixel the class of the smallest covering slot (what = "class") or its slot index
        ("slot"), and `background` where there is none (None: n_classes for classes, N for slots).  `out` is written if
        given (same shape and dtype, contiguous).  Legal sizes: vlg.raster.raster_options."""
        if slot_class.dim() != 3 or tuple(slot_box.shape) != tuple(slot_class.shape) + (BOX_DIM,):
            raise ValueError("rasterize takes slot_class (B,T,N) and slot_box (B,T,N,4)")
        B, Tb, N = slot_class.shape
        if what not in WHATS:
            raise ValueError("what must be one of %s, got %r" % (WHATS, what))
        if dtype not in self._LABEL_KINDS:
            raise ValueError("dtype must be torch.uint8, torch.int64 or torch.float32, got %r" % (dtype,))
        if not 1 <= N <= MAX_SLOTS or (what == "slot" and dtype == torch.uint8 and N > 255):
            raise ValueError("rasterize draws 1 to %d slots per frame (slot indices as uint8: at most 255), got %d" % (MAX_SLOTS, N))
        (H, W), bg = raster_options(size, (self.cfg.n_classes if what == "class" else N) if background is None else background,
                                    self.cfg.n_classes)
        t0, T = (0, Tb) if frames is None else (int(frames[0]), int(frames[1]))
        if T < 1 or t0 < 0 or t0 + T > Tb:
            raise ValueError("frames = (t0, T) must lie inside the clip's %d frames, got %r" % (Tb, frames))
        tensors = [(slot_class, torch.int64, "slot_class", (B, Tb, N)), (slot_box, torch.float32, "slot_box", (B, Tb, N, BOX_DIM))]
        if valid is not None:
            tensors.append((valid, torch.float32, "valid", (B, Tb, N)))
        for t, dt, name, shape in tensors:
            if t.dtype != dt or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != shape:
                raise ValueError("%s must be a contiguous %s HIP tensor of shape %s" % (name, dt, shape))
        if out is None:
            out = torch.empty(B, T, H, W, dtype=dtype, device=self.device)
        elif out.dtype != dtype or tuple(out.shape) != (B, T, H, W) or not out.is_cuda or not out.is_contiguous():
            raise ValueError("out must be a contiguous %s HIP tensor of shape %s" % (dtype, (B, T, H, W)))
        self._timed("raster", 0.0, "vlg_layout_rasterize", ptr(slot_class), ptr(slot_box), ptr(valid), ptr(out), B, Tb, t0, T,
                    N, self.cfg.n_classes, H, W, self._LABEL_KINDS[dtype], WHATS.index(what), bg, self._stream(),
                    nbytes=float(out.numel() * out.element_size()) + 28.0 * B * T * N)
        return out

    def _check_pixels(self, record, S: int, size) -> tuple:
        C = self.cfg.n_classes
        if not isinstance(record, PixelRecord) or record.n_classes != C or not record.counts.is_cuda:
            raise ValueError("pixel_record must be a PixelRecord of %d classes on %s (engine.pixel_record())" % (C, self.device))
        if record.rows < S:
            raise ValueError("the pixel record has %d rows, the rollout %d steps" % (record.rows, S))
        if size is None:
            raise ValueError("a pixel record needs pixel_size=(H, W)")
        return raster_options(size, None, C)[0]

    def _score_pixels(self, gen_cls, gen_box, clip_class, clip_box, P: int, record: PixelRecord, size: tuple) -> None:
        """evaluate_rollout's pixel score: three launches, no host wait"""
        B, S, N = gen_cls.shape
        key = (B, S) + size
        if getattr(self, "_pixel_maps_key", None) != key:                 # the two label buffers, allocated on first use
            self._pixel_maps = torch.empty((2,) + key, dtype=torch.uint8, device=self.device)
            self._pixel_maps_key = key
        drawn, truth = self._pixel_maps[0], self._pixel_maps[1]
        self.rasterize(gen_cls, gen_box, size, dtype=torch.uint8, out=drawn)
        self.rasterize(clip_class, clip_box, size, frames=(P, S), dtype=torch.uint8, out=truth)
        self._timed("confusion", 0.0, "vlg_label_confusion", ptr(drawn), ptr(truth), ptr(record.counts), B, S,
                    size[0] * size[1], record.n_labels, 1, self._stream(), nbytes=2.0 * drawn.numel())

    # ---------------------------------------------------------------- public views
    def outputs_btn(self) -> tuple:
        """(class logits (B,T,N,C), raw boxes (B,T,N,4)) of the last forward, in public order."""
        B, T, N, M = self._shape
        o = self.out[:M].view(B, N, T, self.cfg.n_out).permute(0, 2, 1, 3)
        return o[..., :self.cfg.n_classes], o[..., self.cfg.n_classes:]


class KernelTimer:
    """HIP-event timing of selected launches on the launch stream (bench.py roofline leg).

    Events are recorded on torch's current stream, which is the stream passed to the kernels,
    so each start/end pair brackets exactly one launch; durations are read after a sync."""

    def __init__(self, only=None):
        self.records = {}          # family -> list of (start, end, flops)
        self.only = only           # None = every family, else a tuple of family names to bracket

    class _Section:
        def __init__(self, timer, family, flops, nbytes=0.0):
            self.t, self.family, self.flops, self.nbytes = timer, family, flops, nbytes

        def __enter__(self):
            self.s = torch.cuda.Event(enable_timing=True)
            self.e = torch.cuda.Event(enable_timing=True)
            self.s.record()

        def __exit__(self, *a):
            self.e.record()
            self.t.records.setdefault(self.family, []).append((self.s, self.e, self.flops, self.nbytes))

    def section(self, family: str, flops: float, nbytes: float = 0.0):
        return KernelTimer._Section(self, family, flops, nbytes)

    def summary(self):
        """family -> {launches, avg_ms, total_ms, flops_per_launch} (call after a device sync)."""
        out = {}
        for fam, recs in self.records.items():
            ms = [s.elapsed_time(e) for s, e, _, _ in recs]
            fl = [f for _, _, f, _ in recs]
            nb = [b for _, _, _, b in recs]
            out[fam] = {"launches": len(ms), "avg_ms": sum(ms) / len(ms), "total_ms": sum(ms),
                        "flops_per_launch": sum(fl) / len(fl), "bytes_per_launch": sum(nb) / len(nb)}
        return out
