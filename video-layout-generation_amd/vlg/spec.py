"""Frozen contract of the per-clip layout-generation training step.

Two kinds of constants live here:

* reference-real ones, each citing the reference line it restates
  (loss weights, Adam hyper-parameters, class count, seed, normalisation
  constants), and
* self-chosen ones for the layout-token model that BASELINE.json names but the
  reference does not contain: depth, heads, FFN width,
  attention pattern, box parameterisation.  Those are marked SELF-ORACLE and are
  printed on every bench line.

Nothing in this file touches the GPU; it is shared by the HIP engine, the
trainer, bench.py and the tests.
"""
from __future__ import annotations

import dataclasses
import math
from collections import OrderedDict
from typing import Dict, Tuple

from .attention import FRAME, MODES, layer_kinds
from .cabi import values

# ---- reference-real constants -------------------------------------------------
N_CLASSES = 20                  # reference src/models/gridnet.py:9 (seg_out = 20), trainer.py:31-52
LOSS_W_REG = 40.0               # reference src/trainer.py:248  (L1 term  * 40)
LOSS_W_STRUCT = 20.0            # reference src/trainer.py:249  (CombinedLoss * 20)
LOSS_W_CE = 10.0                # reference src/trainer.py:250  (cross entropy * 10)
ADAM_LR = 2e-4                  # reference src/main.py:139-140
ADAM_BETA1 = 0.5                # reference src/main.py:141
ADAM_BETA2 = 0.999              # reference src/trainer.py:83
ADAM_EPS = 1e-8                 # torch.optim.Adam default used at trainer.py:83
SEED = 1024                     # reference src/main.py:121
IMG_MEAN = (0.485, 0.456, 0.406)        # reference src/trainer.py:123
IMG_STD = (0.229, 0.224, 0.225)         # reference src/trainer.py:122
OUT_MEAN = (-0.03, -0.088, -0.188)      # reference src/trainer.py:120
OUT_STD = (0.448, 0.448, 0.450)         # reference src/trainer.py:121

# ---- SELF-ORACLE constants (no reference counterpart) -------------------------
HEAD_DIM = 64                   # one 64-lane wavefront row per head
SMOOTH_L1_BETA = 0.1            # boxes are normalised to [0,1]; beta=0.1 exercises both branches
IOU_EPS = 1e-7
LN_EPS = 1e-5
BOX_DIM = 4                     # (cx, cy, w, h), all in [0,1]
# the Gaussian box head (LayoutConfig.box_head = "gaussian"; DESIGN.md "Gaussian box head"): log sigma = BOX_S_MIN +
# (BOX_S_MAX - BOX_S_MIN) * sigmoid(raw scale), so sigma lies in [e^-7, 1] on boxes normalised to [0, 1]
# (read from include/vlg_hip.h, where the decoding kernels take them; through the header alone: no library is loaded here)
BOX_S_MIN, BOX_S_MAX = values("VLG_BOX_S_", "MIN", "MAX")
BOX_HEADS = ("point", "gaussian")
BOX_HEAD_EXTRA = 8              # columns a Gaussian head appends to a head-output row: 4 raw scales + 4 of padding


@dataclasses.dataclass(frozen=True)
class LayoutConfig:
    """Shape of one batch of clips and of the token model (SELF-ORACLE)."""
    B: int = 32                 # clips per step per GPU
    T: int = 16                 # frames per clip
    N: int = 64                 # object slots per frame
    d: int = 256                # token width
    n_layers: int = 4
    n_classes: int = N_CLASSES
    # vlg/attention.py MODES: "slot" - the default the headline is quoted on -, "clip", or "factored" (divided space-time
    # attention).  Same parameters and checkpoints in all three; "factored" with n_layers = 1 is "slot"
    attention: str = "slot"
    # "point": the box is sigmoid(raw), as ever.  "gaussian": four learned per-coordinate scales beside the four means - the
    # head-output row grows to [logits | raw mean | raw scale | 4 of padding] (the padding keeps n_out a multiple of 8, which
    # the reduced-precision projections need of N) and head_w / head_b gain those rows; nothing else changes
    box_head: str = "point"

    @property
    def n_heads(self) -> int:
        return self.d // HEAD_DIM

    @property
    def d_ff(self) -> int:
        return 4 * self.d

    @property
    def vocab(self) -> int:
        # classes + 1 reserved id, as the only nn.Embedding in the reference does
        # (src/models/simple.py:23 "29+1(cropped)")
        return self.n_classes + 1

    @property
    def n_out(self) -> int:
        return self.n_classes + BOX_DIM + (BOX_HEAD_EXTRA if self.box_head == "gaussian" else 0)

    @property
    def gaussian_box(self) -> bool:
        return self.box_head == "gaussian"

    @property
    def loss_tail(self) -> int:
        """floats of loss scalars behind the flat gradient (they ride in the first data-parallel bucket): {total, smooth_l1,
        iou, ce}, with the Gaussian head + {box_nll, box_cover, 0, 0}.  THE definition: the engine's gradient buffer,
        loss_out and bucket_ranges' tail_extra all take it"""
        return 8 if self.gaussian_box else 4

    @property
    def tokens(self) -> int:
        return self.B * self.T * self.N

    def validate(self) -> None:
        if self.d % HEAD_DIM != 0:
            raise ValueError("d must be a multiple of %d" % HEAD_DIM)
        if self.T not in (4, 8, 16, 32):
            raise ValueError("T must be one of 4, 8, 16, 32 (temporal tile held by one wavefront)")
        if self.N < 1 or self.B < 1 or self.n_layers < 1:
            raise ValueError("B, N, n_layers must be >= 1")
        if self.attention not in ATTENTION_MODES:
            raise ValueError("attention must be 'slot', 'clip' or 'factored'")
        if self.box_head not in BOX_HEADS:
            raise ValueError("box_head must be one of %s, got %r" % (BOX_HEADS, self.box_head))
        if any(k.per_clip for k in MODES[self.attention]) and (self.T * self.N) % 32 != 0:
            raise ValueError("attention=%r needs T*N to be a multiple of 32 (32-token MFMA tiles)" % self.attention)

    def frame_layer(self, l: int) -> bool:
        """whether layer l attends inside a frame (the odd layers of "factored") instead of along time per slot"""
        return layer_kinds(self.attention, l + 1)[l] is FRAME

    @property
    def n_frame_layers(self) -> int:
        return layer_kinds(self.attention, self.n_layers).count(FRAME)

    def describe(self) -> Dict[str, object]:
        d = self._describe()
        if self.gaussian_box:       # (only with the option on: the default's line does not change)
            d["box_head"] = "gaussian (log sigma in [%g, %g], detached mean)" % (BOX_S_MIN, BOX_S_MAX)
        return d

    def _describe(self) -> Dict[str, object]:
        return {"B": self.B, "T": self.T, "N": self.N, "d": self.d, "layers": self.n_layers,
                "heads": self.n_heads, "d_ff": self.d_ff, "classes": self.n_classes,
                "attention": {"slot": "causal-temporal-per-slot", "clip": "block-causal-per-clip (every slot of frames <= t)",
                              "factored": "factored-space-time (even layers causal-temporal-per-slot, odd layers every slot "
                                          "of the token's own frame)"}[self.attention], "box": "cxcywh-sigmoid",
                "loss": "40*smoothL1(beta=%g)+20*(1-IoU)+10*CE" % SMOOTH_L1_BETA}


ATTENTION_MODES = tuple(MODES)            # "slot", "clip", "factored": vlg/attention.py
BOX_OVERLAPS = ("iou", "giou")


def loss_options(class_weights=None, label_smoothing: float = 0.0, box_overlap: str = "iou", n_classes: int = N_CLASSES):
    """The layout loss's options, checked on the host (LayoutEngine and trainer.loss_knobs refuse the same things):
    (weights as a list of n_classes floats or None, label smoothing, overlap term).  class_weights: n_classes numbers, all
    finite and >= 0, at least one > 0; label_smoothing in [0, 1); box_overlap "iou" or "giou".  ValueError otherwise."""
    weights = None
    if class_weights is not None:
        try:
            weights = [float(w) for w in class_weights]
        except (TypeError, ValueError):
            raise ValueError("class_weights must be a sequence of %d numbers, got %r" % (n_classes, class_weights)) from None
        if len(weights) != n_classes:
            raise ValueError("class_weights must hold %d values (one per class), got %d" % (n_classes, len(weights)))
        if not all(math.isfinite(w) and w >= 0.0 for w in weights) or not any(w > 0.0 for w in weights):
            raise ValueError("class_weights must be finite and >= 0 with at least one > 0, got %r" % (weights,))
    try:
        eps = float(label_smoothing)
    except (TypeError, ValueError):
        raise ValueError("label_smoothing must be a number in [0, 1), got %r" % (label_smoothing,)) from None
    if not 0.0 <= eps < 1.0:                            # (also refuses NaN)
        raise ValueError("label_smoothing must be in [0, 1), got %r" % (label_smoothing,))
    if box_overlap not in BOX_OVERLAPS:
        raise ValueError("box_overlap must be one of %s, got %r" % (BOX_OVERLAPS, box_overlap))
    return weights, eps, box_overlap


def box_options(box_head: str = "point", box_nll_weight=None, names=("box_head", "box_nll_weight")):
    """The box head's options, in loss_options' shape: (box_head, weight of the NLL term in the total).  box_head "point" or
    "gaussian"; box_nll_weight finite and >= 0, and anything but its default 1.0 (None counts as the default) is legal ONLY
    with the Gaussian head - the point head has no such term.  ValueError otherwise."""
    if box_head not in BOX_HEADS:
        raise ValueError("%s must be one of %s, got %r" % (names[0], BOX_HEADS, box_head))
    try:
        w = 1.0 if box_nll_weight is None else float(box_nll_weight)
    except (TypeError, ValueError):
        raise ValueError("%s must be a number, got %r" % (names[1], box_nll_weight)) from None
    if box_head != "gaussian" and w != 1.0:             # (NaN != 1.0 too)
        raise ValueError("%s needs %s=gaussian: the point head has no scale to fit" % (names[1], names[0]))
    if not (math.isfinite(w) and w >= 0.0):
        raise ValueError("%s must be finite and >= 0, got %r" % (names[1], box_nll_weight))
    return box_head, w


def box_temperature_options(box_temperature, box_head: str = "point", name: str = "box_temperature") -> float:
    """the box draw's temperature of rollout / evaluate_rollout: finite and >= 0 (0 = the mean box); > 0 needs the Gaussian head"""
    try:
        tau = float(box_temperature)
    except (TypeError, ValueError):
        raise ValueError("%s must be a number, got %r" % (name, box_temperature)) from None
    if not (math.isfinite(tau) and tau >= 0.0):
        raise ValueError("%s must be finite and >= 0, got %r" % (name, box_temperature))
    if tau > 0.0 and box_head != "gaussian":
        raise ValueError("%s > 0 needs box_head=gaussian: the point head predicts no scale to draw from" % name)
    return tau


def grow_box_head(tensors, cfg: "LayoutConfig"):
    """The named parameters of a POINT-head checkpoint -> the dict a Gaussian-head engine of `cfg` loads: head_w / head_b
    padded with the zero rows init_params gives a Gaussian head (sigma starts at exp((BOX_S_MIN + BOX_S_MAX) / 2)), every
    other tensor passed through.  Fits a scale head onto a trained model."""
    import torch
    if not cfg.gaussian_box:
        raise ValueError("grow_box_head takes the Gaussian-head config the result is for (box_head=%r)" % cfg.box_head)
    point = cfg.n_classes + BOX_DIM
    out = dict(tensors)
    for name, want in (("head_w", (point, cfg.d)), ("head_b", (point,))):
        t = tensors[name]
        if tuple(t.shape) != want:
            raise ValueError("grow_box_head: %s has shape %s, a point head of this config has %s" % (name, tuple(t.shape), want))
        out[name] = torch.cat([t, t.new_zeros((BOX_HEAD_EXTRA,) + tuple(t.shape[1:]))], dim=0)
    return out


# The other options' rules, in loss_options' shape: checked on the host, normalised values back or ValueError.  `names` are
# what the message calls the values - LayoutEngine and FlatAdam pass their keywords, the trainer its environment variables.
def dropout_options(p, name: str = "dropout") -> float:
    """dropout probability in [0, 1); 0 is off"""
    if not 0.0 <= float(p) < 1.0:                       # (also refuses NaN)
        raise ValueError("%s must be in [0, 1), got %r" % (name, p))
    return float(p)


def decode_options(temperature, top_k, n_classes: int = N_CLASSES, names=("temperature", "top_k")):
    """the decoding rule's knobs (rollout, scheduled sampling): temperature finite and >= 0 (0 = argmax), top_k in
    [0, n_classes] (0 = every class)"""
    if not (math.isfinite(temperature) and temperature >= 0.0) or not 0 <= int(top_k) <= n_classes:
        raise ValueError("%s must be finite and >= 0, %s in [0, %d]" % (names + (n_classes,)))
    return float(temperature), int(top_k)


def sched_options(eps_max, ramp_steps=0, temperature=0.0, top_k=0, n_classes: int = N_CLASSES,
                  names=("sched_sampling", "sched_ramp_steps", "sched_temperature", "sched_top_k")):
    """scheduled sampling, once it is on: (eps_max in [0, 1], ramp_steps in [0, 2^31), temperature, top_k as decode_options)"""
    if not 0.0 <= float(eps_max) <= 1.0:                # (also refuses NaN)
        raise ValueError("%s must be in [0, 1], got %r" % (names[0], eps_max))
    if not 0 <= int(ramp_steps) < 2 ** 31:
        raise ValueError("%s must be in [0, 2^31), got %r" % (names[1], ramp_steps))
    return (float(eps_max), int(ramp_steps)) + decode_options(float(temperature), top_k, n_classes, names[2:])


AUG_BOUNDS = {"flip": 1.0, "zoom": 0.5, "shift": 0.5, "jitter": 0.25, "drop": 1.0}      # upper bounds; drop's is open


def augment_options(flip=None, zoom=None, shift=None, jitter=None, drop=None,
                    names=("aug_flip", "aug_zoom", "aug_shift", "aug_jitter", "aug_drop")):
    """augmentation, once it is on (any knob given; a missing one counts as 0): (flip in [0, 1], zoom in [0, 0.5], shift in
    [0, 0.5], jitter in [0, 0.25], drop in [0, 1)) as floats"""
    out = []
    for key, value, name in zip(("flip", "zoom", "shift", "jitter", "drop"), (flip, zoom, shift, jitter, drop), names):
        try:
            x = 0.0 if value is None else float(value)
        except (TypeError, ValueError):
            raise ValueError("%s must be a number, got %r" % (name, value)) from None
        hi = AUG_BOUNDS[key]
        if not (0.0 <= x < hi if key == "drop" else 0.0 <= x <= hi):       # (also refuses NaN)
            raise ValueError("%s must be in [0, %g%s, got %r" % (name, hi, ")" if key == "drop" else "]", value))
        out.append(x)
    return tuple(out)


def recipe_options(weight_decay=0.0, warmup_steps=0, ema_decay=0.0, names=("weight_decay", "warmup_steps", "ema_decay")):
    """the optimiser recipe: (weight_decay >= 0, warmup_steps >= 0, ema_decay in [0, 1)); each is off at 0"""
    weight_decay, warmup_steps, ema_decay = float(weight_decay), int(warmup_steps), float(ema_decay)
    if weight_decay < 0.0 or warmup_steps < 0 or not 0.0 <= ema_decay < 1.0:
        raise ValueError("%s and %s must be >= 0, %s in [0, 1)" % tuple(names))
    return weight_decay, warmup_steps, ema_decay


def param_shapes(cfg: LayoutConfig) ->"OrderedDict[str, Tuple[int, ...]]":
    """Names and shapes of every trainable tensor, in flat-buffer order.

    The order is chosen for the backward pass: the tensors whose gradients are
    finished LAST (embeddings) come first and the ones finished FIRST (heads,
    last layer) come last, so gradient buckets can be all-reduced from the tail
    of the flat buffer while earlier layers are still in backward.
    """
    d, ff = cfg.d, cfg.d_ff
    s: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    s["cls_emb"] = (cfg.vocab, d)
    s["box_w"] = (d, BOX_DIM)
    s["box_b"] = (d,)
    s["time_emb"] = (cfg.T, d)
    for l in range(cfg.n_layers):
        p = "l%d." % l
        s[p + "ln1_g"] = (d,)
        s[p + "ln1_b"] = (d,)
        s[p + "qkv_w"] = (3 * d, d)
        s[p + "qkv_b"] = (3 * d,)
        s[p + "proj_w"] = (d, d)
        s[p + "proj_b"] = (d,)
        s[p + "ln2_g"] = (d,)
        s[p + "ln2_b"] = (d,)
        s[p + "ff1_w"] = (ff, d)
        s[p + "ff1_b"] = (ff,)
        s[p + "ff2_w"] = (d, ff)
        s[p + "ff2_b"] = (d,)
    s["lnf_g"] = (d,)
    s["lnf_b"] = (d,)
    s["head_w"] = (cfg.n_out, d)
    s["head_b"] = (cfg.n_out,)
    return s


def param_layout(cfg: LayoutConfig) -> Tuple["OrderedDict[str, Tuple[int, Tuple[int, ...]]]", int]:
    """name -> (offset in floats, shape); every offset is a multiple of 4 floats (16 B)."""
    out: "OrderedDict[str, Tuple[int, Tuple[int, ...]]]" = OrderedDict()
    off = 0
    for name, shape in param_shapes(cfg).items():
        n = int(math.prod(shape))
        out[name] = (off, shape)
        off += (n + 3) // 4 * 4
    return out, off


def step_flops(cfg: LayoutConfig) -> Dict[str, float]:
    """Algorithmic FLOPs of one training step (Spec N)."""
    M, d = cfg.tokens, cfg.d
    per_layer_fwd = 24.0 * M * d * d            # QKV 6 + proj 2 + FFN 16  (x M d^2)
    # a layer's attention by its kind: 4 d flop per visible (query, key) pair - per slot the causal half T^2 / 2, as ever
    kinds = [4.0 * cfg.B * d * k.pairs(cfg.T, cfg.N) if k.per_clip else 4.0 * cfg.B * cfg.N * cfg.T * cfg.T * d / 2.0
             for k in layer_kinds(cfg.attention, cfg.n_layers)]
    attn_fwd = kinds[0] + sum(f - kinds[0] for f in kinds) / cfg.n_layers       # the mean over the layers
    head_fwd = 2.0 * M * d * cfg.n_out
    fwd = cfg.n_layers * (per_layer_fwd + attn_fwd) + head_fwd
    # backward = 2 x forward for the projections; attention backward = 2.5 x its forward (5 products against 2)
    return {"gemm_fwd_per_layer": per_layer_fwd, "fwd": fwd, "fwd_bwd": 3.0 * fwd + 0.5 * cfg.n_layers * attn_fwd}
