"""Drop-in `trainer` module: same surface the reference's src/main.py consumes.

    from trainer import Trainer            # reference src/main.py:14
    trainer = Trainer(args)                # reference src/main.py:62   (after init_process_group + seeding)
    trainer.set_epoch(epoch); trainer.train(); metrics = trainer.validate()
    trainer.save_checkpoint(metrics)       # reference src/main.py:76-82

`args` is the argparse Namespace of reference src/main.py:86-160 plus the fields main.worker
injects (`logger`, `rank`, `gpus`, `path`, `port`; main.py:51-52,164,173,183).  The step behind
it is the MI355X-native layout-token step (vlg.engine.LayoutEngine -> libvlg_hip.so); the
reference's own step is a 2-D CNN that BASELINE.json does not ask for.

Shape knobs the reference CLI does not have are read with getattr/env defaults so main.py stays
byte-for-byte unchanged:  VLG_FRAMES (T, 16), VLG_SLOTS (N, 64), VLG_DMODEL (d, 256),
VLG_LAYERS (4), VLG_TRAIN_CLIPS (1024), VLG_VAL_CLIPS (256), VLG_VARIABLE_N (0), VLG_PRECISION (fp32 | fp32x3 | bf16 |
bf16_mfma: projection arithmetic / activation storage, vlg/engine.py; with VLG_MODEL=gridnet bf16 / bf16_mfma run the 3x3
convolutions on bf16-rounded operands, csrc/conv_bf16.hip).

VLG_MODEL=gridnet switches the step to the reference's OWN model and losses (vlg/image_engine.py;
VLG_WITH_HED / VLG_WITH_VGG = 1 add the frozen edge net and the VGG19 term, VLG_HED_CKPT / VLG_VGG_CKPT their weights;
--train_dir / --val_dir in the reference's Cityscapes layout are read by vlg/cityscapes.py, else frames are synthetic:
--arch GridNet|CoordGridNet on the conv3x3 MFMA kernels, 40 L1 + 20 (GradientLoss + SSIM) + 10 CE, reference
src/trainer.py:193-258) on synthetic frame triplets of VLG_IMG_SIZE (256) pixels; the default (layout) is the
token step BASELINE.json's metric is quoted on.

Optimiser knobs (all off by default; vlg/optim.py): args.clip_grad / VLG_CLIP_GRAD = global-norm gradient clipping
at that norm (0 = off), args.skip_nonfinite / VLG_SKIP_NONFINITE = 1 skips a step whose gradient holds inf or NaN,
VLG_LR_DECAY = 1 honours --lr_decay_step / --lr_decay_gamma (epochs; the reference parses them and never applies them, so
they stay ignored unless asked for).  Any of them switches the engine to its guarded step; the train log line then also
shows the gradient norm and the number of skipped steps.

The training recipe on that step (all off by default; what each does: FlatAdam in vlg/optim.py, DESIGN.md "Training recipe";
what is legal: vlg.spec.recipe_options): args.weight_decay / VLG_WEIGHT_DECAY, on the weight matrices (layout mode) or
convolution weights (pixel mode); args.warmup_steps / VLG_WARMUP_STEPS - it composes with VLG_LR_DECAY: the epoch's rate is
written into the device record as before and the warm-up scales it on the device; args.ema_decay / VLG_EMA_DECAY and
args.ema_warmup / VLG_EMA_WARMUP = 1, the weights' moving average; args.ema_eval / VLG_EMA_EVAL (default 1, read only
when the average is on): layout mode's validate(), generate_sequence() and evaluate_rollout() run on the averaged weights
(LayoutEngine.ema_weights()).  save_checkpoint adds 'gridnet_ema', the averaged model in 'gridnet''s format; --resume
restores the average through 'optimizer'.

The four options below are LayoutEngine's keyword arguments of the same names - its docstring says what each does, and
vlg/spec.py (dropout_options, sched_options, augment_options, loss_options) which values are legal; here only how they are
asked for.

Dropout in layout mode (off by default; DESIGN.md "Dropout"): args.dropout / VLG_DROPOUT = p; VLG_DROPOUT_SEED (default
args.seed) seeds the stateless mask, and data-parallel rank r uses seed + r so that ranks draw different masks.

Scheduled sampling in layout mode (off by default; DESIGN.md "Scheduled sampling"): args.sched_sampling / VLG_SCHED_SAMPLING
= eps_max, VLG_SCHED_RAMP_STEPS (0), VLG_SCHED_TEMPERATURE (0 = argmax) / VLG_SCHED_TOP_K (0 = every class), VLG_SCHED_SEED
(default args.seed; data-parallel rank r uses seed + r).

Augmentation in layout mode (off by default; DESIGN.md "Augmentation"; legal values: vlg.spec.augment_options):
args.aug_flip / VLG_AUG_FLIP = the probability of a horizontal flip per CLIP, args.aug_zoom / VLG_AUG_ZOOM and args.aug_shift /
VLG_AUG_SHIFT = the per-clip zoom about the centre (1 +- zoom) and shift (+- shift of the image), args.aug_jitter /
VLG_AUG_JITTER = the per-token jitter of the input boxes, args.aug_drop / VLG_AUG_DROP = the probability of dropping a track;
any of them set turns the option on, inside the step (captured steps included), and the ones not set count as 0.
VLG_AUG_SEED (default args.seed; data-parallel rank r uses seed + r).  With VLG_AUG_FLIP set the device's per-clip flip
REPLACES the host's per-batch coin (_flip, the reference's src/trainer.py:199-206); with it unset _flip runs as ever.

Loss options in layout mode (all off by default; DESIGN.md "Loss options"): args.class_weights / VLG_CLASS_WEIGHTS = 20
comma-separated floats (vlg.metrics.balanced_class_weights turns the confusion matrix of VLG_VAL_METRICS=1 into such a
list); args.label_smoothing / VLG_LABEL_SMOOTHING; args.box_overlap / VLG_BOX_OVERLAP = iou (default) or giou.

Gaussian box head in layout mode (off by default; csrc/box_nll.hip, DESIGN.md "Gaussian box head"; box_knobs):
args.box_head / VLG_BOX_HEAD = point (default) | gaussian gives the model four learned box scales beside the four means and
one NLL launch behind the loss launch; args.box_nll_weight / VLG_BOX_NLL_WEIGHT (default 1) weighs that term, and is refused
with the point head; validate() then adds box_nll and box_cover to its result.  args.gen_box_temperature /
VLG_GEN_BOX_TEMPERATURE joins the generation knobs below: > 0 draws every generated box from the predicted distribution
(refused with the point head).

Generation knobs of generate_sequence in layout mode (a keyword argument wins over them; csrc/decode.hip, DESIGN.md
"Generation"): args.gen_temperature / VLG_GEN_TEMPERATURE (0 = argmax; > 0 samples from softmax(logits / temperature)),
args.gen_top_k / VLG_GEN_TOP_K (0 = every class, else only the k largest logits), args.gen_seed / VLG_GEN_SEED (default
args.seed; the same seed, prompt and weights give the same sequence), args.gen_keep_padded / VLG_GEN_KEEP_PADDED = 1 keeps a
slot that is padded (reserved class id) in the window's last frame padded in every generated frame.
args.gen_clip_cache / VLG_GEN_CLIP_CACHE = 1 (off by default) is the engine knob LayoutEngine(clip_cache=True).
Sampled futures (csrc/samples.hip, vlg/samples.py, DESIGN.md "Sampled futures"; sample_knobs): args.gen_samples /
VLG_GEN_SAMPLES = K (default 1 = off) is the number of futures generate_samples draws per prompt in one rollout and
evaluate_samples scores (best-of-K IoU / minADE / minFDE / accuracy, the samples' mean and diversity); args.gen_select /
VLG_GEN_SELECT = iou (default) | ade | fde | acc is the score evaluate_samples selects the best sample by.  generate_sequence
and evaluate_rollout do not read them.
args.attention / VLG_ATTENTION = slot (default) | clip | factored picks the encoder's attention: the kinds of attention, the
layers each mode gives them to and which modes cache grown frames by default are stated in vlg/attention.py.

Validation metrics in layout mode (csrc/metrics.hip, vlg/metrics.py, DESIGN.md "Validation metrics"): args.val_metrics /
VLG_VAL_METRICS = 1 makes validate() also score every batch on the device - class accuracy, top-k accuracy, NLL, mean IoU,
the share of boxes with IoU above a threshold, per-class figures and the confusion matrix - one extra launch per batch and
one host read per pass; the returned dict gains those keys.  args.val_topk / VLG_VAL_TOPK (5) is the k of the top-k
accuracy, args.val_iou_thr / VLG_VAL_IOU_THR (0.5) the IoU threshold; evaluate_rollout uses the same two.  Off (the default)
validate() returns {"loss": ...} as before.

Pixel score of rollouts in layout mode (csrc/raster.hip, vlg/raster.py, DESIGN.md "Rasterised layouts"): args.val_pixels /
VLG_VAL_PIXELS = HxW (off by default; legal sizes: vlg.raster.raster_options) makes evaluate_rollout also draw the decoded
frames and the frames that really followed as H x W class maps on the device and score them pixel by pixel: each
horizon's dict gains pixel_miou, pixel_accuracy, pixel_per_class_iou and pixel_background_iou.  render_layout() draws any
layout into label maps, also as the float maps the pixel model's generate_sequence takes.

Repairs of reference defects, all stated: gradients are overwritten each
step (A-5 zero_grad), the train log line uses the `loss` key (A-6), one checkpoint schema
{'epoch','arch','gridnet','optimizer'} for save/--ckpt/--resume (A-1,A-8,A-9), `.model` exists
(A-11), validate() moves every input to the device (A-13) and all-reduces a size-weighted SUM then
divides by the GLOBAL clip count (the reference divides by the local count, trainer.py:336-339,
which returns world x the mean), visualisation is not run every step (A-15).
"""
from __future__ import annotations

import contextlib
import os
import random
import shutil
from time import time
from typing import Callable, Dict, Optional

import torch
import torch.distributed as dist

from vlg.data import BATCH_KEYS, BucketedClipLoader, ClipLoader, synthetic_clips, to_device
from vlg.dp import GradReducer, bucket_ranges
from vlg.optim import decayed_lr
from vlg.raster import parse_size, raster_options
from vlg.samples import samples_options, select_option
from vlg.spec import (ADAM_BETA1, ADAM_LR, N_CLASSES, SEED, LayoutConfig, augment_options, dropout_options, loss_options,
                      recipe_options, sched_options, box_options, box_temperature_options)


class AverageMeter(object):
    """Running weighted mean; same arithmetic as reference src/utils.py:1-16."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.val = 0
        self.avg = 0
        self.sum = 0
        self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


class _ScalarLog:
    """SummaryWriter stand-in (tensorboardX is not installed here): same add_scalar calls as
    reference src/trainer.py:166,281,377, appended to <path>/scalars.tsv."""

    def __init__(self, path: str):
        os.makedirs(path, exist_ok=True)
        self.f = open(os.path.join(path, "scalars.tsv"), "a")

    def add_scalar(self, tag, value, step):
        self.f.write("%s\t%d\t%.8g\n" % (tag, int(step), float(value)))
        self.f.flush()

    def add_image(self, *a, **k):      # image grids (trainer.py:282-286) are out of scope
        pass


def _make_writer(path: str):
    try:
        from tensorboardX import SummaryWriter      # reference src/trainer.py:17,141-142
        return SummaryWriter(path)
    except Exception:
        return _ScalarLog(path)


def _knob(args, name: str, env: str, default: int) -> int:
    v = getattr(args, name, None)
    return int(v) if v is not None else int(os.environ.get(env, default))


def _fmt(v) -> str:
    return "n/a" if v is None else "%.4f" % v


def _knob_float(args, name: str, env: str, default: float) -> float:
    v = getattr(args, name, None)
    return float(v) if v is not None else float(os.environ.get(env, default))


def optim_knobs(args) -> Dict[str, object]:
    """{clip_grad, skip_nonfinite, lr_decay} from args / environment (module docstring); all off by default.  The recipe's
    knobs join the dict only where they are ON, so with all of them off it is the dict it always was: weight_decay,
    warmup_steps, ema_decay, and with ema_decay also ema_warmup and ema_eval (default on; not read without the average).
    Read them with .get(name, 0)."""
    knobs = {"clip_grad": max(_knob_float(args, "clip_grad", "VLG_CLIP_GRAD", 0.0), 0.0),
             "skip_nonfinite": bool(_knob(args, "skip_nonfinite", "VLG_SKIP_NONFINITE", 0)),
             "lr_decay": os.environ.get("VLG_LR_DECAY", "0") == "1"}
    weight_decay, warmup_steps, ema_decay = recipe_options(
        _knob_float(args, "weight_decay", "VLG_WEIGHT_DECAY", 0.0), _knob(args, "warmup_steps", "VLG_WARMUP_STEPS", 0),
        _knob_float(args, "ema_decay", "VLG_EMA_DECAY", 0.0), names=("VLG_WEIGHT_DECAY", "VLG_WARMUP_STEPS", "VLG_EMA_DECAY"))
    if weight_decay > 0.0:
        knobs["weight_decay"] = weight_decay
    if warmup_steps > 0:
        knobs["warmup_steps"] = warmup_steps
    if ema_decay > 0.0:
        knobs.update(ema_decay=ema_decay, ema_warmup=bool(_knob(args, "ema_warmup", "VLG_EMA_WARMUP", 0)),
                     ema_eval=bool(_knob(args, "ema_eval", "VLG_EMA_EVAL", 1)))
    return knobs


def _rank_seed(args, name: str, env: str) -> int:
    """an option's seed (default args.seed) in [0, 2^63), offset by the data-parallel rank so that ranks draw differently"""
    seed = _knob(args, name, env, int(getattr(args, "seed", SEED)))
    if not 0 <= seed < 2 ** 63:
        raise ValueError("%s must be in [0, 2^63), got %r" % (env, seed))
    return seed + int(getattr(args, "rank", 0) or 0)


def dropout_knobs(args) -> Dict[str, object]:
    """the engine's dropout keyword arguments from args / environment (module docstring): {} with the knob off, so an
    engine without the option is never handed one; else {dropout, dropout_seed}.  The rule is LayoutEngine's:
    vlg.spec.dropout_options, before any engine exists."""
    p = dropout_options(_knob_float(args, "dropout", "VLG_DROPOUT", 0.0), "VLG_DROPOUT")
    seed = _rank_seed(args, "dropout_seed", "VLG_DROPOUT_SEED")
    return {"dropout": p, "dropout_seed": seed} if p else {}


def sched_knobs(args) -> Dict[str, object]:
    """the engine's scheduled-sampling keyword arguments from args / environment (module docstring): {} with
    args.sched_sampling / VLG_SCHED_SAMPLING unset, so an engine without the option is never handed one; else
    {sched_sampling, sched_ramp_steps, sched_temperature, sched_top_k, sched_seed}.  The rule is LayoutEngine's:
    vlg.spec.sched_options, before any engine exists."""
    eps = getattr(args, "sched_sampling", None)
    if eps is None:
        eps = os.environ.get("VLG_SCHED_SAMPLING") or None
    if eps is None:
        return {}
    names = ("sched_sampling", "sched_ramp_steps", "sched_temperature", "sched_top_k")
    values = sched_options(eps, _knob(args, "sched_ramp_steps", "VLG_SCHED_RAMP_STEPS", 0),
                           _knob_float(args, "sched_temperature", "VLG_SCHED_TEMPERATURE", 0.0),
                           _knob(args, "sched_top_k", "VLG_SCHED_TOP_K", 0), N_CLASSES, tuple("VLG_" + n.upper() for n in names))
    return dict(zip(names, values), sched_seed=_rank_seed(args, "sched_seed", "VLG_SCHED_SEED"))


AUG_KNOBS = ("aug_flip", "aug_zoom", "aug_shift", "aug_jitter", "aug_drop")


def augment_knobs(args) -> Dict[str, object]:
    """the engine's augmentation keyword arguments from args / environment (module docstring): {} with none of
    args.aug_* / VLG_AUG_FLIP, VLG_AUG_ZOOM, VLG_AUG_SHIFT, VLG_AUG_JITTER, VLG_AUG_DROP set, so an engine without the option
    is never handed one; else all five (a knob that is not set is 0.0) and aug_seed.  The rule is LayoutEngine's:
    vlg.spec.augment_options, before any engine exists."""
    asked = []
    for name in AUG_KNOBS:
        v = getattr(args, name, None)
        asked.append(v if v is not None else (os.environ.get("VLG_" + name.upper()) or None))
    if all(v is None for v in asked):
        return {}
    values = augment_options(*asked, names=tuple("VLG_" + n.upper() for n in AUG_KNOBS))
    return dict(zip(AUG_KNOBS, values), aug_seed=_rank_seed(args, "aug_seed", "VLG_AUG_SEED"))


def device_flip(args) -> bool:
    """whether the engine's per-clip flip stands in for the host's per-batch one (Trainer._flip): args.aug_flip / VLG_AUG_FLIP set"""
    return getattr(args, "aug_flip", None) is not None or bool(os.environ.get("VLG_AUG_FLIP"))


def loss_knobs(args) -> Dict[str, object]:
    """the engine's loss-option keyword arguments from args / environment (module docstring): {} with all of them off, so an
    engine without the options is never handed one; else those that are on among {class_weights, label_smoothing,
    box_overlap}.  Refuses what LayoutEngine refuses (vlg.spec.loss_options), before any engine exists."""
    weights = getattr(args, "class_weights", None)
    if weights is None:
        weights = os.environ.get("VLG_CLASS_WEIGHTS") or None
    if isinstance(weights, str):
        try:
            weights = [float(x) for x in weights.split(",")]
        except ValueError:
            raise ValueError("VLG_CLASS_WEIGHTS must be %d comma-separated floats, got %r" % (N_CLASSES, weights)) from None
    eps = getattr(args, "label_smoothing", None)
    if eps is None:
        eps = os.environ.get("VLG_LABEL_SMOOTHING", 0.0)
    overlap = str(getattr(args, "box_overlap", None) or os.environ.get("VLG_BOX_OVERLAP", "iou")).lower()
    weights, eps, overlap = loss_options(weights, eps, overlap, N_CLASSES)
    knobs: Dict[str, object] = {}
    if weights is not None:
        knobs["class_weights"] = weights
    if eps > 0.0:
        knobs["label_smoothing"] = eps
    if overlap != "iou":
        knobs["box_overlap"] = overlap
    return knobs


def box_knobs(args) -> Dict[str, object]:
    """the Gaussian box head's knobs from args / environment (DESIGN.md "Gaussian box head"): {} with args.box_head /
    VLG_BOX_HEAD unset or "point", so a config and an engine without the option are never handed one; else {box_head:
    "gaussian", box_nll_weight} (args.box_nll_weight / VLG_BOX_NLL_WEIGHT, default 1).  box_head goes to LayoutConfig
    (layout_config), box_nll_weight to the engine.  Refuses what they refuse (vlg.spec.box_options) - VLG_BOX_NLL_WEIGHT
    with the point head included - before any engine exists."""
    head = str(getattr(args, "box_head", None) or os.environ.get("VLG_BOX_HEAD") or "point").lower()
    weight = getattr(args, "box_nll_weight", None)
    if weight is None:
        weight = os.environ.get("VLG_BOX_NLL_WEIGHT") or None
    head, weight = box_options(head, weight, names=("VLG_BOX_HEAD", "VLG_BOX_NLL_WEIGHT"))
    return {"box_head": head, "box_nll_weight": weight} if head == "gaussian" else {}


def recipe_kwargs(knobs: Dict[str, object]) -> Dict[str, object]:
    """the recipe's engine keyword arguments - only those that are on, so an engine factory without them is never handed one"""
    return {k: knobs[k] for k in ("weight_decay", "warmup_steps", "ema_decay", "ema_warmup") if knobs.get(k)}


def generation_knobs(args) -> Dict[str, object]:
    """{temperature, top_k, seed, keep_padded} of generate_sequence in layout mode, from args / environment (module
    docstring): argmax, every class, the run's seed, padded slots decoded like any other - unless asked otherwise.
    args.gen_box_temperature / VLG_GEN_BOX_TEMPERATURE, where set, joins as box_temperature (the Gaussian box head's box
    draw; refused here with the point head: vlg.spec.box_temperature_options); unset, the dict is the one it always was."""
    knobs = {"temperature": _knob_float(args, "gen_temperature", "VLG_GEN_TEMPERATURE", 0.0),
             "top_k": _knob(args, "gen_top_k", "VLG_GEN_TOP_K", 0),
             "seed": _knob(args, "gen_seed", "VLG_GEN_SEED", int(getattr(args, "seed", SEED))),
             "keep_padded": bool(_knob(args, "gen_keep_padded", "VLG_GEN_KEEP_PADDED", 0))}
    tau = getattr(args, "gen_box_temperature", None)
    if tau is None:
        tau = os.environ.get("VLG_GEN_BOX_TEMPERATURE") or None
    if tau is not None:
        knobs["box_temperature"] = box_temperature_options(tau, box_knobs(args).get("box_head", "point"), "VLG_GEN_BOX_TEMPERATURE")
    return knobs


def sample_knobs(args) -> Dict[str, object]:
    """{samples, select} of generate_samples / evaluate_samples in layout mode, from args.gen_samples / VLG_GEN_SAMPLES (1 = off:
    one future per prompt) and args.gen_select / VLG_GEN_SELECT (iou | ade | fde | acc; default iou).  Refuses what
    vlg.samples refuses.  generate_sequence and evaluate_rollout never read them."""
    select = getattr(args, "gen_select", None) or os.environ.get("VLG_GEN_SELECT") or "iou"
    return {"samples": samples_options(_knob(args, "gen_samples", "VLG_GEN_SAMPLES", 1), name="VLG_GEN_SAMPLES")[0],
            "select": select_option(select)}


def clip_cache_knob(args) -> Dict[str, object]:
    """the engine's clip_cache keyword argument from args / environment (module docstring): {} with the knob off"""
    return {"clip_cache": True} if _knob(args, "gen_clip_cache", "VLG_GEN_CLIP_CACHE", 0) else {}


def metrics_knobs(args) -> Dict[str, object]:
    """{on, top_k, iou_thr} of the validation metrics in layout mode, from args / environment (module docstring): off,
    top-5 accuracy and IoU >= 0.5 unless asked otherwise."""
    return {"on": bool(_knob(args, "val_metrics", "VLG_VAL_METRICS", 0)),
            "top_k": _knob(args, "val_topk", "VLG_VAL_TOPK", 5),
            "iou_thr": _knob_float(args, "val_iou_thr", "VLG_VAL_IOU_THR", 0.5)}


def pixel_knobs(args) -> Dict[str, object]:
    """{size: (H, W)} of the rollouts' pixel score in layout mode from args.val_pixels / VLG_VAL_PIXELS = "HxW" (module
    docstring); {} with the knob off (unset, empty or 0).  An (H, W) pair is taken as it is; a size the rasteriser does not
    take raises ValueError here."""
    v = getattr(args, "val_pixels", None)
    if v is None:
        v = os.environ.get("VLG_VAL_PIXELS", "")
    if v in ("", "0", 0, False):
        return {}
    return {"size": raster_options(parse_size(v) if isinstance(v, str) else v, None, N_CLASSES)[0]}


def epoch_lr(args, epoch: int) -> float:
    """Learning rate of 0-based `epoch` under VLG_LR_DECAY=1: args.lr * lr_decay_gamma ** (epoch // lr_decay_step)."""
    return decayed_lr(float(getattr(args, "lr", ADAM_LR)), epoch, int(args.lr_decay_step), float(args.lr_decay_gamma))


def layout_config(args) -> LayoutConfig:
    """Per-GPU batch = batch_size // gpus, as reference src/trainer.py:148 sizes its loaders."""
    gpus = max(int(getattr(args, "gpus", 1) or 1), 1)
    return LayoutConfig(B=max(int(args.batch_size) // gpus, 1), T=_knob(args, "n_frames", "VLG_FRAMES", 16),
                        N=_knob(args, "n_slots", "VLG_SLOTS", 64), d=_knob(args, "d_model", "VLG_DMODEL", 256),
                        n_layers=_knob(args, "n_layers", "VLG_LAYERS", 4),     # (the attention modes: vlg/attention.py)
                        attention=str(getattr(args, "attention", None) or os.environ.get("VLG_ATTENTION", "slot")),
                        **{k: v for k, v in box_knobs(args).items() if k == "box_head"})


def get_layout_engine(args, cfg: Optional[LayoutConfig] = None, engine_factory: Optional[Callable] = None):
    """Model + optimiser state in one object (counterpart of get_gridnet, reference src/trainer.py:81-94:
    build on args.rank's device, Adam(lr=args.lr, betas=(args.beta1, 0.999)), optional --ckpt load)."""
    cfg = cfg or layout_config(args)
    knobs = optim_knobs(args)
    if engine_factory is None:
        from vlg.engine import LayoutEngine          # HIP only; raises without a GPU / without the .so
        device = torch.device("cuda", int(args.rank))
        precision = str(getattr(args, "precision", None) or os.environ.get("VLG_PRECISION", "fp32"))
        engine = LayoutEngine(cfg, device, seed=int(getattr(args, "seed", SEED)),
                              lr=float(getattr(args, "lr", ADAM_LR)), beta1=float(getattr(args, "beta1", ADAM_BETA1)),
                              precision=precision,
                              padded_slots=bool(_knob(args, "variable_n", "VLG_VARIABLE_N", 0)),   # fixed-N feeds hold no padded slots
                              clip_grad=knobs["clip_grad"], skip_nonfinite=knobs["skip_nonfinite"], **recipe_kwargs(knobs),
                              **dropout_knobs(args), **clip_cache_knob(args), **loss_knobs(args), **sched_knobs(args),
                              **augment_knobs(args), **{k: v for k, v in box_knobs(args).items() if k == "box_nll_weight"})
    else:
        engine = engine_factory(cfg, args)
    if knobs["lr_decay"]:                            # guarded from the start, so a checkpoint's lr and skip count are resumed
        engine.set_lr(float(getattr(args, "lr", ADAM_LR)))
    ckpt_path = getattr(args, "ckpt", None)
    if ckpt_path is not None:
        args.logger.info("Loading from ckpt %s" % ckpt_path)
        ckpt = torch.load(ckpt_path, map_location=torch.device("cpu"), weights_only=True)
        if "gridnet" in ckpt:
            engine.load_params(ckpt["gridnet"])
        if "optimizer" in ckpt:
            engine.load_optimizer(ckpt["optimizer"])
    return engine


get_gridnet = get_layout_engine     # reference name (src/trainer.py:81)


def _load_frozen(net, env: str, args) -> None:
    """Weights of a frozen net (HED / VGG19).  `env` names a state_dict file in the reference's / torchvision's key
    format; the authors' HED checkpoint keeps it under 'generator' (reference src/trainer.py:99), other tools under
    'state_dict'.  Without a file the net gets torch's default conv initialisation from the shared seed (identical on
    every rank) - announced at WARNING level, because the edge maps / perceptual term then mean nothing."""
    path = os.environ.get(env)
    if path:
        sd_ = torch.load(path, map_location="cpu", weights_only=True)
        for key in ("generator", "state_dict"):
            if isinstance(sd_, dict) and key in sd_ and isinstance(sd_[key], dict):
                sd_ = sd_[key]
                break
        net.load_state_dict(sd_)
        args.logger.info("%s: loaded %s" % (type(net).__name__, path))
        return
    gi = torch.Generator().manual_seed(int(getattr(args, "seed", SEED)) + 17)
    shp_ = net.reference_shapes()
    net.load_state_dict({k: (torch.rand(v, generator=gi) * 2 - 1) / float(max(1, (v[1] * v[2] * v[3]) if len(v) == 4 else 64)) ** 0.5
                         for k, v in shp_.items()})
    args.logger.warning("%s not set: %s runs with RANDOMLY INITIALISED frozen weights (the trained ones are not in the "
                        "reference repository: src/trainer.py:97 is an author-local path, vgg19(pretrained=True) a download)"
                        % (env, type(net).__name__))


class _ImageModel:
    """Adapter giving vlg.image_engine.ImageEngine the few methods Trainer uses on the layout engine."""

    def __init__(self, args, batch: int):
        from vlg.image_engine import IMAGE_KEYS, ImageEngine
        size = _knob(args, "img_size", "VLG_IMG_SIZE", 256)
        self.size = size
        self.args = args
        self.device = torch.device("cuda", int(args.rank))
        arch = args.arch if args.arch in ("GridNet", "CoordGridNet") else "CoordGridNet"
        from vlg.cityscapes import is_dataset_root
        self.on_disk = is_dataset_root(getattr(args, "train_dir", None))        # reference layout (src/folder.py:14-46)
        # the frozen edge net feeds two of the ten input channels (trainer.py:190-197): needed as soon as frames come
        # from files; the VGG19 term of CombinedLoss (loss.py:61-62) is opt-in - neither net's trained weights ship
        # with the reference (trainer.py:97 is an author-local path, vgg19(pretrained=True) a download)
        with_hed = self.on_disk or bool(_knob(args, "with_hed", "VLG_WITH_HED", 0))
        with_vgg = bool(_knob(args, "with_vgg", "VLG_WITH_VGG", 0))
        self.keys = tuple(k for k in IMAGE_KEYS if not (with_hed and k in ("e1", "e2")))   # HED makes the edge maps itself
        # VLG_PRECISION as for the layout step: bf16 (and bf16_mfma, the same thing here: every tensor is fp32 already) = the
        # 3x3 convolutions on bf16-rounded operands (fp32 tensors, gradients and Adam state: checkpoints are interchangeable
        # with fp32 runs); fp32x3 has no convolution form and runs fp32
        precision = str(getattr(args, "precision", None) or os.environ.get("VLG_PRECISION", "fp32"))
        if precision == "bf16_mfma":
            precision = "bf16"
        knobs = optim_knobs(args)
        if precision == "fp32x3":
            args.logger.warning("VLG_PRECISION=fp32x3 has no convolution form: the pixel model runs its convolutions in fp32")
            precision = "fp32"
        self.engine = ImageEngine(batch, size, size, self.device, arch=arch, lr=float(getattr(args, "lr", ADAM_LR)),
                                  beta1=float(getattr(args, "beta1", ADAM_BETA1)), with_hed=with_hed, with_vgg=with_vgg,
                                  precision=precision, clip_grad=knobs["clip_grad"], skip_nonfinite=knobs["skip_nonfinite"],
                                  **recipe_kwargs(knobs))
        if knobs["lr_decay"]:
            self.engine.set_lr(float(getattr(args, "lr", ADAM_LR)))
        for net, env in ((self.engine.hed, "VLG_HED_CKPT"), (self.engine.vgg, "VLG_VGG_CKPT")):
            if net is not None:
                _load_frozen(net, env, args)
        # torch's default initialisers for Conv2d (U(+-1/sqrt(fan_in)) for weight and bias) and PReLU (0.25), from one
        # generator seeded like every rank's (main.py:57-60) so replicas start identical without a broadcast
        g = torch.Generator().manual_seed(int(getattr(args, "seed", SEED)))
        shapes = self.engine.net.reference_shapes()
        sd = {}
        for k, shp in shapes.items():
            if shp == (1,):
                sd[k] = torch.full(shp, 0.25)
            else:
                fan_in = (shp[1] if len(shp) == 4 else shapes[k[:-len("bias")] + "weight"][1]) * 9
                sd[k] = (torch.rand(shp, generator=g) * 2 - 1) / fan_in ** 0.5
        self.engine.load_state_dict(sd)
        ckpt_path = getattr(args, "ckpt", None)                       # get_gridnet's --ckpt, reference src/trainer.py:85-92
        if ckpt_path is not None:
            args.logger.info("Loading from ckpt %s" % ckpt_path)
            ckpt = torch.load(ckpt_path, map_location=torch.device("cpu"), weights_only=True)
            if "gridnet" in ckpt:
                self.load_params(ckpt["gridnet"])                     # (the reference wrote `generator.` here: Appendix A-1)
            if "optimizer" in ckpt:
                self.load_optimizer(ckpt["optimizer"])
        self.world = max(int(getattr(args, "gpus", 1) or 1), 1)
        self.step_count = 0
        self._rollouts = {}
        self._hed_master = None

    def named_params(self):
        return self.engine.state_dict()

    def ema_named_params(self):
        return self.engine.ema_state_dict()

    def load_params(self, sd):
        self.engine.load_state_dict(sd)

    def optimizer_state(self):
        return self.engine.optimizer_state()

    def load_optimizer(self, st):
        self.engine.load_optimizer(st)

    def set_lr(self, lr: float):
        self.engine.set_lr(lr)

    def optimizer_stats(self):
        return self.engine.optimizer_stats()

    def train_step(self, batch, flip: bool, reducer=None):
        return self.engine.train_step(batch, flip, reducer).reshape(1)

    def eval_loss(self, batch):
        self.engine.forward(batch, flip=False, want_grads=False)
        return self.engine.total().reshape(1)

    def _edge_net(self):
        """The frozen HED net whose weights the rollout's twin reads: the training step's own, or (synthetic-frame
        training feeds edge maps as inputs) one built for the purpose."""
        if self.engine.hed is not None:
            return self.engine.hed
        if self._hed_master is None:
            from vlg.hned import HNEDHIP
            self._hed_master = HNEDHIP(1, 16, 16, self.device)        # weights only; twins are sized per call
            _load_frozen(self._hed_master, "VLG_HED_CKPT", self.args)
        return self._hed_master

    def rollout(self, img1, img2, seg1, seg2, steps: int = 8):
        """reference src/trainer.py:453-476 on the HIP nets (vlg.image_engine.FrameRollout)."""
        from vlg.image_engine import FrameRollout
        b, _, H, W = img1.shape
        key = (int(b), int(H), int(W))
        if key not in self._rollouts:
            self._rollouts[key] = FrameRollout(self.engine, self._edge_net(), *key)
        return self._rollouts[key].run(img1, img2, seg1, seg2, steps)


class _ModelHandle:
    """`trainer.model` / `trainer.gridnet`: main.py:65 calls trainer.model.eval()."""

    def __init__(self, engine):
        self.engine, self.training = engine, True

    def train(self, mode: bool = True):
        self.training = mode
        return self

    def eval(self):
        return self.train(False)

    def state_dict(self):
        return {k: v.detach().cpu().clone() for k, v in self.engine.named_params().items()}

    def load_state_dict(self, sd):
        self.engine.load_params(sd)


class Trainer:

    def __init__(self, args, engine_factory: Optional[Callable] = None):
        args.logger.info("Initializing trainer")
        # reference src/trainer.py:107-108 creates ../predict relative to the working directory (src/); the default is kept,
        # args.predict_dir / VLG_PREDICT_DIR move it (tests, read-only working directories)
        self.predict_dir = str(getattr(args, "predict_dir", None) or os.environ.get("VLG_PREDICT_DIR") or "../predict")
        if not os.path.isdir(self.predict_dir):
            os.makedirs(self.predict_dir, exist_ok=True)
        self.args = args
        self.world = max(int(getattr(args, "gpus", 1) or 1), 1)
        self.distributed = dist.is_available() and dist.is_initialized() and self.world > 1
        if torch.cuda.is_available() and engine_factory is None:
            torch.cuda.set_device(int(args.rank))               # reference src/trainer.py:110
        self.cfg = layout_config(args)
        self.dropout = dropout_knobs(args)                      # (out-of-range values raise here, before any engine exists)
        self.image_mode = engine_factory is None and os.environ.get("VLG_MODEL", "layout").lower() == "gridnet"
        self.reducer = None
        if self.image_mode and self.dropout:
            raise ValueError("VLG_DROPOUT is a knob of the layout-token step; VLG_MODEL=gridnet has no dropout")
        if sched_knobs(args) and self.image_mode:               # (out-of-range values raise here too)
            raise ValueError("VLG_SCHED_SAMPLING is a knob of the layout-token step; VLG_MODEL=gridnet has no token inputs to sample")
        if augment_knobs(args) and self.image_mode:             # (out-of-range values raise here too)
            raise ValueError("VLG_AUG_* are knobs of the layout-token step; VLG_MODEL=gridnet flips its frames in vlg_prep_input")
        # the HIP engine flips per clip: the host's per-batch _flip stands down (an injected engine is handed no aug_* knob)
        self.device_flip = device_flip(args) and engine_factory is None
        if loss_knobs(args) and self.image_mode:                # (out-of-range values raise here too)
            raise ValueError("VLG_CLASS_WEIGHTS / VLG_LABEL_SMOOTHING / VLG_BOX_OVERLAP are knobs of the layout-token step; "
                             "VLG_MODEL=gridnet's losses have no options")
        if self.image_mode:
            self.engine = _ImageModel(args, self.cfg.B)
            if self.distributed:                                # replaces DDP(gridnet), trainer.py:113: bucket per grid column
                net = self.engine.engine.net
                self.reducer = GradReducer(net.grads_ext, net.bucket_ranges())
        else:
            self.engine = get_layout_engine(args, self.cfg, engine_factory)
            if self.distributed:                                # replaces the DDP wrappers, trainer.py:113,115
                self.reducer = GradReducer(self.engine.grads_ext,       # (the loss scalars' tail: LayoutConfig.loss_tail)
                                           bucket_ranges(self.engine.layout, self.engine.n_params, self.cfg.n_layers,
                                                         tail_extra=self.cfg.loss_tail))
        self.device = self.engine.device
        self.gridnet = self.model = _ModelHandle(self.engine)   # reference attr `gridnet`; main.py:65 wants `.model`
        self.optim = optim_knobs(args)
        self.guarded = bool(self.optim["clip_grad"] > 0.0 or self.optim["skip_nonfinite"] or self.optim["lr_decay"]
                            or recipe_kwargs(self.optim))
        self.global_step = 0
        self.epoch = 0
        if getattr(args, "resume", None) is not None:           # reference src/trainer.py:138-139
            self.load_checkpoint(args.resume)
        self.writer = _make_writer(args.path) if int(args.rank) == 0 else None   # trainer.py:141-142

        seed = int(getattr(args, "seed", SEED))
        variable_n = bool(_knob(args, "variable_n", "VLG_VARIABLE_N", 0))
        n_train = _knob(args, "train_clips", "VLG_TRAIN_CLIPS", 1024)
        n_val = _knob(args, "val_clips", "VLG_VAL_CLIPS", 256)
        common = dict(batch=self.cfg.B, rank=int(args.rank), world=self.world, seed=seed)
        if self.device.type == "cuda":       # device batches, pinned staging + one batch ahead on a side stream (vlg/data.py)
            common["device"] = self.device
        if self.image_mode and self.engine.on_disk:
            # the reference's own data: frame triplets from <train_dir>/{deeplab256_label,leftImg256}/<city>/ (folder.py)
            from vlg.cityscapes import TripletFolder, TripletLoader
            val_dir = getattr(args, "val_dir", None) or args.train_dir
            common["device"] = self.device
            self.train_loader = TripletLoader(TripletFolder(args.train_dir), shuffle=True, **common)
            self.val_loader = TripletLoader(TripletFolder(val_dir), shuffle=False, **common)
            args.logger.debug("Finish init trainer")
            return
        if self.image_mode:
            from vlg.image_engine import synthetic_frames
            sz = self.engine.size
            train_clips, val_clips = synthetic_frames(n_train, sz, sz, seed=seed), synthetic_frames(n_val, sz, sz, seed=seed + 1)
            Loader, common["keys"] = ClipLoader, self.engine.keys
        else:
            mk = dict(T=self.cfg.T, N=self.cfg.N, n_classes=self.cfg.n_classes, variable_n=variable_n)
            train_clips = synthetic_clips(n_train, seed=seed, **mk)      # get_dataset(), trainer.py:144
            val_clips = synthetic_clips(n_val, seed=seed + 1, **mk)
            Loader = BucketedClipLoader if variable_n else ClipLoader
        self.train_loader = Loader(train_clips, shuffle=True, **common)   # DistributedSampler + DataLoader, :145-152
        self.val_loader = Loader(val_clips, shuffle=False, **common)
        args.logger.debug("Finish init trainer")

    # ----------------------------------------------------------------- epoch control
    def set_epoch(self, epoch):
        """0-based in, 1-based stored, samplers reseeded (reference src/trainer.py:158-162)."""
        self.args.logger.info("Start of epoch %d" % (epoch + 1))
        self.epoch = epoch + 1
        if self.optim["lr_decay"]:
            self.engine.set_lr(epoch_lr(self.args, epoch))
        self.train_loader.set_epoch(epoch)
        self.val_loader.set_epoch(epoch)

    # ------------------------------------------------------------------------- train
    def _flip(self, batch: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """Horizontal flip of a layout = cx -> 1 - cx on inputs AND targets.  Drawn from the shared-seed
        `random` stream exactly like reference src/trainer.py:200-206, so all ranks flip together."""
        if random.random() < 0.5:
            batch = dict(batch)
            for k in ("slot_box", "tgt_box"):
                b = batch[k].clone()
                b[..., 0] = 1.0 - b[..., 0]
                batch[k] = b
        return batch

    def train(self):
        self.args.logger.info("Training started")
        self.gridnet.train()
        end = time()
        n_batches = len(self.train_loader)
        for i, batch in enumerate(self.train_loader):
            if self.image_mode:                                   # flip is done by vlg_prep_input (trainer.py:200-206)
                flip = random.random() < 0.5
                batch = to_device(batch, self.device, self.engine.keys)
            else:
                # H2D, reference src/trainer.py:184-187 (with VLG_AUG_FLIP the engine flips per clip on the device instead)
                batch = to_device(batch if self.device_flip else self._flip(batch), self.device)
            load_time = time() - end
            end = time()
            self.global_step += 1
            # forward, 40/20/10 loss, backward, bucketed all-reduce, Adam: reference src/trainer.py:209-258
            if self.image_mode:
                loss = self.engine.train_step(batch, flip, self.reducer)
            else:
                loss = self.engine.train_step(batch, self.reducer)
            if int(self.args.rank) == 0 and i % int(self.args.print_freq) == 0:
                # with a reducer the loss floats were summed over ranks inside a gradient bucket (the first one of
                # the token step, the last one of the pixel step): logged value = cross-rank mean, as sync() gave the
                # reference (trainer.py:256), without a collective of its own
                value = float(loss[0].item()) / (self.world if self.reducer is not None else 1)
                # guarded step: its device record is read here only, next to the loss (one 64-byte copy)
                stats = self.engine.optimizer_stats() if self.guarded else None
                comp_time = time() - end
                self.args.logger.info(
                    "Epoch [{epoch:d}/{tot_epoch:d}][{cur_batch:d}/{tot_batch:d}] "
                    "load [{load_time:.3f}s] comp [{comp_time:.3f}s] "
                    "loss [{loss:.4f}]".format(epoch=self.epoch, tot_epoch=int(self.args.epochs), cur_batch=i + 1,
                                               tot_batch=n_batches, load_time=load_time, comp_time=comp_time,
                                               loss=value)
                    + (" grad_norm [{grad_norm:.4g}] skipped [{skipped_steps:d}]".format(**stats) if stats else ""))
                self.writer.add_scalar("train/gen loss GAN", value, self.global_step)   # tag: trainer.py:281
                if stats:
                    self.writer.add_scalar("train/grad_norm", stats["grad_norm"], self.global_step)
                    self.writer.add_scalar("train/lr", stats["lr"], self.global_step)
            end = time()

    def _eval_weights(self):
        """The weights evaluation and generation run on: the moving average (LayoutEngine.ema_weights()) when it is on and
        VLG_EMA_EVAL is, else the live weights.  Layout mode only: the pixel model is not evaluated under its average."""
        if self.optim.get("ema_eval") and not self.image_mode and hasattr(self.engine, "ema_weights"):
            return self.engine.ema_weights()
        return contextlib.nullcontext()

    # ---------------------------------------------------------------------- validate
    def validate(self):
        with self._eval_weights():
            return self._validate()

    def _validate(self):
        self.args.logger.info("Validation started")
        self.gridnet.eval()
        val_loss = AverageMeter()
        box_head = not self.image_mode and getattr(self.cfg, "gaussian_box", False)
        box_nll, box_cover = AverageMeter(), AverageMeter()
        mk = metrics_knobs(self.args)
        record = None
        if mk["on"] and not self.image_mode:
            if not hasattr(self.engine, "accumulate_metrics"):
                raise ValueError("VLG_VAL_METRICS=1 needs an engine with accumulate_metrics() (vlg.engine.LayoutEngine: the "
                                 "vlg_layout_metrics kernel); %s has none" % type(self.engine).__name__)
            record = self.engine.metrics_record()
        end = time()
        n_batches = len(self.val_loader)
        for i, batch in enumerate(self.val_loader):
            keys = self.engine.keys if self.image_mode else BATCH_KEYS
            batch = to_device(batch, self.device, keys)
            load_time = time() - end
            end = time()
            if self.image_mode:
                loss = self.engine.eval_loss(batch).clone()
            else:
                scalars = self.engine.forward(batch)                # forward only, reference src/trainer.py:320-333
                loss = scalars[0:1].clone()
                if box_head:                                        # the Gaussian box head's {box_nll, box_cover}
                    box = scalars[4:6].clone()
                if record is not None:                              # one launch, adds to the device record; no host wait
                    self.engine.accumulate_metrics(batch, record, top_k=mk["top_k"], iou_thr=mk["iou_thr"])
            size = torch.tensor([float(batch[keys[0]].shape[0])], device=loss.device)
            loss.mul_(size)
            self.sync([loss, size], mean=False)                     # size-weighted SUM, trainer.py:336-338
            loss.div_(size)                                         # / GLOBAL clip count (see module docstring)
            val_loss.update(loss.item(), size.item())
            if box_head:                                            # the same size-weighted mean over the ranks
                box.mul_(float(batch[keys[0]].shape[0]))            # (size is the global count by now)
                self.sync([box], mean=False)
                box.div_(size)
                box_nll.update(box[0].item(), size.item())
                box_cover.update(box[1].item(), size.item())
            comp_time = time() - end
            end = time()
            if int(self.args.rank) == 0 and i % int(self.args.print_freq) == 0:
                self.args.logger.info(
                    "Epoch [{epoch:d}/{tot_epoch:d}][{cur_batch:d}/{tot_batch:d}] "
                    "load [{load_time:.3f}s] comp [{comp_time:.3f}s]".format(
                        epoch=self.epoch, tot_epoch=int(self.args.epochs), cur_batch=i + 1, tot_batch=n_batches,
                        load_time=load_time, comp_time=comp_time))
        if int(self.args.rank) == 0:
            self.args.logger.info("Epoch [{epoch:d}/{tot_epoch:d}] loss [{loss:.4f}] ".format(
                epoch=self.epoch, tot_epoch=int(self.args.epochs), loss=val_loss.avg))
            self.writer.add_scalar("val/loss", val_loss.avg, self.epoch)                # trainer.py:377
        extra = {"box_nll": box_nll.avg, "box_cover": box_cover.avg} if box_head else {}
        if box_head and int(self.args.rank) == 0:
            self.writer.add_scalar("val/box_nll", box_nll.avg, self.epoch)
            self.writer.add_scalar("val/box_cover", box_cover.avg, self.epoch)
        if record is None:
            return dict({"loss": val_loss.avg}, **extra)                                # trainer.py:379
        record.all_reduce(lambda tensors: self.sync(tensors, mean=False))               # counts and sums are additive
        summary = record.summary()[0]                                                   # the pass's one read of the record
        if int(self.args.rank) == 0:
            self.args.logger.info(
                "Epoch [%d/%d] scored [%d] accuracy [%s] top%d [%s] nll [%s] mean_iou [%s] iou>=%g [%s] nonfinite [%d]"
                % (self.epoch, int(self.args.epochs), summary["scored"], _fmt(summary["accuracy"]), mk["top_k"],
                   _fmt(summary["topk_accuracy"]), _fmt(summary["nll"]), _fmt(summary["mean_iou"]), mk["iou_thr"],
                   _fmt(summary["iou_hit"]), summary["nonfinite"]))
            for key in ("accuracy", "mean_iou", "nll", "iou_hit"):
                if summary[key] is not None:
                    self.writer.add_scalar("val/" + key, summary[key], self.epoch)
        return dict(summary, loss=val_loss.avg, **extra)

    def sync(self, tensors, mean=True):
        """Synchronize all tensors given using mean or sum (reference src/trainer.py:381-386)."""
        if not self.distributed:
            return
        for tensor in tensors:
            dist.all_reduce(tensor)
            if mean:
                tensor.div_(self.world)

    # ------------------------------------------------------------------- checkpoints
    def save_checkpoint(self, metrics):
        """Rank 0 only (reference src/main.py:81-82): ../checkpoint/%03d.pth + latest.pth
        (reference src/trainer.py:390-402), schema {'epoch','arch','gridnet','optimizer'}."""
        self.args.logger.info("Saving checkpoint..")
        prefix = "../checkpoint"
        os.makedirs(prefix, exist_ok=True)
        ckpt = {"epoch": self.epoch, "arch": self.args.arch, "gridnet": self.gridnet.state_dict(),
                "optimizer": self.engine.optimizer_state(), "metrics": dict(metrics or {})}
        if self.optim.get("ema_decay") and hasattr(self.engine, "ema_named_params"):
            # the averaged model, in 'gridnet''s format: {'gridnet': ckpt['gridnet_ema']} is a checkpoint --ckpt loads as a model
            ckpt["gridnet_ema"] = {k: v.detach().cpu().clone() for k, v in self.engine.ema_named_params().items()}
        torch.save(ckpt, "%s/%03d.pth" % (prefix, self.epoch))
        shutil.copy("%s/%03d.pth" % (prefix, self.epoch), "%s/latest.pth" % prefix)

    def load_checkpoint(self, resume):
        """--resume (reference src/trainer.py:404-414): arch must match; restores epoch, weights, Adam state - and, when an
        optimiser knob is on (guarded engine), the learning rate and the skipped-step count the entry records."""
        self.args.logger.info("Resuming checkpoint %s" % resume)
        ckpt = torch.load(resume, map_location=torch.device("cpu"), weights_only=True)
        assert ckpt["arch"] == self.args.arch, ("Architecture mismatch: ckpt %s, config %s"
                                                % (ckpt["arch"], self.args.arch))
        self.epoch = ckpt["epoch"]
        self.gridnet.load_state_dict(ckpt["gridnet"])
        self.engine.load_optimizer(ckpt["optimizer"])
        self.args.logger.info("Checkpoint loaded")

    # ----------------------------------------------------------------------- rollout
    def generate_sequence(self, *inputs, steps: int = 8, temperature: Optional[float] = None, top_k: Optional[int] = None,
                          seed: Optional[int] = None, keep_padded: Optional[bool] = None):
        """Autoregressive rollout, `steps` predictions (8 in reference src/trainer.py:460).

        VLG_MODEL=gridnet - the reference's own method: generate_sequence(img1, img2, seg1, seg2) with two
        ImageNet-normalised frames (b,3,H,W) and two segmentation-id maps (b,1,H,W) (what eval_generate_sequence passes,
        trainer.py:440-451).  Runs trainer.py:453-476 on the HIP nets (Appendix A-10 repaired: vlg/image_engine.py
        FrameRollout), writes ../predict/val_<time>_{img,seg}.npy like trainer.py:474-476 and ALSO returns the two
        arrays (b, 3*(steps+2), H, W), (b, steps+2, H, W).

        Layout mode: generate_sequence(slot_class (B,P,N), slot_box (B,P,N,4)) with a prompt of 1 <= P <= T frames: predict
        the frame after the history, append it, and once the history fills the T-frame window slide it; returns classes
        (B,steps,N) and boxes (B,steps,N,4) on the CPU.  A prompt shorter than T (the reference's generate_sequence starts
        from two observed frames) grows to T with a K/V cache where the engine has one (LayoutEngine.rollout).
        temperature / top_k / seed / keep_padded: None takes the generation knob from args or the environment
        (generation_knobs; the module docstring says what each does).  An engine with rollout()
        (vlg.engine.LayoutEngine) generates on the device, without a host wait per frame, and the result is copied to the
        CPU once; any other engine runs the host loop, which can only take the argmax of a full T-frame prompt."""
        if self.image_mode:
            if len(inputs) != 4:
                raise TypeError("generate_sequence(img1, img2, seg1, seg2) in VLG_MODEL=gridnet mode")
            import numpy as np
            p, q = self.engine.rollout(*inputs, steps=steps)
            p, q = p.cpu().numpy(), q.cpu().numpy()
            t = time()
            os.makedirs(self.predict_dir, exist_ok=True)
            np.save(os.path.join(self.predict_dir, "val_" + str(t) + "_img.npy"), p)     # trainer.py:474-476
            np.save(os.path.join(self.predict_dir, "val_" + str(t) + "_seg.npy"), q)
            return p, q
        if len(inputs) != 2:
            raise TypeError("generate_sequence(slot_class, slot_box) in layout mode")
        slot_class, slot_box = inputs
        knobs = generation_knobs(self.args)
        for name, given in (("temperature", temperature), ("top_k", top_k), ("seed", seed), ("keep_padded", keep_padded)):
            if given is not None:
                knobs[name] = type(knobs[name])(given)
        if hasattr(self.engine, "rollout"):
            with self._eval_weights():
                gen_c, gen_b = self.engine.rollout(slot_class.to(self.device).contiguous(), slot_box.to(self.device).contiguous(),
                                                   steps=steps, **knobs)
            return gen_c.cpu(), gen_b.cpu()
        if knobs["temperature"] != 0.0 or knobs["keep_padded"]:
            raise ValueError("temperature > 0 and keep_padded need an engine with rollout() (vlg.engine.LayoutEngine: the "
                             "vlg_layout_decode kernel); %s has none, its host loop takes the argmax of every slot"
                             % type(self.engine).__name__)
        if slot_class.shape[1] != self.cfg.T:
            raise ValueError("a prompt of %d frames needs an engine with rollout() (vlg.engine.LayoutEngine grows a short "
                             "history to the window); the host loop of %s takes exactly T=%d frames"
                             % (slot_class.shape[1], type(self.engine).__name__, self.cfg.T))
        cls = slot_class.clone().to(self.device)
        box = slot_box.clone().to(self.device)
        B, T, N = cls.shape
        out_c, out_b = [], []
        dummy = {"tgt_class": torch.zeros_like(cls), "tgt_box": torch.zeros_like(box)}
        for _ in range(steps):
            # valid: padded slots carry the reserved class id (vlg/data.py) - with attention = "clip" they must not be attended
            # to; the loss the forward also evaluates against the dummy targets is not used.  An engine built for fixed-N
            # training skips the masks (padded_slots False): it is told to mask a window that holds a padded slot
            valid = (cls < self.cfg.n_classes).to(torch.float32).contiguous()
            kw = {}
            if not getattr(self.engine, "padded_slots", True) and bool((valid == 0).any()):
                kw["padded_slots"] = True
            self.engine.forward(dict(dummy, slot_class=cls.contiguous(), slot_box=box.contiguous(), valid=valid), **kw)
            logits, raw = self.engine.outputs_btn()
            nc = torch.argmax(logits[:, -1], dim=-1)                 # (B,N), as trainer.py:467
            nb = torch.sigmoid(raw[:, -1])
            out_c.append(nc.cpu())
            out_b.append(nb.cpu())
            cls = torch.cat([cls[:, 1:], nc[:, None]], dim=1)
            box = torch.cat([box[:, 1:], nb[:, None]], dim=1)
        return torch.stack(out_c, dim=1), torch.stack(out_b, dim=1)

    def evaluate_rollout(self, clip_class, clip_box, temperature: Optional[float] = None, top_k: Optional[int] = None,
                         seed: Optional[int] = None, keep_padded: Optional[bool] = None, val_topk: Optional[int] = None,
                         val_iou_thr: Optional[float] = None, prompt_frames: Optional[int] = None):
        """Layout mode: how prediction quality decays with the horizon.  clip_class (B,P+S,N) / clip_box (B,P+S,N,4), CPU or
        device tensors: the first P = prompt_frames frames (None: T; 1 <= P <= T) prompt a rollout of S steps, and step i is
        scored against frame P+i of the clip on the device (vlg.engine.LayoutEngine.evaluate_rollout; one host read at the end).  temperature / top_k /
        seed / keep_padded are the generation knobs of generate_sequence (None = from args or the environment);
        val_topk / val_iou_thr the metric's (None = metrics_knobs).  A step is scored on the model's distribution at that
        step (arg-max, rank and NLL of the logits, box = sigmoid(raw)), also when the history was sampled.
        Returns a list of S summary dicts (vlg/metrics.py), one per horizon step.  With the pixel knob on (pixel_knobs) the
        decoded frames and the true ones are also drawn and compared pixel by pixel (LayoutEngine.evaluate_rollout's
        pixel_record), and each dict gains pixel_miou, pixel_accuracy, pixel_per_class_iou and pixel_background_iou."""
        if self.image_mode or not hasattr(self.engine, "evaluate_rollout"):
            raise ValueError("evaluate_rollout needs the layout engine with evaluate_rollout() (vlg.engine.LayoutEngine: the "
                             "vlg_layout_metrics kernel); %s has none" % type(self.engine).__name__)
        knobs = generation_knobs(self.args)
        for name, given in (("temperature", temperature), ("top_k", top_k), ("seed", seed), ("keep_padded", keep_padded)):
            if given is not None:
                knobs[name] = type(knobs[name])(given)
        mk = metrics_knobs(self.args)
        pk, pixels = pixel_knobs(self.args), {}
        if pk:
            P = self.cfg.T if prompt_frames is None else int(prompt_frames)
            pixels = {"pixel_record": self.engine.pixel_record(max(1, clip_class.shape[1] - P)), "pixel_size": pk["size"]}
        with self._eval_weights():
            record = self.engine.evaluate_rollout(
                clip_class.to(self.device).contiguous(), clip_box.to(self.device).contiguous(),
                top_k=mk["top_k"] if val_topk is None else int(val_topk),
                iou_thr=mk["iou_thr"] if val_iou_thr is None else float(val_iou_thr),
                temperature=knobs["temperature"], sample_top_k=knobs["top_k"], seed=knobs["seed"], keep_padded=knobs["keep_padded"],
                prompt_frames=prompt_frames, **pixels,
                **({"box_temperature": knobs["box_temperature"]} if "box_temperature" in knobs else {}))
        out = record.summary()
        if pk:
            for s, p in zip(out, pixels["pixel_record"].summary()):
                s.update(pixel_miou=p["miou"], pixel_accuracy=p["pixel_accuracy"], pixel_per_class_iou=p["per_class_iou"],
                         pixel_background_iou=p["background_iou"])
        return out

    def _sampling_knobs(self, what: str, temperature, top_k, seed, keep_padded, samples) -> tuple:
        """(generation knobs with the given overrides, samples) for the two *_samples methods"""
        if self.image_mode or not hasattr(self.engine, "rollout_samples"):
            raise ValueError("%s needs the layout engine with rollout_samples() (vlg.engine.LayoutEngine: the "
                             "vlg_layout_decode_samples kernels); %s has none" % (what, type(self.engine).__name__))
        knobs = generation_knobs(self.args)
        for name, given in (("temperature", temperature), ("top_k", top_k), ("seed", seed), ("keep_padded", keep_padded)):
            if given is not None:
                knobs[name] = type(knobs[name])(given)
        return knobs, sample_knobs(self.args)["samples"] if samples is None else samples_options(samples)[0]

    def generate_samples(self, slot_class, slot_box, steps: int = 8, samples: Optional[int] = None,
                         temperature: Optional[float] = None, top_k: Optional[int] = None, seed: Optional[int] = None,
                         keep_padded: Optional[bool] = None):
        """Layout mode: K = `samples` futures of every prompt from one seed in one device rollout
        (vlg.engine.LayoutEngine.rollout_samples): slot_class (B,P,N) / slot_box (B,P,N,4) as generate_sequence takes them;
        returns classes (K,B,steps,N) and boxes (K,B,steps,N,4) on the CPU.  samples: None takes args.gen_samples /
        VLG_GEN_SAMPLES (sample_knobs; 1 gives generate_sequence's own sequence with a leading axis of 1); the other
        arguments and knobs are generate_sequence's, the averaged weights are used where it uses them."""
        knobs, K = self._sampling_knobs("generate_samples", temperature, top_k, seed, keep_padded, samples)
        with self._eval_weights():
            gen_c, gen_b = self.engine.rollout_samples(slot_class.to(self.device).contiguous(), slot_box.to(self.device).contiguous(),
                                                       steps=steps, samples=K, **knobs)
        return gen_c.cpu(), gen_b.cpu()

    def evaluate_samples(self, clip_class, clip_box, samples: Optional[int] = None, select: Optional[str] = None,
                         temperature: Optional[float] = None, top_k: Optional[int] = None, seed: Optional[int] = None,
                         keep_padded: Optional[bool] = None, prompt_frames: Optional[int] = None):
        """Layout mode: how good the model's DISTRIBUTION over futures is.  clip_class (B,P+S,N) / clip_box (B,P+S,N,4) as
        evaluate_rollout takes them; K = `samples` futures of the P-frame prompt are drawn in one rollout and scored against
        the S frames that really followed on the device (vlg.engine.LayoutEngine.evaluate_samples; one host read at the
        end).  samples / select: None takes args.gen_samples / VLG_GEN_SAMPLES and args.gen_select / VLG_GEN_SELECT
        (sample_knobs); the other arguments are evaluate_rollout's.  Returns one dict (vlg.samples.SampleRecord.summary):
        best_iou / best_ade / best_fde / best_acc - the best of the K samples per clip, averaged over clips (minADE, minFDE) -
        mean_* over the samples, selected_* at the sample `select` picked, diversity_box, diversity_class and clips."""
        knobs, K = self._sampling_knobs("evaluate_samples", temperature, top_k, seed, keep_padded, samples)
        select = sample_knobs(self.args)["select"] if select is None else select_option(select)
        with self._eval_weights():
            record = self.engine.evaluate_samples(
                clip_class.to(self.device).contiguous(), clip_box.to(self.device).contiguous(), samples=K, select=select,
                temperature=knobs["temperature"], sample_top_k=knobs["top_k"], seed=knobs["seed"], keep_padded=knobs["keep_padded"],
                prompt_frames=prompt_frames,
                **({"box_temperature": knobs["box_temperature"]} if "box_temperature" in knobs else {}))
        return record.summary()

    def render_layout(self, slot_class, slot_box, size=None, valid=None, what: str = "class", dtype=torch.float32):
        """Layout mode: draw layouts into label maps on the device (LayoutEngine.rasterize) and return them on the CPU.
        slot_class (B,T,N) / slot_box (B,T,N,4) / valid (B,T,N) or None, CPU or device tensors; size = (H, W), None takes
        the pixel knob's (pixel_knobs).  Returns (B,T,H,W) of `dtype`: with the default float32, [:, t:t+1] is a
        segmentation-id argument of the pixel model's generate_sequence; what = "slot" gives slot indices instead of
        classes."""
        if self.image_mode or not hasattr(self.engine, "rasterize"):
            raise ValueError("render_layout needs the layout engine with rasterize() (vlg.engine.LayoutEngine: the "
                             "vlg_layout_rasterize kernel); %s has none" % type(self.engine).__name__)
        if size is None:
            size = pixel_knobs(self.args).get("size")
            if size is None:
                raise ValueError("render_layout needs size=(H, W) or the pixel knob (args.val_pixels / VLG_VAL_PIXELS=HxW)")
        v = None if valid is None else valid.to(self.device, torch.float32).contiguous()
        return self.engine.rasterize(slot_class.to(self.device).contiguous(), slot_box.to(self.device).contiguous(), size,
                                     valid=v, what=what, dtype=dtype).cpu()

    def eval_generate_sequence(self, img1, img2, seg1, seg2):
        """main.py:64-67 entry (reference src/trainer.py:429-451): read two frames and two segmentation-id maps from
        files, resize the maps to 256 x 256 nearest-neighbour (:439-440; cv2.INTER_NEAREST index rule, vlg/cityscapes.py),
        ToTensor + ImageNet-normalise the frames (:443-447), then generate_sequence.  PIL decodes the files (cv2 is not
        installed here).  An unreadable path logs and returns like :436-438.  A layout-token model has no pixel
        inputs: there the method logs an error and returns None, so that `main.py --img1 ...` (main.py:64-67) ends the
        way the reference's entry does for unusable inputs - a log line, not a traceback."""
        if not self.image_mode:
            self.args.logger.error("eval_generate_sequence reads image files: run with VLG_MODEL=gridnet "
                                   "(layout mode rolls out with generate_sequence(slot_class, slot_box))")
            return None
        from vlg.cityscapes import _load_rgb, _load_seg
        from vlg.spec import IMG_MEAN, IMG_STD
        for pth in (img1, img2, seg1, seg2):
            if not (isinstance(pth, str) and os.path.isfile(pth)):
                self.args.logger.debug("path name not exists")                    # trainer.py:436-438
                return None
        size = self.engine.size
        frames = [_load_rgb(pth) for pth in (img1, img2)]
        segs = [_load_seg(pth, (size, size)).float()[None, None] for pth in (seg1, seg2)]
        for f in frames:
            if tuple(f.shape[1:]) != (size, size):
                raise ValueError("frames must be %d x %d like the reference's pre-scaled leftImg256 (got %s)"
                                 % (size, size, tuple(f.shape[1:])))
        mean = torch.tensor(IMG_MEAN)[:, None, None]
        std = torch.tensor(IMG_STD)[:, None, None]
        frames = [((f - mean) / std)[None] for f in frames]                       # transforms.Normalize, :443-447
        self.args.logger.debug(segs[0].shape)
        self.args.logger.debug(frames[0].shape)
        return self.generate_sequence(frames[0], frames[1], segs[0], segs[1])
