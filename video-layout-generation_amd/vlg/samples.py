"""Host side of the sampled futures: the running record vlg_layout_sample_select (csrc/samples.hip) adds to, the one place it
is read, and the option rules of LayoutEngine.rollout_samples / evaluate_samples.

A SampleRecord is VLG_SMP_REC_SLOTS zeroed float64 sums in the slot order of include/vlg_hip.h (VLG_SMP_REC_*), summed over
the clips that had a scored token.  Launches only ever add to it, so nothing waits for the device until summary() copies it
to the host, once.  It can live on the CPU, where its arithmetic is tested without a GPU.
"""
from __future__ import annotations

from typing import Callable, Dict, Optional

import torch

from . import cabi

COLS, IOU, ADE, FDE, ACC, N_SCORED, N_SCORED_LAST = cabi.values(
    "VLG_SMP_", "COLS", "IOU", "ADE", "FDE", "ACC", "N_SCORED", "N_SCORED_LAST")
REC_BEST, REC_MEAN, REC_SELECTED, REC_DIV_BOX, REC_DIV_CLASS, REC_CLIPS, REC_CLIPS_FDE, REC_SLOTS = cabi.values(
    "VLG_SMP_REC_", "BEST", "MEAN", "SELECTED", "DIV_BOX", "DIV_CLASS", "CLIPS", "CLIPS_FDE", "SLOTS")
# select= of evaluate_samples -> the score column vlg_layout_sample_select chooses by (iou, acc: largest; ade, fde: smallest)
CRITERIA = {"iou": IOU, "ade": ADE, "fde": FDE, "acc": ACC}


def select_option(select) -> str:
    """the legal values of select= / args.gen_select / VLG_GEN_SELECT"""
    s = str(select).lower()
    if s not in CRITERIA:
        raise ValueError("select must be one of %s, got %r" % (", ".join(CRITERIA), select))
    return s


def samples_options(samples, sample0=0, name: str = "samples") -> tuple:
    """(samples, sample0) as ints: samples >= 1, sample0 >= 0, and the last sample index a 31-bit counter word"""
    try:
        k, k0 = int(samples), int(sample0)
    except (TypeError, ValueError):
        raise ValueError("%s must be an integer >= 1, got %r" % (name, samples)) from None
    if k < 1 or k0 < 0 or k0 + k > 0x7FFFFFFF or k != samples or k0 != sample0:
        raise ValueError("%s must be an integer >= 1 and sample0 >= 0 with sample0 + samples < 2^31, got %r, %r"
                         % (name, samples, sample0))
    return k, k0


def sample_passes(samples: int, sample0: int, clip_tokens: int, capacity: int) -> list:
    """How rollout_samples fits K samples of a batch whose window holds `clip_tokens` = B*T*N tokens into a workspace of
    `capacity` tokens: a list of (first sample index, samples) passes, each of k_fit = capacity // clip_tokens samples but
    the last.  ValueError if not even one sample fits."""
    k_fit = capacity // clip_tokens
    if k_fit < 1:
        raise ValueError("one sample's window of %d tokens exceeds workspace capacity %d" % (clip_tokens, capacity))
    return [(sample0 + k, min(k_fit, samples - k)) for k in range(0, samples, k_fit)]


class SampleRecord:
    def __init__(self, device=None):
        self.device = torch.device(device) if device is not None else torch.device("cpu")
        self.sums = torch.zeros(REC_SLOTS, dtype=torch.float64, device=self.device)

    def reset(self) -> None:
        self.sums.zero_()

    def all_reduce(self, sync: Callable) -> None:
        """Sum over ranks with `sync`, a callable taking a list of tensors and summing each in place; every slot is additive."""
        sync([self.sums])

    def summary(self) -> Dict[str, Optional[float]]:
        """The record's only host read.  best_*: the mean over the counted clips of the best value any of the K samples
        reached (iou, acc: the largest; ade, fde: the smallest - minADE / minFDE); mean_*: of the mean over the K samples;
        selected_*: of the value at the sample the call's criterion selected; diversity_box / diversity_class: of the clip's
        pairwise diversity; clips: the clips counted (those with a scored token; the fde figures divide by the clips with a
        scored token in the last frame).  With nothing to divide by a figure is None."""
        s = self.sums.cpu().tolist()
        n, n_fde = s[REC_CLIPS], s[REC_CLIPS_FDE]
        out: Dict[str, Optional[float]] = {}
        for kind, base in (("best", REC_BEST), ("mean", REC_MEAN), ("selected", REC_SELECTED)):
            for name, col in CRITERIA.items():
                d = n_fde if col == FDE else n
                out["%s_%s" % (kind, name)] = s[base + col] / d if d > 0 else None
        out["diversity_box"] = s[REC_DIV_BOX] / n if n > 0 else None
        out["diversity_class"] = s[REC_DIV_CLASS] / n if n > 0 else None
        out["clips"] = int(n)
        return out
