"""Host side of the validation metrics: the running record vlg_layout_metrics (csrc/metrics.hip) adds to, and the one place
it is read.

A MetricsRecord is two zeroed tensors - counts (rows, NCOUNT) int64 and sums (rows, NSUM) float64 - in the slot order of
include/vlg_hip.h (VLG_MET_*).  One row per thing scored separately (a validation pass: one row; a rollout: one row per
horizon step).  Launches only ever add to it, so nothing waits for the device until summary() copies both tensors to the
host, once.  It can live on the CPU, where its arithmetic is tested without a GPU.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, List, Optional

import torch

from . import cabi

# slot indices of include/vlg_hip.h: counts, then sums
SCORED, TOP1, TOPK, IOU_HIT, BOTH_HIT, NONFINITE, UNSCORED, CONF = cabi.values(
    "VLG_MET_", "SCORED", "TOP1", "TOPK", "IOU_HIT", "BOTH_HIT", "NONFINITE", "UNSCORED", "CONF")
NLL, IOU, BOX_L1, IOU_BY_CLASS = cabi.values("VLG_MET_", "NLL", "IOU", "BOX_L1", "IOU_BY_CLASS")


def n_counts(n_classes: int) -> int:
    return CONF + n_classes * n_classes


def n_sums(n_classes: int) -> int:
    return IOU_BY_CLASS + n_classes


def _ratio(a: float, b: float) -> Optional[float]:
    return a / b if b > 0 else None


def _mean_present(values: List[Optional[float]]) -> Optional[float]:
    present = [v for v in values if v is not None]
    return sum(present) / len(present) if present else None


class MetricsRecord:
    def __init__(self, n_classes: int, rows: int = 1, device=None):
        if n_classes < 1 or rows < 1:
            raise ValueError("MetricsRecord needs n_classes >= 1 and rows >= 1")
        self.n_classes, self.rows = int(n_classes), int(rows)
        self.device = torch.device(device) if device is not None else torch.device("cpu")
        self.counts = torch.zeros(self.rows, n_counts(self.n_classes), dtype=torch.int64, device=self.device)
        self.sums = torch.zeros(self.rows, n_sums(self.n_classes), dtype=torch.float64, device=self.device)

    def reset(self) -> None:
        self.counts.zero_()
        self.sums.zero_()

    def all_reduce(self, sync: Callable) -> None:
        """Sum both tensors over ranks with `sync`, a callable taking a list of tensors and summing each in place
        (Trainer.sync with mean=False bound); every count and sum is additive."""
        sync([self.counts, self.sums])

    def summary(self) -> List[Dict[str, object]]:
        """The record's only host read: one dict per row.  Ratios are over the scored tokens (per-class ones over the
        tokens whose target is that class); with nothing to divide by they are None."""
        C = self.n_classes
        counts, sums = self.counts.cpu(), self.sums.cpu()
        out = []
        for r in range(self.rows):
            c, s = counts[r].tolist(), sums[r].tolist()
            n = c[SCORED]
            conf = [c[CONF + t * C:CONF + (t + 1) * C] for t in range(C)]
            per_class_n = [sum(row) for row in conf]
            nll = _ratio(s[NLL], n)
            per_acc = [_ratio(conf[t][t], per_class_n[t]) for t in range(C)]
            per_iou = [_ratio(s[IOU_BY_CLASS + t], per_class_n[t]) for t in range(C)]
            out.append({
                "scored": n, "nonfinite": c[NONFINITE], "unscored": c[UNSCORED],
                "accuracy": _ratio(c[TOP1], n), "topk_accuracy": _ratio(c[TOPK], n),
                "nll": nll, "perplexity": None if nll is None else (math.exp(nll) if nll < 709.0 else float("inf")),
                "mean_iou": _ratio(s[IOU], n), "iou_hit": _ratio(c[IOU_HIT], n), "both_hit": _ratio(c[BOTH_HIT], n),
                "box_l1": _ratio(s[BOX_L1], n),
                "per_class_accuracy": per_acc, "per_class_iou": per_iou,
                "macro_accuracy": _mean_present(per_acc), "macro_iou": _mean_present(per_iou),
                "confusion": conf,
            })
        return out


def balanced_class_weights(counts, power: float = 0.5, row: int = 0) -> List[float]:
    """Class weights for LayoutEngine(class_weights=) / VLG_CLASS_WEIGHTS from per-class target counts n_c (host only):
    w_c proportional to n_c ** -power for the classes that occur (power 0: all equal; 1: inverse frequency; the default
    0.5 lies between), the largest of those weights for a class that does not occur, and the whole scaled so that
    sum_c n_c w_c == sum_c n_c - the weighted cross entropy's denominator is then the valid count's, and the loss stays
    on the scale of the unweighted one.
    `counts` is a sequence of n_classes counts, one dict of MetricsRecord.summary() (its confusion matrix's row sums are
    the target counts), or a MetricsRecord itself, whose row `row` is read."""
    if isinstance(counts, MetricsRecord):
        counts = counts.summary()[row]
    if isinstance(counts, dict):
        counts = [sum(r) for r in counts["confusion"]]
    n = [float(c) for c in counts]
    if not n or not all(math.isfinite(c) and c >= 0.0 for c in n) or not any(c > 0.0 for c in n):
        raise ValueError("balanced_class_weights needs finite counts >= 0 with at least one > 0, got %r" % (n,))
    if not math.isfinite(power) or power < 0.0:
        raise ValueError("power must be finite and >= 0, got %r" % (power,))
    raw = [c ** -power if c > 0.0 else 0.0 for c in n]
    top = max(raw)
    raw = [r if c > 0.0 else top for r, c in zip(raw, n)]
    scale = sum(n) / sum(c * r for c, r in zip(n, raw))
    return [r * scale for r in raw]
