"""Host side of the rasterised layouts: the options' rules, and the running pixel record vlg_label_confusion
(csrc/raster.hip) adds to, with the one place it is read.

A PixelRecord is one zeroed int64 tensor `counts` (rows, L*L + 1) with L = n_classes + 1 labels: the object classes and the
background, label n_classes.  Row r holds a confusion matrix [truth*L + pred] of pixels and, last, the pixels IGNORED
because a label was >= L.  One row per thing scored separately (a rollout: one row per horizon step).  Launches only ever
add to it, so nothing waits for the device until summary() copies the tensor to the host, once.  It can live on the CPU,
where its arithmetic is tested without a GPU.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Tuple

import torch

from .spec import N_CLASSES

MAX_SIDE, MAX_SLOTS, MAX_CLASSES, MAX_LABELS = 16384, 1024, 255, 32      # include/vlg_hip.h, "rasterised layouts"
WHATS = ("class", "slot")


def raster_options(size, background: Optional[int] = None, n_classes: int = N_CLASSES) -> Tuple[Tuple[int, int], int]:
    """The rasteriser's options, checked on the host by vlg_layout_rasterize's rules: ((H, W), background).  size is (H, W)
    with 1 <= H <= 16384 and W a multiple of 16 in [16, 16384]; n_classes in [1, 255]; background in [0, 255], None =
    n_classes (the label after the last class).  ValueError otherwise."""
    try:
        H, W = size
        ok = int(H) == H and int(W) == W
        H, W = int(H), int(W)
    except (TypeError, ValueError):
        raise ValueError("size must be (H, W), got %r" % (size,)) from None
    if not ok or not 1 <= H <= MAX_SIDE or not 16 <= W <= MAX_SIDE or W % 16:
        raise ValueError("size must be (H, W) with 1 <= H <= %d and W a multiple of 16 in [16, %d], got %r" % (MAX_SIDE, MAX_SIDE, size))
    if not 1 <= int(n_classes) <= MAX_CLASSES:
        raise ValueError("n_classes must be in [1, %d], got %r" % (MAX_CLASSES, n_classes))
    bg = int(n_classes) if background is None else background
    if isinstance(bg, bool) or not isinstance(bg, int) or not 0 <= bg <= 255:
        raise ValueError("background must be an integer in [0, 255], got %r" % (background,))
    return (H, W), bg


def parse_size(text) -> Tuple[int, int]:
    """"64x128" -> (64, 128); ValueError for anything else (the values themselves are raster_options' to judge)"""
    parts = str(text).lower().split("x")
    try:
        if len(parts) != 2:
            raise ValueError
        return int(parts[0]), int(parts[1])
    except ValueError:
        raise ValueError("a raster size is written HxW, like 64x128; got %r" % (text,)) from None


def _ratio(a: float, b: float) -> Optional[float]:
    return a / b if b > 0 else None


class PixelRecord:
    def __init__(self, n_classes: int, rows: int = 1, device=None):
        if not 1 <= n_classes < MAX_LABELS or rows < 1:
            raise ValueError("PixelRecord needs 1 <= n_classes <= %d and rows >= 1" % (MAX_LABELS - 1))
        self.n_classes, self.rows = int(n_classes), int(rows)
        self.n_labels = self.n_classes + 1
        self.device = torch.device(device) if device is not None else torch.device("cpu")
        self.counts = torch.zeros(self.rows, self.n_labels * self.n_labels + 1, dtype=torch.int64, device=self.device)

    def reset(self) -> None:
        self.counts.zero_()

    def all_reduce(self, sync: Callable) -> None:
        """Sum the counts over ranks with `sync`, a callable taking a list of tensors and summing each in place
        (Trainer.sync with mean=False bound)."""
        sync([self.counts])

    def summary(self) -> List[Dict[str, object]]:
        """The record's only host read: one dict per row.  pixels = those counted in the matrix, ignored = the rest.
        IoU of a label = TP / (its truth pixels + its predicted pixels - TP), None where that union is empty; miou = the
        mean over the object classes c < n_classes that have one.  Every ratio is None with nothing counted."""
        C, L = self.n_classes, self.n_labels
        counts = self.counts.cpu()
        out = []
        for r in range(self.rows):
            c = counts[r].tolist()
            conf = [c[t * L:(t + 1) * L] for t in range(L)]
            truth = [sum(row) for row in conf]
            pred = [sum(conf[t][p] for t in range(L)) for p in range(L)]
            iou = [_ratio(conf[k][k], truth[k] + pred[k] - conf[k][k]) for k in range(L)]
            present = [v for v in iou[:C] if v is not None]
            out.append({
                "pixels": sum(truth), "ignored": c[L * L],
                "pixel_accuracy": _ratio(sum(conf[k][k] for k in range(L)), sum(truth)),
                "per_class_iou": iou[:C], "miou": sum(present) / len(present) if present else None,
                "background_iou": iou[C], "confusion": conf,
            })
        return out
