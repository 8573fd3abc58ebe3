"""The rasterised layouts restated in fp32 numpy (definition: include/vlg_hip.h, "rasterised layouts").

Every quantity of the definition is one correctly rounded fp32 operation, and numpy's float32 arithmetic rounds each
operation once, so this is not an approximation of the device's result but the result itself: tests compare with equality.
Pixel centres x + 0.5 are exact in fp32 for x <= 16384.
"""
import numpy as np

F = np.float32


def raster_ref(cls, box, valid, size, n_classes, background, what="class", frames=None):
    """cls (B,T,N) int, box (B,T,N,4) float32, valid (B,T,N) or None (numpy or torch) -> int64 labels (B,T',H,W) of frames
    t0 .. t0+T'-1 (frames = (t0, T'), None: all)."""
    cls = np.asarray(cls).astype(np.int64)
    box = np.asarray(box).astype(F)
    valid = None if valid is None else np.asarray(valid).astype(F)
    B, Tb, N = cls.shape
    t0, T = (0, Tb) if frames is None else frames
    H, W = size
    px, py = np.arange(W, dtype=F) + F(0.5), np.arange(H, dtype=F) + F(0.5)
    out = np.full((B, T, H, W), background, dtype=np.int64)
    with np.errstate(all="ignore"):
        for b in range(B):
            for t in range(T):
                c, q = cls[b, t0 + t], box[b, t0 + t]
                cx, cy, w, h = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
                drawn = (c >= 0) & (c < n_classes) & np.isfinite(q).all(-1) & (w > 0) & (h > 0)
                if valid is not None:
                    drawn &= valid[b, t0 + t] != 0
                hw, hh = F(0.5) * w, F(0.5) * h
                x0, x1 = (cx - hw) * F(W), (cx + hw) * F(W)
                y0, y1 = (cy - hh) * F(H), (cy + hh) * F(H)
                area = w * h
                assert area.dtype == F and x0.dtype == F
                # painter's order: largest (area, n) first, so the smallest is drawn last and lies on top
                for n in sorted(np.nonzero(drawn)[0], key=lambda n: (area[n], n), reverse=True):
                    covx = (x0[n] <= px) & (px < x1[n])
                    covy = (y0[n] <= py) & (py < y1[n])
                    out[b, t][np.ix_(covy, covx)] = n if what == "slot" else c[n]
    return out


def confusion_ref(pred, truth, n_labels, per_frame):
    """pred, truth (B,T,...) integer label maps -> int64 (rows, L*L + 1): [truth*L + pred] per row, IGNORED last"""
    pred, truth = np.asarray(pred).astype(np.int64), np.asarray(truth).astype(np.int64)
    B, T = pred.shape[:2]
    L = n_labels
    bins = np.where((pred < L) & (truth < L), truth * L + pred, L * L).reshape(B, T, -1)
    if per_frame:
        return np.stack([np.bincount(bins[:, t].ravel(), minlength=L * L + 1) for t in range(T)]).astype(np.int64)
    return np.bincount(bins.ravel(), minlength=L * L + 1).astype(np.int64)[None]
