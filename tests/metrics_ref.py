"""fp64 restatement of vlg_layout_metrics (include/vlg_hip.h, "validation metrics") on CPU tensors in the public (B,T,N)
order.  A helper, not a test: tests/test_layout_metrics_cpu.py checks it on a case worked out by hand, the GPU tests check
the kernel against it.

Only the arithmetic is fp64: every DECISION that the kernel takes on its fp32 inputs exactly - scored or not, finite or
not, the first maximum, the rank of the target - is taken on the same fp32 values here, so those counts must agree exactly.
The IoU threshold is the one decision on a computed value; iou64 is returned so that a test can count the tokens whose IoU
lies within a band of the threshold."""
import torch

SCORED, TOP1, TOPK, IOU_HIT, BOTH_HIT, NONFINITE, UNSCORED, CONF = 0, 1, 2, 3, 4, 5, 6, 8
NLL, IOU, BOX_L1, IOU_BY_CLASS = 0, 1, 2, 4
COUNT_NAMES = ("SCORED", "TOP1", "TOPK", "IOU_HIT", "BOTH_HIT", "NONFINITE", "UNSCORED")


def iou64(p, t, eps):
    """IoU of (cx, cy, w, h) boxes, the formula of csrc/loss.hip in fp64"""
    ax1, ax2, ay1, ay2 = p[..., 0] - 0.5 * p[..., 2], p[..., 0] + 0.5 * p[..., 2], p[..., 1] - 0.5 * p[..., 3], p[..., 1] + 0.5 * p[..., 3]
    bx1, bx2, by1, by2 = t[..., 0] - 0.5 * t[..., 2], t[..., 0] + 0.5 * t[..., 2], t[..., 1] - 0.5 * t[..., 3], t[..., 1] + 0.5 * t[..., 3]
    iw = (torch.minimum(ax2, bx2) - torch.maximum(ax1, bx1)).clamp(min=0)
    ih = (torch.minimum(ay2, by2) - torch.maximum(ay1, by1)).clamp(min=0)
    inter = iw * ih
    return inter / (p[..., 2] * p[..., 3] + t[..., 2] * t[..., 3] - inter + eps)


def metrics_ref(logits, raw, tgt_class, tgt_box, valid, top_k, iou_thr, iou_eps, t0=0):
    """logits (B,T,N,C) and raw (B,T,N,4) fp32; tgt_class (B,tgt_T,N) int64, tgt_box (B,tgt_T,N,4) fp32, valid (B,tgt_T,N)
    fp32 or None; frame t of the outputs is scored against target frame t0 + t.
    Returns counts (CONF + C*C int64), sums (IOU_BY_CLASS + C float64) and iou (B,T,N) float64, NaN where a token did
    not reach the statistics."""
    B, T, N, C = logits.shape
    tc, tb = tgt_class[:, t0:t0 + T], tgt_box[:, t0:t0 + T].double()
    ok = (tc >= 0) & (tc < C)
    if valid is not None:
        ok = ok & (valid[:, t0:t0 + T] != 0)
    finite = torch.isfinite(logits).all(-1) & torch.isfinite(raw).all(-1)
    use = ok & finite
    counts = torch.zeros(CONF + C * C, dtype=torch.int64)
    sums = torch.zeros(IOU_BY_CLASS + C, dtype=torch.float64)
    counts[UNSCORED], counts[NONFINITE], counts[SCORED] = int((~ok).sum()), int((ok & ~finite).sum()), int(use.sum())
    iou_all = torch.full((B, T, N), float("nan"), dtype=torch.float64)
    if not bool(use.any()):
        return counts, sums, iou_all
    l32, tg = logits[use], tc[use]
    idx = torch.arange(C)
    mx = l32.max(-1, keepdim=True).values
    pred = torch.where(l32 == mx, idx, torch.tensor(C)).min(-1).values             # the FIRST maximum
    lt = l32.gather(1, tg[:, None])
    rank = (l32 > lt).sum(-1) + ((l32 == lt) & (idx[None] < tg[:, None])).sum(-1)    # equal logits: the lower index first
    l = l32.double()
    nll = torch.logsumexp(l, -1) - l.gather(1, tg[:, None])[:, 0]
    p = torch.sigmoid(raw[use].double())
    iou = iou64(p, tb[use], iou_eps)
    l1 = (p - tb[use]).abs().mean(-1)
    top1, hit = pred == tg, iou >= iou_thr
    counts[TOP1], counts[TOPK] = int(top1.sum()), int((rank < top_k).sum())
    counts[IOU_HIT], counts[BOTH_HIT] = int(hit.sum()), int((top1 & hit).sum())
    counts[CONF:] = torch.bincount(tg * C + pred, minlength=C * C)
    sums[NLL], sums[IOU], sums[BOX_L1] = nll.sum(), iou.sum(), l1.sum()
    sums[IOU_BY_CLASS:] = torch.zeros(C, dtype=torch.float64).index_add_(0, tg, iou)
    iou_all[use] = iou
    return counts, sums, iou_all
