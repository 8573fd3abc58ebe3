"""The layout loss with its options, restated in torch: the DEFINITION of vlg_layout_loss_ext (csrc/loss.hip) and of
LayoutEngine(class_weights=, label_smoothing=, box_overlap=).  Run it in float64 for the reference and in float32 for the
torch-CPU error that the bars are multiples of; gradients come from autograd.

    total = W_REG * mean_valid(smoothL1 / 4) + W_IOU * mean_valid(1 - overlap) + W_CE * CE

  CE       F.cross_entropy(z[valid], y[valid], weight=w, label_smoothing=eps, reduction='mean'), written out term for
           term so that it also says what happens where torch divides 0 by 0:
             W  = sum_i v_i w[y_i]
             CE = (1/W) sum_i v_i [ (1-eps) w[y_i] (-log p_i[y_i]) + (eps/C) sum_c w[c] (-log p_i[c]) ]
           W == 0 (every valid target has weight 0): CE = 0 with a zero gradient.  w = None: every weight 1, W = the count.
  overlap  "iou": oracle.layout_spec.box_iou_cxcywh.  "giou": inter/(uni + e) - (ac - uni)/(ac + e), ac the area of the
           smallest box enclosing both, on torch.minimum / torch.maximum / clamp (whose subgradients the kernel follows).
Smooth-L1, the 40/20/10 weights and the box means over the valid count are oracle.layout_spec's, unchanged.
"""
import torch
import torch.nn.functional as F

from oracle import layout_spec as O


def box_giou_cxcywh(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    ax1, ay1 = a[..., 0] - a[..., 2] / 2, a[..., 1] - a[..., 3] / 2
    ax2, ay2 = a[..., 0] + a[..., 2] / 2, a[..., 1] + a[..., 3] / 2
    bx1, by1 = b[..., 0] - b[..., 2] / 2, b[..., 1] - b[..., 3] / 2
    bx2, by2 = b[..., 0] + b[..., 2] / 2, b[..., 1] + b[..., 3] / 2
    iw = (torch.minimum(ax2, bx2) - torch.maximum(ax1, bx1)).clamp(min=0)
    ih = (torch.minimum(ay2, by2) - torch.maximum(ay1, by1)).clamp(min=0)
    inter = iw * ih
    uni = a[..., 2] * a[..., 3] + b[..., 2] * b[..., 3] - inter
    cw = torch.maximum(ax2, bx2) - torch.minimum(ax1, bx1)
    ch = torch.maximum(ay2, by2) - torch.minimum(ay1, by1)
    ac = cw * ch
    return inter / (uni + O.IOU_EPS) - (ac - uni) / (ac + O.IOU_EPS)


def cross_entropy(logits, tgt_class, valid, weight=None, label_smoothing=0.0):
    """the CE term above; logits (..., C), tgt_class and valid (...)"""
    C = logits.shape[-1]
    y = tgt_class.clamp(0, C - 1)
    w = torch.ones(C, dtype=logits.dtype) if weight is None else weight.to(logits.dtype)
    nlp = -F.log_softmax(logits, dim=-1)
    wy = w[y]
    hard = wy * nlp.gather(-1, y.unsqueeze(-1)).squeeze(-1)
    soft = (nlp * w).sum(-1)
    num = (valid * ((1.0 - label_smoothing) * hard + (label_smoothing / C) * soft)).sum()
    W = (valid * wy).sum()
    if float(W.detach()) == 0.0:
        return num * 0.0
    return num / W


def losses(logits, box_raw, tgt_class, tgt_box, valid, weight=None, label_smoothing=0.0, box_overlap="iou", beta=None):
    """(total, smooth_l1, overlap, ce) - oracle.layout_spec.losses with the three options (beta: the smooth-L1 switch,
    oracle.layout_spec.SMOOTH_L1_BETA unless given)"""
    if box_overlap not in ("iou", "giou"):
        raise ValueError("box_overlap must be iou or giou")
    cnt = valid.sum().clamp(min=1.0)
    box = torch.sigmoid(box_raw)
    sl1 = F.smooth_l1_loss(box, tgt_box, beta=O.SMOOTH_L1_BETA if beta is None else beta, reduction="none").sum(-1)
    l_reg = (sl1 * valid).sum() / (4.0 * cnt)
    ov = O.box_iou_cxcywh(box, tgt_box) if box_overlap == "iou" else box_giou_cxcywh(box, tgt_box)
    l_ov = ((1.0 - ov) * valid).sum() / cnt
    l_ce = cross_entropy(logits, tgt_class, valid, weight, label_smoothing)
    total = O.W_REG * l_reg + O.W_IOU * l_ov + O.W_CE * l_ce
    return total, l_reg, l_ov, l_ce


def loss_and_grads(p, batch, n_layers: int, weight=None, label_smoothing=0.0, box_overlap="iou", n_classes: int = 20,
                   attention: str = "slot"):
    """oracle.layout_spec.loss_and_grads with `losses` above on top of the specification's encoder, in p's dtype"""
    q = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    dt = next(iter(p.values())).dtype
    logits, box_raw = O.forward(q, batch["slot_class"], batch["slot_box"].to(dt), n_layers, n_classes, attention,
                                batch["valid"].to(dt) if attention == "clip" else None)
    parts = losses(logits, box_raw, batch["tgt_class"], batch["tgt_box"].to(dt), batch["valid"].to(dt), weight,
                   label_smoothing, box_overlap)
    parts[0].backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in q.items()}
    return tuple(float(x.detach()) for x in parts), grads
