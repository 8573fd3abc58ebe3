"""The specification of attention = "factored" (divided space-time attention), composed from the pinned CPU oracle.
Plain module: test infrastructure only, nothing collected.

Layer l with l % 2 == 0 is the oracle's encoder layer in mode "slot" (causal along time per slot).  Layer l with l % 2 == 1
attends INSIDE a frame: frame attention of a (B,T,N) batch is O.clip_attention on the B*T one-frame clips - token (t, n)
sees the slots m of its own frame with valid[b,t,m] > 0, and itself - and everything else in a layer acts on single rows, so
the whole odd layer is O.encoder_layer in mode "clip" on the (B*T, 1, N) reshape.  No new arithmetic.  Works in the dtype
of the parameters (fp32 or fp64); the batch's floating tensors are cast to it."""
import torch
import torch.nn.functional as F

from oracle import layout_spec as O


def frame_attention(qkv, heads, valid=None):
    """qkv (B,T,N,3d), valid (B,T,N) or None -> (B,T,N,d)"""
    B, T, N, d3 = qkv.shape
    v = None if valid is None else valid.reshape(B * T, 1, N)
    return O.clip_attention(qkv.reshape(B * T, 1, N, d3), heads, v).reshape(B, T, N, d3 // 3)


def encoder_layer(p, l, x, heads, valid=None):
    pre = "l%d." % l
    if l % 2 == 0:
        return O.encoder_layer(p, pre, x, heads, "slot")
    B, T, N, d = x.shape
    v = None if valid is None else valid.reshape(B * T, 1, N)
    return O.encoder_layer(p, pre, x.reshape(B * T, 1, N, d), heads, "clip", v).reshape(B, T, N, d)


def forward(p, slot_class, slot_box, n_layers, n_classes=20, valid=None):
    """(class logits (B,T,N,C), raw box outputs (B,T,N,4)); the time embedding is added before any reshape"""
    dt = p["cls_emb"].dtype
    x = O.embed(p, slot_class, slot_box.to(dt))
    d = x.shape[-1]
    heads = d // O.HEAD_DIM
    v = None if valid is None else valid.to(dt)
    for l in range(n_layers):
        x = encoder_layer(p, l, x, heads, v)
    x = F.layer_norm(x, (d,), p["lnf_g"], p["lnf_b"], O.LN_EPS)
    out = F.linear(x, p["head_w"], p["head_b"])
    return out[..., :n_classes], out[..., n_classes:]


def loss_and_grads(p, batch, n_layers, n_classes=20):
    """One forward + backward, as O.loss_and_grads: (loss parts as floats, {name: grad}).  batch['valid'] masks the odd
    layers' keys, as the oracle's mode "clip" takes it."""
    dt = p["cls_emb"].dtype
    q = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    logits, box_raw = forward(q, batch["slot_class"], batch["slot_box"], n_layers, n_classes, batch["valid"])
    parts = O.losses(logits, box_raw, batch["tgt_class"], batch["tgt_box"].to(dt), batch["valid"].to(dt))
    parts[0].backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in q.items()}
    return tuple(float(x.detach()) for x in parts), grads
