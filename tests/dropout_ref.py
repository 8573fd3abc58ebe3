"""Dropout of the layout-token step, restated on the CPU (definition: include/vlg_hip.h, "dropout").

Sites - the standard residual and embedding dropouts of a pre-LN transformer, 2L + 1 of them:
    site 0        x0      = drop(embed(...))
    site 1 + 2l   xmid_l  = x_l    + drop(proj(att_l) + proj_b)
    site 2 + 2l   x_{l+1} = xmid_l + drop(ff2(gelu(...)) + ff2_b)          (the bias is inside the dropout)
There is no dropout on the attention probabilities.

Mask: thr = min(floor(p * 2^32 + 0.5), 2^32 - 1), scale = fp32(1 / (1 - thr / 2^32)) computed in double.  Element
(row m, column c) of site s at dropout step k under the 64-bit seed is KEPT iff x_w >= thr, where x_w is word w = c % 4 of
Philox4x32-10 with counter (m, c / 4, s, k) and key (seed & 0xffffffff, seed >> 32); m is the internal row index
(b*N + n)*T + t.  One Philox call serves one float4; a mask bit is a function of (m, c, s, k, seed) alone; thr = 0 keeps
everything with scale 1.

Values are chosen by SELECT, not by a product: a kept element contributes y * scale, a dropped one exactly 0 whatever y
holds; backward: dy_drop = kept ? g * scale : 0.

The model below is oracle.layout_spec's embed, attention and losses with the masks inserted at the sites, differentiated
by torch autograd in whatever dtype the parameters have (tests hand it fp64)."""
import numpy as np
import torch
import torch.nn.functional as F

from philox_ref import philox4x32_10
from oracle import layout_spec as O

TWO32 = 2 ** 32


def plan(p):
    """(thr, scale): the integer threshold and the fp32 scale (returned as a Python float holding the fp32 value)"""
    if not 0.0 <= p < 1.0:
        raise ValueError("p must be in [0, 1)")
    thr = min(int(np.floor(np.float64(p) * TWO32 + 0.5)), TWO32 - 1)
    return thr, float(np.float32(1.0 / (1.0 - thr / TWO32)))


def keep_mask(rows, d, site, step, seed, thr, row0=0):
    """bool (rows, d): True = kept, for internal rows row0 .. row0 + rows - 1"""
    if row0 + rows > TWO32:
        raise ValueError("rows >= 2^32")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    q = (d + 3) // 4
    m = np.repeat(np.arange(row0, row0 + rows, dtype=np.uint64), q)
    c4 = np.tile(np.arange(q, dtype=np.uint64), rows)
    z = np.zeros_like(m)
    words = philox4x32_10((m, c4, z + np.uint64(site), z + np.uint64(step)), (z + np.uint64(seed & 0xFFFFFFFF), z + np.uint64(seed >> 32)))
    x = np.stack(words, axis=1).reshape(rows, 4 * q)[:, :d]          # column c = 4 * (c / 4) + w
    return x >= np.uint64(thr)


def select(y, keep, scale):
    """kept ? y * scale : 0 (torch; autograd's backward of where is the select on the gradient)"""
    return torch.where(keep, y * scale, torch.zeros((), dtype=y.dtype))


def site_mask_btn(B, T, N, d, site, step, seed, thr):
    """the site's mask in the PUBLIC (B,T,N,d) order: element [b,t,n] is internal row (b*N + n)*T + t"""
    k = keep_mask(B * N * T, d, site, step, seed, thr)
    return torch.from_numpy(k.reshape(B, N, T, d)).permute(0, 2, 1, 3)


def to64(tensors):
    """parameters or a batch with every floating tensor widened to fp64 (integer tensors as they are)"""
    return {k: (v.double() if v.is_floating_point() else v) for k, v in tensors.items()}


# ------------------------------------------------------------------------------------ the reduced-precision modes
# What a reduced-precision mode computes under dropout, on the CPU in the dtype of the parameters (fp64 in the tests) with
# the mode's roundings to bf16 (contract: tests/step_stages.py's module docstring).  It serves ONE purpose: to say how far
# the MODE ITSELF is from the exact model under a given set of masks, with no kernel involved.
#   "bf16_mfma"  every tensor fp32, both operands of every projection rounded to bf16 on load (forward and both gradients;
#                the bias gradient sums the unrounded dY)
#   "bf16"       in addition h1, qkv, att, h2, gl, the saved gelu'(pre), xf and the gradients dh, du, dqkv are stored as
#                bf16: one rounding on store, forward and backward
# The slot attention kernels compute in fp32 from what is stored, so they need nothing here; per-clip attention under
# "bf16" also rounds P and dS as matrix operands, which this does NOT model.
BF = torch.bfloat16


def _bf(x):
    return x.to(BF).to(x.dtype)


class _LinearBF16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, w, b):
        ctx.save_for_backward(a, w)
        return _bf(a) @ _bf(w).t() + b

    @staticmethod
    def backward(ctx, g):
        a, w = ctx.saved_tensors
        g2, a2 = g.reshape(-1, g.shape[-1]), a.reshape(-1, a.shape[-1])
        return _bf(g) @ _bf(w), _bf(g2).t() @ _bf(a2), g2.sum(0)


class _Stored(torch.autograd.Function):
    """a tensor stored as bf16 whose gradient is stored as bf16 too"""
    @staticmethod
    def forward(ctx, x):
        return _bf(x)

    @staticmethod
    def backward(ctx, g):
        return _bf(g)


class _GeluSaved(torch.autograd.Function):
    """ff1's epilogue under "bf16": gelu(pre) and gelu'(pre) from the unrounded pre, both stored as bf16; du = bf16(dgl * gelu')"""
    @staticmethod
    def forward(ctx, pre):
        import math
        ctx.save_for_backward(_bf(0.5 * (1 + torch.erf(pre / math.sqrt(2))) + pre * torch.exp(-0.5 * pre * pre) / math.sqrt(2 * math.pi)))
        return _bf(F.gelu(pre))

    @staticmethod
    def backward(ctx, g):
        return _bf(g * ctx.saved_tensors[0])


def forward(p, slot_class, slot_box, n_layers, prob, step, seed, n_classes=20, attention="slot", valid=None, taps=None, mode=None):
    """layout_spec.forward with the masks at the sites.  taps: optional dict that receives 'x0' (after site 0).
    mode = None: exact arithmetic; "bf16_mfma" / "bf16": with that mode's roundings (above)."""
    if mode not in (None, "bf16_mfma", "bf16"):
        raise ValueError("mode must be None, bf16_mfma or bf16")
    thr, scale = plan(prob)
    B, T, N = slot_class.shape
    x = O.embed(p, slot_class, slot_box)              # (the embedding is no projection launch: exact in every mode)
    d = x.shape[-1]
    n_heads = d // O.HEAD_DIM
    linear = F.linear if mode is None else _LinearBF16.apply
    stored = _Stored.apply if mode == "bf16" else (lambda t: t)
    gelu = _GeluSaved.apply if mode == "bf16" else F.gelu

    def drop(y, site):
        if thr == 0:            # keeps everything with scale 1: the identity (and the same autograd graph as layout_spec)
            return y
        return select(y, site_mask_btn(B, T, N, d, site, step, seed, thr), scale)

    x = drop(x, 0)
    if taps is not None:
        taps["x0"] = x.detach()
    for l in range(n_layers):
        pre = "l%d." % l
        h = stored(F.layer_norm(x, (d,), p[pre + "ln1_g"], p[pre + "ln1_b"], O.LN_EPS))
        qkv = stored(linear(h, p[pre + "qkv_w"], p[pre + "qkv_b"]))
        o = stored(O.clip_attention(qkv, n_heads, valid) if attention == "clip" else O.temporal_attention(qkv, n_heads))
        x = x + drop(linear(o, p[pre + "proj_w"], p[pre + "proj_b"]), 1 + 2 * l)
        h = stored(F.layer_norm(x, (d,), p[pre + "ln2_g"], p[pre + "ln2_b"], O.LN_EPS))
        u = linear(h, p[pre + "ff1_w"], p[pre + "ff1_b"])
        x = x + drop(linear(gelu(u), p[pre + "ff2_w"], p[pre + "ff2_b"]), 2 + 2 * l)
    x = stored(F.layer_norm(x, (d,), p["lnf_g"], p["lnf_b"], O.LN_EPS))
    out = linear(x, p["head_w"], p["head_b"])
    return out[..., :n_classes], out[..., n_classes:]


def loss_and_grads(p, batch, n_layers, prob, step, seed, n_classes=20, attention="slot", taps=None, mode=None):
    """layout_spec.loss_and_grads under dropout: (loss parts, {name: grad}, logits, raw boxes)"""
    q = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    logits, box_raw = forward(q, batch["slot_class"], batch["slot_box"], n_layers, prob, step, seed, n_classes, attention,
                              batch["valid"] if attention == "clip" else None, taps, mode)
    parts = O.losses(logits, box_raw, batch["tgt_class"], batch["tgt_box"], batch["valid"])
    parts[0].backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in q.items()}
    return tuple(float(x.detach()) for x in parts), grads, logits.detach(), box_raw.detach()


def mode_distance(p, batch, n_layers, prob, step, seed, mode, attention="slot"):
    """{tensor: relative L2 distance} between the mode's gradients and the exact ones under the same masks (CPU only)"""
    _, exact, _, _ = loss_and_grads(p, batch, n_layers, prob, step, seed, attention=attention)
    _, emu, _, _ = loss_and_grads(p, batch, n_layers, prob, step, seed, attention=attention, mode=mode)
    gmax = max(float(v.norm()) for v in exact.values())
    return {n: float((emu[n] - w).norm() / w.norm()) for n, w in exact.items() if float(w.norm()) >= 1e-6 * gmax}
