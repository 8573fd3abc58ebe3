"""Stage references of the layout-token step: one pure function per launch of LayoutEngine.forward / .backward (tensors
in, tensors out, generic in dtype), the schedule of launches the engine makes, and `emulate`, which chains the stage
functions along that schedule.  Plain module: test infrastructure only, no fixtures, nothing collected.

Every stage computes from the values its launch READS, in the dtype it is given: float64 gives the wanted value, float32
the yardstick of helpers.vs_cpu32.  The storage contract of the precision modes ("Layout step: storage
contract of the reduced-precision modes") enters as arguments and is read from vlg/engine.py and the kernels' headers, not from results:

  bf16       h1, qkv, att, h2, u, gl, xf, dh, du, dqkv are bf16 in memory, projection weights come from params_bf16;
             x, xmid, out, dout, dx, stats, lse, delta are fp32; fp32 accumulation; one round-to-nearest-even on store;
             an fp32 operand of a projection (dx, dout as dY) is rounded to bf16 on its way to the matrix cores, the
             bias-gradient column sums take it unrounded (csrc/gemm_tile16.h colsum_add)
  bf16_mfma  every tensor fp32, both operands of every projection rounded to bf16 on load
  fp32 / fp32x3  no rounding
  saved u    gelu_grad_saved: u = gelu'(pre) from the fp32 pre-activation, then stored; else u = pre, gelu' on load
  clip+bf16  scores, softmax statistics, lse fp32; P (forward: exp2(s - running max) per 32-key tile, backward:
             exp2(s - lse)) and dS rounded to bf16 as matrix operands only; delta = <dO, O> on the stored values

Stage outputs are returned UNROUNDED: the comparison allows a bf16 output its one rounding (vs_cpu32 bf16=True) and
`emulate` rounds when it stores.  Rows of every (M, .) tensor are in the engine's order m = (b*N + n)*T + t.

Dropout (Contract(dropout=(p, seed, k)); LayoutEngine._encode with drop and the `_dropped` backward): proj and ff2 write
branch + bias into `ybranch` without a residual epilogue; every layer-norm launch is the fused dropout + add + layer-norm
of its site (0, then 1 + 2l and 2 + 2l; site 0 in place on x[0]); every layer-norm backward is the fused one of the site
that FED it (2L, then 1 + 2l and 2l) and also leaves select(dx) in `ddrop`, which the proj / ff2 backward and the
embedding backward read in place of dx; one counter advance ends the step.  ybranch and ddrop are fp32 in every mode.
The masks are dropout_ref.keep_mask's, in the row order above; tests/dropout_ref.py states the rule.

Options (vlg/engine.py forward_backward; each a Contract field, each restated by the *_ref module named):
  factored   layer l takes vlg.attention.layer_kinds' kind: even layers the per-slot entries, odd layers frame_fwd / frame_bwd -
             the clip entries' operand lists with lse[row], row = vlg.attention.lse_rows, and the clip stage functions under
             tests/frame_walk.py's `visible` (the key's frame is the query's, or the key is the query); `valid` reaches them
             under padded_slots; the bf16 frame kernels are the clip templates (P / dS rounding, operand_flip_slack)
  gaussian   the head, the loss and the head's backward run at cfg.n_out = 32; a box_nll entry follows the loss
             (boxhead_ref.box_nll_closed): scale columns of dout, zeros in the padding columns, loss_out[4:8], the total's share
  loss       any option on: vlg_layout_loss_ext with class_weights (or NULL) after valid (loss_ext_ref.losses + autograd)
  sched      pass 1 = the plain forward through the head (stages "pass1 ...": no dropout, no loss), "sched mix"
             (sched_ref.mix_inputs on pass 1's out), pass 2 = the step with mix_cls / mix_box as the embedding's inputs, forward and
             backward; targets and valid stay the truth
  augment    "augment" first (augment_ref.augment); every later entry names aug_cls / aug_box / aug_tgt_box / aug_valid where it
             named batch:slot_class / slot_box / tgt_box / valid; batch:tgt_class stays the caller's
  counters   one advance per option that has a counter, after the backward, in the order dropout, sched, augment
"""
import functools
import math

import torch
import torch.nn.functional as F

import augment_ref
import boxhead_ref
import dropout_ref
import loss_ext_ref
import sched_ref
from oracle import layout_spec as O
from vlg.attention import layer_kinds, lse_rows

BF = torch.bfloat16
EPI_NONE, EPI_BIAS, EPI_GELU, EPI_RESID, EPI_DGELU, EPI_BF16 = 0, 1, 2, 4, 8, 16
EPI_A_BF16, EPI_B_BF16, EPI_OUT_BF16, EPI_SPLIT3 = 32, 64, 128, 256
EPI_GELU_GRAD, EPI_MUL = 1024, 2048

PRECISIONS = ("fp32", "fp32x3", "bf16", "bf16_mfma")
BF16_BUFFERS = ("h1", "qkv", "att", "h2", "u", "gl", "xf", "dh", "du", "dqkv")      # bf16 in memory under "bf16"
BACKWARD_BUFFERS = ("dx", "dh", "du", "dqkv", "dout", "delta")                        # reused by the backward: snapshot per launch
DROPOUT_BUFFERS = ("ybranch", "x[0]", "ddrop")              # rewritten within a dropout step: snapshot per launch there
GAUSSIAN_BUFFERS = ("loss_out",)                            # the NLL launch adds to the total the loss launch left
AUG_NAMES = {"slot_class": "aug_cls", "slot_box": "aug_box", "tgt_box": "aug_tgt_box", "valid": "aug_valid"}
COUNTERS = ("drop_step", "sched_step", "aug_step")          # the order the engine advances them in
MASK64 = 2 ** 64 - 1
FIXED = ("p:", "pb:", "batch:", "class_weights")           # never written within a step: read at its end
LOG2E = 1.0 / math.log(2.0)


class Contract:
    """What a precision mode stores and rounds (see the module docstring).  dropout = (p, seed, k): the step of an engine
    built with dropout=p, dropout_seed=seed whose counter reads k.  The other options follow that precedent:
    sched = (eps_max, ramp_steps, temperature, top_k, seed, k), augment = (knobs of augment_ref.augment, seed, k),
    loss = (class weights or None, label smoothing, "iou" | "giou") with at least one of them on, box_nll_weight = the
    weight of a LayoutConfig(box_head="gaussian") model's NLL term (None: the point head)."""

    def __init__(self, precision, attention="slot", masked=True, gelu_grad_saved=None, paired=None, dropout=None, sched=None,
                 augment=None, loss=None, box_nll_weight=None):
        assert precision in PRECISIONS
        assert loss is None or loss[0] is not None or loss[1] > 0.0 or loss[2] != "iou"
        self.dropout, self.sched, self.augment, self.loss, self.box_nll_weight = dropout, sched, augment, loss, box_nll_weight
        self.snapshots = snapshot_names(dropout is not None, box_nll_weight is not None)
        self.precision, self.attention = precision, attention
        self.store_bf16 = precision == "bf16"
        self.round_operands = precision in ("bf16", "bf16_mfma")
        self.gemm_flags = {"fp32": 0, "fp32x3": EPI_SPLIT3}.get(precision, EPI_BF16)
        self.gelu_grad_saved = precision != "fp32x3" if gelu_grad_saved is None else gelu_grad_saved
        assert not (self.gelu_grad_saved and precision == "fp32x3")
        self.paired = precision in ("fp32", "bf16") if paired is None else paired
        self.masked = masked and attention in ("clip", "factored")   # per-key validity masks (padded_slots)
        self.sfx = "_bf16" if self.store_bf16 else ""

    def counters(self):
        """{counter name: the k it reads before its advance} of the options that are on"""
        on = {"drop_step": self.dropout, "sched_step": self.sched, "aug_step": self.augment}
        return {n: on[n][-1] for n in COUNTERS if on[n] is not None}

    def snap(self, n):
        """whether buffer n is read from the per-launch snapshots.  Scheduled sampling: pass 2 overwrites every buffer pass 1
        wrote, so every engine buffer is snapshotted (by the launches that name it)"""
        return n in self.snapshots or (self.sched is not None and not n.startswith(FIXED))

    def dtype(self, buf):
        if buf in ("mix_cls", "aug_cls"):
            return torch.int64
        return BF if self.store_bf16 and buf.split("[")[0] in BF16_BUFFERS else torch.float32

    def bits(self, a=None, b=None, out=None):
        """storage bits of a projection call from the CONTRACT's dtypes; b = True for a weight / X operand of the mode"""
        is16 = lambda n: n is not None and (self.store_bf16 if n is True else self.dtype(n) == BF)
        return (EPI_A_BF16 if is16(a) else 0) | (EPI_B_BF16 if is16(b) else 0) | (EPI_OUT_BF16 if is16(out) else 0)

    def weight(self, name):
        return ("pb:" if self.store_bf16 else "p:") + name


def snapshot_names(dropout, gaussian):
    return BACKWARD_BUFFERS + (DROPOUT_BUFFERS if dropout else ()) + (GAUSSIAN_BUFFERS if gaussian else ())


class Raw:
    """an output a mutation stores as it is, storage type included (emulate)"""

    def __init__(self, t):
        self.t = t


def bf(x):
    """round to nearest even to bf16, kept in x's dtype"""
    return x.to(BF).to(x.dtype)


def ident(x):
    return x


def gelu_grad(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


def to_rows(t):
    """(B,T,N,C) -> (M,C) in the engine's row order (b, n, t)"""
    B, T, N = t.shape[:3]
    return t.permute(0, 2, 1, *range(3, t.dim())).reshape(B * N * T, *t.shape[3:])


def from_rows(t, B, T, N):
    return t.reshape(B, N, T, *t.shape[1:]).permute(0, 2, 1, *range(3, t.dim() + 2))


# ------------------------------------------------------------------------------------------------ forward stages
def embed_fwd(cls_emb, box_w, box_b, time_emb, slot_class, slot_box):
    p = {"cls_emb": cls_emb, "box_w": box_w, "box_b": box_b, "time_emb": time_emb}
    return to_rows(O.embed(p, slot_class, slot_box.to(cls_emb.dtype)))


def ln_fwd(x, g, b):
    """-> (y, mean, rstd): the two-pass statistics of csrc/layernorm.hip"""
    mean = x.mean(-1, keepdim=True)
    xc = x - mean
    rstd = 1.0 / torch.sqrt((xc * xc).mean(-1, keepdim=True) + O.LN_EPS)
    return xc * rstd * g + b, mean.squeeze(-1), rstd.squeeze(-1)


@functools.lru_cache(maxsize=64)
def _keep(M, d, site, k, seed, thr):
    return torch.from_numpy(dropout_ref.keep_mask(M, d, site, k, seed, thr))


def site_mask(c, M, d, site, k=None):
    """-> (keep (M, d) bool, rows in the engine's order; scale) of a dropout site under contract c.  k: a counter value
    other than the contract's (the checker's own test)"""
    p, seed, k0 = c.dropout
    thr, scale = dropout_ref.plan(p)
    return _keep(M, d, site, k0 if k is None else k, int(seed) & (2 ** 64 - 1), thr), scale


def dropout_scalars(c, site):
    """the scalar arguments a fused launch of `site` must carry: dropout_ref.plan's thr and fp32 scale, the 64-bit seed"""
    p, seed, _ = c.dropout
    thr, scale = dropout_ref.plan(p)
    return dict(thr=thr, scale=scale, seed=int(seed) & (2 ** 64 - 1), site=site)


def drop_ln_fwd(y, resid, g, b, keep, scale):
    """x_out = (resid or 0) + select(y), h = LN(x_out) -> (x_out, h, mean, rstd): csrc/dropout.hip's forward"""
    x = dropout_ref.select(y, keep, scale)
    if resid is not None:
        x = resid + x
    return (x,) + ln_fwd(x, g, b)


def linear_fwd(a, w, b, rnd=ident, resid=None, gelu=None):
    """c = rnd(a) rnd(w)^T + b (+ resid); gelu = "pre": (gelu(pre), pre), "grad": (gelu(pre), gelu'(pre)) -> (c, aux_out)"""
    pre = rnd(a) @ rnd(w).t() + b
    if gelu is not None:
        return F.gelu(pre), (gelu_grad(pre) if gelu == "grad" else pre)
    return (pre + resid if resid is not None else pre), None


def slot_attention_fwd(qkv, T):
    """causal along T per (clip, slot, head): rows are (sequence, frame)"""
    n_seq, d3 = qkv.shape[0] // T, qkv.shape[1]
    o = O.temporal_attention(qkv.view(n_seq, T, d3).transpose(0, 1)[None], d3 // 192)          # (1, T, n_seq, d)
    return o[0].transpose(0, 1).reshape(n_seq * T, d3 // 3)


def _clip_heads(t, B, T, N):
    """(M, H*64) rows -> (B, H, S, 64), tokens frame-major s = t*N + n"""
    x = from_rows(t, B, T, N).reshape(B, T * N, -1, 64)
    return x.permute(0, 2, 1, 3)


def _clip_rows(t, B, T, N):
    """(B, H, S, 64) -> (M, H*64) rows"""
    return to_rows(t.permute(0, 2, 1, 3).reshape(B, T, N, -1))


def _clip_allowed(valid, B, T, N, frame_only=False):
    """block-causal over the clip; frame_only: tests/frame_walk.py's `visible` - the key's frame is the query's"""
    S = T * N
    frame = torch.arange(S) // N
    allowed = ((frame[None, :] == frame[:, None]) if frame_only else (frame[None, :] <= frame[:, None]))[None, None]
    if valid is not None:
        allowed = allowed & (valid.reshape(B, 1, 1, S) > 0)
    return allowed | torch.eye(S, dtype=torch.bool)[None, None]


def clip_attention_fwd(qkv, valid, B, T, N, rnd=ident, detail=None, frame_only=False):
    """-> (out rows, lse (B*H*S,) in the log2 domain).  The walk of csrc/attention_clip.hip: 32-key tiles in frame-major
    order, a running maximum per query, P = exp2(s - running max) (rounded by `rnd` only as the operand of P.V, the row sum
    takes it unrounded), O rescaled when the maximum moves, one division by the row sum at the end.  `detail`, a dict,
    receives what operand_flip_slack needs: every tile's P before rounding and its weight in the final output."""
    d = qkv.shape[1] // 3
    q, k, v = (_clip_heads(t, B, T, N) for t in qkv.split(d, dim=-1))
    s = (q @ k.transpose(-1, -2)) * (LOG2E / 8.0)
    s = s.masked_fill(~_clip_allowed(valid, B, T, N, frame_only), float("-inf"))
    S = T * N
    m = torch.full(s.shape[:-1], float("-inf"), dtype=s.dtype)
    l = torch.zeros_like(m)
    o = torch.zeros_like(q)
    tiles = []
    for j in range(0, S, 32):
        st = s[..., j:j + 32]
        m_new = torch.maximum(m, st.amax(-1))
        m_use = torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)
        alpha = torch.exp2(m - m_use)
        p = torch.exp2(st - m_use[..., None])
        l = l * alpha + p.sum(-1)
        o = o * alpha[..., None] + rnd(p) @ v[..., j:j + 32, :]
        m = m_new
        tiles.append((p, m_use))
    if detail is not None:
        detail.update(p=torch.cat([t for t, _ in tiles], -1), v=v,        # weight of a tile's P in out: the later rescales / l
                      w=torch.cat([(torch.exp2(mu - m) / l)[..., None].expand_as(t) for t, mu in tiles], -1))
    return _clip_rows(o / l[..., None], B, T, N), (m + torch.log2(l)).reshape(-1)


def loss_fwd(out, tgt_class, tgt_box, valid, B, T, N, n_classes=20, options=None):
    """-> (the four loss scalars, dout rows) by oracle.losses and its autograd; options = Contract.loss: by
    loss_ext_ref.losses.  Columns of `out` past the four raw box means (the Gaussian head's) get a zero gradient here."""
    o = from_rows(out, B, T, N).detach().clone().requires_grad_(True)
    logits, raw = o[..., :n_classes], o[..., n_classes:n_classes + 4]
    if options is None:
        parts = O.losses(logits, raw, tgt_class, tgt_box.to(out.dtype), valid.to(out.dtype))
    else:
        parts = loss_ext_ref.losses(logits, raw, tgt_class, tgt_box.to(out.dtype), valid.to(out.dtype), *options)
    parts[0].backward()
    return torch.stack([p.detach() for p in parts]), to_rows(o.grad)


def box_nll_stage(out, dout, loss_out, tgt_box, valid, B, T, N, C, w_nll):
    """vlg_layout_box_nll on the rows it read -> (dout, loss_out (8,), boxhead_ref.box_nll_closed's dict): the scale
    columns' gradient beside the loss launch's columns (kept as they are: the mean is detached), exact zeros in the four
    padding columns, loss_out[4:8] = {nll, cover, 0, 0} and the total's w_nll * nll share.  Evaluated in fp64 whatever the
    dtype of `out` (boxhead_ref's rule; its bars are its own units, not a torch-CPU fp32 yardstick)."""
    ref = boxhead_ref.box_nll_closed(out, tgt_box.float(), valid.float(), B, T, N, C, w_nll)
    dt = out.dtype
    d = torch.cat([dout[:, :C + 4], ref["dscale"].to(dt), torch.zeros(dout.shape[0], 4, dtype=dt)], dim=1)
    tail = torch.stack([ref["nll"], ref["cover"]]).to(dt)
    lo = torch.cat([(loss_out[0] + w_nll * tail[0]).reshape(1), loss_out[1:4], tail, torch.zeros(2, dtype=dt)])
    return d, lo, ref


def sched_plan(c):
    """(thr_max, ramp_steps, temperature, top_k, 64-bit seed, k) of Contract.sched: what the mix launch is handed"""
    eps_max, ramp, temperature, top_k, seed, k = c.sched
    return sched_ref.thr_max(eps_max), int(ramp), float(temperature), int(top_k), int(seed) & MASK64, k


def sched_mix_stage(c, out, slot_class, slot_box, n_classes, k=None):
    """sched_ref.mix_inputs on the `out` the launch read -> (mixed classes, mixed boxes, replaced, near)"""
    thr_max, ramp, temperature, top_k, seed, k0 = sched_plan(c)
    return sched_ref.mix_inputs(out, slot_class, slot_box.float(), n_classes, k0 if k is None else k, thr_max, ramp, temperature,
                                top_k, seed)


def augment_stage(c, batch, n_classes, k=None):
    """augment_ref.augment on the caller's tensors (fp32, as the kernel reads them) -> its dict"""
    knobs, seed, k0 = c.augment
    b = {n: (t if not t.is_floating_point() else t.float()) for n, t in batch.items()}
    return augment_ref.augment(b, k0 if k is None else k, int(seed) & MASK64, n_classes=n_classes, **knobs)


# ------------------------------------------------------------------------------------------------ backward stages
def linear_dgrad(dy, w, rnd=ident, aux=None, mode=None):
    """dx = rnd(dy) rnd(w), times aux ("mul": the saved gelu') or gelu'(aux) ("dgelu": the saved pre-activation)"""
    dx = rnd(dy) @ rnd(w)
    if mode == "mul":
        dx = dx * aux
    elif mode == "dgelu":
        dx = dx * gelu_grad(aux)
    return dx


def linear_wgrad(dy, x, rnd=ident):
    """-> (dW = rnd(dy)^T rnd(x), db = column sums of dy as stored)"""
    return rnd(dy).t() @ rnd(x), dy.sum(0)


def ln_bwd(dy, x, mean, rstd, g, dres=None):
    """-> (dx (+ dres), dgamma, dbeta) from the SAVED statistics"""
    xh = (x - mean[:, None]) * rstd[:, None]
    a = dy * g
    dx = rstd[:, None] * (a - a.mean(-1, keepdim=True) - xh * (a * xh).mean(-1, keepdim=True))
    return (dx + dres if dres is not None else dx), (dy * xh).sum(0), dy.sum(0)


def ln_bwd_drop(dy, x, mean, rstd, g, dres, keep, scale):
    """ln_bwd and ddrop = select(dx (+ dres)) under the mask of the site that produced x -> (dx, ddrop, dgamma, dbeta)"""
    dx, dg, db = ln_bwd(dy, x, mean, rstd, g, dres)
    return dx, dropout_ref.select(dx, keep, scale), dg, db


def slot_attention_bwd(qkv, do, T):
    q = qkv.detach().clone().requires_grad_(True)
    slot_attention_fwd(q, T).backward(do)
    return q.grad


def clip_attention_bwd(qkv, do, out, lse, valid, B, T, N, rnd=ident, detail=None, frame_only=False):
    """-> (dqkv rows, delta (B*H*S,)).  As the two backward kernels: P = exp2(s - lse) from the SAVED lse, delta = <dO, O> on
    the stored values, dS = P (dP - delta) / 8; `rnd` rounds P and dS only as matrix operands."""
    d = qkv.shape[1] // 3
    q, k, v = (_clip_heads(t, B, T, N) for t in qkv.split(d, dim=-1))
    g, o = _clip_heads(do, B, T, N), _clip_heads(out, B, T, N)
    s = (q @ k.transpose(-1, -2)) * (LOG2E / 8.0)
    p = torch.exp2(s - lse.view(s.shape[:-1])[..., None])
    p = torch.where(_clip_allowed(valid, B, T, N, frame_only), p, torch.zeros_like(p))
    delta = (g * o).sum(-1)
    ds = p * (g @ v.transpose(-1, -2) - delta[..., None]) * 0.125
    dq, dk, dv = rnd(ds) @ k, rnd(ds).transpose(-1, -2) @ q, rnd(p).transpose(-1, -2) @ g
    if detail is not None:
        detail.update(p=p, ds=ds, q=q, k=k, g=g)
    return torch.cat([_clip_rows(t, B, T, N) for t in (dq, dk, dv)], dim=1), delta.reshape(-1)


def flip_step(x64, x32):
    """How far the bf16 rounding of an on-chip matrix operand (P, dS of the bf16 per-clip attention) can land from the
    rounding of its fp64 value, elementwise.  An fp64 reference cannot decide a rounding whose argument carries fp32 noise:
    an element that vs_cpu32's own rule - 4 x torch-CPU fp32's error plus 2^-20 of the value, here per element - cannot
    place on one side of a rounding boundary may round either way.  Zero for every other element (all but ~1 in 3 000)."""
    band = 4.0 * (x32.double() - x64).abs() + 2.0 ** -20 * x64.abs()
    return (bf(x64 + band) - bf(x64 - band)).abs()


def operand_flip_slack(kind, d64, d32, B, T, N):
    """{output: elementwise slack (rows)} of a bf16 per-clip attention launch from the `detail` of its float64 and float32
    evaluations: what the elements of flip_step can move each output by."""
    sp = flip_step(d64["p"], d32["p"])
    if kind.endswith("_fwd"):
        return {"att": _clip_rows((sp * d64["w"]) @ d64["v"].abs(), B, T, N)}
    sd = flip_step(d64["ds"], d32["ds"])
    parts = (sd @ d64["k"].abs(), sd.transpose(-1, -2) @ d64["q"].abs(), sp.transpose(-1, -2) @ d64["g"].abs())
    return {"dqkv": torch.cat([_clip_rows(t, B, T, N) for t in parts], dim=1)}


def embed_bwd(dx, slot_class, slot_box, vocab, B, T, N):
    """-> gradients of cls_emb, box_w, box_b, time_emb"""
    ids, box = to_rows(slot_class[..., None])[:, 0], to_rows(slot_box).to(dx.dtype)
    return {"cls_emb": torch.zeros(vocab, dx.shape[1], dtype=dx.dtype).index_add_(0, ids, dx), "box_w": dx.t() @ box,
            "box_b": dx.sum(0), "time_emb": dx.view(B * N, T, -1).sum(0)}


# ------------------------------------------------------------------------------------------------ the schedule
def forward_launches(out, cfg, c, tag, drop, cls, box, valid, final=True):
    """Appends to `out` the launches from the embedding through the head (LayoutEngine._encode and the head projection); tag: a
    prefix of the stage names (scheduled sampling's pass 1); cls, box, valid: the names of what the embedding and the per-clip
    attention read.  final False: the window encode of a rollout - through x[L], no final norm, no head projection."""
    L = cfg.n_layers
    kinds = layer_kinds(c.attention, L)
    rows = lse_rows(kinds)
    P = lambda n: "p:" + n

    def ln_f(stage, x, gname, y, i, branch=None):
        """the layer-norm of statistics slot i; dropout: the fused launch of site i, which first forms x = resid + drop(branch)
        (resid = the `x` of the launch this one replaces: site 0 has none and runs in place on x[0])"""
        if drop:
            src, resid = (x, None) if branch is None else ("ybranch", branch)
            out.append(dict(stage=tag + stage, kind="drop_ln_fwd", family="ln_fwd", entry="vlg_dropout_add_layernorm_fwd" + c.sfx, y=src,
                            resid=resid, g=gname, x_out=x, h=y, stat=i, site=i,
                            ops=(src, resid, P(gname), P(gname[:-1] + "b"), x, y, "stats[%d].mean" % i, "stats[%d].rstd" % i, "drop_step")))
            return
        out.append(dict(stage=tag + stage, kind="ln_fwd", family="ln_fwd", entry="vlg_layernorm_fwd" + c.sfx, x=x, g=gname, y=y, stat=i,
                        ops=(x, P(gname), P(gname[:-1] + "b"), y, "stats[%d].mean" % i, "stats[%d].rstd" % i)))

    def lin(stage, a, wname, cbuf, epi, aux_in=None, aux_out=None):
        flags = epi | c.gemm_flags | c.bits(a, True, cbuf)
        out.append(dict(stage=tag + stage, kind="linear_fwd", family="gemm_head" if wname == "head_w" else "gemm_fwd", entry="vlg_linear_fwd",
                        a=a, w=wname, c=cbuf, epi=epi, aux_in=aux_in, aux_out=aux_out, flags=flags,
                        ops=(a, c.weight(wname), P(wname[:-1] + "b"), cbuf, aux_in, aux_out)))

    out.append(dict(stage=tag + "embedding", kind="embed_fwd", family="embed_fwd", entry="vlg_embed_fwd", cls=cls, box=box,
                    ops=(cls, box, P("cls_emb"), P("box_w"), P("box_b"), P("time_emb"), "x[0]")))
    epi_ff1 = EPI_BIAS | EPI_GELU | (EPI_GELU_GRAD if c.gelu_grad_saved else 0)
    for l in range(L):
        pre = "l%d." % l
        x, h1, qkv, att, xmid, h2, u, gl = ("%s[%d]" % (n, l) for n in ("x", "h1", "qkv", "att", "xmid", "h2", "u", "gl"))
        ln_f(pre + "ln1", x, pre + "ln1_g", h1, 2 * l, branch="xmid[%d]" % (l - 1) if l else None)
        lin(pre + "qkv", h1, pre + "qkv_w", qkv, EPI_BIAS)
        k = kinds[l]
        if k.per_clip:      # "clip" (block-causal) or "frame": the same operand list, the lse row of vlg.attention.lse_rows
            short = k.family.split("_")[1]
            out.append(dict(stage=tag + pre + "attention", kind=short + "_fwd", family=k.family + "_fwd", entry=k.stem + "_fwd" + c.sfx,
                            l=l, row=rows[l], valid=valid, ops=(qkv, valid, att, "lse[%d]" % rows[l])))
        else:
            out.append(dict(stage=tag + pre + "attention", kind="slot_fwd", family="attn_fwd", entry="vlg_attention_fwd" + c.sfx, l=l,
                            ops=(qkv, att)))
        if drop:
            lin(pre + "proj", att, pre + "proj_w", "ybranch", EPI_BIAS)
        else:
            lin(pre + "proj", att, pre + "proj_w", xmid, EPI_BIAS | EPI_RESID, aux_in=x)
        ln_f(pre + "ln2", xmid, pre + "ln2_g", h2, 2 * l + 1, branch=x)
        lin(pre + "ff1", h2, pre + "ff1_w", gl, epi_ff1, aux_out=u)
        if drop:
            lin(pre + "ff2", gl, pre + "ff2_w", "ybranch", EPI_BIAS)
        else:
            lin(pre + "ff2", gl, pre + "ff2_w", "x[%d]" % (l + 1), EPI_BIAS | EPI_RESID, aux_in=xmid)
    if final:
        ln_f("lnf", "x[%d]" % L, "lnf_g", "xf", 2 * L, branch="xmid[%d]" % (L - 1))
        lin("head", "xf", "head_w", "out", EPI_BIAS)


def schedule(cfg, c):
    """The launches of one forward_backward in order, as vlg/engine.py makes them under contract `c`.  Each entry: stage
    (a name for messages), family, entry (C-ABI name), ops (names of the pointer arguments in order; None = NULL, "arena"
    = a slab arena, "*" = not pinned), flags (projection calls), kind + the operand names the stage function takes.
    Under c.dropout the launches are those of _encode with drop and the `_dropped` backward's (module docstring): a fused entry also
    carries its site.  Options (module docstring, "Options"): augment first, scheduled sampling's pass 1 and mix, the
    step, then one advance per counter in the order dropout, sched, augment."""
    L, d, ff = cfg.n_layers, cfg.d, cfg.d_ff
    kinds = layer_kinds(c.attention, L)
    rows = lse_rows(kinds)
    assert (c.box_nll_weight is not None) == cfg.gaussian_box, "box_nll_weight goes with LayoutConfig(box_head='gaussian') alone"
    bn = lambda k: AUG_NAMES[k] if c.augment is not None and k in AUG_NAMES else "batch:" + k     # what the step trains on
    valid = bn("valid") if c.masked else None
    drop = c.dropout is not None
    P = lambda n: "p:" + n
    out = []

    forward = lambda tag, drop, cls, box: forward_launches(out, cfg, c, tag, drop, cls, box, valid)

    if c.augment is not None:      # builds the batch every later launch reads (tgt_class stays the caller's)
        out.append(dict(stage="augment", kind="augment", family="augment", entry="vlg_layout_augment",
                        ops=tuple("batch:" + k for k in AUG_NAMES) + tuple(AUG_NAMES.values()) + ("aug_step",)))
    cls, box = bn("slot_class"), bn("slot_box")
    if c.sched is not None:        # pass 1: the evaluation forward on the true inputs, no dropout, no loss launch; then the mix
        forward("pass1 ", False, cls, box)
        out.append(dict(stage="sched mix", kind="sched_mix", family="sched_mix", entry="vlg_layout_mix_inputs", cls=cls, box=box,
                        ops=("out", cls, box, "mix_cls", "mix_box", "sched_step")))
        cls, box = "mix_cls", "mix_box"
    forward("", drop, cls, box)
    loss = dict(stage="loss", kind="loss", family="loss", tgt_class="batch:tgt_class", tgt_box=bn("tgt_box"), valid=bn("valid"))
    if c.loss is None:
        out.append(dict(loss, entry="vlg_layout_loss",
                        ops=("out", "batch:tgt_class", bn("tgt_box"), bn("valid"), "dout", "loss_out", "loss_scratch")))
    else:                          # any loss option on: one launch of the _ext entry in its place
        out.append(dict(loss, entry="vlg_layout_loss_ext",
                        ops=("out", "batch:tgt_class", bn("tgt_box"), bn("valid"), None if c.loss[0] is None else "class_weights",
                             "dout", "loss_out", "loss_scratch")))
    if cfg.gaussian_box:
        out.append(dict(stage="box nll", kind="box_nll", family="box_nll", entry="vlg_layout_box_nll", tgt_box=bn("tgt_box"),
                        valid=bn("valid"), ops=("out", bn("tgt_box"), bn("valid"), "dout", "loss_out", "box_nll_scratch")))

    # ---- backward
    def wg(stage, dy, x, wname):
        out.append(dict(stage=stage + " wgrad", kind="wgrad", family="gemm_head" if wname == "head_w" else "gemm_wgrad",
                        entry="vlg_linear_wgrad", dy=dy, x=x, w=wname, flags=c.gemm_flags | c.bits(dy, x), ops=(dy, x, "arena")))

    def dg(stage, dy, wname, dx, epi=EPI_NONE, aux_in=None):
        out.append(dict(stage=stage + " dgrad", kind="dgrad", family="gemm_dgrad", entry="vlg_linear_dgrad", dy=dy, w=wname, dx=dx,
                        epi=epi, aux_in=aux_in, flags=epi | c.gemm_flags | c.bits(dy, True, dx), ops=(dy, c.weight(wname), dx, aux_in)))

    def pair(stage, dy, wname, dx, x, epi=EPI_NONE, aux_in=None):
        if not c.paired:
            wg(stage, dy, x, wname)
            dg(stage, dy, wname, dx, epi, aux_in)
            return
        out.append(dict(stage=stage + " dgrad+wgrad", kind="pair", family="gemm_pair", entry="vlg_linear_dgrad_wgrad", dy=dy, w=wname,
                        dx=dx, x=x, epi=epi, aux_in=aux_in, flags=epi | c.gemm_flags | c.bits(dy, True, dx),
                        ops=(dy, c.weight(wname), dx, aux_in, x, "arena", "*")))

    def ln_b(stage, dy, x, i, gname, dres):
        """dropout: the fused backward under the mask of site i, the site that produced x (its statistics slot)"""
        if drop:
            out.append(dict(stage=stage + " bwd", kind="ln_bwd_drop", family="ln_bwd", entry="vlg_layernorm_bwd_dropout" + c.sfx, dy=dy,
                            x=x, stat=i, g=gname, dres=dres, site=i,
                            ops=(dy, x, "stats[%d].mean" % i, "stats[%d].rstd" % i, P(gname), dres, "dx", "ddrop", "arena", "drop_step")))
            return
        out.append(dict(stage=stage + " bwd", kind="ln_bwd", family="ln_bwd", entry="vlg_layernorm_bwd" + c.sfx, dy=dy, x=x, stat=i,
                        g=gname, dres=dres, ops=(dy, x, "stats[%d].mean" % i, "stats[%d].rstd" % i, P(gname), dres, "dx", "arena")))

    epi_dff2 = EPI_MUL if c.gelu_grad_saved else EPI_DGELU
    dxy = "ddrop" if drop else "dx"             # gradient of a residual BRANCH's output (engine.backward's dxy)
    wg("head", "dout", "xf", "head_w")
    dg("head", "dout", "head_w", "dh")
    ln_b("lnf", "dh", "x[%d]" % L, 2 * L, "lnf_g", None)
    for l in reversed(range(L)):
        pre = "l%d." % l
        x, h1, qkv, att, xmid, h2, u, gl = ("%s[%d]" % (n, l) for n in ("x", "h1", "qkv", "att", "xmid", "h2", "u", "gl"))
        pair(pre + "ff2", dxy, pre + "ff2_w", "du", gl, epi_dff2, aux_in=u)
        pair(pre + "ff1", "du", pre + "ff1_w", "dh", h2)
        ln_b(pre + "ln2", "dh", xmid, 2 * l + 1, pre + "ln2_g", "dx")
        if c.paired:
            pair(pre + "proj", dxy, pre + "proj_w", "dh", att)
        else:
            wg(pre + "proj", dxy, att, pre + "proj_w")
            dg(pre + "proj", dxy, pre + "proj_w", "dh")
        k = kinds[l]
        if k.per_clip:
            short = k.family.split("_")[1]
            out.append(dict(stage=pre + "attention bwd", kind=short + "_bwd", family=k.family + "_bwd", entry=k.stem + "_bwd" + c.sfx,
                            l=l, row=rows[l], valid=valid, pad=bn("valid"),
                            ops=(qkv, valid, att, "dh", "lse[%d]" % rows[l], "delta", "dqkv")))
        else:
            out.append(dict(stage=pre + "attention bwd", kind="slot_bwd", family="attn_bwd", entry="vlg_attention_bwd" + c.sfx, l=l,
                            pad=bn("valid"), ops=(qkv, "dh", "dqkv")))
        pair(pre + "qkv", "dqkv", pre + "qkv_w", "dh", h1)
        ln_b(pre + "ln1", "dh", x, 2 * l, pre + "ln1_g", "dx")
    out.append(dict(stage="embedding bwd", kind="embed_bwd", family="embed_bwd", entry="vlg_embed_bwd", cls=cls, box=box,
                    ops=(dxy, cls, box, "arena")))
    for name, stage, family, on in (("drop_step", "dropout step", "dropout_step", drop), ("sched_step", "sched step", "sched_step", c.sched),
                                    ("aug_step", "augment step", "augment_step", c.augment)):
        if on:      # (False or None: the option is off)
            out.append(dict(stage=stage, kind="advance", family=family, entry="vlg_dropout_step_advance", counter=name, ops=(name,)))
    return out


def epi_modes(epi):
    """(forward gelu mode, data-gradient mode) of an epilogue word"""
    gelu = None if not epi & EPI_GELU else "grad" if epi & EPI_GELU_GRAD else "pre"
    return gelu, ("mul" if epi & EPI_MUL else "dgelu" if epi & EPI_DGELU else None)


# ------------------------------------------------------------------------------------------------ the chain
def run_stage(e, cfg, c, batch, val, detail=None):
    """One schedule entry on the values `val(name)` hands out (floating tensors already in the dtype to compute in, integer
    ones as they are; None -> None; "batch:*" = the caller's tensors, aug_* / mix_* in the public (B,T,N[,4]) shape) ->
    (outputs {buffer name: unrounded tensor}, parameter gradients {name: tensor} this launch is the source of).
    `batch` gives the shape alone.  `detail`: see clip_attention_fwd; the box-NLL, mix and augment stages leave what their
    comparisons need there (`nll`, `replaced` / `near`)."""
    B, T, N = batch["slot_class"].shape
    rnd = bf if c.round_operands else ident
    arnd = bf if c.store_bf16 else ident                     # P and dS of the per-clip attention
    k = e["kind"]
    o, g = {}, {}
    detail = {} if detail is None else detail

    def wgrad(dy):
        g[e["w"]], g[e["w"][:-1] + "b"] = linear_wgrad(dy, val(e["x"]), rnd)

    def dgrad(dy):
        return linear_dgrad(dy, val(c.weight(e["w"])), rnd, val(e["aux_in"]), epi_modes(e["epi"])[1])

    if k == "embed_fwd":
        o["x[0]"] = embed_fwd(val("p:cls_emb"), val("p:box_w"), val("p:box_b"), val("p:time_emb"), val(e["cls"]), val(e["box"]))
    elif k == "ln_fwd":
        o[e["y"]], o["stats[%d].mean" % e["stat"]], o["stats[%d].rstd" % e["stat"]] = ln_fwd(
            val(e["x"]), val("p:" + e["g"]), val("p:" + e["g"][:-1] + "b"))
    elif k == "drop_ln_fwd":
        i = e["stat"]
        o[e["x_out"]], o[e["h"]], o["stats[%d].mean" % i], o["stats[%d].rstd" % i] = drop_ln_fwd(
            val(e["y"]), val(e["resid"]), val("p:" + e["g"]), val("p:" + e["g"][:-1] + "b"), *site_mask(c, B * T * N, cfg.d, e["site"]))
    elif k == "linear_fwd":
        o[e["c"]], aux = linear_fwd(val(e["a"]), val(c.weight(e["w"])), val("p:" + e["w"][:-1] + "b"), rnd,
                                    val(e["aux_in"]) if e["epi"] & EPI_RESID else None, epi_modes(e["epi"])[0])
        if aux is not None:
            o[e["aux_out"]] = aux
    elif k == "slot_fwd":
        o["att[%d]" % e["l"]] = slot_attention_fwd(val("qkv[%d]" % e["l"]), T)
    elif k in ("clip_fwd", "frame_fwd"):
        o["att[%d]" % e["l"]], o["lse[%d]" % e["row"]] = clip_attention_fwd(val("qkv[%d]" % e["l"]), val(e["valid"]), B, T, N, arnd, detail,
                                                                          k == "frame_fwd")
    elif k == "loss":
        opts = None if c.loss is None else (None if c.loss[0] is None else val("class_weights"),) + tuple(c.loss[1:])
        parts, o["dout"] = loss_fwd(val("out"), val(e["tgt_class"]), val(e["tgt_box"]), val(e["valid"]), B, T, N, cfg.n_classes, opts)
        o["loss_out"] = torch.cat([parts, parts.new_zeros(cfg.loss_tail - 4)])      # (the Gaussian head's tail: the NLL launch's)
    elif k == "box_nll":
        o["dout"], o["loss_out"], detail["nll"] = box_nll_stage(val("out"), val("dout"), val("loss_out"), val(e["tgt_box"]), val(e["valid"]),
                                                                B, T, N, cfg.n_classes, c.box_nll_weight)
    elif k == "sched_mix":
        o["mix_cls"], o["mix_box"], detail["replaced"], detail["near"] = sched_mix_stage(c, val("out"), val(e["cls"]), val(e["box"]),
                                                                                         cfg.n_classes)
    elif k == "augment":
        a = augment_stage(c, {n: val("batch:" + n) for n in AUG_NAMES}, cfg.n_classes)
        o.update({name: a[n] for n, name in AUG_NAMES.items()})
    elif k == "wgrad":
        wgrad(val(e["dy"]))
    elif k == "dgrad":
        o[e["dx"]] = dgrad(val(e["dy"]))
    elif k == "pair":
        dy = val(e["dy"])
        wgrad(dy)
        o[e["dx"]] = dgrad(dy)
    elif k == "ln_bwd":
        i = e["stat"]
        o["dx"], g[e["g"]], g[e["g"][:-1] + "b"] = ln_bwd(val(e["dy"]), val(e["x"]), val("stats[%d].mean" % i), val("stats[%d].rstd" % i),
                                                          val("p:" + e["g"]), val(e["dres"]))
    elif k == "ln_bwd_drop":
        i = e["stat"]
        o["dx"], o["ddrop"], g[e["g"]], g[e["g"][:-1] + "b"] = ln_bwd_drop(
            val(e["dy"]), val(e["x"]), val("stats[%d].mean" % i), val("stats[%d].rstd" % i), val("p:" + e["g"]), val(e["dres"]),
            *site_mask(c, B * T * N, cfg.d, e["site"]))
    elif k == "slot_bwd":
        o["dqkv"] = slot_attention_bwd(val("qkv[%d]" % e["l"]), val("dh"), T)
    elif k in ("clip_bwd", "frame_bwd"):
        l = e["l"]
        o["dqkv"], o["delta"] = clip_attention_bwd(val("qkv[%d]" % l), val("dh"), val("att[%d]" % l), val("lse[%d]" % e["row"]),
                                                   val(e["valid"]), B, T, N, arnd, detail, k == "frame_bwd")
    elif k == "embed_bwd":
        g.update(embed_bwd(val(e["ops"][0]), val(e["cls"]), val(e["box"]), cfg.vocab, B, T, N))
    elif k == "advance":
        pass                                                 # the counter: step_trace.check reads it after every launch
    else:
        raise KeyError(k)
    return o, g


def launch_scalars(cfg, c, e):
    """The scalar arguments the launch of entry `e` must carry (None: it has none that the trace records): the restatement's
    plan - thresholds as integers, 64-bit seeds, the engine's constants - as step_trace.trace names them."""
    from vlg.spec import BOX_S_MAX, BOX_S_MIN
    k = e["kind"]
    if "site" in e:
        return dropout_scalars(c, e["site"])
    if k == "loss" and c.loss is not None:
        return dict(label_smoothing=float(c.loss[1]), flags=1 if c.loss[2] == "giou" else 0)
    if k == "box_nll":
        return dict(s_min=BOX_S_MIN, s_max=BOX_S_MAX, w_nll=float(c.box_nll_weight))
    if k == "sched_mix":
        return dict(zip(("thr_max", "ramp_steps", "temperature", "top_k", "seed"), sched_plan(c)))
    if k == "augment":
        knobs, seed, _ = c.augment
        return dict(thr_flip=augment_ref.threshold(knobs.get("flip", 0.0)), thr_drop=augment_ref.threshold(knobs.get("drop", 0.0)),
                    zoom=float(knobs.get("zoom", 0.0)), shift=float(knobs.get("shift", 0.0)), jitter=float(knobs.get("jitter", 0.0)),
                    seed=int(seed) & MASK64)
    return None


def emulate(cfg, c, params, batch, dtype, mutate=None):
    """Chain the stage functions along schedule(cfg, c) in `dtype`, storing every buffer as the contract says (bf16
    buffers as torch.bfloat16 tensors, integer tensors as they are, everything else in `dtype`) -> (records, state) in the
    record format of step_trace.trace: a record = dict(family, name, flags, ops, scalars, counters, after = {snapshotted
    buffer: tensor}); state = every forward buffer, "grads" {name: tensor} and "loss".  In float64 this is the emulated
    oracle of the mode.
    `mutate(entry, val, outputs, grads, record)` may change what a launch leaves behind before it is stored (the checker's
    own test); an output wrapped in Raw is stored as it is.  A record has the scalars of its launch (launch_scalars) and the
    value of every counter after the launch, as step_trace.trace records them."""
    st = {"p:" + k: v.to(dtype) for k, v in params.items()}
    st.update({"pb:" + k: v.to(BF) for k, v in params.items()})
    st.update({"batch:" + k: v for k, v in batch.items()})
    if c.loss is not None and c.loss[0] is not None:
        st["class_weights"] = torch.as_tensor(c.loss[0], dtype=torch.float32)
    grads = {}
    val = lambda n: None if n is None else st[n].to(dtype) if st[n].is_floating_point() else st[n]
    records, counters, after = [], c.counters(), {}
    for e in schedule(cfg, c):
        o, g = run_stage(e, cfg, c, batch, val)
        if e["kind"] == "advance":
            counters[e["counter"]] += 1
        rec = dict(family=e["family"], name=e["entry"], flags=e.get("flags"), ops=e["ops"], scalars=launch_scalars(cfg, c, e),
                   counters=dict(counters))
        if mutate is not None:
            mutate(e, val, o, g, rec)
        for n, t in o.items():
            st[n] = t.t if isinstance(t, Raw) else t if not t.is_floating_point() else t.to(BF if c.dtype(n) == BF else dtype)
        grads.update(g)
        if c.sched is not None:      # every buffer, by the launch that wrote it (stored tensors are replaced, never modified)
            after = dict(after, **{n: st[n] for n in o})
            rec["after"] = after
        else:
            rec["after"] = {n: st[n].clone() for n in c.snapshots if n in st}
        records.append(rec)
    st["grads"], st["loss"], st["caller"] = grads, st["loss_out"], (batch, batch)
    return records, st


def emulated_oracle(cfg, precision, params, batch, attention="slot", masked=True, dropout=None, **options):
    """Loss scalars and gradients of the mode, chained end to end in float64 with its storage roundings."""
    _, st = emulate(cfg, Contract(precision, attention, masked, dropout=dropout, **options), params, batch, torch.float64)
    return st["loss"], st["grads"]


# ------------------------------------------------------------------------------------------------ end-to-end bars
_DISTANCES = {}


def mode_distance(kw, precision, attention="slot", variable_n=False, seed=7):
    """How far a reduced-precision mode is from the fp32 specification, measured on the CPU alone: oracle.layout_spec
    (fp32, as the step tests run it) against the float64 emulation of the mode on the same parameters and batch ->
    (relative distance of the total loss, {gradient tensor: relative L2 distance}).  Tensors whose gradient is
    analytically zero (key bias) are left out, by the rule of the step tests (norm below 1e-6 of the largest)."""
    key = (tuple(sorted(kw.items())), precision, attention, variable_n, seed)
    if key not in _DISTANCES:
        from vlg.spec import LayoutConfig, param_shapes
        cfg = LayoutConfig(attention=attention, **kw)
        params = O.init_params(param_shapes(cfg), seed=1024)
        batch = O.synthetic_batch(cfg.B, cfg.T, cfg.N, seed=seed, variable_n=variable_n, min_valid=3)
        if attention == "factored":      # the specification of that mode: tests/factored_ref.py, composed from the oracle
            import factored_ref
            parts, grads = factored_ref.loss_and_grads(params, batch, cfg.n_layers)
        else:
            parts, grads = O.loss_and_grads(params, batch, cfg.n_layers, attention=attention)
        loss, emu = emulated_oracle(cfg, precision, params, batch, attention, masked=variable_n)
        gmax = max(float(v.norm()) for v in grads.values())
        dist = {n: float((w.double() - emu[n]).norm() / emu[n].norm()) for n, w in grads.items() if float(w.norm()) >= 1e-6 * gmax}
        _DISTANCES[key] = (abs(parts[0] - float(loss[0])) / abs(float(loss[0])), dist)
    return _DISTANCES[key]


def end_to_end_bars(kw, precision, attention="slot", variable_n=False, seed=7, margin=4.0, old_loss=2e-2, old_grad=5e-2):
    """The end-to-end bars of a reduced-precision mode: `margin` x mode_distance per quantity (the emulation's own
    fp32-against-fp64 noise is about a third of the signal, hence 4), never above the bars they replace ->
    (loss bar, {tensor: bar}, {tensor base name: largest bar over the layers} for deeper models of the same width)."""
    dl, dg = mode_distance(kw, precision, attention, variable_n, seed)
    bars = {n: min(old_grad, margin * v) for n, v in dg.items()}
    by_base = {}
    for n, v in bars.items():
        b = n.split(".")[-1]
        by_base[b] = max(by_base.get(b, 0.0), v)
    return min(old_loss, margin * dl), bars, by_base
