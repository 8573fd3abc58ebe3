"""CPU restatement of the generation step (include/vlg_hip.h, vlg_layout_decode; DESIGN.md "Generation"): the decoding
rule in fp64, the window slide.  Plain module: test infrastructure, nothing collected.

The rule, word for word.  Box = sigmoid(raw).  temperature == 0: the first maximum of the logits.  temperature > 0: kept
set = every class (top_k == 0) or the top_k largest raw logits, equal values ordered by lower class index first;
z = logit / temperature, m = max z over the kept set, p = exp(z - m) on the kept set and 0 elsewhere; cum = running sum
of p in class order, S its last value; the class is the first kept c with cum_c >= u * S, the last kept class if none.
u = (x0 >> 8) * 2^-24 + 2^-25 with x0 the first word of Philox4x32-10 (tests/philox_ref.py) on counter (token, step, 0, 0)
under key (seed & 0xffffffff, seed >> 32), token = b*N + n.  keep_padded: a slot whose class in the window's last frame is
>= n_classes keeps that id and its box."""
import numpy as np
import torch

import philox_ref as P
from philox_ref import philox4x32_10  # noqa: F401  (the generator lives in philox_ref; this name keeps working)


def uniform(tokens, step, seed):
    """u of every token index in `tokens` at `step` under `seed`: float64, strictly inside (0, 1)"""
    return P.unit64(P.words(tokens, step, P.CLASS_DRAW, seed)[0])


def decode_step(logits64, step, temperature, top_k, seed, margin=1e-5):
    """logits64 (R, C) float64, row r = token r -> (classes (R,) int64, near (R,) bool).  near marks the draws an fp32
    evaluation may decide differently: u * S within margin * S of a cumulative boundary (never set for temperature 0).
    The temperature is the fp32 value a kernel is handed."""
    l = np.asarray(logits64, dtype=np.float64)
    R, C = l.shape
    if temperature == 0:
        return l.argmax(axis=1).astype(np.int64), np.zeros(R, dtype=bool)
    kept = np.ones((R, C), dtype=bool)
    if top_k > 0:
        order = np.argsort(-l, axis=1, kind="stable")                   # descending; equal values: lower index first
        kept = np.zeros((R, C), dtype=bool)
        np.put_along_axis(kept, order[:, :top_k], True, axis=1)
    z = l / float(np.float32(temperature))
    m = np.where(kept, z, -np.inf).max(axis=1, keepdims=True)
    p = np.where(kept, np.exp(z - m), 0.0)
    cum = np.cumsum(p, axis=1)
    S = cum[:, -1]
    thr = uniform(np.arange(R), step, seed) * S
    hit = kept & (cum >= thr[:, None])
    last_kept = C - 1 - np.argmax(kept[:, ::-1], axis=1)
    cls = np.where(hit.any(axis=1), np.argmax(hit, axis=1), last_kept).astype(np.int64)
    near = (np.abs(cum - thr[:, None]) <= margin * S[:, None]).any(axis=1)
    return cls, near


def next_frame(out_last, cls_in, box_in, n_classes, step, temperature=0.0, top_k=0, seed=0, keep_padded=False):
    """out_last (B*N, n_classes + 4) [logits | raw box], window cls_in (B,T,N) / box_in (B,T,N,4) ->
    (classes (B,N) int64, boxes (B,N,4) float64, near (B,N) bool) of the frame a decoding step generates."""
    B, T, N = cls_in.shape
    o = out_last.detach().cpu().double()
    cls, near = decode_step(o[:, :n_classes].numpy(), step, temperature, top_k, seed)
    cls, near = torch.from_numpy(cls).view(B, N), torch.from_numpy(near).view(B, N)
    box = torch.sigmoid(o[:, n_classes:]).view(B, N, 4)
    if keep_padded:
        pad = cls_in[:, -1] >= n_classes
        cls = torch.where(pad, cls_in[:, -1], cls)
        box = torch.where(pad[..., None], box_in[:, -1].double(), box)
        near = near & ~pad
    return cls, box, near


def slide(cls_in, box_in, new_cls, new_box):
    """the next window: frames 1 .. T-1, then the new frame"""
    return (torch.cat([cls_in[:, 1:], new_cls[:, None].to(cls_in.dtype)], dim=1),
            torch.cat([box_in[:, 1:], new_box[:, None].to(box_in.dtype)], dim=1))


# ---- the distribution check, shared by the CPU test (on decode_step) and the GPU test (on the kernel) ------------------
DIST_TOKENS, DIST_STEPS = 4096, 4                       # 16 384 draws
DIST_SEED = 2024                                        # chosen so that the restatement itself passes check_distribution
DIST_CASES = [(1.0, 0), (1.0, 5), (0.7, 0), (0.7, 5)]   # (temperature, top_k)


def distribution_row():
    """the one logits row every token of the distribution check shares (fp32)"""
    return torch.randn(20, generator=torch.Generator().manual_seed(0)) * 3


def check_distribution(classes, temperature, top_k):
    """classes: every draw of DIST_TOKENS tokens x DIST_STEPS steps on distribution_row().  Each class frequency within
    5 sqrt(p (1 - p) / n) of its probability under the rule; a class outside the top-k is never drawn."""
    row = distribution_row().double()
    z = row / float(np.float32(temperature))
    kept = torch.ones(20, dtype=torch.bool)
    if top_k > 0:
        kept = torch.zeros(20, dtype=torch.bool)
        kept[torch.from_numpy(np.argsort(-row.numpy(), kind="stable")[:top_k].copy())] = True
    p = torch.where(kept, torch.exp(z - z[kept].max()), torch.zeros_like(z))
    p = p / p.sum()
    classes = torch.as_tensor(classes).reshape(-1)
    n = classes.numel()
    assert n == DIST_TOKENS * DIST_STEPS
    freq = torch.bincount(classes, minlength=20).double() / n
    assert freq.numel() == 20, "a class id outside [0, 20) was drawn"
    assert bool((freq[~kept] == 0).all()), "a class outside the top-%d was drawn" % top_k
    bar = 5.0 * torch.sqrt(p * (1 - p) / n)
    worst = ((freq - p).abs() - bar).max()
    assert float(worst) <= 0, "class frequencies %s vs probabilities %s (5 sigma %s)" % (freq.tolist(), p.tolist(), bar.tolist())
