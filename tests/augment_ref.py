"""CPU restatement of the augmentation rule (include/vlg_hip.h, "augmentation"; DESIGN.md "Augmentation"): coins and
thresholds in integers, the box map in numpy fp32 with every operation rounded on its own.  Plain module: test
infrastructure, nothing collected.

The rule, word for word.  k is the device step counter, 0 for the first training step.  Token i = (b*T + t)*N + n, track
r = b*N + n.  W(c0,c1,c2,c3) = the four words of Philox4x32-10 on that counter under key (seed & 0xffffffff, seed >> 32);
v(x) = (float)(x >> 8) * 2^-23 - 1;  coin(x, thr) = (x >> 8) < thr, thr = round(p * 2^24).
  clip draw   (x0..x3) = W(b, k, 2, 0): flip = coin(x0, thr_flip), s = 1 + zoom*v(x1), tx = shift*v(x2), ty = shift*v(x3)
  track draw  drop = coin(first word of W(r, k, 3, 0), thr_drop)
  token draw  (inputs, jitter > 0) (y0..y3) = W(i, k, 4, 0): jx = jitter*v(y0), jy = jitter*v(y1), jw = 1 + jitter*v(y2),
              jh = 1 + jitter*v(y3)
The box map on (cx, cy, w, h): flip: cx = 1 - cx.  Geometric stage iff zoom > 0 or shift > 0 or jitter > 0:
cx = ((cx - 0.5)*s + 0.5) + tx, cy likewise with ty, w = w*s, h = h*s; an input box with jitter > 0: cx += jx, cy += jy,
w *= jw, h *= jh; crop: x0 = max(cx - 0.5*w, 0), x1 = min(cx + 0.5*w, 1), w = max(x1 - x0, 2^-10),
cx = min(max(0.5*(x0 + x1), 0), 1), the y axis likewise; max(a, c) is a > c ? a : c and min(a, c) is a < c ? a : c.
With the stage off a box that is not flipped is a bit copy.
Inputs: a dropped track is class n_classes and a zero box in all T frames; a padded token (class >= n_classes) of a kept
track is copied untouched; every other token keeps its class and takes the map with jitter.  Targets: the map without
jitter where valid > 0, else a bit copy.  valid: 0 on a dropped track, else copied.  tgt_class has no part in it."""
import numpy as np
import torch

import philox_ref as P
from philox_ref import coin, words  # noqa: F401  (words(index, k, stream, seed): the four words of counter (index, k, stream, 0))

TWO24 = P.TWO24
NC = 20
F = np.float32
MIN_SIZE = F(2.0 ** -10)
STREAM_CLIP, STREAM_TRACK, STREAM_TOKEN = P.CLIP_DRAW, P.TRACK_DROP, P.TOKEN_JITTER


def threshold(p):
    """round(p * 2^24): what vlg_augment_plan computes"""
    if not 0.0 <= p <= 1.0:
        raise ValueError("a probability must be in [0, 1]")
    return P.coin_threshold(p)


v = P.signed32          # (float)(x >> 8) * 2^-23 - 1: fp32 in [-1, 1), every step exact


def clip_draw(B, k, seed, thr_flip, zoom, shift):
    """(flip bool (B,), s, tx, ty fp32 (B,))"""
    x = words(np.arange(B), k, STREAM_CLIP, seed)
    return coin(x[0], thr_flip), F(1.0) + F(zoom) * v(x[1]), F(shift) * v(x[2]), F(shift) * v(x[3])


def track_drop(B, N, k, seed, thr_drop):
    """bool (B, N)"""
    return coin(words(np.arange(B * N), k, STREAM_TRACK, seed)[0], thr_drop).reshape(B, N)


def token_draw(shape, k, seed, jitter):
    """(jx, jy, jw, jh) fp32 of every token, each of `shape` = (B, T, N)"""
    y = words(np.arange(int(np.prod(shape))), k, STREAM_TOKEN, seed)
    j = F(jitter)
    return tuple(a.reshape(shape) for a in (j * v(y[0]), j * v(y[1]), F(1.0) + j * v(y[2]), F(1.0) + j * v(y[3])))


def _crop(c, w):
    half = F(0.5) * w
    lo, hi = c - half, c + half
    x0 = np.where(lo > F(0.0), lo, F(0.0)).astype(F)
    x1 = np.where(hi < F(1.0), hi, F(1.0)).astype(F)
    d, m = x1 - x0, F(0.5) * (x0 + x1)
    w = np.where(d > MIN_SIZE, d, MIN_SIZE).astype(F)
    m0 = np.where(m > F(0.0), m, F(0.0)).astype(F)
    return np.where(m0 < F(1.0), m0, F(1.0)).astype(F), w


def box_map(box, flip, s, tx, ty, geo, jit=None):
    """box fp32 (B,T,N,4); flip, s, tx, ty per clip (B,); jit = token_draw's tuple or None -> the mapped boxes, fp32.  Rows
    that the map leaves alone (not flipped, stage off) come back as the same bits."""
    box = np.ascontiguousarray(box, dtype=F)
    cx, cy, w, h = (box[..., j].copy() for j in range(4))
    fl = np.broadcast_to(np.asarray(flip)[:, None, None], cx.shape)
    cx = np.where(fl, F(1.0) - cx, cx).astype(F)
    if geo:
        s, tx, ty = (np.asarray(a, dtype=F)[:, None, None] for a in (s, tx, ty))
        cx = ((cx - F(0.5)) * s + F(0.5)) + tx
        cy = ((cy - F(0.5)) * s + F(0.5)) + ty
        w, h = w * s, h * s
        if jit is not None:
            jx, jy, jw, jh = jit
            cx, cy, w, h = cx + jx, cy + jy, w * jw, h * jh
        cx, w = _crop(cx, w)
        cy, h = _crop(cy, h)
    out = np.stack([cx, cy, w, h], axis=-1)
    assert out.dtype == F
    return out


def augment(batch, k, seed, flip=0.0, zoom=0.0, shift=0.0, jitter=0.0, drop=0.0, n_classes=NC, thr_flip=None, thr_drop=None):
    """batch: dict of CPU tensors slot_class (B,T,N) int64, slot_box, tgt_box (B,T,N,4) fp32, valid (B,T,N) fp32 -> dict of
    new tensors slot_class, slot_box, tgt_box, valid, plus the draws `flip` (B,) and `drop` (B,N) as bool tensors.
    thr_flip / thr_drop override the thresholds of the probabilities (the kernel test's extremes)."""
    sc = batch["slot_class"].numpy()
    sb, tb, va = (np.ascontiguousarray(batch[key].numpy(), dtype=F) for key in ("slot_box", "tgt_box", "valid"))
    B, T, N = sc.shape
    thr_flip = threshold(flip) if thr_flip is None else thr_flip
    thr_drop = threshold(drop) if thr_drop is None else thr_drop
    zoom, shift, jitter = F(zoom), F(shift), F(jitter)
    geo = bool(zoom > 0 or shift > 0 or jitter > 0)
    fl, s, tx, ty = clip_draw(B, k, seed, thr_flip, zoom, shift)
    dr = np.broadcast_to(track_drop(B, N, k, seed, thr_drop)[:, None, :], (B, T, N))
    jit = token_draw((B, T, N), k, seed, jitter) if jitter > 0 else None
    mapped_in, mapped_tgt = box_map(sb, fl, s, tx, ty, geo, jit), box_map(tb, fl, s, tx, ty, geo)
    padded = sc >= n_classes
    out_c = np.where(dr, np.int64(n_classes), sc)
    out_b = np.where(padded[..., None], sb, mapped_in)
    out_b = np.where(dr[..., None], F(0.0), out_b).astype(F)
    out_t = np.where((va > 0)[..., None], mapped_tgt, tb).astype(F)
    out_v = np.where(dr, F(0.0), va).astype(F)
    return {"slot_class": torch.from_numpy(out_c.astype(np.int64)), "slot_box": torch.from_numpy(out_b),
            "tgt_box": torch.from_numpy(out_t), "valid": torch.from_numpy(out_v),
            "flip": torch.from_numpy(fl.copy()), "drop": torch.from_numpy(dr[:, 0].copy())}


def bits(t):
    """a float tensor as its int32 words: torch.equal on these compares bit for bit (-0.0 and NaN included)"""
    return t.contiguous().view(torch.int32)


# ---- the cases of the kernel test (tests/test_hip_augment.py), shared with the CPU tests ----
SHAPES = [(3, 4, 5), (2, 16, 64), (1, 32, 33)]
STEPS = (0, 1, 2 ** 31 - 1)
SEEDS = (20240607, 0xC0FFEE1234567)               # below 2^32, and with high bits set
ALL_ON = dict(flip=0.5, zoom=0.3, shift=0.2, jitter=0.1, drop=0.3)
KNOBS = [dict(flip=0.5), dict(zoom=0.5), dict(shift=0.5), dict(jitter=0.25), dict(drop=0.3), ALL_ON]
COIN_SEED = 11                                    # the flip-share check: chosen so that the restatement itself passes


def _boxes(g, shape):
    """(cx, cy, w, h) of `shape` tokens: a quarter ordinary, a quarter sticking out of the image, a quarter small and within
    0.02 of a border (a shift moves them wholly outside), a quarter centred outside the image already"""
    n = int(np.prod(shape))
    box = torch.rand(n, 4, generator=g)
    box[:, 2:] = box[:, 2:] * 0.5 + 0.01
    kind = torch.arange(n) % 4
    out = kind == 1                                                  # sticking out: centre near a border, size up to 0.9
    box[out, 0] = torch.where(torch.rand(n, generator=g) < 0.5, 0.02, 0.97)[out]
    box[out, 2] = (0.3 + 0.6 * torch.rand(n, generator=g))[out]
    small = kind == 2
    box[small, 2:] = 0.004 + 0.02 * torch.rand(n, 2, generator=g)[small]
    box[small, 0] = torch.where(torch.rand(n, generator=g) < 0.5, 0.015, 0.985)[small]
    box[small, 1] = torch.where(torch.rand(n, generator=g) < 0.5, 0.015, 0.985)[small]
    far = kind == 3
    box[far, 0] = torch.where(torch.rand(n, generator=g) < 0.5, -0.05, 1.04)[far]
    return box[torch.randperm(n, generator=g)].reshape(tuple(shape) + (4,)).contiguous()


def kernel_case(B, T, N, seed, padded=True):
    """a batch as the engine takes it: slot_class with the reserved id on whole tracks and on single tokens when `padded`,
    valid 0 on the padded tracks AND on a fifth of the tokens whose class is real, boxes as _boxes makes them"""
    g = torch.Generator().manual_seed(seed)
    cls = torch.randint(0, NC, (B, T, N), generator=g)
    tgt = torch.randint(0, NC, (B, T, N), generator=g)
    valid = (torch.rand(B, T, N, generator=g) >= 0.2).float()
    if padded:
        track = torch.rand(B, 1, N, generator=g) < 0.25                 # a padded track: every frame, the generator's convention
        token = torch.rand(B, T, N, generator=g) < 0.1
        cls = torch.where(track | token, torch.full_like(cls, NC), cls)
        valid = torch.where(track.expand(B, T, N), torch.zeros_like(valid), valid)
    return {"slot_class": cls.contiguous(), "slot_box": _boxes(g, (B, T, N)), "tgt_class": tgt.contiguous(),
            "tgt_box": _boxes(g, (B, T, N)), "valid": valid.contiguous()}
