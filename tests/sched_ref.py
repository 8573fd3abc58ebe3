"""CPU restatement of scheduled sampling (include/vlg_hip.h, "scheduled sampling"; DESIGN.md "Scheduled sampling"): coins and
thresholds in integers, the decoding rule in fp64.  Plain module: test infrastructure, nothing collected.

The rule, word for word.  k is the device step counter, 0 for the first training step.  A training step on batch
(slot_class (B,T,N), slot_box (B,T,N,4), targets, valid) runs PASS 1, the evaluation forward on the true inputs (live
weights, no dropout, no loss launch) into out, rows in (b*N + n)*T + t order, the row at t predicting frame t + 1.
The input token i = (b*T + t)*N + n keeps the truth when t = 0 (no prediction) or slot_class[i] >= n_classes (a padded
slot keeps its reserved id and its box).  For every other token x is the first word of Philox4x32-10 on counter
(i, k, 1, 0) under key (seed & 0xffffffff, seed >> 32), and the token is replaced iff (x >> 8) < thr(k).
thr_max = round(eps_max * 2^24); thr(k) = thr_max when ramp_steps == 0, else thr_max * min(k + 1, ramp_steps) // ramp_steps
in 64-bit integers.  eps_max = 0 never replaces, eps_max = 1 always does.
Replacement, from out row (b*N + n)*T + (t - 1): class = the decoding rule of tests/decode_ref.py for a slot that is not
padded - temperature == 0: the first maximum; temperature > 0: the kept set (top_k as in generation), fp32 cumulative sums
and u from counter (i, k, 0, 0) under the same key; box = sigmoid(raw).
tgt_class, tgt_box and valid are never touched; PASS 2 is the training forward, backward and optimiser on the mixed
slot_class / slot_box with the true targets.  The counter advances once per training forward+backward."""
import numpy as np
import torch

import decode_ref as D
import philox_ref as P

TWO24 = P.TWO24


def thr_max(eps_max):
    """round(eps_max * 2^24): what vlg_sched_plan computes"""
    if not 0.0 <= eps_max <= 1.0:
        raise ValueError("eps_max must be in [0, 1]")
    return P.coin_threshold(eps_max)


def thr(k, thr_max_, ramp_steps):
    """the integer threshold of training step k"""
    if ramp_steps == 0:
        return int(thr_max_)
    return int(thr_max_) * min(int(k) + 1, int(ramp_steps)) // int(ramp_steps)


def coin_words(tokens, k, seed):
    """x >> 8 of every token's coin: 24-bit integers"""
    return P.bits24(P.words(tokens, k, P.SCHED_COIN, seed)[0])


def draw_words(tokens, k, seed):
    """x >> 8 of every token's class draw (counter stream 0, the one decode_ref.uniform reads)"""
    return P.bits24(P.words(tokens, k, P.CLASS_DRAW, seed)[0])


def eligible(slot_class, n_classes):
    """bool (B,T,N): tokens that may be replaced - not frame 0, not padded"""
    sc = torch.as_tensor(slot_class)
    e = sc < n_classes
    e[:, 0] = False
    return e


def replaced(slot_class, n_classes, k, thr_max_, ramp_steps, seed):
    """bool (B,T,N): the tokens step k replaces"""
    e = eligible(slot_class, n_classes)
    coins = coin_words(np.arange(e.numel()), k, seed).reshape(tuple(e.shape))
    return e & torch.from_numpy(coins < thr(k, thr_max_, ramp_steps))


def decode_tokens(logits64, tokens, k, temperature, top_k, seed, margin=1e-5):
    """decode_ref.decode_step with the Philox counter word of row j = tokens[j] (there it is j itself) ->
    (classes int64, near bool).  near: u * S within margin * S of a cumulative boundary."""
    l = np.asarray(logits64, dtype=np.float64)
    R, C = l.shape
    if temperature == 0 or R == 0:
        return (l.argmax(axis=1) if R else np.zeros(0)).astype(np.int64), np.zeros(R, dtype=bool)
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
    t = D.uniform(tokens, k, seed) * S
    hit = kept & (cum >= t[:, None])
    last_kept = C - 1 - np.argmax(kept[:, ::-1], axis=1)
    cls = np.where(hit.any(axis=1), np.argmax(hit, axis=1), last_kept).astype(np.int64)
    near = (np.abs(cum - t[:, None]) <= margin * S[:, None]).any(axis=1)
    return cls, near


def mix_inputs(out, slot_class, slot_box, n_classes, k, thr_max_, ramp_steps=0, temperature=0.0, top_k=0, seed=0):
    """out (B*N*T, >= n_classes + 4) [logits | raw box | anything], internal row order; slot_class (B,T,N) int64, slot_box
    (B,T,N,4) -> (mixed classes (B,T,N) int64, mixed boxes (B,T,N,4) float64, replaced (B,T,N) bool, near (B,T,N) bool).
    Only the rows of replaced tokens are read.  Boxes of tokens that are not replaced are the truth widened to fp64."""
    sc, sb = torch.as_tensor(slot_class).cpu(), torch.as_tensor(slot_box).cpu()
    B, T, N = sc.shape
    o = out.detach().cpu().double()
    rep = replaced(sc, n_classes, k, thr_max_, ramp_steps, seed)
    b, t, n = torch.meshgrid(torch.arange(B), torch.arange(T), torch.arange(N), indexing="ij")
    tokens = ((b * T + t) * N + n)[rep]
    src = ((b * N + n) * T + (t - 1))[rep]
    rows = o[src]
    cls, near = decode_tokens(rows[:, :n_classes].numpy(), tokens.numpy(), k, temperature, top_k, seed)
    mc, mb = sc.clone(), sb.double().clone()
    mc[rep] = torch.from_numpy(cls)
    mb[rep] = torch.sigmoid(rows[:, n_classes:n_classes + 4])
    nr = torch.zeros(B, T, N, dtype=torch.bool)
    nr[rep] = torch.from_numpy(near)
    return mc, mb, rep, nr


# ---- the cases of the kernel test (tests/test_hip_sched_mix.py), shared with the CPU test that counts their near draws ----
NC = 20
SHAPES = [(1, 2, 1), (1, 1, 3), (3, 8, 5), (2, 4, 33), (2, 3, 70)]
SAMPLING = [(1.0, 0), (0.7, 5)]                  # (temperature, top_k) of the temperature > 0 cases
SAMPLING_SHAPES = [(3, 8, 5), (2, 4, 33), (2, 3, 70)]
SAMPLING_STEPS = (0, 3)                          # counter values each sampling case is launched at
CASE_SEED = 0xC0FFEE12345
COIN_SEED = 2024                                 # the coin-share check: chosen so that the restatement itself passes


def kernel_case(B, T, N, seed, ld=NC + 4, padded=True):
    """(out (B*N*T, ld) fp32 with NaN in every row at t = T-1 and in the columns past n_classes + 4, slot_class with the
    reserved id here and there when `padded`, slot_box)"""
    g = torch.Generator().manual_seed(seed)
    out = torch.randn(B * N * T, ld, generator=g) * 3
    out[:, NC + 4:] = float("nan")
    out.view(B * N, T, ld)[:, T - 1] = float("nan")
    cls = torch.randint(0, NC + 1 if padded else NC, (B, T, N), generator=g)
    box = torch.rand(B, T, N, 4, generator=g)
    return out, cls, box
