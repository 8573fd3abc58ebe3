"""The specification of the per-clip attention step (vlg_attention_clip_step): the N queries of frame p against every slot
of the frames <= p.  It is oracle.clip_attention on the first p + 1 frames alone, read at frame p - frames after p and
valid[:, > p] are not even passed, so they cannot matter (tests/test_clip_step_ref_cpu.py shows that this equals frame p of
the full window).  Also the inputs and masks the GPU tests share."""
import torch

from oracle import layout_spec as O

NAN = float("nan")


def step_ref(qkv, valid, p, dt=torch.float64):
    """qkv (B,T,N,3d), valid (B,T,N) or None -> (B,N,d): frame p of clip_attention on frames 0 .. p"""
    heads = qkv.shape[-1] // 192
    v = valid[:, :p + 1].to(dt) if valid is not None else None
    return O.clip_attention(qkv[:, :p + 1].to(dt), heads, v)[:, p]


def make_qkv(B, T, N, d, seed, bf16=False):
    """(B,T,N,3d); q and k of every other clip x5 (scaled scores of |s| ~ 60-90, softmax rows near one-hot: the max
    subtraction matters), as test_hip_attention_step._qkv scales every other sequence"""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, T, N, 3 * d, generator=g)
    qkv[0::2, ..., :2 * d] *= 5.0
    return qkv.to(torch.bfloat16).float() if bf16 else qkv


MASKS = ("none", "random", "lead-frames", "clip-padded")


def make_valid(kind, B, T, N, seed):
    """none; random: ~30 % of the slots padded, independently, so some queries are themselves padded; lead-frames: the first
    T // 2 frames (at least one) padded whole; clip-padded: the LAST clip entirely padded (with B = 1 the only one), the
    others random"""
    if kind == "none":
        return None
    g = torch.Generator().manual_seed(seed + 17)
    valid = (torch.rand(B, T, N, generator=g) >= 0.3).float()
    if kind == "lead-frames":
        valid = torch.ones(B, T, N)
        valid[:, :max(T // 2, 1)] = 0.0
    elif kind == "clip-padded":
        valid[B - 1] = 0.0
    else:
        assert kind == "random"
    return valid
