"""The forward walk of csrc/attention_clip.hip restated on the CPU, and the edge cases of the per-clip attention tests.
Plain module: test infrastructure only, no fixtures, nothing collected.

  census        which tile paths a (B, T, N, valid[, scores]) input takes in attn_clip_fwd_kernel: 128-query blocks, four
                32-query waves, clip_key_tiles, CLIP_TILE_HIDDEN / CLIP_TILE_ELEMENTWISE / CLIP_VISIBLE with the padded-slot
                rule valid <= 0 - counted per (clip, block, wave, tile)
  census_keys   the same for attn_clip_dkv_kernel: clip_first_query_tile, CLIP_QUERY_TILE_HIDDEN
  walk_forward  the forward evaluated tile by tile in the kernel's order (log2-domain scores, masking to -inf before the row
                maximum, m_use, alpha, l_run, one multiplication by 1 / l_run, lse = m_run + log2(l_run)), with one named
                MUTATION at a time: what a test case must be able to tell from the kernel
  CASES         the inputs of tests/test_clip_walk_cpu.py (which shows what each reaches and which mutation it catches) and
                tests/test_hip_clip_attention_edges.py (which runs them on the kernels)
"""
import math

import torch

CKT, CQB, CINVALID = 32, 128, 0x10000
LOG2E = 1.0 / math.log(2.0)
CLIP_SCALE_LOG2_F32 = 0.18033688011112042          # the kernel's float constant: log2(e) / sqrt(64)
MUTATIONS = ("no_guard", "skip_rescale", "whole_when_elementwise", "no_self", "invalid_lt0", "kend_one_frame_short")


def clip_key_tiles(q0, nq, N, S, short=False):
    kend = ((q0 + nq - 1) // N + (0 if short else 1)) * N
    return (min(kend, S) + CKT - 1) // CKT


def clip_first_query_tile(kb0, N):
    return ((kb0 // N) * N) // CKT


def _frame_code(B, T, N, valid, lt0=False):
    """(B, S) frame of every token, + CINVALID where it is a padded slot"""
    S = T * N
    code = (torch.arange(S) // N)[None].expand(B, S).clone()
    if valid is not None:
        v = valid.reshape(B, S)
        code += CINVALID * (v < 0 if lt0 else v <= 0).long()
    return code


def log2_scores(qkv, heads, dtype=torch.float64):
    """(B, H, S, S) unmasked log2-domain scores, tokens frame-major"""
    B, T, N, d3 = qkv.shape
    x = qkv.to(dtype).reshape(B, T * N, 3, heads, 64)
    q, k = x[:, :, 0].permute(0, 2, 1, 3), x[:, :, 1].permute(0, 2, 1, 3)
    return (q @ k.transpose(-1, -2)) * (LOG2E / 8.0)


def census(B, T, N, valid, scores=None):
    """Counts per (clip, block, wave, tile) of the forward walk; with `scores` ((B, H, S, S) or (B, S, S), log2 domain,
    unmasked) the two score counts are per head as well and `scored` is their denominator (computed tiles x heads)."""
    S = T * N
    assert S % CKT == 0
    c = dict(inactive_wave=0, hidden=0, whole=0, elementwise=0, first_all_masked=0, later_all_masked=0, max_moved=0,
             rescale_skipped=0, scored=0)
    code = _frame_code(B, T, N, valid)
    if scores is not None and scores.dim() == 3:
        scores = scores[:, None]
    for q0 in range(0, S, CQB):
        nq = min(S - q0, CQB)
        ntiles = clip_key_tiles(q0, nq, N, S)
        for w in range(4):
            if not 32 * w < nq:
                c["inactive_wave"] += B
                continue
            sq = q0 + 32 * w + torch.arange(32)
            tq = sq // N
            tq_min, tq_max = (q0 + 32 * w) // N, (q0 + 32 * w + 31) // N
            seen = torch.zeros(B, 32, dtype=torch.bool)
            m_run = None if scores is None else torch.full((B, scores.shape[1], 32), float("-inf"), dtype=scores.dtype)
            first = True
            for j in range(ntiles):
                k0 = j * CKT
                if k0 // N > tq_max:
                    c["hidden"] += B
                    continue
                sk = k0 + torch.arange(32)
                if valid is not None or (k0 + CKT - 1) // N > tq_min:
                    c["elementwise"] += B
                    vis = (code[:, None, k0:k0 + 32] <= tq[None, :, None]) | (sk[None, None, :] == sq[None, :, None])
                else:
                    c["whole"] += B
                    vis = torch.ones(B, 32, 32, dtype=torch.bool)
                none = ~vis.any(-1)                                   # (B, 32): lanes with every key of the tile invisible
                c["first_all_masked"] += int((none & ~seen).any(-1).sum())
                c["later_all_masked"] += int((none & seen).any(-1).sum())
                if scores is not None:
                    st = scores[:, :, sq, k0:k0 + 32].masked_fill(~vis[:, None], float("-inf"))
                    m_new = torch.maximum(m_run, st.amax(-1))
                    moved = m_new > m_run                             # (B, H, 32)
                    c["scored"] += B * scores.shape[1]
                    c["max_moved"] += int((moved & seen[:, None]).any(-1).sum())
                    if not first:                                     # alpha == 1 on every lane: P::rescale is skipped
                        c["rescale_skipped"] += int((~moved & seen[:, None]).all(-1).sum())
                    m_run = m_new
                seen = seen | ~none
                first = False
    return c


def census_keys(B, T, N, valid):
    """Counts per (clip, block, wave[, query tile]) of the key-owner walk (attn_clip_dkv_kernel)."""
    S = T * N
    c = dict(inactive_wave=0, not_staged=0, hidden=0, computed=0, own_all_padded=0)
    code = _frame_code(B, T, N, valid)
    for kb0 in range(0, S, CQB):
        nk = min(S - kb0, CQB)
        jfirst = clip_first_query_tile(kb0, N)
        for w in range(4):
            if not 32 * w < nk:
                c["inactive_wave"] += B
                continue
            lo = kb0 + 32 * w
            c["own_all_padded"] += int((code[:, lo:lo + 32] >= CINVALID).all(-1).sum())
            tk_min = lo // N
            c["not_staged"] += B * jfirst
            for j in range(jfirst, S // CKT):
                c["hidden" if (j * CKT + CKT - 1) // N < tk_min else "computed"] += B
    return c


def walk_forward(qkv, valid, heads, dtype, mutate=None):
    """-> (out (B,T,N,d), lse (B*H*S,) in the log2 domain) in `dtype` (float64, or float32 with the scale folded into q
    as ClipF32 does).  All 32-query waves advance together over the key tiles; a wave whose tile is hidden or beyond its
    block's clip_key_tiles keeps its state."""
    assert mutate is None or mutate in MUTATIONS
    B, T, N, d3 = qkv.shape
    S, G = T * N, T * N // CKT
    x = qkv.to(dtype).reshape(B, S, 3, heads, 64)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))     # (B, H, S, 64)
    scale = CLIP_SCALE_LOG2_F32 if dtype == torch.float32 else LOG2E / 8.0
    s = (q * scale) @ k.transpose(-1, -2)
    frame, tok = torch.arange(S) // N, torch.arange(S)
    code = _frame_code(B, T, N, valid, lt0=mutate == "invalid_lt0")
    g0 = torch.arange(G) * CKT
    q0 = (g0 // CQB) * CQB
    nq = torch.clamp(S - q0, max=CQB)
    kend = ((q0 + nq - 1) // N + (0 if mutate == "kend_one_frame_short" else 1)) * N
    ntiles = (torch.clamp(kend, max=S) + CKT - 1) // CKT
    tq_min, tq_max = g0 // N, (g0 + CKT - 1) // N
    ninf = float("-inf")
    m = torch.full((B, heads, S), ninf, dtype=dtype)
    l = torch.zeros(B, heads, S, dtype=dtype)
    o = torch.zeros(B, heads, S, 64, dtype=dtype)
    for j in range(G):
        k0 = j * CKT
        computed = (j < ntiles) & ~(k0 // N > tq_max)
        if not bool(computed.any()):
            continue
        if valid is not None:
            elem = torch.full((G,), mutate != "whole_when_elementwise")
        else:
            elem = (k0 + CKT - 1) // N > tq_min
        vis = code[:, None, k0:k0 + CKT] <= frame[None, :, None]                        # (B, S, 32)
        if mutate != "no_self":
            vis = vis | (tok[None, None, k0:k0 + CKT] == tok[None, :, None])
        vis = vis | ~elem.repeat_interleave(CKT)[None, :, None]
        st = s[..., k0:k0 + CKT].masked_fill(~vis[:, None], ninf)
        m_new = torch.maximum(m, st.amax(-1))
        m_use = m_new if mutate == "no_guard" else torch.where(m_new == ninf, torch.zeros_like(m_new), m_new)
        alpha = torch.exp2(m - m_use)
        p = torch.exp2(st - m_use[..., None])
        l_new = l * alpha + p.sum(-1)
        o_new = (o if mutate == "skip_rescale" else o * alpha[..., None]) + p @ v[..., k0:k0 + CKT, :]
        cw = computed.repeat_interleave(CKT)
        m, l, o = torch.where(cw, m_new, m), torch.where(cw, l_new, l), torch.where(cw[:, None], o_new, o)
    out = o * (1.0 / l)[..., None]
    return out.permute(0, 2, 1, 3).reshape(B, T, N, heads * 64), (m + torch.log2(l)).reshape(-1)


# ------------------------------------------------------------------------------------------------------------ the cases
def _prefix(B, T, N, n_valid):
    nv = torch.tensor(n_valid)
    return (torch.arange(N)[None, None, :] < nv[:, None, None]).float().expand(B, T, N).contiguous()


def _lead_empty(B, T, N, g):
    v = torch.ones(B, T, N)
    v[0, :4] = 0.0
    v[1, :6] = 0.0
    return v


def _one_slot(B, T, N, g):
    v = torch.zeros(B, T, N)
    v[0, :, 5] = 1.0
    v[1, 2:, 11] = 1.0
    return v


NON_BINARY = (-1.0, -0.0, 0.0, 0.5, 2.0, 1.0, 1e-30, -1e-30)


def _non_binary(B, T, N, g):
    vals = torch.tensor(NON_BINARY)
    return torch.stack([torch.stack([vals.roll(t + 3 * b) for t in range(T)]) for b in range(B)])


def _alt_x5(qkv, d):
    qkv[:, :, ::2, :2 * d] *= 5.0


def _late_max(qkv, d):
    T = qkv.shape[1]
    qkv[..., d:2 * d] *= (1.0 + torch.arange(T, dtype=torch.float32))[None, :, None, None]


def _first_max(qkv, d):
    qkv[:, 0, :, d:2 * d] *= 6.0


MASKS = {
    "null": lambda B, T, N, g: None,
    "random": lambda B, T, N, g: (torch.rand(B, T, N, generator=g) > 0.3).float(),
    "prefix": lambda B, T, N, g: _prefix(B, T, N, [12, 15][:B]),
    "lead-empty": _lead_empty,
    "prefix-64": lambda B, T, N, g: _prefix(B, T, N, [1, 31, 32, 33]),
    "all-invalid": lambda B, T, N, g: torch.zeros(B, T, N),
    "one-slot": _one_slot,
    "non-binary": _non_binary,
}
SCORES = {"alt-x5": _alt_x5, "late-max": _late_max, "first-max": _first_max}

# name -> (B, T, N, d, mask recipe, score recipe)
CASES = {
    "lead-empty": (2, 8, 8, 64, "lead-empty", None),
    "prefix-64": (4, 2, 64, 128, "prefix-64", None),                 # d = 128: the head index matters
    "all-invalid": (1, 4, 16, 64, "all-invalid", None),
    "one-slot": (2, 4, 16, 64, "one-slot", None),
    "non-binary": (2, 4, 8, 64, "non-binary", None),
}
for _s in SCORES:
    for _m in ("null", "prefix"):
        CASES["%s/%s" % (_s, _m)] = (2, 8, 16, 64, _m, _s)
SHAPES = [(1, 32, 1), (1, 64, 1), (2, 64, 2), (1, 1, 32), (1, 1, 160), (1, 2, 160), (1, 3, 96)]
for _b, _t, _n in SHAPES:
    for _m in ("null", "random"):
        CASES["%dx%dx%d/%s" % (_b, _t, _n, _m)] = (_b, _t, _n, 64, _m, None)
MASK_CASES = ("lead-empty", "prefix-64", "all-invalid", "one-slot", "non-binary")
SEEDS = {"first-max/null": 0, "first-max/prefix": 0}    # where a count depends on the draw: chosen by the census


def make_case(name):
    """-> (qkv (B,T,N,3d), gy (B,T,N,d), valid (B,T,N) or None), fp32 on the CPU; the same tensors for every caller"""
    B, T, N, d, mask, score = CASES[name]
    g = torch.Generator().manual_seed(SEEDS.get(name, 4000 + sorted(CASES).index(name)))
    qkv = torch.randn(B, T, N, 3 * d, generator=g)
    gy = torch.randn(B, T, N, d, generator=g)
    valid = MASKS[mask](B, T, N, g)
    if score is not None:
        SCORES[score](qkv, d)
    return qkv, gy, valid
