"""CPU: the table of attention kinds (vlg/attention.py) against brute force - pair counts over every (query, key) pair under
the visibility rules the kernels' walks are stated with (tests/clip_walk.py, tests/frame_walk.py; per slot the plain
causal rule), the per-layer kinds against LayoutConfig, the lse rows, and step_flops against its formulas written out."""
import dataclasses

import pytest

import frame_walk
from vlg import attention as A
from vlg.spec import LayoutConfig, step_flops

CASES = [(4, 8), (8, 4), (4, 24), (16, 2)]           # (T, N)

# token s = t*N + n of a clip, frame-major.  No padded slots: the counts are of the unmasked launch
VISIBLE = {
    A.SLOT: lambda sq, sk, N: sq % N == sk % N and sk // N <= sq // N,        # its own slot, causal along time
    A.CLIP: lambda sq, sk, N: sk // N <= sq // N,                             # clip_walk: every slot of the frames <= t
    A.FRAME: lambda sq, sk, N: frame_walk.visible(sq, sk, N),                 # frame_walk: every slot of its own frame
}


@pytest.mark.parametrize("T,N", CASES)
def test_pair_counts_equal_brute_force(T, N):
    for kind, vis in VISIBLE.items():
        assert kind.pairs(T, N) == sum(vis(sq, sk, N) for sq in range(T * N) for sk in range(T * N)), kind.stem
        for p in range(T):                           # the generation step: the queries of frame p, the keys of the frames <= p
            want = sum(vis(sq, sk, N) for sq in range(p * N, (p + 1) * N) for sk in range((p + 1) * N))
            assert kind.step_pairs(N, p) == want, (kind.stem, p)
        assert sum(kind.step_pairs(N, p) for p in range(T)) == kind.pairs(T, N)


def test_rows_are_the_three_kernels_families():
    assert [(k.stem, k.family, k.per_clip, k.cached) for k in (A.SLOT, A.CLIP, A.FRAME)] == [
        ("vlg_attention", "attn", False, True), ("vlg_attention_clip", "attn_clip", True, False),
        ("vlg_attention_frame", "attn_frame", True, True)]
    assert [A.cached_by_default(m) for m in ("slot", "clip", "factored")] == [True, False, True]
    with pytest.raises(dataclasses.FrozenInstanceError):
        A.SLOT.stem = "other"


@pytest.mark.parametrize("n_layers", [1, 2, 3, 4, 5])
def test_layer_kinds_agree_with_the_config_and_lse_rows_are_ranks(n_layers):
    assert A.layer_kinds("slot", n_layers) == (A.SLOT,) * n_layers
    assert A.layer_kinds("clip", n_layers) == (A.CLIP,) * n_layers
    assert A.layer_kinds("factored", n_layers) == tuple(A.FRAME if l % 2 else A.SLOT for l in range(n_layers))
    for mode in ("slot", "clip", "factored"):
        cfg, kinds = LayoutConfig(attention=mode, n_layers=n_layers), A.layer_kinds(mode, n_layers)
        assert [cfg.frame_layer(l) for l in range(n_layers)] == [k is A.FRAME for k in kinds]
        assert cfg.n_frame_layers == kinds.count(A.FRAME) == (n_layers // 2 if mode == "factored" else 0)
        rows = A.lse_rows(kinds)
        per_clip = [l for l, k in enumerate(kinds) if k.per_clip]
        assert [rows[l] for l in per_clip] == list(range(len(per_clip)))           # its rank among the per-clip layers
        assert [rows[l] for l in per_clip] == [l if mode == "clip" else l // 2 for l in per_clip]


@pytest.mark.parametrize("mode,n_layers", [("slot", 4), ("clip", 4), ("factored", 3)])
def test_step_flops_are_the_formulas_written_out(mode, n_layers):
    cfg = LayoutConfig(B=3, T=8, N=12, d=128, n_layers=n_layers, attention=mode)
    B, T, N, d, L, M = cfg.B, cfg.T, cfg.N, cfg.d, cfg.n_layers, cfg.tokens
    per_layer = 24.0 * M * d * d
    attn = 4.0 * B * N * T * T * d / 2.0                                    # per slot: the causal half
    if mode == "clip":
        attn = 4.0 * B * d * N * N * T * (T + 1) / 2.0
    if mode == "factored":                                                  # the mean over the layers, L // 2 of them FRAME
        attn += (4.0 * B * d * N * N * T - attn) * (L // 2) / L
    fwd = L * (per_layer + attn) + 2.0 * M * d * cfg.n_out
    assert step_flops(cfg) == {"gemm_fwd_per_layer": per_layer, "fwd": fwd, "fwd_bwd": 3.0 * fwd + 0.5 * L * attn}
