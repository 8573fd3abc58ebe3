"""CPU: the specification of the per-clip attention step (tests/clip_step_ref.py) against the specification of the window.
In fp64, step_ref at p - which is handed frames 0 .. p alone - equals frame p of oracle.clip_attention on all T frames:
frames after p and valid[:, > p] cannot matter.  With N = 1 and no mask it is the per-slot attention at p."""
import pytest
import torch

from clip_step_ref import MASKS, make_qkv, make_valid, step_ref
from oracle import layout_spec as O


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("B,T,N,d", [(1, 4, 8, 64), (3, 8, 12, 64), (2, 4, 40, 128)])
def test_step_ref_is_frame_p_of_the_window(B, T, N, d, kind):
    qkv = make_qkv(B, T, N, d, seed=T * 100 + N).double()
    valid = make_valid(kind, B, T, N, seed=N)
    full = O.clip_attention(qkv, d // 64, valid.double() if valid is not None else None)
    for p in range(T):
        got = step_ref(qkv, valid, p)
        assert tuple(got.shape) == (B, N, d) and bool(torch.isfinite(got).all())
        err = float((got - full[:, p]).abs().max())
        assert err <= 1e-12 * float(full.abs().max()), (p, err)
    if kind == "clip-padded":                    # every token of that clip sees only itself: its output is its own V row
        for p in range(T):
            assert torch.allclose(step_ref(qkv, valid, p)[B - 1], qkv[B - 1, p, :, 2 * d:], rtol=0, atol=1e-12)
    if kind == "lead-frames" and T >= 4:         # a query of a padded frame sees itself alone ...
        assert torch.allclose(step_ref(qkv, valid, 1), qkv[:, 1, :, 2 * d:], rtol=0, atol=1e-12)


def test_step_ref_changes_with_what_it_may_see():
    """(the equality above is not vacuous: an earlier frame and the mask of an earlier frame do matter)"""
    B, T, N, d, p = 2, 4, 8, 64, 2
    qkv = make_qkv(B, T, N, d, seed=3).double()
    valid = make_valid("random", B, T, N, seed=3)
    base = step_ref(qkv, valid, p)
    q2 = qkv.clone()
    q2[:, 0, :, d:] += 1.0
    assert not torch.allclose(step_ref(q2, valid, p), base)
    assert not torch.allclose(step_ref(qkv, 1.0 - valid, p), base)


@pytest.mark.parametrize("T,d", [(8, 64), (32, 192)])
def test_one_slot_is_per_slot_attention(T, d):
    qkv = make_qkv(3, T, 1, d, seed=T + d).double()
    full = O.temporal_attention(qkv, d // 64)
    for p in (0, 1, T // 2, T - 1):
        assert torch.allclose(step_ref(qkv, None, p), full[:, p], rtol=0, atol=1e-12 * float(full.abs().max()))
