"""CPU: the frame-local walk rules of tests/frame_walk.py (what the FRAME instantiations of csrc/attention_clip.hip walk and
how they class a tile) against brute force over every (query, key) pair."""
import pytest

import frame_walk as W

SHAPES = [(T, N) for N in (1, 4, 8, 12, 32, 40, 64, 72, 136) for T in (1, 4, 8, 16) if (T * N) % 32 == 0]


def test_the_shape_list_is_not_empty():
    assert len(SHAPES) >= 20 and (4, 40) in SHAPES and (4, 72) in SHAPES and (1, 32) in SHAPES and (8, 4) in SHAPES


def _pairs_of_tiles(T, N):
    """{(query tile, key tile)} that hold at least one visible pair without a mask (same frame), by brute force"""
    S = T * N
    out = set()
    for sq in range(S):
        for sk in range((sq // N) * N, (sq // N + 1) * N):
            out.add((sq // W.CKT, sk // W.CKT))
    return out


@pytest.mark.parametrize("T,N", SHAPES)
def test_owner_walk_covers_every_visible_pair_and_stays_inside_the_frames(T, N):
    S = T * N
    need = _pairs_of_tiles(T, N)
    walked = set()
    for s0 in range(0, S, W.CQB):
        n = min(S - s0, W.CQB)
        lo, hi = W.owner_range(s0, N, S)
        assert 0 <= lo < hi <= S // W.CKT
        # nothing outside the span of the block's frames
        f0, f1 = s0 // N, (s0 + n - 1) // N
        assert lo * W.CKT + W.CKT > f0 * N and (hi - 1) * W.CKT < (f1 + 1) * N
        for w0 in range(s0, s0 + n, W.CKT):
            for j in range(lo, hi):
                cls = W.classify(j * W.CKT, w0, N, False)
                if cls != W.HIDDEN:
                    walked.add((w0 // W.CKT, j))
                pairs = [W.visible(sq, sk, N) for sq in range(w0, w0 + W.CKT) for sk in range(j * W.CKT, (j + 1) * W.CKT)]
                if cls == W.WHOLE:
                    assert all(pairs), "a whole tile holds an invisible pair"
                if cls == W.HIDDEN:
                    assert not any(pairs), "a hidden tile holds a visible pair"
    # the rule is symmetric, so the same set serves query owners (key tiles) and key owners (query tiles)
    assert need <= walked
    assert {(b, a) for a, b in need} <= walked


@pytest.mark.parametrize("T,N", SHAPES)
def test_masks_make_every_walked_tile_elementwise(T, N):
    S = T * N
    for s0 in range(0, S, W.CQB):
        lo, hi = W.owner_range(s0, N, S)
        for w0 in range(s0, min(s0 + W.CQB, S), W.CKT):
            for j in range(lo, hi):
                assert W.classify(j * W.CKT, w0, N, True) in (W.HIDDEN, W.ELEMENTWISE)
                assert (W.classify(j * W.CKT, w0, N, True) == W.HIDDEN) == (W.classify(j * W.CKT, w0, N, False) == W.HIDDEN)


@pytest.mark.parametrize("T,N", SHAPES)
def test_step_walks_the_tiles_of_its_frame_alone(T, N):
    for p in range(T):
        lo, hi = W.step_range(p, N)
        keys = set(range(p * N, (p + 1) * N))
        tiles = {s // W.CKT for s in keys}
        assert set(range(lo, hi)) == tiles                       # every key's tile, no tile without a key
        # (the step's queries all lie in frame p: its classification is taken with t_min = t_max = p)
        for j in range(lo, hi):
            f_min, f_max = (j * W.CKT) // N, (j * W.CKT + W.CKT - 1) // N
            assert f_min <= p <= f_max
            whole = f_min == f_max
            assert whole == all(s in keys for s in range(j * W.CKT, (j + 1) * W.CKT))


def test_visibility_rule():
    N = 4
    valid = [1.0] * 16
    valid[5] = 0.0
    assert W.visible(4, 6, N, valid) and W.visible(6, 4, N, valid)
    assert not W.visible(4, 5, N, valid) and W.visible(5, 5, N, valid) and W.visible(5, 4, N, valid)
    assert not W.visible(4, 3, N, valid) and not W.visible(4, 8, N, valid)
