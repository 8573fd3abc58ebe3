"""The frame-local walk of csrc/attention_clip.hip (its FRAME instantiations, vlg_attention_frame_*) stated once in Python:
which tiles an owner block walks and how a wave classes a tile.  The kernel comments cite these functions;
tests/test_frame_walk_cpu.py checks them by brute force.  Plain module: test infrastructure only, nothing collected.

Tokens of a clip are frame-major, s = t*N + n; a tile is 32 consecutive tokens, an owner block 128 (four waves x 32).
"""
CKT, CQB = 32, 128
HIDDEN, ELEMENTWISE, WHOLE = "hidden", "elementwise", "whole"


def visible(sq, sk, N, valid=None):
    """FRAME_VISIBLE: query token sq sees key token sk iff they share a frame and the key is not padded, or sk is sq itself.
    valid: None or a flat sequence over the clip's tokens (frame-major), padded where <= 0."""
    if sq == sk:
        return True
    return sq // N == sk // N and (valid is None or valid[sk] > 0)


def first_tile(s0, N):
    """frame_first_tile: the tile holding the first token of the frame of token s0"""
    return ((s0 // N) * N) // CKT


def end_tile(s0, n, N, S):
    """clip_key_tiles: one past the tile holding the last token of the frame of token s0 + n - 1"""
    kend = ((s0 + n - 1) // N + 1) * N
    return (min(kend, S) + CKT - 1) // CKT


def owner_range(s0, N, S):
    """The tiles [first, end) an owner block at token s0 walks: a query-owner block (forward, dQ) its key tiles, a key-owner
    block (dK/dV) its query tiles - the rule is the same, from the block's frames alone."""
    n = min(S - s0, CQB)
    return first_tile(s0, N), end_tile(s0, n, N, S)


def step_range(p, N):
    """The key tiles [first, end) of the generation step at position p: those of frame p.  Tokens of a walked tile outside
    [p*N, (p + 1)*N) are not loaded."""
    return (p * N) // CKT, ((p + 1) * N + CKT - 1) // CKT


def classify(k0, w0, N, has_valid):
    """How a wave whose 32 owner tokens start at w0 treats the 32-token tile at k0 (FRAME_TILE_HIDDEN /
    FRAME_TILE_ELEMENTWISE): hidden when none of the tile's frames is among the wave's; element-wise when valid is given or
    the tile or the wave's own tokens hold a frame boundary; whole otherwise."""
    t_min, t_max = w0 // N, (w0 + CKT - 1) // N
    f_min, f_max = k0 // N, (k0 + CKT - 1) // N
    if f_max < t_min or f_min > t_max:
        return HIDDEN
    if has_valid or f_min != f_max or t_min != t_max:
        return ELEMENTWISE
    return WHOLE
