"""Every path the 3x3-convolution planner (conv_plan, csrc/conv.hip) can pick, at chip-filling sizes, against fp64.

The planner chooses the tile, split-K, the tail split and - inside the kernel - the fast or the general main loop and
epilogue from the call's shape and optional operands alone, so a path is reached by choosing a shape.  CASES names the
path each shape is meant to reach, forward and data gradient, in both precisions; `Plan` / `conv_loop` below
restate the planner and the kernel's predicates in Python (with the conv.hip lines they mirror).  The host tests keep
the table and the mirror honest: test_mirror_names_the_path (table vs mirror), test_mirror_matches_the_library_queries
(mirror vs the built library, over the table and sweeps across every threshold) and test_table_covers_every_path.

The GPU tests run each case the two ways the project calls a convolution:
  gridnet  no workspace, a real PReLU slope, slope-gradient partials, the residual epilogue on some rows (vlg/gridnet.py);
  trunk    workspace from the query, slope 0 (ReLU), no partials, VLG_CEPI_ACCUM into a prior gradient (the frozen trunks).
fp32 is compared with fp64 torch-CPU autograd on the same fp32 inputs (test_hip_conv_ops._reference) to
test_hip_conv_ops.TOL = 1e-4 of each tensor's scale; bf16 keeps the contract of test_hip_conv_bf16 (1e-5 of scale against
fp64 on bf16-rounded operands, at least 10x worse against the unrounded result).  Every output buffer - y, dx when not
accumulating, the workspace, the slope partials, the weight-gradient slabs with a tail and a spare slab - starts as NaN
sentinels: owned elements come back finite, halo rows exactly zero, guard rows / slab tails / spare entries untouched,
padding lanes cout..cout_p of y untouched (they stay the zeros the allocation holds), padded weight lanes of dW zero.
test_two_gib_switch sits on both sides of the 1 << 31 byte limit of the fast loop (conv.hip:118-121).

Worst error measured on one MI355X, as a fraction of the tensor's scale (every case prints its own CONVERR / BF16ERR lines):
  fp32, bar 1e-4                        forward   data gradient
    128x32 BK16  fast / general         7.4e-7 / 6.4e-7    7.4e-7 / 6.3e-7
    128x32       fast / general         1.3e-6 / 1.5e-6    1.3e-6 / 6.7e-7
    128x96       fast / general         6.0e-7 / 5.6e-7    1.3e-6 / 1.0e-6
    64x64        fast / general         1.3e-6 / 1.3e-6    1.6e-6 / 6.9e-7
    128x64       fast / general         4.1e-7 / 1.1e-6    9.1e-7 / 7.5e-7
    64x128       fast / general         1.5e-6 / 1.3e-6    2.2e-6 / 6.4e-7
    128x128      fast / general         1.5e-6 / 9.5e-7    1.6e-6 / 4.9e-7
    128x128      tail / split-K         1.6e-6 / 3.0e-7    9.8e-7 / 2.1e-7   (split-K at K = 9 x 512: 8.6e-7 / 5.3e-7)
    fast loop, general epilogue (CoordConv data gradient): 1.3e-6;  dW 1.6e-6, db 7.6e-7, slope gradient 2.7e-7
    2 GiB switch: 1.6e-6 under the limit (fast), 1.4e-6 over it (general)
  bf16 against the bf16-operand reference, bar 1e-5 (against the unrounded one: 9e-4 .. 3e-3)
    128x32 2.8e-7 / 2.5e-7, 64x64 5.0e-7 / 5.2e-7, 128x64 4.1e-7 / 5.4e-7, 128x96 5.3e-7 / 4.9e-7,
    64x128 8.1e-7 / 8.6e-7, 128x128 5.4e-7 / 7.2e-7, split-K 2.5e-7 / 1.5e-7;  dW 4.1e-7, db 3.2e-7, slope 8.8e-10
so the fp32 bar leaves about 45x and the bf16 bar about 12x of room.
"""
import pytest
import torch

from test_hip_conv_bf16 import _check, _padded_view, _ref, _sentinel_checks
from test_hip_conv_ops import TOL, _away_from_kink, _Harness, _reference

FP32, BF16 = "fp32", "bf16"
FWD, DGRAD, WGRAD = "fwd", "dgrad", "wgrad"
NAN = float("nan")
SPARE = 64                                     # sentinel floats kept behind every workspace / partial vector


def _cdiv(a, b):
    return -(-a // b)


def _ceil32(c):
    return _cdiv(c, 32) * 32


# ------------------------------------------------------------------------------------------------ planner mirror
def few_blocks(rows, tiles_n):
    """conv.hip:826-830 - 64-row tiles when they lower the busiest CU's load by more than 15 %."""
    b128, b64 = _cdiv(rows, 128) * tiles_n, _cdiv(rows, 64) * tiles_n
    return b128 < 384 or 10 * _cdiv(b64, 256) < 17 * _cdiv(b128, 256)


def split_96(rows):
    """conv.hip:832 - 96 columns as three 32-wide tiles below 400 row tiles."""
    return _cdiv(rows, 128) < 400


def conv_tail_plan(rows, tile, n_cols, kc, ldc):
    """conv.hip:844-875 -> None, or (tail tiles, K ranges, contraction per range, first tail row, workspace floats)."""
    bm, bn, bk = tile
    if kc % bk:
        return None
    tiles_m, tiles_n = _cdiv(rows, bm), _cdiv(n_cols, bn)
    tiles = tiles_m * tiles_n
    rem = tiles % 256
    if tiles < 256 or rem == 0:
        return None
    tail_rows_t = _cdiv(rem, tiles_n)
    tail_tiles = tail_rows_t * tiles_n
    if tail_tiles >= tiles:
        return None
    ktiles = kc // bk
    tile_us = 2.0 * bm * bn * float(kc) / 0.5e6
    best, best_per = 0.0, 0
    for sp in range(2, 9):
        per = _cdiv(ktiles, sp)
        if per * bk < 128:
            break
        real = _cdiv(ktiles, per)
        rounds = float((tail_tiles * real + 255) // 256)
        saving = tile_us * (1.0 - rounds * per / ktiles) - rounds * 3.0 - 5.0
        if saving > best:
            best, best_per = saving, per
    if best < 3.0:
        return None
    splits = _cdiv(ktiles, best_per)
    row0 = (tiles_m - tail_rows_t) * bm
    return tail_tiles, splits, best_per * bk, row0, splits * (rows - row0) * ldc


def conv_tile(rows, n_cols, n_valid, kc=0):
    """conv.hip:879-892 - fp32 forward (n_cols = cout_p, n_valid = cout) / data gradient (both cin_p) tile; kc > 0 when
    the launch may take the tail plan."""
    if n_cols == 32:
        return (128, 32, 16)
    if n_cols == 96:
        return (128, 32, 32) if split_96(rows) else (128, 96, 32)
    bn = 64 if n_cols == 64 else 128
    tiles_n = 1 if n_cols == 64 else _cdiv(n_valid, 128)
    if kc > 0:
        t128 = _cdiv(rows, 128) * tiles_n
        if t128 >= 256 and (t128 % 256 == 0 or conv_tail_plan(rows, (128, bn, 32), n_valid, kc, 1)):
            return (128, bn, 32)
    return (64 if few_blocks(rows, tiles_n) else 128, bn, 32)


def bf16_tile(rows, n_cols):
    """conv.hip:895-899."""
    bn = n_cols if n_cols in (32, 64, 96) else 128
    t128 = _cdiv(rows, 128) * _cdiv(n_cols, bn)
    return (64 if bn != 96 and bn >= 64 and t128 < 512 else 128, bn, 32)


def conv_splits(prec, rows_out, cin_p, cout, cout_p):
    """conv.hip:914-924 - split-K of the coarse trunk levels: fewer than 200 (fp32) / 256 (bf16) 128 x 128 tiles."""
    if cout_p < 128 or cout != cout_p or cin_p < 128:
        return 1
    if prec == BF16 and cout_p & 127:
        return 1
    b128 = _cdiv(rows_out, 128) * _cdiv(cout_p, 128)
    if b128 >= (256 if prec == BF16 else 200):
        return 1
    s = min(512 // b128, 8)
    ktiles = 9 * cin_p // 32
    while s > 1 and ktiles // s < 8:
        s -= 1
    return 1 if s < 2 else s


def conv_wgrad_bm(prec, cout_p):
    """conv.hip:974-977."""
    if prec == BF16:
        return 128 if cout_p % 128 == 0 else 96 if cout_p == 96 else 64 if cout_p % 64 == 0 else 32
    return cout_p if cout_p in (64, 96) else 32


def wgrad_ranges(prec, rows, cin_p, cout_p):
    """conv.hip:1000-1011 -> (row ranges, rows per range)."""
    tiles = (cout_p // conv_wgrad_bm(prec, cout_p)) * _cdiv(9 * cin_p, 128)
    want = max(min(512 // tiles, _cdiv(rows, 256)), 1)
    per = _cdiv(_cdiv(rows, want), 32) * 32
    return _cdiv(rows, per), per


class Plan:
    """conv.hip:988-1039 (conv_plan) for a forward or data-gradient launch."""

    def __init__(self, prec, mode, rows, cin_p, cout, cout_p, ws=False, ws_cap=None, tables=False, da_slab=False,
                 prelu_epi=False):
        n_cols, n_valid = (cout_p, cout) if mode == FWD else (cin_p, cin_p)
        kc = 9 * (cin_p if mode == FWD else cout_p)
        self.rows, self.n_cols, self.n_valid, self.kc = rows, n_cols, n_valid, kc
        self.splits, self.kc_per_split, self.tail, self.ws_floats = 1, kc, None, 0
        split_ok = ws and (mode == FWD or (not da_slab and not tables))
        splits = 1
        if split_ok:
            splits = conv_splits(prec, rows, cin_p, cout, cout_p) if mode == FWD else conv_splits(prec, rows, cout_p, cin_p, cin_p)
        if splits > 1:
            self.tile, self.splits = (128, 128, 32), splits
            self.kc_per_split = _cdiv(kc // 32, splits) * 32
            self.ws_floats = splits * rows * n_cols
        elif prec == BF16:
            self.tile = bf16_tile(rows, n_cols)
        else:
            # (n_valid == n_cols: the finish kernel sums whole rows, a padded cout would leave workspace lanes unwritten)
            tail_ok = ws and not tables and not da_slab and not prelu_epi and n_valid == n_cols
            self.tile = conv_tile(rows, n_cols, n_valid, kc if tail_ok else 0)
            if tail_ok:
                tl = conv_tail_plan(rows, self.tile, n_valid, kc, n_cols)
                if tl and (ws_cap is None or tl[4] <= ws_cap):
                    self.tail, self.ws_floats = tl, tl[4]
        self.tiles_m, self.tiles_n = _cdiv(rows, self.tile[0]), _cdiv(n_cols, self.tile[1])
        self.slopes = self.tiles_m * self.tiles_n

    @property
    def kind(self):
        if self.splits > 1:
            return "splitK%d" % self.splits
        if self.tail:
            return "tail%dx%d" % (self.tail[0], self.tail[1])
        return "plain"

    @property
    def tile_name(self):
        return "%dx%d" % self.tile[:2] + (" BK16" if self.tile[2] == 16 else "")


LIMIT = 1 << 31


def conv_loop(prec, mode, p, lda, wp, tables, act_ch, cin_p):
    """The main loop and epilogue the blocks of plan p take: conv.hip:115-122 (`fast`) and :553-554 (`fast_epi`) for
    fp32; the bf16 kernel (conv_bf16.hip) has one loop, the general one.  lda = channels of the gathered operand (cin_p
    forward, cout_p data gradient); act_ch as the call passes it."""
    if prec == BF16:
        return "general"
    bm, bn, bk = p.tile
    M, N = p.rows, p.n_valid
    ldb, ldc = 9 * cin_p, p.n_cols
    a_bytes = (M + 2 * (wp + 1)) * lda * 4
    b_bytes = (N if mode == FWD else lda) * ldb * 4
    shape_ok = (not tables and wp > 0 and N % bn == 0 and a_bytes + bm * lda * 4 < LIMIT and b_bytes < LIMIT and
                (mode != FWD or act_ch >= lda))
    # K ranges: every tile's (split-K or one range), and the tail tiles' own
    ranges = [min((s + 1) * p.kc_per_split, p.kc) - s * p.kc_per_split for s in range(p.splits)]
    kinds = set()
    for part, exts in ((False, ranges), (True, [min((s + 1) * p.tail[2], p.kc) - s * p.tail[2] for s in range(p.tail[1])] if p.tail else [])):
        for ext in exts:
            fast = shape_ok and ext % bk == 0
            # (a split-K launch passes act_ch = N: the finish kernel cuts the constant channels, conv.hip:1094)
            act_cut = N if part or p.splits > 1 else act_ch
            fast_epi = fast and (mode != DGRAD or act_cut >= N) and M * ldc * 4 < LIMIT
            kinds.add("fast" if fast_epi else "fast loop, general epilogue" if fast else "general")
    assert len(kinds) == 1, kinds              # (K ranges are whole K tiles: every block of a launch takes the same loop)
    return kinds.pop()


def wgrad_loop(prec, rows, cin_p, cout_p, wp, tables, act_ch):
    """conv.hip:123-128 - the weight gradient's fast loop (fp32; every row range starts on a K tile)."""
    if prec == BF16:
        return "general"
    a_bytes, b_bytes = rows * cout_p * 4, (rows + 2 * (wp + 1)) * cin_p * 4
    fast = not tables and wp > 0 and act_ch >= cin_p and a_bytes < LIMIT and b_bytes < LIMIT and cout_p * 9 * cin_p * 4 < LIMIT
    return "fast" if fast else "general"


# ------------------------------------------------------------------------------------------------ the case table
def _rows(b, H, W):
    return b * (H + 2) * (W + 2)


class Case:
    """One shape, called the gridnet or the trunk way, and the path (tile, kind, loop) it is meant to reach: forward and
    data gradient, fp32 and bf16.  act_ch None = every channel is activated (the call passes cin_p, as GridNetHIP does)."""

    def __init__(self, name, shape, call, paths, act_ch=None, resid=False, slope=0.25):
        self.name, self.shape, self.call, self.paths = name, shape, call, paths
        self.act_ch, self.resid, self.slope = act_ch, resid, 0.0 if call == "trunk" else slope
        b, H, W, cin, cout, stride = shape
        self.cin_p, self.cout_p = _ceil32(cin), _ceil32(cout)
        self.rows_in = _rows(b, H, W)
        self.rows_out = self.rows_in if stride == 1 else _rows(b, H // 2, W // 2)
        self.trunk, self.tables, self.wp = call == "trunk", stride == 2, W + 2
        self.act_arg = self.cin_p if act_ch is None else act_ch

    def plan(self, prec, mode, ws_cap=None):
        if mode == FWD:
            return Plan(prec, FWD, self.rows_out, self.cin_p, self.shape[4], self.cout_p, ws=self.trunk, ws_cap=ws_cap,
                        tables=self.tables)
        return Plan(prec, DGRAD, self.rows_in, self.cin_p, self.shape[4], self.cout_p, ws=self.trunk, ws_cap=ws_cap,
                    tables=self.tables, da_slab=not self.trunk)

    def path(self, prec, mode):
        p = self.plan(prec, mode)
        lda = self.cin_p if mode == FWD else self.cout_p
        return "%s %s %s" % (p.tile_name, p.kind, conv_loop(prec, mode, p, lda, self.wp, self.tables, self.act_arg, self.cin_p))


G, T = "gridnet", "trunk"
FLGE = "fast loop, general epilogue"           # data gradient of a CoordConv: the constant channels are cut per element
CASES = [
    # name, (b, H, W, cin, cout, stride), call, {precision: (forward path, data-gradient path)}
    Case("96ch above split_96", (4, 128, 128, 96, 96, 1), G, resid=True, slope=0.17, paths={
        FP32: ("128x96 plain fast", "128x96 plain fast"), BF16: ("128x96 plain general", "128x96 plain general")}),
    Case("96ch below split_96", (3, 128, 128, 96, 96, 1), G, paths={
        FP32: ("128x32 plain fast", "128x32 plain fast"), BF16: ("128x96 plain general", "128x96 plain general")}),
    Case("64ch 512 full tiles", (4, 126, 126, 64, 64, 1), G, resid=True, paths={
        FP32: ("128x64 plain fast", "128x64 plain fast"), BF16: ("128x64 plain general", "128x64 plain general")}),
    Case("64ch few_blocks", (4, 128, 128, 64, 64, 1), G, slope=-0.3, paths={
        FP32: ("64x64 plain fast", "64x64 plain fast"), BF16: ("128x64 plain general", "128x64 plain general")}),
    Case("128ch 512 full tiles", (4, 126, 126, 128, 128, 1), G, paths={
        FP32: ("128x128 plain fast", "128x128 plain fast"), BF16: ("128x128 plain general", "128x128 plain general")}),
    Case("128ch small", (2, 64, 64, 128, 128, 1), G, resid=True, paths={
        FP32: ("64x128 plain fast", "64x128 plain fast"), BF16: ("64x128 plain general", "64x128 plain general")}),
    Case("32ch", (4, 128, 128, 32, 32, 1), G, paths={
        FP32: ("128x32 BK16 plain fast", "128x32 BK16 plain fast"), BF16: ("128x32 plain general", "128x32 plain general")}),
    Case("two column tiles", (4, 64, 64, 128, 256, 1), G, paths={
        FP32: ("64x128 plain fast", "64x128 plain fast"), BF16: ("64x128 plain general", "64x128 plain general")}),
    Case("down 64->96 at b=8", (8, 128, 128, 64, 96, 2), G, paths={
        FP32: ("128x32 plain general", "128x64 plain general"), BF16: ("128x96 plain general", "128x64 plain general")}),
    Case("down 32->64 at 256x256", (4, 256, 256, 32, 64, 2), G, slope=0.1, paths={
        FP32: ("64x64 plain general", "128x32 BK16 plain general"), BF16: ("128x64 plain general", "128x32 plain general")}),
    Case("coord 96+2 -> 96", (4, 128, 128, 98, 96, 1), G, act_ch=96, resid=True, paths={
        FP32: ("128x96 plain general", "64x128 plain " + FLGE), BF16: ("128x96 plain general", "128x128 plain general")}),
    Case("coord 64+2 -> 64", (4, 126, 126, 66, 64, 1), G, act_ch=64, paths={
        FP32: ("128x64 plain general", "128x96 plain " + FLGE), BF16: ("128x64 plain general", "128x96 plain general")}),
    Case("coord 32+2 -> 32", (4, 128, 128, 34, 32, 1), G, act_ch=32, paths={
        FP32: ("128x32 BK16 plain general", "64x64 plain " + FLGE), BF16: ("128x32 plain general", "128x64 plain general")}),
    Case("partial column tile, padded cout", (4, 128, 128, 64, 130, 1), G, paths={
        FP32: ("128x128 plain general", "64x64 plain fast"), BF16: ("128x128 plain general", "128x64 plain general")}),
    Case("partial column tile, 64 rows", (2, 64, 64, 64, 160, 1), G, resid=True, paths={
        FP32: ("64x128 plain general", "64x64 plain fast"), BF16: ("64x128 plain general", "64x64 plain general")}),
    Case("down 96->128", (4, 128, 128, 96, 128, 2), G, paths={
        FP32: ("64x128 plain general", "128x96 plain general"), BF16: ("64x128 plain general", "128x96 plain general")}),
    Case("down 96->64 small", (2, 64, 64, 96, 64, 2), G, paths={
        FP32: ("64x64 plain general", "128x32 plain general"), BF16: ("64x64 plain general", "128x96 plain general")}),
    Case("down 128->64, 512 tiles", (4, 126, 126, 128, 64, 2), G, paths={
        FP32: ("64x64 plain general", "128x128 plain general"), BF16: ("64x64 plain general", "128x128 plain general")}),
    Case("down 128->96 small", (2, 64, 64, 128, 96, 2), G, slope=-0.2, paths={
        FP32: ("128x32 plain general", "64x128 plain general"), BF16: ("128x96 plain general", "64x128 plain general")}),
    Case("down 64->96 small", (4, 64, 64, 64, 96, 2), G, paths={
        FP32: ("128x32 plain general", "64x64 plain general"), BF16: ("128x96 plain general", "64x64 plain general")}),
    Case("trunk 128ch tail", (4, 128, 128, 128, 128, 1), T, paths={
        FP32: ("128x128 tail17x8 fast", "128x128 tail17x8 fast"), BF16: ("128x128 plain general", "128x128 plain general")}),
    Case("trunk 256ch tail, two column tiles", (4, 64, 64, 256, 256, 1), T, paths={
        FP32: ("128x128 tail18x8 fast", "128x128 tail18x8 fast"), BF16: ("64x128 plain general", "64x128 plain general")}),
    Case("trunk split-K", (2, 64, 64, 256, 128, 1), T, paths={
        FP32: ("128x128 splitK7 fast", "128x128 splitK3 fast"), BF16: ("128x128 splitK7 general", "128x128 splitK3 general")}),
    Case("trunk 512 tiles: no tail", (4, 126, 126, 128, 128, 1), T, paths={
        FP32: ("128x128 plain fast", "128x128 plain fast"), BF16: ("128x128 plain general", "128x128 plain general")}),
    Case("trunk between the split-K limits", (6, 64, 64, 128, 128, 1), T, paths={
        FP32: ("64x128 plain fast", "64x128 plain fast"), BF16: ("128x128 splitK2 general", "128x128 splitK2 general")}),
    Case("trunk 512ch split-K, K = 9 x 512", (4, 32, 32, 512, 512, 1), T, paths={
        FP32: ("128x128 splitK3 fast", "128x128 splitK3 fast"), BF16: ("128x128 splitK3 general", "128x128 splitK3 general")}),
    # (a padded cout takes no tail split forward: its finish kernel would sum workspace lanes no tile writes)
    Case("trunk workspace, padded cout", (4, 128, 128, 64, 130, 1), T, paths={
        FP32: ("128x128 plain general", "128x64 tail17x8 fast"), BF16: ("128x128 plain general", "128x64 plain general")}),
]
PARAMS = [pytest.param(c, id=c.name) for c in CASES]

# every path the issue lists, per precision: (tile, kind class, loop) -> must be named by a row, forward or data gradient
_FP32_TILES = ("128x32 BK16", "128x32", "128x96", "64x64", "128x64", "64x128", "128x128")
_BF16_TILES = ("128x32", "64x64", "128x64", "128x96", "64x128", "128x128")
REQUIRED = {
    FP32: [t + " plain " + lp for t in _FP32_TILES for lp in ("fast", "general")] +
          ["128x128 tail fast", "128x128 splitK fast", "64x128 plain " + FLGE],
    BF16: [t + " plain general" for t in _BF16_TILES] + ["128x128 splitK general"],
}


def _kind_class(path):
    tile, rest = path.split(" plain ") if " plain " in path else (None, None)
    if tile is not None:
        return path
    for k in ("tail", "splitK"):
        if " %s" % k in path:
            head, tail = path.split(" " + k)
            return "%s %s %s" % (head, k, tail.split(" ", 1)[1])
    raise AssertionError(path)


@pytest.mark.parametrize("case", PARAMS)
def test_mirror_names_the_path(case):
    """Host only: each shape reaches the path its row names, under the mirrored planner."""
    for prec in (FP32, BF16):
        assert (case.path(prec, FWD), case.path(prec, DGRAD)) == case.paths[prec], prec


def test_table_covers_every_path():
    """Host only: every tile of launch_conv_tile / conv_bf16_launch in plain mode, the fast and the general loop of each
    fp32 tile, split-K and tail split (also over several column tiles), full and partial last row / column tiles, a
    CoordConv on a wide tile, both sides of few_blocks, split_96 and the split-K limits, a multiple of 256 tiles."""
    for prec in (FP32, BF16):
        reached = {_kind_class(p) for c in CASES for p in c.paths[prec]}
        missing = [r for r in REQUIRED[prec] if r not in reached]
        assert not missing, (prec, missing)
    by = {c.name: c for c in CASES}
    # several column tiles: plain, tail and split-K
    assert by["two column tiles"].plan(FP32, FWD).tiles_n == 2 and by["two column tiles"].plan(BF16, FWD).tiles_n == 2
    p = by["trunk 256ch tail, two column tiles"].plan(FP32, FWD)
    assert p.tail and p.tiles_n == 2 and p.tail[0] % 2 == 0
    assert by["trunk split-K"].plan(FP32, DGRAD).tiles_n == 2 and by["trunk split-K"].plan(BF16, DGRAD).tiles_n == 2
    # last row tile: full (rows a multiple of the tile height) and partial; last column tile partial
    assert by["64ch 512 full tiles"].rows_in % 128 == 0 and by["64ch few_blocks"].rows_in % 64 != 0
    for prec in (FP32, BF16):
        p = by["partial column tile, padded cout"].plan(prec, FWD)
        assert p.n_valid % p.tile[1] != 0 and p.tiles_n == 2
    # CoordConv (act_ch < cin) on tiles wider than 32 columns
    assert by["coord 96+2 -> 96"].act_arg < by["coord 96+2 -> 96"].cin_p
    # both sides of the policy switches
    assert few_blocks(by["64ch few_blocks"].rows_in, 1) and not few_blocks(by["64ch 512 full tiles"].rows_in, 1)
    assert split_96(by["96ch below split_96"].rows_in) and not split_96(by["96ch above split_96"].rows_in)
    lo, mid, hi = by["trunk split-K"], by["trunk between the split-K limits"], by["trunk 128ch tail"]
    assert conv_splits(FP32, lo.rows_out, 256, 128, 128) > 1 and conv_splits(FP32, mid.rows_out, 128, 128, 128) == 1
    assert conv_splits(BF16, mid.rows_out, 128, 128, 128) > 1 and conv_splits(BF16, hi.rows_out, 128, 128, 128) == 1
    # a tile count that is a multiple of 256 takes no tail even with a workspace; one more row tile does
    p = by["trunk 512 tiles: no tail"].plan(FP32, FWD)
    assert p.tiles_m * p.tiles_n == 512 and p.tail is None and p.ws_floats == 0
    assert by["trunk 128ch tail"].plan(FP32, FWD).tail[:2] == (17, 8)


def _query(lib, prec, mode, what):
    return getattr(lib, "vlg_conv3x3_%s%s_%s" % (mode, "" if prec == FP32 else "_bf16", what))


def _assert_queries(lib, prec, rows_in, rows_out, cin_p, cout, cout_p):
    """Every host query of the library against the mirror for one shape."""
    key = (prec, rows_in, rows_out, cin_p, cout, cout_p)
    # one slope partial per block of the no-workspace plan: with the row count that fixes bm x bn (bn follows from n)
    assert _query(lib, prec, DGRAD, "slabs")(rows_in, cin_p) == Plan(prec, DGRAD, rows_in, cin_p, cout, cout_p, da_slab=True).slopes, key
    f = Plan(prec, FWD, rows_out, cin_p, cout, cout_p, ws=True)
    assert _query(lib, prec, FWD, "splits")(rows_out, cin_p, cout, cout_p) == f.splits, key
    # (a tail plan: splits * (rows - row0) * ldc, which fixes row0 and splits and so the 128-row tile behind them)
    assert _query(lib, prec, FWD, "workspace")(rows_out, cin_p, cout, cout_p) == f.ws_floats, key
    d = Plan(prec, DGRAD, rows_in, cin_p, cout, cout_p, ws=True)
    assert _query(lib, prec, DGRAD, "splits")(rows_in, cin_p, cout_p) == d.splits, key
    assert _query(lib, prec, DGRAD, "workspace")(rows_in, cin_p, cout_p) == d.ws_floats, key
    assert _query(lib, prec, WGRAD, "slabs")(rows_out, cin_p, cout_p) == wgrad_ranges(prec, rows_out, cin_p, cout_p)[0], key
    # The forward tile WITHOUT a workspace is conv_tile(rows, cout_p, cout): for cout == cout_p that is the data-gradient
    # tile of the same (rows, n), pinned by the slabs query above at n = cout_p.  Not pinned by any query: the column-tile
    # count of a padded cout (cout < cout_p, where n_valid differs from n_cols), and the tile of a launch WITH a workspace
    # when no tail results (conv_tile's kc > 0 branch falls through to the same few_blocks rule).
    if cout == cout_p:
        assert Plan(prec, FWD, rows_out, cin_p, cout, cout_p).slopes == _query(lib, prec, DGRAD, "slabs")(rows_out, cout_p), key


def test_mirror_matches_the_library_queries():
    """Host only (no launch): slope-partial counts, split counts, workspace sizes and weight-gradient ranges of the mirror
    are the library's for every table row and over sweeps of rows that cross each threshold of the planner."""
    from vlg import hip
    lib = hip.load()
    for c in CASES:
        for prec in (FP32, BF16):
            _assert_queries(lib, prec, c.rows_in, c.rows_out, c.cin_p, c.shape[4], c.cout_p)
    # row tiles around: split-K limits (200 fp32, 256 bf16; halved for two column tiles), few_blocks (b128 < 384 and the
    # cu_units steps at multiples of 256 blocks of either height), split_96 (400), bf16's 512 tiles, tail remainders
    marks = (1, 2, 64, 100, 127, 128, 199, 200, 201, 255, 256, 257, 264, 265, 383, 384, 385, 399, 400, 401, 511, 512, 513, 528, 529,
             640, 767, 768, 769, 1023, 1024, 1025, 1057, 1280, 1281, 2048, 2049, 2113)
    rows_sweep = sorted({128 * m + d for m in marks for d in (-127, -64, -1, 0, 1, 64)} | {c.rows_in for c in CASES} - {0})
    rows_sweep = [r for r in rows_sweep if r > 0]
    n = 0
    for rows in rows_sweep:
        for cin_p in (32, 64, 96, 128, 256, 512):
            for cout, cout_p in ((32, 32), (64, 64), (96, 96), (128, 128), (130, 160), (160, 160), (256, 256), (300, 320), (512, 512), (20, 32)):
                for prec in (FP32, BF16):
                    _assert_queries(lib, prec, rows, rows, cin_p, cout, cout_p)
                    n += 1
    assert n > 10000


# ------------------------------------------------------------------------------------------------ GPU cases
def _line(case, prec, what, err, bar):
    print("CONVERR %-38s %s %-8s %.3e (bar %.0e)" % (case.name, prec, what, err, bar))


def _rel32(case, what, got, want, tol=TOL):
    """fp32: max |err| against fp64 within tol of the tensor's scale; a NaN (an element never written) fails."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), "%s: an element is unwritten or not finite" % what
    err = float((got - want).abs().max()) / max(float(want.abs().max()), 1e-12)
    _line(case, FP32, what, err, tol)
    assert err <= tol, "%s: %.3e of scale (bar %.0e)" % (what, err, tol)


def _owned_and_spare(what, buf, owned):
    """A NaN-sentinel vector: the first `owned` floats were all written (finite), everything behind them is untouched."""
    assert bool(torch.isfinite(buf[:owned]).all()), what + ": a float the plan owns was not written"
    assert bool(torch.isnan(buf[owned:]).all()), what + ": written past the floats the plan owns"


def _run_case(dev, prec, case):
    from vlg import hip
    from vlg.hip import CEPI_ACCUM, CEPI_DPRELU, CEPI_RESID
    lib = hip.load()
    sfx = "" if prec == FP32 else "_bf16"
    b, H, W, cin, cout, stride = case.shape
    trunk, slope = case.trunk, case.slope
    act = cin if case.act_ch is None else case.act_ch
    g = torch.Generator().manual_seed(1000 * cin + 10 * cout + stride + H)
    h = _Harness(dev, b, H, W, cin, cout, stride)
    x = _away_from_kink((b, cin, H, W), g)
    w = (torch.rand(cout, cin, 3, 3, generator=g) * 2 - 1) / (cin * 9) ** 0.5
    bias = (torch.rand(cout, generator=g) * 2 - 1) * 0.1
    Ho, Wo = H // stride, W // stride
    r = torch.randn(b, cout, Ho, Wo, generator=g)
    rs = torch.randn(b, cout, Ho, Wo, generator=g) if case.resid else None
    prior = torch.randn(b, cin, H, W, generator=g) if trunk else None
    add = prior.double() if trunk else 0
    if prec == FP32:
        y_w, dx_w, dw_w, db_w, da_w, da_scale = _reference(x, w, bias, slope, act, stride, rs, r)
    else:
        want = _ref(x, w, bias, slope, act, stride, rs, r, True)
        plain = _ref(x, w, bias, slope, act, stride, rs, r, False)

    def compare(what, got, i32, want32, i16, extra=0):
        if prec == FP32:
            _rel32(case, what, got, want32 + extra)
        else:
            _check(what, got, want[i16] + extra, plain[i16] + extra)

    # the plan the mirror names is the plan the library reports for this call
    pf, pd = case.plan(prec, FWD), case.plan(prec, DGRAD)
    S = h.S
    h.put(x, h.x, cin, h.gi)
    h.put(r, h.dy, cout, h.go)
    if case.resid:
        h.put(rs, h.res, cout, h.go)
    wdev = h.pack_weight(w)
    bdev = torch.zeros(h.cout_p, device=dev)
    bdev[:cout] = bias.to(dev)
    sl = torch.tensor([slope, 0, 0, 0], dtype=torch.float32, device=dev)
    rowtab = h.gi.down_rowtab.data_ptr() if stride == 2 else 0
    taps = h.gi.down_taptabs.data_ptr() if stride == 2 else 0
    fepi = CEPI_RESID if case.resid else 0

    # ---- forward into a NaN-sentinel output (trunk: through a NaN-sentinel workspace)
    need = _query(lib, prec, FWD, "workspace")(h.go.rows, h.cin_p, cout, h.cout_p) if trunk else 0
    assert need == pf.ws_floats and (not trunk or _query(lib, prec, FWD, "splits")(h.go.rows, h.cin_p, cout, h.cout_p) == pf.splits)
    ws = torch.full((need + SPARE,), NAN, device=dev) if trunk else None

    def forward(cap):
        h.y.buf.fill_(NAN)
        return getattr(lib, "vlg_conv3x3_fwd" + sfx)(
            h.x.ptr, wdev.data_ptr(), bdev.data_ptr(), h.y.ptr, h.res.ptr if case.resid else 0, h.go.mask.data_ptr(),
            sl.data_ptr(), rowtab, h.go.rows, h.cin_p, cout, h.cout_p, h.gi.wp, case.act_arg, fepi, hip.ptr(ws), cap, S)

    assert forward(need + SPARE if trunk else 0) == 0
    torch.cuda.synchronize()
    _sentinel_checks("forward", h, h.y, h.go, cout, True)
    compare("forward", h.get(h.y, cout, h.go), 0, y_w if prec == FP32 else None, 0)
    if trunk:
        _owned_and_spare("forward workspace", ws, need)
        if pf.splits > 1:                                      # one float short: refused on the host, before any launch
            assert forward(need - 1) == 1001
        elif pf.tail:                                          # one float short: one block per tile, same result
            assert case.plan(prec, FWD, ws_cap=need - 1).tail is None
            ws.fill_(NAN)
            assert forward(need - 1) == 0
            torch.cuda.synchronize()
            assert bool(torch.isnan(ws).all()), "the fall-back launch used the workspace"
            _sentinel_checks("forward, short workspace", h, h.y, h.go, cout, True)
            compare("fwd-short", h.get(h.y, cout, h.go), 0, y_w if prec == FP32 else None, 0)

    # ---- data gradient.  gridnet: PReLU', slope partials, dx a NaN sentinel; trunk: ReLU', workspace, accumulate
    n_da = _query(lib, prec, DGRAD, "slabs")(h.gi.rows, h.cin_p)
    assert n_da == Plan(prec, DGRAD, h.gi.rows, h.cin_p, cout, h.cout_p, da_slab=True).slopes
    da_part = torch.full((n_da + SPARE,), NAN, device=dev)
    dneed = _query(lib, prec, DGRAD, "workspace")(h.gi.rows, h.cin_p, h.cout_p) if trunk else 0
    assert dneed == pd.ws_floats and (not trunk or _query(lib, prec, DGRAD, "splits")(h.gi.rows, h.cin_p, h.cout_p) == pd.splits)
    dws = torch.full((dneed + SPARE,), NAN, device=dev) if trunk else None
    if trunk:
        h.put(prior, h.dx, cin, h.gi)
    else:
        h.dx.buf.fill_(NAN)

    def dgrad(cap):
        return getattr(lib, "vlg_conv3x3_dgrad" + sfx)(
            h.dy.ptr, wdev.data_ptr(), h.dx.ptr, h.x.ptr, h.gi.mask.data_ptr(), sl.data_ptr(), 0 if trunk else da_part.data_ptr(),
            taps, h.gi.rows if stride == 2 else 0, h.gi.rows, h.cin_p, h.cout_p, h.gi.wp, case.act_arg,
            CEPI_DPRELU | (CEPI_ACCUM if trunk else 0), hip.ptr(dws), cap, n_da, S)

    if trunk and pd.splits > 1:
        assert dgrad(dneed - 1) == 1001                        # (refused before any launch: dx still holds the prior)
    assert dgrad(dneed + SPARE if trunk else 0) == 0
    torch.cuda.synchronize()
    if trunk:
        _owned_and_spare("data-gradient workspace", dws, dneed)
        v = _padded_view(h, h.dx, h.gi)[0]                     # accumulated onto the prior: its zero halo stays zero
        for halo in (v[:, 0], v[:, -1], v[:, :, 0], v[:, :, -1]):
            assert float(halo.abs().max()) == 0.0, "dx: halo rows are not zero"
    else:
        _sentinel_checks("dx", h, h.dx, h.gi, cin, False)
        _owned_and_spare("slope partials", da_part, n_da)
        if cin < h.cin_p:                                      # padding lanes of dx: owned by the kernel, exactly zero
            v = h.dx.buf[h.gi.guard * h.cin_p:(h.gi.guard + h.gi.rows) * h.cin_p].view(-1, h.cin_p)
            assert float(v[:, cin:].abs().max()) == 0.0, "dx: padding lanes are not zero"
    compare("dx", h.get(h.dx, cin, h.gi), 1, dx_w if prec == FP32 else None, 1, add)
    if not trunk:
        da = torch.zeros(4, device=dev)
        hip.call("vlg_sum_partials", da_part.data_ptr(), n_da, da.data_ptr(), 0, S)
        if prec == FP32:                                       # judged against its own term scale (test_hip_conv_ops)
            e = abs(float(da[0]) - float(da_w)) / max(abs(float(da_w)), 1e-2 * da_scale)
            _line(case, prec, "slope", e, TOL)
            assert e <= TOL, ("slope gradient", float(da[0]), float(da_w), da_scale)
        else:
            e = abs(float(da[0]) - want[2]) / max(want[3], 1e-12)
            _line(case, prec, "slope", e, 1e-5)
            assert e <= 1e-5, ("slope gradient", float(da[0]), want[2], want[3])

    # ---- weight + bias gradient into NaN-sentinel slabs with a tail behind each slab and a spare slab
    n_slabs = _query(lib, prec, WGRAD, "slabs")(h.go.rows, h.cin_p, h.cout_p)
    assert n_slabs == wgrad_ranges(prec, h.go.rows, h.cin_p, h.cout_p)[0]
    need_w = h.cout_p * 9 * h.cin_p + h.cout_p
    stride_f = need_w + 4
    slabs = torch.full(((n_slabs + 1) * stride_f,), NAN, device=dev)
    hip.call("vlg_conv3x3_wgrad" + sfx, h.dy.ptr, h.x.ptr, slabs.data_ptr(), stride_f, n_slabs * stride_f, rowtab, sl.data_ptr(),
             h.go.rows, h.cin_p, h.cout_p, h.gi.wp, case.act_arg, S)
    torch.cuda.synchronize()
    sv = slabs.view(n_slabs + 1, stride_f)
    assert bool(torch.isfinite(sv[:n_slabs, :need_w]).all()), "wgrad: a slab element is unwritten or not finite"
    assert bool(torch.isnan(sv[:n_slabs, need_w:]).all()) and bool(torch.isnan(sv[n_slabs]).all()), "wgrad wrote past its slabs"
    gw = torch.empty(stride_f, device=dev)
    hip.call("vlg_reduce_slabs", slabs.data_ptr(), stride_f, n_slabs, gw.data_ptr(), stride_f, S)
    torch.cuda.synchronize()
    compare("dW", h.unpack_weight(gw), 2, dw_w if prec == FP32 else None, 4)
    db = gw.cpu()[h.cout_p * 9 * h.cin_p:][:cout]
    if prec == FP32:
        _rel32(case, "db", db, db_w)
    else:                                                      # (from the fp32 dOut: no rounding to discriminate)
        e = float((db.double() - want[5]).abs().max()) / max(float(want[5].abs().max()), 1e-12)
        _line(case, prec, "db", e, 1e-5)
        assert e <= 1e-5, ("db", e)
    full = gw.cpu()[:h.cout_p * 9 * h.cin_p].view(h.cout_p, 9, h.cin_p)
    assert float(full[cout:].abs().max() if cout < h.cout_p else 0.0) == 0.0, "padded output-channel lanes of dW"
    if case.act_ch is None:
        assert float(full[:, :, cin:].abs().max() if cin < h.cin_p else 0.0) == 0.0, "padded input-channel lanes of dW"


@pytest.mark.gpu
@pytest.mark.parametrize("case", PARAMS)
def test_conv_paths_fp32(dev, case):
    _run_case(dev, FP32, case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", PARAMS)
def test_conv_paths_bf16(dev, case):
    _run_case(dev, BF16, case)


# ------------------------------------------------------------------------------------------------ the 2 GiB switch
def _two_gib_side(dev, b, loop):
    """128 -> 32 channels forward and 32 -> 128 channels data gradient at b x 256 x 256: the gathered operand (x, or dOut
    with lda = cout_p = 128) is just under (b = 63) or just over (b = 64) the 1 << 31 bytes a buffer descriptor of the fast
    loop can span.  The 128-channel tensor is filled on the device image by image; the fp64 reference covers the first and
    the last image (a 3x3 convolution is local to an image, the last one holds the largest offsets)."""
    import torch.nn.functional as F
    from vlg import hip
    from vlg.gridnet import _Geo, _PT
    H = W = 256
    CB, CS = 128, 32
    geo = _Geo(b, H, W, dev)
    # the mirror: which side of conv.hip:118-121 this batch is on, forward and data gradient
    pf = Plan(FP32, FWD, geo.rows, CB, CS, CS)
    pd = Plan(FP32, DGRAD, geo.rows, CS, CB, CB)
    assert pf.tile_name == pd.tile_name == "128x32 BK16"
    assert conv_loop(FP32, FWD, pf, CB, geo.wp, False, CB, CB) == loop
    assert conv_loop(FP32, DGRAD, pd, CB, geo.wp, False, CS, CS) == loop
    a_bytes = (geo.rows + 2 * (geo.wp + 1) + 128) * CB * 4
    assert (a_bytes < LIMIT) == (loop == "fast")
    S = torch.cuda.current_stream().cuda_stream
    big, small, xin = _PT(geo, CB, dev), _PT(geo, CS, dev), _PT(geo, CS, dev)
    img = (H + 2) * (W + 2)
    ends = (0, b - 1)

    def fill(pt, C, seed):
        keep = {}
        for i in range(b):
            g = torch.Generator(device=dev).manual_seed(seed + i)
            v = torch.randn(1, C, H, W, device=dev, generator=g)
            v = torch.where(v >= 0, v + 1e-3, v - 1e-3)        # away from the PReLU kink
            hip.call("vlg_nchw_to_padded", v.data_ptr(), pt.ptr + 4 * i * img * pt.cp, 1, C, H, W, pt.cp, -1, S)
            if i in ends:
                keep[i] = v.cpu()
        return keep

    def image(pt, C, i):
        out = torch.empty(1, C, H, W, device=dev)
        hip.call("vlg_padded_to_nchw", pt.ptr + 4 * i * img * pt.cp, out.data_ptr(), 1, C, H, W, pt.cp, S)
        return out.cpu()

    def sentinels(what, pt, C):
        n0, n1 = geo.guard * pt.cp, (geo.guard + geo.rows) * pt.cp
        assert bool(torch.isnan(pt.buf[:n0]).all()) and bool(torch.isnan(pt.buf[n1:]).all()), what + ": guard rows were written"
        v = pt.buf[n0:n1].view(b, H + 2, W + 2, pt.cp)
        for i in ends:
            assert bool(torch.isfinite(v[i, 1:-1, 1:-1, :C]).all()), what + ": an interior element is unwritten"
            for halo in (v[i, 0], v[i, -1], v[i, :, 0], v[i, :, -1]):
                assert float(halo.abs().max()) == 0.0, what + ": halo rows are not zero"

    case = Case("2 GiB b=%d" % b, (b, H, W, CB, CS, 1), G, {})
    gcpu = torch.Generator().manual_seed(b)
    slope = 0.25
    sl = torch.tensor([slope, 0, 0, 0], device=dev)
    xb = fill(big, CB, 1000)
    # ---- forward 128 -> 32: PReLU on load, bias, halo mask
    w1 = (torch.rand(CS, CB, 3, 3, generator=gcpu) * 2 - 1) / (CB * 9) ** 0.5
    bias = (torch.rand(CS, generator=gcpu) * 2 - 1) * 0.1
    w1d = torch.zeros(CS, 9, CB)
    w1d[:] = w1.permute(0, 2, 3, 1).reshape(CS, 9, CB)
    w1d, bd = w1d.flatten().to(dev), bias.to(dev)
    small.buf.fill_(NAN)
    hip.call("vlg_conv3x3_fwd", big.ptr, w1d.data_ptr(), bd.data_ptr(), small.ptr, 0, geo.mask.data_ptr(), sl.data_ptr(), 0,
             geo.rows, CB, CS, CS, geo.wp, CB, 0, 0, 0, S)
    torch.cuda.synchronize()
    sentinels("forward", small, CS)
    for i in ends:
        y_w = F.conv2d(F.prelu(xb[i].double(), torch.tensor([slope], dtype=torch.float64)), w1.double(), bias.double(), padding=1)
        _rel32(case, "fwd img%d" % i, image(small, CS, i), y_w)
    # ---- data gradient of a 32 -> 128 convolution: dOut is the 128-channel tensor, PReLU' on the 32-channel input
    w2 = (torch.rand(CB, CS, 3, 3, generator=gcpu) * 2 - 1) / (CS * 9) ** 0.5
    w2d = w2.permute(0, 2, 3, 1).reshape(CB, 9, CS).contiguous().flatten().to(dev)
    xs = fill(xin, CS, 5000)
    small.buf.fill_(NAN)
    hip.call("vlg_conv3x3_dgrad", big.ptr, w2d.data_ptr(), small.ptr, xin.ptr, geo.mask.data_ptr(), sl.data_ptr(), 0, 0, 0,
             geo.rows, CS, CB, geo.wp, CS, 8, 0, 0, 0, S)
    torch.cuda.synchronize()
    sentinels("dx", small, CS)
    for i in ends:
        dxa = torch.nn.grad.conv2d_input((1, CS, H, W), w2.double(), xb[i].double(), padding=1)
        dx_w = torch.where(xs[i].double() > 0, dxa, dxa * float(torch.tensor(slope, dtype=torch.float32)))
        _rel32(case, "dx img%d" % i, image(small, CS, i), dx_w)


@pytest.mark.gpu
def test_two_gib_switch(dev):
    """One fp32 case on each side of the 1 << 31 byte limit (conv.hip:118-121): under it the launch takes the fast loop
    (32-bit offsets into buffer descriptors), over it the general one (64-bit pointers) - silently, so both are compared
    with fp64 on the first and the last image."""
    for b, loop in ((63, "fast"), (64, "general")):
        torch.cuda.empty_cache()
        try:
            _two_gib_side(dev, b, loop)
        finally:
            torch.cuda.empty_cache()                           # ~3.9 GiB per side go back before the next test
