"""Where the partial sums ("slabs") of a backward's reductions go, and when they are summed into the flat gradient.

A producer (a weight gradient, a layer-norm or embedding backward) writes `n_slabs` partial results `stride` floats apart;
their sum is `dst_len` floats of the gradient.  A BUCKET is the set of producers whose gradients are complete together (a
layer, the head, the embeddings).  Grouped (the default): a bucket's producers write side by side into one arena and ONE
table-driven launch (vlg_reduce_slabs_table) sums them all when the bucket is closed - or, with `ride`, the closed bucket
waits for rider blocks of the engine's next paired launch, whose own producers write the OTHER arena.  Not grouped: one arena.
"""
from __future__ import annotations

from typing import Callable, Dict, Optional, Sequence

import torch

from .hip import call, ptr


class SlabBuckets:
    def __init__(self, sizes: Sequence[Sequence[int]], device, grouped: bool, ride: bool, launch: Optional[Callable] = None):
        """sizes: for every kind of bucket, the floats each of its producers needs.  launch: hip.call unless given."""
        self.grouped, self.ride, self.device = bool(grouped), bool(ride and grouped), device
        self.launch = launch if launch is not None else call
        floats = max(sum((v + 3) // 4 * 4 for v in b) for b in sizes) if grouped else max(v for b in sizes for v in b)
        self.arenas = [torch.empty(floats, dtype=torch.float32, device=device) for _ in range(2 if grouped else 1)]
        self.tables: Dict[tuple, torch.Tensor] = {}      # device tables by their rows: built once per batch geometry
        self.reset()

    def reset(self) -> None:
        """Forget open rows and a waiting bucket: every step's tables - and a captured hipGraph - see the same pointers."""
        self.sel, self.off, self.rows, self.waiting = 0, 0, [], None

    def reserve(self, need: int) -> torch.Tensor:
        """what the next producer writes: the open bucket's next free `need` floats, or (not grouped) the whole arena"""
        arena = self.arenas[self.sel]
        if not self.grouped:
            return arena
        off = self.off
        if off + need > arena.numel():
            raise RuntimeError("partial-sum arena of %d floats is too small for %d more" % (arena.numel(), need))
        self.off = off + (need + 3) // 4 * 4
        return arena[off:off + need]

    def add(self, slabs: torch.Tensor, stride: int, n_slabs: int, dst: int, dst_len: int, stream: int) -> None:
        """`slabs` (from reserve) now holds n_slabs partial sums, written on `stream`: a table row, or (not grouped) summed there"""
        if self.grouped:
            self.rows.append((slabs.data_ptr(), stride, n_slabs, dst, dst_len))
        else:
            self.launch("vlg_reduce_slabs", ptr(slabs), stride, n_slabs, dst, dst_len, stream)

    def _table(self, rows: tuple) -> torch.Tensor:
        if rows not in self.tables:
            self.tables[rows] = torch.tensor([v for row in rows for v in row], dtype=torch.int64, device=self.device)
        return self.tables[rows]

    def close(self, stream: int, defer: bool = False, then: Optional[Callable] = None) -> None:
        """The open bucket is complete: ONE launch on `stream` sums its rows, then `then` runs - or, with defer and `ride`, it waits
        for take_rider (the next producers write the other arena).  A bucket still waiting then travels in the same table, first."""
        rows, self.rows, self.off = tuple(self.rows), [], 0
        if defer and self.ride and rows and self.waiting is None:
            self.waiting = (rows, then)
            self.sel ^= 1
            return
        (first, first_then), self.waiting = self.waiting or ((), None), None
        if first + rows:
            self.launch("vlg_reduce_slabs_table", ptr(self._table(first + rows)), len(first + rows), 128, stream)
        for fn in (first_then, then):
            if fn is not None:
                fn()

    def take_rider(self) -> tuple:
        """(table pointer, rows, callback to run behind the launch that sums them, bytes moved) of the waiting bucket"""
        if self.waiting is None:
            return 0, 0, None, 0.0
        (rows, then), self.waiting = self.waiting, None
        nbytes = 4.0 * sum((n_slabs + 1) * length for (_, _, n_slabs, _, length) in rows)      # slabs read + sums written
        return ptr(self._table(rows)), len(rows), then, nbytes
