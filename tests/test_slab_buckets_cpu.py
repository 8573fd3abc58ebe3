"""CPU: the partial-sum bucket bookkeeping of the layout step's backward (vlg/slabs.py) with a recording launcher: what is
reserved, which table is launched when, and in what order the callbacks run."""
import pytest
import torch

from vlg.slabs import SlabBuckets

DST = 1 << 20          # "gradient buffer" address: the object only passes it on


class Recorder:
    def __init__(self):
        self.calls, self.events = [], []

    def __call__(self, name, *args):
        self.calls.append((name,) + args)
        self.events.append(name)

    def then(self, tag):
        return lambda: self.events.append(tag)


def buckets(sizes=((10, 7, 5),), ride=True):
    rec = Recorder()
    return SlabBuckets(sizes, "cpu", True, ride, launch=rec), rec


def fill(b, needs, dst0=0):
    """reserve + add one producer per entry of needs = (n_slabs, length); returns the rows a table should hold"""
    rows = []
    for i, (n_slabs, length) in enumerate(needs):
        s = b.reserve(n_slabs * length)
        b.add(s, length, n_slabs, DST + 4 * (dst0 + 100 * i), length, 0)
        rows.append((s.data_ptr(), length, n_slabs, DST + 4 * (dst0 + 100 * i), length))
    return rows


def table_of(b, call):
    name, table_ptr, n_rows, blocks_per_row, stream = call
    assert name == "vlg_reduce_slabs_table" and blocks_per_row == 128
    (table,) = [t for t in b.tables.values() if t.data_ptr() == table_ptr]
    assert table.dtype == torch.int64 and table.numel() == 5 * n_rows
    return [tuple(r) for r in table.view(n_rows, 5).tolist()], stream


def test_reserve_is_aligned_ordered_and_bounded():
    b, rec = buckets(sizes=((10, 7, 5), (3,)))          # arena: max(12 + 8 + 8, 4) = 28 floats
    assert [a.numel() for a in b.arenas] == [28, 28]
    base = b.arenas[0].data_ptr()
    got = [b.reserve(n) for n in (10, 7, 5)]
    assert [t.numel() for t in got] == [10, 7, 5]
    assert [(t.data_ptr() - base) // 4 for t in got] == [0, 12, 20]          # 4-float aligned, in order, no overlap
    with pytest.raises(RuntimeError, match="partial-sum arena of 28 floats is too small for 1 more"):
        b.reserve(1)
    b.reset()
    assert b.reserve(28).data_ptr() == base
    with pytest.raises(RuntimeError, match="too small"):
        b.reserve(1)
    assert rec.calls == []


def test_close_issues_one_table_in_insertion_order_then_calls_then():
    b, rec = buckets()
    rows = fill(b, [(2, 5), (1, 7), (3, 1)])
    b.close(77, then=rec.then("done"))
    assert rec.events == ["vlg_reduce_slabs_table", "done"] and len(rec.calls) == 1
    assert table_of(b, rec.calls[0]) == (rows, 77)
    b.close(77, then=rec.then("empty"))                       # nothing open: no launch, the callback still runs
    assert rec.events == ["vlg_reduce_slabs_table", "done", "empty"]
    assert b.reserve(4).data_ptr() == b.arenas[0].data_ptr()  # the arena is free again


def test_deferred_bucket_waits_for_its_rider():
    b, rec = buckets()
    rows = fill(b, [(2, 5), (1, 7)])
    b.close(77, defer=True, then=rec.then("first"))
    assert rec.calls == [] and rec.events == []
    assert b.reserve(4).data_ptr() == b.arenas[1].data_ptr()  # the next producers write the other arena
    table_ptr, n_rows, then, nbytes = b.take_rider()
    assert n_rows == 2 and nbytes == 4.0 * ((2 + 1) * 5 + (1 + 1) * 7)
    (table,) = b.tables.values()
    assert table.data_ptr() == table_ptr and [tuple(r) for r in table.view(2, 5).tolist()] == rows
    assert rec.events == []
    then()
    assert rec.events == ["first"] and rec.calls == []
    assert b.take_rider() == (0, 0, None, 0.0)


def test_without_ride_a_deferred_close_reduces_at_once():
    b, rec = buckets(ride=False)
    rows = fill(b, [(2, 5)])
    b.close(5, defer=True, then=rec.then("now"))
    assert rec.events == ["vlg_reduce_slabs_table", "now"] and table_of(b, rec.calls[0]) == (rows, 5)
    assert b.take_rider() == (0, 0, None, 0.0) and b.sel == 0


def test_second_deferred_close_flushes_the_waiting_bucket_first():
    b, rec = buckets()
    first = fill(b, [(2, 5), (1, 7)])
    b.close(9, defer=True, then=rec.then("first"))
    second = fill(b, [(3, 2)], dst0=1000)
    assert second[0][0] == b.arenas[1].data_ptr()
    b.close(9, defer=True, then=rec.then("second"))
    assert rec.events == ["vlg_reduce_slabs_table", "first", "second"] and len(rec.calls) == 1
    assert table_of(b, rec.calls[0]) == (first + second, 9)
    assert b.take_rider() == (0, 0, None, 0.0)


def test_reset_drops_open_rows_and_a_waiting_bucket_silently():
    b, rec = buckets()
    fill(b, [(2, 5)])
    b.close(9, defer=True, then=rec.then("waiting"))
    fill(b, [(1, 7)])
    b.reset()
    assert rec.events == [] and b.take_rider() == (0, 0, None, 0.0)
    assert b.reserve(4).data_ptr() == b.arenas[0].data_ptr()
    b.reset()
    b.close(9, then=rec.then("after"))
    assert rec.events == ["after"] and rec.calls == []


def test_identical_rows_reuse_the_cached_table():
    b, rec = buckets()
    for _ in range(2):
        b.reset()
        fill(b, [(2, 5), (1, 7)])
        b.close(3)
    assert len(b.tables) == 1 and len(rec.calls) == 2 and rec.calls[0] == rec.calls[1]
    b.reset()
    fill(b, [(2, 5), (1, 6)])
    b.close(3)
    assert len(b.tables) == 2 and rec.calls[2][1] != rec.calls[0][1]


def test_ungrouped_reduces_right_behind_each_producer():
    """the two-stream mode's form: one arena handed out whole, one vlg_reduce_slabs per producer on the producer's stream"""
    rec = Recorder()
    b = SlabBuckets(((10, 7), (30,)), "cpu", False, True, launch=rec)
    assert [a.numel() for a in b.arenas] == [30] and not b.ride
    for stream, (n_slabs, length) in ((11, (2, 5)), (12, (4, 7))):
        s = b.reserve(n_slabs * length)
        assert s.data_ptr() == b.arenas[0].data_ptr() and s.numel() == 30
        b.add(s, length, n_slabs, DST, length, stream)
        assert rec.calls[-1] == ("vlg_reduce_slabs", s.data_ptr(), length, n_slabs, DST, length, stream)
    b.close(11, defer=True, then=rec.then("done"))
    assert rec.events == ["vlg_reduce_slabs", "vlg_reduce_slabs", "done"] and b.take_rider() == (0, 0, None, 0.0) and not b.tables
