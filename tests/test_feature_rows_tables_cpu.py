"""feature_cache.gather_tables without a GPU: the address tables of the feature cache's one gather launch, over one SlotTable and over a
table with its mirror table, against tables written out by hand.  The addresses are made up: slot s of table k lies at
1_000_000 * (k + 1) + s * STRIDE, computed row j of orientation o at 50_000_000 * (o + 1) + j * RB.  A wrong `keep` address would
overwrite a slot and a wrong `ref` address would switch the box check off, so every entry is compared, and with it the counters and the
slot order of every table."""
import pytest

RB, BB = 64, 32                                                  # a row and its boxes; a slot holds both
STRIDE = RB + BB
PLAIN, MIRRORED = 0, 1


def slot(k, s):
    return 1_000_000 * (k + 1) + s * STRIDE


def row(o, j):
    return 50_000_000 * (o + 1) + j * RB


class _Tables:
    """SlotTables of these capacities (in slots, slabs of two), the fake addresses, and the slabs asked for"""

    def __init__(self, *slots):
        from din_amd.frame_cache import SlotTable
        self.tables = [SlotTable(STRIDE, n * STRIDE, chunk_frames=2) for n in slots]
        assert [t.max_slots for t in self.tables] == list(slots)
        self.grown = [[] for _ in slots]

    def hold(self, k, *fids):
        """table k holds these frames before the call (an earlier batch, a file)"""
        for f in fids:
            assert self.tables[k].insert(f) >= 0
        return self

    def build(self, ids, orient, miss_pos):
        from din_amd.feature_cache import gather_tables
        n = len(self.tables)
        return gather_tables(self.tables, [lambda s, k=k: slot(k, s) for k in range(n)], [lambda m, g=g: (g.append(m), True)[1] for g in self.grown],
                             ids, orient, miss_pos, [(row(o, 0), RB) for o in range(n)], RB)

    def state(self):
        """per table: (hits, misses, inserted, the frames in slot order)"""
        return [(t.hits, t.misses, t.inserted, list(t.slot_of)) for t in self.tables]


def test_the_builder_is_host_arithmetic():
    from din_amd.feature_cache import gather_tables
    assert not {"torch", "np", "data_ptr", "is_cuda"} & set(gather_tables.__code__.co_names)


# ---- one table ---------------------------------------------------------------------------------------------------------------------------
def test_an_all_new_batch_fills_the_slots_in_batch_order_and_grows_a_slab_at_the_third_frame():
    w = _Tables(3)
    src, keep, ref, extra, reported = w.build([10, 11, 12], [PLAIN] * 3, [0, 1, 2])
    assert src == [row(0, 0), row(0, 1), row(0, 2)]
    assert keep == [slot(0, 0), slot(0, 1), slot(0, 2)] and ref == [0, 0, 0]
    assert extra == [] and reported == [10, 11, 12]
    assert w.state() == [(0, 3, 3, [10, 11, 12])] and w.grown == [[2, 1]]


def test_a_frame_at_two_rows_is_stored_once_and_served_twice_from_its_first_copy():
    w = _Tables(3)
    src, keep, ref, extra, reported = w.build([10, 11, 10], [PLAIN] * 3, [0, 1, 2])      # both rows of frame 10 were decoded
    assert src == [row(0, 0), row(0, 1), row(0, 0)]
    assert keep == [slot(0, 0), slot(0, 1), 0] and ref == [0, 0, 0]
    assert extra == [] and reported == [10, 11]
    assert w.state() == [(0, 2, 2, [10, 11])]                    # the second row of frame 10 is not looked up


def test_a_mixed_batch_in_shuffled_order():
    """resident rows come from their slots with the stored boxes' address, computed rows from their copy; the decoded copies arrive in
    another order than their rows (copy 0 is row 2's), and the frames still go in in the order of their first row in the batch"""
    w = _Tables(5).hold(0, 20, 21)
    src, keep, ref, extra, reported = w.build([31, 21, 30, 20], [PLAIN] * 4, [2, 0])
    assert src == [row(0, 1), slot(0, 1), row(0, 0), slot(0, 0)]
    assert keep == [slot(0, 2), 0, slot(0, 3), 0]
    assert ref == [0, slot(0, 1) + RB, 0, slot(0, 0) + RB]
    assert extra == [] and reported == [31, 30]
    assert w.state() == [(2, 2, 4, [20, 21, 31, 30])] and w.grown == [[2]]


def test_a_full_table_serves_computed_rows_without_keeping_them():
    w = _Tables(3).hold(0, 20, 21, 22)
    src, keep, ref, extra, reported = w.build([40, 41, 40], [PLAIN] * 3, [0, 1, 2])
    assert src == [row(0, 0), row(0, 1), row(0, 0)] and keep == [0, 0, 0] and ref == [0, 0, 0]
    assert extra == [] and reported == []
    assert w.state() == [(0, 3, 3, [20, 21, 22])] and w.grown == [[]]        # one miss per row: nothing was inserted


def test_a_resident_batch_needs_no_computed_rows():
    w = _Tables(3).hold(0, 20, 21)
    src, keep, ref, extra, reported = w.build([21, 20, 21], [PLAIN] * 3, [])
    assert src == [slot(0, 1), slot(0, 0), slot(0, 1)] and keep == [0, 0, 0]
    assert ref == [slot(0, 1) + RB, slot(0, 0) + RB, slot(0, 1) + RB]
    assert extra == [] and reported == []
    assert w.state() == [(3, 0, 2, [20, 21])]


def test_a_frame_neither_resident_nor_computed_is_a_key_error():
    w = _Tables(3).hold(0, 20)
    with pytest.raises(KeyError) as e:
        w.build([20, 5], [PLAIN] * 2, [])
    assert e.value.args == ("frame 5 is neither resident nor among the computed rows of this batch",)
    assert w.state() == [(1, 1, 1, [20])]


# ---- a table and its mirror table --------------------------------------------------------------------------------------------------------
def test_a_plain_and_a_mirrored_clip_store_their_other_orientation_by_extra_rows():
    w = _Tables(4, 4)
    src, keep, ref, extra, reported = w.build([10, 11, 12, 13], [PLAIN, PLAIN, MIRRORED, MIRRORED], [0, 1, 2, 3])
    assert extra == [(PLAIN, 12, 2), (PLAIN, 13, 3), (MIRRORED, 10, 0), (MIRRORED, 11, 1)]
    assert src == [row(0, 0), row(0, 1), row(1, 2), row(1, 3)] + [row(0, 2), row(0, 3), row(1, 0), row(1, 1)]
    assert keep == [slot(0, 0), slot(0, 1), slot(1, 2), slot(1, 3)] + [slot(0, 2), slot(0, 3), slot(1, 0), slot(1, 1)]
    assert ref == [0] * 8 and reported == [10, 11, 12, 13]
    assert w.state() == [(0, 2, 4, [10, 11, 12, 13])] * 2 and w.grown == [[2, 2], [2, 2]]


def test_a_frame_asked_for_in_both_orientations_needs_no_extra_row():
    w = _Tables(3, 3)
    src, keep, ref, extra, reported = w.build([10, 11, 10, 11], [PLAIN, PLAIN, MIRRORED, MIRRORED], [0, 1])
    assert src == [row(0, 0), row(0, 1), row(1, 0), row(1, 1)]
    assert keep == [slot(0, 0), slot(0, 1), slot(1, 0), slot(1, 1)] and ref == [0] * 4
    assert extra == [] and reported == [10, 11]
    assert w.state() == [(0, 2, 2, [10, 11])] * 2


def test_three_and_two_slots_keep_two_pairs_and_serve_the_third_frame_from_its_computed_row():
    w = _Tables(3, 2)
    src, keep, ref, extra, reported = w.build([10, 11, 12], [PLAIN, MIRRORED, PLAIN], [0, 1, 2])
    assert extra == [(PLAIN, 11, 1), (MIRRORED, 10, 0)]
    assert src == [row(0, 0), row(1, 1), row(0, 2)] + [row(0, 1), row(1, 0)]
    assert keep == [slot(0, 0), slot(1, 1), 0] + [slot(0, 1), slot(1, 0)]
    assert ref == [0] * 5 and reported == [10, 11]
    assert w.state() == [(0, 2, 2, [10, 11]), (0, 1, 2, [10, 11])]
    assert w.grown == [[2, 1], [2]]                              # (the plain table had room for frame 12; the mirror table had none)


def test_a_frame_one_table_holds_already_goes_into_the_other_only():
    """as after a file was loaded for one orientation: the plain row is served from its slot and checked, the mirrored row of the
    decoded copy goes in by an extra row, and the frame is reported -- both tables hold it since this call"""
    w = _Tables(3, 3).hold(0, 10)
    src, keep, ref, extra, reported = w.build([10, 11], [PLAIN, MIRRORED], [0, 1])
    assert extra == [(PLAIN, 11, 1), (MIRRORED, 10, 0)]
    assert src == [slot(0, 0), row(1, 1)] + [row(0, 1), row(1, 0)]
    assert keep == [0, slot(1, 1)] + [slot(0, 1), slot(1, 0)]
    assert ref == [slot(0, 0) + RB, 0, 0, 0] and reported == [10, 11]
    assert w.state() == [(1, 0, 2, [10, 11]), (0, 1, 2, [10, 11])]


def test_a_batch_without_mirrored_rows_fills_the_mirror_table_by_extra_rows():
    w = _Tables(3, 3)
    src, keep, ref, extra, reported = w.build([10, 11], [PLAIN, PLAIN], [0, 1])
    assert extra == [(MIRRORED, 10, 0), (MIRRORED, 11, 1)]
    assert src == [row(0, 0), row(0, 1)] + [row(1, 0), row(1, 1)]
    assert keep == [slot(0, 0), slot(0, 1)] + [slot(1, 0), slot(1, 1)]
    assert ref == [0] * 4 and reported == [10, 11]
    assert w.state() == [(0, 2, 2, [10, 11]), (0, 0, 2, [10, 11])]


def test_the_key_error_of_two_tables_names_the_orientation():
    w = _Tables(3, 3).hold(0, 10)
    with pytest.raises(KeyError) as e:
        w.build([10, 10], [PLAIN, MIRRORED], [])
    assert e.value.args == ("frame 10 (mirrored) is neither resident nor among the computed rows of this batch",)
    assert w.state() == [(1, 0, 1, [10]), (0, 1, 0, [])]
