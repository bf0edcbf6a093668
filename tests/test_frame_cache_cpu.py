"""Frame cache, host side (no GPU): config defaults, datasets with and without frame ids over tests/golden/dataset_tree, the collate,
the slot bookkeeping, loader workers, and the C ABI of din_copy_rows_u8."""
import os
import pickle
import re

import numpy as np
import pytest
import torch
import torch.utils.data as tud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _volleyball(golden_dir, **kw):
    from din_amd import volleyball as V
    root = os.path.join(golden_dir, "dataset_tree", "volleyball")
    anns = V.volley_read_dataset(root, [1, 4])
    with open(os.path.join(root, "tracks_normalized.pkl"), "rb") as fh:
        tracks = pickle.load(fh)
    return V.VolleyballDataset(anns, tracks, V.volley_all_frames(anns), root, (64, 96), (2, 3), "dynamic_volleyball", num_boxes=12,
                               num_before=1, num_after=1, **kw)


def _collective(golden_dir, **kw):
    from din_amd import collective as Cc
    root = os.path.join(golden_dir, "dataset_tree", "collective")
    anns = Cc.collective_read_dataset(root, [1, 15])
    return Cc.CollectiveDataset(anns, Cc.collective_all_frames(anns), root, (64, 96), (2, 3), num_boxes=13, num_frames=3, **kw)


# ---- defaults: nothing changes ---------------------------------------------------------------------------------------------------------
def test_config_defaults_are_off():
    from din_amd.config import Config
    for name in ("volleyball", "collective"):
        cfg = Config(name)
        assert cfg.frame_cache_gb == 0 and cfg.num_workers == 0


def test_default_datasets_return_todays_tuples(golden_dir):
    z = np.load(os.path.join(golden_dir, "dataset_volleyball.npz"))
    ds = _volleyball(golden_dir)
    assert len(ds) == 3 and not hasattr(ds, "frame_table")
    for i in range(len(ds)):
        item = ds[i]
        assert len(item) == 4 and item[0].dtype == torch.uint8
        for got, key in zip(item, (f"images.{i}", f"boxes.vgg.{i}", f"actions.{i}", f"activities.{i}")):
            assert np.array_equal(got.numpy(), z[key]), key
    z = np.load(os.path.join(golden_dir, "dataset_collective.npz"))
    ds = _collective(golden_dir)
    assert len(ds) == 4 and not hasattr(ds, "frame_table")
    for i in range(len(ds)):
        item = ds[i]
        assert len(item) == 5 and item[0].dtype == torch.uint8
        for got, key in zip(item, (f"images.{i}", f"boxes.{i}", f"actions.{i}", f"activities.{i}", f"bboxes_num.{i}")):
            assert np.array_equal(got.numpy(), z[key]), key


def test_default_loaders_are_the_plain_ones(golden_dir):
    """build_loaders with both settings at 0: DataLoaders with num_workers = 0, the default collate and no cache, as the trainers built"""
    from din_amd import frame_cache as FC
    from din_amd.config import Config
    cfg = Config("volleyball")
    ds = _volleyball(golden_dir)
    for real_tree in (False, True):
        tr, va = FC.build_loaders(cfg, ds, ds, 2, None, "cpu", real_tree)
        for ld in (tr, va):
            assert type(ld) is tud.DataLoader and ld.num_workers == 0 and ld.collate_fn is tud.default_collate and ld.timeout == 0
        assert tr.batch_size == 2 and va.batch_size == cfg.test_batch_size
        assert isinstance(tr.sampler, tud.RandomSampler) and isinstance(va.sampler, tud.SequentialSampler)
    assert not FC.wants_frame_ids(cfg)


def test_workers_and_timeout_reach_both_loaders_only_on_the_real_tree(golden_dir):
    from din_amd import frame_cache as FC
    from din_amd.config import Config
    cfg = Config("volleyball")
    cfg.num_workers = 3
    ds = _volleyball(golden_dir)
    for ld in FC.build_loaders(cfg, ds, ds, 2, None, "cpu", True):
        assert ld.num_workers == 3 and ld.timeout == FC.LOADER_TIMEOUT_S > 0 and ld.multiprocessing_context is None
    for ld in FC.build_loaders(cfg, ds, ds, 2, None, "cpu", False):
        assert ld.num_workers == 0
    src = open(os.path.join(ROOT, "din-group-activity-recognition-benchmark_amd", "frame_cache.py")).read()
    assert "cpu_count" not in src and "set_start_method" not in src


# ---- frame_ids=True --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [_volleyball, _collective], ids=["volleyball", "collective"])
def test_frame_table_is_sorted_unique_and_stable(golden_dir, make):
    a, b = make(golden_dir, frame_ids=True), make(golden_dir, frame_ids=True)
    assert a.frame_table == b.frame_table == sorted(set(a.frame_table))
    assert len(a.frame_table) == len(a) * 3                      # T = 3 frames per clip, no clip shares a frame in this tree
    assert all(os.path.isfile(p) for p in a.frame_table)
    assert a.resident.dtype == torch.uint8 and a.resident.shape == (len(a.frame_table),) and a.resident.is_shared()
    assert int(a.resident.sum()) == 0


@pytest.mark.parametrize("make", [_volleyball, _collective], ids=["volleyball", "collective"])
def test_items_carry_ids_and_only_the_missing_frames(golden_dir, make, monkeypatch):
    from din_amd import collective as Cc, volleyball as V
    plain, ds = make(golden_dir), make(golden_dir, frame_ids=True)
    for i in range(len(ds)):
        ids, miss, *labels, miss_index = ds[i]
        ref = plain[i]
        assert ids.dtype == torch.int64 and ids.shape == (3,) and miss.dtype == torch.uint8 and miss.shape == (3, 3, 64, 96)
        assert miss_index.tolist() == [0, 1, 2]
        for t in range(3):
            assert np.array_equal(miss[t].numpy(), V.load_frame_u8(ds.frame_table[int(ids[t])], (64, 96)))
        assert torch.equal(miss, ref[0])
        assert len(labels) == len(ref) - 1 and all(torch.equal(x, y) for x, y in zip(labels, ref[1:]))
    # flags set: those frames are not decoded, and M shrinks
    calls = []
    real = V.load_frame_u8

    def counting(path, size):
        calls.append(path)
        return real(path, size)

    monkeypatch.setattr(V, "load_frame_u8", counting)
    monkeypatch.setattr(Cc, "load_frame_u8", counting)
    ids0 = ds[0][0]
    assert len(calls) == 3
    del calls[:]
    ds.resident[ids0[1]] = 1
    ids, miss, *labels, miss_index = ds[0]
    assert torch.equal(ids, ids0) and miss.shape[0] == 2 and miss_index.tolist() == [0, 2]
    assert calls == [ds.frame_table[int(ids0[0])], ds.frame_table[int(ids0[2])]]
    assert torch.equal(miss, plain[0][0][[0, 2]])
    del calls[:]
    ds.resident[ids0] = 1
    ids, miss, *labels, miss_index = ds[0]
    assert calls == [] and miss.shape == (0, 3, 64, 96) and miss.dtype == torch.uint8 and miss_index.numel() == 0
    assert all(torch.equal(x, y) for x, y in zip(labels, plain[0][1:]))
    assert ds[1][1].shape[0] == 3                                # another clip is untouched


def test_frame_ids_refuse_float_images(golden_dir):
    with pytest.raises(ValueError):
        _volleyball(golden_dir, frame_ids=True, uint8_images=False)


@pytest.mark.parametrize("make", [_volleyball, _collective], ids=["volleyball", "collective"])
def test_collate_positions_for_empty_partial_and_full_items(golden_dir, make):
    from din_amd import frame_cache as FC
    plain, ds = make(golden_dir), make(golden_dir, frame_ids=True)
    ds.resident[ds[0][0]] = 1                                    # clip 0: M = 0
    ds.resident[ds[1][0][[0, 2]]] = 1                            # clip 1: only its middle frame is decoded; clip 2: all three
    items = [ds[i] for i in range(3)]
    assert [it[1].shape[0] for it in items] == [0, 1, 3]
    frame_ids, miss_images, miss_pos, *labels = FC.collate(items)
    assert frame_ids.shape == (3, 3) and frame_ids.dtype == torch.int64
    assert miss_pos.dtype == torch.int64 and miss_pos.tolist() == [4, 6, 7, 8]
    assert miss_images.shape == (4, 3, 64, 96) and miss_images.dtype == torch.uint8
    want = torch.stack([plain[i][0] for i in range(3)]).reshape(9, 3, 64, 96)
    assert torch.equal(miss_images, want[miss_pos])
    ref = tud.default_collate([plain[i][1:] for i in range(3)])
    assert len(labels) == len(ref) and all(torch.equal(x, y) and x.dtype == y.dtype for x, y in zip(labels, ref))
    # every item empty
    ds.resident[:] = 1
    frame_ids, miss_images, miss_pos, *labels = FC.collate([ds[i] for i in range(3)])
    assert miss_images.shape == (0, 3, 64, 96) and miss_pos.numel() == 0 and frame_ids.shape == (3, 3)


# ---- bookkeeping -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame_bytes,stride", [(1, 16), (16, 16), (17, 32), (84651, 84656)])
def test_slot_stride_is_frame_bytes_rounded_up_to_16(frame_bytes, stride):
    from din_amd.frame_cache import SlotTable
    t = SlotTable(frame_bytes, 10 * stride + 5, chunk_frames=4)
    assert t.stride == stride and t.stride % 16 == 0 and 0 <= t.stride - frame_bytes < 16
    assert t.max_slots == 10


def test_slot_table_growth_capacity_and_counters():
    from din_amd.frame_cache import SlotTable
    t = SlotTable(17, 6 * 32, chunk_frames=4)                    # 6 slots of 32 bytes: a slab of 4 and a slab of 2
    asked = []

    def grow(n):
        asked.append(n)
        return True

    assert t.bytes == 0 and t.counters() == {"hits": 0, "misses": 0, "inserted": 0, "bytes": 0}
    assert [t.insert(100 + i, grow) for i in range(4)] == [0, 1, 2, 3]
    assert asked == [4] and t.bytes == 4 * 32                    # memory grows with use ...
    assert t.insert(104, grow) == 4 and asked == [4, 2] and t.bytes == 6 * 32   # ... a slab at a time, never beyond the capacity
    assert t.locate(3) == (0, 96) and t.locate(4) == (1, 0) and t.locate(5) == (1, 32)
    assert t.insert(105, grow) == 5 and t.full
    assert t.insert(106, grow) == -1 and t.insert(107, grow) == -1 and asked == [4, 2]   # refusal at capacity, no allocation asked
    assert t.inserted == 6 and t.hits == 0
    assert t.insert(102, grow) == 2                              # a re-inserted id is a hit, not a second slot
    assert t.inserted == 6 and t.hits == 1 and len(t.slot_of) == 6
    assert t.lookup(105) == 5 and t.lookup(106) == -1
    assert t.counters() == {"hits": 2, "misses": 1, "inserted": 6, "bytes": 6 * 32}


def test_failed_slab_allocation_freezes_the_table():
    from din_amd.frame_cache import SlotTable
    t = SlotTable(16, 100 * 16, chunk_frames=4)
    answers = iter([True, False])
    for i in range(4):
        assert t.insert(i, lambda n: next(answers)) == i
    assert t.insert(4, lambda n: next(answers)) == -1 and t.frozen and t.full and t.max_slots == 4 and t.bytes == 64
    assert t.insert(5, lambda n: pytest.fail("a frozen table asks for no more memory")) == -1
    assert t.lookup(2) == 2 and t.inserted == 4
    with pytest.raises(ValueError):
        SlotTable(0, 100)


# ---- loader workers --------------------------------------------------------------------------------------------------------------------
def _check_workers_against_main_process(golden_dir):
    """runs in a child process of its own (below), so that no GPU was ever initialised where the workers fork"""
    from din_amd import frame_cache as FC
    from din_amd.config import Config
    for frame_ids in (False, True):
        ds = _volleyball(golden_dir, is_training=False, frame_ids=frame_ids)
        if frame_ids:
            ds.resident[ds[1][0][1]] = 1
        out = []
        for workers in (0, 2):
            cfg = Config("volleyball")
            cfg.num_workers, cfg.test_batch_size = workers, 2
            cfg.frame_cache_gb = 1 if frame_ids else 0
            loader = FC.build_loaders(cfg, ds, ds, 2, None, "cpu", True)[1]
            loader = loader.loader if frame_ids else loader
            assert loader.num_workers == workers
            out.append([tuple(t.clone() for t in batch) for batch in loader])
        assert len(out[0]) == len(out[1]) == 2
        for a, b in zip(*out):
            assert len(a) == len(b) == (6 if frame_ids else 4)
            assert all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))
        if frame_ids:
            assert sum(b[1].shape[0] for b in out[1]) == 8       # 9 frames, one flagged resident before the workers started
    assert not torch.cuda.is_initialized()
    print("workers-ok")


def test_two_workers_yield_the_same_batches_in_the_same_order(golden_dir):
    """the deterministic (is_training=False) split through the trainers' own loader construction, num_workers 0 against 2, plain and
    with frame ids (the flags set in the parent are what the forked workers see), in a fresh process that never initialises a GPU"""
    import subprocess
    import sys
    code = f"import tests.test_frame_cache_cpu as t; t._check_workers_against_main_process({golden_dir!r})"
    res = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert res.returncode == 0 and "workers-ok" in res.stdout, res.stdout


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_makefile_agree_on_copy_rows():
    import ctypes as C
    from din_amd import _lib
    text = open(_lib.HEADER_PATH).read()
    assert "#define DIN_ABI_VERSION 9 " in text and _lib.ABI_VERSION == 9
    assert "din_copy_rows_u8" in _lib.header_symbols() and set(_lib.header_symbols()) == set(_lib.SIGNATURES)
    decl = text[text.index("int din_copy_rows_u8("):]
    decl = decl[:decl.index(");")]
    assert re.sub(r"\s+", " ", decl) == "int din_copy_rows_u8(const uint64_t* src, const uint64_t* dst, int n, int64_t bytes, void* stream"
    res, args = _lib.SIGNATURES["din_copy_rows_u8"]
    assert res is C.c_int and args == [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p]
    assert "volleyball.py:223-275" in text and "train_net_dynamic.py:174" in text
    assert re.search(r"^SRCS = .*\bframe_copy\.hip\b", open(os.path.join(_lib.CSRC_DIR, "Makefile")).read(), flags=re.M)
    assert os.path.isfile(os.path.join(_lib.CSRC_DIR, "frame_copy.hip"))
    if os.path.exists(_lib.LIB_PATH):
        assert hasattr(C.CDLL(_lib.LIB_PATH), "din_copy_rows_u8")
    from din_amd import ops
    assert callable(ops.copy_rows_u8)
