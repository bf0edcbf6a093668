"""Box-feature cache, host side (no GPU): the config default, train_net's refusals, frame ids under the setting, FrameRefs, the slot
bookkeeping with the boxes trailer, the dataset item under the setting, the default loaders, and the C ABI of din_feat_rows."""
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


def _cfg(name="volleyball", **kw):
    from din_amd.config import Config
    cfg = Config(name)
    cfg.backbone, cfg.training_stage, cfg.feature_cache_gb = "vgg16", 2, 1
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_config_default_is_off():
    from din_amd.config import Config
    for name in ("volleyball", "collective"):
        cfg = Config(name)
        assert cfg.feature_cache_gb == 0 and cfg.train_backbone is False


@pytest.mark.parametrize("kw,words", [
    (dict(train_backbone=True), ("feature_cache_gb", "train_backbone")),
    (dict(frame_cache_gb=2), ("feature_cache_gb", "frame_cache_gb")),
    (dict(inference_module_name="dynamic_tce_volleyball"), ("feature_cache_gb", "dynamic_tce_volleyball", "context map")),
    (dict(_dataset="collective"), ("feature_cache_gb", "collective")),
    (dict(backbone="inv3", set_bn_eval=False), ("feature_cache_gb", "inv3", "set_bn_eval")),
], ids=["train_backbone", "frame_cache_too", "tce", "collective", "inv3_batch_stats"])
def test_train_net_refuses_before_any_loader_is_built(kw, words, monkeypatch):
    """each refusal is a ValueError naming the setting, raised before a dataset, a loader or the device is touched"""
    from din_amd import frame_cache as FC, train_net_dynamic as TD
    kw = dict(kw)
    cfg = _cfg(kw.pop("_dataset", "volleyball"), **kw)
    monkeypatch.setattr(FC, "build_loaders", lambda *a, **k: pytest.fail("a loader was built before the refusal"))
    monkeypatch.setattr(TD.parallel, "init_from_env", lambda *a, **k: pytest.fail("the device was set up before the refusal"))
    with pytest.raises(ValueError) as e:
        TD.train_net(cfg)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_accepted_settings_are_not_refused():
    from din_amd import feature_cache as FE
    assert FE.refusal(_cfg()) is None
    assert FE.refusal(_cfg(backbone="inv3", set_bn_eval=True)) is None
    assert FE.refusal(_cfg(inference_module_name="arg_volleyball")) is None
    assert FE.refusal(_cfg(feature_cache_gb=0, train_backbone=True, frame_cache_gb=3)) is None      # off: nothing to refuse


def test_wants_frame_ids():
    from din_amd import frame_cache as FC
    from din_amd.config import Config
    cfg = Config("volleyball")
    assert not FC.wants_frame_ids(cfg)
    cfg.feature_cache_gb = 0.5
    assert FC.wants_frame_ids(cfg)
    cfg.feature_cache_gb, cfg.frame_cache_gb = 0, 2
    assert FC.wants_frame_ids(cfg)


def test_frame_refs_shape_and_reshape():
    from din_amd.feature_cache import FrameRefs
    ids = np.arange(18).reshape(2, 9)
    miss = torch.zeros((4, 3, 64, 96), dtype=torch.uint8)
    refs = FrameRefs(ids, miss, [0, 5, 9, 17], cache="the cache")
    assert refs.shape == (2, 9, 3, 64, 96)
    folded = refs.reshape((6, 3) + refs.shape[2:])                  # ARG_volleyball's eval fold: B*3, T/3
    assert folded.shape == (6, 3, 3, 64, 96) and folded.frame_ids.tolist() == np.arange(18).reshape(6, 3).tolist()
    assert folded.miss_images is miss and folded.cache == "the cache" and folded.miss_pos.tolist() == [0, 5, 9, 17]
    folded.inserted.append(7)                                       # what the model records reaches the object the feed yielded
    assert refs.inserted == [7]
    empty = FrameRefs(ids, miss[:0], [], cache=None)
    assert empty.shape == (2, 9, 3, 64, 96) and empty.reshape((18, 1, 3, 64, 96)).shape == (18, 1, 3, 64, 96)
    for bad in ((2, 9, 3, 96, 64), (3, 9, 3, 64, 96), (18, 3, 64, 96)):
        with pytest.raises(ValueError):
            refs.reshape(bad)
    with pytest.raises(ValueError):
        FrameRefs(ids, miss, [0, 5], cache=None)                    # four frames, two positions
    with pytest.raises(ValueError):
        FrameRefs(ids.reshape(-1), miss, [0, 5, 9, 17], cache=None)


def test_slots_hold_the_row_and_its_boxes():
    """row_bytes 1600 and box_bytes 192: slots 1792 bytes apart, a capacity of 6 slots stops at 6 (no device is needed for the
    bookkeeping: nothing is allocated before the first row arrives)"""
    from din_amd.feature_cache import FeatureCache
    cache = FeatureCache("cpu", 1600, 192, 6 * 1792 + 100, chunk_frames=4)
    t = cache.table
    assert (cache.row_bytes, cache.box_bytes) == (1600, 192) and t.stride == 1792 and t.max_slots == 6
    assert cache.bytes == 0 and not cache.slabs and (cache.hits, cache.misses, cache.inserted) == (0, 0, 0)
    asked = []

    def grow(n):
        asked.append(n)
        return True

    assert [t.insert(100 + i, grow) for i in range(8)] == [0, 1, 2, 3, 4, 5, -1, -1]
    assert asked == [4, 2] and cache.inserted == 6 and cache.bytes == 6 * 1792 and t.full
    assert t.locate(5) == (1, 1792) and cache.resident(105) and not cache.resident(106)
    assert t.lookup(103) == 3 and t.lookup(107) == -1 and (cache.hits, cache.misses) == (1, 1)
    for rb, bb in ((1608, 192), (1600, 24), (0, 192), (1600, 0)):
        with pytest.raises(ValueError):
            FeatureCache("cpu", rb, bb, 1 << 20)


def test_row_and_box_bytes_at_the_launchers_sizes():
    from din_amd.config import Config
    from din_amd.feature_cache import row_and_box_bytes
    cfg = Config("volleyball")
    cfg.emb_features = 512
    assert row_and_box_bytes(cfg) == (614400, 192)                   # VGG16: 12 x 512 x 25 x 4
    cfg.emb_features = 1056
    assert row_and_box_bytes(cfg) == (1267200, 192)                  # Inception-v3


def test_items_under_the_setting_carry_only_non_resident_frames(golden_dir, monkeypatch):
    """cfg.feature_cache_gb > 0 alone makes return_dataset's callers ask for frame ids; an item then decodes what is not resident"""
    from din_amd import frame_cache as FC, volleyball as V
    from din_amd.config import Config
    cfg = Config("volleyball")
    cfg.feature_cache_gb = 1
    plain, ds = _volleyball(golden_dir), _volleyball(golden_dir, frame_ids=FC.wants_frame_ids(cfg))
    assert ds.frame_ids
    calls, real = [], V.load_frame_u8
    monkeypatch.setattr(V, "load_frame_u8", lambda path, size: (calls.append(path), real(path, size))[1])
    ids, miss, *labels, miss_index = ds[0]
    assert miss.shape == (3, 3, 64, 96) and miss_index.tolist() == [0, 1, 2] and len(calls) == 3
    ds.resident[ids[[0, 2]]] = 1
    del calls[:]
    ids2, miss, *labels, miss_index = ds[0]
    assert torch.equal(ids2, ids) and miss_index.tolist() == [1] and calls == [ds.frame_table[int(ids[1])]]
    assert torch.equal(miss, plain[0][0][[1]]) and all(torch.equal(x, y) for x, y in zip(labels, plain[0][1:]))


def test_loaders_with_and_without_the_setting(golden_dir):
    from din_amd import feature_cache as FE, frame_cache as FC
    from din_amd.config import Config
    cfg = Config("volleyball")
    assert cfg.feature_cache_gb == 0 and cfg.frame_cache_gb == 0
    ds = _volleyball(golden_dir)
    for real_tree in (False, True):                                 # both settings 0: the plain loaders
        for ld in FC.build_loaders(cfg, ds, ds, 2, None, "cpu", real_tree):
            assert type(ld) is tud.DataLoader and ld.num_workers == 0 and ld.collate_fn is tud.default_collate
    cfg.feature_cache_gb, cfg.emb_features = 1, 512
    ids = _volleyball(golden_dir, frame_ids=True)
    for ld in FC.build_loaders(cfg, ids, ids, 2, None, "cpu", False):   # like the frame cache: only with the real dataset tree
        assert type(ld) is tud.DataLoader
    tr, va = FC.build_loaders(cfg, ids, ids, 2, None, "cpu", True)
    for ld in (tr, va):
        assert type(ld) is FE.FeatureLoader and isinstance(ld, FC.CachedLoader) and ld.loader.collate_fn is FC.collate
        assert type(ld.cache) is FE.FeatureCache and (ld.cache.row_bytes, ld.cache.box_bytes) == (614400, 192)
        assert ld.cache.table.max_slots == 10 ** 9 // 614592 and ld.cache.bytes == 0
        assert FE.FeatureLoader.feed is not FC.CachedLoader.feed
    assert tr.cache is not va.cache                                 # one for the training set, one for the validation set


def test_stage1_trainer_ignores_the_setting():
    src = open(os.path.join(ROOT, "din-group-activity-recognition-benchmark_amd", "train_net.py")).read()
    assert "lcfg.feature_cache_gb = 0" in src and "build_loaders(lcfg," in src and "wants_frame_ids(lcfg)" in src


def test_header_binding_and_makefile_agree_on_feat_rows():
    import ctypes as C
    from din_amd import _lib, ops
    text = open(_lib.HEADER_PATH).read()
    assert "#define DIN_ABI_VERSION 9 " in text and _lib.ABI_VERSION == 9
    assert "din_feat_rows" in _lib.header_symbols() and set(_lib.header_symbols()) == set(_lib.SIGNATURES)
    decl = text[text.index("int din_feat_rows("):]
    decl = decl[:decl.index(");")]
    assert re.sub(r"\s+", " ", decl) == ("int din_feat_rows(const uint64_t* src, const uint64_t* dst, const uint64_t* keep, "
                                         "const uint64_t* ref_boxes, const void* boxes, uint8_t* flags, int n, int64_t row_bytes, "
                                         "int box_bytes, void* stream")
    res, args = _lib.SIGNATURES["din_feat_rows"]
    assert res is C.c_int and args == [C.c_void_p] * 6 + [C.c_int, C.c_int64, C.c_int, C.c_void_p]
    assert "infer_model.py:152-184" in text
    seg = int(re.search(r"^#define DIN_FEAT_ROWS_SEGMENT (\d+)$", text, flags=re.M).group(1))
    assert ops.FEAT_ROWS_SEGMENT == seg and seg % 16 == 0
    assert re.search(r"^SRCS = .*\bfeat_cache\.hip\b", open(os.path.join(_lib.CSRC_DIR, "Makefile")).read(), flags=re.M)
    kernel = open(os.path.join(_lib.CSRC_DIR, "feat_cache.hip")).read()
    assert "infer_model.py:152-184" in kernel and "DIN_FEAT_ROWS_SEGMENT" in kernel and "atomic" not in kernel.replace("no atomics", "")
    if os.path.exists(_lib.LIB_PATH):
        assert hasattr(C.CDLL(_lib.LIB_PATH), "din_feat_rows")
    assert callable(ops.feat_rows)
