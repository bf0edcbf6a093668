"""The map cache (cfg.map_cache_gb), host side (no GPU): the config default, train_net's new refusals and the old ones word for word,
frame ids under the setting, slot and trailer sizes, FrameRefs carrying a MapCache through ARG's fold and the collective 3-tuple, the slot
bookkeeping with duplicates and a full table, the loaders, and the C ABI, which the setting leaves alone."""
import os

import numpy as np
import pytest
import torch
import torch.utils.data as tud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "din-group-activity-recognition-benchmark_amd")


def _cfg(name="volleyball", **kw):
    from din_amd.config import Config
    cfg = Config(name)
    cfg.backbone, cfg.training_stage, cfg.emb_features, cfg.map_cache_gb = "vgg16", 2, 512, 1
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _refused(cfg, monkeypatch):
    """train_net's ValueError, raised before a dataset, a loader, a process group or the device is touched"""
    from din_amd import frame_cache as FC, train_net_dynamic as TD
    monkeypatch.setattr(FC, "build_loaders", lambda *a, **k: pytest.fail("a loader was built before the refusal"))
    monkeypatch.setattr(TD.parallel, "init_from_env", lambda *a, **k: pytest.fail("the device was set up before the refusal"))
    monkeypatch.setattr(TD, "build_model", lambda *a, **k: pytest.fail("a model was built before the refusal"))
    with pytest.raises(ValueError) as e:
        TD.train_net(cfg)
    return str(e.value)


def test_config_default_is_off():
    from din_amd import feature_cache as FE, frame_cache as FC
    from din_amd.config import Config
    for name in ("volleyball", "collective"):
        cfg = Config(name)
        assert cfg.map_cache_gb == 0 and not FC.wants_maps(cfg) and FE.map_refusal(cfg) is None


@pytest.mark.parametrize("kw,words", [
    (dict(map_cache_gb=-1), ("real number >= 0",)),
    (dict(map_cache_gb=True), ("real number >= 0",)),
    (dict(map_cache_gb="1"), ("real number >= 0",)),
    (dict(map_cache_gb=float("nan")), ("real number >= 0",)),
    (dict(map_cache_gb=None), ("real number >= 0",)),
    (dict(train_backbone=True), ("train_backbone", "FROZEN")),
    (dict(frame_cache_gb=2), ("frame_cache_gb = 2", "choose one")),
    (dict(feature_cache_gb=0.5), ("feature_cache_gb = 0.5", "choose one")),
    (dict(backbone="inv3", set_bn_eval=True), ("inv3", "13 MB a frame", "630 GB")),
    (dict(flip_prob=0.5), ("flip_prob = 0.5", "as decoded")),
    (dict(color_jitter=(0.1, 0.2, 0.3)), ("color_jitter", "as decoded")),
    (dict(test_flip=True), ("test_flip", "as decoded")),
], ids=["negative", "bool", "string", "nan", "none", "train_backbone", "frame_cache_too", "feature_cache_too", "inv3", "flip_prob", "color_jitter",
        "test_flip"])
@pytest.mark.parametrize("dataset", ["volleyball", "collective"])
def test_train_net_refuses_before_any_loader_is_built(kw, words, dataset, monkeypatch):
    said = _refused(_cfg(dataset, **kw), monkeypatch)
    if dataset == "collective" and "feature_cache_gb" in kw:        # (the feature cache's own refusal of the dataset comes first)
        assert said == "feature_cache_gb = 0.5: the collective dataset is not covered (volleyball only)"
        return
    for w in ("map_cache_gb",) + words:
        assert w in said, (w, said)


OLD_REFUSALS = [
    (dict(train_backbone=True), "feature_cache_gb = 1: cached box features are the output of a FROZEN backbone; train_backbone is set"),
    (dict(frame_cache_gb=2), "feature_cache_gb = 1: frame_cache_gb = 2 is set as well; the pixels of a frame whose features are resident are "
                             "never needed: choose one of the two caches"),
    (dict(inference_module_name="dynamic_tce_volleyball"), "feature_cache_gb = 1: dynamic_tce_volleyball reads the backbone's context map of "
                                                           "every frame, which the feature cache does not keep"),
    (dict(_dataset="collective"), "feature_cache_gb = 1: the collective dataset is not covered (volleyball only)"),
    (dict(backbone="inv3", set_bn_eval=False), "feature_cache_gb = 1: backbone 'inv3' without set_bn_eval normalises with batch statistics, so "
                                               "a frame's features depend on the batch it is in and cannot be cached"),
    (dict(flip_prob=0.5), "flip_prob = 0.5: feature_cache_gb = 1 caches the box features of the unmirrored frame; they cannot serve a "
                          "mirrored one"),
    (dict(color_jitter=(0.1, 0.2, 0.3)), "color_jitter = (0.1, 0.2, 0.3): feature_cache_gb = 1 caches the box features of the frame as "
                                         "decoded; they cannot serve a jittered one"),
]


@pytest.mark.parametrize("map_cache_gb", [0, 1], ids=["map_cache_off", "map_cache_on_as_well"])
@pytest.mark.parametrize("kw,text", OLD_REFUSALS, ids=["train_backbone", "frame_cache_too", "tce", "collective", "inv3_batch_stats", "flip", "jitter"])
def test_the_older_refusals_keep_their_words_and_come_first(kw, text, map_cache_gb, monkeypatch):
    kw = dict(kw)
    cfg = _cfg(kw.pop("_dataset", "volleyball"), feature_cache_gb=1, map_cache_gb=map_cache_gb, **kw)
    assert _refused(cfg, monkeypatch) == text


def test_accepted_settings_are_not_refused():
    from din_amd import feature_cache as FE
    for dataset in ("volleyball", "collective"):
        for module in ("dynamic_volleyball", "dynamic_tce_volleyball", "dynamic_collective", "arg_volleyball", "at_volleyball", "pctdm_volleyball"):
            for dt in ("fp32", "bf16", "fp32_bf16x3"):
                assert FE.map_refusal(_cfg(dataset, inference_module_name=module, backbone_dtype=dt, map_cache_gb=0.25)) is None
    assert FE.map_refusal(_cfg(map_cache_gb=0, train_backbone=True, frame_cache_gb=3, backbone="inv3", flip_prob=0.5, test_flip=True)) is None
    assert FE.map_refusal(_cfg(map_cache_gb=0.0, color_jitter=(0.1, 0.1, 0.1))) is None      # off: nothing to refuse


def test_wants_frame_ids():
    from din_amd import frame_cache as FC
    from din_amd.config import Config
    cfg = Config("collective")
    assert not FC.wants_frame_ids(cfg) and not FC.wants_maps(cfg)
    cfg.map_cache_gb = 0.5
    assert FC.wants_frame_ids(cfg) and FC.wants_maps(cfg) and not FC.wants_features(cfg)
    del cfg.map_cache_gb                                            # a cfg of before the setting existed
    assert not FC.wants_frame_ids(cfg) and not FC.wants_maps(cfg)


@pytest.mark.parametrize("dataset,image_size,out_size,dtype,row_bytes", [
    ("volleyball", (720, 1280), (22, 40), "fp32", 1802240),
    ("volleyball", (720, 1280), (22, 40), "bf16", 901120),
    ("volleyball", (720, 1280), (22, 40), "fp32_bf16x3", 1802240),
    ("collective", (480, 720), (15, 22), "fp32", 675840),
    ("volleyball", (96, 160), (3, 5), "fp32", 30720),
    ("collective", (64, 96), (2, 3), "fp32", 12288),
    ("collective", (64, 96), (2, 3), "bf16", 6144),
], ids=["volleyball", "volleyball_bf16", "volleyball_split", "collective", "tiny_volleyball", "tiny_collective", "tiny_collective_bf16"])
def test_slot_and_trailer_sizes(dataset, image_size, out_size, dtype, row_bytes):
    from din_amd.feature_cache import FeatureCache, MapCache, map_shape_and_itemsize
    cfg = _cfg(dataset, image_size=image_size, out_size=out_size, backbone_dtype=dtype)
    shape, itemsize = map_shape_and_itemsize(cfg)
    assert shape == out_size + (512,) and itemsize == (2 if dtype == "bf16" else 4)
    cache = MapCache("cpu", shape, itemsize, 10 ** 9)
    assert isinstance(cache, FeatureCache) and cache.WHAT == "map cache"
    assert (cache.row_bytes, cache.box_bytes, cache.table.stride) == (row_bytes, 16, row_bytes + 16)
    assert cache.table.max_slots == 10 ** 9 // (row_bytes + 16) and cache.table.chunk_frames == 64
    assert cache.bytes == 0 and not cache.slabs and cache.map_dtype is None and cache.relu_masked is None    # nothing before the first map
    t = cache.trailers([0, 48299, 7])
    assert t.dtype == np.float32 and t.nbytes == 3 * 16 and t.tolist() == [[f, out_size[0], out_size[1], 512] for f in (0, 48299, 7)]


def test_the_whole_volleyball_set_fits():
    from din_amd.feature_cache import MapCache
    assert 48300 * 1802240 == 87_048_192_000                        # the 87 GB of the README, 43.5 GB as bf16
    assert MapCache("cpu", (22, 40, 512), 4, 288 * 10 ** 9).table.max_slots > 3 * 48300


def test_what_a_map_cache_refuses_to_be():
    from din_amd.feature_cache import MapCache
    for shape, itemsize in (((22, 40), 4), ((22, 40, 0), 4), ((22, 40, 512), 1), ((22, 40, 512), 8), ((1, 1, 2), 2)):
        with pytest.raises(ValueError):
            MapCache("cpu", shape, itemsize, 1 << 20)                # (the last: 4 bytes are no multiple of 16)
    cache = MapCache("cpu", (2, 3, 512), 4, 1 << 20)
    for ids in ([-1], [1 << 24]):
        with pytest.raises(ValueError, match="exact as fp32"):
            cache.trailers(ids)
    assert np.float32((1 << 24) - 1) == (1 << 24) - 1


def test_frame_refs_carry_a_map_cache_through_the_fold_and_the_collective_tuple():
    from din_amd.feature_cache import FrameRefs, MapCache
    cache = MapCache("cpu", (2, 3, 512), 4, 1 << 20)
    ids = np.arange(18).reshape(2, 9)
    miss = torch.zeros((4, 3, 64, 96), dtype=torch.uint8)
    refs = FrameRefs(ids, miss, [0, 5, 9, 17], cache)
    assert refs.shape == (2, 9, 3, 64, 96) and refs.context is None and refs.mirror is None
    folded = refs.reshape((6, 3) + tuple(refs.shape[2:]))           # ARG_volleyball's eval fold: B*3, T/3
    assert folded.shape == (6, 3, 3, 64, 96) and folded.cache is cache and folded.frame_ids.tolist() == np.arange(18).reshape(6, 3).tolist()
    folded.inserted.append(7)                                       # what the model records reaches the object the feed yielded
    assert refs.inserted == [7]
    images_in, boxes_in, bboxes_num_in = (FrameRefs(ids[:, :3], miss[:0], [], cache), torch.zeros(2, 3, 13, 4), torch.ones(2, 3))
    assert (images_in.shape[0], images_in.shape[1]) == (2, 3)       # all Dynamic_collective.forward and the passes read of it
    with pytest.raises(ValueError):
        refs.reshape((18, 3, 64, 96))


class _Tables:
    """a MapCache's own SlotTable (slabs of two) behind feature_cache.gather_tables, with made-up addresses: slot s at 1_000_000 + s *
    stride, computed map j at 50_000_000 + j * row_bytes"""

    def __init__(self, slots):
        from din_amd.feature_cache import MapCache
        self.cache = MapCache("cpu", (2, 3, 512), 4, slots * (12288 + 16) + 100, chunk_frames=2)
        self.rb, self.stride, self.grown = self.cache.row_bytes, self.cache.table.stride, []
        assert self.cache.table.max_slots == slots and self.stride == 12304

    def slot(self, s):
        return 1_000_000 + s * self.stride

    def row(self, j):
        return 50_000_000 + j * self.rb

    def build(self, ids, miss_pos):
        from din_amd.feature_cache import gather_tables
        return gather_tables([self.cache.table], [self.slot], [lambda n: (self.grown.append(n), True)[1]], ids, [0] * len(ids), miss_pos,
                             [(self.row(0), self.rb)], self.rb)


def test_slot_bookkeeping_with_duplicates_and_a_full_table():
    w = _Tables(3)
    t = w.cache.table
    # frame 10 twice, both decoded: stored once, both rows served from its first computed map, never from the slot this launch writes
    src, keep, ref, extra, reported = w.build([10, 11, 10], [0, 1, 2])
    assert src == [w.row(0), w.row(1), w.row(0)] and keep == [w.slot(0), w.slot(1), 0] and ref == [0, 0, 0]
    assert extra == [] and reported == [10, 11] and (t.hits, t.misses, t.inserted) == (0, 2, 2) and w.grown == [2]
    # served rows come from their slots and name their trailer (slot + row_bytes) for the comparison; one slot is left for frame 12
    src, keep, ref, extra, reported = w.build([11, 12, 13, 10], [1, 2])
    assert src == [w.slot(1), w.row(0), w.row(1), w.slot(0)] and keep == [0, w.slot(2), 0, 0]
    assert ref == [w.slot(1) + 12288, 0, 0, w.slot(0) + 12288] and reported == [12] and t.full and w.grown == [2, 1]
    assert (t.hits, t.misses, t.inserted) == (2, 4, 3)              # (frame 13 was looked up, missed, and found no room)
    # full: a computed map is served and not kept; what is neither resident nor computed is a KeyError
    src, keep, ref, extra, reported = w.build([13, 12], [0])
    assert src == [w.row(0), w.slot(2)] and keep == [0, 0] and ref == [0, w.slot(2) + 12288] and reported == [] and t.inserted == 3
    with pytest.raises(KeyError):
        w.build([13], [])


def test_loaders_with_and_without_the_setting(golden_dir):
    import pickle
    from din_amd import feature_cache as FE, frame_cache as FC, volleyball as V
    root = os.path.join(golden_dir, "dataset_tree", "volleyball")
    anns = V.volley_read_dataset(root, [1, 4])
    with open(os.path.join(root, "tracks_normalized.pkl"), "rb") as fh:
        tracks = pickle.load(fh)
    mk = lambda **kw: V.VolleyballDataset(anns, tracks, V.volley_all_frames(anns), root, (64, 96), (2, 3), "dynamic_volleyball", num_boxes=12,
                                          num_before=1, num_after=1, **kw)
    cfg = _cfg(map_cache_gb=0, image_size=(64, 96), out_size=(2, 3))
    for real_tree in (False, True):                                 # off: the plain loaders
        for ld in FC.build_loaders(cfg, mk(), mk(), 2, None, "cpu", real_tree):
            assert type(ld) is tud.DataLoader and ld.num_workers == 0 and ld.collate_fn is tud.default_collate
    cfg.map_cache_gb = 1
    ids = mk(frame_ids=FC.wants_frame_ids(cfg))
    assert ids.frame_ids
    for ld in FC.build_loaders(cfg, ids, ids, 2, None, "cpu", False):   # like the other caches: only with the real dataset tree
        assert type(ld) is tud.DataLoader
    tr, va = FC.build_loaders(cfg, ids, ids, 2, None, "cpu", True)
    for ld in (tr, va):
        assert type(ld) is FE.FeatureLoader and ld.loader.collate_fn is FC.collate and ld.mirror is None and ld.dataset is ids
        assert type(ld.cache) is FE.MapCache and (ld.cache.row_bytes, ld.cache.box_bytes) == (12288, 16)
        assert ld.cache.table.max_slots == 10 ** 9 // 12304 and ld.cache.bytes == 0
    assert tr.cache is not va.cache                                 # one for the training set, one for the validation set
    assert FE.cache_files(cfg, None, tr, va) == {}                  # no file: map_cache_path is a follow-up


def test_stage1_trainer_ignores_the_setting():
    src = open(os.path.join(PKG, "train_net.py")).read()
    assert "lcfg.map_cache_gb = 0" in src and "lcfg.feature_cache_gb = 0" in src and "build_loaders(lcfg," in src and "wants_frame_ids(lcfg)" in src
    assert "map_refusal" not in src


def test_the_c_abi_is_untouched():
    from din_amd import _lib
    names = _lib.header_symbols()
    assert len(names) == 122 and len(set(names)) == 122 and set(names) == set(_lib.SIGNATURES) and _lib.ABI_VERSION == 9
    assert "#define DIN_ABI_VERSION 9 " in open(_lib.HEADER_PATH).read()
    assert sorted(os.listdir(os.path.dirname(_lib.HEADER_PATH))) == ["din_hip.h"]
    assert not [n for n in names if "map" in n.lower() and "cache" in n.lower()]
    for folder, _, files in os.walk(PKG):
        assert not [f for f in files if f.endswith(".hip") and "map" in f], folder
