"""The box-feature cache on disk, on the MI355X: FeatureCache.save / load across slabs (fp32 and bf16 slots, a capacity smaller than the
file, foreign fingerprints), and train_net_dynamic.train_net over tests/golden/dataset_tree with cfg.feature_cache_path: a run that writes
the files, a second run that starts from them (nothing decoded, no trunk launch, the same weights to the last bit), a run with another
head on the same files, files of another fingerprint, and a file whose boxes are not the dataset's."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

pytestmark = pytest.mark.gpu

ELEMS, BB = 400, 192                                             # 400 features a row, 12 boxes
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from din_amd import _lib
    _lib.load()
    return torch.device("cuda")


def _fingerprint(**kw):
    from din_amd import feature_cache_file as FF
    fp = {k: f"value of {k}" for k in FF.FIELDS}
    fp.update({"digest": "d" * 64, **kw})
    return fp


def _filled(gpu, dtype, count=7, chunk_frames=2, capacity=1 << 30):
    """a cache of `count` rows in slabs of two slots (the last slab part-filled for an odd count), the ids in no particular order"""
    from din_amd.feature_cache import FeatureCache
    g = torch.Generator().manual_seed(21)
    rows, boxes = torch.randn((count, ELEMS), generator=g), torch.rand((count, BB // 4), generator=g) * 40
    rb = ELEMS * (4 if dtype == "fp32" else 2)
    cache = FeatureCache(gpu, rb, BB, capacity, chunk_frames=chunk_frames, dtype=DTYPES[dtype])
    ids = [905, 17, 300, 4, 1000003, 58, 21][:count]
    cache.rows(ids[:4], boxes[:4].to(gpu), range(4), rows[:4].to(gpu).contiguous())
    cache.rows(ids[4:], boxes[4:].to(gpu), range(count - 4), rows[4:].to(gpu).contiguous())
    cache.check()
    return cache, ids, rows.to(DTYPES[dtype]), boxes


def _slot_bytes(cache, fid):
    slab, off = cache.table.locate(cache.table.slot_of[fid])
    return cache.slabs[slab][off:off + cache.table.stride]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_save_then_load_gives_every_slot_back(gpu, tmp_path, dtype):
    from din_amd import feature_cache_file as FF
    from din_amd.feature_cache import FeatureCache
    cache, ids, rows, boxes = _filled(gpu, dtype)
    rb = cache.row_bytes
    assert len(cache.slabs) == 4 and cache.table.slab_slots == [2, 2, 2, 2] and cache.inserted == 7      # three full slabs, one half full
    path, meta = str(tmp_path / "train.dinfc"), _fingerprint()
    assert cache.save(path, meta) == 7 and not os.path.exists(path + ".tmp")
    header, file_ids, records = FF.read(path)
    assert header == {"fingerprint": meta, "row_bytes": rb, "box_bytes": BB, "dtype": dtype, "count": 7}
    assert file_ids.tolist() == ids                               # slot order
    for i, fid in enumerate(ids):                                 # a record is the slot's bytes: the row, then its boxes
        assert records[i].tobytes() == _slot_bytes(cache, fid).cpu().numpy().tobytes()
        assert records[i, :rb].tobytes() == rows[i].contiguous().view(torch.uint8).numpy().tobytes()
        assert records[i, rb:].tobytes() == boxes[i].numpy().tobytes()
    fresh = FeatureCache(gpu, rb, BB, 1 << 30, chunk_frames=2, dtype=DTYPES[dtype])
    assert fresh.load(path, meta) == ids                          # file order
    assert fresh.inserted == 7 and len(fresh.slabs) == 4 and list(fresh.table.slot_of) == ids
    for fid in ids:
        assert torch.equal(_slot_bytes(fresh, fid), _slot_bytes(cache, fid)), fid
    for k in range(3):                                            # whole slabs, byte for byte
        assert torch.equal(fresh.slabs[k], cache.slabs[k])
    order = [6, 0, 3, 3, 5, 1, 4, 2]
    out, new = fresh.rows([ids[i] for i in order], boxes[order].to(gpu))       # served by din_feat_rows, boxes compared
    assert new == [] and out.dtype == DTYPES[dtype] and torch.equal(out.cpu(), rows[order])
    fresh.check()
    wrong = boxes.clone()
    wrong[2, 5] += 0.25
    fresh.rows(ids, wrong.to(gpu))
    with pytest.raises(RuntimeError, match=r"\(2, 300\)"):        # a loaded row is checked against its boxes like a computed one
        fresh.check()
    assert fresh.save(str(tmp_path / "again.dinfc"), meta) == 7   # and what was loaded saves to the same bytes
    assert open(str(tmp_path / "again.dinfc"), "rb").read() == open(path, "rb").read()


def test_a_capacity_smaller_than_the_file_takes_the_prefix(gpu, tmp_path, caplog):
    from din_amd.feature_cache import FeatureCache
    cache, ids, rows, boxes = _filled(gpu, "fp32")
    path, meta = str(tmp_path / "train.dinfc"), _fingerprint()
    cache.save(path, meta)
    small = FeatureCache(gpu, cache.row_bytes, BB, 5 * cache.table.stride + 100, chunk_frames=2)
    with caplog.at_level("WARNING"):
        assert small.load(path, meta) == ids[:5]
    assert any("5 of the 7 frames" in r.getMessage() and "other 2" in r.getMessage() for r in caplog.records)
    assert [small.resident(i) for i in ids] == [True] * 5 + [False] * 2 and small.table.slab_slots == [2, 2, 1] and small.table.full
    for fid in ids[:5]:
        assert torch.equal(_slot_bytes(small, fid), _slot_bytes(cache, fid))
    misses = small.misses
    assert small.table.lookup(ids[5]) == -1 and small.table.lookup(ids[6]) == -1 and small.misses == misses + 2
    with pytest.raises(KeyError):                                 # not resident and not computed: as for any other miss
        small.rows([ids[6]], boxes[6:7].to(gpu))
    out, new = small.rows(ids, boxes.to(gpu), [5, 6], rows[5:].to(gpu).contiguous())     # the rest is computed and served, not kept
    assert new == [] and torch.equal(out.cpu(), rows)
    small.check()


def test_load_into_a_cache_that_already_holds_frames(gpu, tmp_path):
    """ids the cache already has keep their slots; the others follow in file order (a run whose first file was a prefix)"""
    from din_amd.feature_cache import FeatureCache
    cache, ids, rows, boxes = _filled(gpu, "fp32")
    path, meta = str(tmp_path / "train.dinfc"), _fingerprint()
    cache.save(path, meta)
    other = FeatureCache(gpu, cache.row_bytes, BB, 1 << 30, chunk_frames=2)
    other.rows([ids[3], ids[1], ids[2]], boxes[[3, 1, 2]].to(gpu), range(3), rows[[3, 1, 2]].to(gpu).contiguous())
    assert other.load(path, meta) == ids and list(other.table.slot_of) == [ids[3], ids[1], ids[2], ids[0], ids[4], ids[5], ids[6]]
    out, _ = other.rows(ids, boxes.to(gpu))
    assert torch.equal(out.cpu(), rows)
    other.check()


def test_an_empty_cache_saves_and_loads(gpu, tmp_path):
    from din_amd.feature_cache import FeatureCache
    path, meta = str(tmp_path / "val.dinfc"), _fingerprint()
    assert FeatureCache(gpu, 1600, BB, 1 << 30).save(path, meta) == 0
    fresh = FeatureCache(gpu, 1600, BB, 1 << 30)
    assert fresh.load(path, meta) == [] and fresh.inserted == 0 and not fresh.slabs


def test_load_refuses_another_fingerprint_or_geometry_before_inserting(gpu, tmp_path):
    from din_amd.feature_cache import FeatureCache
    cache, ids, rows, boxes = _filled(gpu, "fp32")
    path, meta = str(tmp_path / "train.dinfc"), _fingerprint()
    cache.save(path, meta)
    raw = open(path, "rb").read()
    fresh = FeatureCache(gpu, cache.row_bytes, BB, 1 << 30, chunk_frames=2)
    for field in ("backbone_weights", "crop_size", "digest"):
        with pytest.raises(ValueError) as e:
            fresh.load(path, _fingerprint(**{field: "something else"}))
        assert f"another {field}" in str(e.value) and path in str(e.value)
    with pytest.raises(ValueError, match="another image_size"):   # the first differing field of several
        fresh.load(path, _fingerprint(image_size=[1, 2], backbone_weights="x"))
    for other, what in ((FeatureCache(gpu, cache.row_bytes + 16, BB, 1 << 30), "row_bytes"),
                        (FeatureCache(gpu, cache.row_bytes, BB + 16, 1 << 30), "box_bytes"),
                        (FeatureCache(gpu, cache.row_bytes, BB, 1 << 30, dtype=torch.bfloat16), "dtype")):
        with pytest.raises(ValueError, match=what):
            other.load(path, meta)
        assert other.inserted == 0 and not other.slabs
    assert fresh.inserted == 0 and not fresh.slabs and open(path, "rb").read() == raw


# ---- through the trainer ------------------------------------------------------------------------------------------------------------------
TRAIN_FRAMES, VAL_FRAMES = 6, 3                                  # train sequence 1: two clips of three frames; test sequence 4: one clip


def _cfg(stage1, module="dynamic_volleyball", path=None, epochs=2):
    from din_amd.config import Config
    cfg = Config("volleyball")
    cfg.data_path, cfg.train_seqs, cfg.test_seqs = os.path.join(GOLDEN, "dataset_tree", "volleyball"), [1], [4]
    cfg.backbone, cfg.image_size, cfg.out_size, cfg.emb_features = "vgg16", (96, 160), (3, 5), 512
    cfg.num_boxes, cfg.num_frames, cfg.num_before, cfg.num_after = 12, 3, 1, 1
    cfg.num_features_boxes, cfg.num_features_gcn = 64, 64
    cfg.num_features_relation, cfg.num_graph, cfg.gcn_layers, cfg.pos_threshold = 16, 4, 1, 0.5
    cfg.ST_kernel_size, cfg.sampling_ratio, cfg.beta_factor, cfg.train_backbone = [(3, 3)], [1], False, False
    cfg.training_stage, cfg.batch_size, cfg.test_batch_size, cfg.max_epoch, cfg.test_interval_epoch = 2, 1, 1, epochs, 1
    cfg.train_dropout_prob, cfg.train_learning_rate, cfg.lr_plan, cfg.train_random_seed = 0.0, 1e-4, {}, 5
    cfg.result_path, cfg.deterministic = None, True
    cfg.feature_cache_gb, cfg.frame_cache_gb, cfg.num_workers = 1, 0, 0
    cfg.inference_module_name, cfg.feature_cache_path = module, path
    cfg.load_backbone_stage2, cfg.stage1_model_path = True, stage1
    return cfg


def _stage1(folder, flip_a_bit=False, crop_size=(5, 5)):
    """a stage-1 checkpoint as Basenet writes it: the backbone (the same one for every crop_size: it is built first, from the same
    seed) and fc_emb_1"""
    from din_amd.train_net_dynamic import build_model
    cfg = _cfg(None)
    cfg.crop_size = crop_size
    torch.manual_seed(11)
    model = build_model(cfg)
    if flip_a_bit:
        raw = model.backbone.features[10].weight.data.view(-1).view(torch.uint8)
        raw[1001] ^= 1
    path = os.path.join(folder, f"stage1_{int(flip_a_bit)}_{crop_size[0]}.pth")
    torch.save({"backbone_state_dict": model.backbone.state_dict(), "fc_emb_state_dict": model.fc_emb_1.state_dict()}, path)
    return path


def _run(cfg):
    """train_net(cfg) with the decodes, the trunk calls and the RoIAlign launches counted; the model's final state comes back too"""
    from din_amd import _lib, train_net_dynamic as TD, volleyball as V
    from din_amd.backbone.backbone import MyVGG16
    lib = _lib.load()
    seen = dict(decodes=0, trunks=0, roi=0, models=[])
    real_load, real_trunk, real_build = V.load_frame_u8, MyVGG16.forward_nhwc, TD.build_model
    roi_names = [n for n in _lib.SIGNATURES if "roi" in n]
    real_roi = {n: getattr(lib, n) for n in roi_names}

    def counting_load(path, size):
        seen["decodes"] += 1
        return real_load(path, size)

    def counting_trunk(self, x):
        seen["trunks"] += 1
        return real_trunk(self, x)

    def recording_build(c):
        model = real_build(c)
        load_stage1 = model.loadmodel

        def loadmodel(path):
            load_stage1(path)
            seen["initial"] = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}

        model.loadmodel = loadmodel
        seen["models"].append(model)
        return model

    def counting_roi(name):
        def call(*a):
            seen["roi"] += 1
            return real_roi[name](*a)
        return call

    V.load_frame_u8, MyVGG16.forward_nhwc, TD.build_model = counting_load, counting_trunk, recording_build
    for n in roi_names:
        setattr(lib, n, counting_roi(n))
    try:
        seen["infos"] = TD.train_net(cfg)
        torch.cuda.synchronize()
    finally:
        V.load_frame_u8, MyVGG16.forward_nhwc, TD.build_model = real_load, real_trunk, real_build
        for n in roi_names:
            setattr(lib, n, real_roi[n])
    seen["weights"] = {k: v.detach().cpu().clone() for k, v in seen.pop("models")[0].state_dict().items()}
    return seen


def _files(folder):
    return {n: open(os.path.join(folder, n), "rb").read() for n in sorted(os.listdir(folder))}


@pytest.fixture(scope="module")
def written(gpu, tmp_path_factory):
    """run A: two epochs with the path set, which writes train.dinfc and val.dinfc"""
    folder = str(tmp_path_factory.mktemp("feature_cache_files"))
    stage1 = _stage1(folder)
    cache_dir = os.path.join(folder, "cache")                     # (does not exist yet: the first save makes it)
    a = _run(_cfg(stage1, path=cache_dir))
    return dict(folder=folder, stage1=stage1, cache_dir=cache_dir, a=a, files=_files(cache_dir))


def _same_bits(a, b):
    """the keys whose tensors differ in any bit"""
    assert a.keys() == b.keys()
    return [k for k in a if not torch.equal(a[k].reshape(-1).view(torch.uint8), b[k].reshape(-1).view(torch.uint8))]


def test_the_first_run_writes_both_files_after_the_epoch_that_filled_them(written):
    from din_amd import feature_cache_file as FF
    a = written["a"]
    assert sorted(written["files"]) == ["train.dinfc", "val.dinfc"]
    assert a["decodes"] == TRAIN_FRAMES + VAL_FRAMES and a["trunks"] == 3 and a["roi"] >= 3        # epoch 1 only: one trunk call a step
    first, second = a["infos"]
    assert (first["train"]["feature_cache_loaded"], first["train"]["feature_cache_saved"]) == (0, TRAIN_FRAMES)
    assert (first["test"]["feature_cache_loaded"], first["test"]["feature_cache_saved"]) == (0, VAL_FRAMES)
    assert second["train"]["feature_cache_saved"] == 0 and second["test"]["feature_cache_saved"] == 0   # nothing came in: nothing written
    for name, frames in (("train.dinfc", TRAIN_FRAMES), ("val.dinfc", VAL_FRAMES)):
        header, ids, records = FF.read(os.path.join(written["cache_dir"], name))
        assert header["count"] == frames and (header["row_bytes"], header["box_bytes"], header["dtype"]) == (614400, 192, "fp32")
        assert sorted(ids.tolist()) == list(range(frames)) and records.shape == (frames, 614592)
        assert header["fingerprint"]["sequences"] == ([1] if name == "train.dinfc" else [4])


def test_a_second_run_starts_from_the_files_and_ends_with_the_same_weights(written):
    """run B: a fresh train_net call with run A's cfg decodes nothing and never runs the trunk, in either epoch, writes nothing, and its
    weights after two epochs are run A's to the last bit -- and those of a run that keeps its cache in memory only"""
    b = _run(_cfg(written["stage1"], path=written["cache_dir"]))
    assert (b["decodes"], b["trunks"], b["roi"]) == (0, 0, 0)
    for info in b["infos"]:
        assert (info["train"]["feature_cache_loaded"], info["train"]["feature_cache_saved"]) == (TRAIN_FRAMES, 0)
        assert (info["test"]["feature_cache_loaded"], info["test"]["feature_cache_saved"]) == (VAL_FRAMES, 0)
    assert _files(written["cache_dir"]) == written["files"]       # saved nothing, left no temporary file
    a = written["a"]
    assert _same_bits(a["weights"], b["weights"]) == []
    assert [(i["train"]["loss"], i["test"]["loss"]) for i in a["infos"]] == [(i["train"]["loss"], i["test"]["loss"]) for i in b["infos"]]
    plain = _run(_cfg(written["stage1"], path=None))
    assert plain["decodes"] == TRAIN_FRAMES + VAL_FRAMES and plain["trunks"] == 3
    assert all("feature_cache_loaded" not in i[part] and "feature_cache_saved" not in i[part] for i in plain["infos"] for part in ("train", "test"))
    assert _same_bits(a["weights"], plain["weights"]) == []
    moved = _same_bits(a["initial"], a["weights"])                # (two epochs did train something: the comparisons above compared it)
    assert moved and not any(k.startswith("backbone.") for k in moved)


def test_another_head_trains_from_the_same_files(written):
    """run C: the Actor-Transformer on the files the DIN run wrote"""
    c = _run(_cfg(written["stage1"], module="at_volleyball", path=written["cache_dir"], epochs=1))
    assert (c["decodes"], c["trunks"], c["roi"]) == (0, 0, 0)
    info = c["infos"][0]
    assert (info["train"]["feature_cache_loaded"], info["test"]["feature_cache_loaded"]) == (TRAIN_FRAMES, VAL_FRAMES)
    assert info["train"]["feature_cache_saved"] == 0 and info["test"]["feature_cache_saved"] == 0
    assert np.isfinite(info["train"]["loss"]) and _files(written["cache_dir"]) == written["files"]


def test_files_of_another_backbone_or_crop_size_are_refused_and_left_alone(written):
    flipped = _stage1(written["folder"], flip_a_bit=True)         # one bit of one backbone weight
    with pytest.raises(ValueError) as e:
        _run(_cfg(flipped, path=written["cache_dir"]))
    assert "another backbone_weights" in str(e.value) and os.path.join(written["cache_dir"], "train.dinfc") in str(e.value)
    assert _files(written["cache_dir"]) == written["files"]
    from din_amd import feature_cache_file as FF
    small = _stage1(written["folder"], crop_size=(3, 3))          # the same backbone under an fc_emb_1 for 3 x 3 crops
    same = [torch.load(p, map_location="cpu")["backbone_state_dict"] for p in (small, written["stage1"])]
    assert FF.weights_digest(same[0]) == FF.weights_digest(same[1])
    cfg = _cfg(small, path=written["cache_dir"])
    cfg.crop_size = (3, 3)
    with pytest.raises(ValueError) as e:
        _run(cfg)
    assert "another crop_size" in str(e.value) and "train.dinfc" in str(e.value)
    assert _files(written["cache_dir"]) == written["files"]


def test_a_file_with_other_boxes_for_a_frame_ends_the_pass_in_the_box_check(written, tmp_path):
    from din_amd import feature_cache_file as FF
    folder = str(tmp_path / "cache")
    os.makedirs(folder)
    for name in ("train.dinfc", "val.dinfc"):
        header, ids, records = FF.read(os.path.join(written["cache_dir"], name))
        records = np.array(records)
        if name == "train.dinfc":
            victim = int(ids[4])
            box = records[4, header["row_bytes"]:].view(np.float32)
            box[7] += 0.5                                         # one coordinate of one box of one frame
        FF.write(os.path.join(folder, name), header, ids, [records.reshape(-1)])
    with pytest.raises(RuntimeError) as e:
        _run(_cfg(written["stage1"], path=folder, epochs=1))
    assert "other boxes" in str(e.value) and f", {victim})" in str(e.value) and "1 rows" in str(e.value)


def test_the_build_tool_writes_the_files_a_training_run_writes(written, tmp_path):
    """tools/build_feature_cache.py: one forward-only pass over both splits, no head -- the same records, frame for frame, as the
    training run stored (its order of frames is its own shuffle's), under the same fingerprint; a second call computes nothing"""
    import sys
    from din_amd import feature_cache_file as FF, volleyball as V
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import build_feature_cache as tool
    finally:
        sys.path.pop(0)
    folder = str(tmp_path / "built")
    cfg = _cfg(written["stage1"], module="at_volleyball", path=folder)      # (batch size 1: the trunk sees a clip's three frames, as in run A)
    assert tool.build(cfg) == {"train": TRAIN_FRAMES, "val": VAL_FRAMES}
    for name in ("train.dinfc", "val.dinfc"):
        header, ids, records = FF.read(os.path.join(folder, name))
        theirs, their_ids, their_records = FF.read(os.path.join(written["cache_dir"], name))
        assert header["fingerprint"] == theirs["fingerprint"] and sorted(ids.tolist()) == sorted(their_ids.tolist())
        for i, fid in enumerate(ids.tolist()):
            assert records[i].tobytes() == their_records[their_ids.tolist().index(fid)].tobytes(), (name, fid)
    before, decodes, real_load = _files(folder), [], V.load_frame_u8
    V.load_frame_u8 = lambda path, size: (decodes.append(path), real_load(path, size))[1]
    try:
        assert tool.build(cfg) == {"train": TRAIN_FRAMES, "val": VAL_FRAMES}
    finally:
        V.load_frame_u8 = real_load
    assert decodes == [] and _files(folder) == before
