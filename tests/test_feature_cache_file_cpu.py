"""The box-feature cache on disk, host side (no GPU): the setting's default and its refusal, the file's write / read round trip and every
defect read() names, the atomic replace, and the fingerprint -- what it ignores, what it names, and that it does not depend on the order
a state_dict iterates in."""
import copy
import json
import os
import pickle
import struct
import types

import numpy as np
import pytest
import torch
import torch.utils.data as tud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "din-group-activity-recognition-benchmark_amd")

GEOMETRIES = {"fp32": (12 * 8 * 4 * 4, 192), "bf16": (12 * 8 * 4 * 2, 192)}      # (row_bytes, box_bytes): 12 boxes x 8 channels x 2 x 2
BLOCK = 4                                                                       # records per block handed to write()


def _cfg(_dataset="volleyball", **kw):
    from din_amd.config import Config
    cfg = Config(_dataset)
    cfg.backbone, cfg.image_size, cfg.out_size, cfg.emb_features = "vgg16", (96, 160), (3, 5), 512
    cfg.num_boxes, cfg.num_frames, cfg.num_before, cfg.num_after = 12, 3, 1, 1
    cfg.num_features_boxes, cfg.num_features_gcn = 64, 64
    cfg.num_features_relation, cfg.num_graph, cfg.gcn_layers, cfg.pos_threshold = 16, 4, 1, 0.5
    cfg.ST_kernel_size, cfg.sampling_ratio, cfg.beta_factor, cfg.train_backbone = [(3, 3)], [1], False, False
    cfg.training_stage, cfg.feature_cache_gb = 2, 1
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _volleyball(golden_dir, seqs=(1, 4), **kw):
    from din_amd import volleyball as V
    root = os.path.join(golden_dir, "dataset_tree", "volleyball")
    anns = V.volley_read_dataset(root, list(seqs))
    with open(os.path.join(root, "tracks_normalized.pkl"), "rb") as fh:
        tracks = pickle.load(fh)
    kw = {"num_before": 1, "num_after": 1, "frame_ids": True, **kw}
    return V.VolleyballDataset(anns, tracks, V.volley_all_frames(anns), root, (96, 160), (3, 5), "dynamic_volleyball", num_boxes=12, **kw)


def _meta(dtype="fp32", **kw):
    rb, bb = GEOMETRIES[dtype]
    return {"fingerprint": {"dataset_name": "volleyball", "digest": "0" * 64}, "row_bytes": rb, "box_bytes": bb, "dtype": dtype, **kw}


def _records(count, dtype="fp32", seed=0):
    rb, bb = GEOMETRIES[dtype]
    rng = np.random.default_rng(seed + count)
    return rng.integers(0, 256, size=(count, rb + bb), dtype=np.uint8), rng.permutation(10 * count + 7)[:count].astype(np.int64) * 3 + 11


def _blocks(records, block=BLOCK):
    for at in range(0, len(records), block):
        yield records[at:at + block].reshape(-1)


# ---- the setting ---------------------------------------------------------------------------------------------------------------------------
def test_default_is_off_and_changes_nothing(golden_dir):
    from din_amd import feature_cache as FE, frame_cache as FC
    from din_amd.config import Config
    for name in ("volleyball", "collective"):
        cfg = Config(name)
        assert cfg.feature_cache_path is None and cfg.feature_cache_gb == 0
        assert FE.path_refusal(cfg) is None and FE.refusal(cfg) is None
    cfg = _cfg(feature_cache_gb=0)
    ds = _volleyball(golden_dir, frame_ids=False)
    for real_tree in (False, True):                                 # every cache setting at its default: the plain loaders, as today
        for ld in FC.build_loaders(cfg, ds, ds, 2, None, "cpu", real_tree):
            assert type(ld) is tud.DataLoader and ld.num_workers == 0 and ld.collate_fn is tud.default_collate
    cfg.feature_cache_gb = 1                                        # the cache without the path: FeatureLoaders, and no file objects
    ids = _volleyball(golden_dir)
    tr, va = FC.build_loaders(cfg, ids, ids, 2, None, "cpu", True)
    assert type(tr) is FE.FeatureLoader and type(va) is FE.FeatureLoader
    assert FE.cache_files(cfg, None, tr, va) == {}                  # (the model is not even looked at)
    cfg.feature_cache_path = "/nowhere"                             # the path without caches behind the loaders (no dataset tree): nothing either
    plain = FC.build_loaders(cfg, ids, ids, 2, None, "cpu", False)
    assert FE.cache_files(cfg, None, *plain) == {}


@pytest.mark.parametrize("kw,words", [
    (dict(train_backbone=True), ("feature_cache_gb", "train_backbone")),
    (dict(frame_cache_gb=2), ("feature_cache_gb", "frame_cache_gb")),
    (dict(inference_module_name="dynamic_tce_volleyball"), ("feature_cache_gb", "dynamic_tce_volleyball", "context map")),
    (dict(_dataset="collective"), ("feature_cache_gb", "collective")),
    (dict(backbone="inv3", set_bn_eval=False), ("feature_cache_gb", "inv3", "set_bn_eval")),
    (dict(flip_prob=0.5), ("flip_prob", "feature_cache_gb")),
    (dict(color_jitter=(0.1, 0.1, 0.1)), ("color_jitter", "feature_cache_gb")),
    (dict(deterministic=True, train_backbone=True, feature_cache_gb=0), ("deterministic", "train_backbone")),
], ids=["train_backbone", "frame_cache_too", "tce", "collective", "inv3_batch_stats", "flip", "jitter", "deterministic"])
def test_existing_refusals_are_worded_as_before_with_and_without_the_path(kw, words, monkeypatch):
    from din_amd import frame_cache as FC, train_net_dynamic as TD
    monkeypatch.setattr(FC, "build_loaders", lambda *a, **k: pytest.fail("a loader was built before the refusal"))
    monkeypatch.setattr(TD.parallel, "init_from_env", lambda *a, **k: pytest.fail("the device was set up before the refusal"))
    said = []
    for p in (None, "/some/dir"):
        with pytest.raises(ValueError) as e:
            TD.train_net(_cfg(feature_cache_path=p, **kw))
        said.append(str(e.value))
    assert said[0] == said[1], "an existing refusal changed its words under feature_cache_path"
    for w in words:
        assert w in said[0], (w, said[0])
    assert "feature_cache_path" not in said[0]


@pytest.mark.parametrize("gb", [0, 0.0, None])
def test_a_path_without_the_cache_is_refused_before_any_loader_exists(gb, monkeypatch):
    from din_amd import frame_cache as FC, train_net_dynamic as TD
    monkeypatch.setattr(FC, "build_loaders", lambda *a, **k: pytest.fail("a loader was built before the refusal"))
    monkeypatch.setattr(TD.parallel, "init_from_env", lambda *a, **k: pytest.fail("the device was set up before the refusal"))
    with pytest.raises(ValueError) as e:
        TD.train_net(_cfg(feature_cache_gb=gb, feature_cache_path="/some/dir"))
    assert "feature_cache_path" in str(e.value) and "feature_cache_gb" in str(e.value) and "/some/dir" in str(e.value)


def test_stage1_trainer_does_not_read_the_field():
    assert "feature_cache_path" not in open(os.path.join(PKG, "train_net.py")).read()
    assert "feature_cache_path" in open(os.path.join(PKG, "train_net_dynamic.py")).read()


def test_file_names_per_rank():
    from din_amd import feature_cache_file as FF
    assert FF.file_name("train") == "train.dinfc" and FF.file_name("val", 0, 1) == "val.dinfc"
    assert FF.file_name("train", 3, 8) == "train.rank3of8.dinfc" and FF.file_name("val", 0, 2) == "val.rank0of2.dinfc"


# ---- write / read -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("count", [0, 1, BLOCK, 2 * BLOCK + 3], ids=["empty", "one", "one_block", "ragged_last_block"])
def test_round_trip(tmp_path, dtype, count):
    from din_amd import feature_cache_file as FF
    records, ids = _records(count, dtype)
    path = str(tmp_path / "train.dinfc")
    total = FF.write(path, _meta(dtype), ids, _blocks(records))
    assert total == os.path.getsize(path) and not os.path.exists(path + ".tmp")
    header, got_ids, got = FF.read(path)
    rb, bb = GEOMETRIES[dtype]
    assert header == {**_meta(dtype), "count": count}
    assert got_ids.dtype == np.int64 and got_ids.tolist() == ids.tolist()           # file order, not sorted
    assert got.shape == (count, rb + bb) and got.dtype == np.uint8 and np.array_equal(got, records)
    assert not got.flags.writeable
    if count:
        assert isinstance(got, np.memmap) and got.offset % FF.ALIGN == 0           # the records start on a 4096-byte boundary
        with pytest.raises(ValueError):
            got[0, 0] = 1
    raw = open(path, "rb").read()
    assert raw[:8] == FF.MAGIC == b"DINFCACH"
    magic, version, hlen = struct.unpack("<8sIQ", raw[:20])
    assert version == FF.VERSION and json.loads(raw[20:20 + hlen].decode("utf-8")) == header
    start = FF.records_offset(hlen, count)
    assert start % 4096 == 0 and len(raw) == start + count * (rb + bb) and raw[start:] == records.tobytes()
    assert np.frombuffer(raw[20 + hlen:20 + hlen + 8 * count], dtype=np.int64).tolist() == ids.tolist()


def test_blocks_of_any_size_give_the_same_file(tmp_path):
    from din_amd import feature_cache_file as FF
    records, ids = _records(11)
    files = []
    for block in (1, 4, 11, 64):
        path = str(tmp_path / f"b{block}.dinfc")
        FF.write(path, _meta(), ids, (bytes(b) for b in _blocks(records, block)))  # (bytes objects are blocks too)
        files.append(open(path, "rb").read())
    assert all(f == files[0] for f in files)


def _good_file(tmp_path, count=5):
    from din_amd import feature_cache_file as FF
    records, ids = _records(count)
    path = str(tmp_path / "val.dinfc")
    FF.write(path, _meta(), ids, _blocks(records))
    return path, open(path, "rb").read()


def _with_header(raw, change):
    """the file `raw` with its JSON header passed through `change` (the rest moved as the header's new length demands)"""
    from din_amd import feature_cache_file as FF
    _, _, hlen = struct.unpack("<8sIQ", raw[:20])
    header = json.loads(raw[20:20 + hlen])
    count, rec = header["count"], header["row_bytes"] + header["box_bytes"]
    old_start = FF.records_offset(hlen, count)
    text = change(header)
    text = text if isinstance(text, bytes) else json.dumps(text, sort_keys=True).encode()
    body = raw[:8] + struct.pack("<IQ", FF.VERSION, len(text)) + text + raw[20 + hlen:20 + hlen + 8 * count]
    return body + b"\0" * (FF.records_offset(len(text), count) - len(body)) + raw[old_start:old_start + count * rec]


def _set(**kw):
    return lambda h: {**h, **kw}


DEFECTS = {
    "wrong_magic": (lambda raw: b"DINFCACX" + raw[8:], ("magic",)),
    "empty_file": (lambda raw: b"", ("magic",)),
    "wrong_version": (lambda raw: raw[:8] + struct.pack("<I", 2) + raw[12:], ("version", "2")),
    "header_not_json": (lambda raw: _with_header(raw, lambda h: b"{not json"), ("header does not parse",)),
    "header_not_utf8": (lambda raw: _with_header(raw, lambda h: b"\xff\xfe{}"), ("header does not parse",)),
    "header_not_an_object": (lambda raw: _with_header(raw, lambda h: [1, 2]), ("header does not parse",)),
    "header_length_beyond_file": (lambda raw: raw[:12] + struct.pack("<Q", 1 << 40) + raw[20:], ("header does not parse",)),
    "shorter": (lambda raw: raw[:-1], ("shorter", "count")),
    "one_record_short": (lambda raw: raw[:-(sum(GEOMETRIES["fp32"]))], ("shorter", "count")),
    "longer": (lambda raw: raw + b"\0", ("longer", "count")),
    "count_says_more": (lambda raw: _with_header(raw, lambda h: {**h, "count": h["count"] + 1}), ("shorter", "count")),
    "row_bytes_not_16": (lambda raw: _with_header(raw, _set(row_bytes=GEOMETRIES["fp32"][0] + 8)), ("row_bytes", "multiple of 16")),
    "row_bytes_zero": (lambda raw: _with_header(raw, _set(row_bytes=0)), ("row_bytes", "multiple of 16")),
    "row_bytes_negative": (lambda raw: _with_header(raw, _set(row_bytes=-16)), ("row_bytes", "multiple of 16")),
    "row_bytes_a_string": (lambda raw: _with_header(raw, _set(row_bytes="1536")), ("row_bytes", "multiple of 16")),
    "box_bytes_not_16": (lambda raw: _with_header(raw, _set(box_bytes=200)), ("box_bytes", "multiple of 16")),
    "box_bytes_missing": (lambda raw: _with_header(raw, lambda h: {k: v for k, v in h.items() if k != "box_bytes"}), ("box_bytes", "multiple of 16")),
    "duplicate_ids": (None, ("duplicate ids",)),
}


@pytest.mark.parametrize("name", list(DEFECTS))
def test_read_names_every_defect(tmp_path, name):
    from din_amd import feature_cache_file as FF
    path, raw = _good_file(tmp_path)
    FF.read(path)                                                   # (the file the defects are made from is a good one)
    damage, words = DEFECTS[name]
    if name == "duplicate_ids":
        _, _, hlen = struct.unpack("<8sIQ", raw[:20])
        bad = raw[:20 + hlen + 8] + raw[20 + hlen:20 + hlen + 8] + raw[20 + hlen + 16:]       # the second id is the first again
    else:
        bad = damage(raw)
    with open(path, "wb") as fh:
        fh.write(bad)
    with pytest.raises(ValueError) as e:
        FF.read(path)
    for w in words:
        assert w in str(e.value), (w, str(e.value))
    assert path in str(e.value)


def test_write_refuses_what_read_would(tmp_path):
    from din_amd import feature_cache_file as FF
    records, ids = _records(3)
    path = str(tmp_path / "x.dinfc")
    for meta, what in ((_meta(row_bytes=24), "row_bytes"), (_meta(box_bytes=0), "box_bytes"), ({**_meta(), "dtype": "fp16"}, "dtype")):
        with pytest.raises(ValueError, match=what):
            FF.write(path, meta, ids, _blocks(records))
    with pytest.raises(ValueError, match="duplicate ids"):
        FF.write(path, _meta(), [5, 6, 5], _blocks(records))
    with pytest.raises(ValueError, match="2 records were handed over for 3 ids"):
        FF.write(path, _meta(), ids, _blocks(records[:2]))
    with pytest.raises(ValueError, match="whole number"):
        FF.write(path, _meta(), ids, [records.reshape(-1)[:-1]])
    assert os.listdir(str(tmp_path)) == []                          # nothing was left behind, neither a file nor a .tmp


def test_a_writer_that_raises_midway_leaves_the_old_file_and_no_tmp(tmp_path):
    from din_amd import feature_cache_file as FF
    path, raw = _good_file(tmp_path)
    records, ids = _records(9, seed=5)
    seen = []

    def failing():
        for i, b in enumerate(_blocks(records)):
            if i == 2:
                seen.append(os.path.exists(path + ".tmp"))          # (the new bytes were going to the temporary file)
                raise OSError("the device to host copy failed")
            yield b

    with pytest.raises(OSError, match="copy failed"):
        FF.write(path, _meta(), ids, failing())
    assert seen == [True]
    assert open(path, "rb").read() == raw and sorted(os.listdir(str(tmp_path))) == ["val.dinfc"]
    FF.write(path, _meta(), ids, _blocks(records))                  # and a writer that does not raise replaces it
    assert FF.read(path)[1].tolist() == ids.tolist() and sorted(os.listdir(str(tmp_path))) == ["val.dinfc"]


# ---- the fingerprint ----------------------------------------------------------------------------------------------------------------------
def _model(cfg, seed=3):
    from din_amd.train_net_dynamic import build_model
    torch.manual_seed(seed)
    return build_model(cfg)


@pytest.fixture(scope="module")
def vgg_model():
    return _model(_cfg())


def test_fingerprint_ignores_the_head_and_the_run(golden_dir, vgg_model):
    from din_amd import _lib, feature_cache_file as FF
    ds = _volleyball(golden_dir)
    cfg = _cfg()
    fp = FF.fingerprint(cfg, vgg_model, ds)
    assert tuple(fp) == FF.FIELDS + ("digest",) and len(fp["digest"]) == 64 and json.loads(json.dumps(fp)) == fp
    assert fp["din_abi_version"] == _lib.ABI_VERSION == 9 and fp["sequences"] == [1, 4] and fp["crop_size"] == [5, 5]
    assert fp["image_size"] == [96, 160] and fp["backbone_weights"] == FF.weights_digest(vgg_model.backbone.state_dict())
    for name in ("arg_volleyball", "at_volleyball"):
        other_cfg = _cfg(inference_module_name=name, train_learning_rate=3e-3, train_random_seed=77, batch_size=4, num_features_boxes=128,
                         num_features_gcn=128, max_epoch=7)
        other = _model(other_cfg, seed=99)                           # another head, other fc_emb_1 weights ...
        other.backbone.load_state_dict(vgg_model.backbone.state_dict())      # ... on the same stage-1 backbone
        assert type(other) is not type(vgg_model) and not torch.equal(other.fc_emb_1.weight, vgg_model.fc_emb_1.weight[:1])
        got = FF.fingerprint(other_cfg, other, ds)
        assert got == fp and FF.first_difference(fp, got) is None, name


CFG_FIELDS = [("dataset_name", "dataset_name", "collective"), ("image_size", "image_size", (96, 176)), ("out_size", "out_size", (3, 6)),
              ("crop_size", "crop_size", (3, 3)), ("emb_features", "emb_features", 256), ("num_boxes", "num_boxes", 11),
              ("backbone", "backbone", "inv3"), ("backbone_dtype", "backbone_dtype", "bf16"),
              ("feature_cache_dtype", "feature_cache_dtype", "bf16"), ("set_bn_eval", "set_bn_eval", True)]


@pytest.mark.parametrize("field,attr,value", CFG_FIELDS, ids=[f[0] for f in CFG_FIELDS])
def test_fingerprint_names_a_changed_setting(golden_dir, vgg_model, field, attr, value):
    from din_amd import feature_cache_file as FF
    ds = _volleyball(golden_dir)
    fp = FF.fingerprint(_cfg(), vgg_model, ds)
    other = FF.fingerprint(_cfg(**{attr: value}), vgg_model, ds)
    assert FF.first_difference(fp, other) == field and other["digest"] != fp["digest"]
    assert [k for k in FF.FIELDS if fp[k] != other[k]] == [field]   # and nothing else moved


def test_fingerprint_names_the_sequences_the_frame_table_and_the_abi(golden_dir, vgg_model, monkeypatch):
    from din_amd import _lib, feature_cache_file as FF
    cfg = _cfg()
    fp = FF.fingerprint(cfg, vgg_model, _volleyball(golden_dir))
    one = FF.fingerprint(cfg, vgg_model, _volleyball(golden_dir, seqs=(1,)))
    assert FF.first_difference(fp, one) == "sequences" and one["sequences"] == [1]
    swapped = FF.fingerprint(cfg, vgg_model, _volleyball(golden_dir, seqs=(4, 1)))
    assert swapped["sequences"] == [4, 1] and FF.first_difference(fp, swapped) == "sequences"       # as the dataset holds it
    # the same sequences with another window of frames around each clip: frame ids then index another table
    wider = FF.fingerprint(cfg, vgg_model, _volleyball(golden_dir, num_before=2))
    assert FF.first_difference(fp, wider) == "frames" and wider["sequences"] == fp["sequences"]
    real = _lib.load()
    monkeypatch.setattr(_lib, "load", lambda: types.SimpleNamespace(din_abi_version=lambda: real.din_abi_version() + 1))
    assert FF.first_difference(fp, FF.fingerprint(cfg, vgg_model, _volleyball(golden_dir))) == "din_abi_version"


def _small_backbone():
    torch.manual_seed(1)
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.BatchNorm2d(4), torch.nn.Conv2d(4, 4, 1))
    net[1].running_mean.uniform_(-1, 1)
    net[1].running_var.uniform_(0.5, 2)
    return net


@pytest.mark.parametrize("key", ["0.weight", "2.bias", "1.weight", "1.running_mean", "1.running_var", "1.num_batches_tracked"])
def test_one_flipped_bit_in_a_weight_or_a_running_statistic_changes_the_fingerprint(golden_dir, key):
    from din_amd import feature_cache_file as FF
    ds, cfg = _volleyball(golden_dir), _cfg()
    net = _small_backbone()
    fp = FF.fingerprint(cfg, types.SimpleNamespace(backbone=net), ds)
    assert fp == FF.fingerprint(cfg, types.SimpleNamespace(backbone=copy.deepcopy(net)), ds)
    flipped = copy.deepcopy(net)
    t = flipped.state_dict()[key]                                   # (state_dict tensors share storage with the module's)
    raw = t.view(-1).view(torch.uint8)
    raw[raw.numel() // 2] ^= 1                                      # the lowest bit of one byte in the middle
    other = FF.fingerprint(cfg, types.SimpleNamespace(backbone=flipped), ds)
    assert FF.first_difference(fp, other) == "backbone_weights" and [k for k in FF.FIELDS if fp[k] != other[k]] == ["backbone_weights"]


def test_weights_digest_depends_on_keys_dtypes_shapes_and_bytes_not_on_order():
    from din_amd import feature_cache_file as FF
    sd = _small_backbone().state_dict()
    want = FF.weights_digest(sd)
    backwards = {k: sd[k] for k in reversed(list(sd))}
    assert list(backwards) != list(sd) and FF.weights_digest(backwards) == want
    assert FF.weights_digest({k: v.clone() for k, v in sd.items()}) == want
    renamed = {("x" + k if k == "0.bias" else k): v for k, v in sd.items()}
    reshaped = {k: (v.reshape(4, 3, 9) if k == "0.weight" else v) for k, v in sd.items()}
    retyped = {k: (v.view(torch.int32) if k == "2.bias" else v) for k, v in sd.items()}
    assert len({want, FF.weights_digest(renamed), FF.weights_digest(reshaped), FF.weights_digest(retyped)}) == 4
    assert FF.weights_digest({"a": torch.zeros(0)}) != FF.weights_digest({"a": torch.zeros(0, dtype=torch.int64)})


def test_a_foreign_fingerprint_is_named_by_its_first_differing_field():
    from din_amd import feature_cache_file as FF
    a = {k: i for i, k in enumerate(FF.FIELDS)}
    a["digest"] = "d"
    assert FF.first_difference(a, dict(a)) is None
    assert FF.first_difference(a, {**a, "crop_size": -1, "backbone_weights": -1}) == "crop_size"
    assert FF.first_difference(a, {**a, "digest": "e"}) == "digest"
    assert FF.first_difference(a, {k: v for k, v in a.items() if k != "frames"}) == "frames"


# ---- the C ABI did not move ---------------------------------------------------------------------------------------------------------------
def test_the_abi_is_where_it_was():
    from din_amd import _lib
    text = open(_lib.HEADER_PATH).read()
    assert len(_lib.header_symbols()) == 122 and set(_lib.header_symbols()) == set(_lib.SIGNATURES)
    assert "#define DIN_ABI_VERSION 9 " in text and _lib.ABI_VERSION == 9
    assert os.listdir(os.path.dirname(_lib.HEADER_PATH)) == ["din_hip.h"]
    assert "(122 entry points" in open(os.path.join(ROOT, "README.md")).read()


def test_the_module_needs_no_gpu_and_holds_no_pickle():
    src = open(os.path.join(PKG, "feature_cache_file.py")).read()
    assert "import pickle" not in src and "torch.load" not in src and "torch.save" not in src and "eval(" not in src
    assert "cuda" not in src
