"""Mirrored box features without a GPU (cfg.feature_cache_flip, cfg.test_flip): the settings and their refusals, the pair rule on
SlotTables, which frames count as resident, the feed's draws, the arithmetic of test-time flipping, the files' orientation, the ABI."""
import hashlib
import json
import os
import struct
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RB, BB = 1536, 192


def _cfg(dataset="volleyball", **kw):
    from din_amd.config import Config
    cfg = Config(dataset)
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


# ---- the settings ------------------------------------------------------------------------------------------------------------------------
def test_the_three_defaults():
    from din_amd import feature_cache as FE, frame_cache as FC
    for dataset in ("volleyball", "collective"):
        cfg = _cfg(dataset)
        assert cfg.feature_cache_flip is False and cfg.test_flip is False and cfg.flip_prob == 0.0 and isinstance(cfg.flip_prob, float)
        assert FE.flip_cache_refusal(cfg) is None and FC.flip_refusal(cfg) is None
    doc = __import__("din_amd.config", fromlist=["x"]).__doc__
    assert "feature_cache_flip" in doc and "test_flip" in doc


# what frame_cache.flip_refusal answered before the settings existed, for the parameter sets of tests/test_flip_cpu.py
AS_BEFORE = {
    "negative": "flip_prob = -0.1: the probability of mirroring a clip is a real number in [0, 1]",
    "above_one": "flip_prob = 1.5: the probability of mirroring a clip is a real number in [0, 1]",
    "nan": "flip_prob = nan: the probability of mirroring a clip is a real number in [0, 1]",
    "bool": "flip_prob = True: the probability of mirroring a clip is a real number in [0, 1]",
    "string": "flip_prob = '0.5': the probability of mirroring a clip is a real number in [0, 1]",
    "feature_cache": "flip_prob = 0.5: feature_cache_gb = 1 caches the box features of the unmirrored frame; they cannot serve a mirrored one",
    "five_activities": "flip_prob = 0.5: a mirrored volleyball clip swaps the team side of its label among the 8 activities of "
                       "volleyball.ACTIVITIES; num_activities is 5",
}


def test_with_the_defaults_every_refusal_answers_as_before():
    from din_amd import feature_cache as FE, frame_cache as FC
    from tests.test_flip_cpu import REFUSED, REFUSED_IDS
    assert sorted(REFUSED_IDS) == sorted(AS_BEFORE)
    for (kw, _words), name in zip(REFUSED, REFUSED_IDS):
        cfg = _cfg(**kw)
        assert FC.flip_refusal(cfg) == AS_BEFORE[name], name
        assert FE.flip_cache_refusal(cfg) is None and FC.jitter_refusal(cfg) is None and FE.path_refusal(cfg) is None
        assert FE.refusal(cfg) is None
    for p in (0, 0.5, 1, 1.0):
        assert FC.flip_refusal(_cfg(flip_prob=p)) is None
    jitter = FC.jitter_refusal(_cfg(color_jitter=(0.1, 0.2, 0.3), feature_cache_gb=1, feature_cache_flip=True))
    assert jitter == ("color_jitter = (0.1, 0.2, 0.3): feature_cache_gb = 1 caches the box features of the frame as decoded; they cannot "
                      "serve a jittered one")                        # the mirror cache does not lift the jitter's refusal


def test_flip_refusal_is_lifted_by_feature_cache_flip_and_by_nothing_else():
    from din_amd import frame_cache as FC
    assert FC.flip_refusal(_cfg(flip_prob=0.5, feature_cache_gb=1, feature_cache_flip=True)) is None
    for other in (False, None, 1, "yes"):
        assert FC.flip_refusal(_cfg(flip_prob=0.5, feature_cache_gb=1, feature_cache_flip=other)) == AS_BEFORE["feature_cache"]
    why = FC.flip_refusal(_cfg(flip_prob=0.5, feature_cache_gb=1, feature_cache_flip=True, num_activities=5))
    assert why == AS_BEFORE["five_activities"]                       # the label map is still needed


NEW_REFUSALS = [
    (dict(feature_cache_flip=1, feature_cache_gb=1), ("feature_cache_flip", "True or False")),
    (dict(feature_cache_flip="yes", feature_cache_gb=1), ("feature_cache_flip", "True or False")),
    (dict(test_flip=None), ("test_flip", "True or False")),
    (dict(test_flip=0.5), ("test_flip", "True or False")),
    (dict(feature_cache_flip=True), ("feature_cache_flip", "feature_cache_gb")),
    (dict(feature_cache_flip=True, feature_cache_gb=0.0), ("feature_cache_flip", "feature_cache_gb")),
    (dict(test_flip=True, feature_cache_gb=1), ("test_flip", "feature_cache_flip", "feature_cache_gb")),
    (dict(test_flip=True, num_activities=5), ("test_flip", "num_activities")),
    (dict(test_flip=True, num_activities=5, feature_cache_gb=1, feature_cache_flip=True), ("test_flip", "num_activities")),
]
NEW_IDS = ["flip_an_int", "flip_a_string", "test_flip_none", "test_flip_a_float", "flip_without_the_cache", "flip_with_zero_gb",
           "test_flip_with_the_cache_alone", "test_flip_five_activities", "test_flip_five_activities_cached"]


@pytest.mark.parametrize("kw,words", NEW_REFUSALS, ids=NEW_IDS)
def test_train_net_refuses_before_any_loader_is_built(kw, words, monkeypatch):
    """each new refusal is a ValueError naming the setting, raised before a process group, a loader or the device is touched"""
    from din_amd import feature_cache as FE, frame_cache as FC, train_net_dynamic as TD
    monkeypatch.setattr(FC, "build_loaders", lambda *a, **k: pytest.fail("a loader was built before the refusal"))
    monkeypatch.setattr(TD.parallel, "init_from_env", lambda *a, **k: pytest.fail("the device was set up before the refusal"))
    cfg = _cfg(training_stage=2, **kw)
    with pytest.raises(ValueError) as e:
        TD.train_net(cfg)
    assert str(e.value) == FE.flip_cache_refusal(cfg)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_accepted_combinations_are_not_refused():
    from din_amd import feature_cache as FE
    for kw in (dict(test_flip=True), dict(feature_cache_flip=True, feature_cache_gb=1), dict(test_flip=True, feature_cache_gb=1, feature_cache_flip=True),
               dict(feature_cache_flip=True, feature_cache_gb=0.5, flip_prob=0.5, test_flip=True)):
        assert FE.flip_cache_refusal(_cfg(**kw)) is None, kw
    assert FE.flip_cache_refusal(_cfg("collective", test_flip=True, num_activities=5)) is None      # (the collective labels have no side)


@pytest.mark.parametrize("value", [True, 1, "on"])
def test_stage1_trainer_refuses_test_flip(value, monkeypatch):
    from din_amd import frame_cache as FC, train_net as T1
    monkeypatch.setattr(FC, "build_loaders", lambda *a, **k: pytest.fail("a loader was built before the refusal"))
    monkeypatch.setattr(T1.parallel, "init_from_env", lambda *a, **k: pytest.fail("the device was set up before the refusal"))
    with pytest.raises(ValueError) as e:
        T1.train_net(_cfg(training_stage=1, test_flip=value))
    assert "test_flip" in str(e.value) and "stage" in str(e.value)


def test_which_datasets_get_a_mirror_cache():
    """the training set iff flip_prob > 0, the validation set iff test_flip; none without feature_cache_flip"""
    from din_amd import feature_cache as FE
    for flip_prob, test_flip in ((0.0, False), (0.5, False), (0.0, True), (1.0, True)):
        cfg = _cfg(feature_cache_gb=1, feature_cache_flip=True, flip_prob=flip_prob, test_flip=test_flip, crop_size=(5, 5), emb_features=8)
        tr, va = FE.feature_loaders(cfg, "TL", "VL", "TS", "VS", "cpu")
        assert (tr.mirror is not None, va.mirror is not None) == (flip_prob > 0, test_flip)
        for ld in (tr, va):
            assert ld.cache.orientation == "plain"
            if ld.mirror is not None:
                m, c = ld.mirror, ld.cache
                assert m.orientation == "mirrored" and (m.row_bytes, m.box_bytes, m.dtype, m.table.max_slots) == (c.row_bytes, c.box_bytes, c.dtype, c.table.max_slots)
        cfg.feature_cache_flip = False
        cfg.flip_prob = 0.0
        tr, va = FE.feature_loaders(cfg, "TL", "VL", "TS", "VS", "cpu")
        assert tr.mirror is None and va.mirror is None


# ---- fill and serve rules ----------------------------------------------------------------------------------------------------------------
def test_pair_rule_on_slot_tables():
    """a frame goes into every table that lacks it or into none: three slots each take three pairs; three and two slots take two pairs
    and leave the odd slot empty; a refused slab in one table keeps the frame out of the other"""
    from din_amd.feature_cache import insert_pair
    from din_amd.frame_cache import SlotTable
    a, b = SlotTable(100, 3 * 112, 2), SlotTable(100, 3 * 112, 2)
    assert a.max_slots == b.max_slots == 3
    assert [insert_pair([a, b], f) for f in (10, 11, 12, 13)] == [{0: 0, 1: 0}, {0: 1, 1: 1}, {0: 2, 1: 2}, {}]
    assert list(a.slot_of) == list(b.slot_of) == [10, 11, 12] and a.inserted == b.inserted == 3
    assert insert_pair([a, b], 11) == {} and a.hits == b.hits == 0                # held by both: nothing to do, not a hit
    a, b = SlotTable(100, 3 * 112, 2), SlotTable(100, 2 * 112, 2)
    assert [bool(insert_pair([a, b], f)) for f in (10, 11, 12)] == [True, True, False]
    assert list(a.slot_of) == list(b.slot_of) == [10, 11] and not a.full and b.full
    a, b = SlotTable(100, 8 * 112, 2), SlotTable(100, 8 * 112, 2)
    asked = []
    refuse_second_slab = lambda n: (asked.append(n), len(asked) < 2)[1]
    assert [bool(insert_pair([a, b], f, [lambda n: True, refuse_second_slab])) for f in (1, 2, 3, 4)] == [True, True, False, False]
    assert list(a.slot_of) == list(b.slot_of) == [1, 2] and b.frozen and not a.frozen
    # a table that holds the frame already keeps it; the other takes it in (a file that was loaded for one orientation only)
    a, b = SlotTable(100, 3 * 112, 2), SlotTable(100, 3 * 112, 2)
    a.insert(7)
    assert insert_pair([a, b], 7) == {1: 0} and 7 in b.slot_of and a.inserted == 1
    assert SlotTable(100, 0, 2).reserve() is False


class _FakeCache:
    def __init__(self, ids):
        self.ids, self.table = ids, types.SimpleNamespace(inserted=0, stride=RB + BB)

    def load(self, path, meta):
        self.table.inserted += len(self.ids)
        return list(self.ids)


def test_resident_is_set_only_for_frames_both_caches_hold(tmp_path):
    from din_amd import feature_cache as FE
    for name in ("train.dinfc", "train.flip.dinfc"):
        (tmp_path / name).write_bytes(b"")
    dataset = types.SimpleNamespace(resident=torch.zeros(16, dtype=torch.uint8))
    loader = FE.FeatureLoader("L", _FakeCache([1, 2, 3, 4]), dataset, _FakeCache([3, 4, 5]))
    said = []
    f = FE.CacheFile(loader, str(tmp_path / "train.dinfc"), {}, said.append, str(tmp_path / "train.flip.dinfc"))
    assert f.load() == 4 and (f.loaded, f.flip_loaded) == (4, 3) and f.inserted == 7
    assert dataset.resident.nonzero().reshape(-1).tolist() == [3, 4]
    assert len(said) == 2 and "train.dinfc: 4 frames" in said[0] and "train.flip.dinfc: 3 frames" in said[1]
    assert f.save_if_grown(7) == 0 and f.flip_written == 0           # a pass that only read writes neither file
    plain = FE.FeatureLoader("L", _FakeCache([]), dataset)
    assert FE.CacheFile(plain, "p", {}, said.append, "q").flip_path is None


def test_feed_draws_the_clips_flip_plan_draws(monkeypatch):
    """FeatureFeed with the pass's augmentation: the flags of every batch are FlipPlan's for the same seed / rank / epoch (one stream,
    drawn once per batch), the labels' launch receives them repeated over T before the batch is handed out, a batch without a drawn
    clip is handed out without orientation flags and without that launch"""
    from din_amd import feature_cache as FE, frame_cache as FC
    monkeypatch.setattr(FE, "DeviceFeed", lambda host, device: host)
    launches = []
    monkeypatch.setattr(FC.EpochFlips, "mirror_labels", lambda self, labels, flags: launches.append(flags.clone()))
    T, sizes = 3, (4, 4, 1, 4, 2)
    batches, at = [], 0
    for n in sizes:
        ids = torch.arange(at, at + n * T).reshape(n, T)
        batches.append((ids, torch.zeros((0, 3, 2, 2), dtype=torch.uint8), torch.zeros(0, dtype=torch.int64), torch.zeros(n, T, 2, 4), torch.zeros(n, T, 2),
                        torch.zeros(n, T, dtype=torch.int64)))
        at += n * T
    cache = types.SimpleNamespace(_upload=lambda *tables: [torch.as_tensor(np.asarray(t)) for t in tables])
    for seed, rank, epoch in ((5, 0, 1), (5, 1, 1), (9, 0, 4)):
        cfg = _cfg(flip_prob=0.5, train_random_seed=seed, feature_cache_gb=1, feature_cache_flip=True)
        augment = FC.augmentations(cfg, epoch, rank)
        want = FC.FlipPlan(0.5, seed, rank).epoch(epoch)
        del launches[:]
        feed = FE.FeatureFeed(batches, "cpu", cache, types.SimpleNamespace(resident=torch.zeros(64, dtype=torch.uint8)), augment, "MIRROR")
        expected_launches = 0
        for (refs, *_labels), n in zip(feed, sizes):
            flags = want.draw(n)
            assert refs.mirror == "MIRROR" and refs.shape[:2] == (n, T)
            if flags.any():
                expected_launches += 1
                assert refs.flipped.tolist() == np.repeat(flags, T).reshape(n, T).tolist()
                assert launches[-1].tolist() == np.repeat(flags, T).astype(np.int64).tolist()
            else:
                assert refs.flipped is None
            assert len(launches) == expected_launches
        assert augment.stats() == {"flipped_clips": want.flipped} and want.flipped > 0


def test_feed_marks_resident_what_the_model_call_reports_as_held_by_both(monkeypatch):
    """`FrameRefs.inserted` (with a mirror cache: the frames both caches hold since the call) is what the feed writes into
    `dataset.resident` when the consumer comes back for the next batch -- nothing else, and nothing for a batch that stored nothing"""
    from din_amd import feature_cache as FE
    monkeypatch.setattr(FE, "DeviceFeed", lambda host, device: host)
    none = (torch.zeros((0, 3, 2, 2), dtype=torch.uint8), torch.zeros(0, dtype=torch.int64))
    batches = [(torch.arange(k * 6, k * 6 + 6).reshape(2, 3), *none, torch.zeros(2, 3, 2, 4)) for k in range(3)]
    dataset = types.SimpleNamespace(resident=torch.zeros(32, dtype=torch.uint8))
    reported = [[0, 1, 2], [], [13, 17]]                             # (a full cache keeps some frames of a batch and not others)
    for k, (refs, _boxes) in enumerate(FE.FeatureFeed(batches, "cpu", "CACHE", dataset, None, "MIRROR")):
        assert dataset.resident.nonzero().reshape(-1).tolist() == sorted(f for r in reported[:k] for f in r)
        assert refs.cache == "CACHE" and refs.mirror == "MIRROR" and refs.flipped is None and refs.inserted == []
        refs.inserted.extend(reported[k])                            # what infer_model._cached_crops does during the model call
    assert dataset.resident.nonzero().reshape(-1).tolist() == [0, 1, 2, 13, 17]


def test_loader_without_a_mirror_cache_still_refuses_a_flip_plan(monkeypatch):
    from din_amd import feature_cache as FE, frame_cache as FC
    monkeypatch.setattr(FE, "FeatureFeed", lambda *a: ("features",) + a)
    augment = FC.PassAugment(FC.FlipPlan(0.5, 0, 0).epoch(1))
    with pytest.raises(ValueError, match="flip augmentation"):
        FE.FeatureLoader("L", "C", "D").feed("cpu", augment)
    assert FE.FeatureLoader("L", "C", "D").feed("cpu") == ("features", "L", "cpu", "C", "D")
    assert FE.FeatureLoader("L", "C", "D", "M").feed("cpu", augment) == ("features", "L", "cpu", "C", "D", augment, "M")
    assert FE.FeatureLoader("L", "C", "D", "M").feed("cpu") == ("features", "L", "cpu", "C", "D", None, "M")
    with pytest.raises(ValueError, match="colour jitter"):
        FE.FeatureLoader("L", "C", "D", "M").feed("cpu", FC.PassAugment(None, FC.JitterPlan((0.1, 0.1, 0.1), 0, 0).epoch(1)))


def test_frame_refs_carry_the_orientation_through_reshape_and_mirrored():
    from din_amd.feature_cache import FrameRefs
    ids = np.arange(18).reshape(2, 9)
    flipped = np.repeat([False, True], 9).reshape(2, 9)
    none = torch.zeros((0, 3, 4, 4), dtype=torch.uint8)
    refs = FrameRefs(ids, none, [], "C", None, "M", flipped, "BOXES")
    folded = refs.reshape(6, 3, 3, 4, 4)                             # ARG_volleyball's evaluation fold
    assert folded.flipped.tolist() == np.repeat([False, True], 9).reshape(6, 3).tolist() and folded.mirror == "M" and folded.plain_boxes == "BOXES"
    assert folded.inserted is refs.inserted
    other = refs.mirrored("B2")
    assert other.flipped.tolist() == (~flipped).tolist() and other.plain_boxes == "B2" and other.inserted is refs.inserted
    assert FrameRefs(ids, none, [], "C", None, "M").mirrored("B").flipped.all()
    with pytest.raises(ValueError):
        FrameRefs(ids, none, [], "C", None, None, flipped)           # mirrored rows without a mirror cache
    with pytest.raises(ValueError):
        FrameRefs(ids, none, [], "C", None, "M", flipped[:1])
    plain = FrameRefs(ids, none, [], "C")
    assert plain.mirror is None and plain.flipped is None and plain.reshape(6, 3, 3, 4, 4).flipped is None


# ---- test-time flipping ------------------------------------------------------------------------------------------------------------------
def test_flip_activities_is_an_involution():
    from din_amd.volleyball import ACTIVITIES, FLIP_ACTIVITIES
    assert sorted(FLIP_ACTIVITIES) == list(range(len(ACTIVITIES)))
    assert [FLIP_ACTIVITIES[FLIP_ACTIVITIES[a]] for a in range(len(ACTIVITIES))] == list(range(len(ACTIVITIES)))
    assert all(FLIP_ACTIVITIES[a] != a for a in range(len(ACTIVITIES)))


def test_combination_formula_against_float64():
    """0.5 * (s + s_m[:, map]) on scores made by hand: clip 0 is an r_spike whose mirror image scores l-spike (column 5) highest; without
    the map the average would elect column 5 or tie, with it column 1 wins.  Clip 1 uses a map that is no involution, so that gathering
    (s_m[:, map]) and scattering (s_m[:, inverse]) give different winners."""
    from din_amd.train_net_dynamic import combine_flip_scores
    from din_amd.volleyball import FLIP_ACTIVITIES
    s = torch.tensor([[0.0, 2.0, 0.5, 0.0, 0.0, 1.0, 0.0, 0.0]])
    m = torch.tensor([[0.0, 0.0, 0.0, 0.0, 0.0, 5.0, 0.5, 0.0]])
    got = combine_flip_scores(s, m, FLIP_ACTIVITIES)
    want = 0.5 * (s.double().numpy() + m.double().numpy()[:, FLIP_ACTIVITIES])
    assert got.dtype == torch.float32 and np.array_equal(got.double().numpy(), want)     # (halves and sums of these values are exact)
    assert int(got.argmax(1)) == 1 and int((0.5 * (s + m)).argmax(1)) == 5               # the missing permutation elects l-spike
    assert np.array_equal(combine_flip_scores(s, m, None).numpy(), (0.5 * (s + m)).numpy())          # collective: the identity
    cycle = [1, 2, 0]                                                # column map[a] of the mirrored scores is the evidence for class a
    s3, m3 = torch.tensor([[0.0, 0.0, 0.0]]), torch.tensor([[0.0, 9.0, 1.0]])
    got = combine_flip_scores(s3, m3, cycle)
    assert got.tolist() == [[4.5, 0.5, 0.0]] and int(got.argmax(1)) == 0                 # m3[1] counts for class 0 (map[0] = 1)
    scattered = torch.zeros(1, 3)
    scattered[:, cycle] = m3                                         # the wrong direction puts it on class 2
    assert int((0.5 * (s3 + scattered)).argmax(1)) == 2
    g = torch.Generator().manual_seed(0)
    a, b = torch.randn((16, 8), generator=g), torch.randn((16, 8), generator=g)
    want = (0.5 * (a.double() + b.double()[:, FLIP_ACTIVITIES])).numpy()
    got = combine_flip_scores(a, b, FLIP_ACTIVITIES).double().numpy()
    assert np.abs(got - want).max() <= 2.0 ** -24 * np.abs(want).max() * 2       # one fp32 rounding of the sum (the halving is exact)
    half = combine_flip_scores(a.to(torch.bfloat16), b.to(torch.bfloat16), FLIP_ACTIVITIES)
    assert half.dtype == torch.float32                               # averaged in fp32 whatever the model's scores are


# ---- files -------------------------------------------------------------------------------------------------------------------------------
def _meta(**kw):
    return {"fingerprint": {"dataset_name": "volleyball", "digest": "0" * 64}, "row_bytes": RB, "box_bytes": BB, "dtype": "fp32", **kw}


def test_file_names_of_the_mirror_cache():
    from din_amd import feature_cache_file as FF
    assert FF.flip_file_name("train") == "train.flip.dinfc" and FF.flip_file_name("val", 0, 1) == "val.flip.dinfc"
    assert FF.flip_file_name("train", 3, 8) == "train.flip.rank3of8.dinfc"
    assert FF.file_name("train") == "train.dinfc" and FF.file_name("train", 3, 8) == "train.rank3of8.dinfc"


def test_round_trip_of_both_orientations_and_a_plain_file_is_what_it_was(tmp_path):
    from din_amd import feature_cache_file as FF
    rng = np.random.default_rng(1)
    records, ids = rng.integers(0, 256, size=(5, RB + BB), dtype=np.uint8), np.asarray([4, 9, 2, 30, 11], dtype=np.int64)
    plain, mirror = str(tmp_path / "train.dinfc"), str(tmp_path / "train.flip.dinfc")
    FF.write(plain, _meta(), ids, [records.reshape(-1)])
    FF.write(mirror, _meta(orientation="mirrored"), ids, [records[::-1].reshape(-1)])
    header, got_ids, got = FF.read(plain)
    assert header == {**_meta(), "count": 5} and "orientation" not in header and np.array_equal(got, records) and got_ids.tolist() == ids.tolist()
    header_m, got_ids, got = FF.read(mirror)
    assert header_m == {**_meta(), "orientation": "mirrored", "count": 5} and np.array_equal(got, records[::-1])
    # a plain file, byte for byte, from the layout's own words: the format, the version and the header's keys did not move
    text = json.dumps({**_meta(), "count": 5}, sort_keys=True).encode()
    start = (20 + len(text) + 40 + FF.ALIGN - 1) // FF.ALIGN * FF.ALIGN
    want = struct.pack("<8sIQ", b"DINFCACH", 1, len(text)) + text + ids.tobytes()
    want += b"\0" * (start - len(want)) + records.tobytes()
    assert open(plain, "rb").read() == want
    assert FF.write(str(tmp_path / "again.dinfc"), _meta(orientation="plain"), ids, [records.reshape(-1)]) == len(want)
    assert open(str(tmp_path / "again.dinfc"), "rb").read() == want
    assert FF.VERSION == 1 and "orientation" not in FF.FIELDS


def test_a_renamed_file_is_refused_at_load(tmp_path):
    """a mirror cache's file offered to the plain cache, and the reverse: ValueError saying so, before anything is inserted"""
    from din_amd import feature_cache_file as FF
    from din_amd.feature_cache import FeatureCache
    records, ids = np.zeros((2, RB + BB), dtype=np.uint8), np.asarray([1, 2], dtype=np.int64)
    plain, mirror = str(tmp_path / "a.dinfc"), str(tmp_path / "b.dinfc")
    FF.write(plain, _meta(), ids, [records.reshape(-1)])
    FF.write(mirror, _meta(orientation="mirrored"), ids, [records.reshape(-1)])
    fp = _meta()["fingerprint"]
    for orientation, path, theirs in (("plain", mirror, "mirrored"), ("mirrored", plain, "plain")):
        cache = FeatureCache("cpu", RB, BB, 1 << 20, orientation=orientation)
        with pytest.raises(ValueError) as e:
            cache.load(path, fp)
        assert f"the {theirs} frames" in str(e.value) and f"the {orientation} ones" in str(e.value) and path in str(e.value)
        assert cache.table.inserted == 0 and not cache.slabs
        assert cache.file_meta(fp) == (_meta() if orientation == "plain" else _meta(orientation="mirrored"))
    with pytest.raises(ValueError):
        FeatureCache("cpu", RB, BB, 1 << 20, orientation="upside_down")


PARENT_DIGEST = "1eed767ea904e1a48bc2cc8fa31ce5d9832e2eceee26660990a32d7cc8414728"


def test_plain_fingerprint_is_unchanged(golden_dir):
    """the fingerprint of tests/test_feature_cache_file_cpu.py's seeded VGG16 model over the golden tree is, digest for digest, what the
    commit before the mirror cache computed for these inputs (PARENT_DIGEST and its two sub-digests were taken from that commit); the
    new settings are not part of it: both orientations of a run carry the same fingerprint, the orientation lives beside it"""
    from din_amd import feature_cache_file as FF
    from tests.test_feature_cache_file_cpu import _cfg as file_cfg, _model, _volleyball
    assert FF.FIELDS == ("dataset_name", "sequences", "frames", "image_size", "out_size", "crop_size", "emb_features", "num_boxes", "backbone",
                         "backbone_dtype", "feature_cache_dtype", "set_bn_eval", "din_abi_version", "backbone_weights")
    ds, model = _volleyball(golden_dir), _model(file_cfg())
    fp = FF.fingerprint(file_cfg(), model, ds)
    fields = {k: fp[k] for k in FF.FIELDS}
    assert tuple(fp) == FF.FIELDS + ("digest",)
    assert fp["frames"] == "c97eaad4dd4c0ee231ae8d9f117fa15731113da6169b9b7e7cb5a448aed3ca53"
    assert fp["backbone_weights"] == "d4d49158cf457ec0ec2ea5cee58b30cd7786e1d5e2bf39dc0ac2ce3aff56be92"
    assert fp["digest"] == PARENT_DIGEST
    assert fp["digest"] == hashlib.sha256(json.dumps(fields, sort_keys=True).encode("utf-8")).hexdigest()
    assert FF.fingerprint(file_cfg(feature_cache_flip=True, flip_prob=0.5, test_flip=True), model, ds) == fp


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_no_entry_point_was_added():
    from din_amd import _lib
    assert len(_lib.header_symbols()) == 122 and set(_lib.header_symbols()) == set(_lib.SIGNATURES) and _lib.ABI_VERSION == 9
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "(122 entry points" in readme and "## Mirrored box features" in readme
