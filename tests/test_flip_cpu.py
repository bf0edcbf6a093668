"""Flip augmentation without a GPU: the setting and its refusals, the seeded draws, the label map, the ABI of the two entry points."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(dataset="volleyball", **kw):
    from din_amd.config import Config
    cfg = Config(dataset)
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_the_setting_is_off_by_default():
    from din_amd import frame_cache as FC
    for dataset in ("volleyball", "collective"):
        cfg = _cfg(dataset)
        assert cfg.flip_prob == 0.0 and isinstance(cfg.flip_prob, float)
        assert FC.flip_refusal(cfg) is None and FC.flip_plan(cfg, 1, 0) is None


REFUSED = [(dict(flip_prob=-0.1), ("flip_prob", "[0, 1]")), (dict(flip_prob=1.5), ("flip_prob", "[0, 1]")),
           (dict(flip_prob=float("nan")), ("flip_prob", "[0, 1]")), (dict(flip_prob=True), ("flip_prob", "[0, 1]")),
           (dict(flip_prob="0.5"), ("flip_prob", "[0, 1]")),
           (dict(flip_prob=0.5, feature_cache_gb=1), ("flip_prob", "feature_cache_gb")),
           (dict(flip_prob=0.5, num_activities=5), ("flip_prob", "num_activities"))]
REFUSED_IDS = ["negative", "above_one", "nan", "bool", "string", "feature_cache", "five_activities"]


@pytest.mark.parametrize("kw,words", REFUSED, ids=REFUSED_IDS)
def test_flip_refusal_names_the_setting(kw, words):
    from din_amd import frame_cache as FC
    why = FC.flip_refusal(_cfg(**kw))
    assert why is not None
    for w in words:
        assert w in why, (w, why)


@pytest.mark.parametrize("trainer", ["train_net", "train_net_dynamic"])
@pytest.mark.parametrize("kw,words", REFUSED, ids=REFUSED_IDS)
def test_both_trainers_refuse_before_any_loader_is_built(trainer, kw, words, monkeypatch):
    """each refusal is a ValueError naming flip_prob, raised before a process group, a loader or the device is touched"""
    import importlib
    from din_amd import frame_cache as FC
    T = importlib.import_module("din_amd." + trainer)
    monkeypatch.setattr(FC, "build_loaders", lambda *a, **k: pytest.fail("a loader was built before the refusal"))
    monkeypatch.setattr(T.parallel, "init_from_env", lambda *a, **k: pytest.fail("the device was set up before the refusal"))
    with pytest.raises(ValueError) as e:
        T.train_net(_cfg(**kw))
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_accepted_values_are_not_refused():
    from din_amd import frame_cache as FC
    for p in (0, 0.5, 1, 1.0):
        assert FC.flip_refusal(_cfg(flip_prob=p)) is None, p
    assert FC.flip_refusal(_cfg("collective", flip_prob=0.5)) is None
    assert FC.flip_refusal(_cfg("collective", flip_prob=0.5, num_activities=5)) is None      # (the collective labels have no side)
    assert FC.flip_refusal(_cfg(flip_prob=0, feature_cache_gb=1)) is None                    # off: nothing to refuse


def test_flip_plan_draws_are_seeded_by_seed_rank_and_epoch():
    from din_amd import frame_cache as FC

    def draws(seed, rank, epoch, prob=0.5, batches=(7, 7, 3)):
        e = FC.FlipPlan(prob, seed, rank).epoch(epoch)
        out = [e.draw(n) for n in batches]
        assert all(d.dtype == np.bool_ and d.shape == (n,) for d, n in zip(out, batches))
        assert e.flipped == sum(int(d.sum()) for d in out)
        return np.concatenate(out)

    base = draws(5, 0, 3)
    assert np.array_equal(base, draws(5, 0, 3))                      # a resumed run repeats the flips of an epoch
    assert not np.array_equal(base, draws(5, 0, 4)) and not np.array_equal(base, draws(5, 1, 3)) and not np.array_equal(base, draws(6, 0, 3))
    # draws are taken in batch order out of one stream: the batching does not change them
    assert np.array_equal(base, draws(5, 0, 3, batches=(17,)))
    assert not draws(5, 0, 3, prob=0.0).any() and draws(5, 0, 3, prob=1.0).all()
    f = float(draws(5, 0, 3, prob=0.3, batches=(20000,)).mean())
    assert abs(f - 0.3) < 0.02, f                                    # 5 sigma of sqrt(0.21 / 20000) = 0.0032 is 0.016; the draw is seeded


def test_flip_plan_from_the_config():
    from din_amd import frame_cache as FC, volleyball as V
    assert FC.flip_plan(_cfg(flip_prob=0), 1, 0) is None and FC.flip_plan(_cfg(flip_prob=0.0), 1, 0) is None
    cfg = _cfg(flip_prob=0.5, train_random_seed=11, out_size=(3, 5))
    e = FC.flip_plan(cfg, 2, 1)
    assert np.array_equal(e.draw(64), FC.FlipPlan(0.5, 11, 1).epoch(2).draw(64))
    assert e.label_map == V.FLIP_ACTIVITIES and e.width == 5.0
    c = FC.flip_plan(_cfg("collective", flip_prob=0.5, out_size=(3, 7)), 2, 1)
    assert c.label_map is None and c.width == 7.0
    assert e.rows(4, 3) is None or e.rows(4, 3).shape == (12,)
    all_on = FC.FlipPlan(1.0, 0, 0).epoch(1)
    assert all_on.rows(2, 3).tolist() == [True] * 6 and all_on.flipped == 2
    assert FC.FlipPlan(0.0, 0, 0).epoch(1).rows(2, 3) is None


def test_flip_activities_swaps_the_team_side():
    from din_amd.volleyball import ACTIVITIES, FLIP_ACTIVITIES
    assert FLIP_ACTIVITIES == [4, 5, 6, 7, 0, 1, 2, 3]
    assert [FLIP_ACTIVITIES[j] for j in FLIP_ACTIVITIES] == list(range(len(ACTIVITIES)))      # its own inverse
    for i, j in enumerate(FLIP_ACTIVITIES):
        a, b = ACTIVITIES[i], ACTIVITIES[j]
        # the names differ only in the leading r / l ('-' and '_' are one separator: the reference spells 'r_spike' but 'l-spike')
        assert {a[0], b[0]} == {"r", "l"} and a[1:].replace("-", "_") == b[1:].replace("-", "_"), (a, b)


def test_feed_for_builds_the_feed_of_every_loader_kind_with_the_very_augmentation_given(monkeypatch):
    """the wiring of flip and colour jitter together: none, flip, jitter and both, over a plain loader, a CachedLoader and a
    FeatureLoader.  Each feed receives the very objects given; without an augmentation a training pass is fed exactly as an evaluation
    pass is; the feature cache refuses every augmentation."""
    from din_amd import feature_cache as FE, frame_cache as FC
    monkeypatch.setattr(FC, "DeviceFeed", lambda *a: ("plain",) + a)
    monkeypatch.setattr(FC, "FlippedFeed", lambda *a: ("flipped",) + a)
    monkeypatch.setattr(FC, "CachedFeed", lambda *a: ("cached",) + a)
    monkeypatch.setattr(FE, "FeatureFeed", lambda *a: ("features",) + a)
    flip, jitter = FC.FlipPlan(0.5, 0, 0).epoch(1), FC.JitterPlan((0.4, 0.4, 0.4), 0, 0).epoch(1)
    cached, features = FC.CachedLoader("L", "C", "D"), FE.FeatureLoader("L", "C", "D")
    # none: what an evaluation pass builds (feed_for(loader, device)), and `augmentations` gives None when both settings are off
    assert FC.augmentations(_cfg(), 1, 0) is None and FC.augmentations(_cfg("collective"), 3, 1) is None
    assert FC.feed_for("L", "cpu") == FC.feed_for("L", "cpu", None) == ("plain", "L", "cpu")
    assert FC.feed_for(cached, "cpu") == FC.feed_for(cached, "cpu", None) == cached.feed("cpu") == ("cached", "L", "cpu", "C", "D", None)
    assert FC.feed_for(features, "cpu") == FC.feed_for(features, "cpu", None) == ("features", "L", "cpu", "C", "D")
    for f, j in ((flip, None), (None, jitter), (flip, jitter)):
        augment = FC.PassAugment(f, j)
        assert augment.flip is f and augment.jitter is j
        made = FC.feed_for("L", "cpu", augment)
        assert made == ("flipped", "L", "cpu", augment) and made[-1] is augment
        made = FC.feed_for(cached, "cpu", augment)
        assert made == ("cached", "L", "cpu", "C", "D", augment) and made[-1] is augment
        with pytest.raises(ValueError) as e:
            FC.feed_for(features, "cpu", augment)
        assert ("flip augmentation" if f is not None else "colour jitter") in str(e.value) and "feature cache" in str(e.value)
    # what the trainers hand over: the object `augmentations` makes holds the plans of the two settings
    both = FC.augmentations(_cfg(flip_prob=0.5, color_jitter=(0.4, 0.4, 0.4)), 1, 0)
    assert isinstance(both.flip, FC.EpochFlips) and isinstance(both.jitter, FC.EpochJitter)
    only_flip, only_jitter = FC.augmentations(_cfg(flip_prob=0.5), 1, 0), FC.augmentations(_cfg(color_jitter=(0.4, 0.4, 0.4)), 1, 0)
    assert isinstance(only_flip.flip, FC.EpochFlips) and only_flip.jitter is None
    assert only_jitter.flip is None and isinstance(only_jitter.jitter, FC.EpochJitter)


def test_header_binding_and_readme_agree_on_the_two_entry_points():
    from din_amd import _lib
    text = open(_lib.HEADER_PATH).read()
    assert "#define DIN_ABI_VERSION 9 " in text and _lib.ABI_VERSION == 9
    want = {"din_copy_rows_u8_flip": "int din_copy_rows_u8_flip(const uint64_t* src, const uint64_t* dst, const int64_t* flip, int n, "
                                     "int64_t lines, int64_t width, void* stream",
            "din_flip_clip_labels": "int din_flip_clip_labels(float* boxes, int64_t* activities, const int64_t* flip, "
                                    "const int32_t* n_valid, const int64_t* label_map, int rows, int n, float width, int classes, "
                                    "void* stream"}
    for name, words in want.items():
        decl = text[text.index(f"int {name}("):]
        assert re.sub(r"\s+", " ", decl[:decl.index(");")]) == words
    assert set(_lib.header_symbols()) == set(_lib.SIGNATURES)
    P, I, L, F = C.c_void_p, C.c_int, C.c_int64, C.c_float
    assert _lib.SIGNATURES["din_copy_rows_u8_flip"] == (I, [P, P, P, I, L, L, P])
    assert _lib.SIGNATURES["din_flip_clip_labels"] == (I, [P, P, P, P, P, I, I, F, I, P])
    assert _lib.SIGNATURES["din_copy_rows_u8"] == (I, [P, P, I, L, P])                        # the plain gather keeps its signature
    if os.path.exists(_lib.LIB_PATH):
        lib = C.CDLL(_lib.LIB_PATH)
        assert all(hasattr(lib, n) for n in want)
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert f"({len(_lib.header_symbols())} entry points" in readme and len(_lib.header_symbols()) == 122
    assert "## Flip augmentation" in readme
