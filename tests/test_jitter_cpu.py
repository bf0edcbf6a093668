"""Colour jitter without a GPU: the numpy model (tests/jitter_reference.py) against Pillow's ImageEnhance byte for byte, the integer mean
rule, the setting and its refusals, the seeded draws, the pass's augmentation object, the two declarations and their binding."""
import ctypes as C
import importlib
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests import jitter_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(dataset="volleyball", **kw):
    from din_amd.config import Config
    cfg = Config(dataset)
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


# ---- the model is Pillow ---------------------------------------------------------------------------------------------------------------
def _images():
    rng = np.random.default_rng(12)
    h, w = 24, 40
    out = {"random": rng.integers(0, 256, (3, h, w), dtype=np.uint8),
           "near_white": rng.integers(250, 256, (3, h, w), dtype=np.uint8),
           "near_black": rng.integers(0, 6, (3, h, w), dtype=np.uint8),
           "single_colour": np.broadcast_to(np.array([200, 30, 90], dtype=np.uint8)[:, None, None], (3, h, w)).copy(),
           "odd_7x13": rng.integers(0, 256, (3, 7, 13), dtype=np.uint8),
           "all_255": np.full((3, 5, 9), 255, dtype=np.uint8), "all_0": np.zeros((3, 5, 9), dtype=np.uint8)}
    return out


GRID = (0.0, 0.25, 0.5, 1.0, 1.5, 1.75, 1.999, float(np.nextafter(np.float32(2), np.float32(0))))


def _pillow(frame, c, b, s):
    from PIL import Image, ImageEnhance
    img = Image.fromarray(np.ascontiguousarray(frame.transpose(1, 2, 0)), "RGB")
    img = ImageEnhance.Contrast(img).enhance(c)
    img = ImageEnhance.Brightness(img).enhance(b)
    img = ImageEnhance.Color(img).enhance(s)
    return np.asarray(img).transpose(2, 0, 1)


@pytest.mark.parametrize("name", list(_images()))
def test_model_equals_pillow_image_enhance_byte_for_byte(name):
    """ImageEnhance.Contrast, then .Brightness, then .Color against the model, over the whole grid of factor triples (0, 1 and both ends
    of the range among them); every factor is a float32 value, as the launch takes it"""
    frame = _images()[name]
    compared = 0
    for c in GRID:
        for b in GRID:
            for s in GRID:
                want = _pillow(frame, float(np.float32(c)), float(np.float32(b)), float(np.float32(s)))
                got = R.jitter(frame, c, b, s)
                assert np.array_equal(got, want), (name, c, b, s, int((got != want).sum()))
                compared += got.size
    assert compared == len(GRID) ** 3 * frame.size


def test_each_stage_alone_equals_its_pillow_enhancer():
    frame = _images()["random"]
    for f in GRID:
        assert np.array_equal(R.jitter(frame, f, 1, 1), _pillow(frame, f, 1.0, 1.0))
        assert np.array_equal(R.jitter(frame, 1, f, 1), _pillow(frame, 1.0, f, 1.0))
        assert np.array_equal(R.jitter(frame, 1, 1, f), _pillow(frame, 1.0, 1.0, f))


def test_identity_at_factor_one_and_mirror_commutes():
    for name, frame in _images().items():
        assert np.array_equal(R.jitter(frame, 1, 1, 1), frame), name
        assert np.array_equal(_pillow(frame, 1.0, 1.0, 1.0), frame), name
        assert np.array_equal(R.jitter(frame, 1, 1, 1, mirror=True), frame[:, :, ::-1])
        assert np.array_equal(R.jitter(frame, 0.25, 1.75, 0.5, mirror=True), R.jitter(frame[:, :, ::-1], 0.25, 1.75, 0.5))


def test_integer_mean_rule_next_to_a_half():
    """(2 S + n) // (2 n) is int(S / n + 0.5): sums chosen on, just below and just above k + 1/2, for small, odd and frame-sized n"""
    checked = 0
    for n in (1, 2, 7, 960, 15360, 921600, (1 << 24) - 1):
        for k in (0, 1, 127, 128, 254):
            for delta in (-2, -1, 0, 1, 2):
                for half in (n // 2, (n + 1) // 2):
                    s = k * n + half + delta
                    if s < 0 or s > 255 * n:
                        continue
                    exact = (Fraction(s, n) + Fraction(1, 2)).__floor__()
                    assert R.pivot(s, n) == exact == int(s / n + 0.5), (s, n)
                    checked += 1
        assert R.pivot(255 * n, n) == 255 and R.pivot(0, n) == 0
    assert checked > 200


def test_gray_is_pillows_l_conversion_and_partials_add_up():
    from PIL import Image
    frame = _images()["random"]
    want = np.asarray(Image.fromarray(np.ascontiguousarray(frame.transpose(1, 2, 0)), "RGB").convert("L"))
    assert np.array_equal(R.gray(frame[0], frame[1], frame[2]), want)
    assert int(R.gray(255, 255, 255)) == 255 and int(R.gray(0, 0, 0)) == 0
    for h, w in ((1, 1), (37, 64), (129, 64), (2, 8192), (3, 8208), (5, 100)):
        x = np.random.default_rng(h * w).integers(0, 256, (3, h, w), dtype=np.uint8)
        parts = R.gray_partials(x)
        assert parts.shape == (R.segments(h, w),) and parts.sum() == R.gray(x[0], x[1], x[2]).sum()


def test_ops_states_the_segment_rule_of_the_model():
    from din_amd import ops
    assert ops.GRAY_SEGMENT == R.GRAY_SEGMENT == 8192
    for h, w in ((1, 1), (2, 3), (5, 16), (4, 48), (3, 100), (2, 8192), (1, 8208), (37, 64), (129, 64), (720, 1280), (8193, 1), (7, 4097)):
        assert ops.gray_partial_segments(h, w) == R.segments(h, w), (h, w)
    assert ops.gray_partial_segments(720, 1280) == 120 and ops.gray_partial_segments(0, 5) == 0


# ---- the setting -----------------------------------------------------------------------------------------------------------------------
def test_the_setting_is_off_by_default():
    from din_amd import config, frame_cache as FC
    assert "color_jitter" in config._DEFAULTS and config._DEFAULTS["color_jitter"] is None
    for dataset in ("volleyball", "collective"):
        cfg = _cfg(dataset)
        assert cfg.color_jitter is None
        assert FC.jitter_refusal(cfg) is None and FC.jitter_plan(cfg, 1, 0) is None
        assert FC.augmentations(cfg, 1, 0) is None


REFUSED = [(dict(color_jitter=0.4), ("color_jitter", "[0, 1)")), (dict(color_jitter=(0.4, 0.4)), ("color_jitter", "[0, 1)")),
           (dict(color_jitter=(0.4, 0.4, 0.4, 0.1)), ("color_jitter", "[0, 1)")), (dict(color_jitter=(0.4, -0.1, 0.4)), ("color_jitter", "[0, 1)")),
           (dict(color_jitter=(0.4, 0.4, 1.0)), ("color_jitter", "[0, 1)")), (dict(color_jitter=(float("nan"), 0.4, 0.4)), ("color_jitter", "[0, 1)")),
           (dict(color_jitter=(True, 0.4, 0.4)), ("color_jitter", "[0, 1)")), (dict(color_jitter=("0.4", 0.4, 0.4)), ("color_jitter", "[0, 1)")),
           (dict(color_jitter="0.4"), ("color_jitter", "[0, 1)")), (dict(color_jitter="abc"), ("color_jitter", "[0, 1)")),
           (dict(color_jitter=(0.4, 0.4, 0.4), feature_cache_gb=1), ("color_jitter", "feature_cache_gb"))]
REFUSED_IDS = ["scalar", "two", "four", "negative", "one", "nan", "bool", "string_inside", "string", "three_letters", "feature_cache"]


@pytest.mark.parametrize("kw,words", REFUSED, ids=REFUSED_IDS)
def test_jitter_refusal_names_the_setting(kw, words):
    from din_amd import frame_cache as FC
    why = FC.jitter_refusal(_cfg(**kw))
    assert why is not None
    for w in words:
        assert w in why, (w, why)


@pytest.mark.parametrize("trainer", ["train_net", "train_net_dynamic"])
@pytest.mark.parametrize("kw,words", REFUSED, ids=REFUSED_IDS)
def test_both_trainers_refuse_before_any_loader_is_built(trainer, kw, words, monkeypatch):
    """each refusal is a ValueError naming color_jitter, raised before a process group, a loader or the device is touched"""
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
    for j in ((0.4, 0.4, 0.4), [0, 0, 0], (0, 0.999, 0.5), np.array([0.1, 0.2, 0.3]), (np.float32(0.5), 0, 0)):
        assert FC.jitter_refusal(_cfg(color_jitter=j)) is None, j
        assert FC.jitter_refusal(_cfg("collective", color_jitter=j, flip_prob=0.5)) is None
    assert FC.jitter_refusal(_cfg(color_jitter=None, feature_cache_gb=1)) is None            # off: nothing to refuse


# ---- the draws -------------------------------------------------------------------------------------------------------------------------
def _draws(seed, rank, epoch, amplitudes=(0.4, 0.3, 0.2), batches=(7, 7, 3)):
    from din_amd import frame_cache as FC
    e = FC.JitterPlan(amplitudes, seed, rank).epoch(epoch)
    out = [e.draw(n) for n in batches]
    assert all(d.dtype == np.float32 and d.shape == (n, 3) for d, n in zip(out, batches))
    assert e.jittered == sum(int((d != 1).any(axis=1).sum()) for d in out)
    return np.concatenate(out)


def test_jitter_plan_draws_are_seeded_by_seed_rank_and_epoch():
    base = _draws(5, 0, 3)
    assert np.array_equal(base, _draws(5, 0, 3))                     # a resumed run repeats the draws of an epoch
    assert not np.array_equal(base, _draws(5, 0, 4)) and not np.array_equal(base, _draws(5, 1, 3)) and not np.array_equal(base, _draws(6, 0, 3))
    assert np.array_equal(base, _draws(5, 0, 3, batches=(17,)))      # one stream in batch order: the batching does not change them
    # f = 1 + a u, u in [-1, 1]: the same u whatever the amplitudes, column by column (brightness, contrast, saturation)
    u = np.random.default_rng([5, 0, 3, 1]).uniform(-1.0, 1.0, (17, 3))
    assert np.array_equal(base, (1.0 + np.array([0.4, 0.3, 0.2]) * u).astype(np.float32))
    for col, a in enumerate((0.4, 0.3, 0.2)):
        assert np.all(base[:, col] >= np.float32(1 - a)) and np.all(base[:, col] <= np.float32(1 + a)) and base[:, col].std() > 0.1 * a
    zero = _draws(5, 0, 3, amplitudes=(0.0, 0.3, 0))
    assert np.all(zero[:, 0] == np.float32(1)) and np.all(zero[:, 2] == np.float32(1)) and np.array_equal(zero[:, 1], base[:, 1])
    big = _draws(5, 0, 3, amplitudes=(0.999, 0.999, 0.999), batches=(20000,))
    assert big.min() > 0 and big.max() < 2 and abs(float(big.mean()) - 1) < 0.02        # 5 sigma of 0.577 / sqrt(60000) = 0.012


def test_rows_are_the_launch_order_repeated_over_the_frames():
    from din_amd import frame_cache as FC
    assert FC.KERNEL_ORDER == (1, 0, 2)
    f = FC.JitterPlan((0.4, 0.3, 0.2), 9, 0).epoch(2).draw(4)
    e = FC.JitterPlan((0.4, 0.3, 0.2), 9, 0).epoch(2)
    rows = e.rows(4, 3)
    assert rows.dtype == np.float32 and rows.shape == (12, 3) and rows.flags.c_contiguous and e.jittered == 4
    for k in range(12):
        assert rows[k].tolist() == [f[k // 3, 1], f[k // 3, 0], f[k // 3, 2]]               # (contrast, brightness, saturation)
    off = FC.JitterPlan((0, 0, 0), 9, 0).epoch(2)
    assert off.rows(4, 3) is None and off.jittered == 0
    words = FC._f32_as_table(rows[:3])                                                       # nine floats: padded to ten, five words
    assert words.dtype == np.int64 and words.shape == (5,) and np.array_equal(words.view(np.float32)[:9], rows[:3].reshape(-1))


def test_flip_draws_do_not_change_when_the_jitter_is_turned_on():
    from din_amd import frame_cache as FC
    for epoch in (1, 2, 7):
        off = FC.flip_plan(_cfg(flip_prob=0.5, train_random_seed=11), epoch, 1)
        cfg = _cfg(flip_prob=0.5, train_random_seed=11, color_jitter=(0.4, 0.4, 0.4))
        augment = FC.augmentations(cfg, epoch, 1)
        flip, jitter = augment.flip, augment.jitter
        assert flip is not None and jitter is not None
        for n in (7, 7, 3):
            assert np.array_equal(jitter.draw(n), jitter.draw(n)) is False               # the jitter's own stream advances ...
            assert np.array_equal(off.draw(n), flip.draw(n))                             # ... and the flips are those of the run without
        # the same through the one method a feed calls: each stream drawn once per batch, the flips those of the run without jitter
        off, alone = FC.flip_plan(_cfg(flip_prob=0.5, train_random_seed=11), epoch, 1), FC.jitter_plan(cfg, epoch, 1)
        augment = FC.augmentations(cfg, epoch, 1)
        for n in (7, 7, 3):
            rows, factors = augment.rows(n, 3)
            want_rows, want_factors = off.rows(n, 3), alone.rows(n, 3)
            assert (rows is None and want_rows is None) or np.array_equal(rows, want_rows)
            assert factors.shape == (3 * n, 3) and np.array_equal(factors, want_factors)
        assert augment.flip.flipped == off.flipped and augment.jitter.jittered == alone.jittered == 17
    e = FC.jitter_plan(_cfg(color_jitter=(0.4, 0.3, 0.2), train_random_seed=11), 2, 1)
    assert np.array_equal(e.draw(64), FC.JitterPlan((0.4, 0.3, 0.2), 11, 1).epoch(2).draw(64))


# ---- wiring (the feeds: tests/test_flip_cpu.py, with the flip) ---------------------------------------------------------------------------
def test_train_pass_info_counts_jittered_clips_on_the_host():
    from din_amd import frame_cache as FC
    from din_amd.train_net_dynamic import add_flip_stats
    jitter, flip = FC.JitterPlan((0.4, 0, 0), 0, 0).epoch(1), FC.FlipPlan(1.0, 0, 0).epoch(1)
    jitter.draw(5)
    flip.draw(3)
    assert add_flip_stats({}, None) == {} and add_flip_stats({}, FC.PassAugment(None, None)) == {}
    assert add_flip_stats({}, FC.PassAugment(None, jitter)) == {"jittered_clips": 5}
    # a key is there only when its part is on
    assert add_flip_stats({"loss": 1.0}, FC.PassAugment(flip, None)) == {"loss": 1.0, "flipped_clips": 3}
    assert add_flip_stats({}, FC.PassAugment(flip, jitter)) == {"flipped_clips": 3, "jittered_clips": 5}


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_second_header_binding_and_readme_agree():
    """the jitter half of the one-header check: the two entry points are declared in include/din_hip.h and bound through SIGNATURES"""
    from din_amd import _lib
    text = open(_lib.HEADER_PATH).read()
    want = {"din_rows_gray_partials": "int din_rows_gray_partials(const uint64_t* src, uint32_t* partials, int n, int64_t height, "
                                      "int64_t width, void* stream",
            "din_copy_rows_u8_jitter": "int din_copy_rows_u8_jitter(const uint64_t* src, const uint64_t* dst, const int64_t* flip, "
                                       "const float* factors, const uint32_t* partials, int n, int64_t height, int64_t width, void* stream"}
    for name, words in want.items():
        decl = text[text.index(f"int {name}("):]
        assert re.sub(r"\s+", " ", decl[:decl.index(");")]) == words
    assert set(want) <= set(_lib.header_symbols())
    P, I, L = C.c_void_p, C.c_int, C.c_int64
    assert _lib.SIGNATURES["din_rows_gray_partials"] == (I, [P, P, I, L, L, P])
    assert _lib.SIGNATURES["din_copy_rows_u8_jitter"] == (I, [P, P, P, P, P, I, L, L, P])
    assert "PIL.ImageEnhance" in text
    # one header: 122 functions, each bound, ABI version 9; the second header and its binding are gone
    assert len(_lib.header_symbols()) == 122 and set(_lib.header_symbols()) == set(_lib.SIGNATURES)
    assert "#define DIN_ABI_VERSION 9 " in text and _lib.ABI_VERSION == 9
    assert not os.path.exists(os.path.join(ROOT, "include", "din_hip_aug.h")) and not hasattr(_lib, "SIGNATURES_AUG")
    if os.path.exists(_lib.LIB_PATH):
        lib = C.CDLL(_lib.LIB_PATH)
        assert all(hasattr(lib, n) for n in want)
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "## Colour jitter" in readme and "(122 entry points" in readme


def test_a_library_without_an_aug_symbol_fails_loudly(monkeypatch):
    """load() refuses a library that lacks a bound entry point: one built before the entry points existed, for instance"""
    from din_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "libdin_hip.so missing: run __graft_entry__.build()"
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "SIGNATURES", dict(_lib.SIGNATURES, din_rows_gray_partials_of_a_later_build=(C.c_int, [])))
    with pytest.raises(_lib.DinError) as e:
        _lib.load()
    assert "din_rows_gray_partials_of_a_later_build" in str(e.value) and "stale build?" in str(e.value)
