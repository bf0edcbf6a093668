"""bf16 storage of the box-feature cache, host side (no GPU): the setting's default, the sizes that halve, the new refusals, the slot
bookkeeping at the bf16 slot size, the C ABI of din_feat_rows_bf16, and the integer model of round-to-nearest-even that
tests/test_gpu_feature_cache_bf16.py holds the kernel to."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the rounding model and the values it is checked on (shared with the GPU test) ------------------------------------------------------
def rne_bf16_bits(x: np.ndarray) -> np.ndarray:
    """fp32 -> the 16 bits of its bf16 neighbour, round-to-nearest-even, in integers: add half of the dropped part's range, minus one
    where the kept part is even, and drop 16 bits.  A carry out of the mantissa is the next exponent, out of the largest exponent
    Inf; +-0 and +-Inf have nothing to drop.  NaN is not modelled (the carry could turn one into Inf): the callers exclude it."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    assert not np.isnan(x).any()
    u = x.view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def fp32_values(count: int, seed: int) -> np.ndarray:
    """`count` fp32 values, finite or infinite, none subnormal: normals scaled over 2^+-60, with the special cases spread among them
    -- exact ties towards either neighbour, the values one fp32 step beside a tie, +-0, +-Inf and the largest finite fp32 (which
    rounds to Inf)"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(count) * np.exp2(rng.uniform(-60, 60, count))).astype(np.float32)
    x[(np.abs(x) < 2.0 ** -100)] = 1.5
    ties = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 2 - 2.0 ** -8], dtype=np.float32)     # down to even, up to even, up into 2.0
    beside = np.concatenate([np.nextafter(ties, np.float32(0)), np.nextafter(ties, np.float32(4))]).astype(np.float32)
    fmax = np.finfo(np.float32).max
    special = np.concatenate([ties, -ties, beside, -beside, np.array([0.0, -0.0, np.inf, -np.inf, fmax, -fmax, 1.0, -2.5], dtype=np.float32)])
    at = rng.permutation(count)[:min(count, 4 * len(special))]
    x[at] = np.resize(special, len(at))
    return x


def test_integer_model_of_round_to_nearest_even_is_torchs_cast():
    x = fp32_values(1 << 16, seed=1)
    assert np.isinf(x).any() and (x == 0).any() and (x == np.float32(1 + 2.0 ** -8)).any() and (x == np.finfo(np.float32).max).any()
    assert np.abs(x[np.isfinite(x) & (x != 0)]).min() >= 2.0 ** -100 and np.abs(x[np.isfinite(x)]).max() > 2.0 ** 50
    want = torch.tensor(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = rne_bf16_bits(x)
    assert np.array_equal(got, want), f"{np.count_nonzero(got != want)} values differ, first {x[np.flatnonzero(got != want)[:4]]}"
    fmax, tie = np.finfo(np.float32).max, np.float32(1 + 2.0 ** -8)
    by_hand = [(tie, 0x3F80), (1 + 3 * 2.0 ** -8, 0x3F82), (2 - 2.0 ** -8, 0x4000), (-tie, 0xBF80), (0.0, 0x0000), (-0.0, 0x8000),
               (np.inf, 0x7F80), (-np.inf, 0xFF80), (fmax, 0x7F80), (-fmax, 0xFF80),
               (np.nextafter(tie, np.float32(4)), 0x3F81), (np.nextafter(tie, np.float32(0)), 0x3F80)]
    for v, bits in by_hand:
        assert int(rne_bf16_bits(np.array([v], dtype=np.float32))[0]) == bits, (v, hex(bits))


# ---- the setting ------------------------------------------------------------------------------------------------------------------------
def _cfg(**kw):
    from din_amd.config import Config
    cfg = Config("volleyball")
    cfg.backbone, cfg.training_stage, cfg.emb_features = "vgg16", 2, 512
    cfg.feature_cache_gb, cfg.feature_cache_dtype, cfg.backbone_dtype = 1, "bf16", "bf16"
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_default_is_fp32_and_bf16_halves_the_row_only():
    from din_amd.config import Config
    from din_amd.feature_cache import FeatureCache, row_and_box_bytes
    for name in ("volleyball", "collective"):
        assert Config(name).feature_cache_dtype == "fp32"
    cfg = _cfg()
    assert row_and_box_bytes(cfg) == row_and_box_bytes(cfg, torch.float32) == (614400, 192)
    assert row_and_box_bytes(cfg, torch.bfloat16) == (307200, 192)
    cfg.emb_features = 1056
    assert row_and_box_bytes(cfg, torch.bfloat16) == (633600, 192)
    wide = FeatureCache("cpu", 614400, 192, 10 ** 9)
    half = FeatureCache("cpu", 307200, 192, 10 ** 9, dtype=torch.bfloat16)
    assert wide.dtype == torch.float32 and (wide.row_elems, wide.table.stride) == (153600, 614400 + 192)
    assert half.dtype == torch.bfloat16 and (half.row_bytes, half.box_bytes, half.row_elems) == (307200, 192, 153600)
    assert half.table.stride == 307200 + 192 and half.table.max_slots == 10 ** 9 // (307200 + 192) and half.bytes == 0
    with pytest.raises(ValueError):
        FeatureCache("cpu", 307200, 192, 10 ** 9, dtype=torch.float16)
    with pytest.raises(ValueError):
        FeatureCache("cpu", 307208, 192, 10 ** 9, dtype=torch.bfloat16)


def test_slot_bookkeeping_at_the_bf16_slot_size():
    from din_amd.feature_cache import FeatureCache
    cache = FeatureCache("cpu", 800, 192, 6 * 992 + 100, chunk_frames=4, dtype=torch.bfloat16)      # the fp32 row would be 1600 bytes
    t = cache.table
    assert t.stride == 992 and t.max_slots == 6 and cache.row_elems == 400
    asked = []
    assert [t.insert(100 + i, lambda n: (asked.append(n), True)[1]) for i in range(8)] == [0, 1, 2, 3, 4, 5, -1, -1]
    assert asked == [4, 2] and cache.inserted == 6 and cache.bytes == 6 * 992 and t.full and t.locate(5) == (1, 992)
    frozen = FeatureCache("cpu", 800, 192, 1 << 20, chunk_frames=4, dtype=torch.bfloat16)
    assert [frozen.table.insert(i, lambda n: frozen.table.allocated == 0) for i in range(6)] == [0, 1, 2, 3, -1, -1]
    assert frozen.table.frozen and frozen.bytes == 4 * 992                                           # a failed allocation freezes it


def test_loaders_pass_the_dtype_through(golden_dir):
    from din_amd import feature_cache as FE, frame_cache as FC
    from tests.test_feature_cache_cpu import _volleyball
    ids = _volleyball(golden_dir, frame_ids=True)
    for dtype, want, row in (("fp32", torch.float32, 614400), ("bf16", torch.bfloat16, 307200)):
        for ld in FC.build_loaders(_cfg(feature_cache_dtype=dtype), ids, ids, 2, None, "cpu", True):
            assert type(ld.cache) is FE.FeatureCache and ld.cache.dtype == want and (ld.cache.row_bytes, ld.cache.box_bytes) == (row, 192)
            assert ld.cache.table.max_slots == 10 ** 9 // (row + 192)


@pytest.mark.parametrize("kw,words", [
    (dict(feature_cache_dtype="fp16"), ("feature_cache_dtype", "'fp16'", "bf16", "fp32")),
    (dict(backbone_dtype="fp32"), ("feature_cache_dtype", "'bf16'", "backbone_dtype", "'fp32'")),
    (dict(backbone_dtype="fp32_bf16x3"), ("feature_cache_dtype", "'bf16'", "backbone_dtype", "'fp32_bf16x3'")),
    (dict(emb_features=1052), ("feature_cache_dtype", "emb_features", "26300", "multiples of 8")),
    (dict(num_features_boxes=1020), ("feature_cache_dtype", "num_features_boxes", "1020", "multiples of 8")),
], ids=["unknown_value", "fp32_backbone", "split_backbone", "gemm_k_not_8", "gemm_n_not_8"])
def test_train_net_refuses_before_any_loader_is_built(kw, words, monkeypatch):
    from din_amd import frame_cache as FC, train_net_dynamic as TD
    cfg = _cfg(**kw)
    monkeypatch.setattr(FC, "build_loaders", lambda *a, **k: pytest.fail("a loader was built before the refusal"))
    monkeypatch.setattr(TD.parallel, "init_from_env", lambda *a, **k: pytest.fail("the device was set up before the refusal"))
    with pytest.raises(ValueError) as e:
        TD.train_net(cfg)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_what_is_not_refused_and_what_comes_first():
    from din_amd import feature_cache as FE
    assert FE.refusal(_cfg()) is None
    assert FE.refusal(_cfg(backbone="inv3", emb_features=1056, set_bn_eval=True)) is None
    assert FE.refusal(_cfg(feature_cache_dtype="fp32", backbone_dtype="fp32")) is None
    # the cache off: the setting is never read
    for kw in (dict(feature_cache_dtype="fp16"), dict(backbone_dtype="fp32"), dict(num_features_boxes=1020)):
        assert FE.refusal(_cfg(feature_cache_gb=0, **kw)) is None
    # the five earlier refusals come first, in their order
    assert "train_backbone" in FE.refusal(_cfg(feature_cache_dtype="fp16", train_backbone=True, frame_cache_gb=2))
    assert "frame_cache_gb = 2" in FE.refusal(_cfg(backbone_dtype="fp32", frame_cache_gb=2))
    assert "set_bn_eval" in FE.refusal(_cfg(backbone_dtype="fp32", backbone="inv3", set_bn_eval=False))


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_makefile_agree_on_feat_rows_bf16():
    import inspect
    from din_amd import _lib, ops
    text = open(_lib.HEADER_PATH).read()
    assert "#define DIN_ABI_VERSION 9 " in text and _lib.ABI_VERSION == 9
    assert "din_feat_rows_bf16" in _lib.header_symbols() and set(_lib.header_symbols()) == set(_lib.SIGNATURES)

    def declaration(name):
        decl = text[text.index(f"int {name}("):]
        return re.sub(r"\s+", " ", decl[:decl.index(");")])

    assert declaration("din_feat_rows_bf16") == (
        "int din_feat_rows_bf16(const uint64_t* src, const uint64_t* dst, const uint64_t* keep, const uint64_t* ref_boxes, "
        "const uint64_t* src_f32, const void* boxes, uint8_t* flags, int n, int64_t row_elems, int box_bytes, void* stream")
    # din_feat_rows itself, text and spacing, is what it was
    assert ("int din_feat_rows(const uint64_t* src, const uint64_t* dst, const uint64_t* keep, const uint64_t* ref_boxes,\n"
            "                  const void* boxes, uint8_t* flags, int n, int64_t row_bytes, int box_bytes, void* stream);\n") in text
    assert _lib.SIGNATURES["din_feat_rows"] == (C.c_int, [C.c_void_p] * 6 + [C.c_int, C.c_int64, C.c_int, C.c_void_p])
    assert _lib.SIGNATURES["din_feat_rows_bf16"] == (C.c_int, [C.c_void_p] * 7 + [C.c_int, C.c_int64, C.c_int, C.c_void_p])
    assert len(re.findall(r"^#define DIN_FEAT_ROWS_SEGMENT (\d+)$", text, flags=re.M)) == 1         # one constant for both
    assert re.search(r"^SRCS = .*\bfeat_cache\.hip\b", open(os.path.join(_lib.CSRC_DIR, "Makefile")).read(), flags=re.M)
    kernel = open(os.path.join(_lib.CSRC_DIR, "feat_cache.hip")).read()
    assert 'extern "C" int din_feat_rows_bf16(' in kernel and 'extern "C" int din_feat_rows(' in kernel
    assert "infer_model.py:152-184" in kernel and "DIN_FEAT_ROWS_SEGMENT" in kernel and "atomic" not in kernel.replace("no atomics", "")
    if os.path.exists(_lib.LIB_PATH):
        assert hasattr(C.CDLL(_lib.LIB_PATH), "din_feat_rows_bf16")
    assert list(inspect.signature(ops.feat_rows_bf16).parameters)[:9] == ["src", "dst", "row_elems", "keep", "ref", "boxes", "flags",
                                                                          "box_bytes", "src_f32"]
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert f"({len(_lib.header_symbols())} entry points" in readme
