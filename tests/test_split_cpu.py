"""CPU: the split-bf16 contraction mode (DIN_F32_BF16X3, cfg.backbone_dtype = 'fp32_bf16x3') -- its numerics in emulation, and its host
surface.

Emulation (tools/split_bf16_sim.py: the kernels' split, exact bf16 products, one fp32 accumulator rounding per MFMA): on the small-K
operands of tests/test_gpu_split.py's SMALL_K rows the three-part / six-product form meets the project's fp32 per-element bar (bar_of of
tests/test_gpu_conv_fwd_dgrad.py, imported), while the two-part form and the three-part form with ANY ONE of its six products removed
each leave it on at least one element -- so the GPU rows can fail: a kernel with a wrong operand word does not pass them.  At K = 64 and
K = 1152 the three-part form's rms error is within 1.1x of an fp32-accumulated exact product's and the two-part form's above 4x."""
import os
import sys

import numpy as np
import pytest

from tests.conftest import ROOT
from tests import test_gpu_conv_fwd_dgrad as CF
from tests.test_gpu_split import SMALL_K

sys.path.insert(0, os.path.join(ROOT, "tools"))
import split_bf16_sim as SIM  # noqa: E402


def _small_k_case(row):
    """(a [M][1][K], b [1][N][K], bar [M][N], v [M][N]) of a 1x1 row: the stored operands of the GPU row and its fp32 bar"""
    op = CF._operands(row)
    nb, cin, h, w, cout, k, s, p, dil, oh, ow = CF._geometry(row["shape"])
    wt = op["w"].numpy()[:, :, 0, 0]                                              # [cout][cin]
    if row["which"] == 0:
        a, b = op["x"].numpy().reshape(-1, cin), wt                                  # out[m][co] = sum_ci x[m][ci] w[co][ci]
    else:
        a, b = op["g"].numpy().reshape(-1, cout), wt.T                               # din[m][ci] = sum_co g[m][co] w[co][ci]
    v, S = op["v"].reshape(a.shape[0], -1), op["S"].reshape(a.shape[0], -1)
    bar = CF.bar_of(row, v, S, 0)
    return a[:, None, :], np.ascontiguousarray(b)[None, :, :], bar.numpy(), v.numpy()


@pytest.mark.parametrize("row", SMALL_K, ids=[r["label"] for r in SMALL_K])
def test_three_parts_meet_the_fp32_bar_and_every_missing_product_breaks_it(row):
    a, b, bar, v = _small_k_case(row)
    assert bar.min() > 0
    worst = float((np.abs(SIM.dot_split(a, b, SIM.MFMAS3).astype(np.float64) - v) / bar).max())
    assert worst <= 1.0, f"{row['label']}: the three-part form is {worst:.3f} of the fp32 bar"
    two = float((np.abs(SIM.dot_split(a, b, SIM.MFMAS2).astype(np.float64) - v) / bar).max())
    assert two > 1.0, f"{row['label']}: the two-part form passes the fp32 bar everywhere ({two:.3f})"
    assert len(SIM.SIX) == 6 and len(set(SIM.SIX)) == 6
    for pair in SIM.SIX:
        got = float((np.abs(SIM.dot_split(a, b, SIM.drop(SIM.MFMAS3, pair)).astype(np.float64) - v) / bar).max())
        assert got > 1.0, f"{row['label']}: without the product a{pair[0]} b{pair[1]} the fp32 bar still holds everywhere ({got:.3f})"


def test_split_parts_are_exact_and_finite_near_flt_max():
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.standard_normal(50000).astype(np.float32) * np.float32(10.0) ** rng.integers(-20, 20, 50000).astype(np.float32),
                        np.array([np.finfo(np.float32).max, -np.finfo(np.float32).max, 1.0, -1.0, 0.0, 2.0 ** -100], np.float32)])
    p = SIM.split(x, 3)
    assert all(np.isfinite(q).all() and not (q.view(np.uint32) & 0xFFFF).any() for q in p)
    assert np.array_equal(p[0].astype(np.float64) + p[1].astype(np.float64) + p[2].astype(np.float64), x.astype(np.float64))


@pytest.mark.parametrize("K", (64, 1152))
def test_rms_error_tracks_exact_fp32(K):
    e = SIM.rms_errors(K, 4096)
    print(f"K={K}: rms(err)/rms(result) exact {e['fp32']:.3e}  three-part {e['x3']:.3e} ({e['x3'] / e['fp32']:.2f}x)  two-part {e['x2']:.3e} "
          f"({e['x2'] / e['fp32']:.1f}x)")
    assert e["x3"] <= 1.1 * e["fp32"]
    assert e["x2"] > 4.0 * e["fp32"]


def test_sim_tool_prints_the_table(capsys):
    SIM.main((64,))
    out = capsys.readouterr().out.splitlines()
    assert "3 parts, 6 products" in out[1] and out[2].split()[0] == "64" and len(out[2].split()) == 5


# ---- host surface -----------------------------------------------------------------------------------------------------------------------
def test_host_surface():
    import torch
    from din_amd import _lib, config, infer_model, ops
    from din_amd.backbone.backbone import _dt
    assert _lib.DIN_F32_BF16X3 == 2 and (_lib.DIN_F32, _lib.DIN_BF16) == (0, 1)
    assert _lib.storage_dtype(_lib.DIN_F32_BF16X3) == _lib.DIN_F32 and _lib.storage_dtype(_lib.DIN_BF16) == _lib.DIN_BF16
    assert _dt("fp32_bf16x3") == _lib.DIN_F32_BF16X3 and _dt("fp32") == _lib.DIN_F32 and _dt("bf16") == _lib.DIN_BF16
    with pytest.raises(ValueError):
        _dt("fp32_bf16x2")
    x, w = torch.zeros(2, 8), torch.zeros(8, 8)
    with pytest.raises(ValueError, match="mutually exclusive"):
        ops.linear(x, w, None, lowp=True, split=True)
    with pytest.raises(ValueError, match="mutually exclusive"):
        ops.GridConvFunction.apply(x.reshape(1, 1, 2, 8), w.reshape(8, 8, 1, 1), None, 1, True, True)
    assert "fp32_bf16x3" in config.__doc__ and "fp32_bf16x3" in infer_model.__doc__
    assert config.Config("volleyball").backbone_dtype == "fp32"


def test_abi_is_additive():
    from din_amd import _lib
    assert _lib.ABI_VERSION == 9
    assert set(_lib.header_symbols()) == set(_lib.SIGNATURES)
    header = open(os.path.join(ROOT, "include", "din_hip.h")).read()
    assert "#define DIN_ABI_VERSION 9 " in header and "DIN_F32_BF16X3 = 2" in header


def test_library_takes_the_new_dtype_where_it_takes_fp32():
    """planning calls need no GPU: the new value answers what DIN_F32 answers (sizes, tile, workspace), names its kernels with their own T
    token, is refused nowhere DIN_F32 is taken, and value 3 is still refused"""
    import ctypes as C
    from din_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("libdin_hip.so is not built: run __graft_entry__.build()")
    lib = L.load()
    row = CF._row("x", "", 0, 0, "fp32", (2, 13, 19, 23, 118, (3, 3), (1, 1), (1, 1), 1))
    d, e = CF._desc(L, row), CF._desc(L, row)
    e.dtype = L.DIN_F32_BF16X3
    for which in (0, 1):
        assert lib.din_conv_packed_elems(C.byref(e), which) == lib.din_conv_packed_elems(C.byref(d), which) > 0
    for which in (0, 1, 2):
        assert lib.din_conv_workspace_bytes(C.byref(e), which) == lib.din_conv_workspace_bytes(C.byref(d), which)
        t = [C.c_int32(0) for _ in range(4)]
        L.check(lib.din_conv_kernel_tile(C.byref(d), which, C.byref(t[0]), C.byref(t[1])))
        L.check(lib.din_conv_kernel_tile(C.byref(e), which, C.byref(t[2]), C.byref(t[3])))
        assert (t[0].value, t[1].value) == (t[2].value, t[3].value)
    assert CF._names(lib, e, 0, 0, 0, 0) == [n.replace("<float,", "<f32x3,") for n in CF._names(lib, d, 0, 0, 0, 0)]
    assert CF._names(lib, e, 0, 0, 0, 0)[0].startswith("conv_gather_fast_kernel<f32x3,128,128,")
    buf = C.create_string_buffer(512)
    assert lib.din_conv_kernel_names(C.byref(e), 2, 0, 0, 0, buf, len(buf)) > 0
    assert buf.value.decode().split("\n")[0] == "conv_wgrad_f32x3_kernel"
    assert lib.din_conv_accepts_u8(C.byref(e)) == 0
    e.dtype = 3
    assert lib.din_conv_kernel_names(C.byref(e), 0, 0, 0, 0, buf, len(buf)) == -1                # DIN_E_ARG
    assert b"bad dtype 3" in lib.din_last_error_string()
