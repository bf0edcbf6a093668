"""GPU (-m gpu): the split-bf16 contraction mode DIN_F32_BF16X3 (fp32 storage, three bf16 parts per operand, three
v_mfma_f32_16x16x32_bf16 per 16-byte chunk pair; include/din_hip.h) held to the bars of the EXACT fp32 mode, unchanged.

Kernel rows (SPLIT_ROWS): one per kernel family, on the shapes of the fp32 rows of tests/test_gpu_conv_fwd_dgrad.py so the planner lands on
the same tiles, run through that file's own GPU test body (guarded views, separate mask tensor, per-element bars 2 (K + 2) 2^-24 S, two
launches) with the descriptor's dtype switched to DIN_F32_BF16X3.  Before that each row asserts that din_conv_kernel_names answers the
DIN_F32 lines with only the T token changed (float -> f32x3; the split-K finish stays <float>) and that the packed filter bank is
bit-identical to the DIN_F32 bank.  SMALL_K: 1x1 rows with 4 / 8 reduction channels, where a missing cross product cannot hide behind the
summation term of the bar (tests/test_split_cpu.py shows in emulation that the two-part form and every five-product form fail them).

Weight gradient (WGRAD_ROWS): the two fp32 shapes of tests/test_gpu_wgrad.py and a short reduction (16 pixels, 1x1, 8 -> 64) under that
file's fp32 bars, plain and production epilogues (scale, <w, dW> and the bias gradient included), guard bands around every output.

Same operands, both modes: on the 3x3 128x128 forward row and the first weight-gradient row rms(err_split) <= 4 rms(err_exact) -- a
condition, not a measurement (the emulation gives <= 1.0 for a correct split and >= 17 for a two-part one at these K); the measured ratio
is printed and recorded in profiles/fp32_split_test_margins.txt.

Model level: Dynamic_volleyball under cfg.backbone_dtype = 'fp32_bf16x3' through the very assertions tests/test_gpu_din_model.py holds the
'fp32' mode to on model_vgg16_96x160_nfb64 / model_inv3_139x203_nfb64 (that test's body is called with a Config whose backbone_dtype reads
'fp32_bf16x3'), one stage-1 forward + backward on stage1_vgg16_96x160_t1 through tests/test_gpu_stage1.py's, and a survey of every conv
entry-point call of those runs: all carry the new dtype and resolve to f32x3 kernels, none to a <float> contraction kernel."""
import ctypes as C
import os

import pytest
import torch

from tests.conftest import Measured
from tests import test_gpu_conv_fwd_dgrad as CF
from tests.test_gpu_conv_fwd_dgrad import ACCUM, DG, FWD, K1, K3, K7, K17, K71, MASK, P0, P1, S1, S2, _fast
from tests.test_gpu_kernels import env, rel  # noqa: F401  (env: the module-scoped library fixture)

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _split_row(label, name, which, flags, shape):
    return CF._row(label, name, which, flags, "fp32", shape)


# name: what the row's launch resolves to under DIN_F32_BF16X3 (the DIN_F32 name of the same shape with the T token changed)
SPLIT_ROWS = [
    _split_row("x3_128_fwd", _fast("f32x3", 128, 128, 2, 2, 8, 2, 0, 0, 0, 0), FWD, 0, (2, 13, 19, 23, 118, K3, S1, P1, 1)),
    _split_row("x3_160_dg_accum", _fast("f32x3", 128, 160, 2, 2, 8, 2, 0, 0, 0, 0), DG, ACCUM, (2, 150, 19, 23, 38, K17, S1, (0, 3), 1)),
    _split_row("x3_192_fwd", _fast("f32x3", 128, 192, 2, 2, 8, 2, 0, 0, 0, 0), FWD, 0, (2, 22, 23, 19, 182, K71, S1, (3, 0), 1)),
    _split_row("x3_64_dg_mask", _fast("f32x3", 128, 64, 2, 2, 8, 2, 0, 0, 0, 0), DG, MASK, (2, 13, 19, 23, 22, K3, S1, P1, 1)),
    _split_row("x3_96_fwd_s2", _fast("f32x3", 128, 96, 2, 2, 8, 2, 0, 0, 0, 0), FWD, 0, (2, 18, 39, 47, 86, K3, S2, P1, 1)),
    # the LDS-staged epilogue (produced channels at multiples of 4): plain stores and the batched MASK / ACCUM form
    _split_row("x3_128_staged_fwd", _fast("f32x3", 128, 128, 2, 2, 8, 2, 0, 0, 0, 0), FWD, 0, (2, 13, 19, 23, 116, K3, S1, P1, 1)),
    _split_row("x3_64_staged_dg_mask", _fast("f32x3", 128, 64, 2, 2, 8, 2, 0, 0, 0, 0), DG, MASK, (2, 12, 19, 23, 22, K3, S1, P1, 1)),
    _split_row("x3_160_staged_dg_mask_accum", _fast("f32x3", 128, 160, 2, 2, 8, 2, 0, 0, 0, 0), DG, MASK | ACCUM, (2, 148, 19, 23, 22, K17, S1, (0, 3), 1)),
    _split_row("x3_256x64_fwd_p0", _fast("f32x3", 256, 64, 4, 1, 4, 4, 0, 0, 0, 0), FWD, 0, (2, 6, 365, 367, 27, K3, S1, P0, 1)),
    _split_row("x3_gen64_fwd_7x7", "conv_gather_generic_kernel<f32x3,64>", FWD, 0, (2, 5, 19, 23, 27, K7, S1, (3, 3), 1)),
    _split_row("x3_gen128_dg_s2_d2", "conv_gather_generic_kernel<f32x3,128>", DG, 0, (2, 70, 39, 47, 10, K3, S2, (2, 2), 2)),
    _split_row("x3_splitk_fwd", "conv_splitk_finish_kernel<float>", FWD, 0, (2, 42, 21, 25, 182, K3, S1, P1, 1)),
]
SMALL_K = [
    _split_row("x3_k4_fwd_1x1", _fast("f32x3", 128, 64, 2, 2, 8, 2, 0, 0, 0, 0), FWD, 0, (1, 4, 16, 16, 64, K1, S1, P0, 1)),
    _split_row("x3_k8_fwd_1x1", _fast("f32x3", 128, 64, 2, 2, 8, 2, 0, 0, 0, 0), FWD, 0, (1, 8, 16, 16, 64, K1, S1, P0, 1)),
    _split_row("x3_k4_dg_1x1", _fast("f32x3", 128, 64, 2, 2, 8, 2, 0, 0, 0, 0), DG, 0, (1, 64, 16, 16, 4, K1, S1, P0, 1)),
]
ALL_ROWS = SPLIT_ROWS + SMALL_K


_FP32_DESC = CF._desc                  # (the GPU rows patch CF._desc; this is the fp32 original)


def _descs(L, row):
    d, e = _FP32_DESC(L, row), _FP32_DESC(L, row)
    e.dtype = L.DIN_F32_BF16X3
    return d, e


def _to_split_token(names):
    return [n.replace("<float,", "<f32x3,") if not n.startswith("conv_splitk_finish_kernel") else n for n in names]


def _assert_names(lib, L, row):
    d, e = _descs(L, row)
    ldm, moff = row["views"][4:]
    for flags in CF._modes(row):
        a = (row["which"], flags, ldm if flags & MASK else 0, moff if flags & MASK else 0)
        exact, split = CF._names(lib, d, *a), CF._names(lib, e, *a)
        assert split == _to_split_token(exact), f"{row['label']}: {split} is not {exact} with the T token changed"
        assert row["name"] in split and any("f32x3" in n for n in split) and not any("<float," in n for n in split), (row["label"], split)
    return d, e


@pytest.mark.parametrize("row", ALL_ROWS, ids=[r["label"] for r in ALL_ROWS])
def test_rows_resolve_to_split_kernels(row):
    """(no GPU) every row names the f32x3 form of the kernel its DIN_F32 twin resolves to"""
    lib, L = CF._library()
    _assert_names(lib, L, row)


@pytest.mark.gpu
@pytest.mark.parametrize("row", ALL_ROWS, ids=[r["label"] for r in ALL_ROWS])
def test_split_kernel_against_fp64(env, row, monkeypatch):
    lib, L, nhwc, ops = env
    d, e = _assert_names(lib, L, row)
    which = row["which"]
    w = CF._operands(row, "cuda")["w"].float().cuda()
    banks = []
    for desc in (d, e):
        assert lib.din_conv_packed_elems(C.byref(desc), which) == lib.din_conv_packed_elems(C.byref(d), which)
        wpk = torch.full((lib.din_conv_packed_elems(C.byref(desc), which),), float("nan"), dtype=torch.float32, device="cuda")
        L.check(lib.din_conv_pack_weights(C.byref(desc), w.data_ptr(), None, wpk.data_ptr(), which, None))
        banks.append(wpk)
    torch.cuda.synchronize()
    assert torch.equal(banks[0].view(torch.int32), banks[1].view(torch.int32)), f"{row['label']}: the packed bank differs from the DIN_F32 bank"
    # the fp32 harness, bars and guards of tests/test_gpu_conv_fwd_dgrad.py, on the same row with the new dtype in its descriptor
    monkeypatch.setattr(CF, "_desc", lambda L_, row_: _descs(L_, row_)[1])
    CF.test_conv_kernel_against_fp64(env, row, monkeypatch)


def _rms(t):
    return float(t.double().pow(2).mean().sqrt())


@pytest.mark.gpu
def test_same_operand_ratio_forward(env):
    """the 3x3 128x128 forward row through both modes on the same buffers: rms error against float64, split <= 4 x exact"""
    lib, L, nhwc, ops = env
    row = SPLIT_ROWS[0]
    nb, cin, h, w, cout, k, s, p, dil, oh, ow = CF._geometry(row["shape"])
    ldi, cioff, ldo, cooff, _, _ = row["views"]
    op = CF._operands(row, "cuda")
    src = CF._view(op["x"], torch.float32, ldi, cioff, CF._pad(cin, 4))
    wdev = op["w"].float().cuda()
    err = []
    for desc in _descs(L, row):
        wpk = torch.empty(lib.din_conv_packed_elems(C.byref(desc), 0), dtype=torch.float32, device="cuda")
        L.check(lib.din_conv_pack_weights(C.byref(desc), wdev.data_ptr(), None, wpk.data_ptr(), 0, None))
        wsb = lib.din_conv_workspace_bytes(C.byref(desc), 0)
        ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device="cuda")
        out = torch.zeros(nb, oh, ow, ldo, dtype=torch.float32, device="cuda")
        L.check(lib.din_conv_fwd(C.byref(desc), src.data_ptr(), wpk.data_ptr(), None, out.data_ptr(), 0, ws.data_ptr() if wsb else None, wsb, None))
        torch.cuda.synchronize()
        err.append(_rms(out[..., cooff:cooff + cout].reshape(-1, cout).cpu().double() - op["v"]))
    ratio = Measured(err[1] / max(err[0], 1e-300))
    print(f"forward {row['label']}: rms(err) exact {err[0]:.3e} split {err[1]:.3e} ratio {float(ratio):.3f} (rms(v) {_rms(op['v']):.3e})")
    assert ratio <= 4.0


# ---- weight gradient -------------------------------------------------------------------------------------------------------------------
from tests import test_gpu_wgrad as WG  # noqa: E402

WGRAD_ROWS = [
    WG._row("x3_w_3x3_s2_d2", "conv_wgrad_f32x3_kernel", (128, 128), "fp32", (2, 13, 27, 29, 40, K3, S2, (2, 2), 2), (20, 4, 48, 4)),
    WG._row("x3_w_7x1_p0", "conv_wgrad_f32x3_kernel", (128, 128), "fp32", (1, 20, 23, 19, 136, K71, S1, P0, 1), (28, 4, 148, 8)),
    # a short reduction: ONE 16-pixel k-step -- a missing cross product has no long sum to hide in
    WG._row("x3_w_short_1x1", "conv_wgrad_f32x3_kernel", (128, 128), "fp32", (1, 8, 4, 4, 64, K1, S1, P0, 1), (12, 4, 72, 8)),
]


def _wgrad_desc(L, row, dtype):
    nb, cin, h, w, cout, k, s, p, dil, oh, ow = WG._geometry(row)
    d = L.ConvDesc()
    d.nb, d.h, d.w, d.cin, d.oh, d.ow, d.cout = nb, h, w, cin, oh, ow, cout
    d.kh, d.kw, d.sh, d.sw, d.ph, d.pw, d.dh, d.dw = k[0], k[1], s[0], s[1], p[0], p[1], dil, dil
    d.ldi, d.cioff, d.ldo, d.cooff = row["ld"]
    d.dtype, d.in_u8 = dtype, 0
    return d


def _wgrad_names(lib, d):
    buf = C.create_string_buffer(512)
    assert 0 < lib.din_conv_kernel_names(C.byref(d), 2, 0, 0, 0, buf, len(buf)) <= len(buf), lib.din_last_error_string()
    return buf.value.decode().split("\n")[:-1]


def _wgrad_launch(lib, L, row, d, production):
    """one guarded din_conv_wgrad launch (twice) of the row under descriptor d -> (dw, dbias, wdot) on the host"""
    nb, cin, h, w, cout, k, s, p, dil, oh, ow = WG._geometry(row)
    ldi, cioff, ldo, cooff = row["ld"]
    op = WG._operands(row)
    xin = WG._view(op["x"], torch.float32, ldi, cioff, WG._pad(cin, 4))
    gin = WG._view(op["gz"], torch.float32, ldo, cooff, WG._pad(cout, 8))
    wsb = lib.din_conv_workspace_bytes(C.byref(d), 2)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device="cuda")
    ndw = cout * cin * k[0] * k[1]
    (dw_buf, dw), (db_buf, db), (wd_buf, wdot) = WG._guarded(ndw), WG._guarded(cout), WG._guarded(cout)
    scale_d, w_d = op["scale"].cuda(), op["w"].cuda()
    for _ in range(2):
        ws.fill_(0x7f)
        dw.fill_(float("nan"))
        if production:                                   # what nhwc.py's backbone passes: scale, w, wdot, dbias added into (accumulate 2)
            db.copy_(op["db_pre"]), wdot.copy_(op["wdot_pre"])
            args = (scale_d.data_ptr(), w_d.data_ptr(), wdot.data_ptr(), 2)
        else:
            db.fill_(float("nan")), wdot.fill_(float("nan"))
            args = (None, None, None, 0)
        L.check(lib.din_conv_wgrad(C.byref(d), xin.data_ptr(), gin.data_ptr(), dw.data_ptr(), db.data_ptr(), *args, ws.data_ptr(), wsb, None))
        torch.cuda.synchronize()
        for buf, n in ((dw_buf, ndw), (db_buf, cout), (wd_buf, cout)):
            assert bool((buf[:WG.NG] == WG.GUARD).all()) and bool((buf[WG.NG + n:] == WG.GUARD).all()), f"{row['name']}: wrote outside an output"
    return dw.cpu().reshape(op["raw"].shape), db.cpu(), wdot.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("production", (False, True), ids=("plain", "production"))
@pytest.mark.parametrize("row", WGRAD_ROWS, ids=[r["name"] for r in WGRAD_ROWS])
def test_split_wgrad_against_fp64(env, row, production):
    lib, L, nhwc, ops = env
    d, e = _wgrad_desc(L, row, L.DIN_F32), _wgrad_desc(L, row, L.DIN_F32_BF16X3)
    exact, split = _wgrad_names(lib, d), _wgrad_names(lib, e)
    assert exact[0] == "conv_wgrad_f32_kernel" and split[0] == row["kernel"] and split[1:] == exact[1:], (exact, split)
    bm, bn = C.c_int32(0), C.c_int32(0)
    L.check(lib.din_conv_kernel_tile(C.byref(e), 2, C.byref(bm), C.byref(bn)))
    assert (bm.value, bn.value) == row["code"]
    assert lib.din_conv_workspace_bytes(C.byref(e), 2) == lib.din_conv_workspace_bytes(C.byref(d), 2)
    op = WG._operands(row)
    raw, bar = op["raw"], WG.BAR["fp32"]
    dw, db, wdot = _wgrad_launch(lib, L, row, e, production)
    if not production:
        assert rel(dw, raw) <= bar
        assert WG._channel_err(db, op["colsum"], op["colabs"]) <= WG.BAR_BIAS
        assert bool(wdot.isnan().all()), f"{row['name']}: wdot written without being asked for"
        return
    scale64, w64 = op["scale"].double()[:, None, None, None], op["w"].double()
    dot, dot_abs = (w64 * raw).sum((1, 2, 3)), (w64 * raw).abs().sum((1, 2, 3))
    assert rel(dw, scale64 * raw) <= bar
    assert WG._channel_err(db, op["db_pre"].double() + op["colsum"], op["colabs"] + op["db_pre"].double().abs()) <= WG.BAR_BIAS
    assert WG._channel_err(wdot, op["wdot_pre"].double() + dot, dot_abs + op["wdot_pre"].double().abs()) <= bar


@pytest.mark.gpu
def test_same_operand_ratio_wgrad(env):
    lib, L, nhwc, ops = env
    row = WGRAD_ROWS[0]
    raw = WG._operands(row)["raw"]
    err = [_rms(_wgrad_launch(lib, L, row, _wgrad_desc(L, row, dt), False)[0].double() - raw) for dt in (L.DIN_F32, L.DIN_F32_BF16X3)]
    ratio = Measured(err[1] / max(err[0], 1e-300))
    print(f"wgrad {row['name']}: rms(err) exact {err[0]:.3e} split {err[1]:.3e} ratio {float(ratio):.3f} (rms(dW) {_rms(raw):.3e})")
    assert ratio <= 4.0


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_unknown_dtype_is_still_refused(env):
    lib, L, nhwc, ops = env
    row = SPLIT_ROWS[0]
    d = _FP32_DESC(L, row)
    d.dtype = 3
    t = torch.zeros(1 << 16, dtype=torch.float32, device="cuda")
    before = t.clone()
    p = t.data_ptr()
    assert lib.din_conv_fwd(C.byref(d), p, p, None, p, 0, None, 0, None) == -1
    assert b"bad dtype 3" in lib.din_last_error_string()
    assert lib.din_conv_dgrad(C.byref(d), p, p, p, None, 0, 0, 0, None, 0, None) == -1
    assert lib.din_conv_wgrad(C.byref(d), p, p, p, None, None, None, None, 0, p, 1 << 18, None) == -1
    src = L.ConvSrc() if hasattr(L, "ConvSrc") else None
    if src is not None:
        src.dout, src.wpk_t, src.cout, src.ldo, src.cooff = p, p, 8, 8, 0
        assert lib.din_conv1x1_dgrad_multi(1, C.byref(src), 3, 1, 4, 4, 8, 8, 0, p, None, 0, 0, 0, None) == -1
    torch.cuda.synchronize()
    assert torch.equal(t, before)


# ---- model level -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from din_amd import _lib
    _lib.load()
    return torch.device("cuda")


def _split_config(monkeypatch):
    """din_amd.config.Config as the model tests of the other files import it, with backbone_dtype reading 'fp32_bf16x3' where they set 'fp32'"""
    from din_amd import config

    class SplitConfig(config.Config):
        @property
        def backbone_dtype(self):
            return "fp32_bf16x3"

        @backbone_dtype.setter
        def backbone_dtype(self, value):
            assert value == "fp32", value

    monkeypatch.setattr(config, "Config", SplitConfig)


CONTRACTIONS = ("din_conv_fwd", "din_conv_fwd2", "din_conv_dgrad", "din_conv_dgrad_x", "din_conv_wgrad")


def _survey(monkeypatch):
    """records (entry point, dtype, kernel names) of every conv entry-point call made through the loaded library"""
    from din_amd import _lib as L
    lib, calls = L.load(), []

    def wrap(name, real):
        def call(*a):
            buf = C.create_string_buffer(2048)
            rc = real(*a)
            if name == "din_conv1x1_dgrad_multi":          # (nsrc, srcs, dtype, nb, h, w, cin, ldi, cioff, din, mask, ldm, moff, flags, stream)
                dtype = int(a[2])
                n = lib.din_conv1x1_dgrad_multi_kernel_names(*a[:9], *a[11:14], buf, len(buf))
            elif name == "din_conv_fwd2":                  # (d, in, wpk, bias, out, out2, ldo2, cooff2, csplit, craw, flags, ...)
                dtype = int(a[0]._obj.dtype)
                n = lib.din_conv_fwd2_kernel_names(a[0], *a[6:11], buf, len(buf))
            elif name == "din_conv_dgrad_x":               # (d, dout, wpk_t, din, mask, ldm, moff, flags, x, ...)
                dtype = int(a[0]._obj.dtype)
                n = lib.din_conv_dgrad_x_kernel_names(a[0], a[8], *a[5:8], buf, len(buf))
            else:
                d = a[0]._obj
                dtype = int(d.dtype)
                which = {"din_conv_fwd": 0, "din_conv_wgrad": 2}.get(name, 1)
                flags = 0 if which == 2 else int(a[{"din_conv_fwd": 5, "din_conv_dgrad": 7}[name]])
                ldm, moff = (int(a[5]), int(a[6])) if which == 1 else (0, 0)
                n = lib.din_conv_kernel_names(C.byref(d), which, flags, ldm if flags & MASK else 0, moff if flags & MASK else 0, buf, len(buf))
            assert rc != 0 or 0 < n <= len(buf), f"{name}: launched, but its reporter returned {n}"
            calls.append((name, dtype, buf.value.decode().split()))
            return rc
        return call

    for name in CONTRACTIONS + ("din_conv1x1_dgrad_multi",):
        monkeypatch.setattr(lib, name, wrap(name, getattr(lib, name)))
    return calls


def _assert_survey(calls, L, want=("din_conv_fwd", "din_conv_dgrad", "din_conv_wgrad")):
    assert {c[0] for c in calls} >= set(want), sorted({c[0] for c in calls})
    for name, dtype, names in calls:
        assert dtype == L.DIN_F32_BF16X3, f"{name} was called with dtype {dtype}"
        assert not any(n.startswith(("conv_gather_fast_kernel<float", "conv_gather_generic_kernel<float", "conv_wgrad_f32_kernel")) for n in names), (name, names)
        assert any("f32x3" in n for n in names), (name, names)
    print(f"{len(calls)} conv entry-point calls, all DIN_F32_BF16X3: " + ", ".join(f"{n} x{sum(c[0] == n for c in calls)}" for n in sorted({c[0] for c in calls})))


@pytest.mark.gpu
@pytest.mark.parametrize("fixture", ("model_vgg16_96x160_nfb64", "model_inv3_139x203_nfb64"))
def test_model_under_split_mode_meets_the_fp32_assertions(gpu, fixture, monkeypatch):
    from din_amd import _lib as L
    from tests import test_gpu_din_model as DM
    _split_config(monkeypatch)
    calls = _survey(monkeypatch)
    DM.test_whole_model_logits_match_reference_golden(gpu, os.path.join(GOLDEN, fixture + ".npz"))
    _assert_survey(calls, L)


@pytest.mark.gpu
def test_stage1_under_split_mode_meets_the_fp32_assertions(gpu, monkeypatch):
    from din_amd import _lib as L
    from tests import test_gpu_stage1 as S1
    _split_config(monkeypatch)
    calls = _survey(monkeypatch)
    S1.test_basenet_matches_reference_stage1_golden(gpu, os.path.join(GOLDEN, "stage1_vgg16_96x160_t1.npz"))
    _assert_survey(calls, L)
