"""conv_halo_rf_kernel (csrc/conv_halo_rf.hip: the halo-tiled 3x3 convolution with its filters resident in registers), every instantiation,
by name, against the float64 reference and the per-element bars of tests/test_gpu_conv_fwd_dgrad.py -- its operand builder, references,
bar_of, guard bands, NaN prefill and double launch are imported, not copied; the bars are that file's, unchanged:
    |got - v| <= 2^-7 |v| + 2 (K + 2) 2^-24 S        (K = 9 c_reduction + 2; the kernel never splits its reduction)

The kernel is reached through din_conv_rf_fwd / din_conv_rf_dgrad only; DIN_CONV_HALO_RF=2 forces it on these small maps (unset, the
planner's floor on the pixels of a launch keeps them on the old kernels).  Each row asserts din_conv_rf_eligible and the line
din_conv_rf_kernel_names answers before anything is launched.

Shapes, the smallest on which the kernel can still go wrong: nb = 2, 19 x 45 output pixels = 3 x 2 tiles of 8 x 32, ragged on both axes
(more workgroup items than one, the last tile row 3 pixels high, the last tile column 13 wide); pad 1 (border taps on all four sides: halo
rows above / below the image rely on the buffer range check, halo columns on the column test) and pad-0 rows; reduction channels 72 and 88
(a partial second 64-channel block; its last 32-channel step short of 32) beside 96, 64, 56 and 48; produced channels 88, 72 and 56 (short
of a class, no multiple of 16) beside 96 and 64.  Forward rows run BIAS | RELU and no flags (the harness's two forward modes); the data
gradients none / MASK / ACCUM / MASK | ACCUM.  The mask is the harness's: +0.0, -0.0, the smallest subnormal and negatives at known
positions; views at non-zero offsets (multiples of 8; one forward output at a multiple of 4), strides wider than the views, ldm != ldi.
A mask view at multiples of 4 only is answered "not eligible" (the mask travels by 16-byte LDS-DMA): tests/test_conv_halo_rf_cpu.py."""
import ctypes as C

import pytest
import torch

from tests import test_gpu_conv_fwd_dgrad as CF
from tests.test_gpu_conv_fwd_dgrad import ACCUM, BIAS, DG, FWD, K3, MASK, P0, P1, RELU, S1, _pad, _row
from tests.test_gpu_kernels import env  # noqa: F401  (the module-scoped library fixture)

RF = {"DIN_CONV_HALO_RF": "2"}


def _rf(ti, nks, dg):
    return f"conv_halo_rf_kernel<{ti}, {nks}, {'true' if dg else 'false'}>"


# shape = (nb, cin, h, w, cout, k, s, p, dil): a forward reduces over cin and produces cout, a data gradient reduces over cout and produces cin
RF_ROWS = [
    _row("rf_fwd_96_96", _rf(3, 3, False), FWD, 0, "bf16", (2, 96, 19, 45, 96, K3, S1, P1, 1), RF),
    _row("rf_fwd_64_96", _rf(3, 2, False), FWD, 0, "bf16", (2, 64, 19, 45, 96, K3, S1, P1, 1), RF),
    _row("rf_fwd_72_88_m4", _rf(3, 3, False), FWD, 0, "bf16", (2, 72, 19, 45, 88, K3, S1, P1, 1), RF, m4=True),
    _row("rf_fwd_88_56_p0", _rf(2, 3, False), FWD, 0, "bf16", (2, 88, 21, 47, 56, K3, S1, P0, 1), RF),
    _row("rf_fwd_48_56", _rf(2, 2, False), FWD, 0, "bf16", (2, 48, 19, 45, 56, K3, S1, P1, 1), RF),
    _row("rf_dg_96_96", _rf(3, 3, True), DG, 0, "bf16", (2, 96, 19, 45, 96, K3, S1, P1, 1), RF),
    _row("rf_dg_96_64_mask", _rf(2, 3, True), DG, MASK, "bf16", (2, 64, 19, 45, 96, K3, S1, P1, 1), RF),
    _row("rf_dg_88_72_mask", _rf(3, 3, True), DG, MASK, "bf16", (2, 72, 19, 45, 88, K3, S1, P1, 1), RF),
    _row("rf_dg_72_56_accum", _rf(2, 3, True), DG, ACCUM, "bf16", (2, 56, 19, 45, 72, K3, S1, P1, 1), RF),
    _row("rf_dg_64_88_mask_accum", _rf(3, 2, True), DG, MASK | ACCUM, "bf16", (2, 88, 19, 45, 64, K3, S1, P1, 1), RF),
    _row("rf_dg_48_56_mask_p0", _rf(2, 2, True), DG, MASK, "bf16", (2, 56, 21, 47, 48, K3, S1, P0, 1), RF),
]
IDS = [r["label"] for r in RF_ROWS]


def _rf_names(lib, d, which, flags, ldm, moff):
    buf = C.create_string_buffer(256)
    rc = lib.din_conv_rf_kernel_names(C.byref(d), which, flags, ldm, moff, buf, len(buf))
    assert 0 < rc <= len(buf), f"din_conv_rf_kernel_names returned {rc}: {lib.din_last_error_string()}"
    return buf.value.decode().split("\n")[:-1]


def _assert_named(lib, L, row, monkeypatch):
    """the row's options are set (and stay set for the caller); every mode of the row is eligible and launches the kernel the row names"""
    for name, value in row["opts"].items():
        monkeypatch.setenv(name, value)
    d = CF._desc(L, row)
    ldm, moff = row["views"][4:]
    for flags in CF._modes(row):
        m = (ldm, moff) if flags & MASK else (0, 0)
        assert lib.din_conv_rf_eligible(C.byref(d), row["which"], flags, *m) == 1, f"{row['label']}: flags {flags} not eligible"
        got = _rf_names(lib, d, row["which"], flags, *m)
        assert got == [row["name"]], f"{row['label']}: flags {flags} launch {got}, not {row['name']}"
    return d


def test_rows_cover_every_instantiation_and_flag_form(monkeypatch):
    lib, L = CF._library()
    for row in RF_ROWS:
        _assert_named(lib, L, row, monkeypatch)
    assert {r["name"] for r in RF_ROWS} == {_rf(ti, nks, dg) for ti in (2, 3) for nks in (2, 3) for dg in (False, True)}
    assert {r["flags"] for r in RF_ROWS if r["which"] == DG} == {0, MASK, ACCUM, MASK | ACCUM}


@pytest.mark.parametrize("row", RF_ROWS, ids=IDS)
def test_bars_bite(row, monkeypatch):
    """the harness's check on the new rows (CPU): a kernel that lost the last 8 reduction channels of the last tap moves >= 10 % of the
    produced elements beyond the row's bar; under ACCUM, one that rounded the gradient to bf16 before adding the old value moves at least one"""
    lib, L = CF._library()
    _assert_named(lib, L, row, monkeypatch)
    op = CF._operands(row)
    flags = 0 if row["which"] == 0 else row["flags"]
    v, S, _ = CF._expect(row, op, flags)
    bar = CF.bar_of(row, v, S, 0)
    lost = op["last"] * op["on"] if flags & MASK else op["last"]
    share = float((lost.abs() > bar).double().mean())
    assert share >= 0.10, f"{row['label']}: dropping 8 channels of the last tap moves only {share:.3f} of the elements beyond the bar"
    if flags & ACCUM:
        conv = v - op["old"].double()
        twice = (conv.bfloat16().double() + op["old"].double()).to(op["tdt"]).double()
        assert int(((twice - v).abs() > bar).sum()) >= 1, f"{row['label']}: a second bf16 rounding before the accumulate passes the bar everywhere"


@pytest.mark.gpu
@pytest.mark.parametrize("row", RF_ROWS, ids=IDS)
def test_conv_halo_rf_against_fp64(env, row, monkeypatch):
    lib, L, nhwc, ops = env
    d = _assert_named(lib, L, row, monkeypatch)
    nb, cin, h, w, cout, k, s, p, dil, oh, ow = CF._geometry(row["shape"])
    ldi, cioff, ldo, cooff, ldm, moff = row["views"]
    which = row["which"]
    op = CF._operands(row, "cuda")
    tdt = op["tdt"]
    gen = torch.Generator().manual_seed(11)

    wdev = op["w"].float().cuda()
    wpk = torch.empty(lib.din_conv_packed_elems(C.byref(d), which), dtype=tdt, device="cuda")
    L.check(lib.din_conv_pack_weights(C.byref(d), wdev.data_ptr(), None, wpk.data_ptr(), which, None))
    if which == 0:
        src = CF._view(op["x"], tdt, ldi, cioff, _pad(cin, 8))
        lead, ld, off, c = (nb, oh, ow), ldo, cooff, cout
        bias = op["bias"].cuda()
    else:
        src = CF._view(op["g"], tdt, ldo, cooff, _pad(cout, 8))
        lead, ld, off, c = (nb, h, w), ldi, cioff, cin
        mask = CF._view(op["mask"], tdt, ldm, moff, cin)
    dest = CF._guarded(lead, ld, tdt, gen)
    out = dest["out"]
    wsbuf, _ = CF._guarded_workspace(0)

    for flags in CF._modes(row):
        v, S, exact = CF._expect(row, op, flags)
        bar = CF.bar_of(row, v, S, 0).clamp_min(1e-300)

        def launch():
            if which == 0:
                L.check(lib.din_conv_rf_fwd(C.byref(d), src.data_ptr(), wpk.data_ptr(), bias.data_ptr() if flags & BIAS else None, out.data_ptr(), flags,
                                            None, 0, None))
            else:
                L.check(lib.din_conv_rf_dgrad(C.byref(d), src.data_ptr(), wpk.data_ptr(), out.data_ptr(), mask.data_ptr() if flags & MASK else None,
                                              ldm if flags & MASK else 0, moff if flags & MASK else 0, flags, None, 0, None))

        CF._launch_twice_and_compare(f"{row['label']} flags={flags}", launch, wsbuf, 0,
                                     [dict(dest, off=off, c=c, v=v.reshape(*lead, c), bar=bar.reshape(*lead, c), exact=exact,
                                           old=op["old"] if flags & ACCUM else None)])
