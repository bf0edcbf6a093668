"""conv_halo_rf5_kernel (csrc/conv_halo_rf5.hip: the halo-tiled 5x5 convolution with its filters resident in registers, reduction walked
densely over (tap, chunk)), every instantiation, by name, against the float64 reference and the per-element bars of
tests/test_gpu_conv_fwd_dgrad.py -- its operand builder, references, bar_of, guard bands, NaN prefill and double launch are imported, not
copied; the bars are that file's, unchanged:
    |got - v| <= 2^-7 |v| + 2 (K + 2) 2^-24 S        (K = 25 c_reduction + 2; the kernel never splits its reduction)

The kernel is reached through din_conv_rf5_fwd / din_conv_rf5_dgrad only; DIN_CONV_HALO_RF5=2 forces it on these small maps (unset, the
planner's floor on the pixels of a launch keeps them on the old kernels).  Each row asserts din_conv_rf5_eligible and the line
din_conv_rf5_kernel_names answers before anything is launched.

Shapes, the smallest on which the kernel can still go wrong: nb = 2, 19 x 45 output pixels = 3 x 2 tiles of 8 x 32, ragged on both axes
(more workgroup items than one, the last tile row 3 pixels high, the last tile column 13 wide); pad 2 (border taps two deep on all four
sides: halo rows above / below the image rely on the buffer range check, halo columns on the column test) and one pad-0 row (23 x 49 in);
reduction channels 48 (the dense walk ends in a half step: 150 chunks), 40 (a quarter step; lane groups straddle taps at every position),
56 (three quarters) and 64 (whole steps, no straddle); produced channels 64, 56, 48 and 40 (the second class short, down to 8 channels:
its mask region has 4, 3, 2 and 1 chunks per pixel).  Forward rows run BIAS | RELU and no flags (the harness's two forward modes); the data
gradients none / MASK / ACCUM / MASK | ACCUM.  rf5_dg_64_48_mask is the backbone's launch: 160-byte pitch, the LDS full to the last byte.
The mask is the harness's: +0.0, -0.0, the smallest subnormal and negatives at known positions; views at non-zero offsets (multiples of 8;
one forward output at a multiple of 4), strides wider than the views, ldm != ldi."""
import ctypes as C

import pytest
import torch

from tests import test_gpu_conv_fwd_dgrad as CF
from tests.test_gpu_conv_fwd_dgrad import ACCUM, BIAS, DG, FWD, MASK, P0, RELU, S1, _pad, _row
from tests.test_gpu_kernels import env  # noqa: F401  (the module-scoped library fixture)

RF5 = {"DIN_CONV_HALO_RF5": "2"}
K5, P2 = (5, 5), (2, 2)
TABLE = [(cpt, dg) for dg in (False, True) for cpt in (5, 6, 7, 8)]       # DIN_CONV_HALO_RF5_TABLE: (chunks per tap of the reduction, data gradient)


def _rf5(cpt, dg):
    return f"conv_halo_rf5_kernel<{cpt}, {'true' if dg else 'false'}>"


# shape = (nb, cin, h, w, cout, k, s, p, dil): a forward reduces over cin and produces cout, a data gradient reduces over cout and produces cin
RF5_ROWS = [
    _row("rf5_fwd_48_64", _rf5(6, False), FWD, 0, "bf16", (2, 48, 19, 45, 64, K5, S1, P2, 1), RF5),
    _row("rf5_fwd_40_56", _rf5(5, False), FWD, 0, "bf16", (2, 40, 19, 45, 56, K5, S1, P2, 1), RF5),
    _row("rf5_fwd_56_48_p0", _rf5(7, False), FWD, 0, "bf16", (2, 56, 23, 49, 48, K5, S1, P0, 1), RF5),
    _row("rf5_fwd_64_40_m4", _rf5(8, False), FWD, 0, "bf16", (2, 64, 19, 45, 40, K5, S1, P2, 1), RF5, m4=True),
    _row("rf5_dg_64_48_mask", _rf5(8, True), DG, MASK, "bf16", (2, 48, 19, 45, 64, K5, S1, P2, 1), RF5),
    _row("rf5_dg_48_56_mask_accum", _rf5(6, True), DG, MASK | ACCUM, "bf16", (2, 56, 19, 45, 48, K5, S1, P2, 1), RF5),
    _row("rf5_dg_40_64_accum", _rf5(5, True), DG, ACCUM, "bf16", (2, 64, 19, 45, 40, K5, S1, P2, 1), RF5),
    _row("rf5_dg_40_40_mask", _rf5(5, True), DG, MASK, "bf16", (2, 40, 19, 45, 40, K5, S1, P2, 1), RF5),
    _row("rf5_dg_56_40_p0", _rf5(7, True), DG, 0, "bf16", (2, 40, 23, 49, 56, K5, S1, P0, 1), RF5),
]
IDS = [r["label"] for r in RF5_ROWS]


def _rf5_names(lib, d, which, flags, ldm, moff):
    buf = C.create_string_buffer(256)
    rc = lib.din_conv_rf5_kernel_names(C.byref(d), which, flags, ldm, moff, buf, len(buf))
    assert 0 < rc <= len(buf), f"din_conv_rf5_kernel_names returned {rc}: {lib.din_last_error_string()}"
    return buf.value.decode().split("\n")[:-1]


def _assert_named(lib, L, row, monkeypatch):
    """the row's options are set (and stay set for the caller); every mode of the row is eligible and launches the kernel the row names"""
    for name, value in row["opts"].items():
        monkeypatch.setenv(name, value)
    d = CF._desc(L, row)
    ldm, moff = row["views"][4:]
    for flags in CF._modes(row):
        m = (ldm, moff) if flags & MASK else (0, 0)
        assert lib.din_conv_rf5_eligible(C.byref(d), row["which"], flags, *m) == 1, f"{row['label']}: flags {flags} not eligible"
        got = _rf5_names(lib, d, row["which"], flags, *m)
        assert got == [row["name"]], f"{row['label']}: flags {flags} launch {got}, not {row['name']}"
    return d


def test_rows_cover_every_instantiation_and_flag_form(monkeypatch):
    lib, L = CF._library()
    for row in RF5_ROWS:
        _assert_named(lib, L, row, monkeypatch)
    assert {r["name"] for r in RF5_ROWS} == {_rf5(cpt, dg) for cpt, dg in TABLE}
    assert all(set(CF._modes(r)) == {BIAS | RELU, 0} for r in RF5_ROWS if r["which"] == FWD)
    assert {r["flags"] for r in RF5_ROWS if r["which"] == DG} == {0, MASK, ACCUM, MASK | ACCUM}
    for which, red, prod in ((FWD, 1, 4), (DG, 4, 1)):
        mine = [r for r in RF5_ROWS if r["which"] == which]
        assert {r["shape"][red] for r in mine} == {40, 48, 56, 64} == {r["shape"][prod] for r in mine}
        assert {r["shape"][7] for r in mine} == {P0, P2}


@pytest.mark.parametrize("row", RF5_ROWS, ids=IDS)
def test_bars_bite(row, monkeypatch):
    """the harness's check on the new rows (CPU): a kernel that lost the last 8 reduction channels of the last tap -- the last real chunk of
    the dense walk's partial step -- moves >= 10 % of the produced elements beyond the row's bar; under ACCUM, one that rounded the gradient
    to bf16 before adding the old value moves at least one"""
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
@pytest.mark.parametrize("row", RF5_ROWS, ids=IDS)
def test_conv_halo_rf5_against_fp64(env, row, monkeypatch):
    lib, L, nhwc, ops = env
    d = _assert_named(lib, L, row, monkeypatch)
    nb, cin, h, w, cout, k, s, p, dil, oh, ow = CF._geometry(row["shape"])
    ldi, cioff, ldo, cooff, ldm, moff = row["views"]
    op = CF._operands(row, "cuda")
    tdt = op["tdt"]
    gen = torch.Generator().manual_seed(11)

    which = row["which"]
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
                L.check(lib.din_conv_rf5_fwd(C.byref(d), src.data_ptr(), wpk.data_ptr(), bias.data_ptr() if flags & BIAS else None, out.data_ptr(), flags,
                                             None, 0, None))
            else:
                L.check(lib.din_conv_rf5_dgrad(C.byref(d), src.data_ptr(), wpk.data_ptr(), out.data_ptr(), mask.data_ptr() if flags & MASK else None,
                                               ldm if flags & MASK else 0, moff if flags & MASK else 0, flags, None, 0, None))

        CF._launch_twice_and_compare(f"{row['label']} flags={flags}", launch, wsbuf, 0,
                                     [dict(dest, off=off, c=c, v=v.reshape(*lead, c), bar=bar.reshape(*lead, c), exact=exact,
                                           old=op["old"] if flags & ACCUM else None)])
