"""The two weight-gradient entry points that run more than one layer per launch -- din_conv_wgrad_group (conv_wgrad_pipe_group_kernel<BCO, 256,
WIDE, 8> + conv_wgrad_reduce_group_kernel: up to 16 layers) and din_conv1x1_wgrad_multi (conv_wgrad_1x1_multi_kernel<CPP> + one
conv_wgrad_reduce_kernel per source: the 1x1 convs reading one tensor view) -- by kernel name, against a float64 reference, with the harness of
tests/test_gpu_wgrad.py (_view, _guarded, POISON, GUARD, NG, BAR_BIAS) and the row / reporter / bite layout of tests/test_gpu_conv_multi.py.

One row of ROWS per code path.  `names` are the lines the entry point's own reporter (din_conv_wgrad_group_kernel_names,
din_conv1x1_wgrad_multi_kernel_names) answers under the row's options: asserted before anything is launched and, for all rows, on the CPU.
A group row also states the slice groups of its reduce launch (nsg 1 / 4 / 16) and, where it has one, the item the group plan cuts into
exactly ONE pixel slice: both are the library's answer (din_conv_wgrad_group_slices: the plan the launch makes), not recomputed here.

Group keys.  A sweep of din_conv_wgrad_group_key (host only) over 1x1 / 3x3 / 1x7 / 7x1 filters, 16 ... 776 input and 112 ... 504 output
channels, maps of 1 x 1 x 33 ... 2 x 67 x 68 pixels with rows below and above 32 pixels reaches every key 2 * bco + wide (bco 128 / 192 /
256: the filter tile plan_wgrad pads the bank to; wide: an output row holds a 32-pixel stage): test_group_key_sweep_reaches_every_key
repeats it.  No key is unreachable (UNREACHABLE is empty); each has a row.

Rows of din_conv_wgrad_group carry: 2 and 16 items; 1x7, 7x1, 3x3 and 1x1 layers of different map sizes in one launch; banks of two
filter tiles (384 rows on 192, 504 on 256); kh kw cin_pad no multiple of 256 (all but g128w_nsg16: a 1x1 of 256 channels, so that each item is
one workgroup per slice and 143 slices fit the chip); M no multiple of 32 on every item; input and gradient views at channel offsets that differ
between items and are never 0; an item of one slice; reduce slice groups 1, 4 and 16.  Rows of din_conv1x1_wgrad_multi (DIN_WGRAD_1X1_MULTI=2
forces the kernel on small maps): Cin 192 / 256 / 288, 2 / 3 / 4 sources, the production list (64, 112, 64) with a gradient view at
cooff = 64, ldo = 288 and one at ldo = cout, cooff = 0, a 128-row source alone in its class, a list the greedy deal of plan_wgrad_1x1_multi
must flip to the other class for (the lighter class already holds two sources), a 16-channel source; 37 pixels (127 of the 128 persistent
workgroups of a class have no stage: their slabs must still reduce to zero), 2 x 16 x 24 = 768 (whole stages), 3 x 53 x 59 = 9381 (146
stages + 37 pixels: workgroups with two stages and a ragged last one); the input at cioff = 8 of ldi = cin + 16.

Modes (each row: plain, production, accumulate; one row per entry point also acc3), each launched twice from the same prefill:
    plain        scale = w = wdot = null, accumulate 0: dW, dbias NaN-prefilled and overwritten (the memset path); the wdot buffers are decoys
    production   scale, w, wdot, accumulate 2: dW NaN-prefilled, dbias / wdot added into a random old value; dbias null on one unit (the last
                 source / item 1, as the backbones pass a pooled branch): its decoy buffer stays NaN
    accumulate   accumulate 1: dW += scale * dW_raw from a random old value, dbias / wdot NaN-prefilled and overwritten
    acc3         accumulate 3: the old dW kept and dbias / wdot added into
Operands are bf16 views (POISON outside the view, zeros in the chunk padding); dW / dbias / wdot sit between guard bands; the workspace is
0x7f before every launch between 0x5a guard bytes that must survive; one more unit than the call lists has its outputs allocated and must
keep them.

Reference, float64 on the stored bf16 values: dW[co][ci][r][t] = scale[co] * sum_m g[m][co] * x_shifted[m][ci] and S = the same sum over
absolute values; dbias[co] = sum_m g[m][co]; wdot[co] = sum <w, dW_raw> with S = sum |w| S_dW; an old value that is added into joins both.
Bars: per element |err| <= 1e-5 * S (tests/test_gpu_wgrad.py's BAR_BIAS, unchanged), asserted as max(err / bar) <= 1 (a Measured), printed per
row, mode and launch (profiles/wgrad_multi_test_margins.txt).

Pacing (DIN_WGRAD_GROUP_PACE=1 / 2, rows with 2-3 and 4-5 k tiles): dW must equal the unpaced launch bit for bit -- the slice partials and
conv_wgrad_reduce_group_kernel's fixed-order sum do not depend on timing.  dbias and wdot do: both are fp32 atomicAdds of several workgroups
(one per pixel slice in wgrad_pipe_body, one per 256-column chunk in wgrad_reduce_body), whose order changes from launch to launch with
or without pacing; they are held to the bar instead.
Fallbacks (n = 1, n = 17, two keys, an fp32 item): dW / dbias / wdot bit-identical to din_conv_wgrad per layer on the same workspace.  For
the same reason (atomic order) those rows use operands in {-1, 0, 1} and power-of-two scales: every sum is exact in fp32 whatever its order,
so the outputs also equal the float64 reference exactly.

FOUND with this file:
    kernels: no defect.  The two suspects hold: the 127 idle workgroups per class of the 37-pixel row write zero slabs over the 0x7f
    workspace (m192_four_37), and the dbias atomics of two sources sharing a class land in their own buffers (every multi row).
    host, by reading the code for the refusal rows: din_conv_wgrad_group and din_conv1x1_wgrad_multi checked the pointers of item / source j
    only after they had zeroed the dbias / wdot of items / sources 0 .. j - 1 (accumulate bit 1 clear): a refused call had written.  The
    layer-by-layer path of din_conv_wgrad_group ran layers 0 .. j - 1 before it found the workspace too small for layer j.
FIXED with this file: both entry points check every item / source before the first memset or launch; the layer-by-layer path checks the
    largest single-item workspace need first.  No kernel body changed.  The library gained the reporters and the slice query; launch and
    reporter walk one table each (DIN_WGRAD_PIPE_GROUP_TABLE, DIN_WGRAD_1X1_MULTI_TABLE).
MEASURED (MI355X, two visits, the second in profiles/wgrad_multi_test_margins.txt; max(err / bar) over modes, launches and visits -- dW
    and wdot repeat digit for digit, dbias moves by up to 0.002 with the order of its atomics): dW / dbias / wdot
        m288_production_9381 0.0012 / 0.0043 / 0.0001      m192_four_37 0.0107 / 0.0038 / 0.0008
        m256_two_128alone_768 0.0028 / 0.0018 / 0.0003     m256_flip_16ch_9381 0.0013 / 0.0053 / 0.0001
        g128w_nsg16_one_slice 0.0104 / 0.0039 / 0.0006     g192w_four_filter_shapes 0.0036 / 0.0029 / 0.0002
        g256w_two_tiles_pace23 0.0039 / 0.0030 / 0.0003    g128n_sixteen_items 0.0054 / 0.0029 / 0.0006
        g192n_two_tiles_pace45_one_slice 0.0092 / 0.0043 / 0.0014      g256n 0.0046 / 0.0020 / 0.0005
    i.e. errors of about 1e-7 S, the fp32 rounding of sums of exact products: the 1e-5 bar is two decades above what a correct kernel
    shows, and test_bars_bite holds it at least one decade below what each wrong model of its list moves.

The old tests test_conv1x1_wgrad_multi_source / test_conv_wgrad_group_matches_per_layer_launches (tests/test_gpu_kernels.py) stay: they hold
the exact production source lists (5b_192, 5c_256, 5d_288) and the InceptionC block's shapes, which no row here repeats."""
import ctypes as C
import os
import re

import pytest
import torch

from tests.conftest import ROOT, Measured
from tests.test_gpu_conv_fwd_dgrad import _library
from tests.test_gpu_kernels import env  # noqa: F401  (the module-scoped library fixture)
from tests.test_gpu_wgrad import BAR_BIAS, GUARD, NG, POISON, _guarded, _view

BAR = BAR_BIAS                              # per element, times S (fp32 sums of exact products)
NAMES_FILE = os.path.join(ROOT, "profiles", "wgrad_multi_kernel_names.txt")
MODES = {"plain": (False, 0), "production": (True, 2), "accumulate": (True, 1), "acc3": (True, 3)}      # mode -> (scale / w / wdot given, accumulate)
MULTI_ON = {"DIN_WGRAD_1X1_MULTI": "2"}
WSG = 4096                                  # guard bytes on each side of the workspace
UNREACHABLE = set()                         # group keys no descriptor with slices to reduce reaches (the sweep: none)
K1, K3, K17, K71 = (1, 1), (3, 3), (1, 7), (7, 1)
P0, P1, P03, P30 = (0, 0), (1, 1), (0, 3), (3, 0)


def _pad(n, m):
    return (n + m - 1) // m * m


def _multi(label, cin, srcs, pix, acc3=False):
    """din_conv1x1_wgrad_multi: srcs = (cout, ldo, cooff) per source; the input at cioff = 8 of ldi = cin + 16; production: dbias null on the last"""
    return dict(kind="multi", label=label, cin=cin, srcs=srcs, pix=pix, M=pix[0] * pix[1] * pix[2], ldi=cin + 16, cioff=8, opts=MULTI_ON,
                names=[f"conv_wgrad_1x1_multi_kernel<{cin // 8}>"] + ["conv_wgrad_reduce_kernel"] * len(srcs), null=len(srcs) - 1,
                modes=("plain", "production", "accumulate") + (("acc3",) if acc3 else ()))


def _group(label, key, layers, nsg, one_slice=None, acc3=False):
    """din_conv_wgrad_group: layers = (cin, cout, (kh, kw), (ph, pw), nb, h, w) per item, stride 1; item j reads its input at
    cioff = 8 or 16 of ldi = cin + 24 and its gradient operand at cooff = 8 or 16 of ldo = cout + 24; production: dbias null on item 1"""
    bco, wide = key // 2, key & 1
    return dict(kind="group", label=label, key=key, layers=layers, nsg=nsg, one_slice=one_slice, opts={}, null=1,
                names=[f"conv_wgrad_pipe_group_kernel<{bco}, 256, {'true' if wide else 'false'}, 8>", "conv_wgrad_reduce_group_kernel"],
                modes=("plain", "production", "accumulate") + (("acc3",) if acc3 else ()))


NARROW16 = [(40, 120, K17, P03, 1, 13, 19), (40, 112, K71, P30, 1, 23, 19), (32, 128, K3, P1, 1, 17, 21), (264, 120, K1, P0, 2, 11, 13)] * 4
ROWS = [
    _multi("m288_production_9381", 288, [(64, 288, 64), (112, 176, 0), (64, 64, 0)], (3, 53, 59)),
    _multi("m192_four_37", 192, [(64, 256, 0), (48, 144, 0), (64, 144, 48), (32, 32, 0)], (1, 1, 37)),
    _multi("m256_two_128alone_768", 256, [(128, 152, 16), (48, 72, 8)], (2, 16, 24)),
    _multi("m256_flip_16ch_9381", 256, [(96, 120, 8), (32, 56, 16), (16, 40, 8), (32, 32, 0)], (3, 53, 59), acc3=True),
    # one workgroup per (item, slice): 143 slices of the large item (sixteen slice groups), the 33-pixel item is one slice
    _group("g128w_nsg16_one_slice", 257, [(256, 120, K1, P0, 2, 67, 68), (256, 112, K1, P0, 1, 1, 33)], 16, one_slice=1),
    _group("g192w_four_filter_shapes", 385, [(160, 184, K17, P03, 2, 19, 37), (168, 160, K71, P30, 1, 21, 40), (80, 192, K3, P0, 1, 23, 36),
                                             (776, 176, K1, P0, 2, 19, 37)], 4, acc3=True),
    _group("g256w_two_tiles_pace23", 513, [(64, 504, K3, P1, 1, 19, 37), (264, 248, K1, P0, 2, 19, 37)], 4),
    _group("g128n_sixteen_items", 256, NARROW16, 1),
    _group("g192n_two_tiles_pace45_one_slice", 384, [(160, 176, K17, P03, 2, 19, 23), (96, 384, K3, P1, 1, 17, 29), (264, 168, K1, P0, 1, 5, 7)], 4,
           one_slice=2),
    _group("g256n", 512, [(48, 248, K3, P0, 2, 21, 25), (288, 232, K1, P0, 1, 17, 19)], 4),
]
IDS = [r["label"] for r in ROWS]
CASES = [(r, m) for r in ROWS for m in r["modes"]]
CASE_IDS = [f"{r['label']}-{m}" for r, m in CASES]
PACE_ROWS = {"g256w_two_tiles_pace23": (2, 3), "g192n_two_tiles_pace45_one_slice": (4, 8)}     # row -> the k tiles per item it is there for
# call sequences din_conv_wgrad_group runs layer by layer (label -> items; dtype "fp32" marks the fp32 item)
_L128N = (40, 120, K17, P03, 1, 13, 19)
FALLBACKS = {
    "n1": [(160, 184, K17, P03, 1, 19, 37)],
    "n17": [_L128N] * 17,
    "two_keys": [(160, 184, K17, P03, 1, 19, 37), _L128N],
    "fp32_item": [(40, 120, K17, P03, 1, 13, 19, "fp32"), _L128N],
}
# lists din_conv1x1_wgrad_multi refuses (DIN_E_ARG; the workspace query answers 0): (cin, couts, dtype)
UNFIT = {"cin160": (160, (64, 48), "bf16"), "cout24": (192, (64, 24), "bf16"), "five_sources": (192, (32, 32, 32, 32, 32), "bf16"),
         "both_classes_over_128": (192, (112, 112, 32), "bf16"), "fp32": (192, (64, 48), "fp32")}


# ---- descriptors, reporters -----------------------------------------------------------------------------------------------------------
def _geometry(layer):
    cin, cout, k, p, nb, h, w = layer[:7]
    return cin, cout, k, p, nb, h, w, h + 2 * p[0] - k[0] + 1, w + 2 * p[1] - k[1] + 1


def _views(layer, j):
    """(ldi, cioff, ldo, cooff) of item j: fp32 items on the 4-element grid"""
    cin, cout = layer[0], layer[1]
    return cin + 24, 8 * (1 + j % 2), cout + 24, 16 if j % 2 else 8


def _fill_desc(L, d, layer, j):
    cin, cout, k, p, nb, h, w, oh, ow = _geometry(layer)
    d.nb, d.h, d.w, d.cin, d.oh, d.ow, d.cout = nb, h, w, cin, oh, ow, cout
    d.kh, d.kw, d.sh, d.sw, d.ph, d.pw, d.dh, d.dw = k[0], k[1], 1, 1, p[0], p[1], 1, 1
    d.ldi, d.cioff, d.ldo, d.cooff = _views(layer, j)
    d.dtype, d.in_u8 = (L.DIN_F32 if layer[7:] == ("fp32",) else L.DIN_BF16), 0


def _items(L, layers, extra=0):
    items = (L.ConvWgradItem * (len(layers) + extra))()
    for j, layer in enumerate(layers):
        _fill_desc(L, items[j].desc, layer, j)
    for j in range(extra):                                      # (an item the call does not list: a copy of item 0)
        _fill_desc(L, items[len(layers) + j].desc, layers[0], 0)
    return items


def _wsrcs(L, srcs, extra=0):
    arr = (L.ConvWSrc * (len(srcs) + extra))()
    for s, (cout, ldo, cooff) in zip(arr, srcs):
        s.cout, s.ldo, s.cooff = cout, ldo, cooff
    return arr


def _reported(lib, L, row):
    """(return code, lines) of the row's own reporter under the options now set"""
    buf = C.create_string_buffer(4096)
    if row["kind"] == "multi":
        rc = lib.din_conv1x1_wgrad_multi_kernel_names(len(row["srcs"]), _wsrcs(L, row["srcs"]), L.DIN_BF16, row["M"], row["cin"], buf, len(buf))
    else:
        rc = lib.din_conv_wgrad_group_kernel_names(len(row["layers"]), _items(L, row["layers"]), buf, len(buf))
    return rc, buf.value.decode().split("\n")[:-1]


def _assert_named(lib, L, row, monkeypatch):
    """sets the row's options (they stay set for the caller); the reporter answers the row's lines; a group row's plan has the slice groups
    and the one-slice item the row states -- the library's answers, before anything is launched"""
    for name, value in row["opts"].items():
        monkeypatch.setenv(name, value)
    rc, got = _reported(lib, L, row)
    assert 0 < rc <= 4096, f"{row['label']}: the reporter returned {rc}: {lib.din_last_error_string()}"
    assert got == row["names"], f"{row['label']}: launches {got}, not {row['names']}"
    if row["kind"] == "group":
        n = len(row["layers"])
        items = _items(L, row["layers"])
        assert {lib.din_conv_wgrad_group_key(C.byref(items[j].desc)) for j in range(n)} == {row["key"]}
        slices = (C.c_int32 * n)()
        assert lib.din_conv_wgrad_group_slices(n, items, slices, n) == row["nsg"], f"{row['label']}: slices {list(slices)}"
        assert lib.din_conv_wgrad_group_workspace(n, items) > 0
        if row["one_slice"] is not None:
            assert slices[row["one_slice"]] == 1 and max(slices) > 1, f"{row['label']}: slices {list(slices)}"
        return list(slices)
    assert lib.din_conv1x1_wgrad_multi_workspace(len(row["srcs"]), _wsrcs(L, row["srcs"]), L.DIN_BF16, row["M"], row["cin"]) == 128 * sum(
        c for c, _, _ in row["srcs"]) * row["cin"] * 4
    return None


# ---- operands and the float64 reference -----------------------------------------------------------------------------------------------
def _im2col(x, k, p, oh, ow):
    """x [nb][h][w][cin] float64 -> [M][taps][cin], the tap-shifted input (zeros outside the map), stride 1"""
    xp = torch.nn.functional.pad(x, (0, 0, p[1], p[1], p[0], p[0]))
    return torch.stack([xp[:, r:r + oh, t:t + ow, :].reshape(-1, x.shape[-1]) for r in range(k[0]) for t in range(k[1])], 1)


def _contract(g, X, k):
    """g [m][cout], X [m][taps][cin] -> sum_m g (x) X as [cout][cin][kh][kw]"""
    m, taps, cin = X.shape
    return (g.t() @ X.reshape(m, taps * cin)).reshape(-1, taps, cin).permute(0, 2, 1).reshape(-1, cin, *k)


_CACHE = {}


def _unit(gen, g, X, k, integer=False):
    """the reference terms and the epilogue operands of one source / item"""
    cout, cin = g.shape[1], X.shape[2]
    u = dict(g=g, X=X, k=k, cout=cout, cin=cin, raw=_contract(g, X, k), S=_contract(g.abs(), X.abs(), k), cs=g.sum(0), ca=g.abs().sum(0))
    if integer:
        u["scale"] = 2.0 ** torch.randint(-1, 2, (cout,), generator=gen).float()
        u["w"] = torch.randint(-1, 2, (cout, cin, *k), generator=gen).float()
    else:
        u["scale"] = torch.rand(cout, generator=gen) + 0.5
        u["w"] = torch.randn(cout, cin, *k, generator=gen)
    w64 = u["w"].double()
    u["dw_old"] = torch.randn(cout, cin, *k, generator=gen) * float(u["raw"].std())
    u["db_old"] = torch.randn(cout, generator=gen) * float(u["cs"].abs().max())
    u["wd_old"] = torch.randn(cout, generator=gen) * float((w64 * u["raw"]).sum((1, 2, 3)).abs().max())
    return u


def _random(gen, shape, integer):
    return (torch.randint(-1, 2, shape, generator=gen).float() if integer else torch.randn(shape, generator=gen)).bfloat16()


def _layer_unit(gen, layer, integer=False):
    cin, cout, k, p, nb, h, w, oh, ow = _geometry(layer)
    fp32 = layer[7:] == ("fp32",)
    xb, gb = _random(gen, (nb, h, w, cin), integer), _random(gen, (nb, oh, ow, cout), integer)
    if fp32:
        xb, gb = xb.float(), gb.float()
    u = _unit(gen, gb.double().reshape(-1, cout), _im2col(xb.double(), k, p, oh, ow), k, integer)
    u.update(xb=xb, gb=gb, layer=layer, M=nb * oh * ow)
    return u


def _operands(row):
    """host operands and float64 terms of a row: {"units": [...]}; computed once, shared by the modes, launches and the bite test"""
    if row["label"] in _CACHE:
        return _CACHE[row["label"]]
    _CACHE.clear()
    gen = torch.Generator().manual_seed(sum(map(ord, row["label"])))
    if row["kind"] == "multi":
        xb = torch.randn(*row["pix"], row["cin"], generator=gen).bfloat16()
        X = xb.double().reshape(-1, 1, row["cin"])
        units = []
        for cout, _, _ in row["srcs"]:
            gb = torch.randn(*row["pix"], cout, generator=gen).bfloat16()
            u = _unit(gen, gb.double().reshape(-1, cout), X, K1)
            u.update(gb=gb, M=row["M"])
            units.append(u)
        op = dict(units=units, xb=xb)
    else:
        op = dict(units=[_layer_unit(gen, layer) for layer in row["layers"]])
    _CACHE[row["label"]] = op
    return op


def _expect(u, mode, raw=None, cs=None, no_scale=False, acc_as_0=False, has_db=True):
    """{"dw" | "db" | "wd": (value, S)} of a unit in a mode; None: the output is not asked for.  raw / cs / no_scale / acc_as_0: a wrong
    model's terms (the bars stay those of the right ones)"""
    scaled, acc = MODES[mode]
    raw, cs = u["raw"] if raw is None else raw, u["cs"] if cs is None else cs
    sc = u["scale"].double()[:, None, None, None] if scaled else torch.ones(u["cout"], 1, 1, 1, dtype=torch.float64)
    dw, S = (raw if no_scale else sc * raw), sc * u["S"]
    if acc & 1:
        dw, S = (dw if acc_as_0 else dw + u["dw_old"].double()), S + u["dw_old"].double().abs()
    out = dict(dw=(dw, S), db=None, wd=None)
    if has_db:
        out["db"] = (cs + u["db_old"].double(), u["ca"] + u["db_old"].double().abs()) if acc & 2 else (cs, u["ca"])
    if scaled:
        w64 = u["w"].double()
        wd, Sw = (w64 * raw).sum((1, 2, 3)), (w64.abs() * u["S"]).sum((1, 2, 3))
        out["wd"] = (wd + u["wd_old"].double(), Sw + u["wd_old"].double().abs()) if acc & 2 else (wd, Sw)
    return out


def _has_db(row, mode, j):
    return not (mode == "production" and j == row["null"])


# ---- wrong models (test_bars_bite) ------------------------------------------------------------------------------------------------------
def _without(u, idx):
    """(raw, cs) of a unit that lost the pixels idx"""
    return u["raw"] - _contract(u["g"][idx], u["X"][idx], u["k"]), u["cs"] - u["g"][idx].sum(0)


def _shifted_input(row, op, j):
    """X of unit j read at cioff = 0 instead of the view's offset: the first cioff channels are the POISON in front of the view"""
    if row["kind"] == "multi":
        xb, cioff, k, p, oh, ow = op["xb"], row["cioff"], K1, P0, row["pix"][1], row["pix"][2]
    else:
        u = op["units"][j]
        cin, cout, k, p, nb, h, w, oh, ow = _geometry(u["layer"])
        xb, cioff = u["xb"], _views(u["layer"], j)[1]
    x = torch.cat([torch.full((*xb.shape[:-1], cioff), POISON, dtype=torch.float64), xb.double()[..., :xb.shape[-1] - cioff]], -1)
    return _im2col(x, k, p, oh, ow)


def _wrong_models(row, op, slices):
    """name -> {unit index: (kwargs of _expect, the outputs the model touches)}"""
    units, multi = op["units"], row["kind"] == "multi"
    stage = 64 if multi else 32
    models = {"last_stage": {j: (dict(zip(("raw", "cs"), _without(u, slice((u["M"] - 1) // stage * stage, u["M"])))), ("dw", "db", "wd"))
                             for j, u in enumerate(units)}}
    if multi:
        M = row["M"]                                            # persistent workgroup 0 of both classes: stages 0, 128, ...
        idx = torch.cat([torch.arange(t * 64, min(t * 64 + 64, M)) for t in range(0, (M + 63) // 64, 128)])
        models["slab"] = {j: (dict(raw=_without(u, idx)[0]), ("dw", "wd")) for j, u in enumerate(units)}
        rows = torch.cat([u["raw"] for u in units] + [torch.zeros_like(units[0]["raw"])])      # the slab's rows, source after source
        c0, c1 = units[0]["cout"], units[1]["cout"]
        models["swapped_row_blocks"] = {0: (dict(raw=rows[c0:c0 + c0]), ("dw", "wd")), 1: (dict(raw=rows[:c1]), ("dw", "wd"))}
    else:
        u = units[0]                                            # the first pixel slice of item 0 (slices: the library's answer)
        mps = _pad((u["M"] + slices[0] - 1) // slices[0], 32)
        models["slice"] = {0: (dict(zip(("raw", "cs"), _without(u, slice(0, min(mps, u["M"]))))), ("dw", "db", "wd"))}
    models["cioff0"] = {j: (dict(raw=_contract(u["g"], _shifted_input(row, op, j), u["k"])), ("dw", "wd")) for j, u in enumerate(units)}
    models["no_scale"] = {j: (dict(no_scale=True), ("dw",)) for j in range(len(units))}
    models["accumulate_as_0"] = {j: (dict(acc_as_0=True), ("dw",)) for j in range(len(units))}
    return models


# ---- CPU tests ----------------------------------------------------------------------------------------------------------------------------
def _function_body(text, head):
    i = text.index(head)
    j = text.index("\n}\n", i)
    return text[i:j]


def test_every_group_and_multi_instantiation_has_a_row():
    """the instantiations launch_wgrad_pipe_group and launch_wgrad_1x1_multi hold (their tables, parsed from the sources) equal the main
    kernels the rows name plus the group keys listed as unreachable: a kernel added without a row fails here, on the CPU"""
    csrc = os.path.join(ROOT, "din-group-activity-recognition-benchmark_amd", "csrc")

    def src(name):
        with open(os.path.join(csrc, name)) as fh:
            return re.sub(r"//[^\n]*", "", fh.read())

    def table(text, macro):
        body = re.search(r"#define " + macro + r"\(X\)((?:[^\n]*\\\n)*[^\n]*)", text).group(1)
        return [[a.strip() for a in args.split(",")] for args in re.findall(r"X\(([^()]*)\)", body)]

    pipe, one = src("conv_wgrad_pipe.hip"), src("conv_wgrad_1x1.hip")
    body = _function_body(pipe, "int launch_wgrad_pipe_group(")
    assert "DIN_WGRAD_PIPE_GROUP_TABLE(DIN_GROUP_ROW)" in body and "conv_wgrad_pipe_group_kernel<BCO_, 256, WIDE_, 8>" in body
    assert len(re.findall(r"conv_wgrad_pipe_group_kernel<", body)) == 2 and "DIN_WGRAD_PIPE_GROUP_TABLE(DIN_GROUP_ROW)" in _function_body(
        pipe, "bool wgrad_pipe_group_name(")
    launched = {f"conv_wgrad_pipe_group_kernel<{bco}, 256, {wide}, 8>" for bco, wide in table(pipe, "DIN_WGRAD_PIPE_GROUP_TABLE")}
    body = _function_body(one, "int launch_wgrad_1x1_multi(")
    assert "DIN_WGRAD_1X1_MULTI_TABLE(DIN_MULTI_ROW)" in body and len(re.findall(r"conv_wgrad_1x1_multi_kernel<", body)) == 2
    assert "DIN_WGRAD_1X1_MULTI_TABLE(DIN_MULTI_ROW)" in _function_body(one, "bool wgrad_1x1_multi_name(")
    launched |= {f"conv_wgrad_1x1_multi_kernel<{cpp}>" for _cin, cpp in table(one, "DIN_WGRAD_1X1_MULTI_TABLE")}
    assert len(launched) == 9, sorted(launched)
    unreachable = {f"conv_wgrad_pipe_group_kernel<{key // 2}, 256, {'true' if key & 1 else 'false'}, 8>" for key in UNREACHABLE}
    named = {r["names"][0] for r in ROWS}
    assert launched == named | unreachable and not named & unreachable, (
        f"launched without a row: {sorted(launched - named - unreachable)}; rows naming no launch: {sorted(named - launched)}")


def test_rows_resolve_to_their_kernels_and_cover_the_required_names(monkeypatch):
    """every row's lines are what its reporter answers under the row's options (the planners are host code), with the slice groups and
    the one-slice item it states; every (entry point, kernel) pair of the planned reverse pass of both backbones
    (profiles/wgrad_multi_kernel_names.txt: tools/conv_dispatch_table.py --names --wgrad-multi) has a row"""
    lib, L = _library()
    for row in ROWS:
        _assert_named(lib, L, row, monkeypatch)
        for name in row["opts"]:
            L.set_option(name, None)
    with open(NAMES_FILE) as fh:
        required = {tuple(line.split("  <-  ")[0].split(" ", 1)) for line in fh if line.strip()}
    assert {e for e, _ in required} == {"wgrad_group", "wgrad_multi"} and len(required) >= 6, sorted(required)
    have = {("wgrad_" + r["kind"], n) for r in ROWS for n in r["names"]}
    assert not required - have, f"(entry point, kernel) pairs without a row: {sorted(required - have)}"


def test_rows_carry_the_edges_they_are_there_for(monkeypatch):
    lib, L = _library()
    groups, multis = [r for r in ROWS if r["kind"] == "group"], [r for r in ROWS if r["kind"] == "multi"]
    assert {r["key"] for r in groups} | UNREACHABLE == {2 * bco + wide for bco in (128, 192, 256) for wide in (0, 1)}
    assert {len(r["layers"]) for r in groups} >= {2, 16} and {r["nsg"] for r in groups} == {1, 4, 16}
    assert any(r["one_slice"] is not None for r in groups) and all("acc3" in r["modes"] for r in (groups[1], multis[3]))
    assert any({layer[2] for layer in r["layers"]} == {K1, K3, K17, K71} and len({layer[4:7] for layer in r["layers"]}) > 1 for r in groups)
    assert any(layer[1] > r["key"] // 2 for r in groups for layer in r["layers"])                       # a bank of two filter tiles
    assert any((layer[2][0] * layer[2][1] * layer[0]) % 256 for r in groups for layer in r["layers"])
    for r in groups:
        for j, layer in enumerate(r["layers"]):
            cin, cout, k, p, nb, h, w, oh, ow = _geometry(layer)
            assert (nb * oh * ow) % 32 != 0 and (ow >= 32) == bool(r["key"] & 1) and _views(layer, j)[1] > 0 and _views(layer, j)[3] > 0
        assert len({_views(layer, j)[1::2] for j, layer in enumerate(r["layers"])}) == 2                # views differ between items
    for label, (lo, hi) in PACE_ROWS.items():
        r = next(r for r in groups if r["label"] == label)
        assert all(lo <= _pad(layer[2][0] * layer[2][1] * layer[0], 256) // 256 <= hi for layer in r["layers"][:2]), label
    assert {r["cin"] for r in multis} == {192, 256, 288} and {len(r["srcs"]) for r in multis} == {2, 3, 4}
    assert {r["M"] for r in multis} == {37, 768, 9381} and all(r["cioff"] == 8 and r["ldi"] == r["cin"] + 16 for r in multis)
    assert [s[:1] for s in multis[0]["srcs"]] == [(64,), (112,), (64,)] and multis[0]["srcs"][0][1:] == (288, 64) and multis[0]["srcs"][2][1:] == (64, 0)
    assert any(s[0] == 128 for r in multis for s in r["srcs"]) and any(s[0] == 16 for r in multis for s in r["srcs"])
    # the greedy deal of plan_wgrad_1x1_multi, largest first into the lighter class: the flip row's last source finds the lighter class full
    couts, rows, cnt, flipped = sorted((s[0] for s in multis[3]["srcs"]), reverse=True), [0, 0], [0, 0], False
    for c in couts:
        cls = 0 if rows[0] <= rows[1] else 1
        if cnt[cls] == 2 or rows[cls] + c > 128:
            cls, flipped = cls ^ 1, True
        rows[cls], cnt[cls] = rows[cls] + c, cnt[cls] + 1
    assert flipped and max(rows) <= 128


def test_group_key_sweep_reaches_every_key():
    """din_conv_wgrad_group_key over the sweep of the docstring: every key 2 * bco + wide is reached (UNREACHABLE lists the others), and only those"""
    lib, L = _library()
    found = set()
    d = L.ConvDesc()
    for k, p in ((K1, P0), (K3, P1), (K17, P03), (K71, P30)):
        for cin in (16, 40, 96, 160, 264, 776):
            for cout in (112, 128, 160, 184, 248, 384, 504):
                for nb, h, w in ((1, 1, 33), (1, 13, 19), (2, 19, 37), (2, 67, 68)):
                    _fill_desc(L, d, (cin, cout, k, p, nb, h, w), 0)
                    found.add(lib.din_conv_wgrad_group_key(C.byref(d)))
    assert found - {0} == {2 * bco + wide for bco in (128, 192, 256) for wide in (0, 1)} - UNREACHABLE, sorted(found)


def test_reporters_refuse_what_the_launches_refuse(monkeypatch):
    """no GPU: a list din_conv1x1_wgrad_multi does not take is DIN_E_ARG from the reporter and 0 from the workspace query; the call sequences
    din_conv_wgrad_group runs layer by layer answer din_conv_kernel_names(d, 2) item after item, 0 slice groups and 0 workspace bytes"""
    lib, L = _library()
    monkeypatch.setenv("DIN_WGRAD_1X1_MULTI", "2")
    buf = C.create_string_buffer(8192)
    for label, (cin, couts, dtype) in UNFIT.items():
        srcs = _wsrcs(L, [(c, c, 0) for c in couts])
        dt = L.DIN_F32 if dtype == "fp32" else L.DIN_BF16
        assert lib.din_conv1x1_wgrad_multi_kernel_names(len(couts), srcs, dt, 768, cin, buf, len(buf)) == -1, label
        assert lib.din_conv1x1_wgrad_multi_workspace(len(couts), srcs, dt, 768, cin) == 0, label
    ok = ROWS[2]
    assert lib.din_conv1x1_wgrad_multi_kernel_names(2, _wsrcs(L, ok["srcs"]), L.DIN_BF16, ok["M"], ok["cin"], None, 0) == sum(len(n) + 1 for n in ok["names"]) + 1
    monkeypatch.setenv("DIN_WGRAD_1X1_MULTI", "1")                                   # the shipped rule: launches of >= 128 Ki pixels
    assert lib.din_conv1x1_wgrad_multi_kernel_names(2, _wsrcs(L, ok["srcs"]), L.DIN_BF16, ok["M"], ok["cin"], buf, len(buf)) == -1
    one = C.create_string_buffer(1024)
    for label, layers in FALLBACKS.items():
        n, items = len(layers), _items(L, layers)
        want = []
        for j in range(n):
            assert 0 < lib.din_conv_kernel_names(C.byref(items[j].desc), 2, 0, 0, 0, one, len(one)) <= len(one)
            want += one.value.decode().split("\n")[:-1]
        rc = lib.din_conv_wgrad_group_kernel_names(n, items, buf, len(buf))
        assert 0 < rc <= len(buf) and buf.value.decode().split("\n")[:-1] == want, label
        assert lib.din_conv_wgrad_group_slices(n, items, None, 0) == 0 and lib.din_conv_wgrad_group_workspace(n, items) == 0, label
    assert lib.din_conv_wgrad_group_kernel_names(0, _items(L, FALLBACKS["n1"]), buf, len(buf)) == -1


def test_reference_indexing():
    """the float64 reference against torch.nn.grad.conv2d_weight in float64 (a 1x7 item with padding, a 1x1 source)"""
    row = next(r for r in ROWS if r["label"] == "g192n_two_tiles_pace45_one_slice")
    u = _operands(row)["units"][0]
    cin, cout, k, p, nb, h, w, oh, ow = _geometry(u["layer"])
    want = torch.nn.grad.conv2d_weight(u["xb"].double().permute(0, 3, 1, 2), (cout, cin, *k), u["gb"].double().permute(0, 3, 1, 2), padding=p)
    assert float((u["raw"] - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert bool((u["S"] >= u["raw"].abs() - 1e-9).all()) and u["raw"].shape == (cout, cin, *k)
    row = next(r for r in ROWS if r["label"] == "m192_four_37")
    op = _operands(row)
    u = op["units"][2]
    want = torch.einsum("mo,mi->oi", u["gb"].double().reshape(-1, 64), op["xb"].double().reshape(-1, 192))
    assert float((u["raw"][:, :, 0, 0] - want).abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_bars_bite(row, monkeypatch):
    """float64 only: on the row's data and under the row's bars, each wrong kernel moves at least one element of every output it touches,
    of every unit it touches, by >= 10x that element's bar -- the last ragged stage dropped (the last M % 64 pixels of the multi launch,
    the last 32-pixel stage of each group item); one persistent workgroup's slab (multi) / one pixel slice of one item (group) dropped; two
    sources' row blocks swapped in the slab; scale omitted; accumulate 1 treated as 0; the input read at cioff = 0"""
    lib, L = _library()
    slices = _assert_named(lib, L, row, monkeypatch)
    op = _operands(row)
    for model, touched in _wrong_models(row, op, slices).items():
        for mode in row["modes"]:
            scaled, acc = MODES[mode]
            if (model == "no_scale" and not scaled) or (model == "accumulate_as_0" and not acc & 1):
                continue
            for j, (kwargs, outputs) in touched.items():
                u = op["units"][j]
                right, wrong = _expect(u, mode, has_db=_has_db(row, mode, j)), _expect(u, mode, has_db=_has_db(row, mode, j), **kwargs)
                for name in outputs:
                    if right[name] is None:
                        continue
                    moved = float(((wrong[name][0] - right[name][0]).abs() / (BAR * right[name][1])).max())
                    assert moved >= 10, f"{row['label']} {mode}: {model} moves {name} of unit {j} by only {moved:.2f} bars"


# ---- the GPU tests ------------------------------------------------------------------------------------------------------------------------
_DEV = {}


def _device(row, op, L):
    """the row's operands on the device, its outputs between guard bands (one unit more than the call lists), built once per row"""
    if row["label"] in _DEV:
        return _DEV[row["label"]]
    _DEV.clear()
    units = op["units"]
    dev = dict(units=[])
    if row["kind"] == "multi":
        dev["x"] = _view(op["xb"], torch.bfloat16, row["ldi"], row["cioff"], row["cin"])
    for j, u in enumerate(units + units[:1]):                    # (the last: the unit the call does not list)
        t = dict(scale=u["scale"].cuda(), w=u["w"].cuda())
        if row["kind"] == "multi":
            cout, ldo, cooff = row["srcs"][j] if j < len(units) else row["srcs"][0]
            t["g"] = _view(u["gb"], torch.bfloat16, ldo, cooff, cout)
        else:
            ldi, cioff, ldo, cooff = _views(u["layer"], j if j < len(units) else 0)
            t["x"] = _view(u["xb"], u["xb"].dtype, ldi, cioff, _pad(u["cin"], 8))
            t["g"] = _view(u["gb"], u["gb"].dtype, ldo, cooff, _pad(u["cout"], 8))
        for name, n in (("dw", u["raw"].numel()), ("db", u["cout"]), ("wd", u["cout"])):
            t[name + "_buf"], t[name] = _guarded(n)
        dev["units"].append(t)
    _DEV[row["label"]] = dev
    return dev


def _workspace(wsb):
    buf = torch.empty(wsb + 2 * WSG, dtype=torch.uint8, device="cuda")
    return buf, buf[WSG:WSG + wsb]


def _call(lib, L, row, dev, mode, n, ws, wsb, null_db=None, acc=None):
    """one call of the row's entry point on the first n units in a mode (null_db: the unit whose dbias is null); returns the code"""
    scaled, accumulate = MODES[mode]
    accumulate = accumulate if acc is None else acc

    def ptrs(t, j):
        return dict(dw=t["dw"].data_ptr(), dbias=None if j == null_db else t["db"].data_ptr(), scale=t["scale"].data_ptr() if scaled else None,
                    w=t["w"].data_ptr() if scaled else None, wdot=t["wd"].data_ptr() if scaled else None)
    if row["kind"] == "multi":
        srcs = _wsrcs(L, row["srcs"][:n], extra=1)
        for j in range(n):
            srcs[j].dout = dev["units"][j]["g"].data_ptr()
            for name, v in ptrs(dev["units"][j], j).items():
                setattr(srcs[j], name, v)
        return lib.din_conv1x1_wgrad_multi(n, srcs, L.DIN_BF16, row["M"], row["cin"], row["ldi"], row["cioff"], dev["x"].data_ptr(), accumulate,
                                           ws.data_ptr(), wsb, None)
    items = _items(L, row["layers"][:n], extra=1)
    for j in range(n):
        t = dev["units"][j]
        items[j].in_, items[j].dout, items[j].accumulate = t["x"].data_ptr(), t["g"].data_ptr(), accumulate
        for name, v in ptrs(t, j).items():
            setattr(items[j], name, v)
    return lib.din_conv_wgrad_group(n, items, ws.data_ptr(), wsb, None)


def _prefill(dev, expect_of, units, mode):
    """NaN where the mode overwrites (and in the decoys), the old value where it adds; the unlisted unit holds sevens"""
    scaled, acc = MODES[mode]
    for j, t in enumerate(dev["units"]):
        for name in ("dw", "db", "wd"):
            t[name + "_buf"].fill_(GUARD)
        if j == len(units):
            for name in ("dw", "db", "wd"):
                t[name].fill_(7.0)
            continue
        u, exp = units[j], expect_of[j]
        t["dw"].copy_(u["dw_old"].reshape(-1)) if acc & 1 else t["dw"].fill_(float("nan"))
        for name in ("db", "wd"):
            t[name].copy_(u[name + "_old"]) if acc & 2 and exp[name] is not None else t[name].fill_(float("nan"))


def _check(label, dev, expect_of, units, wsbuf, wsb):
    """guards, decoys and the unlisted unit intact; returns max(err / bar) per output kind"""
    assert bool((wsbuf[:WSG] == 0x5a).all()) and bool((wsbuf[WSG + wsb:] == 0x5a).all()), f"{label}: wrote outside the workspace"
    worst = dict(dw=0.0, db=0.0, wd=0.0)
    for j, t in enumerate(dev["units"]):
        for name in ("dw", "db", "wd"):
            buf, n = t[name + "_buf"], t[name].numel()
            assert bool((buf[:NG] == GUARD).all()) and bool((buf[NG + n:] == GUARD).all()), f"{label}: wrote outside {name} of unit {j}"
            if j == len(units):
                assert bool((t[name] == 7.0).all()), f"{label}: wrote {name} of a unit the call does not list"
            elif expect_of[j][name] is None:
                assert bool(t[name].isnan().all()), f"{label}: {name} of unit {j} written without being asked for"
            else:
                v, S = expect_of[j][name]
                got = t[name].double().cpu().reshape(v.shape)
                assert not bool(got.isnan().any()), f"{label}: NaN left in {name} of unit {j}"
                worst[name] = max(worst[name], float(((got - v).abs() / (BAR * S)).max()))
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("row,mode", CASES, ids=CASE_IDS)
def test_wgrad_multi_launch_against_fp64(env, row, mode, monkeypatch):
    lib, L, nhwc, ops = env
    _assert_named(lib, L, row, monkeypatch)
    op = _operands(row)
    units, dev = op["units"], _device(row, op, L)
    n = len(units)
    if row["kind"] == "multi":
        wsb = lib.din_conv1x1_wgrad_multi_workspace(n, _wsrcs(L, row["srcs"]), L.DIN_BF16, row["M"], row["cin"])
    else:
        wsb = lib.din_conv_wgrad_group_workspace(n, _items(L, row["layers"]))
    assert wsb > 0
    wsbuf, ws = _workspace(wsb)
    null_db = row["null"] if mode == "production" else None
    expect_of = [_expect(u, mode, has_db=_has_db(row, mode, j)) for j, u in enumerate(units)]
    for launch in range(2):
        wsbuf.fill_(0x5a)
        ws.fill_(0x7f)
        _prefill(dev, expect_of, units, mode)
        L.check(_call(lib, L, row, dev, mode, n, ws, wsb, null_db))
        torch.cuda.synchronize()
        worst = _check(f"{row['label']} {mode} launch {launch}", dev, expect_of, units, wsbuf, wsb)
        print(f"MARGIN {row['label']} {mode} launch {launch}: max err/bar dW {worst['dw']:.4f} dbias {worst['db']:.4f} wdot {worst['wd']:.4f}")
        assert Measured(worst["dw"]) <= 1
        assert Measured(worst["db"]) <= 1
        assert Measured(worst["wd"]) <= 1


@pytest.mark.gpu
@pytest.mark.parametrize("label", list(PACE_ROWS))
def test_group_pacing_changes_no_bit_of_dw(env, label, monkeypatch):
    """DIN_WGRAD_GROUP_PACE=1 (items of 2-3 k tiles) and =2 (up to 8): dW bit-identical to the unpaced launch of the same row; dbias / wdot
    (fp32 atomics of several workgroups: the order varies with or without pacing) within the bar"""
    lib, L, nhwc, ops = env
    row = next(r for r in ROWS if r["label"] == label)
    _assert_named(lib, L, row, monkeypatch)
    op = _operands(row)
    units, dev = op["units"], _device(row, op, L)
    n, mode = len(units), "production"
    wsb = lib.din_conv_wgrad_group_workspace(n, _items(L, row["layers"]))
    wsbuf, ws = _workspace(wsb)
    expect_of = [_expect(u, mode, has_db=_has_db(row, mode, j)) for j, u in enumerate(units)]
    unpaced = None
    for pace in ("0", "1", "2"):
        monkeypatch.setenv("DIN_WGRAD_GROUP_PACE", pace)
        assert _reported(lib, L, row)[1] == row["names"] and lib.din_conv_wgrad_group_workspace(n, _items(L, row["layers"])) == wsb
        wsbuf.fill_(0x5a)
        ws.fill_(0x7f)
        _prefill(dev, expect_of, units, mode)
        L.check(_call(lib, L, row, dev, mode, n, ws, wsb, row["null"]))
        torch.cuda.synchronize()
        worst = _check(f"{label} pace {pace}", dev, expect_of, units, wsbuf, wsb)
        print(f"MARGIN {label} DIN_WGRAD_GROUP_PACE={pace}: max err/bar dW {worst['dw']:.4f} dbias {worst['db']:.4f} wdot {worst['wd']:.4f}")
        assert Measured(max(worst.values())) <= 1
        dws = [t["dw"].clone() for t in dev["units"][:n]]
        if unpaced is None:
            unpaced = dws
        else:
            assert all(torch.equal(a, b) for a, b in zip(dws, unpaced)), f"{label}: DIN_WGRAD_GROUP_PACE={pace} changed dW"


@pytest.mark.gpu
@pytest.mark.parametrize("label", list(FALLBACKS))
def test_group_fallbacks_equal_per_layer_launches_bit_for_bit(env, label):
    """a list din_conv_wgrad_group does not run as one launch: dW / dbias / wdot bit-identical to din_conv_wgrad per layer on the same
    workspace, and (operands in {-1, 0, 1}, power-of-two scales: every fp32 sum exact in any order) equal to the float64 reference"""
    lib, L, nhwc, ops = env
    layers = FALLBACKS[label]
    row = dict(kind="group", label="fallback_" + label, layers=layers, opts={})
    gen = torch.Generator().manual_seed(len(label))
    units = [_layer_unit(gen, layer, integer=True) for layer in layers]
    _DEV.clear()
    dev = _device(row, dict(units=units), L)
    n = len(layers)
    items = _items(L, layers)
    assert lib.din_conv_wgrad_group_workspace(n, items) == 0 and lib.din_conv_wgrad_group_slices(n, items, None, 0) == 0
    wsb = max(lib.din_conv_workspace_bytes(C.byref(items[j].desc), 2) for j in range(n))
    wsbuf, ws = _workspace(wsb)
    mode = "accumulate"                                          # scale, w, wdot given; dbias / wdot zeroed by the call, dW += on the old value
    expect_of = [_expect(u, mode) for u in units]
    wsbuf.fill_(0x5a)
    ws.fill_(0x7f)
    _prefill(dev, expect_of, units, mode)
    L.check(_call(lib, L, row, dev, mode, n, ws, wsb))
    torch.cuda.synchronize()
    worst = _check(label, dev, expect_of, units, wsbuf, wsb)
    got = [{name: t[name].clone() for name in ("dw", "db", "wd")} for t in dev["units"][:n]]
    _prefill(dev, expect_of, units, mode)
    for j in range(n):
        t = dev["units"][j]
        ws.fill_(0x7f)
        L.check(lib.din_conv_wgrad(C.byref(items[j].desc), t["x"].data_ptr(), t["g"].data_ptr(), t["dw"].data_ptr(), t["db"].data_ptr(),
                                   t["scale"].data_ptr(), t["w"].data_ptr(), t["wd"].data_ptr(), 1, ws.data_ptr(), wsb, None))
    torch.cuda.synchronize()
    for j in range(n):
        for name in ("dw", "db", "wd"):
            assert torch.equal(got[j][name], dev["units"][j][name]), f"{label}: {name} of item {j} differs from the per-layer launch"
    # exact sums: only the final fp32 rounding of old + scale * dW is left (<= 2^-24 of S)
    assert Measured(max(worst.values())) <= 2.0 ** -24 / BAR


def _sevens(dev):
    for t in dev["units"]:
        for name in ("dw", "db", "wd"):
            t[name + "_buf"].fill_(7.0)


def _all_sevens(dev):
    return all(bool((t[name + "_buf"] == 7.0).all()) for t in dev["units"] for name in ("dw", "db", "wd"))


@pytest.mark.gpu
def test_refusals_return_their_code_and_write_nothing(env, monkeypatch):
    """din_conv1x1_wgrad_multi: every unfit list, fp32 and a workspace one byte short; din_conv_wgrad_group: a workspace one byte short, a
    null dw and a wdot without w in the LAST item (accumulate 0: the items before it would have had their dbias zeroed): the documented
    code, and every output buffer still holds its sevens"""
    lib, L, nhwc, ops = env
    monkeypatch.setenv("DIN_WGRAD_1X1_MULTI", "2")
    row = ROWS[2]
    op = _operands(row)
    dev = _device(row, op, L)
    wsb = lib.din_conv1x1_wgrad_multi_workspace(2, _wsrcs(L, row["srcs"]), L.DIN_BF16, row["M"], row["cin"])
    wsbuf, ws = _workspace(wsb)
    _sevens(dev)
    assert _call(lib, L, row, dev, "plain", 2, ws, wsb - 1) == -3                       # DIN_E_WORKSPACE
    big = torch.zeros(row["M"], 640, dtype=torch.bfloat16, device="cuda")
    sink = dev["units"][0]
    for label, (cin, couts, dtype) in UNFIT.items():
        srcs = _wsrcs(L, [(c, c, 0) for c in couts])
        for s in srcs:
            s.dout, s.dw, s.dbias = big.data_ptr(), sink["dw"].data_ptr(), sink["db"].data_ptr()
        dt = L.DIN_F32 if dtype == "fp32" else L.DIN_BF16
        assert lib.din_conv1x1_wgrad_multi_workspace(len(couts), srcs, dt, row["M"], cin) == 0, label
        assert lib.din_conv1x1_wgrad_multi(len(couts), srcs, dt, row["M"], cin, cin + 16, 8, big.data_ptr(), 0, ws.data_ptr(), wsb, None) == -1, label
    srcs = _wsrcs(L, row["srcs"])
    for j, s in enumerate(srcs):                                 # wdot without w in the last source
        t = dev["units"][j]
        s.dout, s.dw, s.dbias, s.wdot = t["g"].data_ptr(), t["dw"].data_ptr(), t["db"].data_ptr(), t["wd"].data_ptr()
        s.w = t["w"].data_ptr() if j == 0 else None
    assert lib.din_conv1x1_wgrad_multi(2, srcs, L.DIN_BF16, row["M"], row["cin"], row["ldi"], row["cioff"], dev["x"].data_ptr(), 0, ws.data_ptr(), wsb, None) == -1
    torch.cuda.synchronize()
    assert _all_sevens(dev), "a refused din_conv1x1_wgrad_multi call wrote"

    row = next(r for r in ROWS if r["label"] == "g256n")
    op = _operands(row)
    dev = _device(row, op, L)
    n = len(op["units"])
    wsb = lib.din_conv_wgrad_group_workspace(n, _items(L, row["layers"]))
    wsbuf, ws = _workspace(wsb)
    _sevens(dev)
    assert _call(lib, L, row, dev, "accumulate", n, ws, wsb - 1, acc=0) == -3
    items = _items(L, row["layers"])
    for bad in ("dw", "w"):
        for j in range(n):
            t = dev["units"][j]
            items[j].in_, items[j].dout, items[j].dw, items[j].dbias = t["x"].data_ptr(), t["g"].data_ptr(), t["dw"].data_ptr(), t["db"].data_ptr()
            items[j].scale, items[j].w, items[j].wdot, items[j].accumulate = t["scale"].data_ptr(), t["w"].data_ptr(), t["wd"].data_ptr(), 0
        setattr(items[n - 1], bad, None)
        assert lib.din_conv_wgrad_group(n, items, ws.data_ptr(), wsb, None) == -1, bad
    torch.cuda.synchronize()
    assert _all_sevens(dev), "a refused din_conv_wgrad_group call wrote"
