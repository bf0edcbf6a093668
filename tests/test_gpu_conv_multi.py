"""Every kernel din_conv_fwd2 / din_conv1x1_dgrad_multi / din_conv_dgrad_x launch, by name, against a float64 reference with the per-element
bars and the guard / launch / compare loop of tests/test_gpu_conv_fwd_dgrad.py ("CF": _launch_twice_and_compare, bar_of, _view, _bits,
POISON, NG, the mask operand with its special values at known positions, Measured).  These are the MULTI = 1, XSRC = 1, SPLIT = 1 and
csplit forms CF leaves out: the launches every InceptionA/B/C block entry makes, forward and backward.

One row of ROWS per code path.  `name` is a line the entry point's own reporter (din_conv_fwd2_kernel_names,
din_conv1x1_dgrad_multi_kernel_names, din_conv_dgrad_x_kernel_names) answers for every mode of the row -- asserted before anything runs
on the GPU and for all rows on the CPU.  Required names: profiles/conv_multi_kernel_names.txt (tools/conv_dispatch_table.py --names
--multi: fwd_groups, dgrad_groups and x_host of both backbones, three dtypes, four geometries, the reverse pass's flag forms) plus
EXTRA_REQUIRED: what a caller reaches with no option set that no backbone shape reaches, found by sweeping the three reporters (listed
there).  Both are sets of (entry point, instantiation): a name counts as covered only by a row that launches it through that entry point
(conv1x1_regw_kernel<8,0,...> needs a din_conv_fwd2 row and a din_conv1x1_dgrad_multi row).  The large-map kernels among them
(conv1x1_stream_kernel, conv1x1_regw_kernel) are forced onto small maps with their option; the 256-pixel tiles run at the map size the
planner asks for.

Shapes: 2 x 19 x 23 pixels (7 pixel tiles of 128, the last ragged) unless the kernel needs more; produced channels that are no multiple of
the filter tile; sources with their own pixel stride and channel offset, widths that leave a partial 64-channel (fp32: 32-channel) k-step
so that the seam between two sources falls inside padding, one width below 64; fp32 widths that are no multiple of 4; the mask is its own
tensor (ldm != ldi, moff != cioff).  conv1x1_regw_kernel / conv1x1_stream_kernel are forced on these small maps with option value "2"
(CF's REGW / REGW_SHORT / STREAM); a multi-source launch never splits its reduction, a two-destination forward must not (f2_regw24 sits
on CF's 3 x 67 x 61 map: 192 tiles).

Reference, float64 on the stored operands, v and S = the same sum over absolute values:
    multi     v = sum_b g_b . W_b^T
    fwd2      CF.conv_reference; bias and ReLU only on channels below craw when craw > 0; channels [0, csplit) land in the first
              destination, [csplit, cout) in the second -- a filter tile straddles both in every row
    dgrad_x   CF.dgrad_reference of the strided conv + the 1x1 term at the same pixel
Bars: CF.bar_of unchanged with K = the whole reduction length (kh kw c + sum_b cout_b) + 2; f32x3 rows get the fp32 bar (as in
test_gpu_split.py).  A bf16 ACCUM row carries twice=True and bar_of's extra term 2^-7 (1 + 2^-8) |g| only where the code shows the launch
ends in one of the three epilogues that stage the tile as bf16 before adding the old value:
    conv_gather_fast_kernel (MULTI and XSRC forms alike: one template) takes staged_tile_store when produced channels, output view and
        mask view sit on the 8-element grid and the reduction is not split -> every bf16 ACCUM tile row here (mt128_b_accum,
        mt160_b_mask_accum, dx_*_accum, dx_*_mask_accum) except mt128_b_direct_mask_accum (115 produced channels: epilogue_direct adds in
        fp32, plain bar)
    conv1x1_stream_kernel's last block -> ms64_accum, ms96_mask_accum
    conv1x1_regw_kernel refuses ACCUM (conv1x1_regw_eligible): no such row
Two-launch din_conv_dgrad_x (fp32, f32x3, a bf16 tile that is not 96, DIN_DGRAD_X=0) stores the intermediate t = mask(conv^T g) (+ old) and
the one-source din_conv1x1_dgrad_multi launch adds mask(g_x . W_x^T) to it under ACCUM:
    bf16  t is rounded once more when stored: |t' - t| <= 2^-8 |t|, after the suite's factor 2 the bar grows by 2^-7 |t|; the second launch
          (conv_gather_fast_kernel<bf16,...,MULTI>, aligned views) stages its term g2 as bf16: + 2^-7 (1 + 2^-8) |g2|; the first launch stages
          its term g1 only when it runs under ACCUM itself (dx2_b_t64_accum): + 2^-7 (1 + 2^-8) |g1|
    fp32  t rounds once more in fp32: one more summation term (K + 1)
Nothing else is widened.

Every GPU row and mode: two launches from the same prefill (NaN inside the produced ranges, or the old values under ACCUM; a random
pattern outside; guard bands around every destination; 0x5a guards around din_conv_dgrad_x's workspace -- din_conv1x1_dgrad_multi takes
none); everything outside the produced ranges bit-identical afterwards; no NaN left; masked-off elements bit for bit +0.0 / the old value;
max(err / bar) <= 1 as a Measured, printed per row (profiles/conv_multi_test_margins.txt).

FOUND with this file (MI355X, max(err / bar) per row, both launches equal): no defect.  bf16 rows 0.37-0.50 (a correctly rounded bf16 store
    is 0.5 of the 2^-7 |v| term), fp32 and f32x3 rows 0.004-0.06; the twice=True rows 0.37-0.48 under their widened bar; no write outside a
    produced range, no NaN left, every masked-off element bit for bit +0.0 / the old value; the split-K shape is refused by launch and
    reporter alike.
FIXED with this file: nothing in the kernels.  The library gained the three reporters; din_conv_fwd2, din_conv1x1_dgrad_multi and
    din_conv_dgrad_x now check their arguments and build their argument blocks, plans and choices in the one function their reporter
    walks too (for_fwd2_launch, for_multi_launch, for_dgrad_x_launches in csrc/conv_igemm.hip)."""
import ctypes as C
import os

import pytest
import torch

from tests.conftest import ROOT
from tests import test_gpu_conv_fwd_dgrad as CF
from tests.test_gpu_conv_fwd_dgrad import ACCUM, BIAS, K1, K3, MASK, P0, P1, RELU, REGW, REGW_SHORT, S1, S2, STREAM, _fast, _pad
from tests.test_gpu_kernels import env  # noqa: F401  (the module-scoped library fixture)

NAMES_FILE = os.path.join(ROOT, "profiles", "conv_multi_kernel_names.txt")
PIX = (2, 19, 23)
K13 = (1, 3)


def _mt(t, bn, wm):
    return _fast(t, 128, bn, wm, 2, 8, 2, 1, 0, 0, 0)


ENTRY = {"multi": "dgrad_multi", "fwd2": "fwd2", "dgx": "dgrad_x"}      # row kind -> the entry-point word of NAMES_FILE
# (entry point, instantiation) pairs no backbone shape reaches but a caller can with no option set, from a sweep of the three reporters over
# dtypes, 1x1 / 1x3 / 3x3 / 1x7 / 5x5 filters, 3 ... 768 reduction and 16 ... 1024 produced channels, maps of 874 ... 2.7 M pixels, every
# flag form and mask views at multiples of 8 and of 4.  din_conv_fwd2: the 64- / 96-filter tiles, the general loop (cin < 64) and LANEK at
# every width, the two 256-pixel tiles, conv1x1_stream_kernel's SPLIT forms (>= 256 Ki pixels).  din_conv1x1_dgrad_multi: launches producing
# <= 96 channels, the conv1x1_regw_kernel forms the backbones do not use, conv1x1_stream_kernel's MULTI forms (>= 256 Ki pixels).
# din_conv_dgrad_x: its own kernel is the XSRC tile (in NAMES_FILE); the two-launch form runs for_each_dgrad_launch / run_dgrad_launch
# exactly as din_conv_dgrad does (held by CF, kernel by kernel) and then for_multi_launch / run_multi_launch exactly as a one-source
# din_conv1x1_dgrad_multi under ACCUM does (held by the multi rows here): the dx2_* rows hold the composition, not every pairing
_B, _F, _X = "bf16", "float", "f32x3"
EXTRA_REQUIRED = (
    {("fwd2", _fast(_B, 128, bn, 4, 2, 8, 2, 0, fk, 0, lk)) for bn in (64, 128, 160, 192) for fk, lk in ((0, 0), (1, 0), (1, 1))}
    | {("fwd2", _fast(_B, 128, 96, 2, 2, 8, 2, 0, 0, 0, 0)), ("fwd2", _fast(_B, 256, 256, 4, 2, 8, 2, 0, 0, 0, 0))}
    | {("fwd2", _fast(t, 128, bn, 2, 2, 8, 2, 0, 0, 0, 0)) for t in (_F, _X) for bn in (64, 96)}
    | {("fwd2", _fast(t, 256, 64, 4, 1, 4, 4, 0, 0, 0, 0)) for t in (_F, _X)}
    | {("fwd2", f"conv1x1_stream_kernel<{bn},{3 if bn == 192 else 4},0,0,1>") for bn in (64, 96, 192)}
    | {("dgrad_multi", _mt(_B, 64, 4)), ("dgrad_multi", _mt(_B, 96, 2))} | {("dgrad_multi", _mt(t, bn, 2)) for t in (_F, _X) for bn in (64, 96)}
    | {("dgrad_multi", f"conv1x1_regw_kernel<{nks},{m},4,2,2>") for nks in (6, 8, 10) for m in (0, 1)}
    | {("dgrad_multi", f"conv1x1_regw_kernel<{nks},{m},9,1,3>") for nks in (20, 24) for m in (0, 1)}
    | {("dgrad_multi", f"conv1x1_stream_kernel<{bn},4,1,{e},0>") for bn in (64, 96) for e in (0, 1)})


def _multi(label, name, dtype, flags, cin, couts, opts=None, twice=False):
    """din_conv1x1_dgrad_multi: sources of couts channels -> cin produced channels.  Source b sits at channel offset epc (b + 1) of a pixel
    stride that is wider than its view by epc (b + 1) more; the output at cioff = 8 (fp32: 4); the mask at its own stride and offset"""
    epc = 8 if dtype == "bf16" else 4
    srcs = [(c, epc * (b + 1) + _pad(c, epc) + epc * (b + 1), epc * (b + 1)) for b, c in enumerate(couts)]
    cioff = epc
    ldi = cioff + _pad(cin, epc) + 8
    return dict(kind="multi", label=label, name=name, dtype=dtype, flags=flags, cin=cin, srcs=srcs, out=(ldi, cioff), maskv=(ldi + 16, cioff + epc),
                opts=opts or {}, twice=twice)


def _fwd2(label, name, dtype, shape, csplit, craws, opts=None):
    """din_conv_fwd2: shape as in CF; channels [0, csplit) -> (ldo, cooff), [csplit, cout) -> (ldo2, cooff2); modes: craws x (BIAS | RELU, 0)"""
    nb, cin, h, w, cout, k, s, p, dil = shape
    epc = 8 if dtype == "bf16" else 4
    ldi = epc + _pad(cin, epc) + epc
    return dict(kind="fwd2", label=label, name=name, dtype=dtype, shape=shape, csplit=csplit, craws=craws, opts=opts or {},
                views=(ldi, epc, epc + cout + 8, epc, 2 * epc + (cout - csplit) + 16, 2 * epc))      # (check_desc: ldo holds cooff + cout)


def _dgx(label, names, dtype, flags, shape, cx, fused, opts=None, twice=False, stage1=False, split=0, lines=None):
    """din_conv_dgrad_x: shape as in CF (the strided conv), cx = filters of the 1x1 that reads the same view; names: every line the reporter
    answers: the line(s) of one parity class, then the multi launch's where the form is not fused; split: the most ways a parity class's
    reduction is split (terms of the bar, as CF counts them); lines: the whole answer where the parity classes differ"""
    nb, cin, h, w, cout, k, s, p, dil = shape
    epc = 8 if dtype == "bf16" else 4
    ldi, ldo = epc + _pad(cin, epc) + epc, epc + _pad(cout, epc) + 8
    return dict(kind="dgx", label=label, name=names[0], names=list(names), dtype=dtype, flags=flags, shape=shape, x=(cx, 2 * epc + _pad(cx, epc) + 8, 2 * epc),
                views=(ldi, epc, ldo, epc, ldi + 16, 2 * epc), fused=fused, opts=opts or {}, twice=twice, stage1=stage1, split=split, lines=lines)


XSRC = _fast("bf16", 128, 96, 4, 2, 8, 2, 0, 0, 1, 0)
OFF = {"DIN_DGRAD_X": "0"}
FINISH, T96 = "conv_splitk_finish_kernel<bf16>", _fast("bf16", 128, 96, 4, 2, 8, 2, 0, 0, 0, 0)
ROWS = [
    # ---- din_conv1x1_dgrad_multi on conv_gather_fast_kernel<T,128,BN,WM,2,8,2,MULTI=1,...>: bf16 BN 64 / 128 / 192 on eight waves, 96 / 160 on four
    _multi("mt64_b", _mt("bf16", 64, 4), "bf16", 0, 56, (72,)),
    _multi("mt96_b_mask", _mt("bf16", 96, 2), "bf16", MASK, 88, (40, 104)),
    _multi("mt128_b_accum", _mt("bf16", 128, 4), "bf16", ACCUM, 120, (72, 48, 104), twice=True),
    _multi("mt160_b_mask_accum", _mt("bf16", 160, 2), "bf16", MASK | ACCUM, 152, (64, 48, 104, 72), twice=True),
    _multi("mt192_b", _mt("bf16", 192, 4), "bf16", 0, 184, (104, 40)),
    # 115 produced channels: no multiple of 8 -> epilogue_direct (tail stores, MASK / ACCUM in fp32: the plain bar)
    _multi("mt128_b_direct_mask_accum", _mt("bf16", 128, 4), "bf16", MASK | ACCUM, 115, (72, 48)),
    # fp32 / f32x3: four waves; source widths that are no multiple of 4; produced channels at multiples of 4 (staged) and not (direct)
    _multi("mt64_f", _mt("float", 64, 2), "fp32", 0, 54, (70, 38)),
    _multi("mt96_f_mask", _mt("float", 96, 2), "fp32", MASK, 88, (38, 102, 70)),
    _multi("mt128_f_accum", _mt("float", 128, 2), "fp32", ACCUM, 118, (70,)),
    _multi("mt160_f_mask_accum", _mt("float", 160, 2), "fp32", MASK | ACCUM, 148, (22, 38, 70, 46)),
    _multi("mt192_f", _mt("float", 192, 2), "fp32", 0, 182, (102, 38)),
    _multi("mt64_x3_mask_accum", _mt("f32x3", 64, 2), "f32x3", MASK | ACCUM, 52, (70, 38)),
    _multi("mt96_x3_accum", _mt("f32x3", 96, 2), "f32x3", ACCUM, 86, (38, 102, 70)),
    _multi("mt128_x3_mask", _mt("f32x3", 128, 2), "f32x3", MASK, 116, (70, 22, 38, 46)),
    _multi("mt160_x3", _mt("f32x3", 160, 2), "f32x3", 0, 150, (70,)),
    _multi("mt192_x3_mask", _mt("f32x3", 192, 2), "f32x3", MASK, 180, (102, 38)),
    # ---- ... on conv1x1_stream_kernel<BN,4,MULTI=1,EPI,0>: <= 6 blocks of 64 channels, the 48- and 104-channel sources end in partial blocks
    _multi("ms64", "conv1x1_stream_kernel<64,4,1,0,0>", "bf16", 0, 56, (64, 48, 104), STREAM),
    _multi("ms64_mask", "conv1x1_stream_kernel<64,4,1,1,0>", "bf16", MASK, 40, (48, 104), STREAM),
    _multi("ms64_accum", "conv1x1_stream_kernel<64,4,1,1,0>", "bf16", ACCUM, 64, (104, 48, 64), STREAM, twice=True),
    _multi("ms96", "conv1x1_stream_kernel<96,4,1,0,0>", "bf16", 0, 88, (48, 104), STREAM),
    _multi("ms96_mask_accum", "conv1x1_stream_kernel<96,4,1,1,0>", "bf16", MASK | ACCUM, 80, (104, 64, 48), STREAM, twice=True),
    # ---- ... on conv1x1_regw_kernel<NKS,MASKED,NS,OCC,RT>: short form (<= 10 k-steps of 32 channels, classes of 128 filters, a short last
    # class), long forms (20 / 24 k-steps, classes of 192); every source padded to whole 64-channel stages, the 160-channel ones half-padded
    _multi("mr6", "conv1x1_regw_kernel<6,0,4,2,2>", "bf16", 0, 200, (104, 40), REGW_SHORT),
    _multi("mr6_mask", "conv1x1_regw_kernel<6,1,4,2,2>", "bf16", MASK, 136, (72, 40), REGW_SHORT),
    _multi("mr8", "conv1x1_regw_kernel<8,0,4,2,2>", "bf16", 0, 200, (64, 64, 48, 64), REGW_SHORT),
    _multi("mr8_mask", "conv1x1_regw_kernel<8,1,4,2,2>", "bf16", MASK, 136, (64, 48, 104), REGW_SHORT),
    _multi("mr10", "conv1x1_regw_kernel<10,0,4,2,2>", "bf16", 0, 200, (104, 160), REGW_SHORT),
    _multi("mr10_mask", "conv1x1_regw_kernel<10,1,4,2,2>", "bf16", MASK, 264, (160, 104), REGW_SHORT),
    _multi("mr20", "conv1x1_regw_kernel<20,0,9,1,3>", "bf16", 0, 200, (192, 128, 128, 192), REGW),
    _multi("mr20_mask", "conv1x1_regw_kernel<20,1,9,1,3>", "bf16", MASK, 392, (192, 128, 128, 192), REGW),
    _multi("mr24", "conv1x1_regw_kernel<24,0,9,1,3>", "bf16", 0, 392, (192, 160, 160, 192), REGW),
    _multi("mr24_mask", "conv1x1_regw_kernel<24,1,9,1,3>", "bf16", MASK, 200, (192, 160, 160, 192), REGW),
    # ---- din_conv_fwd2: csplit is no multiple of the filter tile (one tile writes to both tensors), cout no tile multiple,
    # craw = 0 / = csplit / > csplit, each with BIAS | RELU and with no flag
    _fwd2("f2_b_fastk_1x1", _fast("bf16", 128, 128, 4, 2, 8, 2, 0, 1, 0, 0), "bf16", (*PIX[:1], 64, *PIX[1:], 120, K1, S1, P0, 1), 40, (0, 40, 80)),
    _fwd2("f2_b_plain_1x1", _fast("bf16", 128, 128, 4, 2, 8, 2, 0, 0, 0, 0), "bf16", (*PIX[:1], 72, *PIX[1:], 120, K1, S1, P0, 1), 40, (0, 40, 80)),
    _fwd2("f2_b_lanek_1x3", _fast("bf16", 128, 160, 4, 2, 8, 2, 0, 1, 0, 1), "bf16", (*PIX[:1], 72, *PIX[1:], 152, K13, S1, (0, 1), 1), 64, (0, 64, 104)),
    _fwd2("f2_b_fastk_192", _fast("bf16", 128, 192, 4, 2, 8, 2, 0, 1, 0, 0), "bf16", (*PIX[:1], 128, *PIX[1:], 184, K1, S1, P0, 1), 72, (0, 72, 128)),
    _fwd2("f2_b_fastk_160", _fast("bf16", 128, 160, 4, 2, 8, 2, 0, 1, 0, 0), "bf16", (*PIX[:1], 64, *PIX[1:], 152, K1, S1, P0, 1), 56, (0, 56, 96)),
    # the remaining bf16 forms a caller reaches: the general loop (cin < 64: no whole k-step), LANEK at 64 / 128 / 192, the 64- and 96-filter
    # tiles (csplit inside the only filter tile), and the 256 x 256 tile (>= 768 tiles of 256 pixels x 256 filters, >= 24 k-steps)
    _fwd2("f2_b_plain_160", _fast("bf16", 128, 160, 4, 2, 8, 2, 0, 0, 0, 0), "bf16", (*PIX[:1], 16, *PIX[1:], 152, K1, S1, P0, 1), 56, (0, 56, 96)),
    _fwd2("f2_b_plain_192", _fast("bf16", 128, 192, 4, 2, 8, 2, 0, 0, 0, 0), "bf16", (*PIX[:1], 40, *PIX[1:], 184, K1, S1, P0, 1), 72, (0, 72, 128)),
    _fwd2("f2_b_lanek_128", _fast("bf16", 128, 128, 4, 2, 8, 2, 0, 1, 0, 1), "bf16", (*PIX[:1], 72, *PIX[1:], 120, K13, S1, (0, 1), 1), 40, (0, 40, 80)),
    _fwd2("f2_b_lanek_192", _fast("bf16", 128, 192, 4, 2, 8, 2, 0, 1, 0, 1), "bf16", (*PIX[:1], 72, *PIX[1:], 184, K13, S1, (0, 1), 1), 72, (0, 72, 128)),
    _fwd2("f2_b_plain_64", _fast("bf16", 128, 64, 4, 2, 8, 2, 0, 0, 0, 0), "bf16", (*PIX[:1], 40, *PIX[1:], 56, K1, S1, P0, 1), 24, (0, 24, 40)),
    _fwd2("f2_b_fastk_64", _fast("bf16", 128, 64, 4, 2, 8, 2, 0, 1, 0, 0), "bf16", (*PIX[:1], 64, *PIX[1:], 56, K1, S1, P0, 1), 24, (0, 24, 40)),
    _fwd2("f2_b_lanek_64", _fast("bf16", 128, 64, 4, 2, 8, 2, 0, 1, 0, 1), "bf16", (*PIX[:1], 72, *PIX[1:], 56, K13, S1, (0, 1), 1), 24, (0, 24, 40)),
    _fwd2("f2_b_96", _fast("bf16", 128, 96, 2, 2, 8, 2, 0, 0, 0, 0), "bf16", (*PIX[:1], 72, *PIX[1:], 88, K1, S1, P0, 1), 40, (0, 40, 64)),
    _fwd2("f2_b_256x256", _fast("bf16", 256, 256, 4, 2, 8, 2, 0, 0, 0, 0), "bf16", (2, 176, 222, 222, 448, K3, S1, P1, 1), 200, (0, 200, 328)),
    _fwd2("f2_f128", _fast("float", 128, 128, 2, 2, 8, 2, 0, 0, 0, 0), "fp32", (*PIX[:1], 13, *PIX[1:], 116, K3, S1, P1, 1), 44, (0, 44, 80)),
    _fwd2("f2_f160", _fast("float", 128, 160, 2, 2, 8, 2, 0, 0, 0, 0), "fp32", (*PIX[:1], 38, *PIX[1:], 148, K1, S1, P0, 1), 52, (0, 52, 100)),
    _fwd2("f2_f192", _fast("float", 128, 192, 2, 2, 8, 2, 0, 0, 0, 0), "fp32", (*PIX[:1], 38, *PIX[1:], 180, K1, S1, P0, 1), 68, (0, 68, 132)),
    _fwd2("f2_f64", _fast("float", 128, 64, 2, 2, 8, 2, 0, 0, 0, 0), "fp32", (*PIX[:1], 13, *PIX[1:], 52, K3, S1, P1, 1), 20, (0, 20, 36)),
    _fwd2("f2_f96", _fast("float", 128, 96, 2, 2, 8, 2, 0, 0, 0, 0), "fp32", (*PIX[:1], 38, *PIX[1:], 84, K1, S1, P0, 1), 28, (0, 28, 60)),
    _fwd2("f2_f256x64", _fast("float", 256, 64, 4, 1, 4, 4, 0, 0, 0, 0), "fp32", (2, 6, 365, 367, 28, K3, S1, P0, 1), 12, (0, 12, 20)),
    _fwd2("f2_x3_64", _fast("f32x3", 128, 64, 2, 2, 8, 2, 0, 0, 0, 0), "f32x3", (*PIX[:1], 13, *PIX[1:], 52, K3, S1, P1, 1), 20, (0, 20, 36)),
    _fwd2("f2_x3_96", _fast("f32x3", 128, 96, 2, 2, 8, 2, 0, 0, 0, 0), "f32x3", (*PIX[:1], 38, *PIX[1:], 84, K1, S1, P0, 1), 28, (0, 28, 60)),
    _fwd2("f2_x3_256x64", _fast("f32x3", 256, 64, 4, 1, 4, 4, 0, 0, 0, 0), "f32x3", (2, 6, 365, 367, 28, K3, S1, P0, 1), 12, (0, 12, 20)),
    _fwd2("f2_x3_128", _fast("f32x3", 128, 128, 2, 2, 8, 2, 0, 0, 0, 0), "f32x3", (*PIX[:1], 13, *PIX[1:], 116, K3, S1, P1, 1), 44, (0, 44, 80)),
    _fwd2("f2_x3_160", _fast("f32x3", 128, 160, 2, 2, 8, 2, 0, 0, 0, 0), "f32x3", (*PIX[:1], 38, *PIX[1:], 148, K1, S1, P0, 1), 52, (0, 52, 100)),
    _fwd2("f2_x3_192", _fast("f32x3", 128, 192, 2, 2, 8, 2, 0, 0, 0, 0), "f32x3", (*PIX[:1], 38, *PIX[1:], 180, K1, S1, P0, 1), 68, (0, 68, 132)),
    _fwd2("f2_stream64", "conv1x1_stream_kernel<64,4,0,0,1>", "bf16", (*PIX[:1], 72, *PIX[1:], 56, K1, S1, P0, 1), 24, (0, 24, 40), STREAM),
    _fwd2("f2_stream96", "conv1x1_stream_kernel<96,4,0,0,1>", "bf16", (*PIX[:1], 72, *PIX[1:], 88, K1, S1, P0, 1), 40, (0, 40, 64), STREAM),
    _fwd2("f2_stream192", "conv1x1_stream_kernel<192,3,0,0,1>", "bf16", (*PIX[:1], 72, *PIX[1:], 136, K1, S1, P0, 1), 72, (0, 72, 104), STREAM),
    _fwd2("f2_regw6", "conv1x1_regw_kernel<6,0,4,2,2>", "bf16", (*PIX[:1], 136, *PIX[1:], 200, K1, S1, P0, 1), 72, (0, 72, 136), REGW_SHORT),
    _fwd2("f2_regw8", "conv1x1_regw_kernel<8,0,4,2,2>", "bf16", (*PIX[:1], 200, *PIX[1:], 200, K1, S1, P0, 1), 72, (0, 72, 136), REGW_SHORT),
    _fwd2("f2_regw10", "conv1x1_regw_kernel<10,0,4,2,2>", "bf16", (*PIX[:1], 280, *PIX[1:], 264, K1, S1, P0, 1), 72, (0, 72, 136), REGW_SHORT),
    _fwd2("f2_regw24", "conv1x1_regw_kernel<24,0,9,1,3>", "bf16", (3, 712, 67, 61, 200, K1, S1, P0, 1), 72, (0, 72, 136), REGW),
    # ---- din_conv_dgrad_x, fused: four parity-class launches of conv_gather_fast_kernel<bf16,128,96,4,2,8,2,0,0,XSRC=1,0>; 3x3 stride 2 with
    # p0 and p1, odd and even map sides (the classes differ in size and in taps), x widths 72 (one whole + one partial k-step) and < 64
    _dgx("dx_p0_odd", [XSRC], "bf16", 0, (2, 88, 39, 47, 72, K3, S2, P0, 1), 72, 1),
    _dgx("dx_p1_even_mask", [XSRC], "bf16", MASK, (2, 88, 40, 46, 72, K3, S2, P1, 1), 40, 1),
    _dgx("dx_p1_mixed_accum", [XSRC], "bf16", ACCUM, (2, 80, 39, 46, 64, K3, S2, P1, 1), 72, 1, twice=True),
    _dgx("dx_p0_even_mask_accum", [XSRC], "bf16", MASK | ACCUM, (2, 88, 40, 48, 72, K3, S2, P0, 1), 56, 1, twice=True),
    # ---- ... the two-launch form: din_conv_dgrad's parity classes, then the one-source multi launch under ACCUM
    _dgx("dx2_f_mask_accum", [_fast("float", 128, 96, 2, 2, 8, 2, 0, 0, 0, 0), _mt("float", 96, 2)], "fp32", MASK | ACCUM, (2, 86, 39, 47, 38, K3, S2, P1, 1), 70, 0),
    _dgx("dx2_x3_mask", [_fast("f32x3", 128, 96, 2, 2, 8, 2, 0, 0, 0, 0), _mt("f32x3", 96, 2)], "f32x3", MASK, (2, 86, 40, 46, 38, K3, S2, P0, 1), 38, 0),
    _dgx("dx2_b_t64_accum", [_fast("bf16", 128, 64, 4, 2, 8, 2, 0, 0, 0, 0), _mt("bf16", 64, 4)], "bf16", ACCUM, (2, 40, 39, 47, 72, K3, S2, P1, 1), 72, 0,
         twice=True, stage1=True),
    _dgx("dx2_b_off", [_fast("bf16", 128, 96, 4, 2, 8, 2, 0, 0, 0, 0), _mt("bf16", 96, 2)], "bf16", 0, (2, 88, 39, 47, 72, K3, S2, P0, 1), 40, 0, OFF, twice=True),
    _dgx("dx2_b_off_mask", [_fast("bf16", 128, 96, 4, 2, 8, 2, 0, 0, 0, 0), _mt("bf16", 96, 2)], "bf16", MASK, (2, 88, 40, 46, 72, K3, S2, P1, 1), 72, 0, OFF, twice=True),
    # the small-geometry Mixed_6a: the classes of 4 / 2 / 2 taps (24 / 12 / 12 k-steps on 6 tiles) split their reduction (at most nk / 2 = 12
    # ways: plan_gather) and conv_splitk_finish_kernel masks in fp32 and stores t; the one-tap class (6 k-steps) does not; the multi launch
    # then stages its own term
    _dgx("dx2_b_splitk_mask", [T96, FINISH, _mt("bf16", 160, 2)], "bf16", MASK, (2, 288, 15, 23, 384, K3, S2, P0, 1), 64, 0, twice=True, split=12,
         lines=[T96, FINISH] * 3 + [T96, _mt("bf16", 160, 2)]),
]
IDS = [r["label"] for r in ROWS]
SPLITK_SHAPE = (2, 88, 21, 25, 184, K3, S1, P0, 1)          # CF's splitk_b_fwd: 13 k-steps on 30 tiles -> the planner splits the reduction


# ---- operands and the float64 reference -----------------------------------------------------------------------------------------------
def _tdt(row):
    return torch.bfloat16 if row["dtype"] == "bf16" else torch.float32


def _kstep(row):
    return 64 if row["dtype"] == "bf16" else 32          # reduction channels of one k-step (8 chunks of 16 bytes)


def _modes(row):
    """(craw, flags) of every launch form of the row (craw: din_conv_fwd2 only)"""
    if row["kind"] == "fwd2":
        return [(craw, flags) for craw in row["craws"] for flags in (BIAS | RELU, 0)]
    return [(0, row["flags"])]


def _mm(a, b):
    """a [M][k] . b [k][n] in float64 -> (product, the same over absolute values)"""
    return a @ b, a.abs() @ b.abs()


_CACHE = {}


def _operands(row, device="cpu"):
    """stored operands (host, storage dtype) and the float64 reference terms of a row, computed once and shared by its modes, launches and
    the bite test.  v / S: the contraction and its absolute-value sum, [*lead][c]; last / first: what the last 8 reduction channels of the
    last source / the last partial k-step of the first source contribute (first: None for one source)"""
    key = (row["label"], device)
    if key in _CACHE:
        return _CACHE[key]
    _CACHE.clear()
    tdt, ks = _tdt(row), _kstep(row)
    gen = torch.Generator().manual_seed(sum(map(ord, row["label"])))
    op = dict(tdt=tdt)

    def d64(t):
        return t.double().to(device)

    if row["kind"] == "multi":
        nb, h, w = PIX
        cin, M = row["cin"], nb * h * w
        ktot = sum(c for c, _, _ in row["srcs"])
        op["g"] = [torch.randn(nb, h, w, c, generator=gen).to(tdt) for c, _, _ in row["srcs"]]
        op["w"] = [(torch.randn(c, cin, 1, 1, generator=gen) * (2.0 / ktot) ** 0.5).to(tdt) for c, _, _ in row["srcs"]]
        v = torch.zeros(M, cin, dtype=torch.float64, device=device)
        S = torch.zeros_like(v)
        for g, wt in zip(op["g"], op["w"]):
            a, b = _mm(d64(g).reshape(M, -1), d64(wt)[:, :, 0, 0])
            v, S = v + a, S + b
        gl, wl = d64(op["g"][-1]).reshape(M, -1), d64(op["w"][-1])[:, :, 0, 0]
        last = gl[:, -8:] @ wl[-8:]
        first = None
        if len(row["srcs"]) > 1:
            c0 = (row["srcs"][0][0] - 1) // ks * ks
            first = d64(op["g"][0]).reshape(M, -1)[:, c0:] @ d64(op["w"][0])[c0:, :, 0, 0]
        lead, c = (nb, h, w), cin
    elif row["kind"] == "fwd2":
        nb, cin, h, w, cout, k, s, p, dil, oh, ow = CF._geometry(row["shape"])
        op["x"] = torch.randn(nb, h, w, cin, generator=gen).to(tdt)
        op["w"] = (torch.randn(cout, cin, *k, generator=gen) * (2.0 / (cin * k[0] * k[1])) ** 0.5).to(tdt)
        op["bias"] = torch.randn(cout, generator=gen) * 0.1
        v, S, last = CF.conv_reference(d64(op["x"]), d64(op["w"]), k, s, p, dil, oh, ow)
        first = None
        lead, c = (nb, oh, ow), cout
    else:
        nb, cin, h, w, cout, k, s, p, dil, oh, ow = CF._geometry(row["shape"])
        cx, M = row["x"][0], nb * h * w
        ktot = k[0] * k[1] * cout // (s[0] * s[1]) + cx                     # (a parity class sees about a quarter of the taps)
        op["g"] = torch.randn(nb, oh, ow, cout, generator=gen).to(tdt)
        op["w"] = (torch.randn(cout, cin, *k, generator=gen) * (2.0 / ktot) ** 0.5).to(tdt)
        op["gx"] = torch.randn(nb, h, w, cx, generator=gen).to(tdt)
        op["wx"] = (torch.randn(cx, cin, 1, 1, generator=gen) * (2.0 / ktot) ** 0.5).to(tdt)
        va, Sa, _ = CF.dgrad_reference(d64(op["g"]), d64(op["w"]), k, s, p, dil, h, w)
        gx, wx = d64(op["gx"]).reshape(M, cx), d64(op["wx"])[:, :, 0, 0]
        vb, Sb = _mm(gx, wx)
        op["va"], op["vb"] = va.reshape(M, cin).cpu(), vb.cpu()
        v, S = va.reshape(M, cin) + vb, Sa.reshape(M, cin) + Sb
        last = gx[:, -8:] @ wx[-8:]
        c0 = (cout - 1) // ks * ks                                           # the strided conv's last tap, its last partial k-step
        part = torch.zeros_like(d64(op["w"]))
        part[c0:, :, -1, -1] = d64(op["w"])[c0:, :, -1, -1]
        first = CF.dgrad_reference(d64(op["g"]), part, k, s, p, dil, h, w)[0].reshape(M, cin)
        lead, c = (nb, h, w), cin
    op.update(v=v.cpu().reshape(*lead, c), S=S.cpu().reshape(*lead, c), last=last.cpu().reshape(*lead, c),
              first=None if first is None else first.cpu().reshape(*lead, c), lead=lead, c=c)
    if row["kind"] != "fwd2":
        op["mask"], op["on"] = CF._mask_tensor((*lead, c), tdt, gen)
        op["old"] = (torch.randn(*lead, c, generator=gen) * float(op["v"].std())).to(tdt)
    _CACHE[key] = op
    return op


def _reduction(row):
    """the whole reduction length kh kw c + sum_b cout_b"""
    if row["kind"] == "multi":
        return sum(c for c, _, _ in row["srcs"])
    nb, cin, h, w, cout, k, s, p, dil = row["shape"]
    return k[0] * k[1] * cin if row["kind"] == "fwd2" else k[0] * k[1] * cout + row["x"][0]


def _expect(row, op, craw, flags):
    """(v, S, exact, staged, extra) of one mode.  exact: elements that must be 0 / the old value bit for bit; staged: the bf16-staged terms
    of a twice=True row (what bar_of multiplies by 2^-7 (1 + 2^-8)); extra: the two-launch form's 2^-7 |t| for its bf16 intermediate"""
    v, S = op["v"], op["S"]
    if row["kind"] == "fwd2":
        cooked = torch.arange(op["c"]) < (craw if craw > 0 else op["c"])
        if flags & BIAS:
            b = op["bias"].double() * cooked
            v, S = v + b, S + b.abs()
        if flags & RELU:
            v = torch.where(cooked, v.clamp_min(0), v)
        return v, S, None, None, 0.0
    exact = None
    on = op["on"] if flags & MASK else torch.ones_like(op["on"])
    if flags & MASK:
        exact = ~op["on"]
        v, S = v * on, S * on
    staged, extra = None, 0.0
    if row.get("twice"):
        if row["kind"] == "dgx" and not row["fused"]:
            g1, g2 = (op["va"].reshape(v.shape) * on).abs(), (op["vb"].reshape(v.shape) * on).abs()
            staged = g2 + (g1 if row["stage1"] else 0.0)
        elif flags & ACCUM:
            staged = v
    if row["kind"] == "dgx" and not row["fused"] and row["dtype"] == "bf16":
        t = op["va"].reshape(v.shape) * on + (op["old"].double() if flags & ACCUM else 0.0)
        extra = 2.0 ** -7 * t.abs()
    if flags & ACCUM:
        v, S = v + op["old"].double(), S + op["old"].double().abs()
    return v, S, exact, staged, extra


def _bar(row, v, S, staged, extra, plain=False):
    """CF.bar_of on a row of the same reduction length (K = length + 2; fp32 two-launch rows: one more summation term)"""
    like = dict(shape=(1, _reduction(row), 1, 1, 1, K1, S1, P0, 1), which=0, dtype="bf16" if row["dtype"] == "bf16" else "fp32", twice=not plain and row.get("twice"))
    more = (1 if row["kind"] == "dgx" and not row["fused"] and row["dtype"] != "bf16" else 0) + row.get("split", 0)
    return CF.bar_of(like, v, S, more, None if plain else staged) + (0.0 if plain else extra)


# ---- descriptors, names -------------------------------------------------------------------------------------------------------------
def _dt(L, row):
    return {"bf16": L.DIN_BF16, "fp32": L.DIN_F32, "f32x3": L.DIN_F32_BF16X3}[row["dtype"]]


def _desc(L, row, shape=None, views=None):
    like = dict(shape=shape or row["shape"], views=views or row["views"], dtype="fp32" if row["dtype"] != "bf16" else "bf16")
    d = CF._desc(L, like)
    d.dtype = _dt(L, row)
    return d


def _desc_1x1(L, row, cin, cout, ldo, cooff):
    """the 1x1 / stride-1 descriptor a source's filter bank is packed under"""
    nb, h, w = row["shape"][0], row["shape"][2], row["shape"][3]
    return _desc(L, row, (nb, cin, h, w, cout, K1, S1, P0, 1), (_pad(cin, 8) + 8, 0, ldo, cooff))


def _sources(L, row, ptrs=None):
    """the din_conv_src array of a multi row / the extra source of a dgrad_x row; ptrs: [(dout, wpk_t)] device pointers (None: left null --
    the reporters read none)"""
    spec = row["srcs"] if row["kind"] == "multi" else [row["x"]]
    srcs = (L.ConvSrc * len(spec))()
    for j, (c, ld, off) in enumerate(spec):
        srcs[j].cout, srcs[j].ldo, srcs[j].cooff = c, ld, off
        if ptrs is not None:
            srcs[j].dout, srcs[j].wpk_t = ptrs[j]
    return srcs


def _names(lib, L, row, craw, flags):
    """what the row's own reporter answers for one mode: (return code, lines)"""
    buf = C.create_string_buffer(4096)
    m = (row["maskv"] if row["kind"] == "multi" else row["views"][4:]) if flags & MASK else (0, 0)
    if row["kind"] == "multi":
        nb, h, w = PIX
        rc = lib.din_conv1x1_dgrad_multi_kernel_names(len(row["srcs"]), _sources(L, row), _dt(L, row), nb, h, w, row["cin"], *row["out"], *m, flags, buf, len(buf))
    elif row["kind"] == "fwd2":
        rc = lib.din_conv_fwd2_kernel_names(C.byref(_desc(L, row)), *row["views"][4:], row["csplit"], craw, flags, buf, len(buf))
    else:
        rc = lib.din_conv_dgrad_x_kernel_names(C.byref(_desc(L, row)), _sources(L, row), *m, flags, buf, len(buf))
    return rc, buf.value.decode().split()


def _assert_named(lib, L, row, monkeypatch):
    """the row's options are set (and stay set for the caller); every mode of the row launches the kernel(s) the row names"""
    for name, value in row["opts"].items():
        monkeypatch.setenv(name, value)
    for craw, flags in _modes(row):
        rc, got = _names(lib, L, row, craw, flags)
        assert 0 < rc <= 4096, f"{row['label']}: the reporter returned {rc}: {lib.din_last_error_string()}"
        if row["kind"] == "dgx":
            assert lib.din_conv_dgrad_x_fused(C.byref(_desc(L, row))) == row["fused"], f"{row['label']}: din_conv_dgrad_x_fused"
            want = row["lines"] or (row["names"] * 4 if row["fused"] else row["names"][:-1] * 4 + row["names"][-1:])   # four parity classes (+ the multi launch)
            assert got == want, f"{row['label']}: flags {flags} launch {got}, not {want}"
        else:
            assert got == [row["name"]], f"{row['label']}: craw {craw} flags {flags} launch {got}, not {row['name']}"


def _library():
    return CF._library()


# ---- CPU tests ----------------------------------------------------------------------------------------------------------------------------
def test_rows_resolve_to_their_kernels_and_cover_the_required_names(monkeypatch):
    lib, L = _library()
    for row in ROWS:
        _assert_named(lib, L, row, monkeypatch)
        for name in row["opts"]:
            L.set_option(name, None)
    with open(NAMES_FILE) as fh:
        required = {tuple(line.split()[:2]) for line in fh if line.strip()} | EXTRA_REQUIRED
    assert len(required) >= 60 and {e for e, _ in required} == set(ENTRY.values())
    have = {(ENTRY[r["kind"]], n) for r in ROWS for n in r.get("names", [r["name"]])}      # a name counts only under the entry point its row launches through
    missing = required - have
    assert not missing, f"(entry point, kernel) pairs without a row: {sorted(missing)}"
    for dtype in ("bf16", "fp32", "f32x3"):
        for flagset in (0, MASK, ACCUM, MASK | ACCUM):
            assert any(r["kind"] == "multi" and r["dtype"] == dtype and r["flags"] == flagset and "fast_kernel" in r["name"] for r in ROWS), (dtype, flagset)
    assert {len(r["srcs"]) for r in ROWS if r["kind"] == "multi"} == {1, 2, 3, 4}
    assert {r["flags"] for r in ROWS if r["kind"] == "dgx" and r["fused"]} == {0, MASK, ACCUM, MASK | ACCUM}


def test_reporters_share_the_argument_checks_of_their_entry_points():
    """no GPU: what the launch would refuse, the reporter refuses with the same code -- a din_conv_fwd2 shape that runs split-K, ACCUM on a
    forward, BIAS on a data gradient, a source view that does not cover its channels; and the size query writes nothing"""
    lib, L = _library()
    row = dict(kind="fwd2", dtype="bf16", shape=SPLITK_SHAPE, views=_fwd2("x", "", "bf16", SPLITK_SHAPE, 72, (0,))["views"], csplit=72)
    assert lib.din_conv_workspace_bytes(C.byref(_desc(L, row)), 0) > 0
    assert _names(lib, L, row, 0, BIAS | RELU)[0] == -1 and b"split-K" in lib.din_last_error_string()          # DIN_E_ARG
    ok = next(r for r in ROWS if r["label"] == "f2_b_fastk_1x1")
    assert _names(lib, L, ok, 0, ACCUM)[0] == -1
    assert _names(lib, L, dict(ok, csplit=44), 0, 0)[0] == -1                                                  # csplit % 8 != 0
    assert lib.din_conv_fwd2_kernel_names(C.byref(_desc(L, ok)), *ok["views"][4:], ok["csplit"], 0, 0, None, 0) == len(ok["name"]) + 2
    m = next(r for r in ROWS if r["label"] == "mt96_b_mask")
    assert _names(lib, L, m, 0, BIAS)[0] == -1
    assert _names(lib, L, dict(m, srcs=[(40, 40, 8)]), 0, 0)[0] == -1                                          # ldo < cooff + cout
    x = next(r for r in ROWS if r["label"] == "dx_p0_odd")
    assert _names(lib, L, x, 0, RELU)[0] == -1
    assert _names(lib, L, dict(x, x=(72, 72, 16)), 0, 0)[0] == -1


def test_reference_indexing():
    """the multi reference against conv2d_input of the concatenated 1x1 in float64; fwd2's two-destination split and craw; dgrad_x's sum"""
    row = next(r for r in ROWS if r["label"] == "mt96_f_mask")
    op = _operands(row)
    g = torch.cat([t.double() for t in op["g"]], -1).permute(0, 3, 1, 2)
    wt = torch.cat([t.double() for t in op["w"]], 0)
    want = torch.nn.grad.conv2d_input((PIX[0], row["cin"], *PIX[1:]), wt, g).permute(0, 2, 3, 1)
    assert float((op["v"] - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert bool((op["S"] >= op["v"].abs() - 1e-12).all())
    row = next(r for r in ROWS if r["label"] == "dx2_f_mask_accum")
    op = _operands(row)
    nb, cin, h, w, cout, k, s, p, dil, oh, ow = CF._geometry(row["shape"])
    want = torch.nn.grad.conv2d_input((nb, cin, h, w), op["w"].double(), op["g"].double().permute(0, 3, 1, 2), stride=s, padding=p)
    want = want + torch.nn.grad.conv2d_input((nb, cin, h, w), op["wx"].double(), op["gx"].double().permute(0, 3, 1, 2))
    assert float((op["v"] - want.permute(0, 2, 3, 1)).abs().max()) <= 1e-12 * float(want.abs().max())
    row = next(r for r in ROWS if r["label"] == "f2_f128")
    op = _operands(row)
    v, S, _, _, _ = _expect(row, op, 80, BIAS | RELU)
    y = torch.nn.functional.conv2d(op["x"].double().permute(0, 3, 1, 2), op["w"].double(), padding=1).permute(0, 2, 3, 1)
    assert float((v[..., :80] - (y[..., :80] + op["bias"].double()[:80]).clamp_min(0)).abs().max()) <= 1e-12
    assert float((v[..., 80:] - y[..., 80:]).abs().max()) <= 1e-12 and float(v[..., 80:].min()) < 0


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_bars_bite(row, monkeypatch):
    """the row's bar on the row's data: a result that lost the last 8 reduction channels of the last source (fwd2: of the last tap) moves
    >= 10 % of the produced elements beyond it, and so does one that lost the last partial k-step of the first source (rows with >= 2
    sources; dgrad_x: of the strided conv's last tap); under ACCUM a second bf16 rounding before the add is caught by the plain bar"""
    lib, L = _library()
    _assert_named(lib, L, row, monkeypatch)
    op = _operands(row)
    craw, flags = (0, 0) if row["kind"] == "fwd2" else (0, row["flags"])
    v, S, _, staged, extra = _expect(row, op, craw, flags)
    on = op["on"] if flags & MASK else 1.0
    for what, lost in (("the last 8 channels of the last source", op["last"]), ("the last partial k-step of the first source", op["first"])):
        if lost is None:
            continue
        for plain in (True, False):
            share = float(((lost * on).abs() > _bar(row, v, S, staged, extra, plain)).double().mean())
            assert share >= 0.10, f"{row['label']}: dropping {what} moves only {share:.3f} of the elements beyond the {'plain' if plain else 'row'} bar"
    if flags & ACCUM:
        conv = v - op["old"].double()
        twice = (conv.bfloat16().double() + op["old"].double()).to(op["tdt"]).double()
        n = int(((twice - v).abs() > _bar(row, v, S, staged, extra, plain=True)).sum())
        assert n >= 1, f"{row['label']}: a second bf16 rounding before the accumulate passes the bar everywhere"


# ---- the GPU tests ------------------------------------------------------------------------------------------------------------------------
def _pack(lib, L, d, wt, transposed):
    tdt = torch.bfloat16 if d.dtype == L.DIN_BF16 else torch.float32
    wdev = wt.float().cuda()
    wpk = torch.empty(lib.din_conv_packed_elems(C.byref(d), transposed), dtype=tdt, device="cuda")
    L.check(lib.din_conv_pack_weights(C.byref(d), wdev.data_ptr(), None, wpk.data_ptr(), transposed, None))
    return wpk


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_multi_kernel_against_fp64(env, row, monkeypatch):
    lib, L, nhwc, ops = env
    _assert_named(lib, L, row, monkeypatch)
    op = _operands(row, "cuda")
    tdt, lead, c = op["tdt"], op["lead"], op["c"]
    epc = 8 if row["dtype"] == "bf16" else 4
    gen = torch.Generator().manual_seed(11)
    keep, wsb = [], 0
    if row["kind"] == "multi":
        ldi, cioff = row["out"]
        ldm, moff = row["maskv"]
        like = dict(row, shape=(PIX[0], row["cin"], *PIX[1:]))
        ptrs = []
        for (co, ld, off), g, wt in zip(row["srcs"], op["g"], op["w"]):
            gd, wp = CF._view(g, tdt, ld, off, _pad(co, epc)), _pack(lib, L, _desc_1x1(L, like, row["cin"], co, ld, off), wt, 1)
            keep += [gd, wp]
            ptrs.append((gd.data_ptr(), wp.data_ptr()))
        srcs = _sources(L, row, ptrs)
        dests = [dict(CF._guarded(lead, ldi, tdt, gen), off=cioff, c=c)]
    elif row["kind"] == "fwd2":
        nb, cin, h, w, cout, k, s, p, dil, oh, ow = CF._geometry(row["shape"])
        ldi, cioff, ldo, cooff, ldo2, cooff2 = row["views"]
        d, cs = _desc(L, row), row["csplit"]
        src, wpk, bias = CF._view(op["x"], tdt, ldi, cioff, _pad(cin, epc)), _pack(lib, L, d, op["w"], 0), op["bias"].cuda()
        dests = [dict(CF._guarded(lead, ldo, tdt, gen), off=cooff, c=cs, lo=0), dict(CF._guarded(lead, ldo2, tdt, gen), off=cooff2, c=cout - cs, lo=cs)]
    else:
        nb, cin, h, w, cout, k, s, p, dil, oh, ow = CF._geometry(row["shape"])
        ldi, cioff, ldo, cooff, ldm, moff = row["views"]
        cx, ldx, offx = row["x"]
        d = _desc(L, row)
        gd, wp = CF._view(op["g"], tdt, ldo, cooff, _pad(cout, epc)), _pack(lib, L, d, op["w"], 1)
        gxd, wxp = CF._view(op["gx"], tdt, ldx, offx, _pad(cx, epc)), _pack(lib, L, _desc_1x1(L, row, cin, cx, ldx, offx), op["wx"], 1)
        srcs = _sources(L, row, [(gxd.data_ptr(), wxp.data_ptr())])
        wsb = lib.din_conv_workspace_bytes(C.byref(d), 1)
        dests = [dict(CF._guarded(lead, ldi, tdt, gen), off=cioff, c=c)]
    if row["kind"] != "fwd2":
        mask = CF._view(op["mask"], tdt, ldm, moff, c)
    wsbuf, ws = CF._guarded_workspace(wsb)
    out = dests[0]["out"]

    for craw, flags in _modes(row):
        v, S, exact, staged, extra = _expect(row, op, craw, flags)
        bar = _bar(row, v, S, staged, extra).clamp_min(1e-300)
        mp, ml, mo = (mask.data_ptr(), ldm, moff) if flags & MASK else (None, 0, 0)

        def launch():
            if row["kind"] == "multi":
                L.check(lib.din_conv1x1_dgrad_multi(len(row["srcs"]), srcs, _dt(L, row), *PIX, row["cin"], ldi, cioff, out.data_ptr(), mp, ml, mo, flags, None))
            elif row["kind"] == "fwd2":
                L.check(lib.din_conv_fwd2(C.byref(d), src.data_ptr(), wpk.data_ptr(), bias.data_ptr() if flags & BIAS else None, out.data_ptr(),
                                          dests[1]["out"].data_ptr(), ldo2, cooff2, cs, craw, flags, None, 0, None))
            else:
                L.check(lib.din_conv_dgrad_x(C.byref(d), gd.data_ptr(), wp.data_ptr(), out.data_ptr(), mp, ml, mo, flags, srcs,
                                             ws.data_ptr() if wsb else None, wsb, None))

        for t in dests:
            lo = t.get("lo", 0)
            t.update(v=v[..., lo:lo + t["c"]], bar=bar[..., lo:lo + t["c"]], exact=exact, old=op["old"] if flags & ACCUM else None)
        CF._launch_twice_and_compare(f"{row['label']} craw={craw} flags={flags}", launch, wsbuf, wsb, dests)


@pytest.mark.gpu
def test_fwd2_refuses_a_split_k_shape_and_writes_nothing(env):
    """a shape whose plan splits the reduction: DIN_E_ARG from the launch and from the reporter, both destinations bit-identical"""
    lib, L, nhwc, ops = env
    row = _fwd2("splitk", "", "bf16", SPLITK_SHAPE, 72, (0,))
    nb, cin, h, w, cout, k, s, p, dil, oh, ow = CF._geometry(row["shape"])
    ldi, cioff, ldo, cooff, ldo2, cooff2 = row["views"]
    d = _desc(L, row)
    assert _names(lib, L, row, 0, BIAS | RELU)[0] == -1
    gen = torch.Generator().manual_seed(11)
    x = CF._view(torch.randn(nb, h, w, cin, generator=gen), torch.bfloat16, ldi, cioff, cin)
    wpk = _pack(lib, L, d, torch.randn(cout, cin, *k, generator=gen), 0)
    bias = torch.randn(cout, generator=gen).cuda()
    a, b = CF._guarded((nb, oh, ow), ldo, torch.bfloat16, gen), CF._guarded((nb, oh, ow), ldo2, torch.bfloat16, gen)
    wsb = lib.din_conv_workspace_bytes(C.byref(d), 0)
    assert wsb > 0
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    for t in (a, b):
        t["buf"].copy_(t["pattern"])
    rc = lib.din_conv_fwd2(C.byref(d), x.data_ptr(), wpk.data_ptr(), bias.data_ptr(), a["out"].data_ptr(), b["out"].data_ptr(), ldo2, cooff2, 72, 0,
                           BIAS | RELU, ws.data_ptr(), wsb, None)
    torch.cuda.synchronize()
    assert rc == -1 and b"split-K" in lib.din_last_error_string()
    for t in (a, b):
        assert torch.equal(CF._bits(t["buf"]), CF._bits(t["pattern"]))
