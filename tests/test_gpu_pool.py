"""Every kernel instantiation csrc/pool.hip launches (max-pool, average pool, bilinear resize; forward and backward) against a float64
reference written here from the definition of the operation, on the stored operands (bf16 rows: rounded to bf16 first, then widened).

One row of POOL_CASES per kernel instantiation and shape; the row's DIN_* options force the kernel, and din_pool_kernel_name -- the
decision function the launchers themselves switch on -- is asserted before anything runs (on the CPU as well: the query is host-only).
The reference is never another kernel of pool.hip.  Bars are per element and derived from the kernels' operation counts
(u32 = 2^-24, u16 = 2^-8):
  max-pool values     equal as numbers to the float64 maximum (-0.0 == +0.0 allowed: the row kernel documents it);
  arg-max bytes       the first maximum in scan order (r * k + s), 255 where the maximum is <= 0; byte for byte;
  max-pool backward   |err| <= (n + 1) u32 sum|terms| (n gradients reach the element; the prior value is a term under accumulate),
                      bf16 + u16 |ref|; the footprint (ref == 0 <=> got == 0) must match exactly in the overwrite modes;
  avg-pool            |err| <= (k^2 + 3) u32 S, S = sum|taps| / k^2 + |bias| + |prior|; bf16 + u16 |ref|; after ReLU max(ref, 0) is compared;
  bilinear            |err| <= (n + 4) u32 (sum w |x| + |prior|), n weighted terms (4 forward; backward: the contributing outputs), the
                      weights taken at the fp32 sample coordinates of the reference project's ATen call (scale = (in - 1) / (out - 1) and
                      src = scale * o, both rounded to fp32: hipcc divides fp32 correctly rounded and the library is built with
                      -ffp-contract=off, so the kernel's coordinates are numpy's bit for bit); bf16 + u16 |ref|.  A resize by exactly 1
                      must return its input bit for bit.
Every destination lies in a buffer with guard bands, its channels outside [coff, coff + c) full of NaN; all of that must come back bit
for bit, NaN poison in the source channels outside the view must not reach the result, and sources are not written.  Backward rows run
overwrite-into-NaN and accumulate-onto-prior, average pool / bilinear / map-free max-pool with and without the ReLU mask; average-pool
forward plain and with BIAS | RELU; max-pool forward with and without an arg-max pointer.  Rows whose 1-D grid has more than 3
workgroups are run again with DIN_POOL_GRID_CAP = 5 or 3 (fewer workgroups than the uncapped grid, so every thread makes several trips of
the grid-stride loop, on a grid xcd_remap cannot split evenly): same bits; every kernel launched on the capped grid has such a row
(test_every_capped_kernel_has_a_row_that_loops).
test_bars_bite (CPU) shows for every row and mode that a deliberately wrong float64 variant misses the bar by >= 10x.
Not covered: the >= 2^31-element index decode (dd.fast == 0) needs tens of GB per tensor."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.conftest import Measured
from tests.test_gpu_kernels import env  # noqa: F401  (the module-scoped library fixture)

U32, U16 = 2.0 ** -24, 2.0 ** -8
NG = 256                                  # guard elements on each side of every buffer (keeps the 16-byte alignment of the view)
BF, FP = "bf16", "fp32"
MAXPOOL_VALUES = torch.tensor([-1.0, -0.25, -0.0, 0.0, 0.5, 1.0, 2.0, 0.0])   # few values, all bf16: ties at zero and tied positive maxima

MODES = {
    "maxpool_fwd": ("amax", "noamax"),
    "maxpool_bwd": ("overwrite", "accumulate"),
    "maxpool_bwd_scan": ("overwrite", "accumulate", "overwrite_mask", "accumulate_mask"),
    "avgpool_fwd": ("plain", "bias_relu"),
    "avgpool_bwd": ("overwrite", "accumulate", "overwrite_mask", "accumulate_mask"),
    "bilinear_fwd": ("plain",),
    "bilinear_bwd": ("overwrite", "accumulate", "overwrite_mask", "accumulate_mask"),
}
OP_CODE = {"maxpool": 0, "avgpool": 1, "bilinear": 2}


def _row(name, kernel, op, dtype, shape, win, ld=None, opts=None, **extra):
    """shape = (nb, h, w, c); win = (k, stride, pad), bilinear: (oh, ow); ld = (ldi, cioff, ldo, cooff), default: dense"""
    c = shape[3]
    return dict(name=name, kernel=kernel, op=op, dtype=dtype, shape=shape, win=win, ld=ld or (c, 0, c, 0), opts=opts or {}, **extra)


def _avg(name, v, kind, dtype, shape, win, ld=None, opts=None):
    """the forward and the backward row of one average-pool shape; kind: 'box' / 'gen' (one thread per output) or 'strip'"""
    if kind == "strip":
        kf, kb = f"avgpool3_strip_kernel<{v}, 8, false>", f"avgpool3_strip_kernel<{v}, 8, true>"
    else:
        b = "true" if kind == "box" else "false"
        kf, kb = f"avgpool_fwd_kernel<{v}, {b}>", f"avgpool_bwd_kernel<{v}, {b}>"
    return [_row(name + "_fwd", kf, "avgpool_fwd", dtype, shape, win, ld, opts), _row(name + "_bwd", kb, "avgpool_bwd", dtype, shape, win, ld, opts)]


def _rowbwd(name, shape, ld=None):
    """the two row-kernel backward instantiations on one shape: <256, false> overwrites, <256, true> accumulates"""
    return [_row("mrowb_" + name, "maxpool3s2_row_bwd_kernel<256, false>", "maxpool_bwd", BF, shape, (3, 2, 0), ld, modes=("overwrite",)),
            _row("mrowba_" + name, "maxpool3s2_row_bwd_kernel<256, true>", "maxpool_bwd", BF, shape, (3, 2, 0), ld, modes=("accumulate",))]


ROWS0 = {"DIN_MAXPOOL_ROWS": "0"}
NOSTRIP = {"DIN_MAXPOOL_ROWS": "0", "DIN_MAXPOOL_STRIP": "0"}
AVG1 = {"DIN_AVGPOOL_STRIP": "0"}
FWD8, FWD4 = "maxpool_fwd_kernel<8, %d>", "maxpool_fwd_kernel<4, %d>"
AMAX8, AMAX4 = "maxpool_bwd_amax_kernel<8, %d>", "maxpool_bwd_amax_kernel<4, %d>"
POOL_CASES = [
    # ---- max-pool forward: one thread per output (window 3 / 2 / runtime), 16-byte bf16 vectors and 4-channel vectors (fp32; bf16 on ldi % 8 == 4)
    _row("mf8_3_s2p1", FWD8 % 3, "maxpool_fwd", BF, (3, 14, 18, 64), (3, 2, 1), (72, 8, 80, 16)),
    _row("mf8_3_s1p1", FWD8 % 3, "maxpool_fwd", BF, (1, 9, 7, 8), (3, 1, 1)),
    _row("mf8_3_exact", FWD8 % 3, "maxpool_fwd", BF, (1, 7, 9, 8), (3, 2, 0), (16, 8, 16, 0), NOSTRIP),
    _row("mf8_2_odd", FWD8 % 2, "maxpool_fwd", BF, (2, 13, 15, 192), (2, 2, 0), (200, 8, 192, 0)),
    _row("mf8_2_one_window", FWD8 % 2, "maxpool_fwd", BF, (1, 2, 2, 64), (2, 2, 0)),
    _row("mf8_0_k5s3p2", FWD8 % 0, "maxpool_fwd", BF, (1, 17, 20, 8), (5, 3, 2), (16, 8, 8, 0)),
    _row("mf4_3_f32_ragged", FWD4 % 3, "maxpool_fwd", FP, (2, 12, 14, 12), (3, 2, 0), (20, 4, 16, 4)),
    _row("mf4_3_bf16_s2p1", FWD4 % 3, "maxpool_fwd", BF, (3, 9, 11, 8), (3, 2, 1), (12, 4, 8, 0)),
    _row("mf4_2_f32_odd", FWD4 % 2, "maxpool_fwd", FP, (3, 13, 15, 4), (2, 2, 0), (8, 4, 4, 0)),
    _row("mf4_2_bf16", FWD4 % 2, "maxpool_fwd", BF, (1, 6, 5, 12), (2, 2, 0), (20, 4, 12, 0)),
    _row("mf4_0_f32_k5s3p2", FWD4 % 0, "maxpool_fwd", FP, (1, 11, 13, 8), (5, 3, 2), (8, 0, 12, 4)),
    _row("mf4_0_bf16_k4s2p1", FWD4 % 0, "maxpool_fwd", BF, (2, 9, 10, 4), (4, 2, 1), (12, 8, 4, 0)),
    _row("mf8_3_one_row", FWD8 % 3, "maxpool_fwd", BF, (2, 1, 9, 8), (3, 1, 1)),
    _row("mf4_3_f32_one_row", FWD4 % 3, "maxpool_fwd", FP, (2, 1, 7, 12), (3, 1, 1), (16, 4, 12, 0)),
    _row("mf8_0_big", FWD8 % 0, "maxpool_fwd", BF, (2, 40, 44, 16), (5, 3, 2)),
    _row("mf4_3_f32_big", FWD4 % 3, "maxpool_fwd", FP, (2, 33, 35, 12), (3, 2, 0), (20, 4, 16, 4)),
    _row("mf4_2_bf16_big", FWD4 % 2, "maxpool_fwd", BF, (2, 26, 30, 12), (2, 2, 0), (20, 4, 12, 0)),
    _row("mf4_0_f32_big", FWD4 % 0, "maxpool_fwd", FP, (2, 40, 44, 8), (5, 3, 2), (8, 0, 12, 4)),
    # column strips (R = 4 output rows; 7 output rows: a full and a partial strip) and with padding
    _row("mstrip_big", "maxpool3s2_strip_kernel<4>", "maxpool_fwd", BF, (2, 35, 47, 192), (3, 2, 0), None, ROWS0),
    _row("mstrip_wide", "maxpool3s2_strip_kernel<4>", "maxpool_fwd", BF, (3, 16, 9, 192), (3, 2, 0), (200, 8, 208, 16), ROWS0),
    _row("mstrip_s2p1", "maxpool3s2_strip_kernel<4>", "maxpool_fwd", BF, (1, 9, 11, 8), (3, 2, 1), None, {"DIN_MAXPOOL_STRIP": "2"}),
    # one workgroup per output row (v_max3 on tagged words)
    _row("mrow_ragged", "maxpool3s2_row_fwd_kernel<256>", "maxpool_fwd", BF, (2, 35, 47, 64), (3, 2, 0), (72, 8, 80, 16)),
    _row("mrow_long_row", "maxpool3s2_row_fwd_kernel<256>", "maxpool_fwd", BF, (1, 7, 600, 16), (3, 2, 0)),
    _row("mrow_one_window", "maxpool3s2_row_fwd_kernel<256>", "maxpool_fwd", BF, (1, 3, 3, 64), (3, 2, 0)),
    _row("mrow_even_uncovered", "maxpool3s2_row_fwd_kernel<256>", "maxpool_fwd", BF, (2, 36, 48, 32), (3, 2, 0), (40, 8, 32, 0)),
    # ---- max-pool backward from the arg-max map: NW windows per axis (2: 3/2/1, 5/3/2, 4/2/1; 1: 2/2/0; loop: 3/1/1)
    _row("mb8_2_s2p1", AMAX8 % 2, "maxpool_bwd", BF, (3, 14, 18, 64), (3, 2, 1), (72, 8, 80, 16)),
    _row("mb8_2_k5s3p2", AMAX8 % 2, "maxpool_bwd", BF, (1, 17, 20, 8), (5, 3, 2), (16, 8, 8, 0)),
    _row("mb8_1_odd", AMAX8 % 1, "maxpool_bwd", BF, (2, 13, 15, 192), (2, 2, 0), (200, 8, 192, 0)),
    _row("mb8_0_s1p1", AMAX8 % 0, "maxpool_bwd", BF, (1, 9, 7, 8), (3, 1, 1)),
    _row("mb4_2_f32_s2p1", AMAX4 % 2, "maxpool_bwd", FP, (2, 9, 11, 12), (3, 2, 1), (20, 4, 16, 4)),
    _row("mb4_2_bf16_k4s2p1", AMAX4 % 2, "maxpool_bwd", BF, (2, 9, 10, 4), (4, 2, 1), (12, 8, 4, 0)),
    _row("mb4_1_f32_odd", AMAX4 % 1, "maxpool_bwd", FP, (3, 13, 15, 4), (2, 2, 0), (8, 4, 4, 0)),
    _row("mb4_1_bf16", AMAX4 % 1, "maxpool_bwd", BF, (1, 6, 5, 12), (2, 2, 0), (20, 4, 12, 0)),
    _row("mb4_0_f32_s1p1", AMAX4 % 0, "maxpool_bwd", FP, (1, 7, 6, 8), (3, 1, 1), (8, 0, 12, 4)),
    _row("mb4_0_bf16_one_column", AMAX4 % 0, "maxpool_bwd", BF, (2, 5, 1, 8), (3, 1, 1), (12, 4, 8, 0)),
    _row("mb8_0_one_row", AMAX8 % 0, "maxpool_bwd", BF, (2, 1, 9, 8), (3, 1, 1)),
    _row("mb4_0_bf16_one_row", AMAX4 % 0, "maxpool_bwd", BF, (2, 1, 9, 8), (3, 1, 1), (12, 4, 8, 0)),
    _row("mb8_0_big", AMAX8 % 0, "maxpool_bwd", BF, (2, 24, 28, 16), (3, 1, 1)),
    _row("mb4_0_f32_big", AMAX4 % 0, "maxpool_bwd", FP, (2, 24, 28, 8), (3, 1, 1), (8, 0, 12, 4)),
    _row("mb4_2_f32_big", AMAX4 % 2, "maxpool_bwd", FP, (2, 33, 35, 12), (3, 2, 1), (20, 4, 16, 4)),
    _row("mb4_1_bf16_big", AMAX4 % 1, "maxpool_bwd", BF, (2, 26, 30, 12), (2, 2, 0), (20, 4, 12, 0)),
    # 3/2/0: a thread owns a 2x2 pixel block
    _row("mbk3s2_4_f32_big", "maxpool_bwd_amax_k3s2_kernel<4>", "maxpool_bwd", FP, (2, 33, 35, 12), (3, 2, 0), (20, 4, 16, 4)),
    _row("mbk3s2_8_ragged", "maxpool_bwd_amax_k3s2_kernel<8>", "maxpool_bwd", BF, (2, 35, 47, 64), (3, 2, 0), (72, 8, 80, 16), ROWS0),
    _row("mbk3s2_8_even", "maxpool_bwd_amax_k3s2_kernel<8>", "maxpool_bwd", BF, (1, 8, 10, 8), (3, 2, 0), None, ROWS0),
    _row("mbk3s2_4_f32", "maxpool_bwd_amax_k3s2_kernel<4>", "maxpool_bwd", FP, (2, 12, 14, 12), (3, 2, 0), (20, 4, 16, 4)),
    _row("mbk3s2_4_bf16", "maxpool_bwd_amax_k3s2_kernel<4>", "maxpool_bwd", BF, (1, 7, 9, 8), (3, 2, 0), (12, 4, 8, 0)),
    # 3/2/0 row kernels: odd h x odd w x cioff != 0 x ldi > c, a row wider than 256 items, one window, even sizes with an uncovered edge
    *_rowbwd("ragged", (2, 35, 47, 64), (72, 8, 80, 16)),
    *_rowbwd("long_row", (1, 7, 600, 16)),
    *_rowbwd("one_window", (1, 3, 3, 64)),
    *_rowbwd("even_uncovered", (2, 36, 48, 32), (40, 8, 32, 0)),
    # map-free backward (recomputes the arg-max from the input), with padding, with and without the ReLU mask
    _row("mscan_f32_s2p1", "maxpool_bwd_kernel", "maxpool_bwd_scan", FP, (2, 9, 11, 8), (3, 2, 1), (12, 4, 8, 0)),
    _row("mscan_bf16_odd", "maxpool_bwd_kernel", "maxpool_bwd_scan", BF, (1, 13, 15, 8), (2, 2, 0)),
    _row("mscan_bf16_s1p1", "maxpool_bwd_kernel", "maxpool_bwd_scan", BF, (2, 6, 7, 4), (3, 1, 1), (12, 4, 4, 0)),
    _row("mscan_f32_one_row", "maxpool_bwd_kernel", "maxpool_bwd_scan", FP, (2, 1, 9, 8), (3, 1, 1)),
    _row("mscan_f32_big", "maxpool_bwd_kernel", "maxpool_bwd_scan", FP, (2, 24, 28, 8), (3, 2, 1), (12, 4, 8, 0)),
    # ---- average pool: one thread per output, the 3/1/1 box as a template constant and the runtime window (2/2/0, 3/2/1, 5/1/2)
    *_avg("a8_box", 8, "box", BF, (2, 9, 11, 64), (3, 1, 1), (72, 8, 80, 16), AVG1),
    *_avg("a8_gen_k2s2", 8, "gen", BF, (2, 13, 15, 8), (2, 2, 0), (16, 8, 8, 0)),
    *_avg("a8_gen_k3s2p1", 8, "gen", BF, (1, 10, 7, 192), (3, 2, 1), (192, 0, 200, 8)),
    *_avg("a8_gen_k5s1p2", 8, "gen", BF, (3, 6, 7, 8), (5, 1, 2)),
    *_avg("a4_box_f32", 4, "box", FP, (2, 9, 5, 12), (3, 1, 1), (16, 4, 12, 0), AVG1),
    *_avg("a4_box_bf16", 4, "box", BF, (1, 4, 6, 8), (3, 1, 1), (12, 4, 8, 0), AVG1),
    *_avg("a4_gen_f32_k3s2p1", 4, "gen", FP, (2, 9, 11, 4), (3, 2, 1), (8, 4, 4, 0)),
    *_avg("a4_gen_f32_k5s1p2", 4, "gen", FP, (1, 5, 8, 8), (5, 1, 2), (8, 0, 12, 4)),
    *_avg("a4_gen_bf16_k2s2", 4, "gen", BF, (3, 7, 6, 12), (2, 2, 0), (20, 4, 12, 0)),
    *_avg("a8_gen_one_window_k2", 8, "gen", BF, (2, 2, 2, 8), (2, 2, 0)),
    *_avg("a8_gen_one_window_k3", 8, "gen", BF, (1, 3, 3, 64), (3, 2, 0), (72, 8, 64, 0)),
    *_avg("a4_gen_f32_one_window_k2", 4, "gen", FP, (2, 2, 2, 4), (2, 2, 0), (8, 4, 4, 0)),
    *_avg("a4_gen_bf16_one_window_k3", 4, "gen", BF, (1, 3, 3, 12), (3, 2, 0), (20, 4, 12, 0)),
    *_avg("a8_box_one_pixel", 8, "box", BF, (2, 1, 1, 8), (3, 1, 1), None, AVG1),
    *_avg("a4_box_f32_one_row", 4, "box", FP, (1, 1, 6, 4), (3, 1, 1), None, AVG1),
    *_avg("a8_gen_big", 8, "gen", BF, (2, 33, 35, 16), (3, 2, 1)),
    *_avg("a4_gen_f32_big", 4, "gen", FP, (2, 33, 35, 12), (3, 2, 1), (16, 4, 12, 0)),
    *_avg("a4_box_f32_big", 4, "box", FP, (2, 24, 20, 12), (3, 1, 1), (16, 4, 12, 0), AVG1),
    # column strips of 8 rows: h below, equal to, above the strip height and not a multiple of it; one column
    *_avg("astrip8_h5", 8, "strip", BF, (2, 5, 11, 64), (3, 1, 1), (72, 8, 80, 16)),
    *_avg("astrip8_h8", 8, "strip", BF, (1, 8, 6, 8), (3, 1, 1)),
    *_avg("astrip8_h19", 8, "strip", BF, (3, 19, 7, 192), (3, 1, 1), (200, 8, 192, 0)),
    *_avg("astrip4_f32_h19", 4, "strip", FP, (2, 19, 5, 12), (3, 1, 1), (16, 4, 12, 0)),
    *_avg("astrip4_f32_h8", 4, "strip", FP, (1, 8, 3, 4), (3, 1, 1), (4, 0, 8, 4)),
    *_avg("astrip4_bf16_one_column", 4, "strip", BF, (1, 5, 1, 8), (3, 1, 1), (12, 4, 8, 0)),
    *_avg("astrip4_bf16_h9", 4, "strip", BF, (3, 9, 4, 4), (3, 1, 1), (12, 8, 4, 0)),
    *_avg("astrip8_one_row", 8, "strip", BF, (2, 1, 9, 8), (3, 1, 1)),
    *_avg("astrip8_one_pixel", 8, "strip", BF, (2, 1, 1, 8), (3, 1, 1), (16, 8, 8, 0)),
    *_avg("astrip4_f32_one_row", 4, "strip", FP, (1, 1, 6, 4), (3, 1, 1)),
    *_avg("astrip4_bf16_one_pixel", 4, "strip", BF, (3, 1, 1, 8), (3, 1, 1), (12, 4, 8, 0)),
    *_avg("astrip4_f32_big", 4, "strip", FP, (3, 40, 30, 12), (3, 1, 1), (16, 4, 12, 0)),
    # ---- bilinear forward, one thread per output: mixed (up in y, down in x), down-sampling, oh = 1, ow = 1, h = 1, up-sampling with the cells off
    _row("bf8_mixed", "bilinear_fwd_kernel<8>", "bilinear_fwd", BF, (2, 7, 20, 64), (15, 9), (72, 8, 80, 16)),
    _row("bf8_down", "bilinear_fwd_kernel<8>", "bilinear_fwd", BF, (1, 15, 23, 8), (7, 11)),
    _row("bf8_oh1", "bilinear_fwd_kernel<8>", "bilinear_fwd", BF, (2, 6, 9, 8), (1, 5), (16, 8, 8, 0)),
    _row("bf8_up_cells_off", "bilinear_fwd_kernel<8>", "bilinear_fwd", BF, (1, 5, 6, 8), (11, 13), None, {"DIN_BILINEAR_CELLS": "0"}),
    _row("bf4_f32_ow1", "bilinear_fwd_kernel<4>", "bilinear_fwd", FP, (3, 5, 9, 4), (8, 1), (8, 4, 4, 0)),
    _row("bf4_f32_h1", "bilinear_fwd_kernel<4>", "bilinear_fwd", FP, (1, 1, 9, 12), (4, 20), (12, 0, 16, 4)),
    _row("bf4_bf16_down", "bilinear_fwd_kernel<4>", "bilinear_fwd", BF, (2, 9, 11, 8), (4, 5), (12, 4, 8, 0)),
    _row("bf8_w1", "bilinear_fwd_kernel<8>", "bilinear_fwd", BF, (2, 5, 1, 8), (9, 4)),
    _row("bf8_c192", "bilinear_fwd_kernel<8>", "bilinear_fwd", BF, (1, 7, 9, 192), (15, 5), (200, 8, 192, 0)),
    _row("bf4_f32_w1", "bilinear_fwd_kernel<4>", "bilinear_fwd", FP, (1, 4, 1, 4), (2, 3)),
    _row("bf4_f32_big", "bilinear_fwd_kernel<4>", "bilinear_fwd", FP, (2, 30, 40, 8), (20, 33), (8, 0, 12, 4)),
    # one thread per source cell (up-sampling): the production fuse, exactly 1, a large ratio, scales whose sc * o rounds onto integers (1/3)
    _row("bc8_fuse", "bilinear_fwd_cells_kernel<8>", "bilinear_fwd", BF, (1, 43, 78, 64), (87, 157), (64, 0, 72, 8)),
    _row("bc8_identity", "bilinear_fwd_cells_kernel<8>", "bilinear_fwd", BF, (2, 9, 11, 8), (9, 11), (16, 8, 8, 0), identity=True),
    _row("bc8_big_ratio", "bilinear_fwd_cells_kernel<8>", "bilinear_fwd", BF, (1, 3, 4, 8), (40, 37)),
    _row("bc4_f32_x_only", "bilinear_fwd_cells_kernel<4>", "bilinear_fwd", FP, (3, 5, 9, 4), (5, 31), (4, 0, 8, 4)),
    _row("bc4_f32_thirds", "bilinear_fwd_cells_kernel<4>", "bilinear_fwd", FP, (1, 4, 11, 8), (10, 31), (8, 0, 12, 4)),
    _row("bc4_f32_identity", "bilinear_fwd_cells_kernel<4>", "bilinear_fwd", FP, (1, 5, 7, 4), (5, 7), identity=True),
    _row("bc4_bf16_c12", "bilinear_fwd_cells_kernel<4>", "bilinear_fwd", BF, (2, 6, 5, 12), (13, 12), (20, 4, 12, 0)),
    _row("bc4_f32_big", "bilinear_fwd_cells_kernel<4>", "bilinear_fwd", FP, (2, 20, 24, 8), (45, 50)),
    # ---- bilinear backward, nested candidate scan: up-sampling by > 2.5x, a scale just below the 2 / sc + 3 <= 8 switch (41 / 103),
    # h = 1, oh = 1, ow = 1 (the sc = 0 branches), the production fuse with the hoisted kernel off
    _row("bb8_up3", "bilinear_bwd_kernel<8>", "bilinear_bwd", BF, (1, 5, 6, 8), (16, 19), (8, 0, 16, 8)),
    _row("bb8_below_switch", "bilinear_bwd_kernel<8>", "bilinear_bwd", BF, (1, 42, 5, 8), (104, 9)),
    _row("bb8_h1", "bilinear_bwd_kernel<8>", "bilinear_bwd", BF, (2, 1, 9, 8), (4, 20)),
    _row("bb8_fuse_hoist_off", "bilinear_bwd_kernel<8>", "bilinear_bwd", BF, (1, 43, 78, 8), (87, 157), None, {"DIN_BILINEAR_HOIST": "0"}),
    _row("bb4_f32_up3", "bilinear_bwd_kernel<4>", "bilinear_bwd", FP, (2, 4, 5, 12), (13, 15), (16, 4, 12, 0)),
    _row("bb4_f32_oh1", "bilinear_bwd_kernel<4>", "bilinear_bwd", FP, (1, 6, 9, 4), (1, 5)),
    _row("bb4_bf16_ow1", "bilinear_bwd_kernel<4>", "bilinear_bwd", BF, (2, 5, 9, 8), (8, 1), (12, 4, 8, 0)),
    _row("bb8_w1", "bilinear_bwd_kernel<8>", "bilinear_bwd", BF, (2, 5, 1, 8), (9, 4)),
    _row("bb4_f32_w1", "bilinear_bwd_kernel<4>", "bilinear_bwd", FP, (1, 4, 1, 4), (2, 3)),
    _row("bb4_f32_big", "bilinear_bwd_kernel<4>", "bilinear_bwd", FP, (2, 16, 20, 8), (50, 60)),
    # hoisted scan (8 candidates per axis): the fuse, a scale just above the switch (41 / 102), exactly 0.4, down-sampling, exactly 1, mixed
    _row("bh8_fuse", "bilinear_bwd_hoisted_kernel<8, 8>", "bilinear_bwd", BF, (1, 43, 78, 64), (87, 157), (72, 8, 64, 0)),
    _row("bh8_above_switch", "bilinear_bwd_hoisted_kernel<8, 8>", "bilinear_bwd", BF, (1, 42, 5, 8), (103, 9)),
    _row("bh8_scale_0.4", "bilinear_bwd_hoisted_kernel<8, 8>", "bilinear_bwd", BF, (1, 3, 5, 8), (6, 11)),
    _row("bh8_down", "bilinear_bwd_hoisted_kernel<8, 8>", "bilinear_bwd", BF, (2, 15, 23, 8), (7, 11)),
    _row("bh8_identity", "bilinear_bwd_hoisted_kernel<8, 8>", "bilinear_bwd", BF, (2, 9, 11, 8), (9, 11), (16, 8, 8, 0)),
    _row("bh8_mixed", "bilinear_bwd_hoisted_kernel<8, 8>", "bilinear_bwd", BF, (2, 7, 20, 64), (15, 9), (72, 8, 80, 16)),
    _row("bh4_f32_up2", "bilinear_bwd_hoisted_kernel<4, 8>", "bilinear_bwd", FP, (2, 7, 11, 8), (15, 23), (8, 0, 16, 8)),
    _row("bh4_f32_down", "bilinear_bwd_hoisted_kernel<4, 8>", "bilinear_bwd", FP, (1, 9, 8, 4), (4, 3), (8, 4, 4, 0)),
    _row("bh8_c192", "bilinear_bwd_hoisted_kernel<8, 8>", "bilinear_bwd", BF, (1, 7, 9, 192), (15, 5), (200, 8, 192, 0)),
    _row("bh4_bf16_c12", "bilinear_bwd_hoisted_kernel<4, 8>", "bilinear_bwd", BF, (2, 6, 5, 12), (13, 10), (20, 4, 12, 0)),
    _row("bh4_f32_big", "bilinear_bwd_hoisted_kernel<4, 8>", "bilinear_bwd", FP, (2, 20, 24, 8), (45, 50)),
]
CASES = [(r, m) for r in POOL_CASES for m in r.get("modes", MODES[r["op"]])]
CASE_IDS = [f"{r['name']}-{m}" for r, m in CASES]
assert len({r["name"] for r in POOL_CASES}) == len(POOL_CASES)


def _geometry(row):
    nb, h, w, c = row["shape"]
    if row["op"].startswith("bilinear"):
        return nb, h, w, c, 1, 1, 0, row["win"][0], row["win"][1]
    k, s, p = row["win"]
    return nb, h, w, c, k, s, p, (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1


def _grid_cap(row):
    """the DIN_POOL_GRID_CAP (5 or 3: not a multiple of the 8 XCDs) below this row's uncapped 1-D grid of 256-thread workgroups, so that
    the capped launch has to loop; None for the row kernels (own grid, no loop) and for rows of at most 3 workgroups"""
    nb, h, w, c, k, s, p, oh, ow = _geometry(row)
    kern, op = row["kernel"], row["op"]
    if "row_" in kern:
        return None
    cg = c // (4 if op == "maxpool_bwd_scan" or not ("<8" in kern or "strip_kernel<4>" in kern) else 8)
    if "maxpool3s2_strip" in kern:
        items = nb * -(-oh // 4) * ow * cg                       # a thread per strip of 4 output rows
    elif "avgpool3_strip" in kern:
        items = nb * -(-h // 8) * w * cg                         # ... of 8 rows
    elif "k3s2" in kern:
        items = nb * -(-h // 2) * -(-w // 2) * cg                # a thread per 2x2 pixel block
    elif op in ("maxpool_fwd", "avgpool_fwd") or kern.startswith("bilinear_fwd_kernel"):
        items = nb * oh * ow * cg                                # a thread per output
    else:
        items = nb * h * w * cg                                  # a thread per input pixel / source cell
    blocks = -(-items // 256)
    return 5 if blocks > 5 else 3 if blocks > 3 else None


# ---- float64 references, NHWC --------------------------------------------------------------------------------------------------------
def _padded(x, p, fill, shift=0):
    """x [nb][h][w][c] with p rows / columns of `fill` around it; shift = 1 moves every window origin one pixel up and left"""
    return F.pad(x, (0, 0, p + shift, p, p + shift, p), value=fill)


def _taps(xp, k, s, oh, ow):
    """(r * k + t, the [nb][oh][ow][c] slice of the padded tensor that tap (r, t) of every window reads), in scan order"""
    for r in range(k):
        for t in range(k):
            yield r * k + t, xp[:, r:r + s * (oh - 1) + 1:s, t:t + s * (ow - 1) + 1:s, :]


def maxpool_reference(x, k, s, p, oh, ow, ties="first", drop_last=False, shift=0):
    """the window maximum and its tap index (first maximum in scan order; ties='last': the wrong rule)"""
    nb, h, w, c = x.shape
    best = torch.full((nb, oh, ow, c), -float("inf"), dtype=torch.float64)
    arg = torch.zeros(nb, oh, ow, c, dtype=torch.long)
    for t, v in _taps(_padded(x, p, -float("inf"), shift), k, s, oh, ow):
        if drop_last and t == k * k - 1:
            continue
        win = v > best if ties == "first" else v >= best
        best, arg = torch.where(win, v, best), torch.where(win, torch.full_like(arg, t), arg)
    return best, arg


def _scatter(src, sel_of_tap, k, s, p, h, w):
    """dx [nb][h][w][c] = sum over windows and taps of src[window] * sel_of_tap(tap)[window] at the pixel the tap reads"""
    nb, oh, ow, c = src.shape
    dxp = torch.zeros(nb, h + 2 * p + k, w + 2 * p + k, c, dtype=torch.float64)
    for r in range(k):
        for t in range(k):
            dxp[:, r:r + s * (oh - 1) + 1:s, t:t + s * (ow - 1) + 1:s, :] += src * sel_of_tap(r * k + t)
    return dxp[:, p:p + h, p:p + w, :].clone()


def _bil_axis(n_in, n_out, align=True):
    """[n_out][n_in] interpolation matrix in float64, its sample coordinates computed in fp32 as ATen does for align_corners=True
    (area_pixel_compute_scale: (in - 1) / (out - 1), 0 for out == 1; src = scale * o); align=False: the wrong, half-pixel coordinates"""
    o = np.arange(n_out, dtype=np.float32)
    if align:
        sc = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
        src = (sc * o).astype(np.float32)
    else:
        src = np.maximum((o + np.float32(0.5)) * np.float32(n_in / n_out) - np.float32(0.5), 0).astype(np.float32)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    lam = (src - i0.astype(np.float32)).astype(np.float64)
    m = np.zeros((n_out, n_in))
    np.add.at(m, (np.arange(n_out), i0), 1.0 - lam)
    np.add.at(m, (np.arange(n_out), i1), lam)
    return torch.from_numpy(m)


def _roll(t):
    """shift by one pixel towards the origin (along w, or along h for one-column tensors); zeros enter at the far edge"""
    out = torch.zeros_like(t)
    if t.shape[2] > 1:
        out[:, :, :-1] = t[:, :, 1:]
    else:
        out[:, :-1] = t[:, 1:]
    return out


def _store(t, dtype):
    return t.to(torch.bfloat16 if dtype == BF else torch.float32)


_CACHE = {}


def _operands(row):
    """the stored operands of a row (torch tensors in the storage type, NHWC, channels of the view only), seeded by the row's name"""
    if row["name"] in _CACHE:
        return _CACHE[row["name"]]
    _CACHE.clear()
    nb, h, w, c, k, s, p, oh, ow = _geometry(row)
    gen = torch.Generator().manual_seed(zlib.crc32(row["name"].encode()))
    dt = row["dtype"]

    def away_from_zero(*shape):
        sign = torch.randint(0, 2, shape, generator=gen).float() * 2 - 1
        return _store(sign * (0.5 + 1.5 * torch.rand(shape, generator=gen)), dt)

    o = dict(g=away_from_zero(nb, oh, ow, c), prior=away_from_zero(nb, h, w, c))
    if row["op"].startswith("maxpool"):
        x = MAXPOOL_VALUES[torch.randint(0, len(MAXPOOL_VALUES), (nb, h, w, c), generator=gen)]
        if nb > 1:
            x[0] = torch.where(x[0] < 0, torch.zeros(()), x[0])         # a post-ReLU image: ties at zero
        if oh * ow > 1:
            neg = -torch.tensor([0.5, 1.0, 3.0])
            x[-1, :k, :k] = neg[torch.randint(0, 3, x[-1, :k, :k].shape, generator=gen)]        # a window where every value is negative
            x[-1, -k:, -k:] = neg[torch.randint(0, 3, x[-1, -k:, -k:].shape, generator=gen)]    # ... and one whose maximum is exactly +0.0
            x[-1, -1, -1] = 0.0
        o["x"] = _store(x, dt)
    else:
        o["x"] = _store(torch.randn(nb, h, w, c, generator=gen), dt)
        o["mask"] = _store(torch.randn(nb, h, w, c, generator=gen), dt)
        o["bias"] = torch.randn(c, generator=gen)
    _CACHE[row["name"]] = o
    return o


WRONG = {
    "maxpool_fwd": ("drop_last", "shift", "ties_last"),
    "maxpool_bwd": ("drop_last", "shift", "ties_last", "no_prior"),
    "maxpool_bwd_scan": ("drop_last", "shift", "ties_last", "no_prior", "flip_mask"),
    "avgpool_fwd": ("drop_last", "shift", "exclude_pad", "no_bias", "no_relu"),
    "avgpool_bwd": ("drop_last", "shift", "exclude_pad", "no_prior", "flip_mask"),
    "bilinear_fwd": ("half_pixel", "shift"),
    "bilinear_bwd": ("half_pixel", "shift", "no_prior", "flip_mask"),
}


def _applies(row, mode, wrong):
    """whether a wrong variant differs from the definition at all for this row and mode"""
    nb, h, w, c, k, s, p, oh, ow = _geometry(row)
    if wrong == "no_prior":
        return "accumulate" in mode
    if wrong in ("no_bias", "no_relu"):
        return mode == "bias_relu"
    if wrong == "exclude_pad":
        return p > 0
    if wrong == "drop_last":                                      # (one-column tensors: the last tap of every window lies in the padding)
        return k - 1 - p < h and k - 1 - p < w
    if wrong == "half_pixel":
        return (oh, ow) != (h, w)
    if wrong == "shift":                                          # (a one-pixel tensor shifted by one pixel is itself)
        return h * w > 1
    return True


def expected(row, mode, wrong=None):
    """float64 result of the row in this mode and the per-element bar; wrong: one of WRONG[op], a deliberately wrong variant.
    maxpool_fwd returns (values, arg-max bytes), every other op (want, bar)."""
    nb, h, w, c, k, s, p, oh, ow = _geometry(row)
    o, op, bf = _operands(row), row["op"], row["dtype"] == BF
    x, g, prior = o["x"].double(), o["g"].double(), o["prior"].double()
    acc, masked = "accumulate" in mode, "mask" in mode
    if wrong == "flip_mask":
        masked = not masked
    if wrong == "no_prior":
        acc = False
    shift, drop = int(wrong == "shift"), wrong == "drop_last"

    if op.startswith("maxpool"):
        fwd = op == "maxpool_fwd"
        best, arg = maxpool_reference(x, k, s, p, oh, ow, "last" if wrong == "ties_last" else "first", drop and fwd, shift if fwd else 0)
        if fwd:
            return best, torch.where(best > 0, arg, torch.full_like(arg, 255)).to(torch.uint8)
        if op == "maxpool_bwd":                                   # the map carries the ReLU mask: no gradient where the winner is <= 0
            arg = torch.where(best > 0, arg, torch.full_like(arg, 255))
        if drop:
            arg = torch.where(arg == k * k - 1, torch.full_like(arg, 255), arg)
        sel = lambda t: (arg == t).double()                      # noqa: E731
        want, terms, n = (_scatter(v, sel, k, s, p, h, w) for v in (g, g.abs(), torch.ones_like(g)))
        if shift:
            want = _roll(want)
        if op == "maxpool_bwd_scan" and masked:
            want = want * (x > 0)
        if acc:
            want, terms, n = want + prior, terms + prior.abs(), n + 1
        return want, (n + 1) * U32 * terms + (U16 * want.abs() if bf else 0)

    if op.startswith("avgpool"):
        ones = torch.ones(nb, h, w, 1, dtype=torch.float64)
        cnt = sum(v for _, v in _taps(_padded(ones, p, 0.0), k, s, oh, ow))                # in-bounds taps per window
        div = cnt.clamp_min(1) if wrong == "exclude_pad" else torch.full_like(cnt, k * k)
        if op == "avgpool_fwd":
            taps = [v for t, v in _taps(_padded(x, p, 0.0, shift), k, s, oh, ow) if not (drop and t == k * k - 1)]
            want, S = sum(taps) / div, sum(v.abs() for v in taps) / (k * k)
            if mode == "bias_relu":
                if wrong != "no_bias":
                    want, S = want + o["bias"].double(), S + o["bias"].double().abs()
                if wrong != "no_relu":
                    want = want.clamp_min(0)
        else:
            sel = lambda t: 0.0 if drop and t == k * k - 1 else 1.0                         # noqa: E731
            want, S = _scatter(g / div, sel, k, s, p, h, w), _scatter(g.abs() / (k * k), sel, k, s, p, h, w)
            if shift:
                want = _roll(want)
            if masked:
                want = want * (o["mask"].double() > 0)
            if acc:
                want, S = want + prior, S + prior.abs()
        return want, (k * k + 3) * U32 * S + (U16 * want.abs() if bf else 0)

    my, mx = _bil_axis(h, oh, wrong != "half_pixel"), _bil_axis(w, ow, wrong != "half_pixel")
    if op == "bilinear_fwd":
        xs = _roll(x) if shift else x
        want, terms = torch.einsum("oh,nhwc,pw->nopc", my, xs, mx), torch.einsum("oh,nhwc,pw->nopc", my, x.abs(), mx)
        n = torch.full_like(want, 4.0)
    else:
        want, terms = torch.einsum("oh,nopc,pw->nhwc", my, g, mx), torch.einsum("oh,nopc,pw->nhwc", my, g.abs(), mx)
        n = ((my != 0).sum(0).double()[:, None] * (mx != 0).sum(0).double()[None, :])[None, :, :, None].expand_as(want)
        if shift:
            want = _roll(want)
        if masked:
            want = want * (o["mask"].double() > 0)
        if acc:
            want, terms = want + prior, terms + prior.abs()
    return want, (n + 4) * U32 * terms + (U16 * want.abs() if bf else 0)


def _ratio(got, want, bar):
    """worst |got - want| / bar over the elements (0 where they agree exactly, so a zero bar asks for equality); NaN if got holds one"""
    diff = (got.double() - want).abs()
    return float(torch.where(diff == 0, torch.zeros_like(diff), diff / bar).max())


# ---- CPU: the bars bite, the rows carry the edges, the query names every row's kernel --------------------------------------------------
@pytest.mark.parametrize("row,mode", CASES, ids=CASE_IDS)
def test_bars_bite(row, mode):
    """every applicable wrong variant of the float64 reference misses this row's bar by >= 10x on at least one element"""
    tried = 0
    for wrong in WRONG[row["op"]]:
        if not _applies(row, mode, wrong):
            continue
        tried += 1
        if row["op"] == "maxpool_fwd":
            (best, amax), (b2, a2) = expected(row, mode), expected(row, mode, wrong)
            if wrong != "ties_last":                              # (the tie rule moves the arg-max, never the value)
                assert bool((b2 != best).any()), f"{row['name']}: {wrong} leaves every pooled value unchanged"
            assert bool((a2 != amax).any()), f"{row['name']}: {wrong} leaves every arg-max byte unchanged"
        else:
            want, bar = expected(row, mode)
            assert bool(torch.isfinite(want).all()) and bool((bar >= 0).all())
            assert _ratio(expected(row, mode, wrong)[0], want, bar) >= 10.0, f"{row['name']}/{mode}: the bar does not see '{wrong}'"
    assert tried >= 1, f"{row['name']}/{mode}: no wrong variant applies"


def test_maxpool_rows_carry_the_documented_edges():
    """tied positive maxima inside a window in every max-pool forward row; an all-negative window and a window whose maximum is exactly
    +0.0 in several of them; gradients and prior values bounded away from zero everywhere"""
    negative = zero = 0
    for row in POOL_CASES:
        o = _operands(row)
        assert float(o["g"].double().abs().min()) >= 0.5 and float(o["prior"].double().abs().min()) >= 0.5
        if row["op"] != "maxpool_fwd":
            continue
        nb, h, w, c, k, s, p, oh, ow = _geometry(row)
        x = o["x"].double()
        best, _ = maxpool_reference(x, k, s, p, oh, ow)
        hits = sum(((v == best) & (best > 0)).long() for _, v in _taps(_padded(x, p, -float("inf")), k, s, oh, ow))
        assert int((hits > 1).sum()) > 0, f"{row['name']}: no tied positive maximum"
        negative, zero = negative + bool((best < 0).any()), zero + bool((best == 0).any())
    assert negative >= 6 and zero >= 6, (negative, zero)


def test_every_capped_kernel_has_a_row_that_loops():
    """every kernel launched on the capped 1-D grid has a row whose uncapped grid exceeds the cap the GPU test sets for it"""
    loops = {r["kernel"] for r in POOL_CASES if _grid_cap(r)}
    assert loops == {r["kernel"] for r in POOL_CASES if "row_" not in r["kernel"]}


def _desc(L, row):
    nb, h, w, c, k, s, p, oh, ow = _geometry(row)
    d = L.PoolDesc()
    d.nb, d.h, d.w, d.c, d.oh, d.ow, d.k, d.stride, d.pad = nb, h, w, c, oh, ow, k, s, p
    d.ldi, d.cioff, d.ldo, d.cooff = row["ld"]
    d.dtype = L.DIN_BF16 if row["dtype"] == BF else L.DIN_F32
    return d


def _kernel_name(lib, L, d, row, mode):
    family, _, direction = row["op"].partition("_")
    buf = C.create_string_buffer(128)
    L.check(lib.din_pool_kernel_name(C.byref(d), OP_CODE[family], int(direction.startswith("bwd")), int(row["op"] == "maxpool_bwd"),
                                     int("accumulate" in mode), buf, len(buf)))
    return buf.value.decode()


@pytest.mark.parametrize("row,mode", CASES, ids=CASE_IDS)
def test_rows_resolve_to_their_kernels(row, mode, monkeypatch):
    """din_pool_kernel_name is host-only: the table's options and shapes pick the kernels it says they pick, without a GPU"""
    from din_amd import _lib as L
    for name, value in row["opts"].items():
        monkeypatch.setenv(name, value)
    d = _desc(L, row)
    assert _kernel_name(L.load(), L, d, row, mode) == row["kernel"]
    v8 = row["dtype"] == BF and all(v % 8 == 0 for v in (row["shape"][3], *row["ld"]))
    if row["op"] != "maxpool_bwd_scan":                           # the view takes the vector width the kernel's name claims
        assert ("<8" in row["kernel"] or "strip_kernel<4>" in row["kernel"] or "row_" in row["kernel"]) == v8, row["name"]


def test_kernel_name_query_rejects_bad_arguments():
    from din_amd import _lib as L
    lib, d = L.load(), _desc(L, POOL_CASES[0])
    buf = C.create_string_buffer(128)
    assert lib.din_pool_kernel_name(C.byref(d), 3, 0, 0, 0, buf, 128) != 0            # no such op
    assert lib.din_pool_kernel_name(C.byref(d), 0, 0, 0, 0, buf, 4) != 0              # buffer too small for the name
    assert lib.din_pool_kernel_name(None, 0, 0, 0, 0, buf, 128) != 0


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.view({torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.uint8: torch.uint8}[t.dtype])


class _View:
    """a device NHWC view [*lead][ld] between two guard bands; channels [off, off + c) hold `content` (poison when None), every other
    channel of the pixel stride poison: NaN (arg-max bytes: 77); guards -1234.5 (bytes: 200)"""

    def __init__(self, lead, c, ld, off, tdt, content=None):
        n = int(np.prod(lead)) * ld
        guard, poison = (200, 77) if tdt == torch.uint8 else (-1234.5, float("nan"))
        host = torch.full((n + 2 * NG,), guard, dtype=tdt)
        body = host[NG:NG + n].view(*lead, ld)
        body[:] = poison
        if content is not None:
            body[..., off:off + c] = content.to(tdt)
        self.flat = host.cuda()
        self.body = self.flat[NG:NG + n].view(*lead, ld)
        self.view = self.body[..., off:off + c]
        self.before = _bits(host).clone()
        self.outside = torch.ones(n + 2 * NG, dtype=torch.bool)
        self.outside[NG:NG + n].view(*lead, ld)[..., off:off + c] = False

    def ptr(self):
        return self.body.data_ptr()

    def untouched_outside(self):
        return torch.equal(_bits(self.flat).cpu()[self.outside], self.before[self.outside])

    def unchanged(self):
        return torch.equal(_bits(self.flat).cpu(), self.before)


@pytest.mark.gpu
@pytest.mark.parametrize("row,mode", CASES, ids=CASE_IDS)
def test_pool_kernel_against_fp64(env, row, mode, monkeypatch):
    lib, L, nhwc, ops = env
    for name, value in row["opts"].items():
        monkeypatch.setenv(name, value)
    nb, h, w, c, k, s, p, oh, ow = _geometry(row)
    ldi, cioff, ldo, cooff = row["ld"]
    d, op, name = _desc(L, row), row["op"], row["name"]
    assert _kernel_name(lib, L, d, row, mode) == row["kernel"], f"{name}: the launch resolves to another kernel"
    o = _operands(row)
    tdt = torch.bfloat16 if row["dtype"] == BF else torch.float32
    acc, masked, fwd = int("accumulate" in mode), "mask" in mode, op.endswith("_fwd")
    # sources: the input (forward, map-free max-pool backward) or the tensor whose sign is the ReLU mask, at the input's view; the
    # output gradient at the output's view; the arg-max map of the float64 reference (never the forward kernel's)
    src_in = _View((nb, h, w), c, ldi, cioff, tdt, o["x"] if fwd or op.startswith("maxpool") else o["mask"])
    src_out = None if fwd else _View((nb, oh, ow), c, ldo, cooff, tdt, o["g"])
    if op == "maxpool_fwd":
        best, amax_want = expected(row, mode)
    else:
        want, bar = expected(row, mode)
    amax_src = _View((nb, oh, ow), c, c, 0, torch.uint8, expected(dict(row, op="maxpool_fwd"), "amax")[1]) if op == "maxpool_bwd" else None
    bias = o["bias"].cuda() if op == "avgpool_fwd" else None

    def run():
        dst = _View((nb, oh, ow), c, ldo, cooff, tdt) if fwd else _View((nb, h, w), c, ldi, cioff, tdt, o["prior"] if acc else None)
        am = None
        if op == "maxpool_fwd":
            am = _View((nb, oh, ow), c, c, 0, torch.uint8) if mode == "amax" else None
            L.check(lib.din_maxpool_fwd(C.byref(d), src_in.ptr(), dst.ptr(), am.ptr() if am else None, None))
        elif op == "maxpool_bwd":
            L.check(lib.din_maxpool_bwd(C.byref(d), None, amax_src.ptr(), src_out.ptr(), dst.ptr(), 1, acc, None))
        elif op == "maxpool_bwd_scan":
            L.check(lib.din_maxpool_bwd(C.byref(d), src_in.ptr(), None, src_out.ptr(), dst.ptr(), int(masked), acc, None))
        elif op == "avgpool_fwd":
            flags = L.CONV_BIAS | L.CONV_RELU if mode == "bias_relu" else 0
            L.check(lib.din_avgpool_fwd(C.byref(d), src_in.ptr(), dst.ptr(), bias.data_ptr() if flags else None, flags, None))
        elif op == "avgpool_bwd":
            L.check(lib.din_avgpool_bwd(C.byref(d), src_out.ptr(), dst.ptr(), src_in.ptr() if masked else None, acc, None))
        elif op == "bilinear_fwd":
            L.check(lib.din_bilinear_fwd(C.byref(d), src_in.ptr(), dst.ptr(), None))
        else:
            L.check(lib.din_bilinear_bwd(C.byref(d), src_out.ptr(), dst.ptr(), src_in.ptr() if masked else None, acc, None))
        torch.cuda.synchronize()
        return dst, am

    dst, am = run()
    assert dst.untouched_outside(), f"{name}: wrote outside its channel view or its buffer"
    for v in (src_in, src_out, amax_src):
        assert v is None or v.unchanged(), f"{name}: a source was written"
    got = dst.view.cpu()
    if op == "maxpool_fwd":
        assert torch.equal(got.double(), best), f"{name}: pooled values differ from the float64 maximum"     # (-0.0 == +0.0)
        if am is not None:
            assert am.untouched_outside(), f"{name}: wrote outside the arg-max map"
            bad = (am.view.cpu() != amax_want).nonzero()
            assert bad.numel() == 0, f"{name}: {bad.shape[0]} arg-max bytes differ, first at {bad[0].tolist()}"
    else:
        worst = Measured(_ratio(got, want, bar))
        print(f"{name}/{mode}: worst |err| / bar = {float(worst):.3g}")
        assert worst <= 1.0, f"{name}/{mode}: worst error is {float(worst):.3g} x the bar"
        if op.startswith("maxpool") and not acc:
            assert torch.equal(got.double() == 0, want == 0), f"{name}: gradient footprint differs"
    if row.get("identity"):
        assert torch.equal(_bits(got.contiguous()), _bits(o["x"].contiguous())), f"{name}: a resize by exactly 1 changed bits"
    cap = _grid_cap(row)
    if cap is None:
        return
    # the grid-stride loop: fewer workgroups than the work needs (and not a multiple of the 8 XCDs) -- the same kernel, the same bits
    monkeypatch.setenv("DIN_POOL_GRID_CAP", str(cap))
    assert _kernel_name(lib, L, d, row, mode) == row["kernel"]
    dst2, am2 = run()
    assert torch.equal(_bits(dst2.flat), _bits(dst.flat)), f"{name}: the capped grid gives other bits"
    if am is not None:
        assert torch.equal(am2.flat, am.flat), f"{name}: the capped grid gives other arg-max bytes"
