"""Every kernel din_conv_fwd / din_conv_dgrad launch with no option set, by name, against a float64 reference with per-element bars.

One row of CONV_ROWS per kernel instantiation: (name, which, flags, dtype, shape, views, opts).  `name` is the line din_conv_kernel_names
answers for exactly that launch -- asserted before anything runs on the GPU, and for all rows on the CPU (test_rows_resolve_...).  The
required names are those of profiles/conv_kernel_names.txt (tools/conv_dispatch_table.py --names: both backbones, both dtypes, four
geometries, the misaligned views) plus EXTRA_REQUIRED: instantiations no backbone shape reaches but a caller can with no option set.

Shapes are the smallest on which the planner picks the kernel: >= 3 pixel tiles with a ragged last one, two images whose maps are no tile
multiple, padding taps on all borders (and p0 rows), produced channels that are no multiple of the filter tile, reduction channels that
leave a partial 64-channel k-step (the scalar-walk FASTK forms need whole k-steps by construction), fp32 channel counts that are no
multiple of 4, split reductions that do not divide by ks_per_split.  Floors the code sets: conv_small_kernel and the fp32 256x64 tile
M >= 256 Ki pixels, conv_halo_kernel M >= 64 Ki, the 256x256 tile 768 tiles with >= 24 k-steps and >= 224 filters.

Views: cioff, cooff != 0 and pixel strides wider than the views; operand channels outside a view hold a finite POISON, the chunk padding
zeros; the mask is its own tensor (ldm != ldi, moff != cioff) holding +0.0, -0.0, the smallest positive bf16 subnormal and negative values
at known positions.  Outputs: NaN inside the produced range (overwrite modes) or random values (ACCUM), a random pattern outside, guard
bands around them and around the workspace (0x7f bytes before every launch).  Every row launches twice; after each launch everything
outside the produced range is bit-identical to the prefill and no NaN is left inside.  bf16 descriptors need input views at multiples of
8, so the multiples-of-4-only views are forward outputs (cooff = 4), mask views (mask4 rows: the tile and halo kernels take them) and the
fp32 rows.

Names are not code paths where a kernel picks its epilogue at run time: conv_gather_fast_kernel stages its tile in LDS (staged_tile_store)
only when the produced channels, the output view and the mask view all sit on the 16-byte chunk grid and the reduction is not split, and
otherwise stores from the accumulators (epilogue_direct, with its own scalar BIAS / RELU / MASK / ACCUM code and tail stores).  Both run
in both dtypes: bf16 rows with 83 / 43 / 13 produced channels and a dgrad with a multiple-of-4 mask view take the direct one, the
*_staged_* fp32 rows (produced channels at multiples of 4) the staged one, its batched MASK / ACCUM form included.

Reference (conv_reference / dgrad_reference): float64 on the stored operands, one GEMM per tap through the one tap indexing of _taps; it
yields v and S = the same sum over absolute values (+ |bias|, + |old| under ACCUM).  Bars, per element, K = kh*kw*c_reduction + 2
(bias / old) + the number of ways the launch splits its reduction (_split_depth: from the workspace size and the named tile):
    bf16 output   |got - v| <= 2^-7 |v| + 2 (K + 2) 2^-24 S
    fp32 output   |got - v| <=            2 (K + 2) 2^-24 S
2^-7 |v| is twice the worst round-to-nearest error of one bf16 store; (K + 2) 2^-24 S bounds any-order fp32 summation of K terms (bf16
products are exact in fp32; fp32 products round once: the + 2); the factor 2 is the suite's 2x margin.  Each assert is a Measured ratio
max(err / bar) <= 1.  Where the reference mask is off the result must hold the bits of +0.0 (of the old value under ACCUM).

NOT covered here (reached only through a tuning option or a -DDIN_EXPERIMENTS build; the MULTI / SPLIT / XSRC / csplit forms of
din_conv_fwd2, din_conv1x1_dgrad_multi and din_conv_dgrad_x have their rows, on this file's harness, in tests/test_gpu_conv_multi.py):
    conv_gather_fast_kernel  256x64 <4,1,8,2> (DIN_CONV_PIPE=0); 128x64 <2,2,8,3>, 128x128 <2,2,4,4>, 256x256 / 256x128 <4,2,4,4>
                             (DIN_CONV_PIPE=1); the bf16 4-wave 128-pixel forms (DIN_CONV_PIPE=4); 128x96 <4,2> without tap remap
                             (DIN_CONV_PIPE=8); 256x96 / 256x128 / 256x160 / 256x192 (DIN_CONV_TILE=256); 128x192 <2,4,8,2> (DIN_CONV_WAVEGRID=24);
                             the general loop where FASTK / LANEK would serve (DIN_CONV_FASTK=0, DIN_CONV_LANEK=0) and LANEK dgrads
                             (DIN_CONV_LANEK=2); every MULTI = 1 and XSRC = 1 form (test_gpu_conv_multi.py); 128x160 / 128x192 <4,2,4,3>, 256x{128,160,192} <8,2,8,2>,
                             128x{128,160,192} <2,2,4,2> (DIN_EXPERIMENTS)
    conv_gather_pipe_kernel<128 | 192 | 256> (DIN_GATHER_PIPE)
    conv_halo_kernel         the 8-wave forms <64 | 96,3,3,8,32,3> (DIN_HALO_WAVES=8) and the 1x7 / 7x1 forms <64 | 96,1,7,16,16,3>,
                             <64 | 96,7,1,16,16,3> (chosen only under DIN_CONV_HALO=2)
    conv_small_kernel        <4,64,2,3,3,1,0,4,0>, <8,32,1,3,3,1,0,4,0> (DIN_CONV_SMALL_WAVES=4); <8,32,2,3,3,1,0,8,0 | 1> (DIN_CONV_SMALL_NBUF8=2);
                             the store-loop epilogue of the dgrad forms (DIN_CONV_SMALL_EPI=0)
    conv1x1_stream_kernel    MULTI = 1 and SPLIT = 1 (test_gpu_conv_multi.py); a forced filter tile (DIN_CONV_STREAM_BN)
    conv1x1_regw_kernel      <6 | 10,1,...>, <10,0,...> dgrads: no shape here asks for them; multi-source and csplit launches
                             (test_gpu_conv_multi.py holds all of these)

FOUND with this file (MI355X, at the plain bars above, max(err / bar) per row): stream64_dg_accum 42.14, stream64_dg_mask_accum 35.08,
    stream192_dg_accum 58.90, small4_32_dg_accum 17.25, small4_32_dg_mask_accum 15.84, small8_32_dg_accum 6.04, small8_32_dg_mask_accum
    5.92 -- with the three conv_gather_fast_kernel ACCUM rows (same epilogue), every bf16 ACCUM row of the three kernels that stage their output tile
    in LDS as bf16 and add the old value to the staged element (their MASK-only rows measure 0.47-0.49; conv_halo_kernel, the split-K
    finish and the generic kernel add in fp32 and pass the plain bar under ACCUM at 0.47-0.49).  The ratio is large where gradient and old
    value cancel (|v| << |g|): the first rounding's 2^-8 |g| is then the whole error.  Two roundings by design (the staging is what makes
    the stores whole 16-byte chunks of pixel rows), so those ten rows carry twice=True and the term derived at bar_of, and no other row does.
FIXED with this file: gen_b128_fwd_7x7 found din_conv_workspace_bytes sizing a split reduction for the planned 96-filter tile while the
    generic kernel, re-tiled to 128 filters, wrote 128-filter rows of partial sums: past the caller's workspace (plan_gather now sizes
    such a re-tiled launch, and only such a launch, for the 128-filter padding; run_gather refuses a workspace smaller than what the chosen
    kernel writes)."""
import ctypes as C
import os

import pytest
import torch

from oracle import din_oracle as O
from tests.conftest import Measured, ROOT
from tests.test_gpu_kernels import env  # noqa: F401  (the module-scoped library fixture)

POISON = 1000.0                           # operand channels outside a view
NG = 256                                  # guard elements on each side of an output (keeps its 16-byte alignment)
WS_GUARD = 4096                           # guard bytes on each side of the workspace
BIAS, RELU, ACCUM, MASK = 1, 2, 4, 8
SUBNORMAL = 2.0 ** -133                   # smallest positive bf16 subnormal (exact in fp32 and fp64): x > 0 holds
NAMES_FILE = os.path.join(ROOT, "profiles", "conv_kernel_names.txt")
EXTRA_REQUIRED = {"conv_gather_generic_kernel<float,64>", "conv_gather_generic_kernel<float,128>", "conv_gather_generic_kernel<bf16,64>",
                  "conv_gather_generic_kernel<bf16,128>", "conv_gather_fast_kernel<float,256,64,4,1,4,4,0,0,0,0>",
                  "conv_splitk_finish_kernel<float>", "conv_splitk_finish_kernel<bf16>"}


def _pad(n, m):
    return (n + m - 1) // m * m


def _row(label, name, which, flags, dtype, shape, opts=None, m4=False, **extra):
    """shape = (nb, cin, h, w, cout, k, s, p, dil).  The views (ldi, cioff, ldo, cooff, ldm, moff) are laid out here: every offset != 0
    and a multiple of 8 (fp32, the forward output of an m4 row and the mask view of a mask4 row: of 4 only), every stride wider than its view,
    ldm != ldi, moff != cioff"""
    nb, cin, h, w, cout, k, s, p, dil = shape
    fp32 = dtype == "fp32"
    epc = 4 if fp32 else 8
    cioff = 4 if fp32 else 8
    cooff = 4 if (fp32 or (m4 and which == 0)) else 8
    ldi = cioff + _pad(cin, epc) + epc
    ldo = cooff + _pad(cout, epc) + 8
    views = (ldi, cioff, ldo, cooff, ldi + 16, cioff + epc)
    if extra.get("mask4"):                                    # bf16: a mask view at multiples of 4 only (the fast and halo kernels take it)
        views = (ldi, cioff, ldo, cooff, ldi + 12, cioff + 4)
    if extra.get("u8"):
        views = (8, 0, ldo, cooff, 0, 0)
    return dict(label=label, name=name, which=which, flags=flags, dtype=dtype, shape=shape, views=views, opts=opts or {}, **extra)


def _fast(t, *a):
    return f"conv_gather_fast_kernel<{t},{','.join(str(x) for x in a)}>"


K1, K3, K7, K17, K71 = (1, 1), (3, 3), (7, 7), (1, 7), (7, 1)
S1, S2, P0, P1 = (1, 1), (2, 2), (0, 0), (1, 1)
REGW, REGW_SHORT, STREAM = {"DIN_CONV_REGW": "2"}, {"DIN_CONV_REGW": "2", "DIN_CONV_REGW_SHORT": "2"}, {"DIN_CONV_STREAM": "2"}
FWD, DG = 0, 1
CONV_ROWS = [
    # ---- conv1x1_regw_kernel<NKS, MASKED, NS, OCC, RT> (filters resident in registers), forced on small maps.  Reductions that end in a
    # partial 64-channel stage, classes of 128 / 192 filters with a short last class, ragged last pixel tile.  A 20 / 24-step launch has
    # >= 8 k-steps: 192 tiles keep the planner from splitting it
    _row("regw6_fwd", "conv1x1_regw_kernel<6,0,4,2,2>", FWD, 0, "bf16", (2, 136, 19, 23, 136, K1, S1, P0, 1), REGW_SHORT),
    _row("regw8_dg", "conv1x1_regw_kernel<8,0,4,2,2>", DG, 0, "bf16", (2, 136, 19, 23, 208, K1, S1, P0, 1), REGW_SHORT),
    _row("regw8_dg_mask", "conv1x1_regw_kernel<8,1,4,2,2>", DG, MASK, "bf16", (2, 152, 17, 23, 200, K1, S1, P0, 1), REGW_SHORT),
    _row("regw10_fwd", "conv1x1_regw_kernel<10,0,4,2,2>", FWD, 0, "bf16", (2, 280, 19, 23, 264, K1, S1, P0, 1), REGW_SHORT),
    _row("regw20_dg", "conv1x1_regw_kernel<20,0,9,1,3>", DG, 0, "bf16", (3, 200, 67, 61, 616, K1, S1, P0, 1), REGW),
    _row("regw20_dg_mask", "conv1x1_regw_kernel<20,1,9,1,3>", DG, MASK, "bf16", (3, 200, 61, 67, 632, K1, S1, P0, 1), REGW),
    _row("regw24_fwd", "conv1x1_regw_kernel<24,0,9,1,3>", FWD, 0, "bf16", (3, 712, 67, 61, 200, K1, S1, P0, 1), REGW),
    _row("regw24_dg_mask", "conv1x1_regw_kernel<24,1,9,1,3>", DG, MASK, "bf16", (3, 200, 67, 61, 744, K1, S1, P0, 1), REGW),
    # ---- conv1x1_stream_kernel<BN, NSW, MULTI, EPI, SPLIT> (persistent streaming 1x1), forced on small maps: one full + one partial
    # 64-channel block, filters short of the tile; EPI (mask / accumulate operands) in all three flag forms
    _row("stream64_fwd", "conv1x1_stream_kernel<64,4,0,0,0>", FWD, 0, "bf16", (2, 72, 19, 23, 40, K1, S1, P0, 1), STREAM),
    _row("stream96_fwd", "conv1x1_stream_kernel<96,4,0,0,0>", FWD, 0, "bf16", (2, 72, 19, 23, 80, K1, S1, P0, 1), STREAM),
    _row("stream192_fwd", "conv1x1_stream_kernel<192,3,0,0,0>", FWD, 0, "bf16", (2, 72, 19, 23, 136, K1, S1, P0, 1), STREAM),
    _row("stream64_dg_mask", "conv1x1_stream_kernel<64,4,0,1,0>", DG, MASK, "bf16", (2, 40, 19, 23, 72, K1, S1, P0, 1), STREAM),
    _row("stream64_dg_accum", "conv1x1_stream_kernel<64,4,0,1,0>", DG, ACCUM, "bf16", (2, 56, 17, 23, 88, K1, S1, P0, 1), STREAM, twice=True),
    _row("stream64_dg_mask_accum", "conv1x1_stream_kernel<64,4,0,1,0>", DG, MASK | ACCUM, "bf16", (2, 48, 19, 21, 136, K1, S1, P0, 1), STREAM, twice=True),
    _row("stream96_dg_mask", "conv1x1_stream_kernel<96,4,0,1,0>", DG, MASK, "bf16", (2, 80, 19, 23, 72, K1, S1, P0, 1), STREAM),
    _row("stream192_dg_accum", "conv1x1_stream_kernel<192,3,0,1,0>", DG, ACCUM, "bf16", (2, 136, 19, 23, 72, K1, S1, P0, 1), STREAM, twice=True),
    # ---- conv_gather_fast_kernel<T, BM, BN, WM, WN, KCS, NS, MULTI, FASTK, XSRC, LANEK>, bf16.  Multi-tap rows with >= 8 k-steps sit on
    # 2 x 111 x 113 pixels: 196 tiles, the fewest at which the planner does not split the reduction (split-K has its own rows)
    _row("t128_plain_dg_mask", _fast("bf16", 128, 128, 4, 2, 8, 2, 0, 0, 0, 0), DG, MASK, "bf16", (2, 120, 111, 113, 72, K3, S1, P1, 1)),
    _row("t128_fastk_fwd", _fast("bf16", 128, 128, 4, 2, 8, 2, 0, 1, 0, 0), FWD, 0, "bf16", (2, 64, 19, 23, 120, K17, S1, (0, 3), 1)),
    _row("t128_lanek_fwd", _fast("bf16", 128, 128, 4, 2, 8, 2, 0, 1, 0, 1), FWD, 0, "bf16", (2, 72, 111, 113, 120, K3, S1, P1, 1)),
    _row("t160_plain_dg_accum", _fast("bf16", 128, 160, 4, 2, 8, 2, 0, 0, 0, 0), DG, ACCUM, "bf16", (2, 152, 19, 23, 40, K17, S1, (0, 3), 1), twice=True),
    _row("t160_fastk_fwd", _fast("bf16", 128, 160, 4, 2, 8, 2, 0, 1, 0, 0), FWD, 0, "bf16", (2, 64, 23, 19, 152, K71, S1, (3, 0), 1)),
    _row("t160_lanek_fwd", _fast("bf16", 128, 160, 4, 2, 8, 2, 0, 1, 0, 1), FWD, 0, "bf16", (2, 72, 111, 113, 152, K3, S1, P1, 1), m4=True),
    _row("t192_plain_dg_mask", _fast("bf16", 128, 192, 4, 2, 8, 2, 0, 0, 0, 0), DG, MASK, "bf16", (2, 184, 111, 113, 72, K3, S1, P1, 1)),
    _row("t192_fastk_dg", _fast("bf16", 128, 192, 4, 2, 8, 2, 0, 1, 0, 0), DG, 0, "bf16", (2, 184, 113, 115, 64, K3, S1, P0, 1)),
    _row("t192_lanek_fwd_p0", _fast("bf16", 128, 192, 4, 2, 8, 2, 0, 1, 0, 1), FWD, 0, "bf16", (2, 80, 113, 115, 184, K3, S1, P0, 1)),
    _row("t64_plain_dg_mask_accum", _fast("bf16", 128, 64, 4, 2, 8, 2, 0, 0, 0, 0), DG, MASK | ACCUM, "bf16", (2, 40, 111, 113, 72, K3, S1, P1, 1), twice=True),
    _row("t64_fastk_fwd", _fast("bf16", 128, 64, 4, 2, 8, 2, 0, 1, 0, 0), FWD, 0, "bf16", (2, 64, 111, 113, 40, K3, S1, P1, 1)),
    _row("t64_lanek_dg", _fast("bf16", 128, 64, 4, 2, 8, 2, 0, 1, 0, 1), DG, 0, "bf16", (2, 48, 111, 113, 72, K3, S1, P1, 1)),
    _row("t96_w4_fwd_s2", _fast("bf16", 128, 96, 2, 2, 8, 2, 0, 0, 0, 0), FWD, 0, "bf16", (2, 40, 39, 47, 88, K3, S2, P0, 1), m4=True),
    _row("t96_w8_dg_s2_parity", _fast("bf16", 128, 96, 4, 2, 8, 2, 0, 0, 0, 0), DG, ACCUM, "bf16", (2, 88, 39, 47, 40, K3, S2, P1, 1), twice=True),
    _row("t256x256_fwd", _fast("bf16", 256, 256, 4, 2, 8, 2, 0, 0, 0, 0), FWD, 0, "bf16", (2, 168, 313, 315, 232, K3, S1, P1, 1)),
    # ---- the un-staged epilogue (epilogue_direct) of the bf16 tiles: produced channels that are no multiple of 8 (tail pairs and single
    # stores), forward and, with cin % 8 != 0, the dgrad under its scalar MASK / ACCUM code; an aligned dgrad that a mask view at multiples
    # of 4 alone sends there.  It adds the old value in fp32: the plain bar.  (Fewer than 8 k-steps: a split launch would leave MASK / ACCUM
    # to the finish kernel)
    _row("t96_direct_fwd_c83", _fast("bf16", 128, 96, 2, 2, 8, 2, 0, 0, 0, 0), FWD, 0, "bf16", (2, 64, 19, 23, 83, K17, S1, (0, 3), 1), m4=True),
    _row("t64_direct_dg_c43_mask_accum", _fast("bf16", 128, 64, 4, 2, 8, 2, 0, 0, 0, 0), DG, MASK | ACCUM, "bf16", (2, 43, 19, 23, 40, K17, S1, (0, 3), 1), mask4=True),
    _row("t64_direct_dg_c13_accum", _fast("bf16", 128, 64, 4, 2, 8, 2, 0, 0, 0, 0), DG, ACCUM, "bf16", (2, 13, 19, 23, 40, K17, S1, (0, 3), 1)),
    _row("t128_direct_dg_mask4", _fast("bf16", 128, 128, 4, 2, 8, 2, 0, 0, 0, 0), DG, MASK, "bf16", (2, 120, 19, 23, 40, K17, S1, (0, 3), 1), mask4=True),
    # ---- fp32: four-wave tiles, channel counts that are no multiple of 4 on both sides (with their dgrads), offsets at multiples of 4
    _row("f128_fwd", _fast("float", 128, 128, 2, 2, 8, 2, 0, 0, 0, 0), FWD, 0, "fp32", (2, 13, 19, 23, 118, K3, S1, P1, 1)),
    _row("f160_dg_accum", _fast("float", 128, 160, 2, 2, 8, 2, 0, 0, 0, 0), DG, ACCUM, "fp32", (2, 150, 19, 23, 38, K17, S1, (0, 3), 1)),
    _row("f192_fwd", _fast("float", 128, 192, 2, 2, 8, 2, 0, 0, 0, 0), FWD, 0, "fp32", (2, 22, 23, 19, 182, K71, S1, (3, 0), 1)),
    _row("f64_dg_mask", _fast("float", 128, 64, 2, 2, 8, 2, 0, 0, 0, 0), DG, MASK, "fp32", (2, 13, 19, 23, 22, K3, S1, P1, 1)),
    _row("f96_fwd_s2", _fast("float", 128, 96, 2, 2, 8, 2, 0, 0, 0, 0), FWD, 0, "fp32", (2, 18, 39, 47, 86, K3, S2, P1, 1)),
    # produced channels at multiples of 4: the LDS-staged epilogue in fp32, plain stores and the batched MASK / ACCUM form (one rounding)
    _row("f128_staged_fwd", _fast("float", 128, 128, 2, 2, 8, 2, 0, 0, 0, 0), FWD, 0, "fp32", (2, 13, 19, 23, 116, K3, S1, P1, 1)),
    _row("f64_staged_dg_mask", _fast("float", 128, 64, 2, 2, 8, 2, 0, 0, 0, 0), DG, MASK, "fp32", (2, 12, 19, 23, 22, K3, S1, P1, 1)),
    _row("f160_staged_dg_mask_accum", _fast("float", 128, 160, 2, 2, 8, 2, 0, 0, 0, 0), DG, MASK | ACCUM, "fp32", (2, 148, 19, 23, 22, K17, S1, (0, 3), 1)),
    _row("f256x64_fwd_p0", _fast("float", 256, 64, 4, 1, 4, 4, 0, 0, 0, 0), FWD, 0, "fp32", (2, 6, 365, 367, 27, K3, S1, P0, 1)),
    # ---- conv_gather_generic_kernel<T, BN>: more than 32 taps (7x7 forward), strided dgrad with dilation 2 (no parity classes)
    _row("gen_f64_fwd_7x7", "conv_gather_generic_kernel<float,64>", FWD, 0, "fp32", (2, 5, 19, 23, 27, K7, S1, (3, 3), 1)),
    _row("gen_f128_dg_s2_d2", "conv_gather_generic_kernel<float,128>", DG, 0, "fp32", (2, 70, 39, 47, 10, K3, S2, (2, 2), 2)),
    _row("gen_b64_dg_s2_d2", "conv_gather_generic_kernel<bf16,64>", DG, ACCUM, "bf16", (2, 40, 39, 47, 24, K3, S2, (2, 2), 2)),
    _row("gen_b128_fwd_7x7", "conv_gather_generic_kernel<bf16,128>", FWD, 0, "bf16", (2, 16, 19, 23, 72, K7, S1, (3, 3), 1)),
    # ---- conv_splitk_finish_kernel<T>: 13 k-steps in 5 splits of 3 (the last split holds one)
    _row("splitk_b_fwd", "conv_splitk_finish_kernel<bf16>", FWD, 0, "bf16", (2, 88, 21, 25, 184, K3, S1, P0, 1)),
    _row("splitk_f_fwd", "conv_splitk_finish_kernel<float>", FWD, 0, "fp32", (2, 42, 21, 25, 182, K3, S1, P1, 1)),
    _row("splitk_b_dg_mask_accum", "conv_splitk_finish_kernel<bf16>", DG, MASK | ACCUM, "bf16", (2, 184, 21, 25, 88, K3, S1, P1, 1)),
    # ---- conv_halo_kernel<BN, 3, 3, 8, 32, 2, 16> (>= 64 Ki pixels): 8 x 32-pixel tiles ragged on both axes, one + a partial 64-channel block
    _row("halo64_dg_mask_accum", "conv_halo_kernel<64,3,3,8,32,2,16>", DG, MASK | ACCUM, "bf16", (2, 56, 183, 181, 72, K3, S1, P1, 1)),
    _row("halo64_dg_mask4", "conv_halo_kernel<64,3,3,8,32,2,16>", DG, MASK, "bf16", (2, 56, 183, 181, 72, K3, S1, P1, 1), mask4=True),
    _row("halo80_fwd_p0", "conv_halo_kernel<80,3,3,8,32,2,16>", FWD, 0, "bf16", (2, 40, 185, 183, 80, K3, S1, P0, 1)),
    _row("halo96_fwd", "conv_halo_kernel<96,3,3,8,32,2,16>", FWD, 0, "bf16", (2, 72, 183, 181, 88, K3, S1, P1, 1), m4=True),
    # ---- conv_small_kernel<CPT, BN, NBUF, 3, 3, ST, U8, NW, EPI> (>= 256 Ki pixels): the image layer (prepared tensor, raw uint8 frames),
    # 32 -> <= 32, 32 -> <= 64, and the dgrads from 32 / 64 channels, plain and with the early operand request (EPI) in its three flag forms
    _row("small_image", "conv_small_kernel<1,32,2,3,3,2,0,4,0>", FWD, 0, "bf16", (2, 5, 727, 729, 24, K3, S2, P1, 1)),
    _row("small_image_u8", "conv_small_kernel<1,32,2,3,3,2,1,4,0>", FWD, 0, "bf16", (2, 3, 727, 729, 24, K3, S2, P0, 1), u8=True),
    _row("small4_32_fwd_p0", "conv_small_kernel<4,32,2,3,3,1,0,4,0>", FWD, 0, "bf16", (2, 32, 365, 367, 24, K3, S1, P0, 1)),
    _row("small4_32_dg_mask", "conv_small_kernel<4,32,2,3,3,1,0,4,1>", DG, MASK, "bf16", (2, 24, 363, 365, 32, K3, S1, P1, 1)),
    _row("small4_32_dg_accum", "conv_small_kernel<4,32,2,3,3,1,0,4,1>", DG, ACCUM, "bf16", (2, 16, 363, 365, 32, K3, S1, P0, 1), twice=True),
    _row("small4_32_dg_mask_accum", "conv_small_kernel<4,32,2,3,3,1,0,4,1>", DG, MASK | ACCUM, "bf16", (2, 32, 363, 365, 32, K3, S1, P1, 1), twice=True),
    _row("small4_64_fwd", "conv_small_kernel<4,64,2,3,3,1,0,8,0>", FWD, 0, "bf16", (2, 32, 363, 365, 56, K3, S1, P1, 1)),
    _row("small8_32_dg", "conv_small_kernel<8,32,1,3,3,1,0,8,0>", DG, 0, "bf16", (2, 24, 363, 365, 64, K3, S1, P1, 1)),
    _row("small8_32_dg_mask", "conv_small_kernel<8,32,1,3,3,1,0,8,1>", DG, MASK, "bf16", (2, 32, 363, 365, 64, K3, S1, P0, 1)),
    _row("small8_32_dg_accum", "conv_small_kernel<8,32,1,3,3,1,0,8,1>", DG, ACCUM, "bf16", (2, 16, 363, 365, 64, K3, S1, P1, 1), twice=True),
    _row("small8_32_dg_mask_accum", "conv_small_kernel<8,32,1,3,3,1,0,8,1>", DG, MASK | ACCUM, "bf16", (2, 24, 363, 365, 64, K3, S1, P1, 1), twice=True),
]
IDS = [r["label"] for r in CONV_ROWS]


# ---- the float64 reference ----------------------------------------------------------------------------------------------------------------
def _geometry(shape):
    nb, cin, h, w, cout, k, s, p, dil = shape
    oh = (h + 2 * p[0] - dil * (k[0] - 1) - 1) // s[0] + 1
    ow = (w + 2 * p[1] - dil * (k[1] - 1) - 1) // s[1] + 1
    return nb, cin, h, w, cout, k, s, p, dil, oh, ow


def _taps(k, s, dil, oh, ow):
    """THE tap indexing, once: output pixel (oy, ox) meets tap (r, t) at row oy * sh + r * dh, column ox * sw + t * dw of the input padded
    by (ph, pw).  Yields (r, t, rows, columns) as slices of the padded map; the forward gathers through them, the dgrad scatters."""
    for r in range(k[0]):
        for t in range(k[1]):
            yield (r, t, slice(r * dil, r * dil + s[0] * (oh - 1) + 1, s[0]), slice(t * dil, t * dil + s[1] * (ow - 1) + 1, s[1]))


def conv_reference(x, w, k, s, p, dil, oh, ow):
    """x [nb][h][w][cin], w [cout][cin][kh][kw], float64 -> (v, S, last) [M][cout]: the convolution, the same sum over absolute values,
    and the share of v that the last 8 reduction channels of the last tap contribute"""
    nb, cin, M = x.shape[0], x.shape[3], x.shape[0] * oh * ow
    xp = torch.nn.functional.pad(x, (0, 0, p[1], p[1], p[0], p[0]))
    v = torch.zeros(M, w.shape[0], dtype=torch.float64, device=x.device)
    S = torch.zeros_like(v)
    for r, t, ys, xs in _taps(k, s, dil, oh, ow):
        a, b = xp[:, ys, xs, :].reshape(M, cin), w[:, :, r, t].t()
        v += a @ b
        S += a.abs() @ b.abs()
    return v, S, a[:, -8:] @ b[-8:]


def dgrad_reference(g, w, k, s, p, dil, h, wd):
    """g [nb][oh][ow][cout], w [cout][cin][kh][kw], float64 -> (v, S, last) [nb][h][w][cin]: the transposed sum over the same taps"""
    nb, oh, ow, cout = g.shape
    cin = w.shape[1]
    size = (nb, h + 2 * p[0], wd + 2 * p[1], cin)
    v, S, last = (torch.zeros(size, dtype=torch.float64, device=g.device) for _ in range(3))
    g2 = g.reshape(-1, cout)
    for r, t, ys, xs in _taps(k, s, dil, oh, ow):
        b = w[:, :, r, t]
        v[:, ys, xs, :] += (g2 @ b).reshape(nb, oh, ow, cin)
        S[:, ys, xs, :] += (g2.abs() @ b.abs()).reshape(nb, oh, ow, cin)
    last[:, ys, xs, :] = (g2[:, -8:] @ b[-8:]).reshape(nb, oh, ow, cin)
    crop = (slice(None), slice(p[0], p[0] + h), slice(p[1], p[1] + wd))
    return v[crop], S[crop], last[crop]


def _terms(row, splitk):
    nb, cin, h, w, cout, k, s, p, dil, oh, ow = _geometry(row["shape"])
    K = k[0] * k[1] * (cin if row["which"] == 0 else cout) + 2
    return K + splitk


def bar_of(row, v, S, splitk, staged=None):
    """the per-element bar of a row for a result v whose absolute-value sum is S.  staged: the (masked) gradient g before the accumulate
    of a row marked twice=True.  Three bf16 kernels stage their output tile in LDS AS bf16 so that it leaves as 16-byte chunks of whole
    pixel rows, and add the old value to that staged element: staged_tile_store of conv_gather_fast_kernel (csrc/conv_gather.h), the last
    block of conv1x1_stream_kernel (csrc/conv_stream.hip) and the store loop of conv_small_kernel (csrc/conv_small.hip), EPI or not.  Two
    roundings by design: g' = bf16(g) with |g' - g| <= 2^-8 |g| (half an ulp of 8 significand bits), then bf16(g' + old) with an error of
    at most 2^-8 |g' + old| <= 2^-8 (|v| + 2^-8 |g|).  The second is the store the plain bar already holds; the first adds
    2^-8 (1 + 2^-8) |g|, and with the suite's factor 2 those rows' bar grows by 2^-7 (1 + 2^-8) |g|.  (conv_halo_kernel, the split-K finish
    and the generic kernel add in fp32 and keep the plain bar.)  The bite test holds every row's data to the plain bar as well"""
    b = 2.0 * (_terms(row, splitk) + 2) * 2.0 ** -24 * S
    if row["dtype"] == "fp32":
        return b
    return b + 2.0 ** -7 * v.abs() + (2.0 ** -7 * (1 + 2.0 ** -8) * staged.abs() if staged is not None and row.get("twice") else 0.0)


_CACHE = {}


def _mask_tensor(shape, tdt, gen):
    """a mask operand (storage dtype) holding +0.0, -0.0, the smallest positive bf16 subnormal and negative values at known positions, and
    where it lets the gradient through (value > 0)"""
    m = torch.randn(*shape, generator=gen)
    flat = m.view(-1)
    special = torch.tensor([0.0, -0.0, SUBNORMAL, -1.0, -SUBNORMAL, 0.0, -0.0, SUBNORMAL])
    pos = (torch.arange(64) * 7919) % flat.numel()                       # the known positions: 64 spread over the tensor, the first at 0
    flat[pos] = special.repeat(8)
    m = m.to(tdt)
    on = m.double() > 0
    assert bool(on.view(-1)[pos[2]]) and not bool(on.view(-1)[pos[1]])   # the subnormal passes the mask, -0.0 does not
    return m, on


def _operands(row, device="cpu"):
    """stored operands (host, storage dtype) and the float64 reference of a row, shared by its modes and launches"""
    key = (row["label"], device)
    if key in _CACHE:
        return _CACHE[key]
    _CACHE.clear()
    nb, cin, h, w, cout, k, s, p, dil, oh, ow = _geometry(row["shape"])
    tdt = torch.float32 if row["dtype"] == "fp32" else torch.bfloat16
    gen = torch.Generator().manual_seed(sum(map(ord, row["label"])))
    op = dict(tdt=tdt, img=None)
    if row.get("u8"):
        op["img"] = torch.randint(0, 256, (nb, cin, h, w), dtype=torch.uint8, generator=gen)
        x = O.prep_images(op["img"].float()).permute(0, 2, 3, 1).contiguous().to(tdt)
    else:
        x = torch.randn(nb, h, w, cin, generator=gen).to(tdt)
    wt = (torch.randn(cout, cin, *k, generator=gen) * (2.0 / (cin * k[0] * k[1])) ** 0.5).to(tdt)
    op.update(x=x, w=wt, bias=torch.randn(cout, generator=gen) * 0.1)
    w64 = wt.double().to(device)
    if row["which"] == 0:
        v, S, last = conv_reference(x.double().to(device), w64, k, s, p, dil, oh, ow)
        op.update(v=v.cpu(), S=S.cpu(), last=last.cpu())
    else:
        g = torch.randn(nb, oh, ow, cout, generator=gen).to(tdt)
        v, S, last = dgrad_reference(g.double().to(device), w64, k, s, p, dil, h, w)
        v, S, last = v.cpu(), S.cpu(), last.cpu()
        m, on = _mask_tensor((nb, h, w, cin), tdt, gen)
        old = (torch.randn(nb, h, w, cin, generator=gen) * float(v.std())).to(tdt)
        op.update(g=g, mask=m, on=on, old=old, v=v, S=S, last=last)
    _CACHE[key] = op
    return op


def _expect(row, op, flags):
    """(v, S, exact) of one mode: exact = the elements that must equal 0 / the old value bit for bit (None: none)"""
    v, S = op["v"], op["S"]
    if row["which"] == 0:
        if flags & BIAS:
            v, S = v + op["bias"].double(), S + op["bias"].double().abs()
        return (v.clamp_min(0) if flags & RELU else v), S, None
    exact = None
    if flags & MASK:
        exact = ~op["on"]
        v, S = v * op["on"], S * op["on"]
    if flags & ACCUM:
        v, S = v + op["old"].double(), S + op["old"].double().abs()
    return v, S, exact


# ---- descriptor, names ---------------------------------------------------------------------------------------------------------------
def _desc(L, row):
    nb, cin, h, w, cout, k, s, p, dil, oh, ow = _geometry(row["shape"])
    d = L.ConvDesc()
    d.nb, d.h, d.w, d.cin, d.oh, d.ow, d.cout = nb, h, w, cin, oh, ow, cout
    d.kh, d.kw, d.sh, d.sw, d.ph, d.pw, d.dh, d.dw = k[0], k[1], s[0], s[1], p[0], p[1], dil, dil
    d.ldi, d.cioff, d.ldo, d.cooff = row["views"][:4]
    d.dtype, d.in_u8 = (L.DIN_F32 if row["dtype"] == "fp32" else L.DIN_BF16), int(bool(row.get("u8")))
    return d


def _names(lib, d, which, flags, ldm, moff):
    buf = C.create_string_buffer(4096)
    rc = lib.din_conv_kernel_names(C.byref(d), which, flags, ldm, moff, buf, len(buf))
    assert 0 < rc <= len(buf), f"din_conv_kernel_names returned {rc}"
    return buf.value.decode().split()


def _split_depth(lib, d, row, names):
    """how many ways the launch splits its reduction (0: not at all), from what the library itself reports: the workspace holds
    [splits][pixels][filter tiles x BN] fp32 partial sums, BN being the filter tile of the kernel the reporter names before the finish"""
    if not any(n.startswith("conv_splitk_finish_kernel") for n in names):
        return 0
    assert len(names) == 2, f"{row['label']}: one split launch and its finish expected, not {names}"
    nb, cin, h, w, cout, k, s, p, dil, oh, ow = _geometry(row["shape"])
    M, c = (nb * oh * ow, cout) if row["which"] == 0 else (nb * h * w, cin)
    args = names[0][names[0].index("<") + 1:-1].split(",")
    bn = int(args[2] if names[0].startswith("conv_gather_fast_kernel") else args[1])
    per_split = M * _pad(c, bn) * 4
    wsb = lib.din_conv_workspace_bytes(C.byref(d), row["which"])
    assert wsb > per_split and wsb % per_split == 0, f"{row['label']}: workspace {wsb} is no multiple of {per_split} ({names[0]})"
    return wsb // per_split


def _assert_named(lib, L, row, monkeypatch):
    """the row's options are set (and stay set for the caller); every mode of the row launches the kernel the row names.  Returns the
    descriptor and the split depth of the row's reduction (a term of its bar)"""
    for name, value in row["opts"].items():
        monkeypatch.setenv(name, value)
    d = _desc(L, row)
    ldm, moff = row["views"][4:]
    splitk = None
    for flags in _modes(row):
        got = _names(lib, d, row["which"], flags, ldm if flags & MASK else 0, moff if flags & MASK else 0)
        assert row["name"] in got, f"{row['label']}: flags {flags} launch {got}, not {row['name']}"
        depth = _split_depth(lib, d, row, got)
        splitk = depth if splitk is None else splitk
        assert depth == splitk, f"{row['label']}: the modes split {splitk} and {depth} ways"
    return d, splitk


def _modes(row):
    return (BIAS | RELU, 0) if row["which"] == 0 else (row["flags"],)


def _library():
    from din_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("libdin_hip.so is not built: run __graft_entry__.build()")
    return L.load(), L


# ---- CPU tests ----------------------------------------------------------------------------------------------------------------------------
def test_rows_resolve_to_their_kernels_and_cover_the_required_names(monkeypatch):
    lib, L = _library()
    for row in CONV_ROWS:
        _assert_named(lib, L, row, monkeypatch)
        for name in row["opts"]:
            L.set_option(name, None)
    with open(NAMES_FILE) as fh:
        required = {line.split()[0] for line in fh if line.strip()} | EXTRA_REQUIRED
    assert len(required) >= 40
    missing = required - {r["name"] for r in CONV_ROWS}
    assert not missing, f"kernels without a row: {sorted(missing)}"
    for flagset, family in ((MASK, "conv_small_kernel"), (ACCUM, "conv_small_kernel"), (MASK | ACCUM, "conv_small_kernel"),
                            (MASK, "conv1x1_stream"), (ACCUM, "conv1x1_stream"), (MASK | ACCUM, "conv1x1_stream"), (MASK, "conv1x1_regw")):
        assert any(r["which"] == 1 and r["flags"] == flagset and r["name"].startswith(family) for r in CONV_ROWS), (flagset, family)


def test_dgrad_reference_indexing_matches_conv2d_input():
    """the per-tap indexing of _taps, as the dgrad scatters through it, against torch.nn.grad.conv2d_input in float64 (strided, dilated,
    padded, sizes that leave unread border rows); and as the forward gathers through it, against conv2d"""
    gen = torch.Generator().manual_seed(5)
    nb, cin, h, w, cout, k, s, p, dil, oh, ow = _geometry((2, 5, 14, 17, 6, (3, 2), (2, 3), (2, 1), 2))
    x = torch.randn(nb, h, w, cin, generator=gen, dtype=torch.float64)
    wt = torch.randn(cout, cin, *k, generator=gen, dtype=torch.float64)
    g = torch.randn(nb, oh, ow, cout, generator=gen, dtype=torch.float64)
    want = torch.nn.grad.conv2d_input((nb, cin, h, w), wt, g.permute(0, 3, 1, 2), stride=s, padding=p, dilation=dil).permute(0, 2, 3, 1)
    v, S, _ = dgrad_reference(g, wt, k, s, p, dil, h, w)
    assert float((v - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert bool((S >= v.abs() - 1e-12).all())
    y = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), wt, stride=s, padding=p, dilation=dil).permute(0, 2, 3, 1).reshape(-1, cout)
    v, S, _ = conv_reference(x, wt, k, s, p, dil, oh, ow)
    assert float((v - y).abs().max()) <= 1e-12 * float(y.abs().max())


@pytest.mark.parametrize("row", CONV_ROWS, ids=IDS)
def test_bars_bite(row, monkeypatch):
    """the row's bar on the row's data: a kernel that lost the last 8 reduction channels of the last tap moves >= 10 % of the produced
    elements beyond it; under ACCUM, one that rounded the gradient to bf16 before adding the old value moves at least one"""
    lib, L = _library()
    _, splitk = _assert_named(lib, L, row, monkeypatch)
    op = _operands(row)
    flags = 0 if row["which"] == 0 else row["flags"]
    v, S, _ = _expect(row, op, flags)
    bar = bar_of(row, v, S, splitk)
    lost = op["last"] * op["on"] if flags & MASK else op["last"]
    share = float((lost.abs() > bar).double().mean())
    assert share >= 0.10, f"{row['label']}: dropping 8 channels of the last tap moves only {share:.3f} of the elements beyond the bar"
    if flags & ACCUM:
        conv = v - op["old"].double()
        if row.get("twice"):                                      # the bar the GPU test holds a twice-rounding row to bites as well
            share = float((lost.abs() > bar_of(row, v, S, splitk, conv)).double().mean())
            assert share >= 0.10, f"{row['label']}: dropping 8 channels moves only {share:.3f} of the elements beyond the widened bar"
        twice = (conv.bfloat16().double() + op["old"].double()).to(op["tdt"]).double()
        n = int(((twice - v).abs() > bar).sum())
        assert n >= 1, f"{row['label']}: a second bf16 rounding before the accumulate passes the bar everywhere"


# ---- the GPU test ---------------------------------------------------------------------------------------------------------------------
def _view(t, dtype, ld, off, cpad):
    """[..][c] host tensor -> device NHWC view: channels [off, off + c) hold t, [off + c, off + cpad) zeros (the chunk padding the kernels
    may read), every other channel of the pixel stride POISON"""
    *lead, c = t.shape
    buf = torch.full((*lead, ld), POISON, dtype=dtype)
    buf[..., off:off + cpad] = 0
    buf[..., off:off + c] = t.to(dtype)
    return buf.cuda()


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _guarded(lead, ld, tdt, gen):
    """an output tensor [*lead][ld] between two guard bands of NG elements, and the random pattern its launches start from"""
    n = lead[0] * lead[1] * lead[2] * ld
    buf = torch.empty(n + 2 * NG, dtype=tdt, device="cuda")
    pattern = torch.randn(n + 2 * NG, generator=gen).to(tdt).cuda()          # outside the produced range, and the guards
    return dict(buf=buf, out=buf[NG:NG + n].view(*lead, ld), pattern=pattern, n=n, lead=lead, ld=ld)


def _guarded_workspace(wsb):
    """(buffer, workspace): wsb bytes between two guard bands of WS_GUARD bytes holding 0x5a"""
    wsbuf = torch.empty(wsb + 2 * WS_GUARD, dtype=torch.uint8, device="cuda")
    wsbuf.fill_(0x5a)
    return wsbuf, wsbuf[WS_GUARD:WS_GUARD + wsb]


def _launch_twice_and_compare(what, launch, wsbuf, wsb, dests):
    """THE guard / launch / compare loop of one mode.  dests: the launch's destinations, each a _guarded() dict with off, c (the produced
    channel range), v, bar ([*lead][c], float64), exact (elements that must equal 0 / the old value bit for bit, or None) and old (the
    host tensor an ACCUM launch adds to, or None: the range starts as NaN).  launch() runs twice from the same prefill; after each run
    everything outside the produced ranges and both guard bands -- the workspace's too -- is bit-identical to the prefill, no NaN is left
    inside, the exact elements hold the bits of +0.0 / of the old value (a -0.0 written there fails) and max(err / bar) <= 1 as a Measured.  Returns the two ratios."""
    ws = wsbuf[WS_GUARD:WS_GUARD + wsb]
    for t in dests:
        n, lead, ld, off, c = t["n"], t["lead"], t["ld"], t["off"], t["c"]
        t["pre"] = t["pattern"].clone()
        inside = t["pre"][NG:NG + n].view(*lead, ld)[..., off:off + c]
        inside.copy_(t["old"].cuda()) if t["old"] is not None else inside.fill_(float("nan"))
        t["outside"] = t["pre"].clone()
        t["outside"][NG:NG + n].view(*lead, ld)[..., off:off + c] = 0
    ratios = []
    for run in range(2):
        ws.fill_(0x7f)
        for t in dests:
            t["buf"].copy_(t["pre"])
        launch()
        torch.cuda.synchronize()
        worst = 0.0
        for t in dests:
            n, lead, ld, off, c = t["n"], t["lead"], t["ld"], t["off"], t["c"]
            got = t["out"][..., off:off + c].clone()
            rest = t["buf"].clone()
            rest[NG:NG + n].view(*lead, ld)[..., off:off + c] = 0
            assert torch.equal(_bits(rest), _bits(t["outside"])), f"{what}: wrote outside the produced channel range"
            assert bool((wsbuf[:WS_GUARD] == 0x5a).all()) and bool((wsbuf[WS_GUARD + wsb:] == 0x5a).all()), f"{what}: wrote outside the workspace"
            assert not bool(got.isnan().any()), f"{what}: produced elements left unwritten"
            got = got.cpu()
            if t["exact"] is not None:
                want = t["old"] if t["old"] is not None else torch.zeros_like(got)
                assert torch.equal(_bits(got[t["exact"]]), _bits(want[t["exact"]])), \
                    f"{what}: masked-off elements are not bit for bit {'the old value' if t['old'] is not None else '+0.0'}"
            worst = max(worst, float(((got.double() - t["v"]).abs() / t["bar"]).max()))
        ratio = Measured(worst)
        print(f"{what} launch={run} max(err/bar)={float(ratio):.4f}")
        assert ratio <= 1.0
        ratios.append(float(ratio))
    return ratios


@pytest.mark.gpu
@pytest.mark.parametrize("row", CONV_ROWS, ids=IDS)
def test_conv_kernel_against_fp64(env, row, monkeypatch):
    lib, L, nhwc, ops = env
    d, splitk = _assert_named(lib, L, row, monkeypatch)
    nb, cin, h, w, cout, k, s, p, dil, oh, ow = _geometry(row["shape"])
    ldi, cioff, ldo, cooff, ldm, moff = row["views"]
    which, fp32 = row["which"], row["dtype"] == "fp32"
    epc = 4 if fp32 else 8
    op = _operands(row, "cuda")
    tdt = op["tdt"]
    gen = torch.Generator().manual_seed(11)

    wdev = op["w"].float().cuda()
    wpk = torch.empty(lib.din_conv_packed_elems(C.byref(d), which), dtype=tdt, device="cuda")
    L.check(lib.din_conv_pack_weights(C.byref(d), wdev.data_ptr(), None, wpk.data_ptr(), which, None))
    if which == 0:
        src = op["img"].cuda() if row.get("u8") else _view(op["x"], tdt, ldi, cioff, _pad(cin, epc))
        lead, ld, off, c = (nb, oh, ow), ldo, cooff, cout
        bias = op["bias"].cuda()
    else:
        src = _view(op["g"], tdt, ldo, cooff, _pad(cout, epc))
        lead, ld, off, c = (nb, h, w), ldi, cioff, cin
        mask = _view(op["mask"], tdt, ldm, moff, cin)
    dest = _guarded(lead, ld, tdt, gen)
    out = dest["out"]
    wsb = lib.din_conv_workspace_bytes(C.byref(d), which)
    wsbuf, ws = _guarded_workspace(wsb)

    for flags in _modes(row):
        v, S, exact = _expect(row, op, flags)
        staged = v - op["old"].double() if flags & ACCUM else None
        bar = bar_of(row, v, S, splitk, staged).clamp_min(1e-300)

        def launch():
            if which == 0:
                L.check(lib.din_conv_fwd(C.byref(d), src.data_ptr(), wpk.data_ptr(), bias.data_ptr() if flags & BIAS else None, out.data_ptr(), flags,
                                         ws.data_ptr() if wsb else None, wsb, None))
            else:
                L.check(lib.din_conv_dgrad(C.byref(d), src.data_ptr(), wpk.data_ptr(), out.data_ptr(), mask.data_ptr() if flags & MASK else None,
                                           ldm if flags & MASK else 0, moff if flags & MASK else 0, flags, ws.data_ptr() if wsb else None, wsb, None))

        _launch_twice_and_compare(f"{row['label']} flags={flags}", launch, wsbuf, wsb,
                                  [dict(dest, off=off, c=c, v=v.reshape(*lead, c), bar=bar.reshape(*lead, c), exact=exact, old=op["old"] if flags & ACCUM else None)])
