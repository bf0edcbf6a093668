"""csrc/roi_align.hip, csrc/bn.hip, the colsum kernels of conv_wgrad.hip, the bn_fold* kernels of conv_pack.hip and the image preparation, frame-index and counter
kernels of elementwise.hip, called through the C ABI and compared with float64 references written here from the definition of each
operation, on the stored fp32 / bf16 operands.  The reference is never another kernel of this library.  Every destination is a _Buf
(guard bands, NaN in the columns outside the view): all of that must come back bit for bit, NaN in unused source columns must reach no
result, sources are not written.  Integer outputs and footprints are compared exactly and no element of any row is left out.  Outputs
written with plain stores repeat bit for bit on a second launch; outputs that meet in atomics (din_roi_align_bwd, din_colsum) are held
to their bar only.

Decisions the kernels take in fp32 are restated in numpy float32, same operations in the same order, and only then widened: the RoI
sample coordinate with its floor / ceil / out-of-range tests (_sample), resize_coord's truncation (_resize), ReLU masks, and the xhat
of the backward statistics.

Bars are per element, (n + 1) u sum|terms|, u = 2^-24 (fp32) or 2^-53 (the fp64 statistics), n the rounded operations that reach the
element, counted from the kernels.  The rule applies per format: a bf16 destination is one more rounded operation in units of
u16 = 2^-8, so it adds (1 + 1) u16 |ref|.
  RoI forward     v = top + (bot - top) ly, top = tl + (tr - tl) lx: three roundings per lerp, two levels: n = 6; the terms are the
                  lerp's own, |tl| + lx (|tl| + |tr|) per level, i.e. sum A_y A_x |pixel| with A = (1 + l at lo, l at hi).  ly, lx
                  (in - floor(in), exact) are the fp32 values widened.
  composed fwd    an axis weight w[i] is the sum of up to four products wl (1 - la): 1 - l, 1 - la, the product, three adds: 6;
                  rowacc += wx q: 1 + 3 adds; acc += wy rowacc: 1 + 3 adds: n = 6 + 4 + 6 + 4 = 20, terms |wy wx pixel|.
  gather bwd      w = wy wx: the axis weights (plain: 1 - l, and + l where hi == lo: 2 each; composed: 6 each), the product 1; acc += w v:
                  1 and one add per contributing sample (cnt of the pixel, counted on the host as the kernel counts them); a frame
                  with more than `cap` boxes re-reads its partial once per later batch (one more add each): n = 5 + cnt + (batches - 1)
                  plain, 14 + cnt + (batches - 1) composed; terms |w dout|.  bf16: one rounding of a partial sum (<= sum|terms|) per
                  batch: (batches + 1) u16 sum|terms|.
  scatter bwd     g (1 - ly) (1 - lx): two coefficient roundings and two products, then the atomic adds that meet in the cell (four per
                  live sample, counted per cell): n = 4 + adds.
  BN statistics   fp64 sums of exact terms ((double)x - (double)shift and its fma square; gz and gz * xhat with xhat the fp32 value): a
                  thread adds ceil(rpb / rpp) terms, the workgroup rpp row lanes, the slab reduction ceil(parts / 16) + 16:
                  n = their sum, u = 2^-53.
  BN finalize     fp64 arithmetic (its cancellation in q2 / M - ms^2 is a term of the rstd bar), one rounding to fp32: mean, rstd n = 1;
                  a = gamma rstd: n = 2; b = beta - mean a: n = 5 on |beta| + |mean a|; the running updates (1 - momentum, two products,
                  the conversion, the add): n = 5.  a and b: twice their worst case, 4 u and 10 u (the reason stands next to the bars).
  BN apply        z = x a + b: n = 2 on |x a| + |b|, twice its worst case: 4 u; the ReLU mask is the fp32 sign, restated.
  BN bwd apply    dy = gamma rstd (g - k1 - xh k2): k = (float)sum * (1 / (float)M): 4, xh 2, their product 1, the subtraction 1, gamma rstd and
                  the last product 2: n = 10 on |gamma rstd| (|g| + |k1| + |xh k2|); dgamma, dbeta: the conversion, n = 1.
  colsum          vector path: ceil(rpb / rows_pp) adds per thread, rows_pp in LDS, one atomic per workgroup; scalar path: 512 adds per
                  thread and the atomics.
  bn_fold         scale = gamma / sqrt(var + eps): n = 3 (worst case 2.5 u: 5 u); shift = beta - mean scale: n = 5;
                  dgamma = (wdot - dshift mean) rstd: n = 6 (worst case 5.5 u: 11 u).
  prep_images     three separately rounded fp32 operations: exact; bf16 its round-to-nearest-even; pad channels exactly 0.
test_bars_bite (CPU) shows for every row that each applicable wrong float64 variant misses a bar by >= 10x (which variant applies to which
row is decided from the row's geometry, never from a result); test_roi_reference_matches_oracle (CPU) ties the RoIAlign restatement to
oracle.din_oracle.roi_align; test_roi_refusals (CPU) is host-only.  Branches of the gather kernel and the rows aimed at them: ballot
rounds (m256, m257, interleaved), the cut inside a round (m260_k9_*), later batches re-reading a rounded partial (m257, m260_k9_*,
interleaved; m260_k9_strided: on a strided view), the 48-entry sample list (over48_*) and its rescan, prezeroed_under48 / strided_under48, dout_c /
dout_coff (fuse_a, fuse_b), lanes beyond nchunk (c288, c768)."""
import ctypes as C
import functools
import itertools
import math

import numpy as np
import pytest
import torch

from tests.test_gpu_head_path import _Buf, _check, _gen, _ratio, _refused, env  # noqa: F401  (env: the module-scoped library fixture)

U32, U16, U64 = 2.0 ** -24, 2.0 ** -8, 2.0 ** -53
BF, FP = torch.bfloat16, torch.float32
F32 = np.float32
_INT = {torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.int32: torch.int32}


def _bits(t):
    return t.contiguous().view(_INT[t.dtype])


def _lib():
    from din_amd import _lib as L
    return L.load(), L


def _code(L, dtype):
    return L.DIN_BF16 if dtype == BF else L.DIN_F32


def _same(*bufs):
    return all(b is None or b.unchanged() for b in bufs)


# =====================================================================================================================================
# 1. RoIAlign
# =====================================================================================================================================
# one box set for every row: (x1, y1, x2, y2) in cells of the grid the boxes live on, frame, class.  The classes are counted on the
# 22 x 40 map at k = 5 by test_roi_box_classes.
BOXES = [
    ((3.3, 2.7, 12.1, 9.4), 0, "interior"), ((20.5, 10.2, 31.7, 19.9), 1, "interior"), ((8.25, 5.5, 15.75, 14.5), 2, "interior"),
    ((25.1, 3.2, 33.3, 8.8), 0, "interior"), ((0.5, 0.5, 1.5, 1.5), 0, "interior"), ((2.2, 1.1, 5.4, 4.3), 1, "interior"),
    ((0.0, 0.0, 0.0, 0.0), 1, "padding"),
    ((-3.0, 5.0, 6.0, 12.0), 0, "left"), ((35.2, 5.0, 44.2, 12.0), 1, "right"), ((10.0, -3.0, 18.0, 4.0), 2, "top"),
    ((10.0, 16.2, 18.0, 24.2), 0, "bottom"),
    ((50.0, 30.0, 60.0, 40.0), 1, "outside"),
    ((4.0, 4.0, 9.0, 9.0), 2, "integer"),
    ((35.0, 17.0, 40.0, 22.0), 0, "last_cell"), ((36.0, 18.0, 41.0, 23.0), 2, "last_grid_cell"),
    ((12.3, 6.0, 12.3, 11.0), 1, "degenerate"),
    ((20.0, 8.0, 14.0, 13.0), 2, "reversed"),
    ((7.6, 7.6, 7.9, 7.9), 0, "subcell"), ((0.6, 0.6, 0.9, 0.9), 1, "subcell"),
    ((6.1, 3.3, 14.2, 10.0), -1, "ind_minus_1"), ((6.1, 3.3, 14.2, 10.0), 3, "ind_nb"),
]
CLASSES = ("interior", "padding", "left", "right", "top", "bottom", "outside", "integer", "last_cell", "last_grid_cell", "degenerate",
           "reversed", "subcell", "ind_minus_1", "ind_nb")
ROI_WRONG = ("no_half", "extent", "step_k", "swap_l", "oob_ge", "clamp", "ceil_plus1", "half_pixel", "mask_ge", "flatten", "no_coff")


def _box_set(nb, tile=None, frames=None, clones=0, sel=None):
    """boxes [m][4] fp32 and box_ind [m] int32.  tile = m: the set repeated with a small shift per repetition (rows that need hundreds of
    boxes); frames: a function i -> frame for those; clones: that many more copies of the first sub-cell box in its own frame (all k x k
    samples of each copy share one cell's corners); a frame index of the set beyond nb - 1 stays out of range on purpose"""
    base = [BOXES[i] for i in sel] if sel is not None else list(BOXES)
    base = base + [BOXES[17]] * clones
    m = tile or len(base)
    box = np.zeros((m, 4), dtype=F32)
    ind = np.zeros(m, dtype=np.int32)
    for i in range(m):
        (x1, y1, x2, y2), fr, _ = base[i % len(base)]
        rep = i // len(base)
        box[i] = F32(x1) + F32(0.21) * F32(rep % 23), F32(y1) + F32(0.13) * F32(rep % 11), F32(x2) + F32(0.21) * F32(rep % 23), \
            F32(y2) + F32(0.13) * F32(rep % 11)
        ind[i] = frames(i) if frames else (fr if fr < 0 or fr >= 3 else fr % nb)
    return torch.from_numpy(box), torch.from_numpy(ind)


def _sample(c1, c2, extent, k, wrong=None):
    """roi_sample of csrc/roi_align.hip (row R of oracle/din_oracle.py) in numpy float32, operation for operation: the coordinate
    [m][k], its clamped floor / ceil cells, l = in - floor(in) and the out-of-range flag"""
    c1, c2 = c1.astype(F32), c2.astype(F32)
    kf, em1 = F32(k), F32(extent if wrong == "extent" else extent - 1)
    sp = (c2 - c1) / kf
    t = c1 + sp / F32(2)
    n0 = (t if wrong == "no_half" else t - F32(0.5)) / em1
    nl = (sp * F32(k - 1)) / em1
    n1 = n0 + nl
    if k > 1:
        step = ((n1 - n0) * em1) / F32(k if wrong == "step_k" else k - 1)
        pos = (n0 * em1)[:, None] + np.arange(k, dtype=F32)[None, :] * step[:, None]
    else:
        pos = ((F32(0.5) * (n0 + n1)) * em1)[:, None]
    assert pos.dtype == F32
    oob = (pos < 0) | ((pos >= em1) if wrong == "oob_ge" else (pos > em1))
    fl = np.floor(pos)
    ce = fl + 1 if wrong == "ceil_plus1" else np.ceil(pos)
    l = pos - fl
    assert l.dtype == F32
    lo, hi = (np.clip(v.astype(np.int64), 0, extent - 1) for v in (fl, ce))
    return pos, lo, hi, l, oob


def _resize(g, extent, grid, wrong=None):
    """resize_coord: grid cell -> the two stored cells and the weight of the second, fp32 operations as the kernel's"""
    if wrong == "half_pixel":
        src = np.maximum((g.astype(F32) + F32(0.5)) * F32(extent) / F32(grid) - F32(0.5), F32(0))
    else:
        src = (F32(extent - 1) / F32(grid - 1)) * g.astype(F32)
    assert src.dtype == F32
    i0 = np.minimum(src.astype(np.int64), extent - 1)               # (int)src truncates
    i1 = np.minimum(i0 + 1, extent - 1)
    return i0, i1, (src - i0.astype(F32)).astype(np.float64)


def _axis(c1, c2, grid, extent, k, wrong=None):
    """the taps of one axis: stored cells idx[t] [m][k], their float64 weights w[t], and mag[t], the sizes the forward bar sums"""
    pos, lo, hi, l, oob = _sample(c1, c2, grid, k, wrong)
    l = l.astype(np.float64)
    out = dict(pos=pos, lo=lo, hi=hi, l=l, oob=oob, plain=grid == extent)
    if grid == extent:
        out.update(idx=[lo, hi], w=[1 - l, l], mag=[1 + l, l])
    else:
        a0, a1, la = _resize(lo, extent, grid, wrong)
        b0, b1, lb = _resize(hi, extent, grid, wrong)
        w = [(1 - l) * (1 - la), (1 - l) * la, l * (1 - lb), l * lb]
        out.update(idx=[a0, a1, b0, b1], w=w, mag=w)
    return out


def _gather_cap(m, k):
    return max(1, min(m, (48 * 1024) // (16 + 20 * k), 256))


def roi_reference(fm, boxes, ind, k, grid=None, dout=None, dout_coff=0, mask=None, wrong=None):
    """RoIAlign(k, k) of the boxes (cells of a gh x gw grid) on the stored map fm [nb][hf][wf][c]: the grid is fm's align-corners bilinear
    resize when it is larger, so a sample is the four-tap by four-tap sum over stored pixels (two by two when the extents are equal).
    Without dout: the crops [m][c][k][k], their bar terms and the index record.  With dout [m][dout_c][k][k]: the map's gradient
    [nb][hf][wf][c] (channels [dout_coff, dout_coff + c) of dout; mask: a stored map whose elements <= 0 block it), its terms, and per
    pixel the contributing samples (cnt, as the gather kernel lists them) and the atomic adds of the scatter form (adds)"""
    nb, hf, wf, c = fm.shape
    gh, gw = grid or (hf, wf)
    b = boxes.numpy().astype(F32)
    ind = ind.numpy().astype(np.int64)
    m = b.shape[0]
    ay, ax = _axis(b[:, 1], b[:, 3], gh, hf, k, wrong), _axis(b[:, 0], b[:, 2], gw, wf, k, wrong)
    live = (ind >= 0) & (ind < nb)
    dead = np.broadcast_to(~live[:, None, None], (m, k, k))
    if wrong != "clamp":
        dead = dead | ay["oob"][:, :, None] | ax["oob"][:, None, :]
    keep = torch.from_numpy(~dead)
    n = np.clip(ind, 0, nb - 1)
    wy = [(w[:, :, None], g[:, :, None]) for w, g in zip(ay["w"], ay["mag"])]
    wx = [(w[:, None, :], g[:, None, :]) for w, g in zip(ax["w"], ax["mag"])]
    if wrong == "swap_l":                                         # (plain rows) the x fraction weights the rows and the y fraction the columns
        ly, lx = ax["l"][:, None, :], ay["l"][:, :, None]
        wy, wx = [(1 - ly, 1 + ly), (ly, ly)], [(1 - lx, 1 + lx), (lx, lx)]
    res = dict(idx=np.stack([np.broadcast_to(ay["lo"][:, :, None], (m, k, k)), np.broadcast_to(ay["hi"][:, :, None], (m, k, k)),
                             np.broadcast_to(ax["lo"][:, None, :], (m, k, k)), np.broadcast_to(ax["hi"][:, None, :], (m, k, k)),
                             np.broadcast_to(ay["oob"][:, :, None], (m, k, k)), np.broadcast_to(ax["oob"][:, None, :], (m, k, k))], -1),
               dead=dead, ay=ay, ax=ax)
    taps = []
    for iy, (wyt, myt) in zip(ay["idx"], wy):
        for ix, (wxt, mxt) in zip(ax["idx"], wx):
            pix = torch.from_numpy((n[:, None, None] * hf + iy[:, :, None]) * wf + ix[:, None, :])
            taps.append((pix, torch.from_numpy(np.broadcast_to(wyt * wxt, (m, k, k)).copy()),
                         torch.from_numpy(np.broadcast_to(myt * mxt, (m, k, k)).copy())))
    composed = not (ay["plain"] and ax["plain"])
    if dout is None:
        flat = fm.double().reshape(nb * hf * wf, c)
        out, terms = torch.zeros(m, k, k, c, dtype=torch.float64), torch.zeros(m, k, k, c, dtype=torch.float64)
        for pix, w, mag in taps:
            v = flat[pix]
            out += w.unsqueeze(-1) * v
            terms += mag.unsqueeze(-1) * v.abs()
        out[~keep], terms[~keep] = 0, 0
        out, terms = out.permute(0, 3, 1, 2).contiguous(), terms.permute(0, 3, 1, 2).contiguous()
        if wrong == "flatten":                                    # the crop written as [m][kk][c]
            out = out.permute(0, 2, 3, 1).reshape(m, c, k, k)
        res.update(out=out, bar=(21 if composed else 7) * U32 * terms)
        return res
    d = dout.double()
    d = d.reshape(m, k, k, -1) if wrong == "flatten" else d.permute(0, 2, 3, 1)
    off = 0 if wrong == "no_coff" else dout_coff
    d = d[..., off:off + c]
    g, terms = torch.zeros(nb * hf * wf, c, dtype=torch.float64), torch.zeros(nb * hf * wf, c, dtype=torch.float64)
    for pix, w, _ in taps:
        g.index_add_(0, pix[keep], (w.unsqueeze(-1) * d)[keep])
        terms.index_add_(0, pix[keep], (w.unsqueeze(-1) * d.abs())[keep])
    g, terms = g.view(nb, hf, wf, c), terms.view(nb, hf, wf, c)
    if mask is not None:
        ok = (mask.double() >= 0) if wrong == "mask_ge" else (mask.double() > 0)
        g, terms = g * ok, terms * ok

    def per_cell(a, extent, merged):
        """[m][extent]: merged: the samples whose (merged) weight on the cell is not zero; else the taps that name the cell"""
        hit = np.zeros((m, k, extent))
        for idx, w in zip(a["idx"], a["w"]):
            np.add.at(hit, (np.arange(m)[:, None], np.arange(k)[None, :], idx), (w != 0) if merged else 1)
        hit = hit * ~a["oob"][:, :, None]
        return ((hit > 0) if merged else hit).sum(1)

    cnt, adds = np.zeros((nb, hf, wf)), np.zeros((nb, hf, wf))
    for tot, merged in ((cnt, True), (adds, False)):
        cy, cx = per_cell(ay, hf, merged), per_cell(ax, wf, merged)
        np.add.at(tot, n[live], cy[live][:, :, None] * cx[live][:, None, :])
    per_frame = np.bincount(ind[live], minlength=nb)
    batches = np.maximum(1, -(-per_frame // _gather_cap(m, k)))
    cnt_t, adds_t = torch.from_numpy(cnt).unsqueeze(-1), torch.from_numpy(adds).unsqueeze(-1)
    bt = torch.from_numpy(batches).double().view(nb, 1, 1, 1)
    res.update(g=g, terms=terms, cnt=cnt, batches=batches,
               bar32=((14 if composed else 5) + cnt_t + bt) * U32 * terms,                  # (n + 1), n = base + cnt + (batches - 1)
               bar16=((14 if composed else 5) + cnt_t + bt) * U32 * terms + (bt + 1) * U16 * terms,
               bar_scatter=(5 + adds_t) * U32 * terms)
    return res


# ---- rows ---------------------------------------------------------------------------------------------------------------------------
def _f(name, c=96, k=5, hw=(22, 40), nb=3, grid=None, ldf=None, foff=0, out_c=None, out_coff=0, idx=False, sel=None):
    return dict(name=name, c=c, k=k, hw=hw, nb=nb, grid=grid, ldf=ldf or c, foff=foff, out_c=out_c or c, out_coff=out_coff, idx=idx, sel=sel)


FWD_ROWS = [
    _f("vector_c96_k5_idx", idx=True),
    _f("c8", c=8),
    _f("padded_ldf", c=32, ldf=48, foff=8),
    _f("k1", c=32, k=1, idx=True),
    _f("k3", c=32, k=3),
    _f("k7_more_samples_than_waves", c=32, k=7),
    _f("out_c_gt_c_coff8", c=32, out_c=56, out_coff=8),
    _f("map2x2", c=16, hw=(2, 2)),
    _f("scalar_c20", c=20, idx=True),                              # (c % v != 0 for bf16's 8-channel chunks; fp32 keeps the vector kernel)
    _f("scalar_c22", c=22),                                        # (... for both)
    _f("scalar_ldf_not_vector", c=96, ldf=98, foff=1),
    _f("scalar_lds_over_64k", c=1056, k=16, hw=(6, 7), nb=1, sel=[4]),
    _f("composed_both_axes", c=32, hw=(11, 20), grid=(23, 41)),
    _f("composed_x_only", c=32, hw=(22, 20), grid=(22, 41)),
    _f("composed_y_only", c=32, hw=(11, 40), grid=(23, 40)),
    _f("composed_grid_one_larger", c=32, hw=(22, 40), grid=(23, 41)),
    _f("composed_last_grid_row_and_column", c=16, hw=(11, 20), grid=(23, 41), sel=[14, 0, 13]),
]
FWD_IDS = [r["name"] for r in FWD_ROWS]


def _g(name, dtype, mask, composed, c=96, k=5, nb=3, ldg=None, goff=0, dout_c=None, dout_coff=0, over48=None, **boxes):
    hw, grid = ((11, 20), (23, 41)) if composed else ((22, 40), None)
    return dict(name=name, dtype=dtype, mask=mask, composed=composed, c=c, k=k, nb=nb, hw=hw, grid=grid, ldg=ldg or c, goff=goff,
                dout_c=dout_c or c, dout_coff=dout_coff, over48=over48, boxes=boxes)


GATHER_ROWS = [
    _g("prezeroed_under48", FP, 1, 0, over48=False),
    _g("strided_under48", BF, 0, 0, ldg=112, goff=8, over48=False),
    _g("fuse_a_dout_coff0", BF, 1, 0, c=32, dout_c=96, dout_coff=0),
    _g("fuse_b_dout_coff32", FP, 0, 1, c=64, dout_c=96, dout_coff=32),
    _g("empty_frame_strided", BF, 1, 0, c=32, ldg=48, goff=8, sel=[0, 2, 3, 7, 9, 12]),          # (no box of these lies in frame 1)
    _g("m1", FP, 0, 0, c=32, over48=False, sel=[0]),
    _g("m256_in_one_frame", BF, 0, 1, c=8, tile=276, frames=lambda i: 0 if i < 256 else 1 + i % 2),
    _g("m257_in_one_frame", FP, 1, 1, c=8, tile=300, frames=lambda i: 0 if (i < 200 or 230 <= i < 287) else 1 + i % 2),
    _g("interleaved_two_frames_three_rounds", BF, 1, 0, c=8, tile=700, frames=lambda i: (i // 3) % 2 if i % 11 else 2),
    _g("m260_k9_strided_cut_inside_round", FP, 0, 0, c=8, k=9, nb=2, ldg=16, goff=4, over48=True, tile=260, frames=lambda i: 0),
    _g("m260_k9_prezeroed_cut_inside_round", BF, 1, 0, c=8, k=9, nb=2, over48=True, tile=260, frames=lambda i: 0),
    _g("c288_over_64_chunks", FP, 1, 0, c=288),
    _g("c768_over_64_chunks", BF, 0, 1, c=768, sel=[0, 1, 2, 5, 12, 14, 17]),
    _g("over48_plain", FP, 0, 0, c=32, over48=True, clones=2),
    _g("over48_composed_strided", BF, 1, 1, c=32, ldg=40, goff=8, over48=True, clones=2),
]
GATHER_IDS = [r["name"] for r in GATHER_ROWS]
SCATTER_ROWS = [dict(name="scatter_c96", c=96, k=5, nb=3, hw=(22, 40)), dict(name="scatter_c20", c=20, k=5, nb=3, hw=(22, 40))]
SCATTER_IDS = [r["name"] for r in SCATTER_ROWS]


@functools.lru_cache(maxsize=None)
def _fwd_operands(name, dtype):
    row = FWD_ROWS[FWD_IDS.index(name)]
    gen = _gen("roi_fwd_" + name)
    fm = torch.randn(row["nb"], *row["hw"], row["c"], generator=gen).to(dtype)
    boxes, ind = _box_set(row["nb"], sel=row["sel"])
    return dict(fm=fm, boxes=boxes, ind=ind)


@functools.lru_cache(maxsize=None)
def _fwd_expected(name, dtype, wrong=None):
    row, o = FWD_ROWS[FWD_IDS.index(name)], _fwd_operands(name, dtype)
    return roi_reference(o["fm"], o["boxes"], o["ind"], row["k"], row["grid"], wrong=wrong)


@functools.lru_cache(maxsize=None)
def _bwd_operands(name):
    row = (GATHER_ROWS + SCATTER_ROWS)[(GATHER_IDS + SCATTER_IDS).index(name)]
    gen = _gen("roi_bwd_" + name)
    boxes, ind = _box_set(row["nb"], **row.get("boxes", {}))
    m, k = boxes.shape[0], row["k"]
    dout = torch.randn(m, row.get("dout_c", row["c"]), k, k, generator=gen)
    # the map whose sign masks the gradient is a ReLU output: half of it exact zeros
    fm = torch.randn(row["nb"], *row["hw"], row["c"], generator=gen).clamp_min(0).to(row.get("dtype", FP))
    return dict(boxes=boxes, ind=ind, dout=dout, fm=fm)


@functools.lru_cache(maxsize=None)
def _bwd_expected(name, wrong=None):
    row = (GATHER_ROWS + SCATTER_ROWS)[(GATHER_IDS + SCATTER_IDS).index(name)]
    o = _bwd_operands(name)
    return roi_reference(o["fm"], o["boxes"], o["ind"], row["k"], row.get("grid"), dout=o["dout"], dout_coff=row.get("dout_coff", 0),
                         mask=o["fm"] if row.get("mask") else None, wrong=wrong)


def _in_live_frame(ref, nb, ind):
    live = ((ind.numpy() >= 0) & (ind.numpy() < nb))[:, None]
    return live


def _roi_applies(wrong, row, ref, ind, forward):
    """whether a wrong variant changes this row, decided from the row's geometry (the fp32 sample coordinates), never from a result"""
    ay, ax, k, nb = ref["ay"], ref["ax"], row["k"], row["nb"]
    live = _in_live_frame(ref, nb, ind)
    plain = ay["plain"] and ax["plain"]
    hf, wf = row["hw"]
    gh, gw = row.get("grid") or (hf, wf)
    alive = live[:, :, None] & ~ref["dead"]                      # samples that read the map
    frac = lambda a: bool(((a["l"] > 0.05) & (a["l"] < 0.95) & ~a["oob"] & live).any())   # noqa: E731
    if wrong in ("no_half", "step_k"):
        return bool(alive.any()) and (wrong == "no_half" or k > 1) and (frac(ay) or frac(ax))
    if wrong == "extent":                                         # a sample in (extent - 1, extent]: alive only under the wrong test
        oy, ox = (ay["pos"] > gh - 1) & (ay["pos"] <= gh), (ax["pos"] > gw - 1) & (ax["pos"] <= gw)
        return bool((live & oy & ~(ax["oob"] & ~ox).all(1, keepdims=True)).any() or (live & ox & ~(ay["oob"] & ~oy).all(1, keepdims=True)).any())
    if wrong == "oob_ge":                                         # a sample exactly on the last cell, its other axis in range
        ey, ex = ay["pos"] == gh - 1, ax["pos"] == gw - 1
        return bool((live & ey & ~ax["oob"].all(1, keepdims=True)).any() or (live & ex & ~ay["oob"].all(1, keepdims=True)).any())
    if wrong == "clamp":
        return bool((live[:, :, None] & (ay["oob"][:, :, None] | ax["oob"][:, None, :])).any())
    if wrong == "swap_l":
        return plain and bool(alive.any()) and k > 1
    if wrong == "ceil_plus1":                                     # values cannot tell (the weight of hi is 0 there): the index record does
        whole = lambda a, ext: bool(((a["pos"] == np.floor(a["pos"])) & (a["pos"] >= 0) & (a["pos"] < ext - 1)).any())   # noqa: E731
        return forward and row["idx"] and (whole(ay, hf) or whole(ax, wf))
    if wrong == "half_pixel":
        return not plain
    if wrong == "mask_ge":
        return not forward and bool(row.get("mask"))
    if wrong == "flatten":
        return row["c"] > 1 and k > 1 and bool(alive.any())
    if wrong == "no_coff":
        return not forward and row.get("dout_coff", 0) > 0
    raise KeyError(wrong)


def _bite_roi_fwd(name, dtype):
    row, o = FWD_ROWS[FWD_IDS.index(name)], _fwd_operands(name, dtype)
    want = _fwd_expected(name, dtype)
    assert (~want["dead"]).any(), f"{name}: no live sample"
    tried = 0
    for wrong in ROI_WRONG:
        if not _roi_applies(wrong, row, want, o["ind"], True):
            continue
        tried += 1
        bad = _fwd_expected(name, dtype, wrong)
        worst = _ratio(bad["out"], want["out"], want["bar"])
        if row["idx"] and not np.array_equal(bad["idx"], want["idx"]):
            worst = float("inf")                                  # (the index record is compared exactly)
        assert worst >= 10.0, f"{name}: the bars do not see '{wrong}' ({worst:.3g})"
    assert tried >= 3, name


def _bite_roi_bwd(name):
    rows = GATHER_ROWS + SCATTER_ROWS
    row, o = rows[(GATHER_IDS + SCATTER_IDS).index(name)], _bwd_operands(name)
    want = _bwd_expected(name)
    key = "bar_scatter" if name in SCATTER_IDS else ("bar16" if row["dtype"] == BF else "bar32")
    tried = 0
    for wrong in ROI_WRONG:
        if not _roi_applies(wrong, dict(row, idx=False), want, o["ind"], False):
            continue
        tried += 1
        worst = _ratio(_bwd_expected(name, wrong)["g"], want["g"], want[key])
        assert worst >= 10.0, f"{name}: the bars do not see '{wrong}' ({worst:.3g})"
    assert tried >= 3, name


def test_roi_box_classes():
    """the box set holds every class, and on the 22 x 40 map at k = 5 each does what its name says"""
    names = [b[2] for b in BOXES]
    for cls in CLASSES:
        assert names.count(cls) >= 1, cls
    assert names.count("interior") == 6 and names.count("subcell") == 2
    boxes, ind = _box_set(3)
    r = roi_reference(torch.zeros(3, 22, 40, 1), boxes, ind, 5)
    ay, ax = r["ay"], r["ax"]
    at = lambda cls: [i for i, n in enumerate(names) if n == cls]   # noqa: E731
    for i in at("interior"):
        assert not ay["oob"][i].any() and not ax["oob"][i].any()
    for i in at("padding") + at("outside"):
        assert r["dead"][i].all()
    assert ax["oob"][at("left")[0]].any() and not ax["oob"][at("left")[0]].all() and (ax["pos"][at("left")[0]] < 0).any()
    assert (ax["pos"][at("right")[0]] > 39).any() and not ax["oob"][at("right")[0]].all()
    assert (ay["pos"][at("top")[0]] < 0).any() and not ay["oob"][at("top")[0]].all()
    assert (ay["pos"][at("bottom")[0]] > 21).any() and not ay["oob"][at("bottom")[0]].all()
    i = at("integer")[0]
    assert (ay["lo"][i] == ay["hi"][i]).all() and (ax["lo"][i] == ax["hi"][i]).all() and not r["dead"][i].any()
    i = at("last_cell")[0]
    assert ay["pos"][i][-1] == 21 and ax["pos"][i][-1] == 39 and not r["dead"][i].any()
    g = roi_reference(torch.zeros(3, 11, 20, 1), boxes, ind, 5, (23, 41))
    i = at("last_grid_cell")[0]
    assert g["ay"]["pos"][i][-1] == 22 and g["ax"]["pos"][i][-1] == 40 and not g["dead"][i].any()
    i = at("degenerate")[0]
    assert (ax["pos"][i] == ax["pos"][i][0]).all() and not r["dead"][i].any()
    i = at("reversed")[0]
    assert (np.diff(ax["pos"][i]) < 0).all() and not r["dead"][i].any()
    for i in at("subcell"):
        assert len(set(ay["lo"][i]) | set(ax["lo"][i])) == 1 and (ay["hi"][i] == ay["lo"][i] + 1).all() and not r["dead"][i].any()
    assert ind[at("ind_minus_1")[0]] == -1 and ind[at("ind_nb")[0]] == 3 and r["dead"][at("ind_minus_1")[0]].all() and r["dead"][at("ind_nb")[0]].all()
    assert not ay["oob"][at("ind_nb")[0]].any()                     # (dead through its frame alone)


def test_roi_gather_rows_cover_every_pair_of_flags():
    """fp32 / bf16, mask / none and plain / composed each meet each other in some gather row (every row runs transposed 0 and 1), and the
    rows aimed at the sample list (over48: True / False) lie on the side of 48 they claim, counted on the host as the kernel counts them"""
    for a, b in itertools.combinations(("dtype", "mask", "composed"), 2):
        seen = {(r[a], r[b]) for r in GATHER_ROWS}
        assert len(seen) == 4, (a, b, seen)
    for row in GATHER_ROWS:
        want = _bwd_expected(row["name"])
        assert row["over48"] is None or (want["cnt"].max() > 48) == row["over48"], (row["name"], want["cnt"].max())
        assert want["cnt"].max() > 0
    frames = lambda name: np.bincount(_bwd_operands(name)["ind"].numpy().clip(0), minlength=3)   # noqa: E731
    assert frames("m256_in_one_frame")[0] == 256 and frames("m257_in_one_frame")[0] == 257 and frames("m260_k9_strided_cut_inside_round")[0] == 260
    assert _gather_cap(260, 9) == 250                              # the cut at slot == cap falls inside the first 256-id round
    inter = frames("interleaved_two_frames_three_rounds")
    assert inter[0] > 256 and inter[1] > 256 and inter[2] > 0
    assert frames("empty_frame_strided")[1] == 0
    for name in ("m257_in_one_frame", "m260_k9_strided_cut_inside_round", "m260_k9_prezeroed_cut_inside_round", "interleaved_two_frames_three_rounds"):
        assert _bwd_expected(name)["batches"].max() == 2


@pytest.mark.parametrize("k", [5, 1, 3])
def test_roi_reference_matches_oracle(k):
    """the restatement's indices equal oracle.din_oracle.roi_align(..., return_index=True) exactly and its values lie within the forward
    bar of the oracle's fp32 output"""
    from oracle import din_oracle as O
    boxes, ind = _box_set(3)
    fm = torch.randn(3, 22, 40, 24, generator=_gen(f"oracle_roi{k}"))
    mine = roi_reference(fm, boxes, ind, k)
    out, ridx = O.roi_align(fm.permute(0, 3, 1, 2).contiguous(), boxes, ind, k, return_index=True)
    idx = mine["idx"]
    for col, key in enumerate(("top", "bot", "left", "right", "oob_y", "oob_x")):
        got = idx[:, :, 0, col] if col in (0, 1, 4) else idx[:, 0, :, col]
        assert np.array_equal(got.astype(np.int64), ridx[key].numpy().astype(np.int64)), key
    frames_ok = ((ind >= 0) & (ind < 3)).view(-1, 1, 1, 1)
    assert _ratio(torch.where(frames_ok, out.double(), torch.zeros((), dtype=torch.float64)), mine["out"], mine["bar"]) <= 1.0


def _dummy():
    return C.c_void_p(4096)                                       # a non-null pointer no refused call may touch


def test_roi_refusals():
    """host-only: each returns its error and message before anything is launched"""
    lib, L = _lib()
    d, nul = _dummy(), None

    def fwd(hf=22, wf=40, c=32, ldf=32, gh=22, gw=40, k=5, out_c=32, out_coff=0, idx=nul, dt=0):
        return lib.din_roi_align_fwd(d, dt, 3, hf, wf, c, ldf, gh, gw, d, d, 4, k, d, out_c, out_coff, idx, nul)

    def bwd(dout_c=32, dout_coff=0, transposed=0, hf=22, wf=40, c=32, gh=22, gw=40, k=5, ldg=32, dt=0):
        return lib.din_roi_align_bwd_nhwc(d, dout_c, dout_coff, transposed, 3, hf, wf, c, gh, gw, d, d, 4, k, nul, dt, c, d, ldg, nul)

    _refused(fwd(gh=21), "must not be smaller")
    _refused(bwd(gh=21), "must not be smaller")
    _refused(fwd(gw=39), "must not be smaller")
    _refused(fwd(gh=23, gw=41, idx=d), "index record describes the plain")
    _refused(fwd(gh=23, gw=41, c=30, ldf=32, out_c=30), "resized sampling needs channels / stride in multiples of 4")
    _refused(fwd(gh=23, gw=41, c=36, ldf=36, out_c=36, dt=1), "multiples of 8")
    _refused(fwd(k=65), "crop size > 64")
    _refused(bwd(k=65), "bad shape")
    _refused(fwd(out_c=40, out_coff=16), "do not fit a 40-channel crop")
    _refused(bwd(dout_c=40, dout_coff=16), "do not fit a 40-channel crop")
    _refused(bwd(dout_c=64, dout_coff=6, transposed=1), "16-byte channel groups")
    _refused(bwd(ldg=34), "pixel strides must be multiples of 4")
    _refused(bwd(ldg=36, dt=1), "pixel strides must be multiples of 8")
    _refused(fwd(hf=1, gh=1), "bad shape")
    _refused(bwd(hf=1, gh=1), "bad shape")
    _refused(lib.din_roi_align_bwd(d, 3, 1, 40, 32, d, d, 4, 5, d, nul), "bad shape")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [FP, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", FWD_IDS)
def test_roi_align_fwd_against_fp64(env, name, dtype):
    lib, L, nhwc, ops = env
    row, o, want = FWD_ROWS[FWD_IDS.index(name)], _fwd_operands(name, dtype), _fwd_expected(name, dtype)
    (hf, wf), (gh, gw) = row["hw"], row["grid"] or row["hw"]
    c, k, nb, m, kk = row["c"], row["k"], row["nb"], o["boxes"].shape[0], row["k"] ** 2
    FM = _Buf((nb, hf, wf), c, dtype, content=o["fm"], ld=row["ldf"], off=row["foff"])
    BX, IND = _Buf((m,), 4, content=o["boxes"]), _Buf((1,), m, torch.int32, content=o["ind"])

    def run():
        OUT = _Buf((m,), c * kk, ld=row["out_c"] * kk, off=row["out_coff"] * kk)
        IDX = _Buf((m, k, k), 6, torch.int32) if row["idx"] else None
        L.check(lib.din_roi_align_fwd(FM.view.data_ptr(), _code(L, dtype), nb, hf, wf, c, row["ldf"], gh, gw, BX.ptr(), IND.ptr(), m, k,
                                      OUT.ptr(), row["out_c"], row["out_coff"], IDX.ptr() if IDX else None, None))
        torch.cuda.synchronize()
        return OUT, IDX

    OUT, IDX = run()
    assert OUT.untouched_outside() and (IDX is None or IDX.untouched_outside()) and _same(FM, BX, IND), f"{name}: wrote outside a destination"
    _check(name, "crops", OUT.get().reshape(m, c, k, k), want["out"], want["bar"])
    assert not bool(OUT.get().reshape(m, c, k, k)[torch.from_numpy(want["dead"].copy()).unsqueeze(1).expand(m, c, k, k)].any()), f"{name}: a dead sample is not 0"
    if IDX:
        bad = (IDX.get().long() != torch.from_numpy(want["idx"].astype(np.int64))).nonzero()
        assert bad.numel() == 0, f"{name}: {bad.shape[0]} index records differ, first at {bad[0].tolist()}"
    OUT2, IDX2 = run()
    assert torch.equal(OUT.bits(), OUT2.bits()) and (IDX is None or torch.equal(IDX.bits(), IDX2.bits())), f"{name}: rerun differs"


@pytest.mark.gpu
@pytest.mark.parametrize("name", GATHER_IDS)
def test_roi_align_bwd_gather_against_fp64(env, name):
    """din_roi_align_bwd_nhwc from the reference layout and from din_roi_crop_grad_transpose's copy: each against float64, and the two bit
    for bit (the kernel promises the same summation order)"""
    lib, L, nhwc, ops = env
    row, o, want = GATHER_ROWS[GATHER_IDS.index(name)], _bwd_operands(name), _bwd_expected(name)
    (hf, wf), (gh, gw) = row["hw"], row["grid"] or row["hw"]
    c, k, nb, m, dtype, dc, dco = row["c"], row["k"], row["nb"], o["boxes"].shape[0], row["dtype"], row["dout_c"], row["dout_coff"]
    kk = k * k
    dout = torch.full((m, dc, k, k), float("nan"))                # the other maps' channels of the crop gradient must reach nothing
    dout[:, dco:dco + c] = o["dout"][:, dco:dco + c]
    D, DT = _Buf((m,), dc * kk, content=dout), _Buf((m,), kk * dc)
    FM = _Buf((nb, hf, wf), c, dtype, content=o["fm"], ld=c + 16, off=8) if row["mask"] else None
    BX, IND = _Buf((m,), 4, content=o["boxes"]), _Buf((1,), m, torch.int32, content=o["ind"])
    L.check(lib.din_roi_crop_grad_transpose(D.ptr(), m, dc, k, DT.ptr(), None))
    torch.cuda.synchronize()
    assert DT.untouched_outside() and D.unchanged()
    assert torch.equal(_bits(DT.get().reshape(m, kk, dc)), _bits(dout.view(m, dc, kk).transpose(1, 2).contiguous())), f"{name}: transpose"
    bar = want["bar16" if dtype == BF else "bar32"]
    first, staged = None, DT.bits()
    for transposed in (0, 1):
        runs = []
        for _ in range(2):
            G = _Buf((nb, hf, wf), c, dtype, ld=row["ldg"], off=row["goff"])
            L.check(lib.din_roi_align_bwd_nhwc((DT if transposed else D).ptr(), dc, dco, transposed, nb, hf, wf, c, gh, gw, BX.ptr(), IND.ptr(),
                                               m, k, FM.view.data_ptr() if FM else None, _code(L, dtype), c + 16, G.view.data_ptr(),
                                               row["ldg"], None))
            torch.cuda.synchronize()
            runs.append(G)
        G = runs[0]
        tag = f"{name}[transposed={transposed}]"
        assert G.untouched_outside() and _same(D, FM, BX, IND) and torch.equal(DT.bits(), staged), f"{tag}: wrote outside the view or into a source"
        _check(tag, "map gradient", G.get(), want["g"], bar)
        assert torch.equal(G.bits(), runs[1].bits()), f"{tag}: rerun differs"
        first = first if first is not None else G.bits()
        assert torch.equal(G.bits(), first), f"{name}: the transposed copy changed the summation order"


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCATTER_IDS)
def test_roi_align_bwd_scatter_against_fp64(env, name):
    lib, L, nhwc, ops = env
    row, o, want = SCATTER_ROWS[SCATTER_IDS.index(name)], _bwd_operands(name), _bwd_expected(name)
    (hf, wf), c, k, nb, m = row["hw"], row["c"], row["k"], row["nb"], o["boxes"].shape[0]
    D = _Buf((m,), c * k * k, content=o["dout"])
    BX, IND = _Buf((m,), 4, content=o["boxes"]), _Buf((1,), m, torch.int32, content=o["ind"])
    G = _Buf((nb, hf, wf), c, content=torch.zeros(nb, hf, wf, c))  # the scatter form accumulates: the caller clears
    L.check(lib.din_roi_align_bwd(D.ptr(), nb, hf, wf, c, BX.ptr(), IND.ptr(), m, k, G.ptr(), None))
    torch.cuda.synchronize()
    assert G.untouched_outside() and _same(D, BX, IND)
    _check(name, "map gradient", G.get(), want["g"], want["bar_scatter"])


@pytest.mark.gpu
def test_boxes_frame_index_exact(env):
    lib, L, nhwc, ops = env
    for bt, n in ((3, 100), (1, 1), (7, 13)):
        I = _Buf((1,), bt * n, torch.int32)
        L.check(lib.din_boxes_frame_index(I.ptr(), bt, n, None))
        torch.cuda.synchronize()
        assert I.untouched_outside() and torch.equal(I.get()[0].long(), torch.arange(bt * n) // n)


# =====================================================================================================================================
# 2. batch-statistics BatchNorm, colsum, fold, image preparation
# =====================================================================================================================================
EPS, MOM = float(F32(1e-3)), float(F32(0.1))
BN_ROWS = [(4, 9), (96, 1003), (1024, 37), (8, 262147), (32, 97), (32, 127), (32, 128), (32, 129), (8, 1)]
BN_CASES = [(c, rows, dt) for c, rows in BN_ROWS for dt in (FP, BF)]
BN_IDS = [f"{c}x{rows}-{'bf16' if dt == BF else 'fp32'}" for c, rows, dt in BN_CASES]
BN_WRONG = ("unbiased_norm", "biased_running", "eps_outside", "no_inv_m", "momentum_side", "no_mean_a")
BN_OUT = ("mean", "rstd", "a", "b", "rm", "rv", "y", "dy", "dgamma", "dbeta")


def _bn_geom(c, rows, dtype):
    """channels as run (bf16 lanes hold 8: the one-chunk and one-row-lane rows double their channels; the trip rows scale with rpp)"""
    v = 8 if dtype == BF else 4
    if dtype == BF and (c, rows) in ((4, 9), (1024, 37)):
        c *= 2
    rpp = 256 // (c // v)
    if c == 32:                                                   # rows were listed for fp32's rpp = 32: keep their place relative to 4 rpp
        rows = {97: 3 * rpp + 1, 127: 4 * rpp - 1, 128: 4 * rpp, 129: 4 * rpp + 1}[rows]
    return c, rows, v, rpp


def _bn_depth(rows, rpp, bwd):
    maxp = 512 if bwd else 1024
    rpb = 256 if -(-rows // 256) <= maxp else -(-rows // maxp)
    parts = -(-rows // rpb)
    return -(-rpb // rpp) + rpp + -(-parts // 16) + 16, parts


@functools.lru_cache(maxsize=None)
def _bn_operands(c, rows, dtype):
    gen = _gen(f"bn{c}x{rows}")
    x = torch.randn(rows, c, generator=gen) * 1.7 + 0.4
    x[:, 0] = 0.3                                                 # a constant channel: var == 0, rstd = 1 / sqrt(eps)
    x[:, 1] = 300.0 + torch.randn(rows, generator=gen)            # |mean| >> std
    return dict(x=x.to(dtype), gz=torch.randn(rows, c, generator=gen).to(dtype), gamma=torch.rand(c, generator=gen) + 0.5,
                beta=torch.randn(c, generator=gen) * 0.2, rm=torch.randn(c, generator=gen) * 0.1, rv=torch.rand(c, generator=gen) + 0.5,
                shift=torch.randn(c, generator=gen) * 0.1 + 0.3)


def _lsum(a):
    return a.astype(np.longdouble).sum(0)


def bn_reference(o, shift, relu, dtype, wrong=None):
    """torch.nn.functional.batch_norm(training=True) + ReLU and its backward, stage by stage as the kernels split it; what one stage hands
    to the next is rounded to fp32 the way it is stored, and the next stage reads the stored value"""
    x, gz = o["x"].double().numpy(), o["gz"].double().numpy()
    gamma, beta, rm, rv = (o[k].double().numpy() for k in ("gamma", "beta", "rm", "rv"))
    M, c = x.shape
    sh = o["shift"].double().numpy() if shift else np.zeros(c)
    d = x - sh
    q1, q2 = _lsum(d), _lsum(d * d)
    ms = q1 / M
    mu = (ms + sh).astype(np.float64)
    var = np.maximum(q2 / M - ms * ms, 0).astype(np.float64)
    cancel = (q2 / M + ms * ms).astype(np.float64)
    var_n = var * M / (M - 1) if wrong == "unbiased_norm" else var
    rstd = 1 / (np.sqrt(var_n) + EPS) if wrong == "eps_outside" else 1 / np.sqrt(var_n + EPS)
    a = gamma * rstd
    b = beta - (0 if wrong == "no_mean_a" else mu * a)
    unb = var if (wrong == "biased_running" or M == 1) else var * M / (M - 1)
    m1, m2 = ((MOM, 1 - MOM) if wrong == "momentum_side" else (1 - MOM, MOM))
    r = dict(q1=q1.astype(np.float64), q2=q2.astype(np.float64), q1_abs=_lsum(np.abs(d)).astype(np.float64), mean=mu, rstd=rstd, a=a, b=b,
             rm=m1 * rm + m2 * mu, rv=m1 * rv + m2 * unb)
    mean32, rstd32, a32, b32 = (v.astype(F32) for v in (mu, rstd, a, b))
    x32 = o["x"].float().numpy()
    z = x * a32.astype(np.float64) + b32.astype(np.float64)
    z32 = x32 * a32 + b32                                         # the ReLU decision, in fp32 as the kernel takes it
    assert z32.dtype == F32
    r["y"] = np.where(z32 > 0, z, 0.0) if relu else z
    xhat32 = ((x32 - mean32) * rstd32)
    assert xhat32.dtype == F32
    s1, s2 = _lsum(gz).astype(np.float64), _lsum(gz * xhat32.astype(np.float64)).astype(np.float64)
    xh = (x - mean32.astype(np.float64)) * rstd32.astype(np.float64)
    gr = gamma * rstd32.astype(np.float64)
    inv = 1.0 if wrong == "no_inv_m" else 1.0 / M
    r.update(s1=s1, s2=s2, s1_abs=_lsum(np.abs(gz)).astype(np.float64), s2_abs=_lsum(np.abs(gz * xhat32)).astype(np.float64),
             dy=gr * (gz - s1 * inv - xh * (s2 * inv)), dgamma=s2, dbeta=s1, mean32=mean32, rstd32=rstd32, a32=a32, b32=b32)
    low = 2 * U16 if dtype == BF else 0.0
    r["bars"] = dict(
        mean=2 * U32 * np.abs(mu), rstd=2 * U32 * rstd + 0.5 * rstd ** 3 * 8 * U64 * cancel,
        # a, b, y: short chains whose roundings all reach their worst case somewhere among 10^3 .. 10^6 elements (a: 2 u |a|; b: the
        # conversion of mean, a's two and the product weigh 4 u |mean a|, the subtraction u (|beta| + |mean a|): 5 u of the terms; y:
        # 2 u of the terms).  (n + 1) u would leave 1.5x, 1.2x and 1.5x at that worst case, and no assert here may pass under 2x: the
        # bar is twice the worst case, as for scale_by_param in tests/test_gpu_head_path.py
        a=4 * U32 * np.abs(a) + np.abs(gamma) * 0.5 * rstd ** 3 * 8 * U64 * cancel,
        b=10 * U32 * (np.abs(beta) + np.abs(mu * a)), rm=6 * U32 * (np.abs(m1 * rm) + np.abs(m2 * mu)), rv=6 * U32 * (np.abs(m1 * rv) + np.abs(m2 * unb)),
        y=4 * U32 * (np.abs(x * a32) + np.abs(b32)) + low * np.abs(r["y"]),
        dy=11 * U32 * np.abs(gr) * (np.abs(gz) + np.abs(s1 / M) + np.abs(xh * (s2 / M))) + low * np.abs(r["dy"]),
        dgamma=2 * U32 * np.abs(s2), dbeta=2 * U32 * np.abs(s1))
    return r


def _bn_applies(wrong, rows):
    # M = 1: M / (M - 1) and 1 / M change nothing (the kernel's guard).  The biased variance in the running update is off by var / M: under
    # fp32's own error beyond a few thousand rows
    return {"unbiased_norm": rows > 1, "biased_running": 1 < rows <= 2000, "no_inv_m": rows > 1}.get(wrong, True)


def _bite_bn(c, rows, dtype):
    c, rows, v, rpp = _bn_geom(c, rows, dtype)
    o = _bn_operands(c, rows, dtype)
    for shift, relu in ((0, 0), (1, 1)):
        want = bn_reference(o, shift, relu, dtype)
        for wrong in BN_WRONG:
            if _bn_applies(wrong, rows):
                bad = bn_reference(o, shift, relu, dtype, wrong)
                worst = max(_ratio(torch.from_numpy(np.asarray(bad[k])), torch.from_numpy(np.asarray(want[k])), torch.from_numpy(np.asarray(want["bars"][k])))
                            for k in BN_OUT)
                assert worst >= 10.0, f"bn {c}x{rows}: the bars do not see '{wrong}' ({worst:.3g})"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


class _Ws:
    """the fp64 workspace between two guard bands, NaN inside: it needs no clearing"""

    def __init__(self, n):
        self.n = n
        self.flat = torch.full((n + 16,), float("nan"), dtype=torch.float64)
        self.flat[:8], self.flat[-8:] = -1234.5, -1234.5
        self.flat = self.flat.cuda()

    def ptr(self):
        return self.flat.data_ptr() + 64

    def body(self):
        return self.flat[8:8 + self.n].cpu()

    def guards_ok(self):
        f = self.flat.cpu()
        return bool((f[:8] == -1234.5).all() and (f[-8:] == -1234.5).all())


@pytest.mark.gpu
@pytest.mark.parametrize("c,rows,dtype", BN_CASES, ids=BN_IDS)
def test_batch_stat_bn_stages_against_fp64(env, c, rows, dtype, monkeypatch):
    """din_bn_stats / _reduce / _finalize / _apply / _bwd_stats / _bwd_apply one stage at a time, each fed the float64 reference's previous
    results as stored; x, gz, y and dy are views with four different strides and offsets"""
    lib, L, nhwc, ops = env
    c, rows, v, rpp = _bn_geom(c, rows, dtype)
    o, code, tag = _bn_operands(c, rows, dtype), _code(L, dtype), f"bn{c}x{rows}"
    X = _Buf((rows,), c, dtype, content=o["x"], ld=c + 16, off=8)
    GZ = _Buf((rows,), c, dtype, content=o["gz"], ld=c + 24, off=16)
    GA, BE, SH = (_Buf((1,), c, content=o[k]) for k in ("gamma", "beta", "shift"))
    depth_f, parts = _bn_depth(rows, rpp, False)
    depth_b, parts_b = _bn_depth(rows, rpp, True)
    assert lib.din_bn_parts(rows) == parts and lib.din_bn_workspace(rows, c) == (max(parts, parts_b) + 1) * 2 * c * 8
    nws = (max(parts, parts_b) + 1) * 2 * c
    modes = ((0, 0, 0), (1, 1, 1)) if rows < 100000 else ((1, 1, 1),)
    for shift, running, relu in modes:
        want = bn_reference(o, shift, relu, dtype)
        bars = want["bars"]
        sp = SH.ptr() if shift else None
        # ---- statistics: stats + reduce, twice; then stats + the finalize that reduces itself ----
        sums = []
        for _ in range(2):
            W = _Ws(nws)
            L.check(lib.din_bn_stats(X.ptr(), code, rows, c, c + 16, 8, sp, W.ptr(), None))
            L.check(lib.din_bn_reduce(W.ptr(), parts, c, None))
            torch.cuda.synchronize()
            assert W.guards_ok() and X.unchanged()
            sums.append(W.body()[:2 * c])
        assert torch.equal(sums[0].view(torch.int64), sums[1].view(torch.int64)), f"{tag}: statistics differ between two runs"
        _check(tag, "sum", sums[0][:c], _t(want["q1"]), (depth_f + 1) * U64 * _t(want["q1_abs"]))
        _check(tag, "sum of squares", sums[0][c:], _t(want["q2"]), (depth_f + 1) * U64 * _t(want["q2"]))
        W = _Ws(nws)
        outs = [_Buf((1,), c) for _ in range(4)]
        L.check(lib.din_bn_stats(X.ptr(), code, rows, c, c + 16, 8, sp, W.ptr(), None))
        L.check(lib.din_bn_finalize(W.ptr(), parts, rows, c, GA.ptr(), BE.ptr(), EPS, MOM, None, None, *[b.ptr() for b in outs], sp, None))
        torch.cuda.synchronize()
        assert torch.equal(W.body()[:2 * c].view(torch.int64), sums[0].view(torch.int64)), f"{tag}: finalize's own reduction differs from din_bn_reduce"
        # ---- finalize, fed the reference sums ----
        W = _Ws(nws)
        W.flat[8:8 + 2 * c] = torch.cat([_t(want["q1"]), _t(want["q2"])]).cuda()
        A, B, ME, RS = (_Buf((1,), c) for _ in range(4))
        RM, RV = (_Buf((1,), c, content=o["rm"]), _Buf((1,), c, content=o["rv"])) if running else (None, None)
        L.check(lib.din_bn_finalize(W.ptr(), 0, rows, c, GA.ptr(), BE.ptr(), EPS, MOM, RM.ptr() if RM else None, RV.ptr() if RV else None,
                                    A.ptr(), B.ptr(), ME.ptr(), RS.ptr(), sp, None))
        torch.cuda.synchronize()
        assert all(b.untouched_outside() for b in (A, B, ME, RS)) and _same(GA, BE, SH) and W.guards_ok()
        for key, buf in (("mean", ME), ("rstd", RS), ("a", A), ("b", B)) + ((("rm", RM), ("rv", RV)) if running else ()):
            assert buf.untouched_outside()
            _check(tag, key, buf.get()[0], _t(want[key]), _t(bars[key]))
        # ---- apply, fed a and b as stored: the row-walk kernel and the element kernel ----
        A32, B32 = _Buf((1,), c, content=_t(want["a32"])), _Buf((1,), c, content=_t(want["b32"]))
        ME32, RS32 = _Buf((1,), c, content=_t(want["mean32"])), _Buf((1,), c, content=_t(want["rstd32"]))
        ys = {}
        for rows_opt in (None, "0", None):
            if rows_opt is None:
                L.set_option("DIN_BN_APPLY_ROWS", None)
            else:
                monkeypatch.setenv("DIN_BN_APPLY_ROWS", rows_opt)
            Y = _Buf((rows,), c, dtype, ld=c + 32, off=24)
            L.check(lib.din_bn_apply(X.ptr(), code, rows, c, c + 16, 8, A32.ptr(), B32.ptr(), relu, Y.ptr(), c + 32, 24, None))
            torch.cuda.synchronize()
            assert Y.untouched_outside() and _same(X, A32, B32)
            _check(f"{tag}[APPLY_ROWS={rows_opt}]", "y", Y.get(), _t(want["y"]), _t(bars["y"]))
            ys.setdefault(rows_opt, []).append(Y.bits())
        assert torch.equal(ys[None][0], ys[None][1]), f"{tag}: apply rerun differs"
        assert torch.equal(ys[None][0], ys["0"][0]), f"{tag}: the row-walk apply kernel and the element kernel differ"
        # ---- backward statistics, fed mean and rstd as stored ----
        sums = []
        for _ in range(2):
            W = _Ws(nws)
            L.check(lib.din_bn_bwd_stats(GZ.ptr(), c + 24, 16, X.ptr(), c + 16, 8, code, rows, c, ME32.ptr(), RS32.ptr(), W.ptr(), None))
            torch.cuda.synchronize()
            assert W.guards_ok() and _same(X, GZ, ME32, RS32)
            sums.append(W.body()[:2 * c])
        assert torch.equal(sums[0].view(torch.int64), sums[1].view(torch.int64)), f"{tag}: backward statistics differ between two runs"
        _check(tag, "sum gz", sums[0][:c], _t(want["s1"]), (depth_b + 1) * U64 * _t(want["s1_abs"]))
        _check(tag, "sum gz xhat", sums[0][c:], _t(want["s2"]), (depth_b + 1) * U64 * _t(want["s2_abs"]))
        # ---- backward apply, fed the reference sums ----
        S = _Ws(2 * c)
        S.flat[8:8 + 2 * c] = torch.cat([_t(want["s1"]), _t(want["s2"])]).cuda()
        dys = {}
        for rows_opt in (None, "0", None):
            if rows_opt is None:
                L.set_option("DIN_BN_APPLY_ROWS", None)
            else:
                monkeypatch.setenv("DIN_BN_APPLY_ROWS", rows_opt)
            DY, DG, DB = _Buf((rows,), c, dtype, ld=c + 8, off=8), _Buf((1,), c), _Buf((1,), c)
            L.check(lib.din_bn_bwd_apply(GZ.ptr(), c + 24, 16, X.ptr(), c + 16, 8, code, rows, c, GA.ptr(), ME32.ptr(), RS32.ptr(), S.ptr(),
                                         DY.ptr(), c + 8, 8, DG.ptr(), DB.ptr(), None))
            torch.cuda.synchronize()
            assert DY.untouched_outside() and DG.untouched_outside() and DB.untouched_outside() and _same(X, GZ, GA, ME32, RS32) and S.guards_ok()
            t2 = f"{tag}[APPLY_ROWS={rows_opt}]"
            _check(t2, "dy", DY.get(), _t(want["dy"]), _t(bars["dy"]))
            _check(t2, "dgamma", DG.get()[0], _t(want["dgamma"]), _t(bars["dgamma"]))
            _check(t2, "dbeta", DB.get()[0], _t(want["dbeta"]), _t(bars["dbeta"]))
            dys.setdefault(rows_opt, []).append(torch.cat([DY.bits().flatten().int(), DG.bits().flatten(), DB.bits().flatten()]))
        assert torch.equal(dys[None][0], dys[None][1]), f"{tag}: backward apply rerun differs"
        assert torch.equal(dys[None][0], dys["0"][0]), f"{tag}: the row-walk backward apply kernel and the element kernel differ"


COLSUM_ROWS = [("vector", 96, 1003, 96, 0), ("vector_coff", 96, 1003, 128, 16), ("scalar_c20", 20, 1003, 20, 0), ("scalar_c22", 22, 1003, 22, 0),
               ("scalar_ld_not_vector", 96, 1003, 99, 0),
               ("rows5", 32, 5, 40, 8), ("rows70001_c8", 8, 70001, 8, 0), ("scalar_two_column_trips", 300, 700, 301, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [FP, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name,c,rows,ld,coff", COLSUM_ROWS, ids=[r[0] for r in COLSUM_ROWS])
def test_colsum_against_fp64(env, name, c, rows, ld, coff, dtype):
    """the destination starts as NaN: the entry point clears it (a prior of zero)"""
    lib, L, nhwc, ops = env
    epc = 8 if dtype == BF else 4
    g = torch.randn(rows, c, generator=_gen("colsum" + name)).to(dtype)
    vector = c % epc == 0 and c // epc <= 256 and ld % epc == 0 and coff % epc == 0
    assert vector == (name.startswith(("vector", "rows")) or (name == "scalar_c20" and dtype == FP)), name   # (20 is five fp32 chunks)
    if vector:
        rpb = max(-(-rows // 256), 64)
        n = -(-rpb // (256 // (c // epc))) + 256 // (c // epc) + -(-rows // rpb)
    else:
        n = 512 + -(-rows // 512)
    G, OUT = _Buf((rows,), c, dtype, content=g, ld=ld, off=coff), _Buf((1,), c)
    L.check(lib.din_colsum(G.ptr(), _code(L, dtype), rows, c, ld, coff, OUT.ptr(), None))
    torch.cuda.synchronize()
    assert OUT.untouched_outside() and G.unchanged()
    _check(f"colsum[{name}]", "column sums", OUT.get()[0], g.double().sum(0), (n + 1) * U32 * g.double().abs().sum(0))


FOLD_LAYERS = {"n1": (37,), "n4": (1, 255, 257, 3)}


def fold_reference(gamma, beta, mean, var, wdot, dshift):
    gamma, beta, mean, var, wdot, dshift = (v.double() for v in (gamma, beta, mean, var, wdot, dshift))
    s = gamma / (var + EPS).sqrt()
    rstd = 1 / (var + EPS).sqrt()
    return dict(scale=s, shift=beta - mean * s, dgamma=(wdot - dshift * mean) * rstd, dbeta=dshift,
                # scale: the add reaches the quotient halved by the root, the root and the division whole: 2.5 u at worst; dgamma: the
                # product and the subtraction 2 u, rstd 2.5 u, the last product u: 5.5 u at worst.  Both worst cases are nearly met among
                # 10^3 elements, where (n + 1) u would leave 1.6x and 1.3x: twice the worst case, so that no assert passes under 2x
                bars=dict(scale=5 * U32 * s.abs(), shift=6 * U32 * (beta.abs() + (mean * s).abs()),
                          dgamma=11 * U32 * (wdot.abs() + (dshift * mean).abs()) * rstd, dbeta=torch.zeros_like(s)))


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(FOLD_LAYERS))
def test_bn_fold_single_and_multi_against_fp64(env, case):
    """din_bn_fold / _bwd per layer and din_bn_fold_multi / _bwd_multi over all layers: each against float64, and the multi forms equal
    to the per-layer calls bit for bit (n4: the layer boundaries fall on, before and after a 256-thread block)"""
    lib, L, nhwc, ops = env
    sizes = FOLD_LAYERS[case]
    gen = _gen("fold" + case)
    total, offs = sum(sizes), np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    assert total % 256 != 0
    layers = [dict(gamma=torch.rand(s, generator=gen) + 0.5, beta=torch.randn(s, generator=gen), mean=torch.randn(s, generator=gen) * (1 + i),
                   var=torch.rand(s, generator=gen) * (i + 1) + 0.01) for i, s in enumerate(sizes)]
    wdot, dshift = torch.randn(total, generator=gen), torch.randn(total, generator=gen)
    bufs = [{k: _Buf((1,), s, content=l[k]) for k in l} for l, s in zip(layers, sizes)]
    WD, DS = _Buf((1,), total, content=wdot), _Buf((1,), total, content=dshift)
    single = {k: _Buf((1,), total) for k in ("scale", "shift", "dgamma", "dbeta")}
    for i, (b, s) in enumerate(zip(bufs, sizes)):
        o4 = int(offs[i]) * 4
        L.check(lib.din_bn_fold(b["gamma"].ptr(), b["beta"].ptr(), b["mean"].ptr(), b["var"].ptr(), EPS, single["scale"].ptr() + o4,
                                single["shift"].ptr() + o4, s, None))
        L.check(lib.din_bn_fold_bwd(WD.ptr() + o4, DS.ptr() + o4, b["mean"].ptr(), b["var"].ptr(), EPS, single["dgamma"].ptr() + o4,
                                    single["dbeta"].ptr() + o4, s, None))
    ptrs = torch.tensor([b[k].ptr() for b in bufs for k in ("gamma", "beta", "mean", "var")], dtype=torch.int64).cuda()
    OF = _Buf((1,), len(sizes) + 1, torch.int32, content=torch.from_numpy(offs))
    multi = {k: _Buf((1,), total) for k in ("scale", "shift", "dgamma", "dbeta")}
    L.check(lib.din_bn_fold_multi(ptrs.data_ptr(), OF.ptr(), len(sizes), total, EPS, multi["scale"].ptr(), multi["shift"].ptr(), None))
    L.check(lib.din_bn_fold_bwd_multi(ptrs.data_ptr(), OF.ptr(), len(sizes), total, EPS, WD.ptr(), DS.ptr(), multi["dgamma"].ptr(),
                                      multi["dbeta"].ptr(), None))
    torch.cuda.synchronize()
    cat = {k: torch.cat([l[k] for l in layers]) for k in layers[0]}
    want = fold_reference(cat["gamma"], cat["beta"], cat["mean"], cat["var"], wdot, dshift)
    assert _same(WD, DS, OF) and all(_same(*b.values()) for b in bufs)
    for k in ("scale", "shift", "dgamma", "dbeta"):
        assert single[k].untouched_outside() and multi[k].untouched_outside()
        _check(f"bn_fold[{case}]", k, single[k].get()[0], want[k], want["bars"][k])
        _check(f"bn_fold_multi[{case}]", k, multi[k].get()[0], want[k], want["bars"][k])
        assert torch.equal(single[k].bits(), multi[k].bits()), f"{case}: {k} of the multi form differs from the per-layer calls"


def _prep_np(v):
    y = v.astype(F32) / F32(255.0)
    y = y - F32(0.5)
    y = y * F32(2.0)
    assert y.dtype == F32
    return y


@pytest.mark.gpu
@pytest.mark.parametrize("cpad", [4, 8])
@pytest.mark.parametrize("out_dtype", [FP, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("u8", [1, 0], ids=["u8", "f32in"])
def test_prep_images_every_byte_value(env, u8, out_dtype, cpad):
    lib, L, nhwc, ops = env
    nb, h, w = 2, 8, 32                                           # 256 pixels a plane: every plane holds all 256 byte values, in another order
    rs = np.random.RandomState(5)
    img = np.stack([rs.permutation(256) for _ in range(nb * 3)]).reshape(nb, 3, h, w).astype(np.uint8)
    want = torch.zeros(nb, h, w, cpad)
    want[..., :3] = torch.from_numpy(_prep_np(img)).permute(0, 2, 3, 1)
    want = want.to(out_dtype)                                     # bf16: round to nearest even
    src = torch.from_numpy(img).cuda() if u8 else torch.from_numpy(img.astype(F32)).cuda()
    before = src.clone()
    OUT = _Buf((nb, h, w), cpad, out_dtype)
    L.check(lib.din_prep_images_nhwc(src.data_ptr(), u8, OUT.ptr(), _code(L, out_dtype), nb, h, w, cpad, None))
    torch.cuda.synchronize()
    assert OUT.untouched_outside() and torch.equal(src, before)
    assert torch.equal(_bits(OUT.get()), _bits(want)) and not bool(OUT.get()[..., 3:].float().abs().sum())
    if not u8 and out_dtype == FP and cpad == 4:
        X, Y = _Buf((1,), 256, content=torch.arange(256.0)), _Buf((1,), 256)
        L.check(lib.din_prep_images_f32(X.ptr(), Y.ptr(), 256, None))
        torch.cuda.synchronize()
        assert Y.untouched_outside() and X.unchanged() and torch.equal(_bits(Y.get()[0]), _bits(torch.from_numpy(_prep_np(np.arange(256)))))


@pytest.mark.gpu
def test_counter_add_masks_to_63_bits(env):
    lib, L, nhwc, ops = env
    top = (1 << 63) - 1
    for start, delta, want in ((7, 10, 17), (top - 4, 10, 5), (top, 1, 0), (3, (1 << 64) - 1, 2)):
        word = torch.tensor([-7777, start, -7777], dtype=torch.int64).cuda()
        L.check(lib.din_counter_add(word.data_ptr() + 8, delta, None))
        torch.cuda.synchronize()
        assert word.cpu().tolist() == [-7777, want, -7777] and want == (start + delta) & top


# =====================================================================================================================================
# the bars bite: every row (CPU)
# =====================================================================================================================================
BITE = ([(_bite_roi_fwd, (n, dt), f"roi-fwd-{n}-{'bf16' if dt == BF else 'fp32'}") for n in FWD_IDS for dt in (FP, BF)]
        + [(_bite_roi_bwd, (n,), "roi-bwd-" + n) for n in GATHER_IDS + SCATTER_IDS]
        + [(_bite_bn, c, "bn-" + i) for c, i in zip(BN_CASES, BN_IDS)])


@pytest.mark.parametrize("check,args", [b[:2] for b in BITE], ids=[b[2] for b in BITE])
def test_bars_bite(check, args):
    """every applicable wrong float64 variant of the row's reference misses one of the row's bars by >= 10x on the row's own inputs"""
    check(*args)
