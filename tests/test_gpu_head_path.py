"""Everything between RoIAlign and the loss of the DIN models -- csrc/din_walk.hip, layernorm.hip, context_encoding.hip, head.hip and the
stage-2 helpers of elementwise.hip -- called through the C ABI and compared with float64 references written here from the definition of
each operation, on the stored fp32 / bf16 operands.  The reference is never another kernel of this library.  Every destination lies in a
buffer with guard bands; where a stride exceeds the width the columns outside the view hold NaN; all of that must come back bit for bit,
NaN in unused source columns must not reach a result, sources are not written.  Integer and byte outputs (idx, argmax, footprints, casts,
layout changes) are compared exactly.  Outputs written with plain stores must repeat bit for bit on a second run; outputs that meet in
atomics (LayerNorm dgamma / dbeta, head dw / dbias, dot_accum, walk dx) are compared with their bar only.

Bars are per element, (n + 1) u sum|terms| with u = 2^-24 and n the rounded operations that reach the element, counted from the kernels:
  walk     a coefficient 1 - |p - c| is one rounding (p - c is exact: c is an integer below |p|'s binade limit); a corner term
           v * (wy * wx) then sees 2 + 1 + 1 and three adds: S_k (the `mad` output): n = 7, terms |v wy wx|.  a_k = softmax: logit - max
           (|logit| <= 2: at most 4 u in the argument), expf 2, the k2-term sum k2, the division 1: n = k2 + 5, terms a_k (1 / k2 without
           scale_factor: one rounding).  z = sum_k S_k a_k: 7 + (k2 + 5) + 1 + k2 adds: n = 2 k2 + 13, terms a_k |v wy wx|.
           dx: a_k (k2 + 5), * gz 1, the coefficient product 3, * 1, m atomic adds (m = corner hits of the cell, counted): n = k2 + 10 + m.
           d offset = a_k mask sum_corner <gz, P_corner> s w: product 1, the 64-lane tree 6, * s * w with its coefficient 3, three adds,
           a_k (k2 + 5), the mask and a_k 2, nch channel chunks: n = k2 + 20 + nch, terms a_k |w| sum_ch |gz v|.
           d logit = a_k (dA_k - sum_j a_j dA_j), dA_k = <gz, S_k>: dA 7 + 1 + 6 + nch; the dot over k2 k2 + 9 with a_j (k2 + 5) in it, the
           difference and a_k (k2 + 5) + 2: n = 3 k2 + 35 + nch, terms a_k (|dA|_k + sum_j a_j |dA|_j), |dA|_k = sum_ch |gz| sum_c |v w|.
           The sampling position is computed in fp32 exactly as the kernel documents ((float)(integer base) + offset, one numpy float32
           add) and only then widened, so floor, clamp, sign and mask decisions cannot differ by rounding: idx is exact and no element is
           skipped in any row.
  LN       D = ceil(len / 512) + 16 is the depth of a row reduction (per-thread trips, the 4-vector, 6 tree levels, 8 waves).
           mean: (D + 1) u mean|h|, h = x + res.  rstd: the sum of squares D + 3, / len, + eps 2, sqrt halves that, the division 1:
           (D + 8) u rstd bounds it.  y: the mean's error times rstd |gamma|, then (h - mean) rstd gamma + beta, ReLU, keep-scale (1 - p
           and the division 2): u (((D + 1) mean|h| + [res] |h|) rstd |gamma| + (D + 14) |xhat gamma| + 2 |beta|) / (1 - p) where the
           mask keeps; under dropout 5 |beta| (the product with the keep-scale and the scale's two roundings reach beta too); [res]: x + res
           is itself a rounded add of h's size.  The backward is fed stats and y of the reference rounded to fp32 and its reference reads
           those stored values, so the ReLU / dropout decisions and the statistics are common to both.
           dbeta += sum_r g: g 3 (dy * keep-scale), A = rows (atomics) or min(rows, 32) + ceil(rows / 32) adds: (A + 4) u (sum|g| + |prior|).
           dgamma += sum_r g xhat: xhat is off by u ([res] 2 |h| rstd + 4 |xhat|) per row, the product 1: (A + 5) u (sum|g xhat| + |prior|).
           dx = rstd (g gamma - m1 - xhat m2) subtracts two reductions: the yard rule, max(4 yard, floor), yard = the row's worst |fp32 torch
           - fp64 torch| of the same expression, floor (D + 6) u rstd (|g gamma| + mean|g gamma| + |xhat| mean|g gamma xhat|).
  ctx      scores: 4 products and 3 adds per 4-vector, c / 4 accumulations: (c / 4 + 5) u sum|q k|.  softmax: the argument x - max is off by
           |x - max| u, expf 2; the row sum Z inherits sum_j a_j (|x_j - max| + 2) u from its terms and adds L + 10 = ceil(len / 256) + 10 of its own;
           reciprocal and product 2: (2 |x - max| + sum_j a_j |x_j - max| + L + 17) u a + 2^-126 (fp32 underflow; 2 |x - max|: see there).
           softmax backward: the yard rule with floor (L + 13) u a (|da| + sum|a da|).  apply: G = 256 / c pixel groups, ceil(p / G) adds per
           group, G to join them: (ceil(p / G) + G + 2) u sum|a kf|.  keys grad: 2 n products and adds: (2 n + 2) u sum(|a dctx| + |ds q|).
           Each entry point reads the previous stage's float64 result rounded to fp32, which is also what its reference reads.
  head     frame score: ceil(c / 256) + 6 + 4 + 2, the mean over t t + 1: (ceil(c / 256) + t + 14) u mean_t(sum_c |pooled w| + |bias|).
           ds = sum_j (dscores_j / t) w_j at the arg-max: (a + 4) u sum_j |dscores_j w_j| / t, exactly 0 elsewhere.  dw, dbias: b t atomic
           adds: (b t + 4) u (sum |dscores pooled| / t + |prior|).
  helpers  axpby 4 u (|a x| + |b y|); scale_by_param 4 u (|prior| + |x s|) (three / two roundings whose sum is at most half of that:
           over 10^3..10^6 elements the worst case is nearly met, and no assert here may pass under 2x); dot_accum: 3 trips, the 6-level tree and 2048 waves meeting
           in one word: 2060 u (sum|x y| + |prior|); Adam: m 6 u, v 11 u of their terms, p from those through sqrt, the two bias
           corrections (1 - beta^step computed in fp32: its cancellation error 2 u beta^step / (1 - beta^step) is part of the bar) and the
           division; casts, layout changes, masks, add_position and dropout given its mask are exact.
test_bars_bite (CPU) shows for every row and mode that each applicable wrong float64 variant misses a bar by >= 10x;
test_walk_reference_matches_oracle (CPU) ties the walk restatement to oracle.din_oracle in float64."""
import ctypes as C
import functools
import math
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.conftest import Measured
from tests.test_gpu_kernels import env  # noqa: F401  (the module-scoped library fixture)

U32, U16 = 2.0 ** -24, 2.0 ** -8
NG = 64                                   # guard elements on each side of every buffer
BF, FP = torch.bfloat16, torch.float32
_INT = {torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.int32: torch.int32, torch.uint8: torch.uint8}


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _bits(t):
    return t.contiguous().view(_INT[t.dtype])


def _ratio(got, want, bar):
    """worst |got - want| / bar over the elements (0 where they agree exactly, so a zero bar asks for equality); NaN if got holds one"""
    diff = (got.double() - want.double()).abs()
    if diff.numel() == 0:
        return 0.0
    return float(torch.where(diff == 0, torch.zeros_like(diff), diff / bar).max())


def _lib():
    from din_amd import _lib as L
    return L.load(), L


class _Buf:
    """a device array [*lead][ld] between two guard bands; columns [off, off + c) hold `content` (poison when None), every other column
    of the stride poison: NaN (integers: -5555); guards -1234.5 (integers: -7777)"""

    def __init__(self, lead, c, dtype=FP, content=None, ld=None, off=0):
        lead, ld = tuple(lead), ld or c
        n = int(np.prod(lead)) * ld
        guard, poison = (-1234.5, float("nan")) if dtype.is_floating_point else (-7777, -5555)
        host = torch.full((n + 2 * NG,), guard, dtype=dtype)
        body = host[NG:NG + n].view(*lead, ld)
        body[:] = poison
        if content is not None:
            body[..., off:off + c] = content.to(dtype).reshape(*lead, c)
        self.flat = host.cuda()
        self.body = self.flat[NG:NG + n].view(*lead, ld)
        self.view = self.body[..., off:off + c]
        self.before = _bits(host).clone()
        self.outside = torch.ones(n + 2 * NG, dtype=torch.bool)
        self.outside[NG:NG + n].view(*lead, ld)[..., off:off + c] = False

    def ptr(self):
        return self.body.data_ptr()

    def get(self):
        return self.view.cpu()

    def bits(self):
        return _bits(self.flat).cpu()

    def untouched_outside(self):
        return torch.equal(self.bits()[self.outside], self.before[self.outside])

    def unchanged(self):
        return torch.equal(self.bits(), self.before)


def _all_outside(*bufs):
    return all(b is None or b.untouched_outside() for b in bufs)


def _all_unchanged(*bufs):
    return all(b is None or b.unchanged() for b in bufs)


def _check(name, what, got, want, bar):
    worst = Measured(_ratio(got, want, bar))
    print(f"{name} {what}: worst |err| / bar = {float(worst):.3g}")
    assert worst <= 1.0, f"{name}: {what} is {float(worst):.3g} x its bar"


def _refused(rc, needle):
    lib, L = _lib()
    assert rc < 0, rc
    msg = lib.din_last_error_string().decode()
    assert needle in msg, (needle, msg)


# =====================================================================================================================================
# 1. dynamic walk
# =====================================================================================================================================
K33 = (2, 3, 5, 64, 3, 3, 1)


def _w(name, shape, scale=1, plain=0, cp_extra=0, mat=None, npc=None, mad=False, salt=0):
    return dict(name=name, shape=shape, scale=scale, plain=plain, cp_extra=cp_extra, mat=mat, npc=npc, mad=mad, salt=salt)


WALK_ROWS = [
    _w("k33", K33, mad=True),
    _w("c32", (2, 2, 4, 32, 3, 3, 1)),
    _w("c96", (1, 3, 5, 96, 3, 3, 1)),
    _w("c200", (1, 2, 3, 200, 3, 3, 2)),
    _w("k13", (2, 3, 6, 64, 1, 3, 1)),
    _w("k31", (2, 3, 6, 64, 3, 1, 1)),
    _w("k55r2_big", (1, 10, 12, 64, 5, 5, 2)),
    _w("k77", (1, 4, 8, 64, 7, 7, 1)),
    _w("one_pos", (3, 1, 1, 64, 3, 3, 1), salt=18),     # (27 taps in all: a mixture draw under which two of the clips' taps meet the one cell with features)
    _w("t10n12", (1, 10, 12, 128, 3, 3, 1)),
    _w("noscale", K33, scale=0),
    _w("padded_cp", K33, cp_extra=5),
    _w("plain_k33", K33, plain=1, mad=True),
    _w("plain_k55r2", (1, 4, 6, 64, 5, 5, 2), plain=1),
    _w("clamp_small", K33, scale=0, mat=(2, 3)),         # person_mat_shape below the grid: clamp maxima inside the padded map
    _w("clamp_large", K33, scale=0, mat=(10, 12)),       # ... above it: the position may pass the last index by several cells
    _w("npc", (4, 3, 7, 96, 3, 3, 1), npc=(7, 1, 4, 2)),
]
WALK_IDS = [r["name"] for r in WALK_ROWS]
WALK_WRONG = ("swap_lb_rt", "clamp_hp", "trunc", "lattice", "widest", "open", "sign0", "no_dot")
COMPONENTS = ("zero", "unit_or_half", "uniform", "below", "above", "on_limit", "on_zero")


def _walk_geom(row):
    b, t, n, c, kh, kw, ratio = row["shape"]
    k2 = kh * kw
    pt, pl = (kh - 1) // 2 * ratio, (kw - 1) // 2 * ratio
    clamp = None
    if row["mat"]:                                                # parallel_infer's maxima from person_mat_shape (:307-317)
        tm, nm = row["mat"]
        clamp = (tm + 2 * ratio - 1, nm + 2 * ratio - 1, tm + 2 * ratio, nm + 2 * ratio)
    return dict(b=b, t=t, n=n, c=c, kh=kh, kw=kw, ratio=ratio, k2=k2, pt=pt, pl=pl, hp=t + 2 * pt, wp=n + 2 * pl, clamp=clamp,
                ncols=(3 if row["scale"] else 2) * k2, cp=(3 if row["scale"] else 2) * k2 + row["cp_extra"], nch=(c + 63) // 64)


def _walk_base(t, n, kh, kw, ratio, shift=0):
    """pos_0 + pos_k of every (frame, tap) and (actor, tap): small integers ([t][k2], [n][k2]); shift = 1: the lattice starts one cell late"""
    pt, pl = (kh - 1) // 2 * ratio, (kw - 1) // 2 * ratio
    ky0, kx0 = (-((kh - 1) * ratio)) // 2 + shift, (-((kw - 1) * ratio)) // 2 + shift
    k = np.arange(kh * kw)
    by = pt + np.arange(t)[:, None] + ky0 + (k // kw)[None, :] * ratio
    bx = pl + np.arange(n)[:, None] + kx0 + (k % kw)[None, :] * ratio
    return by.astype(np.float64), bx.astype(np.float64)


@functools.lru_cache(maxsize=None)
def _walk_operands(name):
    """x, pred (offsets from the mixture, logits in (-2, 2)), gz of a row as stored fp32 tensors, and the component counts"""
    row = WALK_ROWS[WALK_IDS.index(name)]
    g = _walk_geom(row)
    b, t, n, c, k2 = g["b"], g["t"], g["n"], g["c"], g["k2"]
    gen = _gen("walk_" + name)
    rs = np.random.RandomState((zlib.crc32(name.encode()) + row["salt"]) & 0x7FFFFFFF)
    by, bx = _walk_base(t, n, g["kh"], g["kw"], g["ratio"])
    limit_y = g["clamp"][2] if g["clamp"] else g["hp"] - 1
    counts = {}
    off = np.zeros((b, t, n, 2 * k2), dtype=np.float32)
    for axis in (0, 1):
        comp = (rs.permutation(b * t * n * k2) % len(COMPONENTS)).reshape(b, t, n, k2)
        base = np.broadcast_to(by[None, :, None, :] if axis == 0 else bx[None, None, :, :], (b, t, n, k2))
        nb = np.asarray(row["npc"] or [n] * b)[:, None, None, None]
        limit = np.broadcast_to(limit_y if axis == 0 else (g["clamp"][3] if g["clamp"] else nb + 2 * g["pl"] - 1), (b, t, n, k2))
        unit = rs.choice([1.0, -1.0, 0.5, -0.5], size=comp.shape)
        uni = rs.uniform(-1.5, 1.5, size=comp.shape)
        v = np.select([comp == 0, comp == 1, comp == 2, comp == 3, comp == 4, comp == 5, comp == 6],
                      [0.0 * uni, unit, uni, -40.25 + 0 * uni, 40.25 + 0 * uni, limit - base, -base])
        off[..., axis * k2:(axis + 1) * k2] = v.astype(np.float32)
        for i, cname in enumerate(COMPONENTS):
            counts[(axis, cname)] = int((comp == i).sum())
    x = torch.randn(b, t, n, c, generator=gen)
    logits = torch.rand(b, t, n, k2, generator=gen) * 4 - 2
    pred = torch.cat([torch.from_numpy(off), logits], dim=3)[..., :g["ncols"]].contiguous()
    gz = torch.randn(b, t, n, c, generator=gen)
    return dict(x=x, pred=pred, gz=gz, counts=counts)


def _walk_positions(offsets, row):
    """the sampling positions as the kernel documents them: (float)(integer base) + offset, ONE fp32 add; plain: the lattice itself"""
    g = _walk_geom(row)
    by, bx = _walk_base(g["t"], g["n"], g["kh"], g["kw"], g["ratio"])
    k2 = g["k2"]
    off = offsets.numpy().astype(np.float32) * (0 if row["plain"] else 1)
    py0 = by.astype(np.float32)[None, :, None, :] + off[..., :k2]
    px0 = bx.astype(np.float32)[None, None, :, :] + off[..., k2:]
    assert py0.dtype == np.float32 and px0.dtype == np.float32
    return py0, px0


def _soft_abs(v, sign0):
    return v.abs() + ((v - v.detach()) * (v.detach() == 0) if sign0 else 0)


def _soft_clamp(p0, hi, open_interval):
    if not open_interval:
        return p0.clamp(0, hi)                                   # torch: gradient passes on the closed interval
    inside = (p0.detach() > 0) & (p0.detach() < hi)
    return p0.detach().clamp(0, hi) + (p0 - p0.detach()) * inside


def walk_reference(x, py0, px0, logits, shape, scale=1, plain=0, clamp=None, npc=None, gz=None, wrong=None):
    """float64 restatement of dynamic_infer_ratio / plain_infer_ratio / the walk half of parallel_infer (dynamic_infer_module.py:154-341)
    from sampling positions py0, px0 [b][t][n][k2] (any float type, widened exactly).  Every clip runs on its own [T, n_b, C] slice.
    Returns z, a, idx, mad, the sums of |terms| behind them and, with gz, dx / d offset-y / d offset-x / d logits and theirs."""
    b, t, n, c, kh, kw, ratio = shape
    k2 = kh * kw
    pt, pl = (kh - 1) // 2 * ratio, (kw - 1) // 2 * ratio
    hp, wp = t + 2 * pt, n + 2 * pl
    by, bx = (torch.from_numpy(v) for v in _walk_base(t, n, kh, kw, ratio))
    wby, wbx = (torch.from_numpy(v) for v in _walk_base(t, n, kh, kw, ratio, int(wrong == "lattice")))
    x = x.detach().double().clone().requires_grad_(True)
    # the offset as a float64 leaf: the rounded position minus its integer base (exact), so that base + leaf IS the fp32 position
    oy = (torch.from_numpy(np.asarray(py0, dtype=np.float64)) - by[None, :, None, :]).requires_grad_(True)
    ox = (torch.from_numpy(np.asarray(px0, dtype=np.float64)) - bx[None, None, :, :]).requires_grad_(True)
    lg = logits.detach().double().clone().requires_grad_(True) if scale else None
    agz = gz.double().abs() if gz is not None else None
    keys = ("z", "a", "idx", "mad", "z_abs", "mad_abs", "lin_abs", "cnt", "doy_abs", "dox_abs", "dlg_abs")
    out = {k: [] for k in keys}
    for bi in range(b):
        nb = int(npc[bi]) if npc is not None else n
        wpc = (n if wrong == "widest" else nb) + 2 * pl
        hy, hx = (hp, wpc) if wrong == "clamp_hp" else (hp - 1, wpc - 1)
        phy, phx = hy, hx
        if clamp is not None:
            hy, hx, phy, phx = min(clamp[0], hp - 1), min(clamp[1], wp - 1), clamp[2], clamp[3]
        # two spare rows / columns of zeros: the wrong clamp and lattice variants index one cell outside the padded grid
        tile = F.pad(x[bi, :, :nb], (0, 0, pl, wp + 2 - pl - nb, pt, hp + 2 - pt - t))
        atile = tile.detach().abs()
        py0b, px0b = wby[:, None, :] + oy[bi, :, :nb], wbx[None, :nb, :] + ox[bi, :, :nb]
        rnd = torch.trunc if wrong == "trunc" else torch.floor
        fy, fx = rnd(py0b.detach()), rnd(px0b.detach())
        ly, ry, lx, rx = fy.clamp(0, hy), (fy + 1).clamp(0, hy), fx.clamp(0, hx), (fx + 1).clamp(0, hx)

        def fetch(src, cy, cx):
            return src[cy.long(), cx.long()]                     # [t][nb][k2][c]

        if plain:                                                # the feature at the lattice point itself: no clamp, no coefficients
            ry, rx = ly, lx
            cy, cx = wby[:, None, :].expand(t, nb, k2), wbx[None, :nb, :].expand(t, nb, k2)
            one = torch.ones(t, nb, k2, dtype=torch.float64)
            taps = [(cy, cx, one, one)]
        else:
            py, px = _soft_clamp(py0b, phy, wrong == "open"), _soft_clamp(px0b, phx, wrong == "open")
            wy_l, wy_r = 1 - _soft_abs(py - ly, wrong == "sign0"), 1 - _soft_abs(py - ry, wrong == "sign0")
            wx_l, wx_r = 1 - _soft_abs(px - lx, wrong == "sign0"), 1 - _soft_abs(px - rx, wrong == "sign0")
            lb, rt = ((ly, rx), (ry, lx)) if wrong == "swap_lb_rt" else ((ry, lx), (ly, rx))
            taps = [(ly, lx, wy_l, wx_l), (ry, rx, wy_r, wx_r), (*lb, wy_r, wx_l), (*rt, wy_l, wx_r)]   # no de-dup (:255-258)
        S = sum(fetch(tile, cy, cx) * (wy * wx).unsqueeze(-1) for cy, cx, wy, wx in taps)
        wabs = [(wy * wx).detach().abs() for _, _, wy, wx in taps]
        Sabs = sum(fetch(atile, cy, cx) * w.unsqueeze(-1) for (cy, cx, _, _), w in zip(taps, wabs))
        if scale:
            l = lg[bi, :, :nb]
            if wrong == "no_dot":                                # d a_k / d l_j = delta_kj a_k: the backward loses sum_j a_j dA_j
                e = torch.exp(l - l.detach().max(-1, keepdim=True).values)
                a = e / e.detach().sum(-1, keepdim=True)
            else:
                a = torch.softmax(l, dim=-1)
        else:
            a = torch.full((t, nb, k2), 1.0 / k2, dtype=torch.float64)
        ad = a.detach()
        padn = (0, 0, 0, n - nb)
        out["z"].append(F.pad((S * a.unsqueeze(-1)).sum(2), padn))
        out["z_abs"].append(F.pad((Sabs * ad.unsqueeze(-1)).sum(2), padn))
        out["a"].append(F.pad(ad, padn))
        out["idx"].append(F.pad(torch.stack([ly, ry, lx, rx], dim=-1).long(), (0, 0, 0, 0, 0, n - nb)))
        out["mad"].append(F.pad(S, (0, 0, 0, 0, 0, n - nb)))
        out["mad_abs"].append(F.pad(Sabs, (0, 0, 0, 0, 0, n - nb)))
        if gz is None:
            continue
        ag = agz[bi, :, :nb]
        out["lin_abs"].append((sum(fetch(tile, cy, cx) * w.unsqueeze(-1) for (cy, cx, _, _), w in zip(taps, wabs))
                               * ad.unsqueeze(-1) * ag.unsqueeze(2)).sum())
        out["cnt"].append(sum(fetch(tile, cy, cx) for cy, cx, _, _ in taps).sum())
        G = [(ag.unsqueeze(2) * fetch(atile, cy, cx)).sum(-1) for cy, cx, _, _ in taps]
        zero = torch.zeros(t, nb, k2, dtype=torch.float64)
        out["doy_abs"].append(F.pad(zero if plain else ad * sum(Gc * wx.detach().abs() for Gc, (_, _, _, wx) in zip(G, taps)), padn))
        out["dox_abs"].append(F.pad(zero if plain else ad * sum(Gc * wy.detach().abs() for Gc, (_, _, wy, _) in zip(G, taps)), padn))
        dA = (ag.unsqueeze(2) * Sabs).sum(-1)
        out["dlg_abs"].append(F.pad(ad * (dA + (ad * dA).sum(-1, keepdim=True)), padn))
    res = {k: torch.stack(out[k]) for k in ("z", "a", "idx", "mad", "z_abs", "mad_abs")}
    res["valid"] = torch.stack([torch.arange(n) < (int(npc[bi]) if npc is not None else n) for bi in range(b)])[:, None, :].expand(b, t, n)
    if gz is not None:
        leaves = [x, oy, ox] + ([lg] if scale else [])
        grads = torch.autograd.grad((res["z"] * gz.double()).sum(), leaves, allow_unused=True, retain_graph=True)
        grads = [torch.zeros_like(l) if gr is None else gr for gr, l in zip(grads, leaves)]
        res["dx"], res["doy"], res["dox"] = grads[:3]
        res["dlg"] = grads[3] if scale else None
        res["dx_abs"] = torch.autograd.grad(sum(out["lin_abs"]), x, retain_graph=True)[0]
        res["dx_cnt"] = torch.autograd.grad(sum(out["cnt"]), x)[0]
        for k in ("doy_abs", "dox_abs", "dlg_abs"):
            res[k] = torch.stack(out[k])
    return {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in res.items()}


def _walk_bars(r, k2, nch, scale, has_grad=True):
    bars = dict(mad=8 * U32 * r["mad_abs"], a=(k2 + 6) * U32 * r["a"], z=(2 * k2 + 14) * U32 * r["z_abs"])
    if has_grad:
        bars.update(dx=(k2 + 11 + r["dx_cnt"]) * U32 * r["dx_abs"], doy=(k2 + 21 + nch) * U32 * r["doy_abs"],
                    dox=(k2 + 21 + nch) * U32 * r["dox_abs"])
        if scale:
            bars["dlg"] = (3 * k2 + 36 + nch) * U32 * r["dlg_abs"]
    return bars


@functools.lru_cache(maxsize=None)
def _walk_expected(name, wrong=None):
    row = WALK_ROWS[WALK_IDS.index(name)]
    o, g = _walk_operands(name), _walk_geom(row)
    py0, px0 = _walk_positions(o["pred"][..., :2 * g["k2"]], row)
    lg = o["pred"][..., 2 * g["k2"]:3 * g["k2"]] if row["scale"] else None
    return walk_reference(o["x"], py0, px0, lg, row["shape"], row["scale"], row["plain"], g["clamp"], row["npc"], o["gz"], wrong)


def _walk_applies(row, wrong):
    if wrong == "lattice":
        return True
    if row["plain"]:
        return False
    g = _walk_geom(row)
    return {"widest": row["npc"] is not None, "no_dot": bool(row["scale"]), "clamp_hp": row["mat"] is None,
            # a position exactly on a clamp limit has both corners in the zero padding once the padding is two cells deep on both
            # axes: its offset gradient is 0 whichever interval the mask uses
            "open": min(g["pt"], g["pl"]) <= 1,
            # one position per clip: only the centre of the 3 x 3 padded grid holds features, and an integer position weights it with a
            # coefficient whose sign(0) matters only if both axes drew one
            "sign0": g["t"] * g["n"] > 1}.get(wrong, True)


def _walk_outputs(row):
    return ("z", "a", "mad", "dx", "doy", "dox") + (("dlg",) if row["scale"] else ())


def test_walk_rows_carry_every_component():
    """every component of the offset mixture occurs on both axes of every row (the four sides of the padded grid: below / above on y
    and on x), and the positions it promises are what the fp32 add produces: exact integers, exact clamp limits, exact zero"""
    for row in WALK_ROWS:
        o, g = _walk_operands(row["name"]), _walk_geom(row)
        for key, count in o["counts"].items():
            assert count >= 1, (row["name"], key)
        py0, px0 = _walk_positions(o["pred"][..., :2 * g["k2"]], dict(row, plain=0))
        limit = g["clamp"][2] if g["clamp"] else g["hp"] - 1
        assert (py0 == limit).any() and (py0 == 0).any() and (px0 == 0).any() and (py0 < -1).any() and (py0 > limit + 1).any()
        assert (py0 == np.floor(py0)).mean() > 0.3 and (py0 != np.floor(py0)).mean() > 0.1
        want = _walk_expected(row["name"])                       # ... and every clip has taps that meet features, with gradients behind them
        hit = lambda k: 2 * int((want[k].flatten(1).abs().amax(1) > 0).sum()) >= want[k].shape[0]      # noqa: E731
        assert hit("mad_abs") and (row["plain"] or (hit("doy") and hit("dox"))), row["name"]


def _bite_walk(name):
    row = WALK_ROWS[WALK_IDS.index(name)]
    g = _walk_geom(row)
    want = _walk_expected(name)
    bars = _walk_bars(want, g["k2"], g["nch"], row["scale"])
    assert all(bool(torch.isfinite(want[k]).all()) for k in _walk_outputs(row))
    tried = 0
    for wrong in WALK_WRONG:
        if not _walk_applies(row, wrong):
            continue
        tried += 1
        bad = _walk_expected(name, wrong)
        worst = max(_ratio(bad[k], want[k], bars[k]) for k in _walk_outputs(row))
        if not torch.equal(bad["idx"][want["valid"]], want["idx"][want["valid"]]):
            worst = float("inf")                                  # (idx is compared exactly)
        assert worst >= 10.0, f"{name}: the bars do not see '{wrong}' ({worst:.3g})"
    assert tried >= 1


@pytest.mark.parametrize("kernel,ratio", [((3, 3), 1), ((5, 5), 2), ((1, 3), 1), ((3, 1), 2), ((7, 7), 1)])
def test_walk_reference_matches_oracle(kernel, ratio):
    """the restatement above against oracle.din_oracle in float64, on the offsets the oracle's own convs produce: z and S to 1e-12
    relative, corner indices exactly -- lattice start, padding, clamp limits and corner association are the reference project's"""
    from oracle import din_oracle as O
    gen = _gen(f"oracle{kernel}{ratio}")
    b, t, n, c = 2, 4, 6, 16
    kh, kw = kernel
    k2 = kh * kw
    x = torch.randn(b, t, n, c, generator=gen, dtype=torch.float64)
    pw = torch.randn(2 * k2, c, kh, kw, generator=gen, dtype=torch.float64) * 0.3
    pb = torch.randn(2 * k2, generator=gen, dtype=torch.float64) * 4
    sw = torch.randn(k2, c, kh, kw, generator=gen, dtype=torch.float64) * 0.1
    sb = torch.randn(k2, generator=gen, dtype=torch.float64)
    shape = (b, t, n, c, kh, kw, ratio)
    pt, pl = (kh - 1) // 2 * ratio, (kw - 1) // 2 * ratio
    by, bx = _walk_base(t, n, kh, kw, ratio)
    z_o, s_o, aux = O.din_ratio_forward(x, pw, pb, sw, sb, kernel, ratio, want_aux=True)
    off = aux["offset"].numpy()
    py0, px0 = by[None, :, None, :] + off[..., :k2], bx[None, None, :, :] + off[..., k2:]
    assert (py0 < 0).any() and (px0 < 0).any() and (py0 > t + 2 * pt - 1).any() and (px0 > n + 2 * pl - 1).any()   # clamps on each side
    logits = F.conv2d(x.permute(0, 3, 1, 2), sw, sb, padding=(pt, pl), dilation=ratio).permute(0, 2, 3, 1)

    def close(got, want):
        return float((got - want).abs().max() / want.abs().max()) <= 1e-12

    mine = walk_reference(x, py0, px0, logits, shape)
    assert close(mine["z"], z_o) and close(mine["mad"], s_o) and close(mine["a"], aux["a"])
    assert torch.equal(mine["idx"], torch.stack([aux["ly"], aux["ry"], aux["lx"], aux["rx"]], dim=-1).long())
    z_o2, s_o2 = O.din_ratio_forward(x, pw, pb, None, None, kernel, ratio)
    assert close(walk_reference(x, py0, px0, None, shape, scale=0)["z"], z_o2)
    plain = walk_reference(x, by[None, :, None, :] + 0 * py0, bx[None, None, :, :] + 0 * px0, logits, shape, plain=1)
    assert close(plain["z"], O.din_plain_ratio_forward(x, sw, sb, kernel, ratio))
    for mat in ((2, 3), (10, 12)):
        clamp = (mat[0] + 2 * ratio - 1, mat[1] + 2 * ratio - 1, mat[0] + 2 * ratio, mat[1] + 2 * ratio)
        walk = walk_reference(x, py0, px0, None, shape, scale=0, clamp=clamp)
        assert close(plain["z"] + walk["z"], O.din_parallel_ratio_forward(x, pw, pb, sw, sb, kernel, ratio, mat))


def _dummy():
    return C.c_void_p(4096)                                       # a non-null pointer no refused call may touch


def test_walk_refusals():
    """host-only: every one of these returns DIN_E_ARG with its message before anything is launched"""
    lib, L = _lib()
    d, cl, nul = _dummy(), (C.c_int32 * 4)(3, 4, 4, 5), None

    def fwd(cp=27, t=3, n=5, kh=3, kw=3, scale=1, plain=0, clamp=nul, npc=nul, x=d):
        return lib.din_walk_fwd(x, d, cp, 2, t, n, 64, kh, kw, 1, scale, plain, clamp, npc, d, d, d, nul, nul)

    def bwd(cp=27, t=3, n=5, kh=3, kw=3, scale=1, plain=0, clamp=nul, npc=nul, dx=d):
        return lib.din_walk_bwd(d, d, cp, d, d, 2, t, n, 64, kh, kw, 1, scale, plain, clamp, npc, dx, d, d, nul)

    for call in (fwd, bwd):
        _refused(call(cp=192, kh=8, kw=8), "taps unsupported")
        _refused(call(cp=26), "stride too small")
        _refused(call(clamp=cl, npc=d), "mutually exclusive")
        _refused(call(t=40, n=40), "too large")
        _refused(call(cp=12, kh=2, kw=2, plain=1), "odd ST kernel")
        _refused(call(cp=18, kh=3, kw=2, plain=1), "odd ST kernel")
    _refused(fwd(x=nul), "null pointer")
    _refused(bwd(dx=nul), "null pointer")
    assert fwd(cp=18, scale=0, clamp=(C.c_int32 * 4)(3, 4, -1, 5)) < 0


BWD_SETTINGS = (("1", None), ("0", None), (None, "1"), ("0", "1"))   # (DIN_WALK_BWD_GLOBAL, DIN_WALK_BWD_GROUPS)


@pytest.mark.gpu
@pytest.mark.parametrize("name", WALK_IDS)
def test_walk_against_fp64(env, name, monkeypatch):
    lib, L, nhwc, ops = env
    row = WALK_ROWS[WALK_IDS.index(name)]
    g, o, want = _walk_geom(row), _walk_operands(name), _walk_expected(name)
    b, t, n, c, kh, kw, ratio, k2, cp, ncols, nch = (g[k] for k in ("b", "t", "n", "c", "kh", "kw", "ratio", "k2", "cp", "ncols", "nch"))
    bars = _walk_bars(want, k2, nch, row["scale"])
    valid = want["valid"]
    X, P, GZ = _Buf((b, t, n), c, content=o["x"]), _Buf((b, t, n), ncols, content=o["pred"], ld=cp), _Buf((b, t, n), c, content=o["gz"])
    cl = (C.c_int32 * 4)(*g["clamp"]) if g["clamp"] else None
    npc = torch.tensor(row["npc"], dtype=torch.int32).cuda() if row["npc"] else None
    npc_ptr = npc.data_ptr() if npc is not None else None

    def forward():
        Z, A, I = _Buf((b, t, n), c), _Buf((b, t, n), k2), _Buf((b, t, n, k2), 4, torch.int32)
        M = _Buf((b, t, n, k2), c) if row["mad"] else None
        L.check(lib.din_walk_fwd(X.ptr(), P.ptr(), cp, b, t, n, c, kh, kw, ratio, row["scale"], row["plain"], cl, npc_ptr, Z.ptr(), A.ptr(),
                                 I.ptr(), M.ptr() if M else None, None))
        torch.cuda.synchronize()
        return Z, A, I, M

    Z, A, I, M = forward()
    assert _all_outside(Z, A, I, M) and _all_unchanged(X, P), f"{name}: wrote outside a destination or into a source"
    _check(name, "z", Z.get(), want["z"], bars["z"])
    _check(name, "a", A.get()[valid], want["a"][valid], bars["a"][valid])
    bad = (I.get().long()[valid] != want["idx"][valid]).nonzero()
    assert bad.numel() == 0, f"{name}: {bad.shape[0]} corner indices differ, first at {bad[0].tolist()}"
    if row["plain"]:
        got = I.get()
        assert torch.equal(got[..., 0], got[..., 1]) and torch.equal(got[..., 2], got[..., 3])
    if M:
        _check(name, "mad", M.get(), want["mad"], bars["mad"])
    Z2, A2, I2, M2 = forward()
    assert all(torch.equal(u.bits(), v.bits()) for u, v in ((Z, Z2), (A, A2), (I, I2)) + (((M, M2),) if M else ())), f"{name}: rerun differs"

    a_saved = torch.where(valid.unsqueeze(-1), want["a"], torch.full_like(want["a"], 1.0 / k2)).float()
    AS = _Buf((b, t, n), k2, content=a_saved)
    first = None
    for glob, groups in BWD_SETTINGS:
        for opt, val in (("DIN_WALK_BWD_GLOBAL", glob), ("DIN_WALK_BWD_GROUPS", groups)):
            if val is not None:
                monkeypatch.setenv(opt, val)
            else:
                L.set_option(opt, None)
        DX, DP = _Buf((b, t, n), c), _Buf((b, t, n), ncols, ld=cp)
        scratch = torch.full((nch * b * t * n * 3 * k2,), float("nan")).cuda()
        L.check(lib.din_walk_bwd(X.ptr(), P.ptr(), cp, AS.ptr(), GZ.ptr(), b, t, n, c, kh, kw, ratio, row["scale"], row["plain"], cl, npc_ptr,
                                 DX.ptr(), DP.ptr(), scratch.data_ptr(), None))
        torch.cuda.synchronize()
        tag = f"{name}[global={glob},groups={groups}]"
        assert _all_outside(DX, DP) and _all_unchanged(X, P, AS, GZ), f"{tag}: wrote outside a destination or into a source"
        _check(tag, "dx", DX.get(), want["dx"], bars["dx"])
        dp = DP.get()
        _check(tag, "d offset-y", dp[..., :k2], want["doy"], bars["doy"])
        _check(tag, "d offset-x", dp[..., k2:2 * k2], want["dox"], bars["dox"])
        if row["scale"]:
            _check(tag, "d logits", dp[..., 2 * k2:], want["dlg"], bars["dlg"])
        if row["plain"]:
            assert not bool(dp[..., :2 * k2].any()), f"{tag}: plain mode gave an offset a gradient"
        if row["npc"]:
            assert not bool(DX.get()[~valid].any()) and not bool(dp[~valid].any()), f"{tag}: a padding actor received a gradient"
        first = first if first is not None else DP.bits()
        assert torch.equal(DP.bits(), first), f"{tag}: dpred (plain stores) differs between launch shapes"


@pytest.mark.gpu
def test_walk_autograd_wrapper(env):
    """ops.DynamicWalkFunction sizes the scratch and zeroes dpred itself: the padded_cp row through it (NaN in the unused pred columns,
    exact zeros in dpred's)"""
    lib, L, nhwc, ops = env
    name = "padded_cp"
    row = WALK_ROWS[WALK_IDS.index(name)]
    g, o, want = _walk_geom(row), _walk_operands(name), _walk_expected(name)
    k2 = g["k2"]
    bars = _walk_bars(want, k2, g["nch"], 1)
    pred = torch.full((g["b"], g["t"], g["n"], g["cp"]), float("nan"))
    pred[..., :g["ncols"]] = o["pred"]
    xd, pd = o["x"].cuda().requires_grad_(True), pred.cuda().requires_grad_(True)
    z, a, idx, _ = ops.DynamicWalkFunction.apply(xd, pd, g["kh"], g["kw"], g["ratio"], True, False)
    z.backward(o["gz"].cuda())
    _check(name, "z", z.detach().cpu(), want["z"], bars["z"])
    assert torch.equal(idx.cpu().long(), want["idx"])
    _check(name, "dx", xd.grad.cpu(), want["dx"], bars["dx"])
    dp = pd.grad.cpu()
    _check(name, "d offset-y", dp[..., :k2], want["doy"], bars["doy"])
    _check(name, "d offset-x", dp[..., k2:2 * k2], want["dox"], bars["dox"])
    _check(name, "d logits", dp[..., 2 * k2:3 * k2], want["dlg"], bars["dlg"])
    assert not bool(dp[..., 3 * k2:].any())


# =====================================================================================================================================
# 2. LayerNorm
# =====================================================================================================================================
LN_ROWS = [(72, 1024, 0.0), (8, 20, 0.0), (9, 20, 0.0), (3, 7, 0.0), (5, 1030, 0.0), (2, 4608, 0.0), (33, 260, 0.0), (1, 4, 0.0),
           (40, 1024, 300.0)]
LN_MODES = [(res, relu, p) for res in (0, 1) for relu in (0, 1) for p in (0.0, 0.3)]
LN_CASES = [(r, m) for r in LN_ROWS for m in LN_MODES]
LN_IDS = [f"{r[0]}x{r[1]}{'_mean300' if r[2] else ''}-res{m[0]}relu{m[1]}p{m[2]}" for r, m in LN_CASES]
LN_WRONG = ("unbiased", "eps_outside", "relu_from_x", "no_res_in_xhat", "dgamma_unscaled", "no_m2")
EPS = float(np.float32(1e-5))
LN_SEED = 0x1234567


@functools.lru_cache(maxsize=4)
def _ln_operands(rows, length, mean):
    gen = _gen(f"ln{rows}x{length}x{mean}")
    s = 1.0 if mean else 0.1                                      # (small variance: eps matters; the mean-300 row is as the issue states it)
    return dict(x=mean + s * torch.randn(rows, length, generator=gen), res=s * torch.randn(rows, length, generator=gen),
                gamma=1 + 0.5 * torch.randn(length, generator=gen), beta=0.5 * torch.randn(length, generator=gen),
                dy=torch.randn(rows, length, generator=gen), dg0=torch.randn(length, generator=gen), db0=torch.randn(length, generator=gen),
                keep=(torch.rand(rows, length, generator=gen) >= 0.3))


def ln_reference(x, res, gamma, beta, dy, relu, p, keep, dg0=None, db0=None, wrong=None, dtype=torch.float64, stats=None):
    """y, mean, rstd, dx, dgamma, dbeta of LayerNorm(x + res) -> ReLU -> dropout(keep / (1 - p)), written out (the wrong variants are
    one change away from it; test_layernorm_formula_matches_autograd ties the unchanged formula to torch autograd).  stats: the stored
    fp32 [rows][2] (mean, rstd) the backward kernel is handed -- its reference reads the same stored operand"""
    x, gamma, beta, dy = x.to(dtype), gamma.to(dtype), beta.to(dtype), dy.to(dtype)
    h = x + res.to(dtype) if res is not None else x
    length = h.shape[1]
    scale = keep.to(dtype) / (1.0 - float(np.float32(p))) if p > 0 else torch.ones_like(h)
    mean = h.mean(1, keepdim=True)
    var = ((h - mean) ** 2).sum(1, keepdim=True) / (length - 1 if wrong == "unbiased" else length)
    rstd = 1 / (var.sqrt() + EPS) if wrong == "eps_outside" else 1 / (var + EPS).sqrt()
    xhat = (h - mean) * rstd
    pre = xhat * gamma + beta
    y = (pre.clamp_min(0) if relu else pre) * scale
    g = dy * scale
    if relu:
        g = g * ((x if wrong == "relu_from_x" else y) > 0)
    mean_b, rstd_b = (mean, rstd) if stats is None else (stats[:, 0:1].to(dtype), stats[:, 1:2].to(dtype))
    xhat_b = (h - mean_b) * rstd_b
    xb = (x - mean_b) * rstd_b if wrong == "no_res_in_xhat" else xhat_b
    gg = g * gamma
    m1, m2 = gg.mean(1, keepdim=True), (gg * xb).mean(1, keepdim=True)
    dx = rstd_b * (gg - m1 - (0 if wrong == "no_m2" else xb * m2))
    gp = dy * (scale != 0) * ((y > 0) if relu else 1) if wrong == "dgamma_unscaled" else g
    out = dict(y=y, mean=mean[:, 0], rstd=rstd[:, 0], dx=dx, dgamma=(gp * xb).sum(0), dbeta=g.sum(0))
    if dtype == torch.float64:
        D = math.ceil(length / 512) + 16
        rows = h.shape[0]
        acc = rows if rows <= 8 else min(rows, 32) + math.ceil(rows / 32)
        mabs = h.abs().mean(1, keepdim=True)
        hround = h.abs() * rstd if res is not None else 0        # x + res is itself rounded, at the size of h
        bars = dict(mean=(D + 1) * U32 * mabs[:, 0], rstd=(D + 8) * U32 * rstd[:, 0],
                    y=U32 * scale * (((D + 1) * mabs * rstd + hround) * gamma.abs() + (D + 14) * (xhat * gamma).abs()
                                     + (5 if p > 0 else 2) * beta.abs()),
                    dbeta=(acc + 4) * U32 * g.abs().sum(0),
                    # 2 hround: under a mean of 300 the one rounding of x + res outweighs everything else in xhat by 100x, and the worst
                    # of 1024 columns over <= 72 rows comes within 2x of its bound; doubled for the 2x margin every assert here must have
                    dgamma=(g.abs() * U32 * (2 * hround + 4 * xhat_b.abs())).sum(0) + (acc + 5) * U32 * (g * xhat_b).abs().sum(0),
                    dx_floor=(D + 6) * U32 * rstd_b * (gg.abs() + gg.abs().mean(1, keepdim=True)
                                                       + xhat_b.abs() * (gg * xhat_b).abs().mean(1, keepdim=True)))
        if dg0 is not None:
            out["dgamma"], out["dbeta"] = out["dgamma"] + dg0.double(), out["dbeta"] + db0.double()
            bars["dgamma"], bars["dbeta"] = bars["dgamma"] + (acc + 5) * U32 * dg0.double().abs(), bars["dbeta"] + (acc + 4) * U32 * db0.double().abs()
        out["bars"] = bars
    return out


def _ln_expected(row, mode, keep=None, wrong=None):
    o = _ln_operands(*row)
    res, relu, p = mode
    keep = o["keep"] if keep is None else keep
    args = (o["x"], o["res"] if res else None, o["gamma"], o["beta"], o["dy"], relu, p, keep)
    fwd = ln_reference(*args)                                     # the backward reads the forward's float64 statistics rounded to fp32
    stats = torch.stack([fwd["mean"], fwd["rstd"]], dim=1).float()
    want = ln_reference(*args, o["dg0"], o["db0"], wrong, stats=stats)
    if wrong is None:                                             # the yard of dx: the same expression in fp32 torch, worst of each row
        yard = (ln_reference(*args, dtype=torch.float32, stats=stats)["dx"].double() - want["dx"]).abs().max(1, keepdim=True).values
        want["bars"]["dx"] = torch.maximum(4 * yard, want["bars"].pop("dx_floor"))
    return want


def _ln_applies(row, mode, wrong):
    res, relu, p = mode
    return {"relu_from_x": bool(relu), "no_res_in_xhat": bool(res), "dgamma_unscaled": p > 0,
            "eps_outside": row[2] == 0}.get(wrong, True)         # (variance 1 under the mean of 300: eps moves rstd by 5e-6, fp32's own size)


LN_OUT = ("y", "mean", "rstd", "dx", "dgamma", "dbeta")


def _bite_layernorm(row, mode):
    want = _ln_expected(row, mode)
    for wrong in LN_WRONG:
        if _ln_applies(row, mode, wrong):
            bad = _ln_expected(row, mode, wrong=wrong)
            worst = max(_ratio(bad[k], want[k], want["bars"][k]) for k in LN_OUT)
            assert worst >= 10.0, f"{row}/{mode}: the bars do not see '{wrong}' ({worst:.3g})"


@pytest.mark.parametrize("mode", LN_MODES)
def test_layernorm_formula_matches_autograd(mode):
    o = _ln_operands(9, 20, 0.0)
    res, relu, p = mode
    x, r, gm, bt = (o[k].double().requires_grad_(True) for k in ("x", "res", "gamma", "beta"))
    h = x + r if res else x
    y = F.layer_norm(h, (20,), gm, bt, EPS)
    y = (y.clamp_min(0) if relu else y) * (o["keep"].double() / (1.0 - float(np.float32(p))) if p else 1)
    y.backward(o["dy"].double())
    mine = ln_reference(o["x"], o["res"] if res else None, o["gamma"], o["beta"], o["dy"], relu, p, o["keep"])
    for got, ref in ((mine["y"], y), (mine["dx"], x.grad), (mine["dgamma"], gm.grad), (mine["dbeta"], bt.grad)):
        assert float((got - ref.detach()).abs().max().detach()) <= 1e-12 * float(ref.detach().abs().max())
    if res:
        assert torch.equal(x.grad, r.grad)                        # the res gradient is dx


def _keep_mask(lib, L, n, p, seed, word=None):
    """the keep mask of (seed, element index, p), recovered by running din_act_dropout_fwd on ones; word: the device-side seed offset (a
    one-element int64 tensor) or None.  It is the mask of the host model tests/dropout_reference.py, so every row that reads it is
    anchored to the definition and not to this kernel"""
    from tests import dropout_reference
    ones, out = torch.ones(n).cuda(), torch.empty(n).cuda()
    L.check(lib.din_act_dropout_fwd(ones.data_ptr(), out.data_ptr(), n, 0, p, seed, word.data_ptr() if word is not None else None, None))
    keep = out.cpu() != 0
    folded = dropout_reference.fold_seed(seed, None if word is None else int(word.cpu()) & 0xFFFFFFFFFFFFFFFF)
    assert torch.equal(keep, torch.from_numpy(dropout_reference.keep(folded, np.arange(n), p))), "din_act_dropout_fwd's mask is not the model's"
    return keep


def _ln_launch(lib, L, o, res, relu, p, seed, seed_off, stats32, y32, bwd=True):
    rows, length = o["x"].shape
    X, G, B = _Buf((rows,), length, content=o["x"]), _Buf((1,), length, content=o["gamma"]), _Buf((1,), length, content=o["beta"])
    R = _Buf((rows,), length, content=o["res"]) if res else None
    Y, S = _Buf((rows,), length), _Buf((rows,), 2)
    L.check(lib.din_layernorm_fwd(X.ptr(), R.ptr() if R else None, G.ptr(), B.ptr(), 1e-5, Y.ptr(), S.ptr(), rows, length, relu, p, seed,
                                  seed_off, None))
    torch.cuda.synchronize()
    assert _all_outside(Y, S) and _all_unchanged(X, G, B, R), "layernorm_fwd wrote outside a destination or into a source"
    if not bwd:
        return Y, S, None, None, None
    DY, YS, ST = _Buf((rows,), length, content=o["dy"]), _Buf((rows,), length, content=y32), _Buf((rows,), 2, content=stats32)
    DX, DG, DB = _Buf((rows,), length), _Buf((1,), length, content=o["dg0"]), _Buf((1,), length, content=o["db0"])
    L.check(lib.din_layernorm_bwd(DY.ptr(), X.ptr(), R.ptr() if R else None, G.ptr(), YS.ptr(), ST.ptr(), DX.ptr(), DG.ptr(), DB.ptr(), rows,
                                  length, relu, p, seed, seed_off, None))
    torch.cuda.synchronize()
    assert _all_outside(DX, DG, DB) and _all_unchanged(X, G, R, DY, YS, ST), "layernorm_bwd wrote outside a destination or into a source"
    return Y, S, DX, DG, DB


@pytest.mark.gpu
@pytest.mark.parametrize("row,mode", LN_CASES, ids=LN_IDS)
def test_layernorm_against_fp64(env, row, mode):
    lib, L, nhwc, ops = env
    o, (res, relu, p), name = _ln_operands(*row), mode, f"ln{row}/{mode}"
    rows, length = o["x"].shape
    keep = _keep_mask(lib, L, rows * length, p, LN_SEED).view(rows, length) if p else torch.ones(rows, length, dtype=torch.bool)
    want = _ln_expected(row, mode, keep)
    stats32 = torch.stack([want["mean"], want["rstd"]], dim=1).float()
    Y, S, DX, DG, DB = _ln_launch(lib, L, o, res, relu, p, LN_SEED, None, stats32, want["y"].float())
    bars = want["bars"]
    _check(name, "y", Y.get(), want["y"], bars["y"])
    _check(name, "mean", S.get()[:, 0], want["mean"], bars["mean"])
    _check(name, "rstd", S.get()[:, 1], want["rstd"], bars["rstd"])
    _check(name, "dx", DX.get(), want["dx"], bars["dx"])
    _check(name, "dgamma", DG.get()[0], want["dgamma"], bars["dgamma"])
    _check(name, "dbeta", DB.get()[0], want["dbeta"], bars["dbeta"])
    if p:                                                         # LayerNorm's own zero pattern is the recovered mask wherever the value is not ~0
        live = (want["y"].abs() > bars["y"]) | ~keep
        pre_nonzero = ln_reference(o["x"], o["res"] if res else None, o["gamma"], o["beta"], o["dy"], relu, 0.0, keep)["y"].abs() > 4 * bars["y"]
        assert torch.equal((Y.get() == 0)[pre_nonzero], ~keep[pre_nonzero]) and bool(live.any())
    Y2, S2, DX2, _, _ = _ln_launch(lib, L, o, res, relu, p, LN_SEED, None, stats32, want["y"].float())
    assert torch.equal(Y.bits(), Y2.bits()) and torch.equal(S.bits(), S2.bits()) and torch.equal(DX.bits(), DX2.bits()), f"{name}: rerun differs"


@pytest.mark.gpu
def test_layernorm_seed_offset_word(env):
    """seed s with the device word d is seed s + d without one, bit for bit, forward and backward"""
    lib, L, nhwc, ops = env
    row, (res, relu, p) = (9, 20, 0.0), (1, 1, 0.3)
    o = _ln_operands(*row)
    word = torch.tensor([977], dtype=torch.int64).cuda()
    keep = _keep_mask(lib, L, 180, p, LN_SEED + 977).view(9, 20)
    assert not torch.equal(keep, _keep_mask(lib, L, 180, p, LN_SEED).view(9, 20))
    assert torch.equal(keep, _keep_mask(lib, L, 180, p, LN_SEED, word).view(9, 20))
    want = _ln_expected(row, (res, relu, p), keep)
    stats32, y32 = torch.stack([want["mean"], want["rstd"]], dim=1).float(), want["y"].float()
    a = _ln_launch(lib, L, o, res, relu, p, LN_SEED, word.data_ptr(), stats32, y32)
    b = _ln_launch(lib, L, o, res, relu, p, LN_SEED + 977, None, stats32, y32)
    assert torch.equal(a[0].bits(), b[0].bits()) and torch.equal(a[2].bits(), b[2].bits())
    _check("seed_offset", "dgamma", a[3].get()[0], want["dgamma"], want["bars"]["dgamma"])
    assert int(word.cpu()) == 977


@pytest.mark.gpu
def test_layernorm_autograd_wrapper(env):
    """ops.layer_norm derives rows / len from gamma's shape and zeroes the parameter gradients: a per-clip affine [3, 5, 8] on 2 clips"""
    lib, L, nhwc, ops = env
    gen = _gen("ln_wrapper")
    x, res, dy = (0.1 * torch.randn(2, 3, 5, 8, generator=gen) for _ in range(3))
    gamma, beta = 1 + 0.5 * torch.randn(3, 5, 8, generator=gen), 0.5 * torch.randn(3, 5, 8, generator=gen)
    keep = torch.ones(2, 120, dtype=torch.bool)
    args = (x.view(2, 120), res.view(2, 120), gamma.view(120), beta.view(120), dy.view(2, 120), 1, 0.0, keep)
    want = ln_reference(*args)
    yard = (ln_reference(*args, dtype=torch.float32)["dx"].double() - want["dx"]).abs().max(1, keepdim=True).values
    # (the wrapper's backward reads the forward kernel's own stats and y: the yard rule covers dx; dgamma carries the stats' error bar)
    leaves = [t.cuda().requires_grad_(True) for t in (x, res, gamma, beta)]
    y = ops.layer_norm(leaves[0], leaves[2], leaves[3], res=leaves[1], relu=True)
    y.backward(dy.cuda())
    bars = want["bars"]
    _check("ln_wrapper", "y", y.detach().cpu().view(2, 120), want["y"], bars["y"])
    _check("ln_wrapper", "dx", leaves[0].grad.cpu().view(2, 120), want["dx"], torch.maximum(4 * yard, bars["dx_floor"]))
    assert torch.equal(leaves[0].grad, leaves[1].grad)
    D = 17
    stats_err = (dy.view(2, 120).double().abs() * (D + 8) * U32 * (want["mean"].abs() * want["rstd"] + 1)[:, None]).sum(0)
    _check("ln_wrapper", "dgamma", leaves[2].grad.cpu().view(120), want["dgamma"], bars["dgamma"] + stats_err)
    _check("ln_wrapper", "dbeta", leaves[3].grad.cpu().view(120), want["dbeta"], bars["dbeta"])


def test_layernorm_refusals():
    lib, L = _lib()
    d = _dummy()
    _refused(lib.din_layernorm_fwd(None, None, d, d, 1e-5, d, d, 2, 8, 0, 0.0, 0, None, None), "null pointer")
    _refused(lib.din_layernorm_fwd(d, None, d, d, 1e-5, d, d, 2, 0, 0, 0.0, 0, None, None), "bad argument")
    _refused(lib.din_layernorm_fwd(d, None, d, d, 1e-5, d, d, 2, 8, 0, 1.0, 0, None, None), "bad argument")
    _refused(lib.din_layernorm_bwd(d, d, None, d, d, d, d, None, d, 2, 8, 0, 0.0, 0, None, None), "null pointer")
    _refused(lib.din_layernorm_bwd(d, d, None, d, d, d, d, d, d, 2, 8, 0, 1.0, 0, None, None), "layernorm_bwd: bad argument")
    _refused(lib.din_layernorm_bwd(d, d, None, d, d, d, d, d, d, 2, 8, 0, -0.5, 0, None, None), "layernorm_bwd: bad argument")


# =====================================================================================================================================
# 3. context attention
# =====================================================================================================================================
CTX_SHAPES = [(2, 12, 33, 2, 32), (1, 1, 1, 1, 4), (2, 16, 64, 1, 256), (1, 5, 65, 3, 8), (2, 12, 257, 4, 128), (1, 7, 31, 2, 64),
              (1, 12, 600, 2, 128)]
CTX_IDS = ["x".join(map(str, s)) for s in CTX_SHAPES]
CTX_WRONG = ("box_axis", "no_ds_q", "interleaved", "short_dot")
TINY = 2.0 ** -126


def _split(v, heads, wrong=None):
    """[bt][m][heads * c] -> [bt][heads][m][c]: head h owns channels [h c, (h + 1) c) (blocked); wrong: interleaved"""
    bt, m, hc = v.shape
    if wrong == "interleaved":
        return v.reshape(bt, m, hc // heads, heads).permute(0, 3, 1, 2)
    return v.reshape(bt, m, heads, hc // heads).permute(0, 2, 1, 3)


def _merge(v, wrong=None):
    bt, heads, m, c = v.shape
    if wrong == "interleaved":
        return v.permute(0, 2, 3, 1).reshape(bt, m, heads * c)
    return v.permute(0, 2, 1, 3).reshape(bt, m, heads * c)


def softmax_reference(s, wrong_axis=False):
    """(softmax over the last axis in float64, its bar)"""
    s = s.double()
    a = torch.softmax(s, dim=-2 if wrong_axis else -1)
    L_ = math.ceil(s.shape[-1] / 256)
    d = (s - s.max(-1, keepdim=True).values).abs()
    # 2 d: the rounding of x - max is ONE rounding that dominates the small probabilities, and over 10^4..10^5 elements it comes within a
    # few percent of its bound d u -- a bar of d u + slack cannot keep the 2x margin every assert here must have, so that term is doubled
    return a, (2 * d + (a * d).sum(-1, keepdim=True) + L_ + 17) * U32 * a + TINY


def softmax_bwd_reference(a, da, dtype=torch.float64):
    a, da = a.to(dtype), da.to(dtype)
    return a * (da - (a * da).sum(-1, keepdim=True))


def softmax_bwd_bar(a, da):
    a, da = a.double(), da.double()
    want = softmax_bwd_reference(a, da)
    yard = (softmax_bwd_reference(a, da, torch.float32).double() - want).abs().max(-1, keepdim=True).values
    floor = (math.ceil(a.shape[-1] / 256) + 13) * U32 * a.abs() * (da.abs() + (a * da).abs().sum(-1, keepdim=True))
    return want, torch.maximum(4 * yard, floor)


@functools.lru_cache(maxsize=2)
def ctx_stages(shape, wrong=None):
    """the six launches of ContextAttentionFunction as float64 stages; every stage reads the fp32 rounding of the previous one (its
    stored operand on the GPU).  name -> (want, bar); the stored inputs under 'in'."""
    bt, n, p, heads, c = shape
    gen = _gen("ctx" + str(shape))
    q, kf, dctx = (torch.randn(bt, m, heads * c, generator=gen) * s for m, s in ((n, 0.5), (p, 0.5), (n, 1.0)))
    qh, kh, dh = (_split(v.double(), heads, wrong) for v in (q, kf, dctx))
    if wrong == "short_dot":
        qh = torch.cat([qh[..., :-1], torch.zeros_like(qh[..., -1:])], dim=-1)
    G = 256 // c
    st = {}

    def scores(u, what):
        w_ = u @ kh.transpose(2, 3)
        st[what] = (w_, (c // 4 + 5) * U32 * (u.abs() @ kh.abs().transpose(2, 3)))
        return w_.float()

    def apply(a32, what):
        o = _merge(a32.double() @ kh, wrong)
        st[what] = (o, (math.ceil(p / G) + G + 2) * U32 * _merge(a32.double().abs() @ kh.abs(), wrong))
        return o.float()

    s32 = scores(qh, "scores")
    a, abar = softmax_reference(s32, wrong == "box_axis")
    st["softmax"] = (a, abar)
    a32 = a.float()
    apply(a32, "apply")
    da32 = scores(dh, "scores_dctx")
    st["softmax_bwd"] = softmax_bwd_bar(a32, da32)
    ds32 = st["softmax_bwd"][0].float()
    apply(ds32, "apply_dq")
    a64, ds64 = a32.double(), (0 * ds32 if wrong == "no_ds_q" else ds32).double()
    st["keys_grad"] = (_merge(a64.transpose(2, 3) @ dh + ds64.transpose(2, 3) @ qh, wrong),
                       (2 * n + 2) * U32 * _merge(a64.abs().transpose(2, 3) @ dh.abs() + ds32.double().abs().transpose(2, 3) @ qh.abs(), wrong))
    st["in"] = dict(q=q, kf=kf, dctx=dctx, s32=s32, a32=a32, da32=da32, ds32=ds32)
    return st


def _ctx_applies(shape, wrong):
    bt, n, p, heads, c = shape
    return {"box_axis": n > 1 and p > 1, "no_ds_q": p > 1, "interleaved": heads > 1}.get(wrong, True)


CTX_STAGES = ("scores", "softmax", "apply", "scores_dctx", "softmax_bwd", "apply_dq", "keys_grad")


def _bite_context_attention(shape):
    want = ctx_stages(shape)
    tried = 0
    for wrong in CTX_WRONG:
        if _ctx_applies(shape, wrong):
            tried += 1
            bad = ctx_stages(shape, wrong)
            worst = max(_ratio(bad[k][0], want[k][0], want[k][1]) for k in CTX_STAGES)
            assert worst >= 10.0, f"{shape}: the bars do not see '{wrong}' ({worst:.3g})"
    assert tried >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("shape", CTX_SHAPES, ids=CTX_IDS)
def test_context_attention_entry_points_against_fp64(env, shape):
    lib, L, nhwc, ops = env
    bt, n, p, heads, c = shape
    st, name = ctx_stages(shape), "ctx" + str(shape)
    i = st["in"]
    hc, rows = heads * c, bt * heads * n
    Q, K, DC = _Buf((bt, n), hc, content=i["q"]), _Buf((bt, p), hc, content=i["kf"]), _Buf((bt, n), hc, content=i["dctx"])

    def twice(run, srcs):
        outs = [run(), run()]
        torch.cuda.synchronize()
        assert torch.equal(outs[0].bits(), outs[1].bits()), f"{name}: rerun differs"
        assert outs[0].untouched_outside() and _all_unchanged(*srcs), f"{name}: wrote outside a destination or into a source"
        return outs[0]

    def scores(src):
        def run():
            S = _Buf((bt, heads, n), p)
            L.check(lib.din_ctx_scores(src.ptr(), K.ptr(), S.ptr(), bt, n, p, heads, c, None))
            return S
        return twice(run, (src, K))

    def inplace(fn, content, *pre):
        def run():
            S = _Buf((bt, heads, n), p, content=content)
            L.check(fn(*[b.ptr() for b in pre], S.ptr(), rows, p, None))
            return S
        return twice(run, pre)

    def apply(content):
        A = _Buf((bt, heads, n), p, content=content)

        def run():
            O_ = _Buf((bt, n), hc)
            L.check(lib.din_ctx_apply(A.ptr(), K.ptr(), O_.ptr(), bt, n, p, heads, c, None))
            return O_
        return twice(run, (A, K))

    _check(name, "scores", scores(Q).get(), *st["scores"])
    _check(name, "softmax", inplace(lib.din_softmax_rows, i["s32"]).get(), *st["softmax"])
    _check(name, "apply", apply(i["a32"]).get(), *st["apply"])
    _check(name, "scores(dctx)", scores(DC).get(), *st["scores_dctx"])
    A32 = _Buf((bt, heads, n), p, content=i["a32"])
    _check(name, "softmax_bwd", inplace(lib.din_softmax_rows_bwd, i["da32"], A32).get(), *st["softmax_bwd"])
    _check(name, "apply(ds)", apply(i["ds32"]).get(), *st["apply_dq"])
    DS = _Buf((bt, heads, n), p, content=i["ds32"])

    def keys():
        DK = _Buf((bt, p), hc)
        L.check(lib.din_ctx_keys_grad(A32.ptr(), DS.ptr(), DC.ptr(), Q.ptr(), DK.ptr(), bt, n, p, heads, c, None))
        return DK
    _check(name, "keys_grad", twice(keys, (A32, DS, DC, Q)).get(), *st["keys_grad"])


SOFTMAX_ROWS = [(rows, length, span) for rows in (3, 70) for length in (1, 255, 256, 257, 1000) for span in (3.0,)] + [(70, 1000, 200.0)]


@functools.lru_cache(maxsize=None)
def _softmax_table(rows, length, span):
    gen = _gen(f"softmax{rows}x{length}x{span}")
    s = (torch.rand(rows, length, generator=gen) * 2 - 1) * span
    if span > 100:                                                # a few scores within 2 of each row's maximum: neither uniform nor one-hot
        s[:, :4] = s.max(1, keepdim=True).values - 2 * torch.rand(rows, 4, generator=gen)
    return s, torch.randn(rows, length, generator=gen)


def test_softmax_large_scores_table_exercises_the_arithmetic():
    s, _ = _softmax_table(70, 1000, 200.0)
    a, bar = softmax_reference(s)
    assert float(s.max()) > 150 and float(s.min()) < -150
    assert float(a.max(1).values.max()) < 0.9 and float(a.max(1).values.min()) > 10.0 / 1000      # neither one-hot nor uniform
    assert not bool(torch.isfinite(torch.exp(s.float())).all())  # exp without the max subtraction overflows fp32 here
    naive = torch.exp(s.float()) / torch.exp(s.float()).sum(1, keepdim=True)
    assert not _ratio(naive, a, bar) <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("rows,length,span", SOFTMAX_ROWS)
def test_softmax_rows_against_fp64(env, rows, length, span):
    lib, L, nhwc, ops = env
    s, da = _softmax_table(rows, length, span)
    name = f"softmax{rows}x{length}x{span}"
    a, bar = softmax_reference(s)
    S = _Buf((rows,), length, content=s)
    L.check(lib.din_softmax_rows(S.ptr(), rows, length, None))
    S2 = _Buf((rows,), length, content=s)
    L.check(lib.din_softmax_rows(S2.ptr(), rows, length, None))
    torch.cuda.synchronize()
    assert S.untouched_outside() and torch.equal(S.bits(), S2.bits())
    _check(name, "softmax", S.get(), a, bar)
    a32 = a.float()
    want, bbar = softmax_bwd_bar(a32, da)
    A, D = _Buf((rows,), length, content=a32), _Buf((rows,), length, content=da)
    L.check(lib.din_softmax_rows_bwd(A.ptr(), D.ptr(), rows, length, None))
    torch.cuda.synchronize()
    assert D.untouched_outside() and A.unchanged()
    _check(name, "softmax_bwd", D.get(), want, bbar)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [CTX_SHAPES[0], CTX_SHAPES[3]], ids=[CTX_IDS[0], CTX_IDS[3]])
def test_context_attention_function_end_to_end(env, shape):
    """ops.ContextAttentionFunction (its own buffers and launch order) against float64 autograd: the yard rule per tensor,
    floor (c / 4 + p + 20) u max|ref| -- the scores dot, the pixel sum and the softmax behind every element"""
    lib, L, nhwc, ops = env
    bt, n, p, heads, c = shape
    i = ctx_stages(shape)["in"]

    def run(dtype):
        q, kf = i["q"].clone().to(dtype).requires_grad_(True), i["kf"].clone().to(dtype).requires_grad_(True)
        att = torch.softmax(_split(q, heads) @ _split(kf, heads).transpose(2, 3), dim=-1)
        out = _merge(att @ _split(kf, heads))
        out.backward(i["dctx"].to(dtype))
        return dict(att=att.detach(), out=out.detach(), dq=q.grad, dkf=kf.grad)

    r64, r32 = run(torch.float64), run(torch.float32)
    qd, kd = i["q"].detach().cuda().requires_grad_(True), i["kf"].detach().cuda().requires_grad_(True)
    out, att = ops.ContextAttentionFunction.apply(qd, kd, heads)
    out.backward(i["dctx"].cuda())
    for what, got in (("att", att), ("out", out), ("dq", qd.grad), ("dkf", kd.grad)):
        ref = r64[what]
        yard = float((r32[what].double() - ref).abs().max())
        err = Measured(float((got.detach().cpu().double() - ref).abs().max()))
        print(f"ctx e2e {shape} {what}: err {float(err):.3e} yard {yard:.3e}")
        assert err <= max(4 * yard, (c / 4 + p + 20) * U32 * float(ref.abs().max())), what


def test_context_attention_refusals():
    lib, L = _lib()
    d = _dummy()
    for n, c in ((17, 32), (12, 96), (12, 2), (12, 512)):
        _refused(lib.din_ctx_scores(d, d, d, 1, n, 8, 1, c, None), "power-of-two")
        _refused(lib.din_ctx_apply(d, d, d, 1, n, 8, 1, c, None), "power-of-two")
        _refused(lib.din_ctx_keys_grad(d, d, d, d, d, 1, n, 8, 1, c, None), "power-of-two")
    _refused(lib.din_ctx_scores(None, d, d, 1, 12, 8, 1, 32, None), "null pointer")
    _refused(lib.din_softmax_rows(d, 3, 0, None), "bad argument")


# =====================================================================================================================================
# 4. head
# =====================================================================================================================================
HEAD_SHAPES = [(2, 3, 12, 256, 8), (1, 1, 1, 1, 1), (3, 2, 5, 257, 16), (2, 4, 7, 100, 9)]
HEAD_CASES = [(s, m) for s in HEAD_SHAPES for m in ("all", "npc")]
HEAD_IDS = ["x".join(map(str, s)) + "-" + m for s, m in HEAD_CASES]
HEAD_WRONG = ("last_max", "no_mean", "npc_ignored", "all_tied", "no_bias")
HEAD_VALUES = torch.tensor([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0])


@functools.lru_cache(maxsize=None)
def _head_operands(shape):
    b, t, n, c, a = shape
    gen = _gen("head" + str(shape))
    s = HEAD_VALUES[torch.randint(0, 6, (b, t, n, c), generator=gen)]
    if t * n > 1:
        s[-1, -1] = -HEAD_VALUES[3:][torch.randint(0, 3, (n, c), generator=gen)]      # an all-negative frame
    counts = [n, 1, max(1, n // 2)][:b] if b > 1 else [n]
    return dict(s=s, w=torch.randn(a, c, generator=gen), bias=torch.randn(a, generator=gen), dsc=torch.randn(b, a, generator=gen),
                dw0=torch.randn(a, c, generator=gen), db0=torch.randn(a, generator=gen), counts=counts)


def head_reference(shape, mode, wrong=None):
    b, t, n, c, a = shape
    o = _head_operands(shape)
    s, w, bias, dsc = (o[k].double() for k in ("s", "w", "bias", "dsc"))
    counts = o["counts"] if mode == "npc" and wrong != "npc_ignored" else [n] * b
    valid = (torch.arange(n)[None, :] < torch.tensor(counts)[:, None])[:, None, :, None]          # [b][1][n][1]
    sv = torch.where(valid, s, torch.full_like(s, -float("inf")))
    pooled = sv.max(2).values                                     # [b][t][c]
    hit = sv == pooled.unsqueeze(2)
    order = torch.arange(n)[None, None, :, None].expand(b, t, n, c)
    argmax = torch.where(hit, order, torch.full_like(order, -1 if wrong == "last_max" else n))
    argmax = argmax.max(2).values if wrong == "last_max" else argmax.min(2).values
    frame = pooled @ w.t() + (0 if wrong == "no_bias" else bias)
    scores = frame.sum(1) if wrong == "no_mean" else frame.mean(1)
    terms = (pooled.abs() @ w.abs().t() + bias.abs()).mean(1)
    g = (dsc / t) @ w                                             # [b][c]
    sel = hit if wrong == "all_tied" else order == argmax.unsqueeze(2)
    ds = sel * g[:, None, None, :]
    dw = o["dw0"].double() + torch.einsum("ba,btc->ac", dsc / t, pooled)
    db = o["db0"].double() + dsc.sum(0) * t / t
    bars = dict(scores=(math.ceil(c / 256) + t + 15) * U32 * terms, ds=(a + 5) * U32 * sel * ((dsc.abs() / t) @ w.abs())[:, None, None, :],
                dw=(b * t + 5) * U32 * (o["dw0"].double().abs() + torch.einsum("ba,btc->ac", dsc.abs() / t, pooled.abs())),
                db=(b * t + 5) * U32 * (o["db0"].double().abs() + dsc.abs().sum(0)))
    return dict(scores=scores, argmax=argmax, ds=ds, dw=dw, db=db, bars=bars, ties=int((hit.sum(2) > 1).sum()),
                negative=int((pooled < 0).all(-1).sum()))


def _head_applies(shape, mode, wrong):
    b, t, n, c, a = shape
    return {"last_max": n > 1, "all_tied": n > 1, "no_mean": t > 1, "npc_ignored": mode == "npc" and n > 1}.get(wrong, True)


def _bite_head(shape, mode):
    want = head_reference(shape, mode)
    if shape[2] > 1:
        assert want["ties"] > 0 and want["negative"] >= 1, "the inputs promise tied maxima and an all-negative frame"
    tried = 0
    for wrong in HEAD_WRONG:
        if _head_applies(shape, mode, wrong):
            tried += 1
            bad = head_reference(shape, mode, wrong)
            worst = max(_ratio(bad[k], want[k], want["bars"][k]) for k in ("scores", "ds", "dw", "db"))
            moved = not torch.equal(bad["argmax"], want["argmax"])
            assert worst >= 10.0 or moved, f"{shape}/{mode}: nothing sees '{wrong}'"
            if wrong in ("last_max", "all_tied"):
                assert worst >= 10.0, f"{shape}/{mode}: the ds footprint does not see '{wrong}'"
    assert tried >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("shape,mode", HEAD_CASES, ids=HEAD_IDS)
def test_head_against_fp64(env, shape, mode):
    lib, L, nhwc, ops = env
    b, t, n, c, a = shape
    o, want, name = _head_operands(shape), head_reference(shape, mode), f"head{shape}/{mode}"
    S, W, B, DSC = (_Buf(lead, m, content=o[k]) for lead, m, k in (((b, t, n), c, "s"), ((a,), c, "w"), ((1,), a, "bias"), ((b,), a, "dsc")))
    npc = torch.tensor(o["counts"], dtype=torch.int32).cuda() if mode == "npc" else None

    def forward():
        SC, AM = _Buf((1,), b * a + b * t * a), _Buf((b, t), c, torch.int32)
        L.check(lib.din_head_fwd(S.ptr(), W.ptr(), B.ptr(), npc.data_ptr() if npc is not None else None, b, t, n, c, a, SC.ptr(), AM.ptr(), None))
        torch.cuda.synchronize()
        return SC, AM
    SC, AM = forward()
    assert _all_outside(SC, AM) and _all_unchanged(S, W, B), f"{name}: wrote outside a destination or into a source"
    _check(name, "scores", SC.get()[0, :b * a].view(b, a), want["scores"], want["bars"]["scores"])
    assert torch.equal(AM.get().long(), want["argmax"]), f"{name}: argmax is not the first maximum among the valid actors"
    SC2, AM2 = forward()
    assert torch.equal(SC.bits(), SC2.bits()) and torch.equal(AM.bits(), AM2.bits()), f"{name}: rerun differs"
    AMS = _Buf((b, t), c, torch.int32, content=want["argmax"].int())
    DS, DW, DB = _Buf((b, t, n), c), _Buf((a,), c, content=o["dw0"]), _Buf((1,), a, content=o["db0"])
    L.check(lib.din_head_bwd(DSC.ptr(), S.ptr(), W.ptr(), AMS.ptr(), b, t, n, c, a, DS.ptr(), DW.ptr(), DB.ptr(), None))
    torch.cuda.synchronize()
    assert _all_outside(DS, DW, DB) and _all_unchanged(DSC, S, W, AMS), f"{name}: wrote outside a destination or into a source"
    assert torch.equal(DS.get() != 0, want["ds"] != 0), f"{name}: the gradient's footprint is not the arg-max"
    _check(name, "ds", DS.get(), want["ds"], want["bars"]["ds"])
    _check(name, "dw", DW.get(), want["dw"], want["bars"]["dw"])
    _check(name, "dbias", DB.get()[0], want["db"], want["bars"]["db"])


def test_head_refusals():
    lib, L = _lib()
    d = _dummy()
    _refused(lib.din_head_fwd(d, d, d, None, 2, 3, 12, 256, 17, d, d, None), "bad shape")
    _refused(lib.din_head_bwd(d, d, d, d, 2, 3, 12, 256, 17, d, d, d, None), "bad shape")
    _refused(lib.din_head_fwd(d, d, d, None, 2, 3, 12, 256, 8, d, None, None), "null pointer")
    _refused(lib.din_head_bwd(d, d, d, d, 2, 3, 12, 256, 8, d, None, d, None), "null pointer")


# =====================================================================================================================================
# 5. helpers
# =====================================================================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 600001])
@pytest.mark.parametrize("with_y", [0, 1])
def test_axpby_against_fp64(env, n, with_y):
    lib, L, nhwc, ops = env
    gen = _gen(f"axpby{n}")
    x, y, a, b = torch.randn(n, generator=gen), torch.randn(n, generator=gen), 0.75, -1.3
    af, bf = float(np.float32(a)), float(np.float32(b))
    X, Y, O_ = _Buf((1,), n, content=x), _Buf((1,), n, content=y) if with_y else None, _Buf((1,), n)
    L.check(lib.din_axpby(X.ptr(), Y.ptr() if Y else None, O_.ptr(), a, b, n, None))
    torch.cuda.synchronize()
    assert O_.untouched_outside() and _all_unchanged(X, Y)
    want = af * x.double() + (bf * y.double() if with_y else 0)
    _check(f"axpby{n}/{with_y}", "out", O_.get()[0], want, 4 * U32 * ((af * x.double()).abs() + (bf * y.double()).abs() * with_y))


@pytest.mark.gpu
@pytest.mark.parametrize("accumulate", [0, 1])
def test_scale_by_param_and_dot_accum_against_fp64(env, accumulate):
    lib, L, nhwc, ops = env
    gen = _gen("scale_by_param")
    n = 1003
    x, prior, sc = torch.randn(n, generator=gen), torch.randn(n, generator=gen), torch.randn(4, generator=gen)
    X, SC = _Buf((1,), n, content=x), _Buf((1,), 4, content=sc)
    O_ = _Buf((1,), n, content=prior if accumulate else None)     # accumulate = 0: the NaN prior must not survive
    L.check(lib.din_scale_by_param(X.ptr(), SC.ptr(), 2, O_.ptr(), accumulate, n, None))
    torch.cuda.synchronize()
    assert O_.untouched_outside() and _all_unchanged(X, SC)
    want = x.double() * sc[2].double() + (prior.double() if accumulate else 0)
    _check("scale_by_param", "out", O_.get()[0], want, 4 * U32 * ((x.double() * sc[2].double()).abs() + prior.double().abs() * accumulate))
    if accumulate:                                                # dot_accum onto a non-zero prior at idx 3 of 5, above the 512 x 256 capped grid
        n = 300001
        x, y = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
        X, Y, D = _Buf((1,), n, content=x), _Buf((1,), n, content=y), _Buf((1,), 1, content=torch.tensor([0.625]), ld=5, off=3)
        L.check(lib.din_dot_accum(X.ptr(), Y.ptr(), D.ptr(), 3, n, None))
        torch.cuda.synchronize()
        assert D.untouched_outside() and _all_unchanged(X, Y), "dot_accum: a neighbour of out[idx] changed"
        terms = (x.double() * y.double()).abs().sum() + 0.625
        _check("dot_accum", "out[idx]", D.get()[0], 0.625 + (x.double() * y.double()).sum().view(1), 2060 * U32 * terms.view(1))


CAST_VALUES = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -20, 0.0, -0.0, float("inf"), -float("inf"),
               3.4028234663852886e38, -3.4028234663852886e38, 3.3895313892515355e38, 1e-40, -1e-40, float("nan")]


@pytest.mark.gpu
@pytest.mark.parametrize("src,dst", [(FP, FP), (FP, BF), (BF, FP), (BF, BF)])
def test_cast_bitwise(env, src, dst):
    """round-to-nearest-even ties, signed zeros, infinities, the largest finite values, a subnormal: torch's conversion bit for bit; a NaN
    stays a NaN"""
    lib, L, nhwc, ops = env
    gen = _gen("cast")
    v = torch.cat([torch.tensor(CAST_VALUES), torch.randn(1003 - len(CAST_VALUES), generator=gen)]).to(src)
    X, O_ = _Buf((1,), 1003, src, content=v), _Buf((1,), 1003, dst)
    code = {FP: L.DIN_F32, BF: L.DIN_BF16}
    L.check(lib.din_cast(X.ptr(), code[src], O_.ptr(), code[dst], 1003, None))
    torch.cuda.synchronize()
    assert O_.untouched_outside() and X.unchanged()
    got, want = O_.get()[0], v.to(dst)
    nan = torch.isnan(want)
    assert int(nan.sum()) == 1 and torch.equal(torch.isnan(got), nan)
    assert torch.equal(_bits(got[~nan]), _bits(want[~nan]))


@pytest.mark.gpu
def test_mask_actors_exact(env):
    lib, L, nhwc, ops = env
    b, t, n, c = 3, 2, 5, 6
    x = torch.randn(b, t, n, c, generator=_gen("mask_actors"))
    counts = torch.tensor([5, 1, 3], dtype=torch.int32)
    X, O_ = _Buf((b, t, n), c, content=x), _Buf((b, t, n), c)
    L.check(lib.din_mask_actors(X.ptr(), counts.cuda().data_ptr(), b, t, n, c, O_.ptr(), None))
    torch.cuda.synchronize()
    want = torch.where((torch.arange(n)[None, :] < counts[:, None])[:, None, :, None], x, torch.zeros(()))
    assert O_.untouched_outside() and X.unchanged() and torch.equal(_bits(O_.get()), _bits(want))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [FP, BF])
@pytest.mark.parametrize("mask", [0, 1])
def test_grad_cast_mask_exact(env, dtype, mask):
    lib, L, nhwc, ops = env
    gen = _gen("grad_cast_mask")
    pixels, c, ldy, yoff, ldo, ooff = 37, 8, 16, 4, 20, 8
    g, y = torch.randn(pixels, c, generator=gen), torch.randn(pixels, c, generator=gen).to(dtype)
    G, Y, O_ = _Buf((pixels,), c, content=g), _Buf((pixels,), c, dtype, content=y, ld=ldy, off=yoff), _Buf((pixels,), c, dtype, ld=ldo, off=ooff)
    L.check(lib.din_grad_cast_mask(G.ptr(), Y.ptr() if mask else None, O_.ptr(), L.DIN_BF16 if dtype == BF else L.DIN_F32, pixels, c, ldy, yoff,
                                   ldo, ooff, mask, None))
    torch.cuda.synchronize()
    want = (torch.where(y.float() > 0, g, torch.zeros_like(g)) if mask else g).to(dtype)
    assert O_.untouched_outside() and _all_unchanged(G, Y) and torch.equal(_bits(O_.get()), _bits(want))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [FP, BF])
@pytest.mark.parametrize("shape", [(2, 5, 7, 33), (1, 1, 1, 1), (1, 6, 7, 40)])
def test_layout_changes_exact(env, dtype, shape):
    lib, L, nhwc, ops = env
    nb, h, w, c = shape
    ld, coff, code = c + 3, 2, L.DIN_BF16 if dtype == BF else L.DIN_F32
    x = torch.randn(nb, h, w, c, generator=_gen("layout" + str(shape))).to(dtype)
    X, O_ = _Buf((nb, h, w), c, dtype, content=x, ld=ld, off=coff), _Buf((nb, c), h * w)
    L.check(lib.din_nhwc_to_nchw_f32(X.ptr(), code, nb, h, w, c, ld, coff, O_.ptr(), None))
    torch.cuda.synchronize()
    nchw = x.float().permute(0, 3, 1, 2).reshape(nb, c, h * w)
    assert O_.untouched_outside() and X.unchanged() and torch.equal(_bits(O_.get()), _bits(nchw))
    src = torch.randn(nb, c, h * w, generator=_gen("layout_back" + str(shape)))
    I, B = _Buf((nb, c), h * w, content=src), _Buf((nb, h, w), c, dtype, ld=ld, off=coff)
    L.check(lib.din_nchw_f32_to_nhwc(I.ptr(), nb, h, w, c, B.ptr(), code, ld, coff, None))
    torch.cuda.synchronize()
    want = src.view(nb, c, h, w).permute(0, 2, 3, 1).to(dtype)
    assert B.untouched_outside() and I.unchanged() and torch.equal(_bits(B.get()), _bits(want))
    if dtype == FP:                                               # a round trip is the identity
        R = _Buf((nb, c), h * w)
        L.check(lib.din_nhwc_to_nchw_f32(B.ptr(), code, nb, h, w, c, ld, coff, R.ptr(), None))
        torch.cuda.synchronize()
        assert torch.equal(_bits(R.get()), _bits(src))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [FP, BF])
@pytest.mark.parametrize("frames,per_frame", [(3, 4), (3, 1048580)])   # 3 x 1048580 / 4 vectors > the 2048 x 256 capped grid: the loop trips
def test_add_position_exact(env, dtype, frames, per_frame):
    lib, L, nhwc, ops = env
    gen = _gen(f"add_position{per_frame}")
    code = L.DIN_BF16 if dtype == BF else L.DIN_F32
    x, pos, gy = torch.randn(frames, per_frame, generator=gen).to(dtype), torch.randn(per_frame, generator=gen), torch.randn(frames, per_frame, generator=gen)
    X, P, Y = _Buf((frames,), per_frame, dtype, content=x), _Buf((1,), per_frame, content=pos), _Buf((frames,), per_frame)
    L.check(lib.din_add_position(X.ptr(), code, P.ptr(), Y.ptr(), frames, per_frame, None))
    torch.cuda.synchronize()
    assert Y.untouched_outside() and _all_unchanged(X, P) and torch.equal(_bits(Y.get()), _bits(x.float() + pos))
    GY = _Buf((frames,), per_frame, content=gy)
    for mask in (0, 1):
        GX = _Buf((frames,), per_frame, dtype)
        L.check(lib.din_add_position_bwd(GY.ptr(), X.ptr() if mask else None, code, GX.ptr(), frames * per_frame, mask, None))
        torch.cuda.synchronize()
        want = (torch.where(x.float() > 0, gy, torch.zeros_like(gy)) if mask else gy).to(dtype)
        assert GX.untouched_outside() and _all_unchanged(X, GY) and torch.equal(_bits(GX.get()), _bits(want))


@pytest.mark.gpu
@pytest.mark.parametrize("relu", [0, 1])
def test_act_dropout_exact_given_its_mask(env, relu):
    lib, L, nhwc, ops = env
    gen = _gen("act_dropout")
    n, p, seed = 600001, 0.3, 424242                              # above the capped grid's 524288 threads
    x, gy = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    keep = _keep_mask(lib, L, n, p, seed)
    # n Bernoulli(0.7) draws: sigma = sqrt(0.21 n) = 355; 6 sigma has a two-sided tail of 2e-9
    assert abs(int(keep.sum()) - 0.7 * n) <= 6 * math.sqrt(0.21 * n)
    scale = torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p))             # fp32, as the kernel computes it
    X, GY = _Buf((1,), n, content=x), _Buf((1,), n, content=gy)
    word = torch.tensor([31], dtype=torch.int64).cuda()
    outs = []
    for s, off in ((seed, None), (seed - 31, word.data_ptr())):   # the seed_offset word is honoured: (seed - 31) + 31
        Y, GX = _Buf((1,), n), _Buf((1,), n)
        L.check(lib.din_act_dropout_fwd(X.ptr(), Y.ptr(), n, relu, p, s, off, None))
        L.check(lib.din_act_dropout_bwd(GY.ptr(), X.ptr(), GX.ptr(), n, relu, p, s, off, None))
        torch.cuda.synchronize()
        assert _all_outside(Y, GX) and _all_unchanged(X, GY)
        outs.append((Y.get()[0], GX.get()[0]))
    act = x.clamp_min(0) if relu else x
    live = (x > 0) if relu else torch.ones(n, dtype=torch.bool)
    for y, gx in outs:
        assert torch.equal(y, act * (keep * scale)) and torch.equal(gx, torch.where(live, gy * (keep * scale), torch.zeros(n)))


ADAM_MODES = [(step, wd, gs) for step in (1, 2, 1000) for wd in (0.0, 0.01) for gs in (1.0, 1.0 / 128)]
B1, B2, LR, AEPS = (float(np.float32(v)) for v in (0.9, 0.999, 1e-3, 1e-8))


def adam_reference(p, g, m, v, step, wd, gs, wrong=None):
    """torch.optim.Adam in float64 on the stored fp32 state: L2 decay folded into the gradient, bias-corrected moments"""
    p, g, m, v, wd = p.double(), g.double(), m.double(), v.double(), float(np.float32(wd))
    gi = g * (1.0 if wrong == "no_grad_scale" else float(np.float32(gs))) + wd * p
    gabs = (g * gs).abs() + (wd * p).abs()
    m2, v2 = B1 * m + (1 - B1) * gi, B2 * v + (1 - B2) * gi * gi
    mabs, vabs = (B1 * m).abs() + (1 - B1) * gabs, B2 * v + (1 - B2) * gabs * gabs
    bc1, bc2 = (1.0, 1.0) if wrong == "no_bias_correction" else (1 - B1 ** step, math.sqrt(1 - B2 ** step))
    c1, c2 = 2 * B1 ** step / (1 - B1 ** step), B2 ** step / (1 - B2 ** step)              # cancellation in 1 - beta^step (sqrt halves c2's)
    root = v2.sqrt() / bc2
    denom = root + AEPS
    p2 = p - (LR / bc1) * (m2 / denom)
    dm, ddenom = 6 * U32 * mabs, root * (5.5 * vabs / v2.clamp_min(1e-300) + 2 + c2) * U32 + U32 * denom
    bars = dict(m=dm, v=11 * U32 * vabs,
                p=U32 * (p.abs() + p2.abs()) + (LR / bc1) * (dm / denom + m2.abs() / denom * (ddenom / denom + (3 + c1) * U32)))
    return dict(p=p2, m=m2, v=v2, bars=bars)


@functools.lru_cache(maxsize=None)
def _adam_state(n):
    gen = _gen(f"adam{n}")
    p, g, m, v = torch.randn(n, generator=gen), torch.randn(n, generator=gen), 0.1 * torch.randn(n, generator=gen), torch.rand(n, generator=gen) ** 2
    g[::3], v[::6] = 0.0, 0.0                                      # exact zeros: eps dominates the denominator where both vanish
    return p, g, m, v


def _bite_adam(step, wd, gs):
    st = _adam_state(8193)
    want = adam_reference(*st, step, wd, gs)
    for wrong in ("no_bias_correction",) + (("no_grad_scale",) if gs != 1.0 else ()):
        bad = adam_reference(*st, step, wd, gs, wrong)
        assert max(_ratio(bad[k], want[k], want["bars"][k]) for k in "pmv") >= 10.0, wrong


@pytest.mark.gpu
@pytest.mark.parametrize("step,wd,gs", ADAM_MODES)
def test_adam_against_fp64(env, step, wd, gs):
    lib, L, nhwc, ops = env
    sizes = (1, 8192, 8193)
    for multi in (0, 1):
        bufs = [[_Buf((1,), n, content=t) for t in _adam_state(n)] for n in sizes]
        if multi:
            chunk = 8192
            ptrs = torch.tensor([b.ptr() for quad in bufs for b in (quad[0], quad[1], quad[2], quad[3])], dtype=torch.int64).cuda()
            ct, ci = zip(*[(t, i) for t, n in enumerate(sizes) for i in range(-(-n // chunk))])
            dev = [torch.tensor(v, dtype=dt).cuda() for v, dt in ((sizes, torch.int64), (ct, torch.int32), (ci, torch.int32))]
            L.check(lib.din_adam_step_multi(ptrs.data_ptr(), dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), len(ct), chunk, LR, B1, B2,
                                            AEPS, wd, step, gs, None))
        else:
            for (P, G, M, V), n in zip(bufs, sizes):
                L.check(lib.din_adam_step(P.ptr(), G.ptr(), M.ptr(), V.ptr(), n, LR, B1, B2, AEPS, wd, step, gs, None))
        torch.cuda.synchronize()
        for (P, G, M, V), n in zip(bufs, sizes):
            want = adam_reference(*_adam_state(n), step, wd, gs)
            assert _all_outside(P, M, V) and G.unchanged()
            for k, buf in (("p", P), ("m", M), ("v", V)):
                _check(f"adam{'_multi' if multi else ''}[{n}] step {step} wd {wd} gs {gs:.3g}", k, buf.get()[0], want[k], want["bars"][k])


# =====================================================================================================================================
# the bars bite: every family, row and mode (CPU)
# =====================================================================================================================================
BITE = ([(_bite_walk, (n,), "walk-" + n) for n in WALK_IDS] + [(_bite_layernorm, c, "ln-" + i) for c, i in zip(LN_CASES, LN_IDS)]
        + [(_bite_context_attention, (s,), "ctx-" + i) for s, i in zip(CTX_SHAPES, CTX_IDS)]
        + [(_bite_head, c, "head-" + i) for c, i in zip(HEAD_CASES, HEAD_IDS)]
        + [(_bite_adam, m, "adam-step%d-wd%g-gs%.3g" % m) for m in ADAM_MODES])


@pytest.mark.parametrize("check,args", [b[:2] for b in BITE], ids=[b[2] for b in BITE])
def test_bars_bite(check, args):
    """every applicable wrong float64 variant of the row's reference misses one of the row's bars by >= 10x on the row's own inputs"""
    check(*args)
