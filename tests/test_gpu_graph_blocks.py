"""The two baseline blocks added after the head path -- the nine kernels of csrc/arg_graph.hip (Actor Relation Graph) and the five of
csrc/actor_attention.hip (Actor-Transformer position embedding and attention) -- called through the C ABI (din_arg_graph_fwd / bwd,
din_actor_position_fwd / bwd, din_actor_attn_fwd / bwd) and compared element by element with float64 references written here from the
definition of each operation, on the stored fp32 operands.  The reference is never another kernel of this library.  Every buffer lies
between guard bands, padded rows hold NaN outside the view, and all of that must come back bit for bit; sources (the boxes included:
the reference project averages their corners in place) are not written; mask and keep are compared exactly; a second run of every call
returns the same bits (neither file uses atomics).

Each backward entry point is fed the float64 forward's rel / att, z and stats rounded to fp32, and its reference reads those same stored
values, so forward error does not enter a backward bar and the ReLU gate is common to both.  One more pass feeds the kernel's own saved
tensors to the backward and asks only that they are accepted (finite results, guards intact); it does not rejudge the gradients.

Inputs.  theta, phi, q, k ~ N(0, 1).  Y (ARG) is scaled by 0.1 and x, V (attention) by 0.05: the normalised slab / row then has a variance
of about 4e-3 / 2e-3, and eps = 1e-5 moved outside the square root changes rstd by 1e-3 -- at variance 1 the two terms of that change,
eps / sigma and eps / (2 sigma^2), nearly cancel (5e-6) and no fp32 bar can see it.  The mean300 rows keep scale 1 (ulp(300) = 3e-5).
Mask: the threshold sits in the widest gap near the median centre distance (as tests/test_gpu_arg._inputs chooses it), every off-diagonal
distance is >= 1e-3 thr away from it -- or, in the exact_thr row, equal to it in fp32 and fp64 alike -- so the mask is compared exactly.
ReLU: beta is moved by 0.0137 wherever |v| = |zhat gamma + beta| < max(1e-3 (|zhat gamma| + |beta|), 10 bar_v) in any clip, bar_v the fp32
error bound of v below, until no element violates it: no gate can differ by rounding and no element is left out of a comparison.

Bars are per element, (n + 1) u sum|terms| with u = 2^-24 and n the rounded operations that reach the element, counted from the kernels
(built with -ffp-contract=off: a product and its add round separately); a bar also carries the bars of the stored values it reads, pushed
through the same linear map with absolute values.  sqrtf and the division count 1 each, expf 2.
  ARG   s = dot4 / root: nfr / 4 products and adds per chain, two joining adds, sqrtf, the division: n = nfr / 4 + 5 on A = sum|theta phi| / root.
        R = e / den: the argument s - max is off by u (n A + |s - max|), expf 2: eps_j = u (n A_j + |s_j - max| + 2) relative; den = the
        pair add and the 6-level butterfly 7, the division 1: bar R_j = R_j (eps_j + sum_k R_k eps_k + 9 u) + 2^-126, exactly 0 where masked.
        Z = sum_j R_j y_j, TN products and adds in order: (TN + 2) u sum R|y|; R's error reaches it as sum_j dR_j (y_j - c) + c sum_j dR_j
        for any c, and a row of R sums to 1 within the 9 u of its normalisation: + sum bar R |y - c| + 9 u |c|, c the column mean of Y.
        mean: a thread adds ceil(TN / 4) rows, block_sum 6 + 4, the division: a tile mean has rows + 11; the Chan chain adds 4 per tile:
        bar mean = (rows + 4 nchunk + 12) u M + mean(bar Z), M the largest tile mean of |Z|.  rstd: var's relative error is
        (2 mean(|d| bar Z) + mean(bar Z^2) + 2 dev bm + bm^2) / var + (rows + 6 nchunk + 16) u with d = Z - mean, dev the largest |tile mean
        - mean| and bm the rounding part of bar mean (a tile's M2 is second order in its own mean's error, the Chan cross term first order
        in dev); the square root halves it, eps, sqrtf, division: bar rstd = rstd (rel var / 2 + 3 u).
        v = zhat gamma + beta: bar v = |gamma| rstd (bar Z + bar mean) + |zhat gamma| bar rstd / rstd + 4 u (|zhat gamma| + |beta|);
        out = sum_g relu(v_g) in order: sum over the live graphs of bar v + (NG + 1) u out.
        backward, from stored R, Z, stats: zhat is 2 roundings (3 u |zhat|).  d gamma = sum_b dv zhat: (B + 3) u sum|dv zhat| + sum|dv| 3 u |zhat|;
        d beta (B + 1) u sum|dv|.  dZ = rstd (dzhat - m1 - zhat m2) subtracts two reductions: the yard rule, max(4 yard, floor), yard = the
        slab's worst |fp32 torch - fp64 torch| of the same expression, floor (D + 6) u rstd (|dzhat| + mean|dzhat| + |zhat| mean|dzhat zhat|) plus
        zhat's 3 u pushed through, D = rows + nchunk + 16.  d Y = R^T dZ: (TN + 2) u sum R|dZ| + sum R bar dZ.  dR = dot4(dZ, Y): (nfg / 4 + 4) u
        sum|dZ y| + sum bar dZ |y|.  dS = R (dR - sum R dR) / root, the softmax backward: the yard rule again (the row's worst, the fp32 chain
        from dZ on), floor R (err dR + sum R err dR + 13 u (|dR| + sum R|dR|)) / root.  d theta = dS phi, d phi = dS^T theta: (TN + 2) u sum|dS phi|
        + sum bar dS |phi|.
  attn  s = wave_dot / root: t4 = ceil(C / 256) products and adds per chain, two joining adds, the butterfly 6, sqrtf, division: n = t4 + 11.
        softmax on one thread: eps_j as above, den N adds, the division: bar a_j = a_j (eps_j + sum a_k eps_k + (N + 2) u) + 2^-126.
        z = x + ks (a V): N products and adds, * ks, + x: bar z = ks ((N + 4) u sum a|v| + sum bar a |v|) + 2 u |x|; ks = keep / (1 - p) is
        the fp32 quotient of tests/dropout_reference.py, an operand.  mean: tc = ceil(C / 256) adds per thread, butterfly 6, 4 waves, the
        reciprocal and its product: (tc + 13) u mean|z| + mean(bar z).  rstd: rel var = (2 mean(|d| bar z) + mean(bar z^2) + bm^2) / var +
        (tc + 16) u (two-pass: second order in the mean's own error); bar rstd = rstd (rel var / 2 + 3 u).  out: rstd |gamma| (bar z + bar
        mean) + |zhat gamma| bar rstd / rstd + 5 u (|zhat gamma| + |beta|).
        backward, from stored att, stats: z is recomputed (bar z without bar a), zhat = (z - mean) rstd: bar zhat = rstd bar z + 3 u |zhat|.
        d gamma: N rows then G groups in order: (N + G + 2) u sum|g zhat| + sum|g| bar zhat; d beta (N + G + 1) u sum|g|.  dx = dZ: the yard
        rule per row, floor with D = tc + 12 and bar zhat pushed through.  dA = <dZ ks, V>: (t4 + 11) u sum|dZ ks v| + sum bar dx ks |v|.  dS:
        the yard rule per row, floor a (err dA + sum a err dA + (N + 6) u (|dA| + sum a|dA|)) / root.  dQ = dS K, dK = dS^T Q: (N + 2) u sum|dS k|
        + sum bar dS |k|.  dV = A^T (dZ ks): (N + 3) u sum a|dZ ks| + sum a ks bar dx.
  pos   the centre (b0 + b2) / 2 * image / map is 3 roundings (the halving is exact), the division by dim_t 1: the argument a is off by
        4 u |a| and sinf / cosf pass that on unchanged; they add 2 u of the result, the add of x 1: bar y = 5 u |a| + 4 u (|pe| + |x|).
        Pooled: T adds in order and the division: the mean over t of bar y + (T + 2) u mean(|pe| + |x|).  gx = gy exactly, or gy / T: 2 u |gy| / T.
test_bars_bite (CPU) shows for every row that each applicable wrong float64 variant misses a bar by >= 10x; the formulas written out by
hand are tied to float64 autograd at 1e-12 by test_*_formulas_match_autograd.

Worst |err| / bar measured on an MI355X, per stage over all rows (the row in brackets):
  ARG        R 0.19, rstd 0.070, mean 0.044, d theta 0.027, d phi 0.028, d Y 0.078 (stats_second_block); Z 0.17, out 0.060 (mean300);
             d gamma 0.37, d beta 0.33 (norm_second_block: two clips, three roundings allowed)
  attention  att 0.11, d q 0.0058, d k 0.0050 (n16_c4); mean 0.076, rstd 0.028, out 0.11, d gamma 0.18 (mean300); d v 0.064 (peaked);
             d x 0.084 (n13_c100_padded); d beta 0.12 (c260_padded); keep and mask equal everywhere
  position   y 0.38 (c516_1280rad); gx exact (T = 1 and 2: the division is exact)
With eps moved outside the square root in combine_stats and actor_attn_fwd_kernel (a scratch build) rstd misses its bar by 11x (peaked) to
7300x (n16_c4) in the 19 rows the variant applies to, while tests/test_gpu_arg.py / test_gpu_at.py still pass 11 of their 16 shapes."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import dropout_reference
from tests.test_gpu_arg import _inputs
from tests.test_gpu_at import POS_IDS, POS_SHAPES, _pos_inputs, dim_t_table
from tests.test_gpu_head_path import U32, _Buf, _check, _gen, _ratio
from tests.test_gpu_kernels import env  # noqa: F401  (the module-scoped library fixture)

F64 = torch.float64
EPS = float(np.float32(1e-5))
TINY = 2.0 ** -126
INF = float("inf")


def _ceil(a, b):
    return -(-a // b)


class _Bytes:
    """a device byte array between two guard bands of 0xA5 (the float _Buf's guard value does not fit a byte); body 0xEE until written"""

    def __init__(self, n, guard=64):
        host = torch.full((n + 2 * guard,), 0xA5, dtype=torch.uint8)
        host[guard:guard + n] = 0xEE
        self.flat, self.n, self.guard = host.cuda(), n, guard
        self.before = host.clone()

    def ptr(self):
        return self.flat.data_ptr() + self.guard

    def get(self):
        return self.flat[self.guard:self.guard + self.n].cpu()

    def bits(self):
        return self.flat.cpu()

    def untouched_outside(self):
        got = self.bits()
        return torch.equal(got[:self.guard], self.before[:self.guard]) and torch.equal(got[-self.guard:], self.before[-self.guard:])


def _intact(name, outputs, sources):
    """guard bands and padding columns of every output, and every bit of every source, are what they were before the call"""
    for k, buf in outputs.items():
        assert buf.untouched_outside(), f"{name}: wrote outside {k}"
    for k, buf in sources.items():
        diff = (buf.bits() != buf.before).nonzero().flatten().tolist()
        assert not diff, (f"{name}: the source {k} was written ({len(diff)} words, first at {diff[0] - 64} of {buf.before.numel() - 128}: "
                          f"{int(buf.before[diff[0]]):#x} -> {int(buf.bits()[diff[0]]):#x})")


def _ln_bwd(zh, rstd, dzh, dims, no_m2=False):
    """rstd (dzhat - mean(dzhat) - zhat mean(dzhat zhat)) over dims, in the dtype of its operands (float64: the reference; float32: the yard)"""
    m1, m2 = dzh.mean(dims, keepdim=True), (dzh * zh).mean(dims, keepdim=True)
    return rstd * (dzh - m1 - (0 if no_m2 else zh * m2))


def _softmax_bwd(a, da, root, no_rowsum=False):
    return a * (da - (0 if no_rowsum else (da * a).sum(-1, keepdim=True))) / root


def _variance(z, mean, dims, n, wrong):
    if wrong == "naive_variance":                                 # E[x^2] - mean^2 in fp32
        z32 = z.float()
        return ((z32 * z32).mean(dims, keepdim=True) - z32.mean(dims, keepdim=True) ** 2).double()
    return ((z - mean) ** 2).sum(dims, keepdim=True) / (n - 1 if wrong == "unbiased" else n)


def _rstd(var, wrong):
    return 1 / (var.sqrt() + EPS) if wrong == "eps_outside" else 1 / (var + EPS).sqrt()


def _row_yard(got32, want):
    return (got32.double() - want).abs().amax(-1, keepdim=True)


def _miss(bad, want, keys, exact=()):
    """the worst |bad - want| / bar over the outputs `keys`; infinite if an exactly compared output differs or a NaN appears"""
    if any(not torch.equal(bad[k], want[k]) for k in exact):
        return INF
    worst = 0.0
    for k in keys:
        r = _ratio(bad[k], want[k], want["bars"][k])
        if math.isnan(r):
            return INF
        worst = max(worst, r)
    return worst


def _close(got, ref):
    ref = ref.detach()
    return float((got.detach() - ref).abs().max()) <= 1e-12 * max(float(ref.abs().max()), 1e-300)


# =====================================================================================================================================
# 1. Actor Relation Graph (csrc/arg_graph.hip)
# =====================================================================================================================================
def _a(name, shape, kind, pad=0, shift=0.0, rounds=1):
    return dict(name=name, shape=shape, kind=kind, pad=pad, shift=shift, rounds=rounds)


ARG_ROWS = [
    _a("one_actor", (1, 1, 1, 4, 4), "all", pad=4),
    _a("tn12_ragged_chunk", (2, 12, 4, 36, 100), "mixed", pad=8),
    _a("tn63", (1, 63, 1, 8, 8), "mixed"),
    _a("tn64", (1, 64, 1, 8, 8), "mixed"),
    _a("tn65", (1, 65, 2, 8, 68), "mixed"),
    _a("tn120", (1, 120, 2, 20, 72), "mixed"),
    _a("stats_second_block", (3, 2, 100, 4, 4), "all"),
    _a("norm_second_block", (2, 36, 2, 64, 260), "mixed"),
    _a("mean300", (2, 12, 2, 16, 132), "mixed", shift=300.0),
    _a("diag_only", (2, 13, 3, 12, 40), "diag"),
    _a("rounds2", (2, 12, 2, 16, 32), "mixed", rounds=2),
    _a("exact_thr", (1, 4, 3, 8, 16), "exact"),                   # two distances of exactly thr, in fp32 and fp64 alike: `>` keeps them
]
ARG_IDS = [r["name"] for r in ARG_ROWS]
ARG_FWD = ("R", "Z", "mean", "rstd", "out")
ARG_BWD = ("d_theta", "d_phi", "d_Y", "d_gamma", "d_beta")
ARG_WRONG = ("eps_outside", "unbiased", "naive_variance", "ln_per_row", "gamma_without_actor_axis", "sqrt_nfg", "mask_ge", "diag_masked",
             "one_round", "relu_per_graph_after_sum", "no_m2", "dgamma_unscaled", "ds_no_rowsum", "dphi_untransposed", "dy_untransposed")


def _centres(boxes, rounds):
    c = boxes.double().clone()
    for _ in range(rounds):
        c[..., 0] = (c[..., 0] + c[..., 2]) / 2
        c[..., 1] = (c[..., 1] + c[..., 3]) / 2
    return c[..., :2]


def _distances(boxes, rounds):
    c = _centres(boxes, rounds)
    return (c[:, :, None] - c[:, None, :]).pow(2).sum(-1).sqrt()


def _exact_boxes():
    """centres (0,0), (3,4), (6,8), (3,4.5) and thr = 5: 0-1 and 1-2 are EXACTLY 5 (9 + 16 = 25, an exact square root in any precision), the
    other distances 0.5, 4.61, 5.41 and 10; corners centre -+ 1, so the centres are exact in fp32"""
    c = torch.tensor([[0.0, 0.0], [3.0, 4.0], [6.0, 8.0], [3.0, 4.5]])
    return torch.cat([c - 1.0, c + 1.0], -1)[None], 5.0


def _threshold(d, other):
    """the middle of the widest gap near the median distance, as tests/test_gpu_arg._inputs chooses it -- the widest of the gaps in which
    the distances `other` (one round of corner averaging fewer) give another mask"""
    v = d[d > 0].flatten().sort().values
    lo, hi = int(0.3 * len(v)), max(int(0.7 * len(v)), int(0.3 * len(v)) + 2)
    for k in (lo + (v[lo + 1:hi] - v[lo:hi - 1]).argsort(descending=True)).tolist():
        thr = float((v[k] + v[k + 1]) / 2)
        if not torch.equal(d > thr, other > thr):
            return thr
    raise AssertionError("the two centre definitions agree on every threshold")


def reference_arg(theta, phi, y, boxes, thr, gamma, beta, rounds=1, g_out=None, saved=None, wrong=None):
    """theta, phi [B,TN,NG,NFR], y [B,TN,NG,NFG], boxes [B,TN,4], gamma / beta [NG,TN,NFG] -> mask [B,TN,TN], R [B,NG,TN,TN], Z [B,NG,TN,NFG],
    mean / rstd [B,NG], out [B,TN,NFG] and, given g_out [B,TN,NFG], d_theta, d_phi, d_Y (the operands' layout), d_gamma, d_beta.  The
    backward reads saved = (R, Z, mean, rstd) -- what the kernel is handed -- or this forward's own values rounded to fp32.  With
    wrong = None the result carries bars[...] as counted in the module docstring."""
    B, TN, NG, NFR = theta.shape
    NFG = y.shape[-1]
    th, ph, yy = (t.to(F64).permute(0, 2, 1, 3) for t in (theta, phi, y))               # [B][NG][TN][*]
    ga, be = gamma.to(F64), beta.to(F64)
    if wrong == "gamma_without_actor_axis":
        ga = ga[:, :1].expand_as(ga)
    eye = torch.eye(TN, dtype=torch.bool)
    d = _distances(boxes, 1 if wrong == "one_round" else rounds)
    mask = ((d >= thr) if wrong == "mask_ge" else (d > thr)) & ~eye                      # strict; the diagonal is always kept
    if wrong == "diag_masked":
        mask = mask | eye
    root = math.sqrt(NFG if wrong == "sqrt_nfg" else NFR)
    s = (th @ ph.transpose(-1, -2) / root).masked_fill(mask[:, None], -INF)
    R = torch.softmax(s, dim=-1)
    Z = R @ yy
    dims, n = ((-1,), NFG) if wrong == "ln_per_row" else ((-2, -1), TN * NFG)
    mean = Z.mean(dims, keepdim=True)
    var = _variance(Z, mean, dims, n, wrong)
    rstd = _rstd(var, wrong)
    zh = (Z - mean) * rstd
    v = zh * ga + be
    out = v.sum(1).clamp_min(0) if wrong == "relu_per_graph_after_sum" else v.clamp_min(0).sum(1)
    slab = lambda t: t.mean((-2, -1)) if wrong == "ln_per_row" else t[..., 0, 0]          # noqa: E731  (stats are per slab)
    res = dict(mask=mask, R=R, Z=Z, mean=slab(mean), rstd=slab(rstd), out=out, zhat=zh, v=v)
    nchunk, rows = _ceil(NFG, 64), _ceil(TN, 4)
    bars = {}
    if wrong is None:
        kept = ~mask[:, None].expand_as(R)
        A = th.detach().abs() @ ph.detach().abs().transpose(-1, -2) / root
        sd, Rd, Zd, ya = s.detach(), R.detach(), Z.detach(), yy.detach().abs()
        gap = torch.where(kept, (sd - sd.max(-1, keepdim=True).values).abs(), torch.zeros_like(sd))
        e = torch.where(kept, U32 * ((NFR // 4 + 5) * A + gap + 2), torch.zeros_like(sd))
        bars["R"] = torch.where(kept, Rd * (e + (Rd * e).sum(-1, keepdim=True) + 9 * U32) + TINY, torch.zeros_like(sd))
        cen = yy.detach().mean(-2, keepdim=True)
        bars["Z"] = (TN + 2) * U32 * (Rd @ ya) + bars["R"] @ (yy.detach() - cen).abs() + 9 * U32 * cen.abs()
        tiles = torch.stack([Zd[..., k * 64:(k + 1) * 64].abs().mean((-2, -1)) for k in range(nchunk)])
        tmean = torch.stack([Zd[..., k * 64:(k + 1) * 64].mean((-2, -1)) for k in range(nchunk)])
        md, vd, rd = mean.detach(), var.detach(), rstd.detach()
        bm = (rows + 4 * nchunk + 12) * U32 * tiles.max(0).values
        bars["mean"] = bm + bars["Z"].mean((-2, -1))
        dev = (tmean - md[..., 0, 0]).abs().max(0).values
        dd = (Zd - md).abs()
        rel_var = ((2 * (dd * bars["Z"]).mean((-2, -1)) + (bars["Z"] ** 2).mean((-2, -1)) + 2 * dev * bm + bm ** 2) / vd[..., 0, 0]
                   + (rows + 6 * nchunk + 16) * U32)
        bars["rstd"] = rd[..., 0, 0] * (rel_var / 2 + 3 * U32)
        zg = (zh.detach() * ga).abs()
        bars["v"] = (ga.abs() * rd * (bars["Z"] + bars["mean"][..., None, None]) + zg * (bars["rstd"] / rd[..., 0, 0])[..., None, None]
                     + 4 * U32 * (zg + be.abs()))
        bars["out"] = (bars["v"] * (v.detach() > 0)).sum(1) + (NG + 1) * U32 * out.detach()
    if g_out is not None:
        if saved is None:
            saved = (R.float(), Z.float(), res["mean"].float(), res["rstd"].float())
        Rs, Zs = saved[0].double(), saved[1].double()
        ms, rs = saved[2].double()[..., None, None], saved[3].double()[..., None, None]
        go = g_out.double()[:, None]                                                     # [B][1][TN][NFG]
        zhs = (Zs - ms) * rs
        vs = zhs * ga + be
        gate = (vs.sum(1, keepdim=True) > 0) if wrong == "relu_per_graph_after_sum" else (vs > 0)
        dv = go * gate
        dzh = dv * ga
        dZ = _ln_bwd(zhs, rs, dzh, dims, wrong == "no_m2")
        dR = dZ @ yy.transpose(-1, -2)
        dS = _softmax_bwd(Rs, dR, root, wrong == "ds_no_rowsum")
        back = lambda t: t.permute(0, 2, 1, 3)                                           # noqa: E731
        res.update(d_gamma=(dv * ((Zs - ms) if wrong == "dgamma_unscaled" else zhs)).sum(0), d_beta=dv.sum(0),
                   d_Y=back((Rs if wrong == "dy_untransposed" else Rs.transpose(-1, -2)) @ dZ), d_theta=back(dS @ ph),
                   d_phi=back((dS if wrong == "dphi_untransposed" else dS.transpose(-1, -2)) @ th), gate=gate)
        if wrong is None:
            f32 = lambda t: t.float()                                                    # noqa: E731
            zh32 = (f32(saved[1]) - f32(saved[2])[..., None, None]) * f32(saved[3])[..., None, None]
            dzh32 = (g_out.float()[:, None] * gate) * gamma.float()
            dz32 = _ln_bwd(zh32, f32(saved[3])[..., None, None], dzh32, (-2, -1))
            ds32 = _softmax_bwd(f32(saved[0]), dz32 @ y.float().permute(0, 2, 1, 3).transpose(-1, -2), float(np.float32(root)))
            D = rows + nchunk + 16
            bzh = 3 * U32 * zhs.abs()
            mabs = lambda t: t.abs().mean((-2, -1), keepdim=True)                        # noqa: E731
            bars["d_gamma"] = (B + 3) * U32 * (dv * zhs).abs().sum(0) + (dv.abs() * bzh).sum(0)
            bars["d_beta"] = (B + 1) * U32 * dv.abs().sum(0)
            floor = ((D + 6) * U32 * rs * (dzh.abs() + mabs(dzh) + zhs.abs() * mabs(dzh * zhs))
                     + rs * (mabs(dzh * zhs) * bzh + zhs.abs() * (dzh.abs() * bzh).mean((-2, -1), keepdim=True)))
            bdz = torch.maximum(4 * (dz32.double() - dZ).abs().amax((-2, -1), keepdim=True), floor)
            ya, Rt = yy.abs(), Rs.transpose(-1, -2)
            bars["d_Y"] = back((TN + 2) * U32 * (Rt @ dZ.abs()) + Rt @ bdz)
            adR = dZ.abs() @ ya.transpose(-1, -2)
            edR = (NFG // 4 + 4) * U32 * adR + bdz @ ya.transpose(-1, -2)
            floor = Rs * (edR + (Rs * edR).sum(-1, keepdim=True) + 13 * U32 * (dR.abs() + (Rs * dR.abs()).sum(-1, keepdim=True))) / root
            bds = torch.maximum(4 * _row_yard(ds32, dS), floor)
            bars["d_theta"] = back((TN + 2) * U32 * (dS.abs() @ ph.abs()) + bds @ ph.abs())
            bars["d_phi"] = back((TN + 2) * U32 * (dS.abs().transpose(-1, -2) @ th.abs()) + bds.transpose(-1, -2) @ th.abs())
    if wrong is None:
        res["bars"] = bars
    return res


def _relu_violations(want, gamma, beta):
    """[NG][TN][NFG]: some clip has |v| under max(1e-3 (|zhat gamma| + |beta|), 10 bar_v) there"""
    zg = (want["zhat"] * gamma.double()).abs()
    need = torch.maximum(1e-3 * (zg + beta.double().abs()), 10 * want["bars"]["v"])
    return (want["v"].abs() < need).any(0)


@functools.lru_cache(maxsize=None)
def _arg_operands(name):
    row = ARG_ROWS[ARG_IDS.index(name)]
    B, TN, NG, NFR, NFG = row["shape"]
    kind = "all" if row["kind"] == "exact" else row["kind"]
    theta, phi, y, gamma, beta, boxes, thr, _mask, cot = _inputs(B, TN, NG, NFR, NFG, kind, seed=1000 + TN + NG + NFG)
    if row["kind"] == "exact":
        boxes, thr = _exact_boxes()
    elif row["rounds"] != 1:
        thr = _threshold(_distances(boxes, row["rounds"]), _distances(boxes, row["rounds"] - 1))
    thr = float(np.float32(thr))                                  # (the C ABI takes a float)
    y = row["shift"] + (1.0 if row["shift"] else 0.1) * y
    touched = 0
    for _ in range(20):
        want = reference_arg(theta, phi, y, boxes, thr, gamma, beta, row["rounds"])
        bad = _relu_violations(want, gamma, beta)
        if not bool(bad.any()):
            break
        touched += int(bad.sum())
        beta = beta + bad.float() * 0.0137
    return dict(theta=theta, phi=phi, y=y, gamma=gamma, beta=beta.float(), boxes=boxes, thr=thr, cot=cot, touched=touched)


@functools.lru_cache(maxsize=None)
def _arg_expected(name, wrong=None):
    row, o = ARG_ROWS[ARG_IDS.index(name)], _arg_operands(name)
    args = (o["theta"], o["phi"], o["y"], o["boxes"], o["thr"], o["gamma"], o["beta"], row["rounds"], o["cot"])
    if wrong is None:
        return reference_arg(*args)
    fwd = _arg_expected(name)                                     # every variant's backward reads the unchanged forward's stored values
    return reference_arg(*args, saved=(fwd["R"].float(), fwd["Z"].float(), fwd["mean"].float(), fwd["rstd"].float()), wrong=wrong)


def _arg_applies(row, wrong):
    B, TN, NG, NFR, NFG = row["shape"]
    many = TN > 1
    return {
        # variance 0.3 under the mean of 300: eps moves rstd by 1e-5, below what the fp32 rounding of Z (ulp(300) = 3e-5) leaves of it
        "eps_outside": row["shift"] == 0,
        # 1 / (2 n) of rstd, n = TN NFG.  The counted bar of rstd is that of Z, (TN + 2) u of the aggregate's TN-term sum plus R's bar,
        # carried through the variance: 2e-5 of rstd at TN = 65, so n = 4420 (1.1e-4), 8640 and 9360 (5e-5) stay under 10x; the eight
        # rows it is tried on have n <= 1200.  Under the mean of 300 the bar is that of Z's own fp32 rounding (see eps_outside)
        "unbiased": TN * NFG <= 2000 and row["shift"] == 0,
        "naive_variance": row["shift"] != 0,
        "ln_per_row": many, "gamma_without_actor_axis": many,
        "sqrt_nfg": many and NFR != NFG and row["kind"] != "diag",
        "mask_ge": row["kind"] == "exact",                        # elsewhere no distance equals the threshold
        "diag_masked": many, "one_round": row["rounds"] != 1,
        "relu_per_graph_after_sum": NG > 1,
        # R is the identity under the diagonal mask (dS is exactly 0, R^T = R), and a 1 x 1 R is its own transpose
        "ds_no_rowsum": many, "dphi_untransposed": many and row["kind"] != "diag",
        "dy_untransposed": many and row["kind"] != "diag",
    }.get(wrong, True)


def _bite_arg(name):
    row, want = ARG_ROWS[ARG_IDS.index(name)], _arg_expected(name)
    assert all(bool(torch.isfinite(want[k]).all()) for k in ARG_FWD + ARG_BWD)
    tried = 0
    for wrong in ARG_WRONG:
        if _arg_applies(row, wrong):
            tried += 1
            worst = _miss(_arg_expected(name, wrong), want, ARG_FWD + ARG_BWD, exact=("mask",))
            assert worst >= 10.0, f"{name}: the bars do not see '{wrong}' ({worst:.3g})"
    assert tried >= 3


@pytest.mark.parametrize("name", ARG_IDS)
def test_arg_rows_meet_the_input_conditions(name):
    row, o, want = ARG_ROWS[ARG_IDS.index(name)], _arg_operands(name), _arg_expected(name)
    B, TN, NG, NFR, NFG = row["shape"]
    thr, d = o["thr"], _distances(o["boxes"], row["rounds"])
    off = ~torch.eye(TN, dtype=torch.bool)[None].expand_as(d)
    near = off & ((d - thr).abs() < 1e-3 * thr)
    if row["kind"] == "exact":                                    # the distances on the threshold are the same number in fp32
        c32 = _centres(o["boxes"], 1).numpy().astype(np.float32)
        d32 = np.sqrt(((c32[:, :, None] - c32[:, None, :]) ** 2).sum(-1, dtype=np.float32), dtype=np.float32)
        assert int(near.sum()) == 4 and bool((d[near] == thr).all()) and bool((torch.from_numpy(d32)[near] == np.float32(thr)).all())
    else:
        assert not bool(near.any()), f"{name}: a centre distance within 1e-3 of the threshold {thr}"
    share = float(want["mask"][off].double().mean()) if TN > 1 else 0.0
    assert {"mixed": 0.1 < share < 0.9, "exact": 0 < share < 1, "diag": share == 1.0, "all": share == 0.0}[row["kind"]], share
    if row["rounds"] != 1:
        assert not torch.equal(want["mask"], reference_arg(o["theta"], o["phi"], o["y"], o["boxes"], thr, o["gamma"], o["beta"], 1)["mask"])
    assert not bool(_relu_violations(want, o["gamma"], o["beta"]).any()) and o["touched"] <= max(8, B * NG * TN * NFG // 20)
    assert bool((want["v"].abs() >= 10 * want["bars"]["v"]).all())                        # (mean300: 10x the fp32 error bound of v)
    if want["v"].numel() >= 100:
        live = float((want["v"] > 0).double().mean())
        assert 0.25 < live < 0.75, live
    # the backward's gate, taken from the stored fp32 values, is the forward's
    assert torch.equal(want["gate"], want["v"] > 0)
    if row["shift"]:
        assert float(want["mean"].abs().min()) > 250 and float(want["rstd"].min()) > 0.5
    elif TN > 1:
        assert float(want["rstd"].min()) > 5.0                    # variance under 0.04: eps is 2.5e-4 of it or more


def test_arg_formulas_match_autograd():
    for name in ("tn12_ragged_chunk", "rounds2", "diag_only"):
        row, o = ARG_ROWS[ARG_IDS.index(name)], _arg_operands(name)
        leaves = [o[k].double().requires_grad_(True) for k in ("theta", "phi", "y", "gamma", "beta")]
        fwd = reference_arg(*leaves[:3], o["boxes"], o["thr"], *leaves[3:], row["rounds"])
        fwd["out"].backward(o["cot"].double())
        saved = tuple(fwd[k].detach() for k in ("R", "Z", "mean", "rstd"))
        mine = reference_arg(o["theta"], o["phi"], o["y"], o["boxes"], o["thr"], o["gamma"], o["beta"], row["rounds"], o["cot"], saved)
        for k, leaf in zip(ARG_BWD, (leaves[0], leaves[1], leaves[2], leaves[3], leaves[4])):
            assert _close(mine[k], leaf.grad), (name, k)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ARG_IDS)
def test_arg_graph_against_fp64(env, name):
    lib, L, nhwc, ops = env
    row, o, want = ARG_ROWS[ARG_IDS.index(name)], _arg_operands(name), _arg_expected(name)
    B, TN, NG, NFR, NFG = row["shape"]
    bars = want["bars"]
    width = NG * (2 * NFR + NFG)
    ld = width + row["pad"]
    proj = torch.cat([o[k].reshape(B, TN, -1) for k in ("theta", "phi", "y")], -1)
    P, BX = _Buf((B, TN), width, content=proj, ld=ld), _Buf((B * TN,), 4, content=o["boxes"])
    GA, BE = _Buf((NG * TN,), NFG, content=o["gamma"]), _Buf((NG * TN,), NFG, content=o["beta"])
    GO = _Buf((B * TN,), NFG, content=o["cot"])
    three = lambda p: (p, p + 4 * NG * NFR, p + 8 * NG * NFR)                             # noqa: E731  (theta, phi, y column blocks)

    def forward():
        OUT, REL, MSK = _Buf((B * TN,), NFG), _Buf((B * NG * TN,), TN), _Bytes(B * TN * TN)
        Z, ST = _Buf((B * NG * TN,), NFG), _Buf((B * NG,), 2)
        nws = ops.arg_graph_workspace_floats(B, TN, NG, NFG, False)
        ws = torch.full((nws,), float("nan")).cuda()
        L.check(lib.din_arg_graph_fwd(*three(P.ptr()), ld, BX.ptr(), row["rounds"], o["thr"], GA.ptr(), BE.ptr(), 1e-5, B, TN, NG, NFR, NFG,
                                      OUT.ptr(), REL.ptr(), MSK.ptr(), Z.ptr(), ST.ptr(), ws.data_ptr(), nws, None))
        torch.cuda.synchronize()
        _intact(name, dict(OUT=OUT, REL=REL, MSK=MSK, Z=Z, ST=ST), dict(P=P, BX=BX, GA=GA, BE=BE))
        return OUT, REL, MSK, Z, ST

    def backward(RS, ZS, SS):
        DP, DG, DB = _Buf((B, TN), width, ld=ld), _Buf((NG * TN,), NFG), _Buf((NG * TN,), NFG)
        nws = ops.arg_graph_workspace_floats(B, TN, NG, NFG, True)
        ws = torch.full((nws,), float("nan")).cuda()
        saved = [t.bits() for t in (RS, ZS, SS)]
        L.check(lib.din_arg_graph_bwd(GO.ptr(), *three(P.ptr()), ld, GA.ptr(), BE.ptr(), RS.ptr(), ZS.ptr(), SS.ptr(), B, TN, NG, NFR, NFG,
                                      *three(DP.ptr()), ld, DG.ptr(), DB.ptr(), ws.data_ptr(), nws, None))
        torch.cuda.synchronize()
        _intact(name, dict(DP=DP, DG=DG, DB=DB), dict(GO=GO, P=P, GA=GA, BE=BE))
        assert all(torch.equal(t.bits(), w) for t, w in zip((RS, ZS, SS), saved)), f"{name}: the backward wrote into rel, z or stats"
        return DP, DG, DB

    OUT, REL, MSK, Z, ST = forward()
    assert torch.equal(MSK.get().view(B, TN, TN), want["mask"].to(torch.uint8)), f"{name}: position mask differs"
    rel = REL.get().view(B, NG, TN, TN)
    assert not bool(rel[want["mask"][:, None].expand_as(rel)].any()), f"{name}: a masked relation is not exactly 0"
    _check(name, "R", rel, want["R"], bars["R"])
    _check(name, "Z", Z.get().view(B, NG, TN, NFG), want["Z"], bars["Z"])
    _check(name, "mean", ST.get()[:, 0].view(B, NG), want["mean"], bars["mean"])
    _check(name, "rstd", ST.get()[:, 1].view(B, NG), want["rstd"], bars["rstd"])
    _check(name, "out", OUT.get().view(B, TN, NFG), want["out"], bars["out"])
    again = forward()
    assert all(torch.equal(u.bits(), v.bits()) for u, v in zip((OUT, REL, MSK, Z, ST), again)), f"{name}: forward rerun differs"

    stats = torch.stack([want["mean"], want["rstd"]], -1).float()
    stored = (_Buf((B * NG * TN,), TN, content=want["R"].float()), _Buf((B * NG * TN,), NFG, content=want["Z"].float()),
              _Buf((B * NG,), 2, content=stats))
    DP, DG, DB = backward(*stored)
    dp = DP.get()
    split = lambda w, i, c: w[..., i:i + NG * c].reshape(B, TN, NG, c)                    # noqa: E731
    _check(name, "d_theta", split(dp, 0, NFR), want["d_theta"], bars["d_theta"])
    _check(name, "d_phi", split(dp, NG * NFR, NFR), want["d_phi"], bars["d_phi"])
    _check(name, "d_Y", split(dp, 2 * NG * NFR, NFG), want["d_Y"], bars["d_Y"])
    _check(name, "d_gamma", DG.get().view(NG, TN, NFG), want["d_gamma"], bars["d_gamma"])
    _check(name, "d_beta", DB.get().view(NG, TN, NFG), want["d_beta"], bars["d_beta"])
    again = backward(*stored)
    assert all(torch.equal(u.bits(), v.bits()) for u, v in zip((DP, DG, DB), again)), f"{name}: backward rerun differs"
    own = backward(REL, Z, ST)                                    # the kernel's own saved tensors are accepted (not rejudged)
    assert all(bool(torch.isfinite(t.get()).all()) for t in own), f"{name}: the backward of the kernel's own forward is not finite"


# =====================================================================================================================================
# 2. Actor-Transformer attention (csrc/actor_attention.hip)
# =====================================================================================================================================
def _t(name, shape, pad=0, p=0.0, shift=0.0, qscale=1.0, word=None):
    return dict(name=name, shape=shape, pad=pad, p=p, shift=shift, qscale=qscale, word=word)


ATTN_ROWS = [
    _t("smallest", (1, 1, 4)),
    _t("n16_c4", (3, 16, 4)),
    _t("n13_c100_padded", (2, 13, 100), pad=8),
    _t("c1028", (2, 12, 1028)),
    _t("c260_padded", (2, 7, 260), pad=12),
    _t("mean300", (2, 12, 256), shift=300.0),
    _t("peaked", (2, 12, 64), qscale=30.0),
    _t("drop_p01", (2, 13, 100), pad=8, p=0.1, word=5),
    _t("drop_p05", (2, 16, 64), p=0.5),
]
ATTN_IDS = [r["name"] for r in ATTN_ROWS]
ATTN_SEED = 0x2468ACE
ATTN_FWD = ("att", "mean", "rstd", "out")
ATTN_BWD = ("d_q", "d_k", "d_v", "d_x", "d_gamma", "d_beta")
ATTN_WRONG = ("eps_outside", "unbiased", "naive_variance", "sqrt_n", "softmax_axis", "keep_unscaled", "dropout_on_sum", "dv_without_keep",
              "dk_untransposed", "no_m2")


def reference_attn(q, k, v, x, gamma, beta, keep, p, g_out=None, saved=None, wrong=None):
    """q, k, v, x [G,N,C], gamma / beta [C], keep bool [G,N,C] (the mask of tests/dropout_reference.py on the flat index of [G,N,C]) ->
    att [G,N,N], mean / rstd [G,N], out [G,N,C] and, given g_out, d_q, d_k, d_v, d_x, d_gamma, d_beta.  The backward reads
    saved = (att, mean, rstd) or this forward's own values rounded to fp32."""
    G, N, Cc = q.shape
    qq, kk, vv, xx, ga, be = (t.to(F64) for t in (q, k, v, x, gamma, beta))
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if p > 0 else 1.0   # the fp32 quotient: an operand
    ks = keep.double() * (1.0 if wrong == "keep_unscaled" else scale)
    root = math.sqrt(N if wrong == "sqrt_n" else Cc)
    s = qq @ kk.transpose(-1, -2) / root
    att = torch.softmax(s, dim=-2 if wrong == "softmax_axis" else -1)
    av = att @ vv
    z = (xx + av) * ks if wrong == "dropout_on_sum" else xx + ks * av
    mean = z.mean(-1, keepdim=True)
    var = _variance(z, mean, (-1,), Cc, wrong)
    rstd = _rstd(var, wrong)
    zh = (z - mean) * rstd
    out = zh * ga + be
    res = dict(att=att, mean=mean[..., 0], rstd=rstd[..., 0], out=out)
    t4, tc = _ceil(Cc, 256), _ceil(Cc, 256)                       # float4 trips of a lane (C / 4 over 64 lanes); column trips of a thread
    bars = {}
    if wrong is None:
        sd, ad, zd, va = s.detach(), att.detach(), z.detach(), vv.detach().abs()
        A = qq.detach().abs() @ kk.detach().abs().transpose(-1, -2) / root
        e = U32 * ((t4 + 11) * A + (sd - sd.max(-1, keepdim=True).values).abs() + 2)
        bars["att"] = ad * (e + (ad * e).sum(-1, keepdim=True) + (N + 2) * U32) + TINY
        bz = ks * ((N + 4) * U32 * (ad @ va) + bars["att"] @ va) + 2 * U32 * xx.detach().abs()
        bm = (tc + 13) * U32 * zd.abs().mean(-1)
        bars["mean"] = bm + bz.mean(-1)
        md, vd, rd = mean.detach(), var.detach()[..., 0], rstd.detach()
        dd = (zd - md).abs()
        rel_var = (2 * (dd * bz).mean(-1) + (bz ** 2).mean(-1) + bm ** 2) / vd + (tc + 16) * U32
        bars["rstd"] = rd[..., 0] * (rel_var / 2 + 3 * U32)
        zg = (zh.detach() * ga).abs()
        bars["out"] = rd * ga.abs() * (bz + bars["mean"][..., None]) + zg * (bars["rstd"] / rd[..., 0])[..., None] + 5 * U32 * (zg + be.abs())
    if g_out is not None:
        if saved is None:
            saved = (att.float(), res["mean"].float(), res["rstd"].float())
        a, ms, rs = saved[0].double(), saved[1].double()[..., None], saved[2].double()[..., None]
        go = g_out.double()
        zs = xx + ks * (a @ vv)
        zhs = (zs - ms) * rs
        dzh = go * ga
        dz = _ln_bwd(zhs, rs, dzh, (-1,), wrong == "no_m2")
        dzk = dz * ks
        dA = dzk @ vv.transpose(-1, -2)
        dS = _softmax_bwd(a, dA, root)
        res.update(d_gamma=(go * zhs).sum((0, 1)), d_beta=go.sum((0, 1)), d_x=dz, d_q=dS @ kk,
                   d_k=(dS if wrong == "dk_untransposed" else dS.transpose(-1, -2)) @ qq,
                   d_v=a.transpose(-1, -2) @ (dz if wrong == "dv_without_keep" else dzk))
        if wrong is None:
            ks32, a32, rs32 = ks.float(), saved[0].float(), saved[2].float()[..., None]
            zh32 = ((x.float() + ks32 * (a32 @ v.float())) - saved[1].float()[..., None]) * rs32
            dz32 = _ln_bwd(zh32, rs32, g_out.float() * gamma.float(), (-1,))
            ds32 = _softmax_bwd(a32, (dz32 * ks32) @ v.float().transpose(-1, -2), float(np.float32(root)))
            va = vv.abs()
            bzh = rs * (ks * (N + 4) * U32 * (a @ va) + 2 * U32 * xx.abs()) + 3 * U32 * zhs.abs()
            bars["d_gamma"] = (N + G + 2) * U32 * (go * zhs).abs().sum((0, 1)) + (go.abs() * bzh).sum((0, 1))
            bars["d_beta"] = (N + G + 1) * U32 * go.abs().sum((0, 1))
            mabs = lambda t: t.abs().mean(-1, keepdim=True)                              # noqa: E731
            floor = ((tc + 18) * U32 * rs * (dzh.abs() + mabs(dzh) + zhs.abs() * mabs(dzh * zhs))
                     + rs * (mabs(dzh * zhs) * bzh + zhs.abs() * (dzh.abs() * bzh).mean(-1, keepdim=True)))
            bars["d_x"] = torch.maximum(4 * _row_yard(dz32, dz), floor)
            edA = (t4 + 11) * U32 * (dzk.abs() @ va.transpose(-1, -2)) + (bars["d_x"] * ks) @ va.transpose(-1, -2)
            floor = a * (edA + (a * edA).sum(-1, keepdim=True) + (N + 6) * U32 * (dA.abs() + (a * dA.abs()).sum(-1, keepdim=True))) / root
            bds = torch.maximum(4 * _row_yard(ds32, dS), floor)
            at = a.transpose(-1, -2)
            bars["d_q"] = (N + 2) * U32 * (dS.abs() @ kk.abs()) + bds @ kk.abs()
            bars["d_k"] = (N + 2) * U32 * (dS.abs().transpose(-1, -2) @ qq.abs()) + bds.transpose(-1, -2) @ qq.abs()
            bars["d_v"] = (N + 3) * U32 * (at @ dzk.abs()) + at @ (bars["d_x"] * ks)
    if wrong is None:
        res["bars"] = bars
    return res


def _attn_keep(row):
    G, N, Cc = row["shape"]
    folded = dropout_reference.fold_seed(ATTN_SEED, row["word"])
    return torch.from_numpy(dropout_reference.keep(folded, np.arange(G * N * Cc), row["p"])).view(G, N, Cc)


@functools.lru_cache(maxsize=None)
def _attn_operands(name):
    row = ATTN_ROWS[ATTN_IDS.index(name)]
    G, N, Cc = row["shape"]
    gen = _gen("attn_" + name)
    small = 1.0 if row["shift"] else 0.05
    q = row["qscale"] * torch.randn(G, N, Cc, generator=gen)
    k = torch.randn(G, N, Cc, generator=gen)
    v = small * torch.randn(G, N, Cc, generator=gen)
    x = row["shift"] + small * torch.relu(torch.randn(G, N, Cc, generator=gen))          # shaped like the trunk's output (LayerNorm, ReLU)
    gamma, beta = 1.0 + 0.2 * torch.randn(Cc, generator=gen), 0.1 * torch.randn(Cc, generator=gen)
    return dict(q=q, k=k, v=v, x=x, gamma=gamma, beta=beta, cot=torch.randn(G, N, Cc, generator=gen), keep=_attn_keep(row))


@functools.lru_cache(maxsize=None)
def _attn_expected(name, wrong=None):
    row, o = ATTN_ROWS[ATTN_IDS.index(name)], _attn_operands(name)
    args = (o["q"], o["k"], o["v"], o["x"], o["gamma"], o["beta"], o["keep"], row["p"], o["cot"])
    if wrong is None:
        return reference_attn(*args)
    fwd = _attn_expected(name)
    return reference_attn(*args, saved=(fwd["att"].float(), fwd["mean"].float(), fwd["rstd"].float()), wrong=wrong)


def _attn_applies(row, wrong):
    G, N, Cc = row["shape"]
    return {"eps_outside": row["shift"] == 0,                     # (variance 1 under the mean of 300: eps moves rstd by 5e-6, fp32's own size)
            "naive_variance": row["shift"] != 0,
            "sqrt_n": N > 1 and N != Cc, "softmax_axis": N > 1, "dk_untransposed": N > 1,
            "keep_unscaled": row["p"] > 0, "dropout_on_sum": row["p"] > 0, "dv_without_keep": row["p"] > 0}.get(wrong, True)


def _bite_attn(name):
    row, want = ATTN_ROWS[ATTN_IDS.index(name)], _attn_expected(name)
    assert all(bool(torch.isfinite(want[k]).all()) for k in ATTN_FWD + ATTN_BWD)
    for wrong in ATTN_WRONG:
        if _attn_applies(row, wrong):
            worst = _miss(_attn_expected(name, wrong), want, ATTN_FWD + ATTN_BWD)
            assert worst >= 10.0, f"{name}: the bars do not see '{wrong}' ({worst:.3g})"


@pytest.mark.parametrize("name", ATTN_IDS)
def test_attn_rows_meet_the_input_conditions(name):
    row, o, want = ATTN_ROWS[ATTN_IDS.index(name)], _attn_operands(name), _attn_expected(name)
    G, N, Cc = row["shape"]
    att = want["att"]
    if name == "peaked":
        assert float(att.min()) <= 1e-6 and float(att.max()) >= 0.5
        assert bool(((att > 1e-10) & (att < 1e-6)).any())         # small entries that fp32 still holds as normal numbers
    elif N > 1:
        assert 1.2 / N < float(att.max(-1).values.mean()) < 0.95, "the softmax of this row is uniform or one-hot"
    share = float(o["keep"].double().mean())
    if row["p"] > 0:                                              # 5 sigma of the binomial share
        assert abs(share - (1 - row["p"])) <= 5 * math.sqrt(row["p"] * (1 - row["p"]) / (G * N * Cc))
        assert not torch.equal(o["keep"], _attn_keep(dict(row, word=None if row["word"] else 1)))
    else:
        assert share == 1.0
    if row["shift"]:
        assert float(want["mean"].min()) > 250
    else:
        assert float(want["rstd"].min()) > 5.0                    # variance under 0.04: eps is 2.5e-4 of it or more


def test_attn_formulas_match_autograd():
    for name in ("n13_c100_padded", "drop_p01", "n16_c4"):
        row, o = ATTN_ROWS[ATTN_IDS.index(name)], _attn_operands(name)
        leaves = [o[kk].double().requires_grad_(True) for kk in ("q", "k", "v", "x", "gamma", "beta")]
        fwd = reference_attn(*leaves, o["keep"], row["p"])
        fwd["out"].backward(o["cot"].double())
        saved = tuple(fwd[kk].detach() for kk in ("att", "mean", "rstd"))
        mine = reference_attn(o["q"], o["k"], o["v"], o["x"], o["gamma"], o["beta"], o["keep"], row["p"], o["cot"], saved)
        for kk, leaf in zip(ATTN_BWD, leaves):
            assert _close(mine[kk], leaf.grad), (name, kk)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ATTN_IDS)
def test_actor_attention_against_fp64(env, name):
    lib, L, nhwc, ops = env
    row, o, want = ATTN_ROWS[ATTN_IDS.index(name)], _attn_operands(name), _attn_expected(name)
    G, N, Cc = row["shape"]
    p, bars = row["p"], want["bars"]
    ld = 3 * Cc + row["pad"]
    P = _Buf((G, N), 3 * Cc, content=torch.cat([o["q"], o["k"], o["v"]], -1), ld=ld)
    X, GA, BE, GO = (_Buf(lead, Cc, content=o[kk]) for lead, kk in (((G * N,), "x"), ((1,), "gamma"), ((1,), "beta"), ((G * N,), "cot")))
    word = torch.tensor([row["word"]], dtype=torch.int64).cuda() if row["word"] is not None else None
    wptr = word.data_ptr() if word is not None else None
    three = lambda ptr: (ptr, ptr + 4 * Cc, ptr + 8 * Cc)                                 # noqa: E731  (q, k, v column blocks)

    def forward():
        OUT, ATT, ST, KP = _Buf((G * N,), Cc), _Buf((G * N,), N), _Buf((G * N,), 2), _Bytes(G * N * Cc)
        L.check(lib.din_actor_attn_fwd(*three(P.ptr()), ld, X.ptr(), GA.ptr(), BE.ptr(), 1e-5, p, ATTN_SEED, wptr, G, N, Cc, OUT.ptr(), ATT.ptr(),
                                       ST.ptr(), KP.ptr(), None))
        torch.cuda.synchronize()
        _intact(name, dict(OUT=OUT, ATT=ATT, ST=ST, KP=KP), dict(P=P, X=X, GA=GA, BE=BE))
        return OUT, ATT, ST, KP

    def backward(AS, SS):
        DP, DX, DG, DB = _Buf((G, N), 3 * Cc, ld=ld), _Buf((G * N,), Cc), _Buf((1,), Cc), _Buf((1,), Cc)
        nws = ops.actor_attn_workspace_floats(G, Cc)
        ws = torch.full((nws,), float("nan")).cuda()
        saved = [t.bits() for t in (AS, SS)]
        L.check(lib.din_actor_attn_bwd(GO.ptr(), *three(P.ptr()), ld, X.ptr(), GA.ptr(), AS.ptr(), SS.ptr(), p, ATTN_SEED, wptr, G, N, Cc,
                                       *three(DP.ptr()), ld, DX.ptr(), DG.ptr(), DB.ptr(), ws.data_ptr(), nws, None))
        torch.cuda.synchronize()
        _intact(name, dict(DP=DP, DX=DX, DG=DG, DB=DB), dict(GO=GO, P=P, X=X, GA=GA))
        assert all(torch.equal(t.bits(), w) for t, w in zip((AS, SS), saved)), f"{name}: the backward wrote into att or stats"
        return DP, DX, DG, DB

    OUT, ATT, ST, KP = forward()
    assert torch.equal(KP.get().view(G, N, Cc), o["keep"].to(torch.uint8)), f"{name}: the keep mask is not the host model's"
    _check(name, "att", ATT.get().view(G, N, N), want["att"], bars["att"])
    _check(name, "mean", ST.get()[:, 0].view(G, N), want["mean"], bars["mean"])
    _check(name, "rstd", ST.get()[:, 1].view(G, N), want["rstd"], bars["rstd"])
    _check(name, "out", OUT.get().view(G, N, Cc), want["out"], bars["out"])
    again = forward()
    assert all(torch.equal(u.bits(), w.bits()) for u, w in zip((OUT, ATT, ST, KP), again)), f"{name}: forward rerun differs"

    stored = (_Buf((G * N,), N, content=want["att"].float()), _Buf((G * N,), 2, content=torch.stack([want["mean"], want["rstd"]], -1).float()))
    DP, DX, DG, DB = backward(*stored)
    dp = DP.get()
    _check(name, "d_q", dp[..., :Cc], want["d_q"], bars["d_q"])
    _check(name, "d_k", dp[..., Cc:2 * Cc], want["d_k"], bars["d_k"])
    _check(name, "d_v", dp[..., 2 * Cc:], want["d_v"], bars["d_v"])
    _check(name, "d_x", DX.get().view(G, N, Cc), want["d_x"], bars["d_x"])
    _check(name, "d_gamma", DG.get()[0], want["d_gamma"], bars["d_gamma"])
    _check(name, "d_beta", DB.get()[0], want["d_beta"], bars["d_beta"])
    again = backward(*stored)
    assert all(torch.equal(u.bits(), w.bits()) for u, w in zip((DP, DX, DG, DB), again)), f"{name}: backward rerun differs"
    own = backward(ATT, ST)                                       # the kernel's own saved tensors are accepted (not rejudged)
    assert all(bool(torch.isfinite(t.get()).all()) for t in own), f"{name}: the backward of the kernel's own forward is not finite"


# =====================================================================================================================================
# 3. Actor-Transformer position embedding
# =====================================================================================================================================
POS_ROWS = list(POS_SHAPES[2:]) + [(1, 2, 2, 516, (720, 1280), (22, 40), False), (1, 2, 2, 516, (720, 1280), (22, 40), True)]
POS_ROW_IDS = list(POS_IDS[2:]) + ["c516_1280rad", "c516_1280rad_pooled"]
POS_WRONG = ("halves_swapped", "sin_cos_swapped", "feature_px", "pooled_sum", "bwd_no_division")


def reference_position(x, boxes, dim_t, image_size, out_size, pool, gy=None, wrong=None):
    """x [B,T,N,C], boxes [B,T,N,4] (feature px), dim_t fp32 [C/2] -> y = x + PE(box centre in image px) [B,T,N,C], its mean over T when
    pool, and gx [B,T,N,C] given gy.  x half first, then y half; inside a half sin on even, cos on odd indices."""
    B, T, N, Cc = x.shape
    b, dt = boxes.double(), dim_t.double()
    sx, sy = (1.0, 1.0) if wrong == "feature_px" else (image_size[1] / out_size[1], image_size[0] / out_size[0])
    cx, cy = (b[..., 0] + b[..., 2]) / 2 * sx, (b[..., 1] + b[..., 3]) / 2 * sy
    if wrong == "halves_swapped":
        cx, cy = cy, cx
    arg = torch.cat([cx[..., None] / dt, cy[..., None] / dt], -1)
    odd = (torch.arange(Cc // 2) % 2 == 1).repeat(2)
    pe = torch.where(odd != (wrong == "sin_cos_swapped"), arg.cos(), arg.sin())
    y = pe + x.double()
    bar = 5 * U32 * arg.abs() + 4 * U32 * (pe.abs() + x.double().abs())
    if pool:
        y = y.sum(1) if wrong == "pooled_sum" else y.mean(1)
        bar = bar.mean(1) + (T + 2) * U32 * (pe.abs() + x.double().abs()).mean(1)
    res = dict(y=y, largest=float(arg.abs().max()))
    if gy is not None:
        g = gy.double()
        res["gx"] = (g[:, None] / (1 if wrong == "bwd_no_division" else T)).expand(B, T, N, Cc) if pool else g
    if wrong is None:
        res["bars"] = dict(y=bar)
        if gy is not None:
            res["bars"]["gx"] = (2 * U32 * res["gx"].abs()) if pool else torch.zeros_like(res["gx"])
    return res


@functools.lru_cache(maxsize=None)
def _pos_operands(i):
    B, T, N, Cc, image_size, out_size, pool = POS_ROWS[i]
    x, boxes, cot = _pos_inputs(B, T, N, Cc, out_size, seed=2000 + T + N + Cc)
    return dict(x=x, boxes=boxes, gy=cot[:, 0].contiguous() if pool else cot, dim_t=dim_t_table(Cc))


def _pos_expected(i, wrong=None):
    B, T, N, Cc, image_size, out_size, pool = POS_ROWS[i]
    o = _pos_operands(i)
    return reference_position(o["x"], o["boxes"], o["dim_t"], image_size, out_size, pool, o["gy"], wrong)


def _bite_position(i):
    B, T, N, Cc, image_size, out_size, pool = POS_ROWS[i]
    want = _pos_expected(i)
    for wrong in POS_WRONG:
        if wrong in ("pooled_sum", "bwd_no_division") and not (pool and T > 1):
            continue
        worst = _miss(_pos_expected(i, wrong), want, ("y", "gx"))
        assert worst >= 10.0, f"{POS_ROW_IDS[i]}: the bars do not see '{wrong}' ({worst:.3g})"


def test_position_rows_and_formula():
    for i, (B, T, N, Cc, image_size, out_size, pool) in enumerate(POS_ROWS):
        o, want = _pos_operands(i), _pos_expected(i)
        if image_size == (720, 1280):
            assert want["largest"] > 900 and Cc > 2 * 256          # arguments of up to 1280 rad (one ulp: 1e-4); a third column trip
        xs = o["x"].double().requires_grad_(True)
        reference_position(xs, o["boxes"], o["dim_t"], image_size, out_size, pool)["y"].backward(o["gy"].double())
        assert _close(want["gx"], xs.grad)


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(POS_ROWS)), ids=POS_ROW_IDS)
def test_actor_position_against_fp64(env, i):
    lib, L, nhwc, ops = env
    B, T, N, Cc, image_size, out_size, pool = POS_ROWS[i]
    name, o, want = POS_ROW_IDS[i], _pos_operands(i), _pos_expected(i)
    rows_out = B * N if pool else B * T * N
    X, BX, DT = _Buf((B * T * N,), Cc, content=o["x"]), _Buf((B * T * N,), 4, content=o["boxes"]), _Buf((1,), Cc // 2, content=o["dim_t"])
    GY = _Buf((rows_out,), Cc, content=o["gy"])

    def run():
        Y, GX = _Buf((rows_out,), Cc), _Buf((B * T * N,), Cc)
        L.check(lib.din_actor_position_fwd(X.ptr(), BX.ptr(), DT.ptr(), float(image_size[1]), float(image_size[0]), float(out_size[1]),
                                           float(out_size[0]), B, T, N, Cc, int(pool), Y.ptr(), None))
        L.check(lib.din_actor_position_bwd(GY.ptr(), B, T, N, Cc, int(pool), GX.ptr(), None))
        torch.cuda.synchronize()
        _intact(name, dict(Y=Y, GX=GX), dict(X=X, BX=BX, DT=DT, GY=GY))
        return Y, GX

    Y, GX = run()
    _check(name, "y", Y.get().view(want["y"].shape), want["y"], want["bars"]["y"])
    _check(name, "gx", GX.get().view(B, T, N, Cc), want["gx"], want["bars"]["gx"])
    again = run()
    assert torch.equal(Y.bits(), again[0].bits()) and torch.equal(GX.bits(), again[1].bits()), f"{name}: rerun differs"


# =====================================================================================================================================
# the bars bite: every row (CPU)
# =====================================================================================================================================
BITE = ([(_bite_arg, n, "arg-" + n) for n in ARG_IDS] + [(_bite_attn, n, "attn-" + n) for n in ATTN_IDS]
        + [(_bite_position, i, "pos-" + n) for i, n in enumerate(POS_ROW_IDS)])


@pytest.mark.parametrize("check,arg", [b[:2] for b in BITE], ids=[b[2] for b in BITE])
def test_bars_bite(check, arg):
    """every applicable wrong float64 variant of the row's reference misses one of the row's bars by >= 10x on the row's own inputs"""
    check(arg)
