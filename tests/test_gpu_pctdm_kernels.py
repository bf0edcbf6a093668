"""The PCTDM kernels -- the three of csrc/lstm.hip and the five of csrc/pctdm_attention.hip -- called through the C ABI (din_lstm_fwd / bwd,
din_pctdm_pool_fwd / bwd, din_pctdm_att_fwd / bwd and the two workspace queries) and compared element by element with float64 references
written here from the definition of each operation, on the stored fp32 operands.  The reference is never another kernel of this library.
Every buffer lies between guard bands and is poisoned before the call; guards must come back bit for bit, sources are not written, a
second run of every call returns the same bits (neither file uses atomics).  tests/test_gpu_pctdm.py keeps its one-number-per-tensor
comparison against torch.nn.LSTM and the fixtures; this module judges every element, the saved tensors (gates, cells, winner, gamma,
h_prev) and the workspace included.

LSTM forward: every step is judged on its own.  A bar pushed with absolute values through the recurrence grows by sum_k |w_jk|, about
0.5 sqrt(H), per step and is useless after three; din_lstm_fwd returns h, cells and gates of every step, so for step k of direction d the
reference takes the KERNEL'S OWN stored fp32 h and c of step k - 1 (zeros at k = 0) and forms that one step in float64.  LSTM backward:
din_lstm_bwd is fed the float64 forward's gates and cells rounded to fp32 and its reference reads those same stored values, so forward
error does not enter a backward bar; dh of step k uses the kernel's own stored d_pre of the step after, the cell-gradient carry (gain
f <= 1) is chained in the reference.  One more pass feeds the kernel's own forward to the backward and asks that h_prev is the shifted h
bit for bit (the same two operands, the same product).  Pool and attention: att_bwd is fed the float64 forward's gamma rounded to fp32.

Bars are per element, (n + 1) u sum|terms| with u = 2^-24 and n the rounded operations that reach the element, counted from the kernels
(built with -ffp-contract=off: a product and its add round separately); a bar also carries the bars of the values it reads, pushed through
the same map with absolute values.  The division counts 1, expf 2 (the project's count).  tanhf counts 2, like expf: the ROCm installation
this was written against carries no accuracy table of the device library's tanhf, so it is counted as expf is; it is the only constant
here that is not read off the code.  2^-126 is added where a result can leave the normal range.
  lstm  z = pre + W h_prev: wave_rows_dot does t = ceil(H / 64) fmaf per lane (4-byte loads, H % 4 != 0) or 4 ceil(H / 256) (16-byte
        loads), 6 butterfly adds, then the add of pre: n = t + 7, bar z = (n + 1) u (|pre| + sum |w| |h_prev|); exactly 0 at k = 0.
        gate = act(z): act'(z) bar z + c u |gate| + 2^-126; sigmoid c = 4 (expf 2, the add, the division), tanh c = 3 (tanhf 2, + 1).
        c = f c_prev + i g from the stored gates and the stored c_prev: 3 u (|f c_prev| + |i g|).  h = o tanh(c) from the stored o and c:
        tanhf 2, the product 1: 4 u |h|.
        backward, from stored gates / cells: dh = g_out + W^T d_pre_next, always 16-byte loads over 4H: n = 4 ceil(4H / 256) + 7,
        bar dh = (n + 1) u (|g_out| + sum |w| |d_pre_next|), 0 at the last step.  tc = tanhf(c): 1 - tc^2 is off by u (6 tc^2 + (1 - tc^2)).
        term = dh o (1 - tc^2): bar dh |o (1 - tc^2)| + |dh o| u (6 tc^2 + (1 - tc^2)) + 3 u |term|.  dcv = term + carry, carry = dcv_next
        f_next: bar dcv = bar term + bar carry + 2 u (|term| + |carry|), bar carry = f bar dcv + u |carry|: linear in S.  The quarters
        dcv g i (1 - i), dcv c_prev f (1 - f), dcv i (1 - g^2), dh tc o (1 - o) are products of stored factors: the pushed-through bar + 7 u
        of the value + u of the other factors for the subtraction (2 u for 1 - g^2: the square rounds too); where the stored factor makes
        1 - g exactly 0, and in the forget quarter of a first step, the bar is 0: exact zeros are expected.  h_prev: 4 u |h|, exactly 0
        at the first step of each direction.  Workspace after the call: W_hh^T bit for bit; dc = dcv_0 f_0 within bar carry.
  pool  pooled and winner exact (pooled by its bits: a tie keeps the first half's, signed zeros included).  context: n adds in order and
        the division: (n + 2) u mean|pooled|.  pool_bwd: g_context / n and one add: 3 u (|g_pooled| + |g_context| / n) on the winning
        half, exactly 0 on the other.
  att   a = src + ctx is off by u |a|; t = tanhf(a): bar t = (1 - t^2) u |a| + 2 u |t|.  score: ceil(h / 64) fmaf, the butterfly 6, + b_e:
        n = ceil(h / 64) + 7, bar s = (n + 1) u (sum |w t| + |b_e|) + sum |w| bar t.  Team softmax on one thread (m = n / 2; a common shift
        of the scores, the maximum's own error included, cancels): eps_j = bar s_j + u (|s_j - max| + 2) relative, the m adds, the division:
        bar gamma_j = gamma_j (eps_j + sum_k gamma_k eps_k + (m + 2) u) + 2^-126.  y = p + p gamma: |p| bar gamma + 3 u (|p| + |p gamma|).
        backward, from stored gamma: d gamma = <g_y, p>: (ceil(h / 64) + 7) u sum |g_y p|.  ds = gamma (d gamma - sum gamma d gamma)
        subtracts a reduction: the yard rule, max(4 yard, floor), yard = the team's worst |fp32 torch - fp64 torch| of the same
        expression, floor gamma (bar dg + sum gamma bar dg + (m + 6) u (|dg| + sum gamma |dg|)), as dS in tests/test_gpu_graph_blocks.py.
        d_src = ds w (1 - t^2): bar ds |w| (1 - t^2) + |ds w| (2 |t| bar t + 2 u) + 3 u |d_src|.  d_ctx: n adds in order: (n + 1) u sum |d_src| +
        sum bar d_src.  d_w_e: n products and adds per frame, G frames in order: (n + G + 2) u sum |ds t| + sum (bar ds |t| + |ds| bar t).
        d_b_e: n adds per frame, G frames: (n + G + 1) u sum |ds| + sum bar ds.  d_pooled = g_y + g_y gamma: 3 u (|g_y| + |g_y gamma|).
  dW_hh ops._lstm_dw_hh is one call of the weight-gradient contraction per direction: float64 d_pre^T h_prev of the same fp32 operands,
        judged by the rule tests/test_gpu_wgrad.py applies to fp32 rows (its `rel` against its BAR["fp32"], imported, not restated); the
        kernel din_conv_kernel_names reports for the descriptor is printed.

test_bars_bite (CPU) shows for every row that each applicable wrong variant misses a bar by >= 10x; test_honest_fp32_* (CPU) shows that an
fp32 torch evaluation stays under every bar of every row, so the bars hold for the reference alone; test_*_formulas_match_autograd ties
the backward formulas written out here to float64 autograd through tests/pctdm_reference.py at 1e-12.  Variants that do not apply:
  hprev_dir1_shifted_wrong   needs S > 1 and D = 2: not s1_two_directions, not one_fwd_chunk (D = 1)
  fast_tanh                  one variant over the LSTM forward (gates, h) and backward (tc): the worse of the two counts; at S = 1 with 32
                             elements only the forward sees it by 10x.  It never applies to the attention rows: tanh reaches their
                             outputs only inside sums weighted by w_e and as 1 - t^2, where the rewrite's absolute error of about u lies
                             inside the counted bars (0.13 to 0.85 of them); what catches the rewrite is the LSTM, where tanh values are
                             outputs themselves
  ties_to_second             only the ties row has ties
  dctx_missing_last          not teams_of_one (n = 2: ds, and with it d_src, is exactly 0) and not peaked (the last player's ds is 1e-3 of
                             its bar there)
  dbe_one_team               never: a team's ds sums to t (1 - sum gamma), the rounding of the stored gamma alone, with or without the
                             second team -- d_b_e is 0 in exact arithmetic and both values lie far inside its bar (at most 1.4e-3 of it)
carry_without_f and dc_not_reset apply at S = 1 too: they are seen in the dc left in the workspace.

Worst |err| / bar measured on an MI355X, per stage over all rows (the row in brackets; every row: profiles/pctdm_test_margins.txt):
  lstm  gates 0.79, d_pre_o 0.44 (h1024_lds_ceiling); cells 0.63, h 0.73, d_pre_i 0.31, d_pre_f 0.29, d_pre_g 0.27, h_prev 0.75
        (launcher); dc 0.30 (s1_two_directions); W_hh^T, the first-step zeros and the shifted h equal everywhere
  pool  context 0.30 (saturated); d_lstm_out 0.54 (launcher); pooled and winner equal everywhere
  att   gamma 0.059, d_b_e 0.013 (h1); y 0.31 (peaked); d_pooled 0.48 (saturated); d_src 0.23 (h257_five_frames); d_ctx 0.075,
        d_w_e 0.019 (h64)
The smallest margin is 1.26 (gates at H = 1024); the bars are the counts above and were not moved towards these figures.  An fp32 torch
evaluation on the CPU reaches 0.64 of the same bars (test_honest_fp32_*).
With tanhf replaced by 1 - 2 / (1 + expf(2x)) in lstm_fwd_step_kernel (a scratch build) every one of the 13 LSTM rows fails at its gates,
1.2x (saturated) to 2.6e4x (tiny) over the bar, while tests/test_gpu_pctdm.py::test_lstm_matches_float64_torch_lstm passes all 6 shapes."""
import ctypes as C
import functools
import math

import pytest
import torch

from tests import pctdm_reference as R
from tests.test_gpu_graph_blocks import _Bytes, _close, _intact
from tests.test_gpu_head_path import U32, _Buf, _check, _gen, _ratio
from tests.test_gpu_kernels import env  # noqa: F401  (the module-scoped library fixture)

F64, F32 = torch.float64, torch.float32
TINY = 2.0 ** -126
INF = float("inf")
C_SIG, C_TANH = 4, 3


def _ceil(a, b):
    return -(-a // b)


def _tanh(x, fast=False):
    """tanh, or what a fast-math rewrite of tanhf computes: 1 - 2 / (1 + exp(2 x)) evaluated in fp32"""
    if fast:
        x32 = x.float()
        return (1 - 2 / (1 + torch.exp(2 * x32))).to(x.dtype)
    return torch.tanh(x)


def _bits32(t):
    return t.contiguous().view(torch.int32)


def _worse(worst, r):
    """the larger of the two ratios; a NaN (an element the kernel left poisoned) counts as an infinite miss"""
    return INF if math.isnan(r) or math.isnan(worst) else max(worst, r)


# =====================================================================================================================================
# 1. LSTM (csrc/lstm.hip)
# =====================================================================================================================================
HS, RC_F, RC_B = 8, 16, 8                                         # hidden units per workgroup; rows per LDS chunk, forward / backward


def _l(name, shape, pre=1.0, w=1.0):
    return dict(name=name, shape=shape, pre=pre, w=w)


LSTM_ROWS = [
    _l("s1_two_directions", (2, 1, 2, 8)),                        # first and last step at once
    _l("h4_bwd_chunk_plus_1", (9, 3, 2, 4)),                      # H below the 8-unit slice; one backward chunk + 1
    _l("one_fwd_chunk", (16, 2, 1, 12)),
    _l("fwd_chunk_plus_1", (17, 3, 2, 12)),
    _l("one_bwd_chunk_three_slices", (8, 2, 2, 20)),              # three slices of 8 units, the last partial
    _l("saturated", (3, 5, 2, 20), pre=30.0),                     # gates that round to 0 / 1
    _l("tiny", (3, 4, 2, 20), pre=1e-3, w=1e-2),                  # tiny arguments, where relative accuracy is lost first
    _l("h64", (3, 3, 2, 64)),                                     # one full lane stride
    _l("h65", (3, 3, 2, 65)),                                     # one more: 4-byte loads forward, n4 = 65 backward
    _l("h130_scalar", (5, 3, 2, 130)),                            # 4-byte loads over more than one lane stride
    _l("h33_transpose_edge", (4, 2, 2, 33)),
    _l("h1024_lds_ceiling", (9, 2, 2, 1024)),
    _l("launcher", (20, 12, 2, 1000)),
]
EXTRA_ROWS = [_l("dw_h20", (3, 5, 2, 20))]                        # (operands of the dW_hh test only)
LSTM_IDS = [r["name"] for r in LSTM_ROWS]
LSTM_FWD = ("gates", "cells", "h")
LSTM_BWD = ("d_pre_i", "d_pre_f", "d_pre_g", "d_pre_o", "h_prev", "dc")
LSTM_WRONG_BWD = ("fast_tanh", "c_for_c_prev", "carry_without_f", "dc_not_reset", "hprev_dir1_shifted_wrong", "one_minus_tc")


def _lstm_row(name):
    return next(r for r in LSTM_ROWS + EXTRA_ROWS if r["name"] == name)


@functools.lru_cache(maxsize=None)
def _lstm_operands(name):
    row = _lstm_row(name)
    Rr, S, D, H = row["shape"]
    gen = _gen("pctdm_lstm_" + name)
    pre = row["pre"] * torch.randn(Rr, S, D, 4 * H, generator=gen)
    w = row["w"] * (torch.rand(D, 4 * H, H, generator=gen) * 2 - 1) / H ** 0.5
    return dict(pre=pre, w=w, cot=torch.randn(Rr, S, D, H, generator=gen))


def _walk(S, d, k):
    """position of step k of direction d, the position before it in the walk and the one after"""
    return (k, k - 1, k + 1) if d == 0 else (S - 1 - k, S - k, S - 2 - k)


def lstm_forward(pre, w, dtype=F64, wrong=None):
    """pre [R,S,D,4H], w [D,4H,H] -> h, cells [R,S,D,H], gates [R,S,D,4H]: the whole recurrence in `dtype` (float64: what the backward is
    fed; float32: the stand-in for an honest kernel)"""
    Rr, S, D, H4 = pre.shape
    H = H4 // 4
    p, ww = pre.to(dtype), w.to(dtype)
    h, c, g = p.new_zeros(Rr, S, D, H), p.new_zeros(Rr, S, D, H), p.new_zeros(Rr, S, D, H4)
    fast = wrong == "fast_tanh"
    for d in range(D):
        hv, cv = p.new_zeros(Rr, H), p.new_zeros(Rr, H)
        for k in range(S):
            pos = _walk(S, d, k)[0]
            z = p[:, pos, d] + hv @ ww[d].t() if k else p[:, pos, d]
            gi, gf, go = torch.sigmoid(z[:, :H]), torch.sigmoid(z[:, H:2 * H]), torch.sigmoid(z[:, 3 * H:])
            gg = _tanh(z[:, 2 * H:3 * H], fast)
            cv = gf * cv + gi * gg
            hv = go * _tanh(cv, fast)
            h[:, pos, d], c[:, pos, d], g[:, pos, d] = hv, cv, torch.cat([gi, gf, gg, go], -1)
    return dict(h=h, cells=c, gates=g)


def lstm_fwd_judge(pre, w, got):
    """the worst |err| / bar of the stored gates, cells and h of a forward, every step judged from the stored state of the step before"""
    Rr, S, D, H4 = pre.shape
    H = H4 // 4
    n = (4 * _ceil(H, 256) if H % 4 == 0 else _ceil(H, 64)) + 7
    pp, ww = pre.double(), w.double()
    wa = ww.abs()
    hs, cs, gs = got["h"].double(), got["cells"].double(), got["gates"].double()
    cact = torch.cat([torch.full((2 * H,), float(C_SIG)), torch.full((H,), float(C_TANH)), torch.full((H,), float(C_SIG))]).double()
    worst = dict.fromkeys(LSTM_FWD, 0.0)
    for d in range(D):
        for k in range(S):
            pos, prev, _ = _walk(S, d, k)
            if k == 0:
                z, bz, cp = pp[:, pos, d], torch.zeros(Rr, H4, dtype=F64), torch.zeros(Rr, H, dtype=F64)
            else:
                hp, cp = hs[:, prev, d], cs[:, prev, d]
                z = pp[:, pos, d] + hp @ ww[d].t()
                bz = (n + 1) * U32 * (pp[:, pos, d].abs() + hp.abs() @ wa[d].t())
            sg, tg = torch.sigmoid(z), torch.tanh(z[:, 2 * H:3 * H])
            gate = torch.cat([sg[:, :2 * H], tg, sg[:, 3 * H:]], -1)
            slope = torch.cat([(sg * (1 - sg))[:, :2 * H], 1 - tg * tg, (sg * (1 - sg))[:, 3 * H:]], -1)
            bar = slope * bz + cact * U32 * gate.abs() + TINY
            worst["gates"] = _worse(worst["gates"], _ratio(gs[:, pos, d], gate, bar))
            gi, gf, gg, go = gs[:, pos, d].split(H, -1)
            worst["cells"] = _worse(worst["cells"], _ratio(cs[:, pos, d], gf * cp + gi * gg, 3 * U32 * ((gf * cp).abs() + (gi * gg).abs()) + TINY))
            hw = go * torch.tanh(cs[:, pos, d])
            worst["h"] = _worse(worst["h"], _ratio(hs[:, pos, d], hw, 4 * U32 * hw.abs() + TINY))
    return worst


def lstm_backward(cot, gates, cells, w, dtype=F64, wrong=None, stale_dc=None):
    """g_out [R,S,D,H], the stored gates / cells, w -> d_pre [R,S,D,4H], h_prev [R,S,D,H], dc [R,D,H] (what is left in the workspace)"""
    Rr, S, D, H = cells.shape
    go_, gs, cs, ww = (t.to(dtype) for t in (cot, gates, cells, w))
    d_pre, h_prev, dc_out = gs.new_zeros(Rr, S, D, 4 * H), gs.new_zeros(Rr, S, D, H), gs.new_zeros(Rr, D, H)
    fast = wrong == "fast_tanh"
    for d in range(D):
        dc = stale_dc[:, d].to(dtype) if wrong == "dc_not_reset" else gs.new_zeros(Rr, H)
        dpn = None
        for k in range(S - 1, -1, -1):
            pos, prev, _ = _walk(S, d, k)
            gi, gf, gg, go = gs[:, pos, d].split(H, -1)
            tc = _tanh(cs[:, pos, d], fast)
            cp = cs[:, pos, d] if wrong == "c_for_c_prev" else (cs[:, prev, d] if k else torch.zeros_like(tc))
            dh = go_[:, pos, d] + (dpn @ ww[d] if dpn is not None else 0)
            dcv = dh * go * ((1 - tc) if wrong == "one_minus_tc" else (1 - tc * tc)) + dc
            dc = dcv if wrong == "carry_without_f" else dcv * gf
            dpn = torch.cat([dcv * gg * gi * (1 - gi), dcv * cp * gf * (1 - gf), dcv * gi * (1 - gg * gg), dh * tc * go * (1 - go)], -1)
            d_pre[:, pos, d] = dpn
            src = prev
            if wrong == "hprev_dir1_shifted_wrong" and d == 1:
                src = pos - 1
            if (k > 0) if src == prev else (0 <= src < S):
                h_prev[:, pos, d] = gs[:, src, d, 3 * H:] * _tanh(cs[:, src, d], fast)
        dc_out[:, d] = dc
    return dict(d_pre=d_pre, h_prev=h_prev, dc=dc_out)


def lstm_bwd_judge(cot, gates, cells, w, got):
    """the worst |err| / bar of the four d_pre quarters, h_prev and the dc left in the workspace; dh of a step reads got's own d_pre of
    the step after"""
    Rr, S, D, H = cells.shape
    n = 4 * _ceil(4 * H, 256) + 7
    go_, gs, cs, ww = (t.double() for t in (cot, gates, cells, w))
    wa = ww.abs()
    dp, hpv, dcg = got["d_pre"].double(), got["h_prev"].double(), got["dc"].double()
    worst = dict.fromkeys(LSTM_BWD, 0.0)

    def judge(key, have, want, bar):
        worst[key] = _worse(worst[key], _ratio(have, want, bar))

    for d in range(D):
        carry, bcarry = torch.zeros(Rr, H, dtype=F64), torch.zeros(Rr, H, dtype=F64)
        for k in range(S - 1, -1, -1):
            pos, prev, nxt = _walk(S, d, k)
            gi, gf, gg, go = gs[:, pos, d].split(H, -1)
            if k == S - 1:
                dh, bdh = go_[:, pos, d], torch.zeros(Rr, H, dtype=F64)
            else:
                dh = go_[:, pos, d] + dp[:, nxt, d] @ ww[d]
                bdh = (n + 1) * U32 * (go_[:, pos, d].abs() + dp[:, nxt, d].abs() @ wa[d])
            tc = torch.tanh(cs[:, pos, d])
            s2 = 1 - tc * tc
            term = dh * go * s2
            bterm = bdh * (go * s2).abs() + (dh * go).abs() * U32 * (6 * tc * tc + s2) + 3 * U32 * term.abs()
            dcv = term + carry
            bdcv = bterm + bcarry + 2 * U32 * (term.abs() + carry.abs()) + TINY
            cp = cs[:, prev, d] if k else torch.zeros(Rr, H, dtype=F64)

            def quarter(key, lead, blead, rest, one_minus, extra):
                v = lead * rest * one_minus
                bar = blead * (rest * one_minus).abs() + 7 * U32 * v.abs() + extra * U32 * (lead * rest).abs() * (one_minus != 0) + TINY * (v != 0)
                judge(key, dp[:, pos, d, {"i": 0, "f": 1, "g": 2, "o": 3}[key[-1]] * H:][:, :H], v, bar)

            quarter("d_pre_i", dcv, bdcv, gg * gi, 1 - gi, 1)
            quarter("d_pre_f", dcv, bdcv, cp * gf, 1 - gf, 1)
            quarter("d_pre_g", dcv, bdcv, gi, 1 - gg * gg, 2)
            quarter("d_pre_o", dh, bdh, tc * go, 1 - go, 1)
            if k:
                hw = gs[:, prev, d, 3 * H:] * torch.tanh(cs[:, prev, d])
                judge("h_prev", hpv[:, pos, d], hw, 4 * U32 * hw.abs() + TINY)
            else:
                judge("h_prev", hpv[:, pos, d], torch.zeros(Rr, H, dtype=F64), torch.zeros(Rr, H, dtype=F64))
            carry = dcv * gf
            bcarry = bdcv * gf + U32 * carry.abs() + TINY * (carry != 0)
        judge("dc", dcg[:, d], carry, bcarry)
    return worst


@functools.lru_cache(maxsize=None)
def _lstm_stored(name):
    """the float64 forward rounded to fp32 (what the backward is fed) and the float64 backward of it"""
    o = _lstm_operands(name)
    f = lstm_forward(o["pre"], o["w"])
    stored = {k: v.float() for k, v in f.items()}
    return stored, lstm_backward(o["cot"], stored["gates"], stored["cells"], o["w"])


def _lstm_applies(row, wrong):
    Rr, S, D, H = row["shape"]
    return {"hprev_dir1_shifted_wrong": S > 1 and D == 2}.get(wrong, True)


def _bite_lstm(name):
    row, o = _lstm_row(name), _lstm_operands(name)
    stored, back = _lstm_stored(name)
    fast = max(lstm_fwd_judge(o["pre"], o["w"], lstm_forward(o["pre"], o["w"], F32, "fast_tanh")).values())
    for wrong in LSTM_WRONG_BWD:
        if _lstm_applies(row, wrong):
            bad = lstm_backward(o["cot"], stored["gates"], stored["cells"], o["w"], F64, wrong, stale_dc=back["dc"])
            worst = max(lstm_bwd_judge(o["cot"], stored["gates"], stored["cells"], o["w"], bad).values())
            if wrong == "fast_tanh":                              # one variant: the rewrite in the forward's gates and h, and in the backward's tc
                worst = max(worst, fast)
            assert worst >= 10.0, f"{name}: the bars do not see '{wrong}' ({worst:.3g})"


@pytest.mark.parametrize("name", LSTM_IDS)
def test_lstm_rows_meet_the_input_conditions(name):
    Rr, S, D, H = _lstm_row(name)["shape"]
    stored, back = _lstm_stored(name)
    fchunks, bchunks, slices = _ceil(Rr, RC_F), _ceil(Rr, RC_B), _ceil(H, HS)
    want = {"s1_two_directions": S == 1 and D == 2,
            "h4_bwd_chunk_plus_1": H < HS and Rr == RC_B + 1 and bchunks == 2,
            "one_fwd_chunk": Rr == RC_F and fchunks == 1,
            "fwd_chunk_plus_1": Rr == RC_F + 1 and fchunks == 2,
            "one_bwd_chunk_three_slices": Rr == RC_B and bchunks == 1 and slices == 3 and H % HS != 0,
            "h64": H == 64 and H % 4 == 0, "h65": H == 65 and H % 4 != 0 and (4 * H) >> 2 == 65,
            "h130_scalar": H % 4 != 0 and _ceil(H, 64) > 1,
            "h33_transpose_edge": H == 33,
            "h1024_lds_ceiling": H == 1024 and 4 * (RC_F * H + 4 * HS * RC_F) == 66 * 1024 and 4 * (RC_B * 4 * H + HS * RC_B) > 128 * 1024,
            "launcher": (Rr, S, D, H) == (20, 12, 2, 1000)}.get(name, True)
    assert want, name
    g = stored["gates"]
    sig = torch.cat([g[..., :2 * H], g[..., 3 * H:]], -1)
    if name == "saturated":
        assert float(((sig == 0) | (sig == 1)).float().mean()) > 0.2 and float((g[..., 2 * H:3 * H].abs() == 1).float().mean()) > 0.2
        assert bool((sig == 1).any()) and bool((sig == 0).any())
        # exact zeros are expected (and asked for: their bar is 0) where 1 - g is 0
        assert bool((back["d_pre"][..., :H][g[..., :H] == 1] == 0).all()) and int((g[..., :H] == 1).sum()) > 0
    elif name == "tiny":
        assert float(g[..., 2 * H:3 * H].abs().max()) < 1e-2 and float(stored["cells"].abs().max()) < 1e-2
    else:
        assert 0.2 < float(g[..., :2 * H].mean()) < 0.8 and float(((sig == 0) | (sig == 1)).float().mean()) == 0
    assert bool((back["d_pre"].reshape(Rr, S, D, 4, H)[:, 0, 0, 1] == 0).all()), "the forget-gate gradient of a first step is exactly 0"


@pytest.mark.parametrize("name", LSTM_IDS)
def test_honest_fp32_lstm_stays_under_every_bar(name):
    o = _lstm_operands(name)
    stored, _ = _lstm_stored(name)
    fwd = lstm_fwd_judge(o["pre"], o["w"], lstm_forward(o["pre"], o["w"], F32))
    bwd = lstm_bwd_judge(o["cot"], stored["gates"], stored["cells"], o["w"], lstm_backward(o["cot"], stored["gates"], stored["cells"], o["w"], F32))
    print(name, {k: round(v, 3) for k, v in {**fwd, **bwd}.items()})
    assert max(fwd.values()) <= 1.0 and max(bwd.values()) <= 1.0, (fwd, bwd)


def test_lstm_formulas_match_autograd():
    for name in ("fwd_chunk_plus_1", "s1_two_directions", "h33_transpose_edge"):
        o = _lstm_operands(name)
        Rr, S, D, H = _lstm_row(name)["shape"]
        p = o["pre"].double().requires_grad_(True)
        out, cells, gates = R.lstm(p, o["w"].double())
        out.backward(o["cot"].double().reshape(Rr, S, D * H))
        mine = lstm_forward(o["pre"], o["w"])
        assert _close(mine["h"].reshape(Rr, S, D * H), out) and _close(mine["cells"], cells) and _close(mine["gates"], gates)
        back = lstm_backward(o["cot"], mine["gates"], mine["cells"], o["w"])
        assert _close(back["d_pre"], p.grad), name
        hp = torch.zeros_like(mine["h"])
        hp[:, 1:, 0] = mine["h"][:, :-1, 0]
        if D == 2:
            hp[:, :-1, 1] = mine["h"][:, 1:, 1]
        assert torch.equal(back["h_prev"], hp)


def _lstm_launchers(lib, L, ops, name, o):
    Rr, S, D, H = _lstm_row(name)["shape"]
    rows = Rr * S * D
    PRE, W, GO = _Buf((rows,), 4 * H, content=o["pre"]), _Buf((D * 4 * H,), H, content=o["w"]), _Buf((rows,), H, content=o["cot"])
    nws = ops.lstm_workspace_floats(Rr, D, H)
    assert nws == int(lib.din_lstm_bwd_workspace(Rr, D, H)) == D * 4 * H * H + Rr * D * H

    def forward():
        HO, GA, CE = _Buf((rows,), H), _Buf((rows,), 4 * H), _Buf((rows,), H)
        L.check(lib.din_lstm_fwd(PRE.ptr(), W.ptr(), Rr, S, D, H, HO.ptr(), GA.ptr(), CE.ptr(), None))
        torch.cuda.synchronize()
        _intact(name, dict(HO=HO, GA=GA, CE=CE), dict(PRE=PRE, W=W))
        return HO, GA, CE

    def backward(GA, CE):
        DP, HP, WS = _Buf((rows,), 4 * H), _Buf((rows,), H), _Buf((1,), nws)
        saved = [t.bits() for t in (GA, CE)]
        L.check(lib.din_lstm_bwd(GO.ptr(), GA.ptr(), CE.ptr(), W.ptr(), Rr, S, D, H, DP.ptr(), HP.ptr(), WS.ptr(), nws, None))
        torch.cuda.synchronize()
        _intact(name, dict(DP=DP, HP=HP, WS=WS), dict(GO=GO, W=W))
        assert all(torch.equal(t.bits(), s) for t, s in zip((GA, CE), saved)), f"{name}: the backward wrote into gates or cells"
        return DP, HP, WS

    return forward, backward


@pytest.mark.gpu
@pytest.mark.parametrize("name", LSTM_IDS)
def test_lstm_kernels_against_fp64(env, name):
    lib, L, nhwc, ops = env
    o = _lstm_operands(name)
    Rr, S, D, H = _lstm_row(name)["shape"]
    rows = Rr * S * D
    stored, _ = _lstm_stored(name)
    forward, backward = _lstm_launchers(lib, L, ops, name, o)

    HO, GA, CE = forward()
    got = dict(h=HO.get().view(Rr, S, D, H), cells=CE.get().view(Rr, S, D, H), gates=GA.get().view(Rr, S, D, 4 * H))
    for k, v in lstm_fwd_judge(o["pre"], o["w"], got).items():
        _check("lstm-" + name, k, torch.tensor(v), torch.tensor(0.0), torch.tensor(1.0))
    again = forward()
    assert all(torch.equal(u.bits(), v.bits()) for u, v in zip((HO, GA, CE), again)), f"{name}: forward rerun differs"

    SG, SC = _Buf((rows,), 4 * H, content=stored["gates"]), _Buf((rows,), H, content=stored["cells"])
    DP, HP, WS = backward(SG, SC)
    ws = WS.get().flatten()
    nwt = D * 4 * H * H
    assert torch.equal(_bits32(ws[:nwt]).view(D, H, 4 * H), _bits32(o["w"].transpose(1, 2))), f"{name}: the workspace does not hold W_hh^T"
    got = dict(d_pre=DP.get().view(Rr, S, D, 4 * H), h_prev=HP.get().view(Rr, S, D, H), dc=ws[nwt:].view(Rr, D, H))
    for k, v in lstm_bwd_judge(o["cot"], stored["gates"], stored["cells"], o["w"], got).items():
        _check("lstm-" + name, k, torch.tensor(v), torch.tensor(0.0), torch.tensor(1.0))
    again = backward(SG, SC)
    assert all(torch.equal(u.bits(), v.bits()) for u, v in zip((DP, HP, WS), again)), f"{name}: backward rerun differs"

    # the kernel's own forward: h_prev is the shifted h bit for bit (the same two operands, the same product), 0 at each first step
    own = backward(GA, CE)
    assert all(bool(torch.isfinite(t.get()).all()) for t in own), f"{name}: the backward of the kernel's own forward is not finite"
    h = _bits32(HO.get()).view(Rr, S, D, H)
    want = torch.zeros_like(h)
    want[:, 1:, 0] = h[:, :-1, 0]
    if D == 2:
        want[:, :-1, 1] = h[:, 1:, 1]
    assert torch.equal(_bits32(own[1].get()).view(Rr, S, D, H), want), f"{name}: h_prev is not the shifted h"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["dw_h20", "h130_scalar"])
def test_lstm_dw_hh_against_fp64(env, name):
    """dW_hh = d_pre^T h_prev per direction: in place through strides (H % 4 == 0, cioff != 0 for the second direction) or from the padded
    copies; the rule is the one tests/test_gpu_wgrad.py applies to its fp32 rows"""
    from tests.test_gpu_wgrad import BAR, rel
    lib, L, nhwc, ops = env
    o = _lstm_operands(name)
    Rr, S, D, H = _lstm_row(name)["shape"]
    assert D == 2 and (H % 4 == 0) == (name == "dw_h20")
    _, back = _lstm_stored(name)
    hp, dp = back["h_prev"].float(), back["d_pre"].float()
    want = torch.einsum("rsdm,rsdk->dmk", dp.double(), hp.double())
    desc = ops._desc(1, 1, Rr * S, H, 4 * H, 1, 1, 0, 0, 1, D * H if H % 4 == 0 else _ceil(H, 4) * 4, D * 4 * H)
    desc.cioff, desc.cooff = (H if H % 4 == 0 else 0), 4 * H
    names = C.create_string_buffer(512)
    assert 0 < lib.din_conv_kernel_names(C.byref(desc), 2, 0, 0, 0, names, len(names)) <= len(names), lib.din_last_error_string()
    print(f"{name}: dW_hh runs on {names.value.decode().splitlines()[0]}")
    dw = ops._lstm_dw_hh(lib, hp.cuda(), dp.cuda(), o["w"].cuda())
    torch.cuda.synchronize()
    assert tuple(dw.shape) == (D, 4 * H, H)
    for d in range(D):
        assert rel(dw[d], want[d]) <= BAR["fp32"], (name, d)


# =====================================================================================================================================
# 2. pooling and attention (csrc/pctdm_attention.hip)
# =====================================================================================================================================
def _p(name, shape, kind="plain"):
    return dict(name=name, shape=shape, kind=kind)


PA_ROWS = [
    _p("smallest", (1, 4, 4)),
    _p("teams_of_one", (3, 2, 5)),
    _p("odd_team", (3, 6, 100)),
    _p("n32_h70", (2, 32, 70)),                                   # PC_MAX_N, eight players per wave, a second lane stride of 6 lanes
    _p("h1", (2, 4, 1)),
    _p("h64", (2, 4, 64)),
    _p("h65", (2, 4, 65)),
    _p("h257_five_frames", (5, 4, 257)),                          # second thread stride, the reduce kernel's second workgroup
    _p("peaked", (2, 8, 64), "peaked"),
    _p("saturated", (2, 4, 96), "saturated"),
    _p("ties", (2, 6, 33), "ties"),
    _p("launcher", (20, 12, 1000)),
]
PA_IDS = [r["name"] for r in PA_ROWS]
PA_FWD = ("context", "d_lstm_out", "gamma", "y")
PA_BWD = ("d_pooled", "d_src", "d_ctx", "d_w_e", "d_b_e")
PA_EXACT = ("pooled_bits", "winner")
PA_WRONG = ("fast_tanh", "ties_to_second", "context_n_minus_1", "softmax_all", "softmax_bwd_no_sum", "dctx_missing_last", "dbe_one_team")


def _pa_row(name):
    return PA_ROWS[PA_IDS.index(name)]


def _scores(src, ctx, w_e, b_e):
    return torch.tanh(src.double() + ctx.double()[:, None]) @ w_e.double() + b_e.double()


@functools.lru_cache(maxsize=None)
def _pa_operands(name):
    row = _pa_row(name)
    G, N, H = row["shape"]
    gen = _gen("pctdm_pa_" + name)
    lstm_out = torch.tanh(torch.randn(G, N, 2 * H, generator=gen))
    src, ctx = torch.randn(G, N, H, generator=gen), torch.randn(G, H, generator=gen)
    w_e, b_e = 2.0 * torch.randn(H, generator=gen) / H ** 0.5, torch.tensor([0.3])
    if row["kind"] == "ties":                                     # a third of the elements tie, signed zeros of both orders among them
        tie = torch.arange(G * N * H).view(G, N, H) % 3 == 0
        a = lstm_out[..., :H]
        a[tie & (torch.arange(H) % 5 == 1)] = 0.0
        a[tie & (torch.arange(H) % 5 == 3)] = -0.0
        b = torch.where(tie, a, lstm_out[..., H:])
        b[tie & (torch.arange(H) % 5 == 1)] = -0.0
        b[tie & (torch.arange(H) % 5 == 3)] = 0.0
        lstm_out = torch.cat([a, b], -1)
    if row["kind"] == "saturated":                                # |src + ctx| about 12 in half of the elements
        big = torch.rand(G, N, H, generator=gen) < 0.5
        sign = torch.where(torch.rand(G, N, H, generator=gen) < 0.5, -1.0, 1.0)
        ctx = 0.05 * ctx
        src = torch.where(big, sign * 12.0 + 0.1 * src, src)
    if row["kind"] == "peaked":                                   # w_e scaled until a team's scores spread by 25 or more
        for _ in range(20):
            s = _scores(src, ctx, w_e, b_e).view(G, 2, N // 2)
            if float((s.max(-1).values - s.min(-1).values).max()) >= 25:
                break
            w_e = w_e * 1.5
    cot, cot_c, gp = torch.randn(G, N, H, generator=gen), torch.randn(G, H, generator=gen), torch.randn(G, N, H, generator=gen)
    return dict(lstm_out=lstm_out, src=src, ctx=ctx, w_e=w_e, b_e=b_e, cot=cot, cot_c=cot_c, gp=gp)


def _team(t, G, N):
    return t.reshape(G, 2, N // 2)


def pa_chain(o, dtype=F64, wrong=None, saved=None):
    """pool_fwd, pool_bwd (of the cotangents gp, cot_c), att_fwd and att_bwd (of cot, reading the stored gamma `saved`, or this forward's
    own rounded to fp32) in `dtype`"""
    lo, src, ctx, we, be, cot, cot_c, gp = (o[k].to(dtype) for k in ("lstm_out", "src", "ctx", "w_e", "b_e", "cot", "cot_c", "gp"))
    G, N, H2 = lo.shape
    H = H2 // 2
    fast = wrong == "fast_tanh"
    a, b = lo[..., :H], lo[..., H:]
    second = (b >= a) if wrong == "ties_to_second" else (b > a)
    pooled = torch.where(second, b, a)
    acc = torch.zeros_like(pooled[:, 0])
    for i in range(N):                                            # players in order
        acc = acc + pooled[:, i]
    context = acc / ((N - 1) if wrong == "context_n_minus_1" else N)
    v = gp + (cot_c / N)[:, None]
    zero = torch.zeros_like(v)
    res = dict(pooled=pooled, pooled_bits=_bits32(pooled.float()), winner=second.to(torch.uint8), context=context,
               d_lstm_out=torch.cat([torch.where(second, zero, v), torch.where(second, v, zero)], -1))
    arg = src + ctx[:, None]
    t = _tanh(arg, fast)
    score = (t * we).sum(-1) + be
    gamma = torch.softmax(score, -1) if wrong == "softmax_all" else torch.softmax(_team(score, G, N), -1).reshape(G, N)
    res.update(arg=arg, t=t, score=score, gamma=gamma, y=pooled + pooled * gamma[..., None])
    ga = (gamma.float() if saved is None else saved).to(dtype)
    dg = (cot * pooled).sum(-1)
    gt, dt = _team(ga, G, N), _team(dg, G, N)
    tsum = 0 if wrong == "softmax_bwd_no_sum" else (dt * gt).sum(-1, keepdim=True)
    ds = (gt * (dt - tsum)).reshape(G, N)
    d_src = ds[..., None] * we * (1 - t * t)
    res.update(dg=dg, ds=ds, d_src=d_src, d_ctx=(d_src[:, :-1] if wrong == "dctx_missing_last" else d_src).sum(1),
               d_w_e=(ds[..., None] * t).sum((0, 1)), d_b_e=(_team(ds, G, N)[:, 0] if wrong == "dbe_one_team" else ds).sum().reshape(1),
               d_pooled=cot + cot * ga[..., None], saved=ga)
    return res


@functools.lru_cache(maxsize=None)
def _pa_expected(name):
    """the float64 chain with bars[...] as counted in the module docstring"""
    o = _pa_operands(name)
    w = pa_chain(o)
    G, N, H = _pa_row(name)["shape"]
    m, nd = N // 2, _ceil(H, 64) + 7
    saved = w["gamma"].float()
    w32 = pa_chain(o, F32, saved=saved)
    we, be, cot, cot_c, gp = (o[k].double() for k in ("w_e", "b_e", "cot", "cot_c", "gp"))
    p, t, ga = w["pooled"], w["t"], saved.double()
    second = w["winner"].bool()
    bars = {}
    bars["context"] = (N + 2) * U32 * p.abs().sum(1) / N + TINY
    bv = 3 * U32 * (gp.abs() + (cot_c.abs() / N)[:, None])
    zero = torch.zeros_like(bv)
    bars["d_lstm_out"] = torch.cat([torch.where(second, zero, bv), torch.where(second, bv, zero)], -1)
    s2 = 1 - t * t
    bt = s2 * U32 * w["arg"].abs() + 2 * U32 * t.abs()
    bs = (nd + 1) * U32 * ((t * we).abs().sum(-1) + be.abs()) + (bt * we.abs()).sum(-1)
    st, gt = _team(w["score"], G, N), _team(w["gamma"], G, N)
    eps = _team(bs, G, N) + U32 * ((st - st.max(-1, keepdim=True).values).abs() + 2)
    bars["gamma"] = (gt * (eps + (gt * eps).sum(-1, keepdim=True) + (m + 2) * U32) + TINY).reshape(G, N)
    bars["y"] = p.abs() * bars["gamma"][..., None] + 3 * U32 * (p.abs() + (p * w["gamma"][..., None]).abs())
    # backward, from the stored gamma
    bdg = _team(nd * U32 * (cot * p).abs().sum(-1), G, N)
    gs, dgt = _team(ga, G, N), _team(w["dg"], G, N).abs()
    floor = gs * (bdg + (gs * bdg).sum(-1, keepdim=True) + (m + 6) * U32 * (dgt + (gs * dgt).sum(-1, keepdim=True)))
    yard = _team((w32["ds"].double() - w["ds"]).abs(), G, N).amax(-1, keepdim=True)
    bds = torch.maximum(4 * yard, floor).reshape(G, N)
    ds = w["ds"]
    bars["ds"] = bds
    bars["d_src"] = (bds[..., None] * (we * s2).abs() + (ds[..., None] * we).abs() * (2 * t.abs() * bt + 2 * U32) + 3 * U32 * w["d_src"].abs())
    bars["d_ctx"] = (N + 1) * U32 * w["d_src"].abs().sum(1) + bars["d_src"].sum(1)
    bars["d_w_e"] = (N + G + 2) * U32 * (ds[..., None] * t).abs().sum((0, 1)) + (bds[..., None] * t.abs() + ds.abs()[..., None] * bt).sum((0, 1))
    bars["d_b_e"] = ((N + G + 1) * U32 * ds.abs().sum() + bds.sum()).reshape(1)
    bars["d_pooled"] = 3 * U32 * (cot.abs() + (cot * ga[..., None]).abs())
    w["bars"] = bars
    return w


def _pa_ratios(bad, want, keys=PA_FWD + PA_BWD):
    out = {}
    for k in keys:
        r = _ratio(bad[k], want[k], want["bars"][k])
        out[k] = INF if math.isnan(r) else r
    for k in PA_EXACT:
        out[k] = 0.0 if torch.equal(bad[k], want[k]) else INF
    return out


def _pa_applies(row, wrong):
    G, N, H = row["shape"]
    return {"ties_to_second": row["kind"] == "ties", "dctx_missing_last": N > 2 and row["kind"] != "peaked", "dbe_one_team": False,
            "fast_tanh": False}.get(wrong, True)


def _bite_pa(name):
    row, o, want = _pa_row(name), _pa_operands(name), _pa_expected(name)
    assert all(bool(torch.isfinite(want[k]).all()) for k in PA_FWD + PA_BWD)
    for wrong in PA_WRONG:
        if _pa_applies(row, wrong):
            bad = pa_chain(o, F64, wrong, saved=want["saved"].float())
            worst = max(_pa_ratios(bad, want).values())
            assert worst >= 10.0, f"{name}: the bars do not see '{wrong}' ({worst:.3g})"


@pytest.mark.parametrize("name", PA_IDS)
def test_pa_rows_meet_the_input_conditions(name):
    row, o, want = _pa_row(name), _pa_operands(name), _pa_expected(name)
    G, N, H = row["shape"]
    gamma, lo = want["gamma"], o["lstm_out"]
    a, b = lo[..., :H], lo[..., H:]
    tie = a == b
    st = _team(want["score"], G, N)
    if row["kind"] == "ties":
        share = float(tie.float().mean())
        assert 0.3 <= share <= 0.4, share
        sa, sb = torch.signbit(a), torch.signbit(b)
        assert bool((tie & ~sa & sb).any()) and bool((tie & sa & ~sb).any())               # (+0, -0) and (-0, +0)
        assert not bool(want["winner"].bool()[tie].any())
        assert torch.equal(want["pooled_bits"][tie], _bits32(a)[tie])
        assert bool((want["d_lstm_out"][..., H:][tie] == 0).all()) and bool((want["d_lstm_out"][..., :H][tie] != 0).all())
    else:
        assert not bool(tie.any())
    if row["kind"] == "peaked":
        assert float((st.max(-1).values - st.min(-1).values).max()) >= 25
        assert bool((gamma < 1e-9).any()) and float(gamma.min()) > 1e-30
    elif N > 2:
        assert 1.2 / (N // 2) < float(_team(gamma, G, N).max(-1).values.mean()) < 0.95, "the team softmax of this row is uniform or one-hot"
    if row["kind"] == "saturated":
        sat = want["arg"].abs() > 10
        assert 0.3 < float(sat.float().mean()) < 0.7
        assert bool((torch.tanh(want["arg"].float())[sat].abs() == 1).all())               # t = +-1 exactly in fp32
    if name == "teams_of_one":
        assert N == 2 and bool((gamma == 1).all()) and bool((want["ds"] == 0).all())
        assert torch.equal(want["y"], 2 * want["pooled"]) and torch.equal(want["d_pooled"], 2 * o["cot"].double())
        assert all(bool((want[k] == 0).all()) for k in ("d_src", "d_ctx", "d_w_e", "d_b_e"))
    want_shape = {"n32_h70": N == 32 and _ceil(N, 4) == 8 and H - 64 == 6, "h1": H == 1, "h64": H == 64, "h65": H == 65,
                  "h257_five_frames": H == 257 and G == 5 and _ceil(H, 256) == 2, "odd_team": (N // 2) % 2 == 1,
                  "launcher": (G, N, H) == (20, 12, 1000)}.get(name, True)
    assert want_shape, name


@pytest.mark.parametrize("name", PA_IDS)
def test_honest_fp32_pool_and_attention_stay_under_every_bar(name):
    o, want = _pa_operands(name), _pa_expected(name)
    r = _pa_ratios(pa_chain(o, F32, saved=want["saved"].float()), want)
    print(name, {k: round(v, 3) for k, v in r.items()})
    assert max(r.values()) <= 1.0, r


def test_pa_formulas_match_autograd():
    for name in ("odd_team", "smallest", "h65"):
        o = _pa_operands(name)
        ts = [o[k].double().requires_grad_(True) for k in ("lstm_out", "src", "ctx", "w_e", "b_e")]
        pooled, winner, context = R.pool(ts[0])
        pooled.retain_grad()
        y, gamma = R.attention(pooled, ts[1], ts[2], ts[3], ts[4][0])
        mine = pa_chain(o, saved=gamma.detach())
        assert _close(mine["y"], y) and _close(mine["gamma"], gamma) and _close(mine["context"], context)
        assert torch.equal(mine["winner"].bool(), winner)
        (y * o["cot"].double()).sum().backward(retain_graph=True)
        for k, g in (("d_pooled", pooled.grad), ("d_src", ts[1].grad), ("d_ctx", ts[2].grad), ("d_w_e", ts[3].grad)):
            assert _close(mine[k], g), (name, k)
        assert float(mine["d_b_e"].abs()) <= 1e-12 * float(mine["d_w_e"].abs().max()) and float(ts[4].grad.abs()) <= 1e-12
        lo = o["lstm_out"].double().requires_grad_(True)
        pooled, _, context = R.pool(lo)
        ((pooled * o["gp"].double()).sum() + (context * o["cot_c"].double()).sum()).backward()
        assert _close(mine["d_lstm_out"], lo.grad), name


@pytest.mark.gpu
@pytest.mark.parametrize("name", PA_IDS)
def test_pool_and_attention_kernels_against_fp64(env, name):
    lib, L, nhwc, ops = env
    row, o, want = _pa_row(name), _pa_operands(name), _pa_expected(name)
    G, N, H = row["shape"]
    bars = want["bars"]
    LO, SRC, CTX = _Buf((G * N,), 2 * H, content=o["lstm_out"]), _Buf((G * N,), H, content=o["src"]), _Buf((G,), H, content=o["ctx"])
    WE, BE = _Buf((1,), H, content=o["w_e"]), _Buf((1,), 1, content=o["b_e"])
    GY, GC, GP = _Buf((G * N,), H, content=o["cot"]), _Buf((G,), H, content=o["cot_c"]), _Buf((G * N,), H, content=o["gp"])
    nws = ops.pctdm_att_workspace_floats(G, H)
    assert nws == int(lib.din_pctdm_att_bwd_workspace(G, H)) == G * H + G

    def pool():
        PO, WI, CO, DL = _Buf((G * N,), H), _Bytes(G * N * H), _Buf((G,), H), _Buf((G * N,), 2 * H)
        L.check(lib.din_pctdm_pool_fwd(LO.ptr(), G, N, H, PO.ptr(), WI.ptr(), CO.ptr(), None))
        torch.cuda.synchronize()
        kept = WI.bits()
        L.check(lib.din_pctdm_pool_bwd(GP.ptr(), GC.ptr(), WI.ptr(), G, N, H, DL.ptr(), None))
        torch.cuda.synchronize()
        _intact(name, dict(PO=PO, WI=WI, CO=CO, DL=DL), dict(LO=LO, GP=GP, GC=GC))
        assert torch.equal(WI.bits(), kept), f"{name}: pool_bwd wrote into winner"
        return PO, WI, CO, DL

    PO, WI, CO, DL = pool()
    assert torch.equal(WI.get().view(G, N, H), want["winner"]), f"{name}: a winner differs"
    assert torch.equal(_bits32(PO.get()).view(G, N, H), want["pooled_bits"]), f"{name}: pooled does not carry the winner's bits"
    _check("pa-" + name, "context", CO.get().view(G, H), want["context"], bars["context"])
    _check("pa-" + name, "d_lstm_out", DL.get().view(G, N, 2 * H), want["d_lstm_out"], bars["d_lstm_out"])
    again = pool()
    assert all(torch.equal(u.bits(), v.bits()) for u, v in zip((PO, WI, CO, DL), again)), f"{name}: pool rerun differs"

    def att_fwd():
        Y, GA = _Buf((G * N,), H), _Buf((G,), N)
        L.check(lib.din_pctdm_att_fwd(PO.ptr(), SRC.ptr(), CTX.ptr(), WE.ptr(), BE.ptr(), G, N, H, Y.ptr(), GA.ptr(), None))
        torch.cuda.synchronize()
        _intact(name, dict(Y=Y, GA=GA), dict(SRC=SRC, CTX=CTX, WE=WE, BE=BE))
        return Y, GA

    def att_bwd(GA):
        DPO, DS, DC, DW, DB, WS = _Buf((G * N,), H), _Buf((G * N,), H), _Buf((G,), H), _Buf((1,), H), _Buf((1,), 1), _Buf((1,), nws)
        kept = GA.bits()
        L.check(lib.din_pctdm_att_bwd(GY.ptr(), PO.ptr(), SRC.ptr(), CTX.ptr(), WE.ptr(), GA.ptr(), G, N, H, DPO.ptr(), DS.ptr(), DC.ptr(),
                                      DW.ptr(), DB.ptr(), WS.ptr(), nws, None))
        torch.cuda.synchronize()
        _intact(name, dict(DPO=DPO, DS=DS, DC=DC, DW=DW, DB=DB, WS=WS), dict(GY=GY, SRC=SRC, CTX=CTX, WE=WE))
        assert torch.equal(GA.bits(), kept), f"{name}: att_bwd wrote into gamma"
        return DPO, DS, DC, DW, DB, WS

    pooled_before = PO.bits()
    Y, GA = att_fwd()
    gamma = GA.get().view(G, N)
    _check("pa-" + name, "gamma", gamma, want["gamma"], bars["gamma"])
    _check("pa-" + name, "y", Y.get().view(G, N, H), want["y"], bars["y"])
    again = att_fwd()
    assert all(torch.equal(u.bits(), v.bits()) for u, v in zip((Y, GA), again)), f"{name}: att_fwd rerun differs"

    SG = _Buf((G,), N, content=want["saved"])
    outs = att_bwd(SG)
    got = dict(zip(("d_pooled", "d_src", "d_ctx", "d_w_e", "d_b_e"), (t.get() for t in outs[:5])))
    for k in PA_BWD:
        _check("pa-" + name, k, got[k].view(want[k].shape), want[k], bars[k])
    again = att_bwd(SG)
    assert all(torch.equal(u.bits(), v.bits()) for u, v in zip(outs, again)), f"{name}: att_bwd rerun differs"
    own = att_bwd(GA)                                             # the kernel's own gamma is accepted (not rejudged)
    assert all(bool(torch.isfinite(t.get()).all()) for t in own[:5]), f"{name}: the backward of the kernel's own forward is not finite"
    assert torch.equal(PO.bits(), pooled_before), f"{name}: the attention kernels wrote into pooled"

    if row["kind"] == "peaked":                                   # the tiny entries stand inside their relative bar (judged above), and exist
        assert bool((gamma < 1e-9).any()) and bool((gamma > 0).all())
    if row["kind"] == "saturated":
        sat = want["arg"].abs() > 10
        assert bool((got["d_src"].view(G, N, H)[sat] == 0).all()), f"{name}: d_src is not exactly 0 where tanh saturates"
    if name == "teams_of_one":
        p, gy = PO.get().view(G, N, H), o["cot"]
        assert bool((gamma == 1).all()) and torch.equal(Y.get().view(G, N, H), 2 * p) and torch.equal(got["d_pooled"].view(G, N, H), 2 * gy)
        assert all(bool((got[k] == 0).all()) for k in ("d_src", "d_ctx", "d_w_e", "d_b_e"))


# =====================================================================================================================================
# the bars bite: every row (CPU)
# =====================================================================================================================================
BITE = [(_bite_lstm, n, "lstm-" + n) for n in LSTM_IDS] + [(_bite_pa, n, "pa-" + n) for n in PA_IDS]


@pytest.mark.parametrize("check,arg", [b[:2] for b in BITE], ids=[b[2] for b in BITE])
def test_bars_bite(check, arg):
    """every applicable wrong variant of the row's reference misses one of the row's bars by >= 10x on the row's own inputs"""
    check(arg)
