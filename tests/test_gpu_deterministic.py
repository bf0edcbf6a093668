"""Deterministic mode on the GPU (DIN_DETERMINISTIC through ops.deterministic): every entry point the mode covers -- din_walk_bwd,
din_layernorm_bwd, din_head_bwd, din_dot_accum, din_colsum, the bias gradient of GridConvFunction / ops.linear -- runs under the option
against the SAME float64 references and the SAME bars as tests/test_gpu_head_path.py, test_gpu_roi_bn.py and test_gpu_wgrad.py hold the
atomic forms to (no new tolerance), five times into fresh guarded buffers, and every result must repeat bit for bit; the walk also across
DIN_WALK_BWD_GROUPS / DIN_WALK_BWD_GLOBAL.  Then the models: two passes from the same weights give bit-identical gradients, two builds
trained three FusedAdam steps give bit-identical weights, and the ordered launches replay from a captured graph with the same bits.

Walk collision rows (T = 3, N = 4, C = 65: two channel chunks, one of a single channel; 3 x 3, ratio 1; gz = +-2^e, e in -10 .. 10):
  zero      every offset 0: each tap sits on its lattice point, nine taps of neighbouring positions meet in every cell;
  corner    every offset -40: every corner of every tap clamps into padded cell (0, 0) -- 12 * 9 * 4 contributions to one cell.  That cell
            is zero padding (the padded grid starts one cell outside the actors), so its gradient is dropped: dx is exactly 0;
  cells     every tap sampled at padded (1.25, 1.75): the 12 * 9 * 4 contributions land in the four REAL cells (0..1, 0..1), 108 each with
            four different weights -- the collision `corner` describes, where it reaches dx.
test_collision_rows_stay_inside_the_bars_in_any_order (CPU) sums those rows' fp32 terms forwards, backwards and shuffled: the results
differ in their last bits and all stay inside the bars, so the bars alone cannot tell an ordered sum from an atomic one -- bit identity is
what is under test."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.conftest import Measured
from tests.test_gpu_kernels import env  # noqa: F401  (the module-scoped library fixture)
from tests.test_gpu_head_path import (BF, FP, HEAD_CASES, HEAD_IDS, LN_SEED, U32, WALK_IDS, WALK_ROWS, _all_outside, _all_unchanged, _Buf, _check, _gen,
                                      _head_operands, _keep_mask, _ln_expected, _ln_launch, _ln_operands, _refused, _w, _walk_bars, _walk_expected,
                                      _walk_geom, _walk_operands, _walk_positions, head_reference, walk_reference)

OPTION = "DIN_DETERMINISTIC"
ORDERED = "din_walk_bwd_dx_ordered_kernel"
CALLS = 5
WALK_SETTINGS = [(None, None), (None, "1"), (None, "3"), ("0", None), ("0", "3")]       # (DIN_WALK_BWD_GLOBAL, DIN_WALK_BWD_GROUPS)


@pytest.fixture
def det(env):  # noqa: F811
    from din_amd import ops
    with ops.deterministic():
        yield env


def _same_bits(bufs, what):
    first = bufs[0].bits()
    for i, b in enumerate(bufs[1:], 1):
        assert torch.equal(b.bits(), first), f"{what}: call {i} differs from call 0"


# =====================================================================================================================================
# 1. walk
# =====================================================================================================================================
COLL = (2, 3, 4, 65, 3, 3, 1)
EXTRA_ROWS = [_w("coll_zero", COLL), _w("coll_corner", COLL), _w("coll_cells", COLL), _w("k77_t10n12", (1, 10, 12, 64, 7, 7, 1)),
              _w("npc_c65", (3, 3, 5, 65, 3, 3, 1), npc=(5, 1, 3)), _w("plain_c65", COLL, plain=1)]
EXTRA_IDS = [r["name"] for r in EXTRA_ROWS]


@functools.lru_cache(maxsize=None)
def _extra_operands(name):
    row = EXTRA_ROWS[EXTRA_IDS.index(name)]
    g = _walk_geom(row)
    b, t, n, c, k2 = g["b"], g["t"], g["n"], g["c"], g["k2"]
    gen = _gen("det_walk_" + name)
    x = torch.randn(b, t, n, c, generator=gen)
    logits = torch.rand(b, t, n, k2, generator=gen) * 4 - 2
    sign = torch.randint(0, 2, (b, t, n, c), generator=gen) * 2.0 - 1.0
    gz = sign * torch.pow(2.0, torch.randint(-10, 11, (b, t, n, c), generator=gen).float())
    if name == "coll_zero":
        off = torch.zeros(b, t, n, 2 * k2)
    elif name == "coll_corner":
        off = torch.full((b, t, n, 2 * k2), -40.0)
    elif name == "coll_cells":
        from tests.test_gpu_head_path import _walk_base
        by, bx = _walk_base(t, n, g["kh"], g["kw"], g["ratio"])
        off = torch.cat([torch.from_numpy(g["pt"] + 0.25 - by)[None, :, None, :].expand(b, t, n, k2),
                         torch.from_numpy(g["pl"] + 0.75 - bx)[None, None, :, :].expand(b, t, n, k2)], dim=3).float()
    else:
        off = torch.rand(b, t, n, 2 * k2, generator=gen) * 3 - 1.5
    return dict(x=x, pred=torch.cat([off, logits], dim=3).contiguous(), gz=gz)


@functools.lru_cache(maxsize=None)
def _extra_expected(name):
    row = EXTRA_ROWS[EXTRA_IDS.index(name)]
    o, g = _extra_operands(name), _walk_geom(row)
    py0, px0 = _walk_positions_of(o["pred"], row)
    return walk_reference(o["x"], py0, px0, o["pred"][..., 2 * g["k2"]:], row["shape"], 1, row["plain"], None, row["npc"], o["gz"])


def _walk_positions_of(pred, row):
    """_walk_positions for operands that are not a row of WALK_ROWS: the same one fp32 add"""
    from tests.test_gpu_head_path import _walk_base
    g = _walk_geom(row)
    by, bx = _walk_base(g["t"], g["n"], g["kh"], g["kw"], g["ratio"])
    off = pred[..., :2 * g["k2"]].numpy().astype(np.float32) * (0 if row["plain"] else 1)
    return by.astype(np.float32)[None, :, None, :] + off[..., :g["k2"]], bx.astype(np.float32)[None, None, :, :] + off[..., g["k2"]:]


def _walk_backward(env, row, o, want, monkeypatch):  # noqa: F811
    """din_walk_bwd of a row under the option: CALLS launches into fresh guarded buffers under the default launch shape, one more under each
    other setting of WALK_SETTINGS; every dx / dpred against the fp64 bars, all of them bit-identical; the reporter names the ordered kernel"""
    lib, L, nhwc, ops = env
    name = row["name"]
    g = _walk_geom(row)
    b, t, n, c, kh, kw, ratio, k2, cp, ncols, nch = (g[k] for k in ("b", "t", "n", "c", "kh", "kw", "ratio", "k2", "cp", "ncols", "nch"))
    bars, valid = _walk_bars(want, k2, nch, row["scale"]), want["valid"]
    X, P, GZ = _Buf((b, t, n), c, content=o["x"]), _Buf((b, t, n), ncols, content=o["pred"], ld=cp), _Buf((b, t, n), c, content=o["gz"])
    a_saved = torch.where(valid.unsqueeze(-1), want["a"], torch.full_like(want["a"], 1.0 / k2)).float()
    AS = _Buf((b, t, n), k2, content=a_saved)
    cl = (C.c_int32 * 4)(*g["clamp"]) if g["clamp"] else None
    npc = torch.tensor(row["npc"], dtype=torch.int32).cuda() if row["npc"] else None
    buf = C.create_string_buffer(96)
    dxs, dps = [], []
    for glob, groups in [WALK_SETTINGS[0]] * CALLS + WALK_SETTINGS[1:]:
        for opt, val in (("DIN_WALK_BWD_GLOBAL", glob), ("DIN_WALK_BWD_GROUPS", groups)):
            if val is not None:
                monkeypatch.setenv(opt, val)
            else:
                L.set_option(opt, None)
        L.check(lib.din_walk_bwd_kernel_name(b, t, n, c, kh, kw, ratio, buf, 96))
        assert buf.value.decode() == ORDERED
        DX, DP = _Buf((b, t, n), c), _Buf((b, t, n), ncols, ld=cp)
        scratch = torch.full((nch * b * t * n * 3 * k2,), float("nan")).cuda()
        L.check(lib.din_walk_bwd(X.ptr(), P.ptr(), cp, AS.ptr(), GZ.ptr(), b, t, n, c, kh, kw, ratio, row["scale"], row["plain"], cl,
                                 npc.data_ptr() if npc is not None else None, DX.ptr(), DP.ptr(), scratch.data_ptr(), None))
        torch.cuda.synchronize()
        tag = f"{name}[det,global={glob},groups={groups}]"
        assert _all_outside(DX, DP) and _all_unchanged(X, P, AS, GZ), f"{tag}: wrote outside a destination or into a source"
        dxs.append(DX)
        dps.append(DP)
        if len(dxs) in (1, CALLS + 1, len(WALK_SETTINGS) + CALLS - 1):     # (bit identity carries the bars to the launches in between)
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
    _same_bits(dxs, f"{name}: dx")
    _same_bits(dps, f"{name}: dpred")
    return dxs[0]


@pytest.mark.gpu
@pytest.mark.parametrize("name", WALK_IDS)
def test_walk_rows_under_the_option(det, name, monkeypatch):
    row = WALK_ROWS[WALK_IDS.index(name)]
    _walk_backward(det, row, _walk_operands(name), _walk_expected(name), monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("name", EXTRA_IDS)
def test_walk_collision_rows_repeat_bit_for_bit(det, name, monkeypatch):
    row = EXTRA_ROWS[EXTRA_IDS.index(name)]
    want = _extra_expected(name)
    dx = _walk_backward(det, row, _extra_operands(name), want, monkeypatch)
    if name == "coll_corner":
        assert not bool(dx.get().any()) and not bool(want["dx"].any())      # the one cell every corner meets in is zero padding
    if name == "coll_cells":
        cnt = want["dx_cnt"][..., 0]
        assert cnt[:, :2, :2].eq(108).all() and int(cnt.sum()) == 2 * 432


def _fp32_terms(name):
    """the fp32 terms a_k (wy wx) gz of every real cell of a collision row, in (position, k, corner) order, computed as the kernels compute
    them (fp32 products), per clip: {cell: [terms [c]]}"""
    row = EXTRA_ROWS[EXTRA_IDS.index(name)]
    o, g, want = _extra_operands(name), _walk_geom(row), _extra_expected(name)
    b, t, n, k2, pt, pl, hp, wp = (g[k] for k in ("b", "t", "n", "k2", "pt", "pl", "hp", "wp"))
    py0, px0 = _walk_positions_of(o["pred"], row)
    a, gz = want["a"].float().numpy(), o["gz"].numpy()
    f32 = np.float32
    cells = {}
    for bi in range(b):
        for pos in range(t * n):
            tt, nn = divmod(pos, n)
            for k in range(k2):
                y0, x0 = py0[bi, tt, nn, k], px0[bi, tt, nn, k]
                fy, fx = np.floor(y0), np.floor(x0)
                ly, ry = int(min(max(fy, 0), hp - 1)), int(min(max(fy + 1, 0), hp - 1))
                lx, rx = int(min(max(fx, 0), wp - 1)), int(min(max(fx + 1, 0), wp - 1))
                py, px = f32(min(max(y0, 0), hp - 1)), f32(min(max(x0, 0), wp - 1))
                for cy, cx in ((ly, lx), (ry, rx), (ry, lx), (ly, rx)):
                    if 0 <= cy - pt < t and 0 <= cx - pl < n:
                        w = f32(a[bi, tt, nn, k]) * (f32(f32(1) - abs(py - f32(cy))) * f32(f32(1) - abs(px - f32(cx))))
                        cells.setdefault((bi, cy - pt, cx - pl), []).append(f32(w) * gz[bi, tt, nn])
    return cells, want


@pytest.mark.parametrize("name", ["coll_zero", "coll_cells"])
def test_collision_rows_stay_inside_the_bars_in_any_order(name):
    """CPU: the rows' fp32 terms summed forwards, backwards and shuffled all stay inside the fp64 bars, and the three sums differ in their
    last bits somewhere -- the order matters to the bits and not to the bars"""
    cells, want = _fp32_terms(name)
    g = _walk_geom(EXTRA_ROWS[EXTRA_IDS.index(name)])
    bar = _walk_bars(want, g["k2"], g["nch"], 1)["dx"]
    rs = np.random.RandomState(5)
    sums = [np.zeros(want["dx"].shape, dtype=np.float32) for _ in range(3)]
    for (bi, tt, nn), terms in cells.items():
        for out, order in zip(sums, (range(len(terms)), reversed(range(len(terms))), rs.permutation(len(terms)))):
            acc = np.zeros_like(terms[0])
            for i in order:
                acc = acc + terms[i]
            out[bi, tt, nn] = acc
    for s in sums:
        worst = float((torch.from_numpy(s).double() - want["dx"]).abs().div(bar.clamp_min(1e-300)).max())
        assert worst <= 1.0, worst
    assert not np.array_equal(sums[0], sums[1]) and not np.array_equal(sums[0], sums[2])
    # (zero offsets: a centre cell of the 3 x 4 grid is the lt corner of all nine taps that look at it, and a zero-weight corner of more)
    assert max(len(v) for v in cells.values()) >= (108 if name == "coll_cells" else 9)


# =====================================================================================================================================
# 2. LayerNorm, head, dot_accum, colsum
# =====================================================================================================================================
LN_DET_ROWS = [(8, 20, 0.0), (9, 20, 0.0), (72, 1024, 0.0), (5, 1030, 0.0)]       # (rows <= 8 | > 8: the atomic launcher's two branches)
LN_DET_MODES = [(0, 0, 0.0), (1, 1, 0.3)]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", LN_DET_MODES, ids=["plain", "res_relu_p0.3"])
@pytest.mark.parametrize("row", LN_DET_ROWS, ids=[f"{r[0]}x{r[1]}" for r in LN_DET_ROWS])
def test_layernorm_param_grads_under_the_option(det, row, mode):
    lib, L, nhwc, ops = det
    o, (res, relu, p), name = _ln_operands(*row), mode, f"ln{row}/{mode}[det]"
    rows, length = o["x"].shape
    keep = _keep_mask(lib, L, rows * length, p, LN_SEED).view(rows, length) if p else torch.ones(rows, length, dtype=torch.bool)
    want = _ln_expected(row, mode, keep)
    stats32 = torch.stack([want["mean"], want["rstd"]], dim=1).float()
    runs = [_ln_launch(lib, L, o, res, relu, p, LN_SEED, None, stats32, want["y"].float()) for _ in range(CALLS)]     # (guard bands: inside)
    Y, S, DX, DG, DB = runs[0]
    _check(name, "dx", DX.get(), want["dx"], want["bars"]["dx"])
    _check(name, "dgamma", DG.get()[0], want["dgamma"], want["bars"]["dgamma"])     # (onto the priors dg0 / db0: the += contract)
    _check(name, "dbeta", DB.get()[0], want["dbeta"], want["bars"]["dbeta"])
    for k, what in ((2, "dx"), (3, "dgamma"), (4, "dbeta")):
        _same_bits([r[k] for r in runs], f"{name}: {what}")


@pytest.mark.gpu
@pytest.mark.parametrize("shape,mode", HEAD_CASES, ids=HEAD_IDS)
def test_head_param_grads_under_the_option(det, shape, mode):
    lib, L, nhwc, ops = det
    b, t, n, c, a = shape
    o, want, name = _head_operands(shape), head_reference(shape, mode), f"head{shape}/{mode}[det]"
    S, W, DSC = (_Buf(lead, m, content=o[k]) for lead, m, k in (((b, t, n), c, "s"), ((a,), c, "w"), ((b,), a, "dsc")))
    AMS = _Buf((b, t), c, torch.int32, content=want["argmax"].int())
    runs = []
    for _ in range(CALLS):
        DS, DW, DB = _Buf((b, t, n), c), _Buf((a,), c, content=o["dw0"]), _Buf((1,), a, content=o["db0"])
        L.check(lib.din_head_bwd(DSC.ptr(), S.ptr(), W.ptr(), AMS.ptr(), b, t, n, c, a, DS.ptr(), DW.ptr(), DB.ptr(), None))
        torch.cuda.synchronize()
        assert _all_outside(DS, DW, DB) and _all_unchanged(DSC, S, W, AMS), f"{name}: wrote outside a destination or into a source"
        runs.append((DS, DW, DB))
    DS, DW, DB = runs[0]
    assert torch.equal(DS.get() != 0, want["ds"] != 0), f"{name}: the gradient's footprint is not the arg-max"
    _check(name, "ds", DS.get(), want["ds"], want["bars"]["ds"])
    _check(name, "dw", DW.get(), want["dw"], want["bars"]["dw"])
    _check(name, "dbias", DB.get()[0], want["db"], want["bars"]["db"])
    for k, what in enumerate(("ds", "dw", "dbias")):
        _same_bits([r[k] for r in runs], f"{name}: {what}")


@pytest.mark.gpu
@pytest.mark.parametrize("accumulate", [0, 1])
def test_scale_by_param_and_dot_accum_under_the_option(det, accumulate):
    """the operands and bars of test_scale_by_param_and_dot_accum_against_fp64; dot_accum onto a prior (accumulate = 1) and onto zero"""
    lib, L, nhwc, ops = det
    gen = _gen("scale_by_param")
    n = 1003
    x, prior, sc = torch.randn(n, generator=gen), torch.randn(n, generator=gen), torch.randn(4, generator=gen)
    X, SC = _Buf((1,), n, content=x), _Buf((1,), 4, content=sc)
    O_ = _Buf((1,), n, content=prior if accumulate else None)
    L.check(lib.din_scale_by_param(X.ptr(), SC.ptr(), 2, O_.ptr(), accumulate, n, None))
    torch.cuda.synchronize()
    assert O_.untouched_outside() and _all_unchanged(X, SC)
    want = x.double() * sc[2].double() + (prior.double() if accumulate else 0)
    _check("scale_by_param[det]", "out", O_.get()[0], want, 4 * U32 * ((x.double() * sc[2].double()).abs() + prior.double().abs() * accumulate))
    n = 300001
    x, y = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    before = 0.625 * accumulate
    X, Y = _Buf((1,), n, content=x), _Buf((1,), n, content=y)
    outs = []
    for _ in range(CALLS):
        D = _Buf((1,), 1, content=torch.tensor([before]), ld=5, off=3)
        L.check(lib.din_dot_accum(X.ptr(), Y.ptr(), D.ptr(), 3, n, None))
        torch.cuda.synchronize()
        assert D.untouched_outside() and _all_unchanged(X, Y), "dot_accum: a neighbour of out[idx] changed"
        outs.append(D)
    terms = (x.double() * y.double()).abs().sum() + before
    _check("dot_accum[det]", "out[idx]", outs[0].get()[0], before + (x.double() * y.double()).sum().view(1), 2060 * U32 * terms.view(1))
    _same_bits(outs, "dot_accum")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [FP, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("c", [3, 27, 1024])
@pytest.mark.parametrize("rows", [1, 63, 64, 4097])
def test_colsum_under_the_option(det, rows, c, dtype):
    """din_colsum on a view with a channel offset, against the bar test_gpu_roi_bn.py holds the atomic kernels to (its count n of the kernel
    that would serve the view without the option); the destination starts as NaN: the entry point overwrites it"""
    lib, L, nhwc, ops = det
    epc = 8 if dtype == BF else 4
    coff, ld = 8, c + 8 + (8 - c % 8) % 8 + 8
    g = torch.randn(rows, c, generator=_gen(f"det_colsum{rows}x{c}")).to(dtype)
    if c % epc == 0 and c // epc <= 256:
        rpb = max(-(-rows // 256), 64)
        n = -(-rpb // (256 // (c // epc))) + 256 // (c // epc) + -(-rows // rpb)
    else:
        n = 512 + -(-rows // 512)
    G = _Buf((rows,), c, dtype, content=g, ld=ld, off=coff)
    outs = []
    for _ in range(CALLS):
        OUT = _Buf((1,), c)
        L.check(lib.din_colsum(G.ptr(), L.DIN_BF16 if dtype == BF else L.DIN_F32, rows, c, ld, coff, OUT.ptr(), None))
        torch.cuda.synchronize()
        assert OUT.untouched_outside() and G.unchanged()
        outs.append(OUT)
    _check(f"colsum[det,{rows}x{c},{dtype}]", "column sums", outs[0].get()[0], g.double().sum(0), (n + 1) * U32 * g.double().abs().sum(0))
    _same_bits(outs, "colsum")


# =====================================================================================================================================
# 3. GridConvFunction / ops.linear backward
# =====================================================================================================================================
BAR_BIAS = 1e-5                            # tests/test_gpu_wgrad.py: a bias gradient, per channel, of sum |terms|


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fp32", "lowp", "split"])
@pytest.mark.parametrize("rows,cin,cout", [(96, 40, 24), (3840, 64, 1024)], ids=["96x40to24", "3840x64to1024"])
def test_linear_backward_repeats_bit_for_bit(det, rows, cin, cout, mode):
    lib, L, nhwc, ops = det
    gen = _gen(f"det_linear{rows}x{cin}x{cout}")
    x, w, bias, gy = (torch.randn(s, generator=gen) for s in ((rows, cin), (cout, cin), (cout,), (rows, cout)))
    grads = []
    for _ in range(CALLS):
        xd, wd, bd = (v.cuda().requires_grad_(True) for v in (x, w, bias))
        y = ops.linear(xd, wd, bd, lowp=mode == "lowp", split=mode == "split")
        y.backward(gy.cuda())
        torch.cuda.synchronize()
        grads.append((xd.grad.cpu(), wd.grad.cpu(), bd.grad.cpu()))
    for k, what in enumerate(("dx", "dw", "db")):
        for i in range(1, CALLS):
            assert torch.equal(grads[i][k].view(torch.int32), grads[0][k].view(torch.int32)), f"linear[{mode}] {what}: call {i} differs from call 0"
    stored = gy.to(BF if mode == "lowp" else FP).double()          # (the operand as the weight-gradient call is handed it)
    err = Measured(((grads[0][2].double() - stored.sum(0)).abs() / stored.abs().sum(0).clamp_min(1e-300)).max().item())
    print(f"linear[{mode},{rows}x{cin}->{cout}] db: worst |err| / sum|terms| = {float(err):.3g}")
    assert err <= BAR_BIAS


# =====================================================================================================================================
# 4. refusals
# =====================================================================================================================================
@pytest.mark.gpu
def test_refusals_under_the_option(det):
    """no silent fall-back to atomics: a walk grid whose ordered kernel does not fit the LDS, and <w, dW> (wdot), are DIN_E_ARG naming the
    option, before anything is launched (every destination keeps its bits); without the option both calls run"""
    lib, L, nhwc, ops = det
    b, t, n, c, kh, kw = 1, 1, 160, 64, 1, 49
    k2 = kh * kw
    X, P, A, GZ = (_Buf((b, t, n), m, content=torch.zeros(b, t, n, m)) for m in (c, 3 * k2, k2, c))
    DX, DP = _Buf((b, t, n), c), _Buf((b, t, n), 3 * k2)
    scratch = torch.zeros(b * t * n * 3 * k2).cuda()
    call = lambda: lib.din_walk_bwd(X.ptr(), P.ptr(), 3 * k2, A.ptr(), GZ.ptr(), b, t, n, c, kh, kw, 1, 1, 0, None, None, DX.ptr(), DP.ptr(),  # noqa: E731
                                    scratch.data_ptr(), None)
    _refused(call(), OPTION)
    torch.cuda.synchronize()
    assert DX.unchanged() and DP.unchanged()
    d = ops._desc(1, 1, 96, 40, 24, 1, 1, 0, 0, 1, 40, 24)
    xin, gin, w = torch.randn(96, 40).cuda(), torch.randn(96, 24).cuda(), torch.randn(24, 40).cuda()
    dw, db, wdot = _Buf((24,), 40), _Buf((1,), 24), _Buf((1,), 24)
    wsb = lib.din_conv_workspace_bytes(C.byref(d), 2)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device="cuda")
    wcall = lambda: lib.din_conv_wgrad(C.byref(d), xin.data_ptr(), gin.data_ptr(), dw.ptr(), db.ptr(), None, w.data_ptr(), wdot.ptr(), 0,  # noqa: E731
                                       ws.data_ptr(), wsb, None)
    _refused(wcall(), OPTION)
    torch.cuda.synchronize()
    assert dw.unchanged() and db.unchanged() and wdot.unchanged()
    with ops.deterministic(False):
        L.check(call())
        L.check(wcall())
        torch.cuda.synchronize()
    assert not DX.unchanged() and not wdot.unchanged()


# =====================================================================================================================================
# 5. models
# =====================================================================================================================================
def _model_cfg(module, dataset="volleyball"):
    from din_amd.config import Config
    cfg = Config(dataset)
    nfb = 1024 if module == "pctdm_volleyball" else 32              # (PCTDM's recurrent layers are sized for 1024 features)
    cfg.backbone, cfg.image_size, cfg.out_size, cfg.emb_features = "vgg16", (64, 96), (2, 3), 512
    cfg.num_boxes, cfg.num_frames, cfg.num_features_boxes, cfg.num_features_gcn = 4, 2, nfb, nfb
    cfg.num_features_relation, cfg.num_graph, cfg.gcn_layers, cfg.pos_threshold = 16, 16, 1, 0.5
    cfg.ST_kernel_size, cfg.sampling_ratio = [(3, 3)], [1]
    cfg.inference_module_name, cfg.training_stage, cfg.train_backbone, cfg.train_dropout_prob = module, 2, False, 0.3
    return cfg


def _build(module, gpu):
    from din_amd.train_net_dynamic import build_model
    torch.manual_seed(3)
    return build_model(_model_cfg(module)).to(gpu).train()


def _reset_counters(model):
    for m in model.modules():
        if isinstance(getattr(m, "_step", None), int):
            m._step = 0


def _pass(model, images, boxes, labels):
    """one forward + backward from the first dropout masks; the gradients of every parameter that has one"""
    _reset_counters(model)
    for p in model.parameters():
        p.grad = None
    ret = model((images, boxes))
    loss = F.cross_entropy(ret["activities"], labels)
    loss.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    return {k: v.grad.detach().clone() for k, v in model.named_parameters() if v.grad is not None}


def _inputs(gpu):
    from oracle import din_oracle as O
    images, boxes, labels = O.synth_inputs(2, 2, 4, 64, 96, 2, 3, 8, seed=9)
    return images.to(gpu), boxes.to(gpu), labels.to(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("on", [True, False], ids=["option_set", "option_unset"])
@pytest.mark.parametrize("module", ["dynamic_volleyball", "arg_volleyball", "at_volleyball", "dynamic_tce_volleyball", "pctdm_volleyball"])
def test_two_passes_from_the_same_weights_give_the_same_gradients(env, module, on):  # noqa: F811
    """VGG16 fp32, frozen backbone, training mode, dropout on, fixed seeds.  With the option unset the same code runs and nothing is said
    about its bits"""
    lib, L, nhwc, ops = env
    gpu = torch.device("cuda:0")
    with ops.deterministic(on):
        model = _build(module, gpu)
        first = _pass(model, *_inputs(gpu))
        second = _pass(model, *_inputs(gpu))
    assert first and first.keys() == second.keys() and not any(k.startswith("backbone.") for k in first)
    assert all(bool(torch.isfinite(v).all()) for v in first.values()) and any(bool(v.any()) for v in first.values())
    if on:
        differ = [k for k in first if not torch.equal(first[k].view(torch.int32), second[k].view(torch.int32))]
        assert not differ, f"{module}: gradients differ between two passes: {differ}"


@pytest.mark.gpu
@pytest.mark.parametrize("on", [True, False], ids=["option_set", "option_unset"])
def test_two_builds_trained_three_steps_have_the_same_weights(env, on):  # noqa: F811
    from din_amd.optim import FusedAdam
    lib, L, nhwc, ops = env
    gpu = torch.device("cuda:0")
    weights = []
    with ops.deterministic(on):
        for _ in range(2):
            model = _build("dynamic_volleyball", gpu)
            params = [p for p in model.parameters() if p.requires_grad]
            opt = FusedAdam(params, lr=1e-3, weight_decay=0.0)
            images, boxes, labels = _inputs(gpu)
            for _ in range(3):
                opt.zero_grad()
                F.cross_entropy(model((images, boxes))["activities"], labels).backward()
                opt.step()
            torch.cuda.synchronize()
            weights.append({k: v.detach().clone() for k, v in model.named_parameters() if v.requires_grad})
    assert all(bool(torch.isfinite(v).all()) for v in weights[0].values())
    if on:
        differ = [k for k in weights[0] if not torch.equal(weights[0][k].view(torch.int32), weights[1][k].view(torch.int32))]
        assert not differ, f"weights differ after three steps: {differ}"


@pytest.mark.gpu
@pytest.mark.parametrize("module,dataset", [("dynamic_volleyball", "volleyball"), ("dynamic_collective", "collective")])
def test_train_net_twice_under_the_setting_reports_the_same_losses(env, module, dataset, tmp_path):  # noqa: F811
    """cfg.deterministic through the trainer (synthetic clips, two epochs with a test pass each): two runs report the same train and test
    losses to the last bit, and the option is unset again afterwards"""
    from din_amd.train_net_dynamic import train_net
    lib, L, nhwc, ops = env
    runs = []
    for i in range(2):
        cfg = _model_cfg(module, dataset)
        cfg.deterministic, cfg.result_path = True, str(tmp_path / str(i))
        (tmp_path / str(i)).mkdir()
        cfg.batch_size, cfg.test_batch_size, cfg.max_epoch, cfg.test_interval_epoch, cfg.train_learning_rate, cfg.lr_plan = 2, 2, 2, 1, 1e-3, {}
        runs.append([(e["train"]["loss"], e["test"]["loss"]) for e in train_net(cfg)])
        assert L.get_option(OPTION) is None
    assert len(runs[0]) == 2 and runs[0] == runs[1], runs


# =====================================================================================================================================
# 6. graph capture
# =====================================================================================================================================
@pytest.mark.gpu
def test_ordered_launches_replay_from_a_captured_graph(det):
    """the ordered walk, LayerNorm and head backward launches are plain launches on the given stream: recorded into a graph and replayed,
    they write the bits the direct calls wrote"""
    lib, L, nhwc, ops = det
    row = WALK_ROWS[WALK_IDS.index("k33")]
    g, o, want = _walk_geom(row), _walk_operands("k33"), _walk_expected("k33")
    b, t, n, c, kh, kw, k2, cp = (g[k] for k in ("b", "t", "n", "c", "kh", "kw", "k2", "cp"))
    x, pred, gz, a = (v.cuda() for v in (o["x"], o["pred"], o["gz"], want["a"].float()))
    dx, dpred, scratch = torch.empty_like(x), torch.zeros_like(pred), torch.empty(b * t * n * 3 * k2, device="cuda")
    lo = _ln_operands(9, 20, 0.0)
    lwant = _ln_expected((9, 20, 0.0), (0, 0, 0.0))
    lx, lg, ldy = lo["x"].cuda(), lo["gamma"].cuda(), lo["dy"].cuda()
    ly, lst = lwant["y"].float().cuda(), torch.stack([lwant["mean"], lwant["rstd"]], dim=1).float().cuda()
    ldx, ldg, ldb = torch.empty_like(lx), torch.zeros(20, device="cuda"), torch.zeros(20, device="cuda")
    shape = (2, 3, 12, 256, 8)
    hb, ht, hn, hc, ha = shape
    ho, hwant = _head_operands(shape), head_reference(shape, "all")
    hs, hw, hdsc, ham = ho["s"].cuda(), ho["w"].cuda(), ho["dsc"].cuda(), hwant["argmax"].int().cuda()
    hds, hdw, hdb = torch.empty_like(hs), torch.zeros(ha, hc, device="cuda"), torch.zeros(ha, device="cuda")

    def launch():
        st = torch.cuda.current_stream().cuda_stream
        ldg.zero_(), ldb.zero_(), hdw.zero_(), hdb.zero_()
        L.check(lib.din_walk_bwd(x.data_ptr(), pred.data_ptr(), cp, a.data_ptr(), gz.data_ptr(), b, t, n, c, kh, kw, 1, 1, 0, None, None,
                                 dx.data_ptr(), dpred.data_ptr(), scratch.data_ptr(), st))
        L.check(lib.din_layernorm_bwd(ldy.data_ptr(), lx.data_ptr(), None, lg.data_ptr(), ly.data_ptr(), lst.data_ptr(), ldx.data_ptr(),
                                      ldg.data_ptr(), ldb.data_ptr(), 9, 20, 0, 0.0, LN_SEED, None, st))
        L.check(lib.din_head_bwd(hdsc.data_ptr(), hs.data_ptr(), hw.data_ptr(), ham.data_ptr(), hb, ht, hn, hc, ha, hds.data_ptr(),
                                 hdw.data_ptr(), hdb.data_ptr(), st))

    outs = (dx, dpred, ldx, ldg, ldb, hds, hdw, hdb)
    launch()
    torch.cuda.synchronize()
    direct = [v.clone() for v in outs]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for replay in range(2):
        for v in outs:
            v.fill_(float("nan"))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        for v, d in zip(outs, direct):
            assert torch.equal(v.view(torch.int32), d.view(torch.int32)), f"replay {replay} differs from the direct launches"
    _check("graph", "walk dx", dx.cpu(), want["dx"], _walk_bars(want, k2, g["nch"], 1)["dx"])
