"""GPU (-m gpu): every kernel that regenerates the dropout keep-mask -- din_act_dropout_fwd / _bwd, din_layernorm_fwd / _bwd (row kernels,
the atomic and the ordered dgamma / dbeta reductions), din_basenet_head_fwd / _bwd, din_actor_attn_fwd / _bwd -- against the host model
tests/dropout_reference.py.  The contract: the element at flat index i of the masked tensor is scaled by
keep_scale(fold_seed(seed, word), i, p), forward and backward.  Every comparison of a mask is torch.equal against the model: no
tolerance, and no expected value comes from a kernel of this library.  Values that depend on the mask (LayerNorm dx, the head's forward,
the attention backward) are held to the bars tests/test_gpu_head_path.py, test_gpu_stage1.py and test_gpu_at.py already use, their float64
references fed the model's mask.

Seeds: 7919 (= ops.mask_seed_of(0, 0, 1)), 2^40 + 12345 (a seed cut to 32 bits draws another mask), 2^63 - 1; each without a device word,
with a word of graph_step.SEED_STRIDE, and with OFF_WRAP, under which every seed + word passes 2^63.  OFF_WRAP folds 7919 to the seed 1062,
chosen (by a search over the model) because its first 600001 draws hold u == 0 (index 427104) and u == 2^-24 (index 225549): at p = 2^-24
the first is the only element dropped and the second is kept -- `u > p` for `u >= p` fails there.

Shapes: the smallest that reach every index expression -- act_dropout beyond its 2048 x 256 grid cap with a ragged tail; LayerNorm's
float4 path for less than, exactly and more than one pass of 512 threads, and its scalar path; the head plain, collective and T-mean; the
attention with C = 100 (a ragged last pass of the float4 row walk), one actor, and C = 1024.  tests/test_dropout_cpu.py shows on the CPU
that each wrong mask (a period, an index off by one, a cut seed, ^ for +, > for >=) differs from the right one on these very cases."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from din_amd.graph_step import SEED_STRIDE
from tests import dropout_reference as R
from tests.test_gpu_head_path import (_Buf, _all_outside, _all_unchanged, _bits, _check, _gen, _ln_launch, _refused, env,  # noqa: F401
                                      ln_reference)

SEEDS = (7919, (1 << 40) + 12345, (1 << 63) - 1)
EDGE_SEED, EDGE_IDX_ZERO, EDGE_IDX_ONE = 1062, 427104, 225549
OFF_WRAP = (1 << 63) + EDGE_SEED - SEEDS[0]
SEED_CASES = [(s, o) for s in SEEDS for o in (None, SEED_STRIDE, OFF_WRAP)]
P_ALL = (0.3, 0.5)
ACT_P = P_ALL + (0.0, 2.0 ** -24)
ACT_SIZES = (600001, 257, 1)
LN_SHAPES = [(3, 1024), (5, 2052), (4, 1023), (2, 7), (1, 4)]
HEAD_SHAPES = [(2, 1, 5, 128, 9, 8, "plain"), (3, 2, 7, 200, 16, 16, "collective"), (2, 3, 5, 200, 9, 8, "mean")]   # B, T, N, C, A_act, A_grp
AT_SHAPES = [(3, 12, 100), (2, 1, 4), (2, 13, 1024)]
CROSS_SHAPE = (24, 1024)
_ids = lambda shapes: ["x".join(map(str, s)) for s in shapes]  # noqa: E731


def _case_id(seed, off):
    return f"seed {seed:#x}, word {'none' if off is None else hex(off)}"


def _word(off):
    """the device word of a launch (int64 storage of the uint64 value) and its pointer; (None, None) without one"""
    if off is None:
        return None, None
    w = torch.tensor([off - (1 << 64) if off >> 63 else off], dtype=torch.int64).cuda()
    return w, w.data_ptr()


def _word_intact(w, off):
    return w is None or (int(w.cpu()) & ((1 << 64) - 1)) == off


@functools.lru_cache(maxsize=40)
def _model(seed, off, n, p):
    """(keep_scale float32 [n], keep bool [n]) of the model for a launch"""
    s = R.fold_seed(seed, off)
    idx = np.arange(n, dtype=np.int64)
    return torch.from_numpy(R.keep_scale(s, idx, p)), torch.from_numpy(R.keep(s, idx, p))


def _same_bits(got, want):
    return got.shape == want.shape and torch.equal(_bits(got), _bits(want))


# =====================================================================================================================================
# act_dropout
# =====================================================================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize("n", ACT_SIZES)
def test_act_dropout_mask_is_the_model(env, n):
    lib, L, nhwc, ops = env
    ones, neg = _Buf((1,), n, content=torch.ones(n)), _Buf((1,), n, content=-torch.ones(n))
    for seed, off in SEED_CASES:
        word, wp = _word(off)
        for p in ACT_P:
            tag = f"n {n}, {_case_id(seed, off)}, p {p}"
            ks, keep = _model(seed, off, n, p)
            Y, GX = _Buf((1,), n), _Buf((1,), n)
            L.check(lib.din_act_dropout_fwd(ones.ptr(), Y.ptr(), n, 0, p, seed, wp, None))
            L.check(lib.din_act_dropout_bwd(ones.ptr(), ones.ptr(), GX.ptr(), n, 0, p, seed, wp, None))
            torch.cuda.synchronize()
            assert _all_outside(Y, GX), f"{tag}: wrote outside a destination"
            assert _same_bits(Y.get()[0], ks), f"{tag}: the forward's mask is not the model's"
            assert _same_bits(GX.get()[0], ks), f"{tag}: the backward's mask is not the model's"
            if off is None:                                       # ReLU of a negative input: exactly 0 both ways, kept or not
                YN, GN = _Buf((1,), n), _Buf((1,), n)
                L.check(lib.din_act_dropout_fwd(neg.ptr(), YN.ptr(), n, 1, p, seed, wp, None))
                L.check(lib.din_act_dropout_bwd(ones.ptr(), neg.ptr(), GN.ptr(), n, 1, p, seed, wp, None))
                torch.cuda.synchronize()
                assert _all_outside(YN, GN) and not bool(YN.get().any()) and not bool(GN.get().any()), f"{tag}: ReLU let a negative input through"
            if p == 0.0:
                assert bool(keep.all()) and bool((Y.get() == 1.0).all())
        assert _word_intact(word, off)
    assert _all_unchanged(ones, neg)
    if n > EDGE_IDX_ZERO:                                         # the edge of u >= p really is inside this case
        ks, keep = _model(SEEDS[0], OFF_WRAP, n, 2.0 ** -24)
        assert (~keep).nonzero().flatten().tolist() == [EDGE_IDX_ZERO] and bool(keep[EDGE_IDX_ONE])


# =====================================================================================================================================
# LayerNorm
# =====================================================================================================================================
@functools.lru_cache(maxsize=None)
def _ln_inputs(rows, length):
    gen = _gen(f"dropout_ln{rows}x{length}")
    z = torch.zeros(length)
    return dict(x=0.1 * torch.randn(rows, length, generator=gen), res=0.1 * torch.randn(rows, length, generator=gen),
                beta=0.5 * torch.randn(length, generator=gen), dy=torch.randn(rows, length, generator=gen),
                dg0=torch.randn(length, generator=gen), db0=torch.randn(length, generator=gen), zeros=z, ones=torch.ones(length),
                pow2=(2.0 ** torch.arange(rows, dtype=torch.float32))[:, None].expand(rows, length).contiguous())


@pytest.mark.gpu
@pytest.mark.parametrize("rows,length", LN_SHAPES, ids=_ids(LN_SHAPES))
def test_layernorm_fwd_mask_is_the_model(env, rows, length):
    """gamma = 0, beta = 1: (x - mean) * rstd * 0 + 1 == 1 for finite statistics, so y is the keep-scale itself, bit for bit"""
    lib, L, nhwc, ops = env
    i = _ln_inputs(rows, length)
    o = dict(x=i["x"], res=i["res"], gamma=i["zeros"], beta=i["ones"])
    for seed, off in SEED_CASES:
        word, wp = _word(off)
        for p in P_ALL:
            ks, _ = _model(seed, off, rows * length, p)
            for res in (0, 1):
                for relu in (0, 1):
                    Y, S, _, _, _ = _ln_launch(lib, L, o, res, relu, p, seed, wp, None, None, bwd=False)
                    tag = f"{rows}x{length}, {_case_id(seed, off)}, p {p}, res {res}, relu {relu}"
                    assert bool(torch.isfinite(S.get()).all()), f"{tag}: statistics are not finite"
                    assert _same_bits(Y.get(), ks.view(rows, length)), f"{tag}: the forward's mask is not the model's"
        assert _word_intact(word, off)


def _dbeta_case(env, rows, length, seed, off, wp, relu, ordered):
    """gamma = 0 (y is the keep-scale), dy[r][col] = 2^r, p = 0.5: dbeta[col] = sum_r 2^(r + 1) keep(r, col), every partial sum exact in
    fp32 whatever its order (rows <= 24: 24 distinct powers of two), so dbeta decodes to the mask and is compared bit for bit"""
    lib, L, nhwc, ops = env
    i = _ln_inputs(rows, length)
    ks, _ = _model(seed, off, rows * length, 0.5)
    ks = ks.view(rows, length)
    o = dict(x=i["x"], res=i["res"], gamma=i["zeros"], beta=i["ones"], dy=i["pow2"], dg0=i["zeros"], db0=i["zeros"])
    stats = torch.stack([i["x"].mean(1), 1.0 / (i["x"].var(1, unbiased=False) + 1e-5).sqrt()], dim=1)
    with ops.deterministic(ordered):
        Y, S, DX, DG, DB = _ln_launch(lib, L, o, 0, relu, 0.5, seed, wp, stats, ks)
    want = (i["pow2"].double() * ks.double()).sum(0)
    assert float(want.max()) < 2.0 ** 25 and rows <= 24
    tag = f"{rows}x{length}, {_case_id(seed, off)}, relu {relu}, {'ordered' if ordered else 'atomic'}"
    assert _same_bits(DB.get()[0], want.float()), f"{tag}: dbeta does not decode to the model's mask"
    assert bool(torch.isfinite(DG.get()).all()) and bool(torch.isfinite(DX.get()).all()), tag


@pytest.mark.gpu
@pytest.mark.parametrize("ordered", [False, True], ids=["atomic", "ordered"])
@pytest.mark.parametrize("rows,length", LN_SHAPES, ids=_ids(LN_SHAPES))
def test_layernorm_bwd_dbeta_decodes_to_the_model(env, rows, length, ordered):
    lib, L, nhwc, ops = env
    before = L.get_option(ops.DETERMINISTIC_OPTION)
    for seed, off in SEED_CASES:
        word, wp = _word(off)
        for relu in (0, 1):
            _dbeta_case(env, rows, length, seed, off, wp, relu, ordered)
        assert _word_intact(word, off)
    assert L.get_option(ops.DETERMINISTIC_OPTION) == before


@pytest.mark.gpu
@pytest.mark.parametrize("rows,length", LN_SHAPES, ids=_ids(LN_SHAPES))
def test_layernorm_bwd_dx_under_the_model_mask(env, rows, length):
    """gamma = 1, p = 0.5, no ReLU: y and dx at the bars of tests/test_gpu_head_path.py's LayerNorm rows, the float64 reference reading
    the model's mask (the backward is handed the reference's statistics and y rounded to fp32, as there)"""
    lib, L, nhwc, ops = env
    i = _ln_inputs(rows, length)
    o = dict(x=i["x"], res=i["res"], gamma=i["ones"], beta=i["beta"], dy=i["dy"], dg0=i["dg0"], db0=i["db0"])
    for seed, off in SEED_CASES:
        word, wp = _word(off)
        _, keep = _model(seed, off, rows * length, 0.5)
        keep = keep.view(rows, length)
        for res in (0, 1):
            args = (o["x"], o["res"] if res else None, o["gamma"], o["beta"], o["dy"], 0, 0.5, keep)
            fwd = ln_reference(*args)
            stats = torch.stack([fwd["mean"], fwd["rstd"]], dim=1).float()
            want = ln_reference(*args, o["dg0"], o["db0"], None, stats=stats)
            yard = (ln_reference(*args, dtype=torch.float32, stats=stats)["dx"].double() - want["dx"]).abs().max(1, keepdim=True).values
            Y, S, DX, DG, DB = _ln_launch(lib, L, o, res, 0, 0.5, seed, wp, stats, want["y"].float())
            tag = f"ln {rows}x{length}, {_case_id(seed, off)}, res {res}"
            _check(tag, "y", Y.get(), want["y"], want["bars"]["y"])
            _check(tag, "dx", DX.get(), want["dx"], torch.maximum(4 * yard, want["bars"]["dx_floor"]))
            _check(tag, "dbeta", DB.get()[0], want["dbeta"], want["bars"]["dbeta"])
        assert _word_intact(word, off)


@pytest.mark.gpu
def test_layernorm_bwd_refuses_a_drop_p_outside_0_1(env):
    """as the forward and every other consumer of the mask: the argument error, and nothing launched"""
    lib, L, nhwc, ops = env
    rows, length = 3, 8
    i = _ln_inputs(rows, length)
    DY, X, YS = (_Buf((rows,), length, content=i[k]) for k in ("dy", "x", "res"))
    G, ST = _Buf((1,), length, content=i["ones"]), _Buf((rows,), 2, content=torch.ones(rows, 2))
    for p in (1.0, 1.5, -0.1, float("nan")):
        DX, DG, DB = _Buf((rows,), length), _Buf((1,), length, content=i["dg0"]), _Buf((1,), length, content=i["db0"])
        for det in (False, True):
            with ops.deterministic(det):
                rc = lib.din_layernorm_bwd(DY.ptr(), X.ptr(), None, G.ptr(), YS.ptr(), ST.ptr(), DX.ptr(), DG.ptr(), DB.ptr(), rows, length, 0, p,
                                           7919, None, None)
            _refused(rc, "layernorm_bwd: bad argument")
            assert rc == -1                                       # DIN_E_ARG
        torch.cuda.synchronize()
        assert _all_unchanged(DX, DG, DB, DY, X, YS, G, ST), f"drop_p {p}: a refused call wrote"
    _refused(lib.din_layernorm_fwd(X.ptr(), None, G.ptr(), G.ptr(), 1e-5, DX.ptr(), ST.ptr(), rows, length, 0, -0.1, 0, None, None),
             "layernorm_fwd: bad argument")


# =====================================================================================================================================
# stage-1 head
# =====================================================================================================================================
def _head_case(B, T, N, C_, aa, ag, form):
    from tests.test_gpu_stage1 import _head_inputs
    y, wa, ba, wg, bg, counts = _head_inputs(B, T, N, C_, aa, ag, seed=41 + B + T + C_, collective=form == "collective")
    gen = _gen(f"dropout_head{B}x{T}x{N}x{C_}")
    wa, wg = (0.1 + torch.rand(wa.shape, generator=gen)) / C_ ** 0.5, (0.1 + torch.rand(wg.shape, generator=gen)) / C_ ** 0.5   # > 0
    bt, mean = B * T, form == "mean"
    all_n = int(counts.sum()) if counts is not None else (B if mean else bt) * N
    groups = B if mean else bt
    ga, gg = 0.5 + torch.rand(all_n, aa, generator=gen), 0.5 + torch.rand(groups, ag, generator=gen)                             # > 0
    valid = torch.ones(bt, N, dtype=torch.bool) if counts is None else torch.arange(N)[None, :] < counts[:, None]
    return dict(y=y, wa=wa, ba=ba, wg=wg, bg=bg, counts=counts, bt=bt, mean=mean, all_n=all_n, groups=groups, ga=ga, gg=gg, valid=valid)


def _head_launch(env, h, T, N, C_, aa, ag, p, seed, wp):
    """din_basenet_head_fwd then _bwd through the C ABI on guarded buffers -> (actions, activities, g_y)"""
    lib, L, nhwc, ops = env
    bt, all_n, groups = h["bt"], h["all_n"], h["groups"]
    Y, WA, BA, WG, BG = (_Buf(lead, c, content=h[k]) for k, lead, c in (("y", (bt, N), C_), ("wa", (aa,), C_), ("ba", (1,), aa),
                                                                        ("wg", (ag,), C_), ("bg", (1,), ag)))
    cnt = h["counts"].cuda() if h["counts"] is not None else None
    cp = cnt.data_ptr() if cnt is not None else None
    ACT, ACTY, AM = _Buf((all_n,), aa), _Buf((groups,), ag), _Buf((bt,), C_, torch.int32)
    L.check(lib.din_basenet_head_fwd(Y.ptr(), WA.ptr(), BA.ptr(), WG.ptr(), BG.ptr(), cp, all_n, bt, T, int(h["mean"]), N, C_, aa, ag, p, seed, wp,
                                     ACT.ptr(), ACTY.ptr(), AM.ptr(), None))
    torch.cuda.synchronize()
    assert _all_outside(ACT, ACTY, AM) and _all_unchanged(Y, WA, BA, WG, BG), "basenet_head_fwd wrote outside a destination or into a source"
    GA, GG = _Buf((all_n,), aa, content=h["ga"]), _Buf((groups,), ag, content=h["gg"])
    GY, DWA, DBA, DWG, DBG = _Buf((bt, N), C_), _Buf((aa,), C_), _Buf((1,), aa), _Buf((ag,), C_), _Buf((1,), ag)
    am_bits = AM.bits()
    L.check(lib.din_basenet_head_bwd(GA.ptr(), GG.ptr(), Y.ptr(), WA.ptr(), WG.ptr(), AM.ptr(), cp, all_n, bt, T, int(h["mean"]), N, C_, aa, ag, p,
                                     seed, wp, GY.ptr(), DWA.ptr(), DBA.ptr(), DWG.ptr(), DBG.ptr(), None))
    torch.cuda.synchronize()
    assert _all_outside(GY, DWA, DBA, DWG, DBG) and _all_unchanged(Y, WA, WG, GA, GG) and torch.equal(AM.bits(), am_bits), \
        "basenet_head_bwd wrote outside a destination or into a source"
    if cnt is not None:
        assert torch.equal(cnt.cpu(), h["counts"])
    return ACT.get(), ACTY.get(), GY.get()


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,N,C_,aa,ag,form", HEAD_SHAPES, ids=[s[-1] for s in HEAD_SHAPES])
def test_basenet_head_mask_is_the_model(env, B, T, N, C_, aa, ag, form):
    """forward: the bars of tests/test_gpu_stage1.py against its float64 head fed relu(y) * the model's keep-scale.  backward: with
    g_actions, g_activities and both weight matrices strictly positive no product cancels, so g_y is nonzero exactly where y > 0 and the
    model keeps; padding boxes of the collective form get exactly 0"""
    from tests.test_gpu_stage1 import rel, torch_head
    h = _head_case(B, T, N, C_, aa, ag, form)
    y, valid = h["y"], h["valid"]
    assert form != "collective" or not bool(valid.all())
    for seed, off in SEED_CASES:
        word, wp = _word(off)
        for p in P_ALL:
            ks, keep = _model(seed, off, h["bt"] * N * C_, p)
            ks, keep = ks.view(h["bt"], N, C_), keep.view(h["bt"], N, C_)
            act, acty, gy = _head_launch(env, h, T, N, C_, aa, ag, p, seed, wp)
            tag = f"{form}, {_case_id(seed, off)}, p {p}"
            s64 = torch.relu(y).double() * ks.double()
            a64, g64 = torch_head(s64, h["wa"].double(), h["ba"].double(), h["wg"].double(), h["bg"].double(), h["counts"], T, h["mean"])
            assert act.shape == a64.shape and acty.shape == g64.shape
            ea, eg = rel(act, a64), rel(acty, g64)
            print(f"{tag}: actions {float(ea):.3g}, activities {float(eg):.3g}")
            assert ea <= 1e-5 and eg <= 1e-5, tag
            live = (y > 0) & keep
            assert torch.equal((gy != 0)[valid], live[valid]), f"{tag}: g_y is not masked by the model's mask"
            assert not bool(gy[~valid].any()), f"{tag}: a padding box received a gradient"
            assert bool(live[valid].any()) and not bool(live[valid].all())
        assert _word_intact(word, off)


# =====================================================================================================================================
# actor attention
# =====================================================================================================================================
def _attention_run(ops, dev, a, p, seed, word, pad):
    from tests.test_gpu_at import _run_attention
    old, ops.SEED_OFFSET = ops.SEED_OFFSET, word
    try:
        return _run_attention(dev, *a, p=p, seed=seed, want_keep=True, pad=pad)
    finally:
        ops.SEED_OFFSET = old


@pytest.mark.gpu
@pytest.mark.parametrize("G,N,C_", AT_SHAPES, ids=_ids(AT_SHAPES))
def test_actor_attention_mask_is_the_model(env, G, N, C_):
    """the `keep` output over the flat [G, N, C] index (rows of the projection 8 floats wider than 3 C, Q / K / V at column offsets: the
    mask does not depend on the stride), and out, att and the six gradients at the bars of tests/test_gpu_at.py, max(4 yard, 1e-5), against
    float64 torch fed the model's mask -- the only check on the three index expressions of the backward"""
    from tests.test_gpu_at import GRAD_NAMES, _attn_inputs, _torch_attention_grads, rel
    lib, L, nhwc, ops = env
    dev = torch.device("cuda")
    a = _attn_inputs(G, N, C_, seed=61 + G + N + C_)
    for seed, off in SEED_CASES:
        word, _ = _word(off)
        for p in P_ALL:
            tag = f"{G}x{N}x{C_}, {_case_id(seed, off)}, p {p}"
            _, keep = _model(seed, off, G * N * C_, p)
            keep = keep.view(G, N, C_)
            (out, att, got_keep), grads = _attention_run(ops, dev, a, p, seed, word, 8)
            assert torch.equal(got_keep.cpu(), keep), f"{tag}: the forward's mask is not the model's"
            o64, a64, g64 = _torch_attention_grads(torch.float64, *a, keep=keep, p=p)
            o32, a32, g32 = _torch_attention_grads(torch.float32, *a, keep=keep, p=p)
            for name, got, ref64, ref32 in [("out", out, o64, o32), ("att", att, a64, a32)] + list(zip(GRAD_NAMES, grads, g64, g32)):
                yard, err = float(rel(ref32, ref64)), rel(got, ref64)
                print(f"{tag} {name}: err {float(err):.3e} yard {yard:.3e}")
                assert err <= max(4.0 * yard, 1e-5), (tag, name, float(err), yard)
        assert _word_intact(word, off)
    (_, _, unpadded), _ = _attention_run(ops, dev, a, 0.5, SEEDS[1], None, 0)
    assert torch.equal(unpadded.cpu(), _model(SEEDS[1], None, G * N * C_, 0.5)[1].view(G, N, C_))
    assert ops.SEED_OFFSET is None


# =====================================================================================================================================
# all four families on one tensor; graph replay
# =====================================================================================================================================
@pytest.mark.gpu
def test_all_consumers_draw_one_mask(env):
    """one (seed, word, p) on one [24, 1024] tensor through act_dropout, LayerNorm (y, and dbeta through the many-rows reduction and the
    ordered one), the stage-1 head (g_y, as 2 frames of 12 boxes) and the attention (keep, as G = 2, N = 12): four masks equal to the
    model's, hence to each other"""
    lib, L, nhwc, ops = env
    rows, length = CROSS_SHAPE
    n = rows * length
    seed, off, p = SEEDS[1], SEED_STRIDE, 0.5
    word, wp = _word(off)
    ks, keep = _model(seed, off, n, p)
    keep2 = keep.view(rows, length)
    ones, Y = _Buf((1,), n, content=torch.ones(n)), _Buf((1,), n)
    L.check(lib.din_act_dropout_fwd(ones.ptr(), Y.ptr(), n, 0, p, seed, wp, None))
    torch.cuda.synchronize()
    assert _same_bits(Y.get()[0], ks) and _all_outside(Y)
    i = _ln_inputs(rows, length)
    o = dict(x=i["x"], res=i["res"], gamma=i["zeros"], beta=i["ones"])
    LY, S, _, _, _ = _ln_launch(lib, L, o, 1, 1, p, seed, wp, None, None, bwd=False)
    assert bool(torch.isfinite(S.get()).all()) and _same_bits(LY.get(), ks.view(rows, length))
    for ordered in (False, True):
        _dbeta_case(env, rows, length, seed, off, wp, 1, ordered)
    h = _head_case(2, 1, 12, length, 9, 8, "plain")
    h["y"] = h["y"].abs() + 0.1                                   # every element passes the ReLU: g_y != 0 is the mask alone
    _, _, gy = _head_launch(env, h, 1, 12, length, 9, 8, p, seed, wp)
    assert torch.equal((gy != 0).view(rows, length), keep2)
    from tests.test_gpu_at import _attn_inputs
    (_, _, at_keep), _ = _attention_run(ops, torch.device("cuda"), _attn_inputs(2, 12, length, seed=7), p, seed, word, 8)
    assert torch.equal(at_keep.cpu().view(rows, length), keep2)
    assert torch.equal((Y.get()[0] != 0).view(rows, length), keep2) and torch.equal(LY.get() != 0, keep2)
    assert _word_intact(word, off)


@pytest.mark.gpu
def test_replayed_graph_advances_the_mask_by_seed_stride(env):
    """din_act_dropout_fwd on ones and din_counter_add(SEED_STRIDE) captured in one graph: replay k draws the model's mask of
    fold_seed(seed, k * SEED_STRIDE), as a captured training step does"""
    lib, L, nhwc, ops = env
    n, p, seed = 4099, 0.3, SEEDS[0]
    word = torch.zeros(1, dtype=torch.int64).cuda()
    ones, out = torch.ones(n).cuda(), torch.full((n,), float("nan")).cuda()
    L.check(lib.din_act_dropout_fwd(ones.data_ptr(), out.data_ptr(), n, 0, p, seed, word.data_ptr(), None))      # (eager once: the word is 0)
    torch.cuda.synchronize()
    assert _same_bits(out.cpu(), _model(seed, 0, n, p)[0])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        L.check(lib.din_act_dropout_fwd(ones.data_ptr(), out.data_ptr(), n, 0, p, seed, word.data_ptr(), st))
        L.check(lib.din_counter_add(word.data_ptr(), SEED_STRIDE, st))
    seen = []
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        got = out.cpu()
        assert int(word.cpu()) == ((k + 1) * SEED_STRIDE) & ((1 << 63) - 1)
        assert _same_bits(got, _model(seed, (k * SEED_STRIDE) & ((1 << 63) - 1), n, p)[0]), f"replay {k} did not draw the model's mask"
        seen.append(got)
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
