"""GPU (-m gpu): the PCTDM baseline.  The LSTM kernels (csrc/lstm.hip) against torch.nn.LSTM in float64 on the CPU, the pooling and attention
kernels (csrc/pctdm_attention.hip) against float64 torch, guard bands, rerun bit-identity, softmax stability; the PCTDM module and
PCTDM_volleyball against the reference's fixtures (tests/golden/pctdm_*.npz, tools/gen_golden_pctdm.py); the stage-2 trainer with
`inference_module_name = 'pctdm_volleyball'`; the reference launcher's opening lines.

Bars.  Kernel rows: max(4 * yard, 1e-5) relative to the float64 value (max |got - ref| / max |ref|), yard = the same torch module in fp32 on
the CPU against float64 -- the project's rule, tests/test_gpu_at.py: two fp32 evaluations that differ in summation order are each up to one
yard from the float64 value, and no assert may pass under 2x.  torch.nn.LSTM returns the output, the last cell state and the gradients of its
own leaves; the elementwise checks of every saved cell and of d_pre use tests/pctdm_reference.py (checked here against torch.nn.LSTM in
float64 first).  Fixtures: logits and loss 1e-4, intermediates and gradients max(5 * yard, 1e-4) with the fixture's own yard, backbone gsum at
the model_* fixtures' bars, as tests/test_gpu_at.py."""
import ctypes as C
import glob
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import din_oracle as O
from tests import pctdm_reference as R
from tests.conftest import Measured

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tools"))
MODULE_CASES = ["pctdm_module_g3_n4", "pctdm_module_g2_n12"]
MODEL_CASES = ["pctdm_vgg16_96x160", "pctdm_vgg16_96x160_eval_n12"]

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from din_amd import _lib
    _lib.load()
    return torch.device("cuda")


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return Measured(((a - b).abs().max() / (b.abs().max() + 1e-30)).item())


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def C_stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- LSTM -------------------------------------------------------------------------------------------------------------------------------
LSTM_SHAPES = [(1, 1, 1, 4), (3, 5, 2, 20), (70, 3, 1, 36), (5, 2, 2, 130), (20, 12, 2, 1000), (40, 6, 1, 1000)]
LSTM_IDS = ["smallest", "odd_sizes", "rows_beyond_one_chunk", "h130_not_multiple_of_4", "launcher_bi_lstm", "launcher_intra_group"]
LSTM_IN = 16                      # input width of the torch module; the kernel takes the input projection, formed here in float64


def _lstm_case(Rr, S, D, H, seed):
    """float64 torch.nn.LSTM with weights of the usual 1/sqrt(H) scale, an input and a cotangent -> everything both sides need"""
    g = torch.Generator().manual_seed(seed)
    m = torch.nn.LSTM(LSTM_IN, H, num_layers=1, batch_first=True, bidirectional=D == 2).double()
    with torch.no_grad():
        for p in m.parameters():
            p.copy_((torch.rand(p.shape, generator=g, dtype=torch.float64) * 2 - 1) / (H ** 0.5 if p.dim() == 2 and p.shape[1] == H else 1.0))
    x = torch.randn((Rr, S, LSTM_IN), generator=g, dtype=torch.float64)
    cot = torch.randn((Rr, S, D * H), generator=g, dtype=torch.float64)
    return m, x, cot


def _torch_lstm(m, x, cot, dtype):
    import copy
    m = copy.deepcopy(m).to(dtype)
    xs = x.detach().to(dtype).clone().requires_grad_(True)
    out, (_h, c_n) = m(xs)
    out.backward(cot.to(dtype))
    sfx = ["", "_reverse"][:2 if m.bidirectional else 1]
    return dict(out=out.detach(), c_n=c_n.detach(), dx=xs.grad, dw_hh=torch.stack([getattr(m, "weight_hh_l0" + s).grad for s in sfx]),
                dw_ih=torch.stack([getattr(m, "weight_ih_l0" + s).grad for s in sfx]),
                db=torch.stack([getattr(m, "bias_ih_l0" + s).grad for s in sfx]))


def _pre_and_whh(m, x):
    sfx = ["", "_reverse"][:2 if m.bidirectional else 1]
    pre = torch.stack([x @ getattr(m, "weight_ih_l0" + s).t() + getattr(m, "bias_ih_l0" + s) + getattr(m, "bias_hh_l0" + s) for s in sfx], 2)
    return pre.detach(), torch.stack([getattr(m, "weight_hh_l0" + s) for s in sfx]).detach(), sfx


def _restated(pre, w_hh, cot, dtype):
    p = pre.detach().to(dtype).clone().requires_grad_(True)
    out, cells, _ = R.lstm(p, w_hh.detach().to(dtype))
    out.backward(cot.to(dtype))
    return dict(out=out.detach(), cells=cells.detach(), d_pre=p.grad)


def _run_lstm(dev, pre, w_hh, cot):
    from din_amd import ops
    p = pre.detach().float().to(dev).clone().requires_grad_(True)
    w = w_hh.detach().float().to(dev).clone().requires_grad_(True)
    out, gates, cells = ops.LSTMFunction.apply(p, w, True)
    out.backward(cot.float().to(dev))
    return dict(out=out.detach(), cells=cells, gates=gates, d_pre=p.grad, dw_hh=w.grad)


@pytest.mark.parametrize("Rr,S,D,H", LSTM_SHAPES, ids=LSTM_IDS)
def test_lstm_matches_float64_torch_lstm(gpu, Rr, S, D, H):
    m, x, cot = _lstm_case(Rr, S, D, H, seed=100 + Rr + S + D + H)
    t64, t32 = _torch_lstm(m, x, cot, torch.float64), _torch_lstm(m, x, cot, torch.float32)
    pre, w_hh, sfx = _pre_and_whh(m, x)
    r64, r32 = _restated(pre, w_hh, cot, torch.float64), _restated(pre, w_hh, cot, torch.float32)
    assert float(rel(r64["out"], t64["out"])) <= 1e-12, "the restatement in tests/pctdm_reference.py is not torch.nn.LSTM"
    got = _run_lstm(gpu, pre, w_hh, cot)
    gi = float(got["gates"][..., :2 * H].mean())
    assert 0.2 < gi < 0.8, "the i / f gates of this case are saturated"
    # what torch.nn.LSTM itself returns: output, last cell state, input gradient (d_pre through W_ih), dW_hh
    dpre = got["d_pre"].double().cpu()
    w_ih = torch.stack([getattr(m, "weight_ih_l0" + s).detach() for s in sfx])                       # [D, 4H, I]
    last = [S - 1, 0]
    rows = [("out", got["out"], t64["out"], t32["out"]),
            ("c_n", torch.stack([got["cells"][:, last[d], d] for d in range(D)]), t64["c_n"], t32["c_n"]),
            ("dx", torch.einsum("rsdm,dmi->rsi", dpre, w_ih), t64["dx"], t32["dx"]),
            ("dw_ih", torch.einsum("rsdm,rsi->dmi", dpre, x), t64["dw_ih"], t32["dw_ih"]),
            ("db", dpre.sum((0, 1)), t64["db"], t32["db"]),
            ("dw_hh", got["dw_hh"], t64["dw_hh"], t32["dw_hh"]),
            ("cells", got["cells"], r64["cells"], r32["cells"]),
            ("d_pre", got["d_pre"], r64["d_pre"], r32["d_pre"])]
    for name, g_, ref64, ref32 in rows:
        yard, err = float(rel(ref32, ref64)), rel(g_, ref64)
        print(f"{name}: err {float(err):.3e} yard {yard:.3e}")
        assert err <= max(4.0 * yard, 1e-5), (name, float(err), yard)


def test_lstm_h_prev_is_the_shifted_output_and_reruns_are_bit_identical(gpu):
    from din_amd import _lib, ops
    lib = _lib.load()
    Rr, S, D, H = 20, 5, 2, 1000
    m, x, cot = _lstm_case(Rr, S, D, H, seed=7)
    pre, w_hh, _ = _pre_and_whh(m, x)
    runs = [_run_lstm(gpu, pre, w_hh, cot) for _ in range(2)]
    for k in ("out", "cells", "gates", "d_pre"):
        assert torch.equal(runs[0][k], runs[1][k]), k
    a = runs[0]
    go = cot.float().to(gpu).contiguous()
    w = w_hh.float().to(gpu).contiguous()
    outs = []
    for _ in range(2):
        d_pre, h_prev = torch.full_like(a["gates"], float("nan")), torch.full_like(a["cells"], float("nan"))
        nws = ops.lstm_workspace_floats(Rr, D, H)
        ws = torch.empty(nws, device=gpu)
        assert lib.din_lstm_bwd(ptr(go), ptr(a["gates"]), ptr(a["cells"]), ptr(w), Rr, S, D, H, ptr(d_pre), ptr(h_prev), ptr(ws), nws,
                                C_stream()) == 0, lib.din_last_error_string()
        outs.append((d_pre, h_prev))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][0], a["d_pre"])
    h = a["out"].reshape(Rr, S, D, H)
    want = torch.zeros_like(h)
    want[:, 1:, 0] = h[:, :-1, 0]                                       # direction 0 enters position s with h of position s - 1
    want[:, :-1, 1] = h[:, 1:, 1]                                       # direction 1 with h of position s + 1
    assert torch.equal(outs[0][1], want)


# ---- pool and attention --------------------------------------------------------------------------------------------------------------------
PA_SHAPES = [(1, 4, 4), (3, 6, 100), (20, 12, 1000)]
PA_IDS = ["smallest", "g3_n6_h100", "launcher"]


def _pa_inputs(G, N, H, seed, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    lstm_out = torch.tanh(torch.randn((G, N, 2 * H), generator=g, dtype=torch.float64))
    src = torch.randn((G, N, H), generator=g, dtype=torch.float64)
    ctx = torch.randn((G, H), generator=g, dtype=torch.float64)
    w_e = 2.0 * torch.randn((H,), generator=g, dtype=torch.float64) / H ** 0.5
    b_e = torch.tensor([0.3 + shift], dtype=torch.float64)
    cot = torch.randn((G, N, H), generator=g, dtype=torch.float64)
    cot_c = torch.randn((G, H), generator=g, dtype=torch.float64)
    return lstm_out, src, ctx, w_e, b_e, cot, cot_c


def _torch_pa(dtype, lstm_out, src, ctx, w_e, b_e, cot, cot_c):
    ts = [t.detach().to(dtype).clone().requires_grad_(True) for t in (lstm_out, src, ctx, w_e, b_e)]
    pooled, winner, context = R.pool(ts[0])
    pooled.retain_grad()
    y, gamma = R.attention(pooled, ts[1], ts[2], ts[3], ts[4][0])
    (y * cot.to(dtype)).sum().add((context * cot_c.to(dtype)).sum()).backward()
    return dict(pooled=pooled.detach(), winner=winner, context=context.detach(), y=y.detach(), gamma=gamma.detach(), d_lstm_out=ts[0].grad,
                d_src=ts[1].grad, d_ctx=ts[2].grad, d_w_e=ts[3].grad, d_b_e=ts[4].grad)


def _run_pa(dev, lstm_out, src, ctx, w_e, b_e, cot, cot_c):
    from din_amd import ops
    ts = [t.detach().float().to(dev).clone().requires_grad_(True) for t in (lstm_out, src, ctx, w_e, b_e)]
    pooled, context, winner = ops.PctdmPoolFunction.apply(ts[0])
    y, gamma = ops.PctdmAttentionFunction.apply(pooled, ts[1], ts[2], ts[3], ts[4])
    (y * cot.float().to(dev)).sum().add((context * cot_c.float().to(dev)).sum()).backward()
    return dict(pooled=pooled.detach(), winner=winner, context=context.detach(), y=y.detach(), gamma=gamma.detach(), d_lstm_out=ts[0].grad,
                d_src=ts[1].grad, d_ctx=ts[2].grad, d_w_e=ts[3].grad, d_b_e=ts[4].grad)


@pytest.mark.parametrize("G,N,H", PA_SHAPES, ids=PA_IDS)
def test_pool_and_attention_match_float64_torch(gpu, G, N, H):
    a = _pa_inputs(G, N, H, seed=31 + G + N + H)
    # the kernel sees the fp32 rounding of lstm_out: the winners are those of the rounded values, exactly
    a = (a[0].float().double(),) + a[1:]
    t64, t32 = _torch_pa(torch.float64, *a), _torch_pa(torch.float32, *a)
    got = _run_pa(gpu, *a)
    rowmax = float(t64["gamma"].reshape(G, 2, N // 2).max(-1).values.mean())
    assert 1.2 / (N // 2) < rowmax < 0.95, f"the team softmax of this case is uniform or one-hot ({rowmax})"
    assert torch.equal(got["winner"].cpu(), t64["winner"])
    for name in ("pooled", "context", "y", "gamma", "d_lstm_out", "d_src", "d_ctx", "d_w_e"):
        yard, err = float(rel(t32[name], t64[name])), rel(got[name], t64[name])
        print(f"{name}: err {float(err):.3e} yard {yard:.3e}")
        assert err <= max(4.0 * yard, 1e-5), (name, float(err), yard)
    # d b_e is zero in exact arithmetic (a softmax ignores a common shift); the honest sum of the score gradients stays at rounding level
    db = Measured(float(got["d_b_e"].abs().max()))
    print(f"d_b_e {float(db):.3e} against max |d_w_e| {float(t64['d_w_e'].abs().max()):.3e}")
    assert db <= 1e-5 * float(t64["d_w_e"].abs().max())
    again = _run_pa(gpu, *a)
    for k, v in got.items():
        assert torch.equal(v, again[k]), k + " differs on a rerun"


def test_team_softmax_subtracts_the_maximum(gpu):
    G, N, H = 3, 6, 100
    a = _pa_inputs(G, N, H, seed=5)
    b = _pa_inputs(G, N, H, seed=5, shift=80.0)
    got, shifted = _run_pa(gpu, *a), _run_pa(gpu, *b)
    assert bool(torch.isfinite(shifted["gamma"]).all()) and bool(torch.isfinite(shifted["y"]).all())
    assert Measured(float((shifted["gamma"] - got["gamma"]).abs().max())) <= 1e-5
    assert Measured(float((shifted["gamma"].reshape(G, 2, N // 2).sum(-1) - 1).abs().max())) <= 1e-5


# ---- the C ABI on NaN-filled buffers ---------------------------------------------------------------------------------------------------------
def _banded(dev, n, guard, dtype=torch.float32):
    t = torch.full((n + 2 * guard,), float("nan") if dtype == torch.float32 else 255, dtype=dtype, device=dev)
    return t, t[guard:guard + n]


def _check_bands(bufs, guard, skip_body=()):
    torch.cuda.synchronize()
    for kk, (whole, inner) in bufs.items():
        w = whole.cpu()
        if w.dtype == torch.uint8:
            assert bool((w[:guard] == 255).all()) and bool((w[-guard:] == 255).all()), kk + ": guard band written"
            assert bool((inner.cpu() <= 1).all()), kk + ": output element not written"
            continue
        assert bool(torch.isnan(w[:guard]).all()) and bool(torch.isnan(w[-guard:]).all()), kk + ": guard band written"
        if kk not in skip_body:
            assert bool(torch.isfinite(inner.cpu()).all()), kk + ": output element not written"


@pytest.mark.parametrize("Rr,S,D,H", [(3, 5, 2, 20), (17, 2, 1, 130), (9, 3, 2, 36)], ids=["odd", "h130_two_chunks", "h36_bwd_two_chunks"])
def test_lstm_kernels_write_inside_their_outputs_only(gpu, Rr, S, D, H):
    from din_amd import _lib, ops
    lib = _lib.load()
    guard = 64                                                          # (multiple of 4 floats: the 16-byte alignment survives)
    m, x, cot = _lstm_case(Rr, S, D, H, seed=3)
    pre, w_hh, _ = _pre_and_whh(m, x)
    nws = ops.lstm_workspace_floats(Rr, D, H)
    assert nws == D * 4 * H * H + Rr * D * H
    nws4 = (nws + 3) // 4 * 4
    bufs = {k: _banded(gpu, n, guard) for k, n in dict(out=Rr * S * D * H, gates=Rr * S * D * 4 * H, cells=Rr * S * D * H, d_pre=Rr * S * D * 4 * H,
                                                       h_prev=Rr * S * D * H, ws=nws4).items()}
    p, w, go, st = pre.float().to(gpu), w_hh.float().to(gpu).contiguous(), cot.float().to(gpu), C_stream()
    assert lib.din_lstm_fwd(ptr(p), ptr(w), Rr, S, D, H, ptr(bufs["out"][1]), ptr(bufs["gates"][1]), ptr(bufs["cells"][1]), st) == 0, \
        lib.din_last_error_string()
    assert lib.din_lstm_bwd(ptr(go), ptr(bufs["gates"][1]), ptr(bufs["cells"][1]), ptr(w), Rr, S, D, H, ptr(bufs["d_pre"][1]),
                            ptr(bufs["h_prev"][1]), ptr(bufs["ws"][1]), nws, st) == 0, lib.din_last_error_string()
    _check_bands(bufs, guard, skip_body=("ws",))
    assert bool(torch.isfinite(bufs["ws"][1][:nws].cpu()).all()) and bool(torch.isnan(bufs["ws"][1][nws:].cpu()).all())
    r64 = _restated(pre, w_hh, cot, torch.float64)
    assert rel(bufs["out"][1].reshape(Rr, S, D * H), r64["out"]) <= 1e-5
    assert rel(bufs["d_pre"][1].reshape(Rr, S, D, 4 * H), r64["d_pre"]) <= 1e-4
    # refusals: nothing is written
    E_ARG = -1
    seven = torch.full((64,), 7.0, device=gpu)
    assert lib.din_lstm_fwd(ptr(p), ptr(w), Rr, S, 3, H, ptr(seven), ptr(seven), ptr(seven), st) == E_ARG
    assert lib.din_lstm_fwd(ptr(p), ptr(w), Rr, S, D, 1025, ptr(seven), ptr(seven), ptr(seven), st) == E_ARG
    assert lib.din_lstm_fwd(ptr(p), None, Rr, S, D, H, ptr(seven), ptr(seven), ptr(seven), st) == E_ARG
    assert lib.din_lstm_bwd(ptr(go), ptr(bufs["gates"][1]), ptr(bufs["cells"][1]), ptr(w), Rr, S, D, H, ptr(seven), ptr(seven), ptr(bufs["ws"][1]),
                            nws - 1, st) == E_ARG
    torch.cuda.synchronize()
    assert bool((seven == 7.0).all())


@pytest.mark.parametrize("G,N,H", [(3, 6, 100), (2, 4, 257)], ids=["g3_n6_h100", "h257_two_strides"])
def test_pool_and_attention_kernels_write_inside_their_outputs_only(gpu, G, N, H):
    from din_amd import _lib, ops
    lib = _lib.load()
    guard = 64
    lstm_out, src, ctx, w_e, b_e, cot, cot_c = (t.float().to(gpu) for t in _pa_inputs(G, N, H, seed=9))
    nws = ops.pctdm_att_workspace_floats(G, H)
    assert nws == G * H + G
    f, u = torch.float32, torch.uint8
    bufs = {k: _banded(gpu, n, guard, dt) for k, (n, dt) in dict(
        pooled=(G * N * H, f), winner=(G * N * H, u), context=(G * H, f), y=(G * N * H, f), gamma=(G * N, f), d_pooled=(G * N * H, f),
        d_src=(G * N * H, f), d_ctx=(G * H, f), d_w_e=(H, f), d_b_e=(1, f), ws=(nws, f), d_lstm_out=(G * N * 2 * H, f)).items()}
    st = C_stream()
    b = {k: v[1] for k, v in bufs.items()}
    assert lib.din_pctdm_pool_fwd(ptr(lstm_out), G, N, H, ptr(b["pooled"]), ptr(b["winner"]), ptr(b["context"]), st) == 0
    assert lib.din_pctdm_att_fwd(ptr(b["pooled"]), ptr(src), ptr(ctx), ptr(w_e), ptr(b_e), G, N, H, ptr(b["y"]), ptr(b["gamma"]), st) == 0
    assert lib.din_pctdm_att_bwd(ptr(cot), ptr(b["pooled"]), ptr(src), ptr(ctx), ptr(w_e), ptr(b["gamma"]), G, N, H, ptr(b["d_pooled"]),
                                 ptr(b["d_src"]), ptr(b["d_ctx"]), ptr(b["d_w_e"]), ptr(b["d_b_e"]), ptr(b["ws"]), nws, st) == 0
    assert lib.din_pctdm_pool_bwd(ptr(b["d_pooled"]), ptr(cot_c), ptr(b["winner"]), G, N, H, ptr(b["d_lstm_out"]), st) == 0
    _check_bands(bufs, guard)
    E_ARG = -1
    seven = torch.full((64,), 7.0, device=gpu)
    assert lib.din_pctdm_att_fwd(ptr(b["pooled"]), ptr(src), ptr(ctx), ptr(w_e), ptr(b_e), G, 5, H, ptr(seven), ptr(seven), st) == E_ARG
    assert lib.din_pctdm_att_fwd(ptr(b["pooled"]), ptr(src), ptr(ctx), ptr(w_e), ptr(b_e), G, 34, H, ptr(seven), ptr(seven), st) == E_ARG
    assert lib.din_pctdm_pool_fwd(ptr(lstm_out), G, 33, H, ptr(seven), ptr(seven), ptr(seven), st) == E_ARG
    assert lib.din_pctdm_att_bwd(ptr(cot), ptr(b["pooled"]), ptr(src), ptr(ctx), ptr(w_e), ptr(b["gamma"]), G, N, H, ptr(seven), ptr(seven),
                                 ptr(seven), ptr(seven), ptr(seven), ptr(b["ws"]), nws - 1, st) == E_ARG
    torch.cuda.synchronize()
    assert bool((seven == 7.0).all())


# ---- the module and the model against the reference's fixtures -------------------------------------------------------------------------------
def _unpack_winner(z, G, N):
    return torch.as_tensor(np.unpackbits(z["winner"])[:G * N * R.H].reshape(G, N, R.H)).bool()


def _probe_err(z, name, got):
    got = torch.as_tensor(got).detach().double().cpu().flatten()
    if "idx." + name in z.files:
        got, scale = got[torch.as_tensor(z["idx." + name])], float(z["max64_" + name])
    else:
        scale = float(np.abs(z[name + "64"]).max())
    return Measured(float((got - torch.as_tensor(z[name + "64"]).flatten()).abs().max()) / scale)


def _check_block(z, probes, G, N):
    assert torch.equal(probes["winner"].cpu(), _unpack_winner(z, G, N)), "a max-pool winner differs from the fixture's"
    for k, got in (("lstm_out", probes["lstm_out"]), ("pooled", probes["pooled"]), ("gamma", probes["gamma"]), ("out", probes["group_feas"])):
        err = _probe_err(z, k, got)
        print(f"{k}: err {float(err):.3e} yard {float(z['yard_' + k]):.3e}")
        assert err <= max(5.0 * float(z["yard_" + k]), 1e-4), k


def _check_grads(z, named, prefix=""):
    checked = 0
    w_e_max = None
    for k in z.files:
        if k.startswith("g64."):
            name = k[4:]
            got = named[prefix + name].grad.detach().flatten().double().cpu()
            if "gidx." + name in z.files:
                got = got[torch.as_tensor(z["gidx." + name])]
            checked += 1
            if name.endswith("att_extra_weights.0.bias"):
                # zero in exact arithmetic (the fixture's fp64 value is rounding noise, its yard meaningless): bounded absolutely like d_b_e
                # of the kernel test, by 1e-5 of the largest entry of the gradient of att_extra_weights.0.weight
                w_e_max = float(z["gmax64." + name.replace(".bias", ".weight")])
                assert Measured(float(got.abs().max())) <= 1e-5 * w_e_max, name
                continue
            err = Measured(float((got - torch.as_tensor(z[k])).abs().max()) / float(z["gmax64." + name]))
            assert err <= max(5.0 * float(z["yard." + name]), 1e-4), name
        if k.startswith("gsum.") and not k.startswith("gsum64."):
            name = k[5:]
            if name.endswith("att_extra_weights.0.bias"):
                continue
            gs_tol = 6e-3 if name.startswith("backbone.") else 2e-3       # the model_* fixtures' bars
            assert Measured(abs(named[prefix + name].grad.double().sum().item() - float(z[k]))) <= gs_tol * float(z["gabs." + name]) + 1e-6, name
    return checked


@pytest.mark.parametrize("name", MODULE_CASES)
def test_pctdm_module_matches_reference_golden(gpu, name):
    from din_amd.config import Config
    from din_amd.infer_module.pctdm_infer_module import PCTDM
    from gen_golden_pctdm import module_cot, module_input, module_shapes, pctdm_params
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    B, T, N = (int(v) for v in z["meta"][:3])
    cfg = Config("volleyball")
    cfg.num_boxes = N
    m = PCTDM(cfg)
    assert [str(k) for k in z["keys"]] == list(m.state_dict().keys())
    m.load_state_dict(pctdm_params(module_shapes(), int(z["seed"]), float(z["extra_scale"])))
    m = m.to(gpu).train()
    m.probes = {}
    x = module_input(B, T, N, int(z["seed"])).to(gpu).requires_grad_(True)
    out = m(x)
    assert tuple(out.shape) == (B * T, 2000)
    (out * module_cot(B * T, int(z["seed"])).to(gpu)).sum().backward()
    _check_block(z, m.probes, B * T, N)
    err = _probe_err(z, "gx", x.grad)
    assert err <= max(5.0 * float(z["yard_gx"]), 1e-4)
    assert _check_grads(z, dict(m.named_parameters())) == 18


def test_pctdm_output_stays_two_dimensional_for_one_frame(gpu):
    from din_amd.config import Config
    from din_amd.infer_module.pctdm_infer_module import PCTDM
    cfg = Config("volleyball")
    cfg.num_boxes = 4
    m = PCTDM(cfg).to(gpu)
    with torch.no_grad():
        out = m(torch.relu(torch.randn((1, 1, 4, 1024), device=gpu)))
    assert tuple(out.shape) == (1, 2000) and bool(torch.isfinite(out).all())


def _fixture_cfg(z):
    from din_amd.config import Config
    B, T, N, H, W, OH, OW, D, NFB, A = (int(v) for v in z["meta"])
    cfg = Config("volleyball")
    cfg.backbone, cfg.image_size, cfg.out_size, cfg.emb_features = str(z["backbone"]), (H, W), (OH, OW), D
    cfg.num_boxes, cfg.num_frames, cfg.num_features_boxes, cfg.num_activities = N, T, NFB, A
    cfg.train_backbone, cfg.train_dropout_prob = True, 0.0
    cfg.inference_module_name = "pctdm_volleyball"
    return cfg


@pytest.mark.parametrize("name", MODEL_CASES)
def test_pctdm_volleyball_matches_reference_golden(gpu, name):
    from din_amd.train_net_dynamic import build_model, set_bn_eval
    from gen_golden_pctdm import model_shapes, pctdm_params
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    B, T, N, H, W, OH, OW, D, NFB, A = (int(v) for v in z["meta"])
    cfg = _fixture_cfg(z)
    model = build_model(cfg)
    p = pctdm_params(model_shapes(cfg.backbone, D, T, A), int(z["seed"]), float(z["extra_scale"]))
    missing, unexpected = model.load_state_dict(p, strict=False)
    assert not unexpected and all("num_batches_tracked" in k for k in missing), (missing, unexpected)
    model = model.to(gpu)
    if str(z["mode"]) == "eval":
        model.eval()
    else:
        model.train()
        model.apply(set_bn_eval)
    images, boxes, labels = O.synth_inputs(B, T, N, H, W, OH, OW, A, seed=int(z["seed"]))
    assert torch.equal(labels, torch.as_tensor(z["labels"]))
    model.pctdm.probes = {}
    seen = {}
    h = model.pctdm.register_forward_pre_hook(lambda m, i: seen.__setitem__("x_in", i[0].detach()))
    scores = model((images.to(gpu), boxes.to(gpu)))["activities"]
    h.remove()
    loss = F.cross_entropy(scores, labels.to(gpu))
    loss.backward()
    assert rel(scores, z["activities"]) <= 1e-4
    assert Measured(abs(loss.item() - float(z["loss"]))) <= 1e-4 * max(1.0, abs(float(z["loss"])))
    assert _probe_err(z, "x_in", seen["x_in"]) <= 1e-4
    _check_block(z, model.pctdm.probes, B * T, N)
    named = dict(model.named_parameters())
    assert named["fc_actions.weight"].grad is None and named["fc_actions.bias"].grad is None
    assert _check_grads(z, named) == 26                # fc_emb_1, nl_emb_1, 18 PCTDM tensors, pctdm_nl, fc_activities


# ---- trainer -------------------------------------------------------------------------------------------------------------------------
def _small_cfg(tmp_path):
    from din_amd.config import Config
    cfg = Config("volleyball")
    cfg.backbone, cfg.image_size, cfg.out_size, cfg.emb_features = "vgg16", (64, 96), (2, 3), 512
    cfg.num_boxes, cfg.num_frames, cfg.num_features_boxes = 4, 2, 1024
    cfg.inference_module_name, cfg.training_stage = "pctdm_volleyball", 2
    cfg.batch_size, cfg.test_batch_size, cfg.max_epoch, cfg.test_interval_epoch = 2, 2, 1, 1
    cfg.train_dropout_prob, cfg.train_learning_rate, cfg.lr_plan, cfg.train_backbone = 0.3, 1e-4, {}, True
    if tmp_path is not None:
        cfg.result_path = str(tmp_path)
    return cfg


def test_pctdm_trainer_from_a_stage1_checkpoint(gpu, tmp_path, monkeypatch):
    import din_amd.train_net_dynamic as tnd
    from din_amd.train_net import train_net as train_stage1
    cfg1 = _small_cfg(tmp_path)
    cfg1.training_stage, cfg1.num_frames, cfg1.train_dropout_prob, cfg1.inference_module_name = 1, 1, 0.0, "dynamic_volleyball"
    cfg1.num_features_boxes = 32
    train_stage1(cfg1)
    ck = glob.glob(str(tmp_path / "stage1_epoch1_*.pth"))[0]
    state = torch.load(ck, map_location="cpu")
    cfg = _small_cfg(tmp_path)
    cfg.load_backbone_stage2, cfg.stage1_model_path = True, ck
    seen = {"losses": []}
    real = tnd.train_volleyball

    def first_step(loader, model, *a, **k):
        if "before" not in seen:
            for kk, v in state["backbone_state_dict"].items():
                assert torch.equal(model.backbone.state_dict()[kk].cpu(), v), kk
            seen["before"] = {n: p.detach().clone() for n, p in model.named_parameters()}
            seen["model"] = model
            seen["steps"] = len(loader)
            images, boxes, labels = O.synth_inputs(2, cfg.num_frames, cfg.num_boxes, 64, 96, 2, 3, 8, seed=9)
            seen["probe"] = (images.to(gpu), boxes.to(gpu), labels.to(gpu))
        return real(loader, model, *a, **k)
    monkeypatch.setattr(tnd, "train_volleyball", first_step)
    infos = tnd.train_net(cfg)
    assert len(infos) == 1 and seen["steps"] == 2
    assert np.isfinite(infos[0]["train"]["loss"]) and np.isfinite(infos[0]["test"]["loss"])
    model = seen["model"]
    assert type(model).__name__ == "PCTDM_volleyball"
    assert sum(n.startswith("pctdm.") for n in seen["before"]) == 18
    for n, p in model.named_parameters():
        if n.startswith("fc_actions."):
            assert torch.equal(p.detach(), seen["before"][n]), n + " moved"
        else:
            assert not torch.equal(p.detach(), seen["before"][n]), n + " was not updated"
    ck2 = glob.glob(str(tmp_path / "stage2_epoch1_*.pth"))
    assert len(ck2) == 1
    saved = torch.load(ck2[0], map_location="cpu", weights_only=False)
    assert {"epoch", "state_dict", "optimizer"} <= set(saved.keys())
    assert "fc_actions.weight" in saved["state_dict"] and "pctdm.Bi_Lstm.weight_hh_l0_reverse" in saved["state_dict"]
    again = tnd.build_model(cfg)
    tnd.load_stage2_state(again, ck2[0])
    again = again.to(gpu).eval()
    model.eval()
    images, boxes, _ = seen["probe"]
    with torch.no_grad():
        a = model((images, boxes))["activities"]
        b = again((images, boxes))["activities"]
    assert tuple(a.shape) == (2, 8) and torch.equal(a, b)


def test_pctdm_loss_falls_over_two_optimiser_steps(gpu):
    """two Adam steps on one synthetic batch through the model the trainer builds: the loss is finite and falls"""
    from din_amd.optim import FusedAdam
    from din_amd.train_net_dynamic import build_model
    cfg = _small_cfg(None)
    cfg.train_dropout_prob = 0.0
    torch.manual_seed(3)
    model = build_model(cfg).to(gpu).train()
    opt = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=1e-4, weight_decay=0.0)
    images, boxes, labels = O.synth_inputs(2, cfg.num_frames, cfg.num_boxes, 64, 96, 2, 3, 8, seed=4)
    batch, labels = (images.to(gpu), boxes.to(gpu)), labels.to(gpu)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        loss = F.cross_entropy(model(batch)["activities"], labels)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print("losses", losses)
    assert all(np.isfinite(v) for v in losses) and losses[2] < losses[0]


def test_dropin_launcher_lines_build_the_pctdm_model(gpu, tmp_path, monkeypatch):
    """`dropin/` first on the module path, then the first lines of the reference's scripts/train_volleyball_stage2_pctdm.py (its commented
    vgg16 set-up: the default res18 trunk is not ported) with the small geometry: one epoch trains and tests"""
    monkeypatch.syspath_prepend(os.path.join(ROOT, "dropin"))
    for name in ("train_net_dynamic", "config", "infer_model"):
        sys.modules.pop(name, None)
    ns = {}
    exec("from train_net_dynamic import *\ncfg = Config('volleyball')\ncfg.inference_module_name = 'pctdm_volleyball'\n"
         "cfg.use_multi_gpu = False\ncfg.training_stage = 2\ncfg.train_backbone = True\ncfg.test_before_train = False\n"
         "cfg.backbone = 'vgg16'", ns)
    assert ns["train_net"].__module__ == "din_amd.train_net_dynamic"
    cfg, small = ns["cfg"], _small_cfg(tmp_path)
    assert cfg.num_features_boxes == 1024                               # the launcher's default width is PCTDM's fixed width
    for k in ("image_size", "out_size", "emb_features", "num_boxes", "num_frames", "num_features_boxes", "batch_size", "test_batch_size",
              "max_epoch", "lr_plan", "result_path"):
        setattr(cfg, k, getattr(small, k))
    cfg.data_path = str(tmp_path / "no_such_dataset_tree")
    assert type(ns["build_model"](cfg)).__name__ == "PCTDM_volleyball"
    infos = ns["train_net"](cfg)
    assert len(infos) == 1 and np.isfinite(infos[0]["train"]["loss"])
