"""GPU (-m gpu): the Actor-Transformer baseline.  The position and attention kernels (csrc/actor_attention.hip) against fp64 torch over a
table of shapes, dropout with its keep mask, softmax stability, guard bands, rerun determinism and refusals; AT_volleyball against the
reference's fixtures (tests/golden/at_*.npz, tools/gen_golden_at.py); the entry points of one Actor_Transformer block; the stage-2 trainer
with `inference_module_name = 'at_volleyball'` from a stage-1 checkpoint of this package; the reference launcher's opening lines.

Bars.  Kernel outputs and gradients: max(4 * yard, floor) relative to fp64 torch (max |got - ref| / max |ref|), yard = fp32 torch against
fp64 torch on the same input.  Why 4: two fp32 evaluations of one expression that differ in summation order are each up to one yard from
the fp64 value, so 2 * yard is what the other implementation may legitimately show, and the project's rule that no assert passes under 2x
doubles that.  Floors (for outputs whose yard happens to be tiny): attention 1e-5, the bar of the other fp32 kernel tests here
(a 1024-term fp32 dot product is good to about 1e-6); position 4 * 2^-23 * max|argument| / max|y| -- the argument centre * size / out / dim_t
goes through four fp32 roundings, up to 2 ulp of an argument that reaches 1280 rad (1.5e-4 absolute there), and sin / cos pass an argument
error on unchanged; twice that.  Fixtures: logits 1e-4 (the README's fp32 contract), intermediates and non-backbone gradients
max(5 * yard, 1e-4) with the fixture's own yard, backbone gsum at the model_* fixtures' bars -- all as tests/test_gpu_arg.py."""
import ctypes as C
import glob
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import din_oracle as O
from tests.conftest import Measured

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
AT_CASES = sorted(glob.glob(os.path.join(GOLDEN, "at_*.npz")))
sys.path.insert(0, os.path.join(ROOT, "tools"))

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


# ---- the block in torch (reference AT_infer_module.py:66-96 and :130-138), any dtype, autograd ---------------------------------------------
def dim_t_table(c):
    d = torch.arange(c // 2, dtype=torch.float32)
    return 10000 ** (2 * (d // 2) / (c // 2))


def torch_position(x, boxes, image_size, out_size, pool):
    """x [B,T,N,C], boxes [B,T,N,4] -> x + PE [B,T,N,C] (its mean over T when pool); the fp32 dim_t table is an input of both dtypes"""
    dt = x.dtype
    b = boxes.to(dt)
    cx = (b[..., 0] + b[..., 2]) / 2. * image_size[1] / out_size[1]
    cy = (b[..., 1] + b[..., 3]) / 2. * image_size[0] / out_size[0]
    dim_t = dim_t_table(x.shape[-1]).to(dt)
    px, py = cx[..., None] / dim_t, cy[..., None] / dim_t
    px = torch.stack((px[..., 0::2].sin(), px[..., 1::2].cos()), dim=-1).flatten(-2)
    py = torch.stack((py[..., 0::2].sin(), py[..., 1::2].cos()), dim=-1).flatten(-2)
    y = torch.cat((px, py), dim=-1) + x
    return y.mean(dim=1) if pool else y, float(max(cx.abs().max(), cy.abs().max()))


def torch_attention(q, k, v, x, gamma, beta, keep=None, p=0.0):
    """q, k, v, x [G,N,C], keep bool [G,N,C] | None -> (out [G,N,C], att [G,N,N])"""
    c = q.shape[-1]
    att = torch.softmax(torch.matmul(q, k.transpose(1, 2)) / math.sqrt(c), dim=-1)
    av = torch.matmul(att, v)
    if keep is not None:
        av = av * keep.to(av.dtype) / (1.0 - p)
    return F.layer_norm(x + av, (c,), gamma, beta, 1e-5), att


def _attn_inputs(G, N, C, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    q = scale * torch.randn((G, N, C), generator=g)
    k, v = torch.randn((G, N, C), generator=g), torch.randn((G, N, C), generator=g)
    x = torch.relu(torch.randn((G, N, C), generator=g))                  # shaped like the trunk's output (LayerNorm, ReLU)
    gamma, beta = 1.0 + 0.2 * torch.randn((C,), generator=g), 0.1 * torch.randn((C,), generator=g)
    cot = torch.randn((G, N, C), generator=g)
    return q, k, v, x, gamma, beta, cot


def _run_attention(dev, q, k, v, x, gamma, beta, cot, p=0.0, seed=0, want_keep=False, pad=0):
    """pad > 0: the projection is the first 3*C columns of rows that are `pad` floats wider (NaN there), read through the row stride"""
    from din_amd import ops
    c3 = 3 * q.shape[-1]
    buf = torch.full(q.shape[:2] + (c3 + pad,), float("nan"))
    buf[..., :c3] = torch.cat([q, k, v], -1)
    proj = buf.to(dev)[..., :c3].detach().requires_grad_(True)
    assert proj.stride(1) == c3 + pad
    xs, ga, be = (t.to(dev).requires_grad_(True) for t in (x, gamma, beta))
    res = ops.ActorAttentionFunction.apply(proj, xs, ga, be, p, seed, want_keep)
    res[0].backward(cot.to(dev))
    c = q.shape[-1]
    dp = proj.grad
    return res, [dp[..., :c], dp[..., c:2 * c], dp[..., 2 * c:], xs.grad, ga.grad, be.grad]


def _torch_attention_grads(dtype, q, k, v, x, gamma, beta, cot, keep=None, p=0.0):
    ts = [t.to(dtype).clone().requires_grad_(True) for t in (q, k, v, x, gamma, beta)]
    out, att = torch_attention(*ts, keep=keep, p=p)
    out.backward(cot.to(dtype))
    return out.detach(), att.detach(), [t.grad for t in ts]


ATTN_SHAPES = [(20, 12, 1024, 0), (3, 1, 64, 0), (2, 16, 256, 0), (5, 13, 128, 0), (4, 7, 4, 0), (3, 12, 100, 0), (1, 16, 1028, 0),
               (20, 12, 1024, 64), (3, 13, 100, 8)]
ATTN_IDS = ["launcher_g20_n12_c1024", "one_actor", "n16", "n13", "c4", "c100", "n16_c1028", "launcher_padded_rows", "n13_c100_padded_rows"]
GRAD_NAMES = ("d_q", "d_k", "d_v", "d_x", "d_gamma", "d_beta")


@pytest.mark.parametrize("G,N,C,pad", ATTN_SHAPES, ids=ATTN_IDS)
def test_actor_attention_matches_fp64_torch(gpu, G, N, C, pad):
    a = _attn_inputs(G, N, C, seed=11 + G + N + C)
    (out, att), grads = _run_attention(gpu, *a, pad=pad)
    o64, a64, g64 = _torch_attention_grads(torch.float64, *a)
    o32, a32, g32 = _torch_attention_grads(torch.float32, *a)
    if N > 1:
        assert 1.2 / N < float(a64.max(-1).values.mean()) < 0.95, "the softmax of this case is uniform or one-hot"
    for name, got, ref64, ref32 in [("out", out, o64, o32), ("att", att, a64, a32)] + list(zip(GRAD_NAMES, grads, g64, g32)):
        yard, err = float(rel(ref32, ref64)), rel(got, ref64)
        print(f"{name}: err {float(err):.3e} yard {yard:.3e}")
        assert err <= max(4.0 * yard, 1e-5), (name, float(err), yard)


POS_SHAPES = [(2, 10, 12, 1024, (720, 1280), (22, 40), False), (2, 10, 12, 1024, (720, 1280), (22, 40), True),
              (2, 3, 4, 64, (96, 160), (3, 5), False), (1, 1, 1, 4, (96, 160), (3, 5), True), (3, 2, 13, 100, (139, 203), (15, 23), True)]
POS_IDS = ["launcher", "launcher_pooled", "small", "one_box_c4_pooled", "n13_c100_pooled"]


def _pos_inputs(B, T, N, C, out_size, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn((B, T, N, C), generator=g))
    ctr = torch.rand((B, T, N, 2), generator=g) * torch.tensor([float(out_size[1]), float(out_size[0])])
    wh = 0.5 + torch.rand((B, T, N, 2), generator=g)
    boxes = torch.cat([ctr - wh, ctr + wh], -1)
    cot = torch.randn((B, T, N, C), generator=g)
    return x, boxes, cot


@pytest.mark.parametrize("B,T,N,C,image_size,out_size,pool", POS_SHAPES, ids=POS_IDS)
def test_actor_position_matches_fp64_torch(gpu, B, T, N, C, image_size, out_size, pool):
    from din_amd import ops
    x, boxes, cot = _pos_inputs(B, T, N, C, out_size, seed=3 + T + N + C)
    cot = cot[:, 0].contiguous() if pool else cot
    xs = x.to(gpu).requires_grad_(True)
    keep = boxes.clone()
    y = ops.ActorPositionFunction.apply(xs, boxes.to(gpu), dim_t_table(C).to(gpu), image_size, out_size, pool)
    y.backward(cot.to(gpu))
    assert torch.equal(boxes, keep)
    y64, amax = torch_position(x.double(), boxes, image_size, out_size, pool)
    y32, _ = torch_position(x, boxes, image_size, out_size, pool)
    yard, err = float(rel(y32, y64)), rel(y, y64)
    floor = 4.0 * 2.0 ** -23 * amax / float(y64.abs().max())
    print(f"y: err {float(err):.3e} yard {yard:.3e} floor {floor:.3e} (largest argument {amax:.1f} rad)")
    assert err <= max(4.0 * yard, floor), (float(err), yard, floor)
    x64 = x.double().requires_grad_(True)
    torch_position(x64, boxes, image_size, out_size, pool)[0].backward(cot.double())
    assert rel(xs.grad, x64.grad) <= 1e-6                                # (identity, or one fp32 division by T: 6e-8)


def test_position_backward_entry_point_passes_through_and_broadcasts(gpu):
    from din_amd import _lib
    lib = _lib.load()
    B, T, N, C = 2, 3, 5, 8
    st = C_stream()
    for pool in (0, 1):
        gy = torch.randn((B, N, C) if pool else (B, T, N, C), device=gpu)
        gx = torch.full((B, T, N, C), float("nan"), device=gpu)
        assert lib.din_actor_position_bwd(ptr(gy), B, T, N, C, pool, ptr(gx), st) == 0, lib.din_last_error_string()
        # (the division on the host: torch divides by a scalar on the device by multiplying with its reciprocal, the kernel divides)
        want = (gy.cpu() / T)[:, None].expand(B, T, N, C) if pool else gy.cpu()
        assert torch.equal(gx.cpu(), want.contiguous())


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def C_stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- dropout ----------------------------------------------------------------------------------------------------------------------------
def test_actor_attention_dropout_mask_definition_rerun_and_share(gpu):
    G, N, C, p = 20, 12, 1024, 0.1
    a = _attn_inputs(G, N, C, seed=21)
    (out, att, keep), grads = _run_attention(gpu, *a, p=p, seed=1234, want_keep=True)
    keep_c = keep.cpu()
    o64, a64, g64 = _torch_attention_grads(torch.float64, *a, keep=keep_c, p=p)
    o32, a32, g32 = _torch_attention_grads(torch.float32, *a, keep=keep_c, p=p)
    for name, got, ref64, ref32 in [("out", out, o64, o32), ("att", att, a64, a32)] + list(zip(GRAD_NAMES, grads, g64, g32)):
        yard, err = float(rel(ref32, ref64)), rel(got, ref64)
        print(f"p=0.1 {name}: err {float(err):.3e} yard {yard:.3e}")
        assert err <= max(4.0 * yard, 1e-5), (name, float(err), yard)
    (out2, att2, keep2), grads2 = _run_attention(gpu, *a, p=p, seed=1234, want_keep=True)
    assert torch.equal(out, out2) and torch.equal(att, att2) and torch.equal(keep, keep2)
    for g0, g1 in zip(grads, grads2):
        assert torch.equal(g0, g1)
    (_o3, _a3, keep3), _ = _run_attention(gpu, *a, p=p, seed=1235, want_keep=True)
    assert not torch.equal(keep, keep3)
    # kept share: M = 20 * 12 * 1024 = 245760 independent draws with P(keep) = 0.9: sigma = sqrt(0.1 * 0.9 / M) = 6.05e-4; the bound is 5 sigma
    # (two-sided tail 5.7e-7 per mask; two masks are checked)
    m = G * N * C
    sigma = math.sqrt(p * (1 - p) / m)
    for kk in (keep, keep3):
        share = float(kk.double().mean())
        print(f"kept share {share:.5f} (|share - 0.9| = {abs(share - 0.9) / sigma:.2f} sigma)")
        assert abs(share - (1 - p)) <= 5.0 * sigma
    # the seed_offset word of the captured-graph step: seed s with offset d draws the mask of seed s + d
    from din_amd import ops
    off = torch.tensor([1], dtype=torch.int64, device=gpu)
    old = ops.SEED_OFFSET
    ops.SEED_OFFSET = off
    try:
        (_o4, _a4, keep4), _ = _run_attention(gpu, *a, p=p, seed=1234, want_keep=True)
    finally:
        ops.SEED_OFFSET = old
    assert torch.equal(keep4, keep3)


def test_actor_attention_softmax_subtracts_the_row_maximum(gpu):
    a = _attn_inputs(4, 12, 256, seed=5, scale=1e4)
    q, k = a[0], a[1]
    assert float((q @ k.transpose(1, 2)).abs().max() / 16.0) > 1e4
    (out, att), grads = _run_attention(gpu, *a)
    for t in [out, att] + grads:
        assert bool(torch.isfinite(t).all())
    assert Measured(float((att.sum(-1) - 1).abs().max())) <= 1e-5


def test_actor_attention_same_bits_on_a_rerun(gpu):
    a = _attn_inputs(20, 12, 1024, seed=3)
    runs = [_run_attention(gpu, *a) for _ in range(2)]
    assert torch.equal(runs[0][0][0], runs[1][0][0]) and torch.equal(runs[0][0][1], runs[1][0][1])
    for g0, g1 in zip(runs[0][1], runs[1][1]):
        assert torch.equal(g0, g1)


# ---- the C ABI on NaN-filled buffers ------------------------------------------------------------------------------------------------------
def _banded(dev, n, guard, dtype=torch.float32):
    t = torch.full((n + 2 * guard,), float("nan") if dtype == torch.float32 else 255, dtype=dtype, device=dev)
    return t, t[guard:guard + n]


@pytest.mark.parametrize("G,N,C,pad,p", [(3, 12, 100, 8, 0.0), (2, 16, 256, 0, 0.1), (2, 1, 4, 4, 0.0), (3, 13, 72, 12, 0.1)],
                         ids=["n12_c100_padded_rows", "n16", "one_actor_padded_rows", "n13_padded_rows_dropout"])
def test_actor_kernels_write_inside_their_outputs_only(gpu, G, N, C, pad, p):
    from din_amd import _lib, ops
    lib = _lib.load()
    guard = 64
    q, k, v, x, gamma, beta, cot = _attn_inputs(G, N, C, seed=17)
    ld = 3 * C + pad
    proj = torch.full((G, N, ld), float("nan"))
    proj[..., :3 * C] = torch.cat([q, k, v], -1)
    proj = proj.to(gpu)
    bufs = {kk: _banded(gpu, n, guard, dt) for kk, (n, dt) in dict(
        out=(G * N * C, torch.float32), att=(G * N * N, torch.float32), stats=(G * N * 2, torch.float32), keep=(G * N * C, torch.uint8),
        dproj=(G * N * ld, torch.float32), dx=(G * N * C, torch.float32), dgamma=(C, torch.float32), dbeta=(C, torch.float32)).items()}
    xs, ga, be, co = x.to(gpu), gamma.to(gpu), beta.to(gpu), cot.to(gpu)
    st, base = C_stream(), proj.data_ptr()
    rc = lib.din_actor_attn_fwd(base, base + 4 * C, base + 8 * C, ld, ptr(xs), ptr(ga), ptr(be), 1e-5, p, 77, None, G, N, C,
                                ptr(bufs["out"][1]), ptr(bufs["att"][1]), ptr(bufs["stats"][1]), ptr(bufs["keep"][1]), st)
    assert rc == 0, lib.din_last_error_string()
    nws = ops.actor_attn_workspace_floats(G, C)
    ws = torch.empty(nws, device=gpu)
    gb = bufs["dproj"][1].data_ptr()
    rc = lib.din_actor_attn_bwd(ptr(co), base, base + 4 * C, base + 8 * C, ld, ptr(xs), ptr(ga), ptr(bufs["att"][1]), ptr(bufs["stats"][1]),
                                p, 77, None, G, N, C, gb, gb + 4 * C, gb + 8 * C, ld, ptr(bufs["dx"][1]), ptr(bufs["dgamma"][1]),
                                ptr(bufs["dbeta"][1]), ptr(ws), nws, st)
    assert rc == 0, lib.din_last_error_string()
    torch.cuda.synchronize()
    for kk, (whole, inner) in bufs.items():
        w = whole.cpu()
        if w.dtype == torch.uint8:
            assert bool((w[:guard] == 255).all()) and bool((w[-guard:] == 255).all()), kk
            assert bool((inner.cpu() <= 1).all()), kk
            continue
        assert bool(torch.isnan(w[:guard]).all()) and bool(torch.isnan(w[-guard:]).all()), kk + ": guard band written"
        body = inner.cpu()
        if kk == "dproj":
            body = body.reshape(G, N, ld)
            assert bool(torch.isnan(body[..., 3 * C:]).all()), "padding columns of the gradient rows written"
            body = body[..., :3 * C]
        assert bool(torch.isfinite(body).all()), kk + ": output element not written"
    keep = bufs["keep"][1].reshape(G, N, C).bool().cpu()
    assert bool(keep.all()) == (p == 0.0)
    o64, a64, g64 = _torch_attention_grads(torch.float64, q, k, v, x, gamma, beta, cot, keep=keep, p=p)
    assert rel(bufs["out"][1].reshape(G, N, C), o64) <= 1e-5
    assert rel(bufs["att"][1].reshape(G, N, N), a64) <= 1e-5
    dp = bufs["dproj"][1].reshape(G, N, ld)
    for i, name in enumerate(("d_q", "d_k", "d_v")):
        assert rel(dp[..., i * C:(i + 1) * C], g64[i]) <= 1e-4, name
    assert rel(bufs["dx"][1].reshape(G, N, C), g64[3]) <= 1e-4
    assert rel(bufs["dgamma"][1], g64[4]) <= 1e-4 and rel(bufs["dbeta"][1], g64[5]) <= 1e-4
    # position: both modes between guard bands
    B, T = G, 2
    xp, boxes, _ = _pos_inputs(B, T, N, C, (22, 40), seed=4)
    for pool in (0, 1):
        whole, inner = _banded(gpu, (B * N * C) if pool else (B * T * N * C), guard)
        rc = lib.din_actor_position_fwd(ptr(xp.to(gpu)), ptr(boxes.to(gpu)), ptr(dim_t_table(C).to(gpu)), 1280.0, 720.0, 40.0, 22.0, B, T, N, C,
                                        pool, ptr(inner), st)
        assert rc == 0, lib.din_last_error_string()
        torch.cuda.synchronize()
        w = whole.cpu()
        assert bool(torch.isnan(w[:guard]).all()) and bool(torch.isnan(w[-guard:]).all()) and bool(torch.isfinite(inner).all())


def test_actor_kernels_refuse_unsupported_shapes(gpu):
    from din_amd import _lib, ops
    lib = _lib.load()
    text = open(_lib.HEADER_PATH).read()
    E_ARG = int(text[text.index("DIN_E_ARG ="):].split("=")[1].split(",")[0])
    assert E_ARG == -1
    st = C_stream()
    # (G, N, C, ld offset, byte offset of q, drop_p)
    bad = [(2, 17, 16, 0, 0, 0.0), (2, 4, 18, 0, 0, 0.0), (2, 4, 16, 2, 0, 0.0), (2, 4, 16, 0, 4, 0.0), (2, 4, 16, 0, 0, 1.0), (2, 0, 16, 0, 0, 0.0)]
    for G, N, C_, dld, qoff, p in bad:
        n_ = max(N, 1)
        ld = 3 * C_ + dld
        proj = torch.zeros((G * n_ * ld + 16,), device=gpu)
        x, ga, be = torch.zeros((G, n_, C_), device=gpu), torch.ones((C_,), device=gpu), torch.zeros((C_,), device=gpu)
        out, att, stats = torch.full((G, n_, C_), 7.0, device=gpu), torch.full((G, n_, n_), 7.0, device=gpu), torch.full((G * n_, 2), 7.0, device=gpu)
        keep = torch.full((G, n_, C_), 7, dtype=torch.uint8, device=gpu)
        base = proj.data_ptr() + qoff
        rc = lib.din_actor_attn_fwd(base, base + 4 * C_, base + 8 * C_, ld, ptr(x), ptr(ga), ptr(be), 1e-5, p, 1, None, G, N, C_, ptr(out),
                                    ptr(att), ptr(stats), ptr(keep), st)
        assert rc == E_ARG and lib.din_last_error_string(), (rc, G, N, C_)
        dproj, dx, dga, dbe = torch.full_like(proj, 7.0), torch.full_like(x, 7.0), torch.full_like(ga, 7.0), torch.full_like(be, 7.0)
        nws = ops.actor_attn_workspace_floats(G, C_) + 16
        ws = torch.empty(nws, device=gpu)
        gb = dproj.data_ptr()
        rc = lib.din_actor_attn_bwd(ptr(out), base, base + 4 * C_, base + 8 * C_, ld, ptr(x), ptr(ga), ptr(att), ptr(stats), p, 1, None, G, N, C_,
                                    gb, gb + 4 * C_, gb + 8 * C_, ld, ptr(dx), ptr(dga), ptr(dbe), ptr(ws), nws, st)
        assert rc == E_ARG, (rc, G, N, C_)
        torch.cuda.synchronize()
        for t in (out, att, stats, dproj, dx, dga, dbe):
            assert bool((t == 7.0).all())
        assert bool((keep == 7).all())
    # null pointers, a workspace that is too small, and the position kernel's own refusals
    x, ga = torch.zeros((2, 4, 16), device=gpu), torch.ones((16,), device=gpu)
    proj = torch.zeros((2, 4, 48), device=gpu)
    out, att, stats = torch.full((2, 4, 16), 7.0, device=gpu), torch.full((2, 4, 4), 7.0, device=gpu), torch.full((8, 2), 7.0, device=gpu)
    base = proj.data_ptr()
    assert lib.din_actor_attn_fwd(base, base + 64, base + 128, 48, None, ptr(ga), ptr(ga), 1e-5, 0.0, 1, None, 2, 4, 16, ptr(out), ptr(att),
                                  ptr(stats), None, st) == E_ARG
    dproj, dx, dga, dbe, ws = torch.full_like(proj, 7.0), torch.full_like(x, 7.0), torch.full_like(ga, 7.0), torch.full_like(ga, 7.0), torch.empty(64, device=gpu)
    gb = dproj.data_ptr()
    assert lib.din_actor_attn_bwd(ptr(out), base, base + 64, base + 128, 48, ptr(x), ptr(ga), ptr(att), ptr(stats), 0.0, 1, None, 2, 4, 16, gb,
                                  gb + 64, gb + 128, 48, ptr(dx), ptr(dga), ptr(dbe), ptr(ws), 63, st) == E_ARG
    # a float pointer that is not 4-byte aligned (gamma, two bytes in)
    assert lib.din_actor_attn_fwd(base, base + 64, base + 128, 48, ptr(x), ga.data_ptr() + 2, ptr(ga), 1e-5, 0.0, 1, None, 2, 4, 16, ptr(out),
                                  ptr(att), ptr(stats), None, st) == E_ARG
    assert lib.din_actor_attn_bwd(ptr(out), base, base + 64, base + 128, 48, ptr(x), ptr(ga), ptr(att), ptr(stats), 0.0, 1, None, 2, 4, 16, gb,
                                  gb + 64, gb + 128, 48, ptr(dx), dga.data_ptr() + 2, ptr(dbe), ptr(ws), 64, st) == E_ARG
    y = torch.full((2, 3, 4, 18), 7.0, device=gpu)
    bx = torch.zeros((2, 3, 4, 4), device=gpu)
    assert lib.din_actor_position_fwd(ptr(y), ptr(bx), ptr(ga), 160.0, 96.0, 5.0, 3.0, 2, 3, 4, 18, 0, ptr(y), st) == E_ARG
    assert lib.din_actor_position_fwd(ptr(y), None, ptr(ga), 160.0, 96.0, 5.0, 3.0, 2, 3, 4, 16, 0, ptr(y), st) == E_ARG
    assert lib.din_actor_position_bwd(ptr(y), 2, 3, 4, 18, 0, ptr(y), st) == E_ARG
    torch.cuda.synchronize()
    for t in (out, att, stats, dproj, dx, dga, dbe, y):
        assert bool((t == 7.0).all())
    with pytest.raises(_lib.DinError, match=rf"code {E_ARG}\)"):
        ops.ActorAttentionFunction.apply(torch.zeros((1, 17, 48), device=gpu), torch.zeros((1, 17, 16), device=gpu), ga, ga, 0.0, 0)


# ---- whole models against the reference's fixtures ------------------------------------------------------------------------------------
def _fixture_cfg(z):
    from din_amd.config import Config
    B, T, N, H, W, OH, OW, D, NFB, A = (int(v) for v in z["meta"])
    cfg = Config("volleyball")
    cfg.backbone, cfg.image_size, cfg.out_size, cfg.emb_features = str(z["backbone"]), (H, W), (OH, OW), D
    cfg.num_boxes, cfg.num_frames, cfg.num_features_boxes, cfg.num_activities = N, T, NFB, A
    cfg.temporal_pooled_first, cfg.train_backbone = bool(z["pooled"]), True
    cfg.inference_module_name = "at_volleyball"
    return cfg


def _fixture_model(gpu, path):
    from din_amd.infer_model import AT_volleyball
    from din_amd.train_net_dynamic import set_bn_eval
    from gen_golden_at import at_params, at_shapes
    z = np.load(path)
    B, T, N, H, W, OH, OW, D, NFB, A = (int(v) for v in z["meta"])
    cfg = _fixture_cfg(z)
    model = AT_volleyball(cfg)
    p = at_params(at_shapes(cfg.backbone, D, 5, NFB, A), int(z["seed"]))
    missing, unexpected = model.load_state_dict(p, strict=False)
    assert not unexpected and all("num_batches_tracked" in k for k in missing), (missing, unexpected)
    model = model.to(gpu)
    if str(z["mode"]) == "eval":
        model.eval()
    else:
        model.train()
        model.apply(set_bn_eval)
        for m in (model.AT.dropout1, model.AT.dropout2, model.AT.FFN_dropout):
            m.p = 0.0
    images, boxes, labels = O.synth_inputs(B, T, N, H, W, OH, OW, A, seed=int(z["seed"]))
    assert torch.equal(labels, torch.as_tensor(z["labels"]))
    seen = {}
    hooks = [model.PE.register_forward_hook(lambda m, i, o: seen.update(pe_in=i[0].detach(), pe=o.detach())),
             model.AT.register_forward_hook(lambda m, i, o: seen.__setitem__("at_out", o.detach()))]
    scores = model((images.to(gpu), boxes.to(gpu)))["activities"]
    for h in hooks:
        h.remove()
    loss = F.cross_entropy(scores, labels.to(gpu))
    loss.backward()
    return z, model, scores, loss, seen


@pytest.mark.parametrize("path", AT_CASES, ids=[os.path.basename(p)[:-4] for p in AT_CASES])
def test_at_volleyball_matches_reference_golden(gpu, path):
    z, model, scores, loss, seen = _fixture_model(gpu, path)
    assert rel(scores, z["activities"]) <= 1e-4
    assert Measured(abs(loss.item() - float(z["loss"]))) <= 1e-4 * max(1.0, abs(float(z["loss"])))
    assert rel(seen["pe_in"], z["pe_in64"]) <= 1e-4
    pe64 = torch.as_tensor(z["pe64"])
    assert rel(seen["pe"], pe64.mean(1) if bool(z["pooled"]) else pe64) <= max(5.0 * float(z["yard_pe"]), 1e-4)
    assert rel(model.AT.attention, z["att64"]) <= max(5.0 * float(z["yard_att"]), 1e-4)
    assert rel(seen["at_out"], z["at_out64"]) <= max(5.0 * float(z["yard_at_out"]), 1e-4)
    named = dict(model.named_parameters())
    assert named["fc_actions.weight"].grad is None and named["fc_actions.bias"].grad is None
    checked = 0
    for k in z.files:
        if k.startswith("g64."):
            name = k[4:]
            got = named[name].grad.detach().flatten().double().cpu()
            if "gidx." + name in z.files:
                got = got[torch.as_tensor(z["gidx." + name])]
            err = Measured(float((got - torch.as_tensor(z[k])).abs().max()) / float(z["gmax64." + name]))
            assert err <= max(5.0 * float(z["yard." + name]), 1e-4), name
            checked += 1
        if k.startswith("gsum.") and not k.startswith("gsum64."):
            name = k[5:]
            gs_tol = 6e-3 if name.startswith("backbone.") else 2e-3       # the model_* fixtures' bars
            assert Measured(abs(named[name].grad.double().sum().item() - float(z[k]))) <= gs_tol * float(z["gabs." + name]) + 1e-6, name
    assert checked == 17                                                  # fc_emb_1, nl_emb_1, 11 AT tensors, fc_activities


def test_at_fixtures_exist():
    assert len(AT_CASES) == 4, AT_CASES


# ---- one Actor_Transformer block: entry points ------------------------------------------------------------------------------------------
def _small_cfg(tmp_path):
    from din_amd.config import Config
    cfg = Config("volleyball")
    cfg.backbone, cfg.image_size, cfg.out_size, cfg.emb_features = "vgg16", (64, 96), (2, 3), 512
    cfg.num_boxes, cfg.num_frames, cfg.num_features_boxes = 4, 2, 32
    cfg.inference_module_name, cfg.training_stage = "at_volleyball", 2
    cfg.batch_size, cfg.test_batch_size, cfg.max_epoch, cfg.test_interval_epoch = 2, 2, 1, 1
    cfg.train_dropout_prob, cfg.train_learning_rate, cfg.lr_plan, cfg.train_backbone = 0.3, 1e-3, {}, True
    if tmp_path is not None:
        cfg.result_path = str(tmp_path)
    return cfg


def test_at_block_entry_points_of_one_training_step(gpu, monkeypatch):
    """forward + backward of Actor_Transformer in train mode (p = 0.1): three contractions (Q/K/V as one, FFN_linear1, FFN_linear2), each
    with its weight packing, weight gradient and data gradient; one attention launch set forward and one backward (din_actor_attn_bwd
    holds the attention backward and the fixed-order reduce of d gamma / d beta); two dropout calls each way; one LayerNorm each way.  No
    torch matmul / softmax / layer_norm / dropout runs."""
    from din_amd import _lib
    from din_amd.infer_module.AT_infer_module import Actor_Transformer
    lib = _lib.load()
    calls = {}
    for name in _lib.SIGNATURES:
        fn = getattr(lib, name)

        def counting(*a, _fn=fn, _name=name):
            calls[_name] = calls.get(_name, 0) + 1
            return _fn(*a)
        monkeypatch.setattr(lib, name, counting)

    def forbidden(*a, **k):
        raise AssertionError("a torch matmul / softmax / layer_norm / dropout ran on the AT block's path")
    for mod, name in [(torch, "matmul"), (torch, "bmm"), (torch, "softmax"), (torch, "layer_norm"), (F, "softmax"), (F, "layer_norm"),
                      (F, "linear"), (F, "dropout"), (torch, "dropout"), (torch.Tensor, "matmul"), (torch.Tensor, "softmax")]:
        monkeypatch.setattr(mod, name, forbidden)
    at = Actor_Transformer(32, False).to(gpu).train()
    x = torch.randn((2, 3, 12, 32), generator=torch.Generator().manual_seed(1)).to(gpu).requires_grad_(True)
    out = at(x, seeds=(5, 6, 7))
    out.sum().backward()
    torch.cuda.synchronize()
    launches = {k: v for k, v in calls.items() if k not in ("din_conv_packed_elems", "din_conv_workspace_bytes", "din_last_error_string",
                                                            "din_get_option", "din_conv_kernel_tile", "din_conv_kernel_variant")}
    assert launches == {"din_conv_pack_weights": 6, "din_conv_fwd": 3, "din_conv_wgrad": 3, "din_conv_dgrad": 3, "din_actor_attn_fwd": 1,
                        "din_actor_attn_bwd": 1, "din_act_dropout_fwd": 2, "din_act_dropout_bwd": 2, "din_layernorm_fwd": 1,
                        "din_layernorm_bwd": 1}, launches
    assert tuple(out.shape) == (6, 12, 32) and tuple(at.attention.shape) == (6, 12, 12)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in at.parameters())
    assert [n for n, _ in at.named_parameters()] == ["Q_W.weight", "K_W.weight", "V_W.weight", "layernorm1.weight", "layernorm1.bias",
                                                     "FFN_linear1.weight", "FFN_linear1.bias", "FFN_linear2.weight", "FFN_linear2.bias",
                                                     "layernorm2.weight", "layernorm2.bias"]


def test_at_model_draws_three_distinct_mask_seeds_per_step(gpu):
    from din_amd.infer_model import AT_volleyball
    cfg = _small_cfg(None)
    model = AT_volleyball(cfg).to(gpu).train()
    images, boxes, _ = O.synth_inputs(2, cfg.num_frames, cfg.num_boxes, 64, 96, 2, 3, 8, seed=1)
    drawn = []
    model.AT.register_forward_pre_hook(lambda m, args, kwargs: drawn.extend(kwargs["seeds"]), with_kwargs=True)
    model((images.to(gpu), boxes.to(gpu)))
    model((images.to(gpu), boxes.to(gpu)))
    assert len(drawn) == 6 and len(set(drawn)) == 6 and model._step == 6


# ---- trainer -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pooled", [False, True], ids=["per_frame", "pooled_first"])
def test_at_trainer_from_a_stage1_checkpoint(gpu, tmp_path, monkeypatch, pooled):
    import din_amd.train_net_dynamic as tnd
    from din_amd.train_net import train_net as train_stage1
    cfg1 = _small_cfg(tmp_path)
    cfg1.training_stage, cfg1.num_frames, cfg1.train_dropout_prob, cfg1.inference_module_name = 1, 1, 0.0, "dynamic_volleyball"
    train_stage1(cfg1)
    ck = glob.glob(str(tmp_path / "stage1_epoch1_*.pth"))[0]
    state = torch.load(ck, map_location="cpu")
    cfg = _small_cfg(tmp_path)
    cfg.load_backbone_stage2, cfg.stage1_model_path, cfg.temporal_pooled_first = True, ck, pooled
    seen = {}
    real = tnd.train_volleyball

    def first_step(loader, model, *a, **k):
        if "before" not in seen:
            for kk, v in state["backbone_state_dict"].items():
                assert torch.equal(model.backbone.state_dict()[kk].cpu(), v), kk
            seen["before"] = {n: p.detach().clone() for n, p in model.named_parameters()}
            seen["model"] = model
            seen["steps"] = len(loader)
        return real(loader, model, *a, **k)
    monkeypatch.setattr(tnd, "train_volleyball", first_step)
    infos = tnd.train_net(cfg)
    assert len(infos) == 1 and seen["steps"] == 2
    assert np.isfinite(infos[0]["train"]["loss"]) and np.isfinite(infos[0]["test"]["loss"])
    model = seen["model"]
    assert type(model).__name__ == "AT_volleyball"
    assert sum(n.startswith("AT.") for n in seen["before"]) == 11
    for n, p in model.named_parameters():
        if n.startswith("fc_actions."):
            assert torch.equal(p.detach(), seen["before"][n]), n + " moved"
        else:
            assert not torch.equal(p.detach(), seen["before"][n]), n + " was not updated"
    ck2 = glob.glob(str(tmp_path / "stage2_epoch1_*.pth"))
    assert len(ck2) == 1
    saved = torch.load(ck2[0], map_location="cpu", weights_only=False)
    assert {"epoch", "state_dict", "optimizer"} <= set(saved.keys())
    assert "fc_actions.weight" in saved["state_dict"] and "AT.Q_W.weight" in saved["state_dict"]
    again = tnd.build_model(cfg)
    tnd.load_stage2_state(again, ck2[0])
    again = again.to(gpu).eval()
    model.eval()
    images, boxes, _ = O.synth_inputs(2, cfg.num_frames, cfg.num_boxes, 64, 96, 2, 3, 8, seed=9)
    with torch.no_grad():
        a = model((images.to(gpu), boxes.to(gpu)))["activities"]
        b = again((images.to(gpu), boxes.to(gpu)))["activities"]
    assert tuple(a.shape) == (2, 8) and torch.equal(a, b)


def test_dropin_launcher_lines_build_the_at_model(gpu, tmp_path, monkeypatch):
    """`dropin/` first on the module path, then the first lines of the reference's scripts/train_volleyball_stage2_at.py (its vgg16 set-up)
    with the small geometry: one epoch trains and tests"""
    monkeypatch.syspath_prepend(os.path.join(ROOT, "dropin"))
    for name in ("train_net_dynamic", "config", "infer_model"):
        sys.modules.pop(name, None)
    ns = {}
    exec("from train_net_dynamic import *\ncfg = Config('volleyball')\ncfg.inference_module_name = 'at_volleyball'\n"
         "cfg.use_multi_gpu = False\ncfg.training_stage = 2\ncfg.train_backbone = True\ncfg.test_before_train = False\n"
         "cfg.backbone = 'vgg16'\ncfg.temporal_pooled_first = False", ns)
    assert ns["train_net"].__module__ == "din_amd.train_net_dynamic"
    cfg, small = ns["cfg"], _small_cfg(tmp_path)
    for k in ("image_size", "out_size", "emb_features", "num_boxes", "num_frames", "num_features_boxes", "batch_size", "test_batch_size",
              "max_epoch", "lr_plan", "result_path"):
        setattr(cfg, k, getattr(small, k))
    cfg.data_path = str(tmp_path / "no_such_dataset_tree")
    assert type(ns["build_model"](cfg)).__name__ == "AT_volleyball"
    infos = ns["train_net"](cfg)
    assert len(infos) == 1 and np.isfinite(infos[0]["train"]["loss"])
