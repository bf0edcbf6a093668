"""GPU (-m gpu): the ARG baseline.  The relation-graph kernels (csrc/arg_graph.hip) against fp64 torch over a table of shapes, guard bands,
rerun determinism and refusals; ARG_volleyball against the reference's fixtures (tests/golden/arg_*.npz, tools/gen_golden_arg.py); the
entry points of one GCN block; the stage-2 trainer with `inference_module_name = 'arg_volleyball'`, from a stage-1 checkpoint of this
package, and its checkpoint round trip.

Bars: kernel outputs and gradients max(3 * yard, 1e-5) relative to fp64 torch, yard = fp32 torch against fp64 torch on the same input;
fixture logits 1e-4, non-backbone gradients max(5 * yard, 1e-4) with the fixture's own yard, backbone gsum at the model_* fixtures' bars."""
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
ARG_CASES = sorted(glob.glob(os.path.join(GOLDEN, "arg_*.npz")))
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


# ---- the block in torch (reference ARG_infer_module.py:46-89 after its Linear layers), any dtype, autograd ---------------------------------
def torch_graph(theta, phi, y, mask, gamma, beta):
    """theta, phi [B,TN,NG,NFR], y [B,TN,NG,NFG], mask bool [B,TN,TN], gamma / beta [NG,TN,NFG] -> (out [B,TN,NFG], R [B,NG,TN,TN])"""
    nfr, ng = theta.shape[-1], theta.shape[2]
    outs, rels = [], []
    for g in range(ng):
        s = torch.matmul(theta[:, :, g], phi[:, :, g].transpose(1, 2)) / math.sqrt(nfr)
        s = s.masked_fill(mask, -float("inf"))
        r = torch.softmax(s, dim=2)
        z = torch.matmul(r, y[:, :, g])
        outs.append(torch.relu(F.layer_norm(z, z.shape[1:], gamma[g], beta[g], 1e-5)))
        rels.append(r)
    return torch.stack(outs).sum(0), torch.stack(rels, 1)


def _centres_mask(boxes, thr, rounds=1):
    b = boxes.double().clone()
    for _ in range(rounds):
        b[..., 0] = (b[..., 0] + b[..., 2]) / 2
        b[..., 1] = (b[..., 1] + b[..., 3]) / 2
    d = (b[:, :, None, :2] - b[:, None, :, :2]).pow(2).sum(-1).sqrt()
    return d > thr, d


def _inputs(B, TN, NG, NFR, NFG, kind, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    theta = scale * torch.randn((B, TN, NG, NFR), generator=g)
    phi = torch.randn((B, TN, NG, NFR), generator=g)
    y = torch.randn((B, TN, NG, NFG), generator=g)
    gamma = 1.0 + 0.2 * torch.randn((NG, TN, NFG), generator=g)
    beta = 0.1 * torch.randn((NG, TN, NFG), generator=g)
    c = torch.rand((B, TN, 2), generator=g) * torch.tensor([40.0, 22.0])
    wh = 0.5 + torch.rand((B, TN, 2), generator=g)
    boxes = torch.cat([c - wh, c + wh], -1)
    _, d = _centres_mask(boxes, 0.0)
    if kind == "all" or TN == 1:
        thr = 1e6
    elif kind == "diag":
        thr = 0.0
    else:                                            # mixed: the threshold sits in the middle of the widest gap near the median distance
        v = d[d > 0].flatten().sort().values
        lo, hi = int(0.3 * len(v)), max(int(0.7 * len(v)), int(0.3 * len(v)) + 2)
        k = lo + int((v[lo + 1:hi] - v[lo:hi - 1]).argmax())
        thr = float((v[k] + v[k + 1]) / 2)
    mask, _ = _centres_mask(boxes, thr)
    cot = torch.randn((B, TN, NFG), generator=g)
    return theta, phi, y, gamma, beta, boxes, float(thr), mask, cot


def _proj(theta, phi, y):
    B, TN = theta.shape[:2]
    return torch.cat([theta.reshape(B, TN, -1), phi.reshape(B, TN, -1), y.reshape(B, TN, -1)], -1).contiguous()


def _run_kernel(dev, theta, phi, y, gamma, beta, boxes, thr, cot, rounds=1):
    from din_amd import ops
    NG, NFR, NFG = theta.shape[2], theta.shape[3], y.shape[3]
    proj = _proj(theta, phi, y).to(dev).requires_grad_(True)
    ga, be = gamma.to(dev).requires_grad_(True), beta.to(dev).requires_grad_(True)
    out, r, mask = ops.ArgGraphFunction.apply(proj, boxes.to(dev), ga, be, NG, NFR, NFG, thr, rounds)
    out.backward(cot.to(dev))
    B, TN = theta.shape[:2]
    dp = proj.grad
    dth, dph, dy = dp[..., :NG * NFR], dp[..., NG * NFR:2 * NG * NFR], dp[..., 2 * NG * NFR:]
    return out, r, mask, [dth.reshape(B, TN, NG, NFR), dph.reshape(B, TN, NG, NFR), dy.reshape(B, TN, NG, NFG), ga.grad, be.grad]


def _torch_grads(dtype, theta, phi, y, gamma, beta, mask, cot):
    ts = [t.to(dtype).clone().requires_grad_(True) for t in (theta, phi, y, gamma, beta)]
    out, r = torch_graph(*ts[:3], mask, *ts[3:])
    out.backward(cot.to(dtype))
    return out.detach(), r.detach(), [t.grad for t in ts]


GRAPH_SHAPES = [(2, 36, 16, 256, 1024, "mixed"), (1, 1, 1, 4, 4, "all"), (2, 12, 1, 36, 100, "mixed"), (1, 120, 2, 20, 72, "mixed"),
                (3, 36, 16, 12, 40, "diag"), (2, 12, 4, 36, 100, "all"), (1, 120, 1, 256, 1024, "mixed")]
GRAPH_IDS = ["launcher_tn36_ng16", "one_actor", "tn12_odd_widths", "tn120_odd_widths", "diag_only_ng16", "all_kept", "tn120_wide"]


@pytest.mark.parametrize("B,TN,NG,NFR,NFG,kind", GRAPH_SHAPES, ids=GRAPH_IDS)
def test_arg_graph_matches_fp64_torch(gpu, B, TN, NG, NFR, NFG, kind):
    theta, phi, y, gamma, beta, boxes, thr, mask, cot = _inputs(B, TN, NG, NFR, NFG, kind, seed=7 + TN + NG + NFG)
    if kind == "mixed":
        assert 0.1 < float(mask.double().mean()) < 0.9
    if kind == "diag" and TN > 1:
        assert bool((mask == ~torch.eye(TN, dtype=torch.bool)[None]).all())
    out, r, m, grads = _run_kernel(gpu, theta, phi, y, gamma, beta, boxes, thr, cot)
    o64, r64, g64 = _torch_grads(torch.float64, theta, phi, y, gamma, beta, mask, cot)
    o32, r32, g32 = _torch_grads(torch.float32, theta, phi, y, gamma, beta, mask, cot)
    assert torch.equal(m.cpu(), mask), "position mask differs"
    assert bool((r.cpu()[mask[:, None].expand_as(r)] == 0).all())
    for name, got, ref64, ref32 in [("out", out, o64, o32), ("R", r, r64, r32)] + \
            [(n, a, b, c) for n, a, b, c in zip(("d_theta", "d_phi", "d_Y", "d_gamma", "d_beta"), grads, g64, g32)]:
        yard = float(rel(ref32, ref64))
        err = rel(got, ref64)
        print(f"{name}: err {float(err):.3e} yard {yard:.3e}")
        assert err <= max(3.0 * yard, 1e-5), (name, float(err), yard)


def test_arg_graph_second_layer_sees_twice_averaged_corners(gpu):
    theta, phi, y, gamma, beta, boxes, _thr, _mask, cot = _inputs(2, 12, 2, 16, 32, "mixed", seed=31)
    m2, d2 = _centres_mask(boxes, 0.0, rounds=2)
    thr = float(d2[d2 > 0].median())
    want2, want1 = _centres_mask(boxes, thr, rounds=2)[0], _centres_mask(boxes, thr, rounds=1)[0]
    assert not torch.equal(want1, want2)
    keep = boxes.clone()
    _o, _r, m, _g = _run_kernel(gpu, theta, phi, y, gamma, beta, boxes, thr, cot, rounds=2)
    near = ((d2 - thr).abs() / thr < 1e-5)
    assert bool(((m.cpu() == want2) | near).all())
    assert torch.equal(boxes, keep)


def test_arg_graph_softmax_subtracts_the_row_maximum(gpu):
    theta, phi, y, gamma, beta, boxes, thr, mask, cot = _inputs(2, 36, 4, 64, 128, "mixed", seed=5, scale=1e4)
    out, r, _m, grads = _run_kernel(gpu, theta, phi, y, gamma, beta, boxes, thr, cot)
    assert float((theta[:, :, 0] @ phi[:, :, 0].transpose(1, 2)).abs().max() / 8.0) > 1e4
    for t in [out, r] + grads:
        assert bool(torch.isfinite(t).all())
    assert Measured(float((r.sum(-1) - 1).abs().max())) <= 1e-5


def test_arg_graph_same_bits_on_a_rerun(gpu):
    a = _inputs(2, 36, 16, 64, 256, "mixed", seed=3)
    runs = [_run_kernel(gpu, *a[:7], a[8]) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    for g0, g1 in zip(runs[0][3], runs[1][3]):
        assert torch.equal(g0, g1)


def _raw(dev, B, TN, NG, NFR, NFG, seed, pad_cols=0, guard=64):
    """both entry points through the C ABI on NaN-filled buffers: outputs sit between guard bands, the projection rows carry pad_cols
    NaN columns that belong to nobody"""
    from din_amd import _lib, ops
    lib = _lib.load()
    theta, phi, y, gamma, beta, boxes, thr, mask, cot = _inputs(B, TN, NG, NFR, NFG, "mixed", seed)
    ld = NG * (2 * NFR + NFG) + pad_cols
    proj = torch.full((B, TN, ld), float("nan"))
    proj[..., :ld - pad_cols] = _proj(theta, phi, y)
    proj = proj.to(dev)

    def banded(n, dtype=torch.float32):
        t = torch.full((n + 2 * guard,), float("nan") if dtype == torch.float32 else 255, dtype=dtype, device=dev)
        return t, t[guard:guard + n]
    bufs = {k: banded(n, dt) for k, (n, dt) in dict(
        out=(B * TN * NFG, torch.float32), rel=(B * NG * TN * TN, torch.float32), mask=(B * TN * TN, torch.uint8),
        z=(B * NG * TN * NFG, torch.float32), stats=(B * NG * 2, torch.float32), dproj=(B * TN * ld, torch.float32),
        dgamma=(NG * TN * NFG, torch.float32), dbeta=(NG * TN * NFG, torch.float32)).items()}
    ptr = lambda t: C.c_void_p(t.data_ptr())                                     # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ga, be, bx, co = gamma.to(dev), beta.to(dev), boxes.to(dev), cot.to(dev)
    nws = ops.arg_graph_workspace_floats(B, TN, NG, NFG, False)
    ws = torch.empty(nws, device=dev)
    base = proj.data_ptr()
    rc = lib.din_arg_graph_fwd(base, base + 4 * NG * NFR, base + 8 * NG * NFR, ld, ptr(bx), 1, thr, ptr(ga), ptr(be), 1e-5, B, TN, NG, NFR, NFG,
                               ptr(bufs["out"][1]), ptr(bufs["rel"][1]), ptr(bufs["mask"][1]), ptr(bufs["z"][1]), ptr(bufs["stats"][1]),
                               ptr(ws), nws, st)
    assert rc == 0, _lib.load().din_last_error_string()
    nwb = ops.arg_graph_workspace_floats(B, TN, NG, NFG, True)
    wsb = torch.empty(nwb, device=dev)
    gb = bufs["dproj"][1].data_ptr()
    rc = lib.din_arg_graph_bwd(ptr(co), base, base + 4 * NG * NFR, base + 8 * NG * NFR, ld, ptr(ga), ptr(be), ptr(bufs["rel"][1]),
                               ptr(bufs["z"][1]), ptr(bufs["stats"][1]), B, TN, NG, NFR, NFG, gb, gb + 4 * NG * NFR, gb + 8 * NG * NFR, ld,
                               ptr(bufs["dgamma"][1]), ptr(bufs["dbeta"][1]), ptr(wsb), nwb, st)
    assert rc == 0, _lib.load().din_last_error_string()
    torch.cuda.synchronize()
    return bufs, (theta, phi, y, gamma, beta, mask, cot), ld


@pytest.mark.parametrize("B,TN,NG,NFR,NFG,pad", [(2, 36, 3, 20, 72, 8), (1, 120, 2, 12, 100, 0), (2, 1, 1, 4, 4, 4)],
                         ids=["tn36_padded_rows", "tn120", "one_actor_padded_rows"])
def test_arg_graph_writes_inside_its_outputs_only(gpu, B, TN, NG, NFR, NFG, pad):
    guard = 64
    bufs, (theta, phi, y, gamma, beta, mask, cot), ld = _raw(gpu, B, TN, NG, NFR, NFG, seed=17, pad_cols=pad, guard=guard)
    for k, (whole, inner) in bufs.items():
        w = whole.cpu()
        if w.dtype == torch.uint8:
            assert bool((w[:guard] == 255).all()) and bool((w[-guard:] == 255).all()), k
            assert bool((inner.cpu() <= 1).all()), k
        else:
            assert bool(torch.isnan(w[:guard]).all()) and bool(torch.isnan(w[-guard:]).all()), k + ": guard band written"
            body = inner.cpu()
            if k == "dproj":
                body = body.reshape(B, TN, ld)
                assert bool(torch.isnan(body[..., ld - pad:]).all()), "padding columns of the gradient rows written"
                body = body[..., :ld - pad]
            assert bool(torch.isfinite(body).all()), k + ": output element not written"
    o64, _r64, g64 = _torch_grads(torch.float64, theta, phi, y, gamma, beta, mask, cot)
    assert rel(bufs["out"][1].reshape(B, TN, NFG), o64) <= 1e-5
    dp = bufs["dproj"][1].reshape(B, TN, ld)
    assert rel(dp[..., 2 * NG * NFR:ld - pad].reshape(B, TN, NG, NFG), g64[2]) <= 1e-4


def exact_threshold_case():
    """four actors with centres (0,0), (3,4), (3, 4 + 2^-10), (3, 4 - 2^-10) and thr = 5: the distance 0 -> 1 is EXACTLY 5 in fp32 and fp64
    (9 + 16 = 25, an exact square root), 0 -> 2 is just above (5.0008), 0 -> 3 just below.  `>` keeps 0 <-> 1, `>=` would mask it."""
    e = 2.0 ** -10
    c = torch.tensor([[0.0, 0.0], [3.0, 4.0], [3.0, 4.0 + e], [3.0, 4.0 - e]])
    boxes = torch.cat([c - 1.0, c + 1.0], -1)[None]                       # (x1, y1, x2, y2): the centres are exact in fp32
    return boxes, 5.0


def test_arg_graph_comparison_with_the_threshold_is_strict(gpu):
    boxes, thr = exact_threshold_case()
    theta, phi, y, gamma, beta, _b, _t, _m, cot = _inputs(1, 4, 3, 8, 16, "all", seed=41)
    mask, d = _centres_mask(boxes, thr)
    assert float(d[0, 0, 1]) == 5.0 and not bool(mask[0, 0, 1]) and bool(mask[0, 0, 2]) and not bool(mask[0, 0, 3])
    wrong = d >= thr
    wrong[0].fill_diagonal_(False)                                         # (even with the diagonal exempted, as the kernel exempts it)
    assert not torch.equal(wrong, mask) and bool(wrong[0, 0, 1]) and bool(wrong[0, 1, 0])
    out, r, m, grads = _run_kernel(gpu, theta, phi, y, gamma, beta, boxes, thr, cot)
    assert torch.equal(m.cpu(), mask), "an actor at exactly the threshold distance must be kept (strict >)"
    assert float(r[0, :, 0, 1].min()) > 0.0 and float(r[0, :, 0, 2].max()) == 0.0
    o64, r64, g64 = _torch_grads(torch.float64, theta, phi, y, gamma, beta, mask, cot)
    o32, r32, _g32 = _torch_grads(torch.float32, theta, phi, y, gamma, beta, mask, cot)
    w64, wr64, _ = _torch_grads(torch.float64, theta, phi, y, gamma, beta, wrong, cot)
    assert rel(out, o64) <= max(3.0 * float(rel(o32, o64)), 1e-5) and rel(r, r64) <= max(3.0 * float(rel(r32, r64)), 1e-5)
    assert float(rel(w64, o64)) >= 1e-3 and float(rel(wr64, r64)) >= 1e-3, "the case cannot tell >= from >"


def test_arg_graph_refuses_unsupported_shapes(gpu):
    from din_amd import _lib, ops
    lib = _lib.load()
    text = open(_lib.HEADER_PATH).read()
    E_ARG = int(text[text.index("DIN_E_ARG ="):].split("=")[1].split(",")[0])
    assert E_ARG == -1
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())                                     # noqa: E731
    for B, TN, NG, NFR, NFG in [(1, 121, 1, 8, 16), (1, 12, 2, 8, 18), (1, 12, 2, 6, 16), (1, 12, 1025, 4, 4)]:
        ld = NG * (2 * NFR + NFG)
        proj = torch.zeros((B, TN, ld), device=gpu)
        boxes, ga, be = torch.zeros((B, TN, 4), device=gpu), torch.ones((NG, TN, NFG), device=gpu), torch.zeros((NG, TN, NFG), device=gpu)
        with pytest.raises(_lib.DinError, match=rf"code {E_ARG}\)"):
            ops.ArgGraphFunction.apply(proj, boxes, ga, be, NG, NFR, NFG, 1.0, 1)
        # the C ABI with VALID buffers of that shape: the shape check refuses, and no output is touched
        out = torch.full((B, TN, NFG), 7.0, device=gpu)
        relb, msk = torch.full((B, NG, TN, TN), 7.0, device=gpu), torch.full((B, TN, TN), 7, dtype=torch.uint8, device=gpu)
        z, stats = torch.full((B, NG, TN, NFG), 7.0, device=gpu), torch.full((B, NG, 2), 7.0, device=gpu)
        nws = ops.arg_graph_workspace_floats(B, TN, NG, NFG, False) + 16
        ws = torch.empty(nws, device=gpu)
        base = proj.data_ptr()
        rc = lib.din_arg_graph_fwd(base, base + 4 * NG * NFR, base + 8 * NG * NFR, ld, ptr(boxes), 1, 1.0, ptr(ga), ptr(be), 1e-5, B, TN, NG,
                                   NFR, NFG, ptr(out), ptr(relb), ptr(msk), ptr(z), ptr(stats), ptr(ws), nws, st)
        assert rc == E_ARG, (rc, lib.din_last_error_string())
        nwb = ops.arg_graph_workspace_floats(B, TN, NG, NFG, True) + 16
        wsb = torch.empty(nwb, device=gpu)
        dproj, dga, dbe = torch.full_like(proj, 7.0), torch.full_like(ga, 7.0), torch.full_like(be, 7.0)
        gb = dproj.data_ptr()
        rc = lib.din_arg_graph_bwd(ptr(out), base, base + 4 * NG * NFR, base + 8 * NG * NFR, ld, ptr(ga), ptr(be), ptr(relb), ptr(z), ptr(stats),
                                   B, TN, NG, NFR, NFG, gb, gb + 4 * NG * NFR, gb + 8 * NG * NFR, ld, ptr(dga), ptr(dbe), ptr(wsb), nwb, st)
        assert rc == E_ARG, (rc, lib.din_last_error_string())
        torch.cuda.synchronize()
        for t in (out, relb, z, stats, dproj, dga, dbe):
            assert bool((t == 7.0).all())
        assert bool((msk == 7).all())
    # a workspace that is too small, and a negative threshold, are refused the same way
    theta, phi, y, gamma, beta, boxes, thr, _mask, _cot = _inputs(1, 12, 2, 8, 16, "all", seed=2)
    with pytest.raises(_lib.DinError, match=rf"code {E_ARG}\)"):
        ops.ArgGraphFunction.apply(_proj(theta, phi, y).to(gpu), boxes.to(gpu), gamma.to(gpu), beta.to(gpu), 2, 8, 16, -1.0, 1)


# ---- whole models against the reference's fixtures ------------------------------------------------------------------------------------
def _fixture_model(gpu, path):
    from din_amd.config import Config
    from din_amd.infer_model import ARG_volleyball
    from din_amd.train_net_dynamic import set_bn_eval
    from gen_golden_arg import arg_params, arg_shapes
    z = np.load(path)
    B, T, N, H, W, OH, OW, D, NFB, NFR, NG, layers, A = (int(v) for v in z["meta"])
    backbone, mode, seed = str(z["backbone"]), str(z["mode"]), int(z["seed"])
    cfg = Config("volleyball")
    cfg.backbone, cfg.image_size, cfg.out_size, cfg.emb_features = backbone, (H, W), (OH, OW), D
    cfg.num_boxes, cfg.num_frames, cfg.num_features_boxes, cfg.num_features_gcn, cfg.num_activities = N, T, NFB, NFB, A
    cfg.num_features_relation, cfg.num_graph, cfg.gcn_layers, cfg.pos_threshold = NFR, NG, layers, float(z["pos_threshold"])
    cfg.train_backbone, cfg.train_dropout_prob = True, 0.0
    model = ARG_volleyball(cfg)
    p = arg_params(arg_shapes(backbone, D, 5, T, N, NFB, NFR, NG, layers, A), seed)
    missing, unexpected = model.load_state_dict(p, strict=False)
    assert not unexpected and all("num_batches_tracked" in k for k in missing), (missing, unexpected)
    model = model.to(gpu)
    if mode == "eval":
        model.eval()
    else:
        model.train()
        model.apply(set_bn_eval)
    images, boxes, labels = O.synth_inputs(B, T * 3 if mode == "eval" else T, N, H, W, OH, OW, A, seed=seed)
    assert torch.equal(labels, torch.as_tensor(z["labels"]))
    boxes_dev = boxes.to(gpu)
    seen = []
    hook = model.gcn_list[-1].register_forward_hook(lambda m, i, o: seen.append((o[0].detach(), o[1].detach())))
    scores = model((images.to(gpu), boxes_dev))["activities"]
    hook.remove()
    model.graph_features, model.relation_graph = seen[0]
    assert torch.equal(boxes_dev.cpu(), boxes), "the caller's boxes were written"
    loss = F.cross_entropy(scores, labels.to(gpu))
    loss.backward()
    return z, model, scores, loss


@pytest.mark.parametrize("path", ARG_CASES, ids=[os.path.basename(p)[:-4] for p in ARG_CASES])
def test_arg_volleyball_matches_reference_golden(gpu, path):
    z, model, scores, loss = _fixture_model(gpu, path)
    assert rel(scores, z["activities"]) <= 1e-4
    assert Measured(abs(loss.item() - float(z["loss"]))) <= 1e-4 * max(1.0, abs(float(z["loss"])))
    layers = int(z["meta"][11])
    assert torch.equal(model.gcn_list[layers - 1].position_mask.cpu(), torch.as_tensor(z[f"mask.{layers - 1}"]))
    assert rel(model.relation_graph, z["relation_graph64"]) <= max(5.0 * float(z["yard_relation_graph"]), 1e-4)
    assert rel(model.graph_features, z["gcn_out64"]) <= max(5.0 * float(z["yard_gcn_out"]), 1e-4)
    named = dict(model.named_parameters())
    for k in z.files:
        if k.startswith("g64."):
            name = k[4:]
            got = named[name].grad.detach().flatten().double().cpu()
            if "gidx." + name in z.files:
                got = got[torch.as_tensor(z["gidx." + name])]
            err = Measured(float((got - torch.as_tensor(z[k])).abs().max()) / float(z["gmax64." + name]))
            assert err <= max(5.0 * float(z["yard." + name]), 1e-4), name
        if k.startswith("gsum.") and not k.startswith("gsum64."):
            name = k[5:]
            if ".fc_rn_phi_list." in name and name.endswith(".bias"):
                # analytically zero (the bias adds the same amount to every score of a row and the softmax removes it): what arrives is
                # rounding noise of the gradient that reaches the scores, bounded here by 1e-4 of the sibling theta bias's largest entry
                sib = float(z["gmax64." + name.replace("fc_rn_phi_list", "fc_rn_theta_list")])
                assert Measured(float(named[name].grad.abs().max())) <= 1e-4 * sib, name
                continue
            gs_tol = 6e-3 if name.startswith("backbone.") else 2e-3       # the model_* fixtures' bars
            assert Measured(abs(named[name].grad.double().sum().item() - float(z[k]))) <= gs_tol * float(z["gabs." + name]) + 1e-6, name


def test_arg_fixtures_exist():
    assert len(ARG_CASES) == 5, ARG_CASES


def test_eval_refuses_a_frame_count_that_is_not_a_multiple_of_three(gpu):
    from din_amd.config import Config
    from din_amd.infer_model import ARG_volleyball
    cfg = _small_cfg(None)
    model = ARG_volleyball(cfg).to(gpu).eval()
    images, boxes, _ = O.synth_inputs(1, 4, cfg.num_boxes, 64, 96, 2, 3, 8, seed=1)
    with pytest.raises(ValueError, match="multiple of 3"):
        model((images.to(gpu), boxes.to(gpu)))
    assert isinstance(cfg, Config)


# ---- one GCN block: entry points -------------------------------------------------------------------------------------------------------
def _small_cfg(tmp_path):
    from din_amd.config import Config
    cfg = Config("volleyball")
    cfg.backbone, cfg.image_size, cfg.out_size, cfg.emb_features = "vgg16", (64, 96), (2, 3), 512
    cfg.num_boxes, cfg.num_frames, cfg.num_features_boxes, cfg.num_features_gcn = 4, 2, 32, 32
    cfg.num_features_relation, cfg.num_graph, cfg.gcn_layers, cfg.pos_threshold = 16, 16, 1, 0.5
    cfg.inference_module_name, cfg.training_stage = "arg_volleyball", 2
    cfg.batch_size, cfg.test_batch_size, cfg.max_epoch, cfg.test_interval_epoch = 2, 2, 1, 1
    cfg.train_dropout_prob, cfg.train_learning_rate, cfg.lr_plan, cfg.train_backbone = 0.3, 1e-3, {}, True
    if tmp_path is not None:
        cfg.result_path = str(tmp_path)
    return cfg


def test_gcn_block_is_one_projection_and_one_graph_call_each_way(gpu, monkeypatch):
    from din_amd import _lib
    from din_amd.infer_module.ARG_infer_module import GCN_Module
    lib = _lib.load()
    calls = {}
    for name in _lib.SIGNATURES:
        fn = getattr(lib, name)

        def counting(*a, _fn=fn, _name=name):
            calls[_name] = calls.get(_name, 0) + 1
            return _fn(*a)
        monkeypatch.setattr(lib, name, counting)

    def forbidden(*a, **k):
        raise AssertionError("a torch matmul / softmax / layer_norm ran on the GCN block's path")
    for mod, name in [(torch, "matmul"), (torch, "bmm"), (torch, "softmax"), (torch, "layer_norm"), (F, "softmax"), (F, "layer_norm"),
                      (F, "linear"), (torch.Tensor, "matmul"), (torch.Tensor, "softmax")]:
        monkeypatch.setattr(mod, name, forbidden)
    cfg = _small_cfg(None)
    cfg.num_frames, cfg.num_boxes = 3, 12
    gcn = GCN_Module(cfg).to(gpu)
    g = torch.Generator().manual_seed(1)
    x = torch.randn((2, 36, 32), generator=g).to(gpu).requires_grad_(True)
    boxes = (torch.rand((2 * 36, 4), generator=g) * 3).to(gpu)
    out, r = gcn(x, boxes)
    out.sum().backward()
    torch.cuda.synchronize()
    launches = {k: v for k, v in calls.items() if k not in ("din_conv_packed_elems", "din_conv_workspace_bytes", "din_last_error_string",
                                                            "din_get_option", "din_conv_kernel_tile", "din_conv_kernel_variant")}
    assert launches == {"din_conv_pack_weights": 2, "din_conv_fwd": 1, "din_arg_graph_fwd": 1, "din_arg_graph_bwd": 1, "din_conv_wgrad": 1,
                        "din_conv_dgrad": 1}, launches
    assert tuple(out.shape) == (2, 36, 32) and tuple(r.shape) == (2, 36, 36)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in gcn.parameters())
    assert len(list(gcn.parameters())) == 16 * 7


# ---- trainer -------------------------------------------------------------------------------------------------------------------------
def test_train_net_arg_from_a_stage1_checkpoint_and_checkpoint_round_trip(gpu, tmp_path, monkeypatch):
    import din_amd.train_net_dynamic as tnd
    from din_amd.train_net import train_net as train_stage1
    cfg1 = _small_cfg(tmp_path)
    cfg1.training_stage, cfg1.num_frames, cfg1.train_dropout_prob, cfg1.inference_module_name = 1, 1, 0.0, "dynamic_volleyball"
    train_stage1(cfg1)
    ck = glob.glob(str(tmp_path / "stage1_epoch1_*.pth"))[0]
    state = torch.load(ck, map_location="cpu")
    cfg = _small_cfg(tmp_path)
    cfg.load_backbone_stage2, cfg.stage1_model_path = True, ck
    seen = {}
    real = tnd.train_volleyball

    def first_step(loader, model, *a, **k):
        if "before" not in seen:
            for kk, v in state["backbone_state_dict"].items():
                assert torch.equal(model.backbone.state_dict()[kk].cpu(), v), kk
            for kk, v in state["fc_emb_state_dict"].items():
                assert torch.equal(getattr(model.fc_emb_1, kk).detach().cpu(), v), kk
            seen["before"] = {n: p.detach().clone() for n, p in model.named_parameters()}
            seen["model"] = model
            seen["steps"] = len(loader)
        return real(loader, model, *a, **k)
    monkeypatch.setattr(tnd, "train_volleyball", first_step)
    infos = tnd.train_net(cfg)
    assert len(infos) == 1 and seen["steps"] == 2
    assert np.isfinite(infos[0]["train"]["loss"]) and np.isfinite(infos[0]["test"]["loss"])
    model = seen["model"]
    assert type(model).__name__ == "ARG_volleyball"
    gcn_names = [n for n in seen["before"] if n.startswith("gcn_list.")]
    assert len(gcn_names) == 16 * 7
    for n, p in model.named_parameters():
        assert not torch.equal(p.detach(), seen["before"][n]), n + " was not updated"
    ck2 = glob.glob(str(tmp_path / "stage2_epoch1_*.pth"))
    assert len(ck2) == 1
    again = tnd.build_model(cfg)
    tnd.load_stage2_state(again, ck2[0])
    again = again.to(gpu).eval()
    model.eval()
    images, boxes, _ = O.synth_inputs(2, 3 * cfg.num_frames, cfg.num_boxes, 64, 96, 2, 3, 8, seed=9)
    with torch.no_grad():
        a = model((images.to(gpu), boxes.to(gpu)))["activities"]
        b = again((images.to(gpu), boxes.to(gpu)))["activities"]
    assert tuple(a.shape) == (2, 8) and torch.equal(a, b)


def test_dropin_launcher_lines_build_the_arg_model(gpu, tmp_path, monkeypatch):
    """`dropin/` first on the module path, then the first lines of the reference's scripts/train_volleyball_stage2_arg.py (vgg16 set-up)
    with the small geometry: one epoch trains and tests"""
    monkeypatch.syspath_prepend(os.path.join(ROOT, "dropin"))
    for name in ("train_net_dynamic", "config", "infer_model"):
        sys.modules.pop(name, None)
    ns = {}
    exec("from train_net_dynamic import *\ncfg = Config('volleyball')\ncfg.inference_module_name = 'arg_volleyball'\n"
         "cfg.use_multi_gpu = False\ncfg.training_stage = 2\ncfg.train_backbone = False\ncfg.test_before_train = True\n"
         "cfg.backbone = 'vgg16'", ns)
    assert ns["train_net"].__module__ == "din_amd.train_net_dynamic"
    cfg, small = ns["cfg"], _small_cfg(tmp_path)
    for k in ("image_size", "out_size", "emb_features", "num_boxes", "num_frames", "num_features_boxes", "num_features_gcn",
              "num_features_relation", "num_graph", "batch_size", "test_batch_size", "max_epoch", "lr_plan", "result_path"):
        setattr(cfg, k, getattr(small, k))
    cfg.data_path = str(tmp_path / "no_such_dataset_tree")
    infos = ns["train_net"](cfg)
    assert len(infos) == 1 and np.isfinite(infos[0]["train"]["loss"])
