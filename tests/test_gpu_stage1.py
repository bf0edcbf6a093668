"""GPU (-m gpu): stage-1 base model (Basenet): the fused head kernel (csrc/basenet_head.hip) against an fp64 torch head, the whole
Basenet models against the reference's stage-1 golden fixtures (tests/golden/stage1_*.npz, tools/gen_golden_stage1.py), the entry-point
count of a training step, the stage-1 trainer, the stage-1 -> stage-2 checkpoint hand-over and the drop-in launcher lines."""
import glob
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
STAGE1_CASES = sorted(glob.glob(os.path.join(GOLDEN, "stage1_*.npz")))

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


# ---- the head in torch (reference base_model.py:117-139 / :243-268), any dtype, autograd ------------------------------------------------
def torch_head(s, wa, ba, wg, bg, counts, T, mean):
    """s = dropout(relu(y)) [BT, N, C] -> (actions, activities) with the reference's shapes"""
    bt, n, _ = s.shape
    if counts is None:
        actions = s @ wa.t() + ba                                    # [BT, N, A]
        frame = s.max(dim=1)[0] @ wg.t() + bg                        # [BT, A]
        if mean:
            B = bt // T
            return actions.reshape(B, T, n, -1).mean(dim=1).reshape(B * n, -1), frame.reshape(B, T, -1).mean(dim=1)
        return actions.reshape(bt * n, -1), frame
    acts, frames = [], []
    for k in range(bt):
        sk = s[k, :int(counts[k])]
        acts.append(sk @ wa.t() + ba)
        frames.append(sk.max(dim=0)[0][None] @ wg.t() + bg)
    return torch.cat(acts), torch.cat(frames)


def _head_inputs(B, T, N, C, aa, ag, seed, collective=False):
    g = torch.Generator().manual_seed(seed)
    y = torch.randn((B * T, N, C), generator=g)
    wa, ba = torch.randn((aa, C), generator=g) / C ** 0.5, 0.1 * torch.randn(aa, generator=g)
    wg, bg = torch.randn((ag, C), generator=g) / C ** 0.5, 0.1 * torch.randn(ag, generator=g)
    counts = None
    if collective:
        counts = torch.randint(1, N + 1, (B * T,), generator=g, dtype=torch.int32)
        counts[0], counts[-1] = 1, N                                 # ragged inside a clip, 1 and MAX_N
    return y, wa, ba, wg, bg, counts


def _run_kernel(dev, y, wa, ba, wg, bg, counts, T, mean, p, seed, cot_seed):
    from din_amd import ops
    ts = [t.to(dev).requires_grad_(True) for t in (y, wa, ba, wg, bg)]
    cnt = counts.to(dev) if counts is not None else None
    actions, activities = ops.BasenetHeadFunction.apply(*ts, cnt, T, mean, p, seed)
    g = torch.Generator().manual_seed(cot_seed)
    ga, gg = torch.randn(actions.shape, generator=g), torch.randn(activities.shape, generator=g)
    torch.autograd.backward([actions, activities], [ga.to(dev), gg.to(dev)])
    return actions, activities, [t.grad for t in ts], ga, gg


def _torch_grads(dtype, s_or_y, wa, ba, wg, bg, counts, T, mean, ga, gg, relu=True):
    ts = [t.to(dtype).clone().requires_grad_(True) for t in (s_or_y, wa, ba, wg, bg)]
    s = torch.relu(ts[0]) if relu else ts[0]
    actions, activities = torch_head(s, *ts[1:], counts, T, mean)
    torch.autograd.backward([actions, activities], [ga.to(dtype), gg.to(dtype)])
    return actions.detach(), activities.detach(), [t.grad for t in ts]


HEAD_SHAPES = [(8, 1, 12, 1024, 9, 8, False), (1, 10, 12, 1024, 9, 8, False), (2, 10, 13, 1024, 6, 5, True), (2, 3, 5, 200, 9, 8, False),
               (3, 2, 7, 200, 16, 16, True)]


@pytest.mark.parametrize("B,T,N,C,aa,ag,collective", HEAD_SHAPES,
                         ids=["vb_b8_t1", "vb_t10_mean", "collective_ragged", "odd_c200_t3_mean", "collective_c200_a16"])
def test_basenet_head_matches_fp64_torch(gpu, B, T, N, C, aa, ag, collective):
    y, wa, ba, wg, bg, counts = _head_inputs(B, T, N, C, aa, ag, seed=11 + B + T + C)
    mean = (not collective) and T != 1
    act, acty, grads, ga, gg = _run_kernel(gpu, y, wa, ba, wg, bg, counts, T, mean, 0.0, 5, 99)
    a64, g64_, grads64 = _torch_grads(torch.float64, y, wa, ba, wg, bg, counts, T, mean, ga, gg)
    _a32, _g32, grads32 = _torch_grads(torch.float32, y, wa, ba, wg, bg, counts, T, mean, ga, gg)
    assert act.shape == a64.shape and acty.shape == g64_.shape
    assert rel(act, a64) <= 1e-5 and rel(acty, g64_) <= 1e-5
    for name, got, r64, r32 in zip(("g_y", "dW_act", "db_act", "dW_grp", "db_grp"), grads, grads64, grads32):
        yard = float(rel(r32, r64))
        assert rel(got, r64) <= max(3.0 * yard, 1e-5), (name, float(rel(got, r64)), yard)


def test_basenet_head_dropout_matches_act_dropout_and_masks_the_gradient(gpu):
    from din_amd import ops
    B, T, N, C, aa, ag = 2, 3, 6, 256, 9, 8
    y, wa, ba, wg, bg, _ = _head_inputs(B, T, N, C, aa, ag, seed=3)
    seed = ops.mask_seed(7, 3)
    act, acty, grads, ga, gg = _run_kernel(gpu, y, wa, ba, wg, bg, None, T, True, 0.3, seed, 4)
    with torch.no_grad():
        s = ops.ActDropoutFunction.apply(y.to(gpu), True, 0.3, seed).cpu()
    a64, g64_, grads64 = _torch_grads(torch.float64, s, wa, ba, wg, bg, None, T, True, ga, gg, relu=False)
    assert rel(act, a64) <= 1e-5 and rel(acty, g64_) <= 1e-5
    g_y = grads[0].cpu()
    assert bool((g_y[s == 0] == 0).all()), "gradient leaks through a dropped or ReLU-clamped element"
    assert float((s == 0).double().mean()) > 0.55                    # ReLU half + 30 % of the rest
    ref = grads64[0] * (s > 0) * (1.0 / 0.7)                         # d/dy of dropout(relu(y)) = keep scale where s > 0
    assert rel(g_y, ref) <= 1e-5
    for got, r64 in zip(grads[1:], grads64[1:]):
        assert rel(got, r64) <= 1e-5


def test_basenet_head_ties_route_to_the_first_maximum(gpu):
    B, T, N, C, aa, ag = 2, 1, 5, 128, 9, 8
    y, wa, ba, wg, bg, _ = _head_inputs(B, T, N, C, aa, ag, seed=21)
    y[:, 1] = y[:, 1].abs() + 10.0                                   # box 1 is every channel's maximum ...
    y[:, 3] = y[:, 1]                                                # ... and box 3 duplicates it
    from din_amd import ops
    ts = [t.to(gpu).requires_grad_(True) for t in (y, wa, ba, wg, bg)]
    _act, acty = ops.BasenetHeadFunction.apply(*ts, None, T, False, 0.0, 0)
    acty.backward(torch.randn(acty.shape, device=gpu))               # the activity gradient alone
    g = ts[0].grad.cpu()
    assert bool((g[:, 1] != 0).all()) and bool((g[:, 3] == 0).all()) and bool((g[:, [0, 2, 4]] == 0).all())


def test_basenet_head_backward_is_deterministic(gpu):
    y, wa, ba, wg, bg, counts = _head_inputs(2, 10, 13, 1024, 6, 5, seed=8, collective=True)
    runs = [_run_kernel(gpu, y, wa, ba, wg, bg, counts, 10, False, 0.3, 1234, 5) for _ in range(2)]
    for a, b in zip(runs[0][2], runs[1][2]):
        assert torch.equal(a, b)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_basenet_head_refuses_bad_shapes_and_counts(gpu):
    from din_amd import _lib, ops
    y, wa, ba, wg, bg, counts = _head_inputs(1, 2, 4, 64, 17, 8, seed=1)
    with pytest.raises(_lib.DinError, match="A_act 17"):
        ops.BasenetHeadFunction.apply(y.to(gpu), wa.to(gpu), ba.to(gpu), wg.to(gpu), bg.to(gpu), None, 2, True, 0.0, 0)
    y, wa, ba, wg, bg, counts = _head_inputs(1, 2, 4, 64, 9, 8, seed=1)
    for bad in ([0, 3], [2, 5]):
        with pytest.raises(_lib.DinError, match="outside 1..N"):
            ops.BasenetHeadFunction.apply(y.to(gpu), wa.to(gpu), ba.to(gpu), wg.to(gpu), bg.to(gpu),
                                          torch.tensor(bad, dtype=torch.int32, device=gpu), 2, False, 0.0, 0)


# ---- whole models against the reference's stage-1 fixtures ---------------------------------------------------------------------------
def _fixture_model(gpu, path, dtype="fp32"):
    from din_amd.base_model import Basenet_collective, Basenet_volleyball
    from din_amd.config import Config
    z = np.load(path)
    B, T, N, H, W, OH, OW, D, NFB, A_act, A_grp = (int(v) for v in z["meta"])
    dataset, backbone, seed = str(z["dataset"]), str(z["backbone"]), int(z["seed"])
    collective = dataset == "collective"
    cfg = Config(dataset)
    cfg.backbone, cfg.image_size, cfg.out_size, cfg.emb_features = backbone, (H, W), (OH, OW), D
    cfg.num_boxes, cfg.num_frames, cfg.num_features_boxes, cfg.num_actions, cfg.num_activities = N, T, NFB, A_act, A_grp
    cfg.train_backbone, cfg.backbone_dtype = True, dtype
    model = (Basenet_collective if collective else Basenet_volleyball)(cfg)
    fc_emb = "fc_emb_1" if collective else "fc_emb"
    shapes = {k: v for k, v in O.model_param_shapes(O.OracleCfg(backbone=backbone, emb_features=D, num_features_boxes=NFB)).items()
              if k.startswith("backbone.")}
    shapes.update({fc_emb + ".weight": (NFB, 25 * D), fc_emb + ".bias": (NFB,), "fc_actions.weight": (A_act, NFB),
                   "fc_actions.bias": (A_act,), "fc_activities.weight": (A_grp, NFB), "fc_activities.bias": (A_grp,)})
    p = O.synth_params(shapes, seed=seed)                           # same recipe as tools/gen_golden_stage1.py::stage1_params
    p.update({k[2:]: torch.as_tensor(z[k]) for k in z.files if k.startswith("p.")})
    missing, unexpected = model.load_state_dict(p, strict=False)
    assert not unexpected and all("num_batches_tracked" in k for k in missing), (missing, unexpected)
    model = model.to(gpu).eval()
    images, boxes, _ = O.synth_inputs(B, T, N, H, W, OH, OW, A_grp, seed=seed)
    inputs = (images.to(gpu), boxes.to(gpu))
    if collective:
        counts = torch.as_tensor(z["counts"])
        for b in range(B):
            for t in range(T):
                boxes[b, t, int(counts[b, t]):] = 0.0
        inputs = (images.to(gpu), boxes.to(gpu), counts.to(gpu))
    actions, activities = model(inputs)                             # uint8 images straight in
    a_in, g_in = torch.as_tensor(z["actions_in"]), torch.as_tensor(z["activities_in"])
    if collective:
        c = torch.as_tensor(z["counts"]).reshape(-1)
        tgt_a = torch.cat([a_in.reshape(B * T, N)[k, :int(c[k])] for k in range(B * T)])
        la = F.cross_entropy(actions, tgt_a.to(gpu))
        lg = F.cross_entropy(activities, g_in.reshape(-1).to(gpu))
    else:
        w = torch.as_tensor(z["actions_weights"]).to(gpu)
        la = F.cross_entropy(actions, a_in[:, 0, :].reshape(-1).to(gpu), weight=w)
        lg = F.cross_entropy(activities, g_in[:, 0].to(gpu))
    loss = lg + la
    loss.backward()
    return z, model, actions, activities, la, lg, loss


@pytest.mark.parametrize("path", STAGE1_CASES, ids=[os.path.basename(p)[:-4] for p in STAGE1_CASES])
def test_basenet_matches_reference_stage1_golden(gpu, path):
    z, model, actions, activities, la, lg, loss = _fixture_model(gpu, path)
    assert rel(actions, z["actions"]) <= 1e-4 and rel(activities, z["activities"]) <= 1e-4
    for got, ref in ((la, z["actions_loss"]), (lg, z["activities_loss"]), (loss, z["loss"])):
        assert Measured(abs(got.item() - float(ref))) <= 1e-4 * max(1.0, abs(float(ref)))
    named = dict(model.named_parameters())
    for k in z.files:
        if k.startswith("g."):                                       # head + embedding bias: against fp64, the reference's own gap x5
            name = k[2:]
            yard = float(z["yard." + name])
            assert rel(named[name].grad, z["g64." + name]) <= max(5.0 * yard, 1e-4), name
            assert rel(named[name].grad, z[k]) <= max(5.0 * yard, 1e-4) + yard, name
        if k.startswith("gsum.") and not k.startswith("gsum64."):
            name = k[5:]
            gs_tol = 6e-3 if name.startswith("backbone.") else 2e-3       # the model_* fixtures' bars
            assert Measured(abs(named[name].grad.double().sum().item() - float(z[k]))) <= gs_tol * float(z["gabs." + name]) + 1e-6, name


def test_basenet_bf16_tracks_reference_stage1_golden(gpu):
    """bf16 backbone + bf16 embedding GEMM operands: closeness only (bars ~3x the values measured on an MI355X)."""
    path = os.path.join(GOLDEN, "stage1_vgg16_96x160_t1.npz")
    z, model, actions, activities, _la, _lg, loss = _fixture_model(gpu, path, dtype="bf16")
    e_a, e_g = rel(actions, z["actions"]), rel(activities, z["activities"])
    print(f"bf16 stage-1: actions rel err {float(e_a):.3e}, activities rel err {float(e_g):.3e}, loss {loss.item():.5f} vs {float(z['loss']):.5f}")
    assert e_a <= 3e-2 and e_g <= 3e-2                              # measured 9.1e-3 (actions), 3.8e-3 (activities)
    assert Measured(abs(loss.item() - float(z["loss"]))) <= 2e-3 * abs(float(z["loss"]))    # measured 4.4e-4 of the loss


# ---- one training step: entry points -------------------------------------------------------------------------------------------------
def _small_cfg(dataset, tmp_path, backbone="vgg16"):
    from din_amd.config import Config
    cfg = Config(dataset)
    if backbone == "vgg16":
        cfg.backbone, cfg.image_size, cfg.out_size, cfg.emb_features = "vgg16", (64, 96), (2, 3), 512
    else:
        cfg.backbone, cfg.image_size, cfg.out_size, cfg.emb_features = "inv3", (139, 203), (15, 23), 1056
    cfg.num_boxes, cfg.num_frames, cfg.num_features_boxes = 4, 1, 32
    cfg.training_stage, cfg.batch_size, cfg.test_batch_size, cfg.max_epoch, cfg.test_interval_epoch = 1, 2, 2, 1, 1
    cfg.train_dropout_prob, cfg.train_learning_rate, cfg.lr_plan, cfg.train_backbone = 0.0, 1e-3, {}, True
    cfg.result_path = str(tmp_path)
    return cfg


def test_one_training_step_calls_the_fused_head_once_each_way(gpu, tmp_path, monkeypatch):
    from din_amd import _lib
    from din_amd.base_model import Basenet_volleyball
    from din_amd.optim import FusedAdam
    from din_amd.train_net_dynamic import SyntheticVolleyball
    lib = _lib.load()
    calls = {}
    for name in ("din_basenet_head_fwd", "din_basenet_head_bwd", "din_act_dropout_fwd", "din_act_dropout_bwd"):
        fn = getattr(lib, name)

        def counting(*a, _fn=fn, _name=name):
            calls[_name] = calls.get(_name, 0) + 1
            return _fn(*a)
        monkeypatch.setattr(lib, name, counting)
    cfg = _small_cfg("volleyball", tmp_path)
    cfg.train_dropout_prob = 0.3
    model = Basenet_volleyball(cfg).to(gpu).train()
    opt = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=1e-4)
    images, boxes, actions_in, activities_in = [t.unsqueeze(0).to(gpu) for t in SyntheticVolleyball(cfg, length=1)[0]]
    actions, activities = model((images, boxes))
    loss = F.cross_entropy(activities, activities_in[:, 0]) + F.cross_entropy(actions, actions_in[:, 0].reshape(-1))
    opt.zero_grad()
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    assert calls == {"din_basenet_head_fwd": 1, "din_basenet_head_bwd": 1}, calls


# ---- trainer -------------------------------------------------------------------------------------------------------------------------
def test_train_net_stage1_volleyball_first_loss_and_checkpoint(gpu, tmp_path, monkeypatch):
    import din_amd.train_net as tn
    from din_amd import ops
    cfg = _small_cfg("volleyball", tmp_path)
    cfg.actions_weights = [[1., 1., 2., 3., 1., 2., 2., 0.2, 1.]]        # the launcher's nested form
    seen = {}
    real_head, real_losses = ops.BasenetHeadFunction, tn._losses

    class Spy:
        @staticmethod
        def apply(y, wa, ba, wg, bg, *rest):
            if "head" not in seen:
                seen["head"] = [t.detach().double().cpu().clone() for t in (y, wa, ba, wg, bg)] + list(rest)
            return real_head.apply(y, wa, ba, wg, bg, *rest)

    def losses(actions_scores, activities_scores, actions_in, activities_in, batch_data, cfg_, collective):
        out = real_losses(actions_scores, activities_scores, actions_in, activities_in, batch_data, cfg_, collective)
        if "loss" not in seen:
            seen["loss"] = (out[0].item(), actions_in.cpu(), activities_in.cpu())
        return out
    monkeypatch.setattr(ops, "BasenetHeadFunction", Spy)
    monkeypatch.setattr(tn, "_losses", losses)
    infos = tn.train_net(cfg)
    assert len(infos) == 1
    for part in ("train", "test"):
        for key in ("time", "epoch", "loss", "activities_acc", "actions_acc", "activities_conf", "activities_MPCA"):
            assert key in infos[0][part], (part, key)
    y, wa, ba, wg, bg, counts, T, mean, p, _seed = seen["head"]
    assert counts is None and p == 0.0 and not mean
    a, g = torch_head(torch.relu(y), wa, ba, wg, bg, None, T, mean)         # the reference recipe in fp64 on the model's own features
    loss_val, a_in, g_in = seen["loss"]
    w = torch.tensor(cfg.actions_weights, dtype=torch.float64).reshape(-1)
    ref = F.cross_entropy(g, g_in) + F.cross_entropy(a, a_in, weight=w)
    assert Measured(abs(loss_val - ref.item())) <= 1e-4 * max(1.0, abs(ref.item()))
    ck = glob.glob(str(tmp_path / "stage1_epoch1_*.pth"))
    assert len(ck) == 1
    assert set(torch.load(ck[0], map_location="cpu")) == {"backbone_state_dict", "fc_emb_state_dict", "fc_actions_state_dict",
                                                          "fc_activities_state_dict"}


def test_train_net_stage1_collective_runs_one_epoch(gpu, tmp_path):
    from din_amd.train_net import train_net
    cfg = _small_cfg("collective", tmp_path, backbone="inv3")
    cfg.num_frames, cfg.num_actions, cfg.num_activities = 2, 6, 5
    infos = train_net(cfg)
    tr, te = infos[0]["train"], infos[0]["test"]
    assert np.isfinite(tr["loss"]) and np.isfinite(te["loss"]) and "actions_acc" in tr and "actions_acc" in te
    assert 0.0 <= tr["actions_acc"] <= 100.0 and tr["activities_conf"].shape == (5, 5)
    assert int(tr["activities_conf"].sum()) == 4 * cfg.num_frames              # activities per frame (reference :294-295)
    assert glob.glob(str(tmp_path / "stage1_epoch1_*.pth"))


def test_stage1_checkpoint_starts_stage2(gpu, tmp_path, monkeypatch):
    import din_amd.train_net_dynamic as tnd
    from din_amd.train_net import train_net
    cfg1 = _small_cfg("volleyball", tmp_path)
    train_net(cfg1)
    ck = glob.glob(str(tmp_path / "stage1_epoch1_*.pth"))[0]
    state = torch.load(ck, map_location="cpu")
    cfg2 = _small_cfg("volleyball", tmp_path)
    cfg2.training_stage, cfg2.num_frames, cfg2.num_features_gcn = 2, 2, 32
    cfg2.ST_kernel_size, cfg2.sampling_ratio, cfg2.beta_factor = [(3, 3)], [1], False
    cfg2.load_backbone_stage2, cfg2.stage1_model_path = True, ck
    checked = []
    real = tnd.train_volleyball

    def first_step(loader, model, *a, **k):
        if not checked:
            for kk, v in state["backbone_state_dict"].items():
                assert torch.equal(model.backbone.state_dict()[kk].cpu(), v), kk
            for kk, v in state["fc_emb_state_dict"].items():
                assert torch.equal(getattr(model.fc_emb_1, kk).detach().cpu(), v), kk
            checked.append(True)
        return real(loader, model, *a, **k)
    monkeypatch.setattr(tnd, "train_volleyball", first_step)
    infos = tnd.train_net(cfg2)
    assert checked and len(infos) == 1 and np.isfinite(infos[0]["train"]["loss"])


def test_dropin_launcher_lines_run_stage1(gpu, tmp_path, monkeypatch):
    """`dropin/` first on the module path, then the first lines of the reference's scripts/train_volleyball_stage1.py with the small
    geometry: one epoch trains, tests and writes the stage-1 checkpoint"""
    import importlib
    monkeypatch.syspath_prepend(os.path.join(ROOT, "dropin"))
    for name in ("train_net", "config", "base_model"):
        sys.modules.pop(name, None)
    ns = {}
    exec("from train_net import *\ncfg = Config('volleyball')\ncfg.use_multi_gpu = False\ncfg.training_stage = 1\n"
         "cfg.stage1_model_path = ''\ncfg.train_backbone = True\ncfg.test_before_train = True\ncfg.backbone = 'vgg16'", ns)
    assert ns["train_net"].__module__ == "din_amd.train_net"
    cfg, small = ns["cfg"], _small_cfg("volleyball", tmp_path)
    for k in ("image_size", "out_size", "emb_features", "num_boxes", "num_frames", "num_features_boxes", "batch_size", "test_batch_size",
              "max_epoch", "train_dropout_prob", "lr_plan", "result_path"):
        setattr(cfg, k, getattr(small, k))
    cfg.set_bn_eval, cfg.actions_weights = False, [[1., 1., 2., 3., 1., 2., 2., 0.2, 1.]]
    cfg.data_path = str(tmp_path / "no_such_dataset_tree")
    infos = ns["train_net"](cfg)
    assert len(infos) == 1 and np.isfinite(infos[0]["train"]["loss"])
    assert glob.glob(str(tmp_path / "stage1_epoch1_*.pth"))
    importlib.invalidate_caches()
