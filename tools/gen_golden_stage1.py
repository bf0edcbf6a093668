#!/usr/bin/env python3
"""Generate tests/golden/stage1_*.npz by running the REFERENCE's stage-1 base models (base_model.Basenet_volleyball / Basenet_collective)
on CPU, in eval() (dropout off, BatchNorm on running statistics).

Runs ONLY where the reference tree is (it never travels to the GPU box).  Nothing of the reference is copied: its modules are imported
under the dependency stubs of tools/gen_golden.py (install_stubs), fed seeded weights / inputs (oracle.din_oracle synth_params /
synth_inputs) and the numbers they produce are stored.  The oracle has no Basenet, so the yardstick is the same reference model converted
with .double(): every fixture records the fp32-vs-fp64 gap of its outputs and of every stored gradient.

Stored per case: geometry and seeds (the test regenerates weights and inputs from them), the fc_* biases (seeded, non-zero), the labels,
`actions`, `activities`, both cross-entropy losses and their sum, gsum / gabs of every parameter gradient, the full gradients of
fc_actions, fc_activities and fc_emb*.bias (fp32 run `g.*`, fp64 run `g64.*`, relative gap `yard.*`), and the smallest gap between the
two largest box activations of any (frame, channel) -- the margin of the max over boxes.

usage: python tools/gen_golden_stage1.py [--ref /root/reference] [--out tests/golden]
"""
import argparse
import copy
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from oracle.din_oracle import OracleCfg, model_param_shapes, synth_inputs, synth_params  # noqa: E402
from gen_golden import install_stubs  # noqa: E402

VOLLEYBALL_WEIGHTS = [1., 1., 2., 3., 1., 2., 2., 0.2, 1.]          # scripts/train_volleyball_stage1.py (actions_weights)


def stage1_shapes(backbone, D, K, NFB, A_act, A_grp, fc_emb):
    shapes = {k: v for k, v in model_param_shapes(OracleCfg(backbone=backbone, emb_features=D, num_features_boxes=NFB)).items()
              if k.startswith("backbone.")}
    shapes.update({fc_emb + ".weight": (NFB, K * K * D), fc_emb + ".bias": (NFB,), "fc_actions.weight": (A_act, NFB),
                   "fc_actions.bias": (A_act,), "fc_activities.weight": (A_grp, NFB), "fc_activities.bias": (A_grp,)})
    return shapes


def stage1_params(shapes, seed):
    """backbone + heads from oracle.synth_params (kaiming weights), then seeded non-zero fc_* biases (stored in the fixture too)"""
    p = synth_params(shapes, seed=seed)
    g = torch.Generator().manual_seed(seed + 7)
    for k in sorted(p):
        if k.startswith("fc_") and k.endswith(".bias"):
            p[k] = 0.1 * torch.randn(p[k].shape, generator=g, dtype=torch.float64).float()
    return p


def _labels(seed, B, T, N, A_act, A_grp):
    r = np.random.default_rng(seed + 5)
    return (torch.from_numpy(r.integers(0, A_act, size=(B, T, N)).astype(np.int64)),
            torch.from_numpy(r.integers(0, A_grp, size=(B, T)).astype(np.int64)))


def _run(model, images, boxes, counts, actions_in, activities_in, weights, collective, dtype):
    model = model.to(dtype)
    model.eval()
    model.zero_grad()
    B, T, N = boxes.shape[:3]
    inp = (images.to(dtype), boxes.to(dtype)) + ((counts,) if collective else ())
    acts = {}
    fc = model.fc_emb_1 if collective else model.fc_emb
    h = fc.register_forward_hook(lambda m, i, o: acts.__setitem__("y", o.detach()))
    actions, activities = model(inp)
    h.remove()
    if collective:
        tgt_a = torch.cat([actions_in.reshape(B * T, N)[bt, :int(counts.reshape(-1)[bt])] for bt in range(B * T)])
        tgt_g = activities_in.reshape(-1)
        w = None
    else:
        tgt_a, tgt_g = actions_in[:, 0, :].reshape(B * N), activities_in[:, 0]
        w = torch.tensor(weights, dtype=dtype)
    la = F.cross_entropy(actions, tgt_a, weight=w)
    lg = F.cross_entropy(activities, tgt_g)
    loss = lg + 1.0 * la
    loss.backward()
    grads = {k: v.grad.detach().clone() for k, v in model.named_parameters() if v.grad is not None}
    return actions.detach(), activities.detach(), la.item(), lg.item(), loss.item(), grads, acts["y"]


def case(name, refbm, refcfg, out_dir, *, dataset, backbone, H, W, OH, OW, D, B, T, N, NFB, A_act, A_grp, seed, counts=None):
    collective = dataset == "collective"
    cfg = refcfg.Config(dataset)
    cfg.log_path = None
    cfg.backbone, cfg.image_size, cfg.out_size, cfg.emb_features = backbone, (H, W), (OH, OW), D
    cfg.num_boxes, cfg.num_frames, cfg.batch_size = N, T, B
    cfg.num_features_boxes, cfg.num_actions, cfg.num_activities = NFB, A_act, A_grp
    cfg.train_backbone, cfg.train_dropout_prob = True, 0.3
    fc_emb = "fc_emb_1" if collective else "fc_emb"
    torch.manual_seed(0)
    model = (refbm.Basenet_collective if collective else refbm.Basenet_volleyball)(cfg)
    p = stage1_params(stage1_shapes(backbone, D, cfg.crop_size[0], NFB, A_act, A_grp, fc_emb), seed)
    missing, unexpected = model.load_state_dict(p, strict=False)
    assert not unexpected and all("num_batches_tracked" in k for k in missing), (missing, unexpected)
    images, boxes, _ = synth_inputs(B, T, N, H, W, OH, OW, A_grp, seed=seed)
    actions_in, activities_in = _labels(seed, B, T, N, A_act, A_grp)
    cnt = None
    if collective:
        cnt = torch.tensor(counts, dtype=torch.int64)
        for b in range(B):
            for t in range(T):
                boxes[b, t, int(cnt[b, t]):] = 0.0                      # zero padding boxes (collective.py:201-203)
                actions_in[b, t, int(cnt[b, t]):] = -1
    r32 = _run(model, images.float(), boxes, cnt, actions_in, activities_in, VOLLEYBALL_WEIGHTS, collective, torch.float32)
    r64 = _run(copy.deepcopy(model), images.float(), boxes, cnt, actions_in, activities_in, VOLLEYBALL_WEIGHTS, collective, torch.float64)

    def gap(a, b):
        return float((a.double() - b).abs().max() / (b.abs().max() + 1e-300))

    y64 = torch.relu(r64[6]).reshape(B * T, N, NFB)
    if collective:
        valid = torch.arange(N)[None, :, None] < cnt.reshape(B * T, 1, 1)
        y64 = torch.where(valid, y64, torch.full_like(y64, -1.0))
    top2 = y64.topk(2, dim=1).values if N > 1 else torch.cat([y64, torch.zeros_like(y64)], 1)
    pos = top2[:, 0] > 0
    margin = float((top2[:, 0] - top2[:, 1])[pos].min()) if pos.any() else 0.0
    rec = dict(meta=np.array([B, T, N, H, W, OH, OW, D, NFB, A_act, A_grp], dtype=np.int64), dataset=np.array(dataset),
               backbone=np.array(backbone), seed=np.int64(seed), actions_weights=np.array(VOLLEYBALL_WEIGHTS, dtype=np.float32),
               actions_in=actions_in.numpy(), activities_in=activities_in.numpy(),
               actions=r32[0].numpy(), activities=r32[1].numpy(), actions_loss=np.float64(r32[2]), activities_loss=np.float64(r32[3]),
               loss=np.float64(r32[4]), actions64=r64[0].numpy(), activities64=r64[1].numpy(), loss64=np.float64(r64[4]),
               yard_actions=np.float64(gap(r32[0], r64[0])), yard_activities=np.float64(gap(r32[1], r64[1])),
               yard_loss=np.float64(abs(r32[4] - r64[4]) / max(abs(r64[4]), 1e-300)), max_margin=np.float64(margin))
    if collective:
        rec["counts"] = cnt.numpy().astype(np.int32)
    for k in sorted(p):
        if k.startswith("fc_") and k.endswith(".bias"):
            rec["p." + k] = p[k].numpy()
    g32, g64 = r32[5], r64[5]
    for k in sorted(g32):
        rec["gsum." + k] = np.float64(g32[k].double().sum().item())
        rec["gabs." + k] = np.float64(g32[k].double().abs().sum().item())
        rec["gsum64." + k] = np.float64(g64[k].sum().item())
        if k.startswith("fc_actions.") or k.startswith("fc_activities.") or k == fc_emb + ".bias":
            rec["g." + k] = g32[k].numpy()
            rec["g64." + k] = g64[k].numpy()
            rec["yard." + k] = np.float64(gap(g32[k], g64[k]))
    path = os.path.join(out_dir, name + ".npz")
    np.savez_compressed(path, **rec)
    print(f"[stage1] {name}: loss {r32[4]:.6f}, fp32-vs-fp64 actions {rec['yard_actions']:.1e} activities {rec['yard_activities']:.1e} "
          f"worst head grad {max(float(v) for k, v in rec.items() if k.startswith('yard.')):.1e}, max margin {margin:.2e}, "
          f"{os.path.getsize(path) / 1024:.0f} KiB")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    sys.dont_write_bytecode = True
    install_stubs()
    sys.path.insert(0, a.ref)
    os.makedirs(a.out, exist_ok=True)
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    import importlib
    refbm = importlib.import_module("base_model")
    refcfg = importlib.import_module("config")
    vgg = dict(dataset="volleyball", backbone="vgg16", H=96, W=160, OH=3, OW=5, D=512, B=2, N=4, NFB=64, A_act=9, A_grp=8)
    case("stage1_vgg16_96x160_t1", refbm, refcfg, a.out, T=1, seed=500, **vgg)          # the stage-1 training shape (T = 1)
    case("stage1_vgg16_96x160_t3", refbm, refcfg, a.out, T=3, seed=501, **vgg)          # the T-mean path
    inv3 = dict(backbone="inv3", H=139, W=203, OH=15, OW=23, D=1056, NFB=64)           # the geometry of model_inv3_139x203_*
    case("stage1_inv3_139x203", refbm, refcfg, a.out, dataset="volleyball", B=1, T=3, N=6, A_act=9, A_grp=8, seed=502, **inv3)
    case("stage1_collective_inv3_139x203", refbm, refcfg, a.out, dataset="collective", B=2, T=3, N=6, A_act=6, A_grp=5, seed=503,
         counts=[[6, 1, 4], [3, 6, 2]], **inv3)                                          # per-frame counts vary inside a clip, 1 and MAX_N
    print("stage-1 golden vectors written to", a.out)


if __name__ == "__main__":
    main()
