#!/usr/bin/env python3
"""Generate tests/golden/arg_*.npz by running the REFERENCE's ARG baseline (infer_model.ARG_volleyball with infer_module.ARG_infer_module.
GCN_Module) on CPU, in fp32 and converted with .double().

Runs ONLY where the reference tree is.  Nothing of the reference is copied: its modules are imported under the dependency stubs of
tools/gen_golden.py (install_stubs), fed seeded weights / inputs (oracle.din_oracle synth_params / synth_inputs, `arg_params` below) and the
numbers they produce are stored.  The tests rebuild weights and inputs from the stored geometry and seeds with `arg_params` / synth_inputs.

Stored per case: geometry, seeds, mode and pos_threshold; the state_dict key list; labels; `activities` (fp32), `activities64`, their gap;
both losses; the input of the first GCN layer (`gcn_in64`); per GCN layer the position mask (`mask.{l}`, bool) and the centres it was formed from (`centres.{l}`, fp64); the last relation
graph and the GCN output before the residual (fp32, fp64, gap); `min_margin` = smallest |dist - thr| / thr over all pairs and layers and
`masked_share`; for every parameter gsum / gabs / gsum64 of its gradient; for every NON-backbone parameter `yard.*` (fp32-vs-fp64 gap of the
whole gradient, relative to its largest entry), `gmax64.*` (that largest entry) and the gradient itself in fp32 (`g.*`) and fp64 (`g64.*`) --
whole when it has at most GRAD_CAP elements, else at the evenly spaced flat indices `gidx.*` (a [NFB, 25 * D] embedding gradient would not
fit the size limit of a committed file).  The bias of fc_rn_phi_list.{i} has no such entries: it adds the same amount to every score of a
row, the softmax removes it, and its gradient is rounding noise around zero (gsum / gabs are still stored).

The generator asserts (a) min_margin >= 1e-3, so that fp32 rounding (about 1e-6) cannot flip a mask entry whichever way the distance is
formed, (b) 0.15 <= masked_share <= 0.85, so that both branches are exercised, and (c) loss >= 1e-2: with one clip and logits of the size
the sum over 16 graphs gives, a seed whose label is the arg-max leaves a loss of 0 and gradients of pure rounding noise.  Train-mode cases run with dropout 0 and BatchNorm on
running statistics (the trainer's set_bn_eval).

usage: python tools/gen_golden_arg.py [--ref /root/reference] [--out tests/golden] [--only NAME]
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

GRAD_CAP = 512

VGG = dict(backbone="vgg16", H=96, W=160, OH=3, OW=5, D=512, A=8)
CASES = {
    "arg_vgg16_96x160_1layer": dict(B=2, T=3, N=4, NFB=64, NFR=32, NG=4, layers=1, mode="train", pos_threshold=0.5, seed=600, **VGG),
    "arg_vgg16_96x160_2layer": dict(B=2, T=3, N=4, NFB=64, NFR=32, NG=4, layers=2, mode="train", pos_threshold=0.2, seed=601, **VGG),
    "arg_vgg16_96x160_eval9": dict(B=2, T=3, N=4, NFB=64, NFR=32, NG=4, layers=1, mode="eval", pos_threshold=0.2, seed=602, **VGG),
    "arg_vgg16_96x160_n12_ng16": dict(B=1, T=3, N=12, NFB=128, NFR=64, NG=16, layers=1, mode="train", pos_threshold=0.2, seed=606, **VGG),
    "arg_inv3_139x203": dict(B=1, T=3, N=6, NFB=64, NFR=32, NG=4, layers=1, mode="train", pos_threshold=0.2, seed=604,
                             backbone="inv3", H=139, W=203, OH=15, OW=23, D=1056, A=8),     # the geometry of stage1_inv3_139x203
}


def arg_shapes(backbone, D, K, T, N, NFB, NFR, NG, layers, A):
    shapes = {k: v for k, v in model_param_shapes(OracleCfg(backbone=backbone, emb_features=D, num_features_boxes=NFB)).items()
              if k.startswith(("backbone.", "fc_emb_1.", "nl_emb_1."))}
    for l in range(layers):
        for i in range(NG):
            shapes[f"gcn_list.{l}.fc_rn_theta_list.{i}.weight"] = (NFR, NFB)
            shapes[f"gcn_list.{l}.fc_rn_theta_list.{i}.bias"] = (NFR,)
            shapes[f"gcn_list.{l}.fc_rn_phi_list.{i}.weight"] = (NFR, NFB)
            shapes[f"gcn_list.{l}.fc_rn_phi_list.{i}.bias"] = (NFR,)
            shapes[f"gcn_list.{l}.fc_gcn_list.{i}.weight"] = (NFB, NFB)
            shapes[f"gcn_list.{l}.nl_gcn_list.{i}.weight"] = (T * N, NFB)
            shapes[f"gcn_list.{l}.nl_gcn_list.{i}.bias"] = (T * N, NFB)
    shapes["fc_activities.weight"] = (A, NFB)
    shapes["fc_activities.bias"] = (A,)
    return shapes


def arg_params(shapes, seed):
    """oracle.synth_params (kaiming weights), then seeded NON-TRIVIAL Linear biases and LayerNorm affines outside the backbone: at their
    zeros / ones initial values a swapped or dropped term would pass"""
    p = synth_params(shapes, seed=seed)
    g = torch.Generator().manual_seed(seed + 7)
    for k in sorted(p):
        if k.startswith("backbone."):
            continue
        if ".nl_" in k or k.startswith("nl_"):
            r = torch.randn(p[k].shape, generator=g, dtype=torch.float64)
            p[k] = ((1.0 + 0.2 * r) if k.endswith("weight") else 0.1 * r).float()
        elif k.endswith(".bias"):
            p[k] = (0.1 * torch.randn(p[k].shape, generator=g, dtype=torch.float64)).float()
    return p


def case_inputs(c):
    """(images [B, Tin, 3, H, W], boxes [B, Tin, N, 4], labels [B]); Tin = 3 T in eval mode (three sub-clips)"""
    tin = c["T"] * 3 if c["mode"] == "eval" else c["T"]
    return synth_inputs(c["B"], tin, c["N"], c["H"], c["W"], c["OH"], c["OW"], c["A"], seed=c["seed"])


def grad_index(numel):
    return np.arange(numel, dtype=np.int64) if numel <= GRAD_CAP else np.linspace(0, numel - 1, GRAD_CAP).astype(np.int64)


def _bn_eval(m):
    if m.__class__.__name__.find("BatchNorm") != -1:
        m.eval()


def _run(model, refarg, c, images, boxes, labels, dtype):
    model = model.to(dtype)
    if c["mode"] == "eval":
        model.eval()
    else:
        model.train()
        model.apply(_bn_eval)
    model.zero_grad()
    seen = {"dist": [], "pos": []}
    orig = refarg.calc_pairwise_distance_3d

    def spy(x, y):
        d = orig(x, y)
        seen["dist"].append(d.detach().clone())
        seen["pos"].append(x.detach().clone())
        return d

    outs = []
    pre = model.gcn_list[0].register_forward_pre_hook(lambda m, i: seen.__setitem__("gcn_in", i[0].detach().clone()))
    hook = model.gcn_list[-1].register_forward_hook(lambda m, i, o: outs.append((o[0].detach().clone(), o[1].detach().clone())))
    refarg.calc_pairwise_distance_3d = spy
    try:
        scores = model((images.to(dtype), boxes.clone().to(dtype)))["activities"]      # (the reference writes into the boxes it is given)
    finally:
        refarg.calc_pairwise_distance_3d = orig
        hook.remove()
        pre.remove()
    loss = F.cross_entropy(scores, labels)
    loss.backward()
    grads = {k: v.grad.detach().clone() for k, v in model.named_parameters() if v.grad is not None}
    return scores.detach(), loss.item(), grads, outs[0][0], outs[0][1], seen


def case(name, c, refim, refarg, refcfg, out_dir):
    cfg = refcfg.Config("volleyball")
    cfg.log_path = None
    cfg.backbone, cfg.image_size, cfg.out_size, cfg.emb_features = c["backbone"], (c["H"], c["W"]), (c["OH"], c["OW"]), c["D"]
    cfg.num_boxes, cfg.num_frames, cfg.batch_size = c["N"], c["T"], c["B"]
    cfg.num_features_boxes = cfg.num_features_gcn = c["NFB"]
    cfg.num_features_relation, cfg.num_graph, cfg.gcn_layers = c["NFR"], c["NG"], c["layers"]
    cfg.num_activities, cfg.pos_threshold = c["A"], c["pos_threshold"]
    cfg.train_backbone, cfg.train_dropout_prob = True, 0.0
    torch.manual_seed(0)
    model = refim.ARG_volleyball(cfg)
    p = arg_params(arg_shapes(c["backbone"], c["D"], cfg.crop_size[0], c["T"], c["N"], c["NFB"], c["NFR"], c["NG"], c["layers"], c["A"]),
                   c["seed"])
    missing, unexpected = model.load_state_dict(p, strict=False)
    assert not unexpected and all("num_batches_tracked" in k for k in missing), (missing, unexpected)
    images, boxes, labels = case_inputs(c)
    r32 = _run(model, refarg, c, images.float(), boxes, labels, torch.float32)
    r64 = _run(copy.deepcopy(model), refarg, c, images.float(), boxes, labels, torch.float64)

    def gap(a, b):
        return float((a.double() - b).abs().max() / (b.abs().max() + 1e-300))

    thr = c["pos_threshold"] * c["OW"]
    rec = dict(meta=np.array([c[k] for k in ("B", "T", "N", "H", "W", "OH", "OW", "D", "NFB", "NFR", "NG", "layers", "A")], dtype=np.int64),
               backbone=np.array(c["backbone"]), mode=np.array(c["mode"]), seed=np.int64(c["seed"]),
               pos_threshold=np.float64(c["pos_threshold"]), keys=np.array(list(model.state_dict().keys())),
               key_shapes=np.array([",".join(str(s) for s in v.shape) for v in model.state_dict().values()]),
               labels=labels.numpy(), activities=r32[0].numpy(), activities64=r64[0].numpy(),
               yard_activities=np.float64(gap(r32[0], r64[0])), loss=np.float64(r32[1]), loss64=np.float64(r64[1]),
               gcn_in64=r64[5]["gcn_in"].numpy(), gcn_out=r32[3].numpy(), gcn_out64=r64[3].numpy(), yard_gcn_out=np.float64(gap(r32[3], r64[3])),
               relation_graph=r32[4].numpy(), relation_graph64=r64[4].numpy(), yard_relation_graph=np.float64(gap(r32[4], r64[4])))
    margin, shares = float("inf"), []
    for l, (d32, d64, pos) in enumerate(zip(r32[5]["dist"], r64[5]["dist"], r64[5]["pos"])):
        m32, m64 = d32 > thr, d64 > thr
        assert bool((m32 == m64).all()), f"{name}: the fp32 and fp64 runs disagree on the mask of layer {l}"
        off = ~torch.eye(d64.shape[1], dtype=torch.bool)[None].expand_as(m64)
        margin = min(margin, float(((d64 - thr).abs() / thr)[off].min()))
        shares.append(float(m64.double().mean()))
        rec[f"mask.{l}"] = m64.numpy()
        rec[f"centres.{l}"] = pos.numpy()
    if c["layers"] > 1:
        assert not np.array_equal(rec["mask.0"], rec["mask.1"]), f"{name}: both layers see the same mask: the fixture would not pin layer 2"
    rec["min_margin"], rec["masked_share"] = np.float64(margin), np.float64(np.mean(shares))
    assert margin >= 1e-3, f"{name}: smallest |dist - thr| / thr = {margin:.2e} < 1e-3: pick another seed"
    assert all(0.15 <= s <= 0.85 for s in shares), f"{name}: masked share {shares} outside 0.15 .. 0.85"
    assert r64[1] >= 1e-2, f"{name}: loss {r64[1]:.2e}: the seeded label is already predicted with certainty and every gradient vanishes"
    g32, g64 = r32[2], r64[2]
    for k in sorted(g32):
        rec["gsum." + k] = np.float64(g32[k].double().sum().item())
        rec["gabs." + k] = np.float64(g32[k].double().abs().sum().item())
        rec["gsum64." + k] = np.float64(g64[k].sum().item())
        if not k.startswith("backbone.") and not (".fc_rn_phi_list." in k and k.endswith(".bias")):
            idx = grad_index(g32[k].numel())
            rec["yard." + k] = np.float64(gap(g32[k], g64[k]))
            rec["gmax64." + k] = np.float64(g64[k].abs().max().item())
            if len(idx) < g32[k].numel():
                rec["gidx." + k] = idx
            rec["g." + k] = g32[k].flatten()[idx].numpy()
            rec["g64." + k] = g64[k].flatten()[idx].numpy()
    path = os.path.join(out_dir, name + ".npz")
    np.savez_compressed(path, **rec)
    worst = max(float(v) for k, v in rec.items() if k.startswith("yard."))
    print(f"[arg] {name}: loss {r32[1]:.6f}, fp32-vs-fp64 activities {rec['yard_activities']:.1e} gcn {rec['yard_gcn_out']:.1e} "
          f"relation {rec['yard_relation_graph']:.1e} worst grad {worst:.1e}; mask margin {margin:.2e}, masked {np.mean(shares):.2f}; "
          f"{os.path.getsize(path) / 1024:.0f} KiB")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    sys.dont_write_bytecode = True
    from gen_golden import install_stubs
    install_stubs()
    sys.path.insert(0, a.ref)
    os.makedirs(a.out, exist_ok=True)
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    import importlib
    refim = importlib.import_module("infer_model")
    refarg = importlib.import_module("infer_module.ARG_infer_module")
    refcfg = importlib.import_module("config")
    for name, c in CASES.items():
        if a.only is None or a.only == name:
            case(name, c, refim, refarg, refcfg, a.out)
    print("ARG golden vectors written to", a.out)


if __name__ == "__main__":
    main()
