#!/usr/bin/env python3
"""Generate tests/golden/at_*.npz by running the REFERENCE's Actor-Transformer baseline (infer_model.AT_volleyball with
infer_module.AT_infer_module's Embfeature_PositionEmbedding and Actor_Transformer) on CPU, in fp32 and converted with .double().

Runs ONLY where the reference tree is.  Nothing of the reference is copied: its modules are imported under the dependency stubs of
tools/gen_golden.py (install_stubs), fed seeded weights / inputs (oracle.din_oracle synth_params / synth_inputs, `at_params` below) and the
numbers they produce are stored.  The tests rebuild weights and inputs from the stored geometry and seeds with `at_params` / synth_inputs.

Stored per case: geometry (`meta`), seeds, mode, `pooled` (cfg.temporal_pooled_first); the state_dict key list and shapes; labels;
`activities` (fp32), `activities64`, their gap (`yard_activities`); both losses; the trunk's output that enters the position embedding
(`pe_in64`); the position-embedded features (`pe`, `pe64`, `yard_pe`; [B, T, N, NFB], before the mean over T), the attention matrix (`att`,
`att64`, `yard_att`; [G, N, N]) and the Actor_Transformer output (`at_out`, `at_out64`, `yard_at_out`; [G, N, NFB]); `rowmax_mean` = mean
over rows of the largest attention weight; for every parameter that receives a gradient gsum / gabs / gsum64; for every such NON-backbone
parameter `yard.*` (fp32-vs-fp64 gap of the whole gradient, relative to its largest entry), `gmax64.*` (that largest entry) and the gradient
itself in fp32 (`g.*`) and fp64 (`g64.*`) -- whole when it has at most GRAD_CAP elements, else at the evenly spaced flat indices `gidx.*`.
Every gap is max |fp32 - fp64| / max |fp64|.  fc_actions is in the key list and has no gradient entries: the reference computes its scores
and throws them away.

The generator asserts (a) loss64 >= 1e-2: a seed whose label is already predicted with certainty leaves gradients of pure rounding noise;
(b) 1.5 / N <= rowmax_mean <= 0.9: the softmax is neither uniform (a missing row structure would pass) nor one-hot (a missing 1 / sqrt(C)
would pass); (c) the fp32 and fp64 runs pick the same actor at every (frame, channel) of the head's max over N, so the gradients of the two
runs flow through the same elements.  Otherwise pick another seed.  Train-mode cases run with the three dropout modules' p set to 0 on the
instance and BatchNorm on running statistics (the trainer's set_bn_eval).

usage: python tools/gen_golden_at.py --ref <reference tree> [--out tests/golden] [--only NAME]
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
NUM_ACTIONS = 9

VGG = dict(backbone="vgg16", H=96, W=160, OH=3, OW=5, D=512, A=8)
CASES = {
    "at_vgg16_96x160": dict(B=2, T=3, N=4, NFB=64, mode="train", pooled=False, seed=700, **VGG),
    "at_vgg16_96x160_pooled": dict(B=2, T=3, N=4, NFB=64, mode="train", pooled=True, seed=710, **VGG),
    "at_vgg16_96x160_eval_n12": dict(B=2, T=3, N=12, NFB=128, mode="eval", pooled=False, seed=702, **VGG),
    "at_inv3_139x203": dict(B=1, T=3, N=6, NFB=64, mode="train", pooled=False, seed=703,
                            backbone="inv3", H=139, W=203, OH=15, OW=23, D=1056, A=8),      # the geometry of stage1_inv3_139x203
}
META = ("B", "T", "N", "H", "W", "OH", "OW", "D", "NFB", "A")


def at_shapes(backbone, D, K, NFB, A):
    shapes = {k: v for k, v in model_param_shapes(OracleCfg(backbone=backbone, emb_features=D, num_features_boxes=NFB)).items()
              if k.startswith(("backbone.", "fc_emb_1.", "nl_emb_1."))}
    for name in ("Q_W", "K_W", "V_W"):
        shapes[f"AT.{name}.weight"] = (NFB, NFB)
    for name in ("layernorm1", "layernorm2"):
        shapes[f"AT.{name}.weight"] = (NFB,)
        shapes[f"AT.{name}.bias"] = (NFB,)
    for name in ("FFN_linear1", "FFN_linear2"):
        shapes[f"AT.{name}.weight"] = (NFB, NFB)
        shapes[f"AT.{name}.bias"] = (NFB,)
    shapes["fc_activities.weight"] = (A, NFB)
    shapes["fc_activities.bias"] = (A,)
    shapes["fc_actions.weight"] = (NUM_ACTIONS, NFB)
    shapes["fc_actions.bias"] = (NUM_ACTIONS,)
    return shapes


def at_params(shapes, seed):
    """oracle.synth_params (kaiming weights), then seeded NON-TRIVIAL Linear biases and LayerNorm affines outside the backbone: at their
    zeros / ones initial values a swapped or dropped term would pass"""
    p = synth_params(shapes, seed=seed)
    g = torch.Generator().manual_seed(seed + 7)
    for k in sorted(p):
        if k.startswith("backbone."):
            continue
        if "layernorm" in k or k.startswith("nl_"):
            r = torch.randn(p[k].shape, generator=g, dtype=torch.float64)
            p[k] = ((1.0 + 0.2 * r) if k.endswith("weight") else 0.1 * r).float()
        elif k.endswith(".bias"):
            p[k] = (0.1 * torch.randn(p[k].shape, generator=g, dtype=torch.float64)).float()
    return p


def grad_index(numel):
    return np.arange(numel, dtype=np.int64) if numel <= GRAD_CAP else np.linspace(0, numel - 1, GRAD_CAP).astype(np.int64)


def _bn_eval(m):
    if m.__class__.__name__.find("BatchNorm") != -1:
        m.eval()


def _run(model, c, images, boxes, labels, dtype):
    model = model.to(dtype)
    if c["mode"] == "eval":
        model.eval()
    else:
        model.train()
        model.apply(_bn_eval)
    for m in (model.AT.dropout1, model.AT.dropout2, model.AT.FFN_dropout):
        m.p = 0.0
    model.zero_grad()
    seen = {}
    orig = torch.softmax

    def spy(x, *a, **k):
        r = orig(x, *a, **k)
        seen["att"] = r.detach().clone()
        return r

    hooks = [model.PE.register_forward_hook(lambda m, i, o: seen.update(pe_in=i[0].detach().clone(), pe=o.detach().clone())),
             model.AT.register_forward_hook(lambda m, i, o: seen.__setitem__("at_out", o.detach().clone()))]
    torch.softmax = spy
    try:
        scores = model((images.to(dtype), boxes.clone().to(dtype)))["activities"]
    finally:
        torch.softmax = orig
        for h in hooks:
            h.remove()
    loss = F.cross_entropy(scores, labels)
    loss.backward()
    grads = {k: v.grad.detach().clone() for k, v in model.named_parameters() if v.grad is not None}
    return scores.detach(), loss.item(), grads, seen


def case(name, c, refim, refcfg, out_dir):
    cfg = refcfg.Config("volleyball")
    cfg.log_path = None
    cfg.backbone, cfg.image_size, cfg.out_size, cfg.emb_features = c["backbone"], (c["H"], c["W"]), (c["OH"], c["OW"]), c["D"]
    cfg.num_boxes, cfg.num_frames, cfg.batch_size = c["N"], c["T"], c["B"]
    cfg.num_features_boxes, cfg.num_activities, cfg.num_actions = c["NFB"], c["A"], NUM_ACTIONS
    cfg.temporal_pooled_first, cfg.train_backbone = c["pooled"], True
    torch.manual_seed(0)
    model = refim.AT_volleyball(cfg)
    p = at_params(at_shapes(c["backbone"], c["D"], cfg.crop_size[0], c["NFB"], c["A"]), c["seed"])
    missing, unexpected = model.load_state_dict(p, strict=False)
    assert not unexpected and all("num_batches_tracked" in k for k in missing), (missing, unexpected)
    images, boxes, labels = synth_inputs(c["B"], c["T"], c["N"], c["H"], c["W"], c["OH"], c["OW"], c["A"], seed=c["seed"])
    r32 = _run(model, c, images.float(), boxes, labels, torch.float32)
    r64 = _run(copy.deepcopy(model), c, images.float(), boxes, labels, torch.float64)

    def gap(a, b):
        return float((a.double() - b).abs().max() / (b.abs().max() + 1e-300))

    s32, s64 = r32[3], r64[3]
    rec = dict(meta=np.array([c[k] for k in META], dtype=np.int64), backbone=np.array(c["backbone"]), mode=np.array(c["mode"]),
               pooled=np.bool_(c["pooled"]), seed=np.int64(c["seed"]), keys=np.array(list(model.state_dict().keys())),
               key_shapes=np.array([",".join(str(s) for s in v.shape) for v in model.state_dict().values()]),
               labels=labels.numpy(), activities=r32[0].numpy(), activities64=r64[0].numpy(),
               yard_activities=np.float64(gap(r32[0], r64[0])), loss=np.float64(r32[1]), loss64=np.float64(r64[1]),
               pe_in64=s64["pe_in"].numpy())
    for k in ("pe", "att", "at_out"):
        rec[k], rec[k + "64"], rec["yard_" + k] = s32[k].numpy(), s64[k].numpy(), np.float64(gap(s32[k], s64[k]))
    rowmax = float(s64["att"].max(dim=-1).values.mean())
    rec["rowmax_mean"] = np.float64(rowmax)
    assert r64[1] >= 1e-2, f"{name}: loss {r64[1]:.2e}: the seeded label is already predicted with certainty: pick another seed"
    assert 1.5 / c["N"] <= rowmax <= 0.9, f"{name}: mean row maximum of the attention {rowmax:.3f} outside {1.5 / c['N']:.3f} .. 0.9: pick another seed"
    assert torch.equal(s32["at_out"].argmax(dim=1), s64["at_out"].argmax(dim=1)), \
        f"{name}: the fp32 and fp64 runs pick different actors in the head's max over N: pick another seed"
    g32, g64 = r32[2], r64[2]
    assert not any(k.startswith("fc_actions.") for k in g32)
    for k in sorted(g32):
        rec["gsum." + k] = np.float64(g32[k].double().sum().item())
        rec["gabs." + k] = np.float64(g32[k].double().abs().sum().item())
        rec["gsum64." + k] = np.float64(g64[k].sum().item())
        if not k.startswith("backbone."):
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
    print(f"[at] {name}: loss {r32[1]:.6f}, fp32-vs-fp64 activities {rec['yard_activities']:.1e} pe {rec['yard_pe']:.1e} att "
          f"{rec['yard_att']:.1e} at_out {rec['yard_at_out']:.1e} worst grad {worst:.1e}; row max {rowmax:.3f}; "
          f"{os.path.getsize(path) / 1024:.0f} KiB")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="root of the reference tree")
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
    refcfg = importlib.import_module("config")
    for name, c in CASES.items():
        if a.only is None or a.only == name:
            case(name, c, refim, refcfg, a.out)
    print("AT golden vectors written to", a.out)


if __name__ == "__main__":
    main()
