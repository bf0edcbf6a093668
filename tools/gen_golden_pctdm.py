#!/usr/bin/env python3
"""Generate tests/golden/pctdm_*.npz by running the REFERENCE's PCTDM baseline (infer_module.pctdm_infer_module.PCTDM alone for the
`pctdm_module_*` cases, infer_model.PCTDM_volleyball for the `pctdm_vgg16_*` cases) on CPU, in fp32 and converted with .double().

Runs ONLY where the reference tree is.  Nothing of the reference is copied: its modules are imported under the dependency stubs of
tools/gen_golden.py (install_stubs), fed seeded weights / inputs (oracle.din_oracle synth_params / synth_inputs, `pctdm_params` /
`module_input` below) and the numbers they produce are stored.  The ~100 MB of parameters are never stored: the tests rebuild them, and the
inputs, from the stored geometry, seed and `extra_scale`.

Stored per case: geometry (`meta` = B, T, N, H, W, OH, OW, D, NFB, A), seed, mode, `extra_scale`; the state_dict key list and shapes; the
block's output (`out`, `out64`, [B*T, 2000]: the last-step features of both teams) and both attention vectors side by side (`gamma`,
`gamma64`, [B*T, N]) whole; the Bi-LSTM output and the pooled features in fp32 whole (`lstm_out`, `pooled`) and in fp64 at the evenly spaced
flat indices `idx.lstm_out` / `idx.pooled` (`lstm_out64`, `pooled64`); `winner` = np.packbits of "the reverse half won the max-pool" over
[B*T, N, 1000]; each stage's `yard_*` = max |fp32 - fp64| / max |fp64|; `min_gap` = min |h_fwd - h_bwd| and `lstm_err` = max |lstm_out32 -
lstm_out64|; `rowmax_mean`, `gate_mean`; the gradient of the block's input (`gx`, `gx64`, `yard_gx`, sampled like a parameter's); for every
parameter that receives a gradient gsum / gabs / gsum64 and, outside the backbone, `yard.*`, `gmax64.*` and the gradient in fp32 (`g.*`) and
fp64 (`g64.*`) at the flat indices `gidx.*` (at most GRAD_CAP).  Module cases: the loss is <out, cot> with the seeded `module_cot`.  Model
cases also hold labels, `activities`, `activities64`, `yard_activities`, both losses and the block's input in fp64 at `idx.x_in` (`x_in64`).

The generator asserts ("pick another seed" otherwise): (a) model cases: loss64 >= 1e-2; (b) the fp32 and fp64 runs pick the same max-pool
winner everywhere and min_gap >= 20 * lstm_err, so a kernel inside its 4-yard bar cannot flip a winner; (c) the mean row maximum of the
team softmax lies in [1.5 / (N/2), 0.9] -- with plain kaiming att_extra_weights it is too flat for a test to notice a wrong softmax axis,
so that one weight is multiplied by `extra_scale`, doubled from 1 until the condition holds; (d) the mean of the Bi-LSTM's i and f gates
lies in (0.2, 0.8).  Train-mode model cases run with dropout p = 0 and BatchNorm on running statistics (the trainer's set_bn_eval).

usage: python tools/gen_golden_pctdm.py --ref <reference tree> [--out tests/golden] [--only NAME] [--seed S]
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
PROBE_CAP = 8192
NUM_ACTIONS = 9
HID, NFB = 1000, 1024

VGG = dict(backbone="vgg16", H=96, W=160, OH=3, OW=5, D=512, A=8)
CASES = {
    "pctdm_module_g3_n4": dict(scope="module", B=1, T=3, N=4, mode="train", seed=901, **VGG),
    "pctdm_module_g2_n12": dict(scope="module", B=1, T=2, N=12, mode="train", seed=941, **VGG),
    "pctdm_vgg16_96x160": dict(scope="model", B=2, T=2, N=4, mode="train", seed=919, **VGG),
    "pctdm_vgg16_96x160_eval_n12": dict(scope="model", B=1, T=3, N=12, mode="eval", seed=1032, **VGG),
}
META = ("B", "T", "N", "H", "W", "OH", "OW", "D", "NFB", "A")


def module_shapes(prefix=""):
    s = {}
    for sfx in ("", "_reverse"):
        s[f"{prefix}Bi_Lstm.weight_ih_l0{sfx}"] = (4 * HID, NFB)
        s[f"{prefix}Bi_Lstm.weight_hh_l0{sfx}"] = (4 * HID, HID)
        s[f"{prefix}Bi_Lstm.bias_ih_l0{sfx}"] = (4 * HID,)
        s[f"{prefix}Bi_Lstm.bias_hh_l0{sfx}"] = (4 * HID,)
    for name, rows in (("att_source_weights", HID), ("att_context_weights", HID), ("att_extra_weights", 1)):
        s[f"{prefix}{name}.0.weight"] = (rows, HID)
        s[f"{prefix}{name}.0.bias"] = (rows,)
    s[f"{prefix}Intra_Group_LSTM.weight_ih_l0"] = (4 * HID, HID)
    s[f"{prefix}Intra_Group_LSTM.weight_hh_l0"] = (4 * HID, HID)
    s[f"{prefix}Intra_Group_LSTM.bias_ih_l0"] = (4 * HID,)
    s[f"{prefix}Intra_Group_LSTM.bias_hh_l0"] = (4 * HID,)
    return s


def model_shapes(backbone, D, T, A):
    shapes = {k: v for k, v in model_param_shapes(OracleCfg(backbone=backbone, emb_features=D, num_features_boxes=NFB)).items()
              if k.startswith(("backbone.", "fc_emb_1.", "nl_emb_1."))}
    shapes.update(module_shapes("pctdm."))
    shapes["pctdm_nl.weight"] = (T, 2 * HID)
    shapes["pctdm_nl.bias"] = (T, 2 * HID)
    shapes["fc_activities.weight"] = (A, 2 * HID)
    shapes["fc_activities.bias"] = (A,)
    shapes["fc_actions.weight"] = (NUM_ACTIONS, 2 * HID)
    shapes["fc_actions.bias"] = (NUM_ACTIONS,)
    return shapes


def pctdm_params(shapes, seed, extra_scale=1.0):
    """oracle.synth_params (kaiming weights), then seeded NON-TRIVIAL biases (Linear and LSTM) and LayerNorm affines outside the backbone: at
    their zeros / ones initial values a swapped or dropped term would pass; att_extra_weights.0.weight times `extra_scale`"""
    p = synth_params(shapes, seed=seed)
    g = torch.Generator().manual_seed(seed + 7)
    for k in sorted(p):
        if k.startswith("backbone."):
            continue
        leaf = k.split(".")[-1]
        if k.startswith("nl_") or "_nl." in k:
            r = torch.randn(p[k].shape, generator=g, dtype=torch.float64)
            p[k] = ((1.0 + 0.2 * r) if leaf == "weight" else 0.1 * r).float()
        elif leaf.startswith("bias"):
            p[k] = (0.1 * torch.randn(p[k].shape, generator=g, dtype=torch.float64)).float()
        if k.endswith("att_extra_weights.0.weight"):
            p[k] = (p[k].double() * extra_scale).float()
    return p


def module_input(B, T, N, seed):
    """shaped like the trunk's output: ReLU(LayerNorm(noise)), [B, T, N, 1024] fp32"""
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn((B, T, N, NFB), generator=g, dtype=torch.float64)
    return torch.relu(F.layer_norm(x, (NFB,))).float()


def module_cot(G, seed):
    g = torch.Generator().manual_seed(seed + 2)
    return torch.randn((G, 2 * HID), generator=g, dtype=torch.float64).float()


def probe_index(numel, cap=PROBE_CAP):
    return np.arange(numel, dtype=np.int64) if numel <= cap else np.linspace(0, numel - 1, cap).astype(np.int64)


def grad_index(numel):
    return probe_index(numel, GRAD_CAP)


def _bn_eval(m):
    if m.__class__.__name__.find("BatchNorm") != -1:
        m.eval()


def _run_block(pctdm, call):
    """call() runs a forward through `pctdm` (the reference's module); -> what its stages produced"""
    seen = {"gammas": [], "gates": None}
    orig = F.softmax

    def spy(x, *a, **k):
        r = orig(x, *a, **k)
        seen["gammas"].append(r.detach().clone())
        return r

    hooks = [pctdm.register_forward_pre_hook(lambda m, i: seen.__setitem__("x_in", i[0].detach().clone())),
             pctdm.Bi_Lstm.register_forward_hook(lambda m, i, o: seen.__setitem__("lstm_out", o[0].detach().clone())),
             pctdm.early_pooling.register_forward_hook(lambda m, i, o: seen.__setitem__("pooled", o.detach().clone()[:, 0])),
             pctdm.register_forward_hook(lambda m, i, o: seen.__setitem__("out", o.detach().clone()))]
    F.softmax = spy
    try:
        res = call()
    finally:
        F.softmax = orig
        for h in hooks:
            h.remove()
    assert len(seen["gammas"]) == 2
    seen["gamma"] = torch.cat(seen.pop("gammas"), dim=-1)                     # [G, N]: team 0 then team 1
    # the Bi-LSTM's i and f gates at the first step of the forward direction (h = 0 there): sigmoid of the input projection
    with torch.no_grad():
        bl = pctdm.Bi_Lstm
        x0 = seen["x_in"].reshape(-1, seen["x_in"].shape[-2], NFB)[:, 0]
        z = x0 @ bl.weight_ih_l0.t() + bl.bias_ih_l0 + bl.bias_hh_l0
        seen["gate_mean"] = float(torch.sigmoid(z[:, :2 * HID]).mean())
    return res, seen


def case(name, c, refim, refmod, refcfg, out_dir):
    cfg = refcfg.Config("volleyball")
    cfg.log_path = None
    cfg.backbone, cfg.image_size, cfg.out_size, cfg.emb_features = c["backbone"], (c["H"], c["W"]), (c["OH"], c["OW"]), c["D"]
    cfg.num_boxes, cfg.num_frames, cfg.batch_size = c["N"], c["T"], c["B"]
    cfg.num_features_boxes, cfg.num_activities, cfg.num_actions = NFB, c["A"], NUM_ACTIONS
    cfg.train_backbone, cfg.train_dropout_prob = True, 0.0
    G, N, is_model = c["B"] * c["T"], c["N"], c["scope"] == "model"
    torch.manual_seed(0)
    model = refim.PCTDM_volleyball(cfg) if is_model else refmod.PCTDM(cfg)
    shapes = model_shapes(c["backbone"], c["D"], c["T"], c["A"]) if is_model else module_shapes()
    block = (lambda m: m.pctdm) if is_model else (lambda m: m)

    def gap(a, b):
        return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-300))

    def run(model, dtype):
        model = model.to(dtype)
        if c["mode"] == "eval":
            model.eval()
        else:
            model.train()
            model.apply(_bn_eval)
        model.zero_grad()
        if is_model:
            images, boxes, labels = synth_inputs(c["B"], c["T"], N, c["H"], c["W"], c["OH"], c["OW"], c["A"], seed=c["seed"])
            model.dropout_global.p = 0.0
            keep = {}
            def grab(m, i):
                if i[0].requires_grad:
                    i[0].retain_grad()
                keep["x"] = i[0]
            h = model.pctdm.register_forward_pre_hook(grab)
            scores, seen = _run_block(model.pctdm, lambda: model((images.float().to(dtype), boxes.clone().to(dtype)))["activities"])
            h.remove()
            loss = F.cross_entropy(scores, labels)
            if not loss.requires_grad:                                 # (the extra_scale search: forward only)
                return loss.item(), {}, seen
            loss.backward()
            seen.update(scores=scores.detach(), gx=keep["x"].grad.detach().clone(), labels=labels)
        else:
            x = module_input(c["B"], c["T"], N, c["seed"]).to(dtype).requires_grad_(True)
            out, seen = _run_block(model, lambda: model(x))
            loss = (out * module_cot(G, c["seed"]).to(dtype)).sum()
            loss.backward()
            seen["gx"] = x.grad.detach().clone()
        grads = {k: v.grad.detach().clone() for k, v in model.named_parameters() if v.grad is not None}
        return loss.item(), grads, seen

    scale = 1.0
    while True:
        p = pctdm_params(shapes, c["seed"], scale)
        missing, unexpected = model.load_state_dict(p, strict=False)
        assert not unexpected and all("num_batches_tracked" in k for k in missing), (missing, unexpected)
        with torch.no_grad():
            m64 = copy.deepcopy(block(model)).double()
            xin = (run(copy.deepcopy(model), torch.float64)[2]["x_in"] if is_model and scale == 1.0 else None) if is_model else \
                module_input(c["B"], c["T"], N, c["seed"]).double()
        if is_model and scale == 1.0:
            x_model = xin
        if is_model:
            xin = x_model
        with torch.no_grad():
            _, s = _run_block(m64, lambda: m64(xin))
        rowmax = float(s["gamma"].reshape(G, 2, N // 2).max(-1).values.mean())
        if rowmax >= 1.5 / (N // 2):
            break
        scale *= 2.0
        assert scale <= 1024.0
    l32, g32, s32 = run(copy.deepcopy(model), torch.float32)
    l64, g64, s64 = run(copy.deepcopy(model), torch.float64)
    rowmax = float(s64["gamma"].reshape(G, 2, N // 2).max(-1).values.mean())
    assert 1.5 / (N // 2) <= rowmax <= 0.9, f"{name}: mean row maximum of the team softmax {rowmax:.3f} outside {1.5 / (N // 2):.3f} .. 0.9"
    assert 0.2 < s64["gate_mean"] < 0.8, f"{name}: mean i / f gate {s64['gate_mean']:.3f}: saturated"
    lo32, lo64 = s32["lstm_out"].reshape(G, N, 2, HID), s64["lstm_out"].reshape(G, N, 2, HID)
    w32, w64 = lo32[:, :, 1] > lo32[:, :, 0], lo64[:, :, 1] > lo64[:, :, 0]
    min_gap = float((lo64[:, :, 1] - lo64[:, :, 0]).abs().min())
    lstm_err = float((lo32.double() - lo64).abs().max())
    print(f"[pctdm] {name}: seed {c['seed']} scale {scale:g} row max {rowmax:.3f} min gap {min_gap:.2e} lstm err {lstm_err:.2e} "
          f"winners equal {bool(torch.equal(w32, w64))}")
    assert torch.equal(w32, w64), f"{name}: the fp32 and fp64 runs pick different max-pool winners: pick another seed"
    assert min_gap >= 20.0 * lstm_err, f"{name}: min |h_fwd - h_bwd| {min_gap:.2e} < 20 x {lstm_err:.2e}: pick another seed"
    assert torch.equal(s64["pooled"], torch.maximum(lo64[:, :, 0], lo64[:, :, 1]))
    rec = dict(meta=np.array([c[k] if k != "NFB" else NFB for k in META], dtype=np.int64), backbone=np.array(c["backbone"]),
               mode=np.array(c["mode"]), scope=np.array(c["scope"]), seed=np.int64(c["seed"]), extra_scale=np.float64(scale),
               keys=np.array(list(model.state_dict().keys())),
               key_shapes=np.array([",".join(str(s) for s in v.shape) for v in model.state_dict().values()]),
               winner=np.packbits(w64.numpy().reshape(-1)), min_gap=np.float64(min_gap), lstm_err=np.float64(lstm_err),
               rowmax_mean=np.float64(rowmax), gate_mean=np.float64(s64["gate_mean"]), loss=np.float64(l32), loss64=np.float64(l64))
    for k in ("out", "gamma"):
        rec[k], rec[k + "64"], rec["yard_" + k] = s32[k].reshape(G, -1).numpy(), s64[k].reshape(G, -1).numpy(), np.float64(gap(s32[k], s64[k]))
    for k in ("lstm_out", "pooled", "gx"):
        idx = probe_index(s64[k].numel(), GRAD_CAP if k == "gx" else PROBE_CAP)
        rec["idx." + k], rec["yard_" + k] = idx, np.float64(gap(s32[k], s64[k]))
        rec[k + "64"] = s64[k].flatten()[idx].numpy()
        rec["max64_" + k] = np.float64(s64[k].abs().max().item())
        rec[k] = s32[k].flatten()[idx].numpy() if k == "gx" else s32[k].numpy()
    if is_model:
        assert l64 >= 1e-2, f"{name}: loss {l64:.2e}: the seeded label is already predicted with certainty: pick another seed"
        idx = probe_index(s64["x_in"].numel())
        rec.update(labels=s64["labels"].numpy(), activities=s32["scores"].numpy(), activities64=s64["scores"].numpy(),
                   yard_activities=np.float64(gap(s32["scores"], s64["scores"])), x_in64=s64["x_in"].flatten()[idx].numpy(),
                   max64_x_in=np.float64(s64["x_in"].abs().max().item()))
        rec["idx.x_in"] = idx
    assert not any(k.startswith("fc_actions.") for k in g32)
    for k in sorted(g32):
        rec["gsum." + k] = np.float64(g32[k].double().sum().item())
        rec["gabs." + k] = np.float64(g32[k].double().abs().sum().item())
        rec["gsum64." + k] = np.float64(g64[k].sum().item())
        rec["gabs64." + k] = np.float64(g64[k].abs().sum().item())
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
    print(f"[pctdm] {name}: loss {l32:.6f}, fp32-vs-fp64 out {rec['yard_out']:.1e} lstm_out {rec['yard_lstm_out']:.1e} gamma "
          f"{rec['yard_gamma']:.1e} gx {rec['yard_gx']:.1e} worst grad {worst:.1e}; {os.path.getsize(path) / 1024:.0f} KiB")
    assert os.path.getsize(path) < (1 << 20)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="root of the reference tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--only", default=None)
    ap.add_argument("--seed", type=int, default=None, help="try another seed for the case named by --only")
    a = ap.parse_args()
    sys.dont_write_bytecode = True
    from gen_golden import install_stubs
    install_stubs()
    sys.path.insert(0, a.ref)
    os.makedirs(a.out, exist_ok=True)
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    import importlib
    refim = importlib.import_module("infer_model")
    refmod = importlib.import_module("infer_module.pctdm_infer_module")
    refcfg = importlib.import_module("config")
    for name, c in CASES.items():
        if a.only is None or a.only == name:
            if a.seed is not None:
                c = dict(c, seed=a.seed)
            case(name, c, refim, refmod, refcfg, a.out)
    print("PCTDM golden vectors written to", a.out)


if __name__ == "__main__":
    main()
