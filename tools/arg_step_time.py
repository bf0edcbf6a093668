#!/usr/bin/env python3
"""ARG step time at the shape of the reference's scripts/train_volleyball_stage2_arg.py (its vgg16 set-up): ARG_volleyball, vgg16, 720x1280
frames, T = 3, 12 boxes, NFB = NFG = 1024, NFR = 256, 16 graphs, frozen backbone, fused Adam.  Per batch size it reports
  * the full training step,
  * the GCN block alone, forward + backward, (a) through GCN_Module (one projection on the contraction kernel + csrc/arg_graph.hip) and
    (b) the same block written with torch matmul / softmax / layer_norm on the same device and the same parameters -- the library-call
    form a port would have had.  Nothing else could be a baseline: before this block existed the package could not run ARG at all.
Synthetic uint8 clips already on the device; every timed iteration ends in a device synchronise.  The two block forms alternate
inside one timing window.  One JSON line per measurement (median / min / p90 / max in ms), then the GPU clock of the box.

usage: python tools/arg_step_time.py [--steps 20] [--warmup 5] [--batches 2,32] [--block-only]"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def clock():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        return [l.strip() for l in out.splitlines() if "sclk" in l.lower()][:1]
    except Exception as e:                                            # (informational only)
        return [f"unavailable: {e}"]


def torch_block(gcn, x, boxes_flat, thr):
    """GCN_Module.forward in library calls (reference ARG_infer_module.py:46-89; the boxes are not written)"""
    B, TN, _ = x.shape
    NFR, NG = gcn.cfg.num_features_relation, gcn.cfg.num_graph
    b = boxes_flat.reshape(B, TN, 4)
    c = torch.stack([(b[..., 0] + b[..., 2]) / 2, (b[..., 1] + b[..., 3]) / 2], -1)
    mask = torch.cdist(c, c) > thr
    outs = []
    for i in range(NG):
        th, ph = gcn.fc_rn_theta_list[i](x), gcn.fc_rn_phi_list[i](x)
        s = torch.matmul(th, ph.transpose(1, 2)) / math.sqrt(NFR)
        r = torch.softmax(s.masked_fill(mask, -float("inf")), dim=2)
        v = gcn.fc_gcn_list[i](torch.matmul(r, x))
        outs.append(F.relu(gcn.nl_gcn_list[i](v)))
    return torch.stack(outs).sum(0)


def timed(fns, warmup, steps):
    """fns: {name: callable}; the forms ALTERNATE inside one window (a, b, a, b, ...), so that clock and neighbour drift on a shared host hits
    both alike; every call ends in a device synchronise"""
    times = {k: [] for k in fns}
    for it in range(warmup + steps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if it >= warmup:
                times[k].append((time.perf_counter() - t0) * 1e3)
    out = {}
    for k, t in times.items():
        t.sort()
        out[k] = {"median_ms": round(t[len(t) // 2], 3), "min_ms": round(t[0], 3), "p90_ms": round(t[int(0.9 * (len(t) - 1))], 3),
                  "max_ms": round(t[-1], 3), "steps": steps}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batches", default="2,32")
    ap.add_argument("--block-only", action="store_true")
    a = ap.parse_args()
    from din_amd.config import Config
    from din_amd.infer_model import ARG_volleyball
    from din_amd.optim import FusedAdam
    from din_amd.train_net_dynamic import SyntheticVolleyball
    dev = torch.device("cuda")
    for B in (int(v) for v in a.batches.split(",")):
        cfg = Config("volleyball")
        cfg.backbone, cfg.image_size, cfg.out_size, cfg.emb_features = "vgg16", (720, 1280), (22, 40), 512
        cfg.num_frames, cfg.batch_size, cfg.train_backbone, cfg.inference_module_name = 3, B, False, "arg_volleyball"
        model = ARG_volleyball(cfg).to(dev).train()
        shape = {"tool": "arg_step_time", "backbone": "vgg16", "image": [720, 1280], "batch": B, "T": 3, "N": 12, "NFB": 1024, "NFR": 256, "NG": 16}
        gcn = model.gcn_list[0]
        g = torch.Generator().manual_seed(B)
        x = torch.randn((B, 36, 1024), generator=g).to(dev).requires_grad_(True)
        ds = SyntheticVolleyball(cfg, length=B)
        boxes = torch.stack([ds[i][1] for i in range(B)]).to(dev)
        cot = torch.randn((B, 36, 1024), generator=g).to(dev)
        thr = cfg.pos_threshold * cfg.out_size[1]

        def run(block):
            for p in gcn.parameters():
                p.grad = None
            x.grad = None
            block().backward(cot)
        with torch.no_grad():
            d = (gcn(x, boxes.reshape(-1, 4))[0] - torch_block(gcn, x, boxes.reshape(-1, 4), thr)).abs().max().item()
        res = timed({"gcn block fwd+bwd, HIP path": lambda: run(lambda: gcn(x, boxes.reshape(-1, 4))[0]),
                     "gcn block fwd+bwd, torch matmul/softmax/layer_norm": lambda: run(lambda: torch_block(gcn, x, boxes.reshape(-1, 4), thr))},
                    a.warmup, a.steps)
        for what, r in res.items():
            print(json.dumps({**shape, "what": what, "max_abs_diff_between_forms": d, **r}), flush=True)
        if not a.block_only:
            opt = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=1e-4)
            images = torch.stack([ds[i][0] for i in range(B)]).to(dev)
            labels = torch.stack([ds[i][3] for i in range(B)])[:, 0].to(dev)

            def step():
                loss = F.cross_entropy(model((images, boxes))["activities"], labels)
                opt.zero_grad()
                loss.backward()
                opt.step()
            print(json.dumps({**shape, "what": "full training step", **timed({"step": step}, min(a.warmup, 3), min(a.steps, 10))["step"]}), flush=True)
            del opt
        del model
        torch.cuda.empty_cache()
    print(json.dumps({"clock": clock()}))


if __name__ == "__main__":
    main()
