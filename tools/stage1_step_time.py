#!/usr/bin/env python3
"""Stage-1 training-step time at the shape of the reference's scripts/train_volleyball_stage1.py: Basenet_volleyball, vgg16, 720x1280 frames,
batch 8, T = 1, 12 boxes, NFB 1024, dropout 0.3, fused Adam; fp32 and bf16 backbone.  Synthetic uint8 clips already on the device; each
timed step ends in a device synchronise.  Prints one JSON line per dtype (median / min / max step in ms) and the GPU clock of the box.

usage: python tools/stage1_step_time.py [--steps 10] [--warmup 3] [--dtypes fp32,bf16]"""
import argparse
import json
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtypes", default="fp32,bf16")
    a = ap.parse_args()
    from din_amd.base_model import Basenet_volleyball
    from din_amd.config import Config
    from din_amd.optim import FusedAdam
    from din_amd.train_net_dynamic import SyntheticVolleyball
    dev = torch.device("cuda")
    for dt in a.dtypes.split(","):
        cfg = Config("volleyball")
        cfg.backbone, cfg.image_size, cfg.out_size, cfg.emb_features = "vgg16", (720, 1280), (22, 40), 512
        cfg.num_frames, cfg.batch_size, cfg.train_backbone, cfg.backbone_dtype = 1, 8, True, dt
        model = Basenet_volleyball(cfg).to(dev).train()
        opt = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=1e-4)
        ds = SyntheticVolleyball(cfg, length=cfg.batch_size)
        batch = [torch.stack([ds[i][k] for i in range(cfg.batch_size)]).to(dev) for k in range(4)]
        images, boxes, actions_in, activities_in = batch
        w = torch.tensor([1., 1., 2., 3., 1., 2., 2., 0.2, 1.], device=dev)
        times = []
        for it in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            actions, activities = model((images, boxes))
            loss = F.cross_entropy(activities, activities_in[:, 0]) + F.cross_entropy(actions, actions_in[:, 0].reshape(-1), weight=w)
            opt.zero_grad()
            loss.backward()
            opt.step()
            torch.cuda.synchronize()
            if it >= a.warmup:
                times.append((time.perf_counter() - t0) * 1e3)
        times.sort()
        print(json.dumps({"tool": "stage1_step_time", "backbone": "vgg16", "dtype": dt, "image": [720, 1280], "batch": 8, "T": 1,
                          "steps": a.steps, "median_ms": round(times[len(times) // 2], 2), "min_ms": round(times[0], 2),
                          "max_ms": round(times[-1], 2), "loss": round(float(loss.item()), 5)}), flush=True)
        del model, opt
        torch.cuda.empty_cache()
    print(json.dumps({"clock": clock()}))


if __name__ == "__main__":
    main()
