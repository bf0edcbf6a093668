#!/usr/bin/env python3
"""AT step time at the shape of the reference's scripts/train_volleyball_stage2_at.py (its vgg16 set-up): AT_volleyball, vgg16, 720x1280
frames, T = 10, 12 boxes, B = 2, NFB = 1024, backbone trained, fused Adam.  It reports
  * the Actor-Transformer block alone (position embedding + Actor_Transformer), forward + backward, (a) through the modules of
    din_amd/infer_module/AT_infer_module.py (one Q/K/V contraction + csrc/actor_attention.hip + the FFN on the contraction kernel) and
    (b) the same arithmetic written as torch library calls on the same device and the same parameters -- the form a port would have had;
  * the full training step.
Synthetic uint8 clips already on the device.  Each timing is a window of `--inner` iterations between two device synchronisations (the
block takes tens of microseconds: a single iteration would time the synchronise), after `--warmup` untimed windows; the two block forms
alternate window by window, so that clock and neighbour drift hit both alike; median / min / p90 / max of `--windows` windows, per
iteration, in ms.  One JSON line per measurement, then the GPU clock of the box.

usage: python tools/at_step_time.py [--windows 15] [--inner 20] [--warmup 3] [--block-only] [--out profiles/at_step_time.txt]"""
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


def torch_block(pe, at, x, boxes, p):
    """Embfeature_PositionEmbedding + Actor_Transformer in library calls (reference AT_infer_module.py:66-96, :119-144)"""
    B, T, N, C = x.shape
    b = boxes.reshape(B, T, N, 4)
    cx = (b[..., 0] + b[..., 2]) / 2. * pe.image_size[1] / pe.out_size[1]
    cy = (b[..., 1] + b[..., 3]) / 2. * pe.image_size[0] / pe.out_size[0]
    dim_t = pe.dim_t(x.device)
    px, py = cx[..., None] / dim_t, cy[..., None] / dim_t
    px = torch.stack((px[..., 0::2].sin(), px[..., 1::2].cos()), dim=-1).flatten(-2)
    py = torch.stack((py[..., 0::2].sin(), py[..., 1::2].cos()), dim=-1).flatten(-2)
    h = (torch.cat((px, py), -1) + x).reshape(B * T, N, C)
    att = torch.softmax(torch.bmm(at.Q_W(h), at.K_W(h).transpose(1, 2)) / math.sqrt(C), dim=-1)
    h = at.layernorm1(h + F.dropout(torch.bmm(att, at.V_W(h)), p, True))
    f = at.FFN_linear2(F.dropout(F.relu(at.FFN_linear1(h)), p, True))
    return at.layernorm2(h + F.dropout(f, p, True))


def timed(fns, warmup, windows, inner):
    times = {k: [] for k in fns}
    for it in range(warmup + windows):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            if it >= warmup:
                times[k].append((time.perf_counter() - t0) * 1e3 / inner)
    out = {}
    for k, t in times.items():
        t.sort()
        out[k] = {"median_ms": round(t[len(t) // 2], 4), "min_ms": round(t[0], 4), "p90_ms": round(t[int(0.9 * (len(t) - 1))], 4),
                  "max_ms": round(t[-1], 4), "windows": windows, "iterations_per_window": inner}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--block-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from din_amd.config import Config
    from din_amd.infer_model import AT_volleyball
    from din_amd.optim import FusedAdam
    from din_amd.train_net_dynamic import SyntheticVolleyball
    dev = torch.device("cuda")
    B, T, N, C = 2, 10, 12, 1024
    cfg = Config("volleyball")
    cfg.backbone, cfg.image_size, cfg.out_size, cfg.emb_features = "vgg16", (720, 1280), (22, 40), 512
    cfg.num_frames, cfg.batch_size, cfg.train_backbone, cfg.inference_module_name = T, B, True, "at_volleyball"
    cfg.temporal_pooled_first = False
    model = AT_volleyball(cfg).to(dev).train()
    shape = {"tool": "at_step_time", "backbone": "vgg16", "image": [720, 1280], "batch": B, "T": T, "N": N, "NFB": C}
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    g = torch.Generator().manual_seed(B)
    x = torch.relu(torch.randn((B, T, N, C), generator=g)).to(dev).requires_grad_(True)
    ds = SyntheticVolleyball(cfg, length=B)
    boxes = torch.stack([ds[i][1] for i in range(B)]).to(dev)
    cot = torch.randn((B * T, N, C), generator=g).to(dev)
    params = list(model.AT.parameters())

    def run(block):
        for p in params:
            p.grad = None
        x.grad = None
        block().backward(cot)
    model.eval()
    with torch.no_grad():
        d = (model.AT(model.PE(x, boxes.reshape(-1, 4))) - torch_block(model.PE, model.AT, x, boxes, 0.0)).abs().max().item()
    model.train()
    res = timed({"AT block fwd+bwd, HIP path": lambda: run(lambda: model.AT(model.PE(x, boxes.reshape(-1, 4)), seeds=(1, 2, 3))),
                 "AT block fwd+bwd, torch library calls": lambda: run(lambda: torch_block(model.PE, model.AT, x, boxes, 0.1))},
                a.warmup, a.windows, a.inner)
    for what, r in res.items():
        emit({**shape, "what": what, "max_abs_diff_between_forms_p0": d, **r})
    if not a.block_only:
        opt = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=1e-4)
        images = torch.stack([ds[i][0] for i in range(B)]).to(dev)
        labels = torch.stack([ds[i][3] for i in range(B)])[:, 0].to(dev)

        def step():
            loss = F.cross_entropy(model((images, boxes))["activities"], labels)
            opt.zero_grad()
            loss.backward()
            opt.step()
        emit({**shape, "what": "full training step", **timed({"step": step}, min(a.warmup, 2), min(a.windows, 7), min(a.inner, 3))["step"]})
    emit({"clock": clock()})
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("AT block and step time (tools/at_step_time.py), one MI355X, per iteration in ms:\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
