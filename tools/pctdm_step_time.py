#!/usr/bin/env python3
"""PCTDM step time at the shape of the reference's scripts/train_volleyball_stage2_pctdm.py (its commented vgg16 set-up: the default res18
trunk is not ported): PCTDM_volleyball, vgg16, 720x1280 frames, T = 10, 12 boxes, B = 2, NFB = 1024, backbone trained, fused Adam.  It reports
  * the PCTDM block alone, forward + backward, (a) through din_amd/infer_module/pctdm_infer_module.py (the input projections on the
    contraction kernel, csrc/lstm.hip one launch per position, csrc/pctdm_attention.hip) and (b) the same arithmetic written as torch library
    calls on the same device and the same parameters (torch.nn.LSTM, max, softmax) -- the form a port would have had;
  * the full training step.
Synthetic uint8 clips already on the device.  Each timing is a window of `--inner` iterations between two device synchronisations, after
`--warmup` untimed windows; the two block forms alternate window by window, so that clock and neighbour drift hit both alike; median / min /
p90 / max of `--windows` windows, per iteration, in ms.  One JSON line per measurement, then the GPU clock of the box.

usage: python tools/pctdm_step_time.py [--windows 15] [--inner 10] [--warmup 3] [--block-only] [--out profiles/pctdm_step_time.txt]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from at_step_time import clock, timed  # noqa: E402


def torch_block(m, x):
    """PCTDM in library calls (reference pctdm_infer_module.py:69-133 with its default switches)"""
    B, T, N, C = x.shape
    G, H = B * T, m.hidden_size
    lstm_out, _ = m.Bi_Lstm(x.reshape(G, N, C))
    pooled = torch.maximum(lstm_out[..., :H], lstm_out[..., H:])
    ctx = m.att_context_weights(pooled.mean(1))
    score = m.att_extra_weights(torch.tanh(m.att_source_weights(pooled) + ctx[:, None]))[..., 0]
    gamma = torch.softmax(score.reshape(G, 2, N // 2), -1).reshape(G, N, 1)
    feas, _ = m.Intra_Group_LSTM((pooled + pooled * gamma).reshape(2 * G, N // 2, H))
    return feas[:, -1].reshape(G, 2 * H)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--block-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from din_amd.config import Config
    from din_amd.infer_model import PCTDM_volleyball
    from din_amd.optim import FusedAdam
    from din_amd.train_net_dynamic import SyntheticVolleyball
    dev = torch.device("cuda")
    B, T, N, C = 2, 10, 12, 1024
    cfg = Config("volleyball")
    cfg.backbone, cfg.image_size, cfg.out_size, cfg.emb_features = "vgg16", (720, 1280), (22, 40), 512
    cfg.num_frames, cfg.batch_size, cfg.train_backbone, cfg.inference_module_name = T, B, True, "pctdm_volleyball"
    model = PCTDM_volleyball(cfg).to(dev).train()
    shape = {"tool": "pctdm_step_time", "backbone": "vgg16", "image": [720, 1280], "batch": B, "T": T, "N": N, "NFB": C}
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    g = torch.Generator().manual_seed(B)
    x = torch.relu(torch.randn((B, T, N, C), generator=g)).to(dev).requires_grad_(True)
    cot = torch.randn((B * T, 2000), generator=g).to(dev)
    params = list(model.pctdm.parameters())

    def run(block):
        for p in params:
            p.grad = None
        x.grad = None
        block().backward(cot)
    with torch.no_grad():
        d = (model.pctdm(x) - torch_block(model.pctdm, x)).abs().max().item()
    res = timed({"PCTDM block fwd+bwd, HIP path": lambda: run(lambda: model.pctdm(x)),
                 "PCTDM block fwd+bwd, torch library calls": lambda: run(lambda: torch_block(model.pctdm, x))},
                a.warmup, a.windows, a.inner)
    for what, r in res.items():
        emit({**shape, "what": what, "max_abs_diff_between_forms": d, **r})
    if not a.block_only:
        ds = SyntheticVolleyball(cfg, length=B)
        boxes = torch.stack([ds[i][1] for i in range(B)]).to(dev)
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
            fh.write("PCTDM block and step time (tools/pctdm_step_time.py), one MI355X, per iteration in ms:\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
