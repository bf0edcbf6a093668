#!/usr/bin/env python3
"""Exact fp32 (DIN_F32) against the split-bf16 mode (DIN_F32_BF16X3: fp32 storage, three bf16 parts per operand on the bf16 matrix pipe),
same box, same process, same run:
  (a) one layer through the C ABI: Mixed_6's 7x1 192 -> 192 convolution at 24 frames of the 720x1280 geometry (43 x 78 maps) -- forward
      (bias + ReLU), data gradient (ReLU mask) and weight gradient (production epilogue: scale, <w, dW>, bias gradient), each mode on the
      same operands, the same packed banks and the same workspace;
  (b) the Inception-v3 fp32 training step at 8 clips (the shape of bench.py's parity_mode line: T = 3, 12 boxes, 720x1280 uint8 clips on
      the device, fwd + CE + bwd + fused Adam), cfg.backbone_dtype = 'fp32' against 'fp32_bf16x3', both models built in this process
      from the same seed.
Each timing is a window of `--inner` iterations between two device synchronisations after `--warmup` untimed windows; the two modes
alternate window by window, so that clock and neighbour drift hit both alike; median / min / p90 / max of `--windows` windows, per
iteration, in ms.  One JSON line per measurement, then the GPU clock of the box.  The GATE (exit status 1 when missed): the split layer's
forward median beats the exact median by more than the larger of the two p90 - min spreads.

usage: python tools/fp32_split_step_time.py [--windows 15] [--inner 10] [--warmup 3] [--layer-only] [--out profiles/fp32_split_step_time.txt]"""
import argparse
import ctypes as C
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from at_step_time import clock, timed  # noqa: E402


def layer_runs(L, lib, dtype, nb=24, h=43, w=78, c=192):
    """forward / dgrad / wgrad closures of the 7x1 layer under `dtype`, and the FLOPs of one of them"""
    d = L.ConvDesc()
    d.nb, d.h, d.w, d.cin, d.oh, d.ow, d.cout = nb, h, w, c, h, w, c
    d.kh, d.kw, d.sh, d.sw, d.ph, d.pw, d.dh, d.dw = 7, 1, 1, 1, 3, 0, 1, 1
    d.ldi, d.cioff, d.ldo, d.cooff, d.dtype, d.in_u8 = c, 0, c, 0, dtype, 0
    g = torch.Generator().manual_seed(7)
    dev = "cuda"
    x = torch.relu(torch.randn(nb, h, w, c, generator=g)).to(dev)
    gy = torch.randn(nb, h, w, c, generator=g).to(dev)
    wt = (torch.randn(c, c, 7, 1, generator=g) * (2.0 / (7 * c)) ** 0.5).to(dev)
    bias, scale = torch.randn(c, generator=g).to(dev), (torch.rand(c, generator=g) + 0.5).to(dev)
    y, dx, dw = torch.empty_like(x), torch.empty_like(x), torch.empty_like(wt)
    db, wdot = torch.zeros(c, device=dev), torch.zeros(c, device=dev)
    banks = []
    for t in (0, 1):
        wpk = torch.empty(lib.din_conv_packed_elems(C.byref(d), t), dtype=torch.float32, device=dev)
        L.check(lib.din_conv_pack_weights(C.byref(d), wt.data_ptr(), None, wpk.data_ptr(), t, None), "pack")
        banks.append(wpk)
    wsb = max(lib.din_conv_workspace_bytes(C.byref(d), k) for k in (0, 1, 2))
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
    buf = C.create_string_buffer(1024)
    names = {}
    for k, kind in enumerate(("forward", "dgrad", "wgrad")):
        lib.din_conv_kernel_names(C.byref(d), k, (L.CONV_BIAS | L.CONV_RELU) if k == 0 else (L.CONV_MASK if k == 1 else 0), c if k == 1 else 0, 0, buf, len(buf))
        names[kind] = buf.value.decode().split()

    def fwd():
        L.check(lib.din_conv_fwd(C.byref(d), x.data_ptr(), banks[0].data_ptr(), bias.data_ptr(), y.data_ptr(), L.CONV_BIAS | L.CONV_RELU, ws.data_ptr(), wsb, None), "fwd")

    def dgrad():
        L.check(lib.din_conv_dgrad(C.byref(d), gy.data_ptr(), banks[1].data_ptr(), dx.data_ptr(), x.data_ptr(), c, 0, L.CONV_MASK, ws.data_ptr(), wsb, None), "dgrad")

    def wgrad():
        L.check(lib.din_conv_wgrad(C.byref(d), x.data_ptr(), gy.data_ptr(), dw.data_ptr(), db.data_ptr(), scale.data_ptr(), wt.data_ptr(), wdot.data_ptr(), 2,
                                   ws.data_ptr(), wsb, None), "wgrad")
    keep = (x, gy, wt, bias, scale, y, dx, dw, db, wdot, banks, ws, d)
    return {"forward": fwd, "dgrad": dgrad, "wgrad": wgrad}, names, 2.0 * nb * h * w * c * c * 7, (y, dx, dw), keep


def make_step(dt, clips=8):
    sys.path.insert(0, ROOT)
    import bench
    from din_amd.infer_model import Dynamic_volleyball
    from din_amd.optim import FusedAdam
    from din_amd.train_net_dynamic import set_bn_eval
    T, N, H, W = 3, 12, 720, 1280
    backbone, _, (OH, OW), D = bench.WORKLOADS["inv3_fp32"]
    cfg = bench.make_cfg("inv3_fp32", T, N, H, W)
    cfg.backbone_dtype = dt
    torch.manual_seed(0)
    model = Dynamic_volleyball(cfg)
    bench.synth_weights(model)
    model = model.to("cuda").train()
    model.apply(set_bn_eval)
    opt = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=1e-4, weight_decay=0.0)
    g = torch.Generator().manual_seed(2000)
    images = torch.randint(0, 256, (clips, T, 3, H, W), dtype=torch.uint8, generator=g).to("cuda")
    boxes, labels = bench.synth_boxes_labels(clips, T, N, OH, OW, cfg.num_activities, seed=0)
    boxes, labels = boxes.to("cuda"), labels.to("cuda")
    last = {}

    def step():
        opt.zero_grad()
        loss = F.cross_entropy(model((images, boxes))["activities"], labels)
        loss.backward()
        opt.step()
        last["loss"] = loss
    return step, last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layer-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from din_amd import _lib as L
    lib = L.load()
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    shape = {"tool": "fp32_split_step_time", "layer": "7x1 192->192, 24 x 43 x 78 (Mixed_6 at 720x1280)"}
    runs = {m: layer_runs(L, lib, dt) for m, dt in (("exact", L.DIN_F32), ("split", L.DIN_F32_BF16X3))}
    gate_ok = True
    for kind in ("forward", "dgrad", "wgrad"):
        res = timed({m: runs[m][0][kind] for m in ("exact", "split")}, a.warmup, a.windows, a.inner)
        torch.cuda.synchronize()
        i = ("forward", "dgrad", "wgrad").index(kind)
        ex, sp = runs["exact"][3][i].double(), runs["split"][3][i].double()
        diff = float((ex - sp).abs().max() / ex.abs().max())
        for m in ("exact", "split"):
            r = res[m]
            emit({**shape, "what": f"{kind}, {m}", "kernels": runs[m][1][kind], "tflops_at_median": round(runs[m][2] / (r["median_ms"] * 1e-3) / 1e12, 1), **r})
        e, s = res["exact"], res["split"]
        spread = max(e["p90_ms"] - e["min_ms"], s["p90_ms"] - s["min_ms"])
        rec = {**shape, "what": f"{kind}, exact / split", "speedup_at_median": round(e["median_ms"] / s["median_ms"], 3),
               "median_gain_ms": round(e["median_ms"] - s["median_ms"], 4), "larger_p90_minus_min_ms": round(spread, 4),
               "max_abs_diff_split_vs_exact_over_max": float(f"{diff:.3e}")}
        if kind == "forward":
            gate_ok = e["median_ms"] - s["median_ms"] > spread
            rec["gate_forward_gain_exceeds_spread"] = gate_ok
        emit(rec)
    if not a.layer_only:
        steps = {m: make_step(dt) for m, dt in (("exact", "fp32"), ("split", "fp32_bf16x3"))}
        res = timed({m: steps[m][0] for m in steps}, min(a.warmup, 1), min(a.windows, 7), min(a.inner, 3))
        for m in steps:
            r = res[m]
            emit({"tool": "fp32_split_step_time", "what": f"Inception-v3 fp32 training step, 8 clips, {m}", "clips_per_s_at_median": round(8 / (r["median_ms"] * 1e-3), 2),
                  "final_loss": round(float(steps[m][1]["loss"].item()), 5), **r})
        emit({"tool": "fp32_split_step_time", "what": "training step, exact / split", "speedup_at_median": round(res["exact"]["median_ms"] / res["split"]["median_ms"], 3)})
    emit({"clock": clock()})
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("exact fp32 vs split-bf16 (tools/fp32_split_step_time.py), one MI355X, one run, per iteration in ms:\n" + "\n".join(lines) + "\n")
    return 0 if gate_ok else 1


if __name__ == "__main__":
    sys.exit(main())
