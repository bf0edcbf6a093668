#!/usr/bin/env python3
"""What conv_halo_rf_kernel (the filter-stationary halo kernel of the narrow 3x3 layers, csrc/conv_halo_rf.hip) is worth in the training
step, on one MI355X, over the benchmarked model: Dynamic_volleyball, Inception-v3 trunk, bf16, train_backbone, uint8 clips resident on the
device, forward + cross-entropy + backward + fused Adam (lr = 0 keeps the weights where they are).

DIN_CONV_HALO_RF=0 (every launch on the kernels din_conv_fwd / din_conv_dgrad choose: the step without the feature, launch for launch)
against the option unset (the planner's rule) ALTERNATE window by window in one process, so that clock and neighbour drift hit both
alike.  A window is `--inner` steps between two device synchronisations after `--warmup` untimed windows; median / min / max of `--windows`
windows, per step, in ms.  A difference is reported next to the spread of the windows (max - min of each form): inside it, it is noise.
One JSON line per measurement.  The figures are one run on a shared machine.

--option DIN_CONV_HALO_RF5 toggles the 5x5 family instead (conv_halo_rf5_kernel, csrc/conv_halo_rf5.hip), everything else the same.

usage: python tools/halo_rf_time.py [--option DIN_CONV_HALO_RF] [--windows 9] [--inner 3] [--warmup 2] [--clips 32,4] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--clips", default="32,4")
    ap.add_argument("--out", default=None)
    ap.add_argument("--option", default="DIN_CONV_HALO_RF", choices=["DIN_CONV_HALO_RF", "DIN_CONV_HALO_RF5"], help="the kernel family toggled")
    a = ap.parse_args()
    import bench
    from din_amd import _lib as L
    from din_amd.infer_model import Dynamic_volleyball
    from din_amd.optim import FusedAdam
    from din_amd.train_net_dynamic import set_bn_eval
    dev = torch.device("cuda")
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    T, N, H, W = 3, 12, 720, 1280
    _, _, (OH, OW), _ = bench.WORKLOADS["inv3_bf16"]
    cfg = bench.make_cfg("inv3_bf16", T, N, H, W)
    torch.manual_seed(0)
    model = Dynamic_volleyball(cfg)
    bench.synth_weights(model)
    model = model.to(dev).train()
    model.apply(set_bn_eval)
    params = [p for p in model.parameters() if p.requires_grad]
    opt = FusedAdam(params, lr=0.0)
    forms = {"off": "0", "unset": None}
    for clips in [int(c) for c in a.clips.split(",") if c]:
        g = torch.Generator().manual_seed(2000)
        images = torch.randint(0, 256, (clips, T, 3, H, W), dtype=torch.uint8, generator=g).to(dev)
        boxes, labels = bench.synth_boxes_labels(clips, T, N, OH, OW, cfg.num_activities, seed=0)
        boxes, labels = boxes.to(dev), labels.to(dev)

        def step():
            opt.zero_grad()
            F.cross_entropy(model((images, boxes))["activities"], labels).backward()
            opt.step()

        times = {k: [] for k in forms}
        for it in range(a.warmup + a.windows):
            for k, v in forms.items():
                L.set_option(a.option, v)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.inner):
                    step()
                torch.cuda.synchronize()
                if it >= a.warmup:
                    times[k].append((time.perf_counter() - t0) * 1e3 / a.inner)
        L.set_option(a.option, None)
        r = {}
        for k, t in times.items():
            t.sort()
            r[k] = {"median_ms": round(t[len(t) // 2], 4), "min_ms": round(t[0], 4), "max_ms": round(t[-1], 4), "windows": a.windows, "steps_per_window": a.inner}
            emit({"tool": "halo_rf_time", "what": "training step", "clips": clips, a.option: k, **r[k],
                  "clips_per_s": round(clips / r[k]["median_ms"] * 1e3, 1)})
        spread = max(r[k]["max_ms"] - r[k]["min_ms"] for k in r)
        d = r["unset"]["median_ms"] - r["off"]["median_ms"]
        emit({"tool": "halo_rf_time", "what": "training step: unset - off", "clips": clips, "difference_ms": round(d, 4), "spread_ms": round(spread, 4),
              "inside_the_spread": abs(d) <= spread})
        del images
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
