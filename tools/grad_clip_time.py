#!/usr/bin/env python3
"""What cfg.max_grad_norm costs (FusedAdam(max_grad_norm=...): din_grad_sqnorm_multi + din_grad_norm_finish + din_adam_step_multi_clip in
place of din_adam_step_multi), on one MI355X, over the benchmarked model: Dynamic_volleyball, Inception-v3 trunk, bf16, train_backbone.
  * the two norm launches alone over the model's whole parameter list: time per pair and achieved READ bandwidth (4 bytes per parameter;
    the launch never writes a gradient), beside the 6.29 TB/s a plain float4 copy reaches on this part (MI355X_MICROARCH.md);
  * the optimizer call, max_grad_norm = inf against None (None is the path without the feature, launch for launch);
  * the 4-clip and the 32-clip training step (uint8 clips resident on the device, forward + cross-entropy + backward + optimizer) the
    same way.
max_grad_norm = inf runs every launch of the clipped step and never changes a number, so both forms compute the same thing (lr = 0 keeps
the weights where they are).  The two forms ALTERNATE window by window in one process, so that clock and neighbour drift hit both alike.
A window is `--inner` calls between two device synchronisations after `--warmup` untimed windows; median / min / p90 / max of `--windows`
windows, per call, in ms.  A difference is reported next to the spread of the windows (p90 - min of each form): inside it, it is noise.
One JSON line per measurement, then the GPU clock of the box.  The figures are one run on a shared machine.

usage: python tools/grad_clip_time.py [--windows 15] [--inner 20] [--warmup 3] [--clips 4,32] [--out profiles/grad_clip_time.txt]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_TBS = 6.29                                                       # plain float4 copy, MI355X_MICROARCH.md


def clock():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        return [l.strip() for l in out.splitlines() if "sclk" in l.lower()][:1]
    except Exception as e:                                            # (informational only)
        return [f"unavailable: {e}"]


def timed(forms, warmup, windows, inner):
    """forms: name -> callable; window by window, one after the other"""
    times = {k: [] for k in forms}
    for it in range(warmup + windows):
        for k, fn in forms.items():
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


def difference(r, a, b):
    spread = max(r[a]["p90_ms"] - r[a]["min_ms"], r[b]["p90_ms"] - r[b]["min_ms"])
    d = r[a]["median_ms"] - r[b]["median_ms"]
    return {"difference_ms": round(d, 4), "spread_ms": round(spread, 4), "inside_the_spread": abs(d) <= spread}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--clips", default="4,32")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import bench
    from din_amd import _lib as L
    from din_amd.infer_model import Dynamic_volleyball
    from din_amd.optim import CHUNK, FusedAdam
    from din_amd.train_net_dynamic import set_bn_eval
    lib = L.load()
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
    numel = sum(p.numel() for p in params)
    shape = {"model": "Dynamic_volleyball", "backbone": "inv3", "dtype": "bf16", "train_backbone": True, "tensors": len(params), "parameters": numel}
    opts = {"none": FusedAdam(params, lr=0.0), "inf": FusedAdam(params, lr=0.0, max_grad_norm=float("inf"))}
    gen = torch.Generator().manual_seed(1)
    for p in params:
        p.grad = (1e-3 * torch.randn(p.shape, generator=gen)).to(dev)
    for o in opts.values():
        o.step()
    torch.cuda.synchronize()

    # ---- the two norm launches alone ----
    opt = opts["inf"]
    (tb,) = opt._tables.values()
    P = lambda t: C.c_void_p(t.data_ptr())                            # noqa: E731

    def norm_pair():
        L.check(lib.din_grad_sqnorm_multi(P(tb[2]), P(tb[3]), P(tb[4]), P(tb[5]), tb[6], CHUNK, P(opt._partials), None))
        L.check(lib.din_grad_norm_finish(P(opt._partials), tb[6], 1.0, float("inf"), P(opt._gstate), None))
    r = timed({"norm": norm_pair}, a.warmup, a.windows, a.inner)["norm"]
    tbs = 4 * numel / (r["median_ms"] * 1e-3) / 1e12
    emit({"tool": "grad_clip_time", "what": "din_grad_sqnorm_multi + din_grad_norm_finish", **shape, "workgroups": tb[6], **r,
          "read_bytes": 4 * numel, "read_TBps": round(tbs, 3), "plain_copy_TBps": COPY_TBS, "fraction_of_copy_rate": round(tbs / COPY_TBS, 3),
          "note": "back-to-back launches: the gradients (4 bytes per parameter) may stay in the 256 MiB last-level cache between calls"})

    # ---- the optimizer call ----
    r = timed({k: o.step for k, o in opts.items()}, a.warmup, a.windows, a.inner)
    for k in r:
        emit({"tool": "grad_clip_time", "what": "FusedAdam.step()", "max_grad_norm": k, **shape, **r[k]})
    emit({"tool": "grad_clip_time", "what": "FusedAdam.step(): inf - none", **difference(r, "inf", "none")})
    stats = opt.grad_stats()
    emit({"tool": "grad_clip_time", "what": "grad_stats() after the runs above", **stats})

    # ---- the training step ----
    for clips in [int(c) for c in a.clips.split(",") if c]:
        g = torch.Generator().manual_seed(2000)
        images = torch.randint(0, 256, (clips, T, 3, H, W), dtype=torch.uint8, generator=g).to(dev)
        boxes, labels = bench.synth_boxes_labels(clips, T, N, OH, OW, cfg.num_activities, seed=0)
        boxes, labels = boxes.to(dev), labels.to(dev)

        def step(o):
            o.zero_grad()
            F.cross_entropy(model((images, boxes))["activities"], labels).backward()
            o.step()
        r = timed({k: (lambda o=o: step(o)) for k, o in opts.items()}, min(a.warmup, 2), min(a.windows, 9), min(a.inner, 3))
        for k in r:
            emit({"tool": "grad_clip_time", "what": "training step", "clips": clips, "max_grad_norm": k, **shape, **r[k],
                  "clips_per_s": round(clips / r[k]["median_ms"] * 1e3, 1)})
        emit({"tool": "grad_clip_time", "what": "training step: inf - none", "clips": clips, **difference(r, "inf", "none")})
        del images
        torch.cuda.empty_cache()
    emit({"clock": clock()})
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("Gradient clipping inside the fused Adam step, max_grad_norm = inf against None in alternating windows "
                     "(tools/grad_clip_time.py), one MI355X, one run on a shared machine, per call in ms:\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
