#!/usr/bin/env python3
"""What the deterministic mode costs (DIN_DETERMINISTIC, ops.deterministic): the atomic and the ordered form of each kernel family the mode
replaces, and the frozen-backbone Dynamic_volleyball step with the option off and on, on one MI355X.
  * din_walk_bwd at B = 32, T = 10, N = 12, C = 1024, 3 x 3, ratio 1 (the launcher's calls: the offset / relation kernel, the feature
    gradient, the finish kernel);
  * din_layernorm_bwd at 3840 x 1024 (nl_emb_1: many short rows) and at 32 x 122880 (dpi_nl: few long rows);
  * din_colsum at 3840 x 1024 fp32 (the bias gradient of fc_emb_1);
  * the training step of Dynamic_volleyball (inv3 geometry: 26400 features per box, NFB 1024, T = 10, N = 12, B = 32, dropout 0.3, fused
    Adam) fed from box features resident on the device -- what a step is with every frame in the feature cache: fc_emb_1, the inference
    module, the head, the optimizer.
The two forms ALTERNATE window by window in one process, so that clock and neighbour drift hit both alike.  A window is `--inner` calls
between two device synchronisations (a kernel takes tens of microseconds: one call would time the synchronise), after `--warmup` untimed
windows; median / min / p90 / max of `--windows` windows, per call, in ms.  One JSON line per measurement, then the GPU clock of the box.
The figures are one run on a shared machine.

usage: python tools/deterministic_time.py [--windows 15] [--inner 20] [--warmup 3] [--no-step] [--out profiles/deterministic_time.txt]"""
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


def timed(fn, warmup, windows, inner):
    """fn under the option off ("atomic") and on ("ordered"), window by window; the option is set once per window, outside the timed part"""
    from din_amd import ops
    times = {"atomic": [], "ordered": []}
    for it in range(warmup + windows):
        for k in times:
            with ops.deterministic(k == "ordered"):
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
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from din_amd import _lib as L, infer_model, ops
    from din_amd.config import Config
    from din_amd.optim import FusedAdam
    lib = L.load()
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(0)
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    def measure(what, shape, call):
        for form, r in timed(call, a.warmup, a.windows, a.inner).items():
            emit({"tool": "deterministic_time", "what": what, "form": form, **shape, **r})

    P = lambda t: t.data_ptr()                                        # noqa: E731
    # ---- din_walk_bwd ----
    B, T, N, Cc, kh, kw = 32, 10, 12, 1024, 3, 3
    k2 = kh * kw
    x, gz = (torch.randn((B, T, N, Cc), generator=gen).to(dev) for _ in range(2))
    pred = torch.cat([torch.rand((B, T, N, 2 * k2), generator=gen) * 3 - 1.5, torch.rand((B, T, N, k2), generator=gen) * 4 - 2], dim=3).to(dev)
    z, av = torch.empty_like(x), torch.empty((B, T, N, k2), device=dev)
    L.check(lib.din_walk_fwd(P(x), P(pred), 3 * k2, B, T, N, Cc, kh, kw, 1, 1, 0, None, None, P(z), P(av), None, None, None))
    dx, dpred, scratch = torch.empty_like(x), torch.zeros_like(pred), torch.empty((Cc // 64) * B * T * N * 3 * k2, device=dev)
    measure("din_walk_bwd", {"B": B, "T": T, "N": N, "C": Cc, "kernel": [kh, kw], "ratio": 1},
            lambda: L.check(lib.din_walk_bwd(P(x), P(pred), 3 * k2, P(av), P(gz), B, T, N, Cc, kh, kw, 1, 1, 0, None, None, P(dx), P(dpred),
                                             P(scratch), None)))
    # ---- din_layernorm_bwd ----
    for rows, length in ((3840, 1024), (32, 122880)):
        lx, ldy = (torch.randn((rows, length), generator=gen).to(dev) for _ in range(2))
        gamma, beta = torch.ones(length, device=dev), torch.zeros(length, device=dev)
        ly, stats, ldx = torch.empty_like(lx), torch.empty((rows, 2), device=dev), torch.empty_like(lx)
        dg, db = torch.zeros(length, device=dev), torch.zeros(length, device=dev)
        L.check(lib.din_layernorm_fwd(P(lx), None, P(gamma), P(beta), 1e-5, P(ly), P(stats), rows, length, 1, 0.0, 0, None, None))
        measure("din_layernorm_bwd", {"rows": rows, "len": length},
                lambda: L.check(lib.din_layernorm_bwd(P(ldy), P(lx), None, P(gamma), P(ly), P(stats), P(ldx), P(dg), P(db), rows, length, 1, 0.0,
                                                      0, None, None)))
        del lx, ldy, ly, ldx
    # ---- din_colsum ----
    g = torch.randn((3840, 1024), generator=gen).to(dev)
    out = torch.empty(1024, device=dev)
    measure("din_colsum", {"rows": 3840, "c": 1024, "dtype": "fp32"}, lambda: L.check(lib.din_colsum(P(g), L.DIN_F32, 3840, 1024, 1024, 0, P(out), None)))
    # ---- the step from resident box features ----
    if not a.no_step:
        D, K, NFB = 1056, 5, 1024
        cfg = Config("volleyball")
        cfg.backbone, cfg.out_size, cfg.emb_features, cfg.image_size = "inv3", (87, 157), D, (720, 1280)
        cfg.num_frames, cfg.num_boxes, cfg.batch_size, cfg.num_features_boxes, cfg.num_features_gcn = T, N, B, NFB, NFB
        cfg.ST_kernel_size, cfg.sampling_ratio, cfg.num_DIM = [(3, 3)], [1], 1
        cfg.dynamic_sampling, cfg.scale_factor, cfg.beta_factor, cfg.train_backbone, cfg.train_dropout_prob = True, True, False, False, 0.3
        model = infer_model.Dynamic_volleyball(cfg).to(dev).train()
        feats = torch.relu(torch.randn((B, T, N, D * K * K), generator=gen)).to(dev)
        labels = torch.randint(0, cfg.num_activities, (B,), generator=gen).to(dev)
        # the trunk behind a full feature cache: the rows are there, the embedding layer reads them (infer_model.embed_boxes, FrameRefs branch)
        infer_model.embed_boxes = lambda m, images_in, boxes_in, n, fc: (ops.linear(images_in, fc.weight, fc.bias), None, None, None)
        opt = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=1e-4)

        def step():
            loss = F.cross_entropy(model((feats, None))["activities"], labels)
            opt.zero_grad()
            loss.backward()
            opt.step()
        shape = {"model": "Dynamic_volleyball", "B": B, "T": T, "N": N, "features_per_box": D * K * K, "NFB": NFB, "train_backbone": False}
        for form, r in timed(step, min(a.warmup, 2), min(a.windows, 9), min(a.inner, 5)).items():
            emit({"tool": "deterministic_time", "what": "training step from resident box features", "option": "on" if form == "ordered" else "off",
                  **shape, **r, "clips_per_s": round(B / r["median_ms"] * 1e3, 1)})
    emit({"clock": clock()})
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("Deterministic mode, atomic and ordered forms in alternating windows (tools/deterministic_time.py), one MI355X, one run on a "
                     "shared machine, per call in ms:\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
