#!/usr/bin/env python3
"""Map cache timings (cfg.map_cache_gb; din_amd/feature_cache.py: MapCache) on one MI355X.

1. The gather launch for `--rows` VGG16 maps of 22 x 40 x 512 fp32 (1 802 240 bytes, trailer 16 bytes): din_feat_rows over computed maps
   (fm + slot + trailer), din_feat_rows over resident maps (gather + trailer comparison), and a plain din_copy_rows_u8 of the same rows.
2. The Dynamic_TCE_volleyball training step (forward + loss + backward + fused Adam) at the launcher's geometry -- 720 x 1280, out_size
   22 x 40, T = 10, frozen VGG16, `--batch` clips -- under backbone_dtype 'fp32' and 'bf16': fed FrameRefs whose frames are all resident
   (no trunk launch) against the same step fed the images tensor, which is the step with map_cache_gb = 0.
3. Feed rate, in clips/s, of training epochs of dynamic_tce_volleyball through train_net_dynamic.train_volleyball over a throw-away tree
   of synthetic 1280x720 JPEGs the tool writes itself (tools/frame_feed_time.py: write_tree; three frames a clip, batch size 2): the
   first cached epoch once, then epochs with the cache off and later cached epochs.

Everywhere the forms ALTERNATE window by window inside one process; median / min / p90 / max per form.  One JSON line per measurement,
then the GPU clock.  usage: python tools/map_cache_time.py [--out profiles/map_cache_time.txt] [--skip-kernel] [--skip-step] [--skip-feed]
[--windows 15] [--inner 5] [--rows 320] [--batch 8] [--step-windows 7] [--step-inner 2] [--clips 64] [--epochs 5] [--cache-gb 4]"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from at_step_time import clock, timed  # noqa: E402
from frame_feed_time import write_tree  # noqa: E402

OH, OW, C = 22, 40, 512
RB, TB = OH * OW * C * 4, 16


def kernel_timings(a, emit):
    from din_amd import ops
    from din_amd.feature_cache import MapCache
    dev = torch.device("cuda")
    R = a.rows
    g = torch.Generator(device=dev).manual_seed(0)
    computed = torch.randn((R, RB // 4), device=dev, generator=g)
    trailers = torch.from_numpy(MapCache("cpu", (OH, OW, C), 4, 0).trailers(np.arange(R))).to(dev)
    out = torch.empty((R, RB // 4), device=dev)
    slots = torch.zeros(R * (RB + TB), dtype=torch.uint8, device=dev)
    order = np.random.default_rng(0).permutation(R)                       # row i lives in slot order[i]
    tab = lambda v: torch.tensor([int(x) for x in v], dtype=torch.int64, device=dev)
    src_rows = tab(computed.data_ptr() + i * RB for i in range(R))
    dst_rows = tab(out.data_ptr() + i * RB for i in range(R))
    slot_of = tab(slots.data_ptr() + int(order[i]) * (RB + TB) for i in range(R))
    trailer_of = slot_of + RB
    zeros = torch.zeros(R, dtype=torch.int64, device=dev)
    flags = torch.zeros(R, dtype=torch.uint8, device=dev)
    forms = {"computed maps: din_feat_rows (fm + slot + trailer)":
             (lambda: ops.feat_rows(src_rows, dst_rows, RB, slot_of, zeros, trailers, flags, TB), R * (3 * RB + 2 * TB)),
             "resident maps: din_feat_rows (gather + trailer comparison)":
             (lambda: ops.feat_rows(slot_of, dst_rows, RB, zeros, trailer_of, trailers, flags, TB), R * (2 * RB + 2 * TB)),
             "the same rows: din_copy_rows_u8 out of the slots (no trailer, no comparison)": (lambda: ops.copy_rows_u8(slot_of, dst_rows, RB), R * 2 * RB)}
    for what, (fn, _) in forms.items():                                   # (the insert runs first: the other two read what it stored)
        out.zero_()
        fn()
        torch.cuda.synchronize()
        assert torch.equal(out, computed), what
    assert int(flags.sum()) == 0
    for what, r in timed({k: fn for k, (fn, _) in forms.items()}, a.warmup, a.windows, a.inner).items():
        nbytes = forms[what][1]
        gbs = {k.replace("_ms", "_GBps"): round(nbytes / (r[k] * 1e-3) / 1e9, 1) for k in ("median_ms", "min_ms", "p90_ms", "max_ms")}
        emit({"tool": "map_cache_time", "what": f"{R} maps of {RB} B: " + what, "bytes_read_plus_written": nbytes, **r, **gbs})


def _tce_cfg(dtype, batch, frames):
    from din_amd.config import Config
    cfg = Config("volleyball")                                            # scripts/train_volleyball_stage2_dynamic_tce.py
    cfg.inference_module_name, cfg.training_stage, cfg.train_backbone = "dynamic_tce_volleyball", 2, False
    cfg.backbone, cfg.out_size, cfg.emb_features, cfg.image_size, cfg.backbone_dtype = "vgg16", (OH, OW), C, (720, 1280), dtype
    cfg.batch_size, cfg.test_batch_size, cfg.num_frames, cfg.train_learning_rate = batch, 1, frames, 1e-4
    return cfg


def step_timings(a, emit):
    import torch.nn.functional as F
    from din_amd.feature_cache import FrameRefs, MapCache, map_shape_and_itemsize
    from din_amd.infer_model import Dynamic_TCE_volleyball
    from din_amd.optim import FusedAdam
    from din_amd.train_net_dynamic import SyntheticVolleyball
    dev = torch.device("cuda")
    B, T = a.batch, 10
    for dtype in ("bf16", "fp32"):
        cfg = _tce_cfg(dtype, B, T)
        torch.manual_seed(0)
        model = Dynamic_TCE_volleyball(cfg).to(dev).train()
        opt = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=0.0)
        clips = [SyntheticVolleyball(cfg, length=B, seed=2)[i] for i in range(B)]
        images, boxes = torch.stack([c[0] for c in clips]).to(dev), torch.stack([c[1] for c in clips]).to(dev)
        labels = torch.arange(B, device=dev) % cfg.num_activities
        cache = MapCache(dev, *map_shape_and_itemsize(cfg), int(a.cache_gb * 1e9))
        ids = np.arange(B * T).reshape(B, T)

        def step(first):
            opt.zero_grad()
            F.cross_entropy(model((first, boxes))["activities"], labels).backward()
            opt.step()

        step(FrameRefs(ids, images.reshape(B * T, 3, 720, 1280), np.arange(B * T), cache))     # every frame computed and inserted
        assert cache.inserted == B * T, "--cache-gb is too small for the step's frames"
        resident = lambda: step(FrameRefs(ids, images.reshape(B * T, 3, 720, 1280)[:0], [], cache))
        forms = {"every frame resident (gather + RoIAlign + head; no trunk launch)": resident,
                 "images tensor: the step with map_cache_gb = 0 (trunk on every frame)": lambda: step(images)}
        shape = {"tool": "map_cache_time", "model": f"Dynamic_TCE_volleyball vgg16 {dtype}, frozen backbone, 720x1280, out 22x40, T={T}", "batch": B,
                 "map_bytes_per_frame": cache.row_bytes}
        for what, r in timed(forms, 1, a.step_windows, a.step_inner).items():
            emit({**shape, "what": "training step, " + what, **r, "median_clips_per_s": round(B / (r["median_ms"] * 1e-3), 1)})
        cache.check()
        del model, opt, cache, images
        torch.cuda.empty_cache()


def feed_timings(a, emit):
    from din_amd import frame_cache as FC
    from din_amd.dataset import return_dataset
    from din_amd.infer_model import Dynamic_TCE_volleyball
    from din_amd.optim import FusedAdam
    from din_amd.train_net_dynamic import train_volleyball
    dev = torch.device("cuda")
    root = tempfile.mkdtemp(prefix="map_cache_tree_")
    try:
        t0 = time.perf_counter()
        train_seqs, test_seqs, _, _, nbytes = write_tree(root, a.clips, 9)
        emit({"tool": "map_cache_time", "what": "synthetic tree written", "clips": a.clips, "frames_per_clip_on_disk": 9,
              "jpeg_kb_per_frame": round(nbytes / 1e3 / ((a.clips + 2) * 9), 1), "seconds": round(time.perf_counter() - t0, 1)})
        cfg = _tce_cfg("fp32", 2, 3)
        cfg.data_path, cfg.train_seqs, cfg.test_seqs = root, train_seqs, test_seqs
        cfg.num_before, cfg.num_after = 1, 1
        torch.manual_seed(0)
        model = Dynamic_TCE_volleyball(cfg).to(dev)
        opt = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=cfg.train_learning_rate)
        shape = {"tool": "map_cache_time", "model": "Dynamic_TCE_volleyball vgg16 fp32, frozen backbone, 720x1280, T=3", "batch": 2,
                 "clips_per_epoch": a.clips}

        def epoch(loader):
            torch.cuda.synchronize()
            t = time.perf_counter()
            train_volleyball(loader, model, dev, opt, 1, cfg)           # (its meters read the device once at the end: a full sync)
            torch.cuda.synchronize()
            return a.clips / (time.perf_counter() - t)

        def stats(rates):
            r = sorted(rates)
            return {"median_clips_per_s": round(r[len(r) // 2], 2), "min_clips_per_s": round(r[0], 2), "max_clips_per_s": round(r[-1], 2),
                    "p90_low_clips_per_s": round(r[int(0.1 * (len(r) - 1))], 2), "windows": len(r)}

        ds, vs = return_dataset(cfg)
        off, _ = FC.build_loaders(cfg, ds, vs, 2, None, dev, True)
        epoch(off)                                                      # warm-up: code objects, workspaces, the allocator
        cfg.map_cache_gb = a.cache_gb
        ds, vs = return_dataset(cfg, frame_ids=FC.wants_frame_ids(cfg))
        on, _ = FC.build_loaders(cfg, ds, vs, 2, None, dev, True)
        emit({**shape, "what": "first cached epoch (decode + upload + trunk + insert)", **stats([epoch(on)])})
        rates = {"off": [], "on": []}
        for _ in range(a.epochs):                                       # the two alternate, epoch by epoch
            rates["off"].append(epoch(off))
            rates["on"].append(epoch(on))
        emit({**shape, "what": "epoch, cache off (decode + upload + trunk every epoch)", **stats(rates["off"])})
        emit({**shape, "what": "later cached epochs (gather + RoIAlign + head: no decode, no upload, no backbone launch)", **stats(rates["on"]),
              "cache": on.cache.table.counters()})
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=320)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--step-windows", type=int, default=7)
    ap.add_argument("--step-inner", type=int, default=2)
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--cache-gb", type=float, default=4.0)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-feed", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("map_cache_time.py measures on the MI355X: no GPU here, nothing measured")
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        if a.out:                                                        # rewritten after every line: a run cut short keeps what it measured
            with open(a.out, "w") as fh:
                fh.write("Map cache: the gather launch, the TCE step and the feed rate (tools/map_cache_time.py), one MI355X:\n" + "\n".join(lines) + "\n")

    if not a.skip_kernel:
        kernel_timings(a, emit)
    if not a.skip_step:
        step_timings(a, emit)
    if not a.skip_feed:
        feed_timings(a, emit)
    emit({"clock": clock()})


if __name__ == "__main__":
    main()
