#!/usr/bin/env python3
"""The box-feature cache on disk (cfg.feature_cache_path), timed on one MI355X at the ARG launcher's vgg16 shape (rows of 12 x 512 x 5 x 5
fp32 = 614 400 bytes plus 192 bytes of boxes):

1. FeatureCache.save and FeatureCache.load of `--frames` frames to a file under `--dir` (default: a temporary directory, so the file
   system measured is the one temporary files live on), `--repeats` times each, alternating: GB/s of records.  A load follows the save of
   the same file, so it reads what the page cache still holds unless the file is larger than memory: it bounds the copy path (memmap ->
   pinned buffer -> slab), not a cold disk.
2. The wall time of the FIRST training epoch of a run, through train_net_dynamic.train_volleyball over a throw-away tree of synthetic
   1280x720 JPEGs (tools/frame_feed_time.py: write_tree; ARG_volleyball, VGG16 fp32, frozen, 720x1280, out_size 22x40, T = 3, batch
   size 2): started with an empty cache, which is the first epoch of a run without the setting (decode + upload + trunk + insert),
   against started from the file (load, then gather only), alternating, `--epochs` of each, fresh caches every time.  The time of the
   load is part of the second.

One JSON line per measurement, then the GPU clock.  usage: python tools/feature_cache_file_time.py [--out profiles/feature_cache_file_time.txt]
[--frames 2048] [--repeats 3] [--clips 64] [--batch 2] [--epochs 3] [--dir DIR] [--skip-epoch]"""
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
from at_step_time import clock  # noqa: E402
from frame_feed_time import write_tree  # noqa: E402

RB, BB = 12 * 512 * 25 * 4, 12 * 16


def stats(values, unit):
    v = sorted(values)
    return {f"median_{unit}": round(v[len(v) // 2], 3), f"min_{unit}": round(v[0], 3), f"max_{unit}": round(v[-1], 3), "runs": len(v)}


def file_timings(a, folder, emit):
    from din_amd.feature_cache import FeatureCache
    from din_amd.feature_cache_file import FIELDS
    dev = torch.device("cuda")
    meta = {**{k: "timing" for k in FIELDS}, "digest": "0" * 64}
    cache = FeatureCache(dev, RB, BB, 1 << 40)
    ids = np.arange(a.frames)
    for at in range(0, a.frames, 64):                                # filled as a run fills it: slab by slab
        n = min(64, a.frames - at)
        cache.rows(ids[at:at + n], torch.rand((n, BB // 4), device=dev), range(n), torch.randn((n, RB // 4), device=dev))
    cache.check()
    path = os.path.join(folder, "timing.dinfc")
    nbytes = a.frames * (RB + BB)
    saves, loads = [], []
    for _ in range(a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cache.save(path, meta)
        saves.append(nbytes / (time.perf_counter() - t0) / 1e9)
        fresh = FeatureCache(dev, RB, BB, 1 << 40)
        t0 = time.perf_counter()
        got = fresh.load(path, meta)
        torch.cuda.synchronize()
        loads.append(nbytes / (time.perf_counter() - t0) / 1e9)
        assert len(got) == a.frames and all(torch.equal(x, y) for x, y in zip(fresh.slabs[:2], cache.slabs[:2]))
        del fresh
    what = f"{a.frames} frames of {RB} + {BB} B ({nbytes / 1e9:.2f} GB) "
    emit({"tool": "feature_cache_file_time", "what": what + "FeatureCache.save (device -> pinned -> file, fsync, rename)", **stats(saves, "GBps")})
    emit({"tool": "feature_cache_file_time", "what": what + "FeatureCache.load (file just written -> pinned -> device)", **stats(loads, "GBps")})
    os.remove(path)


def epoch_timings(a, folder, emit):
    from din_amd import feature_cache as FE, feature_cache_file as FF, frame_cache as FC
    from din_amd.config import Config
    from din_amd.dataset import return_dataset
    from din_amd.infer_model import ARG_volleyball
    from din_amd.optim import FusedAdam
    from din_amd.train_net_dynamic import train_volleyball
    dev = torch.device("cuda")
    root = os.path.join(folder, "tree")
    os.makedirs(root)
    train_seqs, test_seqs, _, _, _ = write_tree(root, a.clips, 9)
    cfg = Config("volleyball")                                        # scripts/train_volleyball_stage2_arg.py, vgg16 set-up
    cfg.inference_module_name, cfg.training_stage, cfg.train_backbone = "arg_volleyball", 2, False
    cfg.backbone, cfg.out_size, cfg.emb_features, cfg.image_size = "vgg16", (22, 40), 512, (720, 1280)
    cfg.batch_size, cfg.test_batch_size, cfg.num_frames, cfg.train_learning_rate = a.batch, 1, 3, 1e-4
    cfg.data_path, cfg.train_seqs, cfg.test_seqs = root, train_seqs, test_seqs
    cfg.num_before, cfg.num_after = 1, 1
    cfg.feature_cache_gb, cfg.feature_cache_path = 4, os.path.join(folder, "files")
    torch.manual_seed(0)
    model = ARG_volleyball(cfg).to(dev)
    opt = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=cfg.train_learning_rate)

    def first_epoch(from_file):
        """a run's start up to the end of its first training epoch: fresh datasets, loaders and caches; seconds"""
        ds, vs = return_dataset(cfg, frame_ids=True)
        loaders = FC.build_loaders(cfg, ds, vs, a.batch, None, dev, True)
        files = FE.cache_files(cfg, model, *loaders, 0, 1, lambda line: None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if from_file:
            assert files["train"].load() == len(ds.frame_table)
        before = files["train"].inserted
        train_volleyball(loaders[0], model, dev, opt, 1, cfg)
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        if not from_file:
            files["train"].save_if_grown(before)                       # (outside the window: the parent's first epoch writes nothing)
        else:
            assert files["train"].inserted == before
        return seconds

    first_epoch(False)                                                 # warm-up: code objects, workspaces; writes the file
    t = {"empty": [], "file": []}
    for _ in range(a.epochs):
        t["empty"].append(first_epoch(False))
        t["file"].append(first_epoch(True))
    size = os.path.getsize(os.path.join(cfg.feature_cache_path, FF.file_name("train")))
    shape = {"tool": "feature_cache_file_time", "model": "ARG_volleyball vgg16 fp32, frozen backbone, 720x1280, T=3", "batch": a.batch,
             "clips_per_epoch": a.clips, "file_bytes": size}
    emit({**shape, "what": "first epoch, empty cache (decode + upload + trunk + insert): the first epoch without feature_cache_path",
          **stats(t["empty"], "s")})
    emit({**shape, "what": "first epoch started from the file (load included; gather only)", **stats(t["file"], "s")})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--skip-epoch", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("feature_cache_file_time.py measures on the MI355X: no GPU here, nothing measured")
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        if a.out:                                                      # rewritten after every line: a run cut short keeps what it measured
            with open(a.out, "w") as fh:
                fh.write("Box-feature cache on disk: save / load rate and first-epoch time (tools/feature_cache_file_time.py), one MI355X:\n"
                         + "\n".join(lines) + "\n")

    folder = tempfile.mkdtemp(prefix="feature_cache_file_", dir=a.dir)
    try:
        file_timings(a, folder, emit)
        if not a.skip_epoch:
            epoch_timings(a, folder, emit)
    finally:
        shutil.rmtree(folder, ignore_errors=True)
    emit({"clock": clock()})


if __name__ == "__main__":
    main()
