#!/usr/bin/env python3
"""Mirrored box features (cfg.feature_cache_flip, cfg.test_flip; din_amd/feature_cache.py) on one MI355X, Dynamic_volleyball at the
launcher's Inception-v3 geometry (720x1280 frames, out_size 87x157, 1056 channels, 12 boxes, T = 10, frozen backbone):

1. the cached training step at B = `--batch` with every frame resident, at flip_prob 0 / 0.5 / 1: flip_prob = 0 is fed through a loader
   without a mirror cache (FeatureCache.rows: the path as it was before the mirror cache existed, launch for launch) and is the
   yardstick; 0.5 mirrors every other clip, 1 all of them (FeatureCache.rows_both + the one din_flip_clip_labels launch);
2. an evaluation pass (train_net_dynamic._test_pass, `--eval-batches` batches of `--eval-batch` clips, all resident) with test_flip off
   and on, and the ratio of the medians;
3. the fill rate of first-epoch steps (`--fill-batch` clips of decoded frames that no cache holds: upload excluded, trunk + insert) without
   and with the mirror cache: the trunk runs twice with it.

The forms of one measurement alternate window by window in one process (tools/at_step_time.py: timed); median / min / p90 / max over
`--windows` windows of `--inner` calls.  The rows in the slots are random numbers (the head's arithmetic does not care); the frames of
measurement 3 are random pixels.  One JSON line per measurement, then the GPU clock.

usage: python tools/feature_cache_flip_time.py [--out profiles/feature_cache_flip_time.txt] [--windows 15] [--inner 5] [--batch 32]
[--eval-batch 8] [--eval-batches 4] [--fill-batch 4] [--skip-fill]"""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from at_step_time import clock, timed  # noqa: E402

T, N = 10, 12


def config():
    from din_amd.config import Config
    cfg = Config("volleyball")                                              # scripts/train_volleyball_stage2_dynamic.py, inv3 set-up
    cfg.inference_module_name, cfg.training_stage, cfg.train_backbone, cfg.set_bn_eval = "dynamic_volleyball", 2, False, True
    cfg.backbone, cfg.image_size, cfg.out_size, cfg.emb_features, cfg.num_frames = "inv3", (720, 1280), (87, 157), 1056, T
    cfg.feature_cache_gb, cfg.feature_cache_flip = 8, True
    return cfg


def labels(cfg, clips, seed):
    from din_amd.train_net_dynamic import SyntheticVolleyball
    items = [SyntheticVolleyball(cfg, length=clips, seed=seed)[i] for i in range(clips)]
    return [torch.stack([it[k] for it in items]) for k in (1, 2, 3)]        # boxes, actions, activities


def resident_pair(cfg, dev, ids, boxes):
    """a cache and its mirror cache holding random rows for `ids`, with the trailers a real fill would store"""
    from din_amd import ops
    from din_amd.feature_cache import FeatureCache, row_and_box_bytes
    rb, bb = row_and_box_bytes(cfg)
    cache, mirror = FeatureCache(dev, rb, bb, 8 << 30), FeatureCache(dev, rb, bb, 8 << 30, orientation="mirrored")
    flat = ids.reshape(-1)
    plain = boxes.reshape(len(flat), N * 4).contiguous()
    mirrored = plain.clone()
    ops.flip_clip_labels(mirrored.view(len(flat), N, 4), None, torch.ones(len(flat), dtype=torch.int64, device=dev), None, None, float(cfg.out_size[1]))
    g = torch.Generator(device=dev).manual_seed(1)
    for at in range(0, len(flat), 64):                                          # (64 frames a launch: 2 x 81 MB of stand-in rows)
        sl = slice(at, at + 64)
        n = len(flat[sl])
        rows = [torch.randn((n, rb // 4), device=dev, generator=g) for _ in range(2)]
        cache.rows_both(mirror, flat[sl], None, plain[sl], np.arange(n), rows, (plain[sl].contiguous(), mirrored[sl].contiguous()))
    cache.check()
    assert cache.inserted == mirror.inserted == len(flat)
    return cache, mirror


def step_timings(a, emit, cfg, model, dev):
    from din_amd import frame_cache as FC
    from din_amd.feature_cache import FrameRefs
    from din_amd.optim import FusedAdam
    from din_amd.volleyball import FLIP_ACTIVITIES
    B = a.batch
    boxes, _, activities = [t.to(dev) for t in labels(cfg, B, 2)]
    ids = np.arange(B * T).reshape(B, T)
    cache, mirror = resident_pair(cfg, dev, ids, boxes)
    opt = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=1e-5)
    none = torch.zeros((0, 3) + tuple(cfg.image_size), dtype=torch.uint8, device=dev)
    plan = FC.FlipPlan(0.5, 0, 0, FLIP_ACTIVITIES, float(cfg.out_size[1])).epoch(1)
    model.train()
    model.apply(lambda m: m.eval() if m.__class__.__name__.find("BatchNorm") != -1 else None)

    def step(clip_flags):
        def run():
            b, act = boxes.clone(), activities.clone()                          # (the feed's labels arrive fresh every batch; both forms clone)
            if clip_flags is None:
                refs = FrameRefs(ids, none, [], cache)
            else:
                rows = np.repeat(clip_flags, T)
                d_flags, = cache._upload(rows.astype(np.int64))
                plan.mirror_labels([b, None, act], d_flags)
                refs = FrameRefs(ids, none, [], cache, None, mirror, rows.reshape(B, T))
            loss = F.cross_entropy(model((refs, b))["activities"], act[:, 0])
            opt.zero_grad()
            loss.backward()
            opt.step()
        return run

    forms = {"flip_prob 0 (no mirror cache: the path as it was)": step(None),
             "flip_prob 0.5 (every other clip mirrored)": step(np.arange(B) % 2 == 1),
             "flip_prob 1 (every clip mirrored)": step(np.ones(B, dtype=bool))}
    out = timed(forms, a.warmup, a.windows, a.inner)
    cache.check()
    base = out["flip_prob 0 (no mirror cache: the path as it was)"]
    for what, r in out.items():
        emit({"tool": "feature_cache_flip_time", "what": f"cached training step, B = {B}, T = {T}: " + what, **r,
              "median_minus_yardstick_ms": round(r["median_ms"] - base["median_ms"], 4),
              "yardstick_spread_p90_minus_min_ms": round(base["p90_ms"] - base["min_ms"], 4)})


def eval_timings(a, emit, cfg, model, dev):
    import copy
    from din_amd.feature_cache import FeatureLoader
    from din_amd.train_net_dynamic import _test_pass
    B, K = a.eval_batch, a.eval_batches
    boxes, actions, activities = labels(cfg, B * K, 3)
    ids = np.arange(10000, 10000 + B * K * T).reshape(B * K, T)
    cache, mirror = resident_pair(cfg, dev, ids, boxes.to(dev))
    none = torch.zeros((0, 3) + tuple(cfg.image_size), dtype=torch.uint8)
    batches = [(torch.from_numpy(ids[k * B:(k + 1) * B]), none, torch.zeros(0, dtype=torch.int64), boxes[k * B:(k + 1) * B],
                actions[k * B:(k + 1) * B], activities[k * B:(k + 1) * B]) for k in range(K)]
    loader = FeatureLoader(batches, cache, types.SimpleNamespace(resident=torch.ones(1, dtype=torch.uint8)), mirror)
    on = copy.copy(cfg)
    on.test_flip = True
    forms = {"test_flip off": lambda: _test_pass(loader, model, dev, 1, cfg, False), "test_flip on": lambda: _test_pass(loader, model, dev, 1, on, False)}
    out = timed(forms, a.warmup, a.windows, max(1, a.inner // 2))
    for what, r in out.items():
        emit({"tool": "feature_cache_flip_time", "what": f"evaluation pass, {K} batches of {B} clips, all resident: " + what, **r,
              "ratio_of_medians_to_off": round(r["median_ms"] / out["test_flip off"]["median_ms"], 3)})


def fill_timings(a, emit, cfg, model, dev):
    from din_amd import infer_model as IM
    from din_amd.feature_cache import FeatureCache, FrameRefs, row_and_box_bytes
    B = a.fill_batch
    boxes = labels(cfg, B, 4)[0].to(dev)
    frames = torch.randint(0, 256, (B * T, 3) + tuple(cfg.image_size), dtype=torch.uint8, device=dev)
    rb, bb = row_and_box_bytes(cfg)
    total = (a.warmup + a.windows) * 2 * 2 + 4                                  # launches of B * T new frames each (inner = 2)
    capacity = (total + 1) * B * T * (rb + bb)
    alone, cache, mirror = FeatureCache(dev, rb, bb, capacity), FeatureCache(dev, rb, bb, capacity), FeatureCache(dev, rb, bb, capacity, orientation="mirrored")
    serial = [0]

    def fill(with_mirror):
        def run():
            ids = np.arange(serial[0], serial[0] + B * T).reshape(B, T)         # frames no cache has seen
            serial[0] += B * T
            refs = FrameRefs(ids, frames, np.arange(B * T), cache if with_mirror else alone, None, mirror if with_mirror else None)
            with torch.no_grad():
                IM._cached_crops(model, refs, boxes, N)
            assert len(refs.inserted) == B * T
        return run

    out = timed({"plain cache only (the trunk once)": fill(False), "with the mirror cache (the trunk once per orientation)": fill(True)},
                a.warmup, a.windows, 2)
    for what, r in out.items():
        emit({"tool": "feature_cache_flip_time", "what": f"first-epoch step, {B} clips = {B * T} decoded frames: " + what, **r,
              "frames_per_s_at_median": round(B * T / (r["median_ms"] * 1e-3), 1)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--eval-batch", type=int, default=8)
    ap.add_argument("--eval-batches", type=int, default=4)
    ap.add_argument("--fill-batch", type=int, default=4)
    ap.add_argument("--skip-fill", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("feature_cache_flip_time.py measures on the MI355X: no GPU here, nothing measured")
    from din_amd.train_net_dynamic import build_model
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        if a.out:                                                        # rewritten after every line: a run cut short keeps what it measured
            with open(a.out, "w") as fh:
                fh.write("Mirrored box features: cached step, test-time flipping, fill rate (tools/feature_cache_flip_time.py), one MI355X, "
                         "one run:\n" + "\n".join(lines) + "\n")

    cfg, dev = config(), torch.device("cuda")
    torch.manual_seed(0)
    model = build_model(cfg).to(dev)
    step_timings(a, emit, cfg, model, dev)
    model.eval()
    eval_timings(a, emit, cfg, model, dev)
    if not a.skip_fill:
        fill_timings(a, emit, cfg, model, dev)
    emit({"clock": clock()})


if __name__ == "__main__":
    main()
