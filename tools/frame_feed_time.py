#!/usr/bin/env python3
"""Frame cache timings (din_amd/frame_cache.py) on one MI355X.

1. Gather of 320 rows of 3x720x1280 bytes (a 32-clip batch of ten-frame clips) out of a slab of 640 resident frames, random rows with
   repeats, in GB/s counting the bytes read plus the bytes written:
     (a) din_copy_rows_u8, one launch over address tables already on the device (what FrameCache.build_batch issues);
     (b) torch.index_select on the slab viewed as [640, frame_bytes] (only possible while all frames live in ONE allocation);
     (c) 320 hipMemcpyAsync device-to-device copies on the same stream.
   The three alternate window by window; median / min / p90 / max over `--windows` windows of `--inner` gathers each.  For scale: a plain
   float4 copy on this chip measures 6.29 TB/s of read + write traffic (MI355X_MICROARCH.md).
2. Feed rate, in clips/s, of one training epoch through train_net_dynamic.train_volleyball over a throw-away tree of synthetic,
   photo-like 1280x720 JPEGs that the tool writes itself under a temporary directory (PIL, quality 90; `--clips` clips of `--frames`
   frames; nothing is fetched): cache off with 0 and with `--workers` loader workers, the first cached epoch (decode + upload + insert),
   the later cached epochs (gather only; one window per epoch), and the same step fed by input_feed.DeviceFeed from pre-built uint8
   host batches, which is the path without any decode.  The model is the benchmark's: Dynamic_volleyball, Inception-v3 bf16, fused Adam.

One JSON line per measurement, then the GPU clock.  usage: python tools/frame_feed_time.py [--out profiles/frame_cache_time.txt]
[--skip-feed] [--skip-gather] [--windows 15] [--inner 5] [--clips 64] [--frames 10] [--batch 32] [--workers 8] [--epochs 6]"""
import argparse
import ctypes as C
import json
import os
import pickle
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

FRAME = (3, 720, 1280)


def hip_runtime():
    """the HIP runtime this process already holds (torch's): its path is read from the process's own map, never a second copy"""
    with open("/proc/self/maps") as fh:
        paths = sorted({line.split()[-1] for line in fh if "libamdhip64" in line})
    if not paths:
        raise RuntimeError("no libamdhip64 is mapped into this process")
    lib = C.CDLL(paths[0])
    lib.hipMemcpyAsync.restype = C.c_int
    lib.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    return lib


def gather_timings(a, emit):
    from din_amd import ops
    dev = torch.device("cuda")
    rows, resident = 320, 640
    fb = int(np.prod(FRAME))
    slab = torch.randint(0, 256, (resident, fb), dtype=torch.uint8, device=dev)
    out = torch.empty((rows, fb), dtype=torch.uint8, device=dev)
    idx_host = np.random.default_rng(0).integers(0, resident, rows)
    idx = torch.from_numpy(idx_host).to(dev)
    src = torch.tensor([slab.data_ptr() + int(i) * fb for i in idx_host], dtype=torch.int64, device=dev)
    dst = torch.tensor([out.data_ptr() + i * fb for i in range(rows)], dtype=torch.int64, device=dev)
    hip = hip_runtime()
    pairs = [(out.data_ptr() + i * fb, slab.data_ptr() + int(j) * fb) for i, j in enumerate(idx_host)]

    def memcpys():
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for d, s in pairs:
            if hip.hipMemcpyAsync(d, s, fb, 3, stream) != 0:              # 3 = hipMemcpyDeviceToDevice
                raise RuntimeError("hipMemcpyAsync failed")

    forms = {"din_copy_rows_u8, one launch": lambda: ops.copy_rows_u8(src, dst, fb),
             "torch.index_select on one slab": lambda: torch.index_select(slab, 0, idx, out=out),
             "320 x hipMemcpyAsync device-to-device": memcpys}
    want = slab[idx]
    for what, fn in forms.items():
        out.zero_()
        fn()
        torch.cuda.synchronize()
        assert torch.equal(out, want), what
    for what, r in timed(forms, a.warmup, a.windows, a.inner).items():
        gbs = {k.replace("_ms", "_GBps"): round(2 * rows * fb / (r[k] * 1e-3) / 1e9, 1) for k in ("median_ms", "min_ms", "p90_ms", "max_ms")}
        emit({"tool": "frame_feed_time", "what": "gather 320 x 3x720x1280 u8: " + what, "bytes_read_plus_written": 2 * rows * fb, **r, **gbs})


def write_tree(root, clips, frames, seed=0):
    """a volleyball-format tree (annotations.txt per sequence, tracks_normalized.pkl, <sid>/<src>/<fid>.jpg) of synthetic photo-like
    JPEGs: smooth low-frequency colour fields plus fine noise, so that the files have the size and decode cost of camera frames"""
    from PIL import Image
    from din_amd.volleyball import ACTIONS, ACTIVITIES
    rng = np.random.default_rng(seed)
    before = (frames - 1) // 2 + (frames - 1) % 2
    after = frames - 1 - before
    tracks, per_seq, nbytes = {}, 16, 0
    seqs = list(range((clips + per_seq - 1) // per_seq)) + [99]              # 99: the validation sequence, two clips
    yy, xx = np.mgrid[0:720, 0:1280].astype(np.float32)
    for sid in seqs:
        os.makedirs(os.path.join(root, str(sid)))
        lines = []
        count = 2 if sid == 99 else min(per_seq, clips - sid * per_seq)
        for c in range(count):
            src = 100 + 20 * c
            people = []
            boxes = np.empty((12, 4))
            for p in range(12):
                x, y, w, h = int(rng.integers(0, 1100)), int(rng.integers(150, 450)), int(rng.integers(40, 110)), int(rng.integers(90, 200))
                people.append(f"{x} {y} {w} {h} {ACTIONS[int(rng.integers(0, len(ACTIONS)))]}")
                boxes[p] = (y / 720, x / 1280, (y + h) / 720, (x + w) / 1280)
            lines.append(f"{src}.jpg {ACTIVITIES[int(rng.integers(0, len(ACTIVITIES)))]} " + " ".join(people))
            os.makedirs(os.path.join(root, str(sid), str(src)))
            tracks[(sid, src)] = {}
            ph = rng.uniform(0, 6.28, (3, 3))
            base = np.stack([127 + 60 * np.sin(xx / (90 + 40 * ch) + ph[ch, 0]) * np.cos(yy / (70 + 30 * ch) + ph[ch, 1])
                             + 40 * np.sin((xx + yy) / 23.0 + ph[ch, 2]) for ch in range(3)], -1).astype(np.int16)
            for fid in range(src - before, src + after + 1):
                tracks[(sid, src)][fid] = boxes + rng.normal(0, 0.002, boxes.shape)
                img = np.roll(base, 3 * (fid - src), axis=1) + rng.integers(-16, 17, base.shape, dtype=np.int16)   # a pan plus sensor noise
                img = np.clip(img, 0, 255).astype(np.uint8)
                path = os.path.join(root, str(sid), str(src), f"{fid}.jpg")
                Image.fromarray(img).save(path, quality=90)
                nbytes += os.path.getsize(path)
        with open(os.path.join(root, str(sid), "annotations.txt"), "w") as fh:
            fh.write("\n".join(lines) + "\n")
    with open(os.path.join(root, "tracks_normalized.pkl"), "wb") as fh:
        pickle.dump(tracks, fh)
    return seqs[:-1], [99], before, after, nbytes


def feed_timings(a, emit):
    import torch.utils.data as tud
    from bench import make_cfg, synth_weights
    from din_amd import frame_cache as FC
    from din_amd.dataset import return_dataset
    from din_amd.infer_model import Dynamic_volleyball
    from din_amd.optim import FusedAdam
    from din_amd.train_net_dynamic import train_volleyball
    dev = torch.device("cuda")
    root = tempfile.mkdtemp(prefix="frame_feed_tree_")
    try:
        t0 = time.perf_counter()
        train_seqs, test_seqs, before, after, nbytes = write_tree(root, a.clips, a.frames)
        emit({"tool": "frame_feed_time", "what": "synthetic tree written", "clips": a.clips, "frames_per_clip": a.frames,
              "jpeg_kb_per_frame": round(nbytes / 1e3 / ((a.clips + 2) * a.frames), 1), "seconds": round(time.perf_counter() - t0, 1)})
        cfg = make_cfg("inv3_bf16", T=a.frames)
        cfg.data_path, cfg.train_seqs, cfg.test_seqs, cfg.num_before, cfg.num_after = root, train_seqs, test_seqs, before, after
        cfg.training_stage, cfg.batch_size, cfg.train_learning_rate = 2, a.batch, 1e-5
        torch.manual_seed(0)
        model = Dynamic_volleyball(cfg)
        synth_weights(model)
        model = model.to(dev)
        opt = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=cfg.train_learning_rate)
        shape = {"tool": "frame_feed_time", "model": "Dynamic_volleyball inv3 bf16", "batch": a.batch, "T": a.frames, "clips_per_epoch": a.clips}

        def epoch(loader, n=1):
            torch.cuda.synchronize()
            t = time.perf_counter()
            train_volleyball(loader, model, dev, opt, n, cfg)           # (its meters read the device once at the end: a full sync)
            torch.cuda.synchronize()
            return a.clips / (time.perf_counter() - t)

        def stats(rates):
            r = sorted(rates)
            return {"median_clips_per_s": round(r[len(r) // 2], 1), "min_clips_per_s": round(r[0], 1), "max_clips_per_s": round(r[-1], 1),
                    "p90_low_clips_per_s": round(r[int(0.1 * (len(r) - 1))], 1), "windows": len(r)}

        # resident host tensors: pre-built uint8 batches through DeviceFeed (no decode); its first epochs also warm the model up
        plain, _ = return_dataset(cfg)
        batches = [tuple(t.pin_memory() for t in tud.default_collate([plain[i] for i in range(s, min(s + a.batch, len(plain)))]))
                   for s in range(0, len(plain), a.batch)]
        for _ in range(2):
            epoch(batches)
        resident = [epoch(batches) for _ in range(a.epochs)]
        # cache off, 0 and --workers workers; cache on: first epoch, then the later ones; resident tensors again at the end (drift)
        for workers in (0, a.workers):
            cfg.frame_cache_gb, cfg.num_workers = 0, workers
            ds, vs = return_dataset(cfg)
            loader, _ = FC.build_loaders(cfg, ds, vs, a.batch, None, dev, True)
            emit({**shape, "what": f"epoch, cache off, num_workers={workers}", **stats([epoch(loader) for _ in range(2 if workers else 1)])})
        for workers in (0, a.workers):
            cfg.frame_cache_gb, cfg.num_workers = a.cache_gb, workers
            ds, vs = return_dataset(cfg, frame_ids=True)
            loader, _ = FC.build_loaders(cfg, ds, vs, a.batch, None, dev, True)
            emit({**shape, "what": f"first cached epoch (decode + upload + insert), num_workers={workers}", **stats([epoch(loader)])})
            later = [epoch(loader) for _ in range(a.epochs)]
            emit({**shape, "what": f"later cached epochs (gather only), num_workers={workers}", **stats(later),
                  "cache": loader.cache.table.counters()})
        resident += [epoch(batches) for _ in range(a.epochs)]
        emit({**shape, "what": "epoch from pre-built uint8 host batches through DeviceFeed (no decode), before and after the others",
              **stats(resident)})
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--epochs", type=int, default=6)
    ap.add_argument("--cache-gb", type=float, default=8.0)
    ap.add_argument("--skip-gather", action="store_true")
    ap.add_argument("--skip-feed", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        if a.out:                                                        # rewritten after every line: a run cut short keeps what it measured
            with open(a.out, "w") as fh:
                fh.write("Frame cache: gather and feed rate (tools/frame_feed_time.py), one MI355X:\n" + "\n".join(lines) + "\n")

    if not a.skip_gather:
        gather_timings(a, emit)
    if not a.skip_feed:
        feed_timings(a, emit)
    emit({"clock": clock()})


if __name__ == "__main__":
    main()
