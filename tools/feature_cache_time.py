#!/usr/bin/env python3
"""Box-feature cache timings (din_amd/feature_cache.py) on one MI355X.

1. din_feat_rows against the primitive it replaces, din_copy_rows_u8, for `--rows` fp32 rows of 12 x 512 x 5 x 5 features (614 400 bytes,
   the VGG16 row) with 192 bytes of boxes each:
     (a) a batch of computed rows: ONE din_feat_rows launch (source read once, written to the feats tensor and to the slot, boxes
         stored) against TWO din_copy_rows_u8 launches, insert then gather out of the slots (what frame_cache.FrameCache.build_batch
         issues for frames; it stores no boxes);
     (b) a batch of resident rows: one din_feat_rows launch (gather + box comparison) against one din_copy_rows_u8 gather (no comparison).
   The forms alternate window by window; median / min / p90 / max over `--windows` windows of `--inner` calls each, and GB/s counting the
   bytes each form reads plus the bytes it writes.
2. Feed rate, in clips/s, of training epochs through train_net_dynamic.train_volleyball at the ARG launcher's vgg16 set-up
   (ARG_volleyball, VGG16 fp32, frozen backbone, 720x1280 frames, out_size 22x40, three frames a clip, batch size 2) over a throw-away
   tree of synthetic, photo-like 1280x720 JPEGs that the tool writes itself under a temporary directory (tools/frame_feed_time.py:
   write_tree; nothing is fetched): the first cached epoch (decode + upload + trunk + insert) once, then epochs with both caches off,
   epochs fed by the frame cache (frame_cache.py: pixels resident, the trunk still runs) and later cached epochs (gather only)
   ALTERNATING, one window per epoch.
3. With `--dtype bf16`, in place of 1 and 2: slots of fp32 rows against slots of bf16 rows (cfg.feature_cache_dtype), alternated in the
   same windows -- the launch for computed and for resident rows, and the gather of resident rows followed by fc_emb_1's forward, where
   the cast pass the bf16 rows spare shows (dtype_timings).

One JSON line per measurement, then the GPU clock.  usage: python tools/feature_cache_time.py [--out profiles/feature_cache_time.txt]
[--dtype fp32|bf16] [--skip-feed] [--skip-kernel] [--windows 15] [--inner 5] [--rows 320] [--clips 64] [--batch 2] [--epochs 5]
[--cache-gb 4]"""
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

RB, BB = 12 * 512 * 25 * 4, 12 * 16


def kernel_timings(a, emit):
    from din_amd import ops
    dev = torch.device("cuda")
    R = a.rows
    g = torch.Generator(device=dev).manual_seed(0)
    computed = torch.randn((R, RB // 4), device=dev, generator=g)
    boxes = torch.rand((R, BB // 4), device=dev, generator=g) * 40
    out = torch.empty((R, RB // 4), device=dev)
    slots = torch.zeros(R * (RB + BB), dtype=torch.uint8, device=dev)
    order = np.random.default_rng(0).permutation(R)                       # row i lives in slot order[i]
    tab = lambda v: torch.tensor([int(x) for x in v], dtype=torch.int64, device=dev)
    src_rows = tab(computed.data_ptr() + i * RB for i in range(R))
    dst_rows = tab(out.data_ptr() + i * RB for i in range(R))
    slot_of = tab(slots.data_ptr() + int(order[i]) * (RB + BB) for i in range(R))
    trailer_of = tab(slots.data_ptr() + int(order[i]) * (RB + BB) + RB for i in range(R))
    zeros = torch.zeros(R, dtype=torch.int64, device=dev)
    flags = torch.zeros(R, dtype=torch.uint8, device=dev)

    def two_copies():
        ops.copy_rows_u8(src_rows, slot_of, RB)
        ops.copy_rows_u8(slot_of, dst_rows, RB)

    insert = {"computed rows: din_feat_rows, one launch (feats + slot + boxes)":
              (lambda: ops.feat_rows(src_rows, dst_rows, RB, slot_of, zeros, boxes, flags, BB), R * (3 * RB + 2 * BB)),
              "computed rows: 2 x din_copy_rows_u8 (insert, then gather; no boxes)": (two_copies, R * 4 * RB)}
    gather = {"resident rows: din_feat_rows, one launch (gather + box comparison)":
              (lambda: ops.feat_rows(slot_of, dst_rows, RB, zeros, trailer_of, boxes, flags, BB), R * (2 * RB + 2 * BB)),
              "resident rows: din_copy_rows_u8 gather (no comparison)": (lambda: ops.copy_rows_u8(slot_of, dst_rows, RB), R * 2 * RB)}
    for forms in (insert, gather):
        for what, (fn, _) in forms.items():                               # every form builds the same feats tensor
            out.zero_()
            fn()
            torch.cuda.synchronize()
            assert torch.equal(out, computed), what
        assert int(flags.sum()) == 0
        for what, r in timed({k: fn for k, (fn, _) in forms.items()}, a.warmup, a.windows, a.inner).items():
            nbytes = forms[what][1]
            gbs = {k.replace("_ms", "_GBps"): round(nbytes / (r[k] * 1e-3) / 1e9, 1) for k in ("median_ms", "min_ms", "p90_ms", "max_ms")}
            emit({"tool": "feature_cache_time", "what": f"{R} rows of {RB} B: " + what, "bytes_read_plus_written": nbytes, **r, **gbs})


def dtype_timings(a, emit):
    """--dtype bf16: slots of fp32 rows (din_feat_rows) against slots of bf16 rows (din_feat_rows_bf16) for the same `--rows` rows, the two
    alternated window by window: (a) the launch alone, for computed rows (feats + slot + boxes; the bf16 form rounds on the way) and for
    resident rows (gather + box comparison); (b) the gather of resident rows followed by fc_emb_1's forward (ops.linear, lowp: bf16
    operands) -- the fp32 feats tensor is rounded in a pass of its own there, the bf16 one is the operand"""
    from din_amd import ops
    dev = torch.device("cuda")
    R, NE = a.rows, RB // 4
    RB16 = 2 * NE
    g = torch.Generator(device=dev).manual_seed(0)
    computed = torch.randn((R, NE), device=dev, generator=g)
    boxes = torch.rand((R, BB // 4), device=dev, generator=g) * 40
    out32, out16 = torch.empty((R, NE), device=dev), torch.empty((R, NE), device=dev, dtype=torch.bfloat16)
    slots32 = torch.zeros(R * (RB + BB), dtype=torch.uint8, device=dev)
    slots16 = torch.zeros(R * (RB16 + BB), dtype=torch.uint8, device=dev)
    order = np.random.default_rng(0).permutation(R)                       # row i lives in slot order[i]
    tab = lambda v: torch.tensor([int(x) for x in v], dtype=torch.int64, device=dev)
    src_rows = tab(computed.data_ptr() + i * RB for i in range(R))
    dst32, dst16 = tab(out32.data_ptr() + i * RB for i in range(R)), tab(out16.data_ptr() + i * RB16 for i in range(R))
    slot32 = tab(slots32.data_ptr() + int(order[i]) * (RB + BB) for i in range(R))
    slot16 = tab(slots16.data_ptr() + int(order[i]) * (RB16 + BB) for i in range(R))
    trailer32, trailer16 = slot32 + RB, slot16 + RB16
    zeros, ones = torch.zeros(R, dtype=torch.int64, device=dev), torch.ones(R, dtype=torch.int64, device=dev)
    flags = torch.zeros(R, dtype=torch.uint8, device=dev)
    K2D, NFB = 25 * 512, 1024                                             # fc_emb_1 of the VGG16 launchers: Linear(K*K*D, num_features_boxes)
    weight = torch.randn((NFB, K2D), device=dev, generator=g) * 0.01
    bias = torch.zeros(NFB, device=dev)

    def gather32():
        ops.feat_rows(slot32, dst32, RB, zeros, trailer32, boxes, flags, BB)

    def gather16():
        ops.feat_rows_bf16(slot16, dst16, NE, zeros, trailer16, boxes, flags, BB)

    def embed32():
        gather32()
        return ops.linear(out32.view(R * 12, K2D), weight, bias, lowp=True)

    def embed16():
        gather16()
        return ops.linear(out16.view(R * 12, K2D), weight, bias, lowp=True)

    insert = {"computed rows, fp32 slots: din_feat_rows (feats + slot + boxes)":
              (lambda: ops.feat_rows(src_rows, dst32, RB, slot32, zeros, boxes, flags, BB), R * (3 * RB + 2 * BB)),
              "computed rows, bf16 slots: din_feat_rows_bf16 (round once, feats + slot + boxes)":
              (lambda: ops.feat_rows_bf16(src_rows, dst16, NE, slot16, zeros, boxes, flags, BB, ones), R * (RB + 2 * RB16 + 2 * BB))}
    gather = {"resident rows, fp32 slots: din_feat_rows (gather + box comparison)": (gather32, R * (2 * RB + 2 * BB)),
              "resident rows, bf16 slots: din_feat_rows_bf16 (gather + box comparison)": (gather16, R * (2 * RB16 + 2 * BB))}
    with torch.no_grad():
        for forms in (insert, gather):                                    # (the inserts run first: the gathers read what they stored)
            out32.zero_(), out16.zero_()
            for fn, _ in forms.values():
                fn()
            torch.cuda.synchronize()
            assert torch.equal(out32, computed) and torch.equal(out16, computed.to(torch.bfloat16)) and int(flags.sum()) == 0
            for what, r in timed({k: fn for k, (fn, _) in forms.items()}, a.warmup, a.windows, a.inner).items():
                nbytes = forms[what][1]
                gbs = {k.replace("_ms", "_GBps"): round(nbytes / (r[k] * 1e-3) / 1e9, 1) for k in ("median_ms", "min_ms", "p90_ms", "max_ms")}
                emit({"tool": "feature_cache_time", "what": f"{R} rows of {NE} values: " + what, "bytes_read_plus_written": nbytes, **r, **gbs})
        assert torch.equal(embed32(), embed16())                          # the GEMM multiplies the same bf16 operands either way
        embed = {"resident rows, fp32 slots: gather + fc_emb_1 forward (the GEMM rounds feats to bf16 in a pass of its own)": embed32,
                 "resident rows, bf16 slots: gather + fc_emb_1 forward (feats is the bf16 operand)": embed16}
        for what, r in timed(embed, a.warmup, a.windows, a.inner).items():
            emit({"tool": "feature_cache_time", "what": f"{R} rows of {NE} values: " + what, "gemm": [R * 12, K2D, NFB], **r})


def feed_timings(a, emit):
    from din_amd import frame_cache as FC
    from din_amd.config import Config
    from din_amd.dataset import return_dataset
    from din_amd.infer_model import ARG_volleyball
    from din_amd.optim import FusedAdam
    from din_amd.train_net_dynamic import train_volleyball
    dev = torch.device("cuda")
    root = tempfile.mkdtemp(prefix="feature_cache_tree_")
    try:
        t0 = time.perf_counter()
        train_seqs, test_seqs, _, _, nbytes = write_tree(root, a.clips, 9)     # src - 4 .. src + 4: the test split's nine frames exist too
        emit({"tool": "feature_cache_time", "what": "synthetic tree written", "clips": a.clips, "frames_per_clip_on_disk": 9,
              "jpeg_kb_per_frame": round(nbytes / 1e3 / ((a.clips + 2) * 9), 1), "seconds": round(time.perf_counter() - t0, 1)})
        cfg = Config("volleyball")                                              # scripts/train_volleyball_stage2_arg.py, vgg16 set-up
        cfg.inference_module_name, cfg.training_stage, cfg.train_backbone = "arg_volleyball", 2, False
        cfg.backbone, cfg.out_size, cfg.emb_features, cfg.image_size = "vgg16", (22, 40), 512, (720, 1280)
        cfg.batch_size, cfg.test_batch_size, cfg.num_frames, cfg.train_learning_rate = a.batch, 1, 3, 1e-4
        cfg.data_path, cfg.train_seqs, cfg.test_seqs = root, train_seqs, test_seqs
        cfg.num_before, cfg.num_after = 1, 1          # the training draw (3 of the window, no replacement) then takes all 3 frames of a clip
        torch.manual_seed(0)
        model = ARG_volleyball(cfg).to(dev)
        opt = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=cfg.train_learning_rate)
        shape = {"tool": "feature_cache_time", "model": "ARG_volleyball vgg16 fp32, frozen backbone, 720x1280, T=3", "batch": a.batch,
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

        cfg.feature_cache_gb = 0
        ds, vs = return_dataset(cfg)
        off, _ = FC.build_loaders(cfg, ds, vs, a.batch, None, dev, True)
        epoch(off)                                                      # warm-up: code objects, workspaces, the allocator
        cfg.frame_cache_gb = a.cache_gb                                 # the frame cache: pixels resident, the trunk still runs
        ds, vs = return_dataset(cfg, frame_ids=True)
        frames, _ = FC.build_loaders(cfg, ds, vs, a.batch, None, dev, True)
        epoch(frames)
        cfg.frame_cache_gb, cfg.feature_cache_gb = 0, a.cache_gb
        ds, vs = return_dataset(cfg, frame_ids=True)
        on, _ = FC.build_loaders(cfg, ds, vs, a.batch, None, dev, True)
        emit({**shape, "what": "first cached epoch (decode + upload + trunk + insert)", **stats([epoch(on)])})
        rates = {"off": [], "frames": [], "on": []}
        for _ in range(a.epochs):                                       # the three alternate, epoch by epoch
            rates["off"].append(epoch(off))
            rates["frames"].append(epoch(frames))
            rates["on"].append(epoch(on))
        emit({**shape, "what": "epoch, caches off (decode + upload + trunk every epoch)", **stats(rates["off"])})
        emit({**shape, "what": "later epochs with the FRAME cache (cfg.frame_cache_gb: pixels resident, trunk every epoch)", **stats(rates["frames"]),
              "cache": frames.cache.table.counters()})
        emit({**shape, "what": "later cached epochs (gather only: no decode, no upload, no backbone launch)", **stats(rates["on"]),
              "cache": on.cache.table.counters()})
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=320)
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--cache-gb", type=float, default=4.0)
    ap.add_argument("--dtype", choices=("fp32", "bf16"), default="fp32")
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-feed", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("feature_cache_time.py measures on the MI355X: no GPU here, nothing measured")
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        if a.out:                                                        # rewritten after every line: a run cut short keeps what it measured
            with open(a.out, "w") as fh:
                fh.write("Box-feature cache: din_feat_rows and feed rate (tools/feature_cache_time.py), one MI355X:\n" + "\n".join(lines) + "\n")

    if a.dtype == "bf16":
        dtype_timings(a, emit)
    else:
        if not a.skip_kernel:
            kernel_timings(a, emit)
        if not a.skip_feed:
            feed_timings(a, emit)
    emit({"clock": clock()})


if __name__ == "__main__":
    main()
