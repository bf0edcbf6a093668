#!/usr/bin/env python3
"""Flip augmentation: what mirroring costs inside the frame gather (csrc/frame_copy.hip), on one MI355X.

The batch of tools/frame_feed_time.py: 320 rows of 3x720x1280 bytes (32 ten-frame clips) gathered out of a slab of 640 resident frames,
random rows with repeats, address tables and flags already on the device.  Three forms alternate window by window:
  (a) din_copy_rows_u8, the plain gather (the yardstick, measured in the same run);
  (b) din_copy_rows_u8_flip with every row mirrored;
  (c) din_copy_rows_u8_flip with every other clip (ten rows in twenty) mirrored.
Each form's output is checked against torch once before the timing.  Median / min / p90 / max over `--windows` windows of `--inner`
gathers each, GB/s counting the bytes read plus the bytes written, and the ratio of each mirrored form to the plain one.

One JSON line per measurement, then the GPU clock.  usage: python tools/flip_gather_time.py [--out profiles/flip_gather_time.txt]
[--windows 15] [--inner 50] [--warmup 3]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from at_step_time import clock, timed  # noqa: E402

FRAME = (3, 720, 1280)
CLIPS, FRAMES_PER_CLIP, RESIDENT = 32, 10, 640


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from din_amd import ops
    dev = torch.device("cuda")
    rows, fb, width = CLIPS * FRAMES_PER_CLIP, int(np.prod(FRAME)), FRAME[-1]
    lines = fb // width
    slab = torch.randint(0, 256, (RESIDENT, fb), dtype=torch.uint8, device=dev)
    out = torch.empty((rows, fb), dtype=torch.uint8, device=dev)
    idx_host = np.random.default_rng(0).integers(0, RESIDENT, rows)
    idx = torch.from_numpy(idx_host).to(dev)
    src = torch.tensor([slab.data_ptr() + int(i) * fb for i in idx_host], dtype=torch.int64, device=dev)
    dst = torch.tensor([out.data_ptr() + i * fb for i in range(rows)], dtype=torch.int64, device=dev)
    every = torch.ones(rows, dtype=torch.int64, device=dev)
    half_host = np.repeat(np.arange(CLIPS) % 2, FRAMES_PER_CLIP).astype(np.int64)
    half = torch.from_numpy(half_host).to(dev)
    forms = {"din_copy_rows_u8 (plain)": (lambda: ops.copy_rows_u8(src, dst, fb), None),
             "din_copy_rows_u8_flip, every row mirrored": (lambda: ops.copy_rows_u8_flip(src, dst, every, lines, width), every),
             "din_copy_rows_u8_flip, every other clip mirrored": (lambda: ops.copy_rows_u8_flip(src, dst, half, lines, width), half)}
    for what, (fn, flags) in forms.items():                              # the result first: a fast wrong gather is not a gather
        out.zero_()
        fn()
        torch.cuda.synchronize()
        for r0 in range(0, rows, 40):                                    # (in pieces: the mirrored reference needs a copy)
            want = slab[idx[r0:r0 + 40]].view(-1, lines, width)
            if flags is not None:
                want = torch.where(flags[r0:r0 + 40].bool()[:, None, None], want.flip(-1), want)
            assert torch.equal(out[r0:r0 + 40].view(-1, lines, width), want), what
    lines_out = []

    def emit(rec):
        lines_out.append(json.dumps(rec))
        print(lines_out[-1], flush=True)
        if a.out:                                                        # rewritten after every line: a run cut short keeps what it measured
            with open(a.out, "w") as fh:
                fh.write("Flip augmentation: the mirrored against the plain frame gather (tools/flip_gather_time.py), one MI355X:\n"
                         + "\n".join(lines_out) + "\n")

    res = timed({k: fn for k, (fn, _) in forms.items()}, a.warmup, a.windows, a.inner)
    plain = res["din_copy_rows_u8 (plain)"]
    for what, r in res.items():
        gbs = {k.replace("_ms", "_GBps"): round(2 * rows * fb / (r[k] * 1e-3) / 1e9, 1) for k in ("median_ms", "min_ms", "p90_ms", "max_ms")}
        emit({"tool": "flip_gather_time", "what": "gather 320 x 3x720x1280 u8: " + what, "bytes_read_plus_written": 2 * rows * fb, **r, **gbs,
              "median_over_plain_median": round(r["median_ms"] / plain["median_ms"], 4),
              "min_over_plain_min": round(r["min_ms"] / plain["min_ms"], 4)})
    emit({"plain_window_spread_p90_over_min": round(plain["p90_ms"] / plain["min_ms"], 4), "clock": clock()})


if __name__ == "__main__":
    main()
