#!/usr/bin/env python3
"""Colour jitter: what the grey partials and the jittered gather cost against the plain frame gather (csrc/frame_copy.hip), on one MI355X.

The batch of tools/flip_gather_time.py: 320 rows of 3x720x1280 bytes (32 ten-frame clips) gathered out of a slab of 640 resident frames,
random rows with repeats, address tables, flags and factors already on the device, one triple of factors per clip.  The forms alternate
window by window in one process:
  (a) din_copy_rows_u8, the plain gather (the yardstick, measured in the same run);
  (b) din_rows_gray_partials alone;
  (c) din_copy_rows_u8_jitter with all three stages (contrast, brightness, saturation) on every row;
  (d) din_copy_rows_u8_jitter with one stage (brightness) on every row;
  (e) din_copy_rows_u8_jitter with all three stages and every row mirrored;
  (f) (b) then (c): what a jittered batch issues in place of (a).
Rows 0, 1 and the last row of every jittered form are checked against the numpy model (tests/jitter_reference.py) before the timing.
Median / min / p90 / max over `--windows` windows of `--inner` launches each, GB/s counting the bytes a form reads plus the bytes it
writes, and the ratio of each form to the plain gather.

One JSON line per measurement, then the GPU clock.  usage: python tools/jitter_gather_time.py [--out profiles/jitter_gather_time.txt]
[--windows 15] [--inner 30] [--warmup 3]"""
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
from tests import jitter_reference as R  # noqa: E402

FRAME = (3, 720, 1280)
CLIPS, FRAMES_PER_CLIP, RESIDENT = 32, 10, 640


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--inner", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from din_amd import ops
    dev = torch.device("cuda")
    rows, fb, (height, width) = CLIPS * FRAMES_PER_CLIP, int(np.prod(FRAME)), FRAME[1:]
    slab = torch.randint(0, 256, (RESIDENT, fb), dtype=torch.uint8, device=dev)
    out = torch.empty((rows, fb), dtype=torch.uint8, device=dev)
    idx_host = np.random.default_rng(0).integers(0, RESIDENT, rows)
    src = torch.tensor([slab.data_ptr() + int(i) * fb for i in idx_host], dtype=torch.int64, device=dev)
    dst = torch.tensor([out.data_ptr() + i * fb for i in range(rows)], dtype=torch.int64, device=dev)
    every = torch.ones(rows, dtype=torch.int64, device=dev)
    u = np.random.default_rng(1).uniform(-1, 1, (CLIPS, 3))
    three_host = np.repeat((1 + 0.4 * u).astype(np.float32), FRAMES_PER_CLIP, axis=0)         # (contrast, brightness, saturation)
    one_host = np.ones_like(three_host)
    one_host[:, 1] = three_host[:, 1]
    three, one = torch.from_numpy(three_host).to(dev), torch.from_numpy(one_host).to(dev)
    work = torch.empty(rows * ops.gray_partial_segments(height, width), dtype=torch.int32, device=dev)

    def partials():
        ops.rows_gray_partials(src, work, height, width)

    def gather(factors, flags):
        return lambda: ops.copy_rows_u8_jitter(src, dst, flags, factors, work, height, width)

    def both():
        partials()
        gather(three, None)()

    # name -> (launch, bytes read + written, (factors, mirrored) to check against the model or None)
    forms = {"din_copy_rows_u8 (plain)": (lambda: ops.copy_rows_u8(src, dst, fb), 2 * rows * fb, None),
             "din_rows_gray_partials alone": (partials, rows * fb, None),
             "din_copy_rows_u8_jitter, three stages": (gather(three, None), 2 * rows * fb, (three_host, False)),
             "din_copy_rows_u8_jitter, one stage (brightness)": (gather(one, None), 2 * rows * fb, (one_host, False)),
             "din_copy_rows_u8_jitter, three stages, every row mirrored": (gather(three, every), 2 * rows * fb, (three_host, True)),
             "din_rows_gray_partials + din_copy_rows_u8_jitter, three stages": (both, 3 * rows * fb, (three_host, False))}
    partials()
    for what, (fn, _, check) in forms.items():                           # the result first: a fast wrong gather is not a gather
        if check is None:
            continue
        out.zero_()
        fn()
        torch.cuda.synchronize()
        for r in (0, 1, rows - 1):
            frame = slab[int(idx_host[r])].cpu().numpy().reshape(FRAME)
            want = R.jitter(frame, *check[0][r], mirror=check[1])
            assert np.array_equal(out[r].cpu().numpy().reshape(FRAME), want), (what, r)
    parts = work.cpu().numpy().view(np.uint32).reshape(rows, -1)
    assert np.array_equal(parts[0].astype(np.int64), R.gray_partials(slab[int(idx_host[0])].cpu().numpy().reshape(FRAME)))
    lines_out = []

    def emit(rec):
        lines_out.append(json.dumps(rec))
        print(lines_out[-1], flush=True)
        if a.out:                                                        # rewritten after every line: a run cut short keeps what it measured
            with open(a.out, "w") as fh:
                fh.write("Colour jitter: the grey partials and the jittered against the plain frame gather (tools/jitter_gather_time.py), "
                         "one MI355X:\n" + "\n".join(lines_out) + "\n")

    res = timed({k: fn for k, (fn, _, _) in forms.items()}, a.warmup, a.windows, a.inner)
    plain = res["din_copy_rows_u8 (plain)"]
    for what, r in res.items():
        nbytes = forms[what][1]
        gbs = {k.replace("_ms", "_GBps"): round(nbytes / (r[k] * 1e-3) / 1e9, 1) for k in ("median_ms", "min_ms", "p90_ms", "max_ms")}
        emit({"tool": "jitter_gather_time", "what": "320 x 3x720x1280 u8: " + what, "bytes_read_plus_written": nbytes, **r, **gbs,
              "median_over_plain_median": round(r["median_ms"] / plain["median_ms"], 4),
              "min_over_plain_min": round(r["min_ms"] / plain["min_ms"], 4)})
    emit({"plain_window_spread_p90_over_min": round(plain["p90_ms"] / plain["min_ms"], 4), "clock": clock()})


if __name__ == "__main__":
    main()
