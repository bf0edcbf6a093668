"""Box-feature cache: with a frozen backbone the trunk's output for a frame stays in HBM, and a step skips the trunk for it.

`Config` defaults to train_backbone=False and the ARG launcher trains that way; the backbone forward and RoIAlign (reference
infer_model.py:152-184) are then nearly the whole step and do the same work on the same frames every epoch: the volleyball dataset has
no augmentation and a frame's boxes come from the track file, so the fp32 row [N, D, K, K] RoIAlign emits for a frame never changes.
At the launchers' sizes that row is 614 400 bytes for VGG16 (12 x 512 x 25 x 4) and 1 267 200 bytes for Inception-v3 (D = 1056); the
48 300 frames of the whole set are 29.7 GB / 61.2 GB, and an MI355X has 288 GB.  From the second epoch on a step is: gather rows,
fc_emb_1, the head -- nothing decoded, nothing uploaded, no backbone launch.

  * datasets built with `frame_ids=True` and `frame_cache.collate` are the frame cache's (frame_cache.py): a frame whose `resident`
    flag is set is not decoded;
  * `FeatureFeed` uploads only the decoded frames (input_feed.DeviceFeed) and hands the model a `FrameRefs` in place of the images
    tensor: frame ids, the decoded frames, which rows of the batch they are, and the cache;
  * `infer_model.embed_boxes` runs the trunk on those frames only and calls `FeatureCache.rows`: ONE din_feat_rows launch that builds
    feats [B*T, N*D*K*K], stores the new rows in free slots together with their boxes (the slot's trailer), and compares the boxes of
    every row served from a slot with the ones stored there;
  * the feed then marks `dataset.resident` for what went in, and the pass ends with `check()`: one synchronisation, RuntimeError if a
    served row was computed for other boxes than the step's.

One cache or a cache with its mirror cache (below) is one code path throughout, the single cache being the case "every row has
orientation 0": `gather_tables` walks the batch and builds the launch's address tables from SlotTables and plain addresses (host
arithmetic, tested without a device), `FeatureCache.rows` / `rows_both` check their arguments and launch what it built,
infer_model._cached_crops runs the trunk once per orientation, and `CacheFile` loops over one or two (cache, file) entries.

Same store as the frame cache (frame_cache.SlotStore): lazy slabs, no eviction, a full cache stops inserting and the remaining frames
keep being decoded and computed.  Refusals and the cache's lifetime: train_net_dynamic.train_net.

cfg.feature_cache_dtype = 'bf16' (with backbone_dtype = 'bf16' only): the slots hold the row already rounded to bf16, which is what
fc_emb_1's GEMM multiplies in that mode.  Half the bytes per frame, ONE din_feat_rows_bf16 launch that rounds the computed rows on their
way to feats and to the slots, and feats arrives as the GEMM's bf16 operand: no cast pass, the same numbers.

cfg.feature_cache_path (a directory; None = off): the rows outlive the call.  `FeatureCache.save` / `load` move the slots between the
slabs and one data file per cache (feature_cache_file.py: the layout, and the fingerprint that says which runs compute the same rows --
the head, the learning rate and the seed are not part of it); `CacheFile` is a loader's file, loaded before the first pass and written
after every pass in which the cache took frames in.  No kernel of its own: copy_ between pinned buffers and slabs on the current stream.

cfg.feature_cache_flip (with cfg.flip_prob > 0 for the training set, cfg.test_flip for the validation set): the dataset's cache is
accompanied by a MIRROR cache of the same geometry, dtype and capacity, whose row for a frame is the RoIAlign output of the mirrored
frame for the mirrored boxes, and whose trailer holds those boxes -- the bits din_flip_clip_labels produces.  A left-right flip has
exactly two variants, so both can be resident:
  * a decoded frame is computed in both orientations in the step that decodes it (infer_model._cached_crops: one din_copy_rows_u8_flip
    launch over the M decoded frames, one din_flip_clip_labels launch over their boxes, the trunk once per orientation over M frames
    each) and goes into both caches or into neither (`insert_pair`); `dataset.resident` is marked only for frames both caches hold;
  * `FeatureFeed` draws the clips of a training pass as the frame path does (frame_cache.EpochFlips: the same stream) and mirrors the
    batch's labels BEFORE the gather, so the box check compares mirrored boxes with mirrored trailers; `FrameRefs.flipped` tells the
    model call which rows are mirrored;
  * `FeatureCache.rows_both` is `rows` over both caches' slabs: ONE address table, so a batch of resident frames is one din_feat_rows
    (or din_feat_rows_bf16) launch for any mix of orientations;
  * the mirror cache's file stands next to the plain one (`flip_file_name`: train.flip.dinfc); its header says "orientation":
    "mirrored", a plain file's header has no such key, and either offered as the other is refused at load.

cfg.map_cache_gb (`MapCache`, `map_loaders`, `map_refusal`): a second, coarser cache for what the rows above cannot serve --
Dynamic_TCE_volleyball, which reads the backbone's map of every frame, and the collective dataset, whose actor count varies per clip.
A slot keeps the frozen VGG16's output map of a frame (22 x 40 x 512 fp32 = 1 802 240 bytes at the volleyball launchers' sizes, 87 GB for
the 48 300 frames, half of that as bf16; 675 840 bytes for collective at 15 x 22), not the crops cut from it.  Same store, same feed, same
refs and the same one launch (the map is the launch's "row", a 16-byte trailer naming frame and geometry its "boxes"); RoIAlign runs every
step on the gathered maps with the step's own boxes.  No file, no mirror cache, no bf16 slots under an fp32 backbone.
"""
from __future__ import annotations

import collections
import os
import time
from typing import Iterable, Iterator, List, Optional, Tuple

import numpy as np
import torch

from .frame_cache import CachedLoader, SlotStore, _f32_as_table
from .input_feed import DeviceFeed


ORIENTATIONS = ("plain", "mirrored")


def insert_pair(tables, fid: int, grows=None) -> dict:
    """the pair rule: frame `fid` goes into every one of `tables` (frame_cache.SlotTable) that lacks it, or into none of them.
    Returns {index of the table: the new slot} -- empty when a table that lacks the frame has no room (full, frozen, or its slab is
    refused by grows[k]); the tables that already hold the frame keep it.  After a non-empty answer every table holds the frame."""
    fid = int(fid)
    grows = grows or [lambda n: True] * len(tables)
    lacking = [k for k, t in enumerate(tables) if fid not in t.slot_of]
    if not all(tables[k].reserve(grows[k]) for k in lacking):
        return {}
    return {k: tables[k].insert(fid, grows[k]) for k in lacking}


def gather_tables(tables, slot_address, grows, frame_ids, orient, miss_pos, computed, row_bytes: int):
    """the address tables of ONE din_feat_rows launch over one cache, or over a cache and its mirror cache -- host arithmetic only, no
    tensor and no device; ids, orientations and positions are Python ints.  tables: one SlotTable per orientation; slot_address[k](slot) -> address and grows[k] belong to tables[k];
    row i of the batch is frame frame_ids[i] in orientation orient[i] (all 0 with one table); miss_pos: which rows of the batch the
    decoded frames are, each computed in every orientation, copy j of orientation o at computed[o] = (base address, row stride) -- the
    first copy of a frame serves all its rows.  Returns (src, keep, ref, extra, reported):
      * a row whose frame was resident before the call comes from its slot: keep 0, ref = the slot's stored boxes (they are compared);
      * any other row comes from the computed row, ref 0; the first such row of a frame that went in carries keep = its new slot;
      * a decoded frame goes into every table that lacks it or into none (`insert_pair`), the frames taken in the order of their first
        row in the batch; `reported` are the frames for which that took place: every table holds them since this call;
      * `extra`: the inserts of an orientation no row of the batch asks for, as (orientation, frame id, index of the decoded copy),
        plain first, then by copy.  Their entries follow the batch's rows in src / keep / ref; the caller appends their boxes.
    The counters move as if every row were looked up and then stored: one lookup per row of a frame this call did not insert, one miss
    for the row that carries an insert, nothing for the later rows of that frame."""
    ids = list(frame_ids)
    first = {}                                       # frame id -> index of its first decoded copy
    for j, p in enumerate(miss_pos):
        first.setdefault(ids[p], j)
    took, fresh, reported = {}, [set() for _ in tables], []
    for fid in dict.fromkeys(f for f in ids if f in first) if first else ():     # the pair rule, once per decoded frame
        got = insert_pair(tables, fid, grows)
        for k, slot in got.items():
            took[(fid, k)] = slot
            fresh[k].add(fid)
        if got:
            reported.append(fid)
    src, keep, ref = [], [], []
    for fid, o in zip(ids, orient):
        slot = -1 if fid in fresh[o] else tables[o].lookup(fid)
        if slot >= 0:                                # resident before this launch: served from the slot, boxes compared
            src.append(slot_address[o](slot))
            keep.append(0)
            ref.append(src[-1] + row_bytes)
            continue
        if fid not in first:
            which = f" ({ORIENTATIONS[o]})" if len(tables) > 1 else ""
            raise KeyError(f"frame {fid}{which} is neither resident nor among the computed rows of this batch")
        slot = took.pop((fid, o), -1)                # (its first row of this orientation stores it ...
        tables[o].misses += int(slot >= 0)           # ... and is the lookup that missed; the later ones are not looked up)
        base, stride = computed[o]
        src.append(base + first[fid] * stride)
        keep.append(slot_address[o](slot) if slot >= 0 else 0)
        ref.append(0)
    extra = sorted(((k, fid, first[fid]) for fid, k in took), key=lambda e: (e[0], e[2]))
    for k, fid, j in extra:
        base, stride = computed[k]
        src.append(base + j * stride)
        keep.append(slot_address[k](took[(fid, k)]))
        ref.append(0)
    return src, keep, ref, extra, reported


class FeatureCache(SlotStore):
    """Device-resident store of box-feature rows, fp32 or (dtype=torch.bfloat16) rounded to bf16: each slot holds `row_bytes` of
    features in that dtype followed by the `box_bytes` of the boxes they were computed for.  Filled on first use, never beyond
    `capacity_bytes`, no eviction."""

    WHAT, UNIT = "feature cache", "frames"
    MISMATCH = "for other boxes than the ones stored with their features"      # what check() says of a row whose trailer differs
    FLAG_ROWS = 1 << 20                              # rows between two check() calls the flags buffer holds without an extra check

    def __init__(self, device, row_bytes: int, box_bytes: int, capacity_bytes: int, chunk_frames: int = 64,
                 dtype: torch.dtype = torch.float32, orientation: str = "plain"):
        if orientation not in ORIENTATIONS:
            raise ValueError(f"FeatureCache: orientation is one of {ORIENTATIONS}, not {orientation!r}")
        self.orientation = orientation               # "mirrored": the rows of the mirrored frames for the mirrored boxes
        if row_bytes <= 0 or box_bytes <= 0 or row_bytes % 16 or box_bytes % 16:
            raise ValueError(f"FeatureCache: row_bytes {row_bytes} and box_bytes {box_bytes} must be positive multiples of 16")
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"FeatureCache: rows are stored as torch.float32 or torch.bfloat16, not {dtype}")
        self.row_bytes, self.box_bytes, self.dtype = int(row_bytes), int(box_bytes), dtype
        self.row_elems = self.row_bytes // (4 if dtype == torch.float32 else 2)
        super().__init__(device, self.row_bytes + self.box_bytes, capacity_bytes, chunk_frames)
        self.flags: Optional[torch.Tensor] = None    # one uint8 per row gathered since the last check(); din_feat_rows only ever writes 1
        self._flagged: List[np.ndarray] = []         # the frame ids of those rows, in order
        self._used = 0
        self._file_bufs: Optional[List[torch.Tensor]] = None        # save / load: two pinned buffers of one slab each

    def _flag_rows(self, ids: np.ndarray) -> torch.Tensor:
        if self.flags is None:
            self.flags = torch.zeros(max(self.FLAG_ROWS, len(ids)), dtype=torch.uint8, device=self.device)
        if self._used + len(ids) > self.flags.numel():
            self.check()
            if len(ids) > self.flags.numel():
                self.flags = torch.zeros(len(ids), dtype=torch.uint8, device=self.device)
        view = self.flags[self._used:self._used + len(ids)]
        self._flagged.append(ids)
        self._used += len(ids)
        return view

    def _step_boxes(self, who: str, rows: int, boxes: torch.Tensor) -> torch.Tensor:
        """the step's boxes as the launch reads them: fp32 on the device, `box_bytes` a row, contiguous, 16-byte aligned (a row at a
        misaligned address would be left alone by din_feat_rows: no trailer, no box check, no error)"""
        if not boxes.is_cuda or boxes.dtype != torch.float32 or boxes.numel() * 4 != rows * self.box_bytes:
            raise ValueError(f"{who}: {rows} rows need fp32 device boxes of {self.box_bytes} bytes each, got {tuple(boxes.shape)} {boxes.dtype}")
        boxes = boxes.contiguous()
        return boxes.clone() if boxes.data_ptr() % 16 else boxes

    @staticmethod
    def _computed(t, shape) -> bool:
        """whether `t` can be a launch's computed rows, or their boxes: a contiguous, 16-byte aligned fp32 device tensor of this shape"""
        return t is not None and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == tuple(shape) \
            and t.data_ptr() % 16 == 0

    def rows(self, frame_ids, boxes: torch.Tensor, miss_pos=(), miss_rows: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, List[int]]:
        """frame_ids [R] (host), boxes fp32 [R, box_bytes / 4] on the device (this step's boxes of every row), miss_pos [M] (host: which
        of the R rows the computed rows are), miss_rows fp32 [M, row_elems] on the device -> (`dtype` [R, row_elems] on the device,
        the frame ids inserted by this call).  One launch on the current stream: a row comes from its slot (and its boxes are compared
        with the slot's) or from the computed row, which also goes into a free slot with its boxes while the cache has room.  A frame
        that occurs twice is served both times from the computed row, never from the slot written by this launch.  With bf16 storage
        the computed rows still arrive as fp32 and the launch rounds them (din_feat_rows_bf16)."""
        pos = np.asarray(miss_pos, dtype=np.int64).reshape(-1)
        M = len(pos)
        if M and not self._computed(miss_rows, (M, self.row_elems)):
            raise ValueError(f"rows: {M} computed rows need a contiguous, 16-byte aligned fp32 device tensor "
                             f"{(M, self.row_elems)}, got {None if miss_rows is None else tuple(miss_rows.shape)}")
        return self._gather("rows", (self,), frame_ids, None, boxes, pos, (miss_rows,), None)

    def rows_both(self, mirror: "FeatureCache", frame_ids, flipped, boxes: torch.Tensor, miss_pos=(), miss_rows=None,
                  miss_boxes=None) -> Tuple[torch.Tensor, List[int]]:
        """`rows` over this cache and its mirror cache with ONE address table and ONE launch: row i is frame frame_ids[i] as decoded,
        or mirrored where flipped[i] (host, bool [R]; None: no row), and comes from the slot of the cache of its orientation or from
        the computed row of that orientation.  boxes: this step's boxes of every row, mirrored where the row is.  The M decoded
        frames (miss_pos [M]: one row of the batch each) arrive computed in BOTH orientations: miss_rows = (fp32 [M, row_elems] of the
        frames as decoded, the same of the mirrored frames), miss_boxes = (fp32 [M, box_bytes / 4] unmirrored, mirrored).  A decoded
        frame goes into both caches or into neither (`insert_pair`); an orientation that no row of the batch asks for is stored by an
        extra row of the same launch, with its own boxes.  Returns (`dtype` [R, row_elems], the frame ids that BOTH caches hold
        since this call).  The flags of all rows are this cache's: `check()` on it reports a mismatch in either orientation."""
        if not isinstance(mirror, FeatureCache) or (mirror.row_bytes, mirror.box_bytes, mirror.dtype) != (self.row_bytes, self.box_bytes, self.dtype):
            raise ValueError("rows_both: the mirror cache is a FeatureCache of the same row_bytes, box_bytes and dtype")
        pos = np.asarray(miss_pos, dtype=np.int64).reshape(-1)
        M = len(pos)
        for what, pair, shape in (("computed rows", miss_rows, (M, self.row_elems)), ("boxes of the computed rows", miss_boxes, (M, self.box_bytes // 4))):
            if M and (pair is None or len(pair) != 2 or not all(self._computed(t, shape) for t in pair)):
                raise ValueError(f"rows_both: the {what} are two contiguous, 16-byte aligned fp32 device tensors {shape}, one per orientation")
        return self._gather("rows_both", (self, mirror), frame_ids, flipped, boxes, pos, miss_rows, miss_boxes)

    def _gather(self, who: str, caches, frame_ids, flipped, boxes: torch.Tensor, pos: np.ndarray, miss_rows, miss_boxes):
        """`rows` / `rows_both` behind the checks of their computed rows: the address tables (`gather_tables`), `out`, the flags, the launch"""
        ids = np.asarray(frame_ids, dtype=np.int64).reshape(-1)
        orient = [0] * len(ids) if flipped is None else (np.asarray(flipped).reshape(-1) != 0).astype(np.int64).tolist()
        if len(orient) != len(ids):
            raise ValueError(f"{who}: {len(orient)} orientation flags for {len(ids)} rows")
        rb, ne = self.row_bytes, self.row_elems
        boxes = self._step_boxes(who, len(ids), boxes)
        if len(pos) and (pos.min() < 0 or pos.max() >= len(ids)):
            raise ValueError(f"{who}: miss_pos outside the batch")
        computed = [(t.data_ptr(), ne * 4) for t in miss_rows] if len(pos) else []
        src, keep, ref, extra, reported = gather_tables([c.table for c in caches], [c.slot_address for c in caches], [c._grow for c in caches],
                                                        ids.tolist(), orient, pos.tolist(), computed, rb)
        if extra:                                    # (their boxes are the decoded copies' of that orientation; their copies land behind the batch's)
            picks = [miss_boxes[k].index_select(0, torch.tensor([j for kk, _, j in extra if kk == k], dtype=torch.int64, device=boxes.device))
                     for k in sorted({k for k, _, _ in extra})]
            boxes = torch.cat([boxes.reshape(len(ids), -1)] + picks)
            ids = np.concatenate([ids, np.asarray([f for _, f, _ in extra], dtype=np.int64)])
        out = torch.empty((len(ids), ne), dtype=self.dtype, device=self.device)
        out_ptr = out.data_ptr()
        self._launch(src, [out_ptr + i * rb for i in range(len(ids))], keep, ref, boxes, self._flag_rows(ids))
        return out[:len(orient)], reported

    def _launch(self, src, dst, keep, ref, boxes: torch.Tensor, flags: torch.Tensor) -> None:
        """the one launch of a gather: din_feat_rows, or din_feat_rows_bf16 for bf16 slots"""
        from . import ops
        if self.dtype == torch.float32:
            d_src, d_dst, d_keep, d_ref = self._upload(src, dst, keep, ref)
            ops.feat_rows(d_src, d_dst, self.row_bytes, d_keep, d_ref, boxes, flags, self.box_bytes)
        else:                                        # a row without a stored-boxes address is a computed one: fp32, to be rounded
            d_src, d_dst, d_keep, d_ref, d_f32 = self._upload(src, dst, keep, ref, [int(r == 0) for r in ref])
            ops.feat_rows_bf16(d_src, d_dst, self.row_elems, d_keep, d_ref, boxes, flags, self.box_bytes, d_f32)

    def check(self) -> None:
        """end of a pass: synchronise once, read the flags of every row gathered since the last check, clear them; RuntimeError naming
        the frames whose boxes differ from the ones stored with their features"""
        if self.flags is None or self._used == 0:
            return
        got = self.flags[:self._used].cpu().numpy()                  # (the copy synchronises)
        ids = np.concatenate(self._flagged)
        self.flags[:self._used].zero_()
        self._flagged, self._used = [], 0
        bad = np.flatnonzero(got)
        if bad.size:
            raise RuntimeError(f"{self.WHAT}: {bad.size} rows were served {self.MISMATCH} "
                               f"(row, frame id): {[(int(r), int(ids[r])) for r in bad[:16]]}{' ...' if bad.size > 16 else ''}")

    # ---- the cache on disk (feature_cache_file.py: the layout and the fingerprint; train_net_dynamic: when) -------------------------------
    # Bytes move between a file, two pinned host buffers and the slabs with copy_ on the current stream -- the stream whose launches wrote
    # the slots and will read them -- so the copies are ordered with those launches, and the host waits only on the event recorded behind
    # each copy.  No kernel is launched.
    def _staging(self, k: int) -> torch.Tensor:
        """pinned buffer k of the two a slab's worth of records travels through"""
        if self._file_bufs is None:
            n = self.table.chunk_frames * self.table.stride
            self._file_bufs = [torch.empty(n, dtype=torch.uint8).pin_memory() for _ in range(2)]
        return self._file_bufs[k % 2]

    def file_meta(self, fingerprint: dict) -> dict:
        """what a file of this cache says about itself besides its count: the fingerprint and the slots' geometry"""
        meta = {"fingerprint": fingerprint, "row_bytes": self.row_bytes, "box_bytes": self.box_bytes,
                "dtype": "fp32" if self.dtype == torch.float32 else "bf16"}
        if self.orientation != "plain":              # (a plain cache's header is what it always was)
            meta["orientation"] = self.orientation
        return meta

    def _slab_blocks(self, count: int) -> Iterator[np.ndarray]:
        """the first `count` slots as host byte blocks, slab by slab (the slots of a slab are contiguous in device memory): the copy of
        slab k+1 is in flight while the consumer works on slab k"""
        stream = torch.cuda.current_stream(self.device)
        cf, stride = self.table.chunk_frames, self.table.stride
        used = [min(cf, count - k * cf) * stride for k in range((count + cf - 1) // cf)]
        events: List[torch.cuda.Event] = []

        def start(k):
            self._staging(k)[:used[k]].copy_(self.slabs[k][:used[k]], non_blocking=True)
            events.append(torch.cuda.Event())
            events[-1].record(stream)

        if used:
            start(0)
        for k in range(len(used)):
            if k + 1 < len(used):                    # (into the other buffer: the consumer has finished with it, it asked for this block)
                start(k + 1)
            events[k].synchronize()
            yield self._staging(k).numpy()[:used[k]]

    def save(self, path: str, meta: dict) -> int:
        """write every resident row, with its boxes, to `path` (meta: the run's fingerprint, feature_cache_file.fingerprint); returns the
        number of frames written.  Slot order, slab by slab, device to host through two pinned buffers in rotation; the file appears
        under its name only when it is complete (feature_cache_file.write)."""
        from . import feature_cache_file as FF
        ids = np.fromiter(self.table.slot_of.keys(), dtype=np.int64, count=len(self.table.slot_of))
        assert list(self.table.slot_of.values()) == list(range(len(ids)))       # (slots are handed out in order and never given back)
        FF.write(path, self.file_meta(meta), ids, self._slab_blocks(len(ids)))
        return int(len(ids))

    def load(self, path: str, meta: dict) -> List[int]:
        """take in the rows of the file at `path`, written by `save` of a run with the same fingerprint; returns the frame ids that are
        resident afterwards, in file order.  ValueError naming the first field of the fingerprint that differs from `meta`, or the
        geometry that differs from this cache's -- before anything is inserted.  Ids go in in file order (table.insert: slabs grow as for
        computed rows); a file with more frames than the capacity admits gives its prefix, and the rest is logged and left to be
        computed.  The boxes travel inside the records, so din_feat_rows checks a loaded row exactly as a computed one."""
        from . import feature_cache_file as FF
        from .frame_cache import log
        header, ids, records = FF.read(path)
        theirs = header.get("orientation", "plain")
        if theirs != self.orientation:
            raise ValueError(f"feature cache file {path} holds the rows of the {theirs} frames and is offered to the cache of the "
                             f"{self.orientation} ones (a renamed file?): a mirror cache's file is `flip_file_name`'s, next to the plain "
                             f"one.  It is neither used nor overwritten")
        field = FF.first_difference(meta, header["fingerprint"])
        if field is not None:
            raise ValueError(f"feature cache file {path} was written for another {field} ({header['fingerprint'].get(field)!r}, this run "
                             f"has {meta.get(field)!r}): its rows are not the ones this run would compute.  It is neither used nor "
                             f"overwritten: delete it, or point feature_cache_path elsewhere")
        mine = self.file_meta(meta)
        for k in ("row_bytes", "box_bytes", "dtype"):
            if header[k] != mine[k]:
                raise ValueError(f"feature cache file {path} holds {k} = {header[k]!r}, this cache {mine[k]!r}")
        stream = torch.cuda.current_stream(self.device)
        stride, cf = self.table.stride, self.table.chunk_frames
        runs: List[List[int]] = []                   # [first file index, first slot, length]: contiguous in the file and inside one slab
        resident: List[int] = []
        for i, fid in enumerate(ids):
            fid = int(fid)
            if fid in self.table.slot_of:            # (already there, with the same fingerprint: the same bytes)
                resident.append(fid)
                continue
            slot = self.table.insert(fid, self._grow)
            if slot < 0:
                break
            resident.append(fid)
            last = runs[-1] if runs else None
            if last and last[0] + last[2] == i and last[1] + last[2] == slot and slot % cf:
                last[2] += 1
            else:
                runs.append([i, slot, 1])
        events: List[Optional[torch.cuda.Event]] = [None, None]
        for k, (i, slot, n) in enumerate(runs):
            if events[k % 2] is not None:
                events[k % 2].synchronize()          # the copy this buffer last fed has finished
            host = self._staging(k)
            host.numpy()[:n * stride] = records[i:i + n].reshape(-1)      # (the file read: page faults of the memmap)
            slab, off = self.table.locate(slot)
            self.slabs[slab][off:off + n * stride].copy_(host[:n * stride], non_blocking=True)
            events[k % 2] = torch.cuda.Event()
            events[k % 2].record(stream)
        for e in events:
            if e is not None:
                e.synchronize()
        if len(resident) < len(ids):
            log.warning("%s: %d of the %d %s of %s are resident; the capacity admits no more, the other %d will be computed", self.WHAT,
                        len(resident), len(ids), self.UNIT, path, len(ids) - len(resident))
        return resident


class MapCache(FeatureCache):
    """cfg.map_cache_gb: the coarser sibling of the box-feature cache.  A slot holds the raw bytes of one frame of the frozen backbone's
    output map as `forward_nhwc` returns it (NHWC [OH, OW, C], the backbone's dtype, padded channels included), followed by a 16-byte
    trailer of four fp32 numbers that name it: frame id, OH, OW, C.  A map does not depend on boxes, so RoIAlign runs every step on the
    step's own boxes, whatever their number (the collective dataset), and the map itself is the context Dynamic_TCE_volleyball reads.

    The store, the address tables and the ONE din_feat_rows launch per step are FeatureCache's, unchanged: the launch is byte-agnostic,
    so a map travels as the `row_bytes / 4` opaque 32-bit words of a "row" and the trailer as its "boxes".  The comparison the launch
    makes on every served row becomes an integrity check: the slot holds the frame and the geometry that was asked for.

    What infer_model._crops reads off the backbone's graph -- the output tensor's `relu_masked` flag and its dtype -- is not to be had in
    a step that runs no trunk, so it is recorded here with the first insert (`map_dtype`, `relu_masked`)."""

    WHAT = "map cache"
    MISMATCH = "from slots whose trailer names another frame or map geometry than the one asked for"
    TRAILER_BYTES = 16
    MAX_ID = 1 << 24                                 # frame ids and sizes up to here are exact as fp32

    def __init__(self, device, map_shape, itemsize: int, capacity_bytes: int, chunk_frames: int = 64):
        self.map_shape = tuple(int(v) for v in map_shape)
        if len(self.map_shape) != 3 or min(self.map_shape) <= 0 or max(self.map_shape) >= self.MAX_ID or itemsize not in (2, 4):
            raise ValueError(f"MapCache: a map is [OH, OW, C] of 2- or 4-byte elements, got {map_shape!r} x {itemsize} bytes")
        self.itemsize = int(itemsize)
        super().__init__(device, int(np.prod(self.map_shape)) * self.itemsize, self.TRAILER_BYTES, capacity_bytes, chunk_frames)
        self.map_dtype: Optional[torch.dtype] = None
        self.relu_masked: Optional[bool] = None

    def trailers(self, frame_ids) -> np.ndarray:
        """float32 [R, 4]: (frame id, OH, OW, C) of every row -- what a slot's trailer holds and what a served row is compared with"""
        ids = np.asarray(frame_ids, dtype=np.int64).reshape(-1)
        if len(ids) and (ids.min() < 0 or ids.max() >= self.MAX_ID):
            raise ValueError(f"map cache: frame ids lie in [0, {self.MAX_ID}) (exact as fp32), got {int(ids.min())} .. {int(ids.max())}")
        out = np.empty((len(ids), 4), dtype=np.float32)
        out[:, 0], out[:, 1:] = ids, self.map_shape
        return out

    def _describe(self, computed: torch.Tensor, relu_masked: bool) -> None:
        """the first computed maps say what the slots hold; every later call must bring the same"""
        OH, OW, C = self.map_shape
        if not computed.is_cuda or tuple(computed.shape[1:]) != self.map_shape or computed.element_size() != self.itemsize:
            raise ValueError(f"map cache: the slots hold [{OH}, {OW}, {C}] maps of {self.itemsize}-byte elements (cfg.out_size, "
                             f"cfg.emb_features, cfg.backbone_dtype); the backbone returned {tuple(computed.shape[1:])} {computed.dtype}")
        if self.map_dtype is None:
            self.map_dtype, self.relu_masked = computed.dtype, bool(relu_masked)
        elif (self.map_dtype, self.relu_masked) != (computed.dtype, bool(relu_masked)):
            raise ValueError(f"map cache: the slots hold {self.map_dtype} maps with relu_masked = {self.relu_masked}; the backbone now "
                             f"returned {computed.dtype} with relu_masked = {bool(relu_masked)}")

    def maps(self, frame_ids, miss_pos=(), computed: Optional[torch.Tensor] = None, relu_masked: bool = False) -> Tuple[torch.Tensor, List[int]]:
        """frame_ids [R] (host), miss_pos [M] (host: which of the R rows the computed maps are), computed [M, OH, OW, C] on the device
        (bufs[0] of backbone.forward_nhwc over exactly those M frames; relu_masked: its output tensor's flag) -> (fm [R, OH, OW, C] in
        the backbone's dtype, the frame ids inserted by this call).  `FeatureCache.rows` with the trailers as boxes: one launch; a frame
        that occurs twice is served both times from the computed map, a full cache serves computed maps without keeping them."""
        pos = np.asarray(miss_pos, dtype=np.int64).reshape(-1)
        words = None
        if len(pos):
            if computed is None or computed.dim() != 4 or computed.shape[0] != len(pos):
                raise ValueError(f"maps: {len(pos)} computed maps need a device tensor [{len(pos)}, OH, OW, C], got "
                                 f"{None if computed is None else tuple(computed.shape)}")
            self._describe(computed, relu_masked)
            words = computed.contiguous().reshape(len(pos), -1).view(torch.float32)
        t = self.trailers(frame_ids)
        d_trailers, = self._upload(_f32_as_table(t))
        out, new_ids = self.rows(frame_ids, d_trailers.view(torch.float32)[:t.size].reshape(len(t), 4), pos, words)
        if self.map_dtype is None:                   # (no row at all: rows() has raised KeyError for any row it could not serve)
            return out.reshape((0,) + self.map_shape), new_ids
        return out.view(self.map_dtype).reshape((len(t),) + self.map_shape), new_ids


class FrameRefs:
    """what a model receives in place of the images tensor when box features are cached: the frame ids of the batch [B, T] (host), the
    frames that were decoded (uint8 [M, 3, H, W] on the device), which of the B*T rows they are (`miss_pos`, host; `miss_pos_dev` the
    same on the device when the feed uploaded it), and the cache.  `shape` and `reshape` of the two leading dimensions are all the
    models and trainers use of an images tensor besides handing it to infer_model.embed_boxes, which sets `inserted`.  `cache` may be
    a MapCache (cfg.map_cache_gb): the same refs, fed by the same FeatureFeed; embed_boxes then also leaves the gathered maps in `context`.

    With a mirror cache (`mirror`, cfg.feature_cache_flip) every row has an orientation: `flipped` (host, bool [B, T]; None: no row is
    mirrored) says which rows are the mirrored frame, and the boxes the model receives are mirrored in those rows.  `plain_boxes` (the
    batch's boxes before any was mirrored, on the device) is needed only when a decoded frame sits in a mirrored row: its unmirrored
    boxes cannot be had back from the mirrored ones bit for bit.  `inserted` then lists the frames BOTH caches hold since the call."""

    def __init__(self, frame_ids, miss_images: torch.Tensor, miss_pos, cache: FeatureCache, miss_pos_dev: Optional[torch.Tensor] = None,
                 mirror: Optional[FeatureCache] = None, flipped=None, plain_boxes: Optional[torch.Tensor] = None):
        self.frame_ids = np.asarray(frame_ids, dtype=np.int64)
        if self.frame_ids.ndim != 2:
            raise ValueError(f"FrameRefs: frame_ids is [B, T], got shape {self.frame_ids.shape}")
        if miss_images.dim() != 4 or miss_images.shape[1] != 3:
            raise ValueError(f"FrameRefs: miss_images is [M, 3, H, W], got {tuple(miss_images.shape)}")
        self.miss_images, self.cache = miss_images, cache
        self.miss_pos = np.asarray(miss_pos, dtype=np.int64).reshape(-1)
        if len(self.miss_pos) != miss_images.shape[0]:
            raise ValueError(f"FrameRefs: {miss_images.shape[0]} decoded frames but {len(self.miss_pos)} positions")
        self.miss_pos_dev = miss_pos_dev
        self.inserted: List[int] = []
        self.context = None                          # with a MapCache: (fm [B*T, OH, OW, C], its relu_masked flag), set by the model call
        self.mirror, self.plain_boxes = mirror, plain_boxes
        self.flipped = None if flipped is None else np.asarray(flipped).astype(bool)
        if self.flipped is not None and self.flipped.shape != self.frame_ids.shape:
            raise ValueError(f"FrameRefs: flipped is bool {self.frame_ids.shape} like frame_ids, got shape {self.flipped.shape}")
        if self.flipped is not None and mirror is None:
            raise ValueError("FrameRefs: mirrored rows need the mirror cache they are served from")

    @property
    def shape(self) -> Tuple[int, ...]:
        return tuple(self.frame_ids.shape) + tuple(self.miss_images.shape[1:])

    def reshape(self, *shape) -> "FrameRefs":
        shape = tuple(shape[0]) if len(shape) == 1 and isinstance(shape[0], (tuple, list)) else tuple(shape)
        if len(shape) != 5 or tuple(shape[2:]) != self.shape[2:] or shape[0] * shape[1] != self.frame_ids.size:
            raise ValueError(f"FrameRefs.reshape: only the two leading dimensions of {self.shape} can be reshaped, got {shape}")
        return self._but(frame_ids=self.frame_ids.reshape(shape[0], shape[1]),
                         flipped=None if self.flipped is None else self.flipped.reshape(shape[0], shape[1]))

    def mirrored(self, plain_boxes: torch.Tensor) -> "FrameRefs":
        """the same frames in the other orientation, every row (test-time flipping: the caller mirrors the boxes it hands to the model
        and passes the ones it mirrored them from)"""
        return self._but(flipped=np.ones(self.frame_ids.shape, dtype=bool) if self.flipped is None else ~self.flipped, plain_boxes=plain_boxes)

    def _but(self, **changed) -> "FrameRefs":
        """these refs with `changed` constructor arguments; `inserted` is shared: the feed reads it off the object it yielded"""
        out = FrameRefs(**{**dict(frame_ids=self.frame_ids, miss_images=self.miss_images, miss_pos=self.miss_pos, cache=self.cache,
                                  miss_pos_dev=self.miss_pos_dev, mirror=self.mirror, flipped=self.flipped, plain_boxes=self.plain_boxes), **changed})
        out.inserted = self.inserted
        return out


class _HostSide:
    """what FeatureFeed hands to DeviceFeed: the tensors to upload (decoded frames, their positions, labels), the frame ids kept back"""

    def __init__(self, loader, kept: collections.deque):
        self.loader, self.kept = loader, kept

    def __iter__(self):
        for frame_ids, miss_images, miss_pos, *labels in self.loader:
            self.kept.append((frame_ids.numpy(), miss_pos.numpy()))
            yield (miss_images, miss_pos, *labels)

    def __len__(self):
        return len(self.loader)


class FeatureFeed:
    """frame_cache.CachedFeed's contract over the same `collate`d batches: yields (FrameRefs, *labels) with the labels on the device.
    Only the frames the workers decoded are uploaded; after the model call `dataset.resident` is marked for the frames whose features
    went into the cache, so the loader stops decoding them.

    With a mirror cache (`mirror`) the frames go into both caches, `resident` is marked for those both hold, and `augment` (the pass's
    frame_cache.PassAugment, its flips only) mirrors clips: one draw per batch from the stream the frame path draws from, the labels
    mirrored by the one din_flip_clip_labels launch BEFORE the model call, the rows' orientations in `FrameRefs.flipped`.  A batch in
    which nothing is drawn is fed exactly as without `augment`."""

    def __init__(self, loader: Iterable, device, cache: FeatureCache, dataset, augment=None, mirror: Optional[FeatureCache] = None):
        self.loader, self.device, self.cache, self.dataset = loader, torch.device(device), cache, dataset
        self.augment, self.mirror = augment, mirror
        self._kept: collections.deque = collections.deque()
        self._feed = DeviceFeed(_HostSide(loader, self._kept), self.device)

    def __iter__(self) -> Iterator:
        self._kept.clear()
        for miss_images, miss_pos_dev, *labels in self._feed:
            ids, pos = self._kept.popleft()
            rows = None if self.augment is None else self.augment.rows(ids.shape[0], ids.shape[1])[0]
            if rows is None:
                refs = FrameRefs(ids, miss_images, pos, self.cache, miss_pos_dev, self.mirror)
            else:
                plain_boxes = labels[0].clone() if len(pos) else None        # (only a decoded frame's unmirrored boxes are ever needed)
                d_flags, = self.cache._upload(rows.astype(np.int64))
                self.augment.mirror_labels(labels, d_flags)
                refs = FrameRefs(ids, miss_images, pos, self.cache, miss_pos_dev, self.mirror, rows.reshape(ids.shape), plain_boxes)
            yield (refs, *labels)
            if refs.inserted:                        # (filled by embed_boxes during the model call)
                self.dataset.resident[torch.as_tensor(refs.inserted, dtype=torch.int64)] = 1

    def check(self) -> None:
        self.cache.check()

    def __len__(self):
        return len(self.loader)


class FeatureLoader(CachedLoader):
    """a DataLoader of a `frame_ids=True` dataset together with the feature cache of that dataset: what the stage-2 trainer's passes
    receive in place of the loader when cfg.feature_cache_gb > 0.  `mirror`: the mirror cache of the dataset (cfg.feature_cache_flip),
    None without one"""

    def __init__(self, loader, cache, dataset, mirror: Optional[FeatureCache] = None):
        super().__init__(loader, cache, dataset)
        self.mirror = mirror

    def feed(self, device, augment=None) -> FeatureFeed:
        if augment is not None and augment.flip is not None and self.mirror is None:   # (train_net refuses first: frame_cache.flip_refusal)
            raise ValueError("flip augmentation cannot be fed from the feature cache: its rows belong to the unmirrored frames "
                             "(cfg.feature_cache_flip gives the loader a mirror cache)")
        if augment is not None and augment.jitter is not None:     # (likewise: frame_cache.jitter_refusal)
            raise ValueError("colour jitter cannot be fed from the feature cache: its rows belong to the frames as decoded")
        if self.mirror is None:
            return FeatureFeed(self.loader, device, self.cache, self.dataset)
        return FeatureFeed(self.loader, device, self.cache, self.dataset, augment, self.mirror)


class CacheFile:
    """the file one FeatureLoader's cache is kept in between runs (cfg.feature_cache_path): `load` before the first pass, `save_if_grown`
    after every pass.  `loaded` / `saved` count frames; `say` takes the one log line of every load and save.  A loader with a mirror
    cache keeps that one in `flip_path`, by the same rules (`flip_loaded` / `flip_saved`); only frames that both files gave are marked
    resident."""

    def __init__(self, loader: FeatureLoader, path: str, meta: dict, say=print, flip_path: Optional[str] = None):
        self.loader, self.path, self.meta, self.say = loader, path, meta, say
        self.loaded = self.saved = 0
        mirror = getattr(loader, "mirror", None)
        self.flip_path = flip_path if mirror is not None else None
        self.flip_loaded = self.flip_saved = self.flip_written = 0  # (flip_written: by the last save_if_grown call, 0 if it wrote none)
        # (cache, its file, what its counters are called before "loaded" / "saved" / "written"), the plain one first
        self._files = [(loader.cache, path, "")] + ([(mirror, flip_path, "flip_")] if mirror is not None else [])
        self._on_file = [0] * len(self._files)       # each table's `inserted` when its file was last read or written

    @property
    def inserted(self) -> int:
        return sum(cache.table.inserted for cache, _, _ in self._files)

    def _line(self, verb: str, frames: int, seconds: float, path: str) -> None:
        gb = frames * self.loader.cache.table.stride / 1e9
        self.say(f"feature cache {verb} {path}: {frames} frames, {gb:.3f} GB, {seconds:.2f} s")

    def load(self) -> int:
        """take in each file there is, and mark the frames every cache of the loader got from its file resident, so that the loader's
        workers stop decoding them -- what the in-memory cache does from its second epoch.  A file of another fingerprint is a
        ValueError (FeatureCache.load)."""
        got = []
        for k, (cache, path, name) in enumerate(self._files):
            ids = []
            if os.path.exists(path):
                t0 = time.perf_counter()
                ids = cache.load(path, self.meta)
                self._line("loaded from", len(ids), time.perf_counter() - t0, path)
            setattr(self, name + "loaded", len(ids))
            self._on_file[k] = cache.table.inserted
            got.append(ids)
        held = sorted(set(got[0]).intersection(*got[1:]))
        flags = self.loader.dataset.resident
        if held and (held[0] < 0 or held[-1] >= flags.numel()):
            which = f"file {self.path} names" if self.flip_path is None else f"files {self.path} and {self.flip_path} name"
            raise ValueError(f"feature cache {which} frames outside the dataset's table of {flags.numel()} frames")
        if held:
            flags[torch.as_tensor(held, dtype=torch.int64)] = 1
        return self.loaded

    def save_if_grown(self, inserted_before: int) -> int:
        """after a pass: if a cache took frames in during the pass (`inserted_before`: `inserted` read before it), write each cache that
        took frames in since its file was last read or written, whole; returns the frames written to the plain cache's file, 0 for a
        pass that only read (`flip_written`: the same of the mirror cache's file)."""
        self.flip_written = 0
        if self.inserted == inserted_before:
            return 0
        wrote = {}
        for k, (cache, path, name) in enumerate(self._files):
            if cache.table.inserted == self._on_file[k]:
                continue
            t0 = time.perf_counter()
            os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
            wrote[name] = cache.save(path, self.meta)
            self._on_file[k] = cache.table.inserted
            setattr(self, name + "saved", wrote[name])
            self._line("saved to", wrote[name], time.perf_counter() - t0, path)
        self.flip_written = wrote.get("flip_", 0)
        return wrote.get("", 0)


def cache_files(cfg, model, training_loader, validation_loader, rank: int = 0, world: int = 1, say=print) -> dict:
    """{"train": CacheFile, "val": CacheFile} for cfg.feature_cache_path, {} without the setting or without feature caches behind the
    loaders (no real dataset tree).  The fingerprints are taken here: call it when the backbone has its stage-1 weights."""
    from . import feature_cache_file as FF
    folder = getattr(cfg, "feature_cache_path", None)
    if folder is None or not (isinstance(training_loader, FeatureLoader) and isinstance(validation_loader, FeatureLoader)):
        return {}
    return {split: CacheFile(ld, os.path.join(str(folder), FF.file_name(split, rank, world)), FF.fingerprint(cfg, model, ld.dataset), say,
                             os.path.join(str(folder), FF.flip_file_name(split, rank, world)))
            for split, ld in (("train", training_loader), ("val", validation_loader))}


def path_refusal(cfg) -> Optional[str]:
    """why cfg.feature_cache_path cannot be honoured, or None (train_net_dynamic.train_net raises ValueError with it)"""
    if getattr(cfg, "feature_cache_path", None) is None or float(getattr(cfg, "feature_cache_gb", 0) or 0) > 0:
        return None
    return (f"feature_cache_path = {cfg.feature_cache_path!r}: the files there hold the rows of the box-feature cache, and feature_cache_gb "
            f"is {getattr(cfg, 'feature_cache_gb', 0)}: there is no cache to load them into or to save")


DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}      # cfg.feature_cache_dtype -> what the slots hold


def row_and_box_bytes(cfg, dtype: torch.dtype = torch.float32) -> Tuple[int, int]:
    """bytes of one frame's RoIAlign output [N, D, K, K] stored as `dtype` and of its fp32 boxes [N, 4]"""
    K = cfg.crop_size[0]
    return cfg.num_boxes * cfg.emb_features * K * K * (4 if dtype == torch.float32 else 2), cfg.num_boxes * 16


def feature_loaders(cfg, training_loader, validation_loader, training_set, validation_set, device):
    """frame_cache.build_loaders with cfg.feature_cache_gb > 0: one FeatureCache of that many GB per dataset, and with
    cfg.feature_cache_flip a mirror cache beside it where mirrored clips are asked for: the training set's with flip_prob > 0, the
    validation set's with test_flip"""
    capacity = int(float(cfg.feature_cache_gb) * 1e9)
    dtype = DTYPES[getattr(cfg, "feature_cache_dtype", "fp32")]
    rb, bb = row_and_box_bytes(cfg, dtype)
    flip = getattr(cfg, "feature_cache_flip", False)
    mirrored = (flip and bool(getattr(cfg, "flip_prob", 0.0)), flip and bool(getattr(cfg, "test_flip", False)))
    return tuple(FeatureLoader(loader, FeatureCache(device, rb, bb, capacity, dtype=dtype), dataset,
                               FeatureCache(device, rb, bb, capacity, dtype=dtype, orientation="mirrored") if wanted else None)
                 for loader, dataset, wanted in zip((training_loader, validation_loader), (training_set, validation_set), mirrored))


def flip_cache_refusal(cfg) -> Optional[str]:
    """why cfg.feature_cache_flip or cfg.test_flip cannot be honoured, or None (train_net_dynamic.train_net raises ValueError with it)"""
    for name in ("feature_cache_flip", "test_flip"):
        v = getattr(cfg, name, False)
        if not isinstance(v, bool):
            return f"{name} = {v!r}: the setting is True or False"
    gb = float(getattr(cfg, "feature_cache_gb", 0) or 0)
    if getattr(cfg, "feature_cache_flip", False) and gb <= 0:
        return (f"feature_cache_flip = True: the mirror cache accompanies the box-feature cache, and feature_cache_gb is "
                f"{getattr(cfg, 'feature_cache_gb', 0)}: there is no cache to mirror")
    if not getattr(cfg, "test_flip", False):
        return None
    if gb > 0 and not cfg.feature_cache_flip:
        return (f"test_flip = True: feature_cache_gb = {cfg.feature_cache_gb} caches the box features of the unmirrored frame; the mirrored "
                f"clips of an evaluation pass come from the mirror cache, which feature_cache_flip = True adds")
    if cfg.dataset_name == "volleyball":
        from .volleyball import ACTIVITIES
        if cfg.num_activities != len(ACTIVITIES):
            return (f"test_flip = True: a mirrored volleyball clip's scores are read through the team-side swap of the {len(ACTIVITIES)} "
                    f"activities of volleyball.ACTIVITIES; num_activities is {cfg.num_activities}")
    return None


def refusal(cfg) -> Optional[str]:
    """why cfg.feature_cache_gb > 0 cannot be honoured, or None (train_net_dynamic.train_net raises ValueError with it)"""
    if float(getattr(cfg, "feature_cache_gb", 0) or 0) <= 0:
        return None
    pre = f"feature_cache_gb = {cfg.feature_cache_gb}: "
    if cfg.train_backbone:
        return pre + "cached box features are the output of a FROZEN backbone; train_backbone is set"
    if float(getattr(cfg, "frame_cache_gb", 0) or 0) > 0:
        return pre + (f"frame_cache_gb = {cfg.frame_cache_gb} is set as well; the pixels of a frame whose features are resident are never "
                      f"needed: choose one of the two caches")
    if cfg.inference_module_name == "dynamic_tce_volleyball":
        return pre + "dynamic_tce_volleyball reads the backbone's context map of every frame, which the feature cache does not keep"
    if cfg.dataset_name == "collective":
        return pre + "the collective dataset is not covered (volleyball only)"
    if cfg.backbone == "inv3" and not cfg.set_bn_eval:
        return pre + ("backbone 'inv3' without set_bn_eval normalises with batch statistics, so a frame's features depend on the batch it "
                      "is in and cannot be cached")
    dtype = getattr(cfg, "feature_cache_dtype", "fp32")
    if dtype == "fp32":
        return None
    pre = f"feature_cache_dtype = {dtype!r}: "
    if dtype not in DTYPES:
        return pre + f"cached box features are stored as one of {sorted(DTYPES)}"
    if cfg.backbone_dtype != "bf16":
        return pre + (f"bf16 rows are the operand of the embedding GEMM under backbone_dtype = 'bf16' only; with backbone_dtype = "
                      f"{cfg.backbone_dtype!r} rounding the features would change the embeddings")
    K = cfg.crop_size[0]
    if cfg.emb_features * K * K % 8 or cfg.num_features_boxes % 8:
        return pre + (f"the embedding GEMM multiplies bf16 operands only when emb_features * K * K = {cfg.emb_features * K * K} and "
                      f"num_features_boxes = {cfg.num_features_boxes} are multiples of 8")
    return None


# ---- the map cache (cfg.map_cache_gb; MapCache above) --------------------------------------------------------------------------------------
def map_shape_and_itemsize(cfg) -> Tuple[Tuple[int, int, int], int]:
    """([OH, OW, C], bytes per element) of the one map a frozen VGG16 ends in: cfg.out_size, all cfg.emb_features channels, bf16 under
    backbone_dtype = 'bf16' and fp32 otherwise ('fp32_bf16x3' stores fp32).  22 x 40 x 512 x 4 = 1 802 240 bytes at the volleyball
    launchers' sizes, 15 x 22 x 512 x 4 = 675 840 for collective; MapCache refuses a backbone that returns anything else."""
    return (int(cfg.out_size[0]), int(cfg.out_size[1]), int(cfg.emb_features)), (2 if getattr(cfg, "backbone_dtype", "fp32") == "bf16" else 4)


def map_loaders(cfg, training_loader, validation_loader, training_set, validation_set, device):
    """frame_cache.build_loaders with cfg.map_cache_gb > 0: one MapCache of that many GB per dataset behind a FeatureLoader -- the
    feed, the refs and the `resident` marking are the box-feature cache's"""
    capacity = int(float(cfg.map_cache_gb) * 1e9)
    shape, itemsize = map_shape_and_itemsize(cfg)
    return tuple(FeatureLoader(loader, MapCache(device, shape, itemsize, capacity), dataset)
                 for loader, dataset in ((training_loader, training_set), (validation_loader, validation_set)))


def map_refusal(cfg) -> Optional[str]:
    """why cfg.map_cache_gb cannot be honoured, or None (train_net_dynamic.train_net raises ValueError with it, after every other
    refusal)"""
    gb = getattr(cfg, "map_cache_gb", 0)
    if isinstance(gb, (bool, np.bool_)) or not isinstance(gb, (int, float, np.integer, np.floating)) or not 0.0 <= float(gb) < float("inf"):
        return f"map_cache_gb = {gb!r}: the size of the map cache in GB is a real number >= 0 (0 = off)"
    if gb == 0:
        return None
    pre = f"map_cache_gb = {gb}: "
    if cfg.train_backbone:
        return pre + "cached maps are the output of a FROZEN backbone; train_backbone is set"
    for other in ("frame_cache_gb", "feature_cache_gb"):
        if float(getattr(cfg, other, 0) or 0) > 0:
            return pre + f"{other} = {getattr(cfg, other)} is set as well; a step is fed from one cache: choose one of the three"
    if cfg.backbone == "inv3":
        return pre + ("backbone 'inv3' does not end in one map that holds all emb_features channels: its two maps (288 channels at 87 x "
                      "157 and 768 at 43 x 78) are 13 MB a frame even as bf16, 630 GB for the 48300 volleyball frames; the box-feature "
                      "cache (feature_cache_gb) keeps 1.3 MB a frame for it")
    if getattr(cfg, "flip_prob", 0.0):
        return pre + f"flip_prob = {cfg.flip_prob}: a cached map belongs to the frame as decoded; it cannot serve a mirrored one"
    if getattr(cfg, "color_jitter", None) is not None:
        return pre + f"color_jitter = {tuple(cfg.color_jitter)!r}: a cached map belongs to the frame as decoded; it cannot serve a jittered one"
    if getattr(cfg, "test_flip", False):
        return pre + "test_flip = True: a cached map belongs to the frame as decoded; there is no mirror map cache"
    return None
