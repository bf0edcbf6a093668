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

Same store as the frame cache (frame_cache.SlotStore): lazy slabs, no eviction, a full cache stops inserting and the remaining frames
keep being decoded and computed.  Refusals and the cache's lifetime: train_net_dynamic.train_net.

cfg.feature_cache_dtype = 'bf16' (with backbone_dtype = 'bf16' only): the slots hold the row already rounded to bf16, which is what
fc_emb_1's GEMM multiplies in that mode.  Half the bytes per frame, ONE din_feat_rows_bf16 launch that rounds the computed rows on their
way to feats and to the slots, and feats arrives as the GEMM's bf16 operand: no cast pass, the same numbers.

cfg.feature_cache_path (a directory; None = off): the rows outlive the call.  `FeatureCache.save` / `load` move the slots between the
slabs and one data file per cache (feature_cache_file.py: the layout, and the fingerprint that says which runs compute the same rows --
the head, the learning rate and the seed are not part of it); `CacheFile` is a loader's file, loaded before the first pass and written
after every pass in which the cache took frames in.  No kernel of its own: copy_ between pinned buffers and slabs on the current stream.
"""
from __future__ import annotations

import collections
import os
import time
from typing import Iterable, Iterator, List, Optional, Tuple

import numpy as np
import torch

from .frame_cache import CachedLoader, SlotStore
from .input_feed import DeviceFeed


class FeatureCache(SlotStore):
    """Device-resident store of box-feature rows, fp32 or (dtype=torch.bfloat16) rounded to bf16: each slot holds `row_bytes` of
    features in that dtype followed by the `box_bytes` of the boxes they were computed for.  Filled on first use, never beyond
    `capacity_bytes`, no eviction."""

    WHAT, UNIT = "feature cache", "frames"
    FLAG_ROWS = 1 << 20                              # rows between two check() calls the flags buffer holds without an extra check

    def __init__(self, device, row_bytes: int, box_bytes: int, capacity_bytes: int, chunk_frames: int = 64,
                 dtype: torch.dtype = torch.float32):
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

    def rows(self, frame_ids, boxes: torch.Tensor, miss_pos=(), miss_rows: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, List[int]]:
        """frame_ids [R] (host), boxes fp32 [R, box_bytes / 4] on the device (this step's boxes of every row), miss_pos [M] (host: which
        of the R rows the computed rows are), miss_rows fp32 [M, row_elems] on the device -> (`dtype` [R, row_elems] on the device,
        the frame ids inserted by this call).  One launch on the current stream: a row comes from its slot (and its boxes are compared
        with the slot's) or from the computed row, which also goes into a free slot with its boxes while the cache has room.  A frame
        that occurs twice is served both times from the computed row, never from the slot written by this launch.  With bf16 storage
        the computed rows still arrive as fp32 and the launch rounds them (din_feat_rows_bf16)."""
        from . import ops
        ids = np.asarray(frame_ids, dtype=np.int64).reshape(-1)
        pos = np.asarray(miss_pos, dtype=np.int64).reshape(-1)
        rb, bb, ne = self.row_bytes, self.box_bytes, self.row_elems
        if not boxes.is_cuda or boxes.dtype != torch.float32 or boxes.numel() * 4 != len(ids) * bb:
            raise ValueError(f"rows: {len(ids)} rows need fp32 device boxes of {bb} bytes each, got {tuple(boxes.shape)} {boxes.dtype}")
        boxes = boxes.contiguous()
        if boxes.data_ptr() % 16:
            boxes = boxes.clone()
        if len(pos):
            if miss_rows is None or not miss_rows.is_cuda or miss_rows.dtype != torch.float32 or not miss_rows.is_contiguous() \
                    or tuple(miss_rows.shape) != (len(pos), ne) or miss_rows.data_ptr() % 16:
                raise ValueError(f"rows: {len(pos)} computed rows need a contiguous, 16-byte aligned fp32 device tensor "
                                 f"{(len(pos), ne)}, got {None if miss_rows is None else tuple(miss_rows.shape)}")
            if pos.min() < 0 or pos.max() >= len(ids):
                raise ValueError("rows: miss_pos outside the batch")
        row_of = {}                                  # frame id -> address of its computed row (the first one serves all)
        for j, p in enumerate(pos):
            row_of.setdefault(int(ids[p]), miss_rows.data_ptr() + j * ne * 4)
        out = torch.empty((len(ids), ne), dtype=self.dtype, device=self.device)
        out_ptr = out.data_ptr()
        src, keep, ref, new_ids, fresh = [], [], [], [], set()
        for fid in ids:
            fid = int(fid)
            slot = -1 if fid in fresh else self.table.lookup(fid)
            if slot >= 0:                            # resident before this launch: served from the slot, boxes compared
                src.append(self.slot_address(slot))
                keep.append(0)
                ref.append(src[-1] + rb)
                continue
            if fid not in row_of:
                raise KeyError(f"frame {fid} is neither resident nor among the computed rows of this batch")
            slot = -1 if fid in fresh else self.table.insert(fid, self._grow)
            if slot >= 0:
                fresh.add(fid)
                new_ids.append(fid)
            src.append(row_of[fid])
            keep.append(self.slot_address(slot) if slot >= 0 else 0)
            ref.append(0)
        dst = [out_ptr + i * rb for i in range(len(ids))]
        flags = self._flag_rows(ids)
        if self.dtype == torch.float32:
            d_src, d_dst, d_keep, d_ref = self._upload(src, dst, keep, ref)
            ops.feat_rows(d_src, d_dst, rb, d_keep, d_ref, boxes, flags, bb)
        else:                                        # a row without a stored-boxes address is a computed one: fp32, to be rounded
            d_src, d_dst, d_keep, d_ref, d_f32 = self._upload(src, dst, keep, ref, [int(r == 0) for r in ref])
            ops.feat_rows_bf16(d_src, d_dst, ne, d_keep, d_ref, boxes, flags, bb, d_f32)
        return out, new_ids

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
            raise RuntimeError(f"feature cache: {bad.size} rows were served for other boxes than the ones stored with their features "
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
        return {"fingerprint": fingerprint, "row_bytes": self.row_bytes, "box_bytes": self.box_bytes,
                "dtype": "fp32" if self.dtype == torch.float32 else "bf16"}

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


class FrameRefs:
    """what a model receives in place of the images tensor when box features are cached: the frame ids of the batch [B, T] (host), the
    frames that were decoded (uint8 [M, 3, H, W] on the device), which of the B*T rows they are (`miss_pos`, host; `miss_pos_dev` the
    same on the device when the feed uploaded it), and the cache.  `shape` and `reshape` of the two leading dimensions are all the
    models and trainers use of an images tensor besides handing it to infer_model.embed_boxes, which sets `inserted`."""

    def __init__(self, frame_ids, miss_images: torch.Tensor, miss_pos, cache: FeatureCache, miss_pos_dev: Optional[torch.Tensor] = None):
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

    @property
    def shape(self) -> Tuple[int, ...]:
        return tuple(self.frame_ids.shape) + tuple(self.miss_images.shape[1:])

    def reshape(self, *shape) -> "FrameRefs":
        shape = tuple(shape[0]) if len(shape) == 1 and isinstance(shape[0], (tuple, list)) else tuple(shape)
        if len(shape) != 5 or tuple(shape[2:]) != self.shape[2:] or shape[0] * shape[1] != self.frame_ids.size:
            raise ValueError(f"FrameRefs.reshape: only the two leading dimensions of {self.shape} can be reshaped, got {shape}")
        out = FrameRefs(self.frame_ids.reshape(shape[0], shape[1]), self.miss_images, self.miss_pos, self.cache, self.miss_pos_dev)
        out.inserted = self.inserted                 # (shared: the feed reads it off the object it yielded)
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
    went into the cache, so the loader stops decoding them."""

    def __init__(self, loader: Iterable, device, cache: FeatureCache, dataset):
        self.loader, self.device, self.cache, self.dataset = loader, torch.device(device), cache, dataset
        self._kept: collections.deque = collections.deque()
        self._feed = DeviceFeed(_HostSide(loader, self._kept), self.device)

    def __iter__(self) -> Iterator:
        self._kept.clear()
        for miss_images, miss_pos_dev, *labels in self._feed:
            ids, pos = self._kept.popleft()
            refs = FrameRefs(ids, miss_images, pos, self.cache, miss_pos_dev)
            yield (refs, *labels)
            if refs.inserted:                        # (filled by embed_boxes during the model call)
                self.dataset.resident[torch.as_tensor(refs.inserted, dtype=torch.int64)] = 1

    def check(self) -> None:
        self.cache.check()

    def __len__(self):
        return len(self.loader)


class FeatureLoader(CachedLoader):
    """a DataLoader of a `frame_ids=True` dataset together with the feature cache of that dataset: what the stage-2 trainer's passes
    receive in place of the loader when cfg.feature_cache_gb > 0"""

    def feed(self, device, augment=None) -> FeatureFeed:
        if augment is not None and augment.flip is not None:       # (train_net refuses the combination first: frame_cache.flip_refusal)
            raise ValueError("flip augmentation cannot be fed from the feature cache: its rows belong to the unmirrored frames")
        if augment is not None and augment.jitter is not None:     # (likewise: frame_cache.jitter_refusal)
            raise ValueError("colour jitter cannot be fed from the feature cache: its rows belong to the frames as decoded")
        return FeatureFeed(self.loader, device, self.cache, self.dataset)


class CacheFile:
    """the file one FeatureLoader's cache is kept in between runs (cfg.feature_cache_path): `load` before the first pass, `save_if_grown`
    after every pass.  `loaded` / `saved` count frames; `say` takes the one log line of every load and save."""

    def __init__(self, loader: FeatureLoader, path: str, meta: dict, say=print):
        self.loader, self.path, self.meta, self.say = loader, path, meta, say
        self.loaded = self.saved = 0

    @property
    def inserted(self) -> int:
        return self.loader.cache.table.inserted

    def _line(self, verb: str, frames: int, seconds: float) -> None:
        gb = frames * self.loader.cache.table.stride / 1e9
        self.say(f"feature cache {verb} {self.path}: {frames} frames, {gb:.3f} GB, {seconds:.2f} s")

    def load(self) -> int:
        """take the file in if there is one, and mark its frames resident so that the loader's workers stop decoding them -- what the
        in-memory cache does from its second epoch.  A file of another fingerprint is a ValueError (FeatureCache.load)."""
        if not os.path.exists(self.path):
            return 0
        t0 = time.perf_counter()
        ids = self.loader.cache.load(self.path, self.meta)
        flags = self.loader.dataset.resident
        if ids and (min(ids) < 0 or max(ids) >= flags.numel()):
            raise ValueError(f"feature cache file {self.path} names frames outside the dataset's table of {flags.numel()} frames")
        if ids:
            flags[torch.as_tensor(ids, dtype=torch.int64)] = 1
        self.loaded = len(ids)
        self._line("loaded from", self.loaded, time.perf_counter() - t0)
        return self.loaded

    def save_if_grown(self, inserted_before: int) -> int:
        """after a pass: write the whole cache if it took frames in during the pass (`inserted_before`: `inserted` read before it);
        returns the frames written, 0 for a pass that only read"""
        if self.inserted == inserted_before:
            return 0
        t0 = time.perf_counter()
        os.makedirs(os.path.dirname(self.path) or ".", exist_ok=True)
        self.saved = self.loader.cache.save(self.path, self.meta)
        self._line("saved to", self.saved, time.perf_counter() - t0)
        return self.saved


def cache_files(cfg, model, training_loader, validation_loader, rank: int = 0, world: int = 1, say=print) -> dict:
    """{"train": CacheFile, "val": CacheFile} for cfg.feature_cache_path, {} without the setting or without feature caches behind the
    loaders (no real dataset tree).  The fingerprints are taken here: call it when the backbone has its stage-1 weights."""
    from . import feature_cache_file as FF
    folder = getattr(cfg, "feature_cache_path", None)
    if folder is None or not (isinstance(training_loader, FeatureLoader) and isinstance(validation_loader, FeatureLoader)):
        return {}
    return {split: CacheFile(ld, os.path.join(str(folder), FF.file_name(split, rank, world)), FF.fingerprint(cfg, model, ld.dataset), say)
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
    """frame_cache.build_loaders with cfg.feature_cache_gb > 0: one FeatureCache of that many GB per dataset"""
    capacity = int(float(cfg.feature_cache_gb) * 1e9)
    dtype = DTYPES[getattr(cfg, "feature_cache_dtype", "fp32")]
    rb, bb = row_and_box_bytes(cfg, dtype)
    return (FeatureLoader(training_loader, FeatureCache(device, rb, bb, capacity, dtype=dtype), training_set),
            FeatureLoader(validation_loader, FeatureCache(device, rb, bb, capacity, dtype=dtype), validation_set))


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
