"""Frame cache: decoded uint8 frames stay in HBM, and a batch of clips is one gather launch out of them.

The reference decodes, resizes and stacks every frame of every epoch on the host (volleyball.py:223-275) and uploads the batch with a
blocking copy (train_net_dynamic.py:174).  One core decodes about 13 ten-frame 720p clips a second, the trained step runs some 650: on
real data the loader, not the GPU, sets the pace.  The whole Volleyball set is 133.5 GB as uint8 at 720x1280 and an MI355X has 288 GB,
so after the first epoch nothing needs decoding or crossing PCIe again:

  * datasets built with `frame_ids=True` name frames by their index in a fixed table and decode only those whose `resident` flag is
    clear (the flags live in shared memory, so forked loader workers see what the main process marks);
  * `collate` concatenates the decoded frames of a batch and records where they belong;
  * `CachedFeed` uploads only those (through input_feed.DeviceFeed: same copy stream, double buffer, pinned staging) and then, on the
    compute stream, (1) copies the new frames into free slots, (2) marks them resident, (3) builds the uint8 [B, T, 3, H, W] batch the
    models take with one din_copy_rows_u8 launch over all B*T rows -- from a slot, or from the uploaded row where the cache is full.
    Everything is in stream order on one stream: a gather always sees the inserts enqueued before it.

No eviction: an epoch touches every frame once in random order, so least-recently-used would throw away exactly what is needed next; a
full cache stops inserting and the remaining frames keep coming from the loader.  Each rank owns its caches; DistributedSampler
reshuffles clips across ranks every epoch, so a rank's hit rate grows over several epochs instead of reaching 100 % in the second
(rank-stable sharding would change the sampling and is not done here).

Flip augmentation (cfg.flip_prob, training passes only) lives here too, because a clip is mirrored where its batch is built: the gather
becomes din_copy_rows_u8_flip for a batch with a drawn clip (FlipPlan, CachedFeed; FlippedFeed for loaders without a cache).

Colour jitter (cfg.color_jitter, training passes only) is a per-pixel function applied on the same way from slot to batch: Pillow's
ImageEnhance.Contrast, .Brightness and .Color with three factors drawn per clip (JitterPlan), byte for byte.  For a batch with a drawn
clip the gather becomes din_rows_gray_partials (the grey sums the contrast stage pivots on) plus din_copy_rows_u8_jitter, which mirrors
flagged rows as well; the slots keep the frame as decoded.
"""
from __future__ import annotations

import collections
import logging
from typing import Callable, Dict, Iterable, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.utils.data as data

from .input_feed import DeviceFeed

log = logging.getLogger(__name__)

LOADER_TIMEOUT_S = 300          # DataLoader(timeout=...): a stuck worker raises instead of hanging the trainer


class SlotTable:
    """Host bookkeeping of the cache (no device needed): frame id -> slot, slab growth, capacity, counters.

    Slots are `stride` bytes apart (frame_bytes rounded up to 16) and allocated in slabs of `chunk_frames` slots, the last slab shorter
    when the capacity is not a whole number of slabs.  `grow(n_slots) -> bool` is asked for one more slab when the allocated slots run out;
    a False answer freezes the table at its current size."""

    def __init__(self, frame_bytes: int, capacity_bytes: int, chunk_frames: int = 64):
        if frame_bytes <= 0 or chunk_frames <= 0 or capacity_bytes < 0:
            raise ValueError(f"SlotTable: frame_bytes {frame_bytes}, chunk_frames {chunk_frames}, capacity_bytes {capacity_bytes}")
        self.frame_bytes, self.chunk_frames = int(frame_bytes), int(chunk_frames)
        self.stride = (self.frame_bytes + 15) // 16 * 16
        self.max_slots = int(capacity_bytes) // self.stride
        self.slot_of: Dict[int, int] = {}
        self.slab_slots: List[int] = []             # slots of every allocated slab
        self.allocated = 0                          # slots in allocated slabs
        self.frozen = False
        self.hits = self.misses = self.inserted = 0

    @property
    def bytes(self) -> int:
        """device bytes the allocated slabs take"""
        return self.allocated * self.stride

    @property
    def full(self) -> bool:
        return len(self.slot_of) >= self.max_slots

    def lookup(self, fid: int) -> int:
        """slot of a frame, or -1; counts a hit or a miss"""
        slot = self.slot_of.get(int(fid), -1)
        if slot < 0:
            self.misses += 1
        else:
            self.hits += 1
        return slot

    def insert(self, fid: int, grow: Callable[[int], bool] = lambda n: True) -> int:
        """slot for a new frame, or -1 when the cache is full or frozen; an id that is already there is a hit and keeps its slot"""
        fid = int(fid)
        slot = self.slot_of.get(fid, -1)
        if slot >= 0:
            self.hits += 1
            return slot
        if not self.reserve(grow):
            return -1
        slot = len(self.slot_of)
        self.slot_of[fid] = slot
        self.inserted += 1
        return slot

    def reserve(self, grow: Callable[[int], bool] = lambda n: True) -> bool:
        """whether the next `insert` of a new frame will succeed: allocates the slab it would need now (a refused slab freezes the
        table, as in `insert`), so that several tables can be asked before any of them takes the frame in"""
        if self.full:
            return False
        if len(self.slot_of) == self.allocated:
            n = min(self.chunk_frames, self.max_slots - self.allocated)
            if not grow(n):
                self.max_slots, self.frozen = self.allocated, True
                return False
            self.slab_slots.append(n)
            self.allocated += n
        return True

    def locate(self, slot: int) -> Tuple[int, int]:
        """(slab index, byte offset inside the slab): every slab but the last holds chunk_frames slots"""
        return slot // self.chunk_frames, (slot % self.chunk_frames) * self.stride

    def counters(self) -> dict:
        return {"hits": self.hits, "misses": self.misses, "inserted": self.inserted, "bytes": self.bytes}


def _f32_as_table(values: np.ndarray) -> np.ndarray:
    """float32 values as int64 words (an odd count is padded with one zero), so that they travel in TableUpload's buffer"""
    flat = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
    if flat.size % 2:
        flat = np.concatenate([flat, np.zeros(1, dtype=np.float32)])
    return flat.view(np.int64)


class GrayPartials:
    """the uint32 workspace of din_rows_gray_partials, allocated once and reused by every batch of its owner (it only grows); launches
    on one stream are ordered, so the next batch's partials cannot overtake this batch's gather"""

    def __init__(self, device):
        self.device, self.buf = torch.device(device), None

    def of(self, rows: int, height: int, width: int) -> torch.Tensor:
        from . import ops
        need = rows * ops.gray_partial_segments(height, width)
        if self.buf is None or self.buf.numel() < need:
            self.buf = torch.empty(max(need, 1), dtype=torch.int32, device=self.device)
        return self.buf


def drawn_rows(rows: int, frame_shape, flip_rows, jitter_rows) -> Tuple[Optional[np.ndarray], Optional[np.ndarray]]:
    """what a batch of `rows` frames drew, as the gather takes it: (bool [rows] or None, float32 [rows, 3] or None).  No flag set is
    the same as no flags, all factors 1 the same as no factors; ValueError for what cannot be launched."""
    flags = None if flip_rows is None else np.asarray(flip_rows).reshape(-1) != 0
    if flags is not None and len(flags) != rows:
        raise ValueError(f"frame gather: {len(flags)} flip flags for {rows} rows")
    factors = None if jitter_rows is None else np.asarray(jitter_rows, dtype=np.float32)
    if factors is not None and factors.shape != (rows, 3):
        raise ValueError(f"frame gather: jitter factors {factors.shape} for {rows} rows (one triple per row)")
    if factors is not None and not np.isfinite(factors).all():
        raise ValueError("frame gather: a jitter factor is not finite")
    if factors is not None and (factors == 1).all():
        factors = None
    if factors is not None and (len(frame_shape) != 3 or frame_shape[0] != 3):
        raise ValueError(f"frame gather: colour jitter works on [3, H, W] frames, these are {tuple(frame_shape)}")
    return (flags if flags is not None and flags.any() else None), factors


class TableUpload:
    """the rotating pinned buffers the int64 tables of a launch (addresses, flip flags, colour factors) travel in, and the one place
    that chooses the gather launch of a batch (`gather_rows`)"""

    TABLE_SLOTS = 4                                  # pinned address-table buffers in rotation (one batch uses one)

    def __init__(self, device):
        self.device = torch.device(device)
        self._pinned: List[Optional[torch.Tensor]] = [None] * self.TABLE_SLOTS
        self._sent: List[Optional[torch.cuda.Event]] = [None] * self.TABLE_SLOTS
        self._turn = 0
        self._gray = GrayPartials(device)            # colour jitter's workspace (nothing is allocated until a batch is jittered)

    def _upload(self, *tables: Sequence[int]) -> List[torch.Tensor]:
        """int64 address tables -> device, in ONE asynchronous copy on the current stream out of a pinned buffer that is reused only after
        the copy it last fed has finished"""
        total = sum(len(t) for t in tables)
        k = self._turn = (self._turn + 1) % self.TABLE_SLOTS
        if self._sent[k] is not None:
            self._sent[k].synchronize()
        buf = self._pinned[k]
        if buf is None or buf.numel() < total:
            buf = self._pinned[k] = torch.empty(max(total, 1024), dtype=torch.int64).pin_memory()
        host = buf.numpy()
        at, views = 0, []
        for t in tables:
            host[at:at + len(t)] = t
            views.append((at, len(t)))
            at += len(t)
        dev = buf[:total].to(self.device, non_blocking=True)
        self._sent[k] = torch.cuda.Event()
        self._sent[k].record(torch.cuda.current_stream(self.device))
        return [dev[a:a + n] for a, n in views]

    def gather_rows(self, src: Sequence[int], dst: Sequence[int], frame_shape, flip_rows=None, jitter_rows=None,
                    insert: Optional[Tuple[Sequence[int], Sequence[int]]] = None) -> Optional[torch.Tensor]:
        """the gather of a batch on the current stream: row i goes from address src[i] to dst[i], mirrored where flip_rows[i] is set and
        jittered with jitter_rows[i] = (contrast, brightness, saturation) (`drawn_rows`).  All tables cross in ONE upload; the address
        lists `insert` = (src, dst) ride in it and are copied first, by the plain din_copy_rows_u8.  Then din_copy_rows_u8, or
        din_copy_rows_u8_flip where a row is mirrored, or din_rows_gray_partials + din_copy_rows_u8_jitter (mirroring included) where
        one is jittered.  Returns the device flags (int64 [R], for the labels' launch), None when nothing is mirrored."""
        from . import ops
        flags, factors = drawn_rows(len(src), frame_shape, flip_rows, jitter_rows)
        fb, width = int(np.prod(frame_shape)), int(frame_shape[-1])
        tables = [src, dst] + ([] if flags is None else [flags.astype(np.int64)]) + ([] if factors is None else [_f32_as_table(factors)])
        if insert is not None:
            d_ins_src, d_ins_dst, *d = self._upload(*insert, *tables)
            ops.copy_rows_u8(d_ins_src, d_ins_dst, fb)                  # (plain: a slot holds the frame as decoded, never mirrored)
        else:
            d = self._upload(*tables)
        d_src, d_dst, d_flags = d[0], d[1], (None if flags is None else d[2])
        if factors is not None:
            height = int(frame_shape[-2])
            work = self._gray.of(len(src), height, width)
            ops.rows_gray_partials(d_src, work, height, width)
            ops.copy_rows_u8_jitter(d_src, d_dst, d_flags, d[-1].view(torch.float32)[:3 * len(src)], work, height, width)
        elif flags is not None:
            ops.copy_rows_u8_flip(d_src, d_dst, d_flags, fb // width, width)
        else:
            ops.copy_rows_u8(d_src, d_dst, fb)
        return d_flags


class SlotStore(TableUpload):
    """Device side of a SlotTable: the lazily allocated slabs, slot addresses and the rotating pinned buffers the address tables of a
    launch travel in.  FrameCache (uint8 frames) and feature_cache.FeatureCache (fp32 box features) are the two stores."""

    WHAT, UNIT = "frame cache", "frames"             # the words of the freeze log line

    def __init__(self, device, slot_bytes: int, capacity_bytes: int, chunk_frames: int = 64):
        super().__init__(device)
        self.table = SlotTable(slot_bytes, capacity_bytes, chunk_frames)
        self.slabs: List[torch.Tensor] = []

    hits = property(lambda self: self.table.hits)
    misses = property(lambda self: self.table.misses)
    inserted = property(lambda self: self.table.inserted)
    bytes = property(lambda self: self.table.bytes)

    def _grow(self, n_slots: int) -> bool:
        try:
            self.slabs.append(torch.empty(n_slots * self.table.stride, dtype=torch.uint8, device=self.device))
            return True
        except RuntimeError as e:                    # (torch.cuda.OutOfMemoryError is one)
            log.warning("%s frozen at %d %s (%.2f GB): a slab of %d %s could not be allocated: %s", self.WHAT,
                        self.table.allocated, self.UNIT, self.table.bytes / 1e9, n_slots, self.UNIT, str(e).splitlines()[0])
            return False

    def slot_address(self, slot: int) -> int:
        slab, off = self.table.locate(slot)
        return self.slabs[slab].data_ptr() + off

    def resident(self, fid: int) -> bool:
        return int(fid) in self.table.slot_of


class FrameCache(SlotStore):
    """Device-resident uint8 frame store with fixed-size slots, filled on first use, never beyond `capacity_bytes`, no eviction."""

    def __init__(self, device, frame_shape: Sequence[int], capacity_bytes: int, chunk_frames: int = 64):
        self.frame_shape = tuple(int(v) for v in frame_shape)
        self.frame_bytes = int(np.prod(self.frame_shape))
        super().__init__(device, self.frame_bytes, capacity_bytes, chunk_frames)
        self.flip_flags: Optional[torch.Tensor] = None      # the device flags (int64 [R]) of the last build_batch, None when it mirrored nothing

    def build_batch(self, frame_ids, miss_pos=(), miss_rows: Optional[torch.Tensor] = None,
                    flip_rows=None, jitter_rows=None) -> Tuple[torch.Tensor, List[int]]:
        """frame_ids [R] (host), miss_pos [M] (host: which of the R rows the uploaded frames are), miss_rows uint8 [M, *frame_shape] on
        the device -> (uint8 [R, *frame_shape] on the device, the frame ids inserted by this call).  On the current stream: one launch
        that copies the new frames into free slots, then the gather of all R rows (slot, or uploaded row where the cache has no room)
        as `gather_rows` chooses it from flip_rows (host, bool [R]) and jitter_rows (host, float32 [R, 3]): plain, mirrored or jittered
        on the way out -- the slots always hold the frame as decoded.  The device flags of a mirrored batch stay in `self.flip_flags`
        for the labels' launch."""
        ids = np.asarray(frame_ids, dtype=np.int64).reshape(-1)
        pos = np.asarray(miss_pos, dtype=np.int64).reshape(-1)
        drawn = drawn_rows(len(ids), self.frame_shape, flip_rows, jitter_rows)    # (refused here, before the table takes a frame in)
        if len(pos):
            if miss_rows is None or not miss_rows.is_cuda or miss_rows.dtype != torch.uint8 or not miss_rows.is_contiguous() \
                    or tuple(miss_rows.shape) != (len(pos),) + self.frame_shape:
                raise ValueError(f"build_batch: {len(pos)} missed frames need a contiguous uint8 device tensor "
                                 f"{(len(pos),) + self.frame_shape}, got {None if miss_rows is None else tuple(miss_rows.shape)}")
            if pos.min() < 0 or pos.max() >= len(ids):
                raise ValueError("build_batch: miss_pos outside the batch")
        fb = self.frame_bytes
        row_of = {}                                  # frame id -> address of its uploaded pixels (the first copy serves all)
        for j, p in enumerate(pos):
            row_of.setdefault(int(ids[p]), miss_rows.data_ptr() + j * fb)
        out = torch.empty((len(ids),) + self.frame_shape, dtype=torch.uint8, device=self.device)
        out_ptr = out.data_ptr()
        ins_src, ins_dst, new_ids, src = [], [], [], []
        for fid in ids:
            fid = int(fid)
            slot = self.table.lookup(fid)
            if slot < 0 and fid in row_of:
                slot = self.table.insert(fid, self._grow)
                if slot >= 0:
                    ins_src.append(row_of[fid])
                    ins_dst.append(self.slot_address(slot))
                    new_ids.append(fid)
            if slot >= 0:
                src.append(self.slot_address(slot))
            elif fid in row_of:
                src.append(row_of[fid])
            else:
                raise KeyError(f"frame {fid} is neither resident nor among the uploaded frames of this batch")
        dst = [out_ptr + i * fb for i in range(len(ids))]
        self.flip_flags = self.gather_rows(src, dst, self.frame_shape, *drawn, insert=(ins_src, ins_dst))
        return out, new_ids

    def insert(self, frame_ids, rows: torch.Tensor) -> List[int]:
        """store rows[i] as frame frame_ids[i]; returns the ids that are resident afterwards (all of them unless the cache is full)"""
        ids = np.asarray(frame_ids, dtype=np.int64).reshape(-1)
        fb, ins_src, ins_dst = self.frame_bytes, [], []
        if tuple(rows.shape) != (len(ids),) + self.frame_shape or rows.dtype != torch.uint8 or not rows.is_cuda or not rows.is_contiguous():
            raise ValueError(f"insert: {len(ids)} frames need a contiguous uint8 device tensor {(len(ids),) + self.frame_shape}")
        from . import ops
        for j, fid in enumerate(ids):
            known = int(fid) in self.table.slot_of
            slot = self.table.insert(int(fid), self._grow)
            if slot >= 0 and not known:
                ins_src.append(rows.data_ptr() + j * fb)
                ins_dst.append(self.slot_address(slot))
        d_src, d_dst = self._upload(ins_src, ins_dst)
        ops.copy_rows_u8(d_src, d_dst, fb)
        rows.record_stream(torch.cuda.current_stream(self.device))
        return [int(f) for f in ids if int(f) in self.table.slot_of]

    def gather(self, frame_ids) -> torch.Tensor:
        """uint8 [R, *frame_shape] of resident frames (KeyError for one that is not)"""
        return self.build_batch(frame_ids)[0]


def collate(items):
    """DataLoader collate_fn for `frame_ids=True` datasets.  items: (frame_ids [T], miss_images [M_i, 3, H, W], *labels, miss_index [M_i])
    -> (frame_ids [B, T], miss_images [sum M_i, 3, H, W], miss_pos int64 [sum M_i], *labels stacked as the default collate does):
    miss_pos[j] = b * T + t is the row of the batch that uploaded frame j belongs to."""
    T = items[0][0].shape[0]
    frame_ids = torch.stack([it[0] for it in items])
    miss_images = torch.cat([it[1] for it in items])
    miss_pos = torch.cat([it[-1] + b * T for b, it in enumerate(items)])
    labels = data.default_collate([tuple(it[2:-1]) for it in items])
    return (frame_ids, miss_images, miss_pos, *labels)


class _HostSide:
    """what CachedFeed hands to DeviceFeed: the tensors to upload, with the host-only part (ids, positions) kept back in order"""

    def __init__(self, loader, kept: collections.deque):
        self.loader, self.kept = loader, kept

    def __iter__(self):
        for frame_ids, miss_images, miss_pos, *labels in self.loader:
            self.kept.append((tuple(frame_ids.shape), frame_ids.numpy().reshape(-1), miss_pos.numpy()))
            yield (miss_images, *labels)

    def __len__(self):
        return len(self.loader)


class CachedFeed:
    """DeviceFeed's iteration contract over a loader of `collate`d batches: yields (images uint8 [B, T, 3, H, W], *labels) on the
    device.  Only the frames the workers decoded are uploaded (DeviceFeed overlaps that with the previous step); the batch is built on
    the compute stream by `cache.build_batch`, and `dataset.resident` is marked for what went in."""

    def __init__(self, loader: Iterable, device, cache: FrameCache, dataset, augment: Optional["PassAugment"] = None):
        self.loader, self.device, self.cache, self.dataset, self.augment = loader, torch.device(device), cache, dataset, augment
        self._kept: collections.deque = collections.deque()
        self._feed = DeviceFeed(_HostSide(loader, self._kept), self.device)

    def __iter__(self) -> Iterator:
        self._kept.clear()
        for miss_rows, *labels in self._feed:
            shape, ids, pos = self._kept.popleft()
            # one draw per clip, repeated over its T rows; a batch without a drawn clip is built exactly as without augmentation
            rows, factors = (None, None) if self.augment is None else self.augment.rows(shape[0], shape[1])
            images, new_ids = self.cache.build_batch(ids, pos, miss_rows, flip_rows=rows, jitter_rows=factors)
            if new_ids:
                self.dataset.resident[torch.as_tensor(new_ids, dtype=torch.int64)] = 1
            if rows is not None:
                self.augment.mirror_labels(labels, self.cache.flip_flags)
            yield (images.view(shape + self.cache.frame_shape), *labels)

    def __len__(self):
        return len(self.loader)


class CachedLoader:
    """a DataLoader of a `frame_ids=True` dataset together with the cache its batches are built from: what the trainers' passes receive
    in place of the loader when cfg.frame_cache_gb > 0 (`feed_for` turns either into the right feed)"""

    def __init__(self, loader, cache: FrameCache, dataset):
        self.loader, self.cache, self.dataset = loader, cache, dataset

    def feed(self, device, augment: Optional["PassAugment"] = None) -> CachedFeed:
        return CachedFeed(self.loader, device, self.cache, self.dataset, augment)

    def __iter__(self):
        return iter(self.loader)

    def __len__(self):
        return len(self.loader)


# ---- flip augmentation (cfg.flip_prob) ----------------------------------------------------------------------------------------------------
# In a training pass every clip is mirrored left-right with probability cfg.flip_prob, as a whole: all T frames inside the launch that
# builds the batch (din_copy_rows_u8_flip: the same bytes read and written as the plain gather, no host work), its boxes
# (x -> out_size[1] - x) and, for volleyball, the team side of its activity label (din_flip_clip_labels, one launch).  Actions have no
# side and the collective activities neither.  Evaluation passes never flip.
class EpochFlips:
    """the flips of one training pass of one rank: `draw` is called once per batch, in batch order"""

    def __init__(self, plan: "FlipPlan", epoch: int):
        self.prob, self.label_map, self.width = plan.prob, plan.label_map, plan.width
        self._rng = np.random.default_rng([plan.seed, plan.rank, int(epoch)])
        self._device_map: Optional[torch.Tensor] = None
        self.flipped = 0                                # clips mirrored so far (a host count: the info's `flipped_clips`)

    def draw(self, num_clips: int) -> np.ndarray:
        """bool [num_clips]: which clips of the next batch are mirrored"""
        flags = self._rng.random(int(num_clips)) < self.prob
        self.flipped += int(flags.sum())
        return flags

    def rows(self, num_clips: int, num_frames: int) -> Optional[np.ndarray]:
        """the next batch's draw repeated over the T rows of every clip (bool [B * T]), or None when no clip is flagged"""
        flags = self.draw(num_clips)
        return np.repeat(flags, int(num_frames)) if flags.any() else None

    def mirror_labels(self, labels, flags: torch.Tensor) -> None:
        """labels = [boxes [B, T, N, 4], actions, activities [B, T]] (+ [bboxes_num [B, T]], collective) on the device, flags int64 [B * T]
        on the device: the flagged clips' boxes and activities, in place, one launch"""
        from . import ops
        if self.label_map is not None and self._device_map is None:
            self._device_map = torch.tensor(self.label_map, dtype=torch.int64, device=flags.device)
        ops.flip_clip_labels(labels[0], labels[2], flags, labels[3] if len(labels) > 3 else None, self._device_map, self.width)


class FlipPlan:
    """which clips a run mirrors.  The draws of epoch e come from np.random.default_rng([seed, rank, e]): a resumed run repeats the flips
    of an epoch, ranks differ from each other, and a deterministic run stays reproducible.  label_map: the activity label of a mirrored
    clip (volleyball.FLIP_ACTIVITIES; None: labels have no side); width: the feature map's, which the boxes are mirrored in."""

    def __init__(self, prob: float, seed: int, rank: int, label_map: Optional[Sequence[int]] = None, width: float = 0.0):
        self.prob, self.seed, self.rank = float(prob), int(seed) & (2 ** 63 - 1), int(rank)
        self.label_map, self.width = (None if label_map is None else list(label_map)), float(width)

    def epoch(self, e: int) -> EpochFlips:
        return EpochFlips(self, e)


def flip_refusal(cfg) -> Optional[str]:
    """why cfg.flip_prob cannot be honoured, or None (both trainers' train_net raise ValueError with it)"""
    p = getattr(cfg, "flip_prob", 0.0)
    if isinstance(p, bool) or not isinstance(p, (int, float, np.integer, np.floating)) or not 0.0 <= float(p) <= 1.0:
        return f"flip_prob = {p!r}: the probability of mirroring a clip is a real number in [0, 1]"
    if p == 0:
        return None
    pre = f"flip_prob = {p}: "
    if wants_features(cfg) and getattr(cfg, "feature_cache_flip", False) is not True:        # (with it: feature_cache.py's mirror cache)
        return pre + f"feature_cache_gb = {cfg.feature_cache_gb} caches the box features of the unmirrored frame; they cannot serve a mirrored one"
    if cfg.dataset_name == "volleyball":
        from .volleyball import ACTIVITIES
        if cfg.num_activities != len(ACTIVITIES):
            return pre + (f"a mirrored volleyball clip swaps the team side of its label among the {len(ACTIVITIES)} activities of "
                          f"volleyball.ACTIVITIES; num_activities is {cfg.num_activities}")
    return None


def flip_plan(cfg, epoch: int, rank: int) -> Optional[EpochFlips]:
    """the flips of training epoch `epoch` on rank `rank`, or None with cfg.flip_prob == 0 (nothing changes then)"""
    p = getattr(cfg, "flip_prob", 0.0)
    if not p:
        return None
    label_map = None
    if cfg.dataset_name == "volleyball":
        from .volleyball import FLIP_ACTIVITIES as label_map
    return FlipPlan(p, cfg.train_random_seed, rank, label_map, cfg.out_size[1]).epoch(epoch)


class FlippedFeed:
    """DeviceFeed's iteration contract with the augmentations of a training pass (PassAugment) over a plain loader (no frame cache):
    the batch is uploaded as it is and its drawn clips are mirrored and jittered on the device, into a new tensor, by the launches of
    `TableUpload.gather_rows`, plus the labels' launch where a clip is mirrored.  A batch without a drawn clip is handed on untouched.
    The partials workspace is allocated once and reused."""

    def __init__(self, loader: Iterable, device, augment: "PassAugment"):
        self.loader, self.device, self.augment = loader, torch.device(device), augment
        self._feed = DeviceFeed(loader, self.device)
        self._tables = TableUpload(self.device)

    def __iter__(self) -> Iterator:
        for batch in self._feed:
            images, *labels = batch
            if images.dtype != torch.uint8 or images.dim() < 3 or not images.is_contiguous():
                raise ValueError(f"flip_prob and color_jitter work on contiguous uint8 [B, T, ..., W] frames on the device; the loader "
                                 f"gave {images.dtype} {tuple(images.shape)}")
            rows, factors = self.augment.rows(images.shape[0], images.shape[1])
            if rows is None and factors is None:
                yield batch
                continue
            out = torch.empty_like(images)
            fb = images[0, 0].numel()
            src = [images.data_ptr() + i * fb for i in range(images.shape[0] * images.shape[1])]
            dst = [out.data_ptr() + i * fb for i in range(images.shape[0] * images.shape[1])]
            d_flags = self._tables.gather_rows(src, dst, images.shape[2:], rows, factors)
            if rows is not None:
                self.augment.mirror_labels(labels, d_flags)
            yield [out, *labels]

    def __len__(self):
        return len(self.loader)


# ---- colour jitter (cfg.color_jitter) -----------------------------------------------------------------------------------------------------
# In a training pass every clip draws three fp32 factors f = 1 + a * u, u uniform in [-1, 1], with the amplitudes a of
# cfg.color_jitter = (brightness, contrast, saturation); all T frames of the clip go through PIL.ImageEnhance.Contrast, .Brightness and
# .Color with them, in that order, byte for byte as Pillow computes them (include/din_hip.h states the arithmetic), inside the launch
# that builds the batch.  Boxes and labels do not change.  Evaluation passes never jitter.
KERNEL_ORDER = (1, 0, 2)        # cfg.color_jitter and JitterPlan's draws are (brightness, contrast, saturation); the launch takes
#                                 (contrast, brightness, saturation), the order the stages are applied in


class EpochJitter:
    """the factors of one training pass of one rank: `draw` is called once per batch, in batch order"""

    def __init__(self, plan: "JitterPlan", epoch: int):
        self.amplitudes = plan.amplitudes
        self._rng = np.random.default_rng([plan.seed, plan.rank, int(epoch), 1])      # (the flips' stream is [seed, rank, epoch])
        self.jittered = 0                               # clips with a factor other than 1 so far (the info's `jittered_clips`)

    def draw(self, num_clips: int) -> np.ndarray:
        """float32 [num_clips, 3]: the (brightness, contrast, saturation) factors of the clips of the next batch; an amplitude of 0
        gives exactly 1.0"""
        u = self._rng.uniform(-1.0, 1.0, (int(num_clips), 3))
        f = (1.0 + self.amplitudes[None, :] * u).astype(np.float32)
        self.jittered += int((f != 1).any(axis=1).sum())
        return f

    def rows(self, num_clips: int, num_frames: int) -> Optional[np.ndarray]:
        """the next batch's draw as the launch takes it: float32 [B * T, 3] (contrast, brightness, saturation), every clip's triple
        repeated over its T rows; None when every factor is 1"""
        f = self.draw(num_clips)
        if (f == 1).all():
            return None
        return np.ascontiguousarray(np.repeat(f[:, KERNEL_ORDER], int(num_frames), axis=0))


class JitterPlan:
    """the colour factors a run draws.  amplitudes: (brightness, contrast, saturation), each in [0, 1).  The draws of epoch e come from
    np.random.default_rng([seed, rank, e, 1]) -- a stream of its own, so turning the jitter on never changes which clips are mirrored; a
    resumed run repeats the draws of an epoch, ranks differ from each other, and a deterministic run stays reproducible."""

    def __init__(self, amplitudes: Sequence[float], seed: int, rank: int):
        self.amplitudes = np.asarray([float(a) for a in amplitudes], dtype=np.float64)
        if self.amplitudes.shape != (3,):
            raise ValueError(f"JitterPlan: three amplitudes (brightness, contrast, saturation), got {amplitudes!r}")
        self.seed, self.rank = int(seed) & (2 ** 63 - 1), int(rank)

    def epoch(self, e: int) -> EpochJitter:
        return EpochJitter(self, e)


def jitter_refusal(cfg) -> Optional[str]:
    """why cfg.color_jitter cannot be honoured, or None (both trainers' train_net raise ValueError with it)"""
    j = getattr(cfg, "color_jitter", None)
    if j is None:
        return None

    def real(a):
        return not isinstance(a, (bool, np.bool_)) and isinstance(a, (int, float, np.integer, np.floating)) and 0.0 <= float(a) < 1.0

    if isinstance(j, (str, bytes)) or not isinstance(j, (tuple, list, np.ndarray)) or len(j) != 3 or not all(real(a) for a in j):
        return (f"color_jitter = {j!r}: None, or the three amplitudes (brightness, contrast, saturation) of the colour jitter, each a real "
                f"number in [0, 1)")
    if wants_features(cfg):
        return (f"color_jitter = {tuple(j)!r}: feature_cache_gb = {cfg.feature_cache_gb} caches the box features of the frame as decoded; "
                f"they cannot serve a jittered one")
    return None


def jitter_plan(cfg, epoch: int, rank: int) -> Optional[EpochJitter]:
    """the colour factors of training epoch `epoch` on rank `rank`, or None with cfg.color_jitter = None (nothing changes then)"""
    j = getattr(cfg, "color_jitter", None)
    if j is None:
        return None
    return JitterPlan(j, cfg.train_random_seed, rank).epoch(epoch)


class PassAugment:
    """the augmentations of one training pass of one rank: its flips and its colour factors, either may be None"""

    def __init__(self, flip: Optional[EpochFlips] = None, jitter: Optional[EpochJitter] = None):
        self.flip, self.jitter = flip, jitter

    def rows(self, num_clips: int, num_frames: int) -> Tuple[Optional[np.ndarray], Optional[np.ndarray]]:
        """the next batch's draws as the gather takes them: (EpochFlips.rows or None, EpochJitter.rows or None) -- the flips' stream
        first, then the jitter's, each drawn exactly once per batch whether or not the other is on"""
        rows = None if self.flip is None else self.flip.rows(num_clips, num_frames)
        return rows, (None if self.jitter is None else self.jitter.rows(num_clips, num_frames))

    def mirror_labels(self, labels, flags: torch.Tensor) -> None:
        self.flip.mirror_labels(labels, flags)

    def stats(self) -> dict:
        """host counts for the pass's info: clips mirrored (with cfg.flip_prob > 0), clips that drew a colour factor other than 1"""
        return {**({} if self.flip is None else {"flipped_clips": self.flip.flipped}),
                **({} if self.jitter is None else {"jittered_clips": self.jitter.jittered})}


def feed_for(loader, device, augment: Optional[PassAugment] = None):
    """the device feed of a pass: CachedFeed for a CachedLoader, input_feed.DeviceFeed for anything else; with the augmentations of a
    training pass (`augmentations`) the CachedFeed mirrors and jitters inside its gather and a plain loader goes through FlippedFeed"""
    if isinstance(loader, CachedLoader):
        return loader.feed(device, augment)
    return DeviceFeed(loader, device) if augment is None else FlippedFeed(loader, device, augment)


def augmentations(cfg, epoch: int, rank: int) -> Optional[PassAugment]:
    """what a trainer's training pass hands to `feed_for`: the flips and colour factors of epoch `epoch` on rank `rank`, or None with
    cfg.flip_prob == 0 and cfg.color_jitter = None (the pass is fed exactly as an evaluation pass then)"""
    flip, jitter = flip_plan(cfg, epoch, rank), jitter_plan(cfg, epoch, rank)
    return None if flip is None and jitter is None else PassAugment(flip, jitter)


def end_pass(feed) -> None:
    """what a trainer's pass calls after its last batch: the feature cache's box check (feature_cache.FeatureFeed.check); the other
    feeds have nothing to check"""
    check = getattr(feed, "check", None)
    if check is not None:
        check()


def wants_features(cfg) -> bool:
    return float(getattr(cfg, "feature_cache_gb", 0) or 0) > 0


def wants_maps(cfg) -> bool:
    return float(getattr(cfg, "map_cache_gb", 0) or 0) > 0


def wants_frame_ids(cfg) -> bool:
    return float(getattr(cfg, "frame_cache_gb", 0) or 0) > 0 or wants_features(cfg) or wants_maps(cfg)


def build_loaders(cfg, training_set, validation_set, per_rank: int, sampler, device, real_tree: bool):
    """the two DataLoaders of train_net / train_net_dynamic.  With cfg.num_workers = 0 and cfg.frame_cache_gb = 0 (the defaults), or
    without the real dataset tree, exactly the loaders the trainers always built.  Otherwise cfg.num_workers worker processes per loader
    (the platform's default start method; they decode and never touch the GPU; a stuck worker raises after LOADER_TIMEOUT_S), and, when
    the datasets carry frame ids, one FrameCache of cfg.frame_cache_gb per dataset behind a CachedLoader -- or, with cfg.feature_cache_gb > 0
    (train_net_dynamic only, frozen backbone), one feature_cache.FeatureCache of that many GB per dataset behind a FeatureLoader."""
    workers = int(getattr(cfg, "num_workers", 0) or 0) if real_tree else 0
    extra = dict(num_workers=workers, timeout=LOADER_TIMEOUT_S) if workers > 0 else dict(num_workers=0)
    cached = real_tree and wants_frame_ids(cfg) and getattr(training_set, "frame_ids", False) and getattr(validation_set, "frame_ids", False)
    if cached:
        extra["collate_fn"] = collate
    training_loader = data.DataLoader(training_set, batch_size=per_rank, shuffle=sampler is None, sampler=sampler, **extra)
    validation_loader = data.DataLoader(validation_set, batch_size=cfg.test_batch_size, shuffle=False, **extra)
    if not cached:
        return training_loader, validation_loader
    if wants_features(cfg):
        from .feature_cache import feature_loaders
        return feature_loaders(cfg, training_loader, validation_loader, training_set, validation_set, device)
    if wants_maps(cfg):                              # (cfg.map_cache_gb: the frozen backbone's maps instead, feature_cache.MapCache)
        from .feature_cache import map_loaders
        return map_loaders(cfg, training_loader, validation_loader, training_set, validation_set, device)
    capacity = int(float(cfg.frame_cache_gb) * 1e9)
    frame_shape = (3,) + tuple(cfg.image_size)
    return (CachedLoader(training_loader, FrameCache(device, frame_shape, capacity), training_set),
            CachedLoader(validation_loader, FrameCache(device, frame_shape, capacity), validation_set))
