"""The box-feature cache on disk: one data file per cache, and the fingerprint that says which runs may read it.

The rows feature_cache.FeatureCache keeps -- a frame's RoIAlign output [N, D, K, K] and the boxes it was computed for -- depend on the
frames, the boxes and the frozen backbone, and on nothing else: not on the head, the learning rate or the seed.  A file written by one
stage-2 run therefore serves every other run over the same frames with the same backbone (DIN, ARG, AT and PCTDM of one comparison, every
point of a sweep), which then decodes nothing and launches no backbone kernel from its first step.

Layout (little endian, data only -- nothing in it is unpickled or executed):

    bytes 0..7      MAGIC
    bytes 8..11     uint32 format VERSION
    bytes 12..19    uint64 L, the length of the header
    bytes 20..20+L  the header, UTF-8 JSON: {"fingerprint": {field: value, ..., "digest": sha256}, "row_bytes", "box_bytes", "dtype", "count"}
                    (a mirror cache's file, cfg.feature_cache_flip, adds "orientation": "mirrored"; a plain file has no such key)
    then            ids, int64 [count]: the frame ids in slot order
    zero padding up to the next multiple of ALIGN
    then            count records of row_bytes + box_bytes bytes: a slot's bytes exactly as FeatureCache holds them, the row, then its boxes

Pure host code (numpy, hashlib, json): importable and testable without a GPU.  feature_cache.FeatureCache.save / load move the records
between the slabs and a file; train_net_dynamic decides when (cfg.feature_cache_path).
"""
from __future__ import annotations

import hashlib
import json
import os
import struct
from typing import Iterable, Optional, Tuple

import numpy as np

MAGIC = b"DINFCACH"
VERSION = 1
ALIGN = 4096                    # the record region starts on a multiple of this
_PREFIX = struct.Struct("<8sIQ")
MAX_HEADER = 1 << 24            # a header length beyond this is a defect, not something to allocate

# the fingerprint's fields, in the order a mismatch is reported in
FIELDS = ("dataset_name", "sequences", "frames", "image_size", "out_size", "crop_size", "emb_features", "num_boxes", "backbone",
          "backbone_dtype", "feature_cache_dtype", "set_bn_eval", "din_abi_version", "backbone_weights")
DTYPE_BYTES = {"fp32": 4, "bf16": 2}


def records_offset(header_len: int, count: int) -> int:
    """where the record region starts: the first multiple of ALIGN after the prefix, the header and the ids"""
    return (_PREFIX.size + header_len + 8 * count + ALIGN - 1) // ALIGN * ALIGN


def _geometry_defect(meta) -> Optional[str]:
    for k in ("row_bytes", "box_bytes"):
        v = meta.get(k)
        if isinstance(v, bool) or not isinstance(v, int) or v <= 0 or v % 16:
            return f"{k} = {v!r} is not a positive multiple of 16"
    if meta.get("dtype") not in DTYPE_BYTES:
        return f"dtype = {meta.get('dtype')!r} is not one of {sorted(DTYPE_BYTES)}"
    if not isinstance(meta.get("fingerprint"), dict):
        return "the header has no fingerprint"
    return None


def write(path: str, meta: dict, ids, blocks: Iterable) -> int:
    """write a cache file: meta = {"fingerprint", "row_bytes", "box_bytes", "dtype"}, ids int64 [count], blocks an iterator of host byte
    blocks (anything np.frombuffer-able or a uint8 array) of whole records, count records in all, in the order of ids.  Everything goes
    to path + ".tmp", which is flushed to the disk and then renamed over `path`: if anything raises on the way -- the iterator included
    -- the previous file is intact and the temporary file is removed.  Returns the bytes written."""
    ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int64).reshape(-1))
    header = {k: meta.get(k) for k in ("fingerprint", "row_bytes", "box_bytes", "dtype")}
    if meta.get("orientation", "plain") != "plain":              # a mirror cache's file says so; a plain file has no such key
        header["orientation"] = str(meta["orientation"])
    header["count"] = int(ids.size)
    why = _geometry_defect(header)
    if why:
        raise ValueError(f"feature cache file {path}: {why}")
    if np.unique(ids).size != ids.size:
        raise ValueError(f"feature cache file {path}: duplicate ids")
    text = json.dumps(header, sort_keys=True).encode("utf-8")
    rec = header["row_bytes"] + header["box_bytes"]
    start = records_offset(len(text), ids.size)
    tmp = path + ".tmp"
    try:
        with open(tmp, "wb") as fh:
            fh.write(_PREFIX.pack(MAGIC, VERSION, len(text)))
            fh.write(text)
            fh.write(ids.tobytes())
            fh.write(b"\0" * (start - fh.tell()))
            done = 0
            for block in blocks:
                block = np.ascontiguousarray(block).reshape(-1).view(np.uint8) if isinstance(block, np.ndarray) else np.frombuffer(block, dtype=np.uint8)
                if block.size % rec:
                    raise ValueError(f"feature cache file {path}: a block of {block.size} bytes is not a whole number of {rec}-byte records")
                fh.write(memoryview(block))
                done += block.size // rec
            if done != ids.size:
                raise ValueError(f"feature cache file {path}: {done} records were handed over for {ids.size} ids")
            total = fh.tell()
            fh.flush()
            os.fsync(fh.fileno())
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise
    return total


def read(path: str) -> Tuple[dict, np.ndarray, np.ndarray]:
    """(header, ids int64 [count], records): records is a READ-ONLY np.memmap uint8 [count, row_bytes + box_bytes] (a plain empty array
    for count 0: nothing can be mapped).  ValueError naming the defect for a wrong magic or version, a header that does not parse, a
    row_bytes or box_bytes that is not a positive multiple of 16, a file shorter or longer than count says, duplicate ids."""
    bad = lambda why: ValueError(f"feature cache file {path}: {why}")       # noqa: E731
    size = os.path.getsize(path)
    with open(path, "rb") as fh:
        prefix = fh.read(_PREFIX.size)
        if len(prefix) < _PREFIX.size or prefix[:8] != MAGIC:
            raise bad(f"wrong magic {prefix[:8]!r} (a feature cache file starts with {MAGIC!r})")
        _, version, hlen = _PREFIX.unpack(prefix)
        if version != VERSION:
            raise bad(f"format version {version}, this code reads version {VERSION}")
        if hlen > MAX_HEADER or _PREFIX.size + hlen > size:
            raise bad(f"the header does not parse: its length {hlen} is beyond the file")
        try:
            header = json.loads(fh.read(hlen).decode("utf-8"))
        except ValueError as e:                      # (UnicodeDecodeError and json.JSONDecodeError are both ValueErrors)
            raise bad(f"the header does not parse: {e}") from None
        if not isinstance(header, dict):
            raise bad("the header does not parse: it is not a JSON object")
        why = _geometry_defect(header)
        if why:
            raise bad(why)
        count = header.get("count")
        if isinstance(count, bool) or not isinstance(count, int) or count < 0:
            raise bad(f"count = {count!r} is not a number of records")
        rec = header["row_bytes"] + header["box_bytes"]
        start = records_offset(hlen, count)
        want = start + count * rec
        if size != want:
            raise bad(f"the file is {'shorter' if size < want else 'longer'} than its count of {count} records says: {size} bytes, not {want}")
        ids = np.frombuffer(fh.read(8 * count), dtype=np.int64)
    if np.unique(ids).size != ids.size:
        raise bad("duplicate ids")
    if count == 0:
        records = np.empty((0, rec), dtype=np.uint8)
        records.setflags(write=False)
    else:
        records = np.memmap(path, dtype=np.uint8, mode="r", offset=start, shape=(count, rec))
    return header, ids, records


# ---- the fingerprint --------------------------------------------------------------------------------------------------------------------
def _tensor_bytes(t) -> bytes:
    import torch
    t = t.detach().cpu().contiguous()
    return t.reshape(-1).view(torch.uint8).numpy().tobytes() if t.numel() else b""


def weights_digest(state_dict) -> str:
    """sha256 over every entry of a state_dict in sorted key order -- parameters and buffers alike, BatchNorm running statistics included:
    each contributes its key, dtype, shape and raw bytes"""
    h = hashlib.sha256()
    for key in sorted(state_dict):
        t = state_dict[key]
        h.update(f"{key}|{t.dtype}|{tuple(t.shape)}|".encode("utf-8"))
        h.update(_tensor_bytes(t))
    return h.hexdigest()


def frames_digest(dataset) -> str:
    """sha256 over the dataset's frame table, the paths taken relative to its image root: a frame id is an index into that table, so a
    file's ids name the same frames only under the same table (another window of frames around a clip gives another one)"""
    h = hashlib.sha256()
    root = getattr(dataset, "images_path", None)
    for p in dataset.frame_table:
        h.update((os.path.relpath(p, root) if root else p).replace(os.sep, "/").encode("utf-8") + b"\n")
    return h.hexdigest()


def fingerprint(cfg, model, dataset) -> dict:
    """what the rows of `dataset`'s cache depend on, as named fields (FIELDS) plus "digest", a sha256 over them.  Two runs with equal
    fingerprints compute the same rows.  Deliberately absent: inference_module_name, fc_emb_1 and every head parameter, the learning
    rate, the seed, batch_size -- the rows do not depend on them -- and the library build (rows written by an older build of the kernels
    are served as they are; only the ABI version is recorded).  Call it after the backbone has its stage-1 weights."""
    from . import _lib
    seqs = list(dict.fromkeys(int(f[0]) for f in dataset.frames))
    fp = {
        "dataset_name": str(cfg.dataset_name),
        "sequences": seqs,
        "frames": frames_digest(dataset),
        "image_size": [int(v) for v in cfg.image_size],
        "out_size": [int(v) for v in cfg.out_size],
        "crop_size": [int(v) for v in cfg.crop_size],
        "emb_features": int(cfg.emb_features),
        "num_boxes": int(cfg.num_boxes),
        "backbone": str(cfg.backbone),
        "backbone_dtype": str(getattr(cfg, "backbone_dtype", "fp32")),
        "feature_cache_dtype": str(getattr(cfg, "feature_cache_dtype", "fp32")),
        "set_bn_eval": bool(cfg.set_bn_eval),
        "din_abi_version": int(_lib.load().din_abi_version()),
        "backbone_weights": weights_digest(model.backbone.state_dict()),
    }
    assert tuple(fp) == FIELDS
    fp["digest"] = hashlib.sha256(json.dumps(fp, sort_keys=True).encode("utf-8")).hexdigest()
    return fp


def first_difference(ours: dict, theirs: dict) -> Optional[str]:
    """the first field of FIELDS in which two fingerprints differ, "digest" if only that does, None if they are equal"""
    for k in FIELDS + ("digest",):
        if ours.get(k) != theirs.get(k):
            return k
    return None


def file_name(split: str, rank: int = 0, world: int = 1) -> str:
    """the file of the `split` ("train" | "val") cache of rank `rank` of `world`: every rank's cache holds what its sampler showed it, so
    several ranks keep a file each"""
    return f"{split}.dinfc" if world <= 1 else f"{split}.rank{rank}of{world}.dinfc"


def flip_file_name(split: str, rank: int = 0, world: int = 1) -> str:
    """the file of the mirror cache of that split (cfg.feature_cache_flip), next to the plain one: train.flip.dinfc,
    train.flip.rank0of2.dinfc"""
    return file_name(split + ".flip", rank, world)
