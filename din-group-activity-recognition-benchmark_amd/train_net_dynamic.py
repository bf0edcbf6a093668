"""Stage-2 trainer -- drop-in for the reference's train_net_dynamic.py (train_net :27-157, train_volleyball :159-235,
test_volleyball :238-312, train_collective :315-389, test_collective :392-471) on MI355X: one process per GPU (torchrun), clips
sharded over ranks, gradients all-reduced by RCCL (din_amd.parallel) instead of nn.DataParallel, fused Adam.  The info-dict keys of
the reference are kept; train / test loops are picked by cfg.dataset_name as in the reference (:106-109).

Checkpoints follow the reference: `cfg.load_backbone_stage2` loads the stage-1 backbone + embedding (`model.loadmodel`, :80-81),
`cfg.load_stage2model` resumes a stage-2 `{'epoch', 'state_dict', 'optimizer'}` file (:82-88; a `module.` prefix left by nn.DataParallel
is stripped), and the file written after every test epoch has the same three keys with torch.optim.Adam's optimizer format.
BatchNorm follows `cfg.set_bn_eval` exactly like :98-100 / :170-172: model.train(), then BatchNorm modules back to eval() when the flag is
set (train_collective does that unconditionally, :323-324).

Datasets are out of scope: `train_net(cfg, training_set, validation_set)` takes any torch Dataset yielding the
reference's tuples (volleyball: images [T,3,H,W] 0..255, boxes [T,N,4] feature px, actions [T,N], activities [T]; collective: the same
with MAX_N boxes plus bboxes_num [T]); with none given it trains on a synthetic set of that shape.
"""
from __future__ import annotations

import copy
import os

import random
import time

import numpy as np
import torch
import torch.nn.functional as F
import torch.utils.data as data

from . import ops, parallel
from . import feature_cache, frame_cache
from .input_feed import DeviceFeed  # noqa: F401  (re-exported: `from train_net import *` launchers)
from .infer_model import (ARG_volleyball, AT_volleyball, Dynamic_collective, Dynamic_TCE_volleyball, Dynamic_volleyball,
                          PCTDM_volleyball)
from .optim import FusedAdam, grad_norm_refusal
from .utils import AverageMeter, Timer, print_log


def set_bn_eval(m):
    """reference train_net_dynamic.py:17-20"""
    if m.__class__.__name__.find("BatchNorm") != -1:
        m.eval()


def adjust_lr(optimizer, new_lr):
    print("change learning rate:", new_lr)
    for group in optimizer.param_groups:
        group["lr"] = new_lr


class SyntheticVolleyball(data.Dataset):
    """Volleyball-shaped random clips: uint8 images, player-shaped boxes in feature px, labels."""

    def __init__(self, cfg, length=8, seed=0):
        self.cfg, self.length, self.seed = cfg, length, seed

    def __len__(self):
        return self.length

    def _clip(self, i):
        cfg = self.cfg
        T, N = cfg.num_frames, cfg.num_boxes
        H, W = cfg.image_size
        OH, OW = cfg.out_size
        r = np.random.default_rng(self.seed * 100003 + i)
        images = torch.from_numpy(r.integers(0, 256, size=(T, 3, H, W), dtype=np.uint8))
        cx, cy = r.uniform(0.05, 0.95, (T, N)) * OW, r.uniform(0.3, 0.9, (T, N)) * OH
        bw, bh = r.uniform(0.03, 0.08, (T, N)) * OW, r.uniform(0.15, 0.35, (T, N)) * OH
        boxes = np.stack([np.clip(cx - bw / 2, 0, OW), np.clip(cy - bh / 2, 0, OH), np.clip(cx + bw / 2, 0, OW),
                          np.clip(cy + bh / 2, 0, OH)], -1).astype(np.float32)
        actions = torch.from_numpy(r.integers(0, cfg.num_actions, size=(T, N)).astype(np.int64))
        activities = torch.full((T,), int(r.integers(0, cfg.num_activities)), dtype=torch.int64)
        return r, images, torch.from_numpy(boxes), actions, activities

    def __getitem__(self, i):
        return self._clip(i)[1:]


class SyntheticCollective(SyntheticVolleyball):
    """Collective-Activity-shaped clips (reference collective.py:150-215): cfg.num_boxes is MAX_N, each clip has 1..MAX_N actors
    (the same count in all of its frames), padding boxes are zero, plus the `bboxes_num [T]` entry."""

    def __getitem__(self, i):
        r, images, boxes, actions, activities = self._clip(i)
        T, N = self.cfg.num_frames, self.cfg.num_boxes
        n = int(r.integers(1, N + 1))
        boxes[:, n:] = 0.0
        actions[:, n:] = -1
        return images, boxes, actions, activities, torch.full((T,), n, dtype=torch.int32)


def build_model(cfg):
    registry = {"dynamic_volleyball": Dynamic_volleyball, "dynamic_tce_volleyball": Dynamic_TCE_volleyball,
                "dynamic_collective": Dynamic_collective, "arg_volleyball": ARG_volleyball,
                "at_volleyball": AT_volleyball, "pctdm_volleyball": PCTDM_volleyball}          # reference train_net_dynamic.py:66-73
    if cfg.inference_module_name not in registry:
        raise NotImplementedError(f"{cfg.inference_module_name}: only the DIN models and the ARG / AT / PCTDM baselines are on the MI355X hot path")
    return registry[cfg.inference_module_name](cfg)


class _Epoch:
    """meters of one pass: loss / accuracy / confusion matrix, accumulated on the device and read ONCE at the end of the pass (the
    reference reads .item() every batch, a host sync per step)"""

    def __init__(self, cfg, device):
        self.conf = torch.zeros(cfg.num_activities, cfg.num_activities, dtype=torch.int64, device=device)
        self.loss_sum = torch.zeros((), dtype=torch.float64, device=device)
        self.clips = 0
        self.timer = Timer()

    def add(self, scores, target, loss):
        pred = torch.argmax(scores, dim=1)
        self.conf.index_put_((target.long(), pred), torch.ones_like(pred, dtype=torch.int64), accumulate=True)
        self.loss_sum += loss.detach().double() * scores.shape[0]
        self.clips += scores.shape[0]

    def info(self, epoch):
        conf = self.conf.cpu().float()
        total = max(self.clips, 1)
        per_class = conf.diag() / conf.sum(1).clamp(min=1)
        return {"time": self.timer.timeit(), "epoch": epoch, "loss": float(self.loss_sum.item()) / total,
                "activities_acc": float(conf.diag().sum()) / total * 100, "activities_conf": conf.numpy(),
                "activities_MPCA": float(per_class.mean() * 100)}


def _train_pass(data_loader, model, device, optimizer, epoch, cfg, grad_buckets, collective, max_batches=None):
    meters = _Epoch(cfg, device)
    augment = frame_cache.augmentations(cfg, epoch, parallel.current_rank())      # None unless cfg.flip_prob > 0 or cfg.color_jitter is set
    feed = frame_cache.feed_for(data_loader, device, augment)
    for bi, batch_data in enumerate(feed):                             # batch k+1 crosses PCIe on the copy stream during step k
        if max_batches is not None and bi >= max_batches:
            break
        model.train()
        if cfg.set_bn_eval or collective:                              # reference :170-172 / :323-324
            model.apply(set_bn_eval)
        batch_size, num_frames = batch_data[0].shape[0], batch_data[0].shape[1]
        activities_in = batch_data[3].reshape((batch_size, num_frames))[:, 0].reshape((batch_size,))
        inputs = (batch_data[0], batch_data[1], batch_data[4]) if collective else (batch_data[0], batch_data[1])
        ret = model(inputs)
        activities_scores = ret["activities"]
        total_loss = F.cross_entropy(activities_scores, activities_in)
        optimizer.zero_grad()
        total_loss.backward()
        if grad_buckets is not None:
            grad_buckets.allreduce(scale_in_optimizer=True)        # the 1 / world factor rides in the fused Adam kernel
            optimizer.step(grad_scale=grad_buckets.grad_scale)
        else:
            optimizer.step()
        meters.add(activities_scores.detach(), activities_in, total_loss)
    frame_cache.end_pass(feed)                                         # (the feature cache's box check; nothing for the other feeds)
    return add_flip_stats(add_grad_stats(meters.info(epoch), optimizer), augment)


def add_flip_stats(info, augment):
    """the host counts of the pass's augmentations join its info (frame_cache.PassAugment.stats: `flipped_clips`, `jittered_clips`)"""
    if augment is not None:
        info.update(augment.stats())
    return info


def add_grad_stats(info, optimizer):
    """with cfg.max_grad_norm set: the pass's gradient-norm statistics join its info (one device read per pass, like the meters)"""
    if getattr(optimizer, "max_grad_norm", None) is not None:
        st = optimizer.grad_stats()
        info.update(grad_norm_mean=st["norm_mean"], grad_norm_max=st["norm_max"], skipped_steps=st["skipped"], clipped_steps=st["clipped"])
    return info


def grad_stats_line(epoch, info):
    return ("Train epoch %d: grad norm mean %.4g max %.4g, %d steps clipped, %d skipped (non-finite norm)"
            % (epoch, info["grad_norm_mean"], info["grad_norm_max"], info["clipped_steps"], info["skipped_steps"]))


def combine_flip_scores(scores, mirrored_scores, label_map=None):
    """test-time flipping (cfg.test_flip): 0.5 * (s + s_m[:, map]) in fp32.  scores [B, A] of the clips as decoded, mirrored_scores
    [B, A] of their mirror images; label_map (volleyball.FLIP_ACTIVITIES; None: the identity, labels without a side): a mirrored
    l_spike looks like r_spike, so the mirrored clip's column map[a] is the evidence for class a."""
    s, m = scores.float(), mirrored_scores.float()
    if label_map is not None:
        m = m[:, label_map if isinstance(label_map, torch.Tensor) else torch.tensor(list(label_map), dtype=torch.int64, device=m.device)]
    return 0.5 * (s + m)


class _Mirror:
    """the mirror images of an evaluation batch (cfg.test_flip), no random draw: a FrameRefs of a loader with a mirror cache turns
    every row over (feature_cache.FrameRefs.mirrored); an images tensor goes through one din_copy_rows_u8_flip launch; the boxes
    through one din_flip_clip_labels launch either way (the labels stay: the scores are read through the label map instead)"""

    def __init__(self, cfg, device):
        self.width, self.tables, self.flags = float(cfg.out_size[1]), frame_cache.TableUpload(device), None
        self.label_map = None
        if cfg.dataset_name == "volleyball":
            from .volleyball import FLIP_ACTIVITIES
            self.label_map = torch.tensor(FLIP_ACTIVITIES, dtype=torch.int64, device=device)

    def inputs(self, images, boxes, bboxes_num=None):
        rows = images.shape[0] * images.shape[1]
        if isinstance(images, feature_cache.FrameRefs):
            if images.mirror is None:
                raise ValueError("test_flip: the loader's feature cache has no mirror cache (cfg.feature_cache_flip)")
            if self.flags is None or self.flags.numel() != rows:
                self.flags = torch.ones(rows, dtype=torch.int64, device=boxes.device)
            mirrored, flags = images.mirrored(boxes), self.flags
        else:
            if images.dtype != torch.uint8 or not images.is_contiguous():
                raise ValueError(f"test_flip works on contiguous uint8 [B, T, 3, H, W] frames on the device; the loader gave {images.dtype} "
                                 f"{tuple(images.shape)}")
            mirrored = torch.empty_like(images)
            fb = images[0, 0].numel()
            flags = self.tables.gather_rows([images.data_ptr() + i * fb for i in range(rows)], [mirrored.data_ptr() + i * fb for i in range(rows)],
                                            images.shape[2:], np.ones(rows, dtype=bool))
        boxes_m = boxes.clone()
        ops.flip_clip_labels(boxes_m, None, flags, None if bboxes_num is None else bboxes_num.contiguous(), None, self.width)
        return (mirrored, boxes_m) if bboxes_num is None else (mirrored, boxes_m, bboxes_num)


def _test_pass(data_loader, model, device, epoch, cfg, collective):
    model.eval()
    meters = _Epoch(cfg, device)
    feed = frame_cache.feed_for(data_loader, device)
    mirror = _Mirror(cfg, device) if getattr(cfg, "test_flip", False) else None      # (off: the pass below is what it always was)
    with torch.no_grad():
        for batch_data in feed:
            batch_size, num_frames = batch_data[0].shape[0], batch_data[0].shape[1]
            activities_in = batch_data[3].reshape((batch_size, num_frames))[:, 0].reshape((batch_size,))
            inputs = (batch_data[0], batch_data[1], batch_data[4]) if collective else (batch_data[0], batch_data[1])
            scores = model(inputs)["activities"]
            if mirror is not None:                                     # both orientations, averaged; the labels are the unmirrored ones
                scores = combine_flip_scores(scores, model(mirror.inputs(*inputs))["activities"], mirror.label_map)
            meters.add(scores, activities_in, F.cross_entropy(scores, activities_in))
    frame_cache.end_pass(feed)
    return meters.info(epoch)


def train_volleyball(data_loader, model, device, optimizer, epoch, cfg, grad_buckets=None, max_batches=None):
    return _train_pass(data_loader, model, device, optimizer, epoch, cfg, grad_buckets, False, max_batches)


def test_volleyball(data_loader, model, device, epoch, cfg):
    return _test_pass(data_loader, model, device, epoch, cfg, False)


def train_collective(data_loader, model, device, optimizer, epoch, cfg, grad_buckets=None, max_batches=None):
    """reference :315-389 with `ret['activities']` (the reference hands the model's dict to cross_entropy, SURVEY 0 bug 3)"""
    return _train_pass(data_loader, model, device, optimizer, epoch, cfg, grad_buckets, True, max_batches)


def test_collective(data_loader, model, device, epoch, cfg):
    return _test_pass(data_loader, model, device, epoch, cfg, True)


def load_stage2_state(model, path):
    """reference :82-88: `{'epoch', 'state_dict', 'optimizer'}`; keys saved through nn.DataParallel carry a 'module.' prefix"""
    state = torch.load(path, map_location="cpu", weights_only=False)
    sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in state["state_dict"].items()}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    bad = [k for k in missing if "num_batches_tracked" not in k]
    if bad or unexpected:
        raise RuntimeError(f"stage-2 checkpoint {path} does not match the model: missing {bad[:5]}, unexpected {list(unexpected)[:5]}")
    return state


def _mask_counters(model):
    return [(n, m) for n, m in model.named_modules() if hasattr(m, "_step") and isinstance(getattr(m, "_step"), int)]


def train_net(cfg, training_set=None, validation_set=None, max_steps=None):
    """Reference train_net (:27-157).  Launch one process per GPU with torchrun; a single process works too.  max_steps bounds the number
    of epochs (smoke runs).  cfg.deterministic: the whole call runs under ops.deterministic() (frozen backbone, one rank; the option is
    back at its previous value when the call returns or raises).  cfg.max_grad_norm: see din_amd/optim.py (FusedAdam)."""
    why_not = grad_norm_refusal(getattr(cfg, "max_grad_norm", None))       # (before anything else: it needs no device and no loader)
    if why_not:
        raise ValueError(why_not)
    # cfg.deterministic where a sum's order is not ours (first: its answer is the same whatever the caches and workers are set to), then
    # cfg.feature_cache_gb > 0 where cached features would be wrong -- both before any process group or loader exists
    # -- then cfg.flip_prob where a mirrored clip cannot be fed, and cfg.color_jitter likewise
    # -- and cfg.feature_cache_path without a feature cache to keep there
    why_not = (ops.deterministic_refusal(cfg, int(os.environ.get("WORLD_SIZE", "1"))) or feature_cache.refusal(cfg)
               or frame_cache.flip_refusal(cfg) or frame_cache.jitter_refusal(cfg) or feature_cache.path_refusal(cfg)
               or feature_cache.flip_cache_refusal(cfg)                      # (cfg.feature_cache_flip, cfg.test_flip)
               or feature_cache.map_refusal(cfg))                            # (cfg.map_cache_gb: after every other refusal)
    if why_not:
        raise ValueError(why_not)
    if getattr(cfg, "deterministic", False):
        with ops.deterministic():
            return _train_net(cfg, training_set, validation_set, max_steps)
    return _train_net(cfg, training_set, validation_set, max_steps)


def _train_net(cfg, training_set, validation_set, max_steps):
    rank, local_rank, world = parallel.init_from_env()
    np.random.seed(cfg.train_random_seed)
    torch.manual_seed(cfg.train_random_seed)
    random.seed(cfg.train_random_seed)
    device = torch.device("cuda", local_rank)
    torch.cuda.set_device(device)
    collective = cfg.dataset_name == "collective"
    synth = SyntheticCollective if collective else SyntheticVolleyball
    real_tree = False
    if training_set is None and validation_set is None and getattr(cfg, "data_path", None) and os.path.isdir(cfg.data_path):
        # the real datasets (reference train_net_dynamic.py:57-58 -> dataset.return_dataset): annotation trees + JPEG frames -> uint8 clips,
        # feature-px boxes, padded tracks (din_amd/volleyball.py, collective.py); without a data tree the synthetic clips stand in
        from .dataset import return_dataset
        training_set, validation_set = return_dataset(cfg, frame_ids=frame_cache.wants_frame_ids(cfg))
        real_tree = True
    training_set = training_set or synth(cfg, length=max(cfg.batch_size * 2, 4))
    if validation_set is None and cfg.inference_module_name == "arg_volleyball":
        # ARG test clips hold three sub-clips of num_frames frames each (volleyball.py:212-214, infer_model.py:939-943)
        vcfg = copy.copy(cfg)
        vcfg.num_frames = 3 * cfg.num_frames
        validation_set = synth(vcfg, length=max(cfg.test_batch_size, 2), seed=1)
    validation_set = validation_set or synth(cfg, length=max(cfg.test_batch_size, 2), seed=1)
    if cfg.batch_size % world != 0:
        raise ValueError(f"batch_size {cfg.batch_size} must be divisible by the number of ranks {world}: the gradient all-reduce averages "
                         f"per-rank means, which is the global mean only for equal shards")
    per_rank = cfg.batch_size // world
    sampler = data.distributed.DistributedSampler(training_set, world, rank, shuffle=True) if world > 1 else None
    # cfg.num_workers / cfg.frame_cache_gb (both 0 by default: the loaders below are then the plain num_workers=0 DataLoaders) apply to
    # the real dataset tree only: worker processes decode, and decoded frames stay in HBM from their first use on (frame_cache.py); with
    # cfg.feature_cache_gb > 0 the frozen trunk's box features stay there instead (feature_cache.py), with cfg.map_cache_gb > 0 its
    # output maps (feature_cache.MapCache: Dynamic_TCE_volleyball and the collective dataset too).  The caches live for this call;
    # with cfg.feature_cache_path the feature caches start from their files and are written back when they grew (`files` below).
    training_loader, validation_loader = frame_cache.build_loaders(cfg, training_set, validation_set, per_rank, sampler, device, real_tree)
    log_path = getattr(cfg, "log_path", None)
    if cfg.training_stage != 2:
        raise NotImplementedError("training_stage 1 (Basenet) is out of scope: the MI355X hot path is the stage-2 DIN step")
    model = build_model(cfg)
    resume = None
    if cfg.load_backbone_stage2:                                       # :80-81
        model.loadmodel(cfg.stage1_model_path)
    elif cfg.load_stage2model:                                         # :82-88
        resume = load_stage2_state(model, cfg.stage2model)
        print_log(log_path, "Loading stage2 model: " + str(cfg.stage2model))
    else:
        print_log(log_path, "Not loading stage1 or stage2 model.")
    model = model.to(device)
    parallel.broadcast_parameters(model)
    model.train()
    if cfg.set_bn_eval:
        model.apply(set_bn_eval)
    params = [p for p in model.parameters() if p.requires_grad]
    optimizer = FusedAdam(params, lr=cfg.train_learning_rate, weight_decay=cfg.weight_decay, max_grad_norm=getattr(cfg, "max_grad_norm", None))
    start_epoch = 1
    if resume is not None and getattr(cfg, "resume_optimizer", True) and "optimizer" in resume:
        # (the reference reloads only the weights; resuming the moments, the epoch and the dropout-mask counters too is the extension
        #  `cfg.resume_optimizer`, default on)
        try:
            optimizer.load_state_dict(resume["optimizer"])
            start_epoch = int(resume.get("epoch", 0)) + 1
            for name, m in _mask_counters(model):
                if name in resume.get("mask_steps", {}):
                    m._step = int(resume["mask_steps"][name])
        except (ValueError, KeyError) as e:
            print_log(log_path, f"optimizer state of {cfg.stage2model} not resumed: {e}")
    buckets = parallel.GradBuckets(params) if world > 1 else None
    train = train_collective if collective else train_volleyball
    test = test_collective if collective else test_volleyball
    # cfg.feature_cache_path (None: `files` is empty and nothing below differs): the model has its stage-1 weights, so the fingerprints
    # can be taken; each cache takes its file in before the first pass, and is written after every pass in which it took frames in
    files = feature_cache.cache_files(cfg, model, training_loader, validation_loader, rank, world, lambda line: print_log(log_path, line))
    for f in files.values():
        f.load()

    # cfg.map_cache_gb (0: `map_caches` is empty and nothing below differs): a pass's info gains the rows its cache served from slots
    # and the frames it took in, and the log one line per pass
    map_caches = {split: ld.cache for split, ld in (("train", training_loader), ("val", validation_loader))
                  if isinstance(getattr(ld, "cache", None), feature_cache.MapCache)}

    def with_map_stats(split, run_pass):
        cache = map_caches.get(split)
        if cache is None:
            return run_pass()
        hits, inserted = cache.hits, cache.inserted
        info = run_pass()
        info.update(map_cache_hits=cache.hits - hits, map_cache_inserted=cache.inserted - inserted)
        print_log(log_path, f"map cache {split} epoch {info['epoch']}: {info['map_cache_hits']} rows from slots, {info['map_cache_inserted']} "
                            f"frames inserted; {cache.inserted} frames, {cache.bytes / 1e9:.3f} GB resident")
        return info

    def with_file(split, run_pass):
        f = files.get(split)
        if f is None:
            return with_map_stats(split, run_pass)
        before = f.inserted
        info = run_pass()
        info.update(feature_cache_loaded=f.loaded, feature_cache_saved=f.save_if_grown(before))
        if f.flip_path is not None:                                    # (a loader with a mirror cache: its file's counts as well)
            info.update(feature_cache_flip_loaded=f.flip_loaded, feature_cache_flip_saved=f.flip_written)
        return info

    if cfg.test_before_train:
        print(with_file("val", lambda: test(validation_loader, model, device, 0, cfg)))
    infos = []
    best_result = {"epoch": 0, "activities_acc": 0}
    for epoch in range(start_epoch, start_epoch + cfg.max_epoch):
        if epoch in cfg.lr_plan:
            adjust_lr(optimizer, cfg.lr_plan[epoch])
        if sampler is not None:
            sampler.set_epoch(epoch)
        info = with_file("train", lambda: train(training_loader, model, device, optimizer, epoch, cfg, buckets))
        if rank == 0:
            print_log(log_path, "Train epoch %d: loss %.5f acc %.2f%%" % (epoch, info["loss"], info["activities_acc"]))
            if "grad_norm_mean" in info:
                print_log(log_path, grad_stats_line(epoch, info))
        if epoch % cfg.test_interval_epoch == 0:
            tinfo = with_file("val", lambda: test(validation_loader, model, device, epoch, cfg))
            if tinfo["activities_acc"] > best_result["activities_acc"]:
                best_result = tinfo
            if rank == 0:
                print_log(log_path, "Test epoch %d: loss %.5f acc %.2f%%" % (epoch, tinfo["loss"], tinfo["activities_acc"]))
                print_log(log_path, "Best group activity accuracy: %.2f%% at epoch #%d." % (best_result["activities_acc"], best_result["epoch"]))
                result_path = getattr(cfg, "result_path", None)
                if result_path:                                        # :141-147
                    state = {"epoch": epoch, "state_dict": model.state_dict(), "optimizer": optimizer.state_dict(),
                             "mask_steps": {name: m._step for name, m in _mask_counters(model)}}
                    torch.save(state, result_path + "/stage%d_epoch%d_%.2f%%.pth" % (cfg.training_stage, epoch, tinfo["activities_acc"]))
            info = dict(train=info, test=tinfo)
        infos.append(info)
        if max_steps is not None and len(infos) >= max_steps:
            break
    return infos
