"""Stage-1 trainer -- drop-in for the stage-1 branch of the reference's train_net.py (train_net :28-138, train_volleyball :140-200,
test_volleyball :203-258, train_collective :261-336, test_collective :339-408) on MI355X: the Basenet models of base_model.py, one process
per GPU (torchrun), clips sharded over ranks, gradients all-reduced by RCCL (din_amd.parallel) instead of nn.DataParallel, fused Adam, the
input feed overlapped with the step, and meters accumulated on the device and read once per pass.

The checkpoint is the reference's: whenever a test pass reaches the best group-activity accuracy so far, rank 0 writes
`model.savemodel(result_path + '/stage1_epoch%d_%.2f%%.pth')` (:129-135), the file that stage 2 reads through `cfg.load_backbone_stage2`
+ `cfg.stage1_model_path` (train_net_dynamic.train_net).  BatchNorm follows `cfg.set_bn_eval` for volleyball and is always in eval mode
for collective (:148-149, :269).

Deliberate differences from the reference:
  * `cfg.actions_weights is None` trains with an unweighted action loss (the reference crashes on `torch.tensor(None)`, :165); a nested
    list such as the launchers' `[[1., 1., 2., ...]]` is flattened to the 1-D class weights cross_entropy takes.
  * `training_stage == 2` (the ARG / GCN models of gcn_model.py) raises NotImplementedError: the stage-2 model on the MI355X path is DIN,
    trained by train_net_dynamic.train_net.
  * `train_net(cfg, training_set=None, validation_set=None, max_steps=None)` as train_net_dynamic: without datasets (and without a data
    tree at cfg.data_path) it trains on synthetic clips; max_steps bounds the number of epochs.  cfg.init_config() runs only when cfg has
    no result_path yet.
"""
from __future__ import annotations

import copy
import os
import random

import numpy as np
import torch
import torch.nn.functional as F
import torch.utils.data as data

from . import parallel
from .base_model import Basenet_collective, Basenet_volleyball
from .config import Config  # noqa: F401  (the reference's launchers do `from train_net import *` and then `Config('volleyball')`)
from . import frame_cache
from .input_feed import DeviceFeed  # noqa: F401  (re-exported: `from train_net import *` launchers)
from .optim import FusedAdam, grad_norm_refusal
from .train_net_dynamic import SyntheticCollective, SyntheticVolleyball, add_flip_stats, add_grad_stats, adjust_lr, grad_stats_line, set_bn_eval
from .utils import Timer, print_log


class _Meters:
    """loss / action accuracy / activity confusion of one pass, on the device; read ONCE at the end (the reference reads .item() per batch)"""

    def __init__(self, cfg, device):
        self.conf = torch.zeros(cfg.num_activities, cfg.num_activities, dtype=torch.int64, device=device)
        self.actions_correct = torch.zeros((), dtype=torch.int64, device=device)
        self.loss_sum = torch.zeros((), dtype=torch.float64, device=device)
        self.actions = self.activities = self.clips = 0
        self.timer = Timer()

    def add(self, actions_scores, actions_in, activities_scores, activities_in, loss, batch_size):
        pred = torch.argmax(activities_scores, dim=1)
        self.conf.index_put_((activities_in.long(), pred), torch.ones_like(pred, dtype=torch.int64), accumulate=True)
        self.actions_correct += torch.eq(torch.argmax(actions_scores, dim=1), actions_in).sum()
        self.loss_sum += loss.detach().double() * batch_size
        self.actions += actions_scores.shape[0]
        self.activities += activities_scores.shape[0]
        self.clips += batch_size

    def info(self, epoch):
        conf = self.conf.cpu().float()
        per_class = conf.diag() / conf.sum(1).clamp(min=1)
        return {"time": self.timer.timeit(), "epoch": epoch, "loss": float(self.loss_sum.item()) / max(self.clips, 1),
                "activities_acc": float(conf.diag().sum()) / max(self.activities, 1) * 100,
                "actions_acc": float(self.actions_correct.item()) / max(self.actions, 1) * 100,
                "activities_conf": conf.numpy(), "activities_MPCA": float(per_class.mean() * 100)}


def compact_actions(actions_in, bboxes_num, all_n):
    """actions [B*T, MAX_N] -> the labels of the first bboxes_num[bt] boxes of every frame, in (frame, box) order [all_n] (reference
    train_net.py:284-290), without a host loop or a device -> host read: padding entries are scattered into a spare last slot"""
    bt, n = actions_in.shape
    counts = bboxes_num.reshape(bt).long()
    off = torch.cumsum(counts, 0) - counts
    i = torch.arange(n, device=actions_in.device)
    pos = torch.where(i[None, :] < counts[:, None], off[:, None] + i[None, :], torch.full_like(off[:, None], all_n))
    out = torch.empty(all_n + 1, dtype=actions_in.dtype, device=actions_in.device)
    out.scatter_(0, pos.reshape(-1), actions_in.reshape(-1))
    return out[:all_n]


def _step_inputs(batch_data, cfg, collective):
    """model inputs and the targets of its two outputs (reference :151-160 / :275-295)"""
    batch_size, num_frames = batch_data[0].shape[0], batch_data[0].shape[1]
    actions_in = batch_data[2].reshape((batch_size, num_frames, cfg.num_boxes))
    activities_in = batch_data[3].reshape((batch_size, num_frames))
    if collective:
        return (batch_data[0], batch_data[1], batch_data[4]), actions_in, activities_in.reshape(-1), batch_size
    return (batch_data[0], batch_data[1]), actions_in[:, 0, :].reshape(batch_size * cfg.num_boxes), activities_in[:, 0], batch_size


def _losses(actions_scores, activities_scores, actions_in, activities_in, batch_data, cfg, collective):
    if collective:
        actions_in = compact_actions(actions_in.reshape(-1, cfg.num_boxes), batch_data[4], actions_scores.shape[0])
        weight = None
    else:
        weight = None
        if cfg.actions_weights is not None:
            weight = torch.tensor(cfg.actions_weights, dtype=torch.float32, device=actions_scores.device).reshape(-1)
    actions_loss = F.cross_entropy(actions_scores, actions_in, weight=weight)
    activities_loss = F.cross_entropy(activities_scores, activities_in)
    return activities_loss + cfg.actions_loss_weight * actions_loss, actions_in


def _train_pass(data_loader, model, device, optimizer, epoch, cfg, grad_buckets, collective, max_batches=None):
    meters = _Meters(cfg, device)
    augment = frame_cache.augmentations(cfg, epoch, parallel.current_rank())      # None unless cfg.flip_prob > 0 or cfg.color_jitter is set
    for bi, batch_data in enumerate(frame_cache.feed_for(data_loader, device, augment)):
        if max_batches is not None and bi >= max_batches:
            break
        model.train()
        if cfg.set_bn_eval or collective:                              # reference :148-149 / :269
            model.apply(set_bn_eval)
        inputs, actions_in, activities_in, batch_size = _step_inputs(batch_data, cfg, collective)
        actions_scores, activities_scores = model(inputs)
        total_loss, actions_in = _losses(actions_scores, activities_scores, actions_in, activities_in, batch_data, cfg, collective)
        optimizer.zero_grad()
        total_loss.backward()
        if grad_buckets is not None:
            grad_buckets.allreduce(scale_in_optimizer=True)
            optimizer.step(grad_scale=grad_buckets.grad_scale)
        else:
            optimizer.step()
        meters.add(actions_scores.detach(), actions_in, activities_scores.detach(), activities_in, total_loss, batch_size)
    return add_flip_stats(add_grad_stats(meters.info(epoch), optimizer), augment)


def _test_pass(data_loader, model, device, epoch, cfg, collective):
    model.eval()
    meters = _Meters(cfg, device)
    with torch.no_grad():
        for batch_data in frame_cache.feed_for(data_loader, device):
            inputs, actions_in, activities_in, batch_size = _step_inputs(batch_data, cfg, collective)
            actions_scores, activities_scores = model(inputs)
            total_loss, actions_in = _losses(actions_scores, activities_scores, actions_in, activities_in, batch_data, cfg, collective)
            meters.add(actions_scores, actions_in, activities_scores, activities_in, total_loss, batch_size)
    return meters.info(epoch)


def train_volleyball(data_loader, model, device, optimizer, epoch, cfg, grad_buckets=None, max_batches=None):
    return _train_pass(data_loader, model, device, optimizer, epoch, cfg, grad_buckets, False, max_batches)


def test_volleyball(data_loader, model, device, epoch, cfg):
    return _test_pass(data_loader, model, device, epoch, cfg, False)


def train_collective(data_loader, model, device, optimizer, epoch, cfg, grad_buckets=None, max_batches=None):
    return _train_pass(data_loader, model, device, optimizer, epoch, cfg, grad_buckets, True, max_batches)


def test_collective(data_loader, model, device, epoch, cfg):
    return _test_pass(data_loader, model, device, epoch, cfg, True)


def build_model(cfg):
    if cfg.training_stage == 2:
        raise NotImplementedError("train_net: training_stage 2 trains the ARG / GCN models of the reference's gcn_model.py, which are not "
                                  "on the MI355X path; the stage-2 DIN models train with train_net_dynamic.train_net")
    if cfg.training_stage != 1:
        raise ValueError(f"training_stage {cfg.training_stage!r}: train_net trains stage 1 (Basenet)")
    return {"volleyball": Basenet_volleyball, "collective": Basenet_collective}[cfg.dataset_name](cfg)    # :58-64


def train_net(cfg, training_set=None, validation_set=None, max_steps=None):
    """Reference train_net (:28-138), stage 1.  Launch one process per GPU with torchrun; a single process works too.  max_steps bounds
    the number of epochs (smoke runs).  cfg.deterministic is ignored here: stage 1 trains the backbone, whose bias / BatchNorm-scale
    gradients and RoIAlign backward have no fixed-order form (the stage-2 trainer's deterministic mode covers the frozen backbone).
    cfg.max_grad_norm: see din_amd/optim.py (FusedAdam)."""
    why_not = grad_norm_refusal(getattr(cfg, "max_grad_norm", None))       # (before anything else: it needs no device and no loader)
    if why_not:
        raise ValueError(why_not)
    why_not = frame_cache.flip_refusal(cfg) or frame_cache.jitter_refusal(cfg)     # (cfg.flip_prob, cfg.color_jitter: no device and no loader either)
    if why_not:
        raise ValueError(why_not)
    if getattr(cfg, "test_flip", False):
        raise ValueError(f"test_flip = {cfg.test_flip!r}: test-time flipping is the stage-2 trainer's (train_net_dynamic.train_net); stage 1 "
                         f"evaluates every clip as decoded")
    model = build_model(cfg)                                           # (refuses stage 2 before touching the device)
    if getattr(cfg, "result_path", None) is None:
        cfg.init_config()
    rank, local_rank, world = parallel.init_from_env()
    np.random.seed(cfg.train_random_seed)
    torch.manual_seed(cfg.train_random_seed)
    random.seed(cfg.train_random_seed)
    device = torch.device("cuda", local_rank)
    torch.cuda.set_device(device)
    collective = cfg.dataset_name == "collective"
    synth = SyntheticCollective if collective else SyntheticVolleyball
    real_tree = False
    lcfg = copy.copy(cfg)
    lcfg.feature_cache_gb = 0                                          # stage 1 trains the backbone: the box-feature cache is stage 2's
    lcfg.map_cache_gb = 0                                              # ... and so is the map cache
    if training_set is None and validation_set is None and getattr(cfg, "data_path", None) and os.path.isdir(cfg.data_path):
        from .dataset import return_dataset                           # stage-1 frame sampling (is_finetune) follows cfg.training_stage
        training_set, validation_set = return_dataset(cfg, frame_ids=frame_cache.wants_frame_ids(lcfg))
        real_tree = True
    training_set = training_set or synth(cfg, length=max(cfg.batch_size * 2, 4))
    validation_set = validation_set or synth(cfg, length=max(cfg.test_batch_size, 2), seed=1)
    if cfg.batch_size % world != 0:
        raise ValueError(f"batch_size {cfg.batch_size} must be divisible by the number of ranks {world}")
    per_rank = cfg.batch_size // world
    sampler = data.distributed.DistributedSampler(training_set, world, rank, shuffle=True) if world > 1 else None
    # cfg.num_workers / cfg.frame_cache_gb (both 0 by default: the loaders below are then the plain num_workers=0 DataLoaders) apply to
    # the real dataset tree only: worker processes decode, and decoded frames stay in HBM from their first use on (frame_cache.py)
    training_loader, validation_loader = frame_cache.build_loaders(lcfg, training_set, validation_set, per_rank, sampler, device, real_tree)
    log_path = getattr(cfg, "log_path", None)
    model = model.to(device)
    parallel.broadcast_parameters(model)
    model.train()
    if cfg.set_bn_eval:
        model.apply(set_bn_eval)
    params = [p for p in model.parameters() if p.requires_grad]
    optimizer = FusedAdam(params, lr=cfg.train_learning_rate, weight_decay=cfg.weight_decay, max_grad_norm=getattr(cfg, "max_grad_norm", None))
    buckets = parallel.GradBuckets(params) if world > 1 else None
    train = train_collective if collective else train_volleyball
    test = test_collective if collective else test_volleyball
    if cfg.test_before_train:
        print(test(validation_loader, model, device, 0, cfg))
    infos = []
    best_result = {"epoch": 0, "activities_acc": 0}
    for epoch in range(1, 1 + cfg.max_epoch):
        if epoch in cfg.lr_plan:
            adjust_lr(optimizer, cfg.lr_plan[epoch])
        if sampler is not None:
            sampler.set_epoch(epoch)
        info = train(training_loader, model, device, optimizer, epoch, cfg, buckets)
        if rank == 0:
            print_log(log_path, "Train epoch %d: loss %.5f activities acc %.2f%% actions acc %.2f%%"
                      % (epoch, info["loss"], info["activities_acc"], info["actions_acc"]))
            if "grad_norm_mean" in info:
                print_log(log_path, grad_stats_line(epoch, info))
        if epoch % cfg.test_interval_epoch == 0:
            tinfo = test(validation_loader, model, device, epoch, cfg)
            if tinfo["activities_acc"] > best_result["activities_acc"]:
                best_result = tinfo
            if rank == 0:
                print_log(log_path, "Test epoch %d: loss %.5f activities acc %.2f%% actions acc %.2f%%"
                          % (epoch, tinfo["loss"], tinfo["activities_acc"], tinfo["actions_acc"]))
                print_log(log_path, "Best group activity accuracy: %.2f%% at epoch #%d." % (best_result["activities_acc"], best_result["epoch"]))
                if tinfo["activities_acc"] == best_result["activities_acc"]:                 # :129-135
                    model.savemodel(cfg.result_path + "/stage%d_epoch%d_%.2f%%.pth" % (cfg.training_stage, epoch, tinfo["activities_acc"]))
            info = dict(train=info, test=tinfo)
        infos.append(info)
        if max_steps is not None and len(infos) >= max_steps:
            break
    return infos
