#!/usr/bin/env python3
"""Fill the box-feature cache files of a stage-2 configuration (cfg.feature_cache_path) with ONE forward-only pass over both splits:
the frozen backbone and RoIAlign, no model head, no optimizer.  Afterwards train.dinfc and val.dinfc exist before the first training
run, every stage-2 run with the same frames and backbone starts from them (din_amd/feature_cache_file.py: fingerprint), and a machine
that has the files never needs the JPEG tree again.

The pass takes the WHOLE window of frames around every clip (src - num_before .. src + num_after, what the DIN / AT / PCTDM datasets
select), also for a configuration of `arg_volleyball`, whose training items are three random frames of that window.  A frame id is an
index into the dataset's frame table, and the file records the table's digest: with the launchers' num_before = 5 and num_after = 4 the
window holds ARG's nine test offsets too and all four heads share one table; with a narrower window ARG's test table is larger, and an
ARG run refuses these files by naming `frames` instead of misreading them.

`build(cfg)` is the function (launch scripts call it with the very Config they train with); the command line covers the usual fields:

  python tools/build_feature_cache.py --out DIR --stage1 result/stage1.pth [--data-path data/volleyball] [--backbone vgg16|inv3]
         [--backbone-dtype fp32|bf16] [--cache-dtype fp32|bf16] [--cache-gb 64] [--image-size 720 1280] [--out-size 22 40]
         [--emb-features 512] [--set-bn-eval 0|1] [--batch 8] [--workers 4] [--flip]

--flip (cfg.feature_cache_flip): every frame is computed in both orientations in the same pass and train.flip.dinfc / val.flip.dinfc are
written next to the plain files, so that runs with flip_prob > 0 or test_flip start with both caches resident.  --cache-gb is per cache:
the pass holds twice as much.
"""
import argparse
import copy
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Trunk(torch.nn.Module):
    """what infer_model's cached-crops path needs of a model, and nothing else: .cfg, .backbone, .roi_align"""

    def __init__(self, cfg):
        from din_amd.infer_model import make_backbone
        from din_amd.roi_align.roi_align import RoIAlign
        super().__init__()
        self.cfg = cfg
        self.backbone = make_backbone(cfg)
        self.roi_align = RoIAlign(*cfg.crop_size)

    def loadmodel(self, filepath):
        self.backbone.load_state_dict(torch.load(filepath, map_location="cpu")["backbone_state_dict"])


def build(cfg, device=None, say=print) -> dict:
    """fill the files of `cfg` (feature_cache_gb > 0, feature_cache_path set, a real dataset tree at cfg.data_path); returns
    {split: frames in the file}.  Files that exist and match are taken in first, so only what they lack is computed."""
    from din_amd import feature_cache as FE, frame_cache as FC, infer_model as IM
    from din_amd.dataset import return_dataset
    why_not = FE.refusal(cfg) or FE.path_refusal(cfg) or FE.flip_cache_refusal(cfg)
    if why_not:
        raise ValueError(why_not)
    if getattr(cfg, "feature_cache_path", None) is None:
        raise ValueError("feature_cache_path is None: there is no directory to write the files to")
    device = torch.device(device or "cuda:0")
    dcfg = copy.copy(cfg)
    dcfg.inference_module_name, dcfg.training_stage = "dynamic_volleyball", 2       # the whole window of every clip, in both splits
    if getattr(cfg, "feature_cache_flip", False):                  # a mirror cache behind both loaders, whatever the run will ask for
        dcfg.flip_prob, dcfg.test_flip = (getattr(cfg, "flip_prob", 0.0) or 1.0), True
    training_set, validation_set = return_dataset(dcfg, frame_ids=True)
    loaders = FC.build_loaders(dcfg, training_set, validation_set, cfg.batch_size, None, device, True)
    trunk = Trunk(cfg)
    if cfg.load_backbone_stage2:
        trunk.loadmodel(cfg.stage1_model_path)
    trunk = trunk.to(device).eval()                                # (running-statistics BatchNorm: what set_bn_eval gives the trainer)
    for p in trunk.parameters():
        p.requires_grad = False
    done = {}
    for split, f in FE.cache_files(cfg, trunk, *loaders, 0, 1, say).items():
        f.load()
        before, t0 = f.inserted, time.perf_counter()
        table = f.loader.cache.table                               # (frames are counted in the plain cache: the pair rule keeps the mirror cache level with it)
        held = table.inserted
        feed = f.loader.feed(device)
        with torch.no_grad():
            for refs, boxes, *_ in feed:                           # (the feed marks `resident` for what this call stores)
                IM._cached_crops(trunk, refs, boxes, cfg.num_boxes)
        feed.check()
        say(f"{split}: {table.inserted - held} frames computed in {time.perf_counter() - t0:.1f} s, {table.inserted} resident")
        f.save_if_grown(before)
        done[split] = table.inserted
    return done


def main():
    from din_amd.config import Config
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", required=True, help="cfg.feature_cache_path: the directory of train.dinfc and val.dinfc")
    ap.add_argument("--stage1", default=None, help="the stage-1 checkpoint whose backbone the rows are computed with")
    ap.add_argument("--data-path", default=None)
    ap.add_argument("--backbone", default="vgg16", choices=("vgg16", "inv3"))
    ap.add_argument("--backbone-dtype", default="fp32")
    ap.add_argument("--cache-dtype", default="fp32", choices=("fp32", "bf16"))
    ap.add_argument("--cache-gb", type=float, default=64.0)
    ap.add_argument("--image-size", type=int, nargs=2, default=(720, 1280))
    ap.add_argument("--out-size", type=int, nargs=2, default=None)
    ap.add_argument("--emb-features", type=int, default=None)
    ap.add_argument("--set-bn-eval", type=int, choices=(0, 1), default=None, help="cfg.set_bn_eval (default: 1 for inv3, 0 for vgg16)")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--flip", action="store_true", help="cfg.feature_cache_flip: write the mirror caches' files (*.flip.dinfc) as well")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("build_feature_cache.py runs the backbone on the MI355X: no GPU here, nothing written")
    cfg = Config("volleyball")
    cfg.training_stage, cfg.train_backbone = 2, False
    cfg.set_bn_eval = bool(a.set_bn_eval) if a.set_bn_eval is not None else a.backbone == "inv3"
    cfg.backbone, cfg.backbone_dtype, cfg.image_size = a.backbone, a.backbone_dtype, tuple(a.image_size)
    cfg.out_size = tuple(a.out_size) if a.out_size else ((22, 40) if a.backbone == "vgg16" else (87, 157))
    cfg.emb_features = a.emb_features or (512 if a.backbone == "vgg16" else 1056)
    cfg.feature_cache_gb, cfg.feature_cache_dtype, cfg.feature_cache_path = a.cache_gb, a.cache_dtype, a.out
    cfg.batch_size, cfg.num_workers, cfg.feature_cache_flip = a.batch, a.workers, bool(a.flip)
    if a.data_path:
        cfg.data_path = a.data_path
    if a.stage1:
        cfg.load_backbone_stage2, cfg.stage1_model_path = True, a.stage1
    print(build(cfg))


if __name__ == "__main__":
    main()
