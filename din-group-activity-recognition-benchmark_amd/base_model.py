"""Basenet_volleyball / Basenet_collective -- drop-in for the reference's base_model.py:6-142 and :145-284 (stage 1: the backbone and the
box embedding fine-tuned with a per-person action head and a per-frame group-activity head).

Same constructor (`Model(cfg)`), same `forward((images, boxes[, bboxes_num])) -> (actions_scores, activities_scores)` with the reference's
shapes, same attribute / state_dict names (backbone.*, fc_emb | fc_emb_1, fc_actions, fc_activities; dropout_emb | dropout_emb_1 hold p),
same `savemodel(path)` file ({'backbone_state_dict', 'fc_emb_state_dict', 'fc_actions_state_dict', 'fc_activities_state_dict'}), which
the stage-2 models' `loadmodel` reads (infer_model.py `_DynamicBase.loadmodel`).

The front end is the stage-2 one (backbone -> multi-scale RoIAlign -> fc_emb on the MFMA contraction kernel, bf16 operands under
backbone_dtype='bf16'); ReLU, dropout, both linear heads, the max over boxes and the T-mean run in ONE fused kernel per direction
(ops.BasenetHeadFunction, csrc/basenet_head.hip).  Images may be uint8.  Differences from the reference: backbones other than 'vgg16' /
'inv3' raise NotImplementedError (as the stage-2 models do); dropout masks come from the counter-hash of ops.mask_seed (the `_step`
counter), not from torch's RNG.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops
from .backbone.backbone import MyInception_v3
from .infer_model import embed_boxes, make_backbone
from .roi_align.roi_align import RoIAlign


class _Basenet(nn.Module):
    FC_EMB = "fc_emb"

    def _dropout_seed(self):
        self._step += 1
        return ops.mask_seed(int(getattr(self.cfg, "train_random_seed", 0)), self._step)

    def _heads(self, y, n_per_frame, T, mean_over_t):
        p = self.cfg.train_dropout_prob if self.training else 0.0
        seed = self._dropout_seed()
        N, NFB = y.shape[2], y.shape[3]
        return ops.BasenetHeadFunction.apply(y.reshape(-1, N, NFB), self.fc_actions.weight, self.fc_actions.bias, self.fc_activities.weight,
                                             self.fc_activities.bias, n_per_frame, T, mean_over_t, p, seed)

    def savemodel(self, filepath):
        """reference base_model.py:46-55 / :177-185"""
        state = {
            "backbone_state_dict": self.backbone.state_dict(),
            "fc_emb_state_dict": getattr(self, self.FC_EMB).state_dict(),
            "fc_actions_state_dict": self.fc_actions.state_dict(),
            "fc_activities_state_dict": self.fc_activities.state_dict(),
        }
        torch.save(state, filepath)
        print("model saved to:", filepath)


class Basenet_volleyball(_Basenet):
    """main module of the base model for the volleyball dataset (reference base_model.py:6-142)"""

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        NFB, D, K = cfg.num_features_boxes, cfg.emb_features, cfg.crop_size[0]
        self.backbone = make_backbone(cfg)                      # (never frozen here, as in the reference)
        self._step = 0                                          # dropout-mask counter (ops.mask_seed)
        self.roi_align = RoIAlign(*cfg.crop_size)
        self.fc_emb = nn.Linear(K * K * D, NFB)
        self.dropout_emb = nn.Dropout(p=cfg.train_dropout_prob)     # holder of p; the mask is fused in the head kernel
        self.fc_actions = nn.Linear(NFB, cfg.num_actions)
        self.fc_activities = nn.Linear(NFB, cfg.num_activities)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.kaiming_normal_(m.weight)
                nn.init.zeros_(m.bias)

    def loadmodel(self, filepath):
        state = torch.load(filepath, map_location="cpu")
        self.backbone.load_state_dict(state["backbone_state_dict"])
        self.fc_emb.load_state_dict(state["fc_emb_state_dict"])
        self.fc_actions.load_state_dict(state["fc_actions_state_dict"])
        self.fc_activities.load_state_dict(state["fc_activities_state_dict"])
        print("Load model states from: ", filepath)

    def forward(self, batch_data):
        images_in, boxes_in = batch_data[0], batch_data[1]
        T, N = images_in.shape[1], self.cfg.num_boxes
        y, _, _, _ = embed_boxes(self, images_in, boxes_in, N, self.fc_emb)         # [B,T,N,NFB]   (:77-114)
        # relu -> dropout -> fc_actions / max over boxes -> fc_activities (-> mean over T when T != 1)   (:117-139)
        return self._heads(y, None, T, T != 1)


class Basenet_collective(_Basenet):
    """main module of the base model for the Collective Activity dataset (reference base_model.py:145-284): always Inception-v3,
    per-frame box counts; actions compacted to [ALL_N, A] in (frame, box) order, activities per frame [B*T, A]."""

    FC_EMB = "fc_emb_1"

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        NFB, D, K = cfg.num_features_boxes, cfg.emb_features, cfg.crop_size[0]
        self.backbone = make_backbone(cfg, "inv3")              # base_model.py:158
        assert isinstance(self.backbone, MyInception_v3)
        if not cfg.train_backbone:
            for p in self.backbone.parameters():
                p.requires_grad = False
        self._step = 0
        self.roi_align = RoIAlign(*cfg.crop_size)
        self.fc_emb_1 = nn.Linear(K * K * D, NFB)
        self.dropout_emb_1 = nn.Dropout(p=cfg.train_dropout_prob)
        self.fc_actions = nn.Linear(NFB, cfg.num_actions)
        self.fc_activities = nn.Linear(NFB, cfg.num_activities)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.kaiming_normal_(m.weight)              # (biases keep nn.Linear's default init, as in the reference)

    def loadmodel(self, filepath):
        state = torch.load(filepath, map_location="cpu")
        self.backbone.load_state_dict(state["backbone_state_dict"])
        self.fc_emb_1.load_state_dict(state["fc_emb_state_dict"])
        print("Load model states from: ", filepath)

    def forward(self, batch_data):
        images_in, boxes_in, bboxes_num_in = batch_data
        B, T, MAX_N = images_in.shape[0], images_in.shape[1], self.cfg.num_boxes
        y, _, _, _ = embed_boxes(self, images_in, boxes_in, MAX_N, self.fc_emb_1)   # [B,T,MAX_N,NFB]   (:205-240)
        # per frame: the first bboxes_num[bt] boxes (:246-264) -- the counts stay on the device, the kernel compacts the action rows
        return self._heads(y, bboxes_num_in.reshape(B * T), T, False)
