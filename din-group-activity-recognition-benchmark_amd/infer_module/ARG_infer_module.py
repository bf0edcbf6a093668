"""GCN_Module -- the Actor Relation Graph block, drop-in for the reference's infer_module/ARG_infer_module.py:6-91.

Same constructor (`GCN_Module(cfg)`), same parameter names and shapes (`fc_rn_theta_list.{i}`, `fc_rn_phi_list.{i}` with bias,
`fc_gcn_list.{i}` without, `nl_gcn_list.{i}` of shape [T*N, NFG]), so a reference stage-2 ARG checkpoint loads unchanged, and the same
`forward(graph_boxes_features [B, T*N, NFG], boxes_in_flat [B*T*N, 4]) -> (features [B, T*N, NFG], relation_graph [B, T*N, T*N])`.

How it runs: the 3 * NG Linear layers all read the same input, so they are ONE contraction X [B*TN, NFG] x [NFG, NG*(2*NFR+NFG)] on the MFMA
kernel (ops.linear); since R_g (X W_g^T) == (R_g X) W_g^T the graph is applied after the projection, by ops.ArgGraphFunction
(csrc/arg_graph.hip: scores, position mask, softmax, R Y, LayerNorm over [T*N, NFG], ReLU, sum over graphs).  The weights are concatenated per
call with torch.cat, whose backward splits the gradient back into the 3 * NG parameters.

Deliberate differences from the reference:
  * the caller's boxes are NOT written.  The reference overwrites columns 0 / 1 of `boxes_in_flat` (a view of the caller's batch) with the
    box centres, in place, once per GCN layer (:48-49); layer l therefore masks on corners averaged l + 1 times.  The same VALUES are used here:
    set `centre_rounds` to the layer's index + 1 (ARG_volleyball does); the kernel forms them from the untouched boxes.
  * distances are formed as sqrt(dx^2 + dy^2), not as sqrt(rx - 2 xy + ry) (utils.py calc_pairwise_distance_3d), which can give the square root
    of a tiny negative on the diagonal; the diagonal is always kept here.  Entries within fp32 rounding of the threshold may differ.
  * `cfg.dataset_name == 'collective'` (LayerNorm([NFG]), only reached from GCNnet_collective) is not implemented.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import ops


class GCN_Module(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        if cfg.dataset_name != "volleyball":
            raise NotImplementedError("GCN_Module: the collective variant (LayerNorm([NFG]), reference ARG_infer_module.py:29) is only used by "
                                      "GCNnet_collective, which is outside the MI355X path")
        NFR, NG, NFG = cfg.num_features_relation, cfg.num_graph, cfg.num_features_gcn
        T, N = cfg.num_frames, cfg.num_boxes
        self.fc_rn_theta_list = nn.ModuleList([nn.Linear(NFG, NFR) for _ in range(NG)])                # :21
        self.fc_rn_phi_list = nn.ModuleList([nn.Linear(NFG, NFR) for _ in range(NG)])                  # :22
        self.fc_gcn_list = nn.ModuleList([nn.Linear(NFG, NFG, bias=False) for _ in range(NG)])         # :24
        self.nl_gcn_list = nn.ModuleList([nn.LayerNorm([T * N, NFG]) for _ in range(NG)])              # :27
        self.centre_rounds = 1              # this layer's index + 1 in a stack of GCN layers (see the module docstring)
        self.position_mask = None           # bool [B, T*N, T*N] of the last forward (True = masked), for inspection

    def forward(self, graph_boxes_features, boxes_in_flat):
        cfg = self.cfg
        B, TN, NFG = graph_boxes_features.shape
        NFR, NG = cfg.num_features_relation, cfg.num_graph
        assert NFG == cfg.num_features_gcn and TN == self.nl_gcn_list[0].weight.shape[0], (graph_boxes_features.shape, cfg.num_features_gcn)
        OW = cfg.out_size[1]
        weight = torch.cat([m.weight for m in self.fc_rn_theta_list] + [m.weight for m in self.fc_rn_phi_list]
                           + [m.weight for m in self.fc_gcn_list], dim=0)                               # [NG*(2*NFR+NFG), NFG]
        bias = torch.cat([m.bias for m in self.fc_rn_theta_list] + [m.bias for m in self.fc_rn_phi_list]
                         + [weight.new_zeros(NG * NFG)], dim=0)
        proj = ops.linear(graph_boxes_features, weight, bias)                                           # :59-60, :82 (the Linear half)
        gamma = torch.stack([m.weight for m in self.nl_gcn_list])                                       # [NG, TN, NFG]
        beta = torch.stack([m.bias for m in self.nl_gcn_list])
        out, rel, mask = ops.ArgGraphFunction.apply(proj, boxes_in_flat.reshape(B, TN, 4), gamma, beta, NG, NFR, NFG,
                                                    float(cfg.pos_threshold * OW), int(self.centre_rounds))   # :46-89
        self.position_mask = mask
        return out, rel[:, NG - 1]
