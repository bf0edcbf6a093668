"""PCTDM -- the participation-contributed temporal dynamic model block, drop-in for the reference's infer_module/pctdm_infer_module.py:9-133.

Same constructor (`PCTDM(cfg)`), the same fixed sizes (input 1024, hidden 1000, two teams) and the same state-dict keys, held by the same
torch modules so that a reference checkpoint loads unchanged: `Bi_Lstm.weight_ih_l0 ... bias_hh_l0_reverse`, `att_source_weights.0.*`,
`att_context_weights.0.*`, `att_extra_weights.0.*`, `Intra_Group_LSTM.*`.  Only the reference's default switches are built (interaction,
attention, one-to-all and early pooling all on): its other branches cannot run there either (`for g in self.num_groups` over an int,
float pool sizes).

How it runs.  forward: [B, T, N, 1024] -> [B*T, 2000].
  * W_ih of both Bi-LSTM directions is ONE [8000, 1024] contraction over all N positions (ops.linear, bias b_ih + b_hh); the recurrence is
    csrc/lstm.hip (ops.LSTMFunction), one launch per position;
  * max over the two direction halves of every player and the mean over the players: one launch of csrc/pctdm_attention.hip
    (ops.PctdmPoolFunction);
  * att_source_weights / att_context_weights: ops.linear; tanh, the att_extra_weights dot product, the softmax inside each team and
    x + x * gamma: one launch (ops.PctdmAttentionFunction);
  * the two teams share Intra_Group_LSTM, so they run as ONE LSTM call over 2*B*T rows of N/2 positions -- [G, N, H] reshaped to
    [2G, N/2, H] is already that layout; the last position's h of both teams of a frame is concatenated.
The concatenated weights, b_ih + b_hh and the stacked W_hh are formed per call with torch ops, whose backward splits the gradients back into
the parameters.

Deliberate differences from the reference:
  * the output is always 2-D: the reference's final torch.squeeze returns [2000] at B*T = 1;
  * `num_boxes` odd or < 4 raises ValueError: at one player per team the reference's squeeze makes the softmax run over the frames.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import ops


class PCTDM(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.input_size = 1024
        self.hidden_size = 1000
        self.num_players = cfg.num_boxes
        self.num_classes = cfg.num_activities
        self.num_groups = 2
        self.do_attention = True
        self.do_one_to_all = True
        self.do_early_pooling = True
        self.interaction = True
        if self.num_players < 4 or self.num_players % 2:
            raise ValueError(f"PCTDM splits the players into two teams of at least two: num_boxes = {self.num_players} is odd or below 4 "
                             f"(with one player per team the reference's squeeze turns the team softmax into one over the frames)")
        fea_size = self.hidden_size
        self.Bi_Lstm = nn.LSTM(self.input_size, self.hidden_size, num_layers=1, batch_first=True, bidirectional=True)
        self.att_source_weights = nn.Sequential(nn.Linear(fea_size, fea_size, bias=True))
        self.att_context_weights = nn.Sequential(nn.Linear(fea_size, fea_size, bias=True))
        self.att_extra_weights = nn.Sequential(nn.Linear(fea_size, 1, bias=True))
        self.Intra_Group_LSTM = nn.LSTM(fea_size, fea_size, num_layers=1, batch_first=True)
        self.probes = None                  # set to a dict to collect the intermediates of the next forward (detached), for inspection

    def forward(self, x):
        """x [B, T, N, 1024] -> [B*T, 2000]"""
        B, T, N, NFB = x.shape
        if N != self.num_players or NFB != self.input_size:
            raise ValueError(f"PCTDM takes [B, T, {self.num_players}, {self.input_size}], got {tuple(x.shape)}")
        G, H = B * T, self.hidden_size
        bi, ig = self.Bi_Lstm, self.Intra_Group_LSTM
        w_ih = torch.cat([bi.weight_ih_l0, bi.weight_ih_l0_reverse], dim=0)                               # [8H, 1024]
        b = torch.cat([bi.bias_ih_l0 + bi.bias_hh_l0, bi.bias_ih_l0_reverse + bi.bias_hh_l0_reverse], dim=0)
        w_hh = torch.stack([bi.weight_hh_l0, bi.weight_hh_l0_reverse], dim=0)                             # [2, 4H, H]
        pre = ops.linear(x.reshape(G, N, NFB), w_ih, b)                                                   # :83
        lstm_out = ops.LSTMFunction.apply(pre.reshape(G, N, 2, 4 * H), w_hh)                              # [G, N, 2H]
        pooled, context, winner = ops.PctdmPoolFunction.apply(lstm_out)                                   # :94-96, :106
        src = ops.linear(pooled, self.att_source_weights[0].weight, self.att_source_weights[0].bias)      # :58
        cx = ops.linear(context, self.att_context_weights[0].weight, self.att_context_weights[0].bias)
        y, gamma = ops.PctdmAttentionFunction.apply(pooled, src, cx, self.att_extra_weights[0].weight, self.att_extra_weights[0].bias)
        y2 = y.reshape(2 * G, N // 2, H)                                                                  # the two teams of a frame (:105)
        pre2 = ops.linear(y2, ig.weight_ih_l0, ig.bias_ih_l0 + ig.bias_hh_l0)                             # :114
        feas = ops.LSTMFunction.apply(pre2.reshape(2 * G, N // 2, 1, 4 * H), ig.weight_hh_l0.unsqueeze(0))
        out = feas[:, -1, :].reshape(G, 2 * H)                                                            # :115-116
        if self.probes is not None:
            self.probes.update(lstm_out=lstm_out.detach(), pooled=pooled.detach(), winner=winner, gamma=gamma.detach(),
                               group_feas=out.detach())
        return out
