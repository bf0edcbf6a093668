"""Embfeature_PositionEmbedding and Actor_Transformer -- the Actor-Transformer block, drop-in for the reference's
infer_module/AT_infer_module.py:52-144.

Same constructors (`Embfeature_PositionEmbedding(cfg, num_pos_feats=512, temperature=10000, normalize=False, scale=None)`,
`Actor_Transformer(in_dim, temporal_pooled_first, dropout=0.1)`), same parameter names and shapes (`Q_W`, `K_W`, `V_W` without bias,
`layernorm1`, `FFN_linear1`, `FFN_linear2`, `layernorm2`), so a reference AT checkpoint loads unchanged.  The reference's
`PositionEmbeddingSine` in that file is not used by any model and is not provided.

How it runs: Q_W, K_W and V_W read the same input, so they are ONE contraction X [rows, C] x [C, 3*C] on the MFMA kernel (ops.linear); scores,
row softmax, A V, dropout, the residual and layernorm1 are one launch of csrc/actor_attention.hip (ops.ActorAttentionFunction); the two FFN
Linear layers are ops.linear, ReLU + dropout and the second dropout ops.ActDropoutFunction, the last residual + layernorm2 ops.layer_norm.
The weights are concatenated per call with torch.cat, whose backward splits the gradient back into the three parameters.

Reproduced as in the reference: `FFN_dropout` is constructed and never called, `dropout2` is applied twice (:141, :143); all three have
p = `dropout` (0.1), not cfg.train_dropout_prob.

Deliberate differences from the reference:
  * the dropout masks are the counter hash of the other models here (`forward(x, seeds)`), not the host RNG stream;
  * with `temporal_pooled_first` the mean over T is taken by Embfeature_PositionEmbedding in the pass that adds the embedding (its extra
    keyword `pool_t`, which AT_volleyball sets); Actor_Transformer then receives [B, N, C] and refuses a 4-D input: there is one pooling
    path, not two.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from .. import ops


class Embfeature_PositionEmbedding(nn.Module):
    def __init__(self, cfg, num_pos_feats=512, temperature=10000, normalize=False, scale=None, pool_t=False):
        super().__init__()
        self.image_size = cfg.image_size
        self.out_size = cfg.out_size
        self.num_pos_feats = num_pos_feats
        self.temperature = temperature
        self.normalize = normalize
        if scale is not None and normalize is False:
            raise ValueError("normalize should be True if scale is passed")
        self.scale = 2 * math.pi if scale is None else scale           # (kept for parity; unused, as in the reference)
        self.pool_t = bool(pool_t)          # True: return the mean over T of the embedded features, [B, N, C]
        self._dim_t = None

    def dim_t(self, device):
        """temperature ** (2 * (i // 2) / num_pos_feats), formed in fp32 on the host as AT_infer_module.py:82-83 forms it"""
        if self._dim_t is None or self._dim_t.device != device:
            d = torch.arange(self.num_pos_feats, dtype=torch.float32)
            self._dim_t = (self.temperature ** (2 * (d // 2) / self.num_pos_feats)).to(device)
        return self._dim_t

    def forward(self, feature, boxes_in_flat):
        """feature [B, T, N, NFB], boxes_in_flat [B*T*N, 4] -> [B, T, N, NFB] (or [B, N, NFB] when `pool_t`)"""
        B, T, N, NFB = feature.shape
        assert self.num_pos_feats * 2 == NFB, (self.num_pos_feats, NFB)                                  # :76
        return ops.ActorPositionFunction.apply(feature, boxes_in_flat.reshape(B, T, N, 4), self.dim_t(feature.device), self.image_size,
                                               self.out_size, self.pool_t)


class Actor_Transformer(nn.Module):
    def __init__(self, in_dim, temporal_pooled_first, dropout=0.1):
        super().__init__()
        self.in_dim = in_dim
        self.temporal_pooled_first = temporal_pooled_first
        self.Q_W = nn.Linear(in_dim, in_dim, bias=False)
        self.K_W = nn.Linear(in_dim, in_dim, bias=False)
        self.V_W = nn.Linear(in_dim, in_dim, bias=False)
        self.layernorm1 = nn.LayerNorm([in_dim])
        self.dropout1 = nn.Dropout(dropout)                             # holders of p; the masks are formed in the kernels
        self.FFN_linear1 = nn.Linear(in_dim, in_dim, bias=True)
        self.FFN_relu = nn.ReLU(inplace=True)
        self.FFN_dropout = nn.Dropout(dropout)                          # constructed and never called, as in the reference (:113)
        self.FFN_linear2 = nn.Linear(in_dim, in_dim, bias=True)
        self.dropout2 = nn.Dropout(dropout)
        self.layernorm2 = nn.LayerNorm([in_dim])
        self.attention = None               # [G, N, N] of the last forward (detached), for inspection

    def forward(self, x, seeds=(0, 0, 0)):
        """x [B, T, N, NFB] -> [B*T, N, NFB]; with temporal_pooled_first x [B, N, NFB], already pooled over T -> [B, N, NFB].
        seeds: the mask seeds of dropout1, dropout2 (first use) and dropout2 (second use); only read in train mode."""
        if self.temporal_pooled_first:                                                                  # :125-126
            if x.dim() != 3:
                raise ValueError("Actor_Transformer with temporal_pooled_first takes the features already averaged over T, [B, N, NFB]: "
                                 "Embfeature_PositionEmbedding(..., pool_t=True) forms that mean in the pass that adds the embedding")
        else:
            B, T, N, NFB = x.shape
            x = x.reshape(B * T, N, NFB)                                                                # :128
        x = x.contiguous()
        weight = torch.cat([self.Q_W.weight, self.K_W.weight, self.V_W.weight], dim=0)                  # [3*C, C]
        proj = ops.linear(x, weight, None)                                                              # :130-132
        p1 = self.dropout1.p if self.training else 0.0
        p2 = self.dropout2.p if self.training else 0.0
        s1, s2, s3 = seeds
        x, att = ops.ActorAttentionFunction.apply(proj, x, self.layernorm1.weight, self.layernorm1.bias, p1, s1)   # :133-138
        self.attention = att.detach()
        f = ops.linear(x, self.FFN_linear1.weight, self.FFN_linear1.bias)                               # :139
        f = ops.ActDropoutFunction.apply(f, True, p2, s2)                                               # :140-141
        f = ops.linear(f, self.FFN_linear2.weight, self.FFN_linear2.bias)                               # :142
        f = ops.ActDropoutFunction.apply(f, False, p2, s3)                                              # :143 (dropout2 again)
        return ops.layer_norm(f, self.layernorm2.weight, self.layernorm2.bias, res=x)                   # :143

