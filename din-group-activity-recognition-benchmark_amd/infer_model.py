"""Dynamic_volleyball / Dynamic_collective -- drop-in for the reference's infer_model.py:15-234 and :1135-1319.

Same constructor (`Model(cfg)`), same `forward((images, boxes[, bboxes_num])) -> {'activities': [B, A]}`, same
`loadmodel(path)` and state_dict keys (backbone.*, fc_emb_1, nl_emb_1, point_conv, point_ln, DPI.*, dpi_nl,
fc_activities), so stage-1 / stage-2 checkpoints of the reference load unchanged.  Every arithmetic step runs in
hand-written gfx950 kernels behind the C ABI; see DESIGN.md for the kernel map.

Deliberate differences from the reference (all documented in DESIGN.md):
  * `cfg.backbone == 'inv3'` works (the reference has no head branch for it, infer_model.py:203-216 -> crash);
    it uses the vgg16 residual -> LN -> ReLU -> dropout order.
  * no torch.cuda.empty_cache() per step (infer_model.py:200 is a perf bug), images may be uint8.
  * new optional cfg field `backbone_dtype` ('fp32' parity mode | 'bf16' throughput mode | 'fp32_bf16x3'), default 'fp32'.
    'fp32_bf16x3': fp32 storage and fp32 accuracy, every conv / linear contraction of the trunk (backbone, fc_emb_1, point_conv) and of the
    DIN module (p_conv / scale_conv, hidden_weight) multiplied as three bf16 parts per operand on the bf16 matrix pipe
    (DIN_F32_BF16X3, include/din_hip.h); the baselines' own blocks and the TCE context transformer stay on exact fp32.
"""
from __future__ import annotations

import collections

import numpy as np
import torch
import torch.nn as nn

from . import ops
from .backbone.backbone import MyInception_v3, MyVGG16
from .feature_cache import FrameRefs, MapCache
from .infer_module.ARG_infer_module import GCN_Module
from .infer_module.AT_infer_module import Actor_Transformer, Embfeature_PositionEmbedding
from .infer_module.dynamic_infer_module import (Dynamic_Person_Inference, Hierarchical_Dynamic_Inference,
                                                Multi_Dynamic_Inference)
from .infer_module.pctdm_infer_module import PCTDM
from .infer_module.positional_encoding import Context_PositionEmbeddingSine
from .infer_module.TCE_STBiP_module import MultiHeadLayerEmbfeatureContextEncoding
from .roi_align.roi_align import RoIAlign
from .utils import print_log


def _as_kernel_list(k):
    if isinstance(k, (list,)) and len(k) and isinstance(k[0], (tuple, list)):
        return [tuple(x) for x in k]
    if isinstance(k, int):
        return [(k, k)]
    return [tuple(k)]


def make_backbone(cfg, name=None):
    """the backbone of cfg.backbone (or `name`), in cfg.backbone_dtype; shared by the stage-2 models and the stage-1 Basenets"""
    name = cfg.backbone if name is None else name
    dt = getattr(cfg, "backbone_dtype", "fp32")
    if name == "inv3":
        return MyInception_v3(transform_input=False, pretrained=True, compute_dtype=dt)
    if name == "vgg16":
        return MyVGG16(pretrained=True, compute_dtype=dt)
    raise NotImplementedError(f"backbone {name!r}: the MI355X hot path covers 'vgg16' and 'inv3' "
                              f"(BASELINE.json configs); vgg19/res18/alex are out of scope")


def embed_boxes(model, images_in, boxes_in, N, fc):
    """images [B,T,3,H,W] (uint8 | fp32), boxes [B,T,N,4] -> fc(RoIAlign(backbone(images))) [B,T,N,fc.out_features] (reference
    infer_model.py:152-184, base_model.py:77-114), plus (bufs, views, graph) of the backbone run.  `model` holds .cfg, .backbone and
    .roi_align.  No activation: the callers apply their own (LayerNorm + ReLU in stage 2, ReLU + dropout in the stage-1 head)."""
    cfg = model.cfg
    B, T = images_in.shape[0], images_in.shape[1]
    bdt = getattr(cfg, "backbone_dtype", "fp32")
    if isinstance(images_in, FrameRefs):
        feats = _cached_crops(model, images_in, boxes_in, N).reshape(B, T, N, -1)
        return ops.linear(feats, fc.weight, fc.bias, lowp=bdt == "bf16", split=bdt == "fp32_bf16x3"), None, None, None
    H, W = cfg.image_size
    crops, bufs, views, graph = _crops(model, images_in.reshape(B * T, 3, H, W), boxes_in.reshape(B * T * N, 4), N)
    feats = crops.reshape(B, T, N, -1)
    y = ops.linear(feats, fc.weight, fc.bias, lowp=bdt == "bf16", split=bdt == "fp32_bf16x3")                    # :184
    return y, bufs, views, graph


def _crops(model, images_flat, boxes_flat, N):
    """images [F,3,H,W], boxes [F*N,4] -> (RoIAlign(backbone(images)) fp32 [F*N, D, K, K], bufs, views, graph): infer_model.py:155-180"""
    cfg = model.cfg
    F = images_flat.shape[0]
    OH, OW = cfg.out_size
    D = cfg.emb_features
    boxes_idx = ops.boxes_frame_index(F, N, boxes_flat.device)                   # infer_model.py:155-157
    bufs, graph = model.backbone.forward_nhwc(images_flat)                       # prep fused (:161-162)
    fm = bufs[0]
    assert tuple(fm.shape[1:3]) == (OH, OW), f"backbone output {tuple(fm.shape[1:3])} != cfg.out_size {(OH, OW)}"   # (:164)
    views = model.backbone.output_views(graph)
    if fm.shape[3] >= D:                                                         # one map holds all D channels (VGG; materialised fuse)
        tid = graph.output_tids[0]
        crops = model.roi_align(fm, boxes_flat, boxes_idx, nhwc=True, channels=D,
                                relu_masked=graph.tensors[tid].relu_masked)      # [FN, D, K, K]  (:178-180)
    else:
        # multi-scale fuse + RoIAlign in one step (:165-180): every backbone output is sampled through its virtual align_corners
        # resize to (OH, OW); the resized / concatenated map is never built, forward or backward
        assert sum(c for _, _, c in views) == D, f"backbone outputs hold {sum(c for _, _, c in views)} channels, cfg.emb_features = {D}"
        maps = [(b, c, graph.tensors[tid].relu_masked) for b, (tid, _coff, c) in zip(bufs, views)]
        crops = model.roi_align.forward_multiscale(maps, boxes_flat, boxes_idx, (OH, OW))
    return crops, bufs, views, graph


def _cached_crops(model, refs, boxes_in, N):
    """the trunk behind the box-feature cache (feature_cache.py), or behind the cache and its mirror cache (`refs.mirror`,
    cfg.feature_cache_flip; the boxes are then mirrored in the rows `refs.flipped` names): the backbone and RoIAlign run, without
    autograd, on the M frames of `refs` that were decoded, once per orientation over M frames each (never once over 2M: a frame's
    features are then what a batch of M frames gives in either orientation) -- no launch when M == 0, nor with a mirror cache when both
    caches hold every decoded frame already (the second call of a test-time pair, a batch decoded ahead of the step that stored it).
    For the second orientation one din_copy_rows_u8_flip launch mirrors the pixels and one din_flip_clip_labels launch the unmirrored
    boxes.  One din_feat_rows launch builds fp32 [B*T, N*D*K*K] from those rows and the slots of either cache, stores the new rows
    with their boxes and checks the boxes of the rows served from slots (FeatureCache.rows / rows_both).  Caches of bf16 rows
    (cfg.feature_cache_dtype = 'bf16') return feats as bf16, ops.linear's lowp operand: one din_feat_rows_bf16 launch, no cast pass.
    A `refs.cache` that is a feature_cache.MapCache (cfg.map_cache_gb) keeps maps instead of crops: the branch below."""
    cfg = model.cfg
    if cfg.train_backbone:
        raise ValueError("cached box features (cfg.feature_cache_gb) are the output of a frozen backbone; this model trains its backbone")
    B, T = refs.shape[0], refs.shape[1]
    H, W = cfg.image_size
    D, K = cfg.emb_features, cfg.crop_size[0]
    boxes = boxes_in.reshape(B * T, N * 4)
    if boxes.dtype != torch.float32:
        boxes = boxes.float()
    mirror = getattr(refs, "mirror", None)
    ids, pos_h = refs.frame_ids.reshape(-1), refs.miss_pos
    if isinstance(refs.cache, MapCache):
        # cfg.map_cache_gb: the slots hold the backbone's map, not the crops.  The trunk runs once over exactly the M decoded frames, one
        # din_feat_rows launch builds fm [B*T, OH, OW, C] from those maps and the slots, and RoIAlign cuts this step's boxes out of it:
        # any number of boxes (Dynamic_collective), and fm is the context Dynamic_TCE_volleyball reads (`refs.context`).  No autograd
        # edge leads into fm.  What _crops reads off the graph comes from the cache, which recorded it with its first insert.
        computed, masked = None, False
        if len(pos_h):
            with torch.no_grad():
                bufs, graph = model.backbone.forward_nhwc(refs.miss_images.reshape(len(pos_h), 3, H, W).contiguous())
            if len(bufs) != 1 or bufs[0].shape[3] < D:
                raise ValueError(f"cached maps (cfg.map_cache_gb) need a backbone that ends in one map holding all {D} channels; this one "
                                 f"returned {[tuple(b.shape) for b in bufs]}")
            computed, masked = bufs[0], graph.tensors[graph.output_tids[0]].relu_masked
        fm, new_ids = refs.cache.maps(ids, pos_h, computed, masked)
        refs.inserted.extend(new_ids)
        refs.context = (fm, refs.cache.relu_masked)
        return model.roi_align(fm, boxes_in.reshape(B * T * N, 4), ops.boxes_frame_index(B * T, N, boxes_in.device), nhwc=True,
                               channels=D, relu_masked=refs.cache.relu_masked)
    flipped = None if mirror is None or refs.flipped is None else refs.flipped.reshape(-1)
    if mirror is not None and all(refs.cache.resident(ids[p]) and mirror.resident(ids[p]) for p in pos_h):
        pos_h = pos_h[:0]                            # nothing to compute (a cache without a mirror cache computes its M frames regardless)
    M = len(pos_h)
    computed = []                                  # per orientation: (its rows of the M decoded frames, the boxes they were computed for)
    if M:
        pos = refs.miss_pos_dev if refs.miss_pos_dev is not None else torch.from_numpy(np.ascontiguousarray(pos_h)).to(boxes.device)
        if flipped is not None and flipped[pos_h].any():
            if refs.plain_boxes is None:
                raise ValueError("a decoded frame sits in a mirrored row: FrameRefs.plain_boxes (the batch's boxes before mirroring) is needed")
            plain = refs.plain_boxes.reshape(B * T, N * 4).float().index_select(0, pos).contiguous()
        else:
            plain = boxes.index_select(0, pos).contiguous()
        oriented = [(refs.miss_images.reshape(M, 3, H, W).contiguous(), plain)]
        if mirror is not None:
            images = oriented[0][0]
            images_m, boxes_m = torch.empty_like(images), plain.clone()
            fb = 3 * H * W
            d_flags = refs.cache.gather_rows([images.data_ptr() + j * fb for j in range(M)], [images_m.data_ptr() + j * fb for j in range(M)],
                                             (3, H, W), flip_rows=np.ones(M, dtype=bool))
            ops.flip_clip_labels(boxes_m.view(M, N, 4), None, d_flags, None, None, float(cfg.out_size[1]))
            oriented.append((images_m, boxes_m))
        with torch.no_grad():
            computed = [(_crops(model, im, bx.reshape(M * N, 4), N)[0].reshape(M, N * D * K * K).contiguous(), bx) for im, bx in oriented]
    if mirror is None:
        feats, new_ids = refs.cache.rows(ids, boxes, pos_h, computed[0][0] if M else None)
    else:
        feats, new_ids = refs.cache.rows_both(mirror, ids, flipped, boxes, pos_h, [r for r, _ in computed], [bx for _, bx in computed])
    refs.inserted.extend(new_ids)
    return feats


class _DynamicBase(nn.Module):
    def _build_trunk(self, cfg):
        D, K, NFB = cfg.emb_features, cfg.crop_size[0], cfg.num_features_boxes
        self.backbone = make_backbone(cfg)
        if not cfg.train_backbone:
            for p in self.backbone.parameters():
                p.requires_grad = False
        self._step = 0                  # dropout-mask counter (ops.mask_seed); train_net saves / restores it with the checkpoint
        self.roi_align = RoIAlign(*cfg.crop_size)
        self.fc_emb_1 = nn.Linear(K * K * D, NFB)
        self.nl_emb_1 = nn.LayerNorm([NFB])

    def _init_linears(self):
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.kaiming_normal_(m.weight)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    def loadmodel(self, filepath):
        state = torch.load(filepath, map_location="cpu")
        self.backbone.load_state_dict(state["backbone_state_dict"])
        self.fc_emb_1.load_state_dict(state["fc_emb_state_dict"])
        print("Load model states from: ", filepath)

    def loadpart(self, pretrained_state_dict, model, prefix):
        """reference infer_model.py:358-368 (Dynamic_TCE_volleyball.loadpart): copy every entry of `pretrained_state_dict` whose key, with
        `prefix` removed, exists in `model` -- partial initialisation from another checkpoint"""
        num = 0
        model_state_dict = model.state_dict()
        picked = collections.OrderedDict()
        for k, v in pretrained_state_dict.items():
            if k.replace(prefix, "") in model_state_dict:
                picked[k.replace(prefix, "")] = v
                num += 1
        model_state_dict.update(picked)
        model.load_state_dict(model_state_dict)
        print(str(num) + " parameters loaded for " + prefix)

    # ---- shared front: images -> per-box embeddings [B,T,N,NFB] ------------------------------------------
    def _embed(self, images_in, boxes_in, N, return_context: bool = False):
        x, bufs, views, graph = embed_boxes(self, images_in, boxes_in, N, self.fc_emb_1)
        x = ops.layer_norm(x, self.nl_emb_1.weight, self.nl_emb_1.bias, relu=True)   # :185-186
        if return_context and bufs is None:                                          # a FrameRefs: the gathered maps of a map cache
            if images_in.context is None:
                raise ValueError("this model reads the backbone's map of every frame, which the box-feature cache does not keep "
                                 "(cfg.map_cache_gb does)")
            return (x, *images_in.context)
        if return_context:                                                           # the LAST backbone output, pixel-major (:404)
            tid_last, coff, c = views[-1]
            assert coff == 0 and bufs[-1].shape[3] == c
            return x, bufs[-1], graph.tensors[tid_last].relu_masked
        return x

    def _dropout_seed(self):
        self._step += 1
        return ops.mask_seed(int(getattr(self.cfg, "train_random_seed", 0)), self._step)


class Dynamic_volleyball(_DynamicBase):
    """main module of DIN for the volleyball dataset (reference infer_model.py:15-234)"""

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        T, N = cfg.num_frames, cfg.num_boxes
        NFB = cfg.num_features_boxes
        self._build_trunk(cfg)
        in_dim = cfg.lite_dim if cfg.lite_dim else NFB
        print_log(getattr(cfg, "log_path", None), ("Activate" if cfg.lite_dim else "Deactivate") + " lite model inference.")
        kernels = _as_kernel_list(cfg.ST_kernel_size)
        if not cfg.hierarchical_inference:
            self.DPI = Multi_Dynamic_Inference(in_dim=in_dim, person_mat_shape=(10, 12), stride=cfg.stride,
                                               kernel_size=kernels, dynamic_sampling=cfg.dynamic_sampling,
                                               sampling_ratio=cfg.sampling_ratio, group=cfg.group,
                                               scale_factor=cfg.scale_factor, beta_factor=cfg.beta_factor,
                                               parallel_inference=cfg.parallel_inference, num_DIM=cfg.num_DIM, cfg=cfg)
        else:
            self.DPI = Hierarchical_Dynamic_Inference(in_dim=in_dim, person_mat_shape=(T, N), stride=cfg.stride,
                                                      kernel_size=kernels, dynamic_sampling=cfg.dynamic_sampling,
                                                      sampling_ratio=cfg.sampling_ratio, group=cfg.group,
                                                      scale_factor=cfg.scale_factor, beta_factor=cfg.beta_factor,
                                                      parallel_inference=cfg.parallel_inference, cfg=cfg)
        print_log(getattr(cfg, "log_path", None), "Hierarchical Inference : " + str(cfg.hierarchical_inference))
        self.dpi_nl = nn.LayerNorm([T, N, in_dim])
        self.dropout_global = nn.Dropout(p=cfg.train_dropout_prob)      # holder of p; the mask is fused in the LN kernel
        if cfg.lite_dim:
            self.point_conv = nn.Conv2d(NFB, in_dim, kernel_size=1, stride=1)
            self.point_ln = nn.LayerNorm([T, N, in_dim])
            self.fc_activities = nn.Linear(in_dim, cfg.num_activities)
        else:
            self.fc_activities = nn.Linear(cfg.num_features_gcn, cfg.num_activities)
        self._init_linears()

    def forward(self, batch_data):
        images_in, boxes_in = batch_data
        cfg = self.cfg
        B, T, N = images_in.shape[0], images_in.shape[1], cfg.num_boxes
        x = self._embed(images_in, boxes_in, N)                                       # [B,T,N,NFB]
        if cfg.lite_dim:                                                              # :188-193
            x = ops.GridConvFunction.apply(x, self.point_conv.weight, self.point_conv.bias, 1, False,
                                           getattr(cfg, "backbone_dtype", "fp32") == "fp32_bf16x3")
            x = ops.layer_norm(x, self.point_ln.weight, self.point_ln.bias, relu=True)
        graph, _mad = self.DPI(x)                                                     # :199
        p = cfg.train_dropout_prob if self.training else 0.0
        head_mode = "res18" if cfg.backbone == "res18" else "vgg16"
        if head_mode == "vgg16":                                                      # :210-216 (also used for inv3)
            s = ops.layer_norm(graph, self.dpi_nl.weight, self.dpi_nl.bias, res=x, relu=True, drop_p=p,
                               seed=self._dropout_seed())
        else:                                                                         # :203-209
            raise NotImplementedError
        scores = ops.HeadFunction.apply(s, self.fc_activities.weight, self.fc_activities.bias, None)   # :224-232
        return {"activities": scores}


class Dynamic_TCE_volleyball(_DynamicBase):
    """DIN behind a context-encoding transformer (reference infer_model.py:237-468): every box embedding attends over
    the pixels of its frame's last backbone map (+ sine position embedding) with 4 heads of 128 features; [embedding | context
    encoding] (NFB + 512 channels) then goes through the same DIN modules and head as Dynamic_volleyball.

    As in the reference, only the vgg16 / res18 head branches exist (:430-442; 'inv3' leaves `boxes_states` unbound there) and this
    package has no res18 trunk, so cfg.backbone must be 'vgg16'; and lite_dim cannot be combined with it (the reference sizes
    fc_activities for lite_dim but feeds it lite_dim + 512 channels, :341-343 vs :410-456)."""

    NUM_HEADS_CONTEXT, NUM_FEATURES_CONTEXT = 4, 128                                   # :244-245

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        if cfg.backbone != "vgg16":
            raise NotImplementedError("Dynamic_TCE_volleyball: the reference's forward only handles the vgg16 / res18 trunks "
                                      "(infer_model.py:430-442) and its context transformer expects 512 context channels")
        if cfg.lite_dim:
            raise NotImplementedError("Dynamic_TCE_volleyball with lite_dim: the reference model cannot run (fc_activities is sized for "
                                      "lite_dim, its input has lite_dim + 512 channels)")
        T, N = cfg.num_frames, cfg.num_boxes
        NFB, K = cfg.num_features_boxes, cfg.crop_size[0]
        self._build_trunk(cfg)
        print_log(getattr(cfg, "log_path", None), "Deactivate lite model inference.")
        self.multilayer_head_embfeature_context_encoding = MultiHeadLayerEmbfeatureContextEncoding(
            self.NUM_HEADS_CONTEXT, 1, self.NUM_FEATURES_CONTEXT, NFB, K, N, context_dropout_ratio=0.1)       # :287-292
        self.context_positionembedding1 = Context_PositionEmbeddingSine(16, 512 / 2)                          # :293
        context_dim = NFB + self.NUM_HEADS_CONTEXT * self.NUM_FEATURES_CONTEXT                                # :296
        kernels = _as_kernel_list(cfg.ST_kernel_size)
        if not cfg.hierarchical_inference:
            self.DPI = Multi_Dynamic_Inference(in_dim=context_dim, person_mat_shape=(10, 12), stride=cfg.stride,
                                               kernel_size=kernels, dynamic_sampling=cfg.dynamic_sampling,
                                               sampling_ratio=cfg.sampling_ratio, group=cfg.group,
                                               scale_factor=cfg.scale_factor, beta_factor=cfg.beta_factor,
                                               parallel_inference=cfg.parallel_inference, num_DIM=cfg.num_DIM, cfg=cfg)
        else:
            self.DPI = Hierarchical_Dynamic_Inference(in_dim=context_dim, person_mat_shape=(T, N), stride=cfg.stride,
                                                      kernel_size=kernels, dynamic_sampling=cfg.dynamic_sampling,
                                                      sampling_ratio=cfg.sampling_ratio, group=cfg.group,
                                                      scale_factor=cfg.scale_factor, beta_factor=cfg.beta_factor,
                                                      parallel_inference=cfg.parallel_inference, cfg=cfg)
        print_log(getattr(cfg, "log_path", None), "Hierarchical Inference : " + str(cfg.hierarchical_inference))
        self.dpi_nl = nn.LayerNorm([T, N, context_dim])                                                       # :334
        self.dropout_global = nn.Dropout(p=cfg.train_dropout_prob)
        self.fc_activities = nn.Linear(context_dim, cfg.num_activities)                                       # :343
        self._init_linears()

    def forward(self, batch_data):
        images_in, boxes_in = batch_data
        cfg = self.cfg
        B, T, N = images_in.shape[0], images_in.shape[1], cfg.num_boxes
        x, context, masked = self._embed(images_in, boxes_in, N, return_context=True)       # [B,T,N,NFB], NHWC [BT,OH,OW,512]
        context = self.context_positionembedding1(context, nhwc=True, relu_masked=masked)    # :404-406 (fp32)
        enc = self.multilayer_head_embfeature_context_encoding
        enc.seed_base = int(getattr(cfg, "train_random_seed", 0)) + 101
        states = enc(x.reshape(B * T * N, -1), context, nhwc=True)                           # :408
        xc = torch.cat((x, states.reshape(B, T, N, -1)), dim=3)                              # :409-410
        graph, _mad = self.DPI(xc)                                                           # :414
        p = cfg.train_dropout_prob if self.training else 0.0
        s = ops.layer_norm(graph, self.dpi_nl.weight, self.dpi_nl.bias, res=xc, relu=True, drop_p=p,
                           seed=self._dropout_seed())                                        # vgg16 branch :436-442
        scores = ops.HeadFunction.apply(s, self.fc_activities.weight, self.fc_activities.bias, None)   # :452-466
        return {"activities": scores}


class Dynamic_collective(_DynamicBase):
    """DIN for the Collective Activity dataset (reference infer_model.py:1135-1319), variable actors per clip.

    The reference crashes here (tuple/tensor mismatch, SURVEY section 0 bug 3); this implements the intended dataflow:
    per clip b with N_b = bboxes_num[b,0] valid boxes: DIN on [1,T,N_b,C] -> +x -> LayerNorm([T,C]) per actor -> ReLU ->
    dropout -> max over actors -> fc -> mean over T -- as ONE launch set per batch: the DIN walk, and the head take the per-clip
    actor counts as a device array (`n_per_clip`), padding actors are zeroed once (din_mask_actors)."""

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        T, N = cfg.num_frames, cfg.num_boxes
        NFB = cfg.num_features_boxes
        self._build_trunk(cfg)
        in_dim = cfg.lite_dim if cfg.lite_dim else NFB
        k = _as_kernel_list(cfg.ST_kernel_size)[0]
        self.DPI = Dynamic_Person_Inference(in_dim=in_dim, person_mat_shape=(10, 12), stride=cfg.stride, kernel_size=k,
                                            dynamic_sampling=cfg.dynamic_sampling, sampling_ratio=cfg.sampling_ratio,
                                            group=cfg.group, scale_factor=cfg.scale_factor, beta_factor=cfg.beta_factor,
                                            parallel_inference=cfg.parallel_inference, cfg=cfg)
        self.dpi_nl = nn.LayerNorm([T, in_dim])
        self.dropout_global = nn.Dropout(p=cfg.train_dropout_prob)
        if cfg.lite_dim:
            self.point_conv = nn.Conv2d(NFB, in_dim, kernel_size=1, stride=1)
            self.point_ln = nn.LayerNorm([T, N, in_dim])
            self.fc_activities = nn.Linear(in_dim, cfg.num_activities)
        else:
            self.fc_activities = nn.Linear(cfg.num_features_gcn, cfg.num_activities)
        self._init_linears()

    def forward(self, batch_data):
        images_in, boxes_in, bboxes_num_in = batch_data
        cfg = self.cfg
        B, T, MAX_N = images_in.shape[0], images_in.shape[1], cfg.num_boxes
        x = self._embed(images_in, boxes_in, MAX_N)                                   # [B,T,MAX_N,NFB]
        if cfg.lite_dim:
            x = ops.GridConvFunction.apply(x, self.point_conv.weight, self.point_conv.bias, 1, False,
                                           getattr(cfg, "backbone_dtype", "fp32") == "fp32_bf16x3")
            x = ops.layer_norm(x, self.point_ln.weight, self.point_ln.bias, relu=True)
        # Variable actors per clip WITHOUT a host loop or a device->host read (the reference loops over clips and slices
        # boxes_features_all[b, :, :N], infer_model.py:1284-1316): the per-clip counts stay on the device and the kernels take them.
        n_per_clip = bboxes_num_in.reshape(B, T)[:, 0].to(torch.int32).clamp(1, MAX_N).contiguous()
        xm = ops.MaskActorsFunction.apply(x, n_per_clip)                              # padding actors -> 0 (== zero padding of the grid)
        g, _ = self.DPI(xm, n_per_clip)                                               # clip b: DIN on its T x n_b grid (:1291)
        p = cfg.train_dropout_prob if self.training else 0.0
        # (g + x) -> [B, N, T, C]: LayerNorm([T, C]) per actor (:1295-1297), ReLU, dropout fused; padding actors' rows are never read
        s = ops.AxpbyFunction.apply(g, xm, 1.0, 1.0).permute(0, 2, 1, 3).contiguous()
        s = ops.layer_norm(s, self.dpi_nl.weight, self.dpi_nl.bias, relu=True, drop_p=p, seed=self._dropout_seed())
        s = s.permute(0, 2, 1, 3).contiguous()                                        # [B, T, N, C]
        # max over the clip's n_b actors, fc, mean over T (:1306-1309)
        scores = ops.HeadFunction.apply(s, self.fc_activities.weight, self.fc_activities.bias, n_per_clip)
        return {"activities": scores}


class ARG_volleyball(_DynamicBase):
    """the Actor Relation Graph baseline for the volleyball dataset (reference infer_model.py:870-1023): the shared trunk, `gcn_layers`
    GCN_Module blocks over the T*N actors of a clip, `graph + x`, dropout, max over N, fc_activities, mean over T.  Same constructor,
    `forward((images, boxes)) -> {'activities': [B, A]}`, `loadmodel` and state_dict keys (backbone.*, fc_emb_1, nl_emb_1, gcn_list.*,
    fc_activities), so the reference's checkpoints load unchanged.

    In eval() a clip of 3*T frames is folded into three T-frame sub-clips -- flat frame order, consecutive thirds, as :939-947 -- whose
    scores are averaged (:1016-1019).

    Deliberate differences from the reference: the caller's `boxes` are left untouched (GCN_Module's docstring); the dropout mask is
    the counter hash of the other models here, not the host RNG stream; 'res18' / 'vgg19' / 'alex' are out of scope (make_backbone)."""

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        NFB, NFG = cfg.num_features_boxes, cfg.num_features_gcn
        assert NFG == NFB, (f"ARG_volleyball adds the graph features to the box embeddings (infer_model.py:995): num_features_gcn ({NFG}) "
                            f"must equal num_features_boxes ({NFB})")
        self._build_trunk(cfg)
        self.gcn_list = nn.ModuleList([GCN_Module(cfg) for _ in range(cfg.gcn_layers)])            # :909
        for i, m in enumerate(self.gcn_list):
            m.centre_rounds = i + 1
        self.dropout_global = nn.Dropout(p=cfg.train_dropout_prob)      # holder of p; the mask is formed by ops.ActDropoutFunction
        self.fc_activities = nn.Linear(NFG, cfg.num_activities)
        self._init_linears()

    def forward(self, batch_data):
        images_in, boxes_in = batch_data
        cfg = self.cfg
        B, T, N = images_in.shape[0], images_in.shape[1], cfg.num_boxes
        if not self.training:                                                             # :939-943
            if T % 3 != 0:
                raise ValueError(f"ARG_volleyball in eval() folds a clip into three sub-clips (reference infer_model.py:939-943): the clip "
                                 f"has {T} frames, not a multiple of 3")
            B, T = B * 3, T // 3
            images_in = images_in.reshape((B, T) + tuple(images_in.shape[2:]))
            boxes_in = boxes_in.reshape((B, T) + tuple(boxes_in.shape[2:]))
        x = self._embed(images_in, boxes_in, N)                                           # [B,T,N,NFB]  (:946-980)
        graph = x.reshape(B, T * N, -1)
        boxes_flat = boxes_in.reshape(B * T * N, 4)
        for gcn in self.gcn_list:                                                         # :986-987
            graph, _relation_graph = gcn(graph, boxes_flat)
        s = ops.AxpbyFunction.apply(graph.reshape(B, T, N, -1), x, 1.0, 1.0)              # :995
        p = cfg.train_dropout_prob if self.training else 0.0
        s = ops.ActDropoutFunction.apply(s, False, p, self._dropout_seed())               # :997
        scores = ops.HeadFunction.apply(s, self.fc_activities.weight, self.fc_activities.bias, None)   # :1006-1014
        if not self.training:                                                             # :1016-1019
            B = B // 3
            scores = ops.AxpbyFunction.apply(ops.AxpbyFunction.apply(scores.reshape(B, 3, -1)[:, 0], scores.reshape(B, 3, -1)[:, 1], 1.0, 1.0),
                                             scores.reshape(B, 3, -1)[:, 2], 1.0 / 3.0, 1.0 / 3.0)
        return {"activities": scores}


class AT_volleyball(_DynamicBase):
    """the Actor-Transformer baseline for the volleyball dataset (reference infer_model.py:736-867): the shared trunk, the box-centre sine
    embedding, one Actor_Transformer block over the N actors of every frame (of every clip, after the mean over T, with
    `cfg.temporal_pooled_first`), max over N, fc_activities, mean over T.  Same constructor, `forward((images, boxes)) -> {'activities':
    [B, A]}`, `loadmodel` and state_dict keys (backbone.*, fc_emb_1, nl_emb_1, AT.*, fc_activities, fc_actions), so the reference's
    checkpoints load unchanged.

    Deliberate differences from the reference: `fc_actions` is created, initialised and saved but has requires_grad False and is not
    evaluated -- the reference computes its scores and throws them away (:840-851), so it never receives a gradient there either and
    Adam skips it; here the optimiser and the all-reduce buckets (parallel.py) take only parameters that will receive one.  The three
    dropout masks are the counter hash of the other models here (three seeds per step from `_dropout_seed`), not the host RNG stream.
    No torch.cuda.empty_cache() per step (:836).  'res18' / 'vgg19' / 'alex' are out of scope (make_backbone)."""

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        NFB = cfg.num_features_boxes
        self._build_trunk(cfg)
        self.PE = Embfeature_PositionEmbedding(cfg=cfg, num_pos_feats=NFB // 2, pool_t=bool(cfg.temporal_pooled_first))   # :770
        self.AT = Actor_Transformer(in_dim=NFB, temporal_pooled_first=cfg.temporal_pooled_first)       # :771
        self.fc_activities = nn.Linear(NFB, cfg.num_activities)
        self.fc_actions = nn.Linear(NFB, cfg.num_actions)
        self._init_linears()
        self.fc_actions.requires_grad_(False)

    def forward(self, batch_data):
        images_in, boxes_in = batch_data
        cfg = self.cfg
        B, T, N = images_in.shape[0], images_in.shape[1], cfg.num_boxes
        x = self._embed(images_in, boxes_in, N)                                           # [B,T,N,NFB]  (:797-831)
        x = self.PE(x, boxes_in.reshape(B * T * N, 4))                                    # :834 (+ the mean over T of :125-126)
        states = self.AT(x, seeds=tuple(self._dropout_seed() for _ in range(3)))          # :835
        s = states.reshape(B, 1 if cfg.temporal_pooled_first else T, N, -1)
        scores = ops.HeadFunction.apply(s, self.fc_activities.weight, self.fc_activities.bias, None)   # :843-857
        return {"activities": scores}


class PCTDM_volleyball(_DynamicBase):
    """the PCTDM baseline for the volleyball dataset (reference infer_model.py:472-608): the shared trunk, the PCTDM block over the N players
    of every frame (a Bi-LSTM over the players, the direction max, intra-team attention, one LSTM over each team), LayerNorm([T, 2000]), ReLU,
    dropout, fc_activities per frame, mean over T.  Same constructor, `forward((images, boxes)) -> {'activities': [B, A]}`, `loadmodel` and
    state_dict keys (backbone.*, fc_emb_1, nl_emb_1, pctdm.*, pctdm_nl, fc_activities, fc_actions), so the reference's checkpoints load
    unchanged.  `loadmodel` loads the backbone only: the reference comments the embedding out (:522).

    PCTDM's sizes are fixed in the reference (Bi-LSTM input 1024, hidden 1000, LayerNorm([T, 2000]), Linear(2000, ...)), so
    cfg.num_features_boxes must be 1024 -- at any other width the reference's own forward fails -- and anything else is refused before a
    single module is built.

    Deliberate differences from the reference: `fc_actions` is created, initialised and saved but has requires_grad False and is never
    evaluated (the reference has its use commented out, :582-585), as in AT_volleyball.  The dropout mask is the counter hash of the other
    models here, not the host RNG stream.  No torch.cuda.empty_cache() per step (:574).  'res18' / 'vgg19' / 'alex' are out of scope
    (make_backbone)."""

    FEATURES = 2000                                                                        # two teams x hidden 1000

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        if cfg.num_features_boxes != 1024:
            raise NotImplementedError(f"pctdm_volleyball: PCTDM's Bi-LSTM input (1024) and pctdm_nl's 2000 columns are fixed in the reference; "
                                      f"num_features_boxes = {cfg.num_features_boxes} is not on the MI355X hot path")
        T = cfg.num_frames
        self._build_trunk(cfg)
        self.pctdm = PCTDM(cfg)                                                            # :505
        self.pctdm_nl = nn.LayerNorm([T, self.FEATURES])
        self.dropout_global = nn.Dropout(p=cfg.train_dropout_prob)      # holder of p; the mask is fused in the LN kernel
        self.fc_activities = nn.Linear(self.FEATURES, cfg.num_activities)
        self.fc_actions = nn.Linear(self.FEATURES, cfg.num_actions)
        self._init_linears()
        self.fc_actions.requires_grad_(False)

    def loadmodel(self, filepath):
        state = torch.load(filepath, map_location="cpu")
        self.backbone.load_state_dict(state["backbone_state_dict"])                        # (:521; the embedding is not loaded, :522)
        print("Load model states from: ", filepath)

    def forward(self, batch_data):
        images_in, boxes_in = batch_data
        cfg = self.cfg
        B, T, N = images_in.shape[0], images_in.shape[1], cfg.num_boxes
        x = self._embed(images_in, boxes_in, N)                                           # [B,T,N,1024]  (:526-570)
        states = self.pctdm(x).reshape(B, T, self.FEATURES)                               # :573-576
        p = cfg.train_dropout_prob if self.training else 0.0
        s = ops.layer_norm(states, self.pctdm_nl.weight, self.pctdm_nl.bias, relu=True, drop_p=p, seed=self._dropout_seed())   # :577-579
        # fc_activities per frame, mean over T (:589-592): the head kernel with one "actor" per frame, whose max is the identity
        scores = ops.HeadFunction.apply(s.reshape(B, T, 1, self.FEATURES), self.fc_activities.weight, self.fc_activities.bias, None)
        return {"activities": scores}
