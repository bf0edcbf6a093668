"""Config(dataset_name): attribute bag with the field names and defaults the DIN path reads from the reference's
config.py:10-104 (only the fields that exist on the hot path; dataset paths and the other methods' knobs are omitted).
Extra fields: backbone_dtype ('fp32' | 'bf16' | 'fp32_bf16x3': fp32 storage and fp32 accuracy with every trunk / DIN-module contraction
multiplied as three bf16 parts per operand on the bf16 matrix pipe -- DIN_F32_BF16X3, include/din_hip.h); hier_dropout_p (the reference hard-codes F.dropout's defaults -- p = 0.5, always on --
at dynamic_infer_module.py:495; 0.5 keeps that, 0.0 switches it off); frame_cache_gb (> 0: decoded uint8 frames of the real dataset tree
stay in HBM, up to that many GB per dataset, and batches are gathered from them -- din_amd/frame_cache.py; 0 = off) and num_workers (the
DataLoader worker processes of both trainers; the reference hard-codes 4, train_net_dynamic.py:40-48; 0 = decode in the main process);
feature_cache_gb (> 0, stage-2 trainer with a frozen backbone only: the fp32 RoIAlign output of every frame stays in HBM, up to that many
GB per dataset, and a step skips the backbone for resident frames -- din_amd/feature_cache.py; 0 = off); feature_cache_dtype ('fp32' |
'bf16', read only when feature_cache_gb > 0: what the slots hold.  'bf16' needs backbone_dtype = 'bf16', where the embedding GEMM
multiplies bf16 operands anyway: the row is stored already rounded, half the bytes per frame and no cast pass, the same numbers).
deterministic (stage-2 trainer, frozen backbone, one rank: the library's DIN_DETERMINISTIC option is set for the duration of train_net, so
every gradient on that path is summed in a fixed order and two runs with one seed give the same weights bit for bit -- ops.deterministic).
max_grad_norm (both trainers; None = off): the global L2 norm of the gradient is clipped to it inside the fused Adam step --
torch.nn.utils.clip_grad_norm_ semantics, what the reference tried and left commented out at train_net_dynamic.py:222-223 -- and a step
whose norm is not finite is skipped (din_amd/optim.py); float('inf') measures and guards without ever clipping; anything else is a
positive finite number.
flip_prob (both trainers, training passes only; 0.0 = off): every clip of a training batch is mirrored left-right with this probability --
all its frames inside the batch's gather launch, its boxes, and for volleyball the team side of its activity label
(din_amd/frame_cache.py: FlipPlan); refused together with feature_cache_gb > 0 unless feature_cache_flip is set.
color_jitter (both trainers, training passes only; None = off): the amplitudes (brightness, contrast, saturation) of a per-clip colour
jitter, each a real number in [0, 1).  Every clip of a training batch draws three factors f = 1 + a * u, u uniform in [-1, 1], and all its
frames go through PIL.ImageEnhance.Contrast, then .Brightness, then .Color with them -- byte for byte what Pillow computes -- inside the
batch's gather launch (din_amd/frame_cache.py: JitterPlan; include/din_hip.h); boxes and labels do not change, evaluation passes never
jitter; refused together with feature_cache_gb > 0.
feature_cache_path (stage-2 trainer, read only with feature_cache_gb > 0 and refused without it; None = off): a directory in which the
box-feature caches are kept between runs, one data file per cache (train.dinfc, val.dinfc; train.rank{r}of{w}.dinfc ... with several
ranks).  A run that finds a file written for the same frames, boxes geometry and backbone weights (din_amd/feature_cache_file.py:
fingerprint -- the head, the learning rate and the seed are not part of it) starts with those rows resident: it decodes nothing and
launches no backbone kernel from its first step; a cache that took frames in during an epoch is written after it.  A file of another
fingerprint is a ValueError naming the field, never overwritten.
feature_cache_flip (stage-2 trainer, with feature_cache_gb > 0 only and refused without it; False = off): a dataset's feature cache may be
accompanied by a mirror cache of the same geometry, dtype and capacity, whose row for a frame is the RoIAlign output of the mirrored frame
for the mirrored boxes -- the training set gets one iff flip_prob > 0, the validation set iff test_flip.  flip_prob is then served from the
cache: a decoded frame is computed in both orientations in the step that decodes it, a batch of resident frames is one gather launch over
both caches for any mix of orientations, and the mirror cache's file stands next to the plain one (train.flip.dinfc) under
feature_cache_path.  Twice the memory: 61 GB per orientation for the 48300 volleyball frames as fp32 Inception-v3 rows.
test_flip (stage-2 trainer, evaluation passes; False = off; refused by the stage-1 trainer): every clip is scored as decoded and mirrored
and the scores are averaged, 0.5 * (s + s_m[:, volleyball.FLIP_ACTIVITIES]) in fp32 (the identity map for collective); with
feature_cache_gb > 0 the mirrored clips come from the mirror cache, so feature_cache_flip must be set.
map_cache_gb (stage-2 trainer, frozen VGG16 backbone, either dataset, every stage-2 model; 0 = off; ignored by the stage-1 trainer): the
frozen backbone's output map of every frame stays in HBM, up to that many GB per dataset, in the dtype the backbone emits (22 x 40 x 512
fp32 = 1 802 240 bytes a volleyball frame, 87 GB for the 48300 frames, half as bf16; 675 840 bytes a collective frame).  A step runs the
trunk over its decoded frames only, gathers the maps of the others from their slots in the same one launch, and runs RoIAlign on the
step's own boxes -- so it serves what feature_cache_gb refuses: dynamic_tce_volleyball, which reads the map itself, and collective's
per-clip actor counts.  For the other models the feature cache is the smaller choice.  Refused with train_backbone, with another cache
(frame_cache_gb, feature_cache_gb), with backbone 'inv3' (two maps, 13 MB a frame), and with flip_prob, color_jitter or test_flip
(din_amd/feature_cache.py: MapCache, map_refusal).
All are opt-in: at 0 / False / None the trainers behave exactly as without them."""
from __future__ import annotations

import os
import time

_DEFAULTS = dict(
    image_size=(720, 1280), batch_size=32, test_batch_size=8, num_boxes=12,
    use_gpu=True, use_multi_gpu=True, device_list="0,1,2,3",
    backbone="res18", crop_size=(5, 5), train_backbone=False, out_size=(87, 157), emb_features=1056,
    num_actions=9, num_activities=8, actions_loss_weight=1.0, actions_weights=None,
    num_frames=3, num_before=5, num_after=4,
    num_features_boxes=1024, num_features_relation=256, num_graph=16, num_features_gcn=1024, gcn_layers=1, pos_threshold=0.2,
    train_random_seed=0, train_learning_rate=1e-4, lr_plan={11: 3e-5, 21: 1e-5}, train_dropout_prob=0.3, weight_decay=0,
    max_epoch=30, test_interval_epoch=1,
    training_stage=1, stage1_model_path="", test_before_train=False, exp_note="Group-Activity-Recognition", exp_name=None,
    set_bn_eval=False, inference_module_name="dynamic_volleyball",
    stride=1, ST_kernel_size=3, dynamic_sampling=True, sampling_ratio=[1, 3], group=1, scale_factor=True, beta_factor=True,
    load_backbone_stage2=False, parallel_inference=False, hierarchical_inference=False, lite_dim=None, num_DIM=1,
    load_stage2model=False, stage2model=None, temporal_pooled_first=False,
    backbone_dtype="fp32", hier_dropout_p=0.5,
    frame_cache_gb=0, num_workers=0, feature_cache_gb=0, feature_cache_dtype="fp32",
    deterministic=False,
    max_grad_norm=None,
    flip_prob=0.0,
    color_jitter=None,
    feature_cache_path=None,
    feature_cache_flip=False, test_flip=False,
    map_cache_gb=0,
)


class Config(object):
    def __init__(self, dataset_name):
        assert dataset_name in ("volleyball", "collective")
        self.dataset_name = dataset_name
        for k, v in _DEFAULTS.items():
            setattr(self, k, list(v) if isinstance(v, list) else (dict(v) if isinstance(v, dict) else v))
        self.log_path = None
        # dataset trees (reference config.py:24-33): used when the directory exists, else the trainer falls back to synthetic clips
        if dataset_name == "volleyball":
            self.data_path = "data/volleyball/videos"
            self.test_seqs = [4, 5, 9, 11, 14, 20, 21, 25, 29, 34, 35, 37, 43, 44, 45, 47]
            self.train_seqs = [1, 3, 6, 7, 10, 13, 15, 16, 18, 22, 23, 31, 32, 36, 38, 39, 40, 41, 42, 48, 50, 52, 53, 54,
                               0, 2, 8, 12, 17, 19, 24, 26, 27, 28, 30, 33, 46, 49, 51]      # (the reference's order: it fixes the sample order)
        else:
            self.data_path = "data/collective"
            self.test_seqs = [5, 6, 7, 8, 9, 10, 11, 15, 16, 25, 28, 29]
            self.train_seqs = [s for s in range(1, 45) if s not in self.test_seqs]

    def init_config(self, need_new_folder=True):
        if self.exp_name is None:
            stamp = time.strftime("%Y-%m-%d_%H-%M-%S", time.localtime())
            self.exp_name = "[%s_stage%d]<%s>" % (self.exp_note, self.training_stage, stamp)
        self.result_path = "result/%s" % self.exp_name
        self.log_path = "result/%s/log.txt" % self.exp_name
        if need_new_folder:
            os.makedirs(self.result_path, exist_ok=True)
