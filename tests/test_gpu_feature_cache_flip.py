"""Mirrored box features on the MI355X (cfg.feature_cache_flip, cfg.test_flip): the mirror cache against the frame path bit for bit, one
gather launch over both caches, the pair rule, the box check of mirrored rows, two models, two epochs of train_net_dynamic.train_net over
tests/golden/dataset_tree against the same run on the frame path, the files, the deterministic mode, and test-time flipping against a
hand computation from two model calls.

Geometry of tests/test_gpu_feature_cache.py: frozen VGG16, 96 x 160 images, out_size (3, 5), 12 boxes, T = 3, 64 box features."""
import os

import numpy as np
import pytest
import torch

from tests.conftest import Measured

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

pytestmark = pytest.mark.gpu

B, T, N, H, W, OW = 2, 3, 12, 96, 160, 5
ONE_MIRRORED = (False, True)                                     # clip 1 of the B = 2 batch is mirrored


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from din_amd import _lib
    _lib.load()
    return torch.device("cuda")


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t


class _World:
    """a frozen VGG16 model in eval(), one B = 2 batch of synthetic clips on the host, and what the frame path makes of it"""

    def __init__(self, gpu, name="dynamic_volleyball", backbone_dtype="fp32", frames=T):
        import copy
        from din_amd.train_net_dynamic import SyntheticVolleyball, build_model
        from tests.test_gpu_feature_cache import _model_cfg
        self.gpu, self.frames = gpu, frames
        self.cfg = cfg = _model_cfg(name)
        cfg.backbone_dtype = backbone_dtype
        torch.manual_seed(3)
        self.model = build_model(cfg).to(gpu).eval()
        dcfg = copy.copy(cfg)
        dcfg.num_frames = frames
        clips = [SyntheticVolleyball(dcfg, length=B, seed=4)[i] for i in range(B)]
        self.batch = tuple(torch.stack([c[k] for c in clips]) for k in range(4))      # images, boxes, actions, activities [B, frames]
        self.ids = np.arange(1000, 1000 + B * frames).reshape(B, frames)

    def frame_path(self, clip_flags):
        """frame_cache.FlippedFeed over the batch with these clips mirrored: (images uint8 [B, T, 3, H, W], boxes [B, T, N, 4],
        activities [B, T]) on the device -- the pixels, boxes and labels the frame path hands to the model"""
        from din_amd import frame_cache as FC
        flags = np.asarray(clip_flags, dtype=bool)

        class Fixed(FC.EpochFlips):
            def draw(self, num_clips):
                assert num_clips == len(flags)
                self.flipped += int(flags.sum())
                return flags

        augment = FC.PassAugment(Fixed(FC.FlipPlan(0.5, 0, 0, self.label_map(), float(self.cfg.out_size[1])), 1))
        (images, boxes, _actions, activities), = list(FC.FlippedFeed([self.batch], self.gpu, augment))
        return images, boxes, activities

    def label_map(self):
        from din_amd.volleyball import FLIP_ACTIVITIES
        return FLIP_ACTIVITIES

    def crops(self, images, boxes):
        """what fc_emb_1 receives on the frame path: fp32 [B * T, N * D * K * K]"""
        from din_amd import infer_model as IM
        F = images.shape[0] * images.shape[1]
        with torch.no_grad():
            return IM._crops(self.model, images.reshape(F, 3, H, W), boxes.reshape(F * N, 4), N)[0].reshape(F, -1)

    def caches(self, dtype=torch.float32, slots=None):
        from din_amd.feature_cache import FeatureCache, row_and_box_bytes
        rb, bb = row_and_box_bytes(self.cfg, dtype)
        capacity = 1 << 30 if slots is None else slots * (rb + bb) + 100
        return (FeatureCache(self.gpu, rb, bb, capacity, dtype=dtype), FeatureCache(self.gpu, rb, bb, capacity, dtype=dtype, orientation="mirrored"))

    def refs(self, caches, clip_flags, missing_clips, ids=None):
        """the FrameRefs of the batch with these clips mirrored and the frames of `missing_clips` decoded"""
        from din_amd.feature_cache import FrameRefs
        ids = self.ids if ids is None else ids
        Tn = self.frames
        pos = np.concatenate([np.arange(b * Tn, (b + 1) * Tn) for b in missing_clips]) if len(missing_clips) else np.zeros(0, dtype=np.int64)
        images = self.batch[0].reshape(B * Tn, 3, H, W)[torch.from_numpy(pos)].to(self.gpu)
        flipped = np.repeat(np.asarray(clip_flags, dtype=bool), Tn).reshape(B, Tn)
        return FrameRefs(ids, images, pos, caches[0], None, caches[1], flipped if flipped.any() else None, self.batch[1].to(self.gpu))


class _Counting:
    """counts the calls of ops.feat_rows / ops.feat_rows_bf16 and of the backbone (frames per call)"""

    def __init__(self, monkeypatch, model):
        from din_amd import ops
        self.gathers, self.trunks = [], []
        for name in ("feat_rows", "feat_rows_bf16"):
            monkeypatch.setattr(ops, name, self._counted(name, getattr(ops, name)))
        real_trunk = model.backbone.forward_nhwc
        monkeypatch.setattr(model.backbone, "forward_nhwc", lambda x: (self.trunks.append(int(x.shape[0])), real_trunk(x))[1])

    def _counted(self, name, real):
        def call(*a, **kw):
            self.gathers.append(name)
            return real(*a, **kw)
        return call


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_one_mirrored_clip_equals_the_frame_path_in_every_state_of_the_caches(gpu, monkeypatch, dtype):
    """a B = 2 batch with clip 1 mirrored: what `_cached_crops` hands to fc_emb_1 is, bit for bit, what the frame path's trunk gives for
    FlippedFeed's pixels and boxes -- with all six frames missing, with all resident (exactly ONE gather launch and no trunk call),
    and half resident: clip 0 in the caches since an earlier batch, clip 1 not, all six frames decoded (what a loader that decodes
    ahead of the step delivers), so clip 0's rows come from the slots and clip 1's from the trunk.  Every trunk call here is of six
    frames, like the frame path's: the forward planner cuts a conv's reduction by the launch's size (split-K), and a call of three
    frames was measured to give other last bits for the same frame.  With bf16 rows the comparison is of the bf16 operand
    fc_emb_1's GEMM multiplies."""
    from din_amd import infer_model as IM
    w = _World(gpu, backbone_dtype="bf16" if dtype == torch.bfloat16 else "fp32")
    images, boxes, _ = w.frame_path(ONE_MIRRORED)
    want = w.crops(images, boxes).to(dtype)
    count = _Counting(monkeypatch, w.model)
    gather = "feat_rows" if dtype == torch.float32 else "feat_rows_bf16"
    caches = w.caches(dtype)
    for state, missing, trunks in (("all missing", (0, 1), [6, 6]), ("all resident", (), [])):
        refs = w.refs(caches, ONE_MIRRORED, missing)
        del count.gathers[:], count.trunks[:]
        got = IM._cached_crops(w.model, refs, boxes, N)
        assert count.gathers == [gather] and count.trunks == trunks, (state, count.gathers, count.trunks)
        assert got.dtype == dtype and torch.equal(_bits(got), _bits(want)), f"{state}: feats differ from the frame path's"
        assert refs.inserted == (w.ids.reshape(-1).tolist() if missing else [])
    assert [c.inserted for c in caches] == [6, 6] and caches[0].hits + caches[1].hits == 6
    caches[0].check()
    half = w.caches(dtype)
    other = np.stack([w.ids[0], w.ids[1] + 1000])                    # an earlier batch: clip 0 next to frames under other names
    IM._cached_crops(w.model, w.refs(half, (False, False), (0, 1), ids=other), w.batch[1].to(gpu), N)
    assert [sorted(c.table.slot_of) for c in half] == [sorted(other.reshape(-1).tolist())] * 2
    refs = w.refs(half, ONE_MIRRORED, (0, 1))
    del count.gathers[:], count.trunks[:]
    got = IM._cached_crops(w.model, refs, boxes, N)
    assert count.gathers == [gather] and count.trunks == [6, 6] and refs.inserted == w.ids[1].tolist()
    assert [c.hits for c in half] == [3, 0] and [c.inserted for c in half] == [9, 9]
    bad = (_bits(got) != _bits(want)).any(dim=1).nonzero().reshape(-1).tolist()
    print(f"half resident, {dtype}: rows that differ from the frame path's {bad}, largest difference {float((got.float() - want.float()).abs().max())!r}")
    assert torch.equal(_bits(got), _bits(want)), "half resident: feats differ from the frame path's"
    half[0].check()
    # the mirror cache's trailers are the bits din_flip_clip_labels produced
    slab, off = half[1].table.locate(half[1].table.slot_of[int(w.ids[1, 0])])
    rb = half[1].row_bytes
    assert torch.equal(half[1].slabs[slab][off + rb:off + rb + 192].view(torch.float32), boxes[1, 0].reshape(-1))


def test_a_frame_asked_for_in_both_orientations_in_one_call(gpu, monkeypatch):
    """the test-time case: the batch twice in one call, as decoded and mirrored, all frames missing: each half equals the frame path's
    crops of that orientation, and every frame is inserted once per cache"""
    from din_amd import infer_model as IM
    from din_amd.feature_cache import FrameRefs
    w = _World(gpu)
    count = _Counting(monkeypatch, w.model)
    plain_images, plain_boxes, _ = w.frame_path((False, False))
    mirror_images, mirror_boxes, _ = w.frame_path((True, True))
    assert not torch.equal(mirror_images, plain_images) and not torch.equal(mirror_boxes, plain_boxes)
    want = torch.cat([w.crops(plain_images, plain_boxes), w.crops(mirror_images, mirror_boxes)])
    del count.trunks[:]
    caches = w.caches()
    refs = FrameRefs(np.concatenate([w.ids, w.ids]), plain_images.reshape(B * T, 3, H, W), np.arange(B * T), caches[0], None, caches[1],
                     np.repeat([False, False, True, True], T).reshape(2 * B, T), plain_boxes)
    got = IM._cached_crops(w.model, refs, torch.cat([plain_boxes, mirror_boxes]), N)
    assert torch.equal(got, want) and count.gathers == ["feat_rows"] and count.trunks == [6, 6]
    assert refs.inserted == w.ids.reshape(-1).tolist() and [c.inserted for c in caches] == [6, 6]
    again = FrameRefs(np.concatenate([w.ids, w.ids]), plain_images.reshape(B * T, 3, H, W)[:0], [], caches[0], None, caches[1], refs.flipped)
    assert torch.equal(IM._cached_crops(w.model, again, torch.cat([plain_boxes, mirror_boxes]), N), want)
    assert [c.inserted for c in caches] == [6, 6] and [c.hits for c in caches] == [6, 6] and count.trunks == [6, 6]
    caches[0].check()


def test_three_slots_per_cache_keep_pairs_and_serve_the_rest_from_computed_rows(gpu, monkeypatch):
    from din_amd import infer_model as IM
    w = _World(gpu)
    images, boxes, _ = w.frame_path(ONE_MIRRORED)
    want = w.crops(images, boxes)
    caches = w.caches(slots=3)
    refs = w.refs(caches, ONE_MIRRORED, (0, 1))
    assert torch.equal(IM._cached_crops(w.model, refs, boxes, N), want)
    kept = w.ids.reshape(-1)[:3].tolist()
    assert refs.inserted == kept and [sorted(c.table.slot_of) for c in caches] == [kept, kept] and all(c.table.full for c in caches)
    count = _Counting(monkeypatch, w.model)
    refs = w.refs(caches, ONE_MIRRORED, (0, 1))                      # clip 0 is served from the slots, clip 1 from the computed rows
    assert torch.equal(IM._cached_crops(w.model, refs, boxes, N), want) and refs.inserted == [] and count.trunks == [6, 6]
    assert [c.hits for c in caches] == [3, 0]
    assert [c.inserted for c in caches] == [3, 3]
    caches[0].check()


def test_a_mirrored_row_served_with_other_boxes_fails_the_check_at_the_end_of_the_pass(gpu):
    from din_amd import infer_model as IM
    w = _World(gpu)
    images, boxes, _ = w.frame_path(ONE_MIRRORED)
    want = w.crops(images, boxes)
    caches = w.caches()
    IM._cached_crops(w.model, w.refs(caches, ONE_MIRRORED, (0, 1)), boxes, N)
    caches[0].check()
    unmirrored = w.batch[1].to(gpu)                                  # the mirrored clip's rows asked for with the boxes as decoded
    got = IM._cached_crops(w.model, w.refs(caches, ONE_MIRRORED, ()), unmirrored, N)
    assert torch.equal(got, want)                                    # the rows are served all the same; the pass ends with the error
    with pytest.raises(RuntimeError) as e:
        caches[0].check()
    assert "3 rows" in str(e.value) and all(f"({r}, {int(w.ids.reshape(-1)[r])})" in str(e.value) for r in (3, 4, 5))
    IM._cached_crops(w.model, w.refs(caches, ONE_MIRRORED, ()), boxes, N)
    caches[0].check()


@pytest.mark.parametrize("name,frames", [("dynamic_volleyball", 3), ("arg_volleyball", 9)], ids=["dynamic", "arg_eval_fold"])
def test_models_score_a_mirrored_resident_clip_as_the_images_tensor(gpu, monkeypatch, name, frames):
    """the scores of a batch with clip 1 mirrored, through the images tensor FlippedFeed builds and through FrameRefs with every frame
    resident (no trunk call): equal.  ARG_volleyball reads the boxes and folds its nine evaluation frames into three sub-clips."""
    w = _World(gpu, name, frames=frames)
    images, boxes, _ = w.frame_path(ONE_MIRRORED)
    caches = w.caches()
    with torch.no_grad():
        want = w.model((images, boxes))["activities"]
        first = w.model((w.refs(caches, ONE_MIRRORED, (0, 1)), boxes))["activities"]
        count = _Counting(monkeypatch, w.model)
        got = w.model((w.refs(caches, ONE_MIRRORED, ()), boxes))["activities"]
    assert count.trunks == [] and count.gathers == ["feat_rows"]
    print("scores, images tensor | all missing | all resident:", want[1, :3].tolist(), first[1, :3].tolist(), got[1, :3].tolist())
    assert torch.equal(first, want) and torch.equal(got, want)
    caches[0].check()


# ---- end to end through the trainer ----------------------------------------------------------------------------------------------------
STEPS_PER_EPOCH = 3                                              # 2 training clips at batch size 1, then 1 validation clip


def _run(**settings):
    """two epochs of train_net over the volleyball tree of tests/golden/dataset_tree (tests/test_gpu_feature_cache.py's configuration)
    with `settings` on top.  Returns dict(infos, decodes and trunks as the number of model calls made before each (trunks with the frame
    count), caches, weights: the trained model's state_dict)."""
    from din_amd import feature_cache as FE, train_net_dynamic as TD, volleyball as V
    from din_amd.backbone.backbone import MyVGG16
    from din_amd.config import Config
    cfg = Config("volleyball")
    cfg.data_path, cfg.train_seqs, cfg.test_seqs = os.path.join(GOLDEN, "dataset_tree", "volleyball"), [1], [4]
    cfg.backbone, cfg.image_size, cfg.out_size, cfg.emb_features = "vgg16", (96, 160), (3, 5), 512
    cfg.num_boxes, cfg.num_frames, cfg.num_before, cfg.num_after = 12, 3, 1, 1
    cfg.num_features_boxes, cfg.num_features_gcn = 64, 64
    cfg.ST_kernel_size, cfg.sampling_ratio, cfg.beta_factor, cfg.train_backbone = [(3, 3)], [1], False, False
    cfg.training_stage, cfg.batch_size, cfg.test_batch_size, cfg.max_epoch, cfg.test_interval_epoch = 2, 1, 1, 2, 1
    cfg.train_dropout_prob, cfg.train_learning_rate, cfg.lr_plan, cfg.train_random_seed = 0.0, 1e-4, {}, 5
    cfg.result_path = None
    cfg.feature_cache_gb, cfg.frame_cache_gb, cfg.num_workers = 0, 0, 0
    for k, v in settings.items():
        setattr(cfg, k, v)
    decodes, trunks, caches, models, model_calls = [], [], [], [], [0]
    real = V.load_frame_u8, FE.FeatureCache.__init__, MyVGG16.forward_nhwc, TD.build_model

    def counting_load(path, size):
        decodes.append(model_calls[0])
        return real[0](path, size)

    def recording_init(self, *a, **kw):
        real[1](self, *a, **kw)
        caches.append(self)

    def counting_trunk(self, x):
        trunks.append((model_calls[0], int(x.shape[0])))
        return real[2](self, x)

    def recording_build(c):
        models.append(real[3](c))
        models[-1].register_forward_pre_hook(lambda m, a: model_calls.__setitem__(0, model_calls[0] + 1))
        return models[-1]

    V.load_frame_u8, FE.FeatureCache.__init__, MyVGG16.forward_nhwc, TD.build_model = counting_load, recording_init, counting_trunk, recording_build
    try:
        infos = TD.train_net(cfg)
        torch.cuda.synchronize()
    finally:
        V.load_frame_u8, FE.FeatureCache.__init__, MyVGG16.forward_nhwc, TD.build_model = real
    return dict(infos=infos, decodes=decodes, trunks=trunks, caches=caches, weights={k: v.detach().cpu() for k, v in models[0].state_dict().items()})


@pytest.mark.parametrize("flip_prob", [1.0, 0.5])
def test_train_net_serves_mirrored_clips_from_the_caches_from_the_second_epoch(gpu, flip_prob):
    """two epochs with flip_prob, the feature cache and feature_cache_flip against the same two epochs on the frame path (no cache):
    the same clips are mirrored (`flipped_clips`), the per-epoch losses agree at the bound tests/test_gpu_feature_cache.py holds a
    cached run to against an uncached one (1e-4 relative: the step's backward sums fp32 partials with atomics, so two runs of one step
    differ in the last bits), the first epoch runs the trunk twice per training step (once per orientation, three frames each) and
    once per validation step (the validation set has no mirror cache without test_flip), the second epoch decodes nothing and
    launches no trunk kernel."""
    frame = _run(flip_prob=flip_prob)
    cached = _run(flip_prob=flip_prob, feature_cache_gb=1, feature_cache_flip=True)
    assert not frame["caches"] and len(frame["decodes"]) == 2 * 9
    assert [c.orientation for c in cached["caches"]] == ["plain", "mirrored", "plain"]       # training pair, validation
    assert [c.inserted for c in cached["caches"]] == [6, 6, 3]
    assert len([c for c in cached["decodes"] if c < STEPS_PER_EPOCH]) == 9 and [c for c in cached["decodes"] if c >= STEPS_PER_EPOCH] == []
    assert cached["trunks"] == [(1, 3), (1, 3), (2, 3), (2, 3), (3, 3)], cached["trunks"]
    for i0, i1 in zip(frame["infos"], cached["infos"]):
        assert i1["train"]["flipped_clips"] == i0["train"]["flipped_clips"]
        assert "flipped_clips" not in i1["test"]
        for part in ("train", "test"):
            a, b = i1[part]["loss"], i0[part]["loss"]
            print(f"flip_prob {flip_prob} epoch {i0[part]['epoch']} {part}: frame path {b!r}, caches {a!r}, relative difference "
                  f"{abs(a - b) / max(1.0, abs(b)):.3e}, flipped {i0['train']['flipped_clips']}")
            assert Measured(abs(a - b)) <= 1e-4 * max(1.0, abs(b)), (part, a, b)
    if flip_prob == 1.0:
        assert [i["train"]["flipped_clips"] for i in cached["infos"]] == [2, 2]
        assert sum(c.hits for c in cached["caches"][:2]) == 6 and cached["caches"][0].hits == 0      # epoch 2: every row from the mirror cache


def test_a_second_run_starts_from_both_files(gpu, tmp_path):
    """with feature_cache_path the first run writes train.dinfc, train.flip.dinfc and val.dinfc; a second run decodes nothing and
    launches no trunk kernel from its first step, and reports what it loaded from both files"""
    settings = dict(flip_prob=0.5, feature_cache_gb=1, feature_cache_flip=True, feature_cache_path=str(tmp_path), max_epoch=1)
    first = _run(**settings)
    assert sorted(os.listdir(tmp_path)) == ["train.dinfc", "train.flip.dinfc", "val.dinfc"]
    t = first["infos"][0]["train"]
    assert (t["feature_cache_loaded"], t["feature_cache_saved"], t["feature_cache_flip_loaded"], t["feature_cache_flip_saved"]) == (0, 6, 0, 6)
    assert "feature_cache_flip_saved" not in first["infos"][0]["test"]
    second = _run(**settings)
    assert second["decodes"] == [] and second["trunks"] == []
    t = second["infos"][0]["train"]
    assert (t["feature_cache_loaded"], t["feature_cache_saved"], t["feature_cache_flip_loaded"], t["feature_cache_flip_saved"]) == (6, 0, 6, 0)
    assert t["flipped_clips"] == first["infos"][0]["train"]["flipped_clips"]
    # the mirror file offered as the plain one, and the reverse
    os.replace(tmp_path / "train.flip.dinfc", tmp_path / "swap")
    os.replace(tmp_path / "train.dinfc", tmp_path / "train.flip.dinfc")
    os.replace(tmp_path / "swap", tmp_path / "train.dinfc")
    with pytest.raises(ValueError, match="mirrored"):
        _run(**settings)


def test_deterministic_runs_with_mirrored_clips_give_bit_equal_weights(gpu):
    settings = dict(flip_prob=0.5, feature_cache_gb=1, feature_cache_flip=True, deterministic=True)
    a, b = _run(**settings), _run(**settings)
    assert a["weights"].keys() == b["weights"].keys() and len(a["weights"]) > 10
    differing = [k for k in a["weights"] if not torch.equal(a["weights"][k], b["weights"][k])]
    assert differing == [], differing
    assert [i["train"]["loss"] for i in a["infos"]] == [i["train"]["loss"] for i in b["infos"]]


# ---- test-time flipping ----------------------------------------------------------------------------------------------------------------
class _Dataset:
    def __init__(self, frames):
        self.resident = torch.zeros(frames, dtype=torch.uint8)


@pytest.mark.parametrize("name,cached", [("dynamic_volleyball", False), ("dynamic_volleyball", True), ("at_volleyball", True)],
                         ids=["dynamic_frames", "dynamic_caches", "at_caches"])
def test_test_flip_equals_a_hand_computation_from_two_model_calls(gpu, name, cached):
    """an evaluation pass with cfg.test_flip over one B = 2 batch (twice with the caches: filling them, then from them) against
    0.5 * (s + s_m[:, FLIP_ACTIVITIES]) built here from two model calls on the images tensor -- the pixels mirrored with torch.flip,
    the boxes with one fp32 subtraction per coordinate: the same loss, accuracy and confusion matrix, which counts each clip once"""
    import torch.nn.functional as F
    from din_amd import train_net_dynamic as TD
    from din_amd.feature_cache import FeatureLoader
    from din_amd.volleyball import FLIP_ACTIVITIES
    w = _World(gpu, name)
    cfg = w.cfg
    cfg.test_flip = True
    images, boxes, actions, activities = w.batch
    activities = activities.clone()
    activities[0], activities[1] = 1, 6                              # r_spike, l-pass: labels with a side, not mirrored by the pass
    d_images, d_boxes = images.to(gpu), boxes.to(gpu)
    m_boxes = torch.stack([OW - d_boxes[..., 2], d_boxes[..., 1], OW - d_boxes[..., 0], d_boxes[..., 3]], dim=-1)
    with torch.no_grad():
        s = w.model((d_images, d_boxes))["activities"]
        s_m = w.model((torch.flip(d_images, dims=[-1]).contiguous(), m_boxes))["activities"]
    want = 0.5 * (s.float() + s_m.float()[:, FLIP_ACTIVITIES])
    assert not torch.equal(want, s)
    target = activities[:, 0].to(gpu)
    loss = float(F.cross_entropy(want, target).double() * B) / B
    conf = np.zeros((cfg.num_activities, cfg.num_activities), dtype=np.float32)
    for t, p in zip(target.tolist(), want.argmax(1).tolist()):
        conf[t, p] += 1
    if cached:
        caches = w.caches()
        dataset = _Dataset(2000)
        host = (torch.from_numpy(w.ids), images.reshape(B * T, 3, H, W), torch.arange(B * T), boxes, actions, activities)
        passes = [FeatureLoader([host], caches[0], dataset, caches[1]),
                  FeatureLoader([(host[0], host[1][:0], host[2][:0]) + host[3:]], caches[0], dataset, caches[1])]
    else:
        passes = [[(images, boxes, actions, activities)]]
    for k, loader in enumerate(passes):
        info = TD._test_pass(loader, w.model, gpu, 1, cfg, False)
        print(f"pass {k}: loss {info['loss']!r}, by hand {loss!r}")
        assert info["loss"] == loss and info["activities_acc"] == float(np.trace(conf)) / B * 100
        assert np.array_equal(info["activities_conf"], conf) and info["activities_conf"].sum() == B
    if cached:
        assert [c.inserted for c in caches] == [6, 6] and [c.hits for c in caches] == [6, 12]
        assert dataset.resident[torch.from_numpy(w.ids.reshape(-1))].all() and int(dataset.resident.sum()) == 6


def test_train_net_with_test_flip_fills_and_reads_the_validation_mirror_cache(gpu):
    """two epochs with test_flip and the caches: the validation set has a mirror cache (the training set none: flip_prob is 0), its
    first pass runs the trunk once per orientation, its second pass decodes nothing and launches no trunk kernel"""
    run = _run(feature_cache_gb=1, feature_cache_flip=True, test_flip=True)
    assert [c.orientation for c in run["caches"]] == ["plain", "plain", "mirrored"]
    assert [c.inserted for c in run["caches"]] == [6, 3, 3] and [c.hits for c in run["caches"]] == [6, 3, 6]
    # a validation step is two model calls: the trunk runs in the first (both orientations), the second finds the frames resident
    assert run["trunks"] == [(1, 3), (2, 3), (3, 3), (3, 3)], run["trunks"]
    assert [c for c in run["decodes"] if c >= 4] == []
    assert all(i["test"]["activities_conf"].sum() == 1 for i in run["infos"])


# ---- a decoded subset of the batch, as the feed delivers it ---------------------------------------------------------------------------
def _slot_rows(cache, ids, dtype):
    """the rows the slots of `ids` hold, and their trailers as fp32"""
    rows, boxes = [], []
    for f in ids:
        slab, off = cache.table.locate(cache.table.slot_of[int(f)])
        rows.append(cache.slabs[slab][off:off + cache.row_bytes].view(dtype))
        boxes.append(cache.slabs[slab][off + cache.row_bytes:off + cache.row_bytes + cache.box_bytes].view(torch.float32))
    return torch.stack(rows), torch.stack(boxes)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_half_resident_batch_with_only_the_missing_clip_decoded(gpu, monkeypatch, dtype):
    """the steady state of a cache smaller than the dataset: clip 0 resident in both caches, clip 1 mirrored and the only one decoded
    (M = 3 of the B * T = 6 rows; miss_pos = 3, 4, 5, so the index of a computed row differs from its row of the batch, and the
    decoded frames sit in mirrored rows, so their unmirrored boxes come from `plain_boxes`).  One gather launch, the trunk over three
    frames per orientation; clip 1's rows equal, bit for bit, the frame path's trunk call over the same three mirrored frames with their
    mirrored boxes, clip 0's rows what the slots hold.  The orientation no row asked for went in with its own boxes: served
    afterwards, clip 1 as decoded equals the frame path's call over its three frames as decoded, and clip 0 mirrored the mirror
    cache's slots, with check() passing on the boxes of either orientation."""
    from din_amd import infer_model as IM
    from din_amd.feature_cache import FrameRefs
    w = _World(gpu, backbone_dtype="bf16" if dtype == torch.bfloat16 else "fp32")
    images, boxes, _ = w.frame_path(ONE_MIRRORED)                    # clip 0 as decoded, clip 1 mirrored
    images_other, boxes_other, _ = w.frame_path((True, False))       # clip 0 mirrored, clip 1 as decoded
    assert not torch.equal(boxes[1], boxes_other[1]) and torch.equal(boxes_other[1], w.batch[1][1].to(gpu))
    want_mirrored = w.crops(images[1:2], boxes[1:2]).to(dtype)       # the frame path over three frames: clip 1 mirrored ...
    want_plain = w.crops(images_other[1:2], boxes_other[1:2]).to(dtype)      # ... and as decoded
    caches = w.caches(dtype)
    first = FrameRefs(w.ids[:1], w.batch[0][0].to(gpu), np.arange(T), caches[0], None, caches[1])
    IM._cached_crops(w.model, first, w.batch[1][:1].to(gpu), N)
    assert first.inserted == w.ids[0].tolist() and [c.inserted for c in caches] == [3, 3]
    held = [_slot_rows(c, w.ids[0], dtype) for c in caches]
    assert torch.equal(held[0][1], boxes[0].reshape(T, -1)) and torch.equal(held[1][1], boxes_other[0].reshape(T, -1))
    count = _Counting(monkeypatch, w.model)
    gather = "feat_rows" if dtype == torch.float32 else "feat_rows_bf16"
    refs = w.refs(caches, ONE_MIRRORED, (1,))
    assert refs.miss_pos.tolist() == [3, 4, 5] and refs.miss_images.shape[0] == 3
    got = IM._cached_crops(w.model, refs, boxes, N)
    assert count.gathers == [gather] and count.trunks == [3, 3] and refs.inserted == w.ids[1].tolist()
    assert [c.inserted for c in caches] == [6, 6] and [c.hits for c in caches] == [3, 0]
    assert got.shape == (B * T, want_plain.shape[1]) and got.dtype == dtype
    assert torch.equal(_bits(got[T:]), _bits(want_mirrored)), "clip 1: the computed rows differ from the frame path's over the same three frames"
    assert torch.equal(_bits(got[:T]), _bits(held[0][0])), "clip 0: the rows differ from what the slots hold"
    stored = [_slot_rows(c, w.ids[1], dtype) for c in caches]        # both orientations of clip 1 went in, each with its own boxes
    assert torch.equal(_bits(stored[1][0]), _bits(want_mirrored)) and torch.equal(stored[1][1], boxes[1].reshape(T, -1))
    assert torch.equal(_bits(stored[0][0]), _bits(want_plain)) and torch.equal(stored[0][1], boxes_other[1].reshape(T, -1))
    del count.gathers[:], count.trunks[:]
    swapped = IM._cached_crops(w.model, w.refs(caches, (True, False), ()), boxes_other, N)
    assert count.gathers == [gather] and count.trunks == []
    assert torch.equal(_bits(swapped[T:]), _bits(want_plain)) and torch.equal(_bits(swapped[:T]), _bits(held[1][0]))
    caches[0].check()


def test_decoded_rows_scattered_over_both_orientations(gpu, monkeypatch):
    """M = 2 decoded frames at rows 1 and 5 of the batch (one in the clip as decoded, one in the mirrored clip), the other four
    resident: every row equals the frame path's call over those two frames in that orientation, or the slots"""
    from din_amd import infer_model as IM
    from din_amd.feature_cache import FrameRefs
    w = _World(gpu)
    images, boxes, _ = w.frame_path(ONE_MIRRORED)
    flat_i, flat_b = images.reshape(B * T, 3, H, W), boxes.reshape(B * T, N, 4)
    pos = np.asarray([1, 5])
    want = w.crops(flat_i[pos].reshape(1, 2, 3, H, W), flat_b[pos].reshape(1, 2, N, 4))      # row 1 as decoded, row 5 mirrored: two frames
    caches = w.caches()
    rest = np.asarray([0, 2, 3, 4])
    ids = w.ids.reshape(-1)
    filler = FrameRefs(ids[rest].reshape(1, 4), w.batch[0].reshape(B * T, 3, H, W)[rest].to(gpu), np.arange(4), caches[0], None, caches[1])
    IM._cached_crops(w.model, filler, w.batch[1].reshape(1, B * T, N, 4)[:, rest].to(gpu), N)
    held = (_slot_rows(caches[0], ids[[0, 2]], torch.float32)[0], _slot_rows(caches[1], ids[[3, 4]], torch.float32)[0])
    count = _Counting(monkeypatch, w.model)
    flipped = np.repeat(ONE_MIRRORED, T).reshape(B, T)
    refs = FrameRefs(w.ids, w.batch[0].reshape(B * T, 3, H, W)[pos].to(gpu), pos, caches[0], None, caches[1], flipped, w.batch[1].to(gpu))
    got = IM._cached_crops(w.model, refs, boxes, N)
    assert count.gathers == ["feat_rows"] and count.trunks == [2, 2] and refs.inserted == ids[pos].tolist()
    assert torch.equal(got[1], want[0]) and torch.equal(got[5], want[1])
    assert torch.equal(got[[0, 2]], held[0]) and torch.equal(got[[3, 4]], held[1])
    caches[0].check()
    # boxes that do not start on a multiple of 16 bytes are copied first: the rows are served and the box check still compares them
    shifted = torch.empty(boxes.numel() + 1, device=gpu)[1:].view_as(boxes)
    shifted.copy_(boxes)
    assert shifted.data_ptr() % 16 == 4
    again = FrameRefs(w.ids, refs.miss_images[:0], [], caches[0], None, caches[1], flipped)
    assert torch.equal(IM._cached_crops(w.model, again, shifted, N), got)
    caches[0].check()
    shifted[1, 0, 0, 0] += 0.5                                       # (and a changed box is seen through the copy)
    IM._cached_crops(w.model, again, shifted, N)
    with pytest.raises(RuntimeError, match="1 rows"):
        caches[0].check()


# ---- test-time flipping of the collective batch ----------------------------------------------------------------------------------------
def test_mirror_inputs_of_a_collective_batch_leave_the_padding_boxes_alone(gpu):
    """train_net_dynamic._Mirror.inputs with bboxes_num: pixels mirrored, the first bboxes_num boxes of every frame mirrored with one
    fp32 subtraction per coordinate, the padding boxes as they were, the counts handed on, no label map"""
    from din_amd.config import Config
    from din_amd.train_net_dynamic import _Mirror
    cfg = Config("collective")
    cfg.out_size = (3, 7)
    g = torch.Generator().manual_seed(2)
    images = torch.randint(0, 256, (2, 3, 3, 24, 40), dtype=torch.uint8, generator=g).to(gpu)
    boxes = (torch.rand((2, 3, 5, 4), generator=g) * 7).to(gpu)
    counts = torch.tensor([[2, 2, 2], [5, 5, 5]], dtype=torch.int32, device=gpu)
    mirror = _Mirror(cfg, gpu)
    assert mirror.label_map is None
    got_images, got_boxes, got_counts = mirror.inputs(images, boxes, counts)
    assert torch.equal(got_images, torch.flip(images, dims=[-1])) and got_counts is counts
    want = torch.stack([7 - boxes[..., 2], boxes[..., 1], 7 - boxes[..., 0], boxes[..., 3]], dim=-1)
    want[0, :, 2:] = boxes[0, :, 2:]
    assert torch.equal(got_boxes, want) and not torch.equal(got_boxes, boxes)


# ---- tools/build_feature_cache.py --flip -----------------------------------------------------------------------------------------------
def test_build_tool_with_flip_writes_four_files_a_run_starts_from(gpu, tmp_path):
    """build(cfg) with cfg.feature_cache_flip: both splits get a mirror file; the counts it returns and the plain files are those of a
    build without the setting; a run with flip_prob and test_flip from that folder decodes nothing and never calls the trunk"""
    import sys
    from din_amd import feature_cache_file as FF
    from tests.test_gpu_feature_cache_file import TRAIN_FRAMES, VAL_FRAMES, _cfg, _run as run_counted, _stage1
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import build_feature_cache as tool
    finally:
        sys.path.pop(0)
    stage1 = _stage1(str(tmp_path))
    both, plain = str(tmp_path / "both"), str(tmp_path / "plain")
    said = []
    cfg = _cfg(stage1, path=both)
    cfg.feature_cache_flip = True
    assert tool.build(cfg, say=said.append) == {"train": TRAIN_FRAMES, "val": VAL_FRAMES}
    assert any(line.startswith(f"train: {TRAIN_FRAMES} frames computed") and f"{TRAIN_FRAMES} resident" in line for line in said), said
    assert tool.build(_cfg(stage1, path=plain)) == {"train": TRAIN_FRAMES, "val": VAL_FRAMES}
    assert sorted(os.listdir(both)) == ["train.dinfc", "train.flip.dinfc", "val.dinfc", "val.flip.dinfc"]
    for name, frames in (("train", TRAIN_FRAMES), ("val", VAL_FRAMES)):
        assert open(os.path.join(both, name + ".dinfc"), "rb").read() == open(os.path.join(plain, name + ".dinfc"), "rb").read()
        header, ids, records = FF.read(os.path.join(both, name + ".flip.dinfc"))
        theirs, their_ids, their_records = FF.read(os.path.join(both, name + ".dinfc"))
        assert header["orientation"] == "mirrored" and header["count"] == frames and header["fingerprint"] == theirs["fingerprint"]
        assert sorted(ids.tolist()) == sorted(their_ids.tolist()) and not np.array_equal(np.asarray(records), np.asarray(their_records))
    cfg.feature_cache_gb = 0
    with pytest.raises(ValueError, match="feature_cache"):
        tool.build(cfg)
    cfg = _cfg(stage1, path=both, epochs=1)
    cfg.feature_cache_flip, cfg.flip_prob, cfg.test_flip = True, 0.5, True
    run = run_counted(cfg)
    assert (run["decodes"], run["trunks"], run["roi"]) == (0, 0, 0)
    info = run["infos"][0]
    for part, frames in (("train", TRAIN_FRAMES), ("test", VAL_FRAMES)):
        assert (info[part]["feature_cache_loaded"], info[part]["feature_cache_flip_loaded"]) == (frames, frames)
        assert (info[part]["feature_cache_saved"], info[part]["feature_cache_flip_saved"]) == (0, 0)
