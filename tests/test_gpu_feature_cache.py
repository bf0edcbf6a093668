"""Box-feature cache on the MI355X: din_feat_rows against a numpy model (bit-exact, every row kind, guard bands), the FeatureCache round
trip, the trunk skipped inside Dynamic_volleyball / ARG_volleyball, and two epochs of train_net_dynamic.train_net over
tests/golden/dataset_tree with cfg.feature_cache_gb = 1 against the same run with 0."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.conftest import Measured

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

pytestmark = pytest.mark.gpu

GUARD, GUARD_BYTE = 64, 0xA5
# row i is of kind i % 9: with n = 9 every kind occurs once
SKIP, COPY, KEEP, CHECK_EQ, CHECK_FIRST, CHECK_LAST, SHARED_A, SHARED_B, CHECK_EQ_PRESET = range(9)


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from din_amd import _lib
    _lib.load()
    return torch.device("cuda")


class _Case:
    """n rows of every kind, all buffers between guard bands, and the numpy model of what one din_feat_rows launch leaves in them.
    Buffers (host image `*_h`, device tensor `*_d`): dst (n rows), slot (n slots of row_bytes + box_bytes; only KEEP / SHARED_B rows
    name theirs), stored (n rows of box_bytes: the boxes a CHECK row is compared with), flags (n bytes)."""

    def __init__(self, gpu, n, row_bytes, box_bytes, seed):
        rng = np.random.default_rng(seed)
        self.n, self.rb, self.bb = n, row_bytes, box_bytes
        kinds = [i % 9 for i in range(n)]
        self.src_h = rng.integers(0, 256, size=(n, row_bytes), dtype=np.uint8)
        self.boxes_h = rng.integers(0, 256, size=(n, box_bytes), dtype=np.uint8)
        self.dstride, self.sstride, self.bstride = row_bytes + 2 * GUARD, row_bytes + box_bytes + 2 * GUARD, box_bytes + 2 * GUARD
        self.dst_h = np.full(n * self.dstride, GUARD_BYTE, dtype=np.uint8)
        self.slot_h = np.full(n * self.sstride, GUARD_BYTE, dtype=np.uint8)
        self.stored_h = np.full(n * self.bstride, GUARD_BYTE, dtype=np.uint8)
        self.flags_h = np.full(n + 2 * GUARD, GUARD_BYTE, dtype=np.uint8)
        self.flags_h[GUARD:GUARD + n] = 0                            # the host clears the flags at the start of a pass
        for i, k in enumerate(kinds):
            self.dst_h[i * self.dstride + GUARD:i * self.dstride + GUARD + row_bytes] = 0x3C
            self.slot_h[i * self.sstride + GUARD:i * self.sstride + GUARD + row_bytes + box_bytes] = 0x5A
            st = self.boxes_h[i].copy()
            if k == CHECK_FIRST:
                st[3] ^= 0x80                                        # one bit of the first float (its sign)
            elif k == CHECK_LAST:
                st[box_bytes - 4] ^= 0x01                            # the lowest bit of the last float
            self.stored_h[i * self.bstride + GUARD:i * self.bstride + GUARD + box_bytes] = st
            if k == SKIP:
                self.flags_h[GUARD + i] = 0x77                       # must come back untouched
            elif k == CHECK_EQ_PRESET:
                self.flags_h[GUARD + i] = 1                          # the kernel never writes 0
        dev = lambda a: torch.from_numpy(a).to(gpu)
        self.src_d, self.boxes_d = dev(self.src_h), dev(self.boxes_h)
        self.dst_d, self.slot_d, self.stored_d, self.flags_d = dev(self.dst_h), dev(self.slot_h), dev(self.stored_h), dev(self.flags_h)
        src, dst, keep, ref = [], [], [], []
        self.want_dst, self.want_slot, self.want_flags = self.dst_h.copy(), self.slot_h.copy(), self.flags_h.copy()
        for i, k in enumerate(kinds):
            s = i - 1 if k == SHARED_B else i                        # SHARED_B reads the row SHARED_A reads
            src.append(0 if k == SKIP else self.src_d.data_ptr() + s * row_bytes)
            dst.append(self.dst_d.data_ptr() + i * self.dstride + GUARD)
            keep.append(self.slot_d.data_ptr() + i * self.sstride + GUARD if k in (KEEP, SHARED_B) else 0)
            ref.append(self.stored_d.data_ptr() + i * self.bstride + GUARD if k in (CHECK_EQ, CHECK_FIRST, CHECK_LAST, CHECK_EQ_PRESET) else 0)
            if k == SKIP:
                continue
            self.want_dst[i * self.dstride + GUARD:i * self.dstride + GUARD + row_bytes] = self.src_h[s]
            if keep[-1]:
                at = i * self.sstride + GUARD
                self.want_slot[at:at + row_bytes] = self.src_h[s]
                self.want_slot[at + row_bytes:at + row_bytes + box_bytes] = self.boxes_h[i]
            if k in (CHECK_FIRST, CHECK_LAST):
                self.want_flags[GUARD + i] = 1
        assert all(a % 16 == 0 for a in src + dst + keep + ref) and self.boxes_d.data_ptr() % 16 == 0
        tab = lambda v: torch.tensor(v, dtype=torch.int64, device=gpu)
        self.src_t, self.dst_t, self.keep_t, self.ref_t = tab(src), tab(dst), tab(keep), tab(ref)
        self.flags_view = self.flags_d[GUARD:GUARD + n]

    def launch(self):
        from din_amd import ops
        ops.feat_rows(self.src_t, self.dst_t, self.rb, self.keep_t, self.ref_t, self.boxes_d, self.flags_view, self.bb)

    def reset(self):
        for d, h in ((self.dst_d, self.dst_h), (self.slot_d, self.slot_h), (self.flags_d, self.flags_h)):
            d.copy_(torch.from_numpy(h))

    def verify(self, what=""):
        torch.cuda.synchronize()
        for name, got, want in (("dst", self.dst_d, self.want_dst), ("slot", self.slot_d, self.want_slot),
                                ("flags", self.flags_d, self.want_flags), ("stored boxes", self.stored_d, self.stored_h),
                                ("src", self.src_d, self.src_h.reshape(-1)), ("boxes", self.boxes_d, self.boxes_h.reshape(-1))):
            bad = np.flatnonzero(got.cpu().numpy().reshape(-1) != want.reshape(-1))
            assert bad.size == 0, f"{what} row_bytes={self.rb} box_bytes={self.bb} n={self.n}: {name}: {bad.size} bytes differ, first at {bad[:4]}"

    def verify_untouched(self, what):
        torch.cuda.synchronize()
        for name, got, want in (("dst", self.dst_d, self.dst_h), ("slot", self.slot_d, self.slot_h), ("flags", self.flags_d, self.flags_h)):
            assert np.array_equal(got.cpu().numpy(), want), f"{what}: wrote to {name}"


def _row_sizes():
    from din_amd import ops
    seg = ops.FEAT_ROWS_SEGMENT
    return (16, 48, seg - 16, seg, seg + 16, 3 * seg + 32)


@pytest.mark.parametrize("box_bytes", [16, 192])
def test_feat_rows_bit_exact_against_numpy_model(gpu, box_bytes):
    """n = 9 rows, one of every kind (skipped; copy; copy + keep; copy + check with equal boxes, with one bit of the first float changed,
    with one bit of the last float changed; two rows sharing a source, one of them kept; an equal row whose flag was already 1), at row
    sizes around the segment size: destinations, slots with their boxes trailer and flags against the model, guard bands included"""
    for j, row_bytes in enumerate(_row_sizes()):
        case = _Case(gpu, 9, row_bytes, box_bytes, seed=100 * box_bytes + j)
        case.launch()
        case.verify()


def test_feat_rows_beyond_one_grid(gpu):
    """more (row, segment) items than the launch has workgroups (4096): the block-stride loop, all row kinds repeating"""
    case = _Case(gpu, 4200, 48, 16, seed=3)
    case.launch()
    case.verify()


def test_feat_rows_without_keep_and_ref_tables_is_a_plain_gather(gpu):
    from din_amd import ops
    case = _Case(gpu, 9, 48, 16, seed=4)
    ops.feat_rows(case.src_t, case.dst_t, case.rb)
    case.want_slot, case.want_flags = case.slot_h, case.flags_h
    case.verify()


def test_feat_rows_refusals_and_empty_calls_write_nothing(gpu):
    from din_amd import _lib
    lib = _lib.load()
    case = _Case(gpu, 9, 48, 16, seed=5)
    p = lambda t: C.c_void_p(t.data_ptr())
    src, dst, keep, ref, boxes, flags = p(case.src_t), p(case.dst_t), p(case.keep_t), p(case.ref_t), p(case.boxes_d), p(case.flags_view)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    E_ARG = -1                                                   # DIN_E_ARG (include/din_hip.h)
    assert "DIN_E_ARG = -1" in open(_lib.HEADER_PATH).read()
    call = lib.din_feat_rows
    assert call(src, dst, keep, ref, boxes, flags, 9, 24, 16, stream) == E_ARG          # row_bytes not a multiple of 16
    assert call(src, dst, keep, ref, boxes, flags, 9, 48, 8, stream) == E_ARG           # box_bytes not a multiple of 16
    assert call(src, dst, keep, ref, C.c_void_p(case.boxes_d.data_ptr() + 4), flags, 9, 48, 16, stream) == E_ARG    # boxes misaligned
    assert call(src, dst, keep, ref, boxes, flags, -1, 48, 16, stream) == E_ARG
    assert call(src, dst, keep, ref, boxes, flags, 9, -48, 16, stream) == E_ARG
    assert call(src, dst, keep, ref, boxes, flags, 9, 48, -16, stream) == E_ARG
    assert call(None, dst, keep, ref, boxes, flags, 9, 48, 16, stream) == E_ARG
    assert call(src, None, keep, ref, boxes, flags, 9, 48, 16, stream) == E_ARG
    assert call(src, dst, keep, None, None, flags, 9, 48, 16, stream) == E_ARG          # keep without boxes
    assert call(src, dst, None, ref, boxes, None, 9, 48, 16, stream) == E_ARG           # ref_boxes without flags
    assert lib.din_last_error_string()
    assert call(src, dst, keep, ref, boxes, flags, 0, 48, 16, stream) == 0              # n == 0: OK, nothing to do
    assert call(None, None, None, None, None, None, 0, 48, 16, stream) == 0
    case.verify_untouched("a refused or empty call")
    assert call(src, dst, keep, ref, boxes, flags, 9, 48, 16, stream) == 0
    case.verify("after the refusals")


def test_feat_rows_leaves_a_row_with_a_misaligned_address_alone(gpu):
    """the tables live on the device, so the host cannot refuse them: a row whose dst / keep / ref address is no multiple of 16 is
    skipped like a row with src = 0 (the cache never builds one)"""
    case = _Case(gpu, 9, 48, 16, seed=6)
    case.dst_t[COPY] += 8
    case.keep_t[KEEP] += 4
    case.ref_t[CHECK_FIRST] += 8
    case.launch()
    for i in (COPY, KEEP, CHECK_FIRST):
        case.want_dst[i * case.dstride:(i + 1) * case.dstride] = case.dst_h[i * case.dstride:(i + 1) * case.dstride]
        case.want_slot[i * case.sstride:(i + 1) * case.sstride] = case.slot_h[i * case.sstride:(i + 1) * case.sstride]
        case.want_flags[GUARD + i] = case.flags_h[GUARD + i]
    case.verify()


def test_feat_rows_is_capturable(gpu):
    """one plain launch on the given stream: it can be recorded into a HIP graph and replayed"""
    from din_amd import ops
    case = _Case(gpu, 9, ops.FEAT_ROWS_SEGMENT + 16, 192, seed=7)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        case.launch()
    case.reset()
    torch.cuda.synchronize()
    g.replay()
    case.verify("replay")


# ---- FeatureCache ----------------------------------------------------------------------------------------------------------------------
RB, BB = 1600, 192                                               # 400 floats of features, 12 boxes


def _feature_rows(gpu, count=10):
    g = torch.Generator().manual_seed(13)
    rows, boxes = torch.randn((count, RB // 4), generator=g), torch.rand((count, BB // 4), generator=g) * 40
    return rows, boxes, rows.to(gpu), boxes.to(gpu)


def test_feature_cache_round_trip_across_slabs(gpu):
    from din_amd.feature_cache import FeatureCache
    rows, boxes, drows, dboxes = _feature_rows(gpu)
    cache = FeatureCache(gpu, RB, BB, 1 << 30, chunk_frames=4)
    assert cache.bytes == 0 and not cache.slabs and cache.flags is None
    ids = [100 + 7 * i for i in range(10)]                       # frame ids are names, not slot numbers
    out, new = cache.rows(ids[:6], dboxes[:6], range(6), drows[:6].contiguous())
    assert new == ids[:6] and len(cache.slabs) == 2 and torch.equal(out.cpu(), rows[:6])
    # frames 3..5 are resident (their rows are not given), 6..9 are computed
    out, new = cache.rows(ids[3:], dboxes[3:], range(3, 7), drows[6:].contiguous())
    assert new == ids[6:] and len(cache.slabs) == 3 and torch.equal(out.cpu(), rows[3:])
    assert cache.inserted == 10 and cache.bytes == 12 * 1792 and cache.table.stride == 1792
    assert (cache.hits, cache.misses) == (3, 10)
    order = [9, 0, 3, 3, 7, 1, 9, 4, 8, 2, 6, 5, 0]
    out, new = cache.rows([ids[i] for i in order], dboxes[order])
    assert new == [] and out.shape == (len(order), RB // 4) and out.dtype == torch.float32 and torch.equal(out.cpu(), rows[order])
    cache.check()                                                # every served row met the boxes stored with it
    assert cache.misses == 10 and cache.hits == 3 + len(order)
    for i in (0, 5, 9):                                          # the slot's trailer holds the frame's boxes
        slab, off = cache.table.locate(cache.table.slot_of[ids[i]])
        got = cache.slabs[slab][off:off + RB + BB].cpu().numpy()
        assert got[:RB].tobytes() == rows[i].numpy().tobytes() and got[RB:].tobytes() == boxes[i].numpy().tobytes()
    with pytest.raises(KeyError):
        cache.rows([ids[0], 5], dboxes[:2])


def test_a_frame_that_occurs_twice_is_served_from_the_computed_row(gpu):
    from din_amd.feature_cache import FeatureCache
    rows, boxes, drows, dboxes = _feature_rows(gpu)
    cache = FeatureCache(gpu, RB, BB, 1 << 30, chunk_frames=4)
    # frame 20 at rows 0 and 2 of the batch, both computed (the second computation is ignored), frame 21 between them
    b = dboxes[[0, 1, 0]].contiguous()
    out, new = cache.rows([20, 21, 20], b, [0, 1, 2], drows[[0, 1, 5]].contiguous())
    assert new == [20, 21] and cache.inserted == 2
    assert torch.equal(out.cpu(), rows[[0, 1, 0]])
    out, _ = cache.rows([20, 21], dboxes[:2])
    assert torch.equal(out.cpu(), rows[:2])
    cache.check()


def test_full_cache_serves_the_rest_from_the_computed_rows(gpu):
    from din_amd.feature_cache import FeatureCache
    rows, boxes, drows, dboxes = _feature_rows(gpu)
    cache = FeatureCache(gpu, RB, BB, 6 * 1792 + 100, chunk_frames=4)
    ids = list(range(50, 60))
    out, new = cache.rows(ids, dboxes, range(10), drows)
    assert new == ids[:6] and torch.equal(out.cpu(), rows)       # a capacity of 6 slots: the 7th onward are served, not kept
    assert [cache.resident(i) for i in ids] == [True] * 6 + [False] * 4 and cache.bytes == 6 * 1792 and len(cache.slabs) == 2
    order = [8, 1, 6, 6, 0, 9, 5, 7, 2, 8]                       # a mixed batch: resident frames by id only, the others computed
    pos = [r for r, i in enumerate(order) if i >= 6]
    out, new = cache.rows([ids[i] for i in order], dboxes[order], pos, drows[[order[r] for r in pos]].contiguous())
    assert new == [] and cache.inserted == 6 and torch.equal(out.cpu(), rows[order])
    cache.check()
    with pytest.raises(KeyError):
        cache.rows([ids[7]], dboxes[7:8])


def test_check_raises_after_a_gather_with_other_boxes(gpu):
    from din_amd.feature_cache import FeatureCache
    rows, boxes, drows, dboxes = _feature_rows(gpu)
    cache = FeatureCache(gpu, RB, BB, 1 << 30, chunk_frames=4)
    ids = list(range(30, 40))
    cache.rows(ids, dboxes, range(10), drows)
    cache.check()                                                # inserts compare nothing
    altered = dboxes.clone()
    altered[4, 17] += 0.5                                        # one coordinate of one box of frame 34
    altered[8, 0] = -altered[8, 0]
    out, _ = cache.rows(ids, altered)
    assert torch.equal(out.cpu(), rows)                          # the rows are served all the same; the pass ends with the error
    with pytest.raises(RuntimeError) as e:
        cache.check()
    assert "(4, 34)" in str(e.value) and "(8, 38)" in str(e.value) and "2 rows" in str(e.value)
    cache.check()                                                # the flags were cleared
    cache.rows(ids, dboxes)
    cache.check()


# ---- through the models ----------------------------------------------------------------------------------------------------------------
def _model_cfg(name):
    from din_amd.config import Config
    cfg = Config("volleyball")
    cfg.backbone, cfg.image_size, cfg.out_size, cfg.emb_features = "vgg16", (96, 160), (3, 5), 512
    cfg.num_boxes, cfg.num_frames, cfg.num_features_boxes, cfg.num_features_gcn = 12, 3, 64, 64
    cfg.ST_kernel_size, cfg.sampling_ratio, cfg.beta_factor, cfg.train_backbone = [(3, 3)], [1], False, False
    cfg.num_features_relation, cfg.num_graph, cfg.gcn_layers, cfg.pos_threshold = 16, 4, 1, 0.5
    cfg.inference_module_name, cfg.train_dropout_prob = name, 0.0
    return cfg


@pytest.mark.parametrize("name,frames", [("dynamic_volleyball", 3), ("arg_volleyball", 9)], ids=["dynamic", "arg_eval_fold"])
def test_models_skip_the_trunk_for_resident_frames(gpu, monkeypatch, name, frames):
    """the same clips three times through a frozen VGG16 model in eval(): as a plain images tensor, through FrameRefs with every frame
    missed, and through FrameRefs with M = 0.  The feats tensor entering fc_emb_1 is bit-identical in all three (the plain call and the
    all-missed call run the same kernels on the same frames in the same order; the third reads back what the second stored), the
    backbone runs once in the second call and not at all in the third.  ARG_volleyball's eval() folds nine frames into three sub-clips."""
    import copy
    from din_amd import infer_model as IM, ops
    from din_amd.feature_cache import FeatureCache, FrameRefs, row_and_box_bytes
    from din_amd.train_net_dynamic import SyntheticVolleyball, build_model
    cfg = _model_cfg(name)
    torch.manual_seed(3)
    model = build_model(cfg).to(gpu).eval()
    assert not any(p.requires_grad for p in model.backbone.parameters())
    dcfg = copy.copy(cfg)
    dcfg.num_frames = frames
    clips = [SyntheticVolleyball(dcfg, length=2, seed=4)[i] for i in range(2)]
    images = torch.stack([c[0] for c in clips]).to(gpu)          # uint8 [2, frames, 3, 96, 160]
    boxes = torch.stack([c[1] for c in clips]).to(gpu)
    B, T = 2, frames
    seen, calls = [], []
    real_linear, real_trunk = ops.linear, model.backbone.forward_nhwc

    def linear(x, weight, *a, **kw):
        if weight is model.fc_emb_1.weight:
            seen.append(x.detach().clone())
        return real_linear(x, weight, *a, **kw)

    def trunk(x):
        calls.append(int(x.shape[0]))
        return real_trunk(x)

    monkeypatch.setattr(IM.ops, "linear", linear)
    monkeypatch.setattr(model.backbone, "forward_nhwc", trunk)
    cache = FeatureCache(gpu, *row_and_box_bytes(cfg), 1 << 30)
    ids = np.arange(1000, 1000 + B * T).reshape(B, T)
    with torch.no_grad():
        plain = model((images, boxes))["activities"]
        assert calls == [B * T]
        first = FrameRefs(ids, images.reshape(B * T, 3, 96, 160), np.arange(B * T), cache)
        out1 = model((first, boxes))["activities"]
        assert calls == [B * T, B * T] and first.inserted == ids.reshape(-1).tolist() and cache.inserted == B * T
        second = FrameRefs(ids, images.reshape(B * T, 3, 96, 160)[:0], [], cache)
        out2 = model((second, boxes))["activities"]
        assert calls == [B * T, B * T], "the backbone ran for a batch whose frames are all resident"
    torch.cuda.synchronize()
    cache.check()
    assert len(seen) == 3 and seen[0].shape == seen[1].shape == seen[2].shape
    assert seen[0].numel() == B * T * 12 * 512 * 25 and (cache.hits, cache.misses) == (B * T, B * T) and second.inserted == []
    assert torch.equal(seen[1], seen[2]), "feats differ between the computed rows and the rows read back from the slots"
    assert torch.equal(seen[0], seen[1]), "feats through FrameRefs differ from those of the plain images tensor"
    assert out1.shape == plain.shape == (2, cfg.num_activities)
    print("logits, plain | all missed | all resident:", plain[0, :3].tolist(), out1[0, :3].tolist(), out2[0, :3].tolist())


def test_a_trained_backbone_is_refused_by_the_model(gpu):
    from din_amd.feature_cache import FeatureCache, FrameRefs, row_and_box_bytes
    from din_amd.train_net_dynamic import build_model
    cfg = _model_cfg("dynamic_volleyball")
    cfg.train_backbone = True
    model = build_model(cfg).to(gpu).eval()
    refs = FrameRefs(np.zeros((1, 3), dtype=np.int64), torch.zeros((0, 3, 96, 160), dtype=torch.uint8, device=gpu), [],
                     FeatureCache(gpu, *row_and_box_bytes(cfg), 1 << 20))
    with pytest.raises(ValueError):
        model((refs, torch.zeros((1, 3, 12, 4), device=gpu)))


# ---- end to end through the trainer ----------------------------------------------------------------------------------------------------
STEPS_PER_EPOCH = 3                                              # 2 training clips at batch size 1, then 1 validation clip


def _run_two_epochs(feature_cache_gb):
    """train_net over the volleyball tree of tests/golden/dataset_tree (train sequence 1: two clips; test sequence 4: one clip; three
    frames a clip at 96x160, VGG16, frozen).  Returns (decode calls and backbone calls, each as the number of model calls made before
    it, the caches' (hits, misses, inserted) seen at every model call and at the end, the infos, the caches)."""
    from din_amd import feature_cache as FE, volleyball as V
    from din_amd.backbone.backbone import MyVGG16
    from din_amd.config import Config
    from din_amd.infer_model import Dynamic_volleyball
    from din_amd.train_net_dynamic import train_net
    cfg = Config("volleyball")
    cfg.data_path, cfg.train_seqs, cfg.test_seqs = os.path.join(GOLDEN, "dataset_tree", "volleyball"), [1], [4]
    cfg.backbone, cfg.image_size, cfg.out_size, cfg.emb_features = "vgg16", (96, 160), (3, 5), 512
    cfg.num_boxes, cfg.num_frames, cfg.num_before, cfg.num_after = 12, 3, 1, 1
    cfg.num_features_boxes, cfg.num_features_gcn = 64, 64
    cfg.ST_kernel_size, cfg.sampling_ratio, cfg.beta_factor, cfg.train_backbone = [(3, 3)], [1], False, False
    cfg.training_stage, cfg.batch_size, cfg.test_batch_size, cfg.max_epoch, cfg.test_interval_epoch = 2, 1, 1, 2, 1
    cfg.train_dropout_prob, cfg.train_learning_rate, cfg.lr_plan, cfg.train_random_seed = 0.0, 1e-4, {}, 5
    cfg.result_path = None
    cfg.feature_cache_gb, cfg.frame_cache_gb, cfg.num_workers = feature_cache_gb, 0, 0
    decodes, trunks, counters, caches, checks, model_calls = [], [], [], [], [], [0]
    real_load, real_init, real_trunk, real_check = V.load_frame_u8, FE.FeatureCache.__init__, MyVGG16.forward_nhwc, FE.FeatureCache.check

    def counting_load(path, size):
        decodes.append(model_calls[0])
        return real_load(path, size)

    def recording_init(self, *a, **kw):
        real_init(self, *a, **kw)
        caches.append(self)

    def counting_trunk(self, x):
        trunks.append((model_calls[0], int(x.shape[0])))
        return real_trunk(self, x)

    def counting_check(self):
        checks.append(model_calls[0])
        return real_check(self)

    def count():
        return tuple(sum(getattr(c, k) for c in caches) for k in ("hits", "misses", "inserted"))

    def pre_hook(module, args):
        if isinstance(module, Dynamic_volleyball):
            images = args[0][0]
            assert tuple(images.shape) == (1, 3, 3, 96, 160)
            assert isinstance(images, FE.FrameRefs) == (feature_cache_gb > 0)
            counters.append(count())
            model_calls[0] += 1

    handle = torch.nn.modules.module.register_module_forward_pre_hook(pre_hook)
    V.load_frame_u8, FE.FeatureCache.__init__, MyVGG16.forward_nhwc, FE.FeatureCache.check = counting_load, recording_init, counting_trunk, counting_check
    try:
        infos = train_net(cfg)
        torch.cuda.synchronize()
    finally:
        handle.remove()
        V.load_frame_u8, FE.FeatureCache.__init__, MyVGG16.forward_nhwc, FE.FeatureCache.check = real_load, real_init, real_trunk, real_check
    counters.append(count())
    return decodes, trunks, counters, infos, caches, checks


def test_train_net_skips_the_trunk_from_the_second_epoch(gpu):
    """two epochs with cfg.feature_cache_gb = 1 against two epochs with 0, frozen VGG16, same seed: in epoch 1 the nine frames are decoded
    and the backbone runs once per step on the step's three frames; in epoch 2 nothing is decoded, the backbone is not called and the
    caches report only hits; every pass ends with check(), which passes.

    The per-epoch losses agree at the 1e-4 relative bound tests/test_gpu_din_model.py uses for repeated runs of this step
    (test_captured_step_matches_eager); they are not asserted equal because the step's backward kernels (fc_emb_1's weight gradient, the
    DIN walk) sum fp32 partials with atomics, so two runs of the same step differ in the last bits.  Measured on one MI355X
    (profiles/feature_cache_test_margins.txt): all four losses bit-identical when this file ran alone, one of them 4.8e-7 apart (one
    fp32 step; 584x inside the bound) inside the whole suite."""
    decodes0, trunks0, _, infos0, caches0, checks0 = _run_two_epochs(0)
    assert not caches0 and not checks0 and len(decodes0) == 2 * 9 and [n for _, n in trunks0] == [3] * (2 * STEPS_PER_EPOCH)
    decodes, trunks, counters, infos, caches, checks = _run_two_epochs(1)
    assert len(caches) == 2 and all(c.device.type == "cuda" for c in caches)                 # one for training, one for validation
    assert len(counters) == 2 * STEPS_PER_EPOCH + 1
    # a decode call made after the last model call of epoch 1 started belongs to epoch 2 (the feed fetches at most one batch ahead, and
    # the first batch of an epoch is fetched after the previous pass has ended)
    assert len([c for c in decodes if c < STEPS_PER_EPOCH]) == 9 and [c for c in decodes if c >= STEPS_PER_EPOCH] == []
    assert trunks == [(k + 1, 3) for k in range(STEPS_PER_EPOCH)], trunks                     # once per step of epoch 1, then never
    # counters[k] is read before model call k: the rows of call k are counted inside it
    assert counters[STEPS_PER_EPOCH] == (0, 9, 9)                # epoch 1: nine rows, all missed and inserted
    assert counters[-1] == (9, 9, 9)                             # epoch 2: only hits
    assert len(checks) == 4 and sum(c.bytes for c in caches) == 2 * 64 * (614400 + 192)      # one slab of 64 slots each
    for i0, i1 in zip(infos0, infos):
        for part in ("train", "test"):
            a, b = i1[part]["loss"], i0[part]["loss"]
            print(f"epoch {i0[part]['epoch']} {part} loss, cache off {b!r}, cache on {a!r}, relative difference {abs(a - b) / max(1.0, abs(b)):.3e}")
            assert Measured(abs(a - b)) <= 1e-4 * max(1.0, abs(b)), (part, a, b)
