"""Flip augmentation on the MI355X: din_copy_rows_u8_flip against a numpy model (bit-exact, every alignment), FrameCache.build_batch with
mirrored rows, din_flip_clip_labels against numpy float32, the mirror convention against the project's RoIAlign, and both trainers over
tests/golden/dataset_tree with cfg.flip_prob set against the same runs without it."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.conftest import Measured

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

pytestmark = pytest.mark.gpu

GUARD, GUARD_BYTE, FILL_BYTE = 64, 0xA5, 0x3C
# widths below one vector, 16-multiples (the vector path), one off a 16-multiple, odd; 3x96x160 and 3x139x203 frames; lines longer than
# one 8 KB segment, aligned and not
SHAPES = ((1, 1), (3, 2), (5, 3), (4, 15), (6, 16), (6, 17), (3, 31), (2, 32), (7, 48), (288, 160), (417, 203), (2, 8208), (2, 8195))
ROWS = (1, 3, 37)
FLAG_VALUES = (0, 1, 7)


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from din_amd import _lib
    _lib.load()
    return torch.device("cuda")


def _place(base, offset, residue):
    """smallest offset' >= offset with (base + offset') % 16 == residue"""
    return offset + (residue - (base + offset)) % 16


def _residues(k=0, step=lambda k: (k % 16, (k // 16) % 16)):
    """the (source, destination) residues mod 16 of the copied rows: a walk through all 16 x 16 pairs with an aligned (0, 0) row after
    every fourth, so that the vector path is taken often"""
    while True:
        for _ in range(4):
            yield step(k)
            k += 1
        yield 0, 0


def _flip_case(gpu, lines, width, n, combos, flags_of, rng, skip_phase, stats, compare_plain=True):
    """one launch: n destination rows between guard bands, sources out of a pool of 16 rows (one per residue mod 16), every third row
    skipped (src = 0); flags_of() gives the flag of each copied row.  The whole destination buffer is compared with the numpy model;
    flip = None and all-zero flags are compared with din_copy_rows_u8 on the same tables."""
    from din_amd import ops
    nbytes = lines * width
    pool_stride = nbytes + 32
    src_buf = torch.from_numpy(rng.integers(0, 256, size=16 * pool_stride + 64, dtype=np.uint8)).to(gpu)
    row_stride = GUARD + 16 + nbytes + GUARD
    dst_host = np.full(n * row_stride + 64, FILL_BYTE, dtype=np.uint8)
    dst_buf = torch.empty(dst_host.size, dtype=torch.uint8, device=gpu)
    sbase, dbase = src_buf.data_ptr(), dst_buf.data_ptr()
    pool_off = [_place(sbase, r * pool_stride, r) for r in range(16)]                # pool row r starts at residue r
    src_tab, dst_tab, flags, plan = [], [], [], []
    for i in range(n):
        skipped = n > 1 and i % 3 == skip_phase
        rs, rd = (0, i % 16) if skipped else next(combos)
        flag = FLAG_VALUES[i % 3] if skipped else flags_of()                         # (a skipped row's flag must not matter)
        doff = _place(dbase, i * row_stride + GUARD, rd)
        assert doff + nbytes + GUARD <= (i + 1) * row_stride and pool_off[rs] + nbytes <= (rs + 1) * pool_stride
        dst_host[i * row_stride:doff] = GUARD_BYTE                                    # >= 64 guard bytes below the row ...
        dst_host[doff + nbytes:(i + 1) * row_stride] = GUARD_BYTE                     # ... and above it
        src_tab.append(0 if skipped else sbase + pool_off[rs])
        dst_tab.append(dbase + doff)
        flags.append(flag)
        assert skipped or ((src_tab[-1] % 16, dst_tab[-1] % 16) == (rs, rd))
        if not skipped:
            plan.append((pool_off[rs], doff, flag))
            stats["pairs"].add((rs, rd))
            if flag and width % 16 == 0:
                stats["aligned" if (rs, rd) == (0, 0) else "misaligned"] += 1
    src_host = src_buf.cpu().numpy()
    want, plain = dst_host.copy(), dst_host.copy()
    for so, do, flag in plan:                                                         # the numpy model
        row = src_host[so:so + nbytes]
        plain[do:do + nbytes] = row
        want[do:do + nbytes] = row.reshape(lines, width)[:, ::-1].reshape(-1) if flag else row
    d_src = torch.tensor(src_tab, dtype=torch.int64, device=gpu)
    d_dst = torch.tensor(dst_tab, dtype=torch.int64, device=gpu)
    d_flags = torch.tensor(flags, dtype=torch.int64, device=gpu)
    init = torch.from_numpy(dst_host).to(gpu)

    def run(fn):
        dst_buf.copy_(init)
        fn()
        torch.cuda.synchronize()
        return dst_buf.cpu().numpy()

    got = run(lambda: ops.copy_rows_u8_flip(d_src, d_dst, d_flags, lines, width))
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{lines}x{width} n={n}: {bad.size} bytes differ, first at {bad[:4]} (row stride {row_stride}, flags {flags[:6]})"
    if compare_plain:
        ref = run(lambda: ops.copy_rows_u8(d_src, d_dst, nbytes))
        assert np.array_equal(ref, plain)
        assert np.array_equal(run(lambda: ops.copy_rows_u8_flip(d_src, d_dst, None, lines, width)), ref), "flip = NULL is not the plain copy"
        zeros = torch.zeros_like(d_flags)
        assert np.array_equal(run(lambda: ops.copy_rows_u8_flip(d_src, d_dst, zeros, lines, width)), ref), "zero flags are not the plain copy"


def _cycle(values):
    state = {"k": 0}

    def nxt():
        state["k"] += 1
        return values[state["k"] % len(values)]
    return nxt


def test_copy_rows_flip_bit_exact_against_numpy(gpu):
    """every (lines, width, n) of the lists above with flags 0 / 1 / 7 mixed over the rows and the (source, destination) residues mod 16
    walking through all 16 x 16 pairs; guards of 0xA5 and skipped rows must come back unchanged (the whole destination buffer is
    compared); flip = NULL and all-zero flags equal din_copy_rows_u8"""
    stats = {"pairs": set(), "aligned": 0, "misaligned": 0}
    combos, flags_of, rng = _residues(), _cycle(FLAG_VALUES), np.random.default_rng(20241)
    for skip_phase, (lines, width) in enumerate(SHAPES):
        for n in ROWS:
            _flip_case(gpu, lines, width, n, combos, flags_of, rng, 1 + skip_phase % 2, stats)
    assert len(stats["pairs"]) == 256, f"only {len(stats['pairs'])} of the 256 residue pairs were exercised"
    assert stats["aligned"] >= 10 and stats["misaligned"] >= 10, stats     # mirrored 16-multiple widths: the vector path and the byte path


@pytest.mark.parametrize("lines,width,n", [(7, 15, 4200), (288, 160, 900)], ids=["4200x7x15", "900x288x160"])
def test_copy_rows_flip_bit_exact_beyond_one_grid(gpu, lines, width, n):
    """more (row, segment) items than the launch has workgroups (4096): the block-stride loop, alternate rows mirrored"""
    stats = {"pairs": set(), "aligned": 0, "misaligned": 0}
    combos = _residues(7, lambda k: ((5 * k) % 16, (3 * k + k // 16) % 16))
    _flip_case(gpu, lines, width, n, combos, _cycle((1, 0)), np.random.default_rng(7), 1, stats, compare_plain=False)
    if width % 16 == 0:
        assert stats["aligned"] >= 10 and stats["misaligned"] >= 10, stats


def test_copy_rows_flip_bit_exact_refusals_and_empty_calls_launch_nothing(gpu):
    from din_amd import _lib
    lib = _lib.load()
    src = torch.arange(256, dtype=torch.uint8, device=gpu)
    dst = torch.full((256,), FILL_BYTE, dtype=torch.uint8, device=gpu)
    st = torch.tensor([src.data_ptr()], dtype=torch.int64, device=gpu)
    dt = torch.tensor([dst.data_ptr()], dtype=torch.int64, device=gpu)
    ft = torch.ones(1, dtype=torch.int64, device=gpu)
    sp, dp, fp = C.c_void_p(st.data_ptr()), C.c_void_p(dt.data_ptr()), C.c_void_p(ft.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    E_ARG = -1                                                   # DIN_E_ARG (include/din_hip.h)
    assert "DIN_E_ARG = -1" in open(_lib.HEADER_PATH).read()
    f = lib.din_copy_rows_u8_flip
    assert f(None, dp, fp, 1, 4, 16, stream) == E_ARG
    assert f(sp, None, fp, 1, 4, 16, stream) == E_ARG
    assert f(sp, dp, fp, -1, 4, 16, stream) == E_ARG
    assert f(sp, dp, fp, 1, -4, 16, stream) == E_ARG
    assert f(sp, dp, fp, 1, 4, -16, stream) == E_ARG
    assert lib.din_last_error_string()
    assert f(sp, dp, fp, 0, 4, 16, stream) == 0                  # n == 0: OK, nothing to do
    assert f(None, None, None, 0, 4, 16, stream) == 0
    assert f(sp, dp, fp, 1, 0, 16, stream) == 0                  # zero bytes: OK, nothing to do
    assert f(sp, dp, fp, 1, 4, 0, stream) == 0
    g = lib.din_flip_clip_labels
    boxes = torch.ones(2, 3, 4, device=gpu)
    acts = torch.zeros(2, dtype=torch.int64, device=gpu)
    flags2 = torch.ones(2, dtype=torch.int64, device=gpu)
    lmap = torch.tensor([1, 0], dtype=torch.int64, device=gpu)
    bp, ap, f2, mp = (C.c_void_p(t.data_ptr()) for t in (boxes, acts, flags2, lmap))
    assert g(bp, ap, f2, None, mp, -1, 3, 5.0, 2, stream) == E_ARG
    assert g(bp, ap, f2, None, mp, 2, -3, 5.0, 2, stream) == E_ARG
    assert g(bp, ap, f2, None, mp, 2, 3, 5.0, -2, stream) == E_ARG
    assert g(bp, ap, None, None, mp, 2, 3, 5.0, 2, stream) == E_ARG
    assert g(bp, ap, f2, None, mp, 0, 3, 5.0, 2, stream) == 0    # no rows: OK, nothing to do
    assert g(None, None, f2, None, mp, 2, 3, 5.0, 2, stream) == 0
    torch.cuda.synchronize()
    assert bool((dst == FILL_BYTE).all()) and bool((boxes == 1).all()) and bool((acts == 0).all()), "a refused or empty call wrote"
    assert f(sp, dp, fp, 1, 4, 64, stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(dst.view(4, 64), src.view(4, 64).flip(-1))


# ---- FrameCache ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", [(3, 96, 160), (3, 13, 19)], ids=["3x96x160", "3x13x19"])
def test_build_batch_bit_exact_mirrors_flagged_rows_and_keeps_the_slots(gpu, frame):
    """a cache with room for 6 of 10 frames.  One batch inserts six and serves the other rows from the uploaded frames (the full-cache
    case), with mixed flags: every flagged row is np.flip of its frame, whether it came from a slot or from an uploaded row.  A plain
    gather afterwards returns the originals: the slots hold the frames as decoded."""
    from din_amd.frame_cache import FrameCache
    host = torch.randint(0, 256, (10,) + frame, generator=torch.Generator().manual_seed(11), dtype=torch.uint8)
    dev = host.to(gpu)
    fb = int(np.prod(frame))
    cache = FrameCache(gpu, frame, 6 * ((fb + 15) // 16 * 16) + 100, chunk_frames=4)
    ids = list(range(50, 60))
    order = [8, 1, 6, 6, 0, 9, 5, 7, 2, 8, 3, 4, 1]
    flip_rows = np.array([1, 1, 0, 1, 0, 1, 1, 0, 0, 0, 1, 1, 0], dtype=bool)
    pos = list(range(len(order)))                                # every row arrives with its pixels: the first six ids get slots
    batch, new = cache.build_batch([ids[i] for i in order], pos, dev[order].contiguous(), flip_rows=flip_rows)
    torch.cuda.synchronize()
    want = host[order].numpy().copy()
    want[flip_rows] = np.flip(want[flip_rows], -1)
    assert new == [ids[i] for i in (8, 1, 6, 0, 9, 5)] and cache.inserted == 6 and cache.table.full
    assert np.array_equal(batch.cpu().numpy(), want)
    assert cache.flip_flags is not None and cache.flip_flags.cpu().tolist() == flip_rows.astype(int).tolist()
    resident = [i for i in range(10) if cache.resident(ids[i])]
    assert sorted(resident) == [0, 1, 5, 6, 8, 9]
    got = cache.gather([ids[i] for i in resident])
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), host[resident]) and cache.flip_flags is None, "a slot holds a mirrored frame"
    # a mixed batch of resident frames (by id only) and uploaded ones, mixed flags again
    order2 = [9, 2, 0, 7, 7, 5]
    flip2 = np.array([1, 1, 0, 1, 0, 0], dtype=bool)
    pos2 = [r for r, i in enumerate(order2) if i not in resident]
    batch2, new2 = cache.build_batch([ids[i] for i in order2], pos2, dev[[order2[r] for r in pos2]].contiguous(), flip_rows=flip2)
    torch.cuda.synchronize()
    want2 = host[order2].numpy().copy()
    want2[flip2] = np.flip(want2[flip2], -1)
    assert new2 == [] and np.array_equal(batch2.cpu().numpy(), want2)
    # no flagged row: the plain gather, no flags uploaded
    batch3, _ = cache.build_batch([ids[i] for i in resident], flip_rows=np.zeros(len(resident), dtype=bool))
    torch.cuda.synchronize()
    assert cache.flip_flags is None and torch.equal(batch3.cpu(), host[resident])


# ---- labels ----------------------------------------------------------------------------------------------------------------------------
def _label_case(gpu, B, T, N, OW, clip_flags, n_valid, label_map, rng):
    from din_amd import ops
    boxes = rng.uniform(0, OW, (B, T, N, 4)).astype(np.float32)
    boxes[..., 2:] = np.maximum(boxes[..., :2], boxes[..., 2:])
    acts = rng.integers(0, 8, (B, T)).astype(np.int64)
    acts[0, 0], acts[-1, -1] = -1, -1                             # a label outside the map is left alone
    if n_valid is not None:
        for b in range(B):
            boxes[b, :, n_valid[b, 0]:] = 0.0                    # the collective padding
    rows = np.repeat(np.asarray(clip_flags, dtype=np.int64), T)
    want_b, want_a = boxes.copy(), acts.copy()
    w = np.float32(OW)
    for r in np.flatnonzero(rows):
        b, t = divmod(int(r), T)
        k = N if n_valid is None else int(n_valid[b, t])
        x1, x2 = boxes[b, t, :k, 0].copy(), boxes[b, t, :k, 2].copy()
        want_b[b, t, :k, 0], want_b[b, t, :k, 2] = w - x2, w - x1  # one float32 subtraction each
        if label_map is not None and 0 <= acts[b, t] < len(label_map):
            want_a[b, t] = label_map[acts[b, t]]
    d_flags = torch.from_numpy(rows).to(gpu)
    d_map = None if label_map is None else torch.tensor(label_map, dtype=torch.int64, device=gpu)
    d_valid = None if n_valid is None else torch.from_numpy(n_valid.astype(np.int32)).to(gpu)
    d_boxes, d_acts = torch.from_numpy(boxes).to(gpu), torch.from_numpy(acts).to(gpu)
    ops.flip_clip_labels(d_boxes, d_acts, d_flags, d_valid, d_map, OW)
    torch.cuda.synchronize()
    assert np.array_equal(d_boxes.cpu().numpy().view(np.uint32), want_b.view(np.uint32)), "boxes differ from numpy float32"
    assert np.array_equal(d_acts.cpu().numpy(), want_a)
    # each half alone
    d_boxes2, d_acts2 = torch.from_numpy(boxes).to(gpu), torch.from_numpy(acts).to(gpu)
    ops.flip_clip_labels(d_boxes2, None, d_flags, d_valid, d_map, OW)
    ops.flip_clip_labels(None, d_acts2, d_flags, d_valid, d_map, OW)
    torch.cuda.synchronize()
    assert torch.equal(d_boxes2, d_boxes) and torch.equal(d_acts2, d_acts)
    return boxes, want_b, acts, want_a


def test_flip_clip_labels_bit_exact_against_numpy_float32(gpu):
    from din_amd.volleyball import FLIP_ACTIVITIES
    rng = np.random.default_rng(3)
    boxes, got_b, acts, got_a = _label_case(gpu, 2, 3, 12, 5, [0, 1], None, FLIP_ACTIVITIES, rng)       # volleyball, clip 1 flagged
    assert np.array_equal(got_b[0], boxes[0]) and np.array_equal(got_a[0], acts[0])                    # the unflagged clip is untouched
    assert not np.array_equal(got_b[1], boxes[1]) and got_a[1, 0] == FLIP_ACTIVITIES[acts[1, 0]] and got_a[1, 2] == -1
    n_valid = np.repeat(np.array([[1], [7], [13], [7]]), 3, axis=1)                                    # collective: MAX_N = 13
    boxes, got_b, acts, got_a = _label_case(gpu, 4, 3, 13, 23, [1, 1, 1, 0], n_valid, None, rng)
    assert np.array_equal(got_a, acts)                                                                 # no map: the labels have no side
    for b in range(4):
        assert not got_b[b, :, n_valid[b, 0]:].view(np.uint32).any(), "a padding box is no longer bit-zero"
    assert np.array_equal(got_b[3], boxes[3])


# ---- the mirror convention -------------------------------------------------------------------------------------------------------------
def test_roi_align_of_the_mirrored_map_and_boxes_is_the_mirrored_crop(gpu):
    """RoIAlign samples continuous coordinates with pixel centres at +0.5, so column x of a map OW wide mirrors to OW - x: the crops of
    the mirrored map at the mirrored boxes are the crops of the original, mirrored along their last axis.  Bound 1e-4 * max|map|: a
    mirrored coordinate below 80 carries fp32 rounding of about 1e-5 px, and a bilinear sample moves by at most that times twice the
    map's range.  The convention OW - 1 - x must miss the bound by at least 100x."""
    from din_amd import ops
    from din_amd.roi_align.roi_align import RoIAlign
    H, W, Cn, K = 6, 9, 2, 5
    fm = torch.randn(1, Cn, H, W, generator=torch.Generator().manual_seed(4)).to(gpu)
    host_boxes = np.array([[0.0, 1.0, 2.3, 4.1],                 # touches the left border
                           [6.2, 0.0, 9.0, 2.7],                 # the right and the top border
                           [3.1, 2.2, 5.6, 6.0],                 # the bottom border
                           [1.7, 0.6, 7.9, 5.2],
                           [4.0, 3.0, 4.5, 3.5]], dtype=np.float32)
    # no sample column may sit on the edge of the map, where a rounding of 1e-5 px decides between a value and the zero outside it
    sw = (host_boxes[:, 2] - host_boxes[:, 0]) / K
    cols = host_boxes[:, :1] + sw[:, None] * (np.arange(K)[None, :] + 0.5) - 0.5
    assert np.abs(cols).min() > 1e-2 and np.abs(cols - (W - 1)).min() > 1e-2
    boxes = torch.from_numpy(host_boxes).to(gpu)
    ind = torch.zeros(len(host_boxes), dtype=torch.int32, device=gpu)
    roi = RoIAlign(K, K)
    crops = roi(fm, boxes, ind)
    mirrored_map = fm.flip(-1).contiguous()
    mirrored = boxes.clone().view(1, -1, 4)
    ops.flip_clip_labels(mirrored, None, torch.ones(1, dtype=torch.int64, device=gpu), None, None, W)
    assert np.array_equal(mirrored.cpu().numpy()[0], np.stack([np.float32(W) - host_boxes[:, 2], host_boxes[:, 1],
                                                               np.float32(W) - host_boxes[:, 0], host_boxes[:, 3]], -1))
    got = roi(mirrored_map, mirrored.view(-1, 4), ind)
    wrong_boxes = mirrored.view(-1, 4).clone()
    wrong_boxes[:, [0, 2]] -= 1.0                                # OW - 1 - x
    wrong = roi(mirrored_map, wrong_boxes, ind)
    torch.cuda.synchronize()
    scale = float(fm.abs().max())
    err = Measured(float((got - crops.flip(-1)).abs().max()))
    err_wrong = float((wrong - crops.flip(-1)).abs().max())
    print(f"mirror convention: max error {float(err):.3e} (OW - x), {err_wrong:.3e} (OW - 1 - x), max|map| {scale:.3f}")
    assert err <= 1e-4 * scale
    assert err_wrong >= 100 * 1e-4 * scale


# ---- end to end through the trainers ---------------------------------------------------------------------------------------------------
SEED = 5            # FlipPlan(0.5, 5, 0): epoch 1 draws [False, True], epoch 2 [True, True] (one clip per batch) -- checked in the test


def _run(flip_prob, frame_cache_gb, stage=2, result_path=None):
    """train_net over the volleyball tree of tests/golden/dataset_tree with the configuration of tests/test_gpu_frame_cache.py (train
    sequence 1: two clips; test sequence 4: one clip; 96x160, VGG16, batch size 1): stage 2 for two epochs of three-frame clips, or
    stage 1 for one epoch.  Returns what every model call received -- (training?, images, boxes) -- the decode calls by model-call
    index, what the loss received (stage 1), the infos and the caches."""
    import din_amd.train_net as T1
    import din_amd.train_net_dynamic as T2
    from din_amd import frame_cache as FC, volleyball as V
    from din_amd.base_model import Basenet_volleyball
    from din_amd.config import Config
    from din_amd.infer_model import Dynamic_volleyball
    cfg = Config("volleyball")
    cfg.data_path, cfg.train_seqs, cfg.test_seqs = os.path.join(GOLDEN, "dataset_tree", "volleyball"), [1], [4]
    cfg.backbone, cfg.image_size, cfg.out_size, cfg.emb_features = "vgg16", (96, 160), (3, 5), 512
    cfg.num_boxes, cfg.num_frames, cfg.num_before, cfg.num_after = 12, 3, 1, 1
    cfg.num_features_boxes, cfg.num_features_gcn = 64, 64
    cfg.ST_kernel_size, cfg.sampling_ratio, cfg.beta_factor, cfg.train_backbone = [(3, 3)], [1], False, True
    cfg.training_stage, cfg.batch_size, cfg.test_batch_size, cfg.max_epoch, cfg.test_interval_epoch = stage, 1, 1, stage, 1
    cfg.train_dropout_prob, cfg.train_learning_rate, cfg.lr_plan, cfg.train_random_seed = 0.0, 1e-4, {}, SEED
    cfg.result_path = result_path
    cfg.frame_cache_gb, cfg.num_workers, cfg.flip_prob = frame_cache_gb, 0, flip_prob
    calls, decodes, losses, caches = [], [], [], []
    real_load, real_init, real_losses = V.load_frame_u8, FC.FrameCache.__init__, T1._losses

    def counting_load(path, size):
        decodes.append(len(calls))                               # the number of model calls made so far
        return real_load(path, size)

    def recording_init(self, *a, **kw):
        real_init(self, *a, **kw)
        caches.append(self)

    def recording_losses(actions_scores, activities_scores, actions_in, activities_in, *rest):
        losses.append((actions_in.cpu().numpy().copy(), activities_in.cpu().numpy().copy()))
        return real_losses(actions_scores, activities_scores, actions_in, activities_in, *rest)

    def pre_hook(module, args):
        if isinstance(module, (Dynamic_volleyball, Basenet_volleyball)):
            images, boxes = args[0][0], args[0][1]
            assert images.dtype == torch.uint8 and images.is_cuda and tuple(images.shape[2:]) == (3, 96, 160)
            calls.append((module.training, images.cpu().numpy().copy(), boxes.cpu().numpy().copy()))

    handle = torch.nn.modules.module.register_module_forward_pre_hook(pre_hook)
    V.load_frame_u8, FC.FrameCache.__init__, T1._losses = counting_load, recording_init, recording_losses
    try:
        infos = (T2 if stage == 2 else T1).train_net(cfg)
        torch.cuda.synchronize()
    finally:
        handle.remove()
        V.load_frame_u8, FC.FrameCache.__init__, T1._losses = real_load, real_init, real_losses
    print(f"flip_prob {flip_prob}, frame_cache_gb {frame_cache_gb}, stage {stage}: loss per epoch",
          [(i["train"]["loss"], i["test"]["loss"]) for i in infos])
    return dict(calls=calls, decodes=decodes, losses=losses, infos=infos, caches=caches, ow=cfg.out_size[1])


def _mirrored_boxes(boxes, ow):
    out = boxes.copy()
    out[..., 0], out[..., 2] = np.float32(ow) - boxes[..., 2], np.float32(ow) - boxes[..., 0]
    return out


def _check_against_plain(run, plain, flagged_calls):
    """every training call in `flagged_calls` (indices among the training calls) received np.flip of the plain run's images and the
    numpy-mirrored boxes, every other call exactly what the plain run's received"""
    assert len(run["calls"]) == len(plain["calls"])
    k = 0
    for (training, images, boxes), (training0, images0, boxes0) in zip(run["calls"], plain["calls"]):
        assert training == training0
        if training and k in flagged_calls:
            assert np.array_equal(images, np.flip(images0, -1)), f"training call {k}: the images are not the mirrored clip"
            assert np.array_equal(boxes.view(np.uint32), _mirrored_boxes(boxes0, run["ow"]).view(np.uint32)), f"training call {k}: boxes"
        else:
            assert np.array_equal(images, images0), f"call (training {training}, {k}): a clip that was not drawn differs from the plain run"
            assert np.array_equal(boxes.view(np.uint32), boxes0.view(np.uint32))
        k += int(training)
    return k


@pytest.fixture(scope="module")
def plain_run(gpu):
    run = _run(0.0, 0)
    assert [c[0] for c in run["calls"]] == [True, True, False] * 2 and not run["caches"]
    assert all("flipped_clips" not in i["train"] for i in run["infos"])
    return run


@pytest.fixture(scope="module")
def half_run_uncached(gpu):
    return _run(0.5, 0)


@pytest.mark.parametrize("frame_cache_gb", [0, 1], ids=["cache_off", "cache_on"])
def test_train_net_stage2_mirrors_every_training_clip_at_flip_prob_one(gpu, plain_run, frame_cache_gb):
    run = _run(1.0, frame_cache_gb)
    assert _check_against_plain(run, plain_run, {0, 1, 2, 3}) == 4                  # and every validation call is the plain run's
    assert [i["train"]["flipped_clips"] for i in run["infos"]] == [2, 2] and all("flipped_clips" not in i["test"] for i in run["infos"])
    if frame_cache_gb:
        # epoch 2 decodes nothing: its mirrored training clips and its plain validation clip all come out of slots, which therefore
        # hold the frames as decoded
        assert len([c for c in run["decodes"] if c < 3]) == 9 and [c for c in run["decodes"] if c >= 3] == []
        assert len(run["caches"]) == 2 and sum(c.inserted for c in run["caches"]) == 9 and sum(c.hits for c in run["caches"]) == 9
    else:
        assert len(run["decodes"]) == 2 * 9 and not run["caches"]


def test_train_net_stage2_flags_the_drawn_clips_at_flip_prob_half(gpu, plain_run, half_run_uncached):
    from din_amd.frame_cache import FlipPlan
    plan = [[bool(e.draw(1)[0]), bool(e.draw(1)[0])] for e in (FlipPlan(0.5, SEED, 0).epoch(1), FlipPlan(0.5, SEED, 0).epoch(2))]
    assert plan == [[False, True], [True, True]]                                    # at least one flagged and one unflagged clip
    flagged = {k for k, f in enumerate(plan[0] + plan[1]) if f}
    assert _check_against_plain(half_run_uncached, plain_run, flagged) == 4
    assert [i["train"]["flipped_clips"] for i in half_run_uncached["infos"]] == [sum(plan[0]), sum(plan[1])]
    cached = _run(0.5, 1)
    assert _check_against_plain(cached, plain_run, flagged) == 4                    # identical with the cache on and off
    assert [i["train"]["flipped_clips"] for i in cached["infos"]] == [sum(plan[0]), sum(plan[1])]
    assert [c for c in cached["decodes"] if c >= 3] == []


def test_train_net_stage1_mirrors_images_boxes_and_activities(gpu, tmp_path):
    from din_amd.volleyball import FLIP_ACTIVITIES
    plain = _run(0.0, 0, stage=1, result_path=str(tmp_path))
    run = _run(1.0, 0, stage=1, result_path=str(tmp_path))
    n_train = sum(c[0] for c in plain["calls"])
    assert n_train == 2 and _check_against_plain(run, plain, set(range(n_train))) == n_train
    assert run["infos"][0]["train"]["flipped_clips"] == n_train and "flipped_clips" not in plain["infos"][0]["train"]
    assert len(run["losses"]) == len(plain["losses"]) == len(plain["calls"])
    for k, ((actions, activities), (actions0, activities0)) in enumerate(zip(run["losses"], plain["losses"])):
        assert np.array_equal(actions, actions0)                                     # actions have no side
        if plain["calls"][k][0]:
            assert np.array_equal(activities, np.asarray(FLIP_ACTIVITIES)[activities0]), "the activity given to the loss is not mapped"
        else:
            assert np.array_equal(activities, activities0)
