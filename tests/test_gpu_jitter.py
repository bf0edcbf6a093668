"""Colour jitter on the MI355X: din_rows_gray_partials and din_copy_rows_u8_jitter through the C ABI against the numpy model of
tests/jitter_reference.py (which tests/test_jitter_cpu.py holds to Pillow) -- equality, never a tolerance -- then FrameCache.build_batch
with mixed resident and uploaded rows, and both trainers over tests/golden/dataset_tree with cfg.color_jitter set against the same runs
without it."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import jitter_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

pytestmark = pytest.mark.gpu

GUARD, GUARD_BYTE, FILL_BYTE, SENTINEL = 64, 0xA5, 0x3C, 0x5A5A5A5A
# lines shorter than, equal to and longer than a segment of 8192 bytes; widths on and off 16; (37, 64) has one line group per row,
# (2, 8192) and (1, 8208) one line per group, (129, 64) two groups the second of a single line
SHAPES = ((1, 1), (2, 3), (5, 16), (4, 48), (3, 100), (2, 8192), (1, 8208), (37, 64), (129, 64))
ROWS = (1, 3, 7)
# (contrast, brightness, saturation): every combination of stages, factors that saturate at both ends
TRIPLES = ((1, 1, 1), (0.25, 1.75, 1.999), (0, 1, 1), (1, 0, 1), (1, 1, 0), (1.999, 1, 1), (1, 1.999, 1), (1, 1, 1.75), (1.75, 0.25, 0),
           (1, 1.75, 0.25), (0.25, 1, 1.75), (0, 0, 0), (1.999, 1.999, 1.999), (0.25, 1.75, 1), (1.75, 1.999, 1))


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


def _frames(rng, h, w):
    """the pool a case draws its source frames from: random, all 0, all 255, one colour, near white"""
    return [rng.integers(0, 256, (3, h, w), dtype=np.uint8), np.zeros((3, h, w), dtype=np.uint8), np.full((3, h, w), 255, dtype=np.uint8),
            np.broadcast_to(np.array([200, 30, 90], dtype=np.uint8)[:, None, None], (3, h, w)).copy(),
            rng.integers(249, 256, (3, h, w), dtype=np.uint8), rng.integers(0, 256, (3, h, w), dtype=np.uint8)]


class _Case:
    """n rows of [3, h, w] between guard bands: row i reads pool frame i % 6 stored at residue rs and writes at residue rd; every
    `skip`-th row has src = 0.  `plan(i)` gives (rs, rd, flag, triple) of row i.  Expected bytes come from the numpy model, once per
    distinct (frame, flag, triple)."""

    def __init__(self, gpu, h, w, n, plan, rng, skip=3):
        self.gpu, self.h, self.w, self.n = gpu, h, w, n
        fb = self.fb = 3 * h * w
        self.segs = R.segments(h, w)
        pool = _frames(rng, h, w)
        sstride = fb + 32
        dstride = GUARD + 16 + fb + GUARD
        self.src_buf = torch.zeros(n * sstride + 64, dtype=torch.uint8, device=gpu)
        self.dst_buf = torch.empty(n * dstride + 64, dtype=torch.uint8, device=gpu)
        sbase, dbase = self.src_buf.data_ptr(), self.dst_buf.data_ptr()
        src_host = np.zeros(self.src_buf.numel(), dtype=np.uint8)
        dst_host = np.full(self.dst_buf.numel(), FILL_BYTE, dtype=np.uint8)
        want = None
        src_tab, dst_tab, flags, factors, self.rows, memo = [], [], [], [], [], {}
        self.want_parts = np.full(n * self.segs, SENTINEL, dtype=np.int64)
        for i in range(n):
            rs, rd, flag, triple = plan(i)
            skipped = n > 1 and i % skip == 1
            soff, doff = _place(sbase, i * sstride, rs), _place(dbase, i * dstride + GUARD, rd)
            assert soff + fb <= (i + 1) * sstride and doff + fb + GUARD <= (i + 1) * dstride
            dst_host[i * dstride:doff] = GUARD_BYTE
            dst_host[doff + fb:(i + 1) * dstride] = GUARD_BYTE
            k = i % len(pool)
            src_host[soff:soff + fb] = pool[k].reshape(-1)
            src_tab.append(0 if skipped else sbase + soff)
            dst_tab.append(dbase + doff)
            flags.append(flag)
            factors.append(triple)
            if not skipped:
                key = (k, bool(flag), triple)
                if key not in memo:
                    memo[key] = R.jitter(pool[k], *triple, mirror=bool(flag)).reshape(-1)
                self.rows.append((doff, memo[key], (src_tab[-1] % 16, dst_tab[-1] % 16), bool(flag), triple))
                self.want_parts[i * self.segs:(i + 1) * self.segs] = R.gray_partials(pool[k])
        want = dst_host.copy()
        for doff, row, _, _, _ in self.rows:
            want[doff:doff + fb] = row
        self.want = want
        self.src_buf.copy_(torch.from_numpy(src_host))
        self.init = torch.from_numpy(dst_host).to(gpu)
        self.d_src = torch.tensor(src_tab, dtype=torch.int64, device=gpu)
        self.d_dst = torch.tensor(dst_tab, dtype=torch.int64, device=gpu)
        self.flag_values = flags
        self.d_flags = torch.tensor(flags, dtype=torch.int64, device=gpu)
        self.d_factors = torch.tensor(factors, dtype=torch.float32, device=gpu)
        self.parts = torch.empty(GUARD + n * self.segs + GUARD, dtype=torch.int32, device=gpu)
        self.work = self.parts[GUARD:GUARD + n * self.segs]
        self.reset()

    def reset(self):
        self.dst_buf.copy_(self.init)
        self.parts.fill_(SENTINEL)

    def launch(self):
        from din_amd import ops
        ops.rows_gray_partials(self.d_src, self.work, self.h, self.w)
        ops.copy_rows_u8_jitter(self.d_src, self.d_dst, self.d_flags, self.d_factors, self.work, self.h, self.w)

    def verify(self, what=""):
        torch.cuda.synchronize()
        parts = self.parts.cpu().numpy().view(np.uint32).astype(np.int64)
        assert (parts[:GUARD] == SENTINEL).all() and (parts[-GUARD:] == SENTINEL).all(), f"{what}: a partial was written outside its table"
        bad = np.flatnonzero(parts[GUARD:-GUARD] != self.want_parts)
        assert bad.size == 0, f"{what} {self.h}x{self.w} n={self.n}: {bad.size} grey partials differ (or a skipped row's were written), first {bad[:4]}"
        got = self.dst_buf.cpu().numpy()
        bad = np.flatnonzero(got != self.want)
        assert bad.size == 0, (f"{what} {self.h}x{self.w} n={self.n}: {bad.size} bytes differ from the model, first at {bad[:4]}: got "
                               f"{got[bad[:4]]}, want {self.want[bad[:4]]}")
        return got


def _plans():
    """row plans that walk the residues, flags and triples independently: even rows are 16-byte aligned on both sides (offset 0 or 16:
    the vector path where the width allows), odd rows walk all 16 source and all 16 destination residues (the byte path)"""
    state = {"k": 0}

    def plan(i):
        k = state["k"] = state["k"] + 1
        rs, rd = (0, 0) if k % 2 == 0 else ((k // 2) % 16, (5 * (k // 2) + 3) % 16)
        return rs, rd, (0, 1, 7, 0, 1, 0, 7)[k % 7], TRIPLES[k % len(TRIPLES)]        # (periods 2, 7 and 15: every combination turns up)
    return plan


def test_jitter_gather_bit_exact_against_the_model(gpu):
    """every (H, W, n) of the lists above through both launches; the whole destination buffer with its guard bands, the whole partials
    table with its guard bands, skipped rows included, equal the model's"""
    plan, rng = _plans(), np.random.default_rng(20251)
    seen = {"src": set(), "dst": set(), "kinds": set(), "vector": 0, "bytes_on_16": 0, "stages": set()}
    for h, w in SHAPES:
        for n in ROWS:
            case = _Case(gpu, h, w, n, plan, rng)
            case.launch()
            case.verify("launch")
            for _, _, (rs, rd), flag, triple in case.rows:
                jittered = triple != (1, 1, 1)
                seen["kinds"].add((flag, jittered))
                seen["stages"].add(tuple(f != 1 for f in triple))
                if w % 16 == 0 and jittered:
                    seen["vector" if (rs, rd) == (0, 0) else "bytes_on_16"] += 1
                if (rs, rd) != (0, 0):
                    seen["src"].add(rs), seen["dst"].add(rd)
    assert seen["src"] >= set(range(1, 16)) and seen["dst"] == set(range(16)), seen
    assert seen["kinds"] == {(False, False), (True, False), (False, True), (True, True)}       # plain, mirrored, jittered, both
    assert len(seen["stages"]) == 8 and seen["vector"] >= 10 and seen["bytes_on_16"] >= 10, seen


@pytest.mark.parametrize("h,w", [(2, 4112), (2, 4097)], ids=["vector_2x4112", "bytes_2x4097"])
def test_jitter_gather_bit_exact_beyond_one_grid(gpu, h, w):
    """2100 rows of two one-line groups: 4200 items behind 4096 workgroups, both launches block-stride"""
    state = {"k": 0}

    def plan(i):
        state["k"] += 1
        return 0, 0, state["k"] % 2, TRIPLES[1 + state["k"] % 3]
    case = _Case(gpu, h, w, 2100, plan, np.random.default_rng(9), skip=50)
    assert case.segs == 2 and case.n * case.segs > 4096
    case.launch()
    case.verify("beyond one grid")


def test_jitter_gather_bit_exact_five_calls_and_null_factors(gpu):
    """five calls give the same bytes; factors = partials = NULL and all-one factors are din_copy_rows_u8_flip"""
    from din_amd import ops
    case = _Case(gpu, 37, 64, 7, _plans(), np.random.default_rng(3))
    outs = []
    for _ in range(5):
        case.reset()
        case.launch()
        outs.append(case.verify("repeat"))
    assert all(np.array_equal(outs[0], o) for o in outs[1:])
    case.reset()
    ops.copy_rows_u8_flip(case.d_src, case.d_dst, case.d_flags, 3 * case.h, case.w)
    torch.cuda.synchronize()
    flipped = case.dst_buf.cpu().numpy().copy()
    for factors, work in ((None, None), (torch.ones_like(case.d_factors), case.work)):
        case.reset()
        ops.copy_rows_u8_jitter(case.d_src, case.d_dst, case.d_flags, factors, work, case.h, case.w)
        torch.cuda.synchronize()
        assert np.array_equal(case.dst_buf.cpu().numpy(), flipped)
        assert bool((case.parts == SENTINEL).all()), "the gather wrote to the partials"
    case.reset()
    ops.copy_rows_u8_jitter(case.d_src, case.d_dst, None, None, None, case.h, case.w)
    ops.copy_rows_u8(case.d_src, case.d_dst, case.fb)                  # (the same bytes twice: the plain copy agrees)
    torch.cuda.synchronize()
    plain = case.dst_buf.cpu().numpy().copy()
    case.reset()
    ops.copy_rows_u8(case.d_src, case.d_dst, case.fb)
    torch.cuda.synchronize()
    assert np.array_equal(case.dst_buf.cpu().numpy(), plain)


def test_jitter_gather_bit_exact_replays_from_a_captured_graph(gpu):
    """both launches recorded into one HIP graph; a replay over new source bytes gives the model of the new bytes"""
    case = _Case(gpu, 5, 48, 3, _plans(), np.random.default_rng(4))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        case.launch()
    case.reset()
    torch.cuda.synchronize()
    g.replay()
    case.verify("replay")
    other = _Case(gpu, 5, 48, 3, _plans(), np.random.default_rng(5))   # the same plan over other pixels
    assert other.src_buf.numel() == case.src_buf.numel() and not np.array_equal(other.want, case.want)
    rel = (other.d_src - other.src_buf.data_ptr()).clamp(min=0)
    assert torch.equal(rel, (case.d_src - case.src_buf.data_ptr()).clamp(min=0))
    case.src_buf.copy_(other.src_buf)
    case.reset()
    g.replay()
    torch.cuda.synchronize()
    got = case.dst_buf.cpu().numpy()
    for (doff, row, _, _, _), (doff2, row2, _, _, _) in zip(case.rows, other.rows):
        assert np.array_equal(got[doff:doff + case.fb], row2)


def test_jitter_gather_bit_exact_refusals_and_empty_calls_launch_nothing(gpu):
    from din_amd import _lib, ops
    lib = _lib.load()
    case = _Case(gpu, 4, 16, 1, lambda i: (0, 0, 1, (0.25, 1.75, 0.5)), np.random.default_rng(6))
    sp, dp, fp = (C.c_void_p(t.data_ptr()) for t in (case.d_src, case.d_dst, case.d_flags))
    cp, pp = C.c_void_p(case.d_factors.data_ptr()), C.c_void_p(case.work.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    E_ARG = -1                                                   # DIN_E_ARG (include/din_hip.h)
    assert "DIN_E_ARG = -1" in open(_lib.HEADER_PATH).read()
    p, j = lib.din_rows_gray_partials, lib.din_copy_rows_u8_jitter
    big = 1 << 62
    for bad in ((None, pp, 1, 4, 16), (sp, None, 1, 4, 16), (sp, pp, -1, 4, 16), (sp, pp, 1, -4, 16), (sp, pp, 1, 4, -16),
                (sp, pp, 1, 4096, 4096), (sp, pp, 1, 1, 1 << 24), (sp, pp, 1, big, 4), (sp, pp, 1, 3, big)):
        assert p(*bad, stream) == E_ARG, bad
        assert lib.din_last_error_string()
    for bad in ((None, dp, fp, cp, pp, 1, 4, 16), (sp, None, fp, cp, pp, 1, 4, 16), (sp, dp, fp, cp, pp, -1, 4, 16),
                (sp, dp, fp, cp, pp, 1, -4, 16), (sp, dp, fp, cp, pp, 1, 4, -16), (sp, dp, fp, cp, pp, 1, 4096, 4096),
                (sp, dp, fp, cp, pp, 1, 1 << 24, 1), (sp, dp, fp, cp, pp, 1, big, 4), (sp, dp, fp, cp, pp, 1, 3, big),
                (sp, dp, fp, None, pp, 1, 4, 16), (sp, dp, fp, cp, None, 1, 4, 16)):
        assert j(*bad, stream) == E_ARG, bad
    assert "partials" in lib.din_last_error_string().decode()
    for ok in ((sp, pp, 0, 4, 16), (None, None, 0, 4, 16), (sp, pp, 1, 0, 16), (sp, pp, 1, 4, 0)):
        assert p(*ok, stream) == 0, ok                           # nothing to do: OK, no launch
    for ok in ((sp, dp, fp, cp, pp, 0, 4, 16), (None, None, None, None, None, 0, 4, 16), (sp, dp, fp, cp, pp, 1, 0, 16),
               (sp, dp, fp, cp, pp, 1, 4, 0)):
        assert j(*ok, stream) == 0, ok
    torch.cuda.synchronize()
    assert torch.equal(case.dst_buf, case.init) and bool((case.parts == SENTINEL).all()), "a refused or empty call wrote"
    with pytest.raises(_lib.DinError):                           # the workspace is sized through ops: a short one is refused there
        ops.rows_gray_partials(case.d_src, case.work[:0], 4, 16)
    with pytest.raises(_lib.DinError):
        ops.copy_rows_u8_jitter(case.d_src, case.d_dst, None, case.d_factors, None, 4, 16)
    assert (2 ** 24 - 1) * 255 < 2 ** 32                          # why 2^24 pixels: a row's whole grey sum fits 32 bits
    case.launch()
    case.verify("after the refusals")


# ---- FrameCache ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", [(3, 96, 160), (3, 13, 19)], ids=["3x96x160", "3x13x19"])
def test_build_batch_bit_exact_jitters_resident_and_uploaded_rows_and_keeps_the_slots(gpu, frame, monkeypatch):
    """a cache with room for 6 of 10 frames.  One batch inserts six and serves the other rows from the uploaded frames, with mixed flags
    and factors: every row is the model of its frame, from a slot or from an uploaded row.  A plain gather afterwards returns the
    originals: the slots hold the frames as decoded.  All-one factors issue the launches of a batch without them."""
    from din_amd import ops
    from din_amd.frame_cache import FrameCache
    calls = []
    for name in ("copy_rows_u8", "copy_rows_u8_flip", "rows_gray_partials", "copy_rows_u8_jitter"):
        monkeypatch.setattr(ops, name, (lambda real, name: lambda *a, **k: calls.append(name) or real(*a, **k))(getattr(ops, name), name))
    host = torch.randint(0, 256, (10,) + frame, generator=torch.Generator().manual_seed(11), dtype=torch.uint8)
    dev = host.to(gpu)
    fb = int(np.prod(frame))
    cache = FrameCache(gpu, frame, 6 * ((fb + 15) // 16 * 16) + 100, chunk_frames=4)
    ids = list(range(50, 60))
    order = [8, 1, 6, 6, 0, 9, 5, 7, 2, 8, 3, 4, 1]
    flip_rows = np.array([1, 1, 0, 1, 0, 1, 1, 0, 0, 0, 1, 1, 0], dtype=bool)
    factors = np.array([TRIPLES[(3 * r) % len(TRIPLES)] for r in range(len(order))], dtype=np.float32)
    assert (factors == 1).all(axis=1).any() and (factors != 1).any(axis=1).sum() >= 8

    def want_of(order, flips, factors):
        return np.stack([R.jitter(host[i].numpy(), *factors[r], mirror=bool(flips[r])) for r, i in enumerate(order)])

    batch, new = cache.build_batch([ids[i] for i in order], list(range(len(order))), dev[order].contiguous(), flip_rows=flip_rows,
                                   jitter_rows=factors)
    torch.cuda.synchronize()
    assert new == [ids[i] for i in (8, 1, 6, 0, 9, 5)] and cache.inserted == 6 and cache.table.full
    assert np.array_equal(batch.cpu().numpy(), want_of(order, flip_rows, factors))
    assert cache.flip_flags is not None and cache.flip_flags.cpu().tolist() == flip_rows.astype(int).tolist()
    assert calls == ["copy_rows_u8", "rows_gray_partials", "copy_rows_u8_jitter"]
    work = cache._gray.buf
    assert work is not None and work.numel() >= len(order) * ops.gray_partial_segments(*frame[1:])
    resident = [i for i in range(10) if cache.resident(ids[i])]
    assert sorted(resident) == [0, 1, 5, 6, 8, 9]
    got = cache.gather([ids[i] for i in resident])
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), host[resident]) and cache.flip_flags is None, "a slot holds a jittered frame"
    # resident frames (by id only) and uploaded ones mixed, jitter without any flip
    order2 = [9, 2, 0, 7, 7, 5]
    pos2 = [r for r, i in enumerate(order2) if i not in resident]
    del calls[:]
    batch2, new2 = cache.build_batch([ids[i] for i in order2], pos2, dev[[order2[r] for r in pos2]].contiguous(), jitter_rows=factors[1:7])
    torch.cuda.synchronize()
    assert new2 == [] and np.array_equal(batch2.cpu().numpy(), want_of(order2, np.zeros(6, dtype=bool), factors[1:7]))
    assert cache.flip_flags is None and cache._gray.buf is work, "the partials workspace was allocated again"
    assert calls == ["copy_rows_u8", "rows_gray_partials", "copy_rows_u8_jitter"]
    # all-one factors: the launches of a batch without them, with and without flags
    for flips, names in ((None, ["copy_rows_u8", "copy_rows_u8"]), (np.array([1, 0, 0, 1, 0, 0], dtype=bool), ["copy_rows_u8", "copy_rows_u8_flip"])):
        del calls[:]
        batch3, _ = cache.build_batch([ids[i] for i in resident], flip_rows=flips, jitter_rows=np.ones((6, 3), dtype=np.float32))
        torch.cuda.synchronize()
        assert calls == names
        assert np.array_equal(batch3.cpu().numpy(), want_of(resident, np.zeros(6, dtype=bool) if flips is None else flips, np.ones((6, 3))))
    with pytest.raises(ValueError):
        cache.build_batch([ids[i] for i in resident], jitter_rows=np.ones((5, 3), dtype=np.float32))
    with pytest.raises(ValueError):
        cache.build_batch([ids[i] for i in resident], jitter_rows=np.full((6, 3), np.nan, dtype=np.float32))


# ---- end to end through the trainers ---------------------------------------------------------------------------------------------------
SEED = 5            # FlipPlan(0.5, 5, 0): epoch 1 draws [False, True], epoch 2 [True, True] (one clip per batch) -- checked below
AMPLITUDES = (0.4, 0.4, 0.4)
JITTER_OPS = ("rows_gray_partials", "copy_rows_u8_jitter")


def _run(color_jitter, flip_prob, frame_cache_gb, stage=2, result_path=None, deterministic=False):
    """train_net over the volleyball tree of tests/golden/dataset_tree with the configuration of tests/test_gpu_flip.py (train sequence
    1: two clips; test sequence 4: one clip; 96x160, VGG16, batch size 1): stage 2 for two epochs of three-frame clips, or stage 1 for
    one epoch.  Returns what every model call received -- (training?, images, boxes) --, what the loss received (stage 1), the infos and
    the launch survey: the names of the frame-copy launches in order."""
    import din_amd.train_net as T1
    import din_amd.train_net_dynamic as T2
    from din_amd import ops
    from din_amd.base_model import Basenet_volleyball
    from din_amd.config import Config
    from din_amd.infer_model import Dynamic_volleyball
    cfg = Config("volleyball")
    cfg.data_path, cfg.train_seqs, cfg.test_seqs = os.path.join(GOLDEN, "dataset_tree", "volleyball"), [1], [4]
    cfg.backbone, cfg.image_size, cfg.out_size, cfg.emb_features = "vgg16", (96, 160), (3, 5), 512
    cfg.num_boxes, cfg.num_frames, cfg.num_before, cfg.num_after = 12, 3, 1, 1
    cfg.num_features_boxes, cfg.num_features_gcn = 64, 64
    cfg.ST_kernel_size, cfg.sampling_ratio, cfg.beta_factor, cfg.train_backbone = [(3, 3)], [1], False, not deterministic
    cfg.training_stage, cfg.batch_size, cfg.test_batch_size, cfg.max_epoch, cfg.test_interval_epoch = stage, 1, 1, stage, 1
    cfg.train_dropout_prob, cfg.train_learning_rate, cfg.lr_plan, cfg.train_random_seed = 0.0, 1e-4, {}, SEED
    cfg.result_path, cfg.deterministic = result_path, deterministic
    cfg.frame_cache_gb, cfg.num_workers, cfg.flip_prob = frame_cache_gb, 0, flip_prob
    if color_jitter != "default":
        cfg.color_jitter = color_jitter
    calls, losses, survey = [], [], []
    real_losses = T1._losses
    names = ("copy_rows_u8", "copy_rows_u8_flip") + JITTER_OPS
    real_ops = {n: getattr(ops, n) for n in names}

    def recording_losses(actions_scores, activities_scores, actions_in, activities_in, *rest):
        losses.append((actions_in.cpu().numpy().copy(), activities_in.cpu().numpy().copy()))
        return real_losses(actions_scores, activities_scores, actions_in, activities_in, *rest)

    def pre_hook(module, args):
        if isinstance(module, (Dynamic_volleyball, Basenet_volleyball)):
            images, boxes = args[0][0], args[0][1]
            assert images.dtype == torch.uint8 and images.is_cuda and tuple(images.shape[2:]) == (3, 96, 160)
            calls.append((module.training, images.cpu().numpy().copy(), boxes.cpu().numpy().copy()))

    handle = torch.nn.modules.module.register_module_forward_pre_hook(pre_hook)
    T1._losses = recording_losses
    for n in names:
        setattr(ops, n, (lambda real, n: lambda *a, **k: survey.append(n) or real(*a, **k))(real_ops[n], n))
    try:
        infos = (T2 if stage == 2 else T1).train_net(cfg)
        torch.cuda.synchronize()
    finally:
        handle.remove()
        T1._losses = real_losses
        for n in names:
            setattr(ops, n, real_ops[n])
    print(f"color_jitter {color_jitter}, flip_prob {flip_prob}, frame_cache_gb {frame_cache_gb}, stage {stage}: loss per epoch",
          [(i["train"]["loss"], i["test"]["loss"]) for i in infos])
    return dict(calls=calls, losses=losses, infos=infos, survey=survey)


def _drawn(epochs, batches=2):
    """the (contrast, brightness, saturation) factors and the flip flags of every training call, in order (batch size 1)"""
    from din_amd.frame_cache import FlipPlan, JitterPlan
    factors, flags = [], []
    for e in range(1, epochs + 1):
        je, fe = JitterPlan(AMPLITUDES, SEED, 0).epoch(e), FlipPlan(0.5, SEED, 0).epoch(e)
        for _ in range(batches):
            b, c, s = je.draw(1)[0]
            factors.append((c, b, s))
            flags.append(bool(fe.draw(1)[0]))
    return factors, flags


def _check_against(run, plain, boxes_run, factors, flags):
    """every training call received the model of the plain run's images with that call's factors (mirrored where flagged) and the boxes
    of `boxes_run`; every evaluation call exactly what the plain run's received"""
    assert len(run["calls"]) == len(plain["calls"]) == len(boxes_run["calls"])
    k = 0
    for (training, images, boxes), (training0, images0, boxes0), (_, _, boxes1) in zip(run["calls"], plain["calls"], boxes_run["calls"]):
        assert training == training0
        if training:
            flag = bool(flags[k]) if flags is not None else False
            want = np.stack([np.stack([R.jitter(f, *factors[k], mirror=flag) for f in clip]) for clip in images0])
            assert np.array_equal(images, want), f"training call {k}: the images are not the model of the plain run's, factors {factors[k]}"
            assert not np.array_equal(images, images0[..., ::-1] if flag else images0), f"training call {k} was not jittered"
            assert np.array_equal(boxes.view(np.uint32), boxes1.view(np.uint32)), f"training call {k}: boxes"
            k += 1
        else:
            assert np.array_equal(images, images0), "an evaluation clip differs from the plain run"
            assert np.array_equal(boxes.view(np.uint32), boxes0.view(np.uint32))
    return k


@pytest.fixture(scope="module")
def plain_run(gpu):
    run = _run("default", 0.0, 0)
    assert [c[0] for c in run["calls"]] == [True, True, False] * 2 and run["survey"] == []
    assert all("jittered_clips" not in i["train"] for i in run["infos"])
    return run


@pytest.fixture(scope="module")
def flip_only_run(gpu):
    """cfg.color_jitter = None, flip_prob = 0.5, the cache on: the boxes of the mirrored runs, and today's launch survey"""
    run = _run(None, 0.5, 1)
    assert not set(run["survey"]) & set(JITTER_OPS) and "copy_rows_u8_flip" in run["survey"]
    return run


@pytest.mark.parametrize("frame_cache_gb", [0, 1], ids=["cache_off", "cache_on"])
def test_train_net_stage2_jitters_every_training_clip_with_its_drawn_factors(gpu, plain_run, frame_cache_gb):
    factors, _ = _drawn(2)
    assert all(any(f != 1 for f in t) for t in factors)
    run = _run(AMPLITUDES, 0.0, frame_cache_gb)
    assert _check_against(run, plain_run, plain_run, factors, None) == 4
    assert [i["train"]["jittered_clips"] for i in run["infos"]] == [2, 2]
    assert all("jittered_clips" not in i["test"] and "flipped_clips" not in i["train"] for i in run["infos"])
    assert run["survey"].count("copy_rows_u8_jitter") == run["survey"].count("rows_gray_partials") == 4
    assert "copy_rows_u8_flip" not in run["survey"]


@pytest.mark.parametrize("frame_cache_gb", [0, 1], ids=["cache_off", "cache_on"])
def test_train_net_stage2_jitters_and_mirrors_in_one_gather(gpu, plain_run, flip_only_run, frame_cache_gb):
    factors, flags = _drawn(2)
    assert flags == [False, True, True, True]
    run = _run(AMPLITUDES, 0.5, frame_cache_gb)
    assert _check_against(run, plain_run, flip_only_run, factors, flags) == 4
    assert [i["train"]["jittered_clips"] for i in run["infos"]] == [2, 2]
    assert [i["train"]["flipped_clips"] for i in run["infos"]] == [i["train"]["flipped_clips"] for i in flip_only_run["infos"]] == [1, 2]
    assert run["survey"].count("copy_rows_u8_jitter") == 4 and "copy_rows_u8_flip" not in run["survey"]


def test_train_net_stage2_deterministic_run_jitters_the_same_bytes(gpu, plain_run, flip_only_run):
    factors, flags = _drawn(2)
    run = _run(AMPLITUDES, 0.5, 1, deterministic=True)
    assert _check_against(run, plain_run, flip_only_run, factors, flags) == 4


def test_train_net_stage2_all_one_factors_issue_todays_launches(gpu, flip_only_run):
    """amplitudes of zero draw factors of exactly 1: the launch survey is the one of the run with cfg.color_jitter = None, and so is
    every image and box"""
    run = _run((0, 0, 0), 0.5, 1)
    assert run["survey"] == flip_only_run["survey"]
    assert [i["train"]["jittered_clips"] for i in run["infos"]] == [0, 0]
    for (t, images, boxes), (t0, images0, boxes0) in zip(run["calls"], flip_only_run["calls"]):
        assert t == t0 and np.array_equal(images, images0) and np.array_equal(boxes.view(np.uint32), boxes0.view(np.uint32))


def test_train_net_stage1_jitters_images_and_leaves_labels(gpu, tmp_path):
    factors, _ = _drawn(1)
    plain = _run(None, 0.0, 0, stage=1, result_path=str(tmp_path))
    run = _run(AMPLITUDES, 0.0, 0, stage=1, result_path=str(tmp_path))
    n_train = sum(c[0] for c in plain["calls"])
    assert n_train == 2 and _check_against(run, plain, plain, factors, None) == n_train
    assert run["infos"][0]["train"]["jittered_clips"] == n_train and "jittered_clips" not in plain["infos"][0]["train"]
    assert plain["survey"] == [] and run["survey"] == list(JITTER_OPS) * n_train
    assert len(run["losses"]) == len(plain["losses"]) == len(plain["calls"])
    for (actions, activities), (actions0, activities0) in zip(run["losses"], plain["losses"]):
        assert np.array_equal(actions, actions0) and np.array_equal(activities, activities0)
