"""Frame cache on the MI355X: din_copy_rows_u8 against a host memcpy model (bit-exact, every alignment), the FrameCache round trip, and
two epochs of train_net_dynamic.train_net over tests/golden/dataset_tree with the cache on against the same run with it off."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

pytestmark = pytest.mark.gpu

GUARD, GUARD_BYTE, FILL_BYTE = 64, 0xA5, 0x3C
BYTES = (1, 15, 16, 17, 105, 46080, 84651)          # 46080 = 3x96x160, 84651 = 3x139x203 (odd)
ROWS = (1, 3, 37)


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


def _copy_case(gpu, nbytes, n, combos, rng, skip_phase):
    """one launch: n destination rows between guard bands, sources out of a pool of 16 rows (one per residue mod 16, so sources repeat as
    soon as n > 16), every third row skipped (src = 0).  `combos` yields the (src residue, dst residue) of each copied row.  Returns the
    residue pairs used; asserts the whole destination buffer against the host model."""
    from din_amd import ops
    pool_stride = nbytes + 32
    src_buf = torch.from_numpy(rng.integers(0, 256, size=16 * pool_stride + 64, dtype=np.uint8)).to(gpu)
    row_stride = GUARD + 16 + nbytes + GUARD
    dst_host = np.full(n * row_stride + 64, FILL_BYTE, dtype=np.uint8)
    dst_buf = torch.empty(dst_host.size, dtype=torch.uint8, device=gpu)
    sbase, dbase = src_buf.data_ptr(), dst_buf.data_ptr()
    pool_off = [_place(sbase, r * pool_stride, r) for r in range(16)]                # pool row r starts at residue r
    src_tab, dst_tab, used, plan = [], [], [], []
    for i in range(n):
        skipped = n > 1 and i % 3 == skip_phase
        rs, rd = (0, i % 16) if skipped else next(combos)
        doff = _place(dbase, i * row_stride + GUARD, rd)
        assert doff + nbytes + GUARD <= (i + 1) * row_stride and pool_off[rs] + nbytes <= (rs + 1) * pool_stride
        dst_host[i * row_stride:doff] = GUARD_BYTE                                    # >= 64 guard bytes below the row ...
        dst_host[doff + nbytes:(i + 1) * row_stride] = GUARD_BYTE                     # ... and above it
        src_tab.append(0 if skipped else sbase + pool_off[rs])
        dst_tab.append(dbase + doff)
        assert skipped or ((src_tab[-1] % 16, dst_tab[-1] % 16) == (rs, rd))
        if not skipped:
            used.append((rs, rd))
            plan.append((pool_off[rs], doff))
    dst_buf.copy_(torch.from_numpy(dst_host))
    want, src_host = dst_host.copy(), src_buf.cpu().numpy()
    for so, do in plan:                                                               # the host memcpy model
        want[do:do + nbytes] = src_host[so:so + nbytes]
    ops.copy_rows_u8(torch.tensor(src_tab, dtype=torch.int64, device=gpu), torch.tensor(dst_tab, dtype=torch.int64, device=gpu), nbytes)
    torch.cuda.synchronize()
    got = dst_buf.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"bytes={nbytes} n={n}: {bad.size} bytes differ, first at {bad[:4]} (row stride {row_stride})"
    return used


def test_copy_rows_bit_exact_against_host_memcpy(gpu):
    """every (bytes, n) of the lists above, twice, with the (source, destination) residues mod 16 of the copied rows walking through
    all 16 x 16 pairs; guards of 0xA5 and skipped rows must come back unchanged (the whole destination buffer is compared)"""
    def walk():
        k = 0
        while True:
            yield k % 16, (k // 16) % 16
            k += 1

    combos, seen = walk(), set()
    rng = np.random.default_rng(20240)
    for skip_phase in (1, 2):
        for nbytes in BYTES:
            for n in ROWS:
                seen.update(_copy_case(gpu, nbytes, n, combos, rng, skip_phase))
    assert len(seen) == 256, f"only {len(seen)} of the 256 residue pairs were exercised"


@pytest.mark.parametrize("nbytes,n", [(105, 4200), (46080, 900)], ids=["4200x105", "900x46080"])
def test_copy_rows_beyond_one_grid(gpu, nbytes, n):
    """more (row, segment) items than the launch has workgroups (4096): the block-stride loop"""
    def walk():
        k = 7
        while True:
            yield (5 * k) % 16, (3 * k + k // 16) % 16
            k += 1

    _copy_case(gpu, nbytes, n, walk(), np.random.default_rng(7), 1)


def test_copy_rows_refusals_and_empty_calls_launch_nothing(gpu):
    from din_amd import _lib
    lib = _lib.load()
    src = torch.arange(256, dtype=torch.uint8, device=gpu)
    dst = torch.full((256,), FILL_BYTE, dtype=torch.uint8, device=gpu)
    st = torch.tensor([src.data_ptr()], dtype=torch.int64, device=gpu)
    dt = torch.tensor([dst.data_ptr()], dtype=torch.int64, device=gpu)
    sp, dp, stream = C.c_void_p(st.data_ptr()), C.c_void_p(dt.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert _lib.DinError is not None
    E_ARG = -1                                                   # DIN_E_ARG (include/din_hip.h)
    assert "DIN_E_ARG = -1" in open(_lib.HEADER_PATH).read()
    assert lib.din_copy_rows_u8(None, dp, 1, 64, stream) == E_ARG
    assert lib.din_copy_rows_u8(sp, None, 1, 64, stream) == E_ARG
    assert lib.din_copy_rows_u8(sp, dp, -1, 64, stream) == E_ARG
    assert lib.din_copy_rows_u8(sp, dp, 1, -64, stream) == E_ARG
    assert lib.din_last_error_string()
    assert lib.din_copy_rows_u8(sp, dp, 0, 64, stream) == 0      # n == 0: OK, nothing to do
    assert lib.din_copy_rows_u8(None, None, 0, 64, stream) == 0
    assert lib.din_copy_rows_u8(sp, dp, 1, 0, stream) == 0       # bytes == 0: OK, nothing to do
    torch.cuda.synchronize()
    assert bool((dst == FILL_BYTE).all()), "a refused or empty call wrote to the destination"
    assert lib.din_copy_rows_u8(sp, dp, 1, 256, stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(dst, src)


def test_copy_rows_is_capturable(gpu):
    """one plain launch on the given stream: it can be recorded into a HIP graph and replayed"""
    from din_amd import ops
    src = torch.randint(0, 256, (3, 1000), dtype=torch.uint8, device=gpu)
    dst = torch.zeros_like(src)
    st = torch.tensor([src[i].data_ptr() for i in (2, 0, 2)], dtype=torch.int64, device=gpu)
    dt = torch.tensor([dst[i].data_ptr() for i in range(3)], dtype=torch.int64, device=gpu)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.copy_rows_u8(st, dt, 1000)
    dst.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(dst, src[[2, 0, 2]])


# ---- FrameCache ------------------------------------------------------------------------------------------------------------------------
FRAME = (3, 96, 160)


def _frames(gpu, count=10):
    g = torch.Generator().manual_seed(11)
    host = torch.randint(0, 256, (count,) + FRAME, generator=g, dtype=torch.uint8)
    return host, host.to(gpu)


def test_frame_cache_round_trip_across_slabs(gpu):
    from din_amd.frame_cache import FrameCache
    host, dev = _frames(gpu)
    cache = FrameCache(gpu, FRAME, 1 << 30, chunk_frames=4)
    assert cache.bytes == 0 and not cache.slabs                  # nothing is allocated before the first frame arrives
    ids = [100 + 7 * i for i in range(10)]                       # frame ids are names, not slot numbers
    assert cache.insert(ids[:6], dev[:6].contiguous()) == ids[:6] and len(cache.slabs) == 2
    assert cache.insert(ids[5:], dev[5:].contiguous()) == ids[5:] and len(cache.slabs) == 3      # id 135 again: a hit, no second slot
    assert cache.inserted == 10 and cache.bytes == 12 * 46080 and cache.table.stride == 46080
    order = [9, 0, 3, 3, 7, 1, 9, 4, 8, 2, 6, 5, 0]
    got = cache.gather([ids[i] for i in order])
    torch.cuda.synchronize()
    assert got.shape == (len(order),) + FRAME and got.dtype == torch.uint8 and torch.equal(got.cpu(), host[order])
    assert cache.misses == 0 and cache.hits == 1 + len(order)
    with pytest.raises(KeyError):
        cache.gather([ids[0], 5])


def test_full_cache_serves_the_rest_from_the_uploaded_rows(gpu):
    from din_amd.frame_cache import FrameCache
    host, dev = _frames(gpu)
    cache = FrameCache(gpu, FRAME, 6 * 46080 + 100, chunk_frames=4)
    ids = list(range(50, 60))
    assert cache.insert(ids, dev) == ids[:6]                     # a capacity of 6 frames: the 7th onward are not resident
    assert [cache.resident(i) for i in ids] == [True] * 6 + [False] * 4 and cache.bytes == 6 * 46080 and len(cache.slabs) == 2
    order = [8, 1, 6, 6, 0, 9, 5, 7, 2, 8]                       # a mixed batch: resident frames by id only, the others uploaded
    pos = [r for r, i in enumerate(order) if i >= 6]
    rows = dev[[order[r] for r in pos]].contiguous()
    batch, new = cache.build_batch([ids[i] for i in order], pos, rows)
    torch.cuda.synchronize()
    assert new == [] and cache.inserted == 6
    assert torch.equal(batch.cpu(), host[order]), "the mixed batch differs from the uncached one"


# ---- end to end through the trainer ----------------------------------------------------------------------------------------------------
STEPS_PER_EPOCH = 3                                              # 2 training clips at batch size 1, then 1 validation clip


def _run_two_epochs(frame_cache_gb, num_workers, count_calls=True):
    """train_net over the volleyball tree of tests/golden/dataset_tree (train sequence 1: two clips; test sequence 4: one clip; three
    frames a clip at 96x160, VGG16).  Returns (sha1 of the images tensor of every model call, decode calls per step index, the caches'
    (hits, misses, inserted) seen at every model call, the infos)."""
    from din_amd import frame_cache as FC, volleyball as V
    from din_amd.config import Config
    from din_amd.infer_model import Dynamic_volleyball
    from din_amd.train_net_dynamic import train_net
    cfg = Config("volleyball")
    cfg.data_path, cfg.train_seqs, cfg.test_seqs = os.path.join(GOLDEN, "dataset_tree", "volleyball"), [1], [4]
    cfg.backbone, cfg.image_size, cfg.out_size, cfg.emb_features = "vgg16", (96, 160), (3, 5), 512
    cfg.num_boxes, cfg.num_frames, cfg.num_before, cfg.num_after = 12, 3, 1, 1
    cfg.num_features_boxes, cfg.num_features_gcn = 64, 64
    cfg.ST_kernel_size, cfg.sampling_ratio, cfg.beta_factor, cfg.train_backbone = [(3, 3)], [1], False, True
    cfg.training_stage, cfg.batch_size, cfg.test_batch_size, cfg.max_epoch, cfg.test_interval_epoch = 2, 1, 1, 2, 1
    cfg.train_dropout_prob, cfg.train_learning_rate, cfg.lr_plan, cfg.train_random_seed = 0.0, 1e-4, {}, 5
    cfg.result_path = None
    cfg.frame_cache_gb, cfg.num_workers = frame_cache_gb, num_workers
    sums, calls, counters, caches = [], [], [], []
    real_load, real_init = V.load_frame_u8, FC.FrameCache.__init__

    def counting_load(path, size):
        calls.append(len(sums))                                  # the number of model calls made so far
        return real_load(path, size)

    def recording_init(self, *a, **kw):
        real_init(self, *a, **kw)
        caches.append(self)

    def pre_hook(module, args):
        if isinstance(module, Dynamic_volleyball):
            images = args[0][0]
            assert images.dtype == torch.uint8 and images.is_cuda and tuple(images.shape) == (1, 3, 3, 96, 160)
            counters.append(tuple(sum(getattr(c, k) for c in caches) for k in ("hits", "misses", "inserted")))
            sums.append(hashlib.sha1(images.cpu().numpy().tobytes()).hexdigest())

    handle = torch.nn.modules.module.register_module_forward_pre_hook(pre_hook)
    if count_calls:
        V.load_frame_u8 = counting_load
    FC.FrameCache.__init__ = recording_init
    try:
        infos = train_net(cfg)
        torch.cuda.synchronize()
    finally:
        handle.remove()
        V.load_frame_u8, FC.FrameCache.__init__ = real_load, real_init
    counters.append(tuple(sum(getattr(c, k) for c in caches) for k in ("hits", "misses", "inserted")))
    return sums, calls, counters, infos, caches


@pytest.fixture(scope="module")
def uncached_run(gpu):
    return _run_two_epochs(0, 0)


def test_train_net_sees_the_same_images_with_the_cache(gpu, uncached_run):
    """two epochs with cfg.frame_cache_gb = 1 against two epochs with 0, same seed, num_workers = 0: every model call receives the same
    images tensor, step for step; in the second cached epoch nothing is decoded and the caches report only hits.

    The per-epoch losses are printed, not asserted equal: the step is not bit-reproducible run to run on this configuration -- the
    weight-gradient and DIN-walk backward kernels add fp32 partial sums with atomics, whose order changes the last bits (the existing
    trainer tests compare such runs at 1e-4, tests/test_gpu_din_model.py: test_captured_step_matches_eager)."""
    want, calls0, counters0, infos0, caches0 = uncached_run
    assert len(want) == 2 * STEPS_PER_EPOCH and not caches0 and len(calls0) == 2 * 9       # uncached: all 9 frames decoded every epoch
    assert len(set(want[:STEPS_PER_EPOCH])) == STEPS_PER_EPOCH                               # three different clips
    got, calls, counters, infos, caches = _run_two_epochs(1, 0)
    print("loss per epoch, cache off:", [(i["train"]["loss"], i["test"]["loss"]) for i in infos0])
    print("loss per epoch, cache on: ", [(i["train"]["loss"], i["test"]["loss"]) for i in infos])
    assert got == want
    assert len(caches) == 2 and all(c.device.type == "cuda" for c in caches)                # one for training, one for validation
    # a decode call made after the last model call of epoch 1 started belongs to epoch 2 (the feed fetches at most one batch ahead, and
    # the first batch of an epoch is fetched after the previous pass has ended)
    assert len([c for c in calls if c < STEPS_PER_EPOCH]) == 9 and [c for c in calls if c >= STEPS_PER_EPOCH] == []
    end1, end2 = counters[STEPS_PER_EPOCH], counters[-1]         # counters[k]: before model call k, so [3] already holds call 3's batch
    start2 = counters[STEPS_PER_EPOCH - 1]                       # after every batch of epoch 1, before any of epoch 2
    assert start2 == (0, 9, 9)                                   # epoch 1: nine rows, all missed and inserted
    assert end2 == (9, 9, 9) and end1[1] == 9                    # epoch 2: only hits
    assert sum(c.bytes for c in caches) == 2 * 64 * 46080        # one slab of 64 slots each, far below the 1 GB allowed


def test_two_loader_workers_feed_the_same_images_through_the_cache(gpu, uncached_run):
    """cfg.num_workers = 2 with the cache on: forked workers decode (they never open the GPU) and read the resident flags the main
    process sets; the model receives the same images as without workers and without the cache.  A stuck worker would raise after
    frame_cache.LOADER_TIMEOUT_S instead of hanging.  Measured: 5.6 s run alone, 32.7 s at the end of the whole GPU suite -- the four
    loader passes fork eight workers in all, and a fork costs seconds once the parent process has mapped everything the suite loads."""
    want = uncached_run[0]
    got, _, counters, infos, caches = _run_two_epochs(1, 2, count_calls=False)
    assert got == want
    assert counters[-1][2] == 9 and counters[-1][0] + counters[-1][1] == 18
    assert counters[-1][1] == 9                                  # epoch 2 had only hits here too: every frame was resident by then
