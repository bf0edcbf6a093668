"""bf16 storage of the box-feature cache on the MI355X: din_feat_rows_bf16 against a numpy model (bit-exact: a copy and
round-to-nearest-even are fully defined; every row kind, guard bands), the FeatureCache round trip with dtype=torch.bfloat16,
Dynamic_volleyball under backbone_dtype='bf16' fed through caches of both dtypes, and two epochs of train_net_dynamic.train_net with
cfg.feature_cache_dtype = 'bf16' against 'fp32'."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.test_feature_cache_bf16_cpu import fp32_values, rne_bf16_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

pytestmark = pytest.mark.gpu

GUARD, GUARD_BYTE = 64, 0xA5
# row i is of kind KINDS[i % len(KINDS)].  SLOT_*: a resident row (bf16 at src, copied), its boxes compared with stored ones that are equal,
# differ in the first / the last float, or are equal with the flag already 1; SLOT_PLAIN has no stored boxes to compare.  ROW_*: a row
# the trunk computed (fp32 at src, rounded), alone, kept, or two rows reading one source of which the second is kept.
SKIP, SLOT_EQ, SLOT_FIRST, SLOT_LAST, SLOT_PRESET, SLOT_PLAIN, ROW, ROW_KEEP, ROW_SHARED_A, ROW_SHARED_B = range(10)
ALL_KINDS = tuple(range(10))
SLOT_KINDS = (SKIP, SLOT_EQ, SLOT_FIRST, SLOT_LAST, SLOT_PRESET, SLOT_PLAIN)
COMPARED, COMPUTED, KEPT = (SLOT_EQ, SLOT_FIRST, SLOT_LAST, SLOT_PRESET), (ROW, ROW_KEEP, ROW_SHARED_A, ROW_SHARED_B), (ROW_KEEP, ROW_SHARED_B)


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from din_amd import _lib
    _lib.load()
    return torch.device("cuda")


class _Case:
    """tests/test_gpu_feature_cache.py's harness for rows of `ne` bf16 values: n rows of the kinds above, every written buffer between
    guard bands, and the numpy model of what one din_feat_rows_bf16 launch leaves in them.  Buffers (host image `*_h`, device tensor
    `*_d`): slots16 (n bf16 source rows, any bit pattern: they are copied), rows32 (n fp32 source rows, test_feature_cache_bf16_cpu's
    values), dst (n rows), slot (n slots of 2 * ne + box_bytes bytes; only the kept rows name theirs), stored (n rows of box_bytes),
    flags (n bytes)."""

    def __init__(self, gpu, n, ne, box_bytes, seed, kinds=ALL_KINDS, values=None):
        rng = np.random.default_rng(seed)
        self.n, self.ne, self.rb, self.bb = n, ne, 2 * ne, box_bytes
        rb = self.rb
        self.kinds = kinds = [kinds[i % len(kinds)] for i in range(n)]
        self.slots16_h = rng.integers(0, 1 << 16, size=(n, ne), dtype=np.uint16)
        pool = fp32_values(min(n * ne, 1 << 18), seed) if values is None else values
        self.rows32_h = np.resize(pool, (n, ne))
        self.boxes_h = rng.integers(0, 256, size=(n, box_bytes), dtype=np.uint8)
        self.dstride, self.sstride, self.bstride = rb + 2 * GUARD, rb + box_bytes + 2 * GUARD, box_bytes + 2 * GUARD
        self.dst_h = np.full(n * self.dstride, GUARD_BYTE, dtype=np.uint8)
        self.slot_h = np.full(n * self.sstride, GUARD_BYTE, dtype=np.uint8)
        self.stored_h = np.full(n * self.bstride, GUARD_BYTE, dtype=np.uint8)
        self.flags_h = np.full(n + 2 * GUARD, GUARD_BYTE, dtype=np.uint8)
        self.flags_h[GUARD:GUARD + n] = 0                            # the host clears the flags at the start of a pass
        for i, k in enumerate(kinds):
            self.dst_h[i * self.dstride + GUARD:i * self.dstride + GUARD + rb] = 0x3C
            self.slot_h[i * self.sstride + GUARD:i * self.sstride + GUARD + rb + box_bytes] = 0x5A
            st = self.boxes_h[i].copy()
            if k == SLOT_FIRST:
                st[3] ^= 0x80                                        # one bit of the first float (its sign)
            elif k == SLOT_LAST:
                st[box_bytes - 4] ^= 0x01                            # the lowest bit of the last float
            self.stored_h[i * self.bstride + GUARD:i * self.bstride + GUARD + box_bytes] = st
            if k == SKIP:
                self.flags_h[GUARD + i] = 0x77                       # must come back untouched
            elif k == SLOT_PRESET:
                self.flags_h[GUARD + i] = 1                          # the kernel never writes 0
        dev = lambda a: torch.from_numpy(a).to(gpu)
        self.slots16_d, self.rows32_d, self.boxes_d = dev(self.slots16_h.view(np.int16)), dev(self.rows32_h), dev(self.boxes_h)
        self.dst_d, self.slot_d, self.stored_d, self.flags_d = dev(self.dst_h), dev(self.slot_h), dev(self.stored_h), dev(self.flags_h)
        self.rounded_h = rne_bf16_bits(self.rows32_h).reshape(n, ne) if not np.isnan(self.rows32_h).any() else None
        src, dst, keep, ref, f32 = [], [], [], [], []
        for i, k in enumerate(kinds):
            s = i - 1 if k == ROW_SHARED_B else i                    # ROW_SHARED_B reads the row ROW_SHARED_A reads
            computed = k in COMPUTED
            src.append(0 if k == SKIP else self.rows32_d.data_ptr() + s * ne * 4 if computed else self.slots16_d.data_ptr() + s * rb)
            f32.append(int(computed))
            dst.append(self.dst_d.data_ptr() + i * self.dstride + GUARD)
            keep.append(self.slot_d.data_ptr() + i * self.sstride + GUARD if k in KEPT else 0)
            ref.append(self.stored_d.data_ptr() + i * self.bstride + GUARD if k in COMPARED else 0)
        assert all(a % 16 == 0 for a in src + dst + keep + ref) and self.boxes_d.data_ptr() % 16 == 0
        tab = lambda v: torch.tensor(v, dtype=torch.int64, device=gpu)
        self.src_t, self.dst_t, self.keep_t, self.ref_t, self.f32_t = tab(src), tab(dst), tab(keep), tab(ref), tab(f32)
        self.flags_view = self.flags_d[GUARD:GUARD + n]
        self.untouched = set(i for i, k in enumerate(kinds) if k == SKIP)

    def model(self):
        """(dst, slot, flags) as the launch leaves them; rows in self.untouched keep what they held"""
        want_dst, want_slot, want_flags = self.dst_h.copy(), self.slot_h.copy(), self.flags_h.copy()
        for i, k in enumerate(self.kinds):
            if i in self.untouched:
                continue
            s = i - 1 if k == ROW_SHARED_B else i
            row = (self.rounded_h[s] if k in COMPUTED else self.slots16_h[s]).view(np.uint8)
            want_dst[i * self.dstride + GUARD:i * self.dstride + GUARD + self.rb] = row
            if k in KEPT:
                at = i * self.sstride + GUARD
                want_slot[at:at + self.rb] = row
                want_slot[at + self.rb:at + self.rb + self.bb] = self.boxes_h[i]
            if k in (SLOT_FIRST, SLOT_LAST):
                want_flags[GUARD + i] = 1
        return want_dst, want_slot, want_flags

    def launch(self, src_f32=True):
        from din_amd import ops
        ops.feat_rows_bf16(self.src_t, self.dst_t, self.ne, self.keep_t, self.ref_t, self.boxes_d, self.flags_view, self.bb,
                           self.f32_t if src_f32 else None)

    def reset(self):
        for d, h in ((self.dst_d, self.dst_h), (self.slot_d, self.slot_h), (self.flags_d, self.flags_h)):
            d.copy_(torch.from_numpy(h))

    def read(self):
        torch.cuda.synchronize()
        return self.dst_d.cpu().numpy(), self.slot_d.cpu().numpy(), self.flags_d.cpu().numpy()

    def verify(self, what=""):
        got = self.read()
        inputs = ((self.stored_d, self.stored_h), (self.slots16_d, self.slots16_h.view(np.int16).reshape(-1)),
                  (self.rows32_d.view(torch.int32), self.rows32_h.view(np.int32).reshape(-1)), (self.boxes_d, self.boxes_h.reshape(-1)))
        pairs = list(zip(("dst", "slot", "flags"), got, self.model())) + \
            [(name, d.cpu().numpy().reshape(-1), h) for name, (d, h) in zip(("stored boxes", "bf16 sources", "fp32 sources", "boxes"), inputs)]
        for name, g, want in pairs:
            bad = np.flatnonzero(g.reshape(-1) != want.reshape(-1))
            assert bad.size == 0, f"{what} row_elems={self.ne} box_bytes={self.bb} n={self.n}: {name}: {bad.size} elements differ, first at {bad[:4]}"

    def verify_untouched(self, what):
        for name, got, want in zip(("dst", "slot", "flags"), self.read(), (self.dst_h, self.slot_h, self.flags_h)):
            assert np.array_equal(got, want), f"{what}: wrote to {name}"


def _row_elems():
    from din_amd import ops
    seg = ops.FEAT_ROWS_SEGMENT // 2                                 # values of one work item: 8192
    assert seg == 8192
    return (8, seg - 8, seg, seg + 8, 3 * seg + 264)


@pytest.mark.parametrize("box_bytes", [16, 192])
def test_feat_rows_bf16_bit_exact_against_numpy_model(gpu, box_bytes):
    """n = 10 rows, one of every kind, at row sizes of one vector and around the segment size: destinations, slots with their boxes
    trailer and flags against the model, guard bands included, and every input buffer unchanged"""
    for j, ne in enumerate(_row_elems()):
        case = _Case(gpu, 10, ne, box_bytes, seed=100 * box_bytes + j)
        case.launch()
        case.verify()


def test_feat_rows_bf16_beyond_one_grid(gpu):
    """2100 rows of two segments each: more (row, segment) items than the launch has workgroups (4096), all row kinds repeating"""
    case = _Case(gpu, 2100, 8200, 16, seed=3)
    case.launch()
    case.verify()


def test_feat_rows_bf16_without_src_f32_is_feat_rows_at_two_bytes_a_value(gpu):
    """src_f32 null: every row is a slot's, and the launch leaves what din_feat_rows leaves at row_bytes = 2 * row_elems on the same
    tables (which is also what the model says)"""
    from din_amd import ops
    case = _Case(gpu, 12, 8200, 192, seed=4, kinds=SLOT_KINDS)
    case.launch(src_f32=False)
    case.verify("src_f32 null")
    got = case.read()
    case.reset()
    ops.feat_rows(case.src_t, case.dst_t, 2 * case.ne, case.keep_t, case.ref_t, case.boxes_d, case.flags_view, case.bb)
    for name, a, b in zip(("dst", "slot", "flags"), got, case.read()):
        assert np.array_equal(a, b), f"{name} differs from din_feat_rows"
    case.reset()
    case.launch()                                                    # and an all-zero src_f32 table is the null one
    case.verify("src_f32 all zero")


def test_feat_rows_bf16_without_keep_and_ref_tables_rounds_and_gathers(gpu):
    from din_amd import ops
    case = _Case(gpu, 10, 264, 16, seed=8)
    ops.feat_rows_bf16(case.src_t, case.dst_t, case.ne, src_f32=case.f32_t)
    want_dst, _, _ = case.model()
    got = case.read()
    assert np.array_equal(got[0], want_dst) and np.array_equal(got[1], case.slot_h) and np.array_equal(got[2], case.flags_h)


def test_feat_rows_bf16_nan_and_subnormal_inputs(gpu):
    """outside the integer model: a NaN stays a NaN (its payload is the hardware's business), and a subnormal becomes what the cast on
    the device makes of it"""
    ne = 8192 + 8
    x = fp32_values(ne, seed=9)
    tiny = np.array([1e-39, -1e-39, 1.4e-45, -1.4e-45, 2.0 ** -127, 2.0 ** -133 * 1.5, 1.1754942e-38, -1.1754942e-38], dtype=np.float32)
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0x7F80FFFF], dtype=np.uint32).view(np.float32)
    x[5:5 + len(tiny)], x[ne - 20:ne - 20 + len(tiny)] = tiny, -tiny
    x[100:100 + len(nans)], x[8190:8190 + len(nans)] = nans, nans
    case = _Case(gpu, 2, ne, 16, seed=9, kinds=(ROW_KEEP, ROW), values=x)
    case.launch()
    torch.cuda.synchronize()
    want = case.rows32_d.to(torch.bfloat16).view(torch.int16).cpu().numpy().view(np.uint16)         # [2, ne], the device's own cast
    isnan = np.isnan(case.rows32_h)
    assert isnan.sum() == 4 * len(nans)
    for i in range(2):
        got = case.dst_d[i * case.dstride + GUARD:i * case.dstride + GUARD + case.rb].cpu().numpy().view(np.uint16)
        assert np.array_equal(np.isnan(torch.from_numpy(got.view(np.int16)).view(torch.bfloat16).float().numpy()), isnan[i])
        assert np.array_equal(got[~isnan[i]], want[i][~isnan[i]]), f"row {i}"
        normal = ~isnan[i] & ~((np.abs(case.rows32_h[i]) < 2.0 ** -126) & (case.rows32_h[i] != 0))
        assert np.array_equal(got[normal], rne_bf16_bits(case.rows32_h[i][normal]))
    kept = case.slot_d[GUARD:GUARD + case.rb].cpu().numpy()
    assert np.array_equal(kept, case.dst_d[GUARD:GUARD + case.rb].cpu().numpy())                      # the slot holds the very same bits
    assert (case.dst_d[:GUARD] == GUARD_BYTE).all() and (case.dst_d[-GUARD:] == GUARD_BYTE).all()


def test_feat_rows_bf16_refusals_and_empty_calls_write_nothing(gpu):
    from din_amd import _lib
    lib = _lib.load()
    case = _Case(gpu, 10, 24, 16, seed=5)
    p = lambda t: C.c_void_p(t.data_ptr())
    src, dst, keep, ref, f32 = p(case.src_t), p(case.dst_t), p(case.keep_t), p(case.ref_t), p(case.f32_t)
    boxes, flags = p(case.boxes_d), p(case.flags_view)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    E_ARG = -1                                                   # DIN_E_ARG (include/din_hip.h)
    assert "DIN_E_ARG = -1" in open(_lib.HEADER_PATH).read()
    call = lib.din_feat_rows_bf16
    refused = [
        (src, dst, keep, ref, f32, boxes, flags, 10, 20, 16, stream),                                # row_elems not a multiple of 8
        (src, dst, keep, ref, f32, boxes, flags, 10, 4, 16, stream),
        (src, dst, keep, ref, f32, boxes, flags, 10, 24, 8, stream),                                 # box_bytes not a multiple of 16
        (src, dst, keep, ref, f32, C.c_void_p(case.boxes_d.data_ptr() + 4), flags, 10, 24, 16, stream),   # boxes misaligned
        (src, dst, keep, ref, f32, boxes, flags, -1, 24, 16, stream),
        (src, dst, keep, ref, f32, boxes, flags, 10, -24, 16, stream),
        (src, dst, keep, ref, f32, boxes, flags, 10, 24, -16, stream),
        (None, dst, keep, ref, f32, boxes, flags, 10, 24, 16, stream),
        (src, None, keep, ref, f32, boxes, flags, 10, 24, 16, stream),
        (src, dst, keep, None, f32, None, flags, 10, 24, 16, stream),                                # keep without boxes
        (src, dst, None, ref, f32, boxes, None, 10, 24, 16, stream),                                 # ref_boxes without flags
    ]
    for args in refused:
        assert call(*args) == E_ARG, args[7:10]
        assert b"feat_rows_bf16" in lib.din_last_error_string()
    assert call(src, dst, keep, ref, f32, boxes, flags, 0, 24, 16, stream) == 0                      # n == 0: OK, nothing to do
    assert call(None, None, None, None, None, None, None, 0, 24, 16, stream) == 0
    case.verify_untouched("a refused or empty call")
    assert call(src, dst, keep, ref, f32, boxes, flags, 10, 24, 16, stream) == 0
    case.verify("after the refusals")


def test_feat_rows_bf16_leaves_a_row_with_a_misaligned_address_alone(gpu):
    """the tables live on the device, so the host cannot refuse them: a row whose src / dst / keep / ref address is no multiple of 16 is
    skipped like a row with src = 0 -- one row for each table, a computed and a resident source among them"""
    case = _Case(gpu, 20, 8200, 16, seed=6)
    case.src_t[ROW] += 8
    case.src_t[SLOT_PLAIN] += 2
    case.dst_t[10 + ROW_SHARED_A] += 8
    case.keep_t[ROW_KEEP] += 4
    case.ref_t[SLOT_FIRST] += 8
    case.untouched |= {ROW, SLOT_PLAIN, 10 + ROW_SHARED_A, ROW_KEEP, SLOT_FIRST}
    case.launch()
    case.verify()


def test_feat_rows_bf16_is_capturable(gpu):
    """one plain launch on the given stream: it can be recorded into a HIP graph and replayed"""
    case = _Case(gpu, 10, 8192 + 8, 192, seed=7)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        case.launch()
    case.reset()
    torch.cuda.synchronize()
    g.replay()
    case.verify("replay")


def test_linear_takes_a_bf16_operand_only_as_lowp(gpu):
    """a bf16 x is the tensor lowp would have made: same y bit for bit, no copy of it saved; without effective lowp it is refused"""
    from din_amd import ops
    g = torch.Generator().manual_seed(2)
    x = torch.randn((3, 7, 200), generator=g).to(gpu)
    w = (torch.randn((64, 200), generator=g) * 0.1).to(gpu).requires_grad_(True)
    b = torch.randn(64, generator=g).to(gpu)
    x16 = x.to(torch.bfloat16)
    y32 = ops.linear(x, w, b, lowp=True)
    y16 = ops.linear(x16, w, b, lowp=True)
    assert y16.dtype == torch.float32 and y16.shape == (3, 7, 64) and torch.equal(y16, y32)
    node = y16.grad_fn
    while not hasattr(node, "saved_tensors"):                        # (through the views linear() makes of GridConvFunction's result)
        node = node.next_functions[0][0]
    assert node.saved_tensors[0].dtype == torch.bfloat16 and node.saved_tensors[0].data_ptr() == x16.data_ptr()
    y16.sum().backward()
    g16, w.grad = w.grad.clone(), None
    y32.sum().backward()
    # the same kernel on the same bf16 operands; only the order of its fp32 partial sums may differ: 21 rows of |x| <= 6, each addition
    # rounding by at most 2^-24 of a sum below 126
    assert (g16 - w.grad).abs().max() <= 21 * 126 * 2.0 ** -24
    for kw in (dict(), dict(split=True)):
        with pytest.raises(ValueError):
            ops.linear(x16, w, b, **kw)
    with pytest.raises(ValueError):
        ops.linear(x16[..., :100], w[:60, :100].detach(), None, lowp=True)                           # cin = 100, cout = 60: lowp is not in effect


# ---- FeatureCache(dtype=torch.bfloat16) -------------------------------------------------------------------------------------------------
NE, RB, BB = 400, 800, 192                                       # 400 features (1600 bytes as fp32, 800 stored), 12 boxes
SLOT = RB + BB


def _bits(t):
    return t.contiguous().view(torch.int16).cpu()


def _feature_rows(gpu, count=10):
    g = torch.Generator().manual_seed(13)
    rows, boxes = torch.randn((count, NE), generator=g), torch.rand((count, BB // 4), generator=g) * 40
    return rows, rows.to(torch.bfloat16), boxes, rows.to(gpu), boxes.to(gpu)


def test_bf16_feature_cache_round_trip_across_slabs(gpu):
    from din_amd.feature_cache import FeatureCache
    rows, rows16, boxes, drows, dboxes = _feature_rows(gpu)
    assert np.array_equal(_bits(rows16).numpy().view(np.uint16), rne_bf16_bits(rows.numpy()))
    cache = FeatureCache(gpu, RB, BB, 1 << 30, chunk_frames=4, dtype=torch.bfloat16)
    ids = [100 + 7 * i for i in range(10)]
    out, new = cache.rows(ids[:6], dboxes[:6], range(6), drows[:6].contiguous())
    assert out.dtype == torch.bfloat16 and out.shape == (6, NE)
    assert new == ids[:6] and len(cache.slabs) == 2 and torch.equal(_bits(out), _bits(rows16[:6]))
    out, new = cache.rows(ids[3:], dboxes[3:], range(3, 7), drows[6:].contiguous())                  # 3..5 resident, 6..9 computed
    assert new == ids[6:] and len(cache.slabs) == 3 and torch.equal(_bits(out), _bits(rows16[3:]))
    assert cache.inserted == 10 and cache.bytes == 12 * SLOT and cache.table.stride == SLOT and (cache.hits, cache.misses) == (3, 10)
    order = [9, 0, 3, 3, 7, 1, 9, 4, 8, 2, 6, 5, 0]
    out, new = cache.rows([ids[i] for i in order], dboxes[order])
    assert new == [] and out.shape == (len(order), NE) and out.dtype == torch.bfloat16 and torch.equal(_bits(out), _bits(rows16[order]))
    cache.check()
    for i in (0, 5, 9):                                          # the slot: the rounded row, then the frame's boxes
        slab, off = cache.table.locate(cache.table.slot_of[ids[i]])
        got = cache.slabs[slab][off:off + SLOT].cpu().numpy()
        assert got[:RB].tobytes() == _bits(rows16[i]).numpy().tobytes() and got[RB:].tobytes() == boxes[i].numpy().tobytes()
    with pytest.raises(KeyError):
        cache.rows([ids[0], 5], dboxes[:2])
    with pytest.raises(ValueError):                              # the computed rows arrive as fp32, not already rounded
        cache.rows([77], dboxes[:1], [0], drows[:1].to(torch.bfloat16))


def test_bf16_feature_cache_duplicates_and_a_full_cache(gpu):
    from din_amd.feature_cache import FeatureCache
    rows, rows16, boxes, drows, dboxes = _feature_rows(gpu)
    cache = FeatureCache(gpu, RB, BB, 1 << 30, chunk_frames=4, dtype=torch.bfloat16)
    out, new = cache.rows([20, 21, 20], dboxes[[0, 1, 0]].contiguous(), [0, 1, 2], drows[[0, 1, 5]].contiguous())
    assert new == [20, 21] and cache.inserted == 2 and torch.equal(_bits(out), _bits(rows16[[0, 1, 0]]))
    out, _ = cache.rows([20, 21], dboxes[:2])
    assert torch.equal(_bits(out), _bits(rows16[:2]))
    cache.check()
    cache = FeatureCache(gpu, RB, BB, 6 * SLOT + 100, chunk_frames=4, dtype=torch.bfloat16)
    ids = list(range(50, 60))
    out, new = cache.rows(ids, dboxes, range(10), drows)
    assert new == ids[:6] and torch.equal(_bits(out), _bits(rows16))     # a capacity of 6 slots: the 7th onward are served, not kept
    assert [cache.resident(i) for i in ids] == [True] * 6 + [False] * 4 and cache.bytes == 6 * SLOT and len(cache.slabs) == 2
    order = [8, 1, 6, 6, 0, 9, 5, 7, 2, 8]                       # a mixed batch: resident frames by id only, the others computed
    pos = [r for r, i in enumerate(order) if i >= 6]
    out, new = cache.rows([ids[i] for i in order], dboxes[order], pos, drows[[order[r] for r in pos]].contiguous())
    assert new == [] and cache.inserted == 6 and torch.equal(_bits(out), _bits(rows16[order]))
    cache.check()
    with pytest.raises(KeyError):
        cache.rows([ids[7]], dboxes[7:8])


def test_bf16_feature_cache_check_raises_for_a_tampered_trailer(gpu):
    from din_amd.feature_cache import FeatureCache
    rows, rows16, boxes, drows, dboxes = _feature_rows(gpu)
    cache = FeatureCache(gpu, RB, BB, 1 << 30, chunk_frames=4, dtype=torch.bfloat16)
    ids = list(range(30, 40))
    cache.rows(ids, dboxes, range(10), drows)
    cache.check()                                                # inserts compare nothing
    slab, off = cache.table.locate(cache.table.slot_of[34])
    cache.slabs[slab][off + RB + 17] ^= 0x40                     # one bit of the boxes stored with frame 34
    out, _ = cache.rows(ids, dboxes)
    assert torch.equal(_bits(out), _bits(rows16))                # the rows are served all the same; the pass ends with the error
    with pytest.raises(RuntimeError) as e:
        cache.check()
    assert "(4, 34)" in str(e.value) and "1 rows" in str(e.value)
    cache.check()                                                # the flags were cleared
    cache.slabs[slab][off + RB + 17] ^= 0x40
    cache.rows(ids, dboxes)
    cache.check()


# ---- through the model ------------------------------------------------------------------------------------------------------------------
def test_dynamic_volleyball_sees_the_same_bf16_operand_through_either_cache(gpu, monkeypatch):
    """the same clips through a frozen bf16 VGG16 Dynamic_volleyball in eval(): as an images tensor, through a cache of fp32 rows and
    through a cache of bf16 rows, each cache all missed and then all resident.  What fc_emb_1 receives is, after .to(bfloat16) (its GEMM's
    own first step on an fp32 tensor), bit-identical in all five calls; the bf16 cache hands it over as bf16; the outputs of the two
    caches are bit-identical; the backbone does not run on the resident passes."""
    from din_amd import infer_model as IM, ops
    from din_amd.feature_cache import FeatureCache, FrameRefs, row_and_box_bytes
    from din_amd.train_net_dynamic import SyntheticVolleyball, build_model
    from tests.test_gpu_feature_cache import _model_cfg
    cfg = _model_cfg("dynamic_volleyball")
    cfg.backbone_dtype = "bf16"
    torch.manual_seed(3)
    model = build_model(cfg).to(gpu).eval()
    clips = [SyntheticVolleyball(cfg, length=2, seed=4)[i] for i in range(2)]
    images = torch.stack([c[0] for c in clips]).to(gpu)          # uint8 [2, 3, 3, 96, 160]
    boxes = torch.stack([c[1] for c in clips]).to(gpu)
    B, T = 2, 3
    seen, calls = [], []
    real_linear, real_trunk = ops.linear, model.backbone.forward_nhwc

    def linear(x, weight, *a, **kw):
        if weight is model.fc_emb_1.weight:
            assert kw.get("lowp") is True
            seen.append(x.detach().clone())
        return real_linear(x, weight, *a, **kw)

    def trunk(x):
        calls.append(int(x.shape[0]))
        return real_trunk(x)

    monkeypatch.setattr(IM.ops, "linear", linear)
    monkeypatch.setattr(model.backbone, "forward_nhwc", trunk)
    ids = np.arange(1000, 1000 + B * T).reshape(B, T)
    flat = images.reshape(B * T, 3, 96, 160)
    outs = {}
    with torch.no_grad():
        plain = model((images, boxes))["activities"]
        assert calls == [B * T]
        for dtype in (torch.float32, torch.bfloat16):
            cache = FeatureCache(gpu, *row_and_box_bytes(cfg, dtype), 1 << 30, dtype=dtype)
            del calls[:]
            first = FrameRefs(ids, flat, np.arange(B * T), cache)
            missed = model((first, boxes))["activities"]
            assert calls == [B * T] and first.inserted == ids.reshape(-1).tolist() and cache.inserted == B * T
            second = FrameRefs(ids, flat[:0], [], cache)
            resident = model((second, boxes))["activities"]
            assert calls == [B * T], "the backbone ran for a batch whose frames are all resident"
            torch.cuda.synchronize()
            cache.check()
            assert (cache.hits, cache.misses) == (B * T, B * T) and second.inserted == []
            assert cache.bytes == 64 * ((614400 if dtype == torch.float32 else 307200) + 192)
            outs[dtype] = (missed, resident)
    assert [s.dtype for s in seen] == [torch.float32] * 3 + [torch.bfloat16] * 2
    assert all(s.shape == seen[0].shape for s in seen) and seen[0].numel() == B * T * 12 * 512 * 25
    operand = [_bits(s.to(torch.bfloat16)) for s in seen]
    for k, name in enumerate(("fp32 cache, all missed", "fp32 cache, all resident", "bf16 cache, all missed", "bf16 cache, all resident"), 1):
        assert torch.equal(operand[0], operand[k]), f"{name}: fc_emb_1's bf16 operand differs from the one of the plain images tensor"
    for a, b, name in zip(outs[torch.float32], outs[torch.bfloat16], ("all missed", "all resident")):
        print(f"logits, {name}: fp32 cache {a[0, :3].tolist()}, bf16 cache {b[0, :3].tolist()}, plain {plain[0, :3].tolist()}")
        assert torch.equal(a, b), f"{name}: the model's outputs differ between the two cache dtypes"


# ---- end to end through the trainer -----------------------------------------------------------------------------------------------------
STEPS_PER_EPOCH = 3                                              # 2 training clips at batch size 1, then 1 validation clip


def _run_two_epochs(dtype):
    """tests/test_gpu_feature_cache.py's two epochs over tests/golden/dataset_tree (frozen VGG16, here with backbone_dtype = 'bf16'),
    with cfg.feature_cache_gb = 1 and cfg.feature_cache_dtype = dtype.  Returns (the loss of every step in order, the number of model
    calls made before each decode, the same with the frame count for each backbone call, the caches)."""
    from din_amd import feature_cache as FE, train_net_dynamic as TD, volleyball as V
    from din_amd.backbone.backbone import MyVGG16
    from din_amd.config import Config
    from din_amd.infer_model import Dynamic_volleyball
    cfg = Config("volleyball")
    cfg.data_path, cfg.train_seqs, cfg.test_seqs = os.path.join(GOLDEN, "dataset_tree", "volleyball"), [1], [4]
    cfg.backbone, cfg.image_size, cfg.out_size, cfg.emb_features = "vgg16", (96, 160), (3, 5), 512
    cfg.num_boxes, cfg.num_frames, cfg.num_before, cfg.num_after = 12, 3, 1, 1
    cfg.num_features_boxes, cfg.num_features_gcn = 64, 64
    cfg.ST_kernel_size, cfg.sampling_ratio, cfg.beta_factor, cfg.train_backbone = [(3, 3)], [1], False, False
    cfg.training_stage, cfg.batch_size, cfg.test_batch_size, cfg.max_epoch, cfg.test_interval_epoch = 2, 1, 1, 2, 1
    cfg.train_dropout_prob, cfg.train_learning_rate, cfg.lr_plan, cfg.train_random_seed = 0.0, 1e-4, {}, 5
    cfg.result_path = None
    cfg.feature_cache_gb, cfg.frame_cache_gb, cfg.num_workers = 1, 0, 0
    cfg.backbone_dtype, cfg.feature_cache_dtype = "bf16", dtype
    losses, decodes, trunks, caches, model_calls = [], [], [], [], [0]
    real = V.load_frame_u8, FE.FeatureCache.__init__, MyVGG16.forward_nhwc, TD._Epoch.add

    def counting_load(path, size):
        decodes.append(model_calls[0])
        return real[0](path, size)

    def recording_init(self, *a, **kw):
        real[1](self, *a, **kw)
        caches.append(self)

    def counting_trunk(self, x):
        trunks.append((model_calls[0], int(x.shape[0])))
        return real[2](self, x)

    def recording_add(self, scores, target, loss):
        losses.append(loss.detach().clone())
        return real[3](self, scores, target, loss)

    def pre_hook(module, args):
        if isinstance(module, Dynamic_volleyball):
            assert isinstance(args[0][0], FE.FrameRefs)
            model_calls[0] += 1

    handle = torch.nn.modules.module.register_module_forward_pre_hook(pre_hook)
    V.load_frame_u8, FE.FeatureCache.__init__, MyVGG16.forward_nhwc, TD._Epoch.add = counting_load, recording_init, counting_trunk, recording_add
    try:
        TD.train_net(cfg)
        torch.cuda.synchronize()
    finally:
        handle.remove()
        V.load_frame_u8, FE.FeatureCache.__init__, MyVGG16.forward_nhwc, TD._Epoch.add = real
    return [float(v) for v in losses], decodes, trunks, caches


def test_train_net_with_bf16_rows_takes_the_same_steps_in_half_the_bytes(gpu):
    """two epochs with cfg.feature_cache_dtype = 'bf16' against 'fp32', frozen bf16 VGG16, same seed: the loss of every step is the
    same number, the second epoch decodes nothing and calls no backbone, and the slabs of the bf16 run take (307200 + 192) /
    (614400 + 192) of the fp32 run's bytes (this geometry's row is the launcher's VGG16 row: s = 1)."""
    losses32, decodes32, trunks32, caches32 = _run_two_epochs("fp32")
    losses16, decodes16, trunks16, caches16 = _run_two_epochs("bf16")
    for k, (a, b) in enumerate(zip(losses32, losses16)):
        print(f"step {k}: loss with fp32 rows {a!r}, with bf16 rows {b!r}, difference {abs(a - b):.3e}")
    for caches, dtype in ((caches32, torch.float32), (caches16, torch.bfloat16)):
        assert len(caches) == 2 and all(c.dtype == dtype and c.device.type == "cuda" for c in caches)
    for decodes, trunks in ((decodes32, trunks32), (decodes16, trunks16)):
        assert len([c for c in decodes if c < STEPS_PER_EPOCH]) == 9 and [c for c in decodes if c >= STEPS_PER_EPOCH] == []
        assert trunks == [(k + 1, 3) for k in range(STEPS_PER_EPOCH)], trunks                 # once per step of epoch 1, then never
    assert [(c.hits, c.misses, c.inserted) for c in caches16] == [(c.hits, c.misses, c.inserted) for c in caches32]
    bytes32, bytes16 = sum(c.table.bytes for c in caches32), sum(c.table.bytes for c in caches16)
    assert bytes32 == 2 * 64 * (614400 + 192) and bytes16 == 2 * 64 * (307200 + 192)
    assert bytes16 * (614400 + 192) == bytes32 * (307200 + 192)
    assert len(losses32) == len(losses16) == 2 * STEPS_PER_EPOCH
    assert losses16 == losses32, [abs(a - b) for a, b in zip(losses32, losses16)]
