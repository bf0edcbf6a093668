"""NHWC execution graph for the backbone conv stacks (rows V, I, M of SURVEY section 8).

A backbone is described once as a static list of ops over *views* (tensor id, channel offset, channels) of
pixel-major NHWC buffers, then run forward and backward through libdin_hip.so by ONE torch.autograd.Function.
That gives the MI355X design its properties:
  * torch.cat(dim=1) (Inception blocks, infer_model.py:172) costs nothing: producers write channel ranges;
  * ReLU backward is fused into whatever kernel produces a gradient (conv dgrad epilogue / pool backward);
  * BatchNorm(eval) is folded into the packed filters (scale) and the conv bias (shift);
  * images stay uint8 until the fused prep loader (no fp32 image copies, SURVEY 7 hard part 7).
Nothing here falls back to ATen: every arithmetic op is a C-ABI call and raises if the library is absent.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib as L


def _ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def torch_dtype(dt: int):
    return torch.float32 if L.storage_dtype(dt) == L.DIN_F32 else torch.bfloat16


def din_dtype(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return L.DIN_F32
    if t.dtype == torch.bfloat16:
        return L.DIN_BF16
    raise L.DinError(f"unsupported storage dtype {t.dtype}")


def require_gpu(*tensors: torch.Tensor) -> None:
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise L.DinError("din_amd ops run only on MI355X device tensors (no CPU fallback); got a CPU tensor")
        if not t.is_contiguous():
            raise L.DinError("din_amd ops need contiguous tensors")


# ------------------------------------------------------------------------------------------------
# hooks.  LAUNCH_TIMER: optional context-manager factory (kind, desc, name) wrapped around every conv launch -- the measurement side
# (din_amd/profiling.py, used by bench.py) installs it; the product path itself carries no timing code.
# ------------------------------------------------------------------------------------------------
import contextlib as _contextlib
LAUNCH_TIMER = None
TIMING_ACTIVE = lambda: LAUNCH_TIMER is not None      # noqa: E731  (profiling.install narrows it to "events are being recorded right now")


def _timed(kind, d, name=""):
    return LAUNCH_TIMER(kind, d, name) if LAUNCH_TIMER is not None else _contextlib.nullcontext()


# Called as GRAD_HOOK(weight, dweight) right after a conv layer's weight gradient has been enqueued (backward order: last layer
# first).  parallel.GradBuckets uses it to start a bucket's all-reduce while the rest of the backward pass is still running.
GRAD_HOOK = None
# diagnostics (tools/bf16_grad_cosine.py): GRAD_TAP(tensor id, producing op's name, complete gradient buffer [nb, h, w, c_total]) is called in
# graph_backward each time the reverse pass reaches a producer of a tensor -- its gradient is complete then.  None in production.
GRAD_TAP = None
# Called as GRAD_BUFFER(weight) before a conv layer's weight gradient is computed; may return the fp32 tensor (weight's shape) the kernel
# should write into -- parallel.GradBuckets hands out the weight's slot of its flat all-reduce bucket, so no packing copy is needed.
GRAD_BUFFER = None
# Called as GRAD_ASSIGN(weight, dweight) for every parameter gradient when the backward pass returns; True = the callee installed the
# tensor as weight.grad itself (a gradient that was written in place into its all-reduce bucket slot), autograd then gets None for it:
# handing autograd a tensor that somebody else still references makes AccumulateGrad clone it -- one copy launch per parameter per step.
GRAD_ASSIGN = None


def _dw_buffer(w: torch.Tensor) -> torch.Tensor:
    if GRAD_BUFFER is not None:
        buf = GRAD_BUFFER(w)
        if buf is not None:
            return buf
    return torch.empty_like(w)
# Host-layer fusion switches.  None = ask the option table the library's kernel switches live in (din_set_option, `_lib.host_flag`: production
# sets none, nothing reads the environment); a test may also pin one by assigning True / False to the module attribute.
FUSE_1X1_DGRAD = None        # DIN_FUSE_1X1 (default on): fuse the dgrads of 1x1 convs that read the same tensor
FUSE_FWD_SIBLINGS = None     # DIN_FUSE_FWD (on): run Graph.fwd_groups (sibling 1x1 convs) as one two-destination launch
FUSE_WGRAD_SIBLINGS = None   # DIN_FUSE_WGRAD (on): ... and the wgrads of the members that share the second tensor as one launch
FUSE_WGRAD_1X1 = None        # DIN_FUSE_WGRAD_1X1 (on): weight gradients of ALL 1x1 convs reading one view in one launch (din_conv1x1_wgrad_multi)
FUSE_DGRAD_X = None          # DIN_FUSE_DGRAD_X (on): a lone 1x1's dgrad rides in the strided sibling's launches (din_conv_dgrad_x: Mixed_6a)
GROUP_WGRAD = None           # DIN_GROUP_WGRAD (on): weight gradients of up to GROUP_WGRAD_MAX layers share one launch (din_conv_wgrad_group)
# A queue is flushed at GROUP_WGRAD_MAX layers or when the operands it holds back (input + output gradient of every queued layer) reach
# GROUP_WGRAD_MB: measured on one box (profiles/r06_wgrad_group.txt) -- 4 clips (31 MB per Mixed_6 layer): 12 layers 8.80 ms, 8 layers 8.84,
# no grouping 9.74; 32 clips (248 MB per layer): 4 layers 663.6 clips/s = no grouping 663.0, 8 layers 659.7, 16 layers 650 (a deferred launch
# reads operands that have left the 256 MB last-level cache; the slice partials it saves are ~5 % of a launch at that size).
GROUP_WGRAD_MAX = 12         # (<= the library's WGRAD_GROUP_MAX = 16; option DIN_GROUP_WGRAD_MAX overrides)
GROUP_WGRAD_MB = 768         # (option DIN_GROUP_WGRAD_MB overrides)
_SWITCHES = {"FUSE_1X1_DGRAD": ("DIN_FUSE_1X1", True), "FUSE_FWD_SIBLINGS": ("DIN_FUSE_FWD", True), "FUSE_WGRAD_SIBLINGS": ("DIN_FUSE_WGRAD", True),
             "FUSE_WGRAD_1X1": ("DIN_FUSE_WGRAD_1X1", True), "FUSE_DGRAD_X": ("DIN_FUSE_DGRAD_X", True), "GROUP_WGRAD": ("DIN_GROUP_WGRAD", True), "WGRAD_SIDE_STREAM": ("DIN_WGRAD_STREAM", False)}


def switch(attr: str) -> bool:
    v = globals()[attr]
    if v is not None:
        return bool(v)
    name, default = _SWITCHES[attr]
    return L.host_flag(name, default)



# ------------------------------------------------------------------------------------------------
# shared split-K / wgrad workspace (per device; ops on one stream are serialised, so one buffer is safe)
# ------------------------------------------------------------------------------------------------
_WS: Dict[Tuple[int, str], torch.Tensor] = {}


_SIDE: Dict[int, "torch.cuda.Stream"] = {}
WGRAD_SIDE_STREAM = None     # DIN_WGRAD_STREAM (off), opt-in: measured 472 -> 351 clips/s (the LDS-heavy kernels of the two streams evict each other)


def side_stream(device) -> "torch.cuda.Stream":
    """Second HIP stream per device: wgrad (+ slice reduce, BN parameter gradients) of layer l runs here while the main stream goes
    on with the dgrad chain -- both only depend on the gradient at the layer's output, and each kernel's last partial round of
    workgroups leaves CUs idle that the other stream's kernel can fill."""
    key = device.index if device.index is not None else torch.cuda.current_device()
    if key not in _SIDE:
        _SIDE[key] = torch.cuda.Stream(device=device)
    return _SIDE[key]


def workspace(nbytes: int, device, tag: str = "") -> Tuple[Optional[torch.Tensor], int]:
    if nbytes <= 0:
        return None, 0
    key = (device.index if device.index is not None else torch.cuda.current_device(), tag)
    ws = _WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(int(nbytes * 1.25) + 1024, dtype=torch.uint8, device=device)
        _WS[key] = ws
    return ws, ws.numel()


# ------------------------------------------------------------------------------------------------
# graph description
# ------------------------------------------------------------------------------------------------
@dataclass
class TensorSpec:
    h: int
    w: int
    c: int                  # pixel stride (total channels incl. padding)
    relu_masked: bool = False   # some producer applies ReLU -> gradients into it are masked by (value > 0)


@dataclass
class View:
    tid: int
    coff: int
    c: int


@dataclass
class Op:
    kind: str               # conv | maxpool | avgpool | bilinear
    src: View
    dst: View
    name: str = ""
    k: Tuple[int, int] = (1, 1)
    s: Tuple[int, int] = (1, 1)
    p: Tuple[int, int] = (0, 0)
    relu: bool = False
    bias: bool = False      # conv has its own bias parameter (VGG)
    bn: bool = False        # conv followed by BatchNorm (Inception BasicConv2d)
    pooled: Optional[Tuple[int, int, int]] = None   # (k, s, p): the reference runs avg_pool2d(k, s, p) on src BEFORE this 1x1 conv
                                                    # (InceptionA/C branch_pool); executed as conv1x1 -> avgpool(+shift, ReLU) on cout channels
    mid: Optional[View] = None                      # pooled convs only: where the raw conv output goes when the conv runs inside a forward group


@dataclass
class Graph:
    tensors: List[TensorSpec] = field(default_factory=list)
    ops: List[Op] = field(default_factory=list)
    input_tid: int = 0
    output_tids: List[int] = field(default_factory=list)
    cin_image: int = 3
    u8_ok: Dict[Tuple[int, int], bool] = field(default_factory=dict)   # (frames, dtype) -> the image layer takes uint8 frames (_accepts_u8_frames)
    fwd_groups: List[Tuple[int, ...]] = field(default_factory=list)   # consecutive sibling conv ops (same source view, same 1x1 geometry) whose
                                                                      # forward runs as ONE launch: first member -> its own view, the rest -> adjacent views of one tensor

    def add_tensor(self, h, w, c) -> int:
        self.tensors.append(TensorSpec(h, w, c))
        return len(self.tensors) - 1

    def param_names(self) -> List[str]:
        """Parameter (and BN buffer) names in the order the autograd Function receives them."""
        names = []
        for op in self.ops:
            if op.kind != "conv":
                continue
            if op.bn:
                names += [op.name + ".conv.weight", op.name + ".bn.weight", op.name + ".bn.bias",
                          op.name + ".bn.running_mean", op.name + ".bn.running_var"]
            else:
                names.append(op.name + ".weight")
                if op.bias:
                    names.append(op.name + ".bias")
        return names


def conv_out(h, k, s, p, d=1):
    return (h + 2 * p - d * (k - 1) - 1) // s + 1


def group_view(op: Op) -> Optional[View]:
    """where a forward-group member's conv output lands: its dst, or `mid` for a conv whose pool was commuted behind it"""
    return op.mid if op.pooled is not None else op.dst


class GraphBuilder:
    """Tiny helper used by backbone/backbone.py to lay out the layer tables."""

    def __init__(self, h: int, w: int, cpad_image: int):
        self.g = Graph()
        self.g.input_tid = self.g.add_tensor(h, w, cpad_image)

    def tensor(self, h, w, c) -> int:
        return self.g.add_tensor(h, w, c)

    def full(self, tid) -> View:
        return View(tid, 0, self.g.tensors[tid].c)

    def conv(self, name, src: View, cout, k, s=(1, 1), p=(0, 0), relu=True, bias=False, bn=False,
             dst: Optional[View] = None, pooled: Optional[Tuple[int, int, int]] = None, mid: Optional[View] = None) -> View:
        ts = self.g.tensors[src.tid]
        oh, ow = conv_out(ts.h, k[0], s[0], p[0]), conv_out(ts.w, k[1], s[1], p[1])
        if pooled is not None:
            assert tuple(k) == (1, 1) and tuple(s) == (1, 1) and tuple(p) == (0, 0) and pooled[1] == 1 and cout % 8 == 0
            assert conv_out(ts.h, pooled[0], 1, pooled[2]) == ts.h, "commuted pool must keep the grid"
        if dst is None:
            dst = self.full(self.tensor(oh, ow, cout))
        td = self.g.tensors[dst.tid]
        assert (td.h, td.w) == (oh, ow) and dst.c == cout, (name, td, oh, ow)
        td.relu_masked = td.relu_masked or relu
        assert mid is None or pooled is not None
        self.g.ops.append(Op("conv", src, dst, name, tuple(k), tuple(s), tuple(p), relu, bias, bn, pooled, mid))
        return dst

    def fuse_forward(self, n_last: int) -> None:
        """Declare the last n_last conv ops a forward group (see Graph.fwd_groups); checks the layout the fused launch needs.  Members
        with a commuted pool (raw conv output into `mid`, bias + ReLU after the pool) must come last."""
        idx = tuple(range(len(self.g.ops) - n_last, len(self.g.ops)))
        ops = [self.g.ops[i] for i in idx]
        a = ops[0]
        assert a.pooled is None
        assert all(o.kind == "conv" and o.src == a.src and o.k == a.k and o.s == a.s and o.p == a.p and o.bn == a.bn and o.bias == a.bias
                   and o.relu == a.relu for o in ops), "fused siblings must share source and geometry"
        second = [group_view(o) for o in ops[1:]]
        assert all(v is not None and v.tid == second[0].tid for v in second) and second[0].tid != a.dst.tid
        for x, y in zip(second, second[1:]):
            assert y.coff == x.coff + x.c, "second-destination views must be adjacent"
        pooled = [o.pooled is not None for o in ops]
        assert pooled == sorted(pooled), "pooled members last"
        self.g.fwd_groups.append(idx)

    def pool(self, kind, src: View, k, s, p, dst: Optional[View] = None) -> View:
        ts = self.g.tensors[src.tid]
        oh, ow = conv_out(ts.h, k, s, p), conv_out(ts.w, k, s, p)
        if dst is None:
            dst = self.full(self.tensor(oh, ow, src.c))
        td = self.g.tensors[dst.tid]
        assert (td.h, td.w) == (oh, ow) and dst.c == src.c
        self.g.ops.append(Op(kind, src, dst, kind, (k, k), (s, s), (p, p)))
        return dst

    def bilinear(self, src: View, dst: View) -> View:
        assert dst.c == src.c
        self.g.ops.append(Op("bilinear", src, dst, "bilinear"))
        return dst


# ------------------------------------------------------------------------------------------------
# executor
# ------------------------------------------------------------------------------------------------
def _conv_desc(g: Graph, op: Op, nb: int, dt: int, cin: Optional[int] = None) -> L.ConvDesc:
    ts, td = g.tensors[op.src.tid], g.tensors[op.dst.tid]
    d = L.ConvDesc()
    d.nb, d.h, d.w, d.cin = nb, ts.h, ts.w, cin if cin is not None else op.src.c
    d.oh, d.ow, d.cout = td.h, td.w, op.dst.c
    d.kh, d.kw = op.k
    d.sh, d.sw = op.s
    d.ph, d.pw = op.p
    d.dh = d.dw = 1
    d.ldi, d.cioff, d.ldo, d.cooff = ts.c, op.src.coff, td.c, op.dst.coff
    d.dtype = dt
    return d


def _copy_desc(d: L.ConvDesc) -> L.ConvDesc:
    return L.ConvDesc.from_buffer_copy(d)


def _pool_desc(g: Graph, op: Op, nb: int, dt: int) -> L.PoolDesc:
    ts, td = g.tensors[op.src.tid], g.tensors[op.dst.tid]
    d = L.PoolDesc()
    d.nb, d.h, d.w, d.c, d.oh, d.ow = nb, ts.h, ts.w, op.src.c, td.h, td.w
    d.k, d.stride, d.pad = op.k[0], op.s[0], op.p[0]
    d.ldi, d.cioff, d.ldo, d.cooff = ts.c, op.src.coff, td.c, op.dst.coff
    d.dtype = L.storage_dtype(dt)                          # (pools move data: the storage type)
    return d


def _pooled_descs(g: Graph, op: Op, nb: int, dt: int) -> Tuple[L.ConvDesc, L.PoolDesc]:
    """conv1x1 src -> tmp [nb,h,w,cout] and avgpool tmp -> dst view for a conv whose pool was commuted behind it"""
    ts, td = g.tensors[op.src.tid], g.tensors[op.dst.tid]
    d = _conv_desc(g, op, nb, dt)
    d.ldo, d.cooff = op.dst.c, 0
    pd = L.PoolDesc()
    pd.nb, pd.h, pd.w, pd.c, pd.oh, pd.ow = nb, ts.h, ts.w, op.dst.c, td.h, td.w
    pd.k, pd.stride, pd.pad = op.pooled
    pd.ldi, pd.cioff, pd.ldo, pd.cooff = op.dst.c, 0, td.c, op.dst.coff
    pd.dtype = L.storage_dtype(dt)
    return d, pd


BN_EPS = 1e-3      # torchvision BasicConv2d


class _BnTables:
    """device-side pointer / offset tables of a graph's BatchNorm layers (parameters keep their addresses across steps)"""
    def __init__(self, key, ptrs, offs, off_list):
        self.key, self.ptrs, self.offs, self.off_list = key, ptrs, offs, off_list
        self.n, self.total = len(off_list) - 1, off_list[-1]


def param_layout(g: "Graph") -> Tuple[List[int], Dict[int, int]]:
    """Where the parameters of each op sit in `params` (the order of Graph.param_names): (op index -> index of its weight, -1 for an op
    that is no conv; conv + BatchNorm op index -> its slot in the graph's BatchNorm tables).  Behind a weight come gamma, beta, running
    mean and running variance (conv + BatchNorm) or the bias, if the conv has one."""
    offsets, bn_index, pos = [], {}, 0
    for oi, op in enumerate(g.ops):
        if op.kind != "conv":
            offsets.append(-1)
            continue
        offsets.append(pos)
        if op.bn:
            bn_index[oi] = len(bn_index)
        pos += 5 if op.bn else (2 if op.bias else 1)
    return offsets, bn_index


def _bn_tables(g: "Graph", params: Sequence[torch.Tensor], dev) -> Optional[_BnTables]:
    offsets, bn_index = param_layout(g)
    rows, off_list = [], [0]
    for oi in bn_index:
        gamma, beta, mean, var = params[offsets[oi] + 1:offsets[oi] + 5]
        rows.append([gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(), var.data_ptr()])
        off_list.append(off_list[-1] + gamma.numel())
    if not rows:
        return None
    key = tuple(r[0] for r in rows)
    cached = getattr(g, "_bn_tables", None)
    if cached is not None and cached.key == key and cached.ptrs.device == dev:
        return cached
    tb = _BnTables(key, torch.tensor(rows, dtype=torch.int64).to(dev), torch.tensor(off_list, dtype=torch.int32).to(dev), off_list)
    g._bn_tables = tb
    return tb


PACK_CHUNK = 16384


class _PackCache:
    """persistent packed filter banks of a graph (+ the device table that lets ONE launch repack all of them every step)"""
    pass


def _pack_cache(g: Graph, params: Sequence[torch.Tensor], dt: int, dev, with_transposed: bool, bn: Optional[_BnTables]) -> _PackCache:
    lib = L.load()
    key = (tuple(p.data_ptr() for p in params), dt, bool(with_transposed), str(dev))
    pc = getattr(g, "_pack_cache", None)
    if pc is not None and pc.key == key:
        return pc
    pc = _PackCache()
    pc.key = key
    tdt = torch_dtype(dt)
    pc.bn_scale = torch.empty(bn.total, dtype=torch.float32, device=dev) if bn is not None else None
    pc.bn_shift = torch.empty(bn.total, dtype=torch.float32, device=dev) if bn is not None else None
    pc.wpk, pc.wpt = {}, {}
    descs, layer_of, chunk_index = [], [], []
    offsets, bn_index = param_layout(g)
    src_of: Dict[int, tuple] = {}
    pc.wfused = {}
    for oi, op in enumerate(g.ops):
        if op.kind != "conv":
            continue
        cin = g.cin_image if op.src.tid == g.input_tid else op.src.c
        d = _conv_desc(g, op, 1, dt, cin)
        w = params[offsets[oi]]
        scale_ptr = C.c_void_p(pc.bn_scale.data_ptr() + 4 * bn.off_list[bn_index[oi]]) if op.bn else None
        src_of[oi] = (w, scale_ptr)
        for transposed in ((0, 1) if (with_transposed and op.src.tid != g.input_tid) else (0,)):
            n_el = lib.din_conv_packed_elems(C.byref(d), transposed)
            buf = torch.empty(n_el, dtype=tdt, device=dev)
            (pc.wpt if transposed else pc.wpk)[oi] = buf
            pd = L.PackDesc()
            L.check(lib.din_conv_pack_desc(C.byref(d), _ptr(w), scale_ptr, _ptr(buf), transposed, C.byref(pd)), "conv_pack_desc")
            li = len(descs)
            descs.append(pd)
            nchunk = (n_el + PACK_CHUNK - 1) // PACK_CHUNK
            layer_of += [li] * nchunk
            chunk_index += list(range(nchunk))
    # forward groups: the siblings' banks packed row after row into ONE bank (each member writes exactly its own rows; the tail rows of
    # the zero-initialised buffer stay zero), so the fused launch sees a single conv with cout = sum of the members
    esz = 4 if L.storage_dtype(dt) == L.DIN_F32 else 2
    for grp in g.fwd_groups:
        a = g.ops[grp[0]]
        dF = _conv_desc(g, a, 1, dt, a.src.c)
        dF.cout = sum(g.ops[i].dst.c for i in grp)
        fused = torch.zeros(lib.din_conv_packed_elems(C.byref(dF), 0), dtype=tdt, device=dev)
        pc.wfused[grp[0]] = fused
        row0 = 0
        for oi in grp:
            op = g.ops[oi]
            d = _conv_desc(g, op, 1, dt, op.src.c)
            w, scale_ptr = src_of[oi]
            pd = L.PackDesc()
            L.check(lib.din_conv_pack_desc(C.byref(d), _ptr(w), scale_ptr, _ptr(fused), 0, C.byref(pd)), "conv_pack_desc(fused)")
            pd.out = fused.data_ptr() + row0 * pd.kelems * esz
            pd.rows_pad = pd.rows
            li = len(descs)
            descs.append(pd)
            nchunk = (pd.rows * pd.kelems + PACK_CHUNK - 1) // PACK_CHUNK
            layer_of += [li] * nchunk
            chunk_index += list(range(nchunk))
            row0 += op.dst.c
    raw = (L.PackDesc * len(descs))(*descs)
    host = torch.frombuffer(bytearray(bytes(raw)), dtype=torch.uint8).clone()
    pc.table = host.to(dev)
    pc.layer_of = torch.tensor(layer_of, dtype=torch.int32).to(dev)
    pc.chunk_index = torch.tensor(chunk_index, dtype=torch.int32).to(dev)
    pc.nblocks = len(layer_of)
    g._pack_cache = pc
    return pc


BN_MOMENTUM = 0.1  # torch.nn.BatchNorm2d default (torchvision BasicConv2d)


def _bn_train_forward(lib, raw: torch.Tensor, dt: int, rows: int, cout: int, gamma, beta, mean, var, relu: bool, dst: torch.Tensor,
                      ldd: int, coffd: int, st):
    """batch-statistics BatchNorm (+ReLU) of a raw conv output [rows][cout] into the channel view (ldd, coffd) of dst; updates the
    running statistics in place; returns (batch mean, rstd) for the backward pass"""
    dev = raw.device
    dt = L.storage_dtype(dt)
    ws = torch.empty(lib.din_bn_workspace(rows, cout) // 8, dtype=torch.float64, device=dev)   # reduced sums + one slab per workgroup
    ab = torch.empty(4 * cout, dtype=torch.float32, device=dev)
    a, b, bmean, rstd = ab[:cout], ab[cout:2 * cout], ab[2 * cout:3 * cout], ab[3 * cout:]
    # fp64 accumulation with exact products, fixed summation order (csrc/bn.hip): no shift needed, bit-reproducible statistics
    L.check(lib.din_bn_stats(_ptr(raw), dt, rows, cout, cout, 0, None, _ptr(ws), st), "bn_stats")
    L.check(lib.din_bn_finalize(_ptr(ws), lib.din_bn_parts(rows), rows, cout, _ptr(gamma), _ptr(beta), BN_EPS, BN_MOMENTUM, _ptr(mean), _ptr(var),
                                _ptr(a), _ptr(b), _ptr(bmean), _ptr(rstd), None, st), "bn_finalize")
    L.check(lib.din_bn_apply(_ptr(raw), dt, rows, cout, cout, 0, _ptr(a), _ptr(b), int(relu), _ptr(dst), ldd, coffd, st), "bn_apply")
    return bmean, rstd


# the filter-stationary halo kernel families (csrc/conv_halo_rf.h), one row each: kernel size, the four entry points, the BackwardPlan set it fills
RfFamily = NamedTuple("RfFamily", [("k", Tuple[int, int]), ("eligible", str), ("fwd", str), ("dgrad", str), ("names", str), ("plan_set", str)])
RF_FAMILIES = (RfFamily((3, 3), "din_conv_rf_eligible", "din_conv_rf_fwd", "din_conv_rf_dgrad", "din_conv_rf_kernel_names", "rf_dgrad"),
               RfFamily((5, 5), "din_conv_rf5_eligible", "din_conv_rf5_fwd", "din_conv_rf5_dgrad", "din_conv_rf5_kernel_names", "rf5_dgrad"))


# ------------------------------------------------------------------------------------------------
# the two passes, each in three parts: a plan decides (plan_forward / plan_backward: no tensor, no stream, no launch; the only readers
# of the switches and options, and where the library is asked which route or kernel family a launch takes), a pass object does
# (_ForwardPass / _BackwardPass: the buffers, the caches and one method per step), and graph_forward / graph_backward is the loop over the ops.
# profiles/forward_launch_trace.txt and profiles/backward_launch_trace.txt (tools/backward_trace.py, tests/test_forward_trace_cpu.py,
# tests/test_backward_trace_cpu.py) pin every launch, allocation order and hook of both.
# ------------------------------------------------------------------------------------------------
class FwdGroup(NamedTuple):
    """a sibling group that runs as ONE two-destination launch over the members' concatenated filter bank (din_conv_fwd2)"""
    members: Tuple[int, ...]    # op indices, the lead first: it writes its own view, the others the adjacent views of one tensor
    ctot: int                   # output channels of all members ...
    craw: int                   # ... and of those in front of the commuted-pool members, which leave their raw conv output in `mid` (0: no such member)
    v2: View                    # where the second destination starts (group_view of the second member)
    name: str                   # the members' names, as the launch timer sees the launch


@dataclass
class FwdStep:
    """One op's turn in the forward pass.  route is the _ForwardPass method that runs it:
      bn_train  conv -> raw output (-> commuted pool) -> batch statistics -> normalise + ReLU into dst
      member    a sibling launch already produced this conv's output; pd: its commuted pool + shift + ReLU is still to run
      lead      the first conv of a sibling group: one din_conv_fwd2 launch for all of `group`
      pooled    conv1x1 into a temporary, then the commuted average pool with the conv's shift + ReLU as its epilogue
      conv      one conv launch with its epilogue
      maxpool (amax: and its winning-tap map is kept for backward) | avgpool | bilinear
    Only `conv` and `pooled` can run a filter-stationary halo kernel (rf): bn_train and lead have no such entry point and are not asked."""
    route: str
    d: Optional[L.ConvDesc] = None          # conv routes: the descriptor of the conv launch, ready (lead: cout = group.ctot; bn_train: raw output)
    pd: Optional[L.PoolDesc] = None         # the pool's descriptor / the commuted pool's
    flags: int = 0                          # CONV_BIAS | CONV_RELU of the epilogue, on whichever launch writes dst (pooled: the pool's; the conv gets 0)
    rf: Optional[RfFamily] = None           # the family of RF_FAMILIES whose forward entry point runs the conv; None: din_conv_fwd
    ws_bytes: int = 0                       # split-K workspace of the conv launch
    w: int = -1                             # conv: index of its weight in params (param_layout)
    bn: int = -1                            # conv + BatchNorm: its slot in the graph's BatchNorm tables
    group: Optional[FwdGroup] = None
    amax: bool = False


@dataclass
class ForwardPlan:
    """What one forward pass of a graph will launch: a function of the graph, the frame count, the dtype, the BatchNorm mode, whether the
    frames are uint8, whether a reverse pass follows, the FUSE_FWD_SIBLINGS switch and the library's planning queries (plan_forward)."""
    steps: List[FwdStep]                    # one per op
    bn_train: bool                          # batch-statistics BatchNorm (and the graph has BatchNorm layers)
    bn_off: List[int]                       # BatchNorm slot -> first channel in the flat scale / shift arrays (one more entry: their length)
    save_for_backward: bool


def plan_forward(g: Graph, nb: int, dt: int, bn_train: bool, u8: bool, save_for_backward: bool) -> ForwardPlan:
    """Decide the forward pass of g on nb frames.  u8: the image layer reads raw uint8 frames [nb,3,h,w].  The only place of the pass that
    reads FUSE_FWD_SIBLINGS and asks the library (din_conv_workspace_bytes, the `eligible` entries of RF_FAMILIES: once per conv on the
    conv / pooled routes, in turn -- their kernel sizes exclude each other); built on every call (options change between passes)."""
    lib = L.load()
    offsets, bn_index = param_layout(g)
    bn_off = [0]
    for oi in bn_index:
        bn_off.append(bn_off[-1] + g.ops[oi].dst.c)
    bn_train = bool(bn_train) and bool(bn_index)
    group_of = {grp[0]: grp for grp in g.fwd_groups} if (switch("FUSE_FWD_SIBLINGS") and not bn_train) else {}
    fused_done = set()                                     # members whose output a group launch produces
    steps: List[FwdStep] = []
    for oi, op in enumerate(g.ops):
        if op.kind == "maxpool":
            # the winning-tap map is saved when the pooled tensor is a ReLU output: backward then never re-reads the input
            steps.append(FwdStep("maxpool", pd=_pool_desc(g, op, nb, dt),
                                 amax=bool(save_for_backward) and g.tensors[op.src.tid].relu_masked and op.src.tid != g.input_tid))
            continue
        if op.kind in ("avgpool", "bilinear"):
            steps.append(FwdStep(op.kind, pd=_pool_desc(g, op, nb, dt)))
            continue
        if op.kind != "conv":
            raise L.DinError("unknown op " + op.kind)
        cin = g.cin_image if op.src.tid == g.input_tid else op.src.c
        d = _conv_desc(g, op, nb, dt, cin)
        if op.src.tid == g.input_tid and u8:
            d.in_u8, d.ldi, d.cioff = 1, 8, 0                      # raw uint8 frames [nb,3,h,w]: the image layer normalises on load
        w, k = offsets[oi], bn_index.get(oi, -1)
        relu = L.CONV_RELU if op.relu else 0
        if op.bn and bn_train:
            # conv -> raw [nb,oh,ow,cout] (-> commuted pool: also linear, so avgpool(conv(x)) == conv(avgpool(x)) holds before the
            # normalisation) -> batch statistics -> normalise + ReLU into dst's view
            dR, pd = _conv_desc(g, op, nb, dt, cin), None
            dR.in_u8, dR.ldi, dR.cioff = d.in_u8, d.ldi, d.cioff      # (uint8 frames feed the image layer in this mode too)
            dR.ldo, dR.cooff = op.dst.c, 0
            if op.pooled is not None:
                dR.oh, dR.ow = g.tensors[op.src.tid].h, g.tensors[op.src.tid].w
                _, pd = _pooled_descs(g, op, nb, dt)
                pd.ldo, pd.cooff = op.dst.c, 0
            steps.append(FwdStep("bn_train", dR, pd, ws_bytes=lib.din_conv_workspace_bytes(C.byref(dR), 0), w=w, bn=k))
            continue
        if oi in fused_done:
            pd = None
            if op.pooled is not None:                   # the group launch leaves the raw conv output in `mid`: pool + shift + ReLU into dst
                _, pd = _pooled_descs(g, op, nb, dt)
                pd.ldi, pd.cioff = g.tensors[op.mid.tid].c, op.mid.coff
            steps.append(FwdStep("member", None, pd, L.CONV_BIAS | relu, w=w, bn=k))
            continue
        if oi in group_of and op.bn:
            # sibling convs of one source: ONE launch over the concatenated filter bank.  A shape that would run split-K, or members whose
            # BatchNorm slots are not adjacent (one shift array serves the launch), fall through to separate launches.
            grp = group_of[oi]
            rest = [g.ops[i] for i in grp[1:]]
            ctot = op.dst.c + sum(o.dst.c for o in rest)
            craw = ctot - sum(o.dst.c for o in rest if o.pooled is not None)
            dF = _conv_desc(g, op, nb, dt, cin)
            dF.cout = ctot
            if lib.din_conv_workspace_bytes(C.byref(dF), 0) == 0 and bn_off[k + len(grp)] - bn_off[k] == ctot:
                group = FwdGroup(tuple(grp), ctot, craw if craw < ctot else 0, group_view(rest[0]), "+".join(g.ops[i].name for i in grp))
                steps.append(FwdStep("lead", dF, None, L.CONV_BIAS | relu, w=w, bn=k, group=group))
                fused_done.update(grp[1:])
                continue
        flags = (L.CONV_BIAS if (op.bn or op.bias) else 0) | relu
        pd = None
        if op.pooled is not None:
            d, pd = _pooled_descs(g, op, nb, dt)
        conv_flags = 0 if pd is not None else flags
        ws_bytes = lib.din_conv_workspace_bytes(C.byref(d), 0)
        fam = next((f for f in RF_FAMILIES if getattr(lib, f.eligible)(C.byref(d), 0, conv_flags, 0, 0)), None)
        d.rf = (fam.names, conv_flags, 0, 0) if fam else None     # (reporter, flags, ldm, moff): tells the launch timer which reporter names the kernel
        steps.append(FwdStep("pooled" if pd is not None else "conv", d, pd, flags, fam, ws_bytes, w, k))
    return ForwardPlan(steps, bn_train, bn_off, bool(save_for_backward))


class _ForwardPass:
    """The state of one forward pass -- the buffers, what backward needs of each op (aux), the BatchNorm tables and the pack cache -- and
    one method per route of FwdStep, called as route(op index, op, its step, source buffer, destination buffer).  Everything here does;
    which route an op takes, on which kernel family and with which descriptors was decided by plan_forward."""

    def __init__(self, g: Graph, plan: ForwardPlan, image_buf: torch.Tensor, params: Sequence[torch.Tensor], dt: int):
        self.g, self.plan, self.params, self.dt, self.lib = g, plan, params, dt, L.load()
        self.nb, self.dev, self.tdt = image_buf.shape[0], image_buf.device, torch_dtype(dt)
        self.bufs: List[Optional[torch.Tensor]] = [None] * len(g.tensors)
        self.bufs[g.input_tid] = image_buf
        self.aux: list = []
        self.st = _stream()
        self.bn = _bn_tables(g, params, self.dev)
        self.pc = _pack_cache(g, params, dt, self.dev, plan.save_for_backward, self.bn)
        if self.bn is not None and self.bn.off_list != plan.bn_off:
            raise L.DinError("graph_forward: a BatchNorm layer's parameters do not have its conv's output channels")

    def fold_and_pack(self) -> None:
        lib, bn, pc = self.lib, self.bn, self.pc
        if self.plan.bn_train:
            pc.bn_scale.fill_(1.0)                                # filters are packed unscaled: the normalisation happens after the conv
        elif bn is not None:
            # every BatchNorm layer of the graph folded in ONE launch into flat scale / shift arrays (views per layer: shift_scale)
            L.check(lib.din_bn_fold_multi(_ptr(bn.ptrs), _ptr(bn.offs), bn.n, bn.total, BN_EPS, _ptr(pc.bn_scale), _ptr(pc.bn_shift), self.st), "bn_fold_multi")
        # ... and every filter bank (forward and, when training, dgrad orientation) repacked with the folded scale in ONE launch
        L.check(lib.din_conv_pack_multi(_ptr(pc.table), _ptr(pc.layer_of), _ptr(pc.chunk_index), pc.nblocks, PACK_CHUNK, self.st), "conv_pack_multi")

    def empty(self, *shape, dtype=None) -> torch.Tensor:
        return torch.empty(shape, dtype=dtype or self.tdt, device=self.dev)

    def buffer(self, tid: int) -> torch.Tensor:
        if self.bufs[tid] is None:
            t = self.g.tensors[tid]
            self.bufs[tid] = self.empty(self.nb, t.h, t.w, t.c)
        return self.bufs[tid]

    def shift_scale(self, op: Op, s: FwdStep):
        """(what the epilogue adds: the folded BatchNorm shift or the conv's own bias; the folded BatchNorm scale, kept for backward)"""
        if s.bn < 0:
            return (self.params[s.w + 1] if op.bias else None), None
        o0, o1 = self.plan.bn_off[s.bn], self.plan.bn_off[s.bn + 1]
        return self.pc.bn_shift[o0:o1], self.pc.bn_scale[o0:o1]

    def conv_launch(self, oi: int, s: FwdStep, src, bias, dst, flags: int) -> None:
        """the conv launch of the bn_train / pooled / conv routes, through the planned family's entry point"""
        name = self.g.ops[oi].name
        ws, wsb = workspace(s.ws_bytes, self.dev)
        fn = getattr(self.lib, s.rf.fwd if s.rf else "din_conv_fwd")
        with _timed("fwd", s.d, name):
            L.check(fn(C.byref(s.d), _ptr(src), _ptr(self.pc.wpk[oi]), _ptr(bias), _ptr(dst), flags, _ptr(ws), wsb, self.st), "conv_fwd " + name)

    def bn_train(self, oi, op, s, src, dst) -> None:
        pd, td = s.pd, self.g.tensors[op.dst.tid]
        raw = self.empty(self.nb, s.d.oh, s.d.ow, s.d.cout)
        self.conv_launch(oi, s, src, None, raw, 0)
        if pd is not None:
            pooled_raw = self.empty(self.nb, pd.oh, pd.ow, pd.c)
            L.check(self.lib.din_avgpool_fwd(C.byref(pd), _ptr(raw), _ptr(pooled_raw), None, 0, self.st), "avgpool_fwd(raw)")
            raw = pooled_raw
        gamma, beta, mean, var = self.params[s.w + 1:s.w + 5]
        bmean, rstd = _bn_train_forward(self.lib, raw, self.dt, self.nb * td.h * td.w, op.dst.c, gamma, beta, mean, var, op.relu, dst, td.c, op.dst.coff, self.st)
        self.aux.append((None, raw if self.plan.save_for_backward else None, bmean, rstd))

    def member(self, oi, op, s, src, dst) -> None:
        shift, scale = self.shift_scale(op, s)
        if s.pd is not None:
            L.check(self.lib.din_avgpool_fwd(C.byref(s.pd), _ptr(self.bufs[op.mid.tid]), _ptr(dst), _ptr(shift), s.flags, self.st), "avgpool_fwd(epilogue)")
        self.aux.append((scale,))

    def lead(self, oi, op, s, src, dst) -> None:
        grp, o0 = s.group, self.plan.bn_off[s.bn]          # (one shift array for all members: their BatchNorm slots are adjacent)
        second = self.buffer(grp.v2.tid)
        with _timed("fwd", s.d, grp.name):
            L.check(self.lib.din_conv_fwd2(C.byref(s.d), _ptr(src), _ptr(self.pc.wfused[oi]), _ptr(self.pc.bn_shift[o0:o0 + grp.ctot]), _ptr(dst), _ptr(second),
                                           self.g.tensors[grp.v2.tid].c, grp.v2.coff, op.dst.c, grp.craw, s.flags, None, 0, self.st), "conv_fwd2 " + op.name)
        self.aux.append((self.shift_scale(op, s)[1],))

    def pooled(self, oi, op, s, src, dst) -> None:
        shift, scale = self.shift_scale(op, s)
        tmp = self.empty(self.nb, s.pd.h, s.pd.w, s.pd.c)
        self.conv_launch(oi, s, src, None, tmp, 0)
        L.check(self.lib.din_avgpool_fwd(C.byref(s.pd), _ptr(tmp), _ptr(dst), _ptr(shift), s.flags, self.st), "avgpool_fwd(epilogue)")
        self.aux.append((scale,))

    def conv(self, oi, op, s, src, dst) -> None:
        shift, scale = self.shift_scale(op, s)
        self.conv_launch(oi, s, src, shift, dst, s.flags)
        self.aux.append((scale,))

    def maxpool(self, oi, op, s, src, dst) -> None:
        amax = self.empty(self.nb, s.pd.oh, s.pd.ow, s.pd.c, dtype=torch.uint8) if s.amax else None
        L.check(self.lib.din_maxpool_fwd(C.byref(s.pd), _ptr(src), _ptr(dst), _ptr(amax), self.st), "maxpool_fwd")
        self.aux.append((amax,))

    def avgpool(self, oi, op, s, src, dst) -> None:
        L.check(self.lib.din_avgpool_fwd(C.byref(s.pd), _ptr(src), _ptr(dst), None, 0, self.st), "avgpool_fwd")
        self.aux.append(())

    def bilinear(self, oi, op, s, src, dst) -> None:
        L.check(self.lib.din_bilinear_fwd(C.byref(s.pd), _ptr(src), _ptr(dst), self.st), "bilinear_fwd")
        self.aux.append(())


def graph_forward(g: Graph, image_buf: torch.Tensor, params: Sequence[torch.Tensor], dt: int, save_for_backward: bool = True,
                  bn_train: bool = False):
    """Run the graph.  image_buf: NHWC [nb,h,w,cpad] of dtype dt (or the raw uint8 frames [nb,3,h,w] where _accepts_u8_frames).  Returns
    (bufs, aux) for backward: bufs indexed by tensor id, aux one tuple per op.
    bn_train: BatchNorm layers normalise with the statistics of this batch and update their running statistics (the reference's stage-2
    default for Inception-v3: model.train() without set_bn_eval, train_net_dynamic.py:98-100,170-172).  Each BasicConv2d then runs as
    conv (unscaled filters, raw output kept for backward) -> statistics -> normalise + ReLU into the consumer's view; the folded-BN
    fusions (sibling launches, shift in the conv / pool epilogue) do not apply."""
    plan = plan_forward(g, image_buf.shape[0], dt, bn_train, image_buf.dtype == torch.uint8, save_for_backward)
    fp = _ForwardPass(g, plan, image_buf, params, dt)
    fp.fold_and_pack()
    for oi, (op, step) in enumerate(zip(g.ops, plan.steps)):
        dst = fp.buffer(op.dst.tid)
        getattr(fp, step.route)(oi, op, step, fp.bufs[op.src.tid], dst)
    return fp.bufs, fp.aux


# ------------------------------------------------------------------------------------------------
# reverse pass
# ------------------------------------------------------------------------------------------------
ViewKey = Tuple[int, int, int]                 # (tensor id, channel offset, channels)


@dataclass
class BackwardPlan:
    """What one reverse pass of a graph will fuse, group and defer: a function of the graph, the frame count, the dtype, the BatchNorm
    mode, the switches / options and the library's planning queries (plan_backward)."""
    offsets: List[int]                              # op index -> index of its weight in params (-1: not a conv)
    bn_index: Dict[int, int]                        # conv + BatchNorm op index -> its slot in the graph's BatchNorm tables
    bn_train: bool                                  # batch-statistics BatchNorm (and the graph has BatchNorm layers)
    side: bool                                      # weight gradients run on the second stream
    u8: bool                                        # the image layer reads raw uint8 frames
    dgrad_groups: Dict[ViewKey, List[int]]          # 1x1 / stride-1 convs reading one view: their dgrads are ONE launch (din_conv1x1_dgrad_multi)
    member_of: Dict[int, ViewKey]                   # op index -> its dgrad group
    x_host: Dict[int, int]                          # lone 1x1 op index -> the strided op whose dgrad will carry its dgrad (din_conv_dgrad_x)
    siblings: Dict[int, Tuple[int, ...]]            # last member -> the forward-group members that share a tensor: one wgrad launch
    multi_w: Dict[ViewKey, Tuple[List[Tuple[int, ...]], int]]   # dgrad group -> (sources, workspace bytes) of its ONE wgrad launch (din_conv1x1_wgrad_multi)
    group_on: bool                                  # weight gradients queue up for grouped launches (din_conv_wgrad_group) ...
    group_max: int                                  # ... of at most this many layers ...
    group_bytes: int                                # ... holding back at most this many bytes of operands
    partitioned: set                                # tensors whose gradient is first WRITTEN range by range by its readers (see _partitioned)
    first_writer: Dict[int, int]                    # tensor id -> the first op in program order that writes it (its gradient is dead after it)
    rf_dgrad: set = field(default_factory=set)      # op indices whose own data-gradient launch runs the filter-stationary halo kernel (din_conv_rf_dgrad)
    rf5_dgrad: set = field(default_factory=set)     # the same for the 5x5 family (din_conv_rf5_dgrad)


def _partitioned(readers: List[Tuple[int, int]], writers: Sequence[Tuple[int, int]]) -> bool:
    """True when the readers of a tensor use pairwise identical-or-disjoint channel views (`readers`: sorted distinct (offset, channels))
    that together cover every producer's view: then each channel range of the gradient is first WRITTEN by its first reader (no zero
    fill, no accumulate), and nothing is read before it was written (temporaries of sibling convs that share one tensor)."""
    for (a0, ac), (b0, _bc) in zip(readers, readers[1:]):
        if b0 < a0 + ac:
            return False
    for lo, c in writers:
        hi = lo + c
        for c0, cc in readers:
            if c0 <= lo < c0 + cc:
                lo = min(hi, c0 + cc)
        if lo < hi:
            return False
    return True


def wgrad_queue_full(layers: int, held_bytes: int, max_layers: int, max_bytes: int) -> bool:
    """the flush rule of a grouped weight-gradient queue (held_bytes grows with the local batch, so ranks with different
    batches flush at different layers)"""
    return layers >= max_layers or held_bytes >= max_bytes


def plan_backward(g: Graph, nb: int, dt: int, bn_train: bool, side_ok: bool, u8: bool) -> BackwardPlan:
    """Decide the reverse pass of g on nb frames.  side_ok: a second stream may be used (no launch timing in progress).  The only place
    of the pass that reads the host switches and the DIN_GROUP_WGRAD_* options; built on every call (options change between passes)."""
    lib = L.load()
    offsets, bn_index = param_layout(g)
    readers: Dict[int, set] = {}
    writers: Dict[int, list] = {}
    first_writer: Dict[int, int] = {}
    for oi, op in enumerate(g.ops):
        readers.setdefault(op.src.tid, set()).add((op.src.coff, op.src.c))
        writers.setdefault(op.dst.tid, []).append((op.dst.coff, op.dst.c))
        first_writer.setdefault(op.dst.tid, oi)
    partitioned = {tid for tid, views in readers.items() if views != {(0, g.tensors[tid].c)} and _partitioned(sorted(views), writers.get(tid, ()))}
    bn_train = bool(bn_train) and bool(bn_index)
    side = bool(side_ok) and switch("WGRAD_SIDE_STREAM")
    bf16 = dt == L.DIN_BF16

    def entry_1x1(op):
        return op.kind == "conv" and op.k == (1, 1) and op.s == (1, 1) and op.p == (0, 0) and op.src.tid != g.input_tid
    # 1x1 / stride-1 convs that read the same view (branch-entry convs of the Inception blocks): their dgrads are fused into ONE
    # multi-source launch, issued when the last member (first in program order) has been visited
    groups: Dict[ViewKey, List[int]] = {}
    if switch("FUSE_1X1_DGRAD"):
        for oi, op in enumerate(g.ops):
            if entry_1x1(op):
                groups.setdefault((op.src.tid, op.src.coff, op.src.c), []).append(oi)
    groups = {k: v for k, v in groups.items() if 2 <= len(v) <= 4}
    member_of = {oi: key for key, v in groups.items() for oi in v}
    # a lone 1x1 / stride-1 conv whose input view is also read by a STRIDED conv earlier in program order (InceptionB: branch3x3dbl_1 beside
    # branch3x3): the reverse pass meets the 1x1 first, parks its dgrad operands, and the strided conv's dgrad carries them (din_conv_dgrad_x)
    x_host: Dict[int, int] = {}
    if switch("FUSE_DGRAD_X") and bf16:
        for oi, op in enumerate(g.ops):
            if entry_1x1(op) and oi not in member_of and op.pooled is None:
                for oj in range(oi - 1, -1, -1):
                    o2 = g.ops[oj]
                    if o2.kind == "conv" and o2.src == op.src and (o2.s[0] > 1 or o2.s[1] > 1) and oj not in x_host.values():
                        x_host[oi] = oj
                        break
    # sibling groups: the members behind the first one share a tensor -> one wgrad launch, issued when the LAST of them comes up (the
    # reverse pass reaches it first; by then the consumers of every member have written their slice of the shared gradient buffer)
    siblings: Dict[int, Tuple[int, ...]] = {}
    if switch("FUSE_WGRAD_SIBLINGS") and not bn_train and not side:
        for grp in g.fwd_groups:
            mem = tuple(i for i in grp[1:] if g.ops[i].pooled is None)      # (a commuted-pool member keeps its own wgrad: its gradient
            if len(mem) >= 2 and g.ops[mem[-1]].bn:                         #  operand is the un-pooled map, a separate buffer)
                siblings[mem[-1]] = mem
    # 1x1 groups whose weight gradients run as ONE launch (din_conv1x1_wgrad_multi): sources = the members, sibling pairs that share a
    # tensor (siblings) counted as one source; the library says whether the group fits its kernel (0 bytes of workspace: it does not)
    multi_w: Dict[ViewKey, Tuple[List[Tuple[int, ...]], int]] = {}
    if switch("FUSE_WGRAD_1X1") and bn_index and not bn_train and not side and bf16:
        pair_of = {i: mem for mem in siblings.values() for i in mem}
        for key, members in groups.items():
            if not all(g.ops[i].bn for i in members):
                continue
            plan, seen = [], set()
            for i in members:
                if i in seen:
                    continue
                mem = pair_of.get(i, (i,))
                if not all(j in members for j in mem):
                    mem = (i,)
                plan.append(tuple(mem))
                seen.update(mem)
            probe = (L.ConvWSrc * len(plan))()
            for j, mem in enumerate(plan):
                o = g.ops[mem[0]]
                probe[j].cout = sum(g.ops[i].dst.c for i in mem)
                probe[j].ldo, probe[j].cooff = (o.dst.c, 0) if o.pooled is not None else (g.tensors[o.dst.tid].c, o.dst.coff)
            o0 = g.ops[members[0]]
            ts0 = g.tensors[o0.src.tid]
            need = lib.din_conv1x1_wgrad_multi_workspace(len(plan), probe, dt, nb * ts0.h * ts0.w, o0.src.c) if 2 <= len(plan) <= 4 else 0
            if need > 0:
                multi_w[key] = (plan, need)
    # layer-grouped weight gradients (din_conv_wgrad_group).  A weight gradient has no consumer inside the reverse pass, so layers whose
    # kernel allows it (the pipelined wide-bank kernel, equal tile instantiation) are QUEUED with their operands and launched up to
    # GROUP_WGRAD_MAX at a time: the launch's 256 workgroups are shared, every layer is cut into a fraction of the pixel slices it would get
    # alone, and its fp32 slice partials (slices x |dW|, ~50 MB per layer and launch whatever the batch) shrink by the same factor.
    group_on = switch("GROUP_WGRAD") and bf16 and not side
    group_max = max(2, min(16, int(L.get_option("DIN_GROUP_WGRAD_MAX") or GROUP_WGRAD_MAX))) if group_on else 0
    group_bytes = int(L.get_option("DIN_GROUP_WGRAD_MB") or GROUP_WGRAD_MB) << 20 if group_on else 0
    # stride-1 convs whose data gradient the library wants on a filter-stationary halo kernel (RF_FAMILIES, each into the plan set of its
    # own): asked once per op, here, with the launch's gradient view and ReLU-mask view (without ACCUM: whether the launch accumulates is
    # known when the pass reaches it, and _BackwardPass.dgrad asks again for one that does)
    rf_sets = {f.plan_set: set() for f in RF_FAMILIES}
    for oi, op in enumerate(g.ops):
        fam = next((f for f in RF_FAMILIES if op.kind == "conv" and f.k == op.k), None)
        if fam and op.s == (1, 1) and op.pooled is None and op.src.tid != g.input_tid:
            d = _conv_desc(g, op, nb, dt)
            if op.bn and bn_train:
                d.ldo, d.cooff = op.dst.c, 0                       # (the gradient operand is the contiguous dy of bn_train_backward)
            masked = g.tensors[op.src.tid].relu_masked
            if getattr(lib, fam.eligible)(C.byref(d), 1, L.CONV_MASK if masked else 0, g.tensors[op.src.tid].c if masked else 0, op.src.coff if masked else 0):
                rf_sets[fam.plan_set].add(oi)
    return BackwardPlan(offsets, bn_index, bn_train, side, bool(u8), groups, member_of, x_host, siblings, multi_w, group_on, group_max,
                        group_bytes, partitioned, first_writer, **rf_sets)


class _Pending(NamedTuple):
    """a member of a 1x1 dgrad group that has been visited: what the group's launches need from it"""
    oi: int
    gout: torch.Tensor          # gradient at its conv output, as a view (ld, coff) of this buffer
    w: torch.Tensor
    scale: Optional[torch.Tensor]
    ld: int
    coff: int
    pre: bool                   # its shift gradient was already taken in front of a commuted pool (din_colsum)


class _Parked(NamedTuple):
    """a lone 1x1's dgrad operands, waiting for the strided sibling that carries them"""
    oi: int
    gout: torch.Tensor
    ld: int
    coff: int


class _Wgrad(NamedTuple):
    """the arguments of one din_conv_wgrad call, launched at once or queued for a grouped launch"""
    d: L.ConvDesc
    x: torch.Tensor
    gout: torch.Tensor
    dw: torch.Tensor
    dshift: Optional[torch.Tensor]
    scale: Optional[torch.Tensor]
    w: Optional[torch.Tensor]
    wdot: Optional[torch.Tensor]
    acc: int
    name: str
    outs: Tuple[Tuple[int, torch.Tensor], ...]      # (op index, its weight gradient inside dw): reported once the launch is enqueued


@dataclass
class _ConvStep:
    """a conv op's turn in the reverse pass: the descriptor of its wgrad / dgrad launches and where the gradient at its conv output lives
    (BatchNorm-train backward and the commuted-pool epilogue replace both)"""
    d: L.ConvDesc
    gout: torch.Tensor
    ld: int
    coff: int
    dshift_pre: Optional[torch.Tensor] = None       # shift gradient already produced in front of a commuted pool


class _BackwardPass:
    """The state of one reverse pass -- gradient buffers and their written ranges, the parameter gradients, the BatchNorm accumulators,
    pending dgrad groups, parked dgrads, weight-gradient queues -- and the steps that change it.  Everything here does; what to fuse,
    group and defer was decided by plan_backward."""

    def __init__(self, g: Graph, plan: BackwardPlan, bufs, aux, params: Sequence[torch.Tensor], dt: int, out_grads: Dict[int, torch.Tensor]):
        self.g, self.plan, self.bufs, self.aux, self.params, self.dt = g, plan, bufs, aux, params, dt
        self.lib = L.load()
        self.nb, self.dev = bufs[g.input_tid].shape[0], bufs[g.input_tid].device
        self.tdt = torch_dtype(dt)
        self.sdt = L.storage_dtype(dt)             # what the data-moving entry points (bn, colsum) take; conv descriptors carry dt itself
        self.st = _stream()
        self.main = torch.cuda.current_stream()
        self.side = side_stream(self.dev) if plan.side else None
        self.gbufs: Dict[int, torch.Tensor] = dict(out_grads)
        self.gwritten: Dict[int, List[Tuple[int, int]]] = {}    # tid -> channel ranges already written (buffers this pass allocated un-zeroed)
        self.grads: List[Optional[torch.Tensor]] = [None] * len(params)
        self.bn = _bn_tables(g, params, self.dev)
        self.pcache = _pack_cache(g, params, dt, self.dev, True, self.bn)     # the forward pass of this step packed both orientations
        if self.bn is not None:
            # flat, pre-zeroed accumulators for every layer's shift gradient and <W, dW> dot (one memset instead of two per layer)
            self.bn_acc = torch.zeros(2 * self.bn.total, dtype=torch.float32, device=self.dev)
            self.bn_dshift, self.bn_wdot = self.bn_acc[:self.bn.total], self.bn_acc[self.bn.total:]
        self.bn_touched = False
        self.remaining = {key: len(v) for key, v in plan.dgrad_groups.items()}
        self.pending: Dict[ViewKey, List[_Pending]] = {key: [] for key in plan.dgrad_groups}
        self.parked: Dict[int, _Parked] = {}                    # strided op index -> the 1x1 dgrad it will carry
        self.wq: Dict[int, List[_Wgrad]] = {}                   # group key -> queued weight gradients
        self.wq_bytes: Dict[int, int] = {}
        self.wgrad_done = set()                                 # members whose weight gradient a sibling's launch produces

    # ---- helpers
    def bn_range(self, first: int, last: Optional[int] = None) -> Tuple[int, int]:
        """the slice of the flat BatchNorm arrays that belongs to op `first` (.. op `last`: adjacent slots)"""
        off, k = self.bn.off_list, self.plan.bn_index
        return off[k[first]], off[k[first if last is None else last] + 1]

    def mask_of(self, view: View):
        """the forward values that mask a gradient into `view` (ReLU backward), or None"""
        return _ptr(self.bufs[view.tid]) if self.g.tensors[view.tid].relu_masked else None

    def on_side(self, tensors):
        """the main stream's work so far is visible to the side stream; the listed tensors stay alive for it"""
        ev = torch.cuda.Event()
        ev.record(self.main)
        self.side.wait_event(ev)
        for t in tensors:
            if t is not None:
                t.record_stream(self.side)
        return C.c_void_p(self.side.cuda_stream)

    def grad_target(self, view: View) -> Tuple[torch.Tensor, bool]:
        """gradient buffer of view.tid and whether to accumulate into it"""
        ts = self.g.tensors[view.tid]
        rng = (view.coff, view.c)
        if view.tid in self.gbufs:
            wr = self.gwritten.get(view.tid)
            if wr is None:                                  # handed in by the caller or zero-filled: always add
                return self.gbufs[view.tid], True
            acc = any(rng[0] < r0 + rc and r0 < rng[0] + rng[1] for r0, rc in wr)
            wr.append(rng)
            return self.gbufs[view.tid], acc
        full = view.coff == 0 and view.c == ts.c
        if full or view.tid in self.plan.partitioned:
            buf = torch.empty((self.nb, ts.h, ts.w, ts.c), dtype=self.tdt, device=self.dev)
            self.gwritten[view.tid] = [rng]
            self.gbufs[view.tid] = buf
            return buf, False
        buf = torch.zeros((self.nb, ts.h, ts.w, ts.c), dtype=self.tdt, device=self.dev)
        self.gbufs[view.tid] = buf
        return buf, True

    def dgrad_flags(self, view: View, acc: bool) -> int:
        return (L.CONV_ACCUM if acc else 0) | (L.CONV_MASK if self.g.tensors[view.tid].relu_masked else 0)

    def report(self, oi: int, dw: torch.Tensor) -> None:
        """op oi's weight gradient is dw and the launch that produces it has been enqueued (on the main stream: GRAD_HOOK may start its
        all-reduce; the side stream's gradients are complete only when the pass ends)"""
        po = self.plan.offsets[oi]
        self.grads[po] = dw
        if GRAD_HOOK is not None and self.side is None:
            GRAD_HOOK(self.params[po], dw)

    # ---- weight gradients: at once, queued for a grouped launch, or one launch for a 1x1 group
    def wgrad_now(self, it: _Wgrad, side_tensors=None) -> None:
        """launch one layer's weight gradient; side_tensors (the tensors it touches): on the side stream, behind everything the main
        stream has enqueued so far"""
        wsbytes = self.lib.din_conv_workspace_bytes(C.byref(it.d), 2)
        if side_tensors is None:
            st = self.st
            ws, wsb = workspace(wsbytes, self.dev)
        else:
            st = self.on_side(side_tensors)
            with torch.cuda.stream(self.side):
                ws, wsb = workspace(wsbytes, self.dev, "side")
        with _timed("wgrad", it.d, it.name):
            L.check(self.lib.din_conv_wgrad(C.byref(it.d), _ptr(it.x), _ptr(it.gout), _ptr(it.dw), _ptr(it.dshift), _ptr(it.scale), _ptr(it.w),
                                            _ptr(it.wdot), it.acc, _ptr(ws), wsb, st), "conv_wgrad " + it.name)
        for oi, dw in it.outs:
            self.report(oi, dw)

    def wgrad_launch(self, it: _Wgrad) -> None:
        """one layer's weight gradient: queued for a grouped launch when its kernel allows it, launched at once otherwise"""
        plan = self.plan
        key = self.lib.din_conv_wgrad_group_key(C.byref(it.d)) if plan.group_on else 0
        if not key:
            self.wgrad_now(it)
            return
        d = it.d
        q = self.wq.setdefault(key, [])
        q.append(it._replace(d=_copy_desc(d)))
        held = self.wq_bytes.get(key, 0) + 2 * (d.nb * d.h * d.w * d.cin + d.nb * d.oh * d.ow * d.cout)      # bf16 operands held back
        self.wq_bytes[key] = held
        if wgrad_queue_full(len(q), held, plan.group_max, plan.group_bytes):
            self.flush_wq(key)

    def flush_wq(self, key: int) -> None:
        q = self.wq.pop(key, None)
        self.wq_bytes.pop(key, None)
        if not q:
            return
        need = 0
        if len(q) > 1:
            items = (L.ConvWgradItem * len(q))()
            for item, it in zip(items, q):
                item.desc = it.d
                item.in_, item.dout, item.dw = it.x.data_ptr(), it.gout.data_ptr(), it.dw.data_ptr()
                item.dbias = it.dshift.data_ptr() if it.dshift is not None else None
                item.scale = it.scale.data_ptr() if it.scale is not None else None
                item.w = it.w.data_ptr() if it.w is not None else None
                item.wdot = it.wdot.data_ptr() if it.wdot is not None else None
                item.accumulate = it.acc
            need = self.lib.din_conv_wgrad_group_workspace(len(q), items)
        if need <= 0:                                           # a single layer (or a list the library does not take as one launch)
            for it in q:
                self.wgrad_now(it)
            return
        ws, wsb = workspace(need, self.dev, "wgroup")
        dG = _copy_desc(q[0].d)
        dG.flops_override = float(sum(2.0 * it.d.nb * it.d.oh * it.d.ow * it.d.cout * it.d.cin * it.d.kh * it.d.kw for it in q))
        with _timed("wgrad", dG, "group:" + "+".join(it.name for it in q)):
            L.check(self.lib.din_conv_wgrad_group(len(q), items, _ptr(ws), wsb, self.st), "conv_wgrad_group " + q[0].name + "+")
        for it in q:
            for oi, dw in it.outs:
                self.report(oi, dw)

    def flush_wgrad_multi(self, key: ViewKey, items: List[_Pending]) -> None:
        """the deferred weight gradients of a 1x1 group (plan.multi_w): ONE launch reads the block input once and produces every member's dW"""
        g, lib, params, offsets = self.g, self.lib, self.params, self.plan.offsets
        by_oi = {it.oi: it for it in items}
        op0 = g.ops[items[0].oi]
        ts0 = g.tensors[op0.src.tid]
        sources, wsb_need = self.plan.multi_w[key]
        self.bn_touched = True
        if any(i not in by_oi for mem in sources for i in mem):
            # A member received no gradient (a graph that consumes only some branch outputs -- partial heads; not the backbones here): the
            # fused launch's plan does not apply, so the members that DID get one degrade to the per-layer kernel (this used
            # to raise in the middle of backward, after the weight gradients had already been deferred)
            for it in items:
                opj = g.ops[it.oi]
                dj = _conv_desc(g, opj, self.nb, self.dt)
                dj.ldo, dj.cooff = it.ld, it.coff
                o0, o1 = self.bn_range(it.oi)
                dwj = _dw_buffer(it.w)
                self.wgrad_now(_Wgrad(dj, self.bufs[opj.src.tid], it.gout, dwj, None if it.pre else self.bn_dshift[o0:o1], it.scale, it.w,
                                      self.bn_wdot[o0:o1], 2, opj.name, ((it.oi, dwj),)))
            return
        srcs = (L.ConvWSrc * len(sources))()
        outs = []
        for j, mem in enumerate(sources):
            first = by_oi[mem[0]]
            o0, o1 = self.bn_range(mem[0], mem[-1])
            if len(mem) == 1:
                wj = params[offsets[mem[0]]]
                dwj = _dw_buffer(wj)
            else:
                wj = torch.cat([params[offsets[i]] for i in mem])
                dwj = torch.empty_like(wj)
            srcs[j].dout, srcs[j].dw = first.gout.data_ptr(), dwj.data_ptr()
            srcs[j].dbias = 0 if first.pre else self.bn_dshift[o0:o1].data_ptr()
            srcs[j].scale, srcs[j].w, srcs[j].wdot = self.pcache.bn_scale[o0:o1].data_ptr(), wj.data_ptr(), self.bn_wdot[o0:o1].data_ptr()
            srcs[j].cout, srcs[j].ldo, srcs[j].cooff = o1 - o0, first.ld, first.coff
            outs.append((mem, wj, dwj))                          # (wj: a concatenation lives until the launch below is enqueued)
        ws, wsb = workspace(wsb_need, self.dev)
        dM = _conv_desc(g, op0, self.nb, self.dt)
        dM.cout = sum(s.cout for s in srcs)                      # FLOP accounting of the fused launch
        with _timed("wgrad", dM, "1x1multi:" + "+".join(g.ops[i].name for mem in sources for i in mem)):
            L.check(lib.din_conv1x1_wgrad_multi(len(sources), srcs, self.dt, self.nb * ts0.h * ts0.w, op0.src.c, ts0.c, op0.src.coff,
                                                _ptr(self.bufs[op0.src.tid]), 2, _ptr(ws), wsb, self.st), "conv1x1_wgrad_multi")
        for mem, _wj, dwj in outs:
            r0 = 0
            for i in mem:
                c = g.ops[i].dst.c
                self.report(i, dwj if len(mem) == 1 else dwj[r0:r0 + c])
                r0 += c

    # ---- data gradients of the 1x1 groups and of a parked 1x1
    def visited(self, key: ViewKey) -> None:
        """one more member of a 1x1 group has had its turn (with or without a gradient): the last one launches the group"""
        self.remaining[key] -= 1
        if self.remaining[key] == 0:
            self.flush_group(key)

    def flush_group(self, key: ViewKey) -> None:
        items = self.pending[key]
        if not items:
            return
        g = self.g
        if key in self.plan.multi_w:
            self.flush_wgrad_multi(key, items)
        op0 = g.ops[items[0].oi]
        ts0 = g.tensors[op0.src.tid]
        gsrc, acc = self.grad_target(op0.src)
        srcs = (L.ConvSrc * len(items))()
        for j, it in enumerate(items):
            srcs[j].dout, srcs[j].wpk_t = it.gout.data_ptr(), self.pcache.wpt[it.oi].data_ptr()
            srcs[j].cout, srcs[j].ldo, srcs[j].cooff = g.ops[it.oi].dst.c, it.ld, it.coff
        d0 = _conv_desc(g, op0, self.nb, self.dt)
        d0.src_couts = tuple(g.ops[it.oi].dst.c for it in items)   # (measurement side: profiling.LaunchTimer names the instantiation from it)
        d0.cout = sum(d0.src_couts)                                # FLOP accounting of the fused launch
        with _timed("dgrad", d0, "+".join(g.ops[it.oi].name for it in items)):
            L.check(self.lib.din_conv1x1_dgrad_multi(len(items), srcs, self.dt, self.nb, ts0.h, ts0.w, op0.src.c, ts0.c, op0.src.coff, _ptr(gsrc),
                                                     self.mask_of(op0.src), ts0.c, op0.src.coff, self.dgrad_flags(op0.src, acc), self.st),
                    "conv1x1_dgrad_multi")
        self.pending[key] = []

    def dgrad_parked(self, host_oi: int) -> None:
        """the strided conv that was to carry a parked 1x1 dgrad received no gradient itself: the 1x1's dgrad runs alone"""
        pk = self.parked.pop(host_oi)
        opj = self.g.ops[pk.oi]
        dj = _conv_desc(self.g, opj, self.nb, self.dt)
        dj.ldo, dj.cooff = pk.ld, pk.coff
        self.dgrad(pk.oi, dj, pk.gout)

    def dgrad(self, oi: int, d: L.ConvDesc, gout: torch.Tensor) -> None:
        """one conv's data gradient into its source view; a strided conv carries the 1x1 parked with it in the same launches"""
        op = self.g.ops[oi]
        ts = self.g.tensors[op.src.tid]
        gsrc, acc = self.grad_target(op.src)
        wpt = self.pcache.wpt[oi]
        flags = self.dgrad_flags(op.src, acc)
        ws, wsb = workspace(self.lib.din_conv_workspace_bytes(C.byref(d), 1), self.dev)
        pk = self.parked.pop(oi, None)
        if pk is not None:
            xs = L.ConvSrc()
            xs.dout, xs.wpk_t = pk.gout.data_ptr(), self.pcache.wpt[pk.oi].data_ptr()
            xs.cout, xs.ldo, xs.cooff = self.g.ops[pk.oi].dst.c, pk.ld, pk.coff
            with _timed("dgrad", d, op.name + "+" + self.g.ops[pk.oi].name):
                L.check(self.lib.din_conv_dgrad_x(C.byref(d), _ptr(gout), _ptr(wpt), _ptr(gsrc), self.mask_of(op.src), ts.c, op.src.coff, flags,
                                                  C.byref(xs), _ptr(ws), wsb, self.st), "conv_dgrad_x " + op.name)
        else:
            fam = next((f for f in RF_FAMILIES if oi in getattr(self.plan, f.plan_set)), None)
            if fam and acc and not getattr(self.lib, fam.eligible)(C.byref(d), 1, flags, ts.c, op.src.coff):
                fam = None                                           # (the plan asked without ACCUM: an accumulating launch gets its own answer)
            d.rf = (fam.names, flags, ts.c, op.src.coff) if fam else None       # (the launch timer names the kernel from this reporter)
            fn = getattr(self.lib, fam.dgrad if fam else "din_conv_dgrad")
            with _timed("dgrad", d, op.name):
                L.check(fn(C.byref(d), _ptr(gout), _ptr(wpt), _ptr(gsrc), self.mask_of(op.src), ts.c, op.src.coff, flags, _ptr(ws), wsb, self.st),
                        "conv_dgrad " + op.name)

    # ---- the steps of the loop, one op at a time
    def skip(self, oi: int) -> None:
        """nothing flows back through op oi: it still counts as a visited group member, and what was parked with it runs alone"""
        key = self.plan.member_of.get(oi)
        if key is not None:
            self.visited(key)
        if oi in self.parked:
            self.dgrad_parked(oi)

    def conv_step(self, oi: int, gout: torch.Tensor) -> _ConvStep:
        g, op = self.g, self.g.ops[oi]
        image = op.src.tid == g.input_tid
        d = _conv_desc(g, op, self.nb, self.dt, g.cin_image if image else op.src.c)
        if image and self.plan.u8:
            d.in_u8, d.ldi, d.cioff = 1, 8, 0
        return _ConvStep(d, gout, g.tensors[op.dst.tid].c, op.dst.coff)

    def bn_train_backward(self, oi: int, c: _ConvStep) -> None:
        """batch-statistics BatchNorm backward: gz (masked by the ReLU that follows) -> dy at the raw conv output, dgamma, dbeta"""
        g, lib, op, nb, dev, st = self.g, self.lib, self.g.ops[oi], self.nb, self.dev, self.st
        po, cout = self.plan.offsets[oi], op.dst.c
        _, raw, bmean, rstd = self.aux[oi]
        td = g.tensors[op.dst.tid]
        rows = nb * td.h * td.w
        sums = torch.empty(lib.din_bn_workspace(rows, cout) // 8, dtype=torch.float64, device=dev)
        L.check(lib.din_bn_bwd_stats(_ptr(c.gout), c.ld, c.coff, _ptr(raw), cout, 0, self.sdt, rows, cout, _ptr(bmean), _ptr(rstd),
                                     _ptr(sums), st), "bn_bwd_stats")
        dy = torch.empty((nb, td.h, td.w, cout), dtype=self.tdt, device=dev)
        dgb = torch.empty(2 * cout, dtype=torch.float32, device=dev)
        L.check(lib.din_bn_bwd_apply(_ptr(c.gout), c.ld, c.coff, _ptr(raw), cout, 0, self.sdt, rows, cout, _ptr(self.params[po + 1]), _ptr(bmean),
                                     _ptr(rstd), _ptr(sums), _ptr(dy), cout, 0, _ptr(dgb), _ptr(dgb[cout:]), st), "bn_bwd_apply")
        self.grads[po + 1], self.grads[po + 2] = dgb[:cout], dgb[cout:]
        c.gout, c.ld, c.coff = dy, cout, 0
        c.d.ldo, c.d.cooff = cout, 0                               # the gradient operand of wgrad / dgrad is the contiguous dy
        if op.pooled is not None:
            c.d, pd = _pooled_descs(g, op, nb, self.dt)
            gtmp = torch.empty((nb, pd.h, pd.w, pd.c), dtype=self.tdt, device=dev)
            pd.ldo, pd.cooff = cout, 0                             # the pooled-side gradient is the contiguous dy
            L.check(lib.din_avgpool_bwd(C.byref(pd), _ptr(c.gout), _ptr(gtmp), None, 0, st), "avgpool_bwd(raw)")
            c.gout = gtmp

    def pooled_epilogue(self, oi: int, c: _ConvStep) -> None:
        """y = relu(avgpool(conv1x1(x)) + shift): shift gradient = column sums of gout, conv-output gradient = avgpool^T(gout)"""
        g, lib, op = self.g, self.lib, self.g.ops[oi]
        c.d, pd = _pooled_descs(g, op, self.nb, self.dt)
        td = g.tensors[op.dst.tid]
        if op.bn or op.bias:
            if op.bn:                                   # straight into this layer's slice of the flat accumulator
                o0, o1 = self.bn_range(oi)
                c.dshift_pre = self.bn_dshift[o0:o1]
            else:
                c.dshift_pre = torch.empty(op.dst.c, dtype=torch.float32, device=self.dev)
            L.check(lib.din_colsum(_ptr(c.gout), self.sdt, self.nb * td.h * td.w, op.dst.c, td.c, op.dst.coff, _ptr(c.dshift_pre), self.st), "colsum")
        gtmp = torch.empty((self.nb, pd.h, pd.w, pd.c), dtype=self.tdt, device=self.dev)
        L.check(lib.din_avgpool_bwd(C.byref(pd), _ptr(c.gout), _ptr(gtmp), None, 0, self.st), "avgpool_bwd(epilogue)")
        c.gout, c.ld, c.coff = gtmp, pd.c, 0

    def weight_gradient(self, oi: int, c: _ConvStep) -> None:
        """op oi's weight gradient (+ bias / BatchNorm parameter gradients): deferred to its 1x1 group's launch, produced by a sibling's
        launch, one launch for the siblings that share a tensor, or its own -- queued, at once, or on the side stream"""
        g, plan, lib, op, params = self.g, self.plan, self.lib, self.g.ops[oi], self.params
        if plan.member_of.get(oi) in plan.multi_w and op.src.tid != g.input_tid:
            return                                                # produced when its 1x1 group is flushed (flush_wgrad_multi)
        if oi in self.wgrad_done:
            return                                                # produced by the launch of a sibling (below)
        po = plan.offsets[oi]
        w, scale, x, d = params[po], self.aux[oi][0], self.bufs[op.src.tid], c.d
        if oi in plan.siblings:
            # the members of a forward group that share the second tensor: their output gradients are adjacent channel views of ONE
            # buffer, their BatchNorm slots adjacent -> one wgrad over the concatenated filter rows; dW lands in one buffer whose
            # row ranges are the members' gradients
            mem = plan.siblings[oi]
            mops = [g.ops[i] for i in mem]
            dF = _conv_desc(g, mops[0], self.nb, self.dt, d.cin)
            dF.cout = sum(o.dst.c for o in mops)
            o0, o1 = self.bn_range(mem[0], mem[-1])
            assert o1 - o0 == dF.cout
            wcat = torch.cat([params[plan.offsets[i]] for i in mem])
            dwf = torch.empty_like(wcat)
            self.bn_touched = True
            outs, r0 = [], 0
            for i, o in zip(mem, mops):
                outs.append((i, dwf[r0:r0 + o.dst.c]))
                r0 += o.dst.c
            self.wgrad_done.update(mem)
            self.wgrad_launch(_Wgrad(dF, x, c.gout, dwf, self.bn_dshift[o0:o1], self.pcache.bn_scale[o0:o1], wcat, self.bn_wdot[o0:o1], 2,
                                     "+".join(o.name for o in mops), tuple(outs)))
        elif op.bn and plan.bn_train:
            dw = _dw_buffer(w)
            self.wgrad_now(_Wgrad(d, x, c.gout, dw, None, None, None, None, 0, op.name, ((oi, dw),)))
        elif op.bn:
            dw = _dw_buffer(w)
            o0, o1 = self.bn_range(oi)
            dshift = None if c.dshift_pre is not None else self.bn_dshift[o0:o1]     # views of the pre-zeroed flat accumulators
            it = _Wgrad(d, x, c.gout, dw, dshift, scale, w, self.bn_wdot[o0:o1], 2, op.name, ((oi, dw),))
            self.bn_touched = True
            if self.side is not None:
                self.wgrad_now(it, [x, c.gout, dw, self.bn_acc, scale])
            else:
                self.wgrad_launch(it)
        else:
            dw = _dw_buffer(w)
            db = (c.dshift_pre if c.dshift_pre is not None else torch.empty_like(params[po + 1])) if op.bias else None
            it = _Wgrad(d, x, c.gout, dw, None if c.dshift_pre is not None else db, None, None, None, 0, op.name, ((oi, dw),))
            self.wgrad_now(it, [x, c.gout, dw, db] if self.side is not None else None)
            if op.bias:
                self.grads[po + 1] = db

    def data_gradient(self, oi: int, c: _ConvStep) -> None:
        """op oi's data gradient: with its 1x1 group, parked for the strided sibling that will carry it, or its own launch"""
        plan, op = self.plan, self.g.ops[oi]
        key = plan.member_of.get(oi)
        if key is not None:
            self.pending[key].append(_Pending(oi, c.gout, self.params[plan.offsets[oi]], self.aux[oi][0], c.ld, c.coff, c.dshift_pre is not None))
            self.visited(key)
        elif oi in plan.x_host and c.dshift_pre is None:
            self.parked[plan.x_host[oi]] = _Parked(oi, c.gout, c.ld, c.coff)      # carried by the strided sibling's dgrad, when the pass reaches it
        else:
            self.dgrad(oi, c.d, c.gout)

    def pool_backward(self, oi: int, gout: torch.Tensor) -> None:
        op, lib = self.g.ops[oi], self.lib
        relu_masked = self.g.tensors[op.src.tid].relu_masked
        d = _pool_desc(self.g, op, self.nb, self.dt)
        gsrc, acc = self.grad_target(op.src)
        if op.kind == "maxpool":
            (amax,) = self.aux[oi]
            L.check(lib.din_maxpool_bwd(C.byref(d), _ptr(self.bufs[op.src.tid]), _ptr(amax), _ptr(gout), _ptr(gsrc), int(relu_masked), int(acc),
                                        self.st), "maxpool_bwd")
        elif op.kind == "avgpool":
            L.check(lib.din_avgpool_bwd(C.byref(d), _ptr(gout), _ptr(gsrc), self.mask_of(op.src), int(acc), self.st), "avgpool_bwd")
        else:
            L.check(lib.din_bilinear_bwd(C.byref(d), _ptr(gout), _ptr(gsrc), self.mask_of(op.src), int(acc), self.st), "bilinear_bwd")

    def finish(self) -> List[Optional[torch.Tensor]]:
        """the final flushes and the BatchNorm parameter gradients; returns the parameter gradients"""
        for key in list(self.wq):
            self.flush_wq(key)                         # weight gradients still queued for a grouped launch
        #  a 1x1's parked data gradient is only consumed when its strided host op has its turn: a graph whose host takes
        # another path must not drop it silently
        if self.parked:
            raise L.DinError(f"graph_backward: parked 1x1 data gradients were never carried by their strided sibling (ops {sorted(self.parked)}): "
                             "the fused strided + 1x1 dgrad (din_conv_dgrad_x) does not serve this graph shape")
        if self.side is not None:
            self.main.wait_stream(self.side)           # parameter gradients are complete for whoever runs next on the main stream
        bn, grads, offsets = self.bn, self.grads, self.plan.offsets
        if bn is not None and self.bn_touched and not self.plan.bn_train:
            # BatchNorm parameter gradients of every layer in one launch: dgamma = (wdot - dshift * mean) * rstd, dbeta = dshift
            bn_out = torch.empty(2 * bn.total, dtype=torch.float32, device=self.dev)
            L.check(self.lib.din_bn_fold_bwd_multi(_ptr(bn.ptrs), _ptr(bn.offs), bn.n, bn.total, BN_EPS, _ptr(self.bn_wdot), _ptr(self.bn_dshift),
                                                   _ptr(bn_out), _ptr(bn_out[bn.total:]), self.st), "bn_fold_bwd_multi")
            for oi, k in self.plan.bn_index.items():
                if grads[offsets[oi]] is not None:     # the layer took part in this backward
                    o0, o1 = bn.off_list[k], bn.off_list[k + 1]
                    grads[offsets[oi] + 1], grads[offsets[oi] + 2] = bn_out[o0:o1], bn_out[bn.total + o0:bn.total + o1]
        return grads


def graph_backward(g: Graph, bufs, aux, params: Sequence[torch.Tensor], dt: int,
                   out_grads: Dict[int, torch.Tensor], need_param_grad: Sequence[bool], bn_train: bool = False):
    """Reverse pass.  out_grads: tid -> gradient buffer (same geometry/dtype as the tensor, already ReLU-masked where
    the tensor is relu_masked).  Returns the list of parameter gradients aligned with `params` (None for buffers).
    need_param_grad is not read (every weight gradient is computed; NHWCGraphFunction.backward drops the unwanted ones)."""
    image = bufs[g.input_tid]
    plan = plan_backward(g, image.shape[0], dt, bn_train, not TIMING_ACTIVE(), image.dtype == torch.uint8)
    bp = _BackwardPass(g, plan, bufs, aux, params, dt, out_grads)
    for oi in range(len(g.ops) - 1, -1, -1):
        op = g.ops[oi]
        if op.dst.tid not in bp.gbufs:
            bp.skip(oi)                                # nothing flows back through this op
            continue
        gout = bp.gbufs[op.dst.tid]
        if GRAD_TAP is not None:
            GRAD_TAP(op.dst.tid, op.name, gout)
        if op.kind == "conv":
            c = bp.conv_step(oi, gout)
            if op.bn and plan.bn_train:
                bp.bn_train_backward(oi, c)
            elif op.pooled is not None:
                bp.pooled_epilogue(oi, c)
            bp.weight_gradient(oi, c)
            if op.src.tid != g.input_tid:
                bp.data_gradient(oi, c)
        elif op.src.tid != g.input_tid:
            bp.pool_backward(oi, gout)
        if plan.first_writer[op.dst.tid] == oi:        # the gradient of dst is dead once all its producers ran
            bp.gbufs.pop(op.dst.tid, None)
    return bp.finish()


def _accepts_u8_frames(g: Graph, nb: int, dt: int) -> bool:
    """True when the only reader of the graph input is a conv whose forward and weight-gradient launches take the image-layer kernels
    that read uint8 frames directly (din_conv_accepts_u8): Inception's Conv2d_1a_3x3 at full frame size in bf16."""
    readers = [op for op in g.ops if op.src.tid == g.input_tid]
    if len(readers) != 1 or readers[0].kind != "conv" or readers[0].pooled is not None:
        return False
    key = (nb, dt)
    cache = g.u8_ok
    if key not in cache:
        d = _conv_desc(g, readers[0], nb, dt, g.cin_image)
        d.ldi, d.cioff = 8, 0
        cache[key] = bool(L.load().din_conv_accepts_u8(C.byref(d)))
    return cache[key]


class NHWCGraphFunction(torch.autograd.Function):
    """images (uint8|fp32 NCHW, 0..255) -> output NHWC buffers.  One autograd node for the whole conv stack."""

    @staticmethod
    def forward(ctx, graph: Graph, dt: int, images: torch.Tensor, prenormalised: bool, bn_train: bool, *params):
        lib = L.load()
        require_gpu(images, *params)
        nb, _, h, w = images.shape
        ti = graph.tensors[graph.input_tid]
        assert (h, w) == (ti.h, ti.w), f"image {h}x{w} does not match the graph ({ti.h}x{ti.w})"
        st = _stream()
        if not prenormalised and images.dtype == torch.uint8 and _accepts_u8_frames(graph, nb, dt):
            # the image layer (forward and weight gradient) reads the uint8 frames itself: no prepared NHWC copy of the clip batch
            img = images.contiguous()
        elif prenormalised:
            img = torch.empty((nb, h, w, ti.c), dtype=torch_dtype(dt), device=images.device)
            if ti.c > 3:
                img.zero_()
            L.check(lib.din_nchw_f32_to_nhwc(_ptr(images.float().contiguous()), nb, h, w, 3, _ptr(img), L.storage_dtype(dt), ti.c, 0, st),
                    "nchw_to_nhwc")
        else:
            img = torch.empty((nb, h, w, ti.c), dtype=torch_dtype(dt), device=images.device)
            if images.dtype == torch.uint8:
                L.check(lib.din_prep_images_nhwc(_ptr(images), 1, _ptr(img), L.storage_dtype(dt), nb, h, w, ti.c, st), "prep_nhwc")
            else:
                L.check(lib.din_prep_images_nhwc(_ptr(images.float().contiguous()), 0, _ptr(img), L.storage_dtype(dt), nb, h, w, ti.c, st),
                        "prep_nhwc")
        with torch.no_grad():
            bufs, aux = graph_forward(graph, img, params, dt, save_for_backward=any(p.requires_grad for p in params), bn_train=bn_train)
        ctx.graph, ctx.dt, ctx.bufs, ctx.aux, ctx.bn_train = graph, dt, bufs, aux, bn_train
        ctx.params = params
        ctx.need = [p.requires_grad for p in params]
        outs = tuple(bufs[t] for t in graph.output_tids)
        ctx.set_materialize_grads(False)                   # an unused output must not cost a zero-filled gradient map (0.5 GB for Mixed_6e)
        return outs if len(outs) > 1 else outs[0]

    @staticmethod
    def backward(ctx, *gouts):
        graph = ctx.graph
        og = {}
        for tid, go in zip(graph.output_tids, gouts):
            if go is not None:
                og[tid] = go.contiguous()
        with torch.no_grad():
            grads = graph_backward(graph, ctx.bufs, ctx.aux, ctx.params, ctx.dt, og, ctx.need, ctx.bn_train)
        ctx.bufs = ctx.aux = None
        grads = [gr if need else None for gr, need in zip(grads, ctx.need)]
        if GRAD_ASSIGN is not None:
            grads = [None if (gr is not None and GRAD_ASSIGN(p_, gr)) else gr for p_, gr in zip(ctx.params, grads)]
        return (None, None, None, None, None, *grads)
