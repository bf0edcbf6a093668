"""torch.autograd.Function wrappers over the C ABI for everything after the backbone (rows R, E, L, D, H).

Each Function's forward/backward is a handful of C calls; PyTorch provides device memory, the current HIP stream and
the autograd tape only.  All tensors here are fp32 (the tail of the path is always fp32, include/din_hip.h).
"""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib as L
from .nhwc import _ptr, _stream, din_dtype, require_gpu, workspace


# Device-side per-step part of every dropout seed (int64 [1]) or None.  A training step captured in a HIP graph (din_amd.graph_step) bakes
# the host-computed seeds into the launches; the kernels add *SEED_OFFSET, which the captured step advances once per replay.
SEED_OFFSET: Optional[torch.Tensor] = None


DETERMINISTIC_OPTION = "DIN_DETERMINISTIC"


@contextlib.contextmanager
def deterministic(on: bool = True):
    """Inside the block every gradient sum of the frozen-backbone stage-2 path (walk dx, LayerNorm dgamma / dbeta, head dw / dbias,
    dot_accum, the bias gradient of linear / GridConvFunction) runs its fixed-order kernel: same inputs, same bits, whatever the wave
    schedule (include/din_hip.h: DIN_DETERMINISTIC).  on=False switches the option off inside the block.  Options are process-wide: the
    previous value is put back on exit, also when the block raises.  What has no ordered form (a trained backbone's BatchNorm-scale
    gradient, for one) raises DinError under the option instead of running atomics."""
    before = L.get_option(DETERMINISTIC_OPTION)
    L.set_option(DETERMINISTIC_OPTION, 1 if on else None)
    try:
        yield
    finally:
        L.set_option(DETERMINISTIC_OPTION, before)


def deterministic_refusal(cfg, world: int) -> Optional[str]:
    """why cfg.deterministic cannot be honoured, or None (train_net_dynamic.train_net raises ValueError with it)"""
    if not getattr(cfg, "deterministic", False):
        return None
    if cfg.train_backbone:
        return ("deterministic = True: train_backbone is set, and the backbone's bias / BatchNorm-scale gradients and the RoIAlign backward "
                "still sum with atomics; the mode covers the frozen backbone")
    if world > 1:
        return (f"deterministic = True: {world} ranks, and the order in which the gradient all-reduce sums the ranks is RCCL's; the mode "
                f"covers one rank")
    return None


# ------------------------------------------------------------------------------------------------
# Row P (API-parity form)
# ------------------------------------------------------------------------------------------------
def prep_images_f32(images: torch.Tensor) -> torch.Tensor:
    lib = L.load()
    x = images.float().contiguous()
    require_gpu(x)
    out = torch.empty_like(x)
    L.check(lib.din_prep_images_f32(_ptr(x), _ptr(out), x.numel(), _stream()), "prep_images")
    return out


def boxes_frame_index(bt: int, n: int, device) -> torch.Tensor:
    """infer_model.py:155-157 -- int32 [bt*n], box i*n+j crops from frame i."""
    lib = L.load()
    out = torch.empty(bt * n, dtype=torch.int32, device=device)
    require_gpu(out)
    L.check(lib.din_boxes_frame_index(_ptr(out), bt, n, _stream()), "boxes_frame_index")
    return out


# ------------------------------------------------------------------------------------------------
# Row R: RoIAlign
# ------------------------------------------------------------------------------------------------
def _roi_forward(lib, fms, chans, grid, boxes, box_ind, k, want_index):
    """crops fp32 [m, sum(chans), k, k]: one launch per stored map, each writes its channel range (the torch.cat of infer_model.py:172)"""
    m, ctot = boxes.shape[0], sum(chans)
    out = torch.empty((m, ctot, k, k), dtype=torch.float32, device=boxes.device)
    idx = torch.empty((m, k, k, 6), dtype=torch.int32, device=boxes.device) if want_index else None
    coff = 0
    for fm, c in zip(fms, chans):
        nb, hf, wf, ld = fm.shape
        gh, gw = grid if grid is not None else (hf, wf)
        L.check(lib.din_roi_align_fwd(_ptr(fm), din_dtype(fm), nb, hf, wf, c, ld, gh, gw, _ptr(boxes), _ptr(box_ind), m, k,
                                      _ptr(out), ctot, coff, _ptr(idx) if (hf, wf) == (gh, gw) else None, _stream()), "roi_align_fwd")
        coff += c
    return out, idx


def _roi_backward(lib, gout, fms, chans, masked, grid, boxes, box_ind, k):
    """gather form: every stored map's gradient tensor is written once, in the map's storage type, already multiplied by the ReLU mask
    of the map (no fp32 scatter buffer, no cast pass); with a larger box grid this is also the backward of the bilinear resize"""
    st = _stream()
    m, ctot = boxes.shape[0], sum(chans)
    gout = gout.contiguous().float()
    src, transposed = gout, 0
    if ctot % 4 == 0 and all(c % 4 == 0 for c in chans):
        src, transposed = torch.empty_like(gout), 1                  # channel-contiguous copy of the crop gradient, shared by the maps
        L.check(lib.din_roi_crop_grad_transpose(_ptr(gout), m, ctot, k, _ptr(src), st), "roi_crop_grad_transpose")
    grads, coff = [], 0
    for fm, c, mk in zip(fms, chans, masked):
        nb, hf, wf, ld = fm.shape
        gh, gw = grid if grid is not None else (hf, wf)
        gfm = torch.zeros_like(fm) if ld != c else torch.empty_like(fm)
        L.check(lib.din_roi_align_bwd_nhwc(_ptr(src), ctot, coff, transposed, nb, hf, wf, c, gh, gw, _ptr(boxes), _ptr(box_ind), m, k,
                                           _ptr(fm) if mk else None, din_dtype(fm), ld, _ptr(gfm), ld, st), "roi_align_bwd_nhwc")
        grads.append(gfm)
        coff += c
    return grads


class RoIAlignFunction(torch.autograd.Function):
    """fm: NHWC buffer [nb,hf,wf,ld] (fp32|bf16) -> crops fp32 [m, c, k, k] (reference flatten order)."""

    @staticmethod
    def forward(ctx, fm: torch.Tensor, boxes: torch.Tensor, box_ind: torch.Tensor, k: int, c: int, relu_masked: bool,
                want_index: bool = False):
        lib = L.load()
        boxes = boxes.detach().float().contiguous()
        box_ind = box_ind.detach().to(torch.int32).contiguous()
        require_gpu(fm, boxes, box_ind)
        out, idx = _roi_forward(lib, [fm], [c], None, boxes, box_ind, k, want_index)
        ctx.save_for_backward(fm, boxes, box_ind)
        ctx.k, ctx.c, ctx.relu_masked = k, c, relu_masked
        if want_index:
            ctx.mark_non_differentiable(idx)
            return out, idx
        return out

    @staticmethod
    def backward(ctx, gout, *_):
        fm, boxes, box_ind = ctx.saved_tensors
        (gfm,) = _roi_backward(L.load(), gout, [fm], [ctx.c], [ctx.relu_masked], None, boxes, box_ind, ctx.k)
        return gfm, None, None, None, None, None, None


class RoIAlignMultiScaleFunction(torch.autograd.Function):
    """RoIAlign over torch.cat([resize(fm_i, grid) for fm_i in fms], channel) without building it (infer_model.py:165-180): boxes are
    in `grid` = (OH, OW) pixels, every stored map fm_i [nb,h_i,w_i,ld_i] (h_i <= OH, w_i <= OW) is sampled through its virtual
    align_corners resize, and the backward writes each map's gradient directly.  chans / masked: per-map channel count and "apply the
    map's ReLU mask" flag.  Returns crops fp32 [m, sum(chans), k, k]."""

    @staticmethod
    def forward(ctx, boxes: torch.Tensor, box_ind: torch.Tensor, k: int, grid, chans, masked, *fms):
        lib = L.load()
        boxes = boxes.detach().float().contiguous()
        box_ind = box_ind.detach().to(torch.int32).contiguous()
        require_gpu(boxes, box_ind, *fms)
        out, _ = _roi_forward(lib, fms, list(chans), tuple(grid), boxes, box_ind, k, False)
        ctx.save_for_backward(boxes, box_ind, *fms)
        ctx.k, ctx.grid, ctx.chans, ctx.masked = k, tuple(grid), list(chans), list(masked)
        return out

    @staticmethod
    def backward(ctx, gout):
        boxes, box_ind, *fms = ctx.saved_tensors
        grads = _roi_backward(L.load(), gout, fms, ctx.chans, ctx.masked, ctx.grid, boxes, box_ind, ctx.k)
        return (None, None, None, None, None, None, *grads)


# ------------------------------------------------------------------------------------------------
# dense contractions on the MFMA conv kernel (fp32): Linear and the (T x N)-grid p_conv/scale_conv
# ------------------------------------------------------------------------------------------------
def _desc(nb, h, w, cin, cout, kh, kw, ph, pw, dil, ldi, ldo) -> L.ConvDesc:
    d = L.ConvDesc()
    d.nb, d.h, d.w, d.cin = nb, h, w, cin
    d.oh, d.ow, d.cout = h, w, cout          # "same" geometry (stride 1, symmetric dilation-scaled padding)
    d.kh, d.kw, d.sh, d.sw, d.ph, d.pw, d.dh, d.dw = kh, kw, 1, 1, ph, pw, dil, dil
    d.ldi, d.cioff, d.ldo, d.cooff = ldi, 0, ldo, 0
    d.dtype = L.DIN_F32
    return d


class GridConvFunction(torch.autograd.Function):
    """x [nb,h,w,cin] fp32 NHWC, weight [cout,cin,kh,kw], bias [cout]|None -> y [nb,h,w,ldo] (ldo = cout padded to 4,
    padding channels are zero).  Stride 1, padding = (k-1)//2*dil: nn.Linear (1x1), point_conv (infer_model.py:190) and
    the fused p_conv/scale_conv (dynamic_infer_module.py:191,195)."""

    @staticmethod
    def forward(ctx, x, weight, bias, dil: int, lowp: bool = False, split: bool = False):
        """lowp: bf16 operands / fp32 MFMA accumulation (throughput mode, used for the 26400-wide embedding GEMM when the backbone
        already runs in bf16); x, y and all gradients stay fp32 tensors at the interface -- except that x may arrive as the bf16 operand
        itself (rows of the bf16 feature cache): it is then used and saved as it is, and without effective lowp it is a ValueError.
        split: fp32 storage, three-part bf16 MFMA compute (DIN_F32_BF16X3: fp32 accuracy on the bf16 matrix pipe) for the forward, the data
        gradient and the weight gradient; every tensor and buffer is what the exact fp32 call makes.  Not together with lowp."""
        if lowp and split:
            raise ValueError("lowp and split are mutually exclusive: bf16 storage or fp32 storage with three-part bf16 compute")
        lib = L.load()
        x = x.contiguous()
        weight = weight.contiguous()
        require_gpu(x, weight, bias)
        nb, h, w, cin = x.shape
        cout, _, kh, kw = weight.shape
        lowp = bool(lowp) and cin % 8 == 0 and cout % 8 == 0
        tdt = torch.bfloat16 if lowp else torch.float32
        ldo = cout if lowp else (cout + 3) // 4 * 4
        d = _desc(nb, h, w, cin, cout, kh, kw, (kh - 1) // 2 * dil, (kw - 1) // 2 * dil, dil, cin, ldo)
        if x.dtype == torch.bfloat16 and not lowp:
            raise ValueError(f"a bf16 x is the lowp operand itself: it needs lowp=True and cin = {cin}, cout = {cout} multiples of 8")
        if lowp:
            d.dtype = L.DIN_BF16
            x = x.to(torch.bfloat16)             # (no pass over a tensor that is bf16 already, e.g. rows of the bf16 feature cache)
        elif split:
            d.dtype = L.DIN_F32_BF16X3
        st = _stream()
        y = (torch.zeros if ldo != cout else torch.empty)((nb, h, w, ldo), dtype=tdt, device=x.device)
        wpk = torch.empty(lib.din_conv_packed_elems(C.byref(d), 0), dtype=tdt, device=x.device)
        L.check(lib.din_conv_pack_weights(C.byref(d), _ptr(weight), None, _ptr(wpk), 0, st), "conv_pack")
        ws, wsb = workspace(lib.din_conv_workspace_bytes(C.byref(d), 0), x.device)
        L.check(lib.din_conv_fwd(C.byref(d), _ptr(x), _ptr(wpk), _ptr(bias), _ptr(y), L.CONV_BIAS if bias is not None else 0,
                                 _ptr(ws), wsb, st), "grid_conv_fwd")
        ctx.save_for_backward(x, weight)
        ctx.d, ctx.has_bias, ctx.lowp = d, bias is not None, lowp
        return y.float() if lowp else y

    @staticmethod
    def backward(ctx, gy):
        lib = L.load()
        x, weight = ctx.saved_tensors
        d = ctx.d
        tdt = torch.bfloat16 if ctx.lowp else torch.float32
        gy = gy.contiguous().to(tdt)
        st = _stream()
        dx = dw = db = None
        dw_installed = False
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            # data parallelism: the weight gradient goes straight into the parameter's slot of its all-reduce bucket (parallel.GradBuckets through
            # nhwc.GRAD_BUFFER, as for the backbone's conv weights) -- the embedding layer's 108 MB gradient is 93 % of the model's bytes, copying it
            # into the bucket cost a 108 MB device copy per step, and reporting it (GRAD_HOOK) starts its all-reduce under the whole backbone backward
            from . import nhwc as _nhwc
            buf = _nhwc.GRAD_BUFFER(weight) if _nhwc.GRAD_BUFFER is not None else None
            dw = buf if buf is not None else torch.empty_like(weight)
            db = torch.empty(weight.shape[0], dtype=torch.float32, device=x.device) if ctx.has_bias else None
            ws, wsb = workspace(lib.din_conv_workspace_bytes(C.byref(d), 2), x.device, "wgrad")   # not shared with split-K launches
            L.check(lib.din_conv_wgrad(C.byref(d), _ptr(x), _ptr(gy), _ptr(dw), _ptr(db), None, None, None, 0, _ptr(ws), wsb, st),
                    "grid_conv_wgrad")
            if _nhwc.GRAD_HOOK is not None:
                _nhwc.GRAD_HOOK(weight, dw)
            if buf is not None and _nhwc.GRAD_ASSIGN is not None and _nhwc.GRAD_ASSIGN(weight, dw):
                dw_installed = True                              # .grad IS the bucket slot now: autograd gets None (it would clone a shared tensor)
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            wpt = torch.empty(lib.din_conv_packed_elems(C.byref(d), 1), dtype=tdt, device=x.device)
            L.check(lib.din_conv_pack_weights(C.byref(d), _ptr(weight), None, _ptr(wpt), 1, st), "conv_pack_t")
            ws, wsb = workspace(lib.din_conv_workspace_bytes(C.byref(d), 1), x.device)
            L.check(lib.din_conv_dgrad(C.byref(d), _ptr(gy), _ptr(wpt), _ptr(dx), None, 0, 0, 0, _ptr(ws), wsb, st), "grid_conv_dgrad")
            if ctx.lowp:
                dx = dx.float()
        return dx, (None if dw_installed else dw), db, None, None, None


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], lowp: bool = False, split: bool = False) -> torch.Tensor:
    """y = x @ weight.T + bias over the last dim, on the MFMA contraction kernel (cout must be a multiple of 4).
    lowp / split: GridConvFunction's two other numeric modes (mutually exclusive).  A bf16 x is taken as lowp's operand without a cast
    pass (ValueError unless lowp is in effect); y is fp32 either way."""
    if lowp and split:
        raise ValueError("lowp and split are mutually exclusive: bf16 storage or fp32 storage with three-part bf16 compute")
    shp = x.shape
    rows = x.numel() // shp[-1]
    y = GridConvFunction.apply(x.reshape(1, 1, rows, shp[-1]), weight.reshape(weight.shape[0], weight.shape[1], 1, 1), bias, 1, lowp, split)
    cout = weight.shape[0]
    if y.shape[-1] != cout:
        y = y[..., :cout]
    return y.reshape(*shp[:-1], cout)


# ------------------------------------------------------------------------------------------------
# LayerNorm (+residual, +ReLU, +dropout)
# ------------------------------------------------------------------------------------------------
class LayerNormFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, res, gamma, beta, n_norm_dims: int, relu: bool, drop_p: float, seed: int):
        lib = L.load()
        x = x.contiguous()
        res = res.contiguous() if res is not None else None
        gamma, beta = gamma.contiguous(), beta.contiguous()
        require_gpu(x, res, gamma, beta)
        length = gamma.numel()
        assert tuple(x.shape[x.dim() - n_norm_dims:]) == tuple(gamma.shape), (x.shape, gamma.shape)
        rows = x.numel() // length
        y = torch.empty_like(x)
        stats = torch.empty((rows, 2), dtype=torch.float32, device=x.device)
        L.check(lib.din_layernorm_fwd(_ptr(x), _ptr(res), _ptr(gamma), _ptr(beta), 1e-5, _ptr(y), _ptr(stats), rows, length,
                                      int(relu), float(drop_p), int(seed), _ptr(SEED_OFFSET), _stream()), "layernorm_fwd")
        ctx.seed_offset = SEED_OFFSET
        ctx.save_for_backward(x, res if res is not None else x.new_empty(0), gamma, y, stats)
        ctx.has_res, ctx.relu, ctx.drop_p, ctx.seed, ctx.rows, ctx.length = res is not None, relu, drop_p, seed, rows, length
        return y

    @staticmethod
    def backward(ctx, gy):
        lib = L.load()
        x, res, gamma, y, stats = ctx.saved_tensors
        gy = gy.contiguous()
        dx = torch.empty_like(x)
        dgamma = torch.zeros_like(gamma)
        dbeta = torch.zeros_like(gamma)
        L.check(lib.din_layernorm_bwd(_ptr(gy), _ptr(x), _ptr(res) if ctx.has_res else None, _ptr(gamma), _ptr(y), _ptr(stats),
                                      _ptr(dx), _ptr(dgamma), _ptr(dbeta), ctx.rows, ctx.length, int(ctx.relu), float(ctx.drop_p),
                                      int(ctx.seed), _ptr(ctx.seed_offset), _stream()), "layernorm_bwd")
        return dx, (dx if ctx.has_res else None), dgamma, dbeta, None, None, None, None


def mask_seed(base: int, step: int) -> int:
    """Seed of one dropout mask: (stream id `base`, this process' rank, call counter).  Every rank draws different masks (the reference's
    DataParallel replicas share one host RNG stream, so their masks differ too), and a resumed run continues the sequence when the
    caller restores its counter."""
    rank = 0
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        rank = torch.distributed.get_rank()
    return mask_seed_of(base, rank, step)


RANK_SEED_STRIDE = 0x9E3779B97F4A7C15


def mask_seed_of(base: int, rank: int, step: int) -> int:
    return (int(base) * 1000003 + int(rank) * RANK_SEED_STRIDE + int(step) * 7919) & 0x7FFFFFFFFFFFFFFF


def layer_norm(x, gamma, beta, res=None, relu=False, drop_p=0.0, seed=0):
    return LayerNormFunction.apply(x, res, gamma, beta, gamma.dim(), relu, drop_p, seed)


# ------------------------------------------------------------------------------------------------
# Rows D2-D4: Dynamic Relation + Dynamic Walk
# ------------------------------------------------------------------------------------------------
class DynamicWalkFunction(torch.autograd.Function):
    """(x [b,t,n,c], pred [b,t,n,cp]) -> z [b,t,n,c]   (+ non-differentiable a, idx, optional mad)."""

    @staticmethod
    def forward(ctx, x, pred, kh: int, kw: int, ratio: int, scale_factor: bool, want_mad: bool, n_per_clip=None, plain: bool = False,
                clamp=None):
        """plain: lattice gather without walk (plain_infer_ratio / relation half of parallel_infer).  clamp: (iy_max, ix_max, py_max,
        px_max) clamp maxima of parallel_infer's walk half (person_mat_shape based, dynamic_infer_module.py:307-317)."""
        lib = L.load()
        x, pred = x.contiguous(), pred.contiguous()
        require_gpu(x, pred, n_per_clip)
        b, t, n, c = x.shape
        cp = pred.shape[-1]
        k2 = kh * kw
        z = torch.empty_like(x)
        a = torch.empty((b, t, n, k2), dtype=torch.float32, device=x.device)
        idx = torch.empty((b, t, n, k2, 4), dtype=torch.int32, device=x.device)
        mad = torch.empty((b, t, n, k2, c), dtype=torch.float32, device=x.device) if want_mad else None
        cl = (C.c_int32 * 4)(*[int(v) for v in clamp]) if clamp is not None else None
        L.check(lib.din_walk_fwd(_ptr(x), _ptr(pred), cp, b, t, n, c, kh, kw, ratio, int(scale_factor), int(plain), cl, _ptr(n_per_clip),
                                 _ptr(z), _ptr(a), _ptr(idx), _ptr(mad), _stream()), "din_walk_fwd")
        ctx.save_for_backward(x, pred, a)
        ctx.n_per_clip, ctx.plain, ctx.clamp = n_per_clip, bool(plain), clamp
        ctx.geom = (kh, kw, ratio, scale_factor)
        if mad is None:
            mad = x.new_empty(0)
        ctx.mark_non_differentiable(a, idx, mad)
        return z, a, idx, mad

    @staticmethod
    def backward(ctx, gz, *_):
        lib = L.load()
        x, pred, a = ctx.saved_tensors
        kh, kw, ratio, scale_factor = ctx.geom
        b, t, n, c = x.shape
        cp = pred.shape[-1]
        gz = gz.contiguous()
        dx = torch.empty_like(x)
        dpred = torch.zeros_like(pred)
        scratch = torch.empty(((c + 63) // 64) * b * t * n * 3 * kh * kw, dtype=torch.float32, device=x.device)
        cl = (C.c_int32 * 4)(*[int(v) for v in ctx.clamp]) if ctx.clamp is not None else None
        L.check(lib.din_walk_bwd(_ptr(x), _ptr(pred), cp, _ptr(a), _ptr(gz), b, t, n, c, kh, kw, ratio, int(scale_factor), int(ctx.plain), cl,
                                 _ptr(ctx.n_per_clip), _ptr(dx), _ptr(dpred), _ptr(scratch), _stream()), "din_walk_bwd")
        return dx, dpred, None, None, None, None, None, None, None, None


class MaskActorsFunction(torch.autograd.Function):
    """x [b,t,n,c] with actors >= n_per_clip[b] zeroed (Dynamic_collective: the reference slices boxes_features_all[b, :, :N])."""

    @staticmethod
    def forward(ctx, x, n_per_clip):
        lib = L.load()
        x = x.contiguous()
        require_gpu(x, n_per_clip)
        b, t, n, c = x.shape
        out = torch.empty_like(x)
        L.check(lib.din_mask_actors(_ptr(x), _ptr(n_per_clip), b, t, n, c, _ptr(out), _stream()), "mask_actors")
        ctx.n_per_clip = n_per_clip
        return out

    @staticmethod
    def backward(ctx, g):
        lib = L.load()
        g = g.contiguous()
        b, t, n, c = g.shape
        out = torch.empty_like(g)
        L.check(lib.din_mask_actors(_ptr(g), _ptr(ctx.n_per_clip), b, t, n, c, _ptr(out), _stream()), "mask_actors")
        return out, None


class AxpbyFunction(torch.autograd.Function):
    """out = alpha*x + beta*y with scalar python floats (ratio mean, module sum)."""

    @staticmethod
    def forward(ctx, x, y, alpha: float, beta: float):
        lib = L.load()
        x, y = x.contiguous(), y.contiguous()
        require_gpu(x, y)
        out = torch.empty_like(x)
        L.check(lib.din_axpby(_ptr(x), _ptr(y), _ptr(out), alpha, beta, x.numel(), _stream()), "axpby")
        ctx.ab = (alpha, beta)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = L.load()
        g = g.contiguous()
        a, b = ctx.ab
        ga, gb = torch.empty_like(g), torch.empty_like(g)
        st = _stream()
        L.check(lib.din_axpby(_ptr(g), None, _ptr(ga), a, 0.0, g.numel(), st), "axpby")
        L.check(lib.din_axpby(_ptr(g), None, _ptr(gb), b, 0.0, g.numel(), st), "axpby")
        return ga, gb, None, None


# ------------------------------------------------------------------------------------------------
# context-encoding transformer of Dynamic_TCE_volleyball
# ------------------------------------------------------------------------------------------------
class ContextAttentionFunction(torch.autograd.Function):
    """q [BT,N,H*C] (box queries), kf [BT,P,H*C] (per-pixel keys = values) -> (ctx [BT,N,H*C], att [BT,H,N,P]).
    att = softmax_P(<q, kf>) per head; ctx = att @ kf (TCE_STBiP_module.py:271-277).  att is returned for inspection (att_map)."""

    @staticmethod
    def forward(ctx, q: torch.Tensor, kf: torch.Tensor, heads: int):
        lib = L.load()
        q, kf = q.contiguous(), kf.contiguous()
        require_gpu(q, kf)
        bt, n, hc = q.shape
        p = kf.shape[1]
        assert kf.shape[0] == bt and kf.shape[2] == hc and hc % heads == 0, (q.shape, kf.shape, heads)
        c = hc // heads
        st = _stream()
        att = torch.empty((bt, heads, n, p), dtype=torch.float32, device=q.device)
        out = torch.empty_like(q)
        L.check(lib.din_ctx_scores(_ptr(q), _ptr(kf), _ptr(att), bt, n, p, heads, c, st), "ctx_scores")
        L.check(lib.din_softmax_rows(_ptr(att), bt * heads * n, p, st), "softmax_rows")
        L.check(lib.din_ctx_apply(_ptr(att), _ptr(kf), _ptr(out), bt, n, p, heads, c, st), "ctx_apply")
        ctx.save_for_backward(q, kf, att)
        ctx.dims = (bt, n, p, heads, c)
        ctx.mark_non_differentiable(att)
        return out, att

    @staticmethod
    def backward(ctx, gout, _gatt):
        lib = L.load()
        q, kf, att = ctx.saved_tensors
        bt, n, p, heads, c = ctx.dims
        gout = gout.contiguous()
        st = _stream()
        ds = torch.empty_like(att)
        L.check(lib.din_ctx_scores(_ptr(gout), _ptr(kf), _ptr(ds), bt, n, p, heads, c, st), "ctx_scores(dA)")
        L.check(lib.din_softmax_rows_bwd(_ptr(att), _ptr(ds), bt * heads * n, p, st), "softmax_rows_bwd")
        dq, dkf = torch.empty_like(q), torch.empty_like(kf)
        L.check(lib.din_ctx_apply(_ptr(ds), _ptr(kf), _ptr(dq), bt, n, p, heads, c, st), "ctx_apply(dq)")
        L.check(lib.din_ctx_keys_grad(_ptr(att), _ptr(ds), _ptr(gout), _ptr(q), _ptr(dkf), bt, n, p, heads, c, st), "ctx_keys_grad")
        return dq, dkf, None


class AddPositionFunction(torch.autograd.Function):
    """x: backbone output NHWC [BT,OH,OW,C] (fp32 | bf16), pos fp32 [OH,OW,C] -> fp32 x + pos (positional_encoding.py:91).
    relu_masked: the gradient handed back to the backbone graph is multiplied by (x > 0), as the graph expects for ReLU outputs."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, pos: torch.Tensor, relu_masked: bool):
        lib = L.load()
        require_gpu(x, pos)
        assert x.is_contiguous() and tuple(x.shape[1:]) == tuple(pos.shape), (x.shape, pos.shape)
        pos = pos.contiguous().float()
        y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        L.check(lib.din_add_position(_ptr(x), din_dtype(x), _ptr(pos), _ptr(y), x.shape[0], pos.numel(), _stream()), "add_position")
        ctx.save_for_backward(x)
        ctx.relu_masked = relu_masked
        return y

    @staticmethod
    def backward(ctx, gy):
        lib = L.load()
        (x,) = ctx.saved_tensors
        gy = gy.contiguous().float()
        gx = torch.empty_like(x)
        L.check(lib.din_add_position_bwd(_ptr(gy), _ptr(x), din_dtype(x), _ptr(gx), x.numel(), int(ctx.relu_masked), _stream()),
                "add_position_bwd")
        return gx, None, None


class ActDropoutFunction(torch.autograd.Function):
    """y = dropout(relu(x)) / dropout(x): the mask is a counter-based hash of (seed, element index), regenerated in the backward"""

    @staticmethod
    def forward(ctx, x: torch.Tensor, relu: bool, drop_p: float, seed: int):
        lib = L.load()
        x = x.contiguous()
        require_gpu(x)
        y = torch.empty_like(x)
        L.check(lib.din_act_dropout_fwd(_ptr(x), _ptr(y), x.numel(), int(relu), float(drop_p), int(seed), _ptr(SEED_OFFSET), _stream()),
                "act_dropout_fwd")
        ctx.save_for_backward(x)
        ctx.args = (relu, drop_p, seed)
        ctx.seed_offset = SEED_OFFSET
        return y

    @staticmethod
    def backward(ctx, gy):
        lib = L.load()
        (x,) = ctx.saved_tensors
        relu, drop_p, seed = ctx.args
        gy = gy.contiguous()
        gx = torch.empty_like(x)
        L.check(lib.din_act_dropout_bwd(_ptr(gy), _ptr(x), _ptr(gx), x.numel(), int(relu), float(drop_p), int(seed), _ptr(ctx.seed_offset),
                                        _stream()), "act_dropout_bwd")
        return gx, None, None, None


class ScaleByParamFunction(torch.autograd.Function):
    """out = x * scalar[idx] with the scalar read on the device (no host sync): beta-weighted ratio sum (:144-145)."""

    @staticmethod
    def forward(ctx, x, scalar, idx: int):
        lib = L.load()
        x, scalar = x.contiguous(), scalar.contiguous()
        require_gpu(x, scalar)
        out = torch.empty_like(x)
        L.check(lib.din_scale_by_param(_ptr(x), _ptr(scalar), idx, _ptr(out), 0, x.numel(), _stream()), "scale_by_param")
        ctx.save_for_backward(x, scalar)
        ctx.idx = idx
        return out

    @staticmethod
    def backward(ctx, g):
        lib = L.load()
        x, scalar = ctx.saved_tensors
        g = g.contiguous()
        st = _stream()
        dx = torch.empty_like(x)
        L.check(lib.din_scale_by_param(_ptr(g), _ptr(scalar), ctx.idx, _ptr(dx), 0, g.numel(), st), "scale_by_param")
        ds = torch.zeros_like(scalar)
        L.check(lib.din_dot_accum(_ptr(g), _ptr(x), _ptr(ds), ctx.idx, g.numel(), st), "dot_accum")
        return dx, ds, None


# ------------------------------------------------------------------------------------------------
# Row H: head
# ------------------------------------------------------------------------------------------------
class HeadFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s, weight, bias, n_per_clip):
        lib = L.load()
        s, weight, bias = s.contiguous(), weight.contiguous(), bias.contiguous()
        require_gpu(s, weight, bias, n_per_clip)
        b, t, n, c = s.shape
        a = weight.shape[0]
        buf = torch.empty(b * a + b * t * a, dtype=torch.float32, device=s.device)
        argmax = torch.empty((b, t, c), dtype=torch.int32, device=s.device)
        L.check(lib.din_head_fwd(_ptr(s), _ptr(weight), _ptr(bias), _ptr(n_per_clip), b, t, n, c, a, _ptr(buf), _ptr(argmax), _stream()),
                "head_fwd")
        ctx.save_for_backward(s, weight, argmax)
        return buf[: b * a].reshape(b, a).clone()

    @staticmethod
    def backward(ctx, gscores):
        lib = L.load()
        s, weight, argmax = ctx.saved_tensors
        b, t, n, c = s.shape
        a = weight.shape[0]
        gscores = gscores.contiguous()
        ds = torch.empty_like(s)
        dw = torch.zeros_like(weight)
        db = torch.zeros(a, dtype=torch.float32, device=s.device)
        L.check(lib.din_head_bwd(_ptr(gscores), _ptr(s), _ptr(weight), _ptr(argmax), b, t, n, c, a, _ptr(ds), _ptr(dw), _ptr(db), _stream()),
                "head_bwd")
        return ds, dw, db, None


class BasenetHeadFunction(torch.autograd.Function):
    """Stage-1 head (reference base_model.py:117-139 / :243-268): y [BT, N, C] (the fc_emb output) -> (actions, activities) with
    s = dropout(relu(y)) formed on the fly (bitwise ActDropoutFunction.apply(y, True, drop_p, seed)).

    n_per_frame None: actions [BT/T*N, A_act], activities [BT/T, A_grp] when mean_over_t (volleyball, T != 1), else [BT*N] / [BT].
    n_per_frame int32 [BT] (collective): actions compacted to [ALL_N, A_act] in (frame, box) order, activities [BT, A_grp].  ALL_N sizes the
    output, so this path does exactly ONE 4-byte device-to-host read per forward (the sum of the counts, or -1 when a count is outside
    1..N, which the library refuses); the reference does B*T such reads.  Forward one launch, backward one launch, deterministic."""

    @staticmethod
    def forward(ctx, y, w_act, b_act, w_grp, b_grp, n_per_frame, T: int, mean_over_t: bool, drop_p: float, seed: int):
        lib = L.load()
        y = y.contiguous()
        w_act, b_act, w_grp, b_grp = w_act.contiguous(), b_act.contiguous(), w_grp.contiguous(), b_grp.contiguous()
        if n_per_frame is not None:
            n_per_frame = n_per_frame.reshape(-1).to(torch.int32).contiguous()
        require_gpu(y, w_act, b_act, w_grp, b_grp, n_per_frame)
        n, c = y.shape[-2], y.shape[-1]
        bt = y.numel() // (n * c)
        aa, ag = w_act.shape[0], w_grp.shape[0]
        mean = bool(mean_over_t)
        if n_per_frame is not None:
            ok = ((n_per_frame >= 1) & (n_per_frame <= n)).all()
            all_n = int(torch.where(ok, n_per_frame.sum(), -1).to(torch.int32).item())     # the one 4-byte read
        else:
            all_n = (bt // T if mean else bt) * n
        groups = bt // T if mean else bt
        actions = torch.empty((max(all_n, 1), aa), dtype=torch.float32, device=y.device)     # (all_n < 1: refused by the library)
        activities = torch.empty((groups, ag), dtype=torch.float32, device=y.device)
        argmax = torch.empty((bt, c), dtype=torch.int32, device=y.device)
        L.check(lib.din_basenet_head_fwd(_ptr(y), _ptr(w_act), _ptr(b_act), _ptr(w_grp), _ptr(b_grp), _ptr(n_per_frame), all_n, bt, int(T),
                                         int(mean), n, c, aa, ag, float(drop_p), int(seed), _ptr(SEED_OFFSET), _ptr(actions),
                                         _ptr(activities), _ptr(argmax), _stream()), "basenet_head_fwd")
        ctx.save_for_backward(y, w_act, w_grp, argmax)
        ctx.n_per_frame, ctx.seed_offset = n_per_frame, SEED_OFFSET
        ctx.args = (all_n, bt, int(T), int(mean), n, c, aa, ag, float(drop_p), int(seed))
        return actions, activities

    @staticmethod
    def backward(ctx, g_actions, g_activities):
        lib = L.load()
        y, w_act, w_grp, argmax = ctx.saved_tensors
        all_n, bt, T, mean, n, c, aa, ag, drop_p, seed = ctx.args
        g_actions = (g_actions if g_actions is not None else torch.zeros((all_n, aa), device=y.device)).contiguous().float()
        g_activities = (g_activities if g_activities is not None else
                        torch.zeros((bt // T if mean else bt, ag), device=y.device)).contiguous().float()
        g_y = torch.empty_like(y)
        dw_act, dw_grp = torch.empty_like(w_act), torch.empty_like(w_grp)
        db_act = torch.empty(aa, dtype=torch.float32, device=y.device)
        db_grp = torch.empty(ag, dtype=torch.float32, device=y.device)
        L.check(lib.din_basenet_head_bwd(_ptr(g_actions), _ptr(g_activities), _ptr(y), _ptr(w_act), _ptr(w_grp), _ptr(argmax),
                                         _ptr(ctx.n_per_frame), all_n, bt, T, mean, n, c, aa, ag, drop_p, seed, _ptr(ctx.seed_offset),
                                         _ptr(g_y), _ptr(dw_act), _ptr(db_act), _ptr(dw_grp), _ptr(db_grp), _stream()), "basenet_head_bwd")
        return g_y, dw_act, db_act, dw_grp, db_grp, None, None, None, None, None


# ------------------------------------------------------------------------------------------------
# Actor Relation Graph block (ARG baseline)
# ------------------------------------------------------------------------------------------------
def arg_graph_workspace_floats(b: int, tn: int, ng: int, nfg: int, backward: bool) -> int:
    """scratch the two entry points ask for (include/din_hip.h)"""
    nchunk = (nfg + 63) // 64
    if not backward:
        return b * ng * nchunk * 3
    return b * ng * tn * nfg + (b * ng * nchunk * 2 + 3) // 4 * 4 + b * ng * tn * tn


class ArgGraphFunction(torch.autograd.Function):
    """proj [B, TN, NG*(2*NFR+NFG)] = X [W_theta,0.. | W_phi,0.. | W_gcn,0..]^T (+ biases), boxes [B, TN, 4], gamma / beta [NG, TN, NFG]
    -> (out [B, TN, NFG], rel [B, NG, TN, TN], mask bool [B, TN, TN]) -- reference ARG_infer_module.py:46-89 after its Linear layers.
    centre_rounds: the GCN layer's index + 1 (how often the reference has averaged the box corners in place by then)."""

    @staticmethod
    def forward(ctx, proj, boxes, gamma, beta, ng: int, nfr: int, nfg: int, thr: float, centre_rounds: int):
        lib = L.load()
        proj, gamma, beta = proj.contiguous(), gamma.contiguous(), beta.contiguous()
        boxes = boxes.detach().float().contiguous()
        require_gpu(proj, boxes, gamma, beta)
        b, tn, ld = proj.shape
        assert ld == ng * (2 * nfr + nfg), (proj.shape, ng, nfr, nfg)
        assert tuple(boxes.shape) == (b, tn, 4) and tuple(gamma.shape) == (ng, tn, nfg) == tuple(beta.shape), (boxes.shape, gamma.shape)
        dev = proj.device
        out = torch.empty((b, tn, nfg), dtype=torch.float32, device=dev)
        rel = torch.empty((b, ng, tn, tn), dtype=torch.float32, device=dev)
        mask = torch.empty((b, tn, tn), dtype=torch.uint8, device=dev)
        z = torch.empty((b, ng, tn, nfg), dtype=torch.float32, device=dev)
        stats = torch.empty((b, ng, 2), dtype=torch.float32, device=dev)
        nws = arg_graph_workspace_floats(b, tn, ng, nfg, False)
        ws = torch.empty(nws, dtype=torch.float32, device=dev)
        base, esz = proj.data_ptr(), 4
        L.check(lib.din_arg_graph_fwd(base, base + ng * nfr * esz, base + 2 * ng * nfr * esz, ld, _ptr(boxes), int(centre_rounds), float(thr),
                                      _ptr(gamma), _ptr(beta), 1e-5, b, tn, ng, nfr, nfg, _ptr(out), _ptr(rel), _ptr(mask), _ptr(z),
                                      _ptr(stats), _ptr(ws), nws, _stream()), "arg_graph_fwd")
        ctx.save_for_backward(proj, gamma, beta, rel, z, stats)
        ctx.dims = (b, tn, ng, nfr, nfg)
        mask = mask.view(torch.bool)
        ctx.mark_non_differentiable(rel, mask)
        return out, rel, mask

    @staticmethod
    def backward(ctx, gout, _grel, _gmask):
        lib = L.load()
        proj, gamma, beta, rel, z, stats = ctx.saved_tensors
        b, tn, ng, nfr, nfg = ctx.dims
        ld = proj.shape[2]
        gout = gout.contiguous()
        dproj = torch.empty_like(proj)
        dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(beta)
        nws = arg_graph_workspace_floats(b, tn, ng, nfg, True)
        ws = torch.empty(nws, dtype=torch.float32, device=proj.device)
        base, gbase, esz = proj.data_ptr(), dproj.data_ptr(), 4
        L.check(lib.din_arg_graph_bwd(_ptr(gout), base, base + ng * nfr * esz, base + 2 * ng * nfr * esz, ld, _ptr(gamma), _ptr(beta),
                                      _ptr(rel), _ptr(z), _ptr(stats), b, tn, ng, nfr, nfg, gbase, gbase + ng * nfr * esz,
                                      gbase + 2 * ng * nfr * esz, ld, _ptr(dgamma), _ptr(dbeta), _ptr(ws), nws, _stream()), "arg_graph_bwd")
        return dproj, None, dgamma, dbeta, None, None, None, None, None


# ------------------------------------------------------------------------------------------------
# Actor-Transformer block (AT baseline)
# ------------------------------------------------------------------------------------------------
def actor_attn_workspace_floats(g: int, c: int) -> int:
    """scratch din_actor_attn_bwd asks for (include/din_hip.h): the per-group partials of d gamma / d beta"""
    return g * 2 * c


class ActorPositionFunction(torch.autograd.Function):
    """x [B, T, N, C], boxes [B, T, N, 4] (feature px), dim_t fp32 [C/2] -> x + PE(box centre) [B, T, N, C], or its mean over T [B, N, C]
    when pool_t -- reference AT_infer_module.py:66-96 (+ torch.mean(x, dim=1) of :125-126).  The backward is the identity on x (g / T
    broadcast over the frames when pooled); the boxes get no gradient."""

    @staticmethod
    def forward(ctx, x, boxes, dim_t, image_size, out_size, pool_t: bool):
        lib = L.load()
        x, dim_t = x.contiguous(), dim_t.contiguous()
        boxes = boxes.detach().float().contiguous()
        require_gpu(x, boxes, dim_t)
        b, t, n, c = x.shape
        assert boxes.numel() == b * t * n * 4 and dim_t.numel() * 2 == c, (x.shape, boxes.shape, dim_t.shape)
        y = torch.empty((b, n, c) if pool_t else (b, t, n, c), dtype=torch.float32, device=x.device)
        L.check(lib.din_actor_position_fwd(_ptr(x), _ptr(boxes), _ptr(dim_t), float(image_size[1]), float(image_size[0]), float(out_size[1]),
                                           float(out_size[0]), b, t, n, c, int(bool(pool_t)), _ptr(y), _stream()), "actor_position_fwd")
        ctx.dims = (b, t, n, c, bool(pool_t))
        return y

    @staticmethod
    def backward(ctx, gy):
        b, t, n, c, pool_t = ctx.dims
        if not pool_t:
            return gy, None, None, None, None, None                    # (pass-through: no launch)
        lib = L.load()
        gy = gy.contiguous()
        gx = torch.empty((b, t, n, c), dtype=torch.float32, device=gy.device)
        L.check(lib.din_actor_position_bwd(_ptr(gy), b, t, n, c, 1, _ptr(gx), _stream()), "actor_position_bwd")
        return gx, None, None, None, None, None


class ActorAttentionFunction(torch.autograd.Function):
    """proj [G, N, 3*C] = X [Q_W | K_W | V_W]^T, x [G, N, C], gamma / beta [C] -> (LayerNorm(x + dropout(softmax(Q K^T / sqrt(C)) V)) [G, N, C],
    att [G, N, N]) -- reference AT_infer_module.py:130-138 after its three Linear layers.  The mask is the counter hash of (seed, element
    index), regenerated in the backward.  want_keep: also return the keep mask (bool [G, N, C]), for inspection.
    proj may be a view of rows padded to a multiple of 4 floats (the first 3*C columns of a wider buffer): it is read in place through its
    row stride, and its gradient comes back with the same row stride."""

    @staticmethod
    def _rows_in_place(proj, n):
        """True if proj [G, N, 3*C] can be handed to the kernels as it is: unit column stride, one row stride ld (a multiple of 4) for all rows"""
        return proj.stride(2) == 1 and proj.stride(1) % 4 == 0 and proj.stride(1) >= proj.shape[2] and proj.stride(0) == n * proj.stride(1) \
            and proj.data_ptr() % 16 == 0

    @staticmethod
    def forward(ctx, proj, x, gamma, beta, drop_p: float, seed: int, want_keep: bool = False):
        lib = L.load()
        x, gamma, beta = x.contiguous(), gamma.contiguous(), beta.contiguous()
        g, n, c = x.shape
        require_gpu(x, gamma, beta)
        if not ActorAttentionFunction._rows_in_place(proj, n):
            proj = proj.contiguous()
            require_gpu(proj)
        elif not proj.is_cuda:
            require_gpu(proj.contiguous())                              # (raises: no CPU fallback)
        assert tuple(proj.shape) == (g, n, 3 * c) and gamma.numel() == c == beta.numel(), (proj.shape, x.shape, gamma.shape)
        dev = x.device
        out = torch.empty((g, n, c), dtype=torch.float32, device=dev)
        att = torch.empty((g, n, n), dtype=torch.float32, device=dev)
        stats = torch.empty((g * n, 2), dtype=torch.float32, device=dev)
        keep = torch.empty((g, n, c), dtype=torch.uint8, device=dev) if want_keep else None
        base, ld = proj.data_ptr(), proj.stride(1)
        L.check(lib.din_actor_attn_fwd(base, base + 4 * c, base + 8 * c, ld, _ptr(x), _ptr(gamma), _ptr(beta), 1e-5, float(drop_p), int(seed),
                                       _ptr(SEED_OFFSET), g, n, c, _ptr(out), _ptr(att), _ptr(stats), _ptr(keep), _stream()), "actor_attn_fwd")
        ctx.save_for_backward(proj, x, gamma, att, stats)
        ctx.args = (float(drop_p), int(seed))
        ctx.seed_offset = SEED_OFFSET
        ctx.mark_non_differentiable(att)
        if want_keep:
            keep = keep.view(torch.bool)
            ctx.mark_non_differentiable(keep)
            return out, att, keep
        return out, att

    @staticmethod
    def backward(ctx, gout, *_):
        lib = L.load()
        proj, x, gamma, att, stats = ctx.saved_tensors
        drop_p, seed = ctx.args
        g, n, c = x.shape
        gout = gout.contiguous()
        ld = proj.stride(1)
        # same row stride as proj; with padded rows (ld > 3*c) the padding columns stay uninitialised: they are outside the returned view, so no
        # consumer of the gradient can read them (on the model path ld == 3*c and the view is the whole buffer)
        dproj = torch.empty((g, n, ld), dtype=torch.float32, device=x.device)[..., :3 * c]
        dx = torch.empty_like(x)
        dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(gamma)
        nws = actor_attn_workspace_floats(g, c)
        ws = torch.empty(nws, dtype=torch.float32, device=x.device)
        base, gbase = proj.data_ptr(), dproj.data_ptr()
        L.check(lib.din_actor_attn_bwd(_ptr(gout), base, base + 4 * c, base + 8 * c, ld, _ptr(x), _ptr(gamma), _ptr(att), _ptr(stats), drop_p,
                                       seed, _ptr(ctx.seed_offset), g, n, c, gbase, gbase + 4 * c, gbase + 8 * c, ld, _ptr(dx), _ptr(dgamma),
                                       _ptr(dbeta), _ptr(ws), nws, _stream()), "actor_attn_bwd")
        return dproj, dx, dgamma, dbeta, None, None, None


# ------------------------------------------------------------------------------------------------
# PCTDM baseline: LSTM recurrence, direction pooling, intra-team attention
# ------------------------------------------------------------------------------------------------
def lstm_workspace_floats(rows: int, dirs: int, hidden: int) -> int:
    """scratch din_lstm_bwd asks for (include/din_hip.h): W_hh^T of every direction and the carried cell-state gradient"""
    return int(L.load().din_lstm_bwd_workspace(rows, dirs, hidden))


def pctdm_att_workspace_floats(g: int, h: int) -> int:
    """scratch din_pctdm_att_bwd asks for (include/din_hip.h): the per-frame partials of d w_e and d b_e"""
    return int(L.load().din_pctdm_att_bwd_workspace(g, h))


def _lstm_dw_hh(lib, h_prev, d_pre, w_hh):
    """dW_hh [D, 4H, H] = d_pre^T h_prev per direction over the R*S rows: one call of the weight-gradient contraction each, reading the two
    direction slices in place through their row stride (copies padded to a multiple of 4 columns when H is not one)"""
    r, s, dirs, h = h_prev.shape
    rows, st = r * s, _stream()
    dw = torch.empty_like(w_hh)
    for d in range(dirs):
        if h % 4 == 0:
            x, ldi, cioff = h_prev, dirs * h, d * h
        else:
            hp = (h + 3) // 4 * 4
            x = torch.zeros((rows, hp), dtype=torch.float32, device=h_prev.device)
            x[:, :h] = h_prev[:, :, d].reshape(rows, h)
            ldi, cioff = hp, 0
        desc = _desc(1, 1, rows, h, 4 * h, 1, 1, 0, 0, 1, ldi, dirs * 4 * h)
        desc.cioff, desc.cooff = cioff, d * 4 * h
        ws, wsb = workspace(lib.din_conv_workspace_bytes(C.byref(desc), 2), h_prev.device, "wgrad")
        L.check(lib.din_conv_wgrad(C.byref(desc), _ptr(x), _ptr(d_pre), _ptr(dw[d]), None, None, None, None, 0, _ptr(ws), wsb, st),
                "lstm_wgrad")
    return dw


class LSTMFunction(torch.autograd.Function):
    """pre [R, S, D, 4H] = x W_ih^T + b_ih + b_hh of all steps (gate order i, f, g, o), w_hh [D, 4H, H] -> h [R, S, D*H] in torch.nn.LSTM's
    batch_first layout (forward half, then reverse half, each at its own position) -- reference pctdm_infer_module.py:83 / :114 after the
    input projection.  Zero initial state; D = 2 walks the second direction from the last position.  One launch per step.
    want_state: also return the activated gates [R, S, D, 4H] and the cell states [R, S, D, H], for inspection."""

    @staticmethod
    def forward(ctx, pre, w_hh, want_state: bool = False):
        lib = L.load()
        pre, w_hh = pre.contiguous(), w_hh.contiguous()
        require_gpu(pre, w_hh)
        r, s, dirs, h4 = pre.shape
        h = h4 // 4
        assert tuple(w_hh.shape) == (dirs, 4 * h, h) and h4 == 4 * h, (pre.shape, w_hh.shape)
        dev = pre.device
        out = torch.empty((r, s, dirs * h), dtype=torch.float32, device=dev)
        gates = torch.empty((r, s, dirs, 4 * h), dtype=torch.float32, device=dev)
        cells = torch.empty((r, s, dirs, h), dtype=torch.float32, device=dev)
        L.check(lib.din_lstm_fwd(_ptr(pre), _ptr(w_hh), r, s, dirs, h, _ptr(out), _ptr(gates), _ptr(cells), _stream()), "lstm_fwd")
        ctx.save_for_backward(w_hh, gates, cells)
        if want_state:
            ctx.mark_non_differentiable(gates, cells)
            return out, gates, cells
        return out

    @staticmethod
    def backward(ctx, gout, *_):
        lib = L.load()
        w_hh, gates, cells = ctx.saved_tensors
        r, s, dirs, h = cells.shape
        gout = gout.contiguous()
        d_pre = torch.empty_like(gates)
        h_prev = torch.empty_like(cells)
        nws = lstm_workspace_floats(r, dirs, h)
        ws = torch.empty(nws, dtype=torch.float32, device=gout.device)
        L.check(lib.din_lstm_bwd(_ptr(gout), _ptr(gates), _ptr(cells), _ptr(w_hh), r, s, dirs, h, _ptr(d_pre), _ptr(h_prev), _ptr(ws), nws,
                                 _stream()), "lstm_bwd")
        dw = _lstm_dw_hh(lib, h_prev, d_pre, w_hh) if ctx.needs_input_grad[1] else None
        return d_pre, dw, None


class PctdmPoolFunction(torch.autograd.Function):
    """lstm_out [G, N, 2H] -> (pooled [G, N, H] = max of the two direction halves, context [G, H] = mean of pooled over N, winner bool
    [G, N, H] = the reverse half won) -- reference pctdm_infer_module.py:94-96 and :106"""

    @staticmethod
    def forward(ctx, lstm_out):
        lib = L.load()
        lstm_out = lstm_out.contiguous()
        require_gpu(lstm_out)
        g, n, h2 = lstm_out.shape
        h = h2 // 2
        assert h2 == 2 * h, lstm_out.shape
        dev = lstm_out.device
        pooled = torch.empty((g, n, h), dtype=torch.float32, device=dev)
        winner = torch.empty((g, n, h), dtype=torch.uint8, device=dev)
        context = torch.empty((g, h), dtype=torch.float32, device=dev)
        L.check(lib.din_pctdm_pool_fwd(_ptr(lstm_out), g, n, h, _ptr(pooled), _ptr(winner), _ptr(context), _stream()), "pctdm_pool_fwd")
        ctx.save_for_backward(winner)
        wb = winner.view(torch.bool)
        ctx.mark_non_differentiable(wb)
        return pooled, context, wb

    @staticmethod
    def backward(ctx, g_pooled, g_context, _gw):
        lib = L.load()
        (winner,) = ctx.saved_tensors
        g, n, h = winner.shape
        g_pooled = (g_pooled if g_pooled is not None else torch.zeros((g, n, h), device=winner.device)).contiguous()
        g_context = (g_context if g_context is not None else torch.zeros((g, h), device=winner.device)).contiguous()
        d = torch.empty((g, n, 2 * h), dtype=torch.float32, device=winner.device)
        L.check(lib.din_pctdm_pool_bwd(_ptr(g_pooled), _ptr(g_context), _ptr(winner), g, n, h, _ptr(d), _stream()), "pctdm_pool_bwd")
        return d


class PctdmAttentionFunction(torch.autograd.Function):
    """pooled, src = att_source_weights(pooled) [G, N, H], ctx = att_context_weights(context) [G, H], w_e [1, H] | [H], b_e [1] ->
    (y = pooled + pooled * gamma [G, N, H], gamma [G, N] = softmax inside each team of N / 2 players of w_e . tanh(src + ctx) + b_e) --
    reference pctdm_infer_module.py:52-59 and :112-114 around its three Linear layers"""

    @staticmethod
    def forward(ctx, pooled, src, cx, w_e, b_e):
        lib = L.load()
        pooled, src, cx, w_e, b_e = pooled.contiguous(), src.contiguous(), cx.contiguous(), w_e.contiguous(), b_e.contiguous()
        require_gpu(pooled, src, cx, w_e, b_e)
        g, n, h = pooled.shape
        assert tuple(src.shape) == (g, n, h) and tuple(cx.shape) == (g, h) and w_e.numel() == h and b_e.numel() == 1, \
            (pooled.shape, src.shape, cx.shape, w_e.shape, b_e.shape)
        y = torch.empty_like(pooled)
        gamma = torch.empty((g, n), dtype=torch.float32, device=pooled.device)
        L.check(lib.din_pctdm_att_fwd(_ptr(pooled), _ptr(src), _ptr(cx), _ptr(w_e), _ptr(b_e), g, n, h, _ptr(y), _ptr(gamma), _stream()),
                "pctdm_att_fwd")
        ctx.save_for_backward(pooled, src, cx, w_e, gamma)
        ctx.shapes = (w_e.shape, b_e.shape)
        ctx.mark_non_differentiable(gamma)
        return y, gamma

    @staticmethod
    def backward(ctx, g_y, _gg):
        lib = L.load()
        pooled, src, cx, w_e, gamma = ctx.saved_tensors
        g, n, h = pooled.shape
        g_y = g_y.contiguous()
        d_pooled, d_src, d_ctx = torch.empty_like(pooled), torch.empty_like(src), torch.empty_like(cx)
        d_w_e = torch.empty(ctx.shapes[0], dtype=torch.float32, device=pooled.device)
        d_b_e = torch.empty(ctx.shapes[1], dtype=torch.float32, device=pooled.device)
        nws = pctdm_att_workspace_floats(g, h)
        ws = torch.empty(nws, dtype=torch.float32, device=pooled.device)
        L.check(lib.din_pctdm_att_bwd(_ptr(g_y), _ptr(pooled), _ptr(src), _ptr(cx), _ptr(w_e), _ptr(gamma), g, n, h, _ptr(d_pooled), _ptr(d_src),
                                      _ptr(d_ctx), _ptr(d_w_e), _ptr(d_b_e), _ptr(ws), nws, _stream()), "pctdm_att_bwd")
        return d_pooled, d_src, d_ctx, d_w_e, d_b_e


# ------------------------------------------------------------------------------------------------
# layout views for API parity (NOT on the training path)
# ------------------------------------------------------------------------------------------------
class NHWCToNCHWFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, buf, coff: int, c: int, relu_masked: bool = False):
        lib = L.load()
        require_gpu(buf)
        nb, h, w, ld = buf.shape
        out = torch.empty((nb, c, h, w), dtype=torch.float32, device=buf.device)
        L.check(lib.din_nhwc_to_nchw_f32(_ptr(buf), din_dtype(buf), nb, h, w, c, ld, coff, _ptr(out), _stream()), "nhwc_to_nchw")
        ctx.meta = (coff, c, relu_masked)
        ctx.save_for_backward(buf)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = L.load()
        (buf,) = ctx.saved_tensors
        coff, c, relu_masked = ctx.meta
        nb, h, w, ld = buf.shape
        g = g.float().contiguous()
        st = _stream()
        tmp = torch.empty((nb, h, w, c), dtype=torch.float32, device=g.device)
        L.check(lib.din_nchw_f32_to_nhwc(_ptr(g), nb, h, w, c, _ptr(tmp), L.DIN_F32, c, 0, st), "nchw_to_nhwc")
        gb = torch.zeros_like(buf)
        L.check(lib.din_grad_cast_mask(_ptr(tmp), _ptr(buf), _ptr(gb), din_dtype(buf), nb * h * w, c, ld, coff, ld, coff,
                                       int(relu_masked), st), "grad_cast_mask")
        return gb, None, None, None


def adam_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0):
    lib = L.load()
    require_gpu(p, g, m, v)
    L.check(lib.din_adam_step(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), lr, beta1, beta2, eps, weight_decay, step, grad_scale,
                              _stream()), "adam_step")


def copy_rows_u8(src: torch.Tensor, dst: torch.Tensor, nbytes: int, n: Optional[int] = None) -> None:
    """row i: `nbytes` bytes from device address src[i] to device address dst[i], one launch on the current stream; src[i] == 0 leaves
    row i alone.  src, dst: int64 device tables (din_copy_rows_u8: the frame cache's insert and gather)."""
    lib = L.load()
    require_gpu(src, dst)
    if src.dtype != torch.int64 or dst.dtype != torch.int64:
        raise L.DinError("copy_rows_u8: address tables are int64 device tensors")
    n = min(src.numel(), dst.numel()) if n is None else n
    if n > min(src.numel(), dst.numel()):
        raise L.DinError(f"copy_rows_u8: n = {n} rows but the tables hold {src.numel()} / {dst.numel()} addresses")
    L.check(lib.din_copy_rows_u8(_ptr(src), _ptr(dst), n, nbytes, _stream()), "copy_rows_u8")


def copy_rows_u8_flip(src: torch.Tensor, dst: torch.Tensor, flip: Optional[torch.Tensor], lines: int, width: int,
                      n: Optional[int] = None) -> None:
    """copy_rows_u8 over rows of `lines` lines of `width` bytes, with the rows whose flag is set mirrored left-right: where flip[i] != 0,
    dst[i][l * width + x] = src[i][l * width + width - 1 - x].  flip: an int64 device tensor like the tables, or None (no row is
    mirrored).  A mirrored row must not be written over its source (din_copy_rows_u8_flip: the flip augmentation's gather)."""
    lib = L.load()
    require_gpu(src, dst, *(() if flip is None else (flip,)))
    if src.dtype != torch.int64 or dst.dtype != torch.int64 or (flip is not None and flip.dtype != torch.int64):
        raise L.DinError("copy_rows_u8_flip: address tables and flags are int64 device tensors")
    held = [t.numel() for t in (src, dst, flip) if t is not None]
    n = min(held) if n is None else n
    if n > min(held):
        raise L.DinError(f"copy_rows_u8_flip: n = {n} rows but the tables and flags hold {held} entries")
    if flip is not None and not flip.is_contiguous():
        raise L.DinError("copy_rows_u8_flip: flags must be contiguous")
    L.check(lib.din_copy_rows_u8_flip(_ptr(src), _ptr(dst), _ptr(flip), n, lines, width, _stream()), "copy_rows_u8_flip")


def flip_clip_labels(boxes: Optional[torch.Tensor], activities: Optional[torch.Tensor], flip: torch.Tensor,
                     n_valid: Optional[torch.Tensor], label_map: Optional[torch.Tensor], width: float) -> None:
    """the labels of mirrored clips, in place, one launch on the current stream.  flip: int64 device flags, one per frame (row) of the
    batch.  boxes: fp32 [..., n, 4] (x1, y1, x2, y2) in feature px with `rows` frames in all: in a flagged row the first n_valid[row]
    boxes (all n without n_valid, an int32 tensor of one count per row) become (width - x2, y1, width - x1, y2).  activities: int64, one
    per row: a flagged row's label a becomes label_map[a] (an int64 device tensor) when 0 <= a < len(label_map); without a map the
    labels stay.  Either half may be None (din_flip_clip_labels)."""
    lib = L.load()
    require_gpu(*(t for t in (boxes, activities, flip, n_valid, label_map) if t is not None))
    rows = flip.numel()
    if flip.dtype != torch.int64 or not flip.is_contiguous():
        raise L.DinError("flip_clip_labels: flags are a contiguous int64 device tensor")
    n = 0
    if boxes is not None:
        if boxes.dtype != torch.float32 or not boxes.is_contiguous() or boxes.dim() < 2 or boxes.shape[-1] != 4 \
                or boxes.numel() != rows * boxes.shape[-2] * 4:
            raise L.DinError(f"flip_clip_labels: boxes must be contiguous fp32 [..., n, 4] over {rows} rows, got {tuple(boxes.shape)}")
        n = boxes.shape[-2]
    if activities is not None and (activities.dtype != torch.int64 or not activities.is_contiguous() or activities.numel() != rows):
        raise L.DinError(f"flip_clip_labels: activities must be contiguous int64 with {rows} entries")
    if n_valid is not None and (n_valid.dtype != torch.int32 or not n_valid.is_contiguous() or n_valid.numel() != rows):
        raise L.DinError(f"flip_clip_labels: n_valid must be contiguous int32 with {rows} entries")
    if label_map is not None and (label_map.dtype != torch.int64 or not label_map.is_contiguous()):
        raise L.DinError("flip_clip_labels: label_map is a contiguous int64 device tensor")
    classes = 0 if label_map is None else label_map.numel()
    L.check(lib.din_flip_clip_labels(_ptr(boxes), _ptr(activities), _ptr(flip), _ptr(n_valid), _ptr(label_map), rows, n, float(width),
                                     classes, _stream()), "flip_clip_labels")


GRAY_SEGMENT = 8192             # bytes of one plane per (row, line group) item of the colour-jitter launches (include/din_hip.h)
GRAY_MAX_PIXELS = 1 << 24       # height * width of a row stays below this: its grey sum is kept in 32 bits


def gray_partial_segments(height: int, width: int) -> int:
    """line groups per row of din_rows_gray_partials / din_copy_rows_u8_jitter: whole image lines, max(1, 8192 // width) to a group --
    the workspace of n rows is n * gray_partial_segments(height, width) uint32 (SEGS of include/din_hip.h, stated here once)"""
    height, width = int(height), int(width)
    if height <= 0 or width <= 0:
        return 0
    return -(-height // max(1, GRAY_SEGMENT // width))


def _jitter_tables(what: str, tables, n: Optional[int]) -> int:
    require_gpu(*tables)
    if any(t.dtype != torch.int64 or not t.is_contiguous() for t in tables):
        raise L.DinError(f"{what}: address tables and flags are contiguous int64 device tensors")
    held = min(t.numel() for t in tables)
    n = held if n is None else int(n)
    if n > held:
        raise L.DinError(f"{what}: n = {n} rows but the tables hold {[t.numel() for t in tables]} entries")
    return n


def _check_partials(what: str, partials: torch.Tensor, n: int, height: int, width: int) -> None:
    require_gpu(partials)
    need = n * gray_partial_segments(height, width)
    if partials.dtype != torch.int32 or not partials.is_contiguous() or partials.numel() < need:
        raise L.DinError(f"{what}: partials must be a contiguous int32 device tensor (the uint32 sums' bits) of at least {need} entries "
                         f"({n} rows x gray_partial_segments({height}, {width})), got {partials.dtype} x {partials.numel()}")


def rows_gray_partials(src: torch.Tensor, partials: torch.Tensor, height: int, width: int, n: Optional[int] = None) -> None:
    """partials[i * segs + g] = the sum of L = (19595 r + 38470 g + 7471 b + 32768) >> 16 over line group g of the uint8 [3, height,
    width] row at device address src[i], segs = gray_partial_segments(height, width); src[i] == 0 leaves row i's partials alone.  One
    launch on the current stream, no atomics (din_rows_gray_partials: the mean of PIL.ImageEnhance.Contrast)."""
    lib = L.load()
    n = _jitter_tables("rows_gray_partials", (src,), n)
    _check_partials("rows_gray_partials", partials, n, height, width)
    L.check(lib.din_rows_gray_partials(_ptr(src), _ptr(partials), n, height, width, _stream()), "rows_gray_partials")


def copy_rows_u8_jitter(src: torch.Tensor, dst: torch.Tensor, flip: Optional[torch.Tensor], factors: Optional[torch.Tensor],
                        partials: Optional[torch.Tensor], height: int, width: int, n: Optional[int] = None) -> None:
    """copy_rows_u8_flip over uint8 [3, height, width] rows with row i put through PIL.ImageEnhance.Contrast, .Brightness and .Color
    with factors[i] = (contrast, brightness, saturation) on its way (fp32 device tensor [n, 3]); partials: what rows_gray_partials
    wrote for the same src, height and width earlier on this stream.  A row whose factors are all 1 is copied or mirrored as
    copy_rows_u8_flip does it; factors = partials = None means that for every row (din_copy_rows_u8_jitter, include/din_hip.h)."""
    lib = L.load()
    n = _jitter_tables("copy_rows_u8_jitter", (src, dst) + (() if flip is None else (flip,)), n)
    if (factors is None) != (partials is None):
        raise L.DinError("copy_rows_u8_jitter: factors and partials come together")
    if factors is not None:
        require_gpu(factors)
        if factors.dtype != torch.float32 or not factors.is_contiguous() or factors.numel() < 3 * n:
            raise L.DinError(f"copy_rows_u8_jitter: factors must be a contiguous fp32 device tensor of {n} triples, got {factors.dtype} x "
                             f"{factors.numel()}")
        _check_partials("copy_rows_u8_jitter", partials, n, height, width)
    L.check(lib.din_copy_rows_u8_jitter(_ptr(src), _ptr(dst), _ptr(flip), _ptr(factors), _ptr(partials), n, height, width, _stream()),
            "copy_rows_u8_jitter")


FEAT_ROWS_SEGMENT = 16384       # DIN_FEAT_ROWS_SEGMENT (include/din_hip.h): bytes of one row per work item of din_feat_rows


def _feat_rows_count(what: str, tables, boxes, flags, box_bytes: int, n: Optional[int]) -> int:
    """the checks feat_rows and feat_rows_bf16 share: int64 device tables of at least n entries, boxes and flags that cover n rows"""
    require_gpu(*tables, boxes, flags)
    if any(t.dtype != torch.int64 for t in tables):
        raise L.DinError(f"{what}: address tables are int64 device tensors")
    rows = min(t.numel() for t in tables)
    n = rows if n is None else n
    if n > rows:
        raise L.DinError(f"{what}: n = {n} rows but the tables hold {[t.numel() for t in tables]} addresses")
    if boxes is not None and (not boxes.is_contiguous() or boxes.numel() * boxes.element_size() < n * box_bytes):
        raise L.DinError(f"{what}: boxes must be contiguous and hold n * box_bytes = {n * box_bytes} bytes")
    if flags is not None and (flags.dtype != torch.uint8 or not flags.is_contiguous() or flags.numel() < n):
        raise L.DinError(f"{what}: flags is a contiguous uint8 tensor of at least n = {n} entries")
    return n


def feat_rows(src: torch.Tensor, dst: torch.Tensor, row_bytes: int, keep: Optional[torch.Tensor] = None,
              ref_boxes: Optional[torch.Tensor] = None, boxes: Optional[torch.Tensor] = None, flags: Optional[torch.Tensor] = None,
              box_bytes: int = 0, n: Optional[int] = None) -> None:
    """row i: `row_bytes` bytes from device address src[i] to dst[i] and, where keep[i] != 0, to keep[i] too, followed there by row i of
    `boxes` (`box_bytes` bytes); where ref_boxes[i] != 0, row i of `boxes` is compared with the bytes at that address and flags[i] = 1 is
    written on a difference.  One launch on the current stream; src[i] == 0 leaves row i alone.  src, dst, keep, ref_boxes: int64 device
    tables; boxes: a contiguous device tensor of n rows of box_bytes bytes; flags: uint8 on the device, one per row (din_feat_rows: the
    feature cache's gather + insert + box check).  Every address and both sizes are multiples of 16."""
    lib = L.load()
    n = _feat_rows_count("feat_rows", [t for t in (src, dst, keep, ref_boxes) if t is not None], boxes, flags, box_bytes, n)
    L.check(lib.din_feat_rows(_ptr(src), _ptr(dst), _ptr(keep), _ptr(ref_boxes), _ptr(boxes), _ptr(flags), n, row_bytes, box_bytes,
                              _stream()), "feat_rows")


def feat_rows_bf16(src: torch.Tensor, dst: torch.Tensor, row_elems: int, keep: Optional[torch.Tensor] = None,
                   ref: Optional[torch.Tensor] = None, boxes: Optional[torch.Tensor] = None, flags: Optional[torch.Tensor] = None,
                   box_bytes: int = 0, src_f32: Optional[torch.Tensor] = None, n: Optional[int] = None) -> None:
    """feat_rows over rows of `row_elems` bf16 values (the feature cache's bf16 storage): where src_f32[i] != 0, src[i] addresses
    `row_elems` fp32 values, which are rounded to bf16 (round-to-nearest-even) on their way to dst[i] and keep[i]; every other row is
    feat_rows at row_bytes = 2 * row_elems.  `ref`: feat_rows's ref_boxes; src_f32: an int64 device table like the others
    (din_feat_rows_bf16).  One launch on the current stream; every address and box_bytes are multiples of 16, row_elems of 8."""
    lib = L.load()
    n = _feat_rows_count("feat_rows_bf16", [t for t in (src, dst, keep, ref, src_f32) if t is not None], boxes, flags, box_bytes, n)
    L.check(lib.din_feat_rows_bf16(_ptr(src), _ptr(dst), _ptr(keep), _ptr(ref), _ptr(src_f32), _ptr(boxes), _ptr(flags), n, row_elems,
                                   box_bytes, _stream()), "feat_rows_bf16")
