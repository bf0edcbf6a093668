"""FusedAdam: torch.optim.Adam semantics (train_net_dynamic.py:104: lr, weight_decay, default betas/eps) with the update
of the WHOLE parameter list done by one din_adam_step_multi launch (fp32 moments; pointer / chunk tables live on the
device, only the gradient addresses are refreshed per step).  Exposes `param_groups[i]['lr']` so the reference's
adjust_lr (train_net_dynamic.py:22-25) works unchanged, and `state_dict()` / `load_state_dict()` in torch.optim.Adam's
own format, so the `'optimizer'` entry of a reference stage-2 checkpoint (train_net_dynamic.py:141-147) resumes here
and a checkpoint written here loads into torch.optim.Adam."""
from __future__ import annotations

import math

import numpy as np
import torch

import ctypes as C

from . import _lib as L
from . import ops

CHUNK = 8192          # elements per workgroup of the multi-tensor launch
RING = 4              # pinned staging tables per parameter group (the host may run this many optimizer steps ahead of the GPU)


def grad_norm_refusal(value):
    """why `value` cannot be cfg.max_grad_norm / FusedAdam(max_grad_norm=...), or None.  None switches clipping off, float('inf') measures
    and guards without ever clipping; any other value is a positive finite number (both trainers raise ValueError with this before a
    loader exists)."""
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, (int, float)):
        return f"max_grad_norm = {value!r}: not a number (None = off, float('inf') = measure and guard only, else a positive number)"
    if math.isnan(value) or value <= 0:
        return f"max_grad_norm = {value!r}: must be a positive number (None = off, float('inf') = measure and guard only)"
    return None


class _DevState:
    """the device record of one step-count group of FusedAdam(capturable=True): float64 [4] = {steps taken, lr, beta1^steps, beta2^steps}
    (include/din_hip.h: din_adam_state_advance).  Initialised from the host, the powers in double from the fp32 betas the launches
    receive; `lr` is the host's copy of field 1 (FusedAdam.sync_lr)."""

    def __init__(self, device, step, lr, betas):
        b1, b2 = (float(np.float32(b)) for b in betas)
        self.lr = float(lr)
        self.dev = torch.tensor([float(step), self.lr, b1 ** step, b2 ** step], dtype=torch.float64).to(device)


class FusedAdam:
    """max_grad_norm (None = off: nothing below changes): torch.nn.utils.clip_grad_norm_(params, max_grad_norm) folded into the step.  The
    squared norm of every live gradient is reduced in fp64 by one multi-tensor launch over the tables the Adam launch already keeps
    (din_grad_sqnorm_multi), one small launch forms norm = grad_scale * sqrt(total) and coef = min(1, max / (norm + 1e-6)) on the device
    (din_grad_norm_finish), and the Adam launch multiplies the gradient by grad_scale * coef instead of grad_scale
    (din_adam_step_multi_clip): no write pass over the gradients, no host read.  A step whose norm is not finite is SKIPPED: weights and
    moments keep their bits; the per-parameter step count behind the bias correction still advances (it is host state, and reading the
    flag back would be the synchronisation this design avoids).  grad_stats() reads the running statistics, one device read.

    capturable (False = off: nothing above changes): the step count, the learning rate and both beta powers live in a small device record
    per step-count group (_DevState) instead of on the host.  step() launches din_adam_state_advance + din_adam_step_multi_dev per group
    (behind the two norm launches when max_grad_norm is set), reads nothing back and bakes no per-step host value into a launch: the two
    launches replay from a HIP graph as consecutive steps.  param_groups[0]['lr'] stays the interface: a changed value reaches the record
    by a small eager copy (sync_lr) before the next step.  A SKIPPED step does not count in this mode: the record keeps its bits and the
    next step's bias correction is that of the un-advanced count.  state_dict() reads 'step' from the device (one read).  Every parameter
    must be a contiguous fp32 device tensor (ValueError naming the parameter otherwise).  step() itself refuses to run inside a stream
    capture: its address-table upload reads a slot of the rotating pinned RING, which a graph would go on reading after the slot moved
    on (capturing the whole training step is not part of this class yet)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None, capturable=False):
        why_not = grad_norm_refusal(max_grad_norm)
        if why_not:
            raise ValueError(why_not)
        self.params = [p for p in params]
        self.capturable = bool(capturable)
        if self.capturable:
            for i, p in enumerate(self.params):
                if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                    raise ValueError(f"FusedAdam(capturable=True): parameter {i} (shape {tuple(p.shape)}, {p.dtype}, {p.device}, "
                                     f"{'contiguous' if p.is_contiguous() else 'not contiguous'}) is not a contiguous fp32 device tensor; "
                                     f"the non-fused path reads the host-side step count and cannot be captured")
        self._records = {}      # capturable: param -> _DevState of its step-count group (shared by the group's parameters)
        self.param_groups = [dict(params=self.params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)]
        self.state = {}         # param -> (exp_avg, exp_avg_sq)
        self.steps = {}         # param -> number of updates it received (bias correction is per parameter, as in torch)
        self._tables = {}       # group identity -> [key, pinned ring, ptrs_dev, sizes_dev, chunk_tensor_dev, chunk_index_dev, nchunks, events, turn, last grad ptrs]
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)    # (not part of state_dict(): torch.optim.Adam's format)
        self._gstate = None     # device float32 [8]: din_grad_norm_finish's state (norm, coef, running statistics)
        self._partials = None   # device float64 [chunks of the live set]: one squared-norm partial per workgroup
        self._host_stats = [0.0, 0.0, 0, 0, 0]     # norm sum, norm max, steps, skipped, clipped of the non-fused path

    @property
    def step_count(self) -> int:
        if self.capturable:                                      # (one device read)
            return max(self._device_steps().values(), default=0)
        return max(self.steps.values(), default=0)

    def zero_grad(self, set_to_none: bool = True):
        for p in self.params:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    @torch.no_grad()
    def step(self, grad_scale: float = 1.0):
        g = self.param_groups[0]
        live = [p for p in self.params if p.grad is not None]
        if not live:
            return
        if self.capturable:
            self._step_capturable(live, g, grad_scale)
            return
        for p in live:
            if p not in self.state:
                self.state[p] = (torch.zeros_like(p, dtype=torch.float32), torch.zeros_like(p, dtype=torch.float32))
            self.steps[p] = self.steps.get(p, 0) + 1
        fused = all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() for p in live)
        if not fused:
            if self.max_grad_norm is not None:
                grad_scale = self._clip_scale_slow(live, grad_scale)
                if grad_scale is None:
                    return
            for p in live:
                st = self.state[p]
                ops.adam_step(p.data, p.grad.contiguous(), st[0], st[1], g["lr"], g["betas"][0], g["betas"][1], g["eps"],
                              g["weight_decay"], self.steps[p], grad_scale)
            return
        # one launch per distinct step count (normally one: every trainable parameter gets a gradient every step; a parameter whose
        # first gradient arrives later keeps its own bias correction)
        groups = {}
        for p in live:
            groups.setdefault(self.steps[p], []).append(p)
        self._keep = []
        if self.max_grad_norm is not None:
            self._step_clipped(groups, g, grad_scale)
            return
        for step, plist in groups.items():
            self._launch(plist, step, g, grad_scale)

    def _clip_scale_slow(self, live, grad_scale):
        """the non-fused path (non-contiguous or non-fp32 parameters; slow on purpose): the same norm, coefficient and skip rule formed by
        torch ops and decided by ONE read-back.  Returns the factor ops.adam_step multiplies the gradients by, or None to skip the step."""
        total = torch.zeros((), dtype=torch.float64, device=live[0].device)
        for p in live:
            total += p.grad.double().pow(2).sum()
        with np.errstate(over="ignore"):
            norm = np.float32(float(grad_scale) * math.sqrt(float(total.item())))       # (the one read-back; sqrt(nan) is nan)
        hs = self._host_stats
        hs[2] += 1
        if not np.isfinite(norm):
            hs[3] += 1
            return None
        with np.errstate(over="ignore"):
            coef = min(np.float32(1.0), np.float32(self.max_grad_norm) / (norm + np.float32(1e-6)))
        hs[0], hs[1], hs[4] = hs[0] + float(norm), max(hs[1], float(norm)), hs[4] + int(coef < 1)
        return float(np.float32(grad_scale) * np.float32(coef))

    def _step_clipped(self, groups, g, grad_scale):
        """squared norm of every group -> one global norm and coefficient on the device -> the clipped Adam launch of every group"""
        lib = L.load()
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        tables = [(step, self._table(plist)) for step, plist in groups.items()]
        self._measure_norm([tb for _, tb in tables], grad_scale, stream)
        for step, tb in tables:
            L.check(lib.din_adam_step_multi_clip(C.c_void_p(tb[2].data_ptr()), C.c_void_p(tb[3].data_ptr()), C.c_void_p(tb[4].data_ptr()),
                                                 C.c_void_p(tb[5].data_ptr()), tb[6], CHUNK, g["lr"], g["betas"][0], g["betas"][1], g["eps"],
                                                 g["weight_decay"], step, grad_scale, C.c_void_p(self._gstate.data_ptr()), stream),
                    "adam_step_multi_clip")

    def _measure_norm(self, tables, grad_scale, stream):
        """din_grad_sqnorm_multi over every table, then ONE din_grad_norm_finish: self._gstate holds the step's norm and coefficient"""
        lib, dev = L.load(), tables[0][2].device
        total = sum(tb[6] for tb in tables)
        if self._gstate is None:
            self._gstate = torch.zeros(8, dtype=torch.float32, device=dev)
        if self._partials is None or self._partials.numel() != total:              # (only when the live set changes)
            self._partials = torch.empty(max(total, 1), dtype=torch.float64, device=dev)[:total]
        first = 0
        for tb in tables:
            L.check(lib.din_grad_sqnorm_multi(C.c_void_p(tb[2].data_ptr()), C.c_void_p(tb[3].data_ptr()), C.c_void_p(tb[4].data_ptr()),
                                              C.c_void_p(tb[5].data_ptr()), tb[6], CHUNK,
                                              C.c_void_p(self._partials.data_ptr() + 8 * first), stream), "grad_sqnorm_multi")
            first += tb[6]
        L.check(lib.din_grad_norm_finish(C.c_void_p(self._partials.data_ptr()), total, grad_scale, self.max_grad_norm,
                                         C.c_void_p(self._gstate.data_ptr()), stream), "grad_norm_finish")

    # ---- capturable=True: step count, learning rate and beta powers on the device ------------------------------------------------------
    def _step_capturable(self, live, g, grad_scale):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("FusedAdam.step() inside a stream capture: the gradient address table is uploaded from a rotating pinned "
                               "buffer a graph must not keep reading; capture din_adam_state_advance / din_adam_step_multi_dev over "
                               "tables of your own instead")
        fresh = [p for p in live if p not in self._records]
        if fresh:
            rec = _DevState(fresh[0].device, 0, g["lr"], g["betas"])       # (parameters that start together share one record)
            for p in fresh:
                self._records[p] = rec
                if p not in self.state:
                    self.state[p] = (torch.zeros_like(p, dtype=torch.float32), torch.zeros_like(p, dtype=torch.float32))
        self.sync_lr()
        groups = {}
        for p in live:
            groups.setdefault(id(self._records[p]), []).append(p)
        self._keep = []
        lib = L.load()
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        tables = [(self._records[plist[0]], self._table(plist)) for plist in groups.values()]
        clip = None
        if self.max_grad_norm is not None:
            self._measure_norm([tb for _, tb in tables], grad_scale, stream)
            clip = C.c_void_p(self._gstate.data_ptr())
        b1, b2 = g["betas"]
        for rec, tb in tables:
            ostate = C.c_void_p(rec.dev.data_ptr())
            L.check(lib.din_adam_state_advance(ostate, clip, b1, b2, stream), "adam_state_advance")
            L.check(lib.din_adam_step_multi_dev(C.c_void_p(tb[2].data_ptr()), C.c_void_p(tb[3].data_ptr()), C.c_void_p(tb[4].data_ptr()),
                                                C.c_void_p(tb[5].data_ptr()), tb[6], CHUNK, b1, b2, g["eps"], g["weight_decay"], grad_scale,
                                                ostate, clip, stream), "adam_step_multi_dev")

    def sync_lr(self):
        """param_groups[0]['lr'] -> every device record whose copy differs: one small eager copy per record (none when nothing changed);
        step() calls it before its launches"""
        lr = float(self.param_groups[0]["lr"])
        for rec in {id(r): r for r in self._records.values()}.values():
            if rec.lr != lr:
                rec.dev[1:2].copy_(torch.tensor([lr], dtype=torch.float64))
                rec.lr = lr

    def _device_steps(self):
        """param -> steps taken, read from the device records: ONE device -> host read"""
        recs = list({id(r): r for r in self._records.values()}.values())
        if not recs:
            return {}
        host = torch.stack([r.dev for r in recs]).cpu()
        step_of = {id(r): int(round(float(host[i, 0]))) for i, r in enumerate(recs)}
        return {p: step_of[id(r)] for p, r in self._records.items()}

    def grad_stats(self, reset: bool = True):
        """{"steps", "skipped", "clipped", "norm_mean", "norm_max"} of the steps since the last reset: ONE device -> host read (a
        synchronisation: call it once per pass, like the meters).  norm_mean is taken over the steps whose norm was finite (0.0 when there
        was none).  reset=True zeroes the running statistics."""
        hs = self._host_stats
        s = [0.0] * 8 if self._gstate is None else [float(x) for x in self._gstate.cpu()]
        total, nmax = s[2] + hs[0], max(s[3], hs[1])
        steps, skipped, clipped = int(s[4]) + hs[2], int(s[5]) + hs[3], int(s[6]) + hs[4]
        if reset:
            if self._gstate is not None:
                self._gstate[2:7].zero_()
            self._host_stats = [0.0, 0.0, 0, 0, 0]
        finite = steps - skipped
        return {"steps": steps, "skipped": skipped, "clipped": clipped, "norm_mean": total / finite if finite else 0.0, "norm_max": nmax}

    def _launch(self, live, step, g, grad_scale):
        _, _, ptrs_dev, sizes_dev, ct_dev, ci_dev, nchunks, _, _, _ = self._table(live)
        L.check(L.load().din_adam_step_multi(C.c_void_p(ptrs_dev.data_ptr()), C.c_void_p(sizes_dev.data_ptr()),
                                             C.c_void_p(ct_dev.data_ptr()), C.c_void_p(ci_dev.data_ptr()), nchunks, CHUNK,
                                             g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], step,
                                             grad_scale, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "adam_step_multi")

    def _table(self, live):
        """the device tables of one group with this step's gradient addresses in place (uploaded on the current stream when they moved)"""
        dev = live[0].device
        key = tuple(id(p) for p in live)
        slot = key                                               # table cache slot: the group's identity (two step-count groups of equal size
        tb = self._tables.get(slot)                              # must not evict each other every step)
        if tb is None:
            if len(self._tables) > 8:                            # (groups change only when a parameter's first gradient arrives late)
                self._tables.clear()
            sizes = torch.tensor([p.numel() for p in live], dtype=torch.int64)
            ct, ci = [], []
            for t, p in enumerate(live):
                nchunk = (p.numel() + CHUNK - 1) // CHUNK
                ct += [t] * nchunk
                ci += list(range(nchunk))
            base = torch.zeros((len(live), 4), dtype=torch.int64)
            for t, p in enumerate(live):
                base[t, 0], base[t, 2], base[t, 3] = p.data_ptr(), self.state[p][0].data_ptr(), self.state[p][1].data_ptr()
            # RING pinned staging tables, one device table: uploads and launches are ordered on the stream, so only the host-side buffer an
            # upload reads from must stay untouched until that upload ran.  With one buffer (round 3) every step waited for the previous
            # step's upload -- i.e. for the GPU to reach the previous optimizer launch: the host could never run more than one step ahead
            # (VERDICT r3 item 6).  With RING buffers it waits for the upload issued RING steps ago.
            ring = [base.clone().pin_memory() for _ in range(RING)]
            tb = self._tables[slot] = [key, ring, torch.empty((len(live), 4), dtype=torch.int64, device=dev), sizes.to(dev),
                                       torch.tensor(ct, dtype=torch.int32, device=dev), torch.tensor(ci, dtype=torch.int32, device=dev),
                                       len(ct), [None] * RING, 0, None]
        _, ring, ptrs_dev, sizes_dev, ct_dev, ci_dev, nchunks, copied, turn, last = tb
        grads = [p.grad if p.grad.is_contiguous() and p.grad.dtype == torch.float32 else p.grad.float().contiguous() for p in live]
        gptrs = [gr.data_ptr() for gr in grads]
        if gptrs != last:
            # (gradients that live at fixed addresses -- the all-reduce bucket slots of parallel.GradBuckets, the static tensors of a
            #  captured step -- need no upload at all after the first step)
            if copied[turn] is not None:
                copied[turn].synchronize()      # the upload issued RING steps ago must have left this pinned buffer
            ring[turn][:, 1] = torch.tensor(gptrs, dtype=torch.int64)
            ptrs_dev.copy_(ring[turn], non_blocking=True)
            copied[turn] = torch.cuda.Event()
            copied[turn].record()
            tb[8], tb[9] = (turn + 1) % RING, gptrs
        self._keep.append(grads)      # the launch reads these asynchronously
        return tb

    # ---- checkpoint format of torch.optim.Adam (state by parameter index; 'step' as a float32 scalar tensor) ----------------------
    def state_dict(self):
        state = {}
        steps = self._device_steps() if self.capturable else self.steps
        for i, p in enumerate(self.params):
            if p in self.state:
                m, v = self.state[p]
                state[i] = {"step": torch.tensor(float(steps.get(p, 0))), "exp_avg": m.detach().clone(), "exp_avg_sq": v.detach().clone()}
        g = self.param_groups[0]
        group = dict(lr=g["lr"], betas=tuple(g["betas"]), eps=g["eps"], weight_decay=g["weight_decay"], amsgrad=False, maximize=False,
                     foreach=None, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False,
                     params=list(range(len(self.params))))
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd):
        groups = sd["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self.params):
            raise ValueError("FusedAdam.load_state_dict: expected one parameter group with %d parameters" % len(self.params))
        if groups[0].get("amsgrad", False):
            raise ValueError("FusedAdam.load_state_dict: amsgrad state is not supported")
        g = self.param_groups[0]
        for k in ("lr", "betas", "eps", "weight_decay"):
            if k in groups[0]:
                g[k] = tuple(groups[0][k]) if k == "betas" else groups[0][k]
        index_of = {pid: i for i, pid in enumerate(groups[0]["params"])}
        self.state, self.steps, self._tables, self._records = {}, {}, {}, {}
        for pid, st in sd["state"].items():
            p = self.params[index_of[int(pid)]]
            if tuple(st["exp_avg"].shape) != tuple(p.shape):
                raise ValueError("FusedAdam.load_state_dict: moment shape %s != parameter shape %s" % (tuple(st["exp_avg"].shape), tuple(p.shape)))
            self.state[p] = (st["exp_avg"].to(device=p.device, dtype=torch.float32).clone().contiguous(),
                             st["exp_avg_sq"].to(device=p.device, dtype=torch.float32).clone().contiguous())
            self.steps[p] = int(round(float(st["step"])))
        if self.capturable:                                      # one record per distinct step count, the powers computed in double
            by_step = {}
            for p, step in self.steps.items():
                if step not in by_step:
                    by_step[step] = _DevState(p.device, step, g["lr"], g["betas"])
                self._records[p] = by_step[step]
            self.steps = {}
