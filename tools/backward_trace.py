#!/usr/bin/env python3
"""The launch sequence of the backbone's reverse pass (nhwc.graph_backward), recorded with no GPU: profiles/backward_launch_trace.txt
(and, with --forward, of its forward pass: profiles/forward_launch_trace.txt).

libdin_hip.so is loaded as usual, but nhwc sees it through a proxy: the planning queries (workspace sizes, group keys, packed sizes and
descriptors, kernel reporters, din_conv_accepts_u8, din_conv_dgrad_x_fused, din_conv_rf_eligible, din_conv_rf5_eligible, din_bn_parts, the option and error calls) reach the library,
every entry point that would launch is recorded and answered with 0.  Tensors live on the CPU (torch.empty never touches its pages, so
production shapes cost nothing); the stream queries are stubbed.  What is recorded is the complete host behaviour of the pass:

    N nb=<frames> dtype=<dt>          first line of a case: what every descriptor of the case carries unless it says otherwise
    <entry point> <argument> ... [| <kind> <name> <cout> [src_couts=...] [flops=...]]
                                      one line per C-ABI call of the reverse pass, every argument in order; behind the bar the
                                      LAUNCH_TIMER block it ran in (kind, name, and of the descriptor what profiling.LaunchTimer reads)
    H<i>                              GRAD_HOOK(params[i], its gradient): at the end of the line of the call it follows
    G <tid> <op name>                 GRAD_TAP
    R <i>[=<pointer>] ...             the returned weight / bias gradients that are not None (no pointer: the buffer dw<i>)
    R bn=<tensor> x<n> #<hash>        the n returned BatchNorm parameter gradients: the buffer they are slices of (* = several) and a
                                      digest of all their "<i>=<pointer>"

Arguments: integers and floats as they are; a conv / pool descriptor as D:<hash> / P:<hash> of its fields but nb and dtype, their values
listed once in the table at the end of the file (/nb=..,dtype=.. behind it where they are not the case's); an array of ConvSrc / ConvWSrc /
ConvWgradItem as [{value ...} ...], the fields in the order include/din_hip.h declares them (reserved ones left out); a workspace
(pointer, size) pair as ws or null (its size depends on the history of the shared buffer); the stream as st.  Pointers are
allocator-independent: <tensor>[+<byte offset>] with buf<tid> a forward buffer, p<i> a parameter, og<tid> an incoming output gradient,
dw<i> the weight-gradient buffer GRAD_BUFFER handed out for params[i], aux<op>.<j> / wpt<op> / bnscale / bnptrs / bnoffs what the forward
pass kept, g<tid> the gradient buffer of tensor tid that the reverse pass allocated (GRAD_TAP tells which it is), and t<k> the k-th other
tensor the reverse pass allocated, in the order it made them (every tensor is kept alive for the duration of a case, so no address
repeats).  Naming by allocation and not by first appearance in the trace keeps a deferred launch from renumbering everything behind it,
so that a case differs from its base case only where its launches do.

--forward records the forward pass (nhwc.graph_forward) instead, into profiles/forward_launch_trace.txt: the same lines for every C-ABI
call of it (behind the bar also rf=<the d.rf tuple> when nhwc set one: profiling.LaunchTimer names the kernel from it), the same
descriptor table and the same writing of a case as its difference from a base case.  Its pointers are named once the pass has returned,
by role: img the image tensor handed in, buf<tid> the returned buffers, p<i>, aux<op>.<j> (a view of bnscale keeps that name), bnscale /
bnshift / bnptrs / bnoffs, of the pack cache wpk<op> / wpt<op> / wfused<op> (the banks) and packtable / packlayer / packchunk (the tables
of din_conv_pack_multi), t<k> every other tensor the pass allocated.  Its last line:
    R bufs=<tid>,... aux=(<pointer or ->,...) ...      the entries of bufs that are not None; every aux[op] tuple, - for None
It has the cases of the reverse trace and some of its own (FUSE_FWD_SIBLINGS off, save_for_backward=False, bn-train at 40 frames, no
uint8 frames).

Cases (all parameter gradients requested): see cases().  Notes:
  * the side stream (WGRAD_SIDE_STREAM) needs real streams and is not traced (tests/test_gpu_din_model.py runs it on the GPU);
  * `parked` runs the lone-1x1 path (the strided sibling that was to carry the 1x1's data gradient receives no gradient); the DinError
    for a parked gradient that nobody carried cannot be reached through graph_backward: the strided host precedes the 1x1 in program
    order, so the reverse pass always visits it afterwards, and either branch it can take there consumes the parked entry.

    python tools/backward_trace.py > profiles/backward_launch_trace.txt
    python tools/backward_trace.py --forward > profiles/forward_launch_trace.txt

A case that differs from another by a switch, an option, the frame count or the compute type is written as its difference from that
case: '~ <base case>', then for every run of lines that differs '@ i j' (lines [i, j) of the base's section, its '== name' line being
line 0) and the '+ line's that stand there instead.

tests/test_backward_trace_cpu.py and tests/test_forward_trace_cpu.py regenerate every case and compare the file the tool would write with
the committed one."""
import bisect
import contextlib
import ctypes as C
import difflib
import hashlib
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

QUERIES = ("din_conv_packed_elems", "din_conv_pack_desc", "din_conv_accepts_u8", "din_conv_dgrad_x_fused", "din_conv_rf_eligible",
           "din_conv_rf_kernel_names", "din_conv_rf5_eligible", "din_conv_rf5_kernel_names", "din_bn_parts", "din_set_option", "din_get_option", "din_last_error_string", "din_abi_version",
           "din_build_arch")
STREAM = 0x57


def is_query(name):
    return name in QUERIES or "workspace" in name or name.endswith("_group_key") or name.startswith("din_conv_kernel_")


class Recorder:
    """the events of one case, and the names of the tensors its pointers fall into"""

    def __init__(self, descs, nb=0, dtypes=(0, 0)):
        self.lines, self.descs = [], descs
        self.common = {"D": (nb, dtypes[0]), "P": (nb, dtypes[1])}      # frames and dtype every conv / pool descriptor of the case carries
        self.timed = None                         # the LAUNCH_TIMER entry the next call line will carry
        self.bn = None                            # (buffer, count, every "index=pointer") of the returned BatchNorm parameter gradients
        self.known, self.starts = [], []          # sorted (start, end, label) of the tensors with a fixed name
        self.alive, self.made = [], []            # every tensor nhwc allocated; [start, end, its name once known] of the reverse pass's
        self.on = False

    def name(self, label, t):
        if t is None or t.numel() == 0:
            return
        s = t.untyped_storage()
        lo = s.data_ptr()
        i = bisect.bisect_right(self.starts, lo)
        if i and self.known[i - 1][1] > lo:       # a view of something already named
            return
        self.alive.append(t)
        self.starts.insert(i, lo)
        self.known.insert(i, (lo, lo + s.nbytes(), label))

    def keep(self, t):
        self.alive.append(t)
        if t.numel() and self.on:
            s = t.untyped_storage()
            self.made.append([s.data_ptr(), s.data_ptr() + s.nbytes(), None])
        return t

    def gradient_of(self, tid, t):
        """t is the gradient buffer of tensor tid (GRAD_TAP says so): g<tid> if the pass allocated it"""
        for m in self.made:
            if m[0] <= t.data_ptr() < m[1]:
                m[2] = f"g{tid}"

    def role(self, label, t):
        """t is known by its role now that the pass has returned: the name of the allocation of the pass it lives in (unless that has one
        already), or, when the pass did not make it, of the tensor itself"""
        if t is None or t.numel() == 0:
            return
        p = t.untyped_storage().data_ptr()
        for m in self.made:
            if m[0] <= p < m[1]:
                m[2] = m[2] or label
                return
        self.name(label, t)

    def finish(self):
        """the lines with the allocations of the pass named: by role (g<tid>, buf<tid>, ...), the others t<k> in the order they were made;
        a pointer that no tensor held when its call was recorded is looked up again among the tensors named since"""
        k = 0
        for m in self.made:
            if m[2] is None:
                m[2], k = f"t{k}", k + 1

        def named(text):
            text = re.sub("\0@(\\d+)\0", lambda x: self.ptr(int(x.group(1)), final=True), text)
            return re.sub("\0(\\d+)\0", lambda x: self.made[int(x.group(1))][2], text)
        lines = [named(line) for line in self.lines]
        if self.bn is not None:
            base, n, every = self.bn
            lines.append(f"R bn={named(base)} x{n} #{hashlib.blake2s(named(every).encode(), digest_size=4).hexdigest()}")
        return lines

    def ptr(self, p, final=False):
        p = getattr(p, "value", p)
        if not p:
            return "null"
        if p == STREAM:
            return "st"
        i = bisect.bisect_right(self.starts, p)
        if i and p < self.known[i - 1][1]:
            return self.known[i - 1][2] + (f"+{p - self.known[i - 1][0]}" if p > self.known[i - 1][0] else "")
        for i, m in enumerate(self.made):
            if m[0] <= p < m[1]:
                return f"\0{i}\0" + (f"+{p - m[0]}" if p > m[0] else "")       # (named when the case ends: finish)
        return "unknown" if final else f"\0@{p}\0"

    def desc(self, d, tag):
        text = " ".join(str(getattr(d, n)) for n, _ in d._fields_ if n not in ("nb", "dtype"))
        key = tag + ":" + hashlib.blake2s((tag + text).encode(), digest_size=4).hexdigest()
        assert self.descs.setdefault(key, text) == text
        return key + ("" if (d.nb, d.dtype) == self.common[tag] else f"/nb={d.nb},dtype={d.dtype}")

    def hook(self, i):
        if self.timed is None and self.lines and not self.lines[-1].startswith(("G ", "N ")):
            self.lines[-1] += f" H{i}"            # behind the call (or the hooks) it follows
        else:
            self.event(f"H{i}")

    def event(self, line):
        if self.timed is not None:                # (a timed block that made no call: on a line of its own)
            self.lines.append(self.timed)
            self.timed = None
        self.lines.append(line)

    def struct(self, s, L):
        out = []
        for n, ty in s._fields_:
            v = getattr(s, n)
            if ty is L.ConvDesc:
                out.append(self.desc(v, 'D'))
            elif ty is C.c_void_p:
                out.append(self.ptr(v))
            elif n != "reserved":
                out.append(str(v))
        return "{" + " ".join(out) + "}"

    def call(self, L, name, args):
        argtypes = L.SIGNATURES[name][1]
        out, skip = [], False
        for i, (a, ty) in enumerate(zip(args, argtypes)):
            if skip:
                skip = False
            elif ty is C.c_void_p and i + 1 < len(argtypes) and argtypes[i + 1] is C.c_int64:
                out.append("ws" if getattr(a, "value", a) else "null")
                skip = True
            elif ty is C.c_void_p:
                out.append(self.ptr(a))
            elif ty in (C.POINTER(L.ConvDesc), C.POINTER(L.PoolDesc)):
                out.append(self.desc(a._obj, "D" if ty is C.POINTER(L.ConvDesc) else "P"))
            elif isinstance(ty, type) and issubclass(ty, C._Pointer):
                elems = a[:args[0]] if isinstance(a, C.Array) else [a._obj]
                out.append("[" + " ".join(self.struct(e, L) for e in elems) + "]")
            else:
                out.append(repr(a))
        line, self.timed = name + " " + " ".join(out) + (" | " + self.timed if self.timed is not None else ""), None
        self.lines.append(line)


class LibProxy:
    def __init__(self, lib, L, rec):
        self._lib, self._L, self._rec = lib, L, rec

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if is_query(name):
            return fn

        def launch(*args):
            if self._rec.on:
                self._rec.call(self._L, name, args)
            return 0
        return launch


class TorchProxy:
    """torch as nhwc sees it: every tensor it allocates is kept (and known to the recorder)"""

    def __init__(self, torch, rec):
        self._torch, self._rec = torch, rec

    def __getattr__(self, name):
        fn = getattr(self._torch, name)
        if name in ("empty", "zeros", "empty_like", "cat"):
            return lambda *a, **kw: self._rec.keep(fn(*a, **kw))
        return fn


class _Stream:
    cuda_stream = STREAM


@contextlib.contextmanager
def dry_run(rec):
    """nhwc on the CPU: library proxy, allocation proxy, stubbed streams, recording hooks; everything is put back on exit"""
    import torch
    from din_amd import _lib as L, nhwc
    lib = L.load()
    saved = {(nhwc, n): getattr(nhwc, n) for n in ("_stream", "torch", "LAUNCH_TIMER", "GRAD_HOOK", "GRAD_TAP", "GRAD_BUFFER", "GRAD_ASSIGN",
                                                   *nhwc._SWITCHES)}
    saved.update({(L, "load"): L.load, (torch.cuda, "current_stream"): torch.cuda.current_stream,
                  (torch.cuda, "current_device"): torch.cuda.current_device})
    proxy = LibProxy(lib, L, rec)
    try:
        L.load = lambda: proxy
        nhwc._stream = lambda: C.c_void_p(STREAM)
        nhwc.torch = TorchProxy(torch, rec)
        torch.cuda.current_stream = lambda *a, **kw: _Stream()
        torch.cuda.current_device = lambda: 0
        nhwc._WS.clear()
        yield L, nhwc
    finally:
        for (owner, n), v in saved.items():
            setattr(owner, n, v)
        nhwc._WS.clear()


def trace(g, params, dt, nb, descs, u8=False, bn_train=False, grads_for=None, switches=(), options=(), forward=False, save_for_backward=True):
    """the trace of one run of graph g on nb frames: (lines, outcome).  forward: of its forward pass (graph_forward with
    save_for_backward as given); otherwise of the reverse pass that follows a forward pass"""
    import torch
    from din_amd import _lib
    rec = Recorder(descs, nb, (dt, _lib.storage_dtype(dt)))
    with dry_run(rec) as (L, nhwc):
        for o, v in options:
            L.set_option(o, v)
        try:
            for s in switches:
                setattr(nhwc, s, False)
            ti = g.tensors[g.input_tid]
            u8 = u8 and nhwc._accepts_u8_frames(g, nb, dt)
            img = torch.empty((nb, 3, ti.h, ti.w), dtype=torch.uint8) if u8 else torch.empty((nb, ti.h, ti.w, ti.c), dtype=nhwc.torch_dtype(dt))

            @contextlib.contextmanager
            def timer(kind, d, name):
                extra = "".join(f" {a}={getattr(d, a)}" for a in ("src_couts", "flops_override") if hasattr(d, a))
                if forward and getattr(d, "rf", None) is not None:
                    extra += f" rf={d.rf}"
                rec.event("")
                rec.lines.pop()
                rec.timed = f"{kind} {name} {d.cout}{extra}".replace("flops_override", "flops").replace(", ", ",")
                yield
            try:
                if forward:
                    nhwc.LAUNCH_TIMER, rec.on = timer, True
                bufs, aux = nhwc.graph_forward(g, img, params, dt, save_for_backward, bn_train)
                rec.on = False
                # the tensors of the forward pass by role (a view of something named earlier in this list keeps that name)
                pc, bn = g._pack_cache, getattr(g, "_bn_tables", None)
                roles = [("img", img)] if forward else []
                roles += [(f"buf{tid}", b) for tid, b in enumerate(bufs)] + [(f"p{i}", p) for i, p in enumerate(params)]
                roles += [("bnscale", pc.bn_scale), ("bnshift", pc.bn_shift)] + [(f"wpt{oi}", t) for oi, t in pc.wpt.items()]
                if bn is not None:
                    roles += [("bnptrs", bn.ptrs), ("bnoffs", bn.offs)]
                roles += [(f"aux{oi}.{j}", t) for oi, a in enumerate(aux) for j, t in enumerate(a)]
                roles += [(f"wpk{oi}", t) for oi, t in pc.wpk.items()] + [(f"wfused{oi}", t) for oi, t in pc.wfused.items()]
                roles += [("packtable", pc.table), ("packlayer", pc.layer_of), ("packchunk", pc.chunk_index)]
                for label, t in roles:
                    rec.role(label, t)
                if forward:
                    held = ["(" + ",".join("-" if t is None else rec.ptr(t.data_ptr()) for t in a) + ")" for a in aux]
                    rec.event("R bufs=" + ",".join(str(tid) for tid, b in enumerate(bufs) if b is not None) + " aux=" + " ".join(held))
                else:
                    lines_of_backward(rec, nhwc, torch, g, bufs, aux, params, dt, grads_for, bn_train, timer)
                outcome = "ok"
            except L.DinError as e:
                outcome = "DinError: " + str(e)
            rec.on = False
        finally:
            for o, _ in options:
                L.set_option(o, None)
            for attr in ("_pack_cache", "_bn_tables"):
                g.__dict__.pop(attr, None)
    return [f"N nb={nb} dtype={dt}"] + rec.finish(), outcome


def lines_of_backward(rec, nhwc, torch, g, bufs, aux, params, dt, grads_for, bn_train, timer):
    """graph_backward under the recording hooks, and the R lines of what it returned"""
    og = {tid: torch.empty_like(bufs[tid]) for tid in (g.output_tids if grads_for is None else grads_for)}
    for tid, t in og.items():
        rec.name(f"og{tid}", t)
    index = {id(p): i for i, p in enumerate(params)}

    def grad_buffer(w):
        t = torch.empty_like(w)
        rec.name(f"dw{index[id(w)]}", t)
        return t
    nhwc.GRAD_BUFFER = grad_buffer
    nhwc.GRAD_HOOK = lambda w, dw: rec.hook(index[id(w)])
    nhwc.GRAD_TAP = lambda tid, name, gout: (rec.gradient_of(tid, gout), rec.event(f"G {tid} {name}"))
    nhwc.GRAD_ASSIGN = None
    nhwc.LAUNCH_TIMER = timer
    rec.on = True
    grads = nhwc.graph_backward(g, bufs, aux, params, dt, og, [True] * len(params), bn_train)
    named = [(i, rec.ptr(t.data_ptr())) for i, t in enumerate(grads) if t is not None]
    is_bn = [".bn." in n for n in g.param_names()]
    bn = [(i, p) for i, p in named if is_bn[i]]
    rec.event("R " + " ".join(str(i) if p == f"dw{i}" else f"{i}={p}" for i, p in named if not is_bn[i]))
    if bn:                                 # gamma / beta gradients: slices of one or a few buffers, as a count and a digest
        bases = {p.split("+")[0] for _, p in bn}
        rec.bn = (bases.pop() if len(bases) == 1 else "*", len(bn), " ".join(f"{i}={p}" for i, p in bn))


_NETS = {}


def backbone(kind, dtype, h, w):
    """(graph, dt, params) of a backbone on the CPU; one module per backbone serves every compute type"""
    from din_amd.backbone import backbone as B
    if kind not in _NETS:
        _NETS[kind] = (B.MyInception_v3 if kind == "inv3" else B.MyVGG16)(compute_dtype="fp32")
    net = _NETS[kind]
    net.compute_dtype = dtype
    g, dt = net.graph_for(h, w)
    return g, dt, net._ordered_params(g)


def _params(g, shapes):
    import torch
    out = []
    for name in g.param_names():
        shape = shapes[name.split(".")[0]]
        out.append(torch.zeros(shape if name.endswith("conv.weight") else shape[0]))
    return out


def partial_heads():
    """the stem + three 1x1 heads of test_partial_1x1_group_degrades_to_per_layer_wgrad; no gradient into the middle head"""
    from din_amd import _lib as L, nhwc
    gb = nhwc.GraphBuilder(48, 64, 8)
    x = gb.conv("stem", gb.full(gb.g.input_tid), 192, (3, 3), (1, 1), (1, 1), relu=True, bn=True)
    outs = [gb.conv(n, x, c, (1, 1), relu=True, bn=True) for n, c in (("a", 64), ("b", 48), ("c", 64))]
    gb.g.output_tids = [o.tid for o in outs]
    shapes = {"stem": (192, 3, 3, 3), "a": (64, 192, 1, 1), "b": (48, 192, 1, 1), "c": (64, 192, 1, 1)}
    return gb.g, L.DIN_BF16, _params(gb.g, shapes), [outs[0].tid, outs[2].tid]


def parked():
    """a 1x1 / stride-1 conv and a 3x3 / stride-2 conv read one non-input view, a 3x3 / stride-1 conv between them in program order;
    the strided conv's output gets no gradient, so the 1x1's parked data gradient runs alone -- after the middle conv's, which is how
    the trace tells it from a 1x1 that was never parked"""
    from din_amd import _lib as L, nhwc
    gb = nhwc.GraphBuilder(48, 64, 8)
    x = gb.conv("stem", gb.full(gb.g.input_tid), 64, (3, 3), (1, 1), (1, 1), relu=True, bn=True)
    s = gb.conv("strided", x, 96, (3, 3), (2, 2), (0, 0), relu=True, bn=True)
    m = gb.conv("middle", x, 32, (3, 3), (1, 1), (1, 1), relu=True, bn=True)
    p = gb.conv("lone", x, 64, (1, 1), relu=True, bn=True)
    gb.g.output_tids = [s.tid, m.tid, p.tid]
    shapes = {"stem": (64, 3, 3, 3), "strided": (96, 64, 3, 3), "middle": (32, 64, 3, 3), "lone": (64, 64, 1, 1)}
    return gb.g, L.DIN_BF16, _params(gb.g, shapes), [m.tid, p.tid]


def cases(forward=False):
    """(name, the case it is written as a difference from or None, keyword arguments of trace) of every case, lazily; forward: and the
    cases that only the forward trace has"""
    big = lambda nb, **kw: lambda: dict(zip(("g", "dt", "params"), backbone("inv3", "bf16", 720, 1280)), nb=nb, u8=True, **kw)       # noqa: E731
    small = lambda dtype, **kw: lambda: dict(zip(("g", "dt", "params"), backbone("inv3", dtype, 139, 203)), nb=2, **kw)               # noqa: E731
    forced = (("DIN_WGRAD_1X1_MULTI", "2"), ("DIN_WGRAD_HALO", "2"))

    def one_output(j):
        def make():
            kw = big(4)()
            kw["grads_for"] = [kw["g"].output_tids[j]]
            return kw
        return make

    def built(fn, **kw):
        def make():
            g, dt, params, grads_for = fn()
            return dict(g=g, dt=dt, params=params, nb=2, u8=True, grads_for=grads_for, **kw)
        return make
    b4, b40 = "inv3 bf16 4x720x1280 u8", "inv3 bf16 40x720x1280 u8"
    yield b4, None, big(4)
    yield b40, b4, big(40)
    yield b4 + " bn-train", None, big(4, bn_train=True)
    for s in ("FUSE_1X1_DGRAD", "FUSE_WGRAD_SIBLINGS", "FUSE_WGRAD_1X1", "FUSE_DGRAD_X", "GROUP_WGRAD"):
        yield f"{b40} {s}=off", b40, big(40, switches=(s,))
    yield b40 + " DIN_GROUP_WGRAD_MAX=4", b40, big(40, options=(("DIN_GROUP_WGRAD_MAX", "4"),))
    yield "inv3 fp32 2x139x203", None, small("fp32")
    yield "inv3 fp32_bf16x3 2x139x203", "inv3 fp32 2x139x203", small("fp32_bf16x3")
    yield "inv3 bf16 2x139x203", "inv3 fp32 2x139x203", small("bf16")
    yield "inv3 bf16 2x139x203 DIN_WGRAD_1X1_MULTI=2 DIN_WGRAD_HALO=2", "inv3 bf16 2x139x203", small("bf16", options=forced)
    yield b4 + " Mixed_5d-only", b4, one_output(0)
    yield b4 + " Mixed_6e-only", b4, one_output(1)
    yield "vgg16 fp32 2x96x160", None, lambda: dict(zip(("g", "dt", "params"), backbone("vgg16", "fp32", 96, 160)), nb=2)
    yield "vgg16 bf16 4x720x1280", None, lambda: dict(zip(("g", "dt", "params"), backbone("vgg16", "bf16", 720, 1280)), nb=4, u8=True)
    yield "partial-heads bf16 2x48x64 DIN_WGRAD_1X1_MULTI=2", None, built(partial_heads, options=(("DIN_WGRAD_1X1_MULTI", "2"),))
    yield "parked bf16 2x48x64", None, built(parked)
    if forward:
        yield b40 + " FUSE_FWD_SIBLINGS=off", b40, big(40, switches=("FUSE_FWD_SIBLINGS",))
        yield b4 + " save_for_backward=False", b4, big(4, save_for_backward=False)
        yield b40 + " bn-train", b4 + " bn-train", big(40, bn_train=True)
        yield "inv3 bf16 4x720x1280", b4, lambda: dict(big(4)(), u8=False)


def sections(forward=False):
    """[(case name, lines of its section)] + the descriptor table as the last section; of the reverse pass, or of the forward pass"""
    descs, out = {}, []
    for name, _base, make in cases(forward):
        kw = make()
        if forward:
            kw.pop("grads_for", None)
        lines, outcome = trace(descs=descs, forward=forward, **kw)
        out.append((name, [f"== {name}"] + lines + [f"== end: {outcome}"]))
    from din_amd import _lib as L
    fields = ["# " + tag + ": " + " ".join(n for n, _ in ty._fields_ if n not in ("nb", "dtype")) for tag, ty in (("D", L.ConvDesc), ("P", L.PoolDesc))]
    out.append(("descriptors", ["== descriptors"] + fields + [f"{k} {v}" for k, v in sorted(descs.items())]))
    return out


HEADER = ["# tools/backward_trace.py: the launch sequence of nhwc.graph_backward, recorded on the CPU (format and cases: the tool's docstring)",
          "# every listed case is built at its listed shape; the DinError for a parked 1x1 data gradient that nobody carried is not recorded: no "
          "graph reaches it through graph_backward (the tool's docstring says why; tests/test_backward_trace_cpu.py raises it on the pass state)"]


HEADER_FORWARD = ["# tools/backward_trace.py --forward: the launch sequence of nhwc.graph_forward, recorded on the CPU (format and cases: the tool's docstring)"]


def written(secs, forward=False):
    """the lines of the file: a case with a base is written as what replaces lines [i, j) of the base's section ('@ i j', then '+ line's)"""
    full, base_of, out = dict(secs), {name: base for name, base, _ in cases(forward)}, list(HEADER_FORWARD if forward else HEADER)
    for name, lines in secs:
        base = base_of.get(name)
        if base is None:
            out += lines
            continue
        out += [lines[0], f"~ {base}"]
        for op, i1, i2, j1, j2 in difflib.SequenceMatcher(None, full[base], lines, autojunk=False).get_opcodes():
            if op != "equal" and (i1, j1) != (0, 0):
                out += [f"@ {i1} {i2}"] + ["+ " + line for line in lines[j1:j2]]
    return out


def main():
    forward = sys.argv[1:] == ["--forward"]
    if sys.argv[1:] and not forward:
        sys.exit("usage: backward_trace.py [--forward]")
    print("\n".join(written(sections(forward), forward)))


if __name__ == "__main__":
    main()
