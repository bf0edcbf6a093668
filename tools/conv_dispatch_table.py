#!/usr/bin/env python3
"""Which kernel every forward / data-gradient convolution of the two backbones resolves to, as din_conv_kernel_tile /
din_conv_kernel_variant report it (no GPU needed): one line per case,

    <backbone> <dtype> nb<frames> <h>x<w> c<cin>><cout> k<kh>x<kw> s<stride> p<ph>,<pw> ld<ldi>+<cioff>><ldo>+<cooff> [u8] which=<0|1> <option>
        ->  bm bn flags workspace_bytes(0) workspace_bytes(1)

Cases: every distinct conv descriptor of the Inception-v3 trunk (up to Mixed_6e, with the channel-offset views and the fused sibling
groups nhwc.py lays out) and of VGG16, at 12 / 24 / 96 frames of 720x1280 and at the small test geometry, both dtypes, plus one view
per kernel family whose channel offsets are not multiples of 8; each with no option set and with every selection option of
choose_gather (csrc/conv_igemm.hip) and of the family rules it calls (plan_halo in csrc/conv_halo.hip, conv_small_variant in
csrc/conv_small.hip, the eligibility rules of csrc/conv_regw.hip and csrc/conv_stream.hip) set alone to each value its comment documents.

The reporter answers from the launcher's own selection function, so two builds that print the same table launch the same kernels:

    python tools/conv_dispatch_table.py > new.txt;  DIN_LIB_PATH=<other build>/libdin_hip.so python tools/conv_dispatch_table.py > old.txt

The full table has ~47 000 lines.  --summary prints what profiles/conv_dispatch_table.txt holds: the no-option decision only, at 96 frames of
720x1280 and at the small test geometry, forward and data gradient on one line (bm bn flags / bm bn flags  workspace bytes).

--names prints what profiles/conv_kernel_names.txt holds: every distinct kernel instantiation din_conv_kernel_names reports over all those
cases with no option set -- forward, and data gradient with flags 0 / MASK / ACCUM / MASK|ACCUM (mask view = the layer's input view) --
each once, with one descriptor that reaches it.  tests/test_gpu_conv_fwd_dgrad.py holds a row for every name in that file.

--names --multi prints what profiles/conv_multi_kernel_names.txt holds: every distinct kernel instantiation the reporters of the three
multi-source / two-destination entry points (din_conv_fwd2_kernel_names, din_conv1x1_dgrad_multi_kernel_names,
din_conv_dgrad_x_kernel_names) answer, with no option set, over the launches nhwc.py makes through them -- the fwd_groups of both backbones
(BIAS | RELU), and the dgrad_groups and x_host pairs of plan_backward with the mask flag forms the reverse pass uses (MASK where the source
tensor is ReLU-masked, with and without ACCUM) -- in bf16, fp32 and fp32_bf16x3 at the four geometries, each once PER ENTRY POINT
(fwd2 | dgrad_multi | dgrad_x, the first word of the line), with one launch that reaches it.  tests/test_gpu_conv_multi.py holds a row for every name in that file.

--names --wgrad-multi prints what profiles/wgrad_multi_kernel_names.txt holds: every distinct (entry point, kernel) pair the reverse pass of
both backbones reaches through din_conv_wgrad_group (wgrad_group) and din_conv1x1_wgrad_multi (wgrad_multi), with no option set, in bf16,
fp32 and fp32_bf16x3 at the four geometries -- the calls are those of tools/backward_trace.py's walk (profiles/backward_launch_trace.txt), each
handed to its entry point's reporter (din_conv_wgrad_group_kernel_names, din_conv1x1_wgrad_multi_kernel_names) -- with one launch that
reaches it.  tests/test_gpu_wgrad_multi.py holds a row for every pair in that file.

The weight gradient follows (--wgrad: only it): for the same descriptors, geometries and dtypes,

    <label> which=2 <option>  ->  bm bn workspace_bytes(2) group_key

with no option set and with every weight-gradient option of csrc/conv_wgrad.hip (plan_wgrad) set alone to each documented value, and for
the 1x1 sibling groups of the Inception blocks

    <label of the first sibling> multi<n> <option>  ->  din_conv1x1_wgrad_multi_workspace

--names --wgrad prints what profiles/wgrad_kernel_names.txt holds: the first line of din_conv_kernel_names(d, 2) -- the main kernel, spelled
as rocprofv3 prints it -- over all those cases with no option set.  Every name in that file has a row in tests/test_gpu_wgrad.py or in
PIPE_CASES of tests/test_gpu_kernels.py."""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

OPTIONS = [
    ("DIN_CONV_BN", ("96", "128", "160", "192", "256")), ("DIN_CONV_TILE", ("128", "256")), ("DIN_CONV_PIPE", ("0", "1", "4", "8")),
    ("DIN_CONV_FASTK", ("0",)), ("DIN_CONV_LANEK", ("0", "2")), ("DIN_CONV_KORDER", ("0",)), ("DIN_CONV_SMALL", ("0",)),
    ("DIN_CONV_HALO", ("0", "2")), ("DIN_CONV_STREAM", ("0", "2")), ("DIN_CONV_STREAM_WIDE", ("0",)),
    ("DIN_CONV_STREAM_MINPIX", ("32768",)), ("DIN_CONV_STREAM_BN", ("64", "96", "192")), ("DIN_CONV_REGW", ("0", "2")),
    ("DIN_CONV_REGW_SHORT", ("0", "2")), ("DIN_CONV_REGW_MINPIX", ("32768",)), ("DIN_CONV_WAVEGRID", ("24",)),
    ("DIN_CONV_ONESTAGE", ("0",)), ("DIN_CONV_SMALL_WAVES", ("4",)), ("DIN_CONV_SMALL_NBUF8", ("2",)), ("DIN_CONV_SMALL_EPI", ("0",)),
    ("DIN_GATHER_PIPE", ("1", "2")), ("DIN_HALO_WAVES", ("8",)),
]
WGRAD_OPTIONS = [
    ("DIN_CONV_BN", ("128",)), ("DIN_CONV_SMALL", ("0",)), ("DIN_WGRAD_HALO", ("0", "2")), ("DIN_WGRAD_RING", ("0", "2", "3")),
    ("DIN_WGRAD_PIPE", ("0", "3")), ("DIN_WGRAD_PIPE_PAD", ("15",)), ("DIN_WGRAD_ATOMIC", ("1",)), ("DIN_WGRAD_BLOCKS", ("20", "100", "2000")),
    ("DIN_WGRAD_SMALL_WAVES", ("4",)), ("DIN_WGRAD_SMALL_RING", ("2",)), ("DIN_WGRAD_PIPE_WAVES", ("8", "4")), ("DIN_WGRAD_GROUP", ("0",)),
]
GEOMETRIES = [(12, 720, 1280), (24, 720, 1280), (96, 720, 1280), (6, 139, 203)]
FIELDS = ("cin", "h", "w", "cout", "oh", "ow", "kh", "kw", "sh", "sw", "ph", "pw", "ldi", "cioff", "ldo", "cooff", "in_u8")


def descriptors(L, nhwc, backbone, nb, h, w, dt, groups=None):
    """the distinct conv descriptors of one backbone graph, in graph order; groups (a list): gains the 1x1 sibling groups' member descriptors"""
    from din_amd.backbone import backbone as B
    net = (B.MyInception_v3 if backbone == "inv3" else B.MyVGG16)(compute_dtype="bf16" if dt == L.DIN_BF16 else "fp32")
    g = net.build_graph(h, w, dt)
    out = []
    for i, op in enumerate(g.ops):
        if op.kind != "conv":
            continue
        first = op.src.tid == g.input_tid
        d = nhwc._pooled_descs(g, op, nb, dt)[0] if op.pooled is not None else nhwc._conv_desc(g, op, nb, dt, g.cin_image if first else None)
        out.append(d)
        if first and dt == L.DIN_BF16:                     # the image layer on raw uint8 frames
            u = nhwc._copy_desc(d)
            u.in_u8, u.ldi, u.cioff = 1, 8, 0
            out.append(u)
    for idx in g.fwd_groups:                               # fused siblings: one launch over the concatenated filter bank
        d = nhwc._copy_desc(out_of(g, nhwc, idx[0], nb, dt))
        d.cout = sum(g.ops[j].dst.c for j in idx)
        d.ldo, d.cooff = d.cout, 0
        out.append(d)
        if groups is not None and d.kh == 1 and d.kw == 1:
            groups.append([out_of(g, nhwc, j, nb, dt) for j in idx])
    return out


def out_of(g, nhwc, i, nb, dt):
    return nhwc._conv_desc(g, g.ops[i], nb, dt)


def misaligned(L, nhwc, descs):
    """one view per kernel family (by the shapes each family serves) moved to channel offsets that are multiples of 4 only"""
    def family(d):
        if d.in_u8 or d.sh != 1:
            return None
        if d.kh == 1 and d.kw == 1:
            return "regw" if d.cin >= 640 else ("stream" if d.cin <= 288 else "tile1x1")
        if d.kh == 3 and d.kw == 3:
            return "small" if d.cin in (32, 64) and d.cout <= 64 else "halo"
        return "tile"
    seen, out = set(), []
    for d in descs:
        fam = family(d)
        if fam is None or fam in seen:
            continue
        seen.add(fam)
        m = nhwc._copy_desc(d)
        m.ldi, m.cioff, m.ldo, m.cooff = d.ldi + 8, d.cioff + (4 if d.dtype == L.DIN_F32 else 8), d.ldo + 8, d.cooff + 4
        out.append(m)
    return out


def report(lib, d, which):
    bm, bn, fl = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    assert lib.din_conv_kernel_tile(C.byref(d), which, C.byref(bm), C.byref(bn)) == 0
    assert lib.din_conv_kernel_variant(C.byref(d), which, C.byref(fl)) == 0
    return f"{bm.value} {bn.value} {fl.value} {lib.din_conv_workspace_bytes(C.byref(d), 0)} {lib.din_conv_workspace_bytes(C.byref(d), 1)}"


def report_wgrad(lib, d):
    bm, bn = C.c_int32(-1), C.c_int32(-1)
    assert lib.din_conv_kernel_tile(C.byref(d), 2, C.byref(bm), C.byref(bn)) == 0
    return f"{bm.value} {bn.value} {lib.din_conv_workspace_bytes(C.byref(d), 2)} {lib.din_conv_wgrad_group_key(C.byref(d))}"


def report_multi(L, lib, members):
    """din_conv1x1_wgrad_multi_workspace of a sibling group (the siblings read one tensor: pixels and cin of the first)"""
    d0 = members[0]
    srcs = (L.ConvWSrc * len(members))()
    for s, m in zip(srcs, members):
        s.cout, s.ldo, s.cooff = m.cout, m.ldo, m.cooff
    return str(lib.din_conv1x1_wgrad_multi_workspace(len(members), srcs, d0.dtype, d0.nb * d0.h * d0.w, d0.cin))


def wgrad_names_table(lib, cases):
    """{main weight-gradient kernel: label of the first descriptor that reaches it}"""
    found = {}
    for label, d in cases:
        if d.in_u8 and not lib.din_conv_accepts_u8(C.byref(d)):
            continue
        found.setdefault(kernel_names(lib, d, 2, 0, sep="\n")[0], label)
    return found


def kernel_names(lib, d, which, flags, ldm=0, moff=0, sep=None):
    """the lines din_conv_kernel_names answers for one launch"""
    buf = C.create_string_buffer(4096)
    rc = lib.din_conv_kernel_names(C.byref(d), which, flags, ldm, moff, buf, len(buf))
    assert 0 < rc <= len(buf), f"din_conv_kernel_names: {rc}"
    return buf.value.decode().split(sep)


def names_table(L, lib, cases):
    """{kernel name: label of the first launch that reaches it}; forward flags 0 (BIAS | RELU select the same kernel)"""
    found = {}
    for label, d in cases:
        if d.in_u8 and not lib.din_conv_accepts_u8(C.byref(d)):      # (raw frames on a map too small for the image-layer kernel: din_conv_fwd rejects it)
            continue
        launches = [(0, 0)] + ([] if d.in_u8 else [(1, f) for f in (0, L.CONV_MASK, L.CONV_ACCUM, L.CONV_MASK | L.CONV_ACCUM)])
        for which, flags in launches:
            for name in kernel_names(lib, d, which, flags, d.ldi, d.cioff):
                found.setdefault(name, f"{label} which={which} flags={flags}")
    return found


def _reporter_lines(rc, buf, what):
    assert 0 < rc <= len(buf), f"{what}: {rc}"
    return buf.value.decode().split()


def multi_names_table(L, lib, nhwc):
    """{(entry point: fwd2 | dgrad_multi | dgrad_x, kernel name): label of the first launch of a backbone through that entry point that reaches it}"""
    from din_amd.backbone import backbone as B
    found = {}
    buf = C.create_string_buffer(4096)
    for backbone in ("inv3", "vgg16"):
        for dt, dtn in ((L.DIN_BF16, "bf16"), (L.DIN_F32, "fp32"), (L.DIN_F32_BF16X3, "fp32_bf16x3")):
            net = (B.MyInception_v3 if backbone == "inv3" else B.MyVGG16)(compute_dtype="bf16" if dt == L.DIN_BF16 else "fp32")
            for nb, h, w in GEOMETRIES:
                g = net.build_graph(h, w, L.DIN_BF16 if dt == L.DIN_BF16 else L.DIN_F32)
                head = f"{backbone} {dtn} nb{nb}"
                for s in nhwc.plan_forward(g, nb, dt, False, False, True).steps:      # the sibling groups the forward pass runs as one launch
                    if s.route != "lead":
                        continue
                    grp, d, csplit = s.group, s.d, g.ops[s.group.members[0]].dst.c
                    rc = lib.din_conv_fwd2_kernel_names(C.byref(d), g.tensors[grp.v2.tid].c, grp.v2.coff, csplit, grp.craw, s.flags, buf, len(buf))
                    for name in _reporter_lines(rc, buf, "din_conv_fwd2_kernel_names"):
                        found.setdefault(("fwd2", name), f"{head} {grp.name} {d.h}x{d.w} c{d.cin}>{grp.ctot} csplit{csplit} flags={s.flags}")
                plan = nhwc.plan_backward(g, nb, dt, False, False, False)

                def source(oi):                            # the gradient operand of op oi as the reverse pass hands it on (_ConvStep)
                    o = g.ops[oi]
                    s = L.ConvSrc()
                    s.cout = o.dst.c
                    s.ldo, s.cooff = (o.dst.c, 0) if o.pooled is not None else (g.tensors[o.dst.tid].c, o.dst.coff)
                    return s

                def flag_forms(view):
                    base = L.CONV_MASK if g.tensors[view.tid].relu_masked else 0
                    return (base, base | L.CONV_ACCUM)

                for key, members in plan.dgrad_groups.items():
                    op0 = g.ops[members[0]]
                    ts = g.tensors[op0.src.tid]
                    srcs = (L.ConvSrc * len(members))(*[source(oi) for oi in reversed(members)])      # (the reverse pass meets the last member first)
                    for flags in flag_forms(op0.src):
                        rc = lib.din_conv1x1_dgrad_multi_kernel_names(len(members), srcs, dt, nb, ts.h, ts.w, op0.src.c, ts.c, op0.src.coff, ts.c, op0.src.coff,
                                                                      flags, buf, len(buf))
                        for name in _reporter_lines(rc, buf, "din_conv1x1_dgrad_multi_kernel_names"):
                            found.setdefault(("dgrad_multi", name), f"{head} {'+'.join(g.ops[i].name for i in reversed(members))} {ts.h}x{ts.w} "
                                                   f"c{'+'.join(str(s.cout) for s in srcs)}>{op0.src.c} flags={flags}")
                for oi, host in plan.x_host.items():
                    oph = g.ops[host]
                    ts = g.tensors[oph.src.tid]
                    d, x = nhwc._conv_desc(g, oph, nb, dt), source(oi)
                    for flags in flag_forms(oph.src):
                        rc = lib.din_conv_dgrad_x_kernel_names(C.byref(d), C.byref(x), ts.c, oph.src.coff, flags, buf, len(buf))
                        for name in _reporter_lines(rc, buf, "din_conv_dgrad_x_kernel_names"):
                            found.setdefault(("dgrad_x", name), f"{head} {oph.name}+{g.ops[oi].name} {d.h}x{d.w} c{d.cout}+{x.cout}>{d.cin} k{d.kh}x{d.kw} s{d.sh} "
                                                   f"p{d.ph},{d.pw} flags={flags}")
    return found


def wgrad_multi_names_table(L, lib):
    """{(entry point: wgrad_group | wgrad_multi, kernel name): label of the first launch of a backbone's reverse pass through that entry
    point that reaches it}.  The walk is tools/backward_trace.py's (nhwc.graph_forward + graph_backward on the CPU against the recording
    library proxy): every din_conv_wgrad_group / din_conv1x1_wgrad_multi call the pass makes is handed, arguments unchanged, to the entry
    point's reporter"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("backward_trace", os.path.join(os.path.dirname(os.path.abspath(__file__)), "backward_trace.py"))
    bt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bt)
    found, buf, head = {}, C.create_string_buffer(4096), [""]

    class Reporting(bt.Recorder):
        def call(self, L_, name, args):
            if name == "din_conv_wgrad_group":
                n, items = args[0], args[1]
                rc = lib.din_conv_wgrad_group_kernel_names(n, items, buf, len(buf))
                d = items[0].desc
                label = f"{head[0]} {n} items, the first {d.h}x{d.w} c{d.cin}>{d.cout} k{d.kh}x{d.kw} key={lib.din_conv_wgrad_group_key(C.byref(d))}"
                entry = "wgrad_group"
            elif name == "din_conv1x1_wgrad_multi":
                nsrc, srcs, dtype, pixels, cin = args[:5]
                rc = lib.din_conv1x1_wgrad_multi_kernel_names(nsrc, srcs, dtype, pixels, cin, buf, len(buf))
                label = f"{head[0]} {pixels} pixels c{cin}>{'+'.join(str(srcs[j].cout) for j in range(nsrc))}"
                entry = "wgrad_multi"
            else:
                return
            assert 0 < rc <= len(buf), f"{name}: the reporter answered {rc} for a call the reverse pass makes"
            for kernel in buf.value.decode().split("\n")[:-1]:
                found.setdefault((entry, kernel), label)

    saved = bt.Recorder
    bt.Recorder = Reporting
    try:
        for backbone in ("inv3", "vgg16"):
            for dtn in ("bf16", "fp32", "fp32_bf16x3"):
                for nb, h, w in GEOMETRIES:
                    g, dt, params = bt.backbone(backbone, dtn, h, w)
                    head[0] = f"{backbone} {dtn} nb{nb} {h}x{w}"
                    _lines, outcome = bt.trace(g, params, dt, nb, {}, u8=dtn == "bf16")
                    assert outcome == "ok", f"{head[0]}: {outcome}"
    finally:
        bt.Recorder = saved
    return found


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--summary", action="store_true", help="no-option decisions at 96 frames and at the small geometry, one line per descriptor")
    ap.add_argument("--names", action="store_true", help="every distinct kernel instantiation of the no-option decisions, with one launch that reaches it")
    ap.add_argument("--wgrad", action="store_true", help="the weight-gradient part only (with --names: the weight-gradient kernel names)")
    ap.add_argument("--multi", action="store_true", help="with --names: the kernels of din_conv_fwd2 / din_conv1x1_dgrad_multi / din_conv_dgrad_x")
    ap.add_argument("--wgrad-multi", action="store_true", help="with --names: the kernels of din_conv_wgrad_group / din_conv1x1_wgrad_multi")
    args = ap.parse_args()
    if (args.multi or args.wgrad_multi) and not args.names:
        ap.error("--multi / --wgrad-multi select which names --names prints: use --names --multi, --names --wgrad-multi")
    from din_amd import _lib as L, nhwc
    lib = L.load()
    for name, _ in OPTIONS + WGRAD_OPTIONS:
        L.set_option(name, None)
    if args.names and args.wgrad_multi:
        for (entry, name), label in sorted(wgrad_multi_names_table(L, lib).items()):
            print(f"{entry} {name}  <-  {label}")
        return
    if args.names and args.multi:
        for (entry, name), label in sorted(multi_names_table(L, lib, nhwc).items()):
            print(f"{entry} {name}  <-  {label}")
        return
    cases, groups = [], []
    for backbone in ("inv3", "vgg16"):
        for dt, dtn in ((L.DIN_BF16, "bf16"), (L.DIN_F32, "fp32")):
            for nb, h, w in GEOMETRIES:
                sib = []
                descs = descriptors(L, nhwc, backbone, nb, h, w, dt, sib)
                label = lambda d: (f"{backbone} {dtn} nb{nb} {d.h}x{d.w} c{d.cin}>{d.cout} k{d.kh}x{d.kw} s{d.sh} p{d.ph},{d.pw} "
                                   f"ld{d.ldi}+{d.cioff}>{d.ldo}+{d.cooff}{' u8' if d.in_u8 else ''}")
                groups += [(f"{label(m[0])} multi{len(m)}", m) for m in sib]
                seen = set()
                for d in descs + misaligned(L, nhwc, descs):
                    key = tuple(getattr(d, f) for f in FIELDS)
                    if key not in seen:
                        seen.add(key)
                        cases.append((label(d), d))
    if args.names and args.wgrad:
        for name, label in sorted(wgrad_names_table(lib, cases).items()):
            print(f"{name}  <-  {label}")
        return
    if args.names:
        for name, label in sorted(names_table(L, lib, cases).items()):
            print(f"{name}  <-  {label}")
        return
    if args.summary:
        for label, d in cases:
            if d.nb in (96, 6):
                f, g = report(lib, d, 0).split(), report(lib, d, 1).split()
                print(f"{label}  ->  {' '.join(f[:3])} / {' '.join(g[:3])}  {f[3]} {f[4]}")
        return
    for opt, val in [(None, None)] + [(o, v) for o, vals in WGRAD_OPTIONS for v in vals]:
        if opt:
            L.set_option(opt, val)
        try:
            tag = opt + '=' + val if opt else '-'
            for label, d in cases:
                print(f"{label} which=2 {tag}  ->  {report_wgrad(lib, d)}")
            for label, members in groups:
                print(f"{label} {tag}  ->  {report_multi(L, lib, members)}")
        finally:
            if opt:
                L.set_option(opt, None)
    if args.wgrad:
        return
    for opt, val in [(None, None)] + [(o, v) for o, vals in OPTIONS for v in vals]:
        if opt:
            L.set_option(opt, val)
        try:
            for label, d in cases:
                for which in (0, 1):
                    print(f"{label} which={which} {opt + '=' + val if opt else '-'}  ->  {report(lib, d, which)}")
        finally:
            if opt:
                L.set_option(opt, None)


if __name__ == "__main__":
    main()
