"""conv_halo_rf_kernel without a GPU: what din_conv_rf_eligible answers for the backbone's layers and for the shapes the kernel does not
serve, the two options that switch it off, the reporter against the launcher's table, and the built code objects' scratch and registers."""
import ctypes as C
import glob
import os
import re

import pytest

from tests import test_gpu_conv_fwd_dgrad as CF
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "din-group-activity-recognition-benchmark_amd", "csrc")
SEVEN = ["Mixed_5b.branch3x3dbl_2", "Mixed_5b.branch3x3dbl_3", "Mixed_5c.branch3x3dbl_2", "Mixed_5c.branch3x3dbl_3",
         "Mixed_5d.branch3x3dbl_2", "Mixed_5d.branch3x3dbl_3", "Mixed_6a.branch3x3dbl_2"]


def _backbone_descs(nb):
    """{op name: (descriptor, data-gradient flags, ldm, moff)} of every conv of the Inception-v3 trunk at the benchmark's 720 x 1280 frames,
    bf16: the launches graph_forward / the reverse pass make for it"""
    from din_amd import _lib as L
    from din_amd import nhwc
    from din_amd.backbone import backbone as B
    g = B.MyInception_v3(compute_dtype="bf16").build_graph(720, 1280, L.DIN_BF16)
    out = {}
    for op in g.ops:
        if op.kind != "conv" or op.src.tid == g.input_tid:
            continue
        ts = g.tensors[op.src.tid]
        masked = ts.relu_masked
        out[op.name] = (nhwc._conv_desc(g, op, nb, L.DIN_BF16), L.CONV_MASK if masked else 0, ts.c if masked else 0, op.src.coff if masked else 0)
    return out, g


def _eligible(lib, d, which, flags=0, ldm=0, moff=0):
    return lib.din_conv_rf_eligible(C.byref(d), which, flags, ldm, moff)


def test_eligibility_of_the_backbone_layers_and_the_options():
    lib, L = CF._library()
    descs, g = _backbone_descs(96)
    assert set(SEVEN) <= set(descs)
    fwd_flags = L.CONV_BIAS | L.CONV_RELU
    try:
        for forced in (None, "2"):
            L.set_option("DIN_CONV_HALO_RF", forced)
            yes = {n for n, (d, fl, ldm, moff) in descs.items() if _eligible(lib, d, 0, fwd_flags)}
            yes_dg = {n for n, (d, fl, ldm, moff) in descs.items() if _eligible(lib, d, 1, fl, ldm, moff)}
            # the planner's rule and every-eligible-shape agree at 96 frames: the seven layers, both directions, and nothing else of this trunk
            assert yes == set(SEVEN) and yes_dg == set(SEVEN), (forced, sorted(yes), sorted(yes_dg))
        # the planner's rule (profiles/halo_rf_layers.txt): at 12 frames the 64 -> 96 forward stays on the old kernel, the other launches move;
        # accumulating launches stay on the old kernels at any size; forced, all of them are served
        small, _ = _backbone_descs(12)
        for forced in (None, "2"):
            L.set_option("DIN_CONV_HALO_RF", forced)
            d2, fl2, ldm2, moff2 = small["Mixed_5b.branch3x3dbl_2"]
            d3, fl3, ldm3, moff3 = small["Mixed_5b.branch3x3dbl_3"]
            assert bool(_eligible(lib, d2, 0, fwd_flags)) == bool(forced)
            assert _eligible(lib, d2, 1, fl2, ldm2, moff2) and _eligible(lib, d3, 0, fwd_flags) and _eligible(lib, d3, 1, fl3, ldm3, moff3)
            big = descs["Mixed_5b.branch3x3dbl_3"]
            assert bool(_eligible(lib, big[0], 1, big[1] | L.CONV_ACCUM, big[2], big[3])) == bool(forced)
        L.set_option("DIN_CONV_HALO_RF", "2")
        # Conv2d_4a (80 -> 192), the 5x5, 1x7 and 7x1 layers, stride 2: no
        for name in ("Conv2d_4a_3x3", "Mixed_5b.branch5x5_2", "Mixed_6b.branch7x7_2", "Mixed_6b.branch7x7_3", "Mixed_6a.branch3x3", "Mixed_6a.branch3x3dbl_3"):
            d, fl, ldm, moff = descs[name]
            assert not _eligible(lib, d, 0, fwd_flags) and not _eligible(lib, d, 1, fl, ldm, moff), name
        d, fl, ldm, moff = descs["Mixed_5b.branch3x3dbl_3"]
        assert fl == L.CONV_MASK and _eligible(lib, d, 0, fwd_flags) and _eligible(lib, d, 1, fl, ldm, moff) and _eligible(lib, d, 1, fl | L.CONV_ACCUM, ldm, moff)
        # fp32 and the three-part bf16 mode: no
        for dt in (L.DIN_F32, L.DIN_F32_BF16X3):
            d32 = L.ConvDesc.from_buffer_copy(d)
            d32.dtype = dt
            assert not _eligible(lib, d32, 0) and not _eligible(lib, d32, 1)
        # flags of the other direction, a mask view at multiples of 4 only, a mask view that does not cover the produced channels: no
        assert not _eligible(lib, d, 0, L.CONV_MASK) and not _eligible(lib, d, 1, L.CONV_BIAS)
        assert not _eligible(lib, d, 1, L.CONV_MASK, ldm + 4, moff) and not _eligible(lib, d, 1, L.CONV_MASK, ldm, moff + 4)
        assert not _eligible(lib, d, 1, L.CONV_MASK, d.cin - 8, 0)
        # the entries and the reporter refuse what is not eligible: DIN_E_ARG, never another kernel
        buf = C.create_string_buffer(64)
        assert lib.din_conv_rf_kernel_names(C.byref(d), 1, L.CONV_MASK, ldm + 4, moff, buf, len(buf)) == -1
        assert lib.din_conv_rf_dgrad(C.byref(d), C.c_void_p(16), C.c_void_p(16), C.c_void_p(16), C.c_void_p(16), ldm + 4, moff, L.CONV_MASK, None, 0, None) == -1
        # both switches turn it off
        for name, value in (("DIN_CONV_HALO_RF", "0"), ("DIN_CONV_HALO", "0")):
            L.set_option("DIN_CONV_HALO_RF", "2")
            L.set_option(name, value)
            assert not any(_eligible(lib, dd, 0, fwd_flags) or _eligible(lib, dd, 1, fl2, l2, m2) for dd, fl2, l2, m2 in descs.values()), name
            L.set_option(name, None)
    finally:
        L.set_option("DIN_CONV_HALO_RF", None)
        L.set_option("DIN_CONV_HALO", None)


def test_the_plan_asks_once_per_op_and_the_old_entry_points_never_answer_the_new_kernel():
    """plan_backward's rf_dgrad equals the library's answers; din_conv_kernel_names (the reporter of din_conv_fwd / din_conv_dgrad) never
    names the new kernel: it is not reachable through those entry points"""
    lib, L = CF._library()
    from din_amd import nhwc
    descs, g = _backbone_descs(96)
    try:
        L.set_option("DIN_CONV_HALO_RF", "2")
        plan = nhwc.plan_backward(g, 96, L.DIN_BF16, False, False, False)
        assert {g.ops[oi].name for oi in plan.rf_dgrad} == set(SEVEN)
        for name in SEVEN:
            d, fl, ldm, moff = descs[name]
            for which, flags, m in ((0, 0, (0, 0)), (1, fl, (ldm, moff))):
                buf = C.create_string_buffer(4096)
                assert lib.din_conv_kernel_names(C.byref(d), which, flags, *m, buf, len(buf)) > 0
                assert "conv_halo_rf_kernel" not in buf.value.decode()
        L.set_option("DIN_CONV_HALO_RF", "0")
        assert not nhwc.plan_backward(g, 96, L.DIN_BF16, False, False, False).rf_dgrad
    finally:
        L.set_option("DIN_CONV_HALO_RF", None)


def _table_rows():
    text = open(os.path.join(CSRC, "conv_halo_rf.hip")).read()
    body = text[text.index("#define DIN_CONV_HALO_RF_TABLE(X)"):]
    body = body[:body.index("\n\n")]
    rows = re.findall(r"X\((\d+), (\d+), (true|false)\)", body)
    return {f"conv_halo_rf_kernel<{ti}, {nks}, {dg}>" for ti, nks, dg in rows}


def test_every_name_the_reporter_answers_is_a_row_of_the_launch_table():
    lib, L = CF._library()
    rows = _table_rows()
    assert len(rows) == 8
    answered = set()
    try:
        L.set_option("DIN_CONV_HALO_RF", "2")
        for which in (0, 1):
            for cin in range(40, 97, 8):
                for cout in range(40, 97, 8):
                    d = L.ConvDesc()
                    d.nb, d.h, d.w, d.cin, d.oh, d.ow, d.cout = 2, 19, 45, cin, 19, 45, cout
                    d.kh = d.kw = 3
                    d.sh = d.sw = d.ph = d.pw = d.dh = d.dw = 1
                    d.ldi, d.cioff, d.ldo, d.cooff, d.dtype = cin, 0, cout, 0, L.DIN_BF16
                    assert _eligible(lib, d, which)
                    buf = C.create_string_buffer(64)
                    assert lib.din_conv_rf_kernel_names(C.byref(d), which, 0, 0, 0, buf, len(buf)) > 0
                    answered.add(buf.value.decode().strip())
    finally:
        L.set_option("DIN_CONV_HALO_RF", None)
    assert answered == rows, (sorted(answered), sorted(rows))


def test_code_objects_hold_the_filters_without_scratch_at_one_wave_per_simd():
    """csrc/Makefile leaves the compiler's per-kernel resource remarks in csrc/conv_halo_rf.res, read the way the occupancy test of
    tests/test_host_cpu.py reads them.  The design: one wave per SIMD (four waves per workgroup, one workgroup per CU) holding up to 324
    filter registers -- so every instantiation may use the whole 512-register file of a wave, and NOT ONE spill or byte of scratch: a
    fragment reloaded inside the tile loop would sit in the hand-counted vmcnt of the LDS-DMA transfers.  The 96 -> 96 forms must actually
    need more than 256 registers (324 filter + 96 accumulator): at <= 256 the allocator would have dropped the filters somewhere else."""
    files = glob.glob(os.path.join(CSRC, "conv_halo_rf.res"))
    if not files:
        pytest.skip("no csrc/conv_halo_rf.res (library built before the Makefile wrote them): run __graft_entry__.build() after `make clean`")
    usage = {}
    for blk in re.split(r"remark: Function Name: ", open(files[0]).read())[1:]:
        name = blk.split()[0]
        m = re.search(r"conv_halo_rf_kernelILi(\d)ELi(\d)ELb([01])E", name)
        if not m:
            continue
        v, a = re.search(r" VGPRs: (\d+)", blk), re.search(r"AGPRs: (\d+)", blk)
        sp, sc = re.search(r"VGPRs Spill: (\d+)", blk), re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk)
        occ = re.search(r"Occupancy \[waves/SIMD\]: (\d+)", blk)
        usage[tuple(int(x) for x in m.groups())] = (int(v.group(1)) + int(a.group(1)), int(sp.group(1)) + int(sc.group(1)), int(occ.group(1)))
    assert len(usage) == 8, sorted(usage)
    for (ti, nks, dg), (regs, spill, occ) in usage.items():
        assert spill == 0, f"conv_halo_rf_kernel<{ti}, {nks}, {dg}>: {spill} bytes / registers of scratch"
        assert regs <= 512 and occ == 1, f"conv_halo_rf_kernel<{ti}, {nks}, {dg}>: {regs} registers, {occ} waves per SIMD (the design: one)"
        assert regs >= 36 * ti * nks + 32 * ti, f"conv_halo_rf_kernel<{ti}, {nks}, {dg}>: {regs} registers cannot hold {36 * ti * nks} filter + {32 * ti} accumulator registers"
