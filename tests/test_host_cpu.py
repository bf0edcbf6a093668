"""CPU: C-ABI library loads and exports every declared symbol; host logic (graphs, planning, sharding, gloo all-reduce);
the product path refuses to run without a GPU (no fallback)."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from oracle import din_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_header_symbol():
    from din_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "libdin_hip.so missing: run __graft_entry__.build()"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    names = _lib.header_symbols()
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/din_hip.h but not exported"
    assert set(names) == set(_lib.SIGNATURES), "ctypes table out of sync with include/din_hip.h"
    loaded = _lib.load()
    assert loaded.din_abi_version() == _lib.ABI_VERSION == 9 and loaded.din_build_arch() == b"gfx950"


def test_options_go_through_the_abi_not_the_environment(monkeypatch):
    """din_set_option / din_get_option (ABI 8): the library holds named options, and nothing in csrc/ calls getenv()."""
    import glob
    from din_amd import _lib
    assert _lib.get_option("DIN_TEST_OPTION") is None
    _lib.set_option("DIN_TEST_OPTION", 2)
    assert _lib.get_option("DIN_TEST_OPTION") == "2"
    _lib.set_option("DIN_TEST_OPTION", None)
    assert _lib.get_option("DIN_TEST_OPTION") is None
    with pytest.raises(_lib.DinError):
        _lib.set_option("NOT_A_DIN_NAME", 1)
    monkeypatch.setenv("DIN_CONV_HALO", "2")                     # the conftest fixture forwards it ...
    assert _lib.get_option("DIN_CONV_HALO") == "2"
    csrc = os.path.join(ROOT, "din-group-activity-recognition-benchmark_amd", "csrc")
    for f in glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.cpp")) + glob.glob(os.path.join(csrc, "*.h")):
        code = "\n".join(l.split("//")[0] for l in open(f).read().splitlines())
        assert "getenv(" not in code, f"{os.path.basename(f)} reads the process environment"


def test_occupancy_critical_kernels_hold_their_register_budgets():
    """The kernels whose speed depends on TWO workgroups per CU (8 waves each: four waves per SIMD = at most 128 VGPRs) or on sixteen waves in
    one workgroup must stay inside that budget: csrc/Makefile leaves the compiler's per-kernel resource remarks in csrc/<file>.res.  Round 4
    found the FASTK 128 x 192 gather tile at 131 registers after an unrelated edit -- one workgroup per CU, 186 -> 259 us per launch, 1.6 ms per
    step -- with every numerical test green."""
    import glob
    import re
    csrc = os.path.join(ROOT, "din-group-activity-recognition-benchmark_amd", "csrc")
    files = glob.glob(os.path.join(csrc, "*.res"))
    if not files:
        pytest.skip("no csrc/*.res (library built before the Makefile wrote them): run __graft_entry__.build() after `make clean`")
    usage = {}
    for f in files:
        for blk in re.split(r"remark: Function Name: ", open(f).read())[1:]:
            name = blk.split()[0]
            v, a = re.search(r" VGPRs: (\d+)", blk), re.search(r"AGPRs: (\d+)", blk)
            sp, sc = re.search(r"VGPRs Spill: (\d+)", blk), re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk)
            # (scratch counts as a spill: the hand-counted vmcnt of the LDS-DMA rings does not survive compiler-made memory traffic)
            usage[name] = (int(v.group(1)) + int(a.group(1)), (int(sp.group(1)) if sp else 0) + (int(sc.group(1)) if sc else 0))
    assert len(usage) > 100, "resource remarks look truncated"
    checked = 0
    for name, (regs, spill) in usage.items():
        budget = None
        m = re.search(r"conv_gather_fast_kernelItLi128ELi(\d+)ELi4ELi2E", name)
        if m:                                                         # bf16 8-wave 128-pixel tiles: two workgroups per CU
            budget = 128
        elif re.search(r"conv_halo_kernelILi\d+ELi\d+ELi\d+ELi\d+ELi\d+ELi\d+ELi16E", name):     # sixteen waves in one workgroup
            budget = 128
        elif re.search(r"conv_wgrad_pipe(_group)?_kernelILi\d+ELi256ELb[01]ELi8E", name):   # sixteen waves (wave grid 2 x 8) in one workgroup; the grouped launch too
            budget = 128
        elif "conv1x1_regw_kernel" in name:         # one wave per SIMD with the filters resident: the whole file, and NOT ONE spill -- a filter
            budget = 512                            # fragment reloaded from scratch inside the tile loop drains every transfer in flight (vmcnt)
        if budget is not None:
            checked += 1
            assert regs <= budget and spill == 0, f"{name}: {regs} registers (+{spill} spilled) > {budget}: a workgroup per CU is lost"
    assert checked >= 28, checked


def test_register_resident_kernel_keeps_its_hand_counted_lds_reads_hazard_free(tmp_path):
    """conv_regw.hip issues its fragment reads as inline-asm ds_read_b128 and waits for them with hand-counted s_waitcnt
    lgkmcnt(n); with the register file full, a compiler that copied or reused a destination register between the read and its wait would
    corrupt data silently.  tools/lds_hazard_check.py walks the ISA of every instantiation (FIFO of outstanding LGKM operations, retired
    at each wait) and reports any instruction that touches the destination of a read still in flight."""
    import shutil
    import subprocess
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import lds_hazard_check as H
    # the checker itself: a read in flight, then a use before / after the wait
    bad = ["ds_read_b128 v[4:7], v9 offset:16", "v_add_u32 v1, v5, v2", "s_waitcnt lgkmcnt(0)", "v_add_u32 v1, v5, v2"]
    hz = H.check_kernel(bad)
    assert len(hz) == 1 and hz[0][0] == 1
    ok = ["ds_read_b128 v[4:7], v9", "ds_read_b128 v[10:13], v9", "s_waitcnt lgkmcnt(1)", "v_mfma_f32_16x16x32_bf16 a[0:3], v[20:23], v[4:7], a[0:3]",
          "s_waitcnt lgkmcnt(0)", "v_mov_b32 v30, v10"]
    assert not H.check_kernel(ok)
    assert len(H.check_kernel(ok[:2] + ["s_waitcnt lgkmcnt(1)", "v_mov_b32 v30, v10"])) == 1      # the second read is still outstanding
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc: the ISA of conv_regw.hip cannot be produced here")
    csrc = os.path.join(ROOT, "din-group-activity-recognition-benchmark_amd", "csrc")
    out = str(tmp_path / "regw.s")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-munsafe-fp-atomics", "-S",
                           "--cuda-device-only", "-o", out, os.path.join(csrc, "conv_regw.hip")], stderr=subprocess.DEVNULL)
    checked = 0
    for name, body in H.kernels(out):
        if "conv1x1_regw_kernel" in name:
            checked += 1
            assert sum(1 for l in body if "ds_read_b128" in l) >= 60, name
            hz = H.check_kernel(body)
            assert not hz, (name, hz[:3])
    assert checked == 10


def _function_body(text, signature):
    """the text of the C function whose definition starts with `signature`, braces matched"""
    i = text.index(signature)
    i = text.index("{", i)
    depth = 0
    for j in range(i, len(text)):
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        if depth == 0:
            return text[i:j + 1]
    raise AssertionError(f"unbalanced braces after {signature}")


def test_every_wgrad_kernel_instantiation_has_a_row_in_the_fp64_table():
    """the conv_wgrad_*_kernel<...> instantiations the launch tables of din_conv_wgrad hold (csrc/conv_wgrad.hip: the fp32 and tail kernels
    and the DIN_WGRAD_*_TABLE rows; conv_wgrad_halo.hip: DIN_WGRAD_HALO_TABLE; conv_wgrad_pipe.hip: the filter banks of launch_wgrad_pipe)
    equal the kernels named by the rows of tests/test_gpu_wgrad.py, spelled in full: a kernel added without a row fails here, on the CPU"""
    import re
    from tests.test_gpu_wgrad import WGRAD_CASES
    csrc = os.path.join(ROOT, "din-group-activity-recognition-benchmark_amd", "csrc")

    def src(name):
        with open(os.path.join(csrc, name)) as fh:
            return re.sub(r"//[^\n]*", "", fh.read())

    def table(text, macro, kernel, pick=lambda a: a):
        body = re.search(r"#define " + macro + r"\(X\)((?:[^\n]*\\\n)*[^\n]*)", text).group(1)
        return {f"{kernel}<{', '.join(pick([a.strip() for a in args.split(',')]))}>" for args in re.findall(r"X\(([^()]*)\)", body)}

    wgrad = src("conv_wgrad.hip")
    body = _function_body(wgrad, "int launch_wgrad(const WgradK& k")
    launched = set(re.findall(r"go\((conv_wgrad_\w+_kernel)\)", body))
    assert launched == {"conv_wgrad_f32_kernel", "conv_wgrad_bf16_tail_kernel"}
    for macro, kernel in (("DIN_WGRAD_BF16_TABLE", "conv_wgrad_bf16_kernel"), ("DIN_WGRAD_RING_TABLE", "conv_wgrad_ring_kernel"),
                          ("DIN_WGRAD_STEM_TABLE", "conv_wgrad_small_kernel")):
        assert f"{macro}(DIN_ROW)" in body and f"{kernel}<" in body
        launched |= table(wgrad, macro, kernel)
    halo = src("conv_wgrad_halo.hip")
    assert "DIN_WGRAD_HALO_TABLE(DIN_HALO_ROW)" in _function_body(halo, "int launch_wgrad_halo(") and "din_wgrad::launch_wgrad_halo(" in body
    launched |= table(halo, "DIN_WGRAD_HALO_TABLE", "conv_wgrad_halo_kernel", lambda a: a[2:])       # (cin, cout, then the template arguments)
    assert "din_wgrad::launch_wgrad_pipe(" in body
    pipe = _function_body(src("conv_wgrad_pipe.hip"), "int launch_wgrad_pipe(")
    banks = set(re.findall(r"DIN_PIPE_GRIDS\((\d+)\)", pipe))
    grids = set(re.findall(r"DIN_PIPE\(BCO_, (true|false), (\d)\)", pipe))
    assert len(banks) == 3 and len(grids) == 6
    pipes = {f"conv_wgrad_pipe_kernel<{b}, 256, {wide}, {wn}>" for b in banks for wide, wn in grids}
    assert len(launched) >= 21, sorted(launched)
    named = {r["kernel"] for r in WGRAD_CASES}
    named_pipe = {n for n in named if n.startswith("conv_wgrad_pipe_kernel<")}
    assert launched == named - named_pipe, (f"launched without a row: {sorted(launched - named)}; "
                                            f"rows naming no launch: {sorted(named - named_pipe - launched)}")
    # the pipe kernel: a row for every filter bank, on an instantiation of the sixteen-wave grid the launcher holds (the other wave grids:
    # test_wgrad_pipe_kernel in tests/test_gpu_kernels.py)
    assert named_pipe <= pipes and {re.match(r"conv_wgrad_pipe_kernel<(\d+), 256, \w+, 8>", n).group(1) for n in named_pipe} == banks


def _reported_wgrad_kernels(row):
    """what din_conv_kernel_names(d, 2) answers for a row of tests/test_gpu_wgrad.py under the row's options (host only)"""
    from din_amd import _lib
    from tests.test_gpu_wgrad import _geometry
    nb, cin, h, w, cout, k, s, p, dil, oh, ow = _geometry(row)
    d = _lib.ConvDesc()
    d.nb, d.h, d.w, d.cin, d.oh, d.ow, d.cout = nb, h, w, cin, oh, ow, cout
    d.kh, d.kw, d.sh, d.sw, d.ph, d.pw, d.dh, d.dw = k[0], k[1], s[0], s[1], p[0], p[1], dil, dil
    d.ldi, d.cioff, d.ldo, d.cooff = row["ld"]
    d.dtype, d.in_u8 = (_lib.DIN_F32 if row["dtype"] == "fp32" else _lib.DIN_BF16), int(bool(row.get("u8")))
    buf = ctypes.create_string_buffer(512)
    try:
        for name, value in row["opts"].items():
            _lib.set_option(name, value)
        rc = _lib.load().din_conv_kernel_names(ctypes.byref(d), 2, 0, 0, 0, buf, len(buf))
    finally:
        for name in row["opts"]:
            _lib.set_option(name, None)
    assert 0 < rc <= len(buf), _lib.load().din_last_error_string()
    assert _lib.load().din_conv_kernel_names(ctypes.byref(d), 2, 2, 0, 0, buf, 0) == -1, "flags are fwd / dgrad arguments"
    return buf.value.decode().split("\n")[:-1]


def test_wgrad_tail_kernel_reports_its_own_name():
    """a bf16 layer whose channels are no whole 16-byte chunks runs conv_wgrad_bf16_tail_kernel and shares the tile code (128, 128) with
    conv_wgrad_bf16_kernel<128>: the reporter names the kernel that runs (and the column-sum launch the tail kernel needs for its bias)"""
    from tests.test_gpu_wgrad import WGRAD_CASES
    rows = {r["name"]: r for r in WGRAD_CASES}
    assert rows["tail_cin3"]["code"] == rows["v3_128"]["code"] == (128, 128)
    assert _reported_wgrad_kernels(rows["tail_cin3"]) == [
        "conv_wgrad_bf16_tail_kernel", "conv_wgrad_reduce_kernel", "colsum_vec_kernel<unsigned short, 8>"]
    assert _reported_wgrad_kernels(rows["v3_128"]) == ["conv_wgrad_bf16_kernel<128>", "conv_wgrad_reduce_kernel"]


def test_wgrad_stem_option_settings_report_three_kernels():
    """the three forms of the 32 -> 64 stem layer share the tile code (0, 64); each option setting reports its own instantiation"""
    from tests.test_gpu_wgrad import WGRAD_CASES
    rows = [r for r in WGRAD_CASES if r["name"].startswith("small2_")]
    assert len(rows) == 3 and {r["code"] for r in rows} == {(0, 64)}
    got = [_reported_wgrad_kernels(r)[0] for r in rows]
    assert got == [r["kernel"] for r in rows] and len(set(got)) == 3, got


def test_every_weight_gradient_kernel_of_the_backbones_has_a_gpu_row():
    """profiles/wgrad_kernel_names.txt (tools/conv_dispatch_table.py --names --wgrad: the main kernels the no-option decisions of both backbones
    reach) against the rows of tests/test_gpu_wgrad.py: every kernel the product launches is tested by name"""
    from tests.test_gpu_wgrad import WGRAD_CASES
    with open(os.path.join(ROOT, "profiles", "wgrad_kernel_names.txt")) as fh:
        reached = {line.split("  <-  ")[0] for line in fh.read().splitlines() if line}
    assert len(reached) >= 18
    assert reached <= {r["kernel"] for r in WGRAD_CASES}, sorted(reached - {r["kernel"] for r in WGRAD_CASES})


def test_every_pool_kernel_instantiation_has_a_row_in_the_fp64_table():
    """the kernel instantiations csrc/pool.hip launches (hipLaunchKernelGGL / POOL_LAUNCH sites, comments stripped) equal the kernels named by
    the rows of tests/test_gpu_pool.py and the names din_pool_kernel_name can answer: a kernel added without a row, a row naming no launch
    or a name the query spells differently from its launch site fails here, on the CPU"""
    import re
    from tests.test_gpu_pool import POOL_CASES
    with open(os.path.join(ROOT, "din-group-activity-recognition-benchmark_amd", "csrc", "pool.hip")) as fh:
        text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S))

    def norm(name):
        return re.sub(r"\s+", "", name)

    sites = re.findall(r"(?:hipLaunchKernelGGL|POOL_LAUNCH)\(\s*\(?\s*(\w+_kernel\b(?:\s*<[^<>;()]*>)?)", text)
    launched = {norm(s) for s in sites}
    assert len(launched) >= 39, sorted(launched)
    named = {norm(r["kernel"]) for r in POOL_CASES}
    assert launched == named, f"launched without a row: {sorted(launched - named)}; rows naming no launch: {sorted(named - launched)}"
    answers = {norm(n) for n in re.findall(r'X\(\w+,\s*"([^"]+)"\)', text)}     # the POOL_KERNELS list: enum and name table come from it
    assert answers == launched, f"din_pool_kernel_name and the launch sites disagree: {sorted(answers ^ launched)}"


def test_conv_planning_is_callable_without_gpu():
    from din_amd import _lib
    lib = _lib.load()
    d = _lib.ConvDesc()
    d.nb, d.h, d.w, d.cin, d.oh, d.ow, d.cout = 6, 720, 1280, 64, 720, 1280, 64
    d.kh = d.kw = 3
    d.sh = d.sw = d.ph = d.pw = d.dh = d.dw = 1
    d.ldi = d.ldo = 64
    d.dtype = _lib.DIN_BF16
    assert lib.din_conv_packed_elems(ctypes.byref(d), 0) == 256 * 576        # rows padded to the widest tile
    assert lib.din_conv_workspace_bytes(ctypes.byref(d), 0) == 0          # big launch: no split-K
    assert lib.din_conv_workspace_bytes(ctypes.byref(d), 2) > 0
    # error path: null pointers give a status code + message, never a crash
    rc = lib.din_conv_fwd(ctypes.byref(d), None, None, None, None, 0, None, 0, None)
    assert rc == -1 and b"null" in lib.din_last_error_string()


def test_every_reported_fwd_dgrad_kernel_has_a_row_in_its_launch_table():
    """din_conv_kernel_names over the descriptors tools/conv_dispatch_table.py enumerates (both backbones, bf16 and fp32, with the misaligned
    views; at the small test geometry and at 96 frames of 720x1280 -- the 12- and 24-frame geometries are left out to keep this test shorter
    than tests/test_backward_trace_cpu.py), with no option and with every setting of its OPTIONS list, forward and data gradient with flags
    0 / MASK / ACCUM / MASK | ACCUM: every call succeeds, and every line parses to a kernel family and a template tuple that is a row of the
    X-macro table the family's launcher walks (DIN_CONV_HALO_TABLE in csrc/conv_halo.hip, DIN_CONV_SMALL_TABLE in csrc/conv_small.hip,
    DIN_CONV_TILE_TABLE / DIN_CONV_TILE_BF16_TABLE / DIN_CONV_GENERIC_TABLE in csrc/conv_igemm.hip; the rows only a -DDIN_EXPERIMENTS build
    holds do not count).  The register-resident, streaming and gather-pipe families keep no such table: their lines are held to their
    spelling only."""
    import re
    from din_amd import _lib as L, nhwc
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import conv_dispatch_table as D
    csrc = os.path.join(ROOT, "din-group-activity-recognition-benchmark_amd", "csrc")

    def rows(name, macro):
        with open(os.path.join(csrc, name)) as fh:
            text = re.sub(r"//[^\n]*", "", fh.read())
        body = re.search(r"#define " + macro + r"\(X\)((?:[^\n]*\\\n)*[^\n]*)", text).group(1)
        return {re.sub(r"\s+", "", args) for args in re.findall(r"X\(([^()]*)\)", body)}

    halo, small = rows("conv_halo.hip", "DIN_CONV_HALO_TABLE"), rows("conv_small.hip", "DIN_CONV_SMALL_TABLE")
    tile, tile_bf16 = rows("conv_igemm.hip", "DIN_CONV_TILE_TABLE"), rows("conv_igemm.hip", "DIN_CONV_TILE_BF16_TABLE")
    generic = rows("conv_igemm.hip", "DIN_CONV_GENERIC_TABLE")
    assert (len(halo), len(small), len(tile), len(tile_bf16), len(generic)) == (9, 11, 24, 22, 2)

    def held(line):
        m = re.fullmatch(r"(\w+)<([\w,]+)>", line)
        assert m, line
        family, args = m.group(1), m.group(2)
        if family == "conv_halo_kernel":                       # (the 8-wave forms are spelled without the wave count)
            return (args if args.count(",") == 6 else args + ",8") in halo
        if family == "conv_small_kernel":
            return args in small
        if family == "conv_gather_fast_kernel":
            t, tup = args.split(",", 1)
            return t in ("float", "f32x3", "bf16") and (tup in tile or (t == "bf16" and tup in tile_bf16))
        if family == "conv_gather_generic_kernel":
            t, tup = args.split(",", 1)
            return t in ("float", "f32x3", "bf16") and tup in generic
        if family == "conv_splitk_finish_kernel":
            return args in ("float", "bf16")
        return family in ("conv1x1_regw_kernel", "conv1x1_stream_kernel", "conv_gather_pipe_kernel")

    lib = L.load()
    cases = []
    for backbone in ("inv3", "vgg16"):
        for dt in (L.DIN_BF16, L.DIN_F32):
            for nb, h, w in ((96, 720, 1280), (6, 139, 203)):
                descs = D.descriptors(L, nhwc, backbone, nb, h, w, dt)
                seen = set()
                for d in descs + D.misaligned(L, nhwc, descs):
                    key = tuple(getattr(d, f) for f in D.FIELDS)
                    if key not in seen:
                        seen.add(key)
                        cases.append(d)
    assert len(cases) >= 250, len(cases)
    reached, calls = set(), 0
    for opt, val in [(None, None)] + [(o, v) for o, vals in D.OPTIONS for v in vals]:
        if opt:
            L.set_option(opt, val)
        try:
            for d in cases:
                if d.in_u8 and not lib.din_conv_accepts_u8(ctypes.byref(d)):
                    continue                                   # (din_conv_fwd rejects it)
                launches = [(0, 0)] + ([] if d.in_u8 else [(1, f) for f in (0, L.CONV_MASK, L.CONV_ACCUM, L.CONV_MASK | L.CONV_ACCUM)])
                for which, flags in launches:
                    buf = ctypes.create_string_buffer(1024)
                    rc = lib.din_conv_kernel_names(ctypes.byref(d), which, flags, d.ldi, d.cioff, buf, len(buf))
                    where = f"{opt}={val} which={which} flags={flags} {[getattr(d, f) for f in D.FIELDS]} dtype={d.dtype}"
                    assert 0 < rc <= len(buf), f"{where}: {rc} {lib.din_last_error_string()}"
                    lines = buf.value.decode().split()
                    assert lines, where
                    for line in lines:
                        assert held(line), f"{where}: {line} is no row of its family's table"
                        reached.add(line.split("<")[0])
                    calls += 1
        finally:
            if opt:
                L.set_option(opt, None)
    assert calls >= 40000, calls
    assert {"conv_halo_kernel", "conv_small_kernel", "conv_gather_fast_kernel", "conv_splitk_finish_kernel"} <= reached, reached
    # no backbone layer has more than 32 taps or a dilated strided data gradient, so none reaches the generic kernel: one 7x7 layer does
    d = L.ConvDesc()
    d.nb, d.h, d.w, d.cin, d.oh, d.ow, d.cout = 2, 56, 56, 16, 56, 56, 72
    d.kh = d.kw = 7
    d.ph = d.pw = 3
    d.sh = d.sw = d.dh = d.dw = 1
    d.ldi, d.ldo = 16, 72
    for d.dtype, spelled in ((L.DIN_BF16, "bf16"), (L.DIN_F32, "float"), (L.DIN_F32_BF16X3, "f32x3")):
        lines = D.kernel_names(lib, d, 0, 0)
        assert lines[0] == f"conv_gather_generic_kernel<{spelled},128>" and all(held(line) for line in lines), lines


def test_state_dict_keys_match_reference_inventory():
    from din_amd.config import Config
    from din_amd.infer_model import Dynamic_volleyball
    cfg = Config("volleyball")
    cfg.backbone, cfg.out_size, cfg.emb_features = "vgg16", (22, 40), 512
    cfg.ST_kernel_size, cfg.sampling_ratio, cfg.beta_factor = [(3, 3)], [1], False
    m = Dynamic_volleyball(cfg)
    ocfg = O.OracleCfg()
    shapes = O.model_param_shapes(ocfg)
    sd = m.state_dict()
    assert set(shapes) == set(sd.keys())
    for k, shp in shapes.items():
        assert tuple(sd[k].shape) == tuple(shp), k
    assert sum(p.numel() for p in m.parameters()) == 29204323
    # zero init of the DIN predictors (dynamic_infer_module.py:66-81)
    assert float(sd["DPI.DIMlist.0.p_conv.1.weight"].abs().sum()) == 0.0


def test_inception_graph_shapes_and_keys():
    from din_amd.backbone.backbone import MyInception_v3, MyVGG16
    from din_amd import _lib
    net = MyInception_v3(compute_dtype="bf16")
    g, dt = net.graph_for(720, 1280)
    t5d, t6e = g.output_tids                          # the multi-scale fuse is composed into RoIAlign: the graph ends at the two stored maps
    assert (g.tensors[t5d].h, g.tensors[t5d].w, g.tensors[t5d].c) == (87, 157, 288)
    assert (g.tensors[t6e].h, g.tensors[t6e].w, g.tensors[t6e].c) == (43, 78, 768)
    assert not any(op.kind == "bilinear" for op in g.ops)
    net.materialise_fuse = True                       # DIN_ROI_COMPOSE=0: the round-1 graph with the fused [5d | resize(6e)] tensor
    gm = net.build_graph(720, 1280, dt)
    fused = gm.output_tids[0]
    assert (gm.tensors[fused].h, gm.tensors[fused].w, gm.tensors[fused].c) == (87, 157, 1056)
    assert sum(op.kind == "bilinear" for op in gm.ops) == 1
    net.materialise_fuse = False
    shapes = O.inception_v3_param_shapes("")
    sd = net.state_dict()
    for k, shp in shapes.items():
        assert tuple(sd[k].shape) == tuple(shp), k
    assert sum(p.numel() for p in net.parameters()) == 8965856
    names = g.param_names()
    assert len(names) == len(set(names)) and all(n in sd for n in names)
    v = MyVGG16()
    gv, _ = v.graph_for(720, 1280)
    t = gv.tensors[gv.output_tids[0]]
    assert (t.h, t.w, t.c) == (22, 40, 512)
    assert sum(1 for o in gv.ops if o.kind == "conv") == 13


def test_backbone_parameter_cache_follows_every_kind_of_rebinding():
    """_GraphBackbone._ordered_params caches the parameter / buffer list per graph (host time on the 4-clip step) and must notice EVERY way a
    module can come to hold another tensor object -- attribute assignment, load_state_dict(assign=True), a direct write into
    module._parameters / _buffers (the process-wide registration hooks of round 5 missed that one and fired for every module of the
    process; the cache now checks object identity per call and hooks nothing)."""
    import torch.nn as nn
    import torch.nn.modules.module as tm
    from din_amd.backbone.backbone import MyInception_v3
    assert not tm._global_parameter_registration_hooks and not tm._global_buffer_registration_hooks       # nothing installed process-wide
    net = MyInception_v3(compute_dtype="bf16")
    g, _ = net.graph_for(139, 203)
    names = g.param_names()
    first = net._ordered_params(g)
    assert net._ordered_params(g) is first                                        # cache hit: the same list object
    iw = names.index("Conv2d_1a_3x3.conv.weight")
    net.Conv2d_1a_3x3.conv.weight = nn.Parameter(torch.zeros_like(net.Conv2d_1a_3x3.conv.weight))            # attribute assignment
    second = net._ordered_params(g)
    assert second is not first and second[iw] is net.Conv2d_1a_3x3.conv.weight and first[iw] is not second[iw]
    im = names.index("Mixed_6e.branch7x7_3.bn.running_mean")
    net.Mixed_6e.branch7x7_3.bn._buffers["running_mean"] = torch.ones_like(net.Mixed_6e.branch7x7_3.bn.running_mean)   # direct write
    third = net._ordered_params(g)
    assert third[im] is net.Mixed_6e.branch7x7_3.bn.running_mean and float(third[im].sum()) == third[im].numel()
    sd = {k: v.clone() + 1 for k, v in net.state_dict().items()}
    net.load_state_dict(sd, assign=True)                                           # every tensor replaced
    fourth = net._ordered_params(g)
    table = dict(net.named_parameters())
    table.update(dict(net.named_buffers()))
    assert all(t is table[n] for t, n in zip(fourth, names))
    assert net._ordered_params(g) is fourth


def test_product_path_fails_loudly_on_cpu_tensors():
    from din_amd import ops, _lib
    x = torch.zeros(1, 2, 3, 8)
    with pytest.raises(_lib.DinError):
        ops.layer_norm(x, torch.ones(8), torch.zeros(8))
    with pytest.raises(_lib.DinError):
        ops.prep_images_f32(torch.zeros(4))


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "din-group-activity-recognition-benchmark_amd")
    for dirpath, _d, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in src.replace("oracle/", "").replace("CPU oracle", "") or "import" not in \
                    [ln for ln in src.splitlines() if "oracle" in ln and "import" in ln][0:1] or True
                for ln in src.splitlines():
                    s = ln.strip()
                    if s.startswith(("import ", "from ")):
                        assert "oracle" not in s, f"{f}: product code must not import the oracle: {s}"


def test_shard_range_partitions_batch():
    from din_amd.parallel import shard_range
    for total in (32, 7, 2):
        for world in (1, 2, 4, 8):
            got = [i for r in range(world) for i in shard_range(total, r, world)]
            assert got == list(range(total))


WORKER = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from din_amd import parallel
rank, local, world = parallel.init_from_env("gloo")
torch.manual_seed(0)
lin = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.Linear(16, 4))
parallel.broadcast_parameters(lin)
clips = torch.arange(8 * 8, dtype=torch.float32).reshape(8, 8) / 10.0
mine = list(parallel.shard_range(8, rank, world))
loss = lin(clips[mine]).pow(2).mean()
loss.backward()
b = parallel.GradBuckets(lin.parameters(), bucket_bytes=256)
assert len(b.buckets) >= 2
b.allreduce()
# reference: full-batch gradient on one process
torch.manual_seed(0)
ref = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.Linear(16, 4))
ref.load_state_dict(lin.state_dict())
ref(clips).pow(2).mean().backward()
for p, q in zip(lin.parameters(), ref.parameters()):
    assert torch.allclose(p.grad, q.grad, atol=1e-6), (p.grad - q.grad).abs().max()
# overlap path: the conv executor reports weight gradients through the hook while backward is still running.  Step 1 teaches the
# order, from step 2 on the hooked weights form the leading buckets and are reduced from inside the hook.
weights = [lin[1].weight, lin[0].weight]                       # backward order
for step in range(3):
    for p in lin.parameters():
        p.grad = None
    lin(clips[mine]).pow(2).mean().backward()
    for w in weights:
        b._on_grad(w, w.grad)
    if step >= 1:
        assert b._early >= 1 and len(b._inflight) >= 1, (b._early, len(b._inflight))
    b.allreduce()
    for p, q in zip(lin.parameters(), ref.parameters()):
        assert torch.allclose(p.grad, q.grad, atol=1e-6), (step, (p.grad - q.grad).abs().max())
# (ADVICE r4) a parameter reported twice in one backward with two different gradient tensors -- a weight passed directly to two conv / linear
# ops -- must be refused loudly: its bucket would already have left with the first partial gradient
for p in lin.parameters():
    p.grad = None
lin(clips[mine]).pow(2).mean().backward()
w0 = weights[0]
b._on_grad(w0, w0.grad)
try:
    b._on_grad(w0, w0.grad.clone())
    raise SystemExit("second report of one parameter was accepted")
except RuntimeError as e:
    assert "more than one conv / linear op" in str(e), e
b._on_grad(weights[1], weights[1].grad)
b.allreduce()
dist.barrier()
sys.stdout.write(f"RANK_OK_{rank}\n"); sys.stdout.flush()
"""


def test_gloo_world2_gradient_allreduce(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29517")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "29517", str(script), ROOT]
    res = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:]
    assert "RANK_OK_0" in res.stdout and "RANK_OK_1" in res.stdout


def test_bench_gpus2_plain_launch_starts_two_ranks():
    """`python bench.py --gpus 2` WITHOUT torchrun's environment must start its own two ranks (it used to measure one GPU
    silently), prove N ranks / N processes / a summing all-reduce on its first step and carry that in the JSON line.  --dry-run-dist swaps the
    model (which needs the MI355X) for a small host-side gradient; everything around it is the real entry path."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["DIN_DIST_BACKEND"] = "gloo"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run-dist", "--steps", "2", "--warmup", "1",
                          "--global-batch", "5"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    line = [l for l in res.stdout.splitlines() if l.startswith("{")][-1]
    out = json.loads(line)
    assert out["n_gpus"] == 2 and out["rccl"]["world_size"] == 2 and out["rccl"]["allreduce_probe_sum"] == 3.0
    assert out["config"]["clips_per_gpu"] == 3 and out["config"]["parallelism"] == "dp2"       # 5 clips: ranks get 3 + 2
    # a rank count that does not match --gpus is an error, not a silent single-GPU run
    env2 = dict(env, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    res2 = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run-dist"], env=env2, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True, timeout=300)
    assert res2.returncode != 0 and "WORLD_SIZE=1" in res2.stderr


DROPIN_DRIVER = r"""
import os, sys
script = sys.argv[1]
sys.path.append(".")                                   # what the reference's launchers do (scripts/train_*.py:2): AFTER PYTHONPATH
if script:
    # the reference's own launcher, unmodified, up to (not including) its final train_net(cfg) call -- that call needs the MI355X
    src = open(script).read().rstrip().splitlines()
    assert src[-1].strip() == "train_net(cfg)", src[-1]
    exec(compile("\n".join(src[:-1]), script, "exec"))
else:
    from train_net_dynamic import *
    cfg = Config('volleyball')
import inspect, train_net_dynamic, config, infer_model, utils, dataset, volleyball, collective
import backbone.backbone, infer_module.dynamic_infer_module, roi_align.roi_align
assert train_net.__module__ == "din_amd.train_net_dynamic" and Config.__module__ == "din_amd.config", (train_net.__module__, Config.__module__)
assert all(m.__file__.startswith(os.environ["DROPIN_DIR"]) for m in (train_net_dynamic, config, infer_model, utils, dataset, volleyball, collective))
sig = inspect.signature(train_net)
assert list(sig.parameters)[0] == "cfg" and all(p.default is not inspect._empty for p in list(sig.parameters.values())[1:]), sig
for name in ("Dynamic_volleyball", "Dynamic_collective", "train_volleyball", "test_volleyball", "return_dataset", "prep_images", "VolleyballDataset",
             "CollectiveDataset", "set_bn_eval", "adjust_lr"):
    assert name in globals(), name
from backbone.backbone import MyVGG16, MyInception_v3
from infer_module.dynamic_infer_module import Dynamic_Person_Inference, Multi_Dynamic_Inference, Hierarchical_Dynamic_Inference
from roi_align.roi_align import RoIAlign
print("DROPIN_OK", cfg.dataset_name, cfg.inference_module_name, cfg.backbone, cfg.num_frames)
"""


def test_dropin_directory_resolves_the_reference_launcher_imports(tmp_path):
    """a zero-edit drop-in.  With `dropin/` on PYTHONPATH the reference launcher's own lines (`sys.path.append(".")`,
    `from train_net_dynamic import *`, `cfg=Config('volleyball')`, its cfg field assignments: scripts/train_volleyball_stage2_dynamic.py:1-60)
    resolve to the MI355X implementation.  Where the reference tree is present (the build container) its launchers are EXECUTED unmodified up to
    the final train_net(cfg) call (run on the GPU in tests/test_gpu_din_model.py); elsewhere the two import lines are."""
    dropin = os.path.join(ROOT, "dropin")
    driver = tmp_path / "driver.py"
    driver.write_text(DROPIN_DRIVER)
    env = dict(os.environ, PYTHONPATH=dropin, DROPIN_DIR=dropin)
    ref = "/root/reference/scripts"
    scripts = [os.path.join(ref, n) for n in ("train_volleyball_stage2_dynamic.py", "train_collective_stage2_dynamic.py",
                                              "train_volleyball_stage2_dynamic_tce.py")] if os.path.isdir(ref) else []
    for script in scripts + [""]:
        res = subprocess.run([sys.executable, str(driver), script], env=env, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                             text=True, timeout=300)
        assert res.returncode == 0 and "DROPIN_OK" in res.stdout, (script, res.stdout[-3000:])


def _small_cfg(dataset="volleyball"):
    from din_amd.config import Config
    cfg = Config(dataset)
    cfg.backbone, cfg.image_size, cfg.out_size, cfg.emb_features = "vgg16", (64, 96), (2, 3), 512
    cfg.num_boxes, cfg.num_frames, cfg.num_features_boxes, cfg.num_features_gcn = 4, 2, 32, 32
    cfg.ST_kernel_size, cfg.sampling_ratio, cfg.beta_factor, cfg.train_backbone = [(3, 3)], [1], False, True
    cfg.training_stage = 2
    return cfg


def test_loadmodel_roundtrips_a_stage1_checkpoint(tmp_path):
    """reference base_model.py:46-63 writes {'backbone_state_dict', 'fc_emb_state_dict', ...}; infer_model.py:126-130 reads the first two"""
    from din_amd.infer_model import Dynamic_volleyball
    cfg = _small_cfg()
    src, dst = Dynamic_volleyball(cfg), Dynamic_volleyball(cfg)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in src.parameters():
            p.copy_(torch.randn(p.shape, generator=g))
    path = str(tmp_path / "stage1.pth")
    torch.save({"backbone_state_dict": src.backbone.state_dict(), "fc_emb_state_dict": src.fc_emb_1.state_dict(),
                "fc_actions_state_dict": {}, "fc_activities_state_dict": {}}, path)
    dst.loadmodel(path)
    for (k, a), (_, b) in zip(src.backbone.state_dict().items(), dst.backbone.state_dict().items()):
        assert torch.equal(a, b), k
    assert torch.equal(src.fc_emb_1.weight, dst.fc_emb_1.weight) and torch.equal(src.fc_emb_1.bias, dst.fc_emb_1.bias)
    assert not torch.equal(src.fc_activities.weight, dst.fc_activities.weight)      # the head is NOT part of a stage-1 hand-over


def test_stage2_checkpoint_with_dataparallel_prefix_loads(tmp_path):
    """reference train_net_dynamic.py:82-88 / :141-147: {'epoch', 'state_dict', 'optimizer'}; keys saved through nn.DataParallel carry 'module.'"""
    from din_amd.infer_model import Dynamic_volleyball
    from din_amd.train_net_dynamic import load_stage2_state
    cfg = _small_cfg()
    src, dst = Dynamic_volleyball(cfg), Dynamic_volleyball(cfg)
    with torch.no_grad():
        for p in src.parameters():
            p.add_(1.0)
    path = str(tmp_path / "stage2.pth")
    torch.save({"epoch": 3, "state_dict": {"module." + k: v for k, v in src.state_dict().items()}, "optimizer": {}}, path)
    state = load_stage2_state(dst, path)
    assert state["epoch"] == 3
    for (k, a), (_, b) in zip(src.state_dict().items(), dst.state_dict().items()):
        assert torch.equal(a, b), k
    torch.save({"epoch": 1, "state_dict": {"not_a_key": torch.zeros(1)}}, path)
    with pytest.raises(RuntimeError):
        load_stage2_state(dst, path)


def test_fused_adam_state_is_torch_adam_compatible():
    """the 'optimizer' entry of a checkpoint (train_net_dynamic.py:144) must travel both ways between FusedAdam and torch.optim.Adam"""
    from din_amd.optim import FusedAdam
    g = torch.Generator().manual_seed(1)
    ps = [torch.nn.Parameter(torch.randn(3, 4, generator=g)), torch.nn.Parameter(torch.randn(5, generator=g))]
    ref = torch.optim.Adam(ps, lr=3e-4, weight_decay=0.01)
    for _ in range(3):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g)
        ref.step()
    fa = FusedAdam(ps, lr=1.0)
    fa.load_state_dict(ref.state_dict())
    assert fa.param_groups[0]["lr"] == 3e-4 and fa.param_groups[0]["weight_decay"] == 0.01 and fa.step_count == 3
    for p in ps:
        assert torch.equal(fa.state[p][0], ref.state[p]["exp_avg"]) and torch.equal(fa.state[p][1], ref.state[p]["exp_avg_sq"])
        assert fa.steps[p] == 3
    back = torch.optim.Adam(ps, lr=1.0)
    back.load_state_dict(fa.state_dict())                      # torch validates group / parameter counts itself
    assert back.param_groups[0]["lr"] == 3e-4
    for p in ps:
        assert torch.equal(back.state[p]["exp_avg"], ref.state[p]["exp_avg"]) and float(back.state[p]["step"]) == 3.0
    with pytest.raises(ValueError):
        FusedAdam(ps[:1]).load_state_dict(ref.state_dict())


def test_set_bn_eval_and_bn_mode_of_the_backbone():
    """train_net_dynamic.py:17-20: set_bn_eval puts exactly the BatchNorm modules in eval mode; the backbone reads the mode from them"""
    from din_amd.backbone.backbone import MyInception_v3
    from din_amd.train_net_dynamic import set_bn_eval
    net = MyInception_v3()
    net.train()
    bns = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert len(bns) == 70 and all(m.training for m in bns)
    net.apply(set_bn_eval)
    assert net.training and not any(m.training for m in bns)


def test_synthetic_datasets_have_the_reference_tuple_layout():
    from din_amd.train_net_dynamic import SyntheticCollective, SyntheticVolleyball
    cfg = _small_cfg("collective")
    cfg.num_boxes = 5
    v = SyntheticVolleyball(cfg, length=2)[1]
    assert [tuple(t.shape) for t in v] == [(2, 3, 64, 96), (2, 5, 4), (2, 5), (2,)] and v[0].dtype == torch.uint8
    c = SyntheticCollective(cfg, length=3)[2]
    assert [tuple(t.shape) for t in c] == [(2, 3, 64, 96), (2, 5, 4), (2, 5), (2,), (2,)]
    n = int(c[4][0])
    assert 1 <= n <= 5 and bool((c[4] == n).all()) and float(c[1][:, n:].abs().sum()) == 0.0


def test_grad_bucket_order_is_rank_independent_and_late_hooks_do_not_deadlock():
    """GradBuckets learns the bucket layout from the order the conv executor reports weight gradients in.  That order is a property of
    the graph, so it must not depend on the rank; and a gradient reported late (after allreduce() already ran, e.g. a layer that did not
    take part in this backward) must not leave a half-filled bucket in flight."""
    from din_amd.parallel import GradBuckets
    def learn(order):
        lin = torch.nn.Sequential(*[torch.nn.Linear(4, 4) for _ in range(4)])
        b = GradBuckets(lin.parameters(), bucket_bytes=64, overlap=False)
        ws = [lin[i].weight for i in order]
        for w in ws:
            w.grad = torch.zeros_like(w)
            b._on_grad(w, w.grad)
        b._learned = list(dict.fromkeys(b._hook_order))
        hooked = [b._by_ptr[k] for k in b._learned]
        rest = [p for p in reversed(b.params) if p.data_ptr() not in set(b._learned)]
        b._build(hooked + rest, len(hooked))
        index = {p.data_ptr(): i for i, p in enumerate(lin.parameters())}
        return [[index[p.data_ptr()] for p in bk] for bk in b.buckets], b
    layout0, b = learn([3, 2, 1, 0])
    layout1, _ = learn([3, 2, 1, 0])
    assert layout0 == layout1 and layout0[0][0] == 6          # the last layer's weight leads the first bucket on every rank
    # single process: allreduce() is a no-op and must leave no state behind even if hooks fired
    b._on_grad(b.params[0], torch.zeros_like(b.params[0]))
    b.allreduce()
    assert not b._inflight and not b._got


def test_tce_model_keys_and_loadpart():
    """Dynamic_TCE_volleyball on the CPU: constructor limits of the reference model, state_dict key inventory of the oracle's
    shape table, and loadpart() (reference infer_model.py:358-368) copying a prefixed sub-dictionary into one sub-module"""
    from din_amd.config import Config
    from din_amd.infer_model import Dynamic_TCE_volleyball
    cfg = Config("volleyball")
    cfg.backbone, cfg.image_size, cfg.out_size, cfg.emb_features = "vgg16", (96, 160), (3, 5), 512
    cfg.num_features_boxes = cfg.num_features_gcn = 64
    cfg.ST_kernel_size, cfg.sampling_ratio, cfg.beta_factor = [(3, 3)], [1], False
    m = Dynamic_TCE_volleyball(cfg)
    shapes = O.tce_model_param_shapes(O.OracleCfg(backbone="vgg16", image_size=(96, 160), out_size=(3, 5), num_features_boxes=64))
    sd = m.state_dict()
    assert set(shapes) == set(sd.keys())
    for k, shp in shapes.items():
        assert tuple(sd[k].shape) == tuple(shp), k
    assert tuple(m.fc_activities.weight.shape) == (cfg.num_activities, 64 + 4 * 128)         # context_dim = NFB + heads * 128
    src = {"module.fc_emb_1.weight": torch.full_like(m.fc_emb_1.weight, 0.25), "module.fc_emb_1.bias": torch.full_like(m.fc_emb_1.bias, -1.0),
           "module.unrelated.weight": torch.zeros(3)}
    m.loadpart(src, m.fc_emb_1, "module.fc_emb_1.")
    assert float(m.fc_emb_1.weight.min()) == 0.25 and float(m.fc_emb_1.bias.max()) == -1.0
    cfg.backbone = "inv3"
    with pytest.raises(NotImplementedError):
        Dynamic_TCE_volleyball(cfg)
    cfg.backbone, cfg.lite_dim = "vgg16", 128
    with pytest.raises(NotImplementedError):
        Dynamic_TCE_volleyball(cfg)


def test_bench_clock_sampler_degrades_without_a_gpu():
    """bench.py's sclk / power sampler (amdsmi on a background thread) must never break the bench line: with no driver it reports why."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("din_bench_module", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    smp = mod.ClockSampler(0)
    smp.start()
    out = smp.stop()
    assert "sclk_mhz_avg" in out
    if out["sclk_mhz_avg"] is None:
        assert "not sampled" in out["note"]
    else:                                                    # a GPU box: plausible numbers
        assert 50 <= out["sclk_mhz_avg"] <= 3000


def test_bench_dump_outputs_writes_a_fixed_float32_sample(tmp_path):
    """bench.py --dump-outputs: loss, logits and the same seeded sample of the parameters, their gradients and Adam's moments, float32,
    the sample identical from call to call (two builds are compared output for output)."""
    import importlib.util
    import numpy as np
    spec = importlib.util.spec_from_file_location("din_bench_module", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    g = torch.Generator().manual_seed(7)
    params = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((64, 32), (32,), (300,))]
    for p in params:
        p.grad = 2.0 * p.detach()
    ret = {"activities": torch.randn(4, 8, generator=g, dtype=torch.float64)}
    adam = {p: (3.0 * p.detach(), 4.0 * p.detach()) for p in params}
    for d in ("a", "b"):
        mod.dump_outputs(str(tmp_path / d), torch.tensor(1.5), ret, params, adam, sample=256)
    a = {f: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(a) == ["activities.npy", "adam_exp_avg_sample.npy", "adam_exp_avg_sq_sample.npy", "grads_sample.npy", "loss.npy",
                         "params_sample.npy"]
    assert all(v.dtype == np.float32 for v in a.values())
    assert a["activities.npy"].shape == (4, 8) and float(a["loss.npy"][0]) == 1.5
    ps = a["params_sample.npy"]
    assert ps.shape == (256,) and np.array_equal(a["grads_sample.npy"], 2.0 * ps)
    assert np.array_equal(a["adam_exp_avg_sample.npy"], 3.0 * ps) and np.array_equal(a["adam_exp_avg_sq_sample.npy"], 4.0 * ps)
    assert all(np.array_equal(v, np.load(tmp_path / "b" / f)) for f, v in a.items())
    mod.dump_outputs(str(tmp_path / "c"), torch.tensor(0.0), {}, params[1:])           # below the sample size: everything, in order
    assert np.array_equal(np.load(tmp_path / "c" / "params_sample.npy"), torch.cat([params[1], params[2]]).detach().numpy())


def test_bench_plain_run_options():
    """--per-layer comes from the warm-up survey that only --full runs; --steps sets the timed steps and must be positive."""
    for extra in (["--per-layer", "x.txt"], ["--steps", "0"]):
        res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                             text=True, timeout=120)
        assert res.returncode == 2 and "error" in res.stdout, res.stdout


def test_dropout_seeds_distinct_over_ranks_and_replays():
    """Every (rank, step) pair draws its own dropout mask, eager and under graph replay (the replay stride used to equal the
    per-rank stride mod 2^63, so rank r at replay k repeated rank 0's masks of replay k + r).  A captured step's device-side seed is
    mask_seed_of(base, rank, step0) + replay * SEED_STRIDE (csrc/din_common.h fold_seed: sum mod 2^63)."""
    from din_amd import graph_step, ops
    M = 0x7FFFFFFFFFFFFFFF
    assert graph_step.SEED_STRIDE % 2 == 1
    assert (graph_step.SEED_STRIDE - ops.RANK_SEED_STRIDE) & M != 0
    for base in (1, 2, 17):
        seen = {}
        for rank in range(8):
            for replay in range(512):
                s = (ops.mask_seed_of(base, rank, 3) + replay * graph_step.SEED_STRIDE) & M
                assert s not in seen, (base, rank, replay, seen[s])
                seen[s] = (rank, replay)
        eager = {ops.mask_seed_of(base, rank, step) for rank in range(8) for step in range(2048)}
        assert len(eager) == 8 * 2048


# ---- dataset -> tensor contract, pinned by the reference's own datasets (tools/gen_golden.py --only dataset) -------------
def _tree(golden_dir, name):
    return os.path.join(golden_dir, "dataset_tree", name)


def test_volleyball_dataset_matches_reference_golden(golden_dir):
    """annotation parsing, uint8 frames (decode + bilinear resize + CHW), track boxes in feature px (bit-exact float32: the integer-like
    box assignment the RoI stage consumes), short tracks padded by repetition, label tensors -- against what the reference's
    VolleyballDataset produced from the same tree (volleyball.py:223-275)."""
    import pickle
    import numpy as np
    from din_amd import volleyball as V
    z = np.load(os.path.join(golden_dir, "dataset_volleyball.npz"))
    root = _tree(golden_dir, "volleyball")
    anns = V.volley_read_dataset(root, [1, 4])
    frames = V.volley_all_frames(anns)
    assert np.array_equal(np.array(frames), z["frames"])
    for sid in anns:
        for fid, a in anns[sid].items():
            assert np.array_equal(a["bboxes"], z[f"ann.{sid}.{fid}.bboxes"]) and a["actions"] == list(z[f"ann.{sid}.{fid}.actions"])
            assert a["group_activity"] == int(z[f"ann.{sid}.{fid}.group_activity"]) and a["file_name"] == f"{fid}.jpg"
    with open(os.path.join(root, "tracks_normalized.pkl"), "rb") as fh:
        tracks = pickle.load(fh)
    for tag, fsize in (("vgg", (2, 3)), ("inv3", (87, 157))):
        ds = V.VolleyballDataset(anns, tracks, frames, root, (64, 96), fsize, "dynamic_volleyball", num_boxes=12, num_before=1, num_after=1)
        assert len(ds) == 3
        for i in range(len(ds)):
            images, boxes, actions, activities = ds[i]
            assert images.dtype == torch.uint8 and boxes.dtype == torch.float32 and actions.dtype == torch.int64 and activities.dtype == torch.int64
            assert np.array_equal(images.numpy(), z[f"images.{i}"]), "decoded / resized frames differ from the reference's"
            assert np.array_equal(boxes.numpy(), z[f"boxes.{tag}.{i}"]), "feature-px boxes must be bit-identical to the reference's"
            assert np.array_equal(actions.numpy(), z[f"actions.{i}"]) and np.array_equal(activities.numpy(), z[f"activities.{i}"])
    # the padded clips really are padded by repetition of the leading boxes (10 and 7 tracked players of 12)
    b10, b7 = z["boxes.vgg.1"], z["boxes.vgg.2"]
    assert np.array_equal(b10[:, 10:], b10[:, :2]) and np.array_equal(b7[:, 7:], b7[:, :5])
    # float32 mode = the reference's tensor exactly
    f32 = V.VolleyballDataset(anns, tracks, frames, root, (64, 96), (2, 3), num_boxes=12, num_before=1, num_after=1, uint8_images=False)[0][0]
    assert f32.dtype == torch.float32 and np.array_equal(f32.numpy(), z["images.0"].astype(np.float32))
    # fewer than half the players tracked: the reference crashes in its reshape; here the boxes wrap around cyclically
    few = V.pad_by_repetition(np.arange(20.0).reshape(5, 4), 12)
    assert few.shape == (12, 4) and np.array_equal(few[5:10], few[:5]) and np.array_equal(few[10:], few[:2])


def test_collective_dataset_matches_reference_golden(golden_dir):
    """collective.py:40-81,165-225: anchors (fid % 10 == 1), majority activity skipping 'NA', 6->5 / 5->4 class maps, boxes normalised by
    the sequence's frame size then scaled to feature px, zero-box padding with action -1 and the real count in bboxes_num."""
    import numpy as np
    from din_amd import collective as Cc
    z = np.load(os.path.join(golden_dir, "dataset_collective.npz"))
    root = _tree(golden_dir, "collective")
    anns = Cc.collective_read_dataset(root, [1, 15])
    frames = Cc.collective_all_frames(anns)
    assert np.array_equal(np.array(frames), z["frames"])
    for sid in anns:
        for fid, a in anns[sid].items():
            assert np.array_equal(np.asarray(a["bboxes"], dtype=np.float64), z[f"ann.{sid}.{fid}.bboxes"])
            assert a["actions"] == list(z[f"ann.{sid}.{fid}.actions"]) and a["group_activity"] == int(z[f"ann.{sid}.{fid}.group_activity"])
    assert anns[15][11]["group_activity"] == 3                   # 'NA' was the most common action: the runner-up (Walking) decides
    ds = Cc.CollectiveDataset(anns, frames, root, (64, 96), (2, 3), num_boxes=13, num_frames=3)
    for i in range(len(ds)):
        images, boxes, actions, activities, count = ds[i]
        assert images.dtype == torch.uint8 and count.dtype == torch.int32
        assert np.array_equal(images.numpy(), z[f"images.{i}"]) and np.array_equal(boxes.numpy(), z[f"boxes.{i}"])
        assert np.array_equal(actions.numpy(), z[f"actions.{i}"]) and np.array_equal(activities.numpy(), z[f"activities.{i}"])
        assert np.array_equal(count.numpy(), z[f"bboxes_num.{i}"])
        n = int(count[0])
        assert float(boxes[:, n:].abs().max() if n < 13 else 0.0) == 0.0 and (n == 13 or int(actions[:, n:].max()) == -1)
    assert sorted(int(ds[i][4][0]) for i in range(len(ds))) == [3, 5, 6, 13]


def test_return_dataset_builds_both_datasets(golden_dir):
    from din_amd.config import Config
    from din_amd.dataset import return_dataset
    cfg = Config("volleyball")
    cfg.data_path, cfg.train_seqs, cfg.test_seqs = _tree(golden_dir, "volleyball"), [1], [4]
    cfg.image_size, cfg.out_size, cfg.num_before, cfg.num_after, cfg.training_stage = (64, 96), (2, 3), 1, 1, 2
    tr, te = return_dataset(cfg)
    assert len(tr) == 2 and len(te) == 1 and tr[0][0].shape == (3, 3, 64, 96) and te[0][1].shape == (3, 12, 4)
    cfg = Config("collective")
    cfg.data_path, cfg.train_seqs, cfg.test_seqs = _tree(golden_dir, "collective"), [1], [15]
    cfg.image_size, cfg.out_size, cfg.num_frames, cfg.num_boxes, cfg.training_stage = (64, 96), (2, 3), 3, 13, 2
    tr, te = return_dataset(cfg)
    assert len(tr) == 2 and len(te) == 2 and len(tr[0]) == 5 and tr[0][1].shape == (3, 13, 4)


def test_block_entry_shapes_plan_onto_the_register_resident_kernel():
    """din_conv_kernel_tile (no GPU needed): the 1x1 block entries of Mixed_5 / Mixed_6 at 96 frames resolve to conv1x1_regw_kernel (code 5, classes of
    192 | 128 filters), small maps and other reductions do not, and DIN_CONV_REGW=0 hands them back to the tile kernels."""
    from din_amd import _lib
    lib = _lib.load()

    def plan(nb, h, w, cin, cout, which):
        d = _lib.ConvDesc()
        d.nb, d.h, d.w, d.cin, d.oh, d.ow, d.cout = nb, h, w, cin, h, w, cout
        d.kh = d.kw = d.sh = d.sw = d.dh = d.dw = 1
        d.ph = d.pw = 0
        d.ldi, d.cioff, d.ldo, d.cooff, d.dtype = cin, 0, cout, 0, _lib.DIN_BF16
        bm, bn = ctypes.c_int32(0), ctypes.c_int32(0)
        assert lib.din_conv_kernel_tile(ctypes.byref(d), which, ctypes.byref(bm), ctypes.byref(bn)) == 0
        return bm.value, bn.value

    assert plan(96, 43, 78, 768, 576, 0) == (5, 192)            # Mixed_6e sibling group, forward
    assert plan(96, 43, 78, 768, 768, 1) == (5, 192)            # the shape of its four-source data gradient
    assert plan(96, 87, 157, 288, 176, 0) == (5, 128)           # Mixed_5d sibling group: short reduction, two workgroups per CU
    assert plan(96, 87, 157, 256, 64, 0)[0] != 5                # <= 96 filters: the streaming kernel keeps it
    assert plan(12, 43, 78, 768, 576, 0)[0] != 5                # 40 K pixels: below the threshold
    assert plan(96, 43, 78, 512, 192, 0)[0] != 5                # a reduction the kernel is not instantiated for
    _lib.set_option("DIN_CONV_REGW", "0")
    try:
        assert plan(96, 43, 78, 768, 576, 0)[0] != 5
    finally:
        _lib.set_option("DIN_CONV_REGW", None)
