"""Deterministic mode, host side (no GPU): the config default, train_net's two refusals, the option's set / restore around train_net and
ops.deterministic, the host-only reporter din_walk_bwd_kernel_name (symbol, prototype, its answers with the option unset and set, the
refusal of a grid whose ordered kernel does not fit the LDS), the register counts of the two scatter kernels the mode must leave as they
were, and a numpy model of the ordered walk summation -- the per-tap records, the stable per-cell lists and the in-order sums of
csrc/din_walk.hip's din_walk_bwd_dx_ordered_kernel -- against walk_reference's dx in float64: that pins the algorithm, not the kernel."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest
import torch

from tests.test_gpu_head_path import WALK_IDS, WALK_ROWS, _walk_expected, _walk_geom, _walk_operands, _walk_positions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "din-group-activity-recognition-benchmark_amd")
OPTION = "DIN_DETERMINISTIC"
LDS_LIMIT = 160 * 1024


def _cfg(**kw):
    from din_amd.config import Config
    cfg = Config("volleyball")
    cfg.backbone, cfg.training_stage, cfg.deterministic = "vgg16", 2, True
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


@pytest.fixture
def options():
    """the library's option table, with every option this file touches back at its value when the test ends"""
    from din_amd import _lib
    names = (OPTION, "DIN_WALK_BWD_GLOBAL", "DIN_WALK_BWD_GROUPS")
    before = {n: _lib.get_option(n) for n in names}
    for n in names:
        _lib.set_option(n, None)
    yield _lib
    for n, v in before.items():
        _lib.set_option(n, v)


def test_config_default_is_off():
    from din_amd.config import Config
    for name in ("volleyball", "collective"):
        assert Config(name).deterministic is False


CACHES = [dict(), dict(feature_cache_gb=1), dict(frame_cache_gb=2), dict(num_workers=4), dict(feature_cache_gb=1, frame_cache_gb=2, num_workers=3)]


@pytest.mark.parametrize("caches", CACHES, ids=["plain", "feature_cache", "frame_cache", "workers", "all"])
@pytest.mark.parametrize("kw,world,words", [
    (dict(train_backbone=True), "1", ("deterministic", "train_backbone", "frozen")),
    (dict(), "2", ("deterministic", "2 ranks", "one rank")),
], ids=["train_backbone", "two_ranks"])
def test_train_net_refuses_before_any_loader_is_built(kw, world, words, caches, monkeypatch, options):
    """both refusals are ValueErrors naming `deterministic`, raised before a process group, a loader or the device is touched, with the same
    message whatever the caches and the workers are set to; the option is not left set"""
    from din_amd import frame_cache as FC, train_net_dynamic as TD
    monkeypatch.setenv("WORLD_SIZE", world)
    monkeypatch.setattr(FC, "build_loaders", lambda *a, **k: pytest.fail("a loader was built before the refusal"))
    monkeypatch.setattr(TD.parallel, "init_from_env", lambda *a, **k: pytest.fail("the device was set up before the refusal"))
    messages = []
    for extra in (caches, dict()):
        with pytest.raises(ValueError) as e:
            TD.train_net(_cfg(**kw, **extra))
        messages.append(str(e.value))
        for w in words:
            assert w in messages[-1], (w, messages[-1])
    assert messages[0] == messages[1]
    assert options.get_option(OPTION) is None


def test_without_the_setting_nothing_is_refused_or_set(monkeypatch, options):
    from din_amd import train_net_dynamic as TD
    seen = []
    monkeypatch.setattr(TD, "_train_net", lambda *a: seen.append(options.get_option(OPTION)) or "ran")
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert TD.train_net(_cfg(deterministic=False, train_backbone=True)) == "ran" and seen == [None]


@pytest.mark.parametrize("previous", [None, "0", "1"])
def test_option_is_set_for_the_call_and_restored_after_it(previous, monkeypatch, options):
    """train_net sets the option for the duration of the call and puts the previous value back when the call returns and when it raises"""
    from din_amd import train_net_dynamic as TD
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    options.set_option(OPTION, previous)
    seen = []

    def returns(cfg, *rest):
        seen.append(options.get_option(OPTION))
        return ["info"]

    def raises(cfg, *rest):
        seen.append(options.get_option(OPTION))
        raise RuntimeError("the step failed")

    monkeypatch.setattr(TD, "_train_net", returns)
    assert TD.train_net(_cfg()) == ["info"]
    assert options.get_option(OPTION) == previous
    monkeypatch.setattr(TD, "_train_net", raises)
    with pytest.raises(RuntimeError, match="the step failed"):
        TD.train_net(_cfg())
    assert options.get_option(OPTION) == previous
    assert seen == ["1", "1"]


def test_context_manager_sets_and_restores(options):
    from din_amd import ops
    with ops.deterministic():
        assert options.get_option(OPTION) == "1"
        with ops.deterministic(False):
            assert options.get_option(OPTION) is None
        assert options.get_option(OPTION) == "1"
        with pytest.raises(KeyError):
            with ops.deterministic():
                raise KeyError("x")
        assert options.get_option(OPTION) == "1"
    assert options.get_option(OPTION) is None


def test_stage1_trainer_says_it_ignores_the_setting():
    from din_amd import train_net as T1
    assert "deterministic is ignored" in " ".join(T1.train_net.__doc__.split())
    assert "deterministic" not in re.sub(r'""".*?"""', "", open(os.path.join(PKG, "train_net.py")).read(), flags=re.S)


def test_reporter_symbol_and_prototype_match_the_header():
    from din_amd import _lib
    header = " ".join(open(_lib.HEADER_PATH).read().split())
    assert "int din_walk_bwd_kernel_name(int b, int t, int n, int c, int kh, int kw, int ratio, char* buf, int buf_bytes);" in header
    assert "#define DIN_ABI_VERSION 9 " in open(_lib.HEADER_PATH).read() and _lib.ABI_VERSION == 9
    res, args = _lib.SIGNATURES["din_walk_bwd_kernel_name"]
    assert res is C.c_int and args == [C.c_int] * 7 + [C.c_char_p, C.c_int]
    assert hasattr(C.CDLL(_lib.LIB_PATH), "din_walk_bwd_kernel_name")
    assert "din_walk_bwd_kernel_name" in _lib.header_symbols()
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert f"({len(_lib.header_symbols())} entry points" in readme and "## Deterministic mode" in readme


def _name(lib, shape):
    buf = C.create_string_buffer(96)
    rc = lib.din_walk_bwd_kernel_name(*shape, buf, 96)
    return rc, (buf.value.decode() if rc == 0 else lib.din_last_error_string().decode())


def _lds(shape):
    """(one padded tile, the offset / relation tables, the ordered kernel's need) in bytes, from the layouts csrc/din_walk.hip documents"""
    b, t, n, c, kh, kw, ratio = shape
    hp, wp, k2 = t + 2 * ((kh - 1) // 2 * ratio), n + 2 * ((kw - 1) // 2 * ratio), kh * kw
    return hp * wp * 64 * 4, t * n * 3 * k2 * 4, t * n * 64 * 4 + t * n * k2 * 16


REPORT_SHAPES = [(32, 10, 12, 1024, 3, 3, 1), (2, 3, 5, 64, 3, 3, 1), (1, 10, 12, 64, 5, 5, 2), (1, 10, 12, 64, 7, 7, 1), (1, 4, 8, 64, 7, 7, 1),
                 (4, 3, 7, 96, 3, 3, 1), (1, 1, 1, 1, 1, 1, 1)]


def test_reporter_with_the_option_unset(options):
    """the two scatter kernels, chosen as din_walk_bwd chooses: dx itself unless DIN_WALK_BWD_GLOBAL = 0 and two LDS tiles fit"""
    lib = options.load()
    both = set()
    for glob_opt in (None, "1", "0"):
        options.set_option("DIN_WALK_BWD_GLOBAL", glob_opt)
        for shape in REPORT_SHAPES:
            tile, tab, _ = _lds(shape)
            want = "din_walk_bwd_kernel<false>" if glob_opt == "0" and 2 * tile + tab <= LDS_LIMIT else "din_walk_bwd_kernel<true>"
            assert _name(lib, shape) == (0, want), (shape, glob_opt)
            both.add(want)
    assert len(both) == 2
    options.set_option("DIN_WALK_BWD_GROUPS", 3)                   # (the launch shape chooses no kernel)
    assert _name(lib, REPORT_SHAPES[0]) == (0, "din_walk_bwd_kernel<false>")
    options.set_option("DIN_WALK_BWD_GLOBAL", None)
    assert _name(lib, REPORT_SHAPES[0]) == (0, "din_walk_bwd_kernel<true>")
    rc, msg = _name(lib, (1, 40, 40, 64, 3, 3, 1))                 # where the launch refuses, so does the reporter
    assert rc == -1 and "too large" in msg
    assert _name(lib, (1, 3, 5, 64, 8, 8, 1))[0] == -1
    assert lib.din_walk_bwd_kernel_name(2, 3, 5, 64, 3, 3, 1, C.create_string_buffer(8), 8) == -1
    assert lib.din_walk_bwd_kernel_name(2, 3, 5, 64, 3, 3, 1, None, 96) == -1


OVERSIZE = (1, 1, 160, 64, 1, 49, 1)           # 160 positions x 49 taps: the scatter kernel's tile and tables fit, the ordered kernel's records do not


def test_reporter_with_the_option_set(options):
    lib = options.load()
    tile, tab, ordered = _lds(OVERSIZE)
    assert tile + tab <= LDS_LIMIT < ordered
    assert _name(lib, OVERSIZE) == (0, "din_walk_bwd_kernel<true>")
    options.set_option(OPTION, 1)
    for glob_opt in (None, "0"):
        options.set_option("DIN_WALK_BWD_GLOBAL", glob_opt)
        for shape in REPORT_SHAPES:
            assert max(_lds(shape)[2], sum(_lds(shape)[:2])) <= LDS_LIMIT
            assert _name(lib, shape) == (0, "din_walk_bwd_dx_ordered_kernel"), (shape, glob_opt)
        rc, msg = _name(lib, OVERSIZE)
        assert rc == -1 and OPTION in msg and "too large" in msg, msg
    # the launcher refuses the same grid with the same words before it touches a pointer (4096: a non-null address no refused call reads)
    d = C.c_void_p(4096)
    rc = lib.din_walk_bwd(d, d, 147, d, d, *OVERSIZE, 1, 0, None, None, d, d, d, None)
    assert rc == -1 and OPTION in lib.din_last_error_string().decode()
    options.set_option(OPTION, 0)                                  # "0" is off
    assert _name(lib, OVERSIZE) == (0, "din_walk_bwd_kernel<true>")


def test_scatter_kernels_keep_their_registers_and_the_new_ones_spill_nothing():
    """the two scatter instantiations must compile to what they were before the mode existed (82 / 70 VGPRs, 76 / 85 SGPRs, no scratch):
    their body moved into an include shared with the scatter-free instantiation"""
    path = os.path.join(PKG, "csrc", "din_walk.res")
    if not glob.glob(path):
        pytest.skip("no csrc/din_walk.res (library built before the Makefile wrote them): run __graft_entry__.build() after `make clean`")
    usage = {}
    for blk in re.split(r"remark: Function Name: ", open(path).read())[1:]:
        grab = lambda pat: int(re.search(pat, blk).group(1))      # noqa: E731
        usage[blk.split()[0]] = (grab(r" VGPRs: (\d+)"), grab(r"TotalSGPRs: (\d+)"), grab(r"ScratchSize \[bytes/lane\]: (\d+)"))
    pick = lambda key: [v for k, v in usage.items() if key in k]  # noqa: E731
    assert pick("din_walk_bwd_kernelILb1E") == [(82, 76, 0)] and pick("din_walk_bwd_kernelILb0E") == [(70, 85, 0)], usage
    for new in ("din_walk_bwd_nodx_kernel", "din_walk_bwd_dx_ordered_kernel"):
        (vgprs, _, scratch), = pick(new)
        assert scratch == 0 and vgprs <= 128, (new, vgprs, scratch)


# ---- the ordered summation, modelled ------------------------------------------------------------------------------------------------
NONE = 255


def ordered_walk_dx(row, a, gz):
    """dx of a row of WALK_ROWS as din_walk_bwd_dx_ordered_kernel forms it, in float64: one record per tap (position, k) -- the four clamped
    corner coordinates (255: no such corner), the clamped sampling position, a_k; per destination cell the stable list of the corners
    (position, k, corner lt-rb-lb-rt) that fall on it, each weighing a_k (1 - |py - cy|) (1 - |px - cx|) with the CELL's coordinates; the
    list summed in its order, every cell written once.  Returns dx and the longest list."""
    g = _walk_geom(row)
    b, t, n, c, kh, kw, ratio, k2, pt, pl, hp, wp = (g[k] for k in ("b", "t", "n", "c", "kh", "kw", "ratio", "k2", "pt", "pl", "hp", "wp"))
    py0, px0 = _walk_positions(_walk_operands(row["name"])["pred"][..., :2 * k2], row)
    py0, px0 = py0.astype(np.float64), px0.astype(np.float64)
    a, gz = a.numpy().astype(np.float64), gz.numpy().astype(np.float64)
    dx = np.zeros((b, t * n, c))
    longest = 0
    for bi in range(b):
        nb = row["npc"][bi] if row["npc"] else n
        hy, hx = hp - 1, nb + 2 * pl - 1
        phy, phx = hy, hx
        if g["clamp"]:
            hy, hx, phy, phx = min(g["clamp"][0], hp - 1), min(g["clamp"][1], wp - 1), g["clamp"][2], g["clamp"][3]
        records = []                                              # (ly, ry, lx, rx, py, px, a_k) in (position, k) order
        for pos in range(t * n):
            tt, nn = divmod(pos, n)
            for k in range(k2):
                if nn >= nb:
                    records.append((NONE, NONE, NONE, NONE, 0.0, 0.0, 0.0))
                    continue
                y0, x0 = py0[bi, tt, nn, k], px0[bi, tt, nn, k]
                if row["plain"]:
                    records.append((int(y0), NONE, int(x0), NONE, y0, x0, a[bi, tt, nn, k]))
                    continue
                fy, fx = np.floor(y0), np.floor(x0)
                corner = lambda v, hi: int(min(max(v, 0), hi))    # noqa: E731
                records.append((corner(fy, hy), corner(fy + 1, hy), corner(fx, hx), corner(fx + 1, hx), min(max(y0, 0), phy), min(max(x0, 0), phx),
                                a[bi, tt, nn, k]))
        assert max(hp, wp) < NONE
        table = []                                                # (destination cell, weight, source position), four entries per record
        for r, (ly, ry, lx, rx, py, px, ak) in enumerate(records):
            for cy, cx in ((ly, lx), (ry, rx), (ry, lx), (ly, rx)):
                tt2, nn2 = cy - pt, cx - pl
                inside = cy != NONE and cx != NONE and 0 <= tt2 < t and 0 <= nn2 < nb
                table.append((tt2 * n + nn2 if inside else -1, ak * ((1 - abs(py - cy)) * (1 - abs(px - cx))) if inside else 0.0, r // k2))
        cells = np.array([e[0] for e in table])
        order = np.argsort(cells, kind="stable")                 # the per-cell lists: table order kept inside a cell
        for e in order[cells[order] >= 0]:
            cell, weight, src = table[e]
            dx[bi, cell] = dx[bi, cell] + weight * gz[bi].reshape(t * n, c)[src]
        longest = max([longest] + np.bincount(cells[cells >= 0]).tolist())
    return dx.reshape(b, t, n, c), longest


@pytest.mark.parametrize("name", ["k33", "c96", "k13", "one_pos", "noscale", "plain_k33", "plain_k55r2", "clamp_small", "clamp_large", "npc", "k77"])
def test_ordered_summation_model_matches_the_reference(name):
    row = WALK_ROWS[WALK_IDS.index(name)]
    want, o = _walk_expected(name), _walk_operands(name)
    dx, longest = ordered_walk_dx(row, want["a"], o["gz"])
    assert longest == int(want["dx_cnt"].max()) or row["plain"]    # (dx_cnt counts corner hits of features, which is what a list holds)
    err = float(np.abs(dx - want["dx"].numpy()).max())
    assert err <= 1e-12 * float(want["dx"].abs().max()), (name, err)
    if row["npc"]:
        assert not dx[~want["valid"].numpy()].any()
