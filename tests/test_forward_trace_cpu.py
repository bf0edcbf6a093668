"""CPU: the launch sequence of the backbone's forward pass is the one profiles/forward_launch_trace.txt holds.

tools/backward_trace.py --forward runs nhwc.graph_forward on CPU tensors against a library proxy that answers the planning queries and
records every launching call and timed launch (the tool's docstring has the format and the cases).  The committed file was recorded from
the forward pass as one 130-line function that decided, allocated and launched in one loop; nhwc.plan_forward + nhwc._ForwardPass
regenerate it byte for byte.  A change to the forward pass that claims to alter no launch alters none of its lines, and one that means
to alter a launch shows up as a diff of that file."""
import collections
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "profiles", "forward_launch_trace.txt")
B4, B40, SMALL = "inv3 bf16 4x720x1280 u8", "inv3 bf16 40x720x1280 u8", "inv3 fp32 2x139x203"
RF_ENTRIES = ("din_conv_rf_fwd", "din_conv_rf5_fwd")


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("backward_trace", os.path.join(ROOT, "tools", "backward_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def recorded(tool):
    """every case of the forward trace, regenerated once for all tests of this module: [(case name, lines of its section)]"""
    return tool.sections(forward=True)


def calls(lines):
    """entry point -> how often a section calls it"""
    return collections.Counter(line.split()[0] for line in lines if line.startswith("din_"))


def test_switches_hooks_options_and_library_are_put_back(tool, recorded):
    import torch
    from din_amd import _lib as L, nhwc
    assert nhwc.torch is torch and not isinstance(L.load(), tool.LibProxy)
    assert all(getattr(nhwc, s) is None for s in nhwc._SWITCHES)
    assert nhwc.GRAD_HOOK is None and nhwc.GRAD_BUFFER is None and nhwc.GRAD_TAP is None and nhwc.LAUNCH_TIMER is None
    assert L.get_option("DIN_GROUP_WGRAD_MAX") is None and L.get_option("DIN_WGRAD_1X1_MULTI") is None and L.get_option("DIN_WGRAD_HALO") is None
    assert not nhwc._WS


def test_forward_pass_launch_sequence_matches_the_recorded_table(tool, recorded):
    with open(TABLE) as fh:
        want = fh.read().splitlines()
    got = tool.written(recorded, forward=True)
    case = None
    for i, (a, b) in enumerate(zip(got + [None] * (len(want) - len(got) + 1), want + [None] * (len(got) - len(want) + 1))):
        case = b[3:] if b is not None and b.startswith("== ") and not b.startswith("== end") else case
        if a != b:
            print(f"first difference at line {i + 1} of profiles/forward_launch_trace.txt, case [{case}]\n  recorded table: {b}\n  this tree:      {a}")
        assert a == b, f"line {i + 1} (case [{case}]) differs from profiles/forward_launch_trace.txt"


def test_every_case_ends_ok_and_every_pointer_has_a_name(recorded):
    assert all(lines[-1] == "== end: ok" for name, lines in recorded if name != "descriptors")
    for name, lines in recorded:
        for line in lines:
            assert "unknown" not in line and "\0" not in line, f"[{name}] a pointer the recorder could not name: {line}"


def test_plan_forward_needs_no_tensor_stream_or_launch_and_says_what_the_trace_shows(tool, recorded, monkeypatch):
    """plan_forward of the 40-frame case with allocation, stream and the conv launches turned into errors: it still returns, and the
    routes, group leads, kernel families and winning-tap maps of its steps are the calls the trace of that case holds"""
    import torch
    from din_amd import _lib as L, nhwc

    def forbidden(*a, **kw):
        raise AssertionError("plan_forward allocated a tensor, took the stream or launched")
    g, dt, _params = tool.backbone("inv3", "bf16", 720, 1280)
    lib = L.load()
    monkeypatch.setattr(torch, "empty", forbidden)
    monkeypatch.setattr(nhwc, "_stream", forbidden)
    for entry in ("din_conv_fwd", "din_conv_fwd2"):
        monkeypatch.setattr(lib, entry, forbidden)
    plan = nhwc.plan_forward(g, 40, dt, False, True, True)
    monkeypatch.undo()
    expected = []                                   # (entry point, name of its timed block or None, maxpool: whether a map is written)
    for op, s in zip(g.ops, plan.steps):
        conv = (s.rf.fwd if s.rf else "din_conv_fwd", op.name, None)
        expected += {"conv": [conv], "pooled": [conv, ("din_avgpool_fwd", None, None)], "lead": [("din_conv_fwd2", s.group and s.group.name, None)],
                     "member": [("din_avgpool_fwd", None, None)] if s.pd is not None else [], "maxpool": [("din_maxpool_fwd", None, s.amax)],
                     "avgpool": [("din_avgpool_fwd", None, None)], "bilinear": [("din_bilinear_fwd", None, None)]}[s.route]
    seen = []
    for line in dict(recorded)[B40]:
        words = line.split()
        if line.startswith("din_") and words[0] not in ("din_bn_fold_multi", "din_conv_pack_multi"):
            seen.append((words[0], words[words.index("|") + 2] if "|" in words else None, words[4] != "null" if words[0] == "din_maxpool_fwd" else None))
    assert seen == expected
    routes = collections.Counter(s.route for s in plan.steps)
    assert routes["lead"] == 7 and sum(1 for s in plan.steps if s.rf is not None) == 10 and routes["member"] == 21
    assert all(s.rf is None for s in plan.steps if s.route not in ("conv", "pooled"))
    # ... and the loop and the pass decide nothing: no switch, no parameter iterator, no planning query outside plan_forward
    import inspect
    doing = inspect.getsource(nhwc.graph_forward) + inspect.getsource(nhwc._ForwardPass)
    assert not any(word in doing for word in ("switch(", "next(", "din_conv_workspace_bytes", "eligible"))


def test_table_covers_the_routes_it_is_there_for(recorded):
    """the counts are those of the forward pass before it was split into plan and pass"""
    recorded = dict(recorded)
    big = calls(recorded[B40])
    assert sum(big.values()) == 61
    assert {e: big[e] for e in ("din_conv_fwd2", "din_conv_rf_fwd", "din_conv_rf5_fwd", "din_conv_fwd", "din_avgpool_fwd", "din_maxpool_fwd",
                                "din_bn_fold_multi", "din_conv_pack_multi")} == \
        {"din_conv_fwd2": 7, "din_conv_rf_fwd": 7, "din_conv_rf5_fwd": 3, "din_conv_fwd": 32, "din_avgpool_fwd": 7, "din_maxpool_fwd": 3,
         "din_bn_fold_multi": 1, "din_conv_pack_multi": 1}
    four = calls(recorded[B4])
    assert four["din_conv_fwd"] == 42 and not any(four[e] for e in RF_ENTRIES)
    assert calls(recorded[B40 + " FUSE_FWD_SIBLINGS=off"])["din_conv_fwd2"] == 0
    for name in (B4 + " bn-train", B40 + " bn-train"):
        c = calls(recorded[name])
        assert [c[e] for e in ("din_conv_fwd", "din_bn_stats", "din_bn_finalize", "din_bn_apply")] == [70] * 4, name
        assert not any(c[e] for e in ("din_bn_fold_multi", "din_conv_fwd2") + RF_ENTRIES), name
    # the split-K fall-through of the group route is reached: the same 7 groups make 1, 3 and 7 two-destination launches
    assert calls(recorded[SMALL])["din_conv_fwd2"] == 1 and calls(recorded["inv3 bf16 2x139x203"])["din_conv_fwd2"] == 3
    assert big["din_conv_fwd2"] == 7
    pools = [line.split() for line in recorded[B4 + " save_for_backward=False"] if line.startswith("din_maxpool_fwd ")]
    assert len(pools) == 3 and all(words[4] == "null" for words in pools)              # eval: no winning-tap map
    assert any(line.split()[4] != "null" for line in recorded[B4] if line.startswith("din_maxpool_fwd "))
    vgg = calls(recorded["vgg16 fp32 2x96x160"])
    assert vgg["din_conv_fwd"] == 13 and vgg["din_maxpool_fwd"] == 5 and vgg["din_bn_fold_multi"] == 0
    first_conv = lambda name: next(line for line in recorded[name] if line.startswith("din_conv_fwd "))      # noqa: E731
    assert first_conv("inv3 bf16 4x720x1280") != first_conv(B4)                         # (uint8 frames: another image-layer descriptor)
