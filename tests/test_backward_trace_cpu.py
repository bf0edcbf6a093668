"""CPU: the launch sequence of the backbone's reverse pass is the one profiles/backward_launch_trace.txt holds.

tools/backward_trace.py runs nhwc.graph_forward + nhwc.graph_backward on CPU tensors against a library proxy that answers the planning
queries and records every launching call, hook and timed launch (the tool's docstring has the format and the cases).  The committed file
was recorded from the reverse pass as one 516-line function; it is the evidence that a change to nhwc.graph_backward that claims to alter
no launch alters none, and a change that means to alter one shows up as a diff of that file."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "profiles", "backward_launch_trace.txt")


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("backward_trace", os.path.join(ROOT, "tools", "backward_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def recorded(tool):
    """every case, regenerated once for all tests of this module: [(case name, lines of its section)]"""
    return tool.sections()


def test_switches_hooks_and_library_are_put_back(tool, recorded):
    import torch
    from din_amd import _lib as L, nhwc
    assert nhwc.torch is torch and not isinstance(L.load(), tool.LibProxy)
    assert all(getattr(nhwc, s) is None for s in nhwc._SWITCHES)
    assert nhwc.GRAD_HOOK is None and nhwc.GRAD_BUFFER is None and nhwc.GRAD_TAP is None and nhwc.LAUNCH_TIMER is None
    assert L.get_option("DIN_GROUP_WGRAD_MAX") is None and L.get_option("DIN_WGRAD_1X1_MULTI") is None


def test_reverse_pass_launch_sequence_matches_the_recorded_table(tool, recorded):
    with open(TABLE) as fh:
        want = fh.read().splitlines()
    got = tool.written(recorded)
    case = None
    for i, (a, b) in enumerate(zip(got + [None], want + [None])):
        case = b[3:] if b is not None and b.startswith("== ") and not b.startswith("== end") else case
        if a != b:
            print(f"first difference at line {i + 1} of profiles/backward_launch_trace.txt, case [{case}]\n  recorded table: {b}\n  this tree:      {a}")
        assert a == b, f"line {i + 1} (case [{case}]) differs from profiles/backward_launch_trace.txt"


def test_table_covers_the_paths_it_is_there_for(recorded):
    """the cases reach what they were chosen for (a table of cases that all take the common path would pin nothing)"""
    recorded = dict(recorded)

    def count(name, entry):
        return sum(1 for line in recorded[name] if line.startswith(entry + " "))

    def hooks(name):
        return sum(1 for line in recorded[name] for word in line.split() if word[0] == "H" and word[1:].isdigit())
    big = "inv3 bf16 40x720x1280 u8"
    assert count(big, "din_conv1x1_wgrad_multi") and count(big, "din_conv_wgrad_group") and count(big, "din_conv_dgrad_x") == 1
    assert count(big, "din_conv1x1_dgrad_multi") and hooks(big) == 70
    assert count(big, "din_conv_wgrad_group") != count("inv3 bf16 4x720x1280 u8", "din_conv_wgrad_group")     # (batch-dependent flush)
    for off, entry in (("FUSE_1X1_DGRAD", "din_conv1x1_dgrad_multi"), ("FUSE_WGRAD_1X1", "din_conv1x1_wgrad_multi"),
                       ("FUSE_DGRAD_X", "din_conv_dgrad_x"), ("GROUP_WGRAD", "din_conv_wgrad_group")):
        assert count(f"{big} {off}=off", entry) == 0
    assert count("inv3 bf16 4x720x1280 u8 bn-train", "din_bn_bwd_apply") == 70
    assert count("inv3 bf16 2x139x203 DIN_WGRAD_1X1_MULTI=2 DIN_WGRAD_HALO=2", "din_conv1x1_wgrad_multi") == 3
    partial = "partial-heads bf16 2x48x64 DIN_WGRAD_1X1_MULTI=2"
    assert count(partial, "din_conv1x1_wgrad_multi") == 0 and count(partial, "din_conv_wgrad") == 3      # stem + the two heads with a gradient
    timed = [line.split(" | ")[1].split(" H")[0] for line in recorded["parked bf16 2x48x64"] if " | dgrad " in line]
    assert timed == ["dgrad middle 32", "dgrad lone 64"] and count("parked bf16 2x48x64", "din_conv_dgrad_x") == 0    # parked, then run alone
    assert all(lines[-1] == "== end: ok" for name, lines in recorded.items() if name != "descriptors")
    assert not any("unknown" in line or "\0" in line for lines in recorded.values() for line in lines), "a pointer the recorder could not name"


def test_parked_dgrad_nobody_carried_still_raises(tool):
    """No graph reaches this through graph_backward (the strided host always has its turn after the 1x1 and consumes the entry either
    way), so the check at the end of the pass is exercised on the pass state directly: a parked entry left over must raise, not be dropped."""
    import torch
    from din_amd import _lib as L, nhwc
    g, dt, params, _ = tool.parked()
    try:
        with tool.dry_run(tool.Recorder({})):
            bufs, aux = nhwc.graph_forward(g, torch.empty((2, 48, 64, 8), dtype=torch.bfloat16), params, dt, True, False)
            bp = nhwc._BackwardPass(g, nhwc.plan_backward(g, 2, dt, False, True, False), bufs, aux, params, dt, {})
            bp.parked[1] = nhwc._Parked(3, torch.empty_like(bufs[g.ops[3].dst.tid]), 64, 0)
            with pytest.raises(L.DinError, match="never carried"):
                bp.finish()
    finally:
        for attr in ("_pack_cache", "_bn_tables"):
            g.__dict__.pop(attr, None)
