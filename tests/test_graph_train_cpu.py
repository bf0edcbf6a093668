"""FusedAdam(capturable=True) without a GPU: the default, the refusal of the non-fused path, the two additive entry points of the C ABI,
the checkpoint format, and the float64 restatement of the device record's rule -- "the step count advances unless the step is
skipped" (record_adam_model, written here from the definitions in include/din_hip.h) -- that
tests/test_gpu_graph_train.py holds the kernels and the optimizer to.  The restatement is tied to torch.nn.utils.clip_grad_norm_ +
torch.optim.Adam in float64 over the FINITE steps only; a model of the host-side rule (the index advances on a skipped step too,
tests/test_grad_clip_cpu.clip_adam_model) misses the same answer by far more than 10x the bar."""
import inspect
import math
import os
import re

import pytest
import torch

from tests.test_grad_clip_cpu import AEPS, B1, B2, LR, _header_arg_count, clip_adam_model, norm_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("din_adam_state_advance", "din_adam_step_multi_dev")
RTOL, ATOL = 1e-12, 1e-15          # the bar of the float64 restatements (test_grad_clip_cpu uses the same against torch)


# ---- the float64 model of the device record ---------------------------------------------------------------------------------------------
class RecordModel:
    """ostate of din_adam_state_advance in float64: steps taken, lr, beta1^steps, beta2^steps"""

    def __init__(self, lr=LR, step=0):
        self.step, self.lr, self.p1, self.p2 = step, lr, B1 ** step, B2 ** step

    def advance(self, norm=None):
        """norm: the clip state's norm, None without a clip state.  -> whether the step counts"""
        if norm is not None and not math.isfinite(norm):
            return False
        self.step, self.p1, self.p2 = self.step + 1, self.p1 * B1, self.p2 * B2
        return True

    def fields(self):
        return [float(self.step), self.lr, self.p1, self.p2]


def record_adam_model(params, moments, grads, record, wd, grad_scale, max_norm=None):
    """din_adam_state_advance + din_adam_step_multi_dev in float64: advance unless skipped, then Adam with lr and both bias corrections
    taken from the record.  max_norm None: no clip state.  Returns (new params, new moments, coef or None when skipped)."""
    norm, coef = (None, 1.0) if max_norm is None else norm_model(grads, grad_scale, max_norm)
    if not record.advance(norm):
        return [p.clone() for p in params], [(m.clone(), v.clone()) for m, v in moments], None
    new_p, new_mv = [], []
    for p, (m, v), g in zip(params, moments, grads):
        gi = g.double() * (grad_scale * coef) + wd * p
        m2, v2 = B1 * m + (1 - B1) * gi, B2 * v + (1 - B2) * gi * gi
        bc1, bc2 = 1 - record.p1, math.sqrt(1 - record.p2)
        new_p.append(p - (record.lr / bc1) * (m2 / (v2.sqrt() / bc2 + AEPS)))
        new_mv.append((m2, v2))
    return new_p, new_mv, coef


def _toy(step):
    gen = torch.Generator().manual_seed(500 + step)
    grads = [0.05 * torch.randn(shape, generator=gen, dtype=torch.float64) for shape in ((7,), (3, 5), (33,))]
    if step == 2:
        grads[1][2, 3] = float("nan")
    return grads


def _miss(a, b):
    """how many bars a is from b"""
    return float(((a - b).abs() / (ATOL + RTOL * b.abs())).max())


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_advance_unless_skipped_equals_adam_over_the_finite_steps(wd):
    """four steps, the gradient of step 2 not finite: the device rule gives torch.optim.Adam's float64 answer over steps 1, 3, 4 alone;
    today's host rule (the bias-correction index is 3 and 4 for them) does not"""
    max_norm = 10.0                                                    # (never clips: the difference is the skip alone)
    gen = torch.Generator().manual_seed(11)
    init = [torch.randn(shape, generator=gen, dtype=torch.float64) for shape in ((7,), (3, 5), (33,))]
    ref_p = [torch.nn.Parameter(p.clone()) for p in init]
    ref = torch.optim.Adam(ref_p, lr=LR, betas=(B1, B2), eps=AEPS, weight_decay=wd)
    p, mv, rec = [q.clone() for q in init], [(torch.zeros_like(q), torch.zeros_like(q)) for q in init], RecordModel()
    hp, hmv = [q.clone() for q in init], [(torch.zeros_like(q), torch.zeros_like(q)) for q in init]
    counted = []
    for step in range(1, 5):
        grads = _toy(step)
        p, mv, coef = record_adam_model(p, mv, grads, rec, wd, 1.0, max_norm)
        hp, hmv, _, _ = clip_adam_model(hp, hmv, grads, [step] * 3, wd, 1.0, max_norm)
        counted.append(coef is not None)
        if coef is None:
            continue
        for q, g in zip(ref_p, grads):
            q.grad = g.clone()
        torch.nn.utils.clip_grad_norm_(ref_p, max_norm, norm_type=2)
        ref.step()
    assert counted == [True, False, True, True] and rec.step == 3
    assert math.isclose(rec.p1, B1 ** 3, rel_tol=1e-15) and math.isclose(rec.p2, B2 ** 3, rel_tol=1e-15)
    worst = max(_miss(mine, q.detach()) for q, mine in zip(ref_p, p))
    host_rule = max(_miss(theirs, q.detach()) for q, theirs in zip(ref_p, hp))
    print(f"device rule: {worst:.3g} bars from torch.optim.Adam over the finite steps; host rule (index advanced): {host_rule:.3g} bars")
    assert worst <= 1.0
    assert host_rule >= 10.0
    for q, (m, v) in zip(ref_p, mv):
        assert torch.allclose(ref.state[q]["exp_avg"], m, rtol=RTOL, atol=1e-18)
        assert torch.allclose(ref.state[q]["exp_avg_sq"], v, rtol=RTOL, atol=1e-24)
    assert int(ref.state[ref_p[0]]["step"]) == rec.step


def test_record_without_a_clip_state_always_advances():
    rec = RecordModel(step=999)
    assert rec.advance(None) and rec.fields()[0] == 1000.0
    assert math.isclose(rec.p1, B1 ** 1000, rel_tol=1e-14) and math.isclose(rec.p2, B2 ** 1000, rel_tol=1e-14)
    assert not rec.advance(float("inf")) and not rec.advance(float("nan")) and rec.step == 1000


# ---- the setting ------------------------------------------------------------------------------------------------------------------------
def test_the_default_is_off():
    from din_amd.optim import FusedAdam
    assert FusedAdam([torch.zeros(3)]).capturable is False
    assert inspect.signature(FusedAdam.__init__).parameters["capturable"].default is False


def test_capturable_refuses_the_non_fused_path_by_parameter():
    """a CPU tensor is the non-fused path (so is a non-contiguous or a non-fp32 device tensor): refused at construction, by index and shape"""
    from din_amd.optim import FusedAdam
    with pytest.raises(ValueError, match=r"capturable=True\): parameter 0 \(shape \(2, 3\)"):
        FusedAdam([torch.zeros(2, 3), torch.zeros(4)], capturable=True)
    assert FusedAdam([torch.zeros(2, 3), torch.zeros(4)]).capturable is False


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------
def test_the_two_entry_points_are_declared_and_bound():
    from din_amd import _lib
    symbols = _lib.header_symbols()
    for name in NEW_SYMBOLS:
        assert name in symbols and name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == _header_arg_count(name), name
    # the device-state launch takes din_adam_step_multi's tables and hyper-parameters without lr and step, then grad_scale, the record,
    # the optional clip state and the stream
    plain, dev = _lib.SIGNATURES["din_adam_step_multi"][1], _lib.SIGNATURES["din_adam_step_multi_dev"][1]
    assert dev[:6] == plain[:6] and len(dev) == len(plain) and dev[-3:] == [_lib._P] * 3
    assert _header_arg_count("din_adam_state_advance") == 5
    assert _lib.ABI_VERSION == 9 and re.search(r"#define DIN_ABI_VERSION 9\b", open(_lib.HEADER_PATH).read())
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert int(re.search(r"\((\d+) entry points", readme).group(1)) == len(symbols)
    assert "## Adam with device-resident state" in readme


# ---- checkpoints ------------------------------------------------------------------------------------------------------------------------
def test_checkpoint_keys_are_unchanged():
    """the optimizer entry keeps torch.optim.Adam's format (capturable=True is the constructor's, the state lives on a device: its round
    trip is a GPU test); the stage-2 file keeps its keys"""
    from din_amd.optim import FusedAdam
    params = [torch.zeros(4, requires_grad=True), torch.zeros(2, 3, requires_grad=True)]
    opt = FusedAdam(params, lr=1e-3)
    for p in params:
        opt.state[p], opt.steps[p] = (torch.zeros_like(p), torch.zeros_like(p)), 3
    sd = opt.state_dict()
    assert sd.keys() == {"state", "param_groups"} and all(sd["state"][i].keys() == {"step", "exp_avg", "exp_avg_sq"} for i in sd["state"])
    assert sd["param_groups"][0]["capturable"] is False                # (torch's own flag of that name: not this constructor's)
    assert set(sd["param_groups"][0]) == {"lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "foreach", "capturable",
                                          "differentiable", "fused", "decoupled_weight_decay", "params"}
    torch.optim.Adam([torch.nn.Parameter(p.detach().clone()) for p in params], lr=1e-3).load_state_dict(sd)
    source = open(os.path.join(ROOT, "din-group-activity-recognition-benchmark_amd", "train_net_dynamic.py")).read()
    assert '{"epoch": epoch, "state_dict": model.state_dict(), "optimizer": optimizer.state_dict(),' in source
