"""cfg.max_grad_norm / FusedAdam(max_grad_norm=...) without a GPU: the setting and its refusals, the three additive entry points of the C
ABI, the checkpoint format, and the float64 restatement of clip + skip + Adam (clip_adam_model, written here from the definitions in
include/din_hip.h) that tests/test_gpu_grad_clip.py holds the kernels and the optimizer to.  The restatement is tied to
torch.nn.utils.clip_grad_norm_ + torch.optim.Adam in float64, and a numpy emulation of the cheap wrong kernel -- squares and running sum
kept in fp32 -- shows that each adversarial input of the GPU test tells it apart by at least 10x the norm's bar."""
import math
import re

import numpy as np
import pytest
import torch

NORM_BAR = 2.0 ** -22      # relative, state[0]: the final fp32 rounding is 2^-24, the fp64 sum adds n * 2^-53 (2e-12 here): about 4x left
COEF_BAR = 2.0 ** -21      # relative, state[1]: the norm's bar plus one fp32 add and one fp32 divide
B1, B2, LR, AEPS = (float(np.float32(v)) for v in (0.9, 0.999, 1e-3, 1e-8))        # what the C ABI receives: fp32 values


# ---- the float64 model ----------------------------------------------------------------------------------------------------------------
def norm_model(grads, grad_scale, max_norm):
    """(norm, coef) of one step in float64: norm = grad_scale * sqrt(sum of squares of every gradient), coef = min(1, max / (norm + 1e-6))
    (torch's formula); a norm that is not finite has no coefficient (None): the step is skipped"""
    total = sum(float((g.double() ** 2).sum()) for g in grads)
    norm = grad_scale * math.sqrt(total) if total == total else float("nan")
    if not math.isfinite(norm):
        return norm, None
    return norm, min(1.0, max_norm / (norm + 1e-6))


def clip_adam_model(params, moments, grads, steps, wd, grad_scale, max_norm, lr=LR):
    """one clipped step in float64.  params / grads: lists of tensors (float64 state), moments: list of (m, v), steps: the bias-correction
    index of every tensor AFTER this step (it advances on a skipped step too).  Returns (new params, new moments, norm, coef)."""
    norm, coef = norm_model(grads, grad_scale, max_norm)
    if coef is None:
        return [p.clone() for p in params], [(m.clone(), v.clone()) for m, v in moments], norm, None
    new_p, new_mv = [], []
    for p, (m, v), g, step in zip(params, moments, grads, steps):
        gi = g.double() * (grad_scale * coef) + wd * p                   # L2 decay joins AFTER clipping, as in torch
        m2, v2 = B1 * m + (1 - B1) * gi, B2 * v + (1 - B2) * gi * gi
        bc1, bc2 = 1 - B1 ** step, math.sqrt(1 - B2 ** step)
        new_p.append(p - (lr / bc1) * (m2 / (v2.sqrt() / bc2 + AEPS)))
        new_mv.append((m2, v2))
    return new_p, new_mv, norm, coef


class StatsModel:
    """state[2..6] of din_grad_norm_finish in float64: sum and maximum of the finite norms, steps measured, skipped, clipped"""

    def __init__(self):
        self.sum, self.max, self.steps, self.skipped, self.clipped = 0.0, 0.0, 0, 0, 0

    def add(self, norm, coef):
        self.steps += 1
        if coef is None:
            self.skipped += 1
            return
        self.sum, self.max = self.sum + norm, max(self.max, norm)
        self.clipped += int(coef < 1.0)


# ---- the adversarial inputs of the GPU test, each with its float64 answer ---------------------------------------------------------------
def adversarial_inputs():
    """name -> (fp32 gradient, float64 norm).  1e25: the norm is finite in fp32, a square is not.  1e-30: a square underflows fp32 to 0.
    1e4 among 2^20 ones, the large element first: an fp32 running sum stops absorbing the ones at 1e8."""
    big, tiny, n = float(np.float32(1e25)), float(np.float32(1e-30)), 8193
    spike = np.ones(2 ** 20, dtype=np.float32)
    spike[0] = 1e4
    return {"all_1e25": (np.full(n, 1e25, dtype=np.float32), big * math.sqrt(n)),
            "all_1e-30": (np.full(n, 1e-30, dtype=np.float32), tiny * math.sqrt(n)),
            "spike_1e4_in_2^20_ones": (spike, math.sqrt(1e8 + 2 ** 20 - 1))}


def fp32_accumulated_norm(g):
    """the cheap wrong variant: every square and the running sum in fp32"""
    with np.errstate(over="ignore", under="ignore"):
        sq = g.astype(np.float32) * g.astype(np.float32)
        return float(np.sqrt(np.cumsum(sq, dtype=np.float32)[-1]))


@pytest.mark.parametrize("name", sorted(adversarial_inputs()))
def test_fp32_accumulation_misses_the_norm_bar_tenfold(name):
    g, want = adversarial_inputs()[name]
    assert math.isfinite(float(np.float32(want))), "the float64 answer must be a finite fp32 number"
    got = fp32_accumulated_norm(g)
    miss = abs(got - want) / want if math.isfinite(got) else float("inf")
    print(f"{name}: fp32-accumulated norm {got:.9g}, float64 {want:.9g}, relative miss {miss:.3g} = {miss / NORM_BAR:.3g} bars")
    assert miss >= 10 * NORM_BAR


# ---- the setting ------------------------------------------------------------------------------------------------------------------------
def test_default_is_none_and_config_carries_the_field():
    from din_amd import config
    assert "max_grad_norm" in config._DEFAULTS and config._DEFAULTS["max_grad_norm"] is None
    assert config.Config("volleyball").max_grad_norm is None and config.Config("collective").max_grad_norm is None
    assert "max_grad_norm" in config.__doc__


BAD_VALUES = [0, -1.0, float("nan"), "0.1"]


@pytest.mark.parametrize("value", BAD_VALUES, ids=["zero", "negative", "nan", "not_a_number"])
@pytest.mark.parametrize("stage", [1, 2])
def test_bad_values_are_refused_before_any_loader(value, stage, monkeypatch):
    from din_amd import frame_cache, parallel, train_net as stage1, train_net_dynamic as stage2
    from din_amd.config import Config

    def too_late(*a, **k):
        raise AssertionError("the trainer went on past the max_grad_norm check")
    monkeypatch.setattr(frame_cache, "build_loaders", too_late)
    monkeypatch.setattr(parallel, "init_from_env", too_late)
    cfg = Config("volleyball")
    cfg.training_stage, cfg.max_grad_norm, cfg.backbone = stage, value, "vgg16"
    with pytest.raises(ValueError, match="max_grad_norm"):
        (stage1 if stage == 1 else stage2).train_net(cfg)


def test_accepted_values_and_the_optimizer_constructor():
    from din_amd.optim import FusedAdam, grad_norm_refusal
    for ok in (None, float("inf"), 0.1, 5, 1e-3):
        assert grad_norm_refusal(ok) is None
    for bad in BAD_VALUES + [True, -float("inf"), [1.0]]:
        assert "max_grad_norm" in grad_norm_refusal(bad)
        with pytest.raises(ValueError, match="max_grad_norm"):
            FusedAdam([torch.zeros(3, requires_grad=True)], max_grad_norm=bad)
    assert FusedAdam([torch.zeros(3)]).max_grad_norm is None
    assert FusedAdam([torch.zeros(3)], max_grad_norm=2).max_grad_norm == 2.0
    assert FusedAdam([torch.zeros(3)], max_grad_norm=2).grad_stats() == dict(steps=0, skipped=0, clipped=0, norm_mean=0.0, norm_max=0.0)


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("din_grad_sqnorm_multi", "din_grad_norm_finish", "din_adam_step_multi_clip")


def _header_arg_count(name):
    from din_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    args = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, text).group(1)
    return len([a for a in args.split(",") if a.strip() and a.strip() != "void"])


def test_the_three_entry_points_are_declared_and_bound():
    from din_amd import _lib
    import os
    symbols = _lib.header_symbols()
    for name in NEW_SYMBOLS:
        assert name in symbols and name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == _header_arg_count(name), name
    # the clipped launch takes din_adam_step_multi's arguments plus `state`, in front of the stream
    plain, clip = _lib.SIGNATURES["din_adam_step_multi"][1], _lib.SIGNATURES["din_adam_step_multi_clip"][1]
    assert clip[:len(plain) - 1] == plain[:-1] and len(clip) == len(plain) + 1
    assert _lib.ABI_VERSION == 9 and re.search(r"#define DIN_ABI_VERSION 9\b", open(_lib.HEADER_PATH).read())
    readme = open(os.path.join(os.path.dirname(_lib.HEADER_PATH), "..", "README.md")).read()
    assert int(re.search(r"\((\d+) entry points", readme).group(1)) == len(symbols)


# ---- checkpoints ------------------------------------------------------------------------------------------------------------------------
def test_state_dict_is_unchanged_by_the_setting():
    from din_amd.optim import FusedAdam
    params = [torch.zeros(4, requires_grad=True), torch.zeros(2, 3, requires_grad=True)]
    plain, clipped = FusedAdam(params, lr=1e-3), FusedAdam(params, lr=1e-3, max_grad_norm=0.5)
    for opt in (plain, clipped):
        for p in params:
            opt.state[p], opt.steps[p] = (torch.zeros_like(p), torch.zeros_like(p)), 3
    a, b = plain.state_dict(), clipped.state_dict()
    assert a.keys() == b.keys() == {"state", "param_groups"}
    assert a["param_groups"] == b["param_groups"] and "max_grad_norm" not in b["param_groups"][0]
    assert a["state"].keys() == b["state"].keys() and all(a["state"][i].keys() == b["state"][i].keys() == {"step", "exp_avg", "exp_avg_sq"}
                                                          for i in a["state"])
    ref = torch.optim.Adam([torch.nn.Parameter(p.detach().clone()) for p in params], lr=1e-3)
    ref.load_state_dict(b)                                             # torch.optim.Adam reads it
    assert set(ref.state_dict()["param_groups"][0]) >= set(b["param_groups"][0]) - {"decoupled_weight_decay"}
    clipped.load_state_dict(ref.state_dict())
    assert clipped.max_grad_norm == 0.5                                # (the setting is the constructor's, not the checkpoint's)


# ---- the restatement against torch ------------------------------------------------------------------------------------------------------
def _toy(step):
    gen = torch.Generator().manual_seed(100 + step)
    scale = 40.0 if step == 2 else 1.0                                 # step 2 is the clipped one
    return [scale * 0.05 * torch.randn(shape, generator=gen, dtype=torch.float64) for shape in ((7,), (3, 5), (33,))]


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_model_equals_clip_grad_norm_then_adam_in_float64(wd):
    max_norm = 1.0
    gen = torch.Generator().manual_seed(7)
    init = [torch.randn(shape, generator=gen, dtype=torch.float64) for shape in ((7,), (3, 5), (33,))]
    ref_p = [torch.nn.Parameter(p.clone()) for p in init]
    ref = torch.optim.Adam(ref_p, lr=LR, betas=(B1, B2), eps=AEPS, weight_decay=wd)
    p, mv = [q.clone() for q in init], [(torch.zeros_like(q), torch.zeros_like(q)) for q in init]
    clipped = []
    for step in range(1, 5):
        grads = _toy(step)
        for q, g in zip(ref_p, grads):
            q.grad = g.clone()
        torch.nn.utils.clip_grad_norm_(ref_p, max_norm, norm_type=2)
        ref.step()
        p, mv, norm, coef = clip_adam_model(p, mv, grads, [step] * 3, wd, 1.0, max_norm)
        clipped.append(coef < 1.0)
        for q, mine, (m, v) in zip(ref_p, p, mv):
            assert torch.allclose(q.detach(), mine, rtol=1e-12, atol=1e-15)
            assert torch.allclose(ref.state[q]["exp_avg"], m, rtol=1e-12, atol=1e-18)
            assert torch.allclose(ref.state[q]["exp_avg_sq"], v, rtol=1e-12, atol=1e-24)
    assert clipped == [False, True, False, False]


def test_model_grad_scale_is_the_norm_of_the_averaged_gradient():
    grads = _toy(2)
    n1, c1 = norm_model([g / 4 for g in grads], 1.0, 0.3)
    n2, c2 = norm_model(grads, 0.25, 0.3)
    assert math.isclose(n1, n2, rel_tol=1e-14) and math.isclose(c1, c2, rel_tol=1e-14) and c2 < 1.0


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_model_skips_a_non_finite_step_and_the_step_index_still_advances(bad):
    """the one addition to torch's semantics: state unchanged on a skipped step; the bias-correction index is host state and advances, so
    the step after a skipped step 2 is corrected as step 3"""
    gen = torch.Generator().manual_seed(3)
    p = [torch.randn(5, generator=gen, dtype=torch.float64), torch.randn(9, generator=gen, dtype=torch.float64)]
    mv = [(0.1 * torch.randn_like(q), torch.rand_like(q)) for q in p]
    grads = _toy(1)[:2]
    grads[0], grads[1] = grads[0][:5].clone(), grads[1].reshape(-1)[:9].clone()
    poisoned = [g.clone() for g in grads]
    poisoned[1][-1] = bad
    p2, mv2, norm, coef = clip_adam_model(p, mv, poisoned, [2, 2], 1e-2, 1.0, 1.0)
    assert coef is None and not math.isfinite(norm)
    assert all(torch.equal(a, b) for a, b in zip(p, p2)) and all(torch.equal(a[i], b[i]) for a, b in zip(mv, mv2) for i in (0, 1))
    stats = StatsModel()
    stats.add(norm, coef)
    assert (stats.steps, stats.skipped, stats.clipped, stats.sum, stats.max) == (1, 1, 0, 0.0, 0.0)
    after3, _, _, _ = clip_adam_model(p2, mv2, grads, [3, 3], 0.0, 1.0, 1.0)
    after2, _, _, _ = clip_adam_model(p2, mv2, grads, [2, 2], 0.0, 1.0, 1.0)
    assert not torch.equal(after3[0], after2[0])                       # the index the optimizer uses next is 3, and it matters


def test_fused_adam_advances_the_step_index_on_the_host():
    """FusedAdam.step() counts the step before any launch: with no gradient nothing happens, and the count is per parameter"""
    from din_amd.optim import FusedAdam
    p = torch.zeros(3, requires_grad=True)
    opt = FusedAdam([p], max_grad_norm=1.0)
    opt.step()
    assert opt.step_count == 0 and opt.state_dict()["state"] == {}
