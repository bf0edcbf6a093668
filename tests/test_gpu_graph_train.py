"""Adam with device-resident state, on the GPU: din_adam_state_advance and din_adam_step_multi_dev through the C ABI against adam_reference
(tests/test_gpu_head_path.py, per-element bars unchanged) and the float64 record model of tests/test_graph_train_cpu.py; order and
replay from a captured HIP graph; FusedAdam(capturable=True).  Every buffer a kernel writes has guard bands; gradient views start at
float offsets 0, 1, 2 and 3 from a 16-byte boundary.

Bars.  p / m / v: adam_reference's, unchanged (they allow the fp32 cancellation in 1 - beta^step that the host launches have; the
device launch forms 1 - beta^step in fp64 and rounds once, so it sits well inside them).  The record: the step count and lr exactly,
the two powers to 4 * 2^-53 relative against beta^step in float64 (the record is uploaded at step - 1 and multiplied ONCE on the
device: an ulp each for the uploaded pow, the multiply and the pow it is compared with, one to spare).  Replays against eager calls, skipped steps and refusals are exact.
Measured margins: profiles/graph_train_test_margins.txt."""
import math

import numpy as np
import pytest
import torch

from tests.conftest import Measured
from tests.test_gpu_kernels import env  # noqa: F401  (the module-scoped library fixture)
from tests.test_gpu_head_path import ADAM_MODES, AEPS, B1, B2, LR, _adam_state, _bits, _check, _gen, _refused, adam_reference
from tests.test_gpu_grad_clip import INF, _count_launches, _Table
from tests.test_grad_clip_cpu import norm_model
from tests.test_graph_train_cpu import RecordModel

SIZES = (1, 8192, 8193, 8192)              # one element, one whole chunk, a chunk and one element; gradient offsets 0, 1, 2, 3
E_ARG = -1
GUARD = -4321.5


def _contents(sizes=SIZES):
    return [tuple(t.clone() for t in _adam_state(n)) for n in sizes]


class _Rec:
    """the device record double[4] between two guard bands"""

    def __init__(self, fields):
        host = torch.full((4 + 16,), GUARD, dtype=torch.float64)
        host[8:12] = torch.tensor(fields, dtype=torch.float64)
        self.flat = host.cuda()

    def ptr(self):
        return self.flat.data_ptr() + 64

    def get(self):
        return self.flat[8:12].cpu()

    def bits(self):
        return self.flat.cpu().view(torch.int64)

    def guards_intact(self):
        flat = self.flat.cpu()
        return bool((flat[:8] == GUARD).all() and (flat[12:] == GUARD).all())


def _advance(lib, L, rec, clip=None, stream=None):
    L.check(lib.din_adam_state_advance(rec.ptr(), clip, B1, B2, stream))


def _dev(lib, L, tb, rec, wd, gs, clip=None, stream=None):
    L.check(lib.din_adam_step_multi_dev(*tb.tables(), B1, B2, AEPS, wd, gs, rec.ptr(), clip, stream))


def _power_bar(step):
    return 4 * 2.0 ** -53


def _check_record(rec, step, lr=LR):
    got = rec.get()
    e1 = Measured(abs(float(got[2]) - B1 ** step) / B1 ** step)
    e2 = Measured(abs(float(got[3]) - B2 ** step) / B2 ** step)
    print(f"record at step {step}: beta1^step rel err {float(e1):.3g}, beta2^step rel err {float(e2):.3g} (bar {_power_bar(step):.3g})")
    assert float(got[0]) == float(step) and float(got[1]) == lr and rec.guards_intact()
    assert e1 <= _power_bar(step)
    assert e2 <= _power_bar(step)


# =====================================================================================================================================
# 1. the two launches through the C ABI
# =====================================================================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize("step,wd,gs", ADAM_MODES)
def test_device_state_adam_against_fp64(env, step, wd, gs):  # noqa: F811
    """the record is uploaded at step - 1 (beta^999 computed in double for step 1000), advanced on the device, and the update is held to
    adam_reference at `step`"""
    lib, L, nhwc, ops = env
    tb = _Table(SIZES, _contents())
    rec = _Rec(RecordModel(step=step - 1).fields())
    _advance(lib, L, rec)
    _dev(lib, L, tb, rec, wd, gs)
    torch.cuda.synchronize()
    assert tb.guards_intact()
    _check_record(rec, step)
    for t, n in enumerate(SIZES):
        want = adam_reference(*_adam_state(n), step, wd, gs)
        for k, buf in (("p", tb.P[t]), ("m", tb.M[t]), ("v", tb.V[t])):
            _check(f"adam_dev[{n}, grad offset {t % 4}] step {step} wd {wd} gs {gs:.3g}", k, buf.get()[0], want[k], want["bars"][k])


@pytest.mark.gpu
@pytest.mark.parametrize("step,wd,gs", [(1, 0.0, 1.0), (1000, 0.01, 1.0 / 128)])
def test_device_state_adam_behind_a_clip(env, step, wd, gs):  # noqa: F811
    lib, L, nhwc, ops = env
    tb = _Table(SIZES, _contents())
    base = norm_model([c[1] for c in _contents()], gs, INF)[0]
    tb.norm(lib, L, gs, 0.5 * base)
    rec = _Rec(RecordModel(step=step - 1).fields())
    _advance(lib, L, rec, tb.state.ptr())
    _dev(lib, L, tb, rec, wd, gs, tb.state.ptr())
    st = tb.st()
    assert 0.4 < float(st[1]) < 0.6 and tb.guards_intact()
    _check_record(rec, step)
    gs_eff = float(np.float32(gs) * np.float32(float(st[1])))          # the ONE factor the launch forms
    for t, n in enumerate(SIZES):
        want = adam_reference(*_adam_state(n), step, wd, gs_eff)
        for k, buf in (("p", tb.P[t]), ("m", tb.M[t]), ("v", tb.V[t])):
            _check(f"adam_dev clipped [{n}] step {step} wd {wd} gs {gs:.3g}", k, buf.get()[0], want[k], want["bars"][k])


@pytest.mark.gpu
def test_unclipped_device_state_launch_gives_the_bits_of_the_launch_without_a_clip_state(env):  # noqa: F811
    lib, L, nhwc, ops = env
    a, b = _Table(SIZES, _contents()), _Table(SIZES, _contents())
    ra, rb = _Rec(RecordModel(step=6).fields()), _Rec(RecordModel(step=6).fields())
    a.norm(lib, L, 0.5, INF)
    _advance(lib, L, ra, a.state.ptr()), _dev(lib, L, a, ra, 0.01, 0.5, a.state.ptr())
    _advance(lib, L, rb), _dev(lib, L, b, rb, 0.01, 0.5)
    assert float(a.st()[1]) == 1.0
    assert all(torch.equal(x, y) for x, y in zip(a.pmv_bits(), b.pmv_bits())) and torch.equal(ra.bits(), rb.bits())


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [float("nan"), INF], ids=["nan", "inf"])
def test_a_non_finite_norm_changes_no_byte(env, bad):  # noqa: F811
    lib, L, nhwc, ops = env
    contents = _contents()
    contents[2][1][-1] = bad                                            # the one-element tail of the last chunk of the 8193 tensor
    tb = _Table(SIZES, contents)
    rec = _Rec(RecordModel(step=2).fields())
    before = rec.bits().clone()
    tb.norm(lib, L, 1.0, 1.0)
    _advance(lib, L, rec, tb.state.ptr())
    _dev(lib, L, tb, rec, 0.01, 1.0, tb.state.ptr())
    st = tb.st()
    assert not math.isfinite(float(st[0])) and float(st[1]) == 0.0 and float(st[5]) == 1.0
    assert tb.guards_intact() and all(b.unchanged() for b in tb.P + tb.M + tb.V + tb.G)
    assert torch.equal(rec.bits(), before)


@pytest.mark.gpu
def test_refusals_touch_nothing(env):  # noqa: F811
    lib, L, nhwc, ops = env
    tb = _Table(SIZES, _contents())
    rec = _Rec(RecordModel(step=3).fields())
    before = rec.bits().clone()
    ptrs, sz, ct, ci, nch, chunk = tb.tables()
    o, state = rec.ptr(), tb.state.ptr()
    adv, dev = lib.din_adam_state_advance, lib.din_adam_step_multi_dev
    hyper, nan = (B1, B2, AEPS, 0.0), float("nan")
    refused = [
        (adv(None, None, B1, B2, None), "adam_state_advance"), (adv(o + 4, None, B1, B2, None), "8-byte"),
        (adv(o, state + 2, B1, B2, None), "4-byte"), (adv(o, None, 1.0, B2, None), "betas"), (adv(o, None, B1, -0.1, None), "betas"),
        (adv(o, None, nan, B2, None), "betas"),
        (dev(None, sz, ct, ci, nch, chunk, *hyper, 1.0, o, None, None), "adam_step_multi_dev"),
        (dev(ptrs, None, ct, ci, nch, chunk, *hyper, 1.0, o, None, None), "adam_step_multi_dev"),
        (dev(ptrs, sz, None, ci, nch, chunk, *hyper, 1.0, o, None, None), "adam_step_multi_dev"),
        (dev(ptrs, sz, ct, None, nch, chunk, *hyper, 1.0, o, None, None), "adam_step_multi_dev"),
        (dev(ptrs, sz, ct, ci, -1, chunk, *hyper, 1.0, o, None, None), "adam_step_multi_dev"),
        (dev(ptrs, sz, ct, ci, nch, 0, *hyper, 1.0, o, None, None), "adam_step_multi_dev"),
        (dev(ptrs, sz, ct, ci, nch, chunk, *hyper, 1.0, None, None, None), "adam_step_multi_dev"),
        (dev(ptrs, sz, ct, ci, nch, chunk, *hyper, 1.0, o + 4, None, None), "8-byte"),
        (dev(ptrs, sz, ct, ci, nch, chunk, *hyper, 1.0, o, state + 2, None), "4-byte"),
        (dev(ptrs, sz, ct, ci, nch, chunk, *hyper, INF, o, None, None), "grad_scale"),
        (dev(ptrs, sz, ct, ci, nch, chunk, *hyper, nan, o, None, None), "grad_scale"),
    ]
    torch.cuda.synchronize()
    for rc, _ in refused:
        assert rc == E_ARG
    _refused(adv(o + 4, None, B1, B2, None), "8-byte")
    _refused(dev(ptrs, sz, ct, ci, nch, chunk, *hyper, 1.0, o + 4, None, None), "8-byte")
    _refused(dev(ptrs, sz, ct, ci, nch, chunk, *hyper, nan, o, None, None), "grad_scale")
    _refused(dev(ptrs, sz, ct, ci, nch, chunk, *hyper, 1.0, o, state + 2, None), "4-byte")
    torch.cuda.synchronize()
    assert torch.equal(rec.bits(), before) and tb.state.unchanged() and all(b.unchanged() for b in tb.P + tb.G + tb.M + tb.V)
    assert dev(ptrs, sz, ct, ci, 0, chunk, *hyper, 1.0, o, None, None) == 0          # an empty table is no refusal and no launch
    torch.cuda.synchronize()
    assert torch.equal(rec.bits(), before) and all(b.unchanged() for b in tb.P + tb.G + tb.M + tb.V)


# =====================================================================================================================================
# 2. order and replay
# =====================================================================================================================================
SEQ_SIZES = (257, 8193)


def _seq_contents():
    return _contents(SEQ_SIZES)


def _seq_grads(k):
    return [(1.0 + 0.5 * k) * torch.randn(n, generator=_gen(f"seq{k}-{n}")) for n in SEQ_SIZES]


def _load_grads(tb, grads):
    for t, g in enumerate(grads):
        tb.G[t].view.copy_(g.cuda())


def _result(tb, rec):
    torch.cuda.synchronize()
    return tb.pmv_bits() + [rec.bits().clone()]


def _eager_sequence(lib, L, steps=3, lr_at=None):
    tb, rec = _Table(SEQ_SIZES, _seq_contents()), _Rec(RecordModel().fields())
    out = []
    for k in range(steps):
        if lr_at is not None and k == lr_at[0]:
            rec.flat[9:10].copy_(torch.tensor([lr_at[1]], dtype=torch.float64))
        _load_grads(tb, _seq_grads(k))
        _advance(lib, L, rec), _dev(lib, L, tb, rec, 0.01, 1.0)
        out.append(_result(tb, rec))
    return out


@pytest.mark.gpu
def test_five_call_sequences_give_the_same_bits(env):  # noqa: F811
    lib, L, nhwc, ops = env
    runs = [_eager_sequence(lib, L) for _ in range(5)]
    for run in runs[1:]:
        assert all(torch.equal(a, b) for sa, sb in zip(run, runs[0]) for a, b in zip(sa, sb))
    assert float(runs[0][-1][-1].view(torch.float64)[8]) == 3.0


@pytest.mark.gpu
def test_three_replays_equal_three_eager_calls(env):  # noqa: F811
    """advance + step captured ONCE: every replay is the next step -- count, bias corrections, p, m, v and the record bit for bit what
    three eager calls give.  (A captured din_adam_step_multi replays the step count it was captured with.)"""
    lib, L, nhwc, ops = env
    eager = _eager_sequence(lib, L)
    tb, rec = _Table(SEQ_SIZES, _seq_contents()), _Rec(RecordModel().fields())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st = torch.cuda.current_stream().cuda_stream
        _advance(lib, L, rec, None, st), _dev(lib, L, tb, rec, 0.01, 1.0, None, st)
    torch.cuda.synchronize()
    assert float(rec.get()[0]) == 0.0                                   # (the capture ran nothing)
    for k, want in enumerate(eager):
        _load_grads(tb, _seq_grads(k))
        graph.replay()
        assert all(torch.equal(a, b) for a, b in zip(_result(tb, rec), want)), k
    assert all(b.untouched_outside() for b in tb.P + tb.G + tb.M + tb.V) and rec.guards_intact() and float(rec.get()[0]) == 3.0
    # the launch it replaces, captured at step 1, stays at step 1: its third replay is not the third eager step
    plain, frozen = _Table(SEQ_SIZES, _seq_contents()), _Table(SEQ_SIZES, _seq_contents())
    for k in range(3):
        _load_grads(plain, _seq_grads(k))
        plain.adam_plain(lib, L, k + 1, 0.01, 1.0)
    torch.cuda.synchronize()
    graph2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph2):
        L.check(lib.din_adam_step_multi(*frozen.tables(), LR, B1, B2, AEPS, 0.01, 1, 1.0, torch.cuda.current_stream().cuda_stream))
    for k in range(3):
        _load_grads(frozen, _seq_grads(k))
        graph2.replay()
    torch.cuda.synchronize()
    assert not all(torch.equal(a, b) for a, b in zip(frozen.pmv_bits(), plain.pmv_bits()))


@pytest.mark.gpu
def test_a_learning_rate_change_between_replays_needs_no_recapture(env):  # noqa: F811
    lib, L, nhwc, ops = env
    new_lr = float(np.float32(3e-5))
    eager = _eager_sequence(lib, L, lr_at=(2, new_lr))
    assert not all(torch.equal(a, b) for a, b in zip(eager[2], _eager_sequence(lib, L)[2]))
    tb, rec = _Table(SEQ_SIZES, _seq_contents()), _Rec(RecordModel().fields())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st = torch.cuda.current_stream().cuda_stream
        _advance(lib, L, rec, None, st), _dev(lib, L, tb, rec, 0.01, 1.0, None, st)
    for k, want in enumerate(eager):
        if k == 2:
            rec.flat[9:10].copy_(torch.tensor([new_lr], dtype=torch.float64))     # a small eager copy, outside the graph
        _load_grads(tb, _seq_grads(k))
        graph.replay()
        assert all(torch.equal(a, b) for a, b in zip(_result(tb, rec), want)), k
    assert float(rec.get()[1]) == new_lr


# =====================================================================================================================================
# 3. FusedAdam(capturable=True)
# =====================================================================================================================================
TOY = ((5,), (300, 3), (8200,), (70,))          # the last one gets its first gradient at step 2: two step-count groups


def _toy_grads(step, poison_at=None):
    gen = _gen(f"graph-toy{step}")
    grads = [0.01 * torch.randn(shape, generator=gen) for shape in TOY]
    if step == poison_at:
        grads[1][17, 1] = float("nan")
    return grads[:3] + [grads[3] if step >= 2 else None]


def _snapshot(opt, params, live):
    out = {}
    for i in live:
        m, v = opt.state.get(params[i], (torch.zeros(TOY[i]), torch.zeros(TOY[i])))
        out[i] = (params[i].detach().cpu().clone().reshape(-1), m.cpu().clone().reshape(-1), v.cpu().clone().reshape(-1))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("wd,gs", [(0.0, 1.0), (1e-4, 0.5)])
def test_capturable_fused_adam_against_adam_reference(env, monkeypatch, wd, gs):  # noqa: F811
    """four steps over two step-count groups, each checked from the stored fp32 state before it; the launches are the two new ones,
    per group, and nothing is read back"""
    from din_amd.optim import FusedAdam
    lib, L, nhwc, ops = env
    gen = _gen("graph_toy_params")
    params = [torch.randn(shape, generator=gen).cuda().requires_grad_(True) for shape in TOY]
    opt = FusedAdam(params, lr=LR, betas=(B1, B2), eps=AEPS, weight_decay=wd, capturable=True)
    calls = _count_launches(monkeypatch, lib, L)
    for step in range(1, 5):
        grads = _toy_grads(step)
        for p, g in zip(params, grads):
            p.grad = None if g is None else g.cuda()
        live = [i for i, g in enumerate(grads) if g is not None]
        before = _snapshot(opt, params, live)
        del calls[:]
        opt.step(grad_scale=gs)
        groups = 1 if step == 1 else 2
        assert calls == ["din_adam_state_advance", "din_adam_step_multi_dev"] * groups
        torch.cuda.synchronize()
        for i in live:
            index = step if i < 3 else step - 1                          # (the late tensor's own record counts from its first gradient)
            want = adam_reference(before[i][0], grads[i].reshape(-1), before[i][1], before[i][2], index, wd, gs)
            got = dict(p=params[i].detach().cpu(), m=opt.state[params[i]][0].cpu(), v=opt.state[params[i]][1].cpu())
            for k in "pmv":
                _check(f"FusedAdam(capturable) step {step} tensor {i}", k, got[k].reshape(-1), want[k], want["bars"][k])
    monkeypatch.undo()
    assert opt.step_count == 4 and not opt.steps
    steps = {i: float(st["step"]) for i, st in opt.state_dict()["state"].items()}
    assert steps == {0: 4.0, 1: 4.0, 2: 4.0, 3: 3.0}


@pytest.mark.gpu
def test_capturable_state_dict_round_trip_through_torch_adam(env):  # noqa: F811
    from din_amd.optim import FusedAdam
    lib, L, nhwc, ops = env
    gen = _gen("graph_roundtrip")
    values = [torch.randn(shape, generator=gen) for shape in TOY]

    def fresh():
        params = [v.clone().cuda().requires_grad_(True) for v in values]
        return params, FusedAdam(params, lr=LR, betas=(B1, B2), eps=AEPS, weight_decay=1e-4, capturable=True)

    def run(params, opt, steps):
        for step in steps:
            for p, g in zip(params, _toy_grads(step)):
                p.grad = None if g is None else g.cuda()
            opt.step()
        torch.cuda.synchronize()

    pa, a = fresh()
    run(pa, a, (1, 2, 3, 4))
    pb, b = fresh()
    run(pb, b, (1, 2))
    sd = b.state_dict()
    assert sd.keys() == {"state", "param_groups"} and all(sd["state"][i].keys() == {"step", "exp_avg", "exp_avg_sq"} for i in sd["state"])
    assert [float(sd["state"][i]["step"]) for i in range(4)] == [2.0, 2.0, 2.0, 1.0]
    ref_params = [torch.nn.Parameter(p.detach().clone()) for p in pb]
    ref = torch.optim.Adam(ref_params, lr=LR, betas=(B1, B2), eps=AEPS, weight_decay=1e-4)
    ref.load_state_dict(sd)                                              # torch.optim.Adam reads it ...
    pc = [p.detach().clone().requires_grad_(True) for p in pb]
    c = FusedAdam(pc, lr=1.0, capturable=True)
    c.load_state_dict(ref.state_dict())                                  # ... and what it writes comes back: lr, moments and both counts
    assert c.param_groups[0]["lr"] == LR and c.step_count == 2
    run(pc, c, (3, 4))
    for x, y in zip(pa, pc):                                             # the resumed run continues the uninterrupted one bit for bit
        assert torch.equal(_bits(x.detach().cpu()), _bits(y.detach().cpu()))
        assert all(torch.equal(_bits(s.cpu()), _bits(t.cpu())) for s, t in zip(a.state[x], c.state[y]))
    assert [float(st["step"]) for st in c.state_dict()["state"].values()] == [4.0, 4.0, 4.0, 3.0]
    # a record resumed at step 1000 holds beta^1000 computed in double
    big = ref.state_dict()
    for st in big["state"].values():
        st["step"] = torch.tensor(1000.0)
    c.load_state_dict(big)
    rec = next(iter(c._records.values())).dev.cpu()
    assert float(rec[0]) == 1000.0 and float(rec[2]) == B1 ** 1000 and float(rec[3]) == B2 ** 1000


@pytest.mark.gpu
def test_capturable_skipped_step_does_not_count(env):  # noqa: F811
    """max_grad_norm set, the gradient of step 2 holds a NaN: weights, moments and the record keep their bits, grad_stats counts the skip,
    and step 3 is corrected as the SECOND step (the host-side optimizer corrects it as the third)"""
    from din_amd.optim import FusedAdam
    lib, L, nhwc, ops = env
    gen = _gen("graph_skip")
    shapes = TOY[:3]
    params = [torch.randn(shape, generator=gen).cuda().requires_grad_(True) for shape in shapes]
    opt = FusedAdam(params, lr=LR, betas=(B1, B2), eps=AEPS, max_grad_norm=1e6, capturable=True)
    for step in (1, 2, 3):
        grads = _toy_grads(step, poison_at=2)[:3]
        for p, g in zip(params, grads):
            p.grad = g.cuda()
        before = [(p.detach().cpu().clone().reshape(-1),) + tuple(t.cpu().clone().reshape(-1) for t in opt.state.get(p, (torch.zeros_like(p),) * 2))
                  for p in params]
        rec_before = None if step == 1 else next(iter(opt._records.values())).dev.cpu().view(torch.int64).clone()
        opt.step()
        torch.cuda.synchronize()
        if step == 2:
            for p, (p0, m0, v0) in zip(params, before):
                assert torch.equal(_bits(p.detach().cpu().reshape(-1)), _bits(p0))
                assert torch.equal(_bits(opt.state[p][0].cpu().reshape(-1)), _bits(m0)) and torch.equal(_bits(opt.state[p][1].cpu().reshape(-1)), _bits(v0))
            assert torch.equal(next(iter(opt._records.values())).dev.cpu().view(torch.int64), rec_before)
            continue
        index = {1: 1, 3: 2}[step]
        for i, (p, (p0, m0, v0)) in enumerate(zip(params, before)):
            want = adam_reference(p0, grads[i].reshape(-1), m0, v0, index, 0.0, 1.0)
            for k, got in (("p", p.detach().cpu()), ("m", opt.state[p][0].cpu()), ("v", opt.state[p][1].cpu())):
                _check(f"skip: step {step} corrected as {index}, tensor {i}", k, got.reshape(-1), want[k], want["bars"][k])
        if step == 3:                                                    # ... and the host-side index (3) is outside the bars
            wrong = adam_reference(*before[2][:1], grads[2].reshape(-1), before[2][1], before[2][2], 3, 0.0, 1.0)
            miss = float(((params[2].detach().cpu().reshape(-1).double() - wrong["p"]).abs() / wrong["bars"]["p"]).max())
            print(f"skip: step 3 against the bias correction of index 3: {miss:.3g} bars")
            assert miss >= 10.0
    stats = opt.grad_stats()
    assert (stats["steps"], stats["skipped"], stats["clipped"]) == (3, 1, 0) and opt.step_count == 2
