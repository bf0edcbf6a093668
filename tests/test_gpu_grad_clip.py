"""Global gradient-norm clipping inside the fused Adam step, on the GPU: din_grad_sqnorm_multi, din_grad_norm_finish and
din_adam_step_multi_clip through the C ABI against the float64 model of tests/test_grad_clip_cpu.py, then FusedAdam(max_grad_norm=...)
and both trainers.  Every buffer a kernel writes has guard bands; gradient views start at float offsets 0, 1, 2 and 3 from a 16-byte
boundary.

Bars.  state[0] (norm): relative 2^-22 -- the final fp32 rounding is 2^-24 and the fp64 sum adds at most n * 2^-53 (2e-12 at these
sizes), so about 4x is left.  state[1] (coef): relative 2^-21, the norm's bar plus one fp32 add and one fp32 divide.  The running sum
state[2] of k finite norms: each term 2^-24 and k - 1 fp32 adds of at most 2^-24 of the sum each: (2 k - 1) * 2^-24 (k = 3 here);
state[3] is one of the norms: the norm's bar.  Clipped Adam: the per-element bars of tests/test_gpu_head_path.py (adam_reference) unchanged, with
float32(grad_scale * coef) -- coef as the finish launch stored it -- in place of grad_scale.  Bit identity, the skip and the repeats
are exact.  Measured margins: profiles/grad_clip_test_margins.txt."""
import functools
import math

import numpy as np
import pytest
import torch

from tests.conftest import Measured
from tests.test_gpu_kernels import env  # noqa: F401  (the module-scoped library fixture)
from tests.test_gpu_head_path import AEPS, B1, B2, LR, _bits, _Buf, _check, _gen, _refused, adam_reference
from tests.test_grad_clip_cpu import COEF_BAR, NORM_BAR, StatsModel, adversarial_inputs, norm_model

CHUNK = 8192
SIZES = (1, 255, 256, 257, 8191, 8192, 8193, 2 * 8192 + 3)
INF = float("inf")
E_ARG = -1


def sum_bar(k):
    return (2 * k - 1) * 2.0 ** -24


def _rel(got, want):
    return Measured(abs(float(got) - want) / abs(want))


class _F64:
    """`n` doubles between two guard bands (tests/test_gpu_head_path._Buf holds 4-byte types only)"""

    def __init__(self, n, guard=-4321.5):
        self.n, self.guard = n, guard
        self.flat = torch.full((n + 16,), guard, dtype=torch.float64).cuda()

    def ptr(self):
        return self.flat.data_ptr() + 8 * 8

    def get(self):
        return self.flat[8:8 + self.n].cpu()

    def untouched_outside(self):
        flat = self.flat.cpu()
        return bool((flat[:8] == self.guard).all() and (flat[8 + self.n:] == self.guard).all())

    def unchanged(self):
        return bool((self.flat.cpu() == self.guard).all())


class _Table:
    """the device tables of din_adam_step_multi over `sizes`: tensor t's gradient view starts t % 4 floats past a 16-byte boundary (a
    view into a bucket); p, m, v are ordinary buffers"""

    def __init__(self, sizes, contents, chunk=CHUNK, state=None):
        self.sizes, self.chunk = tuple(sizes), chunk
        self.P, self.G, self.M, self.V = [], [], [], []
        for t, (n, (p, g, m, v)) in enumerate(zip(sizes, contents)):
            self.P.append(_Buf((1,), n, content=p))
            self.G.append(_Buf((1,), n, content=g, ld=n + 4, off=t % 4))
            self.M.append(_Buf((1,), n, content=m))
            self.V.append(_Buf((1,), n, content=v))
            assert self.G[-1].view.data_ptr() % 16 == 4 * (t % 4)
        rows = [[P.ptr(), G.view.data_ptr(), M.ptr(), V.ptr()] for P, G, M, V in zip(self.P, self.G, self.M, self.V)]
        self.ptrs = torch.tensor(rows, dtype=torch.int64).cuda()
        ct, ci = zip(*[(t, i) for t, n in enumerate(sizes) for i in range(-(-n // chunk))])
        self.nchunks = len(ct)
        self.sz, self.ct, self.ci = (torch.tensor(v, dtype=dt).cuda() for v, dt in ((sizes, torch.int64), (ct, torch.int32), (ci, torch.int32)))
        self.partials = _F64(self.nchunks)
        self.state = _Buf((1,), 8, content=torch.zeros(8) if state is None else torch.tensor(state, dtype=torch.float32))

    def tables(self):
        return self.ptrs.data_ptr(), self.sz.data_ptr(), self.ct.data_ptr(), self.ci.data_ptr(), self.nchunks, self.chunk

    def norm(self, lib, L, gs, max_norm, stream=None):
        L.check(lib.din_grad_sqnorm_multi(*self.tables(), self.partials.ptr(), stream))
        L.check(lib.din_grad_norm_finish(self.partials.ptr(), self.nchunks, gs, max_norm, self.state.ptr(), stream))

    def adam_clip(self, lib, L, step, wd, gs, stream=None):
        L.check(lib.din_adam_step_multi_clip(*self.tables(), LR, B1, B2, AEPS, wd, step, gs, self.state.ptr(), stream))

    def adam_plain(self, lib, L, step, wd, gs):
        L.check(lib.din_adam_step_multi(*self.tables(), LR, B1, B2, AEPS, wd, step, gs, None))

    def st(self):
        torch.cuda.synchronize()
        return self.state.get()[0]

    def guards_intact(self):
        return (all(b.untouched_outside() for b in self.P + self.M + self.V) and all(b.unchanged() for b in self.G)
                and self.partials.untouched_outside() and self.state.untouched_outside())

    def pmv_bits(self):
        return [_bits(b.get()) for bufs in (self.P, self.M, self.V) for b in bufs]


@functools.lru_cache(maxsize=None)
def _contents(scale=1.0):
    out = []
    for n in SIZES:
        gen = _gen(f"clip{n}")
        p, g, m, v = torch.randn(n, generator=gen), scale * torch.randn(n, generator=gen), 0.1 * torch.randn(n, generator=gen), torch.rand(n, generator=gen) ** 2
        g[::5] = 0.0
        out.append((p, g, m, v))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _norm64(scale=1.0):
    return norm_model([c[1] for c in _contents(scale)], 1.0, INF)[0]


# =====================================================================================================================================
# 1. the kernels through the C ABI
# =====================================================================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize("gs", [1.0, 0.5])
@pytest.mark.parametrize("max_rel", [INF, 4.0, 0.5, 1e-3], ids=["inf", "above", "half", "tiny"])
def test_norm_and_coefficient_against_fp64(env, gs, max_rel):  # noqa: F811
    lib, L, nhwc, ops = env
    tb = _Table(SIZES, _contents())
    max_norm = max_rel if max_rel == INF else max_rel * _norm64() * gs
    norm, coef = norm_model([c[1] for c in _contents()], gs, max_norm)
    tb.norm(lib, L, gs, max_norm)
    st = tb.st()
    assert tb.guards_intact() and all(b.unchanged() for b in tb.P + tb.M + tb.V)
    e_norm, e_coef = _rel(st[0], norm), _rel(st[1], coef)
    print(f"norm gs {gs} max {max_rel}: rel err {float(e_norm):.3g} (bar {NORM_BAR:.3g}); coef rel err {float(e_coef):.3g} (bar {COEF_BAR:.3g})")
    assert e_norm <= NORM_BAR
    assert e_coef <= COEF_BAR
    assert (float(st[1]) < 1.0) == (coef < 1.0)
    want_tail = [float(st[0]), float(st[0]), 1.0, 0.0, float(coef < 1.0), 0.0]
    assert [float(x) for x in st[2:]] == want_tail
    part = tb.partials.get()
    want = torch.tensor([float((c[1][i * CHUNK:(i + 1) * CHUNK].double() ** 2).sum()) for c in _contents() for i in range(-(-c[1].numel() // CHUNK))],
                        dtype=torch.float64)
    e_part = Measured(float(((part - want).abs() / want.clamp_min(1e-300)).max()))
    assert e_part <= CHUNK * 2.0 ** -53                                # n roundings of an fp64 sum of n positive terms


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(adversarial_inputs()))
def test_adversarial_inputs_against_fp64(env, name):  # noqa: F811
    lib, L, nhwc, ops = env
    g, want = adversarial_inputs()[name]
    g = torch.from_numpy(g)
    z = torch.zeros_like(g)
    tb = _Table((g.numel(),), ((z, g, z, z),))
    tb.norm(lib, L, 1.0, INF)
    st = tb.st()
    err = _rel(st[0], want)
    print(f"{name}: norm {float(st[0]):.9g}, float64 {want:.9g}, rel err {float(err):.3g} (bar {NORM_BAR:.3g})")
    assert err <= NORM_BAR
    assert float(st[1]) == 1.0 and float(st[5]) == 0.0 and tb.guards_intact()


ADAM_MODES = [(step, wd, gs) for step in (1, 1000) for wd in (0.0, 1e-4) for gs in (1.0, 0.5)]


@pytest.mark.gpu
@pytest.mark.parametrize("step,wd,gs", ADAM_MODES)
def test_clipped_adam_against_fp64(env, step, wd, gs):  # noqa: F811
    lib, L, nhwc, ops = env
    tb = _Table(SIZES, _contents())
    tb.norm(lib, L, gs, 0.5 * _norm64() * gs)
    tb.adam_clip(lib, L, step, wd, gs)
    st = tb.st()
    assert 0.4 < float(st[1]) < 0.6 and tb.guards_intact()
    gs_eff = float(np.float32(gs) * np.float32(float(st[1])))          # the ONE factor the launch forms
    for t, (n, c) in enumerate(zip(SIZES, _contents())):
        want = adam_reference(*c, step, wd, gs_eff)
        for k, buf in (("p", tb.P[t]), ("m", tb.M[t]), ("v", tb.V[t])):
            _check(f"adam_clip[{n}] step {step} wd {wd} gs {gs}", k, buf.get()[0], want[k], want["bars"][k])
        assert not torch.equal(_bits(tb.P[t].get()[0]), _bits(c[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("max_rel", [INF, 2.0], ids=["inf", "above_the_norm"])
@pytest.mark.parametrize("step,wd,gs", [(1, 0.0, 1.0), (1000, 1e-4, 0.5)])
def test_unclipped_launch_gives_the_bits_of_the_plain_launch(env, max_rel, step, wd, gs):  # noqa: F811
    lib, L, nhwc, ops = env
    a, b = _Table(SIZES, _contents()), _Table(SIZES, _contents())
    a.norm(lib, L, gs, max_rel if max_rel == INF else max_rel * _norm64() * gs)
    a.adam_clip(lib, L, step, wd, gs)
    b.adam_plain(lib, L, step, wd, gs)
    assert float(a.st()[1]) == 1.0 and a.guards_intact()
    assert all(torch.equal(x, y) for x, y in zip(a.pmv_bits(), b.pmv_bits()))
    assert not any(torch.equal(x[0], _bits(c[0])) for x, c in zip(a.pmv_bits(), _contents()))       # (every p moved)


@pytest.mark.gpu
@pytest.mark.parametrize("where,bad", [("last_of_ragged_tail", float("nan")), ("first", INF)])
def test_non_finite_gradient_skips_the_step(env, where, bad):  # noqa: F811
    lib, L, nhwc, ops = env
    contents = [tuple(t.clone() for t in c) for c in _contents()]
    if where == "first":
        contents[0][1][0] = bad
    else:
        contents[-1][1][-1] = bad                                       # element 2 of the 3-element tail of the last chunk
    before = [3.5, 2.25, 4.0, 1.0, 2.0]
    tb = _Table(SIZES, contents, state=[9.0, 9.0] + before + [9.0])
    tb.norm(lib, L, 1.0, 1.0)
    tb.adam_clip(lib, L, 3, 1e-4, 1.0)
    st = tb.st()
    assert not math.isfinite(float(st[0])) and float(st[1]) == 0.0
    assert [float(x) for x in st[2:]] == [3.5, 2.25, 5.0, 2.0, 2.0, 0.0]
    assert tb.guards_intact() and all(b.unchanged() for b in tb.P + tb.M + tb.V)


@pytest.mark.gpu
def test_four_step_sequence_keeps_the_running_statistics(env):  # noqa: F811
    """normal, clipped, skipped, normal on one state word"""
    lib, L, nhwc, ops = env
    base = _norm64()
    plan = [(1.0, None), (40.0, None), (1.0, float("nan")), (0.5, None)]
    model, tb0 = StatsModel(), _Table(SIZES, _contents())
    state = tb0.state
    for scale, poison in plan:
        contents = [tuple(t.clone() for t in c) for c in _contents(scale)]
        if poison is not None:
            contents[3][1][7] = poison
        tb = _Table(SIZES, contents)
        tb.state = state
        tb.norm(lib, L, 1.0, 2.0 * base)
        tb.adam_clip(lib, L, 1, 0.0, 1.0)
        torch.cuda.synchronize()
        model.add(*norm_model([c[1] for c in contents], 1.0, 2.0 * base))
        assert tb.guards_intact()
    st = state.get()[0]
    assert (model.steps, model.skipped, model.clipped) == (4, 1, 1)
    assert [float(x) for x in st[4:]] == [4.0, 1.0, 1.0, 0.0]
    e_sum, e_max = _rel(st[2], model.sum), _rel(st[3], model.max)
    print(f"sequence: running sum rel err {float(e_sum):.3g} (bar {sum_bar(3):.3g}), running max rel err {float(e_max):.3g} (bar {NORM_BAR:.3g})")
    assert e_sum <= sum_bar(3)
    assert e_max <= NORM_BAR


@pytest.mark.gpu
def test_five_calls_give_the_same_bits(env):  # noqa: F811
    lib, L, nhwc, ops = env
    n = 2 ** 20
    g = torch.randn(n, generator=_gen("repeat"))
    z = torch.zeros(n)
    tb = _Table((n,), ((z, g, z, z),))
    seen = []
    for _ in range(5):
        tb.partials.flat.fill_(tb.partials.guard)
        tb.norm(lib, L, 1.0, INF)
        torch.cuda.synchronize()
        seen.append((_bits(tb.state.get()[0][:1]).clone(), tb.partials.get().view(torch.int64).clone()))
    assert all(torch.equal(s[0], seen[0][0]) and torch.equal(s[1], seen[0][1]) for s in seen)
    assert _rel(tb.st()[0], norm_model([g], 1.0, INF)[0]) <= NORM_BAR
    assert float(tb.st()[4]) == 5.0


@pytest.mark.gpu
def test_the_three_launches_replay_from_a_captured_graph(env):  # noqa: F811
    """one stream, no parallel branch; the gradient contents change between the replays, and each replay gives the bits of the direct
    calls on the same contents"""
    lib, L, nhwc, ops = env
    sizes = (257, 8193)
    cont = [c for n, c in zip(SIZES, _contents()) if n in sizes]
    grads = [[c[1] for c in cont], [3.0 * c[1].flip(0) for c in cont]]
    max_norm = 1.5 * norm_model(grads[0], 1.0, INF)[0]                 # the first contents pass, the second are clipped

    def load(tb, gr):
        for t, c in enumerate(cont):
            tb.P[t].view.copy_(c[0].cuda()), tb.M[t].view.copy_(c[2].cuda()), tb.V[t].view.copy_(c[3].cuda())
            tb.G[t].view.copy_(gr[t].cuda())
        tb.state.view.zero_()

    def result(tb):
        torch.cuda.synchronize()
        return tb.pmv_bits() + [_bits(tb.state.get())]

    eager = []
    for gr in grads:
        tb = _Table(sizes, cont)
        load(tb, gr)
        tb.norm(lib, L, 1.0, max_norm)
        tb.adam_clip(lib, L, 2, 1e-4, 1.0)
        eager.append(result(tb))
    assert float(eager[0][-1].view(torch.float32)[0, 1]) == 1.0 and float(eager[1][-1].view(torch.float32)[0, 1]) < 1.0
    tb = _Table(sizes, cont)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st = torch.cuda.current_stream().cuda_stream
        tb.norm(lib, L, 1.0, max_norm, st)
        tb.adam_clip(lib, L, 2, 1e-4, 1.0, st)
    for gr, want in zip(grads, eager):
        load(tb, gr)
        graph.replay()
        got = result(tb)
        assert all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.gpu
def test_refusals_touch_nothing(env):  # noqa: F811
    lib, L, nhwc, ops = env
    tb = _Table((257, 8193), [c for n, c in zip(SIZES, _contents()) if n in (257, 8193)])
    ptrs, sz, ct, ci, nch, chunk = tb.tables()
    part, state = tb.partials.ptr(), tb.state.ptr()
    sq, fin, clip = lib.din_grad_sqnorm_multi, lib.din_grad_norm_finish, lib.din_adam_step_multi_clip
    adam = (LR, B1, B2, AEPS, 0.0, 1, 1.0)
    nan = float("nan")
    refused = [
        (sq(None, sz, ct, ci, nch, chunk, part, None), "grad_sqnorm_multi"), (sq(ptrs, None, ct, ci, nch, chunk, part, None), "grad_sqnorm_multi"),
        (sq(ptrs, sz, None, ci, nch, chunk, part, None), "grad_sqnorm_multi"), (sq(ptrs, sz, ct, None, nch, chunk, part, None), "grad_sqnorm_multi"),
        (sq(ptrs, sz, ct, ci, nch, chunk, None, None), "grad_sqnorm_multi"), (sq(ptrs, sz, ct, ci, -1, chunk, part, None), "grad_sqnorm_multi"),
        (sq(ptrs, sz, ct, ci, nch, 0, part, None), "grad_sqnorm_multi"), (sq(ptrs, sz, ct, ci, nch, -8, part, None), "grad_sqnorm_multi"),
        (sq(ptrs, sz, ct, ci, nch, chunk, part + 4, None), "8-byte"),
        (fin(None, nch, 1.0, 1.0, state, None), "grad_norm_finish"), (fin(part, nch, 1.0, 1.0, None, None), "grad_norm_finish"),
        (fin(part, -1, 1.0, 1.0, state, None), "grad_norm_finish"), (fin(part + 4, nch, 1.0, 1.0, state, None), "8-byte"),
        (fin(part, nch, 1.0, 1.0, state + 2, None), "4-byte"), (fin(part, nch, 1.0, 0.0, state, None), "max_norm"),
        (fin(part, nch, 1.0, -1.0, state, None), "max_norm"), (fin(part, nch, 1.0, nan, state, None), "max_norm"),
        (fin(part, nch, INF, 1.0, state, None), "grad_scale"), (fin(part, nch, nan, 1.0, state, None), "grad_scale"),
        (clip(None, sz, ct, ci, nch, chunk, *adam, state, None), "adam_step_multi_clip"),
        (clip(ptrs, None, ct, ci, nch, chunk, *adam, state, None), "adam_step_multi_clip"),
        (clip(ptrs, sz, None, ci, nch, chunk, *adam, state, None), "adam_step_multi_clip"),
        (clip(ptrs, sz, ct, None, nch, chunk, *adam, state, None), "adam_step_multi_clip"),
        (clip(ptrs, sz, ct, ci, nch, chunk, *adam, None, None), "adam_step_multi_clip"),
        (clip(ptrs, sz, ct, ci, -1, chunk, *adam, state, None), "adam_step_multi_clip"),
        (clip(ptrs, sz, ct, ci, nch, 0, *adam, state, None), "adam_step_multi_clip"),
        (clip(ptrs, sz, ct, ci, nch, chunk, *adam[:5], 0, 1.0, state, None), "adam_step_multi_clip"),
        (clip(ptrs, sz, ct, ci, nch, chunk, *adam, state + 2, None), "4-byte"),
        (clip(ptrs, sz, ct, ci, nch, chunk, *adam[:6], INF, state, None), "grad_scale"),
        (clip(ptrs, sz, ct, ci, nch, chunk, *adam[:6], nan, state, None), "grad_scale"),
    ]
    torch.cuda.synchronize()
    for rc, _ in refused:
        assert rc == E_ARG
    _refused(fin(part, nch, 1.0, nan, state, None), "max_norm")
    _refused(sq(ptrs, sz, ct, ci, nch, chunk, part + 4, None), "8-byte")
    _refused(clip(ptrs, sz, ct, ci, nch, chunk, *adam, state + 2, None), "4-byte")
    torch.cuda.synchronize()
    assert tb.partials.unchanged() and tb.state.unchanged() and all(b.unchanged() for b in tb.P + tb.G + tb.M + tb.V)
    # an empty table is not a refusal: no launch from the two multi-tensor calls, norm 0 and coefficient 1 from the finish
    assert sq(ptrs, sz, ct, ci, 0, chunk, part, None) == 0 and clip(ptrs, sz, ct, ci, 0, chunk, *adam, state, None) == 0
    assert fin(None, 0, 1.0, 1.0, state, None) == 0
    assert [float(x) for x in tb.st()] == [0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
    assert tb.partials.unchanged() and all(b.unchanged() for b in tb.P + tb.G + tb.M + tb.V)


# =====================================================================================================================================
# 2. FusedAdam
# =====================================================================================================================================
def _count_launches(monkeypatch, lib, L):
    calls = []
    for name in L.SIGNATURES:
        fn = getattr(lib, name)

        def counting(*a, _fn=fn, _name=name):
            calls.append(_name)
            return _fn(*a)
        monkeypatch.setattr(lib, name, counting)
    return calls


TOY = ((5,), (300, 3), (8200,), (70,))          # the last one gets its first gradient at step 2: two step-count groups, ONE norm


def _toy_grads(step):
    gen = _gen(f"toy{step}")
    scale = {2: 30.0}.get(step, 1.0)
    grads = [scale * 0.01 * torch.randn(shape, generator=gen) for shape in TOY]
    if step == 3:
        grads[1][17, 1] = float("nan")
    return grads[:3] + [grads[3] if step >= 2 else None]


@pytest.mark.gpu
@pytest.mark.parametrize("wd,gs", [(0.0, 1.0), (1e-4, 0.5)])
def test_fused_adam_against_the_fp64_model(env, monkeypatch, wd, gs):  # noqa: F811
    """four steps -- normal, clipped, skipped (a NaN), normal -- each checked from the stored fp32 state before it: the norm and the
    coefficient against the global float64 norm of BOTH step-count groups, p / m / v per element with adam_reference's bars"""
    from din_amd.optim import FusedAdam
    lib, L, nhwc, ops = env
    gen = _gen("toy_params")
    params = [torch.randn(shape, generator=gen).cuda().requires_grad_(True) for shape in TOY]
    max_norm = 1.2 * gs                                                    # (the plain steps' norm is about 0.96 gs, step 2's 30x that)
    opt = FusedAdam(params, lr=LR, betas=(B1, B2), eps=AEPS, weight_decay=wd, max_grad_norm=max_norm)
    calls = _count_launches(monkeypatch, lib, L)
    model = StatsModel()
    for step in range(1, 5):
        grads = _toy_grads(step)
        for p, g in zip(params, grads):
            p.grad = None if g is None else g.cuda()
        live = [i for i, g in enumerate(grads) if g is not None]
        before = {}
        for i in live:
            m, v = opt.state.get(params[i], (torch.zeros(TOY[i]), torch.zeros(TOY[i])))
            before[i] = (params[i].detach().cpu().clone(), m.cpu().clone(), v.cpu().clone())
        del calls[:]
        opt.step(grad_scale=gs)
        groups = 1 if step == 1 else 2
        assert sorted(calls) == sorted(["din_grad_sqnorm_multi"] * groups + ["din_grad_norm_finish"] + ["din_adam_step_multi_clip"] * groups)
        assert calls.index("din_grad_norm_finish") == groups               # every group's squares first, then ONE finish, then the updates
        torch.cuda.synchronize()
        st = opt._gstate.cpu()
        norm, coef = norm_model([grads[i] for i in live], gs, max_norm)
        model.add(norm, coef)
        if coef is None:
            assert step == 3 and not math.isfinite(float(st[0]))
            for i in live:
                now = (params[i].detach().cpu(),) + tuple(t.cpu() for t in opt.state[params[i]])
                assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(now, before[i]))
            continue
        assert _rel(st[0], norm) <= NORM_BAR
        assert _rel(st[1], coef) <= COEF_BAR
        assert (coef < 1.0) == (step == 2)
        gs_eff = float(np.float32(gs) * np.float32(float(st[1])))
        for i in live:
            p0, m0, v0 = (t.reshape(-1) for t in before[i])
            want = adam_reference(p0, grads[i].reshape(-1), m0, v0, opt.steps[params[i]], wd, gs_eff)
            got = dict(p=params[i].detach().cpu(), m=opt.state[params[i]][0].cpu(), v=opt.state[params[i]][1].cpu())
            for k in "pmv":
                _check(f"FusedAdam clip step {step} tensor {i}", k, got[k].reshape(-1), want[k], want["bars"][k])
    assert [opt.steps[p] for p in params] == [4, 4, 4, 3]                  # the skipped step advanced the host-side index
    stats = opt.grad_stats(reset=False)
    assert (stats["steps"], stats["skipped"], stats["clipped"]) == (model.steps, model.skipped, model.clipped) == (4, 1, 1)
    assert _rel(stats["norm_mean"], model.sum / 3) <= sum_bar(3)
    assert _rel(stats["norm_max"], model.max) <= NORM_BAR
    assert opt.grad_stats() == stats                                       # reset=False left the running part alone
    assert opt.grad_stats() == dict(steps=0, skipped=0, clipped=0, norm_mean=0.0, norm_max=0.0)
    assert set(opt.state_dict()) == {"state", "param_groups"} and "max_grad_norm" not in opt.state_dict()["param_groups"][0]


@pytest.mark.gpu
def test_setting_off_launches_what_it_launched_before(env, monkeypatch):  # noqa: F811
    from din_amd.optim import FusedAdam
    lib, L, nhwc, ops = env
    gen = _gen("survey")
    values = [torch.randn(shape, generator=gen) for shape in TOY[:3]]
    grads = [torch.randn(shape, generator=gen) for shape in TOY[:3]]
    results = {}
    for setting in (None, INF):
        params = [v.clone().cuda().requires_grad_(True) for v in values]
        opt = FusedAdam(params, lr=LR, max_grad_norm=setting)
        calls = _count_launches(monkeypatch, lib, L)
        for _ in range(2):
            for p, g in zip(params, grads):
                p.grad = g.cuda()
            opt.step()
        torch.cuda.synchronize()
        results[setting] = ([c for c in calls if c != "din_last_error_string"], [_bits(p.detach().cpu()) for p in params])
        monkeypatch.undo()
    assert results[None][0] == ["din_adam_step_multi"] * 2
    assert results[INF][0] == ["din_grad_sqnorm_multi", "din_grad_norm_finish", "din_adam_step_multi_clip"] * 2
    assert all(torch.equal(a, b) for a, b in zip(results[None][1], results[INF][1]))


@pytest.mark.gpu
def test_non_fused_path_keeps_the_semantics(env, monkeypatch):  # noqa: F811
    """a non-contiguous parameter sends the whole list down the per-parameter path: same norm over ALL live gradients, same clip, same
    skip (decided by one read-back there), same statistics.  ops.adam_step itself refuses non-contiguous storage, as it did before this
    feature, so the launch of that one tensor is recorded here instead of made; the contiguous tensor's launch is real"""
    from din_amd import optim
    from din_amd.optim import FusedAdam
    lib, L, nhwc, ops = env
    gen = _gen("slow")
    p = torch.randn(6, 8, generator=gen).cuda().t().requires_grad_(True)          # non-contiguous view
    q = torch.randn(9, generator=gen).cuda().requires_grad_(True)
    assert not p.is_contiguous()
    launches, real = [], ops.adam_step

    def adam_step(t, g, m, v, lr, b1, b2, eps, wd, step, grad_scale=1.0):
        launches.append((tuple(t.shape), step, grad_scale))
        if t.is_contiguous():
            real(t, g, m, v, lr, b1, b2, eps, wd, step, grad_scale)
    monkeypatch.setattr(optim.ops, "adam_step", adam_step)
    opt = FusedAdam([p, q], lr=LR, betas=(B1, B2), eps=AEPS, max_grad_norm=0.5)
    gp, gq = torch.randn(8, 6, generator=gen), torch.randn(9, generator=gen)
    p.grad, q.grad = gp.cuda(), gq.cuda()
    q0 = q.detach().cpu().clone()
    opt.step()
    norm, coef = norm_model([gp, gq], 1.0, 0.5)
    assert [(s, k) for s, k, _ in launches] == [((8, 6), 1), ((9,), 1)] and launches[0][2] == launches[1][2]
    factor = launches[1][2]
    assert coef < 1.0 and _rel(factor, coef) <= COEF_BAR and factor == float(np.float32(factor))
    want = adam_reference(q0, gq, torch.zeros(9), torch.zeros(9), 1, 0.0, factor)
    for k, got in (("p", q.detach().cpu()), ("m", opt.state[q][0].cpu()), ("v", opt.state[q][1].cpu())):
        _check("slow path", k, got, want[k], want["bars"][k])
    kept = q.detach().cpu().clone()
    q.grad[3] = float("inf")
    opt.step()
    assert len(launches) == 2 and torch.equal(_bits(q.detach().cpu()), _bits(kept)) and opt.steps[q] == 2
    stats = opt.grad_stats()
    assert (stats["steps"], stats["skipped"], stats["clipped"]) == (2, 1, 1) and _rel(stats["norm_max"], norm) <= NORM_BAR
    assert _rel(stats["norm_mean"], norm) <= NORM_BAR


# =====================================================================================================================================
# 3. the trainers
# =====================================================================================================================================
KEYS = ("grad_norm_mean", "grad_norm_max", "skipped_steps", "clipped_steps")


def _trainer_cfg(tmp_path, max_grad_norm, deterministic=False):
    from din_amd.config import Config
    cfg = Config("volleyball")
    cfg.backbone, cfg.image_size, cfg.out_size, cfg.emb_features = "vgg16", (96, 160), (3, 5), 512
    cfg.num_boxes, cfg.num_frames, cfg.num_features_boxes, cfg.num_features_gcn = 4, 3, 64, 64
    cfg.ST_kernel_size, cfg.sampling_ratio, cfg.beta_factor, cfg.train_backbone = [(3, 3)], [1], False, False
    cfg.training_stage, cfg.batch_size, cfg.test_batch_size, cfg.max_epoch, cfg.test_interval_epoch = 2, 2, 2, 3, 1
    cfg.train_dropout_prob, cfg.train_learning_rate, cfg.lr_plan, cfg.train_random_seed = 0.0, 1e-3, {}, 5
    cfg.result_path, cfg.deterministic = None, deterministic
    if max_grad_norm != "unset":
        cfg.max_grad_norm = max_grad_norm
    return cfg


_RUNS = {}


def _train(tmp_path, max_grad_norm, deterministic, repeat=0):
    """three one-step epochs on two synthetic clips; returns (infos, the trained weights).  Runs are kept: the tests below share them"""
    from din_amd import train_net_dynamic as tnd
    key = (max_grad_norm, deterministic, repeat)
    if key in _RUNS:
        return _RUNS[key]
    cfg = _trainer_cfg(tmp_path, max_grad_norm, deterministic)
    seen = {}
    real = tnd.train_volleyball

    def spy(loader, model, *a, **k):
        seen["model"] = model
        return real(loader, model, *a, **k)
    tnd.train_volleyball = spy
    try:
        infos = tnd.train_net(cfg, tnd.SyntheticVolleyball(cfg, length=2), tnd.SyntheticVolleyball(cfg, length=2, seed=1), max_steps=3)
    finally:
        tnd.train_volleyball = real
    torch.cuda.synchronize()
    _RUNS[key] = infos, {k: v.detach().cpu().clone() for k, v in seen["model"].named_parameters() if v.requires_grad}
    return _RUNS[key]


def _same_bits(a, b):
    return a.keys() == b.keys() and all(torch.equal(_bits(a[k]), _bits(b[k])) for k in a)


@pytest.mark.gpu
@pytest.mark.parametrize("deterministic", [False, True], ids=["default", "deterministic"])
def test_trainer_measures_clips_and_reports(env, tmp_path, deterministic):  # noqa: F811
    """Without cfg.deterministic the gradient sums of this path meet in fp32 atomics and two runs of the SAME configuration may differ in
    their last bits, so there only the first step's loss (formed before any update) is compared exactly; under cfg.deterministic the
    run with max_grad_norm = inf has the bits of the run without the setting: nothing but the clip moved"""
    off_infos, off = _train(tmp_path, "unset", deterministic)
    inf_infos, guard = _train(tmp_path, INF, deterministic)
    clip_infos, clipped = _train(tmp_path, 1e-3, deterministic)
    assert len(off_infos) == len(inf_infos) == len(clip_infos) == 3
    assert not any(k in e["train"] for e in off_infos for k in KEYS)
    assert all(k in e["train"] for e in inf_infos + clip_infos for k in KEYS)
    assert off_infos[0]["train"]["loss"] == inf_infos[0]["train"]["loss"] == clip_infos[0]["train"]["loss"]
    if deterministic:
        assert _same_bits(off, guard), "max_grad_norm = inf moved the weights: something besides the clip changed"
        assert [e["train"]["loss"] for e in off_infos] == [e["train"]["loss"] for e in inf_infos]
    assert sum(e["train"]["clipped_steps"] for e in inf_infos) == 0 and sum(e["train"]["skipped_steps"] for e in inf_infos) == 0
    assert all(math.isfinite(e["train"]["grad_norm_mean"]) and 0 < e["train"]["grad_norm_mean"] <= e["train"]["grad_norm_max"] for e in inf_infos)
    assert sum(e["train"]["clipped_steps"] for e in clip_infos) == 3 and sum(e["train"]["skipped_steps"] for e in clip_infos) == 0
    assert not _same_bits(off, clipped) and all(bool(torch.isfinite(v).all()) for v in clipped.values())


@pytest.mark.gpu
def test_trainer_with_clipping_is_bit_reproducible_in_deterministic_mode(env, tmp_path):  # noqa: F811
    lib, L, nhwc, ops = env
    runs = [_train(tmp_path, 1e-3, True, repeat) for repeat in range(2)]
    assert L.get_option("DIN_DETERMINISTIC") is None
    assert _same_bits(runs[0][1], runs[1][1])
    assert [[e["train"][k] for k in KEYS] for e in runs[0][0]] == [[e["train"][k] for k in KEYS] for e in runs[1][0]]
    assert sum(e["train"]["clipped_steps"] for e in runs[0][0]) == 3


@pytest.mark.gpu
def test_stage1_trainer_reaches_the_keys(env, tmp_path):  # noqa: F811
    from din_amd import train_net as stage1
    from din_amd.train_net_dynamic import SyntheticVolleyball
    cfg = _trainer_cfg(tmp_path, 1e-3)
    cfg.training_stage, cfg.train_backbone, cfg.max_epoch, cfg.num_frames = 1, True, 1, 1
    cfg.result_path, cfg.log_path = str(tmp_path), str(tmp_path / "log.txt")
    infos = stage1.train_net(cfg, SyntheticVolleyball(cfg, length=2), SyntheticVolleyball(cfg, length=2, seed=1), max_steps=1)
    train = infos[0]["train"]
    assert all(k in train for k in KEYS) and train["clipped_steps"] == 1 and train["skipped_steps"] == 0
    assert "grad norm mean" in open(cfg.log_path).read()
