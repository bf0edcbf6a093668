"""CPU: the host model of the dropout keep-mask (tests/dropout_reference.py) tied to facts outside itself, the edges of its definition,
the statistical conditions the design must meet, the seed schedule of the models, and proof that the exact comparisons of
tests/test_gpu_dropout.py see each way a kernel could get the mask wrong.

Anchors.  The 64-bit finaliser on 0 is the published first output of splitmix64 (0xE220A8397B1DCDAF); the bit strings and the count
were computed with two separate writings of the hash -- the numpy model and the plain Python integers of `_py_keep` below -- which
agree.  Nothing here reads a kernel: the numbers hold for the definition in csrc/din_common.h or they do not.

Statistical conditions (on the design, not measurements of a kernel): n = 2^20 draws, q = 1 - ceil(p32 2^24) / 2^24 the exact keep
probability, every share within 5 sigma of its binomial expectation; the worst of the 240 statistics is 3.2 sigma, a mask that repeats
with one of the lags or is shared between two seeds is off by hundreds."""
import math

import numpy as np
import pytest

from tests import dropout_reference as R
from tests import test_gpu_dropout as G

M63 = (1 << 63) - 1
M64 = (1 << 64) - 1
N_STAT = 1 << 20
LAGS = (1, 2, 3, 4, 64, 256, 1024, 4096)
STAT_P = (0.1, 0.3, 0.5, 0.9)
STAT_BASES = (0, 1, 0x9E3779B1, 101)


def _py_mix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def _py_keep(seed, i, p):
    """the second writing: plain Python integers, the comparison in exact rationals (u and float32(p) are both dyadic)"""
    u24 = (_py_mix64(seed ^ ((i * 0xD1342543DE82EF95) & M64)) >> 32) >> 8
    return u24 >= float(np.float32(p)) * 16777216.0          # (exact: a float32 times 2^24 is a double)


def _bits(mask):
    return "".join("1" if k else "0" for k in mask)


def _q(p):
    return 1.0 - math.ceil(float(np.float32(p)) * 16777216.0) / 16777216.0


# ---- anchors ----------------------------------------------------------------------------------------------------------------------------
def test_anchor_splitmix64_first_output():
    assert int(R.mix64(0)) == 0xE220A8397B1DCDAF == _py_mix64(0)
    assert int(R.mix32(0)) == 0xE220A839
    assert R.mix32(np.zeros(3, dtype=np.uint64)).dtype == np.uint32


def test_anchor_first_step_mask():
    from din_amd import ops
    seed = ops.mask_seed_of(0, 0, 1)
    assert seed == 7919
    got = R.keep(seed, np.arange(32), 0.3)
    assert _bits(got) == "01111110011101110010101111100111" == _bits(_py_keep(seed, i, 0.3) for i in range(32))
    assert not got[0]


def test_anchor_largest_seed_far_index():
    seed = 0x7FFFFFFFFFFFFFFF
    idx = np.arange(1000000, 1000032)
    assert _bits(R.keep(seed, idx, 0.5)) == "11111111110001010011010010110101" == _bits(_py_keep(seed, int(i), 0.5) for i in idx)


def test_anchor_kept_count():
    got = R.keep(7919, np.arange(600001), 0.3)
    assert int(got.sum()) == 420131
    assert all(bool(got[i]) == _py_keep(7919, i, 0.3) for i in range(0, 600001, 997))
    ks = R.keep_scale(7919, np.arange(600001), 0.3)
    assert ks.dtype == np.float32 and np.array_equal(ks != 0, got)
    assert set(np.unique(ks).tolist()) == {0.0, float(np.float32(1.0) / (np.float32(1.0) - np.float32(0.3)))}


# ---- edges of the definition ------------------------------------------------------------------------------------------------------------
def test_p_zero_keeps_everything_at_scale_one():
    idx = np.arange(4099)
    for p in (0.0, -0.0, -1.0):
        assert R.keep(7919, idx, p).all()
        ks = R.keep_scale(7919, idx, p)
        assert ks.dtype == np.float32 and np.array_equal(ks.view(np.uint32), np.full(4099, 0x3F800000, dtype=np.uint32))


def test_draws_lie_on_the_24_bit_lattice_and_keep_probability_is_exact():
    u = R.draw_u(7919, np.arange(1 << 16))
    assert u.dtype == np.float32
    k = u.astype(np.float64) * 16777216.0
    assert np.array_equal(k, np.floor(k)) and k.min() >= 0 and k.max() < 16777216.0
    h = R.mix32(np.uint64(7919) ^ (np.arange(1 << 16, dtype=np.uint64) * R.IDX_MUL))
    assert np.array_equal(k.astype(np.uint32), h >> np.uint32(8))             # the top 24 bits, nothing else
    lattice = np.arange(1 << 24, dtype=np.float32) * np.float32(2.0 ** -24)    # every value a draw can take, each equally likely
    for p in STAT_P + (0.3, 2.0 ** -24, 1.0 - 2.0 ** -24):
        kept = int((lattice >= np.float32(p)).sum())
        assert kept == (1 << 24) - math.ceil(float(np.float32(p)) * 16777216.0)
        assert kept / 16777216.0 == _q(p)
    for p in (0.3, 0.5):
        idx = np.arange(5000)
        assert np.array_equal(R.keep(7919, idx, p), R.draw_u(7919, idx) >= np.float32(p))


def test_smallest_p_drops_zero_and_keeps_the_next_draw():
    """p = 2^-24: u == 0 is dropped (u >= p fails), u == 2^-24 is kept (u >= p, where u > p would drop it).  The two indices belong to
    the seed that test_gpu_dropout.py's wrapping offset folds 7919 to, inside the 600001 elements of its act_dropout case"""
    seed, p = G.EDGE_SEED, 2.0 ** -24
    assert R.fold_seed(G.SEEDS[0], G.OFF_WRAP) == seed
    u = R.draw_u(seed, np.array([G.EDGE_IDX_ZERO, G.EDGE_IDX_ONE]))
    assert u[0] == 0.0 and u[1] == np.float32(2.0 ** -24)
    assert max(G.EDGE_IDX_ZERO, G.EDGE_IDX_ONE) < max(G.ACT_SIZES)
    k = R.keep(seed, np.array([G.EDGE_IDX_ZERO, G.EDGE_IDX_ONE]), p)
    assert not k[0] and k[1]
    ks = R.keep_scale(seed, np.array([G.EDGE_IDX_ZERO, G.EDGE_IDX_ONE]), p)
    assert ks[0] == 0.0 and ks[1] == np.float32(1.0) / (np.float32(1.0) - np.float32(p)) and ks[1] > 1.0
    assert _q(p) == 1.0 - 2.0 ** -24


def test_fold_seed_wraps_modulo_2_63():
    assert R.fold_seed(5, 7) == 12
    assert R.fold_seed(M63, 1) == 0
    assert R.fold_seed(M63, M63) == M63 - 1
    assert R.fold_seed((1 << 62) + 5, 1 << 62) == 5
    assert R.fold_seed(M63, (1 << 63) + 3) == 2                  # the 64-bit sum wraps too, as the device's does
    assert R.fold_seed(1 << 63, 0) == 0                          # a word, even zero, folds: the top bit goes
    for seed in (0, 7919, M63, 1 << 63, M64):
        assert R.fold_seed(seed, None) == seed                   # no word: the seed as it is, at or above 2^63 too
    idx = np.arange(64)
    assert not np.array_equal(R.keep(1 << 63, idx, 0.5), R.keep(0, idx, 0.5))


# ---- statistical conditions on the design ----------------------------------------------------------------------------------------------
def _sigmas(share, expect, n):
    return abs(share - expect) / math.sqrt(expect * (1.0 - expect) / n)


def _lag_sigmas(mask, q, lag):
    return _sigmas(float((mask[:N_STAT] & mask[lag:lag + N_STAT]).mean()), q * q, N_STAT)


@pytest.mark.parametrize("p", STAT_P)
def test_statistical_conditions(p):
    from din_amd import graph_step, ops
    q = _q(p)
    idx = np.arange(N_STAT + max(LAGS))
    worst = 0.0
    for base in STAT_BASES:
        seed = ops.mask_seed_of(base, 0, 1)
        full = R.keep(seed, idx, p)
        mask = full[:N_STAT]
        stats = {"kept": _sigmas(float(mask.mean()), q, N_STAT)}
        others = {"next step": ops.mask_seed_of(base, 0, 2), "rank 1": ops.mask_seed_of(base, 1, 1), "rank 7": ops.mask_seed_of(base, 7, 1),
                  "replay": (seed + graph_step.SEED_STRIDE) & M63, "encoder": ops.mask_seed_of(base + 101, 0, 1),
                  "next TCE site": ops.mask_seed_of(base + 7919, 0, 1)}
        for name, other in others.items():
            assert other != seed
            stats[name] = _sigmas(float((mask & R.keep(other, idx[:N_STAT], p)).mean()), q * q, N_STAT)
        for lag in LAGS:
            stats[f"lag {lag}"] = _lag_sigmas(full, q, lag)
        assert len(stats) == 15
        for name, s in stats.items():
            assert s <= 5.0, f"p {p}, base {base:#x}: {name} is {s:.2f} sigma from its expectation"
        worst = max(worst, max(stats.values()))
    print(f"p {p}: worst of {15 * len(STAT_BASES)} statistics {worst:.2f} sigma")


def test_chi_square_of_the_top_byte():
    h = R.mix32(np.uint64(7919) ^ (np.arange(N_STAT, dtype=np.uint64) * R.IDX_MUL))
    counts = np.bincount((h >> np.uint32(24)).astype(np.int64), minlength=256)
    expect = N_STAT / 256.0
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    print(f"chi-square over the top 8 bits: {chi2:.1f} at 255 degrees of freedom")
    assert chi2 <= 400.0                                          # (the 1e-8 tail of chi-square(255) lies below 400)


# ---- seed schedule ------------------------------------------------------------------------------------------------------------------------
def _schedule(bases, steps, ranks, replays):
    """every folded seed the models issue for these stream ids: ops.mask_seed_of over (base, rank, step), plus replays * SEED_STRIDE mod
    2^63 (fold_seed with the captured step's device word).  mask_seed_of is affine modulo 2^63; its coefficients are read from it"""
    from din_amd import graph_step, ops
    cb, cr, cs = ops.mask_seed_of(1, 0, 0), ops.mask_seed_of(0, 1, 0), ops.mask_seed_of(0, 0, 1)
    assert ops.mask_seed_of(0, 0, 0) == 0 and cr == ops.RANK_SEED_STRIDE & M63
    rs = np.random.RandomState(5)
    for _ in range(200):                                          # ... and the affine form is checked against the function itself
        b, r, s = int(rs.randint(0, 1 << 31)), int(rs.randint(0, 8)), int(rs.randint(0, 1 << 20))
        assert ops.mask_seed_of(b, r, s) == (b * cb + r * cr + s * cs) & M63
    u = np.uint64
    with np.errstate(over="ignore"):
        a = np.array([b & M64 for b in bases], dtype=u)[:, None, None, None] * u(cb) \
            + np.arange(ranks, dtype=u)[None, :, None, None] * u(cr) \
            + np.arange(replays, dtype=u)[None, None, :, None] * u(graph_step.SEED_STRIDE) \
            + np.asarray(steps, dtype=u)[None, None, None, :] * u(cs)
    return (a & u(M63)).ravel()


@pytest.mark.parametrize("train_random_seed", [0, 1, 7])
def test_seed_schedule_is_pairwise_distinct(train_random_seed):
    """the stream ids of one run: the models' own (train_random_seed), the infer module's, the encoder's seed_base = seed + 101 and its
    TCE sites seed_base + 7919 m; steps 1..20000, ranks 0..7, replays 0..3"""
    from din_amd import ops
    bases = [train_random_seed, 0x9E3779B1] + [train_random_seed + 101 + 7919 * m for m in range(1, 33)]
    assert len(set(bases)) == 34
    seeds = _schedule(bases, np.arange(1, 20001), 8, 4)
    assert seeds.size == 34 * 8 * 4 * 20000
    assert int(seeds[0]) == ops.mask_seed_of(train_random_seed, 0, 1)
    seeds.sort()
    assert bool((seeds[1:] != seeds[:-1]).all()), "two (stream, rank, replay, step) tuples fold to one mask seed"


# ---- the exact comparisons bite -----------------------------------------------------------------------------------------------------------
def _flat(shape):
    return np.arange(int(np.prod(shape)))


def _row_shapes():
    """(name, shape, row length) of every GPU case whose tensor has rows"""
    out = [(f"layernorm{s}", s, s[1]) for s in G.LN_SHAPES]
    out += [(f"actor_attn{s}", s, s[2]) for s in G.AT_SHAPES]
    out += [(f"basenet_head{s}", (s[0] * s[1], s[2], s[3]), s[3]) for s in G.HEAD_SHAPES]
    return out + [("cross", G.CROSS_SHAPE, G.CROSS_SHAPE[1])]


def _all_shapes():
    return [(f"act_dropout({n})", (n,)) for n in G.ACT_SIZES] + [(name, shape) for name, shape, _ in _row_shapes()]


def _differs(right, wrong, changed):
    """wrong != right; asked only where at least 64 elements hash another value (64 coincidences of two fair draws: below 1e-15)"""
    if changed < 64:
        return None
    return not np.array_equal(right, wrong)


def test_wrong_index_forms_differ_on_the_gpu_shapes():
    tried = {"row": set(), "256": set(), "plus1": set()}

    def note(kind, name, verdict):
        if verdict is not None:
            tried[kind].add(name.split("(")[0])
    for seed, off in G.SEED_CASES:
        s = R.fold_seed(seed, off)
        for p in G.P_ALL:
            for name, shape, length in _row_shapes():
                idx = _flat(shape)
                right = R.keep(s, idx, p)
                v = _differs(right, R.keep(s, idx % length, p), idx.size - length)
                assert v is not False, f"{name}: a mask that repeats every row passes"
                note("row", name, v)
            for name, shape in _all_shapes():
                idx = _flat(shape)
                right = R.keep(s, idx, p)
                v = _differs(right, R.keep(s, idx % 256, p), idx.size - 256)
                assert v is not False, f"{name}: a mask that repeats every 256 elements passes"
                note("256", name, v)
                v = _differs(right, R.keep(s, idx + 1, p), idx.size)
                assert v is not False, f"{name}: an index off by one passes"
                note("plus1", name, v)
    rows = {"layernorm", "actor_attn", "basenet_head", "cross"}    # every consumer family has a shape large enough to see each of the three
    assert tried["row"] == rows and tried["256"] == tried["plus1"] == rows | {"act_dropout"}, tried


def test_wrong_seed_forms_differ_on_the_gpu_seeds():
    idx = np.arange(1024)
    truncated = xored = 0
    for seed, off in G.SEED_CASES:
        s = R.fold_seed(seed, off)
        for p in G.P_ALL:
            right = R.keep(s, idx, p)
            if seed >> 32:                                        # a by-value seed cut to 32 bits
                assert not np.array_equal(right, R.keep(R.fold_seed(seed & 0xFFFFFFFF, off), idx, p)), (seed, off)
                truncated += 1
            if s >> 32:                                           # ... or the folded one
                assert not np.array_equal(right, R.keep(s & 0xFFFFFFFF, idx, p)), (seed, off)
            if off is not None:                                   # the word folded in with ^ where the definition adds
                assert ((seed ^ off) & M63) != s
                assert not np.array_equal(right, R.keep((seed ^ off) & M63, idx, p)), (seed, off)
                assert not np.array_equal(right, R.keep(seed ^ off, idx, p)), (seed, off)
                xored += 1
                if seed + off > M63:                              # the lost & 0x7FFF... on wrap
                    assert not np.array_equal(right, R.keep((seed + off) & M64, idx, p)), (seed, off)
    assert truncated == 2 * 3 * len(G.P_ALL) and xored == 3 * 2 * len(G.P_ALL)
    assert sum(1 for seed, off in G.SEED_CASES if off is not None and seed + off > M63) >= 3


def test_strict_comparison_differs_at_the_smallest_p():
    """u > p where the definition says u >= p: at p = 2^-24 the two differ exactly where u == 2^-24, which the act_dropout case of
    n = 600001 under (7919, wrapping offset) contains"""
    p = 2.0 ** -24
    assert p in G.ACT_P and (G.SEEDS[0], G.OFF_WRAP) in G.SEED_CASES
    idx = np.arange(max(G.ACT_SIZES))
    u = R.draw_u(R.fold_seed(G.SEEDS[0], G.OFF_WRAP), idx)
    right, wrong = R.keep(R.fold_seed(G.SEEDS[0], G.OFF_WRAP), idx, p), u > np.float32(p)
    assert np.array_equal(right, u >= np.float32(p))
    assert np.flatnonzero(right != wrong).tolist() == [G.EDGE_IDX_ONE]
    assert np.flatnonzero(~right).tolist() == [G.EDGE_IDX_ZERO]


def test_periodic_masks_fail_the_lag_conditions():
    """index modulo the row length (1024, 4: the LayerNorm / attention rows) or modulo 256 (a workgroup): the jointly-kept share at every
    lag that is a multiple of the period is q instead of q^2 -- more than 50 sigma"""
    idx = np.arange(N_STAT + max(LAGS))
    for p in (0.3, 0.5):
        q = _q(p)
        for period in (4, 256, 1024):
            bad = R.keep(7919, idx % period, p)
            hit = [lag for lag in LAGS if lag % period == 0]
            assert hit
            for lag in hit:
                assert _lag_sigmas(bad, q, lag) > 50.0, (p, period, lag)
        shared = R.keep(7919, idx[:N_STAT], p)                    # one mask for two seeds
        assert _sigmas(float((shared & shared).mean()), q * q, N_STAT) > 50.0
