"""Host model of the counter-based dropout mask of csrc/din_common.h (mix32, fold_seed, keep_scale), in numpy uint64, line by line.

The contract every consumer of the mask meets:

    the element at flat index i of the tensor being masked is multiplied by keep_scale(fold_seed(seed, off), i, p),
    in the forward pass and again in the backward pass,

where `seed` is the by-value seed of the launch, `off` the optional device word added to it (None: no word), `p` the drop probability
as the float the C ABI takes, and i counts the elements of the masked tensor in its logical row-major order -- never a position inside a
launch, a row, a wave or a padded stride.  tests/test_gpu_dropout.py holds every kernel that regenerates the mask to this file with
torch.equal; tests/test_dropout_cpu.py ties this file to facts outside it (the published splitmix64 output, bit strings computed with
plain Python integers) and to the seed schedule of the models.

All arithmetic wraps modulo 2^64 as the C code's does: that is intended, hence np.errstate(over="ignore")."""
import numpy as np

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
MUL1 = np.uint64(0xBF58476D1CE4E5B9)
MUL2 = np.uint64(0x94D049BB133111EB)
IDX_MUL = np.uint64(0xD1342543DE82EF95)
MASK63 = 0x7FFFFFFFFFFFFFFF
MASK64 = 0xFFFFFFFFFFFFFFFF


def _u64(x):
    """x (Python int of any sign or size, or an integer array) as uint64 modulo 2^64"""
    if isinstance(x, (int, np.integer)):
        return np.uint64(int(x) & MASK64)
    x = np.asarray(x)
    return x if x.dtype == np.uint64 else x.astype(np.int64).view(np.uint64)


def mix64(x):
    """the splitmix64 finaliser, all 64 bits (mix32 is its upper half)"""
    with np.errstate(over="ignore"):
        x = _u64(x) + GOLDEN
        x = (x ^ (x >> np.uint64(30))) * MUL1
        x = (x ^ (x >> np.uint64(27))) * MUL2
        return x ^ (x >> np.uint64(31))


def mix32(x):
    return (mix64(x) >> np.uint64(32)).astype(np.uint32)


def fold_seed(seed, off):
    """the mask seed of a launch: seed itself without a device word (whatever its size), else (seed + word) mod 2^63"""
    seed = int(seed) & MASK64
    if off is None:
        return seed
    return ((seed + (int(off) & MASK64)) & MASK64) & MASK63


def draw_u(seed, idx):
    """the uniform draw of element idx: the top 24 bits of the hash, as float32 multiples of 2^-24 in [0, 1)"""
    with np.errstate(over="ignore"):
        h = mix32(_u64(seed) ^ (_u64(np.asarray(idx, dtype=np.int64)) * IDX_MUL))
    return (h >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def keep(seed, idx, p):
    """bool: element idx survives.  p is rounded to float32 first (the C ABI takes a float) and u is compared in float32"""
    p32 = np.float32(p)
    idx = np.asarray(idx, dtype=np.int64)
    if p32 <= np.float32(0):
        return np.ones(idx.shape, dtype=bool)
    return draw_u(seed, idx) >= p32


def keep_scale(seed, idx, p):
    """float32: 1 / (1 - p) (the float32 quotient) where the element is kept, 0 where it is dropped; 1 everywhere for p <= 0"""
    p32 = np.float32(p)
    idx = np.asarray(idx, dtype=np.int64)
    if p32 <= np.float32(0):
        return np.ones(idx.shape, dtype=np.float32)
    scale = np.float32(1.0) / (np.float32(1.0) - p32)
    return np.where(draw_u(seed, idx) >= p32, scale, np.float32(0)).astype(np.float32)
