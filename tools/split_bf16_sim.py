"""numpy emulation of the split-bf16 contraction of DIN_F32_BF16X3 (include/din_hip.h; csrc/conv_shared.h: mma_f32_bf16x3), and the table
of its accuracy against float64 beside exact fp32, plain bf16 and the two-part form.

    python tools/split_bf16_sim.py

What is emulated, and how:
  split        x = x0 + x1 + x2: x0 = the top 16 bits of x (TRUNCATED: finite near FLT_MAX), x1 = the remainder rounded to the nearest
               bf16, x2 = what is left; the remainders are formed by fp32 subtractions, which are exact -- three parts reproduce an fp32
               value exactly (8 + 8 + 8 significand bits), as in the kernels (csrc/conv_shared.h: split_bf16x3).  split(x, n, "trunc")
               truncates every part instead: all parts then carry the sign of x, the dropped terms a1 b2 + a2 b1 add up one-sidedly and
               the three-part form measures 1.17x the exact-product figure at K = 64 instead of 0.89x.
  products     bf16 x bf16 products are exact in fp32 (16 significand bits), so they are formed in float64 without loss.
  one MFMA     the exact sum of its products, added to the fp32 accumulator with ONE rounding.  (How v_mfma_f32_16x16x32_bf16 rounds inside
               its 8-product sum is not documented; the GPU tests hold the kernels to the fp32 bar and record the margin.)
  k order      the four lane groups of a wave bring 4 k-values each: 16 k-values per MFMA group.  Exact fp32 = four 4-product
               v_mfma_f32_16x16x4_f32 (one k-value of every lane group each: exact products, one accumulator rounding per MFMA -- the
               "fp32-accumulated exact product" the split forms are measured against); split forms = the MFMAs of MFMAS3 / MFMAS2 below over
               the same 16 k-values, 32 products each (16 k-values x 2 part pairs), smallest terms first.

The forms: MFMAS3 = the kernels' three MFMAs (six products a0b0, a1b0, a0b1, a1b1, a0b2, a2b0); MFMAS2 = two parts, four products;
drop(MFMAS3, pair) = the three-part form with one product removed (what a kernel with a wrong operand word would compute)."""
import numpy as np


def split(x, n, middle="nearest"):
    """x (float32) -> n float32 arrays, each a bf16 value (low 16 bits zero): the first truncated, the others rounded to nearest (or
    truncated too: middle="trunc"); sum(parts) == x exactly for n = 3"""
    parts, r = [], np.asarray(x, np.float32).copy()
    for i in range(n):
        h = (r.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32) if i == 0 or middle == "trunc" else bf16_rne(r)
        parts.append(h)
        r = (r - h).astype(np.float32)
    return parts


def bf16_rne(x):
    """round-to-nearest-even bf16 (plain bf16 storage), as float32"""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + ((u >> 16) & 1) + 0x7FFF) >> 16) << 16
    return u.astype(np.uint32).view(np.float32)


# (part of a, part of b) per product, one list per MFMA, in the kernels' issue order
MFMAS3 = [[(2, 0), (0, 2)], [(1, 1), (0, 1)], [(1, 0), (0, 0)]]
MFMAS2 = [[(1, 1), (0, 1)], [(1, 0), (0, 0)]]
SIX = [p for m in MFMAS3 for p in m]


def drop(mfmas, pair):
    return [[p for p in m if p != pair] for m in mfmas]


def _pad4(a, m=4):
    k = a.shape[-1]
    return a if k % m == 0 else np.concatenate([a, np.zeros(a.shape[:-1] + (m - k % m,), a.dtype)], -1)


def dot_split(a, b, mfmas):
    """sum over the last axis of a * b (broadcast over the leading axes) in the split form `mfmas`; float32 result"""
    a, b = _pad4(np.asarray(a, np.float32), 16), _pad4(np.asarray(b, np.float32), 16)
    nparts = 1 + max(max(i, j) for m in mfmas for i, j in m)
    ap, bp = [p.astype(np.float64) for p in split(a, nparts)], [p.astype(np.float64) for p in split(b, nparts)]
    acc = np.zeros(np.broadcast_shapes(a.shape[:-1], b.shape[:-1]), np.float32)
    for k0 in range(0, a.shape[-1], 16):
        for m in mfmas:
            s = sum((ap[i][..., k0:k0 + 16] * bp[j][..., k0:k0 + 16]).sum(-1) for i, j in m)
            acc = (acc.astype(np.float64) + s).astype(np.float32)
    return acc


def dot_fp32(a, b):
    """exact-fp32 form: exact products, 4 per MFMA (element e of each lane group's chunk), fp32 accumulator"""
    a, b = _pad4(np.asarray(a, np.float32), 16).astype(np.float64), _pad4(np.asarray(b, np.float32), 16).astype(np.float64)
    acc = np.zeros(np.broadcast_shapes(a.shape[:-1], b.shape[:-1]), np.float32)
    for k0 in range(0, a.shape[-1], 16):
        for e in range(4):
            s = (a[..., k0 + e:k0 + 16:4] * b[..., k0 + e:k0 + 16:4]).sum(-1)
            acc = (acc.astype(np.float64) + s).astype(np.float32)
    return acc


def dot_bf16(a, b):
    """plain bf16 operands (round-to-nearest), 32 exact products per MFMA, fp32 accumulator"""
    a, b = _pad4(bf16_rne(a), 32), _pad4(bf16_rne(b), 32)
    acc = np.zeros(np.broadcast_shapes(a.shape[:-1], b.shape[:-1]), np.float32)
    for k0 in range(0, a.shape[-1], 32):
        s = (a[..., k0:k0 + 32].astype(np.float64) * b[..., k0:k0 + 32].astype(np.float64)).sum(-1)
        acc = (acc.astype(np.float64) + s).astype(np.float32)
    return acc


def operands(K, M, seed=0):
    """post-ReLU activations x N(0, 1/K) weights: M independent dot products of length K"""
    rng = np.random.default_rng(seed + K)
    a = np.maximum(rng.standard_normal((M, K)), 0).astype(np.float32)
    b = (rng.standard_normal((M, K)) / np.sqrt(K)).astype(np.float32)
    return a, b


def rms_errors(K, M, seed=0):
    """rms(err) / rms(result) against float64 of the four forms on operands(K, M)"""
    a, b = operands(K, M, seed)
    ref = (a.astype(np.float64) * b.astype(np.float64)).sum(-1)
    rr = np.sqrt((ref ** 2).mean())
    forms = {"fp32": dot_fp32(a, b), "bf16": dot_bf16(a, b), "x2": dot_split(a, b, MFMAS2), "x3": dot_split(a, b, MFMAS3)}
    return {k: float(np.sqrt(((v - ref) ** 2).mean()) / rr) for k, v in forms.items()}


def main(ks=(64, 1152, 26400)):
    print("rms(err) / rms(result) against float64; post-ReLU activations x N(0, 1/K) weights")
    print(f"{'K':>7} {'exact fp32':>12} {'bf16':>10} {'2 parts, 4 products':>20} {'3 parts, 6 products':>20}")
    for K in ks:
        e = rms_errors(K, 4096 if K < 20000 else 512)
        print(f"{K:7d} {e['fp32']:12.2e} {e['bf16']:10.1e} {e['x2']:20.1e} {e['x3']:20.2e}")


if __name__ == "__main__":
    main()
