"""Host model of the colour jitter (include/din_hip.h), in numpy: PIL.ImageEnhance.Contrast, then .Brightness, then .Color on a uint8
[3, H, W] frame, restated as integer and separately rounded float32 arithmetic.  tests/test_jitter_cpu.py holds this model to Pillow
itself, byte for byte; tests/test_gpu_jitter.py holds the kernels to this model."""
import numpy as np

GRAY_SEGMENT = 8192             # bytes of one plane per (row, line group) item of the two launches


def gray(r, g, b):
    """Pillow's RGB -> L: (19595 r + 38470 g + 7471 b + 32768) >> 16, in integers"""
    r, g, b = (np.asarray(v).astype(np.int64) for v in (r, g, b))
    return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16


def pivot(gray_sum: int, pixels: int) -> int:
    """the contrast stage's mean, int(gray_sum / pixels + 0.5), from integers only"""
    return (2 * int(gray_sum) + int(pixels)) // (2 * int(pixels))


def blend(d, v, f):
    """Image.blend(degenerate, image, f) for one byte plane: t = d + f * (v - d) in float32, the product and the sum rounded
    separately; t <= 0 -> 0, t >= 255 -> 255, otherwise truncated towards zero"""
    d, v, f = np.asarray(d, dtype=np.float32), np.asarray(v, dtype=np.float32), np.float32(f)
    diff = (v - d).astype(np.float32)
    t = (d + (f * diff).astype(np.float32)).astype(np.float32)
    out = np.where(t <= 0, np.float32(0), np.where(t >= 255, np.float32(255), np.trunc(t)))
    return out.astype(np.uint8)


def jitter(frame, contrast, brightness, saturation, mirror=False):
    """uint8 [3, H, W] -> uint8 [3, H, W]: the three stages in their fixed order, then (or before: it is the same) the left-right
    mirror.  A stage whose factor is exactly 1 is the identity."""
    x = np.asarray(frame)
    assert x.dtype == np.uint8 and x.ndim == 3 and x.shape[0] == 3
    c, b, s = np.float32(contrast), np.float32(brightness), np.float32(saturation)
    if c != 1:
        mean = pivot(gray(x[0], x[1], x[2]).sum(), x.shape[1] * x.shape[2])
        x = blend(np.float32(mean), x, c)
    if b != 1:
        x = blend(np.float32(0), x, b)
    if s != 1:
        x = blend(gray(x[0], x[1], x[2])[None], x, s)
    return np.ascontiguousarray(x[:, :, ::-1]) if mirror else x


def segments(height: int, width: int) -> int:
    """line groups per row: whole image lines, max(1, 8192 // width) to a group"""
    return -(-int(height) // max(1, GRAY_SEGMENT // int(width)))


def gray_partials(frame):
    """int64 [segments(H, W)]: the sum of L over every line group of a uint8 [3, H, W] frame"""
    x = np.asarray(frame)
    h, w = x.shape[1:]
    lps = max(1, GRAY_SEGMENT // w)
    lines = gray(x[0], x[1], x[2]).sum(axis=1)
    return np.array([lines[l0:l0 + lps].sum() for l0 in range(0, h, lps)], dtype=np.int64)
