/* din_hip_aug.h -- C ABI of libdin_hip.so, second header: the colour augmentation of the frame gather (cfg.color_jitter,
 * din_amd/frame_cache.py).  The conventions are those of din_hip.h (plain C types, DEVICE pointers owned by the caller, 0 or a negative
 * DIN_E_* code with din_last_error_string(), `stream` a hipStream_t passed as void*, no allocation, no synchronisation).  The entry points
 * here are additive: din_hip.h does not include this header, and DIN_ABI_VERSION stays 9.
 *
 * What they replace: PIL.ImageEnhance.Contrast, .Brightness and .Color (Pillow: ImageEnhance.py, Image.blend), applied in that order to
 * a decoded uint8 RGB frame -- what a loader of the reference's kind (volleyball.py:223-275 decodes with Pillow) would do on the host
 * between decode and stack, once per frame and epoch.  Here the frames stay as decoded in their HBM slots and the three stages are a
 * per-pixel function applied inside the launch that builds the batch.  The results are Pillow's, byte for byte.
 *
 * A row is a uint8 [3, height, width] frame: three planes R, G, B of `height` lines of `width` bytes.
 *   L(r, g, b)      = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16, in integers          (Pillow's "L" conversion);
 *   blend(d, v, f)  = t = (float)d + f * ((float)v - (float)d) in fp32, multiply and add rounded separately; t <= 0 gives 0,
 *                     t >= 255 gives 255, anything else is truncated towards zero               (Image.blend outside [0, 1]);
 *   S               = the sum of L over the height * width pixels of the row AS STORED (before any stage);
 *   mean            = (2 * S + height * width) / (2 * height * width) in integer division      (= int(S / (height * width) + 0.5)).
 * With the row's factors (c, b, s) -- contrast, brightness, saturation, fp32 -- every pixel goes through
 *   1. contrast     each of r, g, b becomes blend(mean, v, c);
 *   2. brightness   each becomes blend(0, v, b);
 *   3. saturation   with g = L of the pixel after stages 1 and 2, each becomes blend(g, v, s);
 * every stage produces uint8.  A stage whose factor is exactly 1.0f is the identity and is skipped.
 *
 * Work items: a row is cut at whole image lines into "line groups" of LPS = max(1, 8192 / width) lines (integer division), the
 * same lines in all three planes; SEGS(height, width) = ceil(height / LPS) groups per row.  Both launches walk (row, line group) items
 * block-strided behind at most 4096 workgroups; both derive SEGS by this one rule, and so does the caller that sizes `partials`.
 */
#ifndef DIN_HIP_AUG_H
#define DIN_HIP_AUG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * The grey sums of n rows, by line group (the first half of PIL.ImageEnhance.Contrast: the mean of image.convert("L")).
 * src: a DEVICE array of n device addresses of [3, height, width] uint8 rows; src[i] == 0 leaves the partials of row i alone.
 * partials: DEVICE uint32 [n * SEGS(height, width)]; partials[i * SEGS + g] = the sum of L over the pixels of line group g of row i,
 * ONE plain store per item: no atomics, nothing for the caller to clear.  Integer sums: the result does not depend on any order.
 * Rows may start at any byte alignment (16-byte loads where width and the address are multiples of 16, single bytes otherwise).
 * One plain launch on `stream`, capturable.  n == 0 or height * width == 0 returns DIN_OK without a launch.  DIN_E_ARG before any
 * launch: a null src or partials with work to do; a negative n, height or width; height * width that overflows or is >= 2^24 (a
 * partial, and the whole row's sum, must fit 32 bits with room to spare).
 * ---------------------------------------------------------------------------------------------- */
int din_rows_gray_partials(const uint64_t* src, uint32_t* partials, int n, int64_t height, int64_t width, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The frame gather of din_copy_rows_u8_flip (din_hip.h) with row i transformed by factors[3 * i .. 3 * i + 2] = (contrast, brightness,
 * saturation) on its way, as defined at the top of this header (PIL.ImageEnhance.Contrast, then .Brightness, then .Color).
 * src, dst: DEVICE arrays of n device addresses of [3, height, width] uint8 rows; src[i] == 0 leaves row i alone.  flip: DEVICE int64
 * [n] or null (all zero); where flip[i] != 0 every line of row i is written in reverse byte order, jittered or not -- a batch that is
 * both mirrored and jittered is still one gather launch.  factors: DEVICE fp32 [3 * n], finite.  partials: what din_rows_gray_partials
 * wrote for the SAME src, n, height and width, earlier on the same stream; each workgroup adds its row's SEGS partials (integers, served
 * from L2) to S.  Only rows with a contrast factor other than 1 read them.
 * A row whose three factors are all exactly 1.0f is copied (or mirrored) exactly as din_copy_rows_u8_flip does it; factors == null and
 * partials == null together mean that for every row.  Where width and both addresses of a row are multiples of 16 (every real frame) a
 * jittered row moves as 16-byte vectors, two loads per plane in flight before the first store; any other width or alignment goes byte
 * by byte.  Every access lies inside the two ranges of its row; all stores are plain vector stores, no atomics: capturable.  Sources
 * may repeat; a destination row must not overlap any source or any other destination.
 * n == 0 or height * width == 0 returns DIN_OK without a launch.  DIN_E_ARG before any launch: a null src or dst with work to do; a
 * negative n, height or width; height * width that overflows or is >= 2^24; factors null with partials non-null, or the reverse.
 * ---------------------------------------------------------------------------------------------- */
int din_copy_rows_u8_jitter(const uint64_t* src, const uint64_t* dst, const int64_t* flip, const float* factors,
                            const uint32_t* partials, int n, int64_t height, int64_t width, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIN_HIP_AUG_H */
