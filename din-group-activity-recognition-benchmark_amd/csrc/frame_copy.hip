// din_copy_rows_u8: n independent byte-row copies (device address tables) in ONE launch -- the frame cache's insert and gather
// (din_amd/frame_cache.py).  Replaces the per-epoch decode + host stack + blocking upload of every frame (reference volleyball.py:223-275,
// train_net_dynamic.py:174) from the second epoch on: a batch of B*T frames becomes one gather out of HBM-resident slots.
//
// Work decomposition: the grid walks (row, segment) items, SEG bytes of one row each, block-strided -- one 2.7 MB frame is 338 items (more
// than one per CU), 320 frames are 108k items behind a grid capped at GRID_CAP workgroups, not 320 small launches.
// Alignment: per row, W = the widest power of two <= 16 that divides (src - dst); a head of (-dst) mod W single bytes brings BOTH addresses
// to a multiple of W, the body moves W-byte vectors (16-byte loads and stores whenever the two addresses agree mod 16, narrower otherwise),
// a tail of < W single bytes finishes the row.  Head and tail belong to the row's item 0.  The branch on W is uniform over the workgroup.
// Every access lies inside [src, src + bytes) / [dst, dst + bytes); all stores are ordinary vector stores.
//
// din_copy_rows_u8_flip is the same gather with flagged rows mirrored left-right on their way (flip augmentation, cfg.flip_prob), and
// din_flip_clip_labels mirrors the boxes and activity labels of those clips: see the second half of this file.
//
// din_rows_gray_partials and din_copy_rows_u8_jitter are the colour augmentation (cfg.color_jitter): the gather
// with Pillow's ImageEnhance.Contrast / Brightness / Color applied to drawn rows on their way, mirrored or not: the last part of this file.
#include "din_common.h"

namespace {

constexpr int BLOCK = 256;
constexpr int64_t SEG = 8192;             // bytes of one row per work item: a multiple of 16, so a segment keeps the body's alignment
constexpr int GRID_CAP = 256 * 16;        // workgroups: 256 CUs x 16, the rest of the items block-stride

inline int capped_grid(int64_t items) { return (int)(items < GRID_CAP ? items : GRID_CAP); }

// the one rule the flip, grey-partials and jitter launches cut a row by (ops.gray_partial_segments states it for the workspace)
inline int64_t lines_per_item(int64_t width) { return width >= SEG ? 1 : SEG / width; }

// nbytes is a multiple of sizeof(V); s and d are sizeof(V)-aligned
template <typename V>
__device__ __forceinline__ void copy_vectors(const uint8_t* __restrict__ s, uint8_t* __restrict__ d, int64_t nbytes) {
    const V* sv = reinterpret_cast<const V*>(s);
    V* dv = reinterpret_cast<V*>(d);
    const int64_t nv = nbytes / (int64_t)sizeof(V);
    int64_t i = threadIdx.x;
    for (; i + BLOCK < nv; i += 2 * BLOCK) {              // two loads in flight per thread before the first store
        V a = sv[i], b = sv[i + BLOCK];
        dv[i] = a;
        dv[i + BLOCK] = b;
    }
    if (i < nv) dv[i] = sv[i];
}

// one (row, segment) item of a plain copy: segment `seg` of the `bytes` bytes from s to d (see the file comment for head, body and tail)
__device__ __forceinline__ void copy_segment(const uint8_t* __restrict__ s, uint8_t* __restrict__ d, int64_t bytes, int64_t seg) {
    const uint64_t sa = reinterpret_cast<uint64_t>(s), da = reinterpret_cast<uint64_t>(d);
    const uint64_t diff = (sa - da) & 15u;
    const int64_t w = diff == 0 ? 16 : (int64_t)(diff & (~diff + 1));   // lowest set bit of the difference: 1, 2, 4 or 8
    int64_t head = (int64_t)((w - (da & (uint64_t)(w - 1))) & (uint64_t)(w - 1));
    if (head > bytes) head = bytes;
    const int64_t body = (bytes - head) / w * w;                     // whole W-byte vectors after the head
    if (seg == 0) {
        const int64_t tail0 = head + body, tail = bytes - tail0;     // head < 16 and tail < 16: one byte per thread
        if ((int64_t)threadIdx.x < head) d[threadIdx.x] = s[threadIdx.x];
        if ((int64_t)threadIdx.x < tail) d[tail0 + threadIdx.x] = s[tail0 + threadIdx.x];
    }
    const int64_t b0 = seg * SEG;
    if (b0 >= body) return;
    const int64_t len = body - b0 < SEG ? body - b0 : SEG;           // a multiple of w
    const uint8_t* sp = s + head + b0;
    uint8_t* dp = d + head + b0;
    switch (w) {
        case 16: copy_vectors<uint4>(sp, dp, len); break;
        case 8:  copy_vectors<uint2>(sp, dp, len); break;
        case 4:  copy_vectors<uint32_t>(sp, dp, len); break;
        case 2:  copy_vectors<uint16_t>(sp, dp, len); break;
        default: copy_vectors<uint8_t>(sp, dp, len); break;
    }
}

__global__ __launch_bounds__(BLOCK) void copy_rows_u8_kernel(const uint64_t* __restrict__ src, const uint64_t* __restrict__ dst,
                                                              int64_t bytes, int64_t segs, int64_t items) {
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t row = item / segs, seg = item - row * segs;
        const uint64_t sa = src[row];
        if (sa == 0) continue;                                           // "leave this row alone"
        copy_segment(reinterpret_cast<const uint8_t*>(sa), reinterpret_cast<uint8_t*>(dst[row]), bytes, seg);
    }
}

// ---- mirrored rows (din_copy_rows_u8_flip) -------------------------------------------------------------------------------------------------
// A row is `lines` lines of `width` bytes; a flagged row has every line written in reverse byte order.  The (row, segment) items are cut
// at whole lines: LPS = lines_per_item(width) lines each, so a wave still covers contiguous memory on both sides (the source runs
// backwards vector by vector).  An unflagged row's segment goes through copy_segment as a copy of its own.

// item `item` of a walk over (row, line group) items: lines [seg * lps, seg * lps + nl) of row `row`, s and d at the first of them (d:
// null where the launch has no dst table); vec: width and the row's addresses are multiples of 16 (every real frame), 16-byte vectors
// serve it.  All of it follows from `item` and the kernel's arguments: uniform over the workgroup.
struct Item { int64_t row, seg, nl; const uint8_t* s; uint8_t* d; bool vec; };

// false: src[row] == 0, "leave this row alone"
__device__ __forceinline__ bool decode_item(int64_t item, int64_t segs, int64_t lps, int64_t lines, int64_t width,
                                            const uint64_t* __restrict__ src, const uint64_t* __restrict__ dst, Item& it) {
    it.row = item / segs;
    it.seg = item - it.row * segs;
    const uint64_t sa = src[it.row];
    if (sa == 0) return false;
    const uint64_t da = dst ? dst[it.row] : 0;
    const int64_t l0 = it.seg * lps;
    it.nl = lines - l0 < lps ? lines - l0 : lps;
    it.s = reinterpret_cast<const uint8_t*>(sa) + l0 * width;
    it.d = reinterpret_cast<uint8_t*>(da + (uint64_t)(l0 * width));      // (in integers: da may be 0)
    it.vec = ((uint64_t)width | sa | da) % 16 == 0;
    return true;
}

__device__ __forceinline__ uint4 mirrored(uint4 a) {                 // the 16 bytes in reverse order: one v_perm_b32 per dword
    return make_uint4(__builtin_bswap32(a.w), __builtin_bswap32(a.z), __builtin_bswap32(a.y), __builtin_bswap32(a.x));
}
__device__ __forceinline__ uint8_t mirrored(uint8_t a) { return a; }

// nlines lines of wv V-sized units each, d[l][v] = mirrored(s[l][wv - 1 - v]); s and d are sizeof(V)-aligned, lines are contiguous.
// Thread t owns units t, t + BLOCK, ... of the segment's destination (contiguous); its (line, unit) position advances by a uniform
// step, so the loop divides nothing.  nlines > 1 only for wv <= SEG (the caller's LPS), where 32-bit arithmetic finds the start.
template <typename V>
__device__ __forceinline__ void flip_lines(const uint8_t* __restrict__ s, uint8_t* __restrict__ d, int64_t wv, int64_t nlines) {
    const V* sv = reinterpret_cast<const V*>(s);
    V* dv = reinterpret_cast<V*>(d);
    const int64_t nv = nlines * wv;
    int64_t l = 0, v = threadIdx.x, dl = 0, dx = BLOCK;
    if (nlines > 1) {
        const uint32_t w32 = (uint32_t)wv;
        l = threadIdx.x / w32;
        v = threadIdx.x % w32;
        dl = (uint32_t)BLOCK / w32;
        dx = (uint32_t)BLOCK % w32;
    }
    int64_t i = threadIdx.x;
    for (; i + BLOCK < nv; i += 2 * BLOCK) {                             // two loads in flight per thread before the first store
        int64_t l2 = l + dl, v2 = v + dx;
        if (v2 >= wv) { v2 -= wv; ++l2; }
        V a = sv[l * wv + (wv - 1 - v)], b = sv[l2 * wv + (wv - 1 - v2)];
        dv[i] = mirrored(a);
        dv[i + BLOCK] = mirrored(b);
        l = l2 + dl; v = v2 + dx;
        if (v >= wv) { v -= wv; ++l; }
    }
    if (i < nv) dv[i] = mirrored(sv[l * wv + (wv - 1 - v)]);
}

// nl lines of `width` bytes from s to d, as they are or mirrored; the branches are the caller's row-uniform ones
__device__ __forceinline__ void copy_or_mirror_lines(const uint8_t* __restrict__ s, uint8_t* __restrict__ d, int64_t width, int64_t nl,
                                                     bool mirror, bool vec) {
    if (!mirror) {
        const int64_t nb = nl * width;                                   // (one segment unless a single line is longer than SEG)
        for (int64_t k = 0; k * SEG < nb; ++k) copy_segment(s, d, nb, k);
    } else if (vec) {
        flip_lines<uint4>(s, d, width / 16, nl);                         // every real frame: 16-byte loads and stores
    } else {
        flip_lines<uint8_t>(s, d, width, nl);
    }
}

__global__ __launch_bounds__(BLOCK) void copy_rows_u8_flip_kernel(const uint64_t* __restrict__ src, const uint64_t* __restrict__ dst,
                                                                   const int64_t* __restrict__ flip, int64_t lines, int64_t width,
                                                                   int64_t lps, int64_t segs, int64_t items) {
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        Item it;
        if (!decode_item(item, segs, lps, lines, width, src, dst, it)) continue;
        copy_or_mirror_lines(it.s, it.d, width, it.nl, flip != nullptr && flip[it.row] != 0, it.vec);
    }
}

__global__ __launch_bounds__(BLOCK) void flip_clip_labels_kernel(float* __restrict__ boxes, int64_t* __restrict__ activities,
                                                                  const int64_t* __restrict__ flip, const int32_t* __restrict__ n_valid,
                                                                  const int64_t* __restrict__ label_map, int rows, int per_row, int n,
                                                                  float width, int classes) {
    const int64_t total = (int64_t)rows * per_row;
    for (int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x; t < total; t += (int64_t)gridDim.x * BLOCK) {
        const int64_t r = t / per_row;
        const int j = (int)(t - r * per_row);
        if (flip[r] == 0) continue;
        if (boxes && j < n && j < (n_valid ? n_valid[r] : n)) {
            float* b = boxes + (r * n + j) * 4;
            const float x1 = b[0], x2 = b[2];
            b[0] = width - x2;                                           // one fp32 subtraction each
            b[2] = width - x1;
        }
        if (activities && label_map && j == 0) {
            const int64_t a = activities[r];
            if (a >= 0 && a < classes) activities[r] = label_map[a];
        }
    }
}

// ---- colour jitter (din_rows_gray_partials, din_copy_rows_u8_jitter) ----------------------------------------------------------------------
// A row is three planes of `height` lines of `width` bytes, and an item covers the SAME lines in all three planes (saturation and the
// grey value need r, g and b of one pixel): line group `seg` of a row is its lines [seg * LPS, seg * LPS + LPS) with LPS =
// lines_per_item(width), so an item is at most SEG pixels unless a single line is longer.  height * width < MAX_PIXELS keeps every pixel
// index, every partial sum (<= 255 per pixel) and a row's whole sum inside 32 bits.
constexpr int64_t MAX_PIXELS = (int64_t)1 << 24;

// the sum of v over the workgroup, in every thread (integers: exact in any order)
__device__ __forceinline__ uint32_t block_sum(uint32_t v) {
    __shared__ uint32_t part[BLOCK / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    __syncthreads();                                                     // (the previous item's readers of part[] are done)
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t s = 0;
#pragma unroll
    for (int w = 0; w < BLOCK / 64; ++w) s += part[w];
    return s;
}

__device__ __forceinline__ uint32_t gray(uint32_t r, uint32_t g, uint32_t b) { return (19595u * r + 38470u * g + 7471u * b + 32768u) >> 16; }

__device__ __forceinline__ uint32_t gray_sum4(uint32_t r, uint32_t g, uint32_t b) {      // four pixels, one byte of each dword each
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < 32; k += 8) s += gray((r >> k) & 255u, (g >> k) & 255u, (b >> k) & 255u);
    return s;
}

__global__ __launch_bounds__(BLOCK) void rows_gray_partials_kernel(const uint64_t* __restrict__ src, uint32_t* __restrict__ partials,
                                                                    int64_t height, int64_t width, int64_t lps, int64_t segs,
                                                                    int64_t items) {
    const int64_t plane = height * width;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        Item it;
        if (!decode_item(item, segs, lps, height, width, src, nullptr, it)) continue;
        const uint32_t np = (uint32_t)(it.nl * width);                   // pixels of this item
        uint32_t acc = 0;
        if (it.vec) {                                                    // (then `plane` is a multiple of 16 too)
            const uint4* r = reinterpret_cast<const uint4*>(it.s);
            const uint4* g = reinterpret_cast<const uint4*>(it.s + plane);
            const uint4* b = reinterpret_cast<const uint4*>(it.s + 2 * plane);
            for (uint32_t i = threadIdx.x; i < np / 16; i += BLOCK) {
                const uint4 x = r[i], y = g[i], z = b[i];
                acc += gray_sum4(x.x, y.x, z.x) + gray_sum4(x.y, y.y, z.y) + gray_sum4(x.z, y.z, z.z) + gray_sum4(x.w, y.w, z.w);
            }
        } else {
            for (uint32_t i = threadIdx.x; i < np; i += BLOCK) acc += gray(it.s[i], it.s[plane + i], it.s[2 * plane + i]);
        }
        acc = block_sum(acc);
        if (threadIdx.x == 0) partials[item] = acc;                      // item = row * segs + seg: one plain store
    }
}

// Pixel values travel through the stages as floats holding integers 0..255, so a stage costs no conversion.
struct Jitter { float c, b, s, mean; };

// Image.blend's store: t <= 0 -> 0, t >= 255 -> 255, otherwise truncated towards zero
__device__ __forceinline__ float to_byte(float t) { return truncf(fminf(fmaxf(t, 0.f), 255.f)); }
// multiply and add rounded separately, whatever -ffp-contract says
__device__ __forceinline__ float blend(float d, float v, float f) { return to_byte(__fadd_rn(d, __fmul_rn(f, v - d))); }
// L of integer-valued floats: every product and partial sum is an integer below 2^24 (at most 65536 * 255 + 32768), so the fused
// multiply-adds, the scaling by 2^-16 and the floor are all exact -- this IS the integer expression of gray()
__device__ __forceinline__ float gray_f(float r, float g, float b) {
    return floorf(fmaf(19595.f, r, fmaf(38470.f, g, fmaf(7471.f, b, 32768.f))) * (1.f / 65536.f));
}

template <bool DC, bool DB, bool DS>
__device__ __forceinline__ void jitter_px(float& r, float& g, float& b, const Jitter& j) {
    if (DC) { r = blend(j.mean, r, j.c); g = blend(j.mean, g, j.c); b = blend(j.mean, b, j.c); }
    if (DB) { r = blend(0.f, r, j.b); g = blend(0.f, g, j.b); b = blend(0.f, b, j.b); }
    if (DS) {
        const float l = gray_f(r, g, b);
        r = blend(l, r, j.s); g = blend(l, g, j.s); b = blend(l, b, j.s);
    }
}

template <bool DC, bool DB, bool DS>
__device__ __forceinline__ void jitter_dword(uint32_t& r4, uint32_t& g4, uint32_t& b4, const Jitter& j) {
    uint32_t ro = 0, go = 0, bo = 0;
#pragma unroll
    for (int k = 0; k < 32; k += 8) {
        float r = (float)((r4 >> k) & 255u), g = (float)((g4 >> k) & 255u), b = (float)((b4 >> k) & 255u);     // v_cvt_f32_ubyte0..3
        jitter_px<DC, DB, DS>(r, g, b, j);
        ro |= (uint32_t)r << k; go |= (uint32_t)g << k; bo |= (uint32_t)b << k;       // (integers already: no rounding left to do)
    }
    r4 = ro; g4 = go; b4 = bo;
}

template <bool DC, bool DB, bool DS>
__device__ __forceinline__ void jitter_unit(uint4& r, uint4& g, uint4& b, const Jitter& j) {
    jitter_dword<DC, DB, DS>(r.x, g.x, b.x, j);
    jitter_dword<DC, DB, DS>(r.y, g.y, b.y, j);
    jitter_dword<DC, DB, DS>(r.z, g.z, b.z, j);
    jitter_dword<DC, DB, DS>(r.w, g.w, b.w, j);
}

// 16-byte unit `i` of the item's nl lines of wv units, from the three planes; a mirrored row reads unit wv - 1 - v of the same line and
// reverses its bytes (the stages are per pixel and `mean` belongs to the whole frame, so they commute with the mirror)
__device__ __forceinline__ void load_unit(const uint8_t* __restrict__ s, int64_t plane, uint32_t wv, bool flip, uint32_t i, uint4& r,
                                          uint4& g, uint4& b) {
    uint32_t si = i;
    if (flip) {
        const uint32_t l = i / wv, v = i - l * wv;
        si = l * wv + (wv - 1 - v);
    }
    r = reinterpret_cast<const uint4*>(s)[si];
    g = reinterpret_cast<const uint4*>(s + plane)[si];
    b = reinterpret_cast<const uint4*>(s + 2 * plane)[si];
    if (flip) { r = mirrored(r); g = mirrored(g); b = mirrored(b); }
}

__device__ __forceinline__ void store_unit(uint8_t* __restrict__ d, int64_t plane, uint32_t i, uint4 r, uint4 g, uint4 b) {
    reinterpret_cast<uint4*>(d)[i] = r;
    reinterpret_cast<uint4*>(d + plane)[i] = g;
    reinterpret_cast<uint4*>(d + 2 * plane)[i] = b;
}

// one item, 16-byte path: s, d and plane are multiples of 16, lines are wv units; nl * wv < 2^20
template <bool DC, bool DB, bool DS>
__device__ __forceinline__ void jitter_units(const uint8_t* __restrict__ s, uint8_t* __restrict__ d, int64_t plane, uint32_t wv,
                                             uint32_t nl, bool flip, const Jitter& j) {
    const uint32_t nv = nl * wv;
    uint32_t i = threadIdx.x;
    for (; i + BLOCK < nv; i += 2 * BLOCK) {                             // two loads per plane in flight before the first store
        uint4 r0, g0, b0, r1, g1, b1;
        load_unit(s, plane, wv, flip, i, r0, g0, b0);
        load_unit(s, plane, wv, flip, i + BLOCK, r1, g1, b1);
        jitter_unit<DC, DB, DS>(r0, g0, b0, j);
        store_unit(d, plane, i, r0, g0, b0);
        jitter_unit<DC, DB, DS>(r1, g1, b1, j);
        store_unit(d, plane, i + BLOCK, r1, g1, b1);
    }
    if (i < nv) {
        uint4 r0, g0, b0;
        load_unit(s, plane, wv, flip, i, r0, g0, b0);
        jitter_unit<DC, DB, DS>(r0, g0, b0, j);
        store_unit(d, plane, i, r0, g0, b0);
    }
}

// one item, byte by byte: any width, any alignment; nl * width < 2^24
template <bool DC, bool DB, bool DS>
__device__ __forceinline__ void jitter_bytes(const uint8_t* __restrict__ s, uint8_t* __restrict__ d, int64_t plane, uint32_t width,
                                             uint32_t nl, bool flip, const Jitter& j) {
    const uint32_t np = nl * width;
    for (uint32_t i = threadIdx.x; i < np; i += BLOCK) {
        uint32_t si = i;
        if (flip) {
            const uint32_t l = i / width, x = i - l * width;
            si = l * width + (width - 1 - x);
        }
        float r = (float)s[si], g = (float)s[plane + si], b = (float)s[2 * plane + si];
        jitter_px<DC, DB, DS>(r, g, b, j);
        d[i] = (uint8_t)r;
        d[plane + i] = (uint8_t)g;
        d[2 * plane + i] = (uint8_t)b;
    }
}

template <bool DC, bool DB, bool DS>
__device__ __forceinline__ void jitter_item(const uint8_t* __restrict__ s, uint8_t* __restrict__ d, int64_t plane, int64_t width,
                                            int64_t nl, bool vec, bool flip, const Jitter& j) {
    if (vec) jitter_units<DC, DB, DS>(s, d, plane, (uint32_t)(width / 16), (uint32_t)nl, flip, j);
    else     jitter_bytes<DC, DB, DS>(s, d, plane, (uint32_t)width, (uint32_t)nl, flip, j);
}

__global__ __launch_bounds__(BLOCK) void copy_rows_u8_jitter_kernel(const uint64_t* __restrict__ src, const uint64_t* __restrict__ dst,
                                                                     const int64_t* __restrict__ flip, const float* __restrict__ factors,
                                                                     const uint32_t* __restrict__ partials, int64_t height, int64_t width,
                                                                     int64_t lps, int64_t segs, int64_t items) {
    const int64_t plane = height * width;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        Item it;
        if (!decode_item(item, segs, lps, height, width, src, dst, it)) continue;
        const bool mirror = flip != nullptr && flip[it.row] != 0;          // (it.vec: then `plane` is a multiple of 16 too)
        Jitter j = {1.f, 1.f, 1.f, 0.f};
        if (factors) { j.c = factors[3 * it.row]; j.b = factors[3 * it.row + 1]; j.s = factors[3 * it.row + 2]; }
        // everything below branches on the row alone: uniform over the workgroup
        const int stages = (j.c != 1.f ? 1 : 0) | (j.b != 1.f ? 2 : 0) | (j.s != 1.f ? 4 : 0);
        if (stages == 0) {                                               // the plain or mirrored body, plane by plane
            for (int p = 0; p < 3; ++p) copy_or_mirror_lines(it.s + p * plane, it.d + p * plane, width, it.nl, mirror, it.vec);
            continue;
        }
        if (stages & 1) {                                                // the contrast pivot: the row's partials, in integers
            uint32_t acc = 0;
            for (int64_t t = threadIdx.x; t < segs; t += BLOCK) acc += partials[it.row * segs + t];
            const uint64_t sum = block_sum(acc);
            j.mean = (float)(uint32_t)((2 * sum + (uint64_t)plane) / (2 * (uint64_t)plane));
        }
        switch (stages) {
            case 1: jitter_item<true, false, false>(it.s, it.d, plane, width, it.nl, it.vec, mirror, j); break;
            case 2: jitter_item<false, true, false>(it.s, it.d, plane, width, it.nl, it.vec, mirror, j); break;
            case 3: jitter_item<true, true, false>(it.s, it.d, plane, width, it.nl, it.vec, mirror, j); break;
            case 4: jitter_item<false, false, true>(it.s, it.d, plane, width, it.nl, it.vec, mirror, j); break;
            case 5: jitter_item<true, false, true>(it.s, it.d, plane, width, it.nl, it.vec, mirror, j); break;
            case 6: jitter_item<false, true, true>(it.s, it.d, plane, width, it.nl, it.vec, mirror, j); break;
            default: jitter_item<true, true, true>(it.s, it.d, plane, width, it.nl, it.vec, mirror, j); break;
        }
    }
}

}  // namespace

extern "C" int din_copy_rows_u8(const uint64_t* src, const uint64_t* dst, int n, int64_t bytes, void* stream) {
    DIN_REQUIRE(n >= 0 && bytes >= 0, "copy_rows_u8: n = %d, bytes = %lld must not be negative", n, (long long)bytes);
    if (n == 0 || bytes == 0) return DIN_OK;
    DIN_REQUIRE(src && dst, "copy_rows_u8: null address table with n = %d", n);
    const int64_t segs = ceil_div64(bytes, SEG), items = segs * (int64_t)n;
    hipLaunchKernelGGL(copy_rows_u8_kernel, dim3(capped_grid(items)), dim3(BLOCK), 0, as_stream(stream), src, dst, bytes, segs, items);
    DIN_CHECK_LAUNCH("copy_rows_u8");
    return DIN_OK;
}

extern "C" int din_copy_rows_u8_flip(const uint64_t* src, const uint64_t* dst, const int64_t* flip, int n, int64_t lines, int64_t width,
                                     void* stream) {
    DIN_REQUIRE(n >= 0 && lines >= 0 && width >= 0, "copy_rows_u8_flip: n = %d, lines = %lld, width = %lld must not be negative", n,
                (long long)lines, (long long)width);
    if (n == 0 || lines == 0 || width == 0) return DIN_OK;
    DIN_REQUIRE(lines <= INT64_MAX / width, "copy_rows_u8_flip: lines * width = %lld * %lld overflows", (long long)lines, (long long)width);
    DIN_REQUIRE(src && dst, "copy_rows_u8_flip: null address table with n = %d", n);
    const int64_t lps = lines_per_item(width), segs = ceil_div64(lines, lps), items = segs * (int64_t)n;
    hipLaunchKernelGGL(copy_rows_u8_flip_kernel, dim3(capped_grid(items)), dim3(BLOCK), 0, as_stream(stream), src, dst, flip, lines, width,
                       lps, segs, items);
    DIN_CHECK_LAUNCH("copy_rows_u8_flip");
    return DIN_OK;
}

extern "C" int din_flip_clip_labels(float* boxes, int64_t* activities, const int64_t* flip, const int32_t* n_valid,
                                    const int64_t* label_map, int rows, int n, float width, int classes, void* stream) {
    DIN_REQUIRE(rows >= 0 && n >= 0 && classes >= 0, "flip_clip_labels: rows = %d, n = %d, classes = %d must not be negative", rows, n,
                classes);
    if (n == 0) boxes = nullptr;
    if (!label_map) activities = nullptr;                                // (no map: the labels have no side)
    if (rows == 0 || (!boxes && !activities)) return DIN_OK;
    DIN_REQUIRE(flip, "flip_clip_labels: null flags with rows = %d", rows);
    const int per_row = boxes ? n : 1;
    hipLaunchKernelGGL(flip_clip_labels_kernel, dim3(grid_1d((int64_t)rows * per_row, BLOCK)), dim3(BLOCK), 0, as_stream(stream), boxes,
                       activities, flip, n_valid, label_map, rows, per_row, n, width, classes);
    DIN_CHECK_LAUNCH("flip_clip_labels");
    return DIN_OK;
}

// the checks the two colour-jitter launches share; 1: nothing to do, 0: go on, negative: refused
static int jitter_geometry(const char* what, int n, int64_t height, int64_t width) {
    DIN_REQUIRE(n >= 0 && height >= 0 && width >= 0, "%s: n = %d, height = %lld, width = %lld must not be negative", what, n,
                (long long)height, (long long)width);
    if (n == 0 || height == 0 || width == 0) return 1;
    DIN_REQUIRE(height <= INT64_MAX / width && height * width < MAX_PIXELS,
                "%s: height * width = %lld * %lld must stay below 2^24 pixels (a row's grey sum is kept in 32 bits)", what,
                (long long)height, (long long)width);
    return 0;
}

extern "C" int din_rows_gray_partials(const uint64_t* src, uint32_t* partials, int n, int64_t height, int64_t width, void* stream) {
    const int rc = jitter_geometry("rows_gray_partials", n, height, width);
    if (rc != 0) return rc < 0 ? rc : DIN_OK;
    DIN_REQUIRE(src && partials, "rows_gray_partials: null address table or partials with n = %d", n);
    const int64_t lps = lines_per_item(width), segs = ceil_div64(height, lps), items = segs * (int64_t)n;
    hipLaunchKernelGGL(rows_gray_partials_kernel, dim3(capped_grid(items)), dim3(BLOCK), 0, as_stream(stream), src, partials, height, width,
                       lps, segs, items);
    DIN_CHECK_LAUNCH("rows_gray_partials");
    return DIN_OK;
}

extern "C" int din_copy_rows_u8_jitter(const uint64_t* src, const uint64_t* dst, const int64_t* flip, const float* factors,
                                       const uint32_t* partials, int n, int64_t height, int64_t width, void* stream) {
    const int rc = jitter_geometry("copy_rows_u8_jitter", n, height, width);
    if (rc != 0) return rc < 0 ? rc : DIN_OK;
    DIN_REQUIRE(src && dst, "copy_rows_u8_jitter: null address table with n = %d", n);
    DIN_REQUIRE((factors == nullptr) == (partials == nullptr), "copy_rows_u8_jitter: factors and partials come together (%s is null)",
                factors ? "partials" : "factors");
    const int64_t lps = lines_per_item(width), segs = ceil_div64(height, lps), items = segs * (int64_t)n;
    hipLaunchKernelGGL(copy_rows_u8_jitter_kernel, dim3(capped_grid(items)), dim3(BLOCK), 0, as_stream(stream), src, dst, flip, factors,
                       partials, height, width, lps, segs, items);
    DIN_CHECK_LAUNCH("copy_rows_u8_jitter");
    return DIN_OK;
}
