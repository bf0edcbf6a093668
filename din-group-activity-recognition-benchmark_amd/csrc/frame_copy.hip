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
#include "din_common.h"

namespace {

constexpr int BLOCK = 256;
constexpr int64_t SEG = 8192;             // bytes of one row per work item: a multiple of 16, so a segment keeps the body's alignment
constexpr int GRID_CAP = 256 * 16;        // workgroups: 256 CUs x 16, the rest of the items block-stride

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
// at whole lines: LPS = max(1, SEG / width) lines each, so a wave still covers contiguous memory on both sides (the source runs backwards
// vector by vector).  An unflagged row's segment goes through copy_segment as a copy of its own.
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

__global__ __launch_bounds__(BLOCK) void copy_rows_u8_flip_kernel(const uint64_t* __restrict__ src, const uint64_t* __restrict__ dst,
                                                                   const int64_t* __restrict__ flip, int64_t lines, int64_t width,
                                                                   int64_t lps, int64_t segs, int64_t items) {
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t row = item / segs, seg = item - row * segs;
        const uint64_t sa = src[row];
        if (sa == 0) continue;                                           // "leave this row alone"
        const uint64_t da = dst[row];
        const int64_t l0 = seg * lps, nl = lines - l0 < lps ? lines - l0 : lps;
        const uint8_t* s = reinterpret_cast<const uint8_t*>(sa) + l0 * width;
        uint8_t* d = reinterpret_cast<uint8_t*>(da) + l0 * width;
        if (flip == nullptr || flip[row] == 0) {
            const int64_t nb = nl * width;                               // (one segment unless a single line is longer than SEG)
            for (int64_t k = 0; k * SEG < nb; ++k) copy_segment(s, d, nb, k);
        } else if (((uint64_t)width | sa | da) % 16 == 0) {
            flip_lines<uint4>(s, d, width / 16, nl);                     // every real frame: 16-byte loads and stores
        } else {
            flip_lines<uint8_t>(s, d, width, nl);
        }
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

}  // namespace

extern "C" int din_copy_rows_u8(const uint64_t* src, const uint64_t* dst, int n, int64_t bytes, void* stream) {
    DIN_REQUIRE(n >= 0 && bytes >= 0, "copy_rows_u8: n = %d, bytes = %lld must not be negative", n, (long long)bytes);
    if (n == 0 || bytes == 0) return DIN_OK;
    DIN_REQUIRE(src && dst, "copy_rows_u8: null address table with n = %d", n);
    const int64_t segs = ceil_div64(bytes, SEG), items = segs * (int64_t)n;
    const int grid = (int)(items < GRID_CAP ? items : GRID_CAP);
    hipLaunchKernelGGL(copy_rows_u8_kernel, dim3(grid), dim3(BLOCK), 0, as_stream(stream), src, dst, bytes, segs, items);
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
    const int64_t lps = width >= SEG ? 1 : SEG / width;                  // whole lines per work item
    const int64_t segs = ceil_div64(lines, lps), items = segs * (int64_t)n;
    const int grid = (int)(items < GRID_CAP ? items : GRID_CAP);
    hipLaunchKernelGGL(copy_rows_u8_flip_kernel, dim3(grid), dim3(BLOCK), 0, as_stream(stream), src, dst, flip, lines, width, lps, segs,
                       items);
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
