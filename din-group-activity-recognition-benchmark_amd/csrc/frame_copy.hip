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

__global__ __launch_bounds__(BLOCK) void copy_rows_u8_kernel(const uint64_t* __restrict__ src, const uint64_t* __restrict__ dst,
                                                              int64_t bytes, int64_t segs, int64_t items) {
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t row = item / segs, seg = item - row * segs;
        const uint64_t sa = src[row];
        if (sa == 0) continue;                                           // "leave this row alone"
        const uint64_t da = dst[row];
        const uint8_t* s = reinterpret_cast<const uint8_t*>(sa);
        uint8_t* d = reinterpret_cast<uint8_t*>(da);
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
        if (b0 >= body) continue;
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
