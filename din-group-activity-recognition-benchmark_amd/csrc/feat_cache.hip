// din_feat_rows: the box-feature cache's one launch per step (din_amd/feature_cache.py).  With a frozen backbone the trunk of the reference
// (infer_model.py:152-184: backbone, multi-scale fuse, RoIAlign) is a pure function of a frame and its boxes, so its fp32 output row
// [N, D, K, K] stays in an HBM slot after the first epoch and a step skips the trunk.  Per row i of the B*T rows of a batch, in ONE launch:
//   * src[i] -> dst[i]            build the feats tensor fc_emb_1 reads (from a slot, or from the row the trunk just computed);
//   * src[i] -> keep[i]           also insert a freshly computed row into its slot: the source is read once and stored twice;
//   * boxes[i] -> keep[i] + row   the slot's trailer: the boxes the features were computed for;
//   * boxes[i] vs ref_boxes[i]    a row served from a slot: are this step's boxes the ones stored with it?  flags[i] = 1 if not.
//
// Work decomposition (as frame_copy.hip): the grid walks (row, segment) items, DIN_FEAT_ROWS_SEGMENT bytes of one row each, block-strided
// behind a grid capped at GRID_CAP workgroups -- a 614 400-byte VGG16 row is 38 items, 320 rows are 12k items, not 320 launches.  Every
// address, row_bytes and box_bytes is a multiple of 16, so all traffic is 16-byte vectors; a segment is UNROLL vectors per lane, all loaded
// before the first store.  The boxes (a few hundred bytes) belong to the row's item 0.  Every access lies inside [src, src + row_bytes),
// [dst, dst + row_bytes), [keep, keep + row_bytes + box_bytes), [ref_boxes, ref_boxes + box_bytes), boxes[i] or flags[i]; all stores are
// ordinary vector stores, no atomics: several lanes that see a difference store the same 1.
//
// din_feat_rows_bf16: the same launch over slots of bf16 rows (cfg.feature_cache_dtype = 'bf16': under backbone_dtype = 'bf16' the only
// reader of feats is the embedding GEMM, which used to round the whole tensor to bf16 in a pass of its own).  Rows are row_elems bf16
// values; a resident row is the copy above at row_bytes = 2 * row_elems.  A row the trunk just computed (src_f32[i] != 0) is row_elems
// fp32 values at src[i]: read once, rounded once (round-to-nearest-even, the hardware conversion: pack_bf16x2), stored to dst[i] and
// keep[i].  Items stay DIN_FEAT_ROWS_SEGMENT bytes of the DESTINATION row; a converting lane loads two 16-byte fp32 vectors per 16-byte
// store, all eight before its first store, and every fp32 read lies inside [src, src + 4 * row_elems).
#include "din_common.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));     // one 16-byte access (a native vector: stays in registers)
// the tables hold plain integers: naming the global address space makes every access a global_ (not a flat_) instruction
typedef const u32x4 __attribute__((address_space(1)))* gsrc_t;
typedef u32x4 __attribute__((address_space(1)))* gdst_t;

constexpr int BLOCK = 256;
constexpr int UNROLL = 4;                        // 16-byte loads in flight per lane
constexpr int64_t SEG = DIN_FEAT_ROWS_SEGMENT;   // bytes of one row per work item
static_assert(UNROLL == 4 && SEG == (int64_t)BLOCK * UNROLL * 16, "a segment is four 16-byte vectors per lane");
constexpr int GRID_CAP = 256 * 16;               // workgroups: 256 CUs x 16, the rest of the items block-stride

// eight fp32 values (two 16-byte vectors, lo first in memory) -> eight bf16 values (one 16-byte vector)
__device__ __forceinline__ u32x4 round_to_bf16(u32x4 lo, u32x4 hi) {
    return u32x4{pack_bf16x2(__uint_as_float(lo.x), __uint_as_float(lo.y)), pack_bf16x2(__uint_as_float(lo.z), __uint_as_float(lo.w)),
                 pack_bf16x2(__uint_as_float(hi.x), __uint_as_float(hi.y)), pack_bf16x2(__uint_as_float(hi.z), __uint_as_float(hi.w))};
}

// BF16 = false: din_feat_rows (src_f32 is not read).  BF16 = true: din_feat_rows_bf16, row_bytes = 2 * row_elems.
template <bool BF16>
__global__ __launch_bounds__(BLOCK) void feat_rows_kernel(const uint64_t* __restrict__ src, const uint64_t* __restrict__ dst,
                                                           const uint64_t* __restrict__ keep, const uint64_t* __restrict__ ref_boxes,
                                                           const uint64_t* __restrict__ src_f32, const uint8_t* __restrict__ boxes,
                                                           uint8_t* __restrict__ flags, int64_t row_bytes, int box_bytes, int64_t segs,
                                                           int64_t items) {
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t row = item / segs, seg = item - row * segs;
        const uint64_t sa = src[row];
        if (sa == 0) continue;                                           // "leave this row alone"
        const uint64_t da = dst[row];
        const uint64_t ka = keep ? keep[row] : 0;
        const uint64_t ra = ref_boxes ? ref_boxes[row] : 0;
        if (((sa | da | ka | ra) & 15u) != 0 || da == 0) continue;       // not what the cache builds: no access at all for this row
        const int64_t b0 = seg * SEG;
        if (b0 < row_bytes) {
            const int64_t left = row_bytes - b0;
            const int64_t nv = (left < SEG ? left : SEG) / 16;
            gdst_t d = (gdst_t)(da + (uint64_t)b0);
            // four named registers, not an array: the compiler moves a conditionally written private array to LDS
            const int64_t i0 = threadIdx.x, i1 = i0 + BLOCK, i2 = i1 + BLOCK, i3 = i2 + BLOCK;
            const u32x4 zero = {0, 0, 0, 0};
            u32x4 v0, v1, v2, v3;
            if (BF16 && src_f32 != nullptr && src_f32[row] != 0) {       // a computed fp32 row (uniform over the workgroup)
                gsrc_t s = (gsrc_t)(sa + 2 * (uint64_t)b0);              // destination vector i is fp32 vectors 2i and 2i + 1
                const u32x4 a0 = i0 < nv ? s[2 * i0] : zero, c0 = i0 < nv ? s[2 * i0 + 1] : zero;
                const u32x4 a1 = i1 < nv ? s[2 * i1] : zero, c1 = i1 < nv ? s[2 * i1 + 1] : zero;
                const u32x4 a2 = i2 < nv ? s[2 * i2] : zero, c2 = i2 < nv ? s[2 * i2 + 1] : zero;
                const u32x4 a3 = i3 < nv ? s[2 * i3] : zero, c3 = i3 < nv ? s[2 * i3 + 1] : zero;
                v0 = round_to_bf16(a0, c0), v1 = round_to_bf16(a1, c1), v2 = round_to_bf16(a2, c2), v3 = round_to_bf16(a3, c3);
            } else {
                gsrc_t s = (gsrc_t)(sa + (uint64_t)b0);
                v0 = i0 < nv ? s[i0] : zero, v1 = i1 < nv ? s[i1] : zero, v2 = i2 < nv ? s[i2] : zero, v3 = i3 < nv ? s[i3] : zero;
            }
            if (i0 < nv) d[i0] = v0;
            if (i1 < nv) d[i1] = v1;
            if (i2 < nv) d[i2] = v2;
            if (i3 < nv) d[i3] = v3;
            if (ka != 0) {                                               // uniform over the workgroup
                gdst_t k = (gdst_t)(ka + (uint64_t)b0);
                if (i0 < nv) k[i0] = v0;
                if (i1 < nv) k[i1] = v1;
                if (i2 < nv) k[i2] = v2;
                if (i3 < nv) k[i3] = v3;
            }
        }
        if (seg == 0 && (ka != 0 || ra != 0)) {
            gsrc_t b = (gsrc_t)((uint64_t)(uintptr_t)boxes + (uint64_t)(row * (int64_t)box_bytes));
            gdst_t trailer = (gdst_t)(ka + (uint64_t)row_bytes);
            gsrc_t stored = (gsrc_t)ra;
            bool differ = false;
            for (int i = threadIdx.x; i < box_bytes / 16; i += BLOCK) {
                const u32x4 now = b[i];
                if (ka != 0) trailer[i] = now;
                if (ra != 0) {
                    const u32x4 was = stored[i];
                    differ |= now.x != was.x || now.y != was.y || now.z != was.z || now.w != was.w;
                }
            }
            if (differ) flags[row] = 1;
        }
    }
}

}  // namespace

extern "C" int din_feat_rows(const uint64_t* src, const uint64_t* dst, const uint64_t* keep, const uint64_t* ref_boxes, const void* boxes,
                             uint8_t* flags, int n, int64_t row_bytes, int box_bytes, void* stream) {
    DIN_REQUIRE(n >= 0 && row_bytes >= 0 && box_bytes >= 0, "feat_rows: n = %d, row_bytes = %lld, box_bytes = %d must not be negative", n,
                (long long)row_bytes, box_bytes);
    DIN_REQUIRE(row_bytes % 16 == 0 && box_bytes % 16 == 0, "feat_rows: row_bytes = %lld and box_bytes = %d must be multiples of 16",
                (long long)row_bytes, box_bytes);
    DIN_REQUIRE(((uintptr_t)boxes & 15u) == 0, "feat_rows: boxes must be 16-byte aligned");
    if (n == 0) return DIN_OK;
    DIN_REQUIRE(src && dst, "feat_rows: null address table with n = %d", n);
    DIN_REQUIRE(!(keep || ref_boxes) || (boxes && flags), "feat_rows: keep / ref_boxes given without boxes and flags");
    const int64_t segs = row_bytes > 0 ? ceil_div64(row_bytes, SEG) : 1, items = segs * (int64_t)n;
    const int grid = (int)(items < GRID_CAP ? items : GRID_CAP);
    hipLaunchKernelGGL(feat_rows_kernel<false>, dim3(grid), dim3(BLOCK), 0, as_stream(stream), src, dst, keep, ref_boxes,
                       static_cast<const uint64_t*>(nullptr), static_cast<const uint8_t*>(boxes), flags, row_bytes, box_bytes, segs, items);
    DIN_CHECK_LAUNCH("feat_rows");
    return DIN_OK;
}

extern "C" int din_feat_rows_bf16(const uint64_t* src, const uint64_t* dst, const uint64_t* keep, const uint64_t* ref_boxes,
                                  const uint64_t* src_f32, const void* boxes, uint8_t* flags, int n, int64_t row_elems, int box_bytes,
                                  void* stream) {
    DIN_REQUIRE(n >= 0 && row_elems >= 0 && box_bytes >= 0, "feat_rows_bf16: n = %d, row_elems = %lld, box_bytes = %d must not be negative",
                n, (long long)row_elems, box_bytes);
    DIN_REQUIRE(row_elems % 8 == 0 && box_bytes % 16 == 0,
                "feat_rows_bf16: row_elems = %lld must be a multiple of 8 and box_bytes = %d a multiple of 16", (long long)row_elems, box_bytes);
    DIN_REQUIRE(((uintptr_t)boxes & 15u) == 0, "feat_rows_bf16: boxes must be 16-byte aligned");
    if (n == 0) return DIN_OK;
    DIN_REQUIRE(src && dst, "feat_rows_bf16: null address table with n = %d", n);
    DIN_REQUIRE(!(keep || ref_boxes) || (boxes && flags), "feat_rows_bf16: keep / ref_boxes given without boxes and flags");
    const int64_t row_bytes = 2 * row_elems;                             // of a destination row: what the items are measured in
    const int64_t segs = row_bytes > 0 ? ceil_div64(row_bytes, SEG) : 1, items = segs * (int64_t)n;
    const int grid = (int)(items < GRID_CAP ? items : GRID_CAP);
    hipLaunchKernelGGL(feat_rows_kernel<true>, dim3(grid), dim3(BLOCK), 0, as_stream(stream), src, dst, keep, ref_boxes, src_f32,
                       static_cast<const uint8_t*>(boxes), flags, row_bytes, box_bytes, segs, items);
    DIN_CHECK_LAUNCH("feat_rows_bf16");
    return DIN_OK;
}
