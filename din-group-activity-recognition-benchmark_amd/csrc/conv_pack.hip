// Filter-bank packing for the convolution kernels (fp32 OIHW weights, optionally scaled per filter, -> the packed banks of conv_shared.h's
// pack_geom) and the BatchNorm folds that produce those scales and shifts, with their gradients.  Nothing here is an implicit GEMM.
#include "din_common.h"
#include "conv_shared.h"
#include <stdlib.h>

namespace {

// ------------------------------------------------------------------------------------------------
// weight packing:  w[cout][cin][kh][kw] fp32 (* scale[cout]) -> T[rows_pad][nk*KC*EPC]
//   transposed = 0: row = co, k = (r,s,ci)      (fwd)
//   transposed = 1: row = ci, k = (r,s,co)      (dgrad)
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ void conv_pack_kernel(const float* __restrict__ w, const float* __restrict__ scale, T* __restrict__ out,
                                 int cout, int cin, int kh, int kw, int rows, int rows_pad, int inner, int inner_pad,
                                 int kelems, int transposed) {
    // inner = reduction channels per tap (cin or cout), inner_pad = padded to EPC; kelems = padded row length
    int64_t total = (int64_t)rows_pad * kelems;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int row = (int)(i / kelems), k = (int)(i - (int64_t)row * kelems);
        int tap = k / inner_pad, c = k - tap * inner_pad;
        float v = 0.f;
        if (row < rows && tap < kh * kw && c < inner) {
            int r = tap / kw, s = tap - r * kw;
            int co = transposed ? c : row, ci = transposed ? row : c;
            v = w[(((int64_t)co * cin + ci) * kh + r) * kw + s];
            if (scale) v *= scale[co];
        }
        Elem<T>::st(out + i, v);
    }
}

// 1x1 filter banks (the 26400 x 1024 embedding filter is re-packed twice per step: 108 MB in, 54 MB out per orientation): 64 x 64 tiles
// through LDS, reads coalesced along the filter's contiguous axis (ci), writes coalesced along the packed row -- instead of one element
// per thread with two 64-bit divisions (106 -> ~35 us per orientation).  out[row][k]: row = co (k = ci) or, transposed, row = ci (k = co).
template <typename T>
__global__ __launch_bounds__(256) void conv_pack_1x1_kernel(const float* __restrict__ w, const float* __restrict__ scale, T* __restrict__ out,
                                                            int cout, int cin, int rows_pad, int kelems, int transposed) {
    __shared__ float tile[64][65];
    const int r0 = blockIdx.y * 64, k0 = blockIdx.x * 64;                  // tile of the packed matrix
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;                // 64 x 4
    if (!transposed) {
#pragma unroll 4
        for (int rr = ty; rr < 64; rr += 4) {
            const int co = r0 + rr, ci = k0 + tx;
            float v = 0.f;
            if (co < cout && ci < cin) { v = w[(int64_t)co * cin + ci]; if (scale) v *= scale[co]; }
            if (co < rows_pad && ci < kelems) Elem<T>::st(out + (int64_t)co * kelems + ci, v);
        }
        return;
    }
    // transposed: packed row = ci, packed column = co; read w[co][ci] with ci fastest
#pragma unroll 4
    for (int cc = ty; cc < 64; cc += 4) {
        const int co = k0 + cc, ci = r0 + tx;
        float v = 0.f;
        if (co < cout && ci < cin) { v = w[(int64_t)co * cin + ci]; if (scale) v *= scale[co]; }
        tile[cc][tx] = v;
    }
    __syncthreads();
#pragma unroll 4
    for (int rr = ty; rr < 64; rr += 4) {
        const int ci = r0 + rr, co = k0 + tx;
        if (ci < rows_pad && co < kelems) Elem<T>::st(out + (int64_t)ci * kelems + co, tile[tx][rr]);
    }
}

// every filter bank of a backbone (both orientations) in one launch: workgroup b packs elements [chunk_index[b] * chunk, +chunk) of
// bank layer_of[b]; the table lives on the device and is built once (weights, scales and packed buffers keep their addresses)
__global__ __launch_bounds__(256) void conv_pack_multi_kernel(const din_pack_desc* __restrict__ table, const int32_t* __restrict__ layer_of,
                                                              const int32_t* __restrict__ chunk_index, int chunk) {
    const din_pack_desc d = table[layer_of[blockIdx.x]];
    const float* __restrict__ w = reinterpret_cast<const float*>(d.w);
    const float* __restrict__ scale = reinterpret_cast<const float*>(d.scale);
    const int64_t total = (int64_t)d.rows_pad * d.kelems;
    const int64_t i0 = (int64_t)chunk_index[blockIdx.x] * chunk;
    int64_t i1 = i0 + chunk;
    if (i1 > total) i1 = total;
    const int taps = d.kh * d.kw;
    // (banks below 2^31 elements -- every backbone bank -- take 32-bit index arithmetic: the 64-bit divisions cost more than the traffic)
    const bool small = total < (1ll << 31);
    for (int64_t i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
        int row, k;
        if (small) { row = (int)((uint32_t)i / (uint32_t)d.kelems); k = (int)((uint32_t)i - (uint32_t)row * (uint32_t)d.kelems); }
        else { row = (int)(i / d.kelems); k = (int)(i - (int64_t)row * d.kelems); }
        const int tap = k / d.inner_pad, c = k - tap * d.inner_pad;
        float v = 0.f;
        if (row < d.rows && tap < taps && c < d.inner) {
            const int r = tap / d.kw, s2 = tap - r * d.kw;
            const int co = d.transposed ? c : row, ci = d.transposed ? row : c;
            v = small ? w[(uint32_t)(((co * d.cin + ci) * d.kh + r) * d.kw + s2)] : w[(((int64_t)co * d.cin + ci) * d.kh + r) * d.kw + s2];
            if (scale) v *= scale[co];
        }
        if (d.dtype == DIN_F32) reinterpret_cast<float*>(d.out)[i] = v;
        else reinterpret_cast<bf16_t*>(d.out)[i] = f32_to_bf16(v);
    }
}

__global__ void bn_fold_kernel(const float* gamma, const float* beta, const float* mean, const float* var, float eps,
                               float* scale, float* shift, int c) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < c) {
        float s = gamma[i] / sqrtf(var[i] + eps);
        scale[i] = s;
        shift[i] = beta[i] - mean[i] * s;
    }
}
__global__ void bn_fold_bwd_kernel(const float* wdot, const float* dshift, const float* mean, const float* var, float eps,
                                   float* dgamma, float* dbeta, int c) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < c) {
        float rstd = 1.f / sqrtf(var[i] + eps);
        dgamma[i] = (wdot[i] - dshift[i] * mean[i]) * rstd;
        dbeta[i] = dshift[i];
    }
}

// all BatchNorm layers of a backbone in one launch: ptrs[l] = {gamma, beta, mean, var}, channel l-range = [offs[l], offs[l+1])
__device__ __forceinline__ int bn_layer_of(const int32_t* __restrict__ offs, int n, int i) {
    int lo = 0, hi = n;                                       // offs[lo] <= i < offs[hi]
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (offs[mid] <= i) lo = mid; else hi = mid; }
    return lo;
}
__global__ void bn_fold_multi_kernel(const uint64_t* __restrict__ ptrs, const int32_t* __restrict__ offs, int n, int total, float eps,
                                     float* __restrict__ scale, float* __restrict__ shift) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int l = bn_layer_of(offs, n, i), c = i - offs[l];
    const float* gamma = reinterpret_cast<const float*>(ptrs[4 * l + 0]);
    const float* beta = reinterpret_cast<const float*>(ptrs[4 * l + 1]);
    const float* mean = reinterpret_cast<const float*>(ptrs[4 * l + 2]);
    const float* var = reinterpret_cast<const float*>(ptrs[4 * l + 3]);
    const float s = gamma[c] / sqrtf(var[c] + eps);
    scale[i] = s;
    shift[i] = beta[c] - mean[c] * s;
}
__global__ void bn_fold_bwd_multi_kernel(const uint64_t* __restrict__ ptrs, const int32_t* __restrict__ offs, int n, int total, float eps,
                                         const float* __restrict__ wdot, const float* __restrict__ dshift, float* __restrict__ dgamma,
                                         float* __restrict__ dbeta) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int l = bn_layer_of(offs, n, i), c = i - offs[l];
    const float* mean = reinterpret_cast<const float*>(ptrs[4 * l + 2]);
    const float* var = reinterpret_cast<const float*>(ptrs[4 * l + 3]);
    const float rstd = 1.f / sqrtf(var[c] + eps);
    dgamma[i] = (wdot[i] - dshift[i] * mean[c]) * rstd;
    dbeta[i] = dshift[i];
}

}  // namespace

extern "C" {

int64_t din_conv_packed_elems(const din_conv_desc* d, int transposed) {
    if (!d) return 0;
    const SplitDesc sd(d);
    const PackGeom g = pack_geom(d, transposed);
    return (int64_t)g.rows_pad * g.kelems;
}

int din_conv_pack_weights(const din_conv_desc* d, const float* w, const float* scale, void* wpk, int transposed, void* stream) {
    DIN_REQUIRE(d && w && wpk, "conv_pack: null pointer");
    const SplitDesc sd(d);
    const PackGeom g = pack_geom(d, transposed);
    int64_t total = (int64_t)g.rows_pad * g.kelems;
    hipStream_t st = as_stream(stream);
    if (d->kh == 1 && d->kw == 1 && total >= (1 << 20) && !(DIN_OPT("DIN_PACK_TILES") && atoi(DIN_OPT("DIN_PACK_TILES")) == 0)) {
        // (tap-major k = channel index for a single tap; the padded tail of every row / the padded rows are written as zeros)
        dim3 grid((g.kelems + 63) / 64, (g.rows_pad + 63) / 64);
        if (d->dtype == DIN_F32) hipLaunchKernelGGL(conv_pack_1x1_kernel<float>, grid, dim3(256), 0, st, w, scale, (float*)wpk, d->cout, d->cin, g.rows_pad, g.kelems, transposed);
        else hipLaunchKernelGGL(conv_pack_1x1_kernel<bf16_t>, grid, dim3(256), 0, st, w, scale, (bf16_t*)wpk, d->cout, d->cin, g.rows_pad, g.kelems, transposed);
        DIN_CHECK_LAUNCH("conv_pack(1x1)");
        return DIN_OK;
    }
    if (d->dtype == DIN_F32)
        hipLaunchKernelGGL(conv_pack_kernel<float>, dim3(grid_1d(total, 256)), dim3(256), 0, st, w, scale, (float*)wpk,
                           d->cout, d->cin, d->kh, d->kw, g.cprod, g.rows_pad, g.cred, g.inner_pad, g.kelems, transposed);
    else
        hipLaunchKernelGGL(conv_pack_kernel<bf16_t>, dim3(grid_1d(total, 256)), dim3(256), 0, st, w, scale, (bf16_t*)wpk,
                           d->cout, d->cin, d->kh, d->kw, g.cprod, g.rows_pad, g.cred, g.inner_pad, g.kelems, transposed);
    DIN_CHECK_LAUNCH("conv_pack");
    return DIN_OK;
}

int din_conv_pack_desc(const din_conv_desc* d, const float* w, const float* scale, void* wpk, int transposed, din_pack_desc* out) {
    DIN_REQUIRE(d && w && wpk && out, "conv_pack_desc: null pointer");
    const SplitDesc sd(d);
    const PackGeom g = pack_geom(d, transposed);
    out->w = (uint64_t)(uintptr_t)w; out->scale = (uint64_t)(uintptr_t)scale; out->out = (uint64_t)(uintptr_t)wpk;
    out->cout = d->cout; out->cin = d->cin; out->kh = d->kh; out->kw = d->kw;
    out->rows = g.cprod; out->rows_pad = g.rows_pad; out->inner = g.cred; out->inner_pad = g.inner_pad; out->kelems = g.kelems;
    out->transposed = transposed; out->dtype = d->dtype;
    return DIN_OK;
}

int din_conv_pack_multi(const din_pack_desc* table, const int32_t* layer_of, const int32_t* chunk_index, int nblocks, int chunk_elems,
                        void* stream) {
    DIN_REQUIRE(table && layer_of && chunk_index && nblocks >= 0 && chunk_elems > 0, "conv_pack_multi: bad argument");
    if (nblocks == 0) return DIN_OK;
    hipLaunchKernelGGL(conv_pack_multi_kernel, dim3(nblocks), dim3(256), 0, as_stream(stream), table, layer_of, chunk_index, chunk_elems);
    DIN_CHECK_LAUNCH("conv_pack_multi");
    return DIN_OK;
}

int din_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var, float eps, float* scale,
                float* shift, int c, void* stream) {
    DIN_REQUIRE(gamma && beta && mean && var && scale && shift && c > 0, "bn_fold: bad argument");
    hipLaunchKernelGGL(bn_fold_kernel, dim3((c + 255) / 256), dim3(256), 0, as_stream(stream), gamma, beta, mean, var, eps, scale, shift, c);
    DIN_CHECK_LAUNCH("bn_fold");
    return DIN_OK;
}
int din_bn_fold_bwd(const float* wdot, const float* dshift, const float* mean, const float* var, float eps, float* dgamma,
                    float* dbeta, int c, void* stream) {
    DIN_REQUIRE(wdot && dshift && mean && var && dgamma && dbeta && c > 0, "bn_fold_bwd: bad argument");
    hipLaunchKernelGGL(bn_fold_bwd_kernel, dim3((c + 255) / 256), dim3(256), 0, as_stream(stream), wdot, dshift, mean, var, eps, dgamma, dbeta, c);
    DIN_CHECK_LAUNCH("bn_fold_bwd");
    return DIN_OK;
}

int din_bn_fold_multi(const uint64_t* ptrs, const int32_t* offs, int n, int total, float eps, float* scale, float* shift, void* stream) {
    DIN_REQUIRE(ptrs && offs && scale && shift && n > 0 && total > 0, "bn_fold_multi: bad argument");
    hipLaunchKernelGGL(bn_fold_multi_kernel, dim3((total + 255) / 256), dim3(256), 0, as_stream(stream), ptrs, offs, n, total, eps, scale, shift);
    DIN_CHECK_LAUNCH("bn_fold_multi");
    return DIN_OK;
}
int din_bn_fold_bwd_multi(const uint64_t* ptrs, const int32_t* offs, int n, int total, float eps, const float* wdot, const float* dshift,
                          float* dgamma, float* dbeta, void* stream) {
    DIN_REQUIRE(ptrs && offs && wdot && dshift && dgamma && dbeta && n > 0 && total > 0, "bn_fold_bwd_multi: bad argument");
    hipLaunchKernelGGL(bn_fold_bwd_multi_kernel, dim3((total + 255) / 256), dim3(256), 0, as_stream(stream), ptrs, offs, n, total, eps, wdot,
                       dshift, dgamma, dbeta);
    DIN_CHECK_LAUNCH("bn_fold_bwd_multi");
    return DIN_OK;
}

}  // extern "C"
