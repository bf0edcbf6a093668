// Actor-Transformer block (reference infer_module/AT_infer_module.py:52-96 Embfeature_PositionEmbedding, :119-138 Actor_Transformer up to
// layernorm1), everything around the Q / K / V projection:
//   position   y = x + PE(box centre)  (optionally the mean over the T frames of a clip in the same pass)
//   attention  per group of N <= 16 actors (a frame, or a clip after the T-mean):
//                  A = softmax_rows(Q K^T / sqrt(C));  Z = x + dropout(A V);  out = LayerNorm_C(Z) * gamma + beta
// Q / K / V are three column blocks of ONE projection output (row stride ld), as theta / phi / y are in arg_graph.hip, so the projection and
// both of its gradients stay one contraction each.
//
// VALU + LDS, not the fp32 MFMA: a group is N * N * C <= 16 * 16 * 1024 multiply-adds per product (0.3 MFLOP at the launcher's 12 x 1024),
// there are B * T = 20 groups, and on gfx950 the 16x16x4 fp32 MFMA issues at the same rate as the fp32 VALU; the block's time is launches and
// load latency, not arithmetic.  What the fusion buys is one launch forward and two backward instead of about a dozen library calls each
// way, with A (N x N) in LDS and nothing but A and (mean, rstd) kept for the backward.
//
// One workgroup of 256 threads per group.  The N x N dot products over C go one (i, j) pair per wave (lanes over float4 chunks of the row,
// butterfly sum); everything per column goes one column per thread, all N rows in registers.  The dropout mask is the counter hash of
// din_common.h on the flat element index of the [G, N, C] output, regenerated in the backward.
// House rules of bn.hip / arg_graph.hip: every sum has a fixed order, no atomics, same bits on a rerun.  fp32 throughout.
#include "din_common.h"

namespace {

constexpr int AT_THREADS = 256;
constexpr int AT_WAVES = AT_THREADS / 64;
constexpr int AT_MAX_N = 16;
static_assert(AT_THREADS == AT_MAX_N * AT_MAX_N, "one thread per entry of the N x N tile");

// ---------------------------------------------------------------- position ---------------------------------------------------------------
// PE of column cc for a box with image-px centre (cx, cy): x half first, then y half; inside a half sin on even, cos on odd indices.
// True division and full-precision sinf / cosf: the argument reaches 1280 rad, where one ulp is already 1e-4.
__device__ __forceinline__ float actor_pe(float cx, float cy, const float* __restrict__ dim_t, int half, int cc) {
    const int k = cc < half ? cc : cc - half;
    const float a = (cc < half ? cx : cy) / dim_t[k];
    return (k & 1) ? cosf(a) : sinf(a);
}

// one workgroup per output row ((b, t, n), or (b, n) when pooled over t)
__global__ __launch_bounds__(AT_THREADS) void actor_position_fwd_kernel(
        const float* __restrict__ x, const float* __restrict__ boxes, const float* __restrict__ dim_t, float img_w, float img_h, float out_w,
        float out_h, int t, int n, int c, int pool, float* __restrict__ y) {
    const int64_t row = blockIdx.x;
    const int half = c >> 1;
    if (!pool) {
        const float* bx = boxes + row * 4;
        const float cx = (bx[0] + bx[2]) / 2.f * img_w / out_w, cy = (bx[1] + bx[3]) / 2.f * img_h / out_h;
        for (int cc = threadIdx.x; cc < c; cc += AT_THREADS) y[row * c + cc] = actor_pe(cx, cy, dim_t, half, cc) + x[row * c + cc];
        return;
    }
    const int64_t b = row / n, i = row - b * n;
    for (int cc = threadIdx.x; cc < c; cc += AT_THREADS) {
        float acc = 0.f;
        for (int f = 0; f < t; ++f) {                                  // frames in order
            const int64_t r = (b * t + f) * n + i;
            const float* bx = boxes + r * 4;
            const float cx = (bx[0] + bx[2]) / 2.f * img_w / out_w, cy = (bx[1] + bx[3]) / 2.f * img_h / out_h;
            acc += actor_pe(cx, cy, dim_t, half, cc) + x[r * c + cc];
        }
        y[row * c + cc] = acc / (float)t;
    }
}

// gx [b][t][n][c] = gy [b][t][n][c], or gy [b][n][c] / t when the forward pooled over t
__global__ __launch_bounds__(AT_THREADS) void actor_position_bwd_kernel(const float* __restrict__ gy, int t, int n, int c, int pool,
                                                                        float* __restrict__ gx) {
    const int64_t row = blockIdx.x;                                    // (b, t, n)
    int64_t src = row;
    if (pool) {
        const int64_t b = row / ((int64_t)t * n), i = row % n;
        src = b * n + i;
    }
    for (int cc = threadIdx.x; cc < c; cc += AT_THREADS) {
        const float g = gy[src * c + cc];
        gx[row * c + cc] = pool ? g / (float)t : g;
    }
}

// --------------------------------------------------------------- attention ---------------------------------------------------------------
// <a[0 .. c), b[0 .. c)> over the wave: lane l takes float4 chunks l, l + 64, ...; four chains per lane joined as (x + y) + (z + w), then the
// butterfly.  Every lane gets the sum.
__device__ __forceinline__ float wave_dot(const float4* __restrict__ a, const float4* __restrict__ b, int n4, int lane) {
    float sx = 0.f, sy = 0.f, sz = 0.f, sw = 0.f;
    for (int k = lane; k < n4; k += 64) {
        const float4 u = a[k], v = b[k];
        sx += u.x * v.x;
        sy += u.y * v.y;
        sz += u.z * v.z;
        sw += u.w * v.w;
    }
    return wave_sum((sx + sy) + (sz + sw));
}

// Row sums over the workgroup.  Every thread adds what its columns contribute to row i into its own LDS slot acc[i][tid]: the row loops
// are runtime loops (n is an argument), and a register array indexed by them would live in scratch.  Here the slots of a wave are added by
// the butterfly and the four wave sums in wave order -> dst[i] * scale (dst in LDS, valid after the call).
__device__ __forceinline__ void block_row_sums(const float (*acc)[AT_THREADS], int n, float (*red)[AT_MAX_N], float* dst, float scale) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int i = 0; i < n; ++i) {
        const float s = wave_sum(acc[i][threadIdx.x]);
        if (lane == 0) red[wv][i] = s;
    }
    __syncthreads();
    if (threadIdx.x < n) {
        float s = 0.f;
        for (int w = 0; w < AT_WAVES; ++w) s += red[w][threadIdx.x];
        dst[threadIdx.x] = s * scale;
    }
    __syncthreads();
}

__device__ __forceinline__ void clear_slots(float (*acc)[AT_THREADS], int n) {
    for (int i = 0; i < n; ++i) acc[i][threadIdx.x] = 0.f;
}

// column cc of rows row0 .. row0 + n of a matrix with row stride ld, into registers (0 beyond n)
__device__ __forceinline__ void load_column(const float* m, int64_t row0, int64_t ld, int cc, int n, float (&col)[AT_MAX_N]) {
#pragma unroll
    for (int j = 0; j < AT_MAX_N; ++j) col[j] = j < n ? m[(row0 + j) * ld + cc] : 0.f;
}

// sum_j t[j * sj] * col[j], j in order (forward and backward form (A V) with the same call, hence the same bits)
__device__ __forceinline__ float tile_dot(const float* t, int sj, const float (&col)[AT_MAX_N], int n) {
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < AT_MAX_N; ++j)
        if (j < n) acc += t[j * sj] * col[j];
    return acc;
}

__global__ __launch_bounds__(AT_THREADS) void actor_attn_fwd_kernel(
        const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, int64_t ld, const float* __restrict__ x,
        const float* __restrict__ gamma, const float* __restrict__ beta, float eps, float p, uint64_t seed, const uint64_t* seed_offset,
        int n, int c, float* out, float* __restrict__ att, float* __restrict__ stats, uint8_t* __restrict__ keep) {
    __shared__ float a[AT_MAX_N * AT_MAX_N];
    __shared__ float acc[AT_MAX_N][AT_THREADS];
    __shared__ float red[AT_WAVES][AT_MAX_N];
    __shared__ float mean[AT_MAX_N], rstd[AT_MAX_N];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t row0 = (int64_t)blockIdx.x * n;
    const uint64_t sd = fold_seed(seed, seed_offset);
    const float root = sqrtf((float)c);
    a[tid] = 0.f;                                                      // (AT_THREADS == AT_MAX_N^2)
    clear_slots(acc, n);
    __syncthreads();
    for (int pr = wv; pr < n * n; pr += AT_WAVES) {
        const int i = pr / n, j = pr - i * n;
        const float d = wave_dot(reinterpret_cast<const float4*>(q + (row0 + i) * ld), reinterpret_cast<const float4*>(k + (row0 + j) * ld),
                                 c >> 2, lane);
        if (lane == 0) a[i * AT_MAX_N + j] = d / root;
    }
    __syncthreads();
    if (tid < n) {                                                     // row softmax, the row maximum subtracted
        float* r = a + tid * AT_MAX_N;
        float mx = r[0];
        for (int j = 1; j < n; ++j) mx = fmaxf(mx, r[j]);
        float den = 0.f;
        for (int j = 0; j < n; ++j) {
            r[j] = expf(r[j] - mx);
            den += r[j];
        }
        for (int j = 0; j < n; ++j) {
            r[j] = r[j] / den;
            att[(row0 + tid) * n + j] = r[j];
        }
    }
    __syncthreads();
    // Z = x + dropout(A V) into `out` (each thread re-reads only what it wrote), then the two-pass row statistics and the affine
    for (int cc = tid; cc < c; cc += AT_THREADS) {
        float vcol[AT_MAX_N];
        load_column(v, row0, ld, cc, n, vcol);
#pragma unroll 1
        for (int i = 0; i < n; ++i) {
            const int64_t e = (row0 + i) * c + cc;
            const float ks = keep_scale(sd, e, p);
            const float z = x[e] + ks * tile_dot(a + i * AT_MAX_N, 1, vcol, n);
            out[e] = z;
            if (keep) keep[e] = ks != 0.f ? 1 : 0;
            acc[i][tid] += z;
        }
    }
    block_row_sums(acc, n, red, mean, 1.f / (float)c);
    clear_slots(acc, n);
    for (int cc = tid; cc < c; cc += AT_THREADS) {
#pragma unroll 1
        for (int i = 0; i < n; ++i) {
            const float d = out[(row0 + i) * c + cc] - mean[i];
            acc[i][tid] += d * d;
        }
    }
    block_row_sums(acc, n, red, rstd, 1.f / (float)c);                 // (the variance for now)
    if (tid < n) {
        const float r = 1.f / sqrtf(rstd[tid] + eps);
        stats[(row0 + tid) * 2] = mean[tid];
        stats[(row0 + tid) * 2 + 1] = r;
        rstd[tid] = r;
    }
    __syncthreads();
    for (int cc = tid; cc < c; cc += AT_THREADS) {
        const float ga = gamma[cc], be = beta[cc];
#pragma unroll 1
        for (int i = 0; i < n; ++i) {
            const int64_t e = (row0 + i) * c + cc;
            out[e] = (out[e] - mean[i]) * rstd[i] * ga + be;
        }
    }
}

// dx (gradient of the residual input), dQ / dK / dV (row stride ldg), part[g][0][c] = sum_i gout * zhat, part[g][1][c] = sum_i gout
__global__ __launch_bounds__(AT_THREADS) void actor_attn_bwd_kernel(
        const float* __restrict__ gout, const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, int64_t ld,
        const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ att, const float* __restrict__ stats, float p,
        uint64_t seed, const uint64_t* seed_offset, int n, int c, float* __restrict__ dq, float* __restrict__ dk, float* __restrict__ dv,
        int64_t ldg, float* dx, float* __restrict__ part) {
    __shared__ float a[AT_MAX_N * AT_MAX_N], ds[AT_MAX_N * AT_MAX_N];
    __shared__ float s1[AT_MAX_N][AT_THREADS], s2[AT_MAX_N][AT_THREADS];
    __shared__ float red[AT_WAVES][AT_MAX_N];
    __shared__ float mean[AT_MAX_N], rstd[AT_MAX_N], m1[AT_MAX_N], m2[AT_MAX_N];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t row0 = (int64_t)blockIdx.x * n;
    const uint64_t sd = fold_seed(seed, seed_offset);
    const float root = sqrtf((float)c);
    {
        const int i = tid / AT_MAX_N, j = tid - i * AT_MAX_N;
        a[tid] = (i < n && j < n) ? att[(row0 + i) * n + j] : 0.f;
        ds[tid] = 0.f;
        if (tid < n) {
            mean[tid] = stats[(row0 + tid) * 2];
            rstd[tid] = stats[(row0 + tid) * 2 + 1];
        }
        clear_slots(s1, n);
        clear_slots(s2, n);
    }
    __syncthreads();
    // pass 1: zhat (recomputed; parked in dx), the affine partials of this group, the two row sums of the LayerNorm backward
    for (int cc = tid; cc < c; cc += AT_THREADS) {
        float vcol[AT_MAX_N];
        load_column(v, row0, ld, cc, n, vcol);
        const float ga = gamma[cc];
        float pg = 0.f, pb = 0.f;
#pragma unroll 1
        for (int i = 0; i < n; ++i) {
            const int64_t e = (row0 + i) * c + cc;
            const float z = x[e] + keep_scale(sd, e, p) * tile_dot(a + i * AT_MAX_N, 1, vcol, n);
            const float zh = (z - mean[i]) * rstd[i];
            const float go = gout[e], dzh = go * ga;
            dx[e] = zh;
            pg += go * zh;
            pb += go;
            s1[i][tid] += dzh;
            s2[i][tid] += dzh * zh;
        }
        part[((int64_t)blockIdx.x * 2) * c + cc] = pg;
        part[((int64_t)blockIdx.x * 2 + 1) * c + cc] = pb;
    }
    block_row_sums(s1, n, red, m1, 1.f / (float)c);
    block_row_sums(s2, n, red, m2, 1.f / (float)c);
    // pass 2: dZ, which is also the gradient of the residual input
    for (int cc = tid; cc < c; cc += AT_THREADS) {
        const float ga = gamma[cc];
#pragma unroll 1
        for (int i = 0; i < n; ++i) {
            const int64_t e = (row0 + i) * c + cc;
            dx[e] = rstd[i] * (gout[e] * ga - m1[i] - dx[e] * m2[i]);
        }
    }
    __syncthreads();                                                   // dx of the whole group is visible to the workgroup
    // dA[i][j] = <dZ_i o keep_i, V_j>;  dS = A o (dA - rowsum(dA o A)) / sqrt(C)
    for (int pr = wv; pr < n * n; pr += AT_WAVES) {
        const int i = pr / n, j = pr - i * n;
        const float4* dz4 = reinterpret_cast<const float4*>(dx + (row0 + i) * c);
        const float4* v4 = reinterpret_cast<const float4*>(v + (row0 + j) * ld);
        float sx = 0.f, sy = 0.f, sz = 0.f, sw = 0.f;
        for (int k4 = lane; k4 < (c >> 2); k4 += 64) {
            const float4 u = dz4[k4], w = v4[k4];
            const int64_t e = (row0 + i) * c + 4 * k4;
            sx += u.x * keep_scale(sd, e, p) * w.x;
            sy += u.y * keep_scale(sd, e + 1, p) * w.y;
            sz += u.z * keep_scale(sd, e + 2, p) * w.z;
            sw += u.w * keep_scale(sd, e + 3, p) * w.w;
        }
        const float d = wave_sum((sx + sy) + (sz + sw));
        if (lane == 0) ds[i * AT_MAX_N + j] = d;
    }
    __syncthreads();
    if (tid < n) {
        float* r = ds + tid * AT_MAX_N;
        const float* ar = a + tid * AT_MAX_N;
        float t = 0.f;
        for (int j = 0; j < n; ++j) t += r[j] * ar[j];
        for (int j = 0; j < n; ++j) r[j] = ar[j] * (r[j] - t) / root;
    }
    __syncthreads();
    // dQ = dS K,  dK = dS^T Q,  dV = A^T (dZ o keep): one column per thread, one operand column in registers at a time
    for (int cc = tid; cc < c; cc += AT_THREADS) {
        float col[AT_MAX_N];
        load_column(k, row0, ld, cc, n, col);
#pragma unroll 1
        for (int i = 0; i < n; ++i) dq[(row0 + i) * ldg + cc] = tile_dot(ds + i * AT_MAX_N, 1, col, n);
        load_column(q, row0, ld, cc, n, col);
#pragma unroll 1
        for (int i = 0; i < n; ++i) dk[(row0 + i) * ldg + cc] = tile_dot(ds + i, AT_MAX_N, col, n);
        load_column(dx, row0, c, cc, n, col);
#pragma unroll
        for (int j = 0; j < AT_MAX_N; ++j)
            if (j < n) col[j] *= keep_scale(sd, (row0 + j) * c + cc, p);
#pragma unroll 1
        for (int i = 0; i < n; ++i) dv[(row0 + i) * ldg + cc] = tile_dot(a + i, AT_MAX_N, col, n);
    }
}

// d gamma [c] / d beta [c]: one thread per column, groups added in order
__global__ __launch_bounds__(AT_THREADS) void actor_attn_affine_reduce_kernel(const float* __restrict__ part, int g, int c,
                                                                              float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int cc = blockIdx.x * AT_THREADS + threadIdx.x;
    if (cc >= c) return;
    float dg = 0.f, db = 0.f;
    for (int i = 0; i < g; ++i) {
        dg += part[((int64_t)i * 2) * c + cc];
        db += part[((int64_t)i * 2 + 1) * c + cc];
    }
    dgamma[cc] = dg;
    dbeta[cc] = db;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }    // (a null pointer passes: nullable arguments)

int check_attn_shape(const char* what, int64_t ld, int g, int n, int c, float p) {
    DIN_REQUIRE(g >= 1 && n >= 1 && n <= AT_MAX_N, "%s: bad shape (g %d, n %d outside 1..%d)", what, g, n, AT_MAX_N);
    DIN_REQUIRE(c >= 4 && c % 4 == 0, "%s: c %d must be a positive multiple of 4", what, c);
    DIN_REQUIRE(ld % 4 == 0 && ld >= c, "%s: row stride %lld must be a multiple of 4 and hold c columns", what, (long long)ld);
    DIN_REQUIRE(p >= 0.f && p < 1.f, "%s: dropout probability %g outside [0, 1)", what, (double)p);
    return DIN_OK;
}

}  // namespace

extern "C" {

int din_actor_position_fwd(const float* x, const float* boxes, const float* dim_t, float img_w, float img_h, float out_w, float out_h,
                           int b, int t, int n, int c, int pool_t, float* y, void* stream) {
    DIN_REQUIRE(x && boxes && dim_t && y, "actor_position_fwd: null pointer");
    DIN_REQUIRE(b >= 1 && t >= 1 && n >= 1 && (int64_t)b * t * n <= 0x7FFFFFFF, "actor_position_fwd: bad shape (b %d, t %d, n %d)", b, t, n);
    DIN_REQUIRE(c >= 4 && c % 4 == 0, "actor_position_fwd: c %d must be a positive multiple of 4 (sin / cos pairs in each half)", c);
    DIN_REQUIRE(img_w > 0.f && img_h > 0.f && out_w > 0.f && out_h > 0.f, "actor_position_fwd: image / feature-map size must be positive");
    DIN_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)boxes & 3) == 0 && ((uintptr_t)dim_t & 3) == 0 && ((uintptr_t)y & 3) == 0,
                "actor_position_fwd: misaligned pointer");
    const unsigned rows = (unsigned)(pool_t ? (int64_t)b * n : (int64_t)b * t * n);
    hipLaunchKernelGGL(actor_position_fwd_kernel, dim3(rows), dim3(AT_THREADS), 0, as_stream(stream), x, boxes, dim_t, img_w, img_h, out_w,
                       out_h, t, n, c, pool_t ? 1 : 0, y);
    DIN_CHECK_LAUNCH("actor_position_fwd");
    return DIN_OK;
}

int din_actor_position_bwd(const float* gy, int b, int t, int n, int c, int pool_t, float* gx, void* stream) {
    DIN_REQUIRE(gy && gx, "actor_position_bwd: null pointer");
    DIN_REQUIRE(b >= 1 && t >= 1 && n >= 1 && (int64_t)b * t * n <= 0x7FFFFFFF, "actor_position_bwd: bad shape (b %d, t %d, n %d)", b, t, n);
    DIN_REQUIRE(c >= 4 && c % 4 == 0, "actor_position_bwd: c %d must be a positive multiple of 4", c);
    DIN_REQUIRE(((uintptr_t)gy & 3) == 0 && ((uintptr_t)gx & 3) == 0, "actor_position_bwd: misaligned pointer");
    hipLaunchKernelGGL(actor_position_bwd_kernel, dim3((unsigned)((int64_t)b * t * n)), dim3(AT_THREADS), 0, as_stream(stream), gy, t, n, c,
                       pool_t ? 1 : 0, gx);
    DIN_CHECK_LAUNCH("actor_position_bwd");
    return DIN_OK;
}

int din_actor_attn_fwd(const float* q, const float* k, const float* v, int64_t ld, const float* x, const float* gamma, const float* beta,
                       float eps, float drop_p, uint64_t seed, const uint64_t* seed_offset, int g, int n, int c, float* out, float* att,
                       float* stats, uint8_t* keep, void* stream) {
    DIN_REQUIRE(q && k && v && x && gamma && beta && out && att && stats, "actor_attn_fwd: null pointer");
    int rc = check_attn_shape("actor_attn_fwd", ld, g, n, c, drop_p);
    if (rc != DIN_OK) return rc;
    DIN_REQUIRE(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(x) && aligned16(out), "actor_attn_fwd: q / k / v / x / out must be "
                "16-byte aligned");
    DIN_REQUIRE(aligned4(gamma) && aligned4(beta) && aligned4(att) && aligned4(stats) && ((uintptr_t)seed_offset & 7) == 0,
                "actor_attn_fwd: misaligned gamma / beta / att / stats / seed_offset");
    hipLaunchKernelGGL(actor_attn_fwd_kernel, dim3(g), dim3(AT_THREADS), 0, as_stream(stream), q, k, v, ld, x, gamma, beta, eps, drop_p, seed,
                       seed_offset, n, c, out, att, stats, keep);
    DIN_CHECK_LAUNCH("actor_attn_fwd");
    return DIN_OK;
}

int din_actor_attn_bwd(const float* g_out, const float* q, const float* k, const float* v, int64_t ld, const float* x, const float* gamma,
                       const float* att, const float* stats, float drop_p, uint64_t seed, const uint64_t* seed_offset, int g, int n, int c,
                       float* d_q, float* d_k, float* d_v, int64_t ld_grad, float* d_x, float* d_gamma, float* d_beta, float* ws,
                       int64_t ws_floats, void* stream) {
    DIN_REQUIRE(g_out && q && k && v && x && gamma && att && stats && d_q && d_k && d_v && d_x && d_gamma && d_beta && ws,
                "actor_attn_bwd: null pointer");
    int rc = check_attn_shape("actor_attn_bwd", ld, g, n, c, drop_p);
    if (rc != DIN_OK) return rc;
    rc = check_attn_shape("actor_attn_bwd (gradient)", ld_grad, g, n, c, drop_p);
    if (rc != DIN_OK) return rc;
    DIN_REQUIRE(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(x) && aligned16(g_out) && aligned16(d_q) && aligned16(d_k) &&
                aligned16(d_v) && aligned16(d_x), "actor_attn_bwd: q / k / v / x / g_out and the gradients must be 16-byte aligned");
    DIN_REQUIRE(aligned4(gamma) && aligned4(att) && aligned4(stats) && aligned4(d_gamma) && aligned4(d_beta) && aligned4(ws) &&
                ((uintptr_t)seed_offset & 7) == 0, "actor_attn_bwd: misaligned gamma / att / stats / d_gamma / d_beta / ws / seed_offset");
    DIN_REQUIRE(ws_floats >= (int64_t)g * 2 * c, "actor_attn_bwd: workspace of %lld floats, %lld needed", (long long)ws_floats,
                (long long)g * 2 * c);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(actor_attn_bwd_kernel, dim3(g), dim3(AT_THREADS), 0, st, g_out, q, k, v, ld, x, gamma, att, stats, drop_p, seed,
                       seed_offset, n, c, d_q, d_k, d_v, ld_grad, d_x, ws);
    DIN_CHECK_LAUNCH("actor_attn_bwd");
    hipLaunchKernelGGL(actor_attn_affine_reduce_kernel, dim3((c + AT_THREADS - 1) / AT_THREADS), dim3(AT_THREADS), 0, st, ws, g, c, d_gamma,
                       d_beta);
    DIN_CHECK_LAUNCH("actor_attn_affine_reduce");
    return DIN_OK;
}

}  // extern "C"
