// Actor Relation Graph block (reference infer_module/ARG_infer_module.py:46-89 GCN_Module), everything after the projections:
//   per (clip b, graph g):  S = theta_g phi_g^T / sqrt(NFR);  S[i][j] = -inf where dist(centre_i, centre_j) > thr (i != j);
//                           R = softmax_rows(S);  Z = R Y_g;  V = relu(LayerNorm_[TN,NFG](Z) * gamma_g + beta_g)
//   out[b] = sum_g V_g  (g in order 0 .. NG-1)
// theta / phi / Y are column slices of ONE projection output (row stride ld): Y_g = X W_g^T was formed before the graph is applied,
// R (X W^T) == (R X) W^T.
//
// TWO-PASS form (statistics, then apply), not an LDS-resident slab: a (clip, graph) slab of Z is TN x NFG floats (144 KB at 36 x 1024) and
// would pin one workgroup per CU, B * NG of them in all -- 32 workgroups for 256 CUs at the ARG launcher's batch of 2.  Splitting a slab
// over 64-column chunks gives B * NG * NFG / 64 workgroups (512 at that batch), each needing R and a TN x 64 tile of Y in LDS
// (14 KB at TN = 36, 88 KB at TN = 120); the price is one round trip of Z through memory (it is kept for the backward anyway).
//
// Forward, 4 launches:   relation  (B*NG x TN/4 workgroups; a wave per row i, lanes over j: scores, mask, row softmax -> R, mask)
//                        aggregate (NFG/64 x B*NG: Z tile = R Y tile, written; per-workgroup (count, mean, M2) of its tile)
//                        stats     (a thread per (b, g): Chan-combines its tile statistics in chunk order -> mean, rstd)
//                        norm_sum  (per (b, i, 256 columns): normalises, applies gamma / beta / ReLU and adds the NG graphs in order)
// Backward, 5 launches:  ln_sums   (per tile: sum dzhat, sum dzhat * zhat)          affine (d gamma, d beta: clips added in order)
//                        dz        (dZ tile -> memory; dY tile = R^T dZ tile)        relation_bwd (dR = dZ Y^T, softmax backward -> dS)
//                        proj      (d theta = dS phi / sqrt(NFR), d phi = dS^T theta / sqrt(NFR))
// House rules of bn.hip / basenet_head.hip: every sum has a fixed order, no atomics, same bits on a rerun.  fp32 throughout.
#include "din_common.h"

namespace {

constexpr int AG_THREADS = 256;
constexpr int AG_WAVES = AG_THREADS / 64;
constexpr int AG_MAX_TN = 120;
constexpr int AG_MAX_NG = 1024;
constexpr int AG_COLS = 64;                                   // columns of one aggregate / dz / proj tile (one per lane)
constexpr int AG_ROWS = (AG_MAX_TN + AG_WAVES - 1) / AG_WAVES;   // rows a wave owns at most (row i belongs to wave i % 4)

// centre of box (x1, y1, x2, y2) after `rounds` applications of the reference's in-place update col0 = (col0 + col2) / 2,
// col1 = (col1 + col3) / 2 (ARG_infer_module.py:48-49 runs once per GCN layer on the caller's tensor: layer l sees l + 1 rounds)
__device__ __forceinline__ void box_centre(const float* bx, int rounds, float& cx, float& cy) {
    float x = bx[0], y = bx[1];
    const float x2 = bx[2], y2 = bx[3];
    for (int r = 0; r < rounds; ++r) {
        x = (x + x2) / 2.f;
        y = (y + y2) / 2.f;
    }
    cx = x;
    cy = y;
}

// sum over the workgroup, the four wave sums added in wave order; every thread gets the result.  `red` is reusable after the call.
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.f;
    for (int w = 0; w < AG_WAVES; ++w) t += red[w];
    return t;
}

// <a[0 .. n4*4), p[0 .. n4*4)>: four independent chains (one per float4 component, sequential in k), joined as (x + y) + (z + w)
__device__ __forceinline__ float dot4(const float4* __restrict__ a, const float4* __restrict__ p, int n4) {
    float sx = 0.f, sy = 0.f, sz = 0.f, sw = 0.f;
    for (int k = 0; k < n4; ++k) {
        const float4 u = a[k], v = p[k];
        sx += u.x * v.x;
        sy += u.y * v.y;
        sz += u.z * v.z;
        sw += u.w * v.w;
    }
    return (sx + sy) + (sz + sw);
}

// ---------------------------------------------------------------- forward ----------------------------------------------------------------
__global__ __launch_bounds__(AG_THREADS) void arg_relation_kernel(
        const float* __restrict__ theta, const float* __restrict__ phi, int64_t ld, const float* __restrict__ boxes, int rounds, float thr,
        int tn, int ng, int nfr, float* __restrict__ rel, uint8_t* __restrict__ mask) {
    __shared__ float cx[AG_MAX_TN], cy[AG_MAX_TN];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int bg = blockIdx.x, b = bg / ng, g = bg - b * ng;
    for (int i = tid; i < tn; i += AG_THREADS) box_centre(boxes + ((int64_t)b * tn + i) * 4, rounds, cx[i], cy[i]);
    __syncthreads();
    const float* th = theta + (int64_t)b * tn * ld + (int64_t)g * nfr;
    const float* ph = phi + (int64_t)b * tn * ld + (int64_t)g * nfr;
    const float root = sqrtf((float)nfr);
    const int n4 = nfr >> 2;
    const int j0 = lane, j1 = lane + 64;
    const bool v0 = j0 < tn, v1 = j1 < tn;
    for (int i = blockIdx.y * AG_WAVES + wv; i < tn; i += AG_WAVES * gridDim.y) {     // (grid y = row blocks: one row per wave)
        const float4* a = reinterpret_cast<const float4*>(th + (int64_t)i * ld);
        float s0 = -INFINITY, s1 = -INFINITY;
        bool m0 = false, m1 = false;
        if (v0) {
            const float dx = cx[i] - cx[j0], dy = cy[i] - cy[j0];
            m0 = j0 != i && sqrtf(dx * dx + dy * dy) > thr;          // strict; the diagonal is always kept, a NaN distance is not masked
            if (!m0) s0 = dot4(a, reinterpret_cast<const float4*>(ph + (int64_t)j0 * ld), n4) / root;
        }
        if (v1) {
            const float dx = cx[i] - cx[j1], dy = cy[i] - cy[j1];
            m1 = j1 != i && sqrtf(dx * dx + dy * dy) > thr;
            if (!m1) s1 = dot4(a, reinterpret_cast<const float4*>(ph + (int64_t)j1 * ld), n4) / root;
        }
        const float mx = wave_max(fmaxf(s0, s1));                     // finite: column i of row i is kept
        const float e0 = (v0 && !m0) ? expf(s0 - mx) : 0.f;
        const float e1 = (v1 && !m1) ? expf(s1 - mx) : 0.f;
        const float den = wave_sum(e0 + e1);
        float* r = rel + ((int64_t)bg * tn + i) * tn;
        if (v0) r[j0] = e0 / den;
        if (v1) r[j1] = e1 / den;
        if (g == 0) {
            uint8_t* m = mask + ((int64_t)b * tn + i) * tn;
            if (v0) m[j0] = m0 ? 1 : 0;
            if (v1) m[j1] = m1 ? 1 : 0;
        }
    }
}

// Z tile [tn][64] of (b, g) = R [tn][tn] x Y tile [tn][64]; part[(bg * nchunk + chunk) * 3] = (count, mean, M2) of the tile
__global__ __launch_bounds__(AG_THREADS) void arg_aggregate_kernel(
        const float* __restrict__ y, int64_t ld, const float* __restrict__ rel, int tn, int ng, int nfg, int nchunk, float* __restrict__ z,
        float* __restrict__ part) {
    extern __shared__ float ag_lds[];
    float* rl = ag_lds;                                       // [tn][tn]
    float* yl = ag_lds + tn * tn;                             // [tn][64]
    __shared__ float red[AG_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int chunk = blockIdx.x, bg = blockIdx.y, b = bg / ng, g = bg - b * ng;
    const int c = chunk * AG_COLS + lane;
    const bool live = c < nfg;
    for (int e = tid; e < tn * tn; e += AG_THREADS) rl[e] = rel[(int64_t)bg * tn * tn + e];
    const float* yg = y + (int64_t)b * tn * ld + (int64_t)g * nfg;
    for (int j = wv; j < tn; j += AG_WAVES) yl[j * AG_COLS + lane] = live ? yg[(int64_t)j * ld + c] : 0.f;
    __syncthreads();
    float zr[AG_ROWS];
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < AG_ROWS; ++r) {
        const int i = wv + r * AG_WAVES;
        float acc = 0.f;
        if (i < tn) {
            for (int j = 0; j < tn; ++j) acc += rl[i * tn + j] * yl[j * AG_COLS + lane];
            if (live) z[((int64_t)bg * tn + i) * nfg + c] = acc;
        }
        zr[r] = acc;
        sum += acc;                                           // (0 for a dead column or row)
    }
    const int cols = min(AG_COLS, nfg - chunk * AG_COLS);
    const float cnt = (float)tn * (float)cols;
    const float mean = block_sum(sum, red) / cnt;
    float m2 = 0.f;
#pragma unroll
    for (int r = 0; r < AG_ROWS; ++r) {
        const int i = wv + r * AG_WAVES;
        const float d = zr[r] - mean;
        if (i < tn && live) m2 += d * d;
    }
    m2 = block_sum(m2, red);
    if (tid == 0) {
        float* p = part + ((int64_t)bg * nchunk + chunk) * 3;
        p[0] = cnt;
        p[1] = mean;
        p[2] = m2;
    }
}

// mean / rstd of slab bg from its tiles' (count, mean, M2), combined in chunk order (Chan et al.)
__device__ __forceinline__ void combine_stats(const float* __restrict__ part, int64_t bg, int nchunk, float eps, float& mean, float& rstd) {
    float n = 0.f, mu = 0.f, m2 = 0.f;
    for (int k = 0; k < nchunk; ++k) {
        const float* p = part + (bg * nchunk + k) * 3;
        const float nb = p[0], d = p[1] - mu, tot = n + nb;
        mu += d * nb / tot;
        m2 += p[2] + d * d * n * nb / tot;
        n = tot;
    }
    mean = mu;
    rstd = 1.f / sqrtf(m2 / n + eps);
}

// stats[bg] = (mean, rstd) of slab bg: one thread per (clip, graph)
__global__ __launch_bounds__(AG_THREADS) void arg_stats_kernel(const float* __restrict__ part, int nbg, int nchunk, float eps,
                                                               float* __restrict__ stats) {
    const int bg = blockIdx.x * AG_THREADS + threadIdx.x;
    if (bg >= nbg) return;
    float mean, rstd;
    combine_stats(part, bg, nchunk, eps, mean, rstd);
    stats[2 * bg] = mean;
    stats[2 * bg + 1] = rstd;
}

__global__ __launch_bounds__(AG_THREADS) void arg_norm_sum_kernel(
        const float* __restrict__ z, const float* __restrict__ stats, const float* __restrict__ gamma, const float* __restrict__ beta,
        int tn, int ng, int nfg, float* __restrict__ out) {
    const int i = blockIdx.y, b = blockIdx.z;
    const int c = blockIdx.x * AG_THREADS + threadIdx.x;
    if (c >= nfg) return;
    float acc = 0.f;
    for (int g = 0; g < ng; ++g) {
        const int64_t bg = (int64_t)b * ng + g;
        const float zh = (z[(bg * tn + i) * nfg + c] - stats[2 * bg]) * stats[2 * bg + 1];      // (wave-uniform loads)
        const int64_t a = ((int64_t)g * tn + i) * nfg + c;
        acc += fmaxf(zh * gamma[a] + beta[a], 0.f);
    }
    out[((int64_t)b * tn + i) * nfg + c] = acc;
}

// ---------------------------------------------------------------- backward ---------------------------------------------------------------
// gradient reaching zhat at (bg, i, c), and zhat itself
__device__ __forceinline__ float dzhat_at(const float* __restrict__ z, const float* __restrict__ gout, const float* __restrict__ gamma,
                                          const float* __restrict__ beta, float mean, float rstd, int64_t zi, int64_t oi, int64_t ai,
                                          float& zh) {
    zh = (z[zi] - mean) * rstd;
    const float ga = gamma[ai];
    const float v = zh * ga + beta[ai];
    return v > 0.f ? gout[oi] * ga : 0.f;
}

// part2[(bg * nchunk + chunk) * 2] = (sum dzhat, sum dzhat * zhat) over the tile
__global__ __launch_bounds__(AG_THREADS) void arg_bwd_ln_sums_kernel(
        const float* __restrict__ z, const float* __restrict__ gout, const float* __restrict__ gamma, const float* __restrict__ beta,
        const float* __restrict__ stats, int tn, int ng, int nfg, int nchunk, float* __restrict__ part2) {
    __shared__ float red[AG_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int chunk = blockIdx.x, bg = blockIdx.y, b = bg / ng, g = bg - b * ng;
    const int c = chunk * AG_COLS + lane;
    const float mean = stats[2 * bg], rstd = stats[2 * bg + 1];
    float s1 = 0.f, s2 = 0.f;
    if (c < nfg)
        for (int i = wv; i < tn; i += AG_WAVES) {
            float zh;
            const float d = dzhat_at(z, gout, gamma, beta, mean, rstd, ((int64_t)bg * tn + i) * nfg + c, ((int64_t)b * tn + i) * nfg + c,
                                     ((int64_t)g * tn + i) * nfg + c, zh);
            s1 += d;
            s2 += d * zh;
        }
    s1 = block_sum(s1, red);
    s2 = block_sum(s2, red);
    if (tid == 0) {
        part2[((int64_t)bg * nchunk + chunk) * 2] = s1;
        part2[((int64_t)bg * nchunk + chunk) * 2 + 1] = s2;
    }
}

// d gamma / d beta [ng][tn][nfg]: one thread per element, clips in order
__global__ __launch_bounds__(AG_THREADS) void arg_bwd_affine_kernel(
        const float* __restrict__ z, const float* __restrict__ gout, const float* __restrict__ gamma, const float* __restrict__ beta,
        const float* __restrict__ stats, int nb, int tn, int ng, int nfg, float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int64_t per_g = (int64_t)tn * nfg;
    const int64_t e = (int64_t)blockIdx.x * AG_THREADS + threadIdx.x;
    if (e >= per_g * ng) return;
    const int g = (int)(e / per_g);
    const int64_t ic = e - (int64_t)g * per_g;
    const float ga = gamma[e], be = beta[e];
    float dg = 0.f, db = 0.f;
    for (int b = 0; b < nb; ++b) {
        const int64_t bg = (int64_t)b * ng + g;
        const float zh = (z[bg * per_g + ic] - stats[2 * bg]) * stats[2 * bg + 1];
        const float dv = zh * ga + be > 0.f ? gout[(int64_t)b * per_g + ic] : 0.f;
        dg += dv * zh;
        db += dv;
    }
    dgamma[e] = dg;
    dbeta[e] = db;
}

// dZ tile (LayerNorm backward over the whole slab) -> dz; dY tile = R^T dZ tile -> dy (row stride ld)
__global__ __launch_bounds__(AG_THREADS) void arg_bwd_dz_kernel(
        const float* __restrict__ z, const float* __restrict__ gout, const float* __restrict__ gamma, const float* __restrict__ beta,
        const float* __restrict__ stats, const float* __restrict__ part2, const float* __restrict__ rel, int tn, int ng, int nfg, int nchunk,
        float* __restrict__ dz, float* __restrict__ dy, int64_t ld) {
    extern __shared__ float ag_lds[];
    float* rl = ag_lds;                                       // [tn][tn]
    float* dl = ag_lds + tn * tn;                             // [tn][64]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int chunk = blockIdx.x, bg = blockIdx.y, b = bg / ng, g = bg - b * ng;
    const int c = chunk * AG_COLS + lane;
    const bool live = c < nfg;
    float s1 = 0.f, s2 = 0.f;
    for (int k = 0; k < nchunk; ++k) {                        // every thread forms the same sums in the same order
        s1 += part2[((int64_t)bg * nchunk + k) * 2];
        s2 += part2[((int64_t)bg * nchunk + k) * 2 + 1];
    }
    const float inv = 1.f / ((float)tn * (float)nfg);
    const float m1 = s1 * inv, m2 = s2 * inv;
    const float mean = stats[2 * bg], rstd = stats[2 * bg + 1];
    for (int e = tid; e < tn * tn; e += AG_THREADS) rl[e] = rel[(int64_t)bg * tn * tn + e];
    for (int i = wv; i < tn; i += AG_WAVES) {
        float v = 0.f;
        if (live) {
            float zh;
            const int64_t zi = ((int64_t)bg * tn + i) * nfg + c;
            const float d = dzhat_at(z, gout, gamma, beta, mean, rstd, zi, ((int64_t)b * tn + i) * nfg + c, ((int64_t)g * tn + i) * nfg + c, zh);
            v = rstd * (d - m1 - zh * m2);
            dz[zi] = v;
        }
        dl[i * AG_COLS + lane] = v;
    }
    __syncthreads();
    if (!live) return;
    float* dyg = dy + (int64_t)b * tn * ld + (int64_t)g * nfg;
    for (int j = wv; j < tn; j += AG_WAVES) {
        float acc = 0.f;
        for (int i = 0; i < tn; ++i) acc += rl[i * tn + j] * dl[i * AG_COLS + lane];
        dyg[(int64_t)j * ld + c] = acc;
    }
}

// dR[i][j] = <dZ[i], Y[j]>;  dS = R o (dR - rowsum(dR o R)) / sqrt(NFR)  (masked entries have R == 0)
__global__ __launch_bounds__(AG_THREADS) void arg_bwd_relation_kernel(
        const float* __restrict__ dz, const float* __restrict__ y, int64_t ld, const float* __restrict__ rel, int tn, int ng, int nfr, int nfg,
        float* __restrict__ ds) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int bg = blockIdx.x, b = bg / ng, g = bg - b * ng;
    const float* yg = y + (int64_t)b * tn * ld + (int64_t)g * nfg;
    const float root = sqrtf((float)nfr);
    const int n4 = nfg >> 2;
    const int j0 = lane, j1 = lane + 64;
    const bool v0 = j0 < tn, v1 = j1 < tn;
    for (int i = blockIdx.y * AG_WAVES + wv; i < tn; i += AG_WAVES * gridDim.y) {
        const float4* a = reinterpret_cast<const float4*>(dz + ((int64_t)bg * tn + i) * nfg);
        const float* r = rel + ((int64_t)bg * tn + i) * tn;
        const float r0 = v0 ? r[j0] : 0.f, r1 = v1 ? r[j1] : 0.f;
        const float d0 = r0 != 0.f ? dot4(a, reinterpret_cast<const float4*>(yg + (int64_t)j0 * ld), n4) : 0.f;
        const float d1 = r1 != 0.f ? dot4(a, reinterpret_cast<const float4*>(yg + (int64_t)j1 * ld), n4) : 0.f;
        const float t = wave_sum(d0 * r0 + d1 * r1);
        float* o = ds + ((int64_t)bg * tn + i) * tn;
        if (v0) o[j0] = r0 * (d0 - t) / root;
        if (v1) o[j1] = r1 * (d1 - t) / root;
    }
}

// d theta tile [tn][64] = dS phi tile, d phi tile = dS^T theta tile (columns k of graph g; row stride ld)
__global__ __launch_bounds__(AG_THREADS) void arg_bwd_proj_kernel(
        const float* __restrict__ ds, const float* __restrict__ theta, const float* __restrict__ phi, int64_t ld, int tn, int ng, int nfr,
        float* __restrict__ dtheta, float* __restrict__ dphi, int64_t ldg) {
    extern __shared__ float ag_lds[];
    float* sl = ag_lds;                                       // [tn][tn]
    float* tl = sl + tn * tn;                                 // [tn][64] theta
    float* pl = tl + tn * AG_COLS;                            // [tn][64] phi
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int chunk = blockIdx.x, bg = blockIdx.y, b = bg / ng, g = bg - b * ng;
    const int k = chunk * AG_COLS + lane;
    const bool live = k < nfr;
    const int64_t base = (int64_t)b * tn * ld + (int64_t)g * nfr, gbase = (int64_t)b * tn * ldg + (int64_t)g * nfr;
    for (int e = tid; e < tn * tn; e += AG_THREADS) sl[e] = ds[(int64_t)bg * tn * tn + e];
    for (int i = wv; i < tn; i += AG_WAVES) {
        tl[i * AG_COLS + lane] = live ? theta[base + (int64_t)i * ld + k] : 0.f;
        pl[i * AG_COLS + lane] = live ? phi[base + (int64_t)i * ld + k] : 0.f;
    }
    __syncthreads();
    if (!live) return;
    for (int i = wv; i < tn; i += AG_WAVES) {
        float at = 0.f, ap = 0.f;
        for (int j = 0; j < tn; ++j) {
            at += sl[i * tn + j] * pl[j * AG_COLS + lane];
            ap += sl[j * tn + i] * tl[j * AG_COLS + lane];
        }
        dtheta[gbase + (int64_t)i * ldg + k] = at;
        dphi[gbase + (int64_t)i * ldg + k] = ap;
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int check_shape(const char* what, int64_t ld, int b, int tn, int ng, int nfr, int nfg) {
    DIN_REQUIRE(b > 0 && ng >= 1 && ng <= AG_MAX_NG && tn >= 1 && tn <= AG_MAX_TN, "%s: bad shape (b %d, ng %d outside 1..%d, tn %d outside 1..%d)",
                what, b, ng, AG_MAX_NG, tn, AG_MAX_TN);
    DIN_REQUIRE(nfr >= 4 && nfr % 4 == 0 && nfg >= 4 && nfg % 4 == 0, "%s: nfr %d / nfg %d must be positive multiples of 4", what, nfr, nfg);
    DIN_REQUIRE(ld % 4 == 0 && ld >= (int64_t)ng * nfg && ld >= (int64_t)ng * nfr, "%s: row stride %lld must be a multiple of 4 and hold "
                "ng * nfr and ng * nfg columns", what, (long long)ld);
    DIN_REQUIRE((int64_t)b * ng <= 65535 && (int64_t)b <= 65535, "%s: b * ng %lld above the grid limit 65535", what, (long long)b * ng);
    return DIN_OK;
}

}  // namespace

extern "C" {

int din_arg_graph_fwd(const float* theta, const float* phi, const float* y, int64_t ld, const float* boxes, int centre_rounds, float thr,
                      const float* gamma, const float* beta, float eps, int b, int tn, int ng, int nfr, int nfg, float* out, float* rel,
                      uint8_t* mask, float* z, float* stats, float* ws, int64_t ws_floats, void* stream) {
    DIN_REQUIRE(theta && phi && y && boxes && gamma && beta && out && rel && mask && z && stats && ws, "arg_graph_fwd: null pointer");
    int rc = check_shape("arg_graph_fwd", ld, b, tn, ng, nfr, nfg);
    if (rc != DIN_OK) return rc;
    DIN_REQUIRE(aligned16(theta) && aligned16(phi), "arg_graph_fwd: theta / phi must be 16-byte aligned");
    DIN_REQUIRE(centre_rounds >= 0 && centre_rounds <= 64, "arg_graph_fwd: centre_rounds %d outside 0..64", centre_rounds);
    DIN_REQUIRE(thr >= 0.f, "arg_graph_fwd: threshold %g is negative (or NaN)", (double)thr);
    const int nchunk = (nfg + AG_COLS - 1) / AG_COLS;
    DIN_REQUIRE(ws_floats >= (int64_t)b * ng * nchunk * 3, "arg_graph_fwd: workspace of %lld floats, %lld needed", (long long)ws_floats,
                (long long)b * ng * nchunk * 3);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(arg_relation_kernel, dim3(b * ng, (tn + AG_WAVES - 1) / AG_WAVES), dim3(AG_THREADS), 0, st, theta, phi, ld, boxes, centre_rounds, thr, tn, ng, nfr,
                       rel, mask);
    DIN_CHECK_LAUNCH("arg_relation");
    const size_t lds = (size_t)(tn * tn + tn * AG_COLS) * sizeof(float);
    din_raise_lds(reinterpret_cast<const void*>(arg_aggregate_kernel), lds);
    hipLaunchKernelGGL(arg_aggregate_kernel, dim3(nchunk, b * ng), dim3(AG_THREADS), lds, st, y, ld, rel, tn, ng, nfg, nchunk, z, ws);
    DIN_CHECK_LAUNCH("arg_aggregate");
    hipLaunchKernelGGL(arg_stats_kernel, dim3((b * ng + AG_THREADS - 1) / AG_THREADS), dim3(AG_THREADS), 0, st, ws, b * ng, nchunk, eps, stats);
    DIN_CHECK_LAUNCH("arg_stats");
    hipLaunchKernelGGL(arg_norm_sum_kernel, dim3((nfg + AG_THREADS - 1) / AG_THREADS, tn, b), dim3(AG_THREADS), 0, st, z, stats, gamma, beta, tn,
                       ng, nfg, out);
    DIN_CHECK_LAUNCH("arg_norm_sum");
    return DIN_OK;
}

int din_arg_graph_bwd(const float* g_out, const float* theta, const float* phi, const float* y, int64_t ld, const float* gamma,
                      const float* beta, const float* rel, const float* z, const float* stats, int b, int tn, int ng, int nfr, int nfg,
                      float* d_theta, float* d_phi, float* d_y, int64_t ld_grad, float* d_gamma, float* d_beta, float* ws, int64_t ws_floats,
                      void* stream) {
    DIN_REQUIRE(g_out && theta && phi && y && gamma && beta && rel && z && stats && d_theta && d_phi && d_y && d_gamma && d_beta && ws,
                "arg_graph_bwd: null pointer");
    int rc = check_shape("arg_graph_bwd", ld, b, tn, ng, nfr, nfg);
    if (rc != DIN_OK) return rc;
    rc = check_shape("arg_graph_bwd (gradient)", ld_grad, b, tn, ng, nfr, nfg);
    if (rc != DIN_OK) return rc;
    DIN_REQUIRE(aligned16(y) && aligned16(ws), "arg_graph_bwd: y / workspace must be 16-byte aligned");
    const int nchunk = (nfg + AG_COLS - 1) / AG_COLS;
    const int64_t n_part = ((int64_t)b * ng * nchunk * 2 + 3) / 4 * 4, n_dz = (int64_t)b * ng * tn * nfg, n_ds = (int64_t)b * ng * tn * tn;
    DIN_REQUIRE(ws_floats >= n_part + n_dz + n_ds, "arg_graph_bwd: workspace of %lld floats, %lld needed", (long long)ws_floats,
                (long long)(n_part + n_dz + n_ds));
    float* dz = ws;                                           // (first: keeps the 16-byte alignment of its rows)
    float* part2 = dz + n_dz;
    float* ds = part2 + n_part;
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(arg_bwd_ln_sums_kernel, dim3(nchunk, b * ng), dim3(AG_THREADS), 0, st, z, g_out, gamma, beta, stats, tn, ng, nfg, nchunk,
                       part2);
    DIN_CHECK_LAUNCH("arg_bwd_ln_sums");
    const int64_t n_aff = (int64_t)ng * tn * nfg;
    hipLaunchKernelGGL(arg_bwd_affine_kernel, dim3((unsigned)((n_aff + AG_THREADS - 1) / AG_THREADS)), dim3(AG_THREADS), 0, st, z, g_out, gamma,
                       beta, stats, b, tn, ng, nfg, d_gamma, d_beta);
    DIN_CHECK_LAUNCH("arg_bwd_affine");
    const size_t lds = (size_t)(tn * tn + tn * AG_COLS) * sizeof(float);
    din_raise_lds(reinterpret_cast<const void*>(arg_bwd_dz_kernel), lds);
    hipLaunchKernelGGL(arg_bwd_dz_kernel, dim3(nchunk, b * ng), dim3(AG_THREADS), lds, st, z, g_out, gamma, beta, stats, part2, rel, tn, ng, nfg,
                       nchunk, dz, d_y, ld_grad);
    DIN_CHECK_LAUNCH("arg_bwd_dz");
    hipLaunchKernelGGL(arg_bwd_relation_kernel, dim3(b * ng, (tn + AG_WAVES - 1) / AG_WAVES), dim3(AG_THREADS), 0, st, dz, y, ld, rel, tn, ng, nfr, nfg, ds);
    DIN_CHECK_LAUNCH("arg_bwd_relation");
    const size_t lds_p = (size_t)(tn * tn + 2 * tn * AG_COLS) * sizeof(float);
    din_raise_lds(reinterpret_cast<const void*>(arg_bwd_proj_kernel), lds_p);
    hipLaunchKernelGGL(arg_bwd_proj_kernel, dim3((nfr + AG_COLS - 1) / AG_COLS, b * ng), dim3(AG_THREADS), lds_p, st, ds, theta, phi, ld, tn, ng,
                       nfr, d_theta, d_phi, ld_grad);
    DIN_CHECK_LAUNCH("arg_bwd_proj");
    return DIN_OK;
}

}  // extern "C"
