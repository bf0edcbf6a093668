// Stage-1 base-model head (reference base_model.py:117-139 Basenet_volleyball, :243-268 Basenet_collective), fused:
//   s        = dropout(relu(y))                       y = fc_emb output fp32 [bt, n, c]; never materialised
//   actions  = s @ W_act^T + b_act                    one row per valid box
//   frame    = max_over_boxes(s) @ W_grp^T + b_grp    one row per frame; arg-max box per channel saved (first maximum wins)
//   mean_over_t (volleyball, T != 1): both averaged over the T frames of a clip (:135-137)
//   n_per_frame (collective): frame k holds n_per_frame[k] valid boxes; action rows compacted in (frame, box) order (:247-264)
//
// Forward: ONE launch.  One 256-thread workgroup per output group (a clip under mean_over_t, else a frame); it walks its frames and
// boxes in order, reads every y element once, applies ReLU and the counter-hash keep mask of din_act_dropout_fwd (same seed, same flat
// element index: bitwise the same s), reduces the <= 16 action dots of each box across the workgroup (wave_sum + one LDS slab per row,
// double-buffered so one barrier per row suffices) and keeps the running channel maximum / arg-max in LDS slots each thread owns.
// Compacted row offsets are prefix sums of n_per_frame, formed by each workgroup on the device.
//
// Backward: ONE launch, deterministic, no atomics.  A grid over 64-channel blocks: each lane owns one channel, its four waves take every
// fourth frame and walk that frame's boxes in order, so a lane's dW partials are fixed-order sums; the four waves' partials are then
// added in wave order through LDS.  g_y is written for every element (zero for padding boxes).  Workgroup 0 also forms the bias
// gradients, one thread per class, walking the rows in order.  Tiny and latency-bound (~100 rows x 1024 channels per stage-1 step).
#include "din_common.h"

namespace {

constexpr int BH_THREADS = 256;
constexpr int BH_WAVES = BH_THREADS / 64;
constexpr int BH_MAX_ACT = 16;
constexpr int BH_MAX_C = 4096;       // forward LDS: c floats (max) + c ints (arg-max) + n * a_act floats (T-mean sums) <= 64 KiB
constexpr int BH_MAX_N = 256;

__device__ __forceinline__ int frame_count(const int32_t* npf, int k, int n) {
    int v = npf ? npf[k] : n;
    return v < 0 ? 0 : (v > n ? n : v);
}

__global__ __launch_bounds__(BH_THREADS) void basenet_head_fwd_kernel(
        const float* __restrict__ y, const float* __restrict__ wa, const float* __restrict__ ba, const float* __restrict__ wg,
        const float* __restrict__ bg, const int32_t* __restrict__ npf, int all_n, int tg, int mean, int n, int c, int aa, int ag,
        float p, uint64_t seed, const uint64_t* __restrict__ seed_off, float* __restrict__ actions, float* __restrict__ activities,
        int32_t* __restrict__ argmax) {
    extern __shared__ float bh_lds[];
    float* mx = bh_lds;                                       // [c] running maximum of s over the frame's boxes
    int32_t* am = reinterpret_cast<int32_t*>(bh_lds + c);     // [c] its box
    float* asum = bh_lds + 2 * c;                             // [n][aa] per-box action sums over the clip's frames (mean only)
    __shared__ float red[2][BH_WAVES][BH_MAX_ACT];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int grp = blockIdx.x;
    seed = fold_seed(seed, seed_off);
    if (mean)
        for (int e = tid; e < n * aa; e += BH_THREADS) asum[e] = 0.f;   // (first read after the barrier of the first row)
    float gsum = 0.f;                                         // thread j < ag: activity sum over the clip's frames
    int par = 0;
    for (int tf = 0; tf < tg; ++tf) {
        const int bt = grp * tg + tf;
        const int nv = frame_count(npf, bt, n);
        int off = bt * n;                                     // first action row of this frame
        if (npf) {
            off = 0;
            for (int k = 0; k < bt; ++k) off += frame_count(npf, k, n);
        }
        for (int ch = tid; ch < c; ch += BH_THREADS) { mx[ch] = -INFINITY; am[ch] = 0; }
        for (int i = 0; i < nv; ++i) {
            const int64_t base = ((int64_t)bt * n + i) * c;
            float acc[BH_MAX_ACT];
#pragma unroll
            for (int j = 0; j < BH_MAX_ACT; ++j) acc[j] = 0.f;
            for (int ch = tid; ch < c; ch += BH_THREADS) {
                const float s = fmaxf(y[base + ch], 0.f) * keep_scale(seed, base + ch, p);   // == din_act_dropout_fwd(relu=1)
                if (s > mx[ch]) { mx[ch] = s; am[ch] = i; }    // first maximum wins (head.hip, torch.max on CPU)
#pragma unroll
                for (int j = 0; j < BH_MAX_ACT; ++j) if (j < aa) acc[j] += s * wa[(int64_t)j * c + ch];
            }
#pragma unroll
            for (int j = 0; j < BH_MAX_ACT; ++j) {
                if (j < aa) {
                    const float v = wave_sum(acc[j]);
                    if (lane == 0) red[par][wv][j] = v;
                }
            }
            __syncthreads();
            if (tid < aa) {
                float v = 0.f;
                for (int w = 0; w < BH_WAVES; ++w) v += red[par][w][tid];
                v += ba[tid];
                if (mean) {
                    asum[i * aa + tid] += v;
                } else {
                    const int row = off + i;
                    if (row < all_n) actions[(int64_t)row * aa + tid] = v;
                }
            }
            par ^= 1;                                         // the next row writes the other slab; this one is rewritten after a barrier
        }
        // activity of the frame: max over its boxes, fc_activities
        float acc[BH_MAX_ACT];
#pragma unroll
        for (int j = 0; j < BH_MAX_ACT; ++j) acc[j] = 0.f;
        for (int ch = tid; ch < c; ch += BH_THREADS) {
            const float m = nv > 0 ? mx[ch] : 0.f;
            argmax[(int64_t)bt * c + ch] = am[ch];
#pragma unroll
            for (int j = 0; j < BH_MAX_ACT; ++j) if (j < ag) acc[j] += m * wg[(int64_t)j * c + ch];
        }
#pragma unroll
        for (int j = 0; j < BH_MAX_ACT; ++j) {
            if (j < ag) {
                const float v = wave_sum(acc[j]);
                if (lane == 0) red[par][wv][j] = v;
            }
        }
        __syncthreads();
        if (tid < ag) {
            float v = 0.f;
            for (int w = 0; w < BH_WAVES; ++w) v += red[par][w][tid];
            v += bg[tid];
            if (mean) gsum += v;
            else activities[(int64_t)bt * ag + tid] = v;
        }
        par ^= 1;
    }
    if (mean) {
        const float inv = (float)tg;
        if (tid < ag) activities[(int64_t)grp * ag + tid] = gsum / inv;
        if (tid < aa)
            for (int i = 0; i < n; ++i) {
                const int row = grp * n + i;
                if (row < all_n) actions[(int64_t)row * aa + tid] = asum[i * aa + tid] / inv;
            }
    }
}

__global__ __launch_bounds__(BH_THREADS) void basenet_head_bwd_kernel(
        const float* __restrict__ ga, const float* __restrict__ gg, const float* __restrict__ y, const float* __restrict__ wa,
        const float* __restrict__ wg, const int32_t* __restrict__ argmax, const int32_t* __restrict__ npf, int all_n, int bt_total,
        int t, int mean, int n, int c, int aa, int ag, float p, uint64_t seed, const uint64_t* __restrict__ seed_off,
        float* __restrict__ gy, float* __restrict__ dwa, float* __restrict__ dba, float* __restrict__ dwg, float* __restrict__ dbg) {
    __shared__ float part[BH_WAVES][2 * BH_MAX_ACT][64];      // per-wave dW partials, added in wave order
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int ch = blockIdx.x * 64 + lane;
    const bool live = ch < c;
    seed = fold_seed(seed, seed_off);
    const float sc = mean ? 1.f / (float)t : 1.f;             // the T-mean folded into the incoming gradients
    float wa_r[BH_MAX_ACT], wg_r[BH_MAX_ACT], da[BH_MAX_ACT], dg[BH_MAX_ACT];
#pragma unroll
    for (int j = 0; j < BH_MAX_ACT; ++j) {
        wa_r[j] = (live && j < aa) ? wa[(int64_t)j * c + ch] : 0.f;
        wg_r[j] = (live && j < ag) ? wg[(int64_t)j * c + ch] : 0.f;
        da[j] = 0.f;
        dg[j] = 0.f;
    }
    int off = 0;                                              // compacted row offset of frame bt (n_per_frame)
    for (int bt = 0; bt < bt_total; ++bt) {
        const int nv = frame_count(npf, bt, n);
        if (bt % BH_WAVES == wv && live) {
            const int grow = mean ? bt / t : bt;
            float ggj[BH_MAX_ACT];
            float gpool = 0.f;
#pragma unroll
            for (int j = 0; j < BH_MAX_ACT; ++j) {
                ggj[j] = j < ag ? gg[(int64_t)grow * ag + j] * sc : 0.f;
                gpool += ggj[j] * wg_r[j];
            }
            const int amx = argmax[(int64_t)bt * c + ch];
            for (int i = 0; i < n; ++i) {
                const int64_t e = ((int64_t)bt * n + i) * c + ch;
                if (i >= nv) { gy[e] = 0.f; continue; }
                const int row = mean ? (bt / t) * n + i : (npf ? off + i : bt * n + i);
                const float v = y[e];
                const float k = keep_scale(seed, e, p);
                const float s = fmaxf(v, 0.f) * k;
                float gs = 0.f;
#pragma unroll
                for (int j = 0; j < BH_MAX_ACT; ++j) {
                    const float gaj = (j < aa && row < all_n) ? ga[(int64_t)row * aa + j] * sc : 0.f;
                    da[j] += gaj * s;
                    gs += gaj * wa_r[j];
                }
                if (i == amx) {
                    gs += gpool;
#pragma unroll
                    for (int j = 0; j < BH_MAX_ACT; ++j) dg[j] += ggj[j] * s;
                }
                float g = gs * k;                             // == din_act_dropout_bwd(relu=1)
                if (!(v > 0.f)) g = 0.f;
                gy[e] = g;
            }
        }
        off += nv;
    }
#pragma unroll
    for (int j = 0; j < BH_MAX_ACT; ++j) {
        part[wv][j][lane] = da[j];
        part[wv][BH_MAX_ACT + j][lane] = dg[j];
    }
    __syncthreads();
    for (int q = threadIdx.x; q < 2 * BH_MAX_ACT * 64; q += BH_THREADS) {
        const int j2 = q >> 6, l = q & 63, cc = blockIdx.x * 64 + l;
        const int j = j2 % BH_MAX_ACT;
        const bool act = j2 < BH_MAX_ACT;
        if (cc >= c || j >= (act ? aa : ag)) continue;
        float v = 0.f;
        for (int w = 0; w < BH_WAVES; ++w) v += part[w][j2][l];
        (act ? dwa : dwg)[(int64_t)j * c + cc] = v;
    }
    if (blockIdx.x == 0) {                                    // bias gradients: one thread per class, rows in order
        const int tid = threadIdx.x;
        if (tid < aa) {
            float v = 0.f;
            int o = 0;
            for (int bt = 0; bt < bt_total; ++bt) {
                const int nv = frame_count(npf, bt, n);
                for (int i = 0; i < nv; ++i) {
                    const int row = mean ? (bt / t) * n + i : (npf ? o + i : bt * n + i);
                    if (row < all_n) v += ga[(int64_t)row * aa + tid] * sc;
                }
                o += nv;
            }
            dba[tid] = v;
        } else if (tid >= 64 && tid - 64 < ag) {
            const int j = tid - 64;
            float v = 0.f;
            for (int bt = 0; bt < bt_total; ++bt) v += gg[(int64_t)(mean ? bt / t : bt) * ag + j] * sc;
            dbg[j] = v;
        }
    }
}

int check_shape(const char* what, const int32_t* npf, int all_n, int bt, int t, int mean, int n, int c, int aa, int ag, float p) {
    DIN_REQUIRE(bt > 0 && t > 0 && n > 0 && n <= BH_MAX_N && c > 0 && c <= BH_MAX_C, "%s: bad shape (bt %d, t %d, n %d <= %d, c %d <= %d)",
                what, bt, t, n, BH_MAX_N, c, BH_MAX_C);
    DIN_REQUIRE(aa >= 1 && aa <= BH_MAX_ACT && ag >= 1 && ag <= BH_MAX_ACT, "%s: A_act %d / A_grp %d outside 1..%d", what, aa, ag, BH_MAX_ACT);
    DIN_REQUIRE(p >= 0.f && p < 1.f, "%s: drop_p %g outside [0, 1)", what, (double)p);
    if (mean) {
        DIN_REQUIRE(!npf, "%s: mean_over_t with n_per_frame (the collective head has no T-mean)", what);
        DIN_REQUIRE(bt % t == 0, "%s: bt %d is not a multiple of t %d", what, bt, t);
        DIN_REQUIRE(all_n == (bt / t) * n, "%s: all_n %d != clips * n", what, all_n);
    } else if (npf) {
        DIN_REQUIRE(all_n >= 1 && all_n <= bt * n, "%s: n_per_frame[bt] outside 1..N (all_n %d)", what, all_n);
    } else {
        DIN_REQUIRE(all_n == bt * n, "%s: all_n %d != bt * n", what, all_n);
    }
    return DIN_OK;
}

}  // namespace

extern "C" {

int din_basenet_head_fwd(const float* y, const float* w_act, const float* b_act, const float* w_grp, const float* b_grp,
                         const int32_t* n_per_frame, int all_n, int bt, int t, int mean_over_t, int n, int c, int a_act, int a_grp,
                         float drop_p, uint64_t seed, const uint64_t* seed_offset, float* actions, float* activities, int32_t* argmax,
                         void* stream) {
    DIN_REQUIRE(y && w_act && b_act && w_grp && b_grp && actions && activities && argmax, "basenet_head_fwd: null pointer");
    int rc = check_shape("basenet_head_fwd", n_per_frame, all_n, bt, t, mean_over_t, n, c, a_act, a_grp, drop_p);
    if (rc != DIN_OK) return rc;
    const int tg = mean_over_t ? t : 1;
    const size_t lds = (size_t)2 * c * sizeof(float) + (mean_over_t ? (size_t)n * a_act * sizeof(float) : 0);
    hipLaunchKernelGGL(basenet_head_fwd_kernel, dim3(bt / tg), dim3(BH_THREADS), lds, as_stream(stream), y, w_act, b_act, w_grp, b_grp,
                       n_per_frame, all_n, tg, mean_over_t, n, c, a_act, a_grp, drop_p, seed, seed_offset, actions, activities, argmax);
    DIN_CHECK_LAUNCH("basenet_head_fwd");
    return DIN_OK;
}

int din_basenet_head_bwd(const float* g_actions, const float* g_activities, const float* y, const float* w_act, const float* w_grp,
                         const int32_t* argmax, const int32_t* n_per_frame, int all_n, int bt, int t, int mean_over_t, int n, int c,
                         int a_act, int a_grp, float drop_p, uint64_t seed, const uint64_t* seed_offset, float* g_y, float* dw_act,
                         float* db_act, float* dw_grp, float* db_grp, void* stream) {
    DIN_REQUIRE(g_actions && g_activities && y && w_act && w_grp && argmax && g_y && dw_act && db_act && dw_grp && db_grp,
                "basenet_head_bwd: null pointer");
    int rc = check_shape("basenet_head_bwd", n_per_frame, all_n, bt, t, mean_over_t, n, c, a_act, a_grp, drop_p);
    if (rc != DIN_OK) return rc;
    hipLaunchKernelGGL(basenet_head_bwd_kernel, dim3((c + 63) / 64), dim3(BH_THREADS), 0, as_stream(stream), g_actions, g_activities, y,
                       w_act, w_grp, argmax, n_per_frame, all_n, bt, t, mean_over_t, n, c, a_act, a_grp, drop_p, seed, seed_offset, g_y,
                       dw_act, db_act, dw_grp, db_grp);
    DIN_CHECK_LAUNCH("basenet_head_bwd");
    return DIN_OK;
}

}  // extern "C"
