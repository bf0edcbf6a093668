// PCTDM between its two LSTMs (reference infer_module/pctdm_infer_module.py:94-96 early pooling, :106 context, :52-59 and :112-114
// intra-group attention), around the att_source / att_context projections:
//   pool       pooled [g][n][h] = max(lstm_out[g][n][0 .. h), lstm_out[g][n][h .. 2h)): the reference views the Bi-LSTM output [g][n][2h] as
//              [g][1][2n][h] and max-pools pairs of rows, which are the two DIRECTION halves of one player, not two players;
//              context [g][h] = mean of pooled over the n players
//   attention  score[g][i] = <w_e, tanh(src[g][i] + ctx[g])> + b_e;  gamma = softmax of the scores inside each of the two teams of n / 2
//              players;  y = pooled + pooled * gamma
// One workgroup of 256 threads per frame g.  Dot products over h go one player per wave (lanes over the row, butterfly sum), everything per
// column one column per thread.  The reduction of d w_e / d b_e over the frames is two-stage: per-frame partials, then one launch that adds
// them in frame order.  Accurate tanhf / expf, fixed-order sums, no atomics, same bits on a rerun.  fp32 throughout.
#include "din_common.h"

namespace {

constexpr int PC_THREADS = 256;
constexpr int PC_WAVES = PC_THREADS / 64;
constexpr int PC_MAX_N = 32;

__global__ __launch_bounds__(PC_THREADS) void pctdm_pool_fwd_kernel(const float* __restrict__ lstm_out, int n, int h, float* __restrict__ pooled,
                                                                    uint8_t* __restrict__ winner, float* __restrict__ context) {
    const int64_t g = blockIdx.x;
    for (int k = threadIdx.x; k < h; k += PC_THREADS) {
        float acc = 0.f;
        for (int i = 0; i < n; ++i) {                                  // players in order
            const int64_t row = g * n + i;
            const float a = lstm_out[row * 2 * h + k], b = lstm_out[row * 2 * h + h + k];
            const bool second = b > a;                                 // the first of two equal values wins, as in the max-pool
            const float m = second ? b : a;
            pooled[row * h + k] = m;
            winner[row * h + k] = second ? 1 : 0;
            acc += m;
        }
        context[g * h + k] = acc / (float)n;
    }
}

__global__ __launch_bounds__(PC_THREADS) void pctdm_pool_bwd_kernel(const float* __restrict__ g_pooled, const float* __restrict__ g_context,
                                                                    const uint8_t* __restrict__ winner, int n, int h,
                                                                    float* __restrict__ d_lstm_out) {
    const int64_t g = blockIdx.x;
    for (int k = threadIdx.x; k < h; k += PC_THREADS) {
        const float gc = g_context[g * h + k] / (float)n;
        for (int i = 0; i < n; ++i) {
            const int64_t row = g * n + i;
            const float v = g_pooled[row * h + k] + gc;
            const bool second = winner[row * h + k] != 0;
            d_lstm_out[row * 2 * h + k] = second ? 0.f : v;
            d_lstm_out[row * 2 * h + h + k] = second ? v : 0.f;
        }
    }
}

// softmax of s[0 .. m) in place, the maximum subtracted
__device__ __forceinline__ void softmax_group(float* s, int m) {
    float mx = s[0];
    for (int j = 1; j < m; ++j) mx = fmaxf(mx, s[j]);
    float den = 0.f;
    for (int j = 0; j < m; ++j) {
        s[j] = expf(s[j] - mx);
        den += s[j];
    }
    for (int j = 0; j < m; ++j) s[j] = s[j] / den;
}

__global__ __launch_bounds__(PC_THREADS) void pctdm_att_fwd_kernel(const float* __restrict__ pooled, const float* __restrict__ src,
                                                                   const float* __restrict__ ctx, const float* __restrict__ w_e,
                                                                   const float* __restrict__ b_e, int n, int h, float* __restrict__ y,
                                                                   float* __restrict__ gamma) {
    __shared__ float sc[PC_MAX_N];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t g = blockIdx.x;
    for (int i = wv; i < n; i += PC_WAVES) {
        const float* s = src + (g * n + i) * h;
        float acc = 0.f;
        for (int k = lane; k < h; k += 64) acc = fmaf(w_e[k], tanhf(s[k] + ctx[g * h + k]), acc);
        acc = wave_sum(acc);
        if (lane == 0) sc[i] = acc + b_e[0];
    }
    __syncthreads();
    if (tid < 2) softmax_group(sc + tid * (n / 2), n / 2);
    __syncthreads();
    if (tid < n) gamma[g * n + tid] = sc[tid];
    for (int k = tid; k < h; k += PC_THREADS)
        for (int i = 0; i < n; ++i) {
            const int64_t e = (g * n + i) * h + k;
            const float p = pooled[e];
            y[e] = p + p * sc[i];
        }
}

// d_pooled, d_src [g][n][h], d_ctx [g][h]; part [g][h] = this frame's share of d w_e, partb [g] = its share of d b_e
__global__ __launch_bounds__(PC_THREADS) void pctdm_att_bwd_kernel(const float* __restrict__ g_y, const float* __restrict__ pooled,
                                                                   const float* __restrict__ src, const float* __restrict__ ctx,
                                                                   const float* __restrict__ w_e, const float* __restrict__ gamma, int n, int h,
                                                                   float* __restrict__ d_pooled, float* __restrict__ d_src,
                                                                   float* __restrict__ d_ctx, float* __restrict__ part,
                                                                   float* __restrict__ partb) {
    __shared__ float ga[PC_MAX_N], ds[PC_MAX_N];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t g = blockIdx.x;
    if (tid < n) ga[tid] = gamma[g * n + tid];
    for (int i = wv; i < n; i += PC_WAVES) {                           // d gamma[i] = <g_y[i], pooled[i]>
        const float* a = g_y + (g * n + i) * h;
        const float* b = pooled + (g * n + i) * h;
        float acc = 0.f;
        for (int k = lane; k < h; k += 64) acc = fmaf(a[k], b[k], acc);
        acc = wave_sum(acc);
        if (lane == 0) ds[i] = acc;
    }
    __syncthreads();
    if (tid < 2) {                                                     // softmax backward inside the team
        const int m = n / 2;
        float* d = ds + tid * m;
        const float* p = ga + tid * m;
        float t = 0.f;
        for (int j = 0; j < m; ++j) t += d[j] * p[j];
        for (int j = 0; j < m; ++j) d[j] = p[j] * (d[j] - t);
    }
    __syncthreads();
    if (tid == 0) {
        float t = 0.f;
        for (int i = 0; i < n; ++i) t += ds[i];
        partb[g] = t;
    }
    for (int k = tid; k < h; k += PC_THREADS) {
        const float c = ctx[g * h + k], we = w_e[k];
        float dc = 0.f, dw = 0.f;
        for (int i = 0; i < n; ++i) {
            const int64_t e = (g * n + i) * h + k;
            const float t = tanhf(src[e] + c);
            const float v = ds[i] * we * (1.f - t * t);
            d_src[e] = v;
            dc += v;
            dw += ds[i] * t;
            d_pooled[e] = g_y[e] + g_y[e] * ga[i];
        }
        d_ctx[g * h + k] = dc;
        part[g * h + k] = dw;
    }
}

// d w_e [h] and d b_e [1]: frames added in order
__global__ __launch_bounds__(PC_THREADS) void pctdm_att_reduce_kernel(const float* __restrict__ part, const float* __restrict__ partb, int g,
                                                                      int h, float* __restrict__ d_w_e, float* __restrict__ d_b_e) {
    const int k = blockIdx.x * PC_THREADS + threadIdx.x;
    if (k < h) {
        float acc = 0.f;
        for (int i = 0; i < g; ++i) acc += part[(int64_t)i * h + k];
        d_w_e[k] = acc;
    }
    if (k == 0) {
        float acc = 0.f;
        for (int i = 0; i < g; ++i) acc += partb[i];
        d_b_e[0] = acc;
    }
}

inline bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

int check_pctdm_shape(const char* what, int g, int n, int h, bool teams) {
    DIN_REQUIRE(g >= 1 && g <= 0x7FFFFF && n >= 1 && n <= PC_MAX_N && h >= 1, "%s: bad shape (g %d, n %d outside 1..%d, h %d)", what, g, n,
                PC_MAX_N, h);
    DIN_REQUIRE(!teams || n % 2 == 0, "%s: n %d must be even (two teams of n / 2 players)", what, n);
    return DIN_OK;
}

}  // namespace

extern "C" {

int din_pctdm_pool_fwd(const float* lstm_out, int g, int n, int h, float* pooled, uint8_t* winner, float* context, void* stream) {
    DIN_REQUIRE(lstm_out && pooled && winner && context, "pctdm_pool_fwd: null pointer");
    int rc = check_pctdm_shape("pctdm_pool_fwd", g, n, h, false);
    if (rc != DIN_OK) return rc;
    DIN_REQUIRE(aligned4(lstm_out) && aligned4(pooled) && aligned4(context), "pctdm_pool_fwd: misaligned pointer");
    hipLaunchKernelGGL(pctdm_pool_fwd_kernel, dim3(g), dim3(PC_THREADS), 0, as_stream(stream), lstm_out, n, h, pooled, winner, context);
    DIN_CHECK_LAUNCH("pctdm_pool_fwd");
    return DIN_OK;
}

int din_pctdm_pool_bwd(const float* g_pooled, const float* g_context, const uint8_t* winner, int g, int n, int h, float* d_lstm_out,
                       void* stream) {
    DIN_REQUIRE(g_pooled && g_context && winner && d_lstm_out, "pctdm_pool_bwd: null pointer");
    int rc = check_pctdm_shape("pctdm_pool_bwd", g, n, h, false);
    if (rc != DIN_OK) return rc;
    DIN_REQUIRE(aligned4(g_pooled) && aligned4(g_context) && aligned4(d_lstm_out), "pctdm_pool_bwd: misaligned pointer");
    hipLaunchKernelGGL(pctdm_pool_bwd_kernel, dim3(g), dim3(PC_THREADS), 0, as_stream(stream), g_pooled, g_context, winner, n, h, d_lstm_out);
    DIN_CHECK_LAUNCH("pctdm_pool_bwd");
    return DIN_OK;
}

int din_pctdm_att_fwd(const float* pooled, const float* src, const float* ctx, const float* w_e, const float* b_e, int g, int n, int h,
                      float* y, float* gamma, void* stream) {
    DIN_REQUIRE(pooled && src && ctx && w_e && b_e && y && gamma, "pctdm_att_fwd: null pointer");
    int rc = check_pctdm_shape("pctdm_att_fwd", g, n, h, true);
    if (rc != DIN_OK) return rc;
    DIN_REQUIRE(aligned4(pooled) && aligned4(src) && aligned4(ctx) && aligned4(w_e) && aligned4(b_e) && aligned4(y) && aligned4(gamma),
                "pctdm_att_fwd: misaligned pointer");
    hipLaunchKernelGGL(pctdm_att_fwd_kernel, dim3(g), dim3(PC_THREADS), 0, as_stream(stream), pooled, src, ctx, w_e, b_e, n, h, y, gamma);
    DIN_CHECK_LAUNCH("pctdm_att_fwd");
    return DIN_OK;
}

int64_t din_pctdm_att_bwd_workspace(int g, int h) {
    if (g < 1 || h < 1) return 0;
    return (int64_t)g * h + g;
}

int din_pctdm_att_bwd(const float* g_y, const float* pooled, const float* src, const float* ctx, const float* w_e, const float* gamma, int g,
                      int n, int h, float* d_pooled, float* d_src, float* d_ctx, float* d_w_e, float* d_b_e, float* ws, int64_t ws_floats,
                      void* stream) {
    DIN_REQUIRE(g_y && pooled && src && ctx && w_e && gamma && d_pooled && d_src && d_ctx && d_w_e && d_b_e && ws,
                "pctdm_att_bwd: null pointer");
    int rc = check_pctdm_shape("pctdm_att_bwd", g, n, h, true);
    if (rc != DIN_OK) return rc;
    DIN_REQUIRE(aligned4(g_y) && aligned4(pooled) && aligned4(src) && aligned4(ctx) && aligned4(w_e) && aligned4(gamma) && aligned4(d_pooled) &&
                aligned4(d_src) && aligned4(d_ctx) && aligned4(d_w_e) && aligned4(d_b_e) && aligned4(ws), "pctdm_att_bwd: misaligned pointer");
    const int64_t need = din_pctdm_att_bwd_workspace(g, h);
    DIN_REQUIRE(ws_floats >= need, "pctdm_att_bwd: workspace of %lld floats, %lld needed", (long long)ws_floats, (long long)need);
    hipStream_t st = as_stream(stream);
    float* part = ws;
    float* partb = ws + (int64_t)g * h;
    hipLaunchKernelGGL(pctdm_att_bwd_kernel, dim3(g), dim3(PC_THREADS), 0, st, g_y, pooled, src, ctx, w_e, gamma, n, h, d_pooled, d_src, d_ctx,
                       part, partb);
    DIN_CHECK_LAUNCH("pctdm_att_bwd");
    hipLaunchKernelGGL(pctdm_att_reduce_kernel, dim3((h + PC_THREADS - 1) / PC_THREADS), dim3(PC_THREADS), 0, st, part, partb, g, h, d_w_e,
                       d_b_e);
    DIN_CHECK_LAUNCH("pctdm_att_reduce");
    return DIN_OK;
}

}  // extern "C"
