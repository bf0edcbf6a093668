// One-layer LSTM, forward and backward, for the PCTDM baseline (reference infer_module/pctdm_infer_module.py:23-24 Bi_Lstm, :47
// Intra_Group_LSTM, run at :83 and :114): everything after the input projection.  pre [R][S][D][4H] = x W_ih^T + b_ih + b_hh of ALL steps is
// one contraction on the MFMA kernel (ops.linear); what is left is the recurrence, S dependent steps of
//     z = pre[:, pos] + h W_hh^T;  i, f, o = sigmoid(z_i, z_f, z_o);  g = tanh(z_g);  c = f c + i g;  h = o tanh(c)
// with R rows (frames, or the two teams of every frame), H hidden units and D directions (direction 1 walks the positions S-1 .. 0).
//
// One plain launch per step, issued here on the caller's stream: every hidden unit of step s needs every hidden unit of step s - 1, and the
// launch boundary is that all-to-all dependency.  No grid-wide barrier, no cooperative launch, no workgroup ever waits for another one.
//
// Grid = (slices of LSTM_HS hidden units) x D.  A workgroup owns its 4 * LSTM_HS rows of W_hh (backward: its LSTM_HS rows of W_hh^T, each 4H
// long) and reads them with 16-byte loads, one row per wave at a time; the previous h (backward: the next step's d_pre) of a chunk of the R
// rows sits in LDS and every weight element loaded is used for all rows of the chunk.  More rows than a chunk are further chunks (the
// weight slice is read again, from cache).  At H = 1000 that is 125 x D workgroups of 32 weight rows each.
// The backward contracts over the 4H gate rows, i.e. along the COLUMNS of W_hh: din_lstm_bwd first writes W_hh^T into its workspace (one
// launch, 16 MB per direction at H = 1000), so that its step kernel streams contiguous rows exactly as the forward does.
//
// Accurate expf / tanhf, true division, fmaf chains in a fixed order, one butterfly per dot product: no atomics, same bits on a rerun.
// H need not be a multiple of the slice or of 4 (then the rows are read with 4-byte loads).  fp32 throughout.
#include "din_common.h"

namespace {

constexpr int LSTM_THREADS = 256;
constexpr int LSTM_WAVES = LSTM_THREADS / 64;
constexpr int LSTM_HS = 8;             // hidden units per workgroup
constexpr int LSTM_RC_F = 16;          // rows per LDS chunk, forward (16 x H floats)
constexpr int LSTM_RC_B = 8;           // rows per LDS chunk, backward (8 x 4H floats)
constexpr int LSTM_MAX_H = 1024;       // forward 64 KiB, backward 128 KiB of the 160 KiB LDS

__device__ __forceinline__ float sigmoid_acc(float x) { return 1.f / (1.f + expf(-x)); }

// acc[r] = <wrow[0 .. len), vec[r][0 .. len)> for the n rows of the chunk in LDS (row stride len), over the wave; every lane gets the sums
template <int RC, bool VEC>
__device__ __forceinline__ void wave_rows_dot(const float* __restrict__ wrow, const float* vec, int len, int n, int lane, float (&acc)[RC]) {
#pragma unroll
    for (int r = 0; r < RC; ++r) acc[r] = 0.f;
    if (VEC) {
        const float4* w4 = reinterpret_cast<const float4*>(wrow);
        const int n4 = len >> 2;
        for (int k = lane; k < n4; k += 64) {
            const float4 w = w4[k];
#pragma unroll
            for (int r = 0; r < RC; ++r) {
                if (r < n) {
                    const float4 v = reinterpret_cast<const float4*>(vec + (size_t)r * len)[k];
                    acc[r] = fmaf(w.w, v.w, fmaf(w.z, v.z, fmaf(w.y, v.y, fmaf(w.x, v.x, acc[r]))));
                }
            }
        }
    } else {
        for (int k = lane; k < len; k += 64) {
            const float w = wrow[k];
#pragma unroll
            for (int r = 0; r < RC; ++r)
                if (r < n) acc[r] = fmaf(w, vec[(size_t)r * len + k], acc[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < RC; ++r)
        if (r < n) acc[r] = wave_sum(acc[r]);
}

// step `step` of the walk: direction 0 is at position step, direction 1 at s - 1 - step
template <bool VEC>
__global__ __launch_bounds__(LSTM_THREADS) void lstm_fwd_step_kernel(const float* __restrict__ pre, const float* __restrict__ w_hh, int rows,
                                                                     int s, int dirs, int h, int step, float* h_out,
                                                                     float* __restrict__ gates, float* cells) {
    extern __shared__ float4 lstm_smem[];
    float* hs = reinterpret_cast<float*>(lstm_smem);                  // [LSTM_RC_F][h]: h of the previous step
    float* z = hs + (size_t)LSTM_RC_F * h;                            // [4 * LSTM_HS][LSTM_RC_F]: the recurrent part of the gates
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int j0 = blockIdx.x * LSTM_HS, d = blockIdx.y;
    const int pos = d == 0 ? step : s - 1 - step, prev = d == 0 ? pos - 1 : pos + 1;
    const float* w = w_hh + (size_t)d * 4 * h * h;
    for (int r0 = 0; r0 < rows; r0 += LSTM_RC_F) {
        const int n = min(LSTM_RC_F, rows - r0);
        if (step > 0) {
            for (int e = tid; e < n * h; e += LSTM_THREADS) {
                const int r = e / h, k = e - r * h;
                hs[e] = h_out[(((size_t)(r0 + r) * s + prev) * dirs + d) * h + k];
            }
            __syncthreads();
            for (int q = wv; q < 4 * LSTM_HS; q += LSTM_WAVES) {
                const int gate = q / LSTM_HS, j = j0 + q % LSTM_HS;
                if (j >= h) continue;
                float acc[LSTM_RC_F];
                wave_rows_dot<LSTM_RC_F, VEC>(w + ((size_t)gate * h + j) * h, hs, h, n, lane, acc);
#pragma unroll
                for (int r = 0; r < LSTM_RC_F; ++r)
                    if (lane == 0 && r < n) z[q * LSTM_RC_F + r] = acc[r];
            }
            __syncthreads();
        }
        if (tid < LSTM_HS * LSTM_RC_F) {
            const int jl = tid % LSTM_HS, r = tid / LSTM_HS, j = j0 + jl;
            if (j < h && r < n) {
                const size_t rp = (((size_t)(r0 + r) * s + pos) * dirs + d);
                const float* pr = pre + rp * 4 * h;
                float zi = pr[j], zf = pr[h + j], zg = pr[2 * h + j], zo = pr[3 * h + j], c_prev = 0.f;
                if (step > 0) {
                    zi += z[(0 * LSTM_HS + jl) * LSTM_RC_F + r];
                    zf += z[(1 * LSTM_HS + jl) * LSTM_RC_F + r];
                    zg += z[(2 * LSTM_HS + jl) * LSTM_RC_F + r];
                    zo += z[(3 * LSTM_HS + jl) * LSTM_RC_F + r];
                    c_prev = cells[(((size_t)(r0 + r) * s + prev) * dirs + d) * h + j];
                }
                const float gi = sigmoid_acc(zi), gf = sigmoid_acc(zf), gg = tanhf(zg), go = sigmoid_acc(zo);
                const float c = gf * c_prev + gi * gg;
                float* ga = gates + rp * 4 * h;
                ga[j] = gi;
                ga[h + j] = gf;
                ga[2 * h + j] = gg;
                ga[3 * h + j] = go;
                cells[rp * h + j] = c;
                h_out[rp * h + j] = go * tanhf(c);
            }
        }
        __syncthreads();                                               // hs / z are rewritten by the next chunk
    }
}

// wt [d][k][m] = w_hh [d][m][k]  (m over the 4H gate rows, k over H)
__global__ __launch_bounds__(LSTM_THREADS) void lstm_transpose_kernel(const float* __restrict__ w_hh, int h, float* __restrict__ wt) {
    __shared__ float tile[32][33];
    const int d = blockIdx.z, m0 = blockIdx.y * 32, k0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;            // 32 x 8
    const float* src = w_hh + (size_t)d * 4 * h * h;
    float* dst = wt + (size_t)d * 4 * h * h;
    for (int i = ty; i < 32; i += 8)
        if (m0 + i < 4 * h && k0 + tx < h) tile[i][tx] = src[(size_t)(m0 + i) * h + k0 + tx];
    __syncthreads();
    for (int i = ty; i < 32; i += 8)
        if (k0 + i < h && m0 + tx < 4 * h) dst[(size_t)(k0 + i) * 4 * h + m0 + tx] = tile[tx][i];
}

// step `step` of the walk, called with step = s - 1 .. 0.  dc [rows][dirs][h]: the cell-state gradient handed to the step before
__global__ __launch_bounds__(LSTM_THREADS) void lstm_bwd_step_kernel(const float* __restrict__ g_out, const float* __restrict__ gates,
                                                                     const float* __restrict__ cells, const float* __restrict__ wt, int rows,
                                                                     int s, int dirs, int h, int step, float* d_pre,
                                                                     float* __restrict__ h_prev, float* __restrict__ dc) {
    extern __shared__ float4 lstm_smem[];
    float* ds = reinterpret_cast<float*>(lstm_smem);                  // [LSTM_RC_B][4h]: d_pre of the step after this one
    float* z = ds + (size_t)LSTM_RC_B * 4 * h;                        // [LSTM_HS][LSTM_RC_B]: its product with W_hh
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int j0 = blockIdx.x * LSTM_HS, d = blockIdx.y;
    const int pos = d == 0 ? step : s - 1 - step, prev = d == 0 ? pos - 1 : pos + 1, next = d == 0 ? pos + 1 : pos - 1;
    const bool last = step == s - 1, first = step == 0;
    const int h4 = 4 * h;
    const float* w = wt + (size_t)d * h4 * h;
    for (int r0 = 0; r0 < rows; r0 += LSTM_RC_B) {
        const int n = min(LSTM_RC_B, rows - r0);
        if (!last) {
            for (int e = tid; e < n * h4; e += LSTM_THREADS) {
                const int r = e / h4, m = e - r * h4;
                ds[e] = d_pre[(((size_t)(r0 + r) * s + next) * dirs + d) * h4 + m];
            }
            __syncthreads();
            for (int q = wv; q < LSTM_HS; q += LSTM_WAVES) {
                if (j0 + q >= h) continue;
                float acc[LSTM_RC_B];
                wave_rows_dot<LSTM_RC_B, true>(w + (size_t)(j0 + q) * h4, ds, h4, n, lane, acc);
#pragma unroll
                for (int r = 0; r < LSTM_RC_B; ++r)
                    if (lane == 0 && r < n) z[q * LSTM_RC_B + r] = acc[r];
            }
            __syncthreads();
        }
        if (tid < LSTM_HS * LSTM_RC_B) {
            const int jl = tid % LSTM_HS, r = tid / LSTM_HS, j = j0 + jl;
            if (j < h && r < n) {
                const size_t rp = (((size_t)(r0 + r) * s + pos) * dirs + d);
                const size_t rq = (((size_t)(r0 + r) * s + prev) * dirs + d);          // (only formed into an address when !first)
                const float* ga = gates + rp * h4;
                const float gi = ga[j], gf = ga[h + j], gg = ga[2 * h + j], go = ga[3 * h + j];
                const float tc = tanhf(cells[rp * h + j]);
                const float c_prev = first ? 0.f : cells[rq * h + j];
                float dh = g_out[rp * h + j];
                if (!last) dh += z[jl * LSTM_RC_B + r];
                float dcv = dh * go * (1.f - tc * tc);
                const size_t ce = ((size_t)(r0 + r) * dirs + d) * h + j;
                if (!last) dcv += dc[ce];
                dc[ce] = dcv * gf;
                float* dp = d_pre + rp * h4;
                dp[j] = dcv * gg * gi * (1.f - gi);
                dp[h + j] = dcv * c_prev * gf * (1.f - gf);
                dp[2 * h + j] = dcv * gi * (1.f - gg * gg);
                dp[3 * h + j] = dh * tc * go * (1.f - go);
                // the h that entered this step, formed as the forward formed it (same two operands, same bits)
                h_prev[rp * h + j] = first ? 0.f : gates[rq * h4 + 3 * h + j] * tanhf(cells[rq * h + j]);
            }
        }
        __syncthreads();
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int check_lstm_shape(const char* what, int rows, int s, int dirs, int h) {
    DIN_REQUIRE(rows >= 1 && s >= 1 && (dirs == 1 || dirs == 2), "%s: bad shape (rows %d, steps %d, directions %d)", what, rows, s, dirs);
    DIN_REQUIRE(h >= 1 && h <= LSTM_MAX_H, "%s: hidden size %d outside 1..%d", what, h, LSTM_MAX_H);
    DIN_REQUIRE((int64_t)rows * s <= 0x7FFFFFFF, "%s: too many rows", what);
    return DIN_OK;
}

size_t fwd_lds(int h) { return sizeof(float) * ((size_t)LSTM_RC_F * h + 4 * LSTM_HS * LSTM_RC_F); }
size_t bwd_lds(int h) { return sizeof(float) * ((size_t)LSTM_RC_B * 4 * h + LSTM_HS * LSTM_RC_B); }

}  // namespace

extern "C" {

int din_lstm_fwd(const float* pre, const float* w_hh, int rows, int steps, int dirs, int hidden, float* h_out, float* gates, float* cells,
                 void* stream) {
    DIN_REQUIRE(pre && w_hh && h_out && gates && cells, "lstm_fwd: null pointer");
    int rc = check_lstm_shape("lstm_fwd", rows, steps, dirs, hidden);
    if (rc != DIN_OK) return rc;
    DIN_REQUIRE(aligned16(pre) && aligned16(w_hh) && aligned16(h_out) && aligned16(gates) && aligned16(cells),
                "lstm_fwd: every pointer must be 16-byte aligned");
    hipStream_t st = as_stream(stream);
    const bool vec = hidden % 4 == 0;
    auto kern = vec ? lstm_fwd_step_kernel<true> : lstm_fwd_step_kernel<false>;
    const size_t lds = fwd_lds(hidden);
    din_raise_lds(reinterpret_cast<const void*>(kern), lds);
    const dim3 grid((hidden + LSTM_HS - 1) / LSTM_HS, dirs);
    for (int step = 0; step < steps; ++step) {
        hipLaunchKernelGGL(kern, grid, dim3(LSTM_THREADS), lds, st, pre, w_hh, rows, steps, dirs, hidden, step, h_out, gates, cells);
        DIN_CHECK_LAUNCH("lstm_fwd");
    }
    return DIN_OK;
}

int64_t din_lstm_bwd_workspace(int rows, int dirs, int hidden) {
    if (rows < 1 || dirs < 1 || hidden < 1) return 0;
    return (int64_t)dirs * 4 * hidden * hidden + (int64_t)rows * dirs * hidden;
}

int din_lstm_bwd(const float* g_out, const float* gates, const float* cells, const float* w_hh, int rows, int steps, int dirs, int hidden,
                 float* d_pre, float* h_prev, float* ws, int64_t ws_floats, void* stream) {
    DIN_REQUIRE(g_out && gates && cells && w_hh && d_pre && h_prev && ws, "lstm_bwd: null pointer");
    int rc = check_lstm_shape("lstm_bwd", rows, steps, dirs, hidden);
    if (rc != DIN_OK) return rc;
    DIN_REQUIRE(aligned16(g_out) && aligned16(gates) && aligned16(cells) && aligned16(w_hh) && aligned16(d_pre) && aligned16(h_prev) &&
                aligned16(ws), "lstm_bwd: every pointer must be 16-byte aligned");
    const int64_t need = din_lstm_bwd_workspace(rows, dirs, hidden);
    DIN_REQUIRE(ws_floats >= need, "lstm_bwd: workspace of %lld floats, %lld needed", (long long)ws_floats, (long long)need);
    hipStream_t st = as_stream(stream);
    float* wt = ws;
    float* dc = ws + (int64_t)dirs * 4 * hidden * hidden;
    hipLaunchKernelGGL(lstm_transpose_kernel, dim3((hidden + 31) / 32, (4 * hidden + 31) / 32, dirs), dim3(LSTM_THREADS), 0, st, w_hh, hidden,
                       wt);
    DIN_CHECK_LAUNCH("lstm_transpose");
    auto kern = lstm_bwd_step_kernel;                                  // (rows of 4H floats: always 16-byte loads)
    const size_t lds = bwd_lds(hidden);
    din_raise_lds(reinterpret_cast<const void*>(kern), lds);
    const dim3 grid((hidden + LSTM_HS - 1) / LSTM_HS, dirs);
    for (int step = steps - 1; step >= 0; --step) {
        hipLaunchKernelGGL(kern, grid, dim3(LSTM_THREADS), lds, st, g_out, gates, cells, wt, rows, steps, dirs, hidden, step, d_pre, h_prev, dc);
        DIN_CHECK_LAUNCH("lstm_bwd");
    }
    return DIN_OK;
}

}  // extern "C"
