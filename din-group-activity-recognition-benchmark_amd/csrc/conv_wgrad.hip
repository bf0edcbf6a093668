// Weight gradient of the convolutions for gfx950 (MI355X): every weight-gradient kernel family that is not in a file of its own (fp32, bf16
// two-workgroup, bf16 tail, ring, stem), the slice reduce and the column-sum (bias gradient) kernels, the one place that chooses among ALL
// families (plan_wgrad; the pipelined, halo and 1x1-multi kernels live in conv_wgrad_pipe.hip, conv_wgrad_halo.hip and conv_wgrad_1x1.hip),
// and the entry points din_conv_wgrad, din_conv_wgrad_group, din_conv1x1_wgrad_multi (each of the two with its host-only kernel-name reporter)
// and din_colsum.
//
//   dW[co][(r,s,ci)] = sum_pix G[pix][co] * im2col(X)[pix][(r,s,ci)]
//
// Replaces the weight-gradient arithmetic of torch.nn.Conv2d / nn.Linear reached from the reference at backbone/backbone.py:44-99,
// infer_model.py:184,190,226 and infer_module/dynamic_infer_module.py:149,191,195.
#include "din_common.h"
#include "conv_wgrad.h"
#include "conv_shared.h"
#include <atomic>
#include <string>

using din_wgrad::WgradK;
using din_wgrad::WgradChoice;
using din_wgrad::lds_dma16;
using din_conv::check_desc;

namespace {

// ------------------------------------------------------------------------------------------------
// wgrad:  dW[co][(r,s,ci)] = sum_pix G[pix][co] * im2col(X)[pix][(r,s,ci)]
// 128 (co) x 128 (k columns) tile per workgroup, reduction over a slice of the pixels; partials to a
// workspace [slice][cout_pad][kcols_pad] fp32, reduced (and un-permuted to [cout][cin][kh][kw]) afterwards.
// ------------------------------------------------------------------------------------------------
constexpr int WG_TILE = 128;

// fp32: 16 pixels per k-step, operands read with ds_read_b32 (lane k-index = pixel row)
// SPLIT (conv_wgrad_f32x3_kernel, DIN_F32_BF16X3): the same tiles, slices, LDS images and partial layout; the k-step's 16 pixels go through
// ONE three-MFMA group (mma_f32_bf16x3: each lane group holds 4 pixels x 2 parts) instead of four v_mfma_f32_16x16x4_f32.
template <bool SPLIT>
__device__ __forceinline__ void conv_wgrad_f32_body(const WgradK& p) {
    constexpr int PK = 16;
    constexpr int RS = WG_TILE + 16;     // padded row (floats): 4 k-rows hit 4 disjoint bank ranges
    __shared__ float Gs[2][PK][RS];
    __shared__ float Xs[2][PK][RS];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid >> 1, wn = wid & 1;
    int bid, slice_;
    xcd_block(bid, slice_);
    const int k_tile = bid % p.n_k_tiles;
    const int co_tile = bid / p.n_k_tiles;
    const int slice = slice_;
    const int m_begin = slice * p.m_per_slice;
    int m_end = m_begin + p.m_per_slice;
    if (m_end > p.M) m_end = p.M;

    // loader: 16 rows x 32 chunks (of 4 floats) per operand -> 2 chunks per thread per operand
    const int cc = tid & 31, rr = tid >> 5;         // chunk column 0..31, row 0..7 (+8)
    // fixed k column of this thread's X chunk
    const int kcol = k_tile * WG_TILE + cc * 4;
    const bool kok = kcol < p.kcols;
    const int tap = kok ? kcol / p.cin_pad : 0;
    const int ci = kcol - tap * p.cin_pad;
    const int r = tap / p.kw, s = tap - r * p.kw;
    const bool ci_ok = kok && ci < p.Cin;           // Cin % 4 == 0 is enforced by the host unless cin_pad>Cin (conv1)
    const int gco = co_tile * WG_TILE + cc * 4;
    const float* __restrict__ inp = reinterpret_cast<const float*>(p.in);
    const float* __restrict__ gp = reinterpret_cast<const float*>(p.g);

    // pixel coordinates of the two rows this thread loads, advanced incrementally (no divisions in the loop)
    int pn[2], py[2], px[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        int m = m_begin + rr + 8 * i;
        int n = m / (p.OH * p.OW);
        int rem = m - n * (p.OH * p.OW);
        pn[i] = n; py[i] = rem / p.OW; px[i] = rem - py[i] * p.OW;
    }
    f32x4 xa[2], ga[2];
    auto load_global = [&](int m0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            int m = m0 + rr + 8 * i;
            f32x4 xv = {0.f, 0.f, 0.f, 0.f}, gv = {0.f, 0.f, 0.f, 0.f};
            if (m < m_end) {
                int iy = py[i] * p.sh - p.ph + r * p.dh, ix = px[i] * p.sw - p.pw + s * p.dw;
                if (ci_ok && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W) {
                    const float* src = inp + (int64_t)((pn[i] * p.H + iy) * p.W + ix) * p.ldi + p.cioff + ci;
                    if (ci + 3 < p.Cin) xv = *reinterpret_cast<const f32x4*>(src);
                    else for (int e = 0; e < 4 && ci + e < p.Cin; ++e) xv[e] = src[e];
                }
                if (gco < p.Cout) {
                    const float* src = gp + (int64_t)m * p.ldo + p.cooff + gco;
                    if (gco + 3 < p.Cout) gv = *reinterpret_cast<const f32x4*>(src);
                    else for (int e = 0; e < 4 && gco + e < p.Cout; ++e) gv[e] = src[e];
                }
            }
            xa[i] = xv; ga[i] = gv;
            // advance this row by PK pixels
            px[i] += PK;
            while (px[i] >= p.OW) { px[i] -= p.OW; if (++py[i] == p.OH) { py[i] = 0; ++pn[i]; } }
        }
    };
    auto store_lds = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            *reinterpret_cast<f32x4*>(&Xs[buf][rr + 8 * i][cc * 4]) = xa[i];
            *reinterpret_cast<f32x4*>(&Gs[buf][rr + 8 * i][cc * 4]) = ga[i];
        }
    };

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int fcol = lane & 15, frow = lane >> 4;
    if (m_begin < m_end) {
        load_global(m_begin);
        store_lds(0);
        __syncthreads();
        int it = 0;
        for (int m0 = m_begin; m0 < m_end; m0 += PK, ++it) {
            const int cur = it & 1;
            const bool more = m0 + PK < m_end;
            if (more) load_global(m0 + PK);
            if constexpr (SPLIT) {
                // lane group g holds pixels g, g + 4, g + 8, g + 12: read e touches the rows the exact kernel's MFMA e touches (rows 4 e + g
                // of the four groups lie in four disjoint bank ranges), and a sum does not care about the k order
                u32x4 gf[4], xf[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) gf[i][e] = __float_as_uint(Gs[cur][e * 4 + frow][wm * 64 + i * 16 + fcol]);
#pragma unroll
                    for (int j = 0; j < 4; ++j) xf[j][e] = __float_as_uint(Xs[cur][e * 4 + frow][wn * 64 + j * 16 + fcol]);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) mma_f32_bf16x3(gf[i], xf[j], acc[i][j]);
            } else
#pragma unroll
            for (int kk = 0; kk < PK / 4; ++kk) {
                float gf[4], xf[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) gf[i] = Gs[cur][kk * 4 + frow][wm * 64 + i * 16 + fcol];
#pragma unroll
                for (int j = 0; j < 4; ++j) xf[j] = Xs[cur][kk * 4 + frow][wn * 64 + j * 16 + fcol];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(gf[i], xf[j], acc[i][j], 0, 0, 0);
            }
            if (more) store_lds(cur ^ 1);
            __syncthreads();
        }
    }
    // D[i = co][j = kcol]: lane holds co = ..+(lane>>4)*4+e, kcol = ..+(lane&15)
    float* dst = p.partial + (int64_t)slice * p.cout_pad * p.kcols_pad;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int co = co_tile * WG_TILE + wm * 64 + i * 16 + (lane >> 4) * 4;
            int kc = k_tile * WG_TILE + wn * 64 + j * 16 + (lane & 15);
#pragma unroll
            for (int e = 0; e < 4; ++e) dst[(int64_t)(co + e) * p.kcols_pad + kc] = acc[i][j][e];
        }
}
__global__ __launch_bounds__(NTHREADS, 2) void conv_wgrad_f32_kernel(WgradK p) { conv_wgrad_f32_body<false>(p); }
__global__ __launch_bounds__(NTHREADS, 2) void conv_wgrad_f32x3_kernel(WgradK p) { conv_wgrad_f32_body<true>(p); }

// bf16: 32 pixels per k-step; operands are stored [pixel][channel] in LDS (as they sit in HBM) and read with the
// gfx950 transpose read ds_read_b64_tr_b16, which hands lane i of a 16-lane group column i of a 4x16 block.
// k (pixel) order inside the k-step: lane group g, element e -> pixel 4g+e (e<4) or 16+4g+(e-4): the two
// 32-lane halves of each ds_read_b64 then cover 8 consecutive rows = one full 256-byte bank row (RS pad 32 B).
__device__ __forceinline__ u32x2 lds_tr_read(uint32_t byte_addr) {
    u32x2 r;
    asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(r) : "v"(byte_addr) : "memory");
    return r;
}

// v3: 64 pixels per k-step; operands arrive by LDS-DMA (buffer_load ... lds, issued through inline asm and counted by hand like the
// gather kernel): G: constant per-lane offset + scalar row offset; X: per-row offset advanced incrementally, out-of-image taps ->
// hardware zero.  LDS-DMA is lane-linear, so the tiles are UNPADDED [pixel][channel] images; bank conflicts of the transpose reads
// are avoided by rotating each row's 16-byte chunks by 2*(row & 7) -- applied on the SOURCE side (the lane fetches the logical chunk
// that belongs at its slot) and in the read addresses.  BCO in {64,96,128,160} filter rows x 128 k columns per workgroup; the bias
// gradient is fused in: the k_tile == 0 workgroups' kcol-half-0 waves also multiply their G fragments with an all-ones operand.
template <int BCO>
__global__ __launch_bounds__(NTHREADS, 2) void conv_wgrad_bf16_kernel(WgradK p) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int PK = 64;
    constexpr int CG = BCO / 8, CX = WG_TILE / 8;                 // 16-byte chunks per G / X row
    constexpr int RBG = BCO * 2, RBX = WG_TILE * 2;               // row bytes (unpadded)
    constexpr int OPG = PK * RBG, OPX = PK * RBX, STAGE = OPG + OPX;
    constexpr int TI = BCO / 32;                                  // 16-row filter tiles per wave (wave tile = BCO/2 x 64)
    constexpr int GP = PK * CG / NTHREADS;                        // G DMA chunks per thread per stage (= BCO/32)
    constexpr int XP = PK * CX / NTHREADS;                        // X DMA chunks per thread per stage (= 4)
    constexpr unsigned OOB = 0x80000000u;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid >> 1, wn = wid & 1;
    int bx_, by_;
    xcd_block(bx_, by_);
    const int k_tile = bx_ % p.n_k_tiles, co_tile = bx_ / p.n_k_tiles;
    const int slice = by_;
    const int m_begin = slice * p.m_per_slice;                   // multiple of PK
    int m_end = m_begin + p.m_per_slice;
    if (m_end > p.M) m_end = p.M;

    // ---- buffer resources (base moved to the slice's first image / first pixel so 32-bit offsets always suffice) ----
    const int ohw = p.OH * p.OW;
    const int n_first = m_begin / ohw;
    const long long img_bytes = (long long)p.H * p.W * p.ldi * 2ll;
    const long long x_off = (long long)n_first * img_bytes;
    long long x_rem = (long long)p.NB * img_bytes - x_off;
    if (x_rem > 0x7fffffffll) x_rem = 0x7fffffffll;
    __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(p.in)) + x_off, 0, (int)x_rem, 0x00020000);
    const long long g_off = (long long)m_begin * p.ldo * 2ll;
    long long g_rem = (long long)p.M * p.ldo * 2ll - g_off;
    if (g_rem > 0x7fffffffll) g_rem = 0x7fffffffll;
    __amdgpu_buffer_rsrc_t rsG = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(p.g)) + g_off, 0, (int)g_rem, 0x00020000);

    // ---- G DMA: wave-level transfer t of this wave covers chunk ids [(wid + 4 t) * 64, +64): id -> (row id / CG, slot id % CG);
    //      the lane fetches logical chunk (slot - 2*(row & 7)) mod CG of that row ---------------------------------------------
    unsigned voffG[GP];
#pragma unroll
    for (int t = 0; t < GP; ++t) {
        const int id = (wid + 4 * t) * 64 + lane;
        const int grow = id / CG, slot = id - grow * CG;
        int gc = slot - 2 * (grow & 7);
        gc += gc < 0 ? CG : 0;
        gc += gc < 0 ? CG : 0;                                      // 2*(row&7) <= 14 may exceed CG = 8 or 12 once
        const int gco = co_tile * BCO + gc * 8;
        voffG[t] = (gco + 7 < p.Cout) ? (unsigned)((grow * p.ldo + p.cooff + gco) * 2) : OOB;   // Cout % 8 == 0 enforced
    }
    // ---- X DMA: transfer t covers rows (wid + 4 t) * 4 + (lane >> 4); rotation 2*(row & 7) is the same for all t, so the lane's
    //      logical chunk -- hence its (tap, ci) -- is fixed -------------------------------------------------------------------
    const int xrow0 = wid * 4 + (lane >> 4);                       // rows xrow0 + 16 t
    int xc = (lane & 15) - 2 * (xrow0 & 7);
    xc += xc < 0 ? CX : 0;
    const int kcol = k_tile * WG_TILE + xc * 8;
    const bool kok = kcol < p.kcols;
    const int tap = kok ? kcol / p.cin_pad : 0;
    const int ci = kcol - tap * p.cin_pad;
    const int tr_ = tap / p.kw, ts_ = tap - tr_ * p.kw;
    const bool ci_ok = kok && ci + 7 < p.Cin;                       // Cin % 8 == 0 enforced (conv1 uses the tail kernel)
    const int dy0 = -p.ph + tr_ * p.dh, dx0 = -p.pw + ts_ * p.dw;   // iy = oy*sh + dy0, ix = ox*sw + dx0
    const int step_bytes = p.sw * p.ldi * 2;                        // +1 output column
    int px[XP], py[XP];          // output coordinates of this thread's rows
    int rowoff[XP];              // byte offset of (n, iy, ix = dx0) for the current (n, oy): may be "virtual"
#pragma unroll
    for (int t = 0; t < XP; ++t) {
        int m = m_begin + xrow0 + 16 * t;
        int n = m / ohw;
        int rem = m - n * ohw;
        py[t] = rem / p.OW; px[t] = rem - py[t] * p.OW;
        rowoff[t] = (((n - n_first) * p.H + py[t] * p.sh + dy0) * p.W + dx0) * p.ldi * 2 + (p.cioff + ci) * 2;
    }
    const int row_jump = p.sh * p.W * p.ldi * 2;                    // +1 output row
    const int img_jump = (p.H - p.OH * p.sh) * p.W * p.ldi * 2;     // extra when wrapping to the next image

    const uint32_t lds_base = (uint32_t)(uintptr_t)smem_raw;
    const uint32_t ldsW = __builtin_amdgcn_readfirstlane(lds_base + (uint32_t)(wid * 1024));   // this wave's first 1-KiB slot
    auto issue_dma = [&](int buf, int m0) {
        const uint32_t Gd = ldsW + (uint32_t)(buf * STAGE), Xd = Gd + (uint32_t)OPG;
        const int soffG = (m0 - m_begin) * p.ldo * 2;                // uniform
#pragma unroll
        for (int t = 0; t < GP; ++t) lds_dma16(Gd + (uint32_t)(t * 4096), rsG, (int)voffG[t], soffG);
#pragma unroll
        for (int t = 0; t < XP; ++t) {
            const int iy = py[t] * p.sh + dy0, ix = px[t] * p.sw + dx0;
            const bool ok = ci_ok && (m0 + xrow0 + 16 * t < m_end) && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
            const unsigned vo = ok ? (unsigned)(rowoff[t] + px[t] * step_bytes) : OOB;
            lds_dma16(Xd + (uint32_t)(t * 4096), rsX, (int)vo, 0);
            // advance this row by PK output pixels
            px[t] += PK;
            while (px[t] >= p.OW) {
                px[t] -= p.OW; rowoff[t] += row_jump;
                if (++py[t] == p.OH) { py[t] = 0; rowoff[t] += img_jump; }
            }
        }
    };

    f32x4 acc[TI][4], accb[TI];
#pragma unroll
    for (int i = 0; i < TI; ++i) {
        accb[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const bool do_bias = p.dbias != nullptr && k_tile == 0 && wn == 0;       // wave-uniform
    const u32x4 ones = {0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};

    // transpose-read addressing: lane i of a 16-lane group supplies the 8-byte piece (row 4*lg + (i>>2), cols 4*(i&3)..+3) of a
    // 16-column tile, i.e. chunk (tile_chunk + ((i&3)>>1)), half (i&1); rows of the second read are +16 (same row & 7 -> same rotation)
    const int li = lane & 15, lg = lane >> 4;
    const int prow = 4 * lg + (li >> 2);
    const int rot = 2 * (prow & 7);
    uint32_t colG[TI], colX[4];
#pragma unroll
    for (int i = 0; i < TI; ++i) {
        int ch = (wm * (BCO / 2) + i * 16) / 8 + rot;                         // even
        ch -= ch >= CG ? CG : 0;
        ch -= ch >= CG ? CG : 0;
        colG[i] = (uint32_t)(prow * RBG + (ch + ((li & 3) >> 1)) * 16 + (li & 1) * 8);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int ch = (wn * 64 + j * 16) / 8 + rot;
        ch -= ch >= CX ? CX : 0;
        colX[j] = (uint32_t)(prow * RBX + (ch + ((li & 3) >> 1)) * 16 + (li & 1) * 8);
    }
    auto compute = [&](int cur) {
#pragma unroll
        for (int kg = 0; kg < 2; ++kg) {                                       // two 32-pixel MFMA k-groups per stage
            const uint32_t Gb = lds_base + cur * STAGE + kg * 32 * RBG;
            const uint32_t Xb = lds_base + cur * STAGE + OPG + kg * 32 * RBX;
            u32x4 gf[TI], xf[4];
#pragma unroll
            for (int i = 0; i < TI; ++i) {
                u32x2 lo = lds_tr_read(Gb + colG[i]), hi = lds_tr_read(Gb + colG[i] + 16 * RBG);
                gf[i] = u32x4{lo[0], lo[1], hi[0], hi[1]};
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                u32x2 lo = lds_tr_read(Xb + colX[j]), hi = lds_tr_read(Xb + colX[j] + 16 * RBX);
                xf[j] = u32x4{lo[0], lo[1], hi[0], hi[1]};
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < TI; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, gf[i]),
                                                                        __builtin_bit_cast(bf16x8, xf[j]), acc[i][j], 0, 0, 0);
            if (do_bias) {
#pragma unroll
                for (int i = 0; i < TI; ++i)
                    accb[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, gf[i]),
                                                                      __builtin_bit_cast(bf16x8, ones), accb[i], 0, 0, 0);
            }
        }
    };

    if (m_begin < m_end) {
        issue_dma(0, m_begin);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        int it = 0;
        for (int m0 = m_begin; m0 < m_end; m0 += PK, ++it) {
            const int cur = it & 1;
            if (m0 + PK < m_end && p.probe != 2) issue_dma(cur ^ 1, m0 + PK);
            if (p.probe != 1) compute(cur);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
        }
    }
    float* dst = p.partial + (int64_t)slice * p.cout_pad * p.kcols_pad;
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int co = co_tile * BCO + wm * (BCO / 2) + i * 16 + (lane >> 4) * 4;
            int kc = k_tile * WG_TILE + wn * 64 + j * 16 + (lane & 15);
#pragma unroll
            for (int e = 0; e < 4; ++e) dst[(int64_t)(co + e) * p.kcols_pad + kc] = acc[i][j][e];
        }
    if (do_bias && (lane & 15) == 0) {
#pragma unroll
        for (int i = 0; i < TI; ++i) {
            int co = co_tile * BCO + wm * (BCO / 2) + i * 16 + (lane >> 4) * 4;
#pragma unroll
            for (int e = 0; e < 4; ++e) if (co + e < p.Cout) atomicAdd(p.dbias + co + e, accb[i][e]);
        }
    }
#endif
}

// v4 ("ring"): the v3 kernel is bound by the global->LDS stream (DIN_WGRAD_PROBE=1: streaming alone takes 75-87 % of its time, at
// ~9-10 TB/s of LDS-DMA traffic), so the lever is bytes per FLOP: BCO x BK = {128,192,256} x 256 tiles (per-wave (BCO/2) x 128) move
// 1.3-2.3x fewer bytes than BCO x 128.  One workgroup per CU (accumulators fill the register file), so latency is hidden inside
// the wave: a 4-stage ring of 32-pixel stages with the LDS-DMA issued THREE stages ahead (hand-counted vmcnt), and the transpose
// reads of stage s in flight while the MFMAs of stage s-1 run (register double buffer).  One s_barrier per stage.
template <int BCO, int BK>
__global__ __launch_bounds__(512, (4 * (((32 * (BCO / 8) + 511) / 512) * 8192 + 32 * BK * 2) <= 80 * 1024) ? 2 : 1) void conv_wgrad_ring_kernel(WgradK p) {
#if defined(__HIP_DEVICE_COMPILE__)
    // 8 waves (2 x 4: filter half wm, k-column quarter wn), two per SIMD: one wave's barrier / vmcnt / transpose-read waits hide
    // behind the other's MFMAs (with one wave per SIMD they are all serial; cf. profiles/r01_halo_probe.txt)
    constexpr int PK = 32, NS = 4, NWV = 8, NTH = 64 * NWV;
    constexpr int CG = BCO / 8, CX = BK / 8;                      // 16-byte chunks per G / X row
    constexpr int RBG = BCO * 2, RBX = BK * 2;                    // row bytes (unpadded)
    constexpr int TI = BCO / 32, XJ = BK / 64;                    // 16-row / 16-column MFMA tiles per wave (wave tile = BCO/2 x BK/4)
    constexpr int GP = (PK * CG + NTH - 1) / NTH, XP = PK * CX / NTH;
    static_assert(PK * CX % NTH == 0, "whole X DMA transfers per thread");
    // every wave issues the same number of transfers (the vmcnt bookkeeping is a compile-time constant): when the G tile is not a
    // whole number of 4-KiB rounds (BCO = 160) the surplus transfers fetch nothing and land in a pad behind the G tile
    constexpr int OPG = GP * 1024 * NWV, OPX = PK * RBX, STAGE = OPG + OPX;
    static_assert(OPG >= PK * RBG, "G region");
    constexpr int RPT = 64 / CX;                                  // X rows per wave-level transfer
    constexpr int NDMA = GP + XP;                                 // DMA instructions per stage per wave
    constexpr unsigned OOB = 0x80000000u;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid >> 2, wn = wid & 3;
    int bx_, by_;
    xcd_block(bx_, by_);
    const int k_tile = bx_ % p.n_k_tiles, co_tile = bx_ / p.n_k_tiles;
    const int slice = by_;
    const int m_begin = slice * p.m_per_slice;                   // multiple of PK
    int m_end = m_begin + p.m_per_slice;
    if (m_end > p.M) m_end = p.M;

    const int ohw = p.OH * p.OW;
    const int n_first = m_begin / ohw;
    const long long img_bytes = (long long)p.H * p.W * p.ldi * 2ll;
    const long long x_off = (long long)n_first * img_bytes;
    long long x_rem = (long long)p.NB * img_bytes - x_off;
    if (x_rem > 0x7fffffffll) x_rem = 0x7fffffffll;
    __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(p.in)) + x_off, 0, (int)x_rem, 0x00020000);
    const long long g_off = (long long)m_begin * p.ldo * 2ll;
    long long g_rem = (long long)p.M * p.ldo * 2ll - g_off;
    if (g_rem > 0x7fffffffll) g_rem = 0x7fffffffll;
    __amdgpu_buffer_rsrc_t rsG = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(p.g)) + g_off, 0, (int)g_rem, 0x00020000);

    // ---- G DMA plan: transfer t covers chunk ids [(wid + 4 t) * 64, +64): id -> (row id / CG, slot id % CG); the lane fetches the
    //      logical chunk (slot - 2*(row & 7)) mod CG of that row (rotation against transpose-read bank conflicts) --------------
    unsigned voffG[GP];
#pragma unroll
    for (int t = 0; t < GP; ++t) {
        const int id = (wid + NWV * t) * 64 + lane;
        const int grow = id / CG, slot = id - grow * CG;
        int gc = slot - 2 * (grow & 7);
        gc += gc < 0 ? CG : 0;
        gc += gc < 0 ? CG : 0;                                      // 2*(row&7) <= 14 exceeds CG = 8 / 12 once more
        const int gco = co_tile * BCO + gc * 8;
        voffG[t] = (grow < PK && gco + 7 < p.Cout) ? (unsigned)((grow * p.ldo + p.cooff + gco) * 2) : OOB;   // Cout % 8 == 0 enforced
    }
    // ---- X DMA plan: transfer t covers rows (wid + 4 t) * RPT + lane / CX; (row & 7) is the same for all t -----------------------
    const int xrow0 = wid * RPT + lane / CX;                       // rows xrow0 + NWV RPT t
    int xc = (lane % CX) - 2 * (xrow0 & 7);
    xc += xc < 0 ? CX : 0;
    const int kcol = k_tile * BK + xc * 8;
    const bool kok = kcol < p.kcols;
    const int tap = kok ? kcol / p.cin_pad : 0;
    const int ci = kcol - tap * p.cin_pad;
    const int tr_ = tap / p.kw, ts_ = tap - tr_ * p.kw;
    const bool ci_ok = kok && ci + 7 < p.Cin;
    const int dy0 = -p.ph + tr_ * p.dh, dx0 = -p.pw + ts_ * p.dw;   // iy = oy*sh + dy0, ix = ox*sw + dx0
    const int step_bytes = p.sw * p.ldi * 2;
    int px[XP], py[XP], rowoff[XP];
#pragma unroll
    for (int t = 0; t < XP; ++t) {
        int m = m_begin + xrow0 + NWV * RPT * t;
        int n = m / ohw;
        int rem = m - n * ohw;
        py[t] = rem / p.OW; px[t] = rem - py[t] * p.OW;
        rowoff[t] = (((n - n_first) * p.H + py[t] * p.sh + dy0) * p.W + dx0) * p.ldi * 2 + (p.cioff + ci) * 2;
    }
    const int row_jump = p.sh * p.W * p.ldi * 2;
    const int img_jump = (p.H - p.OH * p.sh) * p.W * p.ldi * 2;

    const uint32_t lds_base = (uint32_t)(uintptr_t)smem_raw;
    const uint32_t ldsW = __builtin_amdgcn_readfirstlane(lds_base + (uint32_t)(wid * 1024));
    auto issue_dma = [&](int buf, int m0) {                         // called with consecutive m0 (the X cursors advance by PK)
        const uint32_t Gd = ldsW + (uint32_t)(buf * STAGE), Xd = Gd + (uint32_t)OPG;
        const int soffG = (m0 - m_begin) * p.ldo * 2;
#pragma unroll
        for (int t = 0; t < GP; ++t) lds_dma16(Gd + (uint32_t)(t * 1024 * NWV), rsG, (int)voffG[t], soffG);   // rows past M: out of range -> zeros
#pragma unroll
        for (int t = 0; t < XP; ++t) {
            const int iy = py[t] * p.sh + dy0, ix = px[t] * p.sw + dx0;
            const bool ok = ci_ok && (m0 + xrow0 + NWV * RPT * t < m_end) && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
            lds_dma16(Xd + (uint32_t)(t * 1024 * NWV), rsX, ok ? rowoff[t] + px[t] * step_bytes : (int)OOB, 0);
            px[t] += PK;
            while (px[t] >= p.OW) {
                px[t] -= p.OW; rowoff[t] += row_jump;
                if (++py[t] == p.OH) { py[t] = 0; rowoff[t] += img_jump; }
            }
        }
    };

    f32x4 acc[TI][XJ], accb[TI];
#pragma unroll
    for (int i = 0; i < TI; ++i) {
        accb[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < XJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const bool do_bias = p.dbias != nullptr && k_tile == 0 && wn == 0;       // wave-uniform
    const u32x4 ones = {0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};

    const int li = lane & 15, lg = lane >> 4;
    const int prow = 4 * lg + (li >> 2);
    const int rot = 2 * (prow & 7);
    uint32_t colG[TI], colX[XJ];
#pragma unroll
    for (int i = 0; i < TI; ++i) {
        int ch = (wm * (BCO / 2) + i * 16) / 8 + rot;                         // even
        ch -= ch >= CG ? CG : 0;
        ch -= ch >= CG ? CG : 0;
        colG[i] = (uint32_t)(prow * RBG + (ch + ((li & 3) >> 1)) * 16 + (li & 1) * 8);
    }
#pragma unroll
    for (int j = 0; j < XJ; ++j) {
        int ch = (wn * (BK / 4) + j * 16) / 8 + rot;
        ch -= ch >= CX ? CX : 0;
        colX[j] = (uint32_t)(prow * RBX + (ch + ((li & 3) >> 1)) * 16 + (li & 1) * 8);
    }
    u32x4 gf[TI], xf[XJ];
    auto load_frags = [&](int buf) {
        const uint32_t Gb = lds_base + (uint32_t)(buf * STAGE), Xb = Gb + (uint32_t)OPG;
#pragma unroll
        for (int i = 0; i < TI; ++i) {
            u32x2 lo = lds_tr_read(Gb + colG[i]), hi = lds_tr_read(Gb + colG[i] + 16 * RBG);
            gf[i] = u32x4{lo[0], lo[1], hi[0], hi[1]};
        }
#pragma unroll
        for (int j = 0; j < XJ; ++j) {
            u32x2 lo = lds_tr_read(Xb + colX[j]), hi = lds_tr_read(Xb + colX[j] + 16 * RBX);
            xf[j] = u32x4{lo[0], lo[1], hi[0], hi[1]};
        }
    };

    const int nst = (m_end - m_begin + PK - 1) / PK;                          // stages of this slice (>= 0)
    if (nst > 0) {
        // prologue: stages 0..2 in flight
#pragma unroll
        for (int s0 = 0; s0 < NS - 1; ++s0)
            if (s0 < nst) issue_dma(s0, m_begin + s0 * PK);
        // iteration s: [stage s landed] barrier, DMA stage s+3, transpose reads + MFMAs of stage s (the SIMD's other wave overlaps)
        for (int s2 = 0; s2 < nst; ++s2) {
            // stages s2+1, s2+2 may stay in flight (issued after stage s2); near the end fewer are outstanding -> drain
            if (s2 + 2 < nst) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 * NDMA) : "memory");
            else if (s2 + 1 < nst) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(NDMA) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            if (s2 + NS - 1 < nst) issue_dma((s2 + NS - 1) & (NS - 1), m_begin + (s2 + NS - 1) * PK);
            load_frags(s2 & (NS - 1));
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < TI; ++i)
#pragma unroll
                for (int j = 0; j < XJ; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, gf[i]), __builtin_bit_cast(bf16x8, xf[j]), acc[i][j], 0, 0, 0);
            if (do_bias) {
#pragma unroll
                for (int i = 0; i < TI; ++i)
                    accb[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, gf[i]), __builtin_bit_cast(bf16x8, ones), accb[i], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    float* dst = p.partial + (int64_t)slice * p.cout_pad * p.kcols_pad;
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < XJ; ++j) {
            int co = co_tile * BCO + wm * (BCO / 2) + i * 16 + (lane >> 4) * 4;
            int kc = k_tile * BK + wn * (BK / 4) + j * 16 + (lane & 15);
#pragma unroll
            for (int e = 0; e < 4; ++e) dst[(int64_t)(co + e) * p.kcols_pad + kc] = acc[i][j][e];
        }
    if (do_bias && (lane & 15) == 0) {
#pragma unroll
        for (int i = 0; i < TI; ++i) {
            int co = co_tile * BCO + wm * (BCO / 2) + i * 16 + (lane >> 4) * 4;
#pragma unroll
            for (int e = 0; e < 4; ++e) if (co + e < p.Cout) atomicAdd(p.dbias + co + e, accb[i][e]);
        }
    }
#endif
}

// ------------------------------------------------------------------------------------------------
// wgrad of the stem layers (3x3; 32 -> 32/64 channels stride 1, and the image layer <= 8 padded channels -> 32, stride 2): millions of
// pixels, a few thousand filter gradients.  The general kernel re-pulls every input pixel once per tap and every G pixel once per
// k-column tile; here each 8x32 output tile brings its G tile and its input HALO in once (LDS-DMA, out-of-image -> hardware zeros),
// all (tap, ci) columns are formed from LDS by transpose reads, and persistent workgroups keep the whole dW block
// (BN x 9*cin_pad fp32) in registers across their tiles: HBM traffic = the two tensors once.
//   k (pixel) assignment inside a 32-pixel k-step = one tile row: read rd, lane group g4, sub-row q -> x = 16 rd + 4 g4 + q; each
//   32-lane half of a ds_read_b64_tr_b16 then covers 8 consecutive pixels, conflict-free with the unit swizzles below.
//   wave w owns the 16-column tiles w, w+4, ... of the (tap, ci) axis and all BN filter rows; wave 0 also forms the bias gradient
//   (G^T x ones).  Result: one fp32 partial slab per workgroup in the layout conv_wgrad_reduce_kernel expects.
// ------------------------------------------------------------------------------------------------
// NW: waves per workgroup.  The 32 -> 64 layer (Conv2d_2b) needs 108 KiB of LDS, i.e. one workgroup per CU: with four waves that is ONE wave
// per SIMD (3.1 TB/s); eight waves split the 18 column tiles 3 / 2 per wave instead of 5 / 4 and give every SIMD two waves.
// TH_ / RING (round 6): the 32 -> 64 layer runs ONE workgroup per CU, and with two 54 KB stages only one tile's operands are in flight per CU
// while the current tile is multiplied -- the tile time was the memory latency + transfer of one stage (3.05 us, 4.1 TB/s), not max(compute,
// transfer).  <..., TH_ = 6, RING = 3>: 6 x 32 tiles (42 KB per stage: 24.6 KB of G + 17.4 KB of halo) in a THREE-slot ring with TWO stages in
// flight (126 KB), the oldest waited for with a counted vmcnt.  The halo overhead grows from 10/8 to 8/6 of the input (+2 % bytes).
template <int CPP, int BN, int ST, bool U8 = false, int NW = 4, int TH_ = 8, int RING = 2>
__global__ __launch_bounds__(64 * NW, (CPP == 4 && BN == 64) ? 1 : 2) void conv_wgrad_small_kernel(WgradK p) {
    static_assert(!U8 || CPP == 1, "uint8 frames feed the image layer only");
    static_assert(RING == 2 || (RING == 3 && !U8), "three-slot ring: LDS-DMA operands only");
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int TH = TH_, TW = 32, NPX = TH * TW, KH = 3, KW = 3;
    constexpr int HWW = (TW - 1) * ST + KW, HWH = (TH - 1) * ST + KH, HPX = HWW * HWH, HC = HPX * CPP;
    constexpr int HBYTES = (HC * 16 + 1023) / 1024 * 1024, NSLOT_H = HBYTES / 1024, NTR_H = (NSLOT_H + NW - 1) / NW;
    constexpr int CG = BN / 8, GBYTES = NPX * CG * 16, NTR_G = GBYTES / (1024 * NW);
    constexpr int STAGE = HBYTES + GBYTES;
    constexpr int NCT = CPP == 4 ? 18 : 5, TI = BN / 16, TJ = (NCT + NW - 1) / NW;
    constexpr unsigned OOB = 0x80000000u;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    auto swzX = [](int hp) { return CPP == 4 ? ((hp >> 2) & 1) * 2 : 0; };
    auto swzG = [](int t) { return BN == 32 ? ((t >> 2) & 1) * 2 : ((t >> 1) & 3) * 2; };

    // ---- DMA plans (per lane, tile independent) ----------------------------------------------------------------------------
    int relH[NTR_H]; short hyv[NTR_H], hxv[NTR_H];
#pragma unroll
    for (int i = 0; i < NTR_H; ++i) {
        const int id = (wid + NW * i) * 64 + lane;
        const int hp = id / CPP, slot = id - hp * CPP;
        const int cc = slot ^ swzX(hp);
        const int hy = hp / HWW, hx = hp - hy * HWW;
        relH[i] = id < HC ? (hy * p.W + hx) * p.ldi * 2 + cc * 16 : -1;
        hyv[i] = (short)hy; hxv[i] = (short)hx;
    }
    int relG[NTR_G]; short gyv[NTR_G], gxv[NTR_G];
#pragma unroll
    for (int i = 0; i < NTR_G; ++i) {
        const int id = (wid + NW * i) * 64 + lane;
        const int t = id / CG, slot = id - t * CG;
        const int cc = slot ^ swzG(t);
        gyv[i] = (short)(t >> 5); gxv[i] = (short)(t & 31);
        relG[i] = (cc * 8 + 7 < p.Cout) ? ((t >> 5) * p.OW + (t & 31)) * p.ldo * 2 + cc * 16 : -1;     // Cout % 8 == 0
    }
    const int tiles_x = (p.OW + TW - 1) / TW, tiles_y = (p.OH + TH - 1) / TH;
    const int tiles_img = tiles_x * tiles_y, ntiles = tiles_img * p.NB;
    const long long ximg = (long long)p.H * p.W * p.ldi * 2ll, gimg = (long long)p.OH * p.OW * p.ldo * 2ll;
    const uint32_t lds_base = (uint32_t)(uintptr_t)smem_raw;
    const uint32_t ldsW = __builtin_amdgcn_readfirstlane(lds_base + (uint32_t)(wid * 1024));

    auto issue = [&](int buf, int tile) {
        const int n = tile / tiles_img;
        const int tr = tile - n * tiles_img;
        const int ty = tr / tiles_x, tx = tr - ty * tiles_x;
        const int gy0 = ty * TH * ST - p.ph, gx0 = tx * TW * ST - p.pw;
        __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<char*>(reinterpret_cast<const char*>(p.in)) + (long long)n * ximg, 0, (int)ximg, 0x00020000);
        __amdgpu_buffer_rsrc_t rsG = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<char*>(reinterpret_cast<const char*>(p.g)) + (long long)n * gimg, 0, (int)gimg, 0x00020000);
        const int baseX = (gy0 * p.W + gx0) * p.ldi * 2 + p.cioff * 2;
        const int baseG = ((ty * TH) * p.OW + tx * TW) * p.ldo * 2 + p.cooff * 2;
        const uint32_t dH = ldsW + (uint32_t)(buf * STAGE), dG = dH + (uint32_t)HBYTES;
        if (!U8) {
#pragma unroll
            for (int i = 0; i < NTR_H; ++i) {
                if (wid + NW * i < NSLOT_H) {
                    const int gy = gy0 + hyv[i], gx = gx0 + hxv[i];
                    const bool ok = relH[i] >= 0 && gy >= 0 && gy < p.H && gx >= 0 && gx < p.W;
                    lds_dma16(dH + (uint32_t)(i * 1024 * NW), rsX, ok ? baseX + relH[i] : (int)OOB, 0);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < NTR_G; ++i) {
            const bool ok = relG[i] >= 0 && ty * TH + gyv[i] < p.OH && tx * TW + gxv[i] < p.OW;
            lds_dma16(dG + (uint32_t)(i * 1024 * NW), rsG, ok ? baseG + relG[i] : (int)OOB, 0);
        }
    };

    f32x4 acc[TI][TJ], accb[TI];
#pragma unroll
    for (int i = 0; i < TI; ++i) {
        accb[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < TJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const bool do_bias = p.dbias != nullptr && wid == 0;
    const u32x4 ones = {0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};

    // ---- transpose-read addressing (per lane, tile independent): lane i16 of a 16-lane group supplies the 8-byte piece
    //      (k row = i16 >> 2, columns 4*(i16&3)..+3) and receives column i16 ---------------------------------------------------
    const int i16 = lane & 15, g4 = lane >> 4;
    const int xq = g4 * 4 + (i16 >> 2);                                 // x inside the 16-pixel read (add 16 * rd)
    const int csel = (i16 & 3) >> 1, chalf = (i16 & 1) * 8;
    int tapoff[TJ];                                                     // halo pixel offset of this lane's tap for its column tiles
    int unitX[TJ];
#pragma unroll
    for (int jj = 0; jj < TJ; ++jj) {
        const int j = min(wid + NW * jj, NCT - 1);
        const int tap = CPP == 4 ? (j >> 1) : min(2 * j + csel, KH * KW - 1);
        const int r = tap / KW, s2 = tap - r * KW;
        tapoff[jj] = r * HWW + s2;
        unitX[jj] = j & 1;
    }

    // uint8 frames (U8): the input halo is fetched as bytes into registers where the DMA is issued, and written (normalised, bf16) to the
    // other stage's halo buffer after this tile's MFMAs; the G tile still arrives by LDS-DMA
    U8Halo<NTR_H> u8h;
    bf16_t* u8lut = reinterpret_cast<bf16_t*>(smem_raw + 2 * STAGE);                    // 512 bytes behind the two stages (host adds them)
    if (U8) { u8_lut_init(u8lut, tid); __syncthreads(); }
    auto u8_load = [&](int tile) {
        const int n = tile / tiles_img;
        const int tr = tile - n * tiles_img;
        const int ty = tr / tiles_x, tx = tr - ty * tiles_x;
        u8h.template load<NSLOT_H>(p.u8, n, p.H, p.W, ty * TH * ST - p.ph, tx * TW * ST - p.pw, wid, hyv, hxv, relH);
    };
    // one tile's MFMAs from ring slot `slot` (shared by both ring forms)
    auto multiply = [&](int slot) {
        const uint32_t Hb = lds_base + (uint32_t)(slot * STAGE), Gb = Hb + (uint32_t)HBYTES;
        u32x4 gf[2][TI], xf[2][TJ];
        auto load_frags = [&](int ks, u32x4 (&gfr)[TI], u32x4 (&xfr)[TJ]) {
#pragma unroll
            for (int i = 0; i < TI; ++i) {
                u32x2 rr[2];
#pragma unroll
                for (int rd = 0; rd < 2; ++rd) {
                    const int t = ks * 32 + rd * 16 + xq;
                    const int ch = (i * 2) ^ swzG(t);
                    rr[rd] = lds_tr_read(Gb + (uint32_t)((t * CG + ch + csel) * 16 + chalf));
                }
                gfr[i] = u32x4{rr[0][0], rr[0][1], rr[1][0], rr[1][1]};
            }
#pragma unroll
            for (int jj = 0; jj < TJ; ++jj) {
                u32x2 rr[2];
#pragma unroll
                for (int rd = 0; rd < 2; ++rd) {
                    const int hp = ks * ST * HWW + (rd * 16 + xq) * ST + tapoff[jj];
                    uint32_t a;
                    if (CPP == 4) a = (uint32_t)((hp * 4 + ((unitX[jj] * 2) ^ swzX(hp)) + csel) * 16 + chalf);
                    else a = (uint32_t)(hp * 16 + chalf);
                    rr[rd] = lds_tr_read(Hb + a);
                }
                xfr[jj] = u32x4{rr[0][0], rr[0][1], rr[1][0], rr[1][1]};
            }
        };
        load_frags(0, gf[0], xf[0]);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ks = 0; ks < TH; ++ks) {
            if (ks + 1 < TH) load_frags(ks + 1, gf[(ks + 1) & 1], xf[(ks + 1) & 1]);
#pragma unroll
            for (int i = 0; i < TI; ++i)
#pragma unroll
                for (int jj = 0; jj < TJ; ++jj)
                    acc[i][jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, gf[ks & 1][i]),
                                                                         __builtin_bit_cast(bf16x8, xf[ks & 1][jj]), acc[i][jj], 0, 0, 0);
            if (do_bias) {
#pragma unroll
                for (int i = 0; i < TI; ++i)
                    accb[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, gf[ks & 1][i]), __builtin_bit_cast(bf16x8, ones), accb[i], 0, 0, 0);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    int cur = 0;
    int tile = xcd_remap((int)blockIdx.x, (int)gridDim.x);
    if constexpr (RING == 3) {
        // transfers per wave and stage: NTR_G for the G tile + the halo slots this wave owns (wave w: slots w, w + NW, ... < NSLOT_H)
        constexpr int HREM = NSLOT_H % NW, NH_LO = NSLOT_H / NW;            // waves < HREM issue NH_LO + 1 halo transfers, the others NH_LO
        const bool more_h = HREM != 0 && wid < HREM;                        // wave-uniform
        const int stride = (int)gridDim.x;
        if (tile < ntiles) issue(0, tile);
        if (tile + stride < ntiles) issue(1, tile + stride);
        int fill = 2;                                                       // slot the next issue goes to
        for (; tile < ntiles; tile += stride) {
            // stage `cur` (this tile) must have landed; the stage of tile + stride, if it exists, stays in flight
            if (tile + stride < ntiles) {
                if (more_h) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NTR_G + NH_LO + 1) : "memory");
                else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NTR_G + NH_LO) : "memory");
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            __builtin_amdgcn_s_barrier();                                   // stage(cur) complete; everyone finished reading the slot consumed last (= fill)
            asm volatile("" ::: "memory");
            if (tile + 2 * stride < ntiles) issue(fill, tile + 2 * stride);
            multiply(cur);
            cur = cur + 1 == 3 ? 0 : cur + 1;
            fill = fill + 1 == 3 ? 0 : fill + 1;
        }
    } else {
    if (tile < ntiles) {
        issue(0, tile);
        if (U8) { u8_load(tile); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); u8h.landed(); u8h.template store<NSLOT_H>(smem_raw, u8lut, wid, lane); }
    }
    for (; tile < ntiles; tile += gridDim.x) {
        if (U8) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                                   // stage(cur) landed; everyone finished reading stage(cur^1)
        asm volatile("" ::: "memory");
        const bool have_next = tile + (int)gridDim.x < ntiles;
        if (have_next) issue(cur ^ 1, tile + gridDim.x);
        if (U8 && have_next) u8_load(tile + gridDim.x);
        multiply(cur);                                                  // (the transpose reads of k-step ks+1 are in flight while the MFMAs of k-step ks run)
        if (U8 && have_next) {                                          // requested at the top of this tile (after the next G tile's transfers)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); u8h.landed();
            u8h.template store<NSLOT_H>(smem_raw + (cur ^ 1) * STAGE, u8lut, wid, lane);
        }
        cur ^= 1;
    }
    }
    // ---- this workgroup's partial slab: [BN][NCT * 16] fp32 ------------------------------------------------------------------
    float* dst = p.partial + (int64_t)blockIdx.x * p.cout_pad * p.kcols_pad;
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int jj = 0; jj < TJ; ++jj) {
            const int j = wid + NW * jj;
            if (j < NCT) {
                const int co = i * 16 + g4 * 4, kc = j * 16 + i16;
#pragma unroll
                for (int e = 0; e < 4; ++e) dst[(int64_t)(co + e) * p.kcols_pad + kc] = acc[i][jj][e];
            }
        }
    if (do_bias && i16 == 0) {
#pragma unroll
        for (int i = 0; i < TI; ++i) {
            const int co = i * 16 + g4 * 4;
#pragma unroll
            for (int e = 0; e < 4; ++e) if (co + e < p.Cout) atomicAdd(p.dbias + co + e, accb[i][e]);
        }
    }
#endif
}

// tail kernel for channel counts that are not multiples of 8 (conv1: cin = 3): the round-1 32-pixel kernel
__global__ __launch_bounds__(NTHREADS, 2) void conv_wgrad_bf16_tail_kernel(WgradK p) {
    constexpr int PK = 32;
    constexpr int RSB = WG_TILE * 2 + 32;          // row stride in bytes (288)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr int OPB = PK * RSB;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid >> 1, wn = wid & 1;
    int bid, slice_;
    xcd_block(bid, slice_);
    const int k_tile = bid % p.n_k_tiles;
    const int co_tile = bid / p.n_k_tiles;
    const int slice = slice_;
    const int m_begin = slice * p.m_per_slice;
    int m_end = m_begin + p.m_per_slice;
    if (m_end > p.M) m_end = p.M;
    const int cc = tid & 15, rr = tid >> 4;
    const int kcol = k_tile * WG_TILE + cc * 8;
    const bool kok = kcol < p.kcols;
    const int tap = kok ? kcol / p.cin_pad : 0;
    const int ci = kcol - tap * p.cin_pad;
    const int r = tap / p.kw, s = tap - r * p.kw;
    const bool ci_ok = kok && ci < p.Cin;
    const int gco = co_tile * WG_TILE + cc * 8;
    const bf16_t* __restrict__ inp = reinterpret_cast<const bf16_t*>(p.in);
    const bf16_t* __restrict__ gp = reinterpret_cast<const bf16_t*>(p.g);
    int pn[2], py[2], px[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        int m = m_begin + rr + 16 * i;
        int n = m / (p.OH * p.OW);
        int rem = m - n * (p.OH * p.OW);
        pn[i] = n; py[i] = rem / p.OW; px[i] = rem - py[i] * p.OW;
    }
    u32x4 xa[2], ga[2];
    auto load_global = [&](int m0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            int m = m0 + rr + 16 * i;
            u32x4 xv = {0u, 0u, 0u, 0u}, gv = {0u, 0u, 0u, 0u};
            if (m < m_end) {
                int iy = py[i] * p.sh - p.ph + r * p.dh, ix = px[i] * p.sw - p.pw + s * p.dw;
                if (ci_ok && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W) {
                    const bf16_t* src = inp + (int64_t)((pn[i] * p.H + iy) * p.W + ix) * p.ldi + p.cioff + ci;
                    if (ci + 7 < p.Cin) xv = *reinterpret_cast<const u32x4*>(src);
                    else {
                        bf16_t tmp[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                        for (int e = 0; e < 8 && ci + e < p.Cin; ++e) tmp[e] = src[e];
                        xv = *reinterpret_cast<u32x4*>(tmp);
                    }
                }
                if (gco < p.Cout) {
                    const bf16_t* src = gp + (int64_t)m * p.ldo + p.cooff + gco;
                    if (gco + 7 < p.Cout) gv = *reinterpret_cast<const u32x4*>(src);
                    else {
                        bf16_t tmp[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                        for (int e = 0; e < 8 && gco + e < p.Cout; ++e) tmp[e] = src[e];
                        gv = *reinterpret_cast<u32x4*>(tmp);
                    }
                }
            }
            xa[i] = xv; ga[i] = gv;
            px[i] += PK;
            while (px[i] >= p.OW) { px[i] -= p.OW; if (++py[i] == p.OH) { py[i] = 0; ++pn[i]; } }
        }
    };
    auto store_lds = [&](int buf) {
        unsigned char* G = smem_raw + buf * 2 * OPB;
        unsigned char* X = G + OPB;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            *reinterpret_cast<u32x4*>(G + (rr + 16 * i) * RSB + cc * 16) = ga[i];
            *reinterpret_cast<u32x4*>(X + (rr + 16 * i) * RSB + cc * 16) = xa[i];
        }
    };
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int li = lane & 15, lg = lane >> 4;
    const uint32_t lds_base = (uint32_t)(uintptr_t)smem_raw;
    const uint32_t piece = (uint32_t)((4 * lg + (li >> 2)) * RSB + (li & 3) * 8);
    if (m_begin < m_end) {
        load_global(m_begin);
        store_lds(0);
        __syncthreads();
        int it = 0;
        for (int m0 = m_begin; m0 < m_end; m0 += PK, ++it) {
            const int cur = it & 1;
            const bool more = m0 + PK < m_end;
            if (more) load_global(m0 + PK);
            const uint32_t Gb = lds_base + cur * 2 * OPB + piece;
            const uint32_t Xb = Gb + OPB;
            u32x4 gf[4], xf[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                uint32_t a = Gb + (wm * 64 + i * 16) * 2;
                u32x2 lo = lds_tr_read(a), hi = lds_tr_read(a + 16 * RSB);
                gf[i] = u32x4{lo[0], lo[1], hi[0], hi[1]};
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint32_t a = Xb + (wn * 64 + j * 16) * 2;
                u32x2 lo = lds_tr_read(a), hi = lds_tr_read(a + 16 * RSB);
                xf[j] = u32x4{lo[0], lo[1], hi[0], hi[1]};
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, gf[i]),
                                                                        __builtin_bit_cast(bf16x8, xf[j]), acc[i][j], 0, 0, 0);
            if (more) store_lds(cur ^ 1);
            __syncthreads();
        }
    }
    float* dst = p.partial + (int64_t)slice * p.cout_pad * p.kcols_pad;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int co = co_tile * WG_TILE + wm * 64 + i * 16 + (lane >> 4) * 4;
            int kc = k_tile * WG_TILE + wn * 64 + j * 16 + (lane & 15);
#pragma unroll
            for (int e = 0; e < 4; ++e) dst[(int64_t)(co + e) * p.kcols_pad + kc] = acc[i][j][e];
        }
}

// reduce the slices, un-permute to the reference layout [cout][cin][kh][kw], apply scale, optional <w, dw_raw>
__device__ __forceinline__ void wgrad_reduce_body(const float* __restrict__ partial, float* __restrict__ dw,
                                                  const float* __restrict__ scale, const float* __restrict__ w,
                                                  float* __restrict__ wdot, int cout, int cin, int kh, int kw, int cin_pad,
                                                  int cout_pad, int kcols_pad, int slices, int accumulate, const int co, const int kchunk) {
    // (co, 256-column chunk) per workgroup, block (64 lanes x 4 columns, SG slice groups): every wave reads 1 KiB contiguous of one slice per
    // step as float4 (partials keep their own column order; cin_pad % 4 == 0, so a float4 never straddles a tap), the SG partial sums
    // meet in LDS in a fixed order (deterministic result).  50 MB of partials per layer: 16-byte lanes run this 14 -> ~8 us.
    __shared__ f32x4 red[16][64];
    const int taps = kh * kw;
    const int per = cin * taps;
    const int kc = (kchunk * 64 + threadIdx.x) * 4;
    const int sg = threadIdx.y, nsg = blockDim.y;
    const bool col_ok = kc < taps * cin_pad;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (col_ok) {
        const f32x4* __restrict__ pp = reinterpret_cast<const f32x4*>(partial + (int64_t)co * kcols_pad + kc);
        const int64_t sstride = (int64_t)cout_pad * kcols_pad / 4;
        f32x4 v0 = v, v1 = v, v2 = v, v3 = v;
        int s = sg;
        for (; s + 3 * nsg < slices; s += 4 * nsg) {
            v0 += pp[(int64_t)s * sstride];
            v1 += pp[(int64_t)(s + nsg) * sstride];
            v2 += pp[(int64_t)(s + 2 * nsg) * sstride];
            v3 += pp[(int64_t)(s + 3 * nsg) * sstride];
        }
        for (; s < slices; s += nsg) v0 += pp[(int64_t)s * sstride];
        v = (v0 + v1) + (v2 + v3);
    }
    red[sg][threadIdx.x] = v;
    __syncthreads();
    if (sg != 0) return;
    for (int g = 1; g < nsg; ++g) v += red[g][threadIdx.x];
    float dot = 0.f;
    if (col_ok) {
        const int t = kc / cin_pad, ci0 = kc - t * cin_pad;    // t = r*kw + s
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int ci = ci0 + e;
            if (ci < cin) {
                const int64_t o = (int64_t)co * per + (int64_t)ci * taps + t;
                float x = v[e];
                if (wdot) dot += x * w[o];
                if (scale) x *= scale[co];
                dw[o] = accumulate ? dw[o] + x : x;
            }
        }
    }
    if (wdot) {
        dot = wave_sum(dot);
        if (threadIdx.x == 0) atomicAdd(wdot + co, dot);
    }
}

__global__ void conv_wgrad_reduce_kernel(const float* __restrict__ partial, float* __restrict__ dw,
                                         const float* __restrict__ scale, const float* __restrict__ w,
                                         float* __restrict__ wdot, int cout, int cin, int kh, int kw, int cin_pad,
                                         int cout_pad, int kcols_pad, int slices, int accumulate) {
    wgrad_reduce_body(partial, dw, scale, w, wdot, cout, cin, kh, kw, cin_pad, cout_pad, kcols_pad, slices, accumulate, (int)blockIdx.x, (int)blockIdx.y);
}

// the slice reduces of all layers of a grouped weight-gradient launch (din_conv_wgrad_group) as ONE launch: block l of item g
// (first[g] <= l < first[g + 1]) is (filter l' / kchunks, 256-column chunk l' % kchunks) of that layer
struct WgradReduceItem { const float* partial; float* dw; const float* scale; const float* w; float* wdot;
                         int cout, cin, kh, kw, cin_pad, cout_pad, kcols_pad, slices, accumulate, kchunks; };
struct WgradReduceGroupK { WgradReduceItem it[din_wgrad::WGRAD_GROUP_MAX]; int first[din_wgrad::WGRAD_GROUP_MAX + 1]; int n; };
__global__ void conv_wgrad_reduce_group_kernel(WgradReduceGroupK grp) {
    const int l = (int)blockIdx.x;
    int gi = 0;
#pragma unroll
    for (int i = 1; i < din_wgrad::WGRAD_GROUP_MAX; ++i) gi += (i < grp.n && l >= grp.first[i]) ? 1 : 0;
    const WgradReduceItem it = grp.it[gi];
    const int local = l - grp.first[gi], co = local / it.kchunks;
    wgrad_reduce_body(it.partial, it.dw, it.scale, it.w, it.wdot, it.cout, it.cin, it.kh, it.kw, it.cin_pad, it.cout_pad, it.kcols_pad, it.slices,
                      it.accumulate, co, local - co * it.kchunks);
}

// column sums of G [M][cout] (pixel stride ld, offset coff) -> dbias[cout] (atomic accumulate; caller zeroes)
template <typename T>
__global__ void colsum_kernel(const T* __restrict__ g, float* __restrict__ out, int64_t M, int cout, int ld, int coff,
                              int64_t rows_per_block) {
    // block handles rows [b*rpb, (b+1)*rpb); thread t handles columns t, t+256, ...
    int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    int64_t r1 = r0 + rows_per_block;
    if (r1 > M) r1 = M;
    for (int c = threadIdx.x; c < cout; c += blockDim.x) {
        float s = 0.f;
        for (int64_t r = r0; r < r1; ++r) s += Elem<T>::ld(g + r * ld + coff + c);
        atomicAdd(out + c, s);
    }
}

// vectorised form: thread = (row lane r, 16-byte channel chunk c); four rows in flight per thread, LDS cross-row reduce, one atomic
// per column per block
template <typename T, int U = 4>
__global__ __launch_bounds__(256) void colsum_vec_kernel(const T* __restrict__ g, float* __restrict__ out, int64_t M, int cout, int ld,
                                                         int coff, int64_t rows_per_block) {
    constexpr int EPC = 16 / sizeof(T);
    __shared__ float red[256][EPC + 1];
    const int ncg = cout / EPC;                      // <= 256
    const int rows_pp = 256 / ncg;
    const int r = threadIdx.x / ncg, c = threadIdx.x - r * ncg;
    int64_t r0 = (int64_t)xcd_remap((int)blockIdx.x, (int)gridDim.x) * rows_per_block, r1 = r0 + rows_per_block;
    if (r1 > M) r1 = M;
    float acc[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) acc[e] = 0.f;
    auto add = [&](const u32x4& v) {
        if constexpr (sizeof(T) == 4) {
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] += __uint_as_float(v[e]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) { acc[2 * e] += __uint_as_float(v[e] << 16); acc[2 * e + 1] += __uint_as_float(v[e] & 0xffff0000u); }
        }
    };
    if (r < rows_pp) {
        const T* base = g + coff + c * EPC;
        int64_t row = r0 + r;
        for (; row + (U - 1) * rows_pp < r1; row += U * rows_pp) {         // U independent 16-byte loads in flight per thread
            u32x4 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = *reinterpret_cast<const u32x4*>(base + (row + u * rows_pp) * ld);
#pragma unroll
            for (int u = 0; u < U; ++u) add(v[u]);
        }
        for (; row < r1; row += rows_pp) add(*reinterpret_cast<const u32x4*>(base + row * ld));
    }
#pragma unroll
    for (int e = 0; e < EPC; ++e) red[threadIdx.x][e] = acc[e];
    __syncthreads();
    for (int idx = threadIdx.x; idx < ncg * EPC; idx += 256) {
        const int cc = idx / EPC, e = idx - cc * EPC;
        float t = 0.f;
        for (int k = 0; k < rows_pp; ++k) t += red[k * ncg + cc][e];
        atomicAdd(out + idx, t);
    }
}

// DIN_DETERMINISTIC: the column sums in a fixed order, no atomics (the structure of layernorm_param_grad_ordered_kernel).  One workgroup per
// 16-column chunk, 64 row groups: group g sums rows g, g + 64, ... in ascending order, the partial sums meet in an LDS tree of fixed shape,
// one thread per column writes out[c] (add: adds into it once -- the accumulate-bit-1 contract of din_conv_wgrad).
constexpr int COLSUM_ORD_COLS = 16, COLSUM_ORD_GROUPS = 64;
template <typename T>
__global__ __launch_bounds__(COLSUM_ORD_COLS * COLSUM_ORD_GROUPS) void colsum_ordered_kernel(const T* __restrict__ g, float* __restrict__ out, int64_t M,
                                                                                             int cout, int ld, int coff, int add) {
    __shared__ float part[COLSUM_ORD_GROUPS][COLSUM_ORD_COLS + 1];
    const int cl = threadIdx.x % COLSUM_ORD_COLS, rg = threadIdx.x / COLSUM_ORD_COLS;
    const int c = (int)blockIdx.x * COLSUM_ORD_COLS + cl;
    float s = 0.f;
    if (c < cout)
        for (int64_t r = rg; r < M; r += COLSUM_ORD_GROUPS) s += Elem<T>::ld(g + r * ld + coff + c);
    part[rg][cl] = s;
    __syncthreads();
    for (int h = COLSUM_ORD_GROUPS / 2; h > 0; h >>= 1) {
        if (rg < h) part[rg][cl] += part[rg + h][cl];
        __syncthreads();
    }
    if (rg == 0 && c < cout) out[c] = add ? out[c] + part[0][cl] : part[0][cl];
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
constexpr int WGRAD_SMALL_GRID = 512;
constexpr int WGRAD_HALO_GRID = 128;       // persistent workgroups per filter-row class of conv_wgrad_halo_kernel (2 classes x 128 = one per CU)

// the instantiations of this file's kernel families, X(template arguments): the launch table below switches on them, and a chosen tuple that
// is not listed is an error (the pipe and halo kernels keep theirs next to their launchers)
#define DIN_WGRAD_BF16_TABLE(X) X(64) X(96) X(128) X(160)
#define DIN_WGRAD_RING_TABLE(X) X(64, 128) X(96, 128) X(128, 128) X(160, 128) X(128, 256) X(160, 256) X(192, 256)
#define DIN_WGRAD_STEM_TABLE(X) X(4, 32, 1, false, 4, 8, 2) X(4, 64, 1, false, 8, 6, 3) X(4, 64, 1, false, 8, 8, 2) X(4, 64, 1, false, 4, 8, 2) \
                                X(1, 32, 2, true, 4, 8, 2) X(1, 32, 2, false, 4, 8, 2)

// the main kernel of a choice as the demangler spells it (what rocprofv3 prints): every template argument, defaults included
std::string wgrad_kernel_name(const WgradChoice& c) {
    char s[96];
    const auto tf = [](bool b) { return b ? "true" : "false"; };
    switch (c.family) {
    case din_wgrad::WGRAD_F32: return "conv_wgrad_f32_kernel";
    case din_wgrad::WGRAD_F32X3: return "conv_wgrad_f32x3_kernel";
    case din_wgrad::WGRAD_BF16_TAIL: return "conv_wgrad_bf16_tail_kernel";
    case din_wgrad::WGRAD_BF16: snprintf(s, sizeof s, "conv_wgrad_bf16_kernel<%d>", c.bco); break;
    case din_wgrad::WGRAD_RING: snprintf(s, sizeof s, "conv_wgrad_ring_kernel<%d, %d>", c.bco, c.bk); break;
    case din_wgrad::WGRAD_PIPE: snprintf(s, sizeof s, "conv_wgrad_pipe_kernel<%d, %d, %s, %d>", c.pipe.bco, c.pipe.bk, tf(c.pipe.wide), c.pipe.wn); break;
    case din_wgrad::WGRAD_STEM:
        snprintf(s, sizeof s, "conv_wgrad_small_kernel<%d, %d, %d, %s, %d, %d, %d>", c.stem.cpp, c.stem.bn, c.stem.st, tf(c.stem.u8), c.stem.nw, c.stem.th, c.stem.ring);
        break;
    case din_wgrad::WGRAD_HALO:
        snprintf(s, sizeof s, "conv_wgrad_halo_kernel<%d, %d, %d, %d, %d>", c.halo.cpp, c.halo.bnt, c.halo.kh, c.halo.kw, c.halo.th);
        break;
    }
    return s;
}

// DIN_F32_BF16X3: the fp32 plan (grid, slices, partial layout) on the kernel that multiplies in three bf16 parts
int launch_wgrad_f32x3(const WgradK& k, const WgradChoice& c, hipStream_t st) {
    hipLaunchKernelGGL(conv_wgrad_f32x3_kernel, c.grid, c.block, 0, st, k);
    return DIN_OK;
}

// the launch table: family and tuple -> template
int launch_wgrad(const WgradK& k, const WgradChoice& c, hipStream_t st) {
    auto go = [&](auto kern) {
        if (c.lds > 65536 || c.family == din_wgrad::WGRAD_RING) raise_lds_limit(kern, c.lds);      // (the ring kernels: whatever their size)
        hipLaunchKernelGGL(kern, c.grid, c.block, c.lds, st, k);
        return DIN_OK;
    };
    switch (c.family) {
    case din_wgrad::WGRAD_F32: return go(conv_wgrad_f32_kernel);
    case din_wgrad::WGRAD_F32X3: return launch_wgrad_f32x3(k, c, st);
    case din_wgrad::WGRAD_BF16_TAIL: return go(conv_wgrad_bf16_tail_kernel);
    case din_wgrad::WGRAD_BF16:
#define DIN_ROW(BCO_) if (c.bco == BCO_) return go(conv_wgrad_bf16_kernel<BCO_>);
        DIN_WGRAD_BF16_TABLE(DIN_ROW)
#undef DIN_ROW
        break;
    case din_wgrad::WGRAD_RING:
#define DIN_ROW(BCO_, BK_) if (c.bco == BCO_ && c.bk == BK_) return go(conv_wgrad_ring_kernel<BCO_, BK_>);
        DIN_WGRAD_RING_TABLE(DIN_ROW)
#undef DIN_ROW
        break;
    case din_wgrad::WGRAD_STEM:
#define DIN_ROW(CPP_, BN_, ST_, U8_, NW_, TH_, RING_)                                                                                        \
        if (c.stem.cpp == CPP_ && c.stem.bn == BN_ && c.stem.st == ST_ && c.stem.u8 == U8_ && c.stem.nw == NW_ && c.stem.th == TH_ && c.stem.ring == RING_) \
            return go(conv_wgrad_small_kernel<CPP_, BN_, ST_, U8_, NW_, TH_, RING_>);
        DIN_WGRAD_STEM_TABLE(DIN_ROW)
#undef DIN_ROW
        break;
    case din_wgrad::WGRAD_PIPE: return din_wgrad::launch_wgrad_pipe(k, c.pipe, c.grid, c.block, c.lds, st);
    case din_wgrad::WGRAD_HALO: return din_wgrad::launch_wgrad_halo(k, c.halo, c.grid, c.block, c.lds, st);
    }
    DIN_FAIL(DIN_E_ARG, "conv_wgrad: %s is not instantiated", wgrad_kernel_name(c).c_str());
}

// the kernel argument block of a layer under its choice (both entry points; the grouped launch then sets its own pixel slicing)
void fill_wgrad_k(WgradK& k, const din_conv_desc* d, const WgradChoice& c, const void* in, const void* dout, void* partial) {
    k.in = in; k.g = dout; k.partial = reinterpret_cast<float*>(partial); k.dbias = nullptr;
    k.NB = d->nb; k.H = d->h; k.W = d->w; k.Cin = d->cin; k.ldi = d->ldi; k.cioff = d->cioff;
    k.OH = d->oh; k.OW = d->ow; k.Cout = d->cout; k.ldo = d->ldo; k.cooff = d->cooff;
    k.kh = d->kh; k.kw = d->kw; k.sh = d->sh; k.sw = d->sw; k.ph = d->ph; k.pw = d->pw; k.dh = d->dh; k.dw = d->dw;
    k.cin_pad = c.cin_pad; k.kcols = c.kcols; k.kcols_pad = c.kcols_pad; k.cout_pad = c.cout_pad;
    k.M = d->nb * d->oh * d->ow; k.n_co_tiles = c.n_co_tiles; k.n_k_tiles = c.n_k_tiles;
    k.slices = c.slices; k.m_per_slice = c.m_per_slice;
    if (c.family == din_wgrad::WGRAD_STEM && c.stem.u8) k.u8 = reinterpret_cast<const unsigned char*>(in);
}

// which column-sum kernel serves a view: 0 = colsum_kernel (any channel count), otherwise the unroll of colsum_vec_kernel
int colsum_unroll(int dtype, int c, int ld, int coff) {
    const int epc = dtype == DIN_F32 ? 4 : 8;
    if (!(c % epc == 0 && c / epc <= 256 && ld % epc == 0 && coff % epc == 0)) return 0;
    const int unr = DIN_OPT("DIN_COLSUM_UNROLL") ? atoi(DIN_OPT("DIN_COLSUM_UNROLL")) : 8;          // DIN_COLSUM_WGS / DIN_COLSUM_UNROLL: tuning aids
    return dtype == DIN_F32 ? 4 : (unr == 8 || unr == 16) ? unr : 4;
}

// column sums of a pixel-major tensor view -> out[c] (fp32 atomics across row slabs): zeroed here first, or added into when `zero` is false
int launch_colsum(int dtype, const void* g, float* out, int64_t M, int c, int ld, int coff, hipStream_t st, bool zero = true) {
    if (din_deterministic()) {                                // fixed-order form: no memset, no atomics, whatever DIN_COLSUM_* say
        const dim3 grid((c + COLSUM_ORD_COLS - 1) / COLSUM_ORD_COLS), block(COLSUM_ORD_COLS * COLSUM_ORD_GROUPS);
        if (dtype == DIN_F32) hipLaunchKernelGGL(colsum_ordered_kernel<float>, grid, block, 0, st, (const float*)g, out, M, c, ld, coff, zero ? 0 : 1);
        else hipLaunchKernelGGL(colsum_ordered_kernel<bf16_t>, grid, block, 0, st, (const bf16_t*)g, out, M, c, ld, coff, zero ? 0 : 1);
        DIN_CHECK_LAUNCH("colsum_ordered");
        return DIN_OK;
    }
    if (zero && hipMemsetAsync(out, 0, sizeof(float) * c, st) != hipSuccess) DIN_FAIL(DIN_E_LAUNCH, "colsum: memset");
    const int unr = colsum_unroll(dtype, c, ld, coff);
    if (unr) {
        // 256 workgroups (one per CU), eight 16-byte loads in flight per thread, each streaming a contiguous slab of rows (XCD-contiguous order).
        // Every workgroup ends with `c` float atomics on the SAME few cache lines, which L2 serialises at ~44 ns per workgroup: the kernel's time
        // grew with its workgroup count (1024: 45 us, 2048: 64 us, 4096: 110 us on the 192-channel maps; 256: 30 us -- tools/colsum_probe.py;
        // the seven launches of the default step 335 -> 248 us)
        const int wgs = DIN_OPT("DIN_COLSUM_WGS") ? atoi(DIN_OPT("DIN_COLSUM_WGS")) : 256;
        int64_t rpb = ceil_div64(M, wgs > 0 ? wgs : 1024);
        if (rpb < 64) rpb = 64;
        int blocks = (int)ceil_div64(M, rpb);
        if (dtype == DIN_F32)
            hipLaunchKernelGGL(colsum_vec_kernel<float>, dim3(blocks), dim3(256), 0, st, (const float*)g, out, M, c, ld, coff, rpb);
        else if (unr == 8)
            hipLaunchKernelGGL((colsum_vec_kernel<bf16_t, 8>), dim3(blocks), dim3(256), 0, st, (const bf16_t*)g, out, M, c, ld, coff, rpb);
        else if (unr == 16)
            hipLaunchKernelGGL((colsum_vec_kernel<bf16_t, 16>), dim3(blocks), dim3(256), 0, st, (const bf16_t*)g, out, M, c, ld, coff, rpb);
        else
            hipLaunchKernelGGL(colsum_vec_kernel<bf16_t>, dim3(blocks), dim3(256), 0, st, (const bf16_t*)g, out, M, c, ld, coff, rpb);
    } else {
        int64_t rpb = 512;
        int blocks = (int)ceil_div64(M, rpb);
        if (dtype == DIN_F32)
            hipLaunchKernelGGL(colsum_kernel<float>, dim3(blocks), dim3(256), 0, st, (const float*)g, out, M, c, ld, coff, rpb);
        else
            hipLaunchKernelGGL(colsum_kernel<bf16_t>, dim3(blocks), dim3(256), 0, st, (const bf16_t*)g, out, M, c, ld, coff, rpb);
    }
    DIN_CHECK_LAUNCH("colsum");
    return DIN_OK;
}

}  // namespace

namespace din_wgrad {

// The weight-gradient choice.  Every option that selects a kernel is read HERE, each once: DIN_CONV_BN (its weight-gradient use), DIN_CONV_SMALL
// (conv_small_wanted) and the DIN_WGRAD_* switches of the main launch and of the grouped launch's key.  What is left to din_conv_wgrad are the
// per-call run-time switches that choose no kernel: DIN_WGRAD_PACE, DIN_WGRAD_DIRECT (and the atomic epilogue's memset).
WgradChoice plan_wgrad(const din_conv_desc* d, bool split) {
    const int conv_bn = opt_int(DIN_OPT("DIN_CONV_BN"), 0);                  // 128: filter tiles of 128 rows only
    const bool stem_wanted = conv_small_wanted();
    const int halo_mode = opt_int(DIN_OPT("DIN_WGRAD_HALO"), 1);             // 0: off, 1: launches of >= 128K pixels (12 frames of 87x157 measured +3..34 %), 2: any size (tests)
    const int ring_mode = opt_int(DIN_OPT("DIN_WGRAD_RING"), 1);
    const int pipe_mode = opt_int(DIN_OPT("DIN_WGRAD_PIPE"), 1);             // 0: ring kernel, 1: pipe (wide choice), 3: pipe (round-1 tile choice)
    const int pipe_pad_pct = opt_int(DIN_OPT("DIN_WGRAD_PIPE_PAD"), 20);     // tuning aid, see below
    const int atomic_mode = opt_int(DIN_OPT("DIN_WGRAD_ATOMIC"), 0);
    const int blocks_wanted = opt_int(DIN_OPT("DIN_WGRAD_BLOCKS"), 0);
    const int stem_waves = opt_int(DIN_OPT("DIN_WGRAD_SMALL_WAVES"), 8);
    const int stem_ring = opt_int(DIN_OPT("DIN_WGRAD_SMALL_RING"), 3);
    const int pipe_waves = opt_int(DIN_OPT("DIN_WGRAD_PIPE_WAVES"), 16);
    const bool group_wanted = opt_int(DIN_OPT("DIN_WGRAD_GROUP"), 1) != 0;

    WgradChoice w{};
    int epc = epc_of(d->dtype);
    // bf16 v2 kernel needs whole 16-byte channel chunks on both operands; otherwise the tail kernel (conv1: cin = 3)
    bool v2 = d->dtype == DIN_BF16 && d->cin % 8 == 0 && d->cout % 8 == 0 && d->ldi % 8 == 0 && d->cioff % 8 == 0;
    w.bco = 128;
    if (v2) {
        // filter-tile width in {64,96,128,160}: least padding, ties to the wider tile (192 -> 2 x 96, 288 -> 3 x 96, 384 -> 3 x 128)
        if (d->cout <= 64) w.bco = 64;
        else if (conv_bn != 128) {
            // fewest filter tiles first; on a tie keep 128 when cout > 128 (measured: 192 as 2 x 96 is slower than 2 x 128),
            // otherwise the least padded width
            int best = 128, best_tiles = (d->cout + 127) / 128, best_pad = best_tiles * 128;
            const int cands[2] = {96, 160};
            for (int ci = 0; ci < 2; ++ci) {
                int bc = cands[ci], tl = (d->cout + bc - 1) / bc, pad = tl * bc;
                if (tl < best_tiles || (tl == best_tiles && d->cout <= 128 && pad < best_pad)) { best = bc; best_tiles = tl; best_pad = pad; }
            }
            w.bco = best;
        }
    }
    // stem layers (conv_wgrad_small_kernel): small = 1: 32 -> <=32, 2: 32 -> <=64 (stride 1), 3: image layer (<= 8 channels, stride 2)
    int small = 0;
    {
        const int64_t M = (int64_t)d->nb * d->oh * d->ow;
        const bool common = stem_wanted && d->dtype == DIN_BF16 && d->kh == 3 && d->kw == 3 && d->dh == 1 && d->dw == 1 && d->cout % 8 == 0 &&
                            d->ldi % 8 == 0 && d->cioff % 8 == 0 && d->ldo % 8 == 0 && d->cooff % 8 == 0 && M >= 256 * 1024 &&
                            (long long)d->h * d->w * d->ldi * 2 < 0x7fffffffll && (long long)d->oh * d->ow * d->ldo * 2 < 0x7fffffffll;
        if (common && d->sh == 1 && d->sw == 1 && d->cin == 32 && d->cout <= 64) small = d->cout <= 32 ? 1 : 2;
        else if (common && d->sh == 2 && d->sw == 2 && d->cin <= 8 && d->ldi >= d->cioff + 8 && d->cout <= 32) small = 3;
    }
    // narrow mid-network layers (conv_wgrad_halo.hip): dW stationary in registers, halo tiles, two filter-row classes
    if (!small) {
        const int64_t M = (int64_t)d->nb * d->oh * d->ow;
        HaloInst hi{};
        if (halo_mode && d->dtype == DIN_BF16 && d->sh == 1 && d->sw == 1 && d->dh == 1 && d->dw == 1 &&
            wgrad_halo_shape(d->cin, d->cout, d->kh, d->kw, &hi) && d->ldi % 8 == 0 && d->cioff % 8 == 0 && d->ldo % 8 == 0 &&
            d->cooff % 8 == 0 && (M >= 128 * 1024 || halo_mode == 2) && d->ow >= 32 && (long long)d->h * d->w * d->ldi * 2 < 0x7fffffffll &&
            (long long)d->oh * d->ow * d->ldo * 2 < 0x7fffffffll) {
            w.family = WGRAD_HALO; w.halo = hi; w.bco = hi.bnt; w.bk = 0;
            w.cin_pad = d->cin;
            w.kcols = w.kcols_pad = d->kh * d->kw * d->cin;
            w.cout_pad = d->cout; w.n_co_tiles = 2; w.n_k_tiles = 1;
            w.slices = WGRAD_HALO_GRID; w.m_per_slice = 0;
            w.ws_bytes = (int64_t)w.slices * w.cout_pad * w.kcols_pad * 4;
            w.grid = dim3(WGRAD_HALO_GRID, 2); w.block = dim3(1024); w.lds = wgrad_halo_lds_bytes(hi);
            w.bias_fused = true;
            return w;
        }
    }
    if (small) {
        w.family = WGRAD_STEM; w.bco = small == 2 ? 64 : 32; w.bk = 0;
        w.cin_pad = pad_to(d->cin, 8);
        w.kcols = 9 * w.cin_pad;
        w.kcols_pad = (small == 3 ? 5 : 18) * 16;
        w.cout_pad = w.bco; w.n_co_tiles = 1; w.n_k_tiles = 1;
        w.slices = WGRAD_SMALL_GRID; w.m_per_slice = 0;
        w.ws_bytes = (int64_t)w.slices * w.cout_pad * w.kcols_pad * 4;
        const int st_ = small == 3 ? 2 : 1, cpp = small == 3 ? 1 : 4;
        const int hbytes = ((7 * st_ + 3) * (31 * st_ + 3) * cpp * 16 + 1023) / 1024 * 1024;
        w.stem = StemInst{cpp, w.bco, st_, false, 4, 8, 2};
        w.lds = 2 * ((size_t)hbytes + 256 * (size_t)w.bco * 2) + (d->in_u8 ? 512 : 0);
        w.block = dim3(NTHREADS);
        if (small == 2 && stem_waves != 4) {                        // eight waves; DIN_WGRAD_SMALL_WAVES=4: the four-wave form
            w.block = dim3(512);
            w.stem.nw = 8;
            if (stem_ring == 3) {                                   // 6 x 32 tiles, three-slot ring, two stages in flight (126 KB)
                const size_t hb6 = ((size_t)(5 + 3) * (31 + 3) * 4 * 16 + 1023) / 1024 * 1024;
                w.lds = 3 * (hb6 + 192 * (size_t)w.bco * 2);
                w.stem.th = 6; w.stem.ring = 3;
            }
        } else if (small == 3 && d->in_u8) w.stem.u8 = true;        // the image layer from raw uint8 frames
        w.grid = dim3(WGRAD_SMALL_GRID);
        w.bias_fused = true;
        return w;
    }
    w.cin_pad = pad_to(d->cin, epc);
    w.kcols = d->kh * d->kw * w.cin_pad;
    // ring kernel (BCO x 256 tiles, one workgroup per CU): wide filter banks with enough k columns -- fewest filter tiles, then least padding
    int ring = 0;
    if (v2 && ring_mode && d->cout >= (ring_mode == 2 ? 64 : 112) && w.kcols >= 256) {
        ring = 1;
        int best = 128, best_tiles = (d->cout + 127) / 128, best_pad = best_tiles * 128;
        const int cands[2] = {160, 192};
        for (int ci = 0; ci < 2; ++ci) {
            int bc = cands[ci], tl = (d->cout + bc - 1) / bc, pad = tl * bc;
            if (tl < best_tiles || (tl == best_tiles && pad < best_pad)) { best = bc; best_tiles = tl; best_pad = pad; }
        }
        // measured (profiles/r01_wgrad_ring.txt): the ring wins where the 128-row tiles pad badly (cout 192 -> 2 x 128 wastes a
        // quarter of the MFMAs); at equal tile height the two-workgroups-per-CU v3 kernel is faster
        // (8-wave ring: +25..40 % on 192-row banks, +5..11 % on exact 128 / 256-row banks, behind v3 when rows or k columns pad)
        const int kpad = pad_to(w.kcols, 256);
        if (pipe_mode == 1) {
            // wide banks run the pipelined kernel with rows padded to the next of {128, 192, 256} whatever their k-column padding:
            // measured against the round-1 choice below (DIN_WGRAD_PIPE=3; profiles/r02_wgrad_ring_vs_pipe_vs_atomic.txt) it is
            // 11-17 % faster on the 112 / 128 / 256-row banks the k-padding rule used to send to the two-workgroup kernels
            int pb = 128, pt = (d->cout + 127) / 128, pp = pt * 128;
            const int pc[2] = {192, 256};
            for (int ci = 0; ci < 2; ++ci) {
                int bc = pc[ci], tl = (d->cout + bc - 1) / bc, pad = tl * bc;
                if (tl < pt || (tl == pt && pad < pp)) { pb = bc; pt = tl; pp = pad; }
            }
            // (row padding above 15 % -- the 160-row banks as 192 -- measured +5 % only: those stay on the round-1 choice below)
            // allowed row padding in percent: 20 admits the 160-row banks of Mixed_6c / 6d (160 -> 192 rows: 168 -> 155 us per launch
            // against conv_wgrad_bf16_kernel<160>, steady-state clocks; profiles/r03_power_clocks.txt).  DIN_WGRAD_PIPE_PAD: tuning aid
            if (pp * 100 <= d->cout * (100 + pipe_pad_pct)) w.bco = pb;
            else if (best_pad * 100 <= d->cout * 105 && (best == 192 || kpad * 100 <= w.kcols * 112)) w.bco = best;
            else ring = 0;
        } else if ((best_pad * 100 <= d->cout * 105 && (best == 192 || kpad * 100 <= w.kcols * 112)) || ring_mode == 2) w.bco = best;
        else ring = 0;
    }
    int ring_bk = 256;
    // 64 / 96-row banks: the 8-wave ring with 128 k columns (two workgroups per CU) beats v3 by ~20 %; 128 rows: equal, 160: behind
    if (!ring && v2 && ring_mode != 0 && (ring_mode == 3 || w.bco == 64 || w.bco == 96)) { ring = 1; ring_bk = 128; }
    const int bk = ring ? ring_bk : WG_TILE;
    // BCO x 256 ring tiles whose wave tile is whole 32x32 MFMA tiles run the software-pipelined kernel (conv_wgrad_pipe.hip)
    const bool pipe = ring && ring_bk == 256 && (w.bco == 128 || w.bco == 192 || w.bco == 256) && pipe_mode;
    if (pipe) w.atomic = atomic_mode;
    int pk = d->dtype == DIN_F32 ? 16 : (ring ? 32 : (v2 ? 64 : 32));
    w.bk = bk;
    w.kcols_pad = pad_to(w.kcols, bk);
    w.n_co_tiles = (d->cout + w.bco - 1) / w.bco;
    w.cout_pad = pad_to(w.n_co_tiles * w.bco, WG_TILE);            // partial-sum rows cover every filter tile
    w.n_k_tiles = w.kcols_pad / bk;
    int M = d->nb * d->oh * d->ow;
    int tiles = w.n_co_tiles * w.n_k_tiles;
    // v2/v3 kernels: ~4 workgroups per CU; short reductions (small per-GPU batch) take 2 -- every workgroup writes a full partial tile, so
    // halving them halves the partial traffic (4-clip step 12.47 -> 12.14 ms).  The ring kernel sets its own count below.
    const int want_total = blocks_wanted > 0 ? blocks_wanted : (M < 128 * 1024 ? 512 : 1024);
    int want = (want_total + tiles - 1) / tiles;
    if (ring) {                                        // one resident workgroup per CU: a single full round (or two for long slices)
        const int rounds = (int64_t)M * tiles >= (int64_t)256 * 64 * 1024 ? 2 : 1;
        want = 256 * rounds * (ring_bk == 128 ? 2 : 1) / tiles;
        if (want < 1) want = 1;
    }
    int64_t max_by_ws = ((int64_t)1 << 30) / ((int64_t)w.cout_pad * w.kcols_pad * 4);   // keep workspace <= 1 GiB
    if (max_by_ws < 1) max_by_ws = 1;
    if (want > max_by_ws) want = (int)max_by_ws;
    int mps = (M + want - 1) / want;
    mps = pad_to(mps < pk ? pk : mps, pk);
    w.m_per_slice = mps;
    w.slices = (M + mps - 1) / mps;
    w.ws_bytes = (int64_t)w.slices * w.cout_pad * w.kcols_pad * 4;
    if (pipe) w.ws_bytes += (int64_t)w.slices * w.n_co_tiles * 8 * 4 + 64;      // pacing words
    w.grid = dim3(w.n_co_tiles * w.n_k_tiles, w.slices);
    w.block = dim3(NTHREADS);
    if (d->dtype == DIN_F32) {
        w.family = split ? WGRAD_F32X3 : WGRAD_F32;      // (split: d is the DIN_F32 form of a DIN_F32_BF16X3 descriptor -- SplitDesc)
    } else if (pipe) {
        // wave grid 2 x WN: sixteen waves by default, DIN_WGRAD_PIPE_WAVES=8: 2 x 4, =4: 2 x 2 (not for the 256-row tile, which would spill)
        w.family = WGRAD_PIPE;
        w.pipe = PipeInst{w.bco, w.bk, d->ow >= 32, pipe_waves == 16 ? 8 : (pipe_waves == 4 && w.bco <= 192) ? 2 : 4};
        w.block = dim3(128 * w.pipe.wn);
        w.lds = wgrad_pipe_lds_bytes(w.bco, w.bk);
        // the grouped launch (din_conv_wgrad_group) is instantiated for the sixteen-wave grid and serves plans with slices to reduce
        // (one slice: nothing to reduce, the single launch writes dW directly)
        if (group_wanted && w.pipe.wn == 8 && !w.atomic && w.slices >= 2 && !d->in_u8 && d->ldo % 8 == 0 && d->cooff % 8 == 0)
            w.group_key = w.bco * 2 + (w.pipe.wide ? 1 : 0);
    } else if (ring) {
        w.family = WGRAD_RING;
        w.block = dim3(512);
        w.lds = 4 * ((size_t)((32 * w.bco / 8 + 511) / 512) * 8192 + 32 * (size_t)w.bk * 2);      // four 32-pixel stages (G tile in 8-KiB rounds)
    } else if (v2) {
        w.family = WGRAD_BF16;
        w.lds = 2 * 64 * ((size_t)(w.bco * 2) + (WG_TILE * 2));                                   // two unpadded stages
    } else {
        w.family = WGRAD_BF16_TAIL;
        w.lds = 2 * 2 * 32 * (WG_TILE * 2 + 32);
    }
    w.bias_fused = w.family != WGRAD_F32 && w.family != WGRAD_F32X3 && w.family != WGRAD_BF16_TAIL;
    return w;
}

// the codes of din_conv_kernel_tile(d, 2), from the choice
void wgrad_tile_code(const WgradChoice& c, int32_t* bm, int32_t* bn) {
    switch (c.family) {
    case WGRAD_HALO: *bm = 3; *bn = c.bco; break;
    case WGRAD_STEM: *bm = 0; *bn = c.bco; break;
    case WGRAD_PIPE: *bm = c.bco; *bn = 2000 + c.bk; break;
    case WGRAD_RING: *bm = c.bco; *bn = 1000 + c.bk; break;
    default: *bm = c.bco; *bn = WG_TILE; break;
    }
}

// the launches of a production-style din_conv_wgrad call (dbias, scale, w and wdot given), in launch order
void append_wgrad_names(const din_conv_desc* d, const WgradChoice& c, std::string& out) {
    out += wgrad_kernel_name(c); out += '\n';
    out += "conv_wgrad_reduce_kernel\n";
    if (!c.bias_fused) {
        const int unr = colsum_unroll(d->dtype, d->cout, d->ldo, d->cooff);
        const char* T = d->dtype == DIN_F32 ? "float" : "unsigned short";
        char s[64];
        if (unr) snprintf(s, sizeof s, "colsum_vec_kernel<%s, %d>\n", T, unr); else snprintf(s, sizeof s, "colsum_kernel<%s>\n", T);
        out += s;
    }
}

}  // namespace din_wgrad

extern "C" {

int din_conv_wgrad(const din_conv_desc* d, const void* in, const void* dout, float* dw, float* dbias, const float* scale,
                   const float* w, float* wdot, int accumulate, void* workspace, int64_t workspace_bytes, void* stream) {
    const SplitDesc sd(d);
    if (int e = check_desc(d)) return e;
    DIN_REQUIRE(in && dout && dw, "conv_wgrad: null pointer");
    DIN_REQUIRE(!wdot || w, "conv_wgrad: wdot needs w");
    DIN_REQUIRE(!d->in_u8 || din_conv_accepts_u8(d), "conv_wgrad: in_u8 on a layer din_conv_accepts_u8() rejects");
    hipStream_t st = as_stream(stream);
    const bool prezeroed = (accumulate & 2) != 0;            // dbias / wdot were zeroed by the caller (one memset for a whole backbone)
    accumulate &= 1;
    const WgradChoice c = din_wgrad::plan_wgrad(d, sd.split);
    // DIN_DETERMINISTIC: dW is slice partials + a fixed-order reduce already; dbias leaves the main kernel's atomic epilogue for the ordered
    // column sum below; <w, dW> and the atomic split-K epilogue have no ordered form: refused, never run
    const bool ordered = din_deterministic();
    DIN_REQUIRE(!ordered || !wdot, "conv_wgrad: DIN_DETERMINISTIC: wdot (the BatchNorm-eval scale gradient) is summed with atomics; train_backbone is not covered");
    DIN_REQUIRE(!ordered || !c.atomic, "conv_wgrad: DIN_DETERMINISTIC: DIN_WGRAD_ATOMIC selects an atomic split-K epilogue");
    if (workspace_bytes < c.ws_bytes || !workspace)
        DIN_FAIL(DIN_E_WORKSPACE, "conv_wgrad: workspace %lld < %lld bytes", (long long)workspace_bytes, (long long)c.ws_bytes);
    DIN_REQUIRE(d->dtype == DIN_F32 || (d->ldo % 8 == 0 && d->cooff % 8 == 0), "conv_wgrad: bf16 dout stride/offset must be multiples of 8");
    WgradK k{};
    fill_wgrad_k(k, d, c, in, dout, workspace);
#ifdef DIN_EXPERIMENTS
    { const char* pv = DIN_OPT("DIN_WGRAD_PROBE"); k.probe = pv ? atoi(pv) : 0; }      // timing probe: results are WRONG when set
#else
    k.probe = 0;
#endif
    if (dbias && c.bias_fused && !ordered) {
        if (!prezeroed && hipMemsetAsync(dbias, 0, sizeof(float) * d->cout, st) != hipSuccess) DIN_FAIL(DIN_E_LAUNCH, "conv_wgrad: memset");
        k.dbias = dbias;
    }
    if (c.family == din_wgrad::WGRAD_PIPE) {
        k.atomic = c.atomic;
        if (c.atomic && hipMemsetAsync(k.partial, 0, sizeof(float) * (size_t)c.cout_pad * c.kcols_pad, st) != hipSuccess)
            DIN_FAIL(DIN_E_LAUNCH, "conv_wgrad: memset");
        {   // sibling pacing words behind the partial tiles (workspace sized for them in plan_wgrad): rows of 8 words (one s_load_dwordx8)
            const char* pe = DIN_OPT("DIN_WGRAD_PACE");
            const int want = pe ? atoi(pe) : 1;
            // measured (tools/pace_experiment.sh, profiles/r02_wgrad_pacing.txt): Conv2d_4a (3 k tiles) 6.67 -> 3.12 GB fetched per launch at
            // unchanged time; with 6+ siblings the naps cost 4-10 % and the L2 hit rate was 74 % anyway -> default: up to 3 siblings
            if (want && c.n_k_tiles >= 2 && c.n_k_tiles <= (want >= 2 ? 8 : 3) && !c.atomic && c.m_per_slice / 32 < (1 << 20) - 1) {
                k.pace = reinterpret_cast<int*>(reinterpret_cast<char*>(workspace) + (((size_t)c.slices * c.cout_pad * c.kcols_pad * 4 + 31) & ~(size_t)31));
                // no memset: every launch tags its words (1..1023 << 20, never 0); words of older launches or stale workspace contents
                // are out of range for this tag (an alias once in 1023 launches costs one bounded spin, never correctness)
                static std::atomic<unsigned> pace_epoch{0};
                k.pace_base = (int)(((pace_epoch.fetch_add(1) % 1023u) + 1u) << 20);
            }
        }
        // one slice of a 1x1 layer, nothing for the reduce launch to do (no scale, no <w, dW>, no accumulate, no channel padding): straight into dW
        if (c.slices == 1 && !c.atomic && d->kh * d->kw == 1 && !scale && !wdot && !accumulate && c.cin_pad == d->cin &&
            opt_int(DIN_OPT("DIN_WGRAD_DIRECT"), 1) != 0) k.direct = dw;
    }
    if (int e = launch_wgrad(k, c, st)) return e;
    DIN_CHECK_LAUNCH("conv_wgrad");
    if (wdot && !prezeroed && hipMemsetAsync(wdot, 0, sizeof(float) * d->cout, st) != hipSuccess) DIN_FAIL(DIN_E_LAUNCH, "conv_wgrad: memset");
    if (k.direct == nullptr) {
        int kc_total = d->kh * d->kw * c.cin_pad;
        dim3 rgrid(d->cout, (kc_total + 255) / 256);
        const int rslices = (c.family == din_wgrad::WGRAD_PIPE && c.atomic) ? 1 : c.slices;
        const int nsg = rslices >= 64 ? 16 : rslices >= 8 ? 4 : 1;
        hipLaunchKernelGGL(conv_wgrad_reduce_kernel, rgrid, dim3(64, nsg), 0, st, k.partial, dw, scale, w, wdot,
                           d->cout, d->cin, d->kh, d->kw, c.cin_pad, c.cout_pad, c.kcols_pad, rslices, accumulate);
        DIN_CHECK_LAUNCH("conv_wgrad_reduce");
    }
    if (dbias && (!c.bias_fused || ordered)) {
        // (fp32 / bf16 tail kernels: no fused bias sum.  accumulate bit 1 adds into the caller-zeroed dbias, as the fused paths do)
        if (int e = launch_colsum(d->dtype, dout, dbias, k.M, d->cout, d->ldo, d->cooff, st, !prezeroed)) return e;
    }
    return DIN_OK;
}

// ---- din_conv_wgrad_group: the weight gradients of several LAYERS in one launch of the pipelined kernel (conv_wgrad.h: WgradGroupK) -------
// Plan: every item keeps the tile geometry plan_wgrad gives it alone; what changes is the pixel slicing.  One common slice length mps
// (whole 32-pixel stages) is chosen so that the items' tiles x slices fill the chip's CUs ONCE: sum_g tiles_g * ceil(M_g / mps) <= CUs.
struct WgradGroupPlan { WgradChoice wp[din_wgrad::WGRAD_GROUP_MAX]; int slices[din_wgrad::WGRAD_GROUP_MAX]; int64_t part_off[din_wgrad::WGRAD_GROUP_MAX], pace_off[din_wgrad::WGRAD_GROUP_MAX]; int mps, bco, wide;
                        int nsg;      // slice groups of the reduce launch's workgroups (1 / 4 / 16), from the largest slice count
                        int64_t ws_bytes; };

static int wgrad_group_key(const din_conv_desc* d, WgradChoice* out) {
    if (!d || d->dtype != DIN_BF16 || d->in_u8 || d->nb <= 0 || d->oh <= 0 || d->ow <= 0) return 0;
    const WgradChoice c = din_wgrad::plan_wgrad(d);                 // (the key is part of the choice: a sixteen-wave pipe plan with slices to reduce)
    if (c.group_key && out) *out = c;
    return c.group_key;
}

static int wgrad_group_cus() {
    static std::atomic<int> cached{0};
    int c = cached.load(std::memory_order_relaxed);
    if (!c) {
        int dev = 0, n = 0;
        (void)hipGetDevice(&dev);
        (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
        c = n > 0 ? n : 256;
        cached.store(c, std::memory_order_relaxed);
    }
    return c;
}

static bool plan_wgrad_group(int n, const din_conv_wgrad_item* items, WgradGroupPlan& gp) {
    if (!items || n < 2 || n > din_wgrad::WGRAD_GROUP_MAX) return false;
    int key0 = 0;
    int64_t cost = 0;
    for (int g = 0; g < n; ++g) {
        const int key = wgrad_group_key(&items[g].desc, &gp.wp[g]);
        if (!key || (g && key != key0)) return false;
        key0 = key;
        cost += (int64_t)gp.wp[g].n_co_tiles * gp.wp[g].n_k_tiles * ((int64_t)items[g].desc.nb * items[g].desc.oh * items[g].desc.ow);
    }
    gp.bco = key0 / 2; gp.wide = key0 & 1;
    const int budget = wgrad_group_cus();
    int64_t mps = (cost + budget - 1) / budget;
    mps = (mps + 31) / 32 * 32;
    if (mps < 32) mps = 32;
    for (int iter = 0; iter < 4096; ++iter) {
        int64_t wgs = 0, next = INT64_MAX;
        for (int g = 0; g < n; ++g) {
            const int64_t M = (int64_t)items[g].desc.nb * items[g].desc.oh * items[g].desc.ow, sl = (M + mps - 1) / mps;
            wgs += sl * gp.wp[g].n_co_tiles * gp.wp[g].n_k_tiles;
            if (sl > 1) {                                           // the smallest slice length that takes one slice off this item
                int64_t m2 = ((M + sl - 2) / (sl - 1) + 31) / 32 * 32;
                if (m2 <= mps) m2 = mps + 32;
                if (m2 < next) next = m2;
            }
        }
        if (wgs <= budget || next == INT64_MAX) break;
        mps = next;
    }
    if (mps >= (1ll << 30)) return false;
    gp.mps = (int)mps;
    int64_t off = 0;
    int max_slices = 1;
    for (int g = 0; g < n; ++g) {
        const int64_t M = (int64_t)items[g].desc.nb * items[g].desc.oh * items[g].desc.ow;
        gp.slices[g] = (int)((M + mps - 1) / mps);
        if (gp.slices[g] > max_slices) max_slices = gp.slices[g];
        gp.part_off[g] = off;
        off += ((int64_t)gp.slices[g] * gp.wp[g].cout_pad * gp.wp[g].kcols_pad * 4 + 255) / 256 * 256;
    }
    for (int g = 0; g < n; ++g) {                                   // sibling-pacing words (WgradK::pace) behind the partial tiles
        gp.pace_off[g] = off;
        off += ((int64_t)gp.slices[g] * gp.wp[g].n_co_tiles * 8 * 4 + 255) / 256 * 256;
    }
    gp.ws_bytes = off;
    gp.nsg = max_slices >= 64 ? 16 : max_slices >= 8 ? 4 : 1;
    return true;
}

// the lines a planned group launches: the group kernel's instantiation (a filter tile launch_wgrad_pipe_group holds no row for: DIN_E_ARG)
// and the one reduce launch.  din_conv_wgrad_group checks here before it touches anything; din_conv_wgrad_group_kernel_names answers from here
static int wgrad_group_lines(const WgradGroupPlan& gp, std::string* names) {
    std::string main_kernel;
    DIN_REQUIRE(din_wgrad::wgrad_pipe_group_name(gp.bco, gp.wide != 0, &main_kernel), "conv_wgrad_group: no group kernel for filter tile %d, wide %d", gp.bco, gp.wide);
    if (names) { *names += main_kernel; *names += "\nconv_wgrad_reduce_group_kernel\n"; }
    return DIN_OK;
}

int din_conv_wgrad_group_key(const din_conv_desc* d) { return wgrad_group_key(d, nullptr); }

int64_t din_conv_wgrad_group_workspace(int n, const din_conv_wgrad_item* items) {
    WgradGroupPlan gp;
    return plan_wgrad_group(n, items, gp) ? gp.ws_bytes : 0;
}

int din_conv_wgrad_group(int n, const din_conv_wgrad_item* items, void* workspace, int64_t workspace_bytes, void* stream) {
    DIN_REQUIRE(items && n >= 1, "conv_wgrad_group: no items");
    WgradGroupPlan gp;
    if (!plan_wgrad_group(n, items, gp)) {                          // not a group this launch serves: layer by layer
        for (int g = 0; g < n; ++g) {                               // (the largest single-item need, checked before the first layer runs)
            const int64_t need = din_conv_workspace_bytes(&items[g].desc, 2);
            if (need > workspace_bytes) DIN_FAIL(DIN_E_WORKSPACE, "conv_wgrad_group: workspace %lld < %lld bytes", (long long)workspace_bytes, (long long)need);
        }
        for (int g = 0; g < n; ++g) {
            const din_conv_wgrad_item& it = items[g];
            if (int e = din_conv_wgrad(&it.desc, it.in, it.dout, it.dw, it.dbias, it.scale, it.w, it.wdot, it.accumulate, workspace, workspace_bytes, stream)) return e;
        }
        return DIN_OK;
    }
    if (!workspace || workspace_bytes < gp.ws_bytes)
        DIN_FAIL(DIN_E_WORKSPACE, "conv_wgrad_group: workspace %lld < %lld bytes", (long long)workspace_bytes, (long long)gp.ws_bytes);
    if (int e = wgrad_group_lines(gp, nullptr)) return e;
    for (int g = 0; g < n; ++g) {                                   // every item is checked before anything is written (the memsets below)
        const din_conv_wgrad_item& it = items[g];
        if (int e = check_desc(&it.desc)) return e;
        DIN_REQUIRE(it.in && it.dout && it.dw, "conv_wgrad_group: null pointer in item %d", g);
        DIN_REQUIRE(!it.wdot || it.w, "conv_wgrad_group: wdot needs w");
    }
    hipStream_t st = as_stream(stream);
    din_wgrad::WgradGroupK G{};
    G.n = n;
    int first = 0;
    for (int g = 0; g < n; ++g) {
        const din_conv_wgrad_item& it = items[g];
        const din_conv_desc* d = &it.desc;
        const WgradChoice& wp = gp.wp[g];
        const bool prezeroed = (it.accumulate & 2) != 0;
        din_wgrad::WgradK& k = G.k[g];
        fill_wgrad_k(k, d, wp, it.in, it.dout, reinterpret_cast<char*>(workspace) + gp.part_off[g]);
        k.slices = gp.slices[g]; k.m_per_slice = gp.mps;
        if (it.dbias) {
            if (!prezeroed && hipMemsetAsync(it.dbias, 0, sizeof(float) * d->cout, st) != hipSuccess) DIN_FAIL(DIN_E_LAUNCH, "conv_wgrad_group: memset");
            k.dbias = it.dbias;
        }
        if (it.wdot && !prezeroed && hipMemsetAsync(it.wdot, 0, sizeof(float) * d->cout, st) != hipSuccess) DIN_FAIL(DIN_E_LAUNCH, "conv_wgrad_group: memset");
        {   // the k-tile siblings of one (filter tile, pixel slice) stream the same dY rows.  Pacing them as the single-layer launch does was
            // measured inside groups (tools/ab_group_pace.sh, profiles/r06_group_pace.txt): HBM fetch 1617 -> 1549 MB per launch, but the naps cost
            // time -- 32 clips 656.3 -> 654.7 clips/s, 4 clips 9.04 -> 9.15 ms: OFF unless DIN_WGRAD_GROUP_PACE=1 (2: up to 8 siblings)
            const char* pe = DIN_OPT("DIN_WGRAD_GROUP_PACE");
            const int want = pe ? atoi(pe) : 0;
            if (want && wp.n_k_tiles >= 2 && wp.n_k_tiles <= (want >= 2 ? 8 : 3) && gp.mps / 32 < (1 << 20) - 1) {
                static std::atomic<unsigned> group_pace_epoch{0};
                k.pace = reinterpret_cast<int*>(reinterpret_cast<char*>(workspace) + gp.pace_off[g]);
                k.pace_base = (int)(((group_pace_epoch.fetch_add(1) % 1023u) + 1u) << 20);
            }
        }
        G.first[g] = first;
        first += wp.n_co_tiles * wp.n_k_tiles * gp.slices[g];
    }
    for (int g = n; g <= din_wgrad::WGRAD_GROUP_MAX; ++g) G.first[g] = first;
    if (int e = din_wgrad::launch_wgrad_pipe_group(G, gp.bco, gp.wide != 0, st)) return e;
    DIN_CHECK_LAUNCH("conv_wgrad_group");
    WgradReduceGroupK R{};
    R.n = n;
    int rfirst = 0;
    for (int g = 0; g < n; ++g) {
        const din_conv_wgrad_item& it = items[g];
        const din_conv_desc* d = &it.desc;
        const WgradChoice& wp = gp.wp[g];
        WgradReduceItem& r = R.it[g];
        r.partial = G.k[g].partial; r.dw = it.dw; r.scale = it.scale; r.w = it.w; r.wdot = it.wdot;
        r.cout = d->cout; r.cin = d->cin; r.kh = d->kh; r.kw = d->kw; r.cin_pad = wp.cin_pad; r.cout_pad = wp.cout_pad; r.kcols_pad = wp.kcols_pad;
        r.slices = gp.slices[g]; r.accumulate = it.accumulate & 1; r.kchunks = (d->kh * d->kw * wp.cin_pad + 255) / 256;
        R.first[g] = rfirst;
        rfirst += d->cout * r.kchunks;
    }
    for (int g = n; g <= din_wgrad::WGRAD_GROUP_MAX; ++g) R.first[g] = rfirst;
    hipLaunchKernelGGL(conv_wgrad_reduce_group_kernel, dim3(rfirst), dim3(64, gp.nsg), 0, st, R);
    DIN_CHECK_LAUNCH("conv_wgrad_group reduce");
    return DIN_OK;
}

int din_conv_wgrad_group_kernel_names(int n, const din_conv_wgrad_item* items, char* buf, int buf_bytes) {
    DIN_REQUIRE(items && n >= 1 && buf_bytes >= 0 && (buf || buf_bytes == 0), "conv_wgrad_group_kernel_names: bad argument");
    std::string names;
    WgradGroupPlan gp;
    const bool planned = plan_wgrad_group(n, items, gp);
    for (int g = 0; g < n; ++g) {
        const din_conv_desc* d = &items[g].desc;
        const SplitDesc sd(d);
        if (int e = check_desc(d)) return e;
        if (planned) continue;                                      // not a group the launch serves: din_conv_wgrad's lines, layer by layer
        DIN_REQUIRE(!d->in_u8 || din_conv_accepts_u8(d), "conv_wgrad_group_kernel_names: in_u8 on a layer din_conv_accepts_u8() rejects");
        din_wgrad::append_wgrad_names(d, din_wgrad::plan_wgrad(d, sd.split), names);
    }
    if (planned) if (int e = wgrad_group_lines(gp, &names)) return e;
    return copy_names(names, buf, buf_bytes);
}

int din_conv_wgrad_group_slices(int n, const din_conv_wgrad_item* items, int32_t* slices, int cap) {
    DIN_REQUIRE(items && n >= 1 && cap >= 0 && (slices || cap == 0), "conv_wgrad_group_slices: bad argument");
    WgradGroupPlan gp;
    if (!plan_wgrad_group(n, items, gp)) return 0;
    for (int g = 0; g < n && g < cap; ++g) slices[g] = gp.slices[g];
    return gp.nsg;
}

static bool wgrad_multi_plan(int nsrc, const din_conv_wsrc* srcs, int dtype, int64_t pixels, int cin, din_wgrad::Wg1x1K* k) {
    dtype = storage_dtype(dtype);                              // (DIN_F32_BF16X3 answers as DIN_F32 does: the kernel serves bf16 groups)
    const char* ev = DIN_OPT("DIN_WGRAD_1X1_MULTI");
    const int mode = ev ? atoi(ev) : 1;                        // 0: off, 1: launches of >= 128K pixels, 2: any size (tests)
    if (!mode || dtype != DIN_BF16 || !srcs || nsrc < 2 || nsrc > 4 || (pixels < 128 * 1024 && mode != 2) || pixels <= 0) return false;
    int couts[4];
    for (int s = 0; s < nsrc; ++s) {
        couts[s] = srcs[s].cout;
        if (srcs[s].ldo % 8 != 0 || srcs[s].cooff % 8 != 0 || srcs[s].ldo < srcs[s].cooff + srcs[s].cout || pixels >= 0x7fffffffll / 64) return false;
    }
    return din_wgrad::plan_wgrad_1x1_multi(nsrc, couts, cin, k);
}

int64_t din_conv1x1_wgrad_multi_workspace(int nsrc, const din_conv_wsrc* srcs, int dtype, int64_t pixels, int cin) {
    din_wgrad::Wg1x1K k{};
    if (!wgrad_multi_plan(nsrc, srcs, dtype, pixels, cin, &k)) return 0;
    return (int64_t)WGRAD_HALO_GRID * k.rows_pad * cin * 4;
}

// the lines a din_conv1x1_wgrad_multi call launches: the plan (a group the kernel does not take: DIN_E_ARG), the instantiation for this input
// width, one reduce launch per source.  The launch checks and plans here; din_conv1x1_wgrad_multi_kernel_names answers from here
static int wgrad_multi_lines(int nsrc, const din_conv_wsrc* srcs, int dtype, int64_t pixels, int cin, din_wgrad::Wg1x1K* k, std::string* names) {
    DIN_REQUIRE(wgrad_multi_plan(nsrc, srcs, dtype, pixels, cin, k), "conv1x1_wgrad_multi: this group does not fit the kernel "
                "(din_conv1x1_wgrad_multi_workspace returns 0 for it: run din_conv_wgrad per layer)");
    std::string main_kernel;
    DIN_REQUIRE(din_wgrad::wgrad_1x1_multi_name(cin, &main_kernel), "conv1x1_wgrad_multi: Cin %d not instantiated", cin);
    if (names) {
        *names += main_kernel; *names += '\n';
        for (int s = 0; s < nsrc; ++s) *names += "conv_wgrad_reduce_kernel\n";
    }
    return DIN_OK;
}

int din_conv1x1_wgrad_multi_kernel_names(int nsrc, const din_conv_wsrc* srcs, int dtype, int64_t pixels, int cin, char* buf, int buf_bytes) {
    DIN_REQUIRE(buf_bytes >= 0 && (buf || buf_bytes == 0), "conv1x1_wgrad_multi_kernel_names: bad argument");
    din_wgrad::Wg1x1K k{};
    std::string names;
    if (int e = wgrad_multi_lines(nsrc, srcs, dtype, pixels, cin, &k, &names)) return e;
    return copy_names(names, buf, buf_bytes);
}

int din_conv1x1_wgrad_multi(int nsrc, const din_conv_wsrc* srcs, int dtype, int64_t pixels, int cin, int ldi, int cioff, const void* in,
                            int accumulate, void* workspace, int64_t workspace_bytes, void* stream) {
    din_wgrad::Wg1x1K k{};
    DIN_REQUIRE(in && workspace, "conv1x1_wgrad_multi: null pointer");
    if (int e = wgrad_multi_lines(nsrc, srcs, dtype, pixels, cin, &k, nullptr)) return e;
    DIN_REQUIRE(ldi % 8 == 0 && cioff % 8 == 0 && ldi >= cioff + cin, "conv1x1_wgrad_multi: bad input view");
    const int64_t need = (int64_t)WGRAD_HALO_GRID * k.rows_pad * cin * 4;
    if (workspace_bytes < need) DIN_FAIL(DIN_E_WORKSPACE, "conv1x1_wgrad_multi: workspace %lld < %lld bytes", (long long)workspace_bytes, (long long)need);
    for (int s = 0; s < nsrc; ++s)                                  // every source is checked before anything is written (the memsets below)
        DIN_REQUIRE(srcs[s].dout && srcs[s].dw && (!srcs[s].wdot || srcs[s].w), "conv1x1_wgrad_multi: null pointer in source %d", s);
    hipStream_t st = as_stream(stream);
    const bool prezeroed = (accumulate & 2) != 0;
    accumulate &= 1;
    k.x = in; k.partial = reinterpret_cast<float*>(workspace);
    k.M = (int)pixels; k.Cin = cin; k.ldi = ldi; k.cioff = cioff; k.nsrc = nsrc;
    for (int s = 0; s < nsrc; ++s) {
        k.src[s].g = srcs[s].dout; k.src[s].dbias = srcs[s].dbias; k.src[s].cout = srcs[s].cout; k.src[s].ld = srcs[s].ldo; k.src[s].coff = srcs[s].cooff;
        if (!prezeroed) {
            if (srcs[s].dbias && hipMemsetAsync(srcs[s].dbias, 0, sizeof(float) * srcs[s].cout, st) != hipSuccess) DIN_FAIL(DIN_E_LAUNCH, "conv1x1_wgrad_multi: memset");
            if (srcs[s].wdot && hipMemsetAsync(srcs[s].wdot, 0, sizeof(float) * srcs[s].cout, st) != hipSuccess) DIN_FAIL(DIN_E_LAUNCH, "conv1x1_wgrad_multi: memset");
        }
    }
    if (int e = din_wgrad::launch_wgrad_1x1_multi(k, WGRAD_HALO_GRID, st)) return e;
    DIN_CHECK_LAUNCH("conv1x1_wgrad_multi");
    for (int s = 0; s < nsrc; ++s) {
        dim3 rgrid(srcs[s].cout, (cin + 255) / 256);
        hipLaunchKernelGGL(conv_wgrad_reduce_kernel, rgrid, dim3(64, 16), 0, st, k.partial + (int64_t)k.src[s].row0 * cin, srcs[s].dw, srcs[s].scale,
                           srcs[s].w, srcs[s].wdot, srcs[s].cout, cin, 1, 1, cin, k.rows_pad, cin, WGRAD_HALO_GRID, accumulate);
        DIN_CHECK_LAUNCH("conv1x1_wgrad_multi reduce");
    }
    return DIN_OK;
}

int din_colsum(const void* g, int dtype, int64_t rows, int c, int ld, int coff, float* out, void* stream) {
    DIN_REQUIRE(g && out && rows > 0 && c > 0 && ld >= coff + c && coff >= 0, "colsum: bad argument");
    DIN_REQUIRE(dtype == DIN_F32 || dtype == DIN_BF16, "colsum: bad dtype");
    return launch_colsum(dtype, g, out, rows, c, ld, coff, as_stream(stream));
}

}  // extern "C"
