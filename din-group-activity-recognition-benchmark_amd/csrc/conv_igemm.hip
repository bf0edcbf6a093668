// Implicit-GEMM convolution for gfx950 (MI355X): fwd / dgrad share one gather kernel; the weight gradient lives in conv_wgrad.hip.
// This file holds the tile kernel (conv_gather_fast_kernel) with its epilogues, the generic kernel, the split-K finish, the host planning
// (plan_gather, choose_tile, choose_gather: the ONE place a forward / data-gradient launch is given its kernel), launch_choice / run_gather,
// the name reporters and the conv entry points.  The other kernel families sit behind conv_gather.h in files of their own:
// conv_regw.hip, conv_stream.hip, conv_halo.hip, conv_small.hip, conv_gather_pipe.hip; filter packing and the BatchNorm folds: conv_pack.hip.
// Every family keeps ONE X-macro table of its instantiations (here: DIN_CONV_TILE_TABLE, DIN_CONV_GENERIC_TABLE) that its launcher and its
// namer both walk, so a chosen tuple the library does not hold is an error from the launch and from the reporter alike.
//
//   D[co][pix] = sum_k  Wpk[co][k] * im2col(X)[pix][k]          k = (r, s, ci)   (NHWC, ci contiguous)
//
// One template covers both storage types because the byte geometry is identical: every operand moves in
// 16-byte "chunks" along the reduction axis (4 fp32 or 8 bf16).  A lane feeds the MFMA one chunk:
//   bf16 : v_mfma_f32_16x16x32_bf16  -- the chunk is the lane's 8 k-values          (1 MFMA / chunk set)
//   fp32 : v_mfma_f32_16x16x4_f32    -- element j of the chunk feeds the j-th of 4 MFMAs (exact fp32)
//   f32x3: fp32 storage, the chunk's 4 values split into three bf16 parts each, 3 x v_mfma_f32_16x16x32_bf16 (DIN_F32_BF16X3)
// (the k order inside a k-step is permuted identically for both operands, which a sum does not care about).
//
// Tiles: 128 or 256 pixels x BN (64 .. 256) filters per workgroup of 4, 8 or 16 waves (wave grid WM x WN; the rows of DIN_CONV_TILE_TABLE,
// chosen by choose_tile); the generic kernel: 128 pixels x 64 | 128 filters on 4 waves as 2x2.  k-step = 8 chunks (128 B per row; the
// deep-ring tiles step 4), an LDS ring of 2-4 stages with an XOR swizzle (chunk ^ ((row>>1)&7)) that makes both the
// 8-lane ds_write_b128 groups and the 16-lane ds_read_b128 groups conflict-free.  The MFMA's i index is the
// FILTER and j the PIXEL so that a lane ends up holding 4 consecutive output channels of one pixel
// (16-/8-byte NHWC stores).  Epilogue fuses bias, ReLU, the ReLU-backward mask, accumulation and the
// channel-offset write that makes torch.cat free.
//
// Replaces the arithmetic of torch.nn.Conv2d / nn.Linear reached from the reference at
// backbone/backbone.py:44-99, infer_model.py:184,190,226 and infer_module/dynamic_infer_module.py:149,191,195.
#include "din_common.h"
#include "conv_wgrad.h"
#include "conv_gather.h"
#include "conv_shared.h"
#include <atomic>
#include <unordered_map>
#include <mutex>
#include <stdlib.h>
#include <string.h>
#include <string>

using din_conv::check_desc;
using din_wgrad::lds_dma16;
using din_gather::ConvK;
using din_gather::out_pixel;
using din_gather::staged_tile_store;

namespace {

#ifndef DIN_GATHER_PRIO
#define DIN_GATHER_PRIO 0         // experiment: raised wave priority over the MFMA stream of the interleaved k-step
#endif
#ifndef DIN_GATHER_ILV
#define DIN_GATHER_ILV 1          // in-wave interleaved schedule of the FASTK gather loop (0: the compiler-scheduled loop, for A/B builds)
#endif
constexpr int BM = 128;      // pixels per workgroup tile

__device__ __forceinline__ int lds_slot(int row, int chunk) { return row * KC + (chunk ^ ((row >> 1) & 7)); }

// ------------------------------------------------------------------------------------------------
// fwd / dgrad gather kernels
// ------------------------------------------------------------------------------------------------
// One k-step of the FASTK loop: NA pixel-tile + NB filter-tile wave-level DMAs into consecutive STRIDE-byte slots of a ring stage, as
// ONE asm statement: M0 is written once and then advanced (declared clobbered instead of saved/restored around every transfer),
// 3 instructions per transfer instead of 5 -- the scalar unit is shared by the CU's 16 waves and was 40 % busy (SQ_ACTIVE_INST_SCA).
template <int NA, int NB, int STRIDE>
__device__ __forceinline__ void lds_dma_stage(uint32_t lds_addr, __amdgpu_buffer_rsrc_t rsA, const unsigned (&va)[NA], int soffA,
                                              __amdgpu_buffer_rsrc_t rsB, const int (&vb)[NB], int soffB) {
#define DIN_DMA_FIRST(V, R, S) "s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 " V ", " R ", " S " offen lds\n\t"
#define DIN_DMA_NEXT(V, R, S) "s_add_u32 m0, m0, %5\n\ts_nop 0\n\tbuffer_load_dwordx4 " V ", " R ", " S " offen lds\n\t"
    static_assert(NA == 2 && NB >= 1 && NB <= 3, "instantiated for the 8-wave 128-pixel tiles");
    if constexpr (NB == 1)
        asm volatile(DIN_DMA_FIRST("%6", "%1", "%3") DIN_DMA_NEXT("%7", "%1", "%3") DIN_DMA_NEXT("%8", "%2", "%4")
                     :: "s"(lds_addr), "s"(rsA), "s"(rsB), "s"(soffA), "s"(soffB), "n"(STRIDE), "v"(va[0]), "v"(va[1]), "v"(vb[0])
                     : "memory", "m0", "scc");
    else if constexpr (NB == 2)
        asm volatile(DIN_DMA_FIRST("%6", "%1", "%3") DIN_DMA_NEXT("%7", "%1", "%3") DIN_DMA_NEXT("%8", "%2", "%4") DIN_DMA_NEXT("%9", "%2", "%4")
                     :: "s"(lds_addr), "s"(rsA), "s"(rsB), "s"(soffA), "s"(soffB), "n"(STRIDE), "v"(va[0]), "v"(va[1]), "v"(vb[0]), "v"(vb[1])
                     : "memory", "m0", "scc");
    else
        asm volatile(DIN_DMA_FIRST("%6", "%1", "%3") DIN_DMA_NEXT("%7", "%1", "%3") DIN_DMA_NEXT("%8", "%2", "%4") DIN_DMA_NEXT("%9", "%2", "%4")
                     DIN_DMA_NEXT("%10", "%2", "%4")
                     :: "s"(lds_addr), "s"(rsA), "s"(rsB), "s"(soffA), "s"(soffB), "n"(STRIDE), "v"(va[0]), "v"(va[1]), "v"(vb[0]), "v"(vb[1]), "v"(vb[2])
                     : "memory", "m0", "scc");
#undef DIN_DMA_FIRST
#undef DIN_DMA_NEXT
}

// direct (un-staged) epilogue shared by both kernels: lane holds D[co0 + i*16 + (lane>>4)*4 + e][pix0 + j*16 + (lane&15)]
template <typename T, int TI, int TJ, int BN, int BMT = BM, int WM = 2, int WN = 2>
__device__ __forceinline__ void epilogue_direct(const ConvK& p, f32x4 (&acc)[TI][TJ], int co_tile, int px_tile, int wm, int wn, int lane, int split) {
    const int co_base = co_tile * BN + wn * (BN / WN) + (lane >> 4) * 4;
    const int px_base = px_tile * BMT + wm * (BMT / WM) + (lane & 15);
    if (p.splitk > 1) {
        // raw fp32 partial sums: partial[split][pix][cout_pad]   (cout_pad = n_co_tiles*BN)
        const int cpad = p.n_co_tiles * BN;
#pragma unroll
        for (int j = 0; j < TJ; ++j) {
            int m = px_base + j * 16;
            if (m >= p.M) continue;
            float* dst = p.partial + ((int64_t)split * p.M + m) * cpad;
#pragma unroll
            for (int i = 0; i < TI; ++i) *reinterpret_cast<f32x4*>(dst + co_base + i * 16) = acc[i][j];
        }
        return;
    }
    T* __restrict__ outp = reinterpret_cast<T*>(p.out);
    const T* __restrict__ maskp = reinterpret_cast<const T*>(p.mask);
#pragma unroll
    for (int j = 0; j < TJ; ++j) {
        int m = px_base + j * 16;
        if (m >= p.M) continue;
#pragma unroll
        for (int i = 0; i < TI; ++i) {
            int co = co_base + i * 16;
            if (co >= p.Cout) continue;
            f32x4 v = acc[i][j];
            const int64_t opx = out_pixel(p, m);
            int64_t o = opx * p.ldo + p.cooff + co;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (co + e >= p.Cout) break;
                float x = v[e];
                if (p.flags & DIN_CONV_BIAS) x += p.bias[co + e];
                if (p.flags & DIN_CONV_RELU) x = fmaxf(x, 0.f);
                if (p.flags & DIN_CONV_MASK) {
                    float y = Elem<T>::ld(maskp + opx * p.ldm + p.moff + co + e);
                    x = y > 0.f ? x : 0.f;
                }
                if (p.flags & DIN_CONV_ACCUM) x += Elem<T>::ld(outp + o + e);
                v[e] = x;
            }
            if (co + 3 < p.Cout && ((o & 3) == 0)) {
                if constexpr (sizeof(T) == 4) {
                    *reinterpret_cast<f32x4*>(outp + o) = v;
                } else {
                    u32x2 pk = {pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
                    *reinterpret_cast<u32x2*>(outp + o) = pk;
                }
            } else {
                for (int e = 0; e < 4 && co + e < p.Cout; ++e) Elem<T>::st(outp + o + e, v[e]);
            }
        }
    }
}

// Generic addressing (strided dgrad / > 64 taps): plain loads with per-k-step coordinate arithmetic.
template <typename T, int BN>
__global__ __launch_bounds__(NTHREADS, 2) void conv_gather_generic_kernel(ConvK p) {
    constexpr int EPC = Elem<T>::EPC;
    constexpr int TI = BN / 32, TJ = BM / 32, PA = BM / 32, PB = BN / 32;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    u32x4* smem = reinterpret_cast<u32x4*>(smem_raw);
    constexpr int BUF = (BM + BN) * KC;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid >> 1, wn = wid & 1;
    int bx_, by_;
    xcd_block(bx_, by_);
    const int co_tile = bx_ % p.n_co_tiles, px_tile = bx_ / p.n_co_tiles;
    const int split = by_;
    const int ks_begin = split * p.ks_per_split;
    int ks_end = ks_begin + p.ks_per_split;
    if (ks_end > p.nk) ks_end = p.nk;
    const int cq = tid & 7, r0 = tid >> 3;
    int tyb[PA], txb[PA], nbase[PA];
#pragma unroll
    for (int i = 0; i < PA; ++i) {
        int m = px_tile * BM + r0 + 32 * i;
        tyb[i] = -(1 << 28); txb[i] = 0; nbase[i] = 0;
        if (m < p.M) {
            int n = m / (p.OH * p.OW);
            int rem = m - n * (p.OH * p.OW);
            int oy = rem / p.OW, ox = rem - oy * p.OW;
            tyb[i] = oy * p.ay + p.by; txb[i] = ox * p.ax + p.bx; nbase[i] = n * p.H * p.W;
        }
    }
    const T* __restrict__ inp = reinterpret_cast<const T*>(p.in);
    const u32x4* __restrict__ wp = reinterpret_cast<const u32x4*>(p.w);
    u32x4 ga[PA], gb[PB];
    auto load_global = [&](int ks) {
        const int q = ks * KC + cq;
        const bool qok = q < p.Q;
        int tap = qok ? q / p.cpt : 0;
        int cc = q - tap * p.cpt;
        int r = tap / p.kw, s = tap - r * p.kw;
        const int dyk = r * p.cy, dxk = s * p.cx;
#pragma unroll
        for (int i = 0; i < PA; ++i) {
            int ty = tyb[i] + dyk, tx = txb[i] + dxk;
            bool ok = qok && ty >= 0 && tx >= 0;
            int iy = ty, ix = tx;
            if (p.divy > 1) { iy = ty / p.divy; ok = ok && (iy * p.divy == ty); }
            if (p.divx > 1) { ix = tx / p.divx; ok = ok && (ix * p.divx == tx); }
            ok = ok && iy < p.H && ix < p.W;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (ok) v = *reinterpret_cast<const u32x4*>(inp + (int64_t)(nbase[i] + iy * p.W + ix) * p.ldi + p.cioff + cc * EPC);
            ga[i] = v;
        }
#pragma unroll
        for (int i = 0; i < PB; ++i) gb[i] = wp[(int64_t)(co_tile * BN + r0 + 32 * i) * p.wld + ks * KC + cq];
    };
    auto store_lds = [&](int buf) {
        u32x4* A = smem + buf * BUF;
        u32x4* B = A + BM * KC;
#pragma unroll
        for (int i = 0; i < PA; ++i) A[lds_slot(r0 + 32 * i, cq)] = ga[i];
#pragma unroll
        for (int i = 0; i < PB; ++i) B[lds_slot(r0 + 32 * i, cq)] = gb[i];
    };
    f32x4 acc[TI][TJ];
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int frow = lane & 15, fchunk = lane >> 4;
    if (ks_begin < ks_end) {
        load_global(ks_begin);
        store_lds(0);
        __syncthreads();
        for (int ks = ks_begin; ks < ks_end; ++ks) {
            const int cur = (ks - ks_begin) & 1;
            const bool more = ks + 1 < ks_end;
            if (more) load_global(ks + 1);
            const u32x4* A = smem + cur * BUF;
            const u32x4* B = A + BM * KC;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                u32x4 wf[TI], xf[TJ];
#pragma unroll
                for (int i = 0; i < TI; ++i) wf[i] = B[lds_slot(wn * (BN / 2) + i * 16 + frow, kk * 4 + fchunk)];
#pragma unroll
                for (int j = 0; j < TJ; ++j) xf[j] = A[lds_slot(wm * (BM / 2) + j * 16 + frow, kk * 4 + fchunk)];
#pragma unroll
                for (int i = 0; i < TI; ++i)
#pragma unroll
                    for (int j = 0; j < TJ; ++j) Mma<T>::run(wf[i], xf[j], acc[i][j]);
            }
            if (more) store_lds(cur ^ 1);
            __syncthreads();
        }
    }
    epilogue_direct<T, TI, TJ, BN>(p, acc, co_tile, px_tile, wm, wn, lane, split);
}

// Fast addressing (stride-1 gathers, <= 32 taps: every forward conv and every stride-1 dgrad).
//  * operands are fetched with BUFFER loads: one 32-bit byte offset per tile row, recomputed only when the tap changes;
//    padding taps get an out-of-range offset and the hardware returns zeros; the k-offset inside a tap is a scalar.
//    The resource base is moved to the first image of the tile so 32-bit offsets suffice for any tensor size.
//  * prefetch distance 2 through two register sets; LDS double buffer; one barrier per k-step.
//  * epilogue staged through LDS: bias/ReLU applied in registers, tile transposed in LDS, then 16-byte coalesced
//    stores with vector loads for the ReLU-backward mask and the accumulate input.
// Tile variants <BMT, BN, WM x WN waves, DEEP>: 128x128 (2x2), 128x64 (2x2) and 256x64 (4x1; twice the work per barrier for the
// short-K, latency-bound 64-filter layers; single register set to stay under 256 VGPRs, no LDS tables so two workgroups fit a CU).
// 512-thread variants 256x128 (4x2 waves) and 256x256 (4x2 waves, 64x128 wave tiles) raise the FLOPs per byte streamed into LDS
// from 64 to 85 / 128; measured throughput follows that ratio (128x128 ~770, 256x256 ~1150 TFLOP/s) although the L2->LDS path itself
// is not the limiter (profiles/r01_stream_probe.txt: 37 TB/s raw; the k-loop structure tops out at ~68 % of MFMA peak, and the MFMA
// rate drops a further ~27 % on real, toggling operands).
// Pipeline: an NS-stage ring of LDS stages of KCS 16-byte chunks per row, filled by LDS-DMA, NS-1 stages in flight: per stage ONE
// counted s_waitcnt vmcnt(N) (VMEM completes in order: N = DMAs of the younger stages) + ONE raw s_barrier (every wave's share of
// the stage landed, and every wave is done reading the stage about to be refilled).
// FASTK (bf16 8-wave tiles; host: whole k-steps per tap, no tap remap, k-order = taps inside channel chunks): every piece of per-step
// loader state is scalar except one validity select per tile row, the offsets of the NEXT transfer are prepared while the current
// stage is multiplied (so only the transfers themselves sit between the barrier and the MFMAs), and no other mode is compiled in.
// LANEK (with FASTK; bf16 8-wave tiles whose reduction channels are NOT whole k-steps per tap -- Conv2d_4a's 80, the 160-channel 7-tap layers of
// Mixed_6c / 6d): the same double-buffered, in-wave interleaved step, with the k-walk PER LANE: a lane's 16-byte chunk of a k-step is chunk
// q = 8 ks + cq of the flattened (tap, channel) axis, so every lane carries its own (tap, channel chunk) and forms its own tap delta / validity
// bit (~10 VALU per step); the filter side stays a scalar offset (the packed bank IS the flattened axis).  These launches used to run the
// general loop below -- compiler-scheduled, no interleaving: Conv2d_4a forward 718 TF where the same tile reaches 1004 TF on FASTK.
template <typename T, int BMT, int BN, int WM, int WN, int KCS, int NS, bool MULTI = false, bool FASTK = false, bool XSRC = false, bool LANEK = false>
// (second argument = waves per SIMD the register allocation must leave room for: the 8-wave 128-pixel bf16 tiles run TWO workgroups per CU
//  = four waves per SIMD = at most 128 VGPRs.  Left at 2, a harmless-looking edit -- round 4: the knock-out switches turned compile-time
//  constants -- moved the FASTK 128 x 192 instantiation from 125 to 131 registers: one workgroup per CU, 186 -> 259 us per launch, -1.6 ms per
//  step, caught only by diffing kernel_stats.csv against the previous round's.)
#ifdef DIN_EXPERIMENTS
// (experiment, round 4: four-wave 128-pixel tiles on 32-deep stages, THREE workgroups per CU = three barrier domains: <= 168 VGPRs)
__global__ __launch_bounds__(64 * WM * WN, (sizeof(T) == 2 && BMT == 128 && WM * WN == 8) ? 4 : ((sizeof(T) == 2 && BMT == 128 && WM * WN == 4 && KCS == 4 && NS == 2 && FASTK) ? 3 : 2)) void conv_gather_fast_kernel(ConvK p) {
#else
__global__ __launch_bounds__(64 * WM * WN, (sizeof(T) == 2 && BMT == 128 && WM * WN == 8) ? 4 : 2) void conv_gather_fast_kernel(ConvK p) {
#endif
#if defined(__HIP_DEVICE_COMPILE__)      // the host pass only needs the launch stub (the LDS-DMA builtin is device-only)
    constexpr int EPC = Elem<T>::EPC;
    constexpr int BM = BMT;                                  // shadows the file-level default inside this kernel
    constexpr int KC = KCS;                                  // chunks per stage row (shadows the packing granularity of 8)
    constexpr int NT = 64 * WM * WN;                         // threads per workgroup
    constexpr int LR = NT / KC;                              // tile rows covered by one loader pass (KC chunk lanes per row)
    constexpr int RW = 64 / KC;                              // rows written by one wave-level DMA (1 KiB)
    // the loader covers LR rows per pass: a filter tile that is not a multiple (160 or 96 rows on 8 waves) is loaded as PB whole passes
    // into a padded LDS region; the surplus rows (next tile's filters or zeros) are never read
    constexpr int TI = BN / WN / 16, TJ = BM / WM / 16, PA = BM / LR, PB = (BN + LR - 1) / LR, BNP = PB * LR;
    static_assert(BM % LR == 0, "pixel tile must be whole loader passes");
    constexpr int BUF = (BM + BNP) * KC;                     // 16-byte units per stage
    auto lds_slot = [](int row, int chunk) { return row * KCS + (chunk ^ ((row >> 1) & (KCS - 1))); };   // conflict-free for 4 and 8
    constexpr int CPITCH = BN * (int)sizeof(T) + 16;         // epilogue tile row pitch (bytes): +16 B kills bank conflicts
    constexpr unsigned OOB = 0x80000000u;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    u32x4* smem = reinterpret_cast<u32x4*>(smem_raw);
    int* wtap_lds = reinterpret_cast<int*>(smem_raw + NS * BUF * 16);  // [32] tap -> tap of the packed bank (remap launches only)

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid / WN, wn = wid % WN;
    int bx_, by_;
    xcd_block(bx_, by_);
    const int co_tile = bx_ % p.n_co_tiles, px_tile = bx_ / p.n_co_tiles;
    const int split = by_;
    // host counts k-steps in units of 8 chunks (the packing granularity); this kernel steps KCS chunks
    const int ks_begin = split * p.ks_per_split * (8 / KCS);
    int ks_end = ks_begin + p.ks_per_split * (8 / KCS);
    {
        const int nk_s = (p.Q + KCS - 1) / KCS;
        if (ks_end > nk_s) ks_end = nk_s;
    }
    [[maybe_unused]] const int ks_x0 = ks_end;                 // XSRC: k-steps >= ks_x0 read the extra 1x1 source (never with split-K)
    if constexpr (XSRC) {
        static_assert(!MULTI && !FASTK && KCS == 8, "XSRC: general single-source loop");
        ks_end += p.xsteps;
    }
    const int ntaps = p.kh * p.kw;
    if (p.remap && tid < 32) wtap_lds[tid] = tid < ntaps ? (int)p.wtap[tid] : 0;
    // byte offset of tap t = (r,s) relative to tap (0,0): r*dA + s*dB, r = t / kw by an exact multiply-shift (t < 32)
    const int dA = p.cy * p.W * p.ldi * (int)sizeof(T), dB = p.cx * p.ldi * (int)sizeof(T);
    const int inv_kw = 65536 / p.kw + 1;
    auto tapdelta = [&](int t) { int r = (t * inv_kw) >> 16; return r * dA + (t - r * p.kw) * dB; };

    // ---- buffer resources ---------------------------------------------------------------------------------
    const int m_first = px_tile * BM;
    const int n_first = m_first / (p.OH * p.OW);                              // uniform
    const long long img_bytes = (long long)p.H * p.W * p.ldi * (long long)sizeof(T);
    const long long a_off = (long long)n_first * img_bytes;
    long long a_rem = p.in_bytes - a_off;
    if (a_rem > 0x7fffffffll) a_rem = 0x7fffffffll;
    __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(p.in)) + a_off, 0, (int)a_rem, 0x00020000);
    __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.w), 0, (int)p.w_bytes, 0x00020000);

    // ---- per-row state --------------------------------------------------------------------------------------
    // LDS-DMA writes lane-linearly (wave base + lane*16 B; measured: profiles/r01_probe_lds_dma.txt), i.e. lane -> (row lane>>3,
    // slot lane&7).  The XOR swizzle of the LDS image is therefore applied to the SOURCE: the lane fetches logical chunk
    // cq = slot ^ swizzle(row) (guide rule 21: linear destination + permuted source + same permutation on the read).
    const int r0 = tid / KC;
    const int cq = (tid % KC) ^ ((r0 >> 1) & (KC - 1));
    int pixoff[PA];                       // byte offset (from the resource base) of tap (0,0), channel cioff, chunk 0
                                          // (MULTI: pixel index relative to the first image of the tile, -1 = row beyond M)
    unsigned vmask[PA];                   // bit t set <=> tap t of this pixel lies inside the image (<= 32 taps)
    {
        const unsigned full_row = p.kw >= 32 ? 0xffffffffu : ((1u << p.kw) - 1u);
#pragma unroll
        for (int i = 0; i < PA; ++i) {
            int m = m_first + r0 + LR * i;
            vmask[i] = 0u; pixoff[i] = 0;
            if (m < p.M) {
                int n = m / (p.OH * p.OW);
                int rem = m - n * (p.OH * p.OW);
                int oy = rem / p.OW, ox = rem - oy * p.OW;
                const int ty0 = oy * p.ay + p.by, tx0 = ox * p.ax + p.bx;
                // valid s: 0 <= tx0 + s*cx < W   (cx may be negative for dgrad) -- build the kw-bit column mask once
                unsigned cmask = 0u;
                for (int s2 = 0; s2 < p.kw; ++s2) {
                    int tx = tx0 + s2 * p.cx;
                    cmask |= (tx >= 0 && tx < p.W) ? (1u << s2) : 0u;
                }
                cmask &= full_row;
                unsigned mk = 0u;
                for (int r = 0; r < p.kh; ++r) {
                    int ty = ty0 + r * p.cy;
                    mk |= (ty >= 0 && ty < p.H) ? (cmask << (r * p.kw)) : 0u;
                }
                vmask[i] = mk;
                pixoff[i] = (((n - n_first) * p.H + ty0) * p.W + tx0) * p.ldi * (int)sizeof(T) + p.cioff * (int)sizeof(T);
                if constexpr (MULTI) pixoff[i] = m - n_first * (p.OH * p.OW);      // 1x1, stride 1: output pixel == input pixel
            } else if constexpr (MULTI) pixoff[i] = -1;
        }
    }
    int voffB[PB];
#pragma unroll
    for (int i = 0; i < PB; ++i) voffB[i] = ((co_tile * BN + r0 + LR * i) * p.wld + (p.remap ? 0 : cq)) * 16;
    if (p.remap) __syncthreads();                                             // wtap table visible (uniform branch)

    const bool tap_uniform = (p.cpt % KC) == 0;
    // uniform-tap bookkeeping (scalar).  korder: ks = cchunk * ntaps + tap
    int tap_s, cc_s;
    if (p.korder) { const int cch = ks_begin / ntaps; tap_s = ks_begin - cch * ntaps; cc_s = cch * KC; }
    else { tap_s = (ks_begin * KC) / p.cpt; cc_s = ks_begin * KC - tap_s * p.cpt; }
    unsigned voffA[PA];
    auto refresh_uniform = [&]() {
        const int td = tapdelta(tap_s) + cq * 16;
#pragma unroll
        for (int i = 0; i < PA; ++i) voffA[i] = (tap_s < ntaps && ((vmask[i] >> tap_s) & 1u)) ? (unsigned)(pixoff[i] + td) : OOB;
    };
    // per-lane bookkeeping for k-steps that straddle taps
    int tap_l = (ks_begin * KC + cq) / p.cpt, cc_l = ks_begin * KC + cq - tap_l * p.cpt;
    if (tap_uniform) refresh_uniform();

    // ---- multi-source bookkeeping (uniform): current source, chunk position inside it ----------------------------------------
    int sb = 0, cc_m = 0;
    [[maybe_unused]] auto open_source = [&](int bsrc) {
        const ConvK::Src& sr = p.src[bsrc];
        const long long imgb = (long long)p.H * p.W * sr.ld * (long long)sizeof(T);
        long long rem = sr.in_bytes - (long long)n_first * imgb;
        if (rem > 0x7fffffffll) rem = 0x7fffffffll;
        rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(reinterpret_cast<const char*>(sr.in)) + (long long)n_first * imgb, 0, (int)rem, 0x00020000);
        rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(sr.w), 0, (int)sr.w_bytes, 0x00020000);
#pragma unroll
        for (int i = 0; i < PB; ++i) voffB[i] = ((co_tile * BN + r0 + LR * i) * sr.wld + cq) * 16;
    };
    if constexpr (MULTI) {
        // position at this split's first k-step (split-K is never used with MULTI, but keep the walk general)
        int skip = ks_begin;
        while (sb < p.nsrc) {
            const int steps = (p.src[sb].cpt + KC - 1) / KC;
            if (skip < steps) break;
            skip -= steps; ++sb;
        }
        cc_m = skip * KC;
        if (sb < p.nsrc) open_source(sb);
    }

    // LDS byte address of this wave's RW rows of pass 0 in stage 0 (wave-uniform -> SGPR)
    const uint32_t ldsA0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(smem + (wid * RW) * KC));
    // XSRC: resources of the extra source (its tensor from the first image of the tile on, its packed 1x1 bank)
    [[maybe_unused]] __amdgpu_buffer_rsrc_t rsXA = rsA, rsXB = rsB;
    [[maybe_unused]] long long x_px0 = 0;
    if constexpr (XSRC) {
        const ConvK::Src& sr = p.src[0];
        x_px0 = (long long)n_first * (p.out_sy == 0 ? p.OH * p.OW : p.out_H * p.out_W);
        long long rem = sr.in_bytes - x_px0 * sr.ld * (long long)sizeof(T);
        if (rem > 0x7fffffffll) rem = 0x7fffffffll;
        rsXA = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(reinterpret_cast<const char*>(sr.in)) + x_px0 * sr.ld * (long long)sizeof(T), 0,
                                                 (int)(rem > 0 ? rem : 0), 0x00020000);
        rsXB = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(sr.w), 0, (int)sr.w_bytes, 0x00020000);
    }
    // issue the DMA of k-step ks into stage `buf`: PA + PB wave-level 1-KiB transfers per wave, no VGPRs, no ds_write
    auto issue_dma = [&](int buf, int ks) {
        const uint32_t A = ldsA0 + (uint32_t)(buf * BUF * 16);
        const uint32_t B = A + (uint32_t)(BM * KC * 16);
        if constexpr (XSRC) {
            if (ks >= ks_x0) {
                const ConvK::Src& sr = p.src[0];
                const int cc = (ks - ks_x0) * KC;
                const bool cok = (cc + cq) < sr.cpt;
                const int chan = sr.coff * (int)sizeof(T) + (cc + cq) * 16, ldb = sr.ld * (int)sizeof(T);
#pragma unroll
                for (int i = 0; i < PA; ++i) {
                    const int m = m_first + r0 + LR * i;
                    unsigned vo = OOB;
                    if (cok && m < p.M) vo = (unsigned)((int)(out_pixel(p, m) - x_px0) * ldb + chan);
                    lds_dma16(A + (uint32_t)(LR * i * KC * 16), rsXA, (int)vo, 0);
                }
#pragma unroll
                for (int i = 0; i < PB; ++i)
                    lds_dma16(B + (uint32_t)(LR * i * KC * 16), rsXB, ((co_tile * BN + r0 + LR * i) * sr.wld + cq) * 16, cc * 16);
                return;
            }
        }
        int remapB = 0;                                    // per-lane chunk offset (bytes) into the packed bank, remap mode only
        int korderB = 0;                                   // scalar chunk offset of this k-step in the packed bank (korder mode)
        if constexpr (MULTI) {
            const ConvK::Src& sr = p.src[sb < p.nsrc ? sb : 0];
            const bool cok = sb < p.nsrc && (cc_m + cq) < sr.cpt;         // chunk inside this source's channels
            const int chan = sr.coff * (int)sizeof(T) + (cc_m + cq) * 16;
            const int ldb = sr.ld * (int)sizeof(T);
#pragma unroll
            for (int i = 0; i < PA; ++i) {
                unsigned vo = (cok && pixoff[i] >= 0) ? (unsigned)(pixoff[i] * ldb + chan) : OOB;
                lds_dma16(A + (uint32_t)(LR * i * KC * 16), rsA, (int)vo, 0);
            }
            const int soffB = cc_m * 16;
#pragma unroll
            for (int i = 0; i < PB; ++i) lds_dma16(B + (uint32_t)(LR * i * KC * 16), rsB, voffB[i], soffB);
            cc_m += KC;
            if (sb < p.nsrc && cc_m >= sr.cpt) { cc_m = 0; ++sb; if (sb < p.nsrc) open_source(sb); }
            return;
        }
        if (tap_uniform) {
            const int soff = cc_s * 16;
            if (p.remap) remapB = ((tap_s < ntaps ? wtap_lds[tap_s] : 0) * p.cpt + cc_s + cq) * 16;
            korderB = (tap_s * p.cpt + cc_s) * 16;
#pragma unroll
            for (int i = 0; i < PA; ++i)
                lds_dma16(A + (uint32_t)(LR * i * KC * 16), rsA, (int)voffA[i], soff);
            if (p.korder) {
                if (++tap_s == ntaps) { tap_s = 0; cc_s += KC; }
                refresh_uniform();
            } else {
                cc_s += KC;
                if (cc_s >= p.cpt) { cc_s = 0; ++tap_s; refresh_uniform(); }
            }
        } else {
            // k-step straddles taps: per-lane tap index; cost kept to ~5 VALU per row (bit test, add, select)
            const bool ok = tap_l < ntaps;
            const int td = tapdelta(tap_l) + cc_l * 16;
            const unsigned bit = ok ? (1u << tap_l) : 0u;
            if (p.remap) remapB = ok ? (wtap_lds[tap_l] * p.cpt + cc_l) * 16 : 0;
#pragma unroll
            for (int i = 0; i < PA; ++i) {
                unsigned vo = (vmask[i] & bit) ? (unsigned)(pixoff[i] + td) : OOB;
                lds_dma16(A + (uint32_t)(LR * i * KC * 16), rsA, (int)vo, 0);
            }
            cc_l += KC;
            if (p.cpt >= KC) {                       // at most one tap boundary per k-step: branch-free
                const bool wrap = cc_l >= p.cpt;
                cc_l -= wrap ? p.cpt : 0;
                tap_l += wrap ? 1 : 0;
            } else {
                while (cc_l >= p.cpt) { cc_l -= p.cpt; ++tap_l; }
            }
        }
        if (p.remap) {
#pragma unroll
            for (int i = 0; i < PB; ++i)
                lds_dma16(B + (uint32_t)(LR * i * KC * 16), rsB, voffB[i] + remapB, 0);
        } else {
            const int soffB = p.korder ? korderB : ks * KC * 16;
#pragma unroll
            for (int i = 0; i < PB; ++i)
                lds_dma16(B + (uint32_t)(LR * i * KC * 16), rsB, voffB[i], soffB);
        }
    };

    f32x4 acc[TI][TJ];
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int frow = lane & 15, fchunk = lane >> 4;
    auto compute = [&](int cur) {
        const u32x4* A = smem + cur * BUF;
        const u32x4* B = A + BM * KC;
#pragma unroll
        for (int kk = 0; kk < KCS / 4; ++kk) {
            u32x4 wf[TI], xf[TJ];
#pragma unroll
            for (int i = 0; i < TI; ++i) wf[i] = B[lds_slot(wn * (BN / WN) + i * 16 + frow, kk * 4 + fchunk)];
#pragma unroll
            for (int j = 0; j < TJ; ++j) xf[j] = A[lds_slot(wm * (BM / WM) + j * 16 + frow, kk * 4 + fchunk)];
#pragma unroll
            for (int i = 0; i < TI; ++i)
#pragma unroll
                for (int j = 0; j < TJ; ++j) Mma<T>::run(wf[i], xf[j], acc[i][j]);
        }
    };

    constexpr int NDMA = PA + PB;                                  // wave-level DMAs per stage per wave (issued unconditionally)
    static_assert((NS - 2) * NDMA <= 63, "vmcnt field");
    if constexpr (FASTK) {
        static_assert(!MULTI && NS == 2 && PA == 2, "FASTK: 128-pixel tiles whose loader covers 64 rows per pass, double-buffered");
        static_assert(!LANEK || KCS == 8, "LANEK: 8-chunk k-steps");
        // scalar walk over k-steps: ks -> (channel chunk ks / ntaps, tap ks % ntaps); td = byte delta of the tap, fa / fb = scalar byte
        // offsets of the step inside a pixel's channels / inside a packed filter row
        int tap = ks_begin % ntaps, tr = (tap * inv_kw) >> 16, tc = tap - tr * p.kw;
        int td = tr * dA + tc * dB;
        int fa = (ks_begin / ntaps) * KC * 16, fb = (tap * p.cpt) * 16 + fa;
        const int tap_row_wrap = dA - p.kw * dB, cpt16 = p.cpt * 16;
        unsigned pixq[PA];
#pragma unroll
        for (int i = 0; i < PA; ++i) pixq[i] = (unsigned)(pixoff[i] + cq * 16);
        unsigned va[PA];
        int soffA = 0, soffB = 0;
        const bool knockA = DIN_KNOCK(p.flags, 0x200);
        if (DIN_KNOCK(p.flags, 0x400)) {
#pragma unroll
            for (int i = 0; i < PB; ++i) voffB[i] = (int)OOB;
        }
        // LANEK: this lane's chunk of the flattened (tap, channel-chunk) axis at the walk's current step
        [[maybe_unused]] int tap_v = (ks_begin * KC + cq) / p.cpt, cc_v = (ks_begin * KC + cq) - tap_v * p.cpt;
        if constexpr (LANEK) fb = ks_begin * KC * 16;
        auto prepare = [&]() {                                     // offsets of the transfer for the walk's current step, then advance it
            if constexpr (LANEK) {
                const int r = (tap_v * inv_kw) >> 16;
                const int tdv = r * dA + (tap_v - r * p.kw) * dB + cc_v * 16;
                const unsigned bit = tap_v < ntaps ? (1u << tap_v) : 0u;         // (past the last tap: zeros; the bank's rows are padded to whole k-steps)
#pragma unroll
                for (int i = 0; i < PA; ++i) va[i] = ((vmask[i] & bit) && !knockA) ? (unsigned)(pixoff[i] + tdv) : OOB;
                soffA = 0; soffB = fb;
                fb += KC * 16;
                cc_v += KC;
                const bool wrap = cc_v >= p.cpt;                                 // cpt >= 8 (host): at most one tap boundary per k-step
                cc_v -= wrap ? p.cpt : 0;
                tap_v += wrap ? 1 : 0;
                return;
            }
            const unsigned bit = 1u << tap;
#pragma unroll
            for (int i = 0; i < PA; ++i) va[i] = ((vmask[i] & bit) && !knockA) ? pixq[i] + (unsigned)td : OOB;
            soffA = fa; soffB = fb;
            ++tap; ++tc; td += dB; fb += cpt16;
            if (tc == p.kw) { tc = 0; td += tap_row_wrap; }
            if (tap == ntaps) { tap = 0; td = 0; fa += KC * 16; fb = fa; }
        };
        if (ks_begin < ks_end) {
            prepare();
            lds_dma_stage<PA, PB, LR * KC * 16>(ldsA0, rsA, va, soffA, rsB, voffB, soffB);
            prepare();
            int cur = 0;
#if DIN_GATHER_ILV
            // In-wave schedule of a k-step (round 3, late): the compiler's own placement of compute() kept ONE fragment of lookahead
            // (ds_read x2 -> s_waitcnt lgkmcnt -> 2 MFMAs: twelve exposed LDS latencies per k-step) behind five back-to-back transfer
            // issues that stall the wave while the CU's vector-memory path drains the other seven waves' transfers.  Here: the fragments
            // of half-step 0 are requested first, the next stage's transfers and the fragment reads of half-step 1 sit one per MFMA between
            // the MFMAs of half-step 0 (pinned with sched_barrier; a second fragment register set, ~10 fragments live at the peak).
            // Same operands, same accumulation order: bit-identical results.
            auto step = [&](auto more_t) {
                constexpr bool MORE = decltype(more_t)::value;
                const u32x4* A = smem + cur * BUF;
                const u32x4* B = A + BM * KC;
                const uint32_t nx = ldsA0 + (uint32_t)((cur ^ 1) * BUF * 16);
                constexpr int NKK = KCS / 4, NMF = TI * TJ;
                u32x4 xf[2][TJ], wf[2][TI];
                auto rd = [&](int set, int kk, int f) {                  // fragment f of half-step kk: pixel rows first, then filter rows
                    if (f < TJ) xf[set][f] = A[lds_slot(wm * (BM / WM) + f * 16 + frow, kk * 4 + fchunk)];
                    else wf[set][f - TJ] = B[lds_slot(wn * (BN / WN) + (f - TJ) * 16 + frow, kk * 4 + fchunk)];
                };
#pragma unroll
                for (int f = 0; f < TI + TJ; ++f) rd(0, 0, f);
                __builtin_amdgcn_sched_barrier(0);
#if DIN_GATHER_PRIO
                __builtin_amdgcn_s_setprio(1);
#endif
#pragma unroll
                for (int kk = 0; kk < NKK; ++kk) {
                    const int set = kk & 1;
                    const int ndma = (kk == 0 && MORE) ? NDMA : 0, nrd = (kk + 1 < NKK) ? TI + TJ : 0;
                    const int nitems = ndma + nrd, per = (nitems + NMF - 1) / NMF;
#pragma unroll
                    for (int mf = 0; mf < NMF; ++mf) {
                        Mma<T>::run(wf[set][mf / TJ], xf[set][mf % TJ], acc[mf / TJ][mf % TJ]);
#pragma unroll
                        for (int q = 0; q < per; ++q) {
                            const int it = mf * per + q;
                            if (it < ndma) {
                                if (it < PA) lds_dma16(nx + (uint32_t)(it * LR * KC * 16), rsA, (int)va[it < PA ? it : 0], soffA);
                                else lds_dma16(nx + (uint32_t)(it * LR * KC * 16), rsB, voffB[it >= PA ? it - PA : 0], soffB);
                            } else if (it < nitems) rd(set ^ 1, kk + 1, it - ndma);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
#if DIN_GATHER_PRIO
                __builtin_amdgcn_s_setprio(0);
#endif
            };
            // the last k-step (nothing left to request) is peeled: two accumulating variants merging inside one loop body cost a copy of
            // every accumulator per k-step and 192 VGPRs
            for (int ks = ks_begin; ks + 1 < ks_end; ++ks) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                if (DIN_KNOCK(p.flags, 0x800)) lds_dma_stage<PA, PB, LR * KC * 16>(ldsA0 + (uint32_t)((cur ^ 1) * BUF * 16), rsA, va, soffA, rsB, voffB, soffB);
                else step(std::true_type{});
                prepare();
                cur ^= 1;
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            if (!DIN_KNOCK(p.flags, 0x800)) step(std::false_type{});
#else
            for (int ks = ks_begin; ks < ks_end; ++ks) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                if (ks + 1 < ks_end) lds_dma_stage<PA, PB, LR * KC * 16>(ldsA0 + (uint32_t)((cur ^ 1) * BUF * 16), rsA, va, soffA, rsB, voffB, soffB);
                if (!DIN_KNOCK(p.flags, 0x800)) compute(cur);
                prepare();
                cur ^= 1;
            }
#endif
        }
    } else
    if (ks_begin < ks_end) {
#pragma unroll
        for (int s0 = 0; s0 < NS - 1; ++s0)
            if (ks_begin + s0 < ks_end) issue_dma(s0, ks_begin + s0);
        int cur = 0, nxt = NS - 1;                                 // stage of ks / stage the next DMA goes to
        for (int ks = ks_begin; ks < ks_end; ++ks) {
            // stage ks must have landed; younger stages (at most NS-2, fewer at the tail) may stay in flight
            int younger = ks_end - 1 - ks;
            if (younger > NS - 2) younger = NS - 2;
            if constexpr (NS >= 4) { if (younger >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NDMA) : "memory"); }
            if constexpr (NS >= 3) { if (younger == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(1 * NDMA) : "memory"); }
            if (younger <= 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");                       // LDS contents changed behind the compiler's back
            if (ks + NS - 1 < ks_end) issue_dma(nxt, ks + NS - 1);
            compute(cur);
            cur = cur + 1 == NS ? 0 : cur + 1;
            nxt = nxt + 1 == NS ? 0 : nxt + 1;
        }
    }
    __syncthreads();                                                // all waves done with the stages: the epilogue reuses them

    // ---- epilogue ---------------------------------------------------------------------------------------------
    const bool aligned = (p.Cout % EPC == 0) && (p.cooff % EPC == 0) && (p.ldo % EPC == 0) &&
                         (!(p.flags & DIN_CONV_MASK) || ((p.ldm % EPC == 0) && (p.moff % EPC == 0)));
    if (p.splitk > 1 || !aligned) {
        epilogue_direct<T, TI, TJ, BN, BM, WM, WN>(p, acc, co_tile, px_tile, wm, wn, lane, split);
        return;
    }
    {
        const int co_l = wn * (BN / WN) + (lane >> 4) * 4;         // channel inside the tile
        const int px_l = wm * (BM / WM) + (lane & 15);
#pragma unroll
        for (int i = 0; i < TI; ++i) {
            f32x4 bv = {0.f, 0.f, 0.f, 0.f};
            const int co = co_tile * BN + co_l + i * 16;
            const bool cooked = p.craw <= 0 || co < p.craw;             // (craw is a multiple of 4: uniform over the lane's 4 channels)
            if ((p.flags & DIN_CONV_BIAS) && co < p.Cout && cooked) bv = *reinterpret_cast<const f32x4*>(p.bias + co);   // Cout % 4 == 0 here
#pragma unroll
            for (int j = 0; j < TJ; ++j) {
                f32x4 v = acc[i][j] + bv;
                if ((p.flags & DIN_CONV_RELU) && cooked) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
                }
                unsigned char* dst = smem_raw + (px_l + j * 16) * CPITCH + (co_l + i * 16) * (int)sizeof(T);
                if constexpr (sizeof(T) == 4) *reinterpret_cast<f32x4*>(dst) = v;
                else *reinterpret_cast<u32x2*>(dst) = u32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
            }
        }
    }
    staged_tile_store<T, BM, BN, NT>(p, smem_raw, tid, co_tile, m_first);
#endif
}

// split-K finish: out = epilogue(sum_s partial[s])
template <typename T>
__global__ void conv_splitk_finish_kernel(ConvK p, int cpad) {
    int64_t total = (int64_t)p.M * p.Cout;
    T* __restrict__ outp = reinterpret_cast<T*>(p.out);
    const T* __restrict__ maskp = reinterpret_cast<const T*>(p.mask);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int m = (int)(i / p.Cout), co = (int)(i - (int64_t)m * p.Cout);
        float x = 0.f;
        for (int s = 0; s < p.splitk; ++s) x += p.partial[((int64_t)s * p.M + m) * cpad + co];
        if (p.flags & DIN_CONV_BIAS) x += p.bias[co];
        if (p.flags & DIN_CONV_RELU) x = fmaxf(x, 0.f);
        const int64_t opx = out_pixel(p, m);
        if (p.flags & DIN_CONV_MASK) {
            float y = Elem<T>::ld(maskp + opx * p.ldm + p.moff + co);
            x = y > 0.f ? x : 0.f;
        }
        int64_t o = opx * p.ldo + p.cooff + co;
        if (p.flags & DIN_CONV_ACCUM) x += Elem<T>::ld(outp + o);
        Elem<T>::st(outp + o, x);
    }
}

// ---- host-side planning ----------------------------------------------------------------------------

struct GatherPlan { int bm, bn, n_co_tiles, n_px_tiles, cpt, Q, nk, splitk, ks_per_split, cout_pad; int64_t ws_bytes; };

// geometry of a gather launch whose reduction runs over `cred` channels x taps and produces `cprod` channels
// retile: choose_gather will move the launch to the generic kernel (more than 32 taps, a strided dgrad not split by parity)
GatherPlan plan_gather(int M, int cred, int cprod, int taps, int dtype, bool strided_out = false, bool retile = false) {
    GatherPlan g;
    int epc = epc_of(dtype);
    g.cpt = pad_to(cred, epc) / epc;
    g.Q = taps * g.cpt;
    g.nk = (g.Q + KC - 1) / KC;
    g.bn = cprod <= 64 ? 64 : 128;
    g.bm = 128;
    if (cprod > 64 && !(DIN_OPT("DIN_CONV_BN") && atoi(DIN_OPT("DIN_CONV_BN")) == 128)) {
        // filter-tile width in {96,128,160,192}: least padded filters, ties to the wider tile (fewer re-reads of the pixel tile).
        // Inception's 96/160/192/288/384-filter layers otherwise waste 25-37 % of a 128-wide tile.
        // fewest filter tiles first (each tile re-reads the pixel tile), then least padding
        int best = 128, best_tiles = (cprod + 127) / 128, best_pad = best_tiles * 128;
        const int cands[3] = {96, 160, 192};
        for (int ci = 0; ci < 3; ++ci) {
            int bnc = cands[ci], tl = (cprod + bnc - 1) / bnc, pad = tl * bnc;
            if (tl < best_tiles || (tl == best_tiles && pad < best_pad)) { best = bnc; best_tiles = tl; best_pad = pad; }
        }
        g.bn = best;
        if (const char* fb = DIN_OPT("DIN_CONV_BN")) { const int v = atoi(fb); if (v == 96 || v == 128 || v == 160 || v == 192 || v == 256) g.bn = v; }   // tuning / test override
        // parity classes of a strided dgrad write every other pixel of dX: each tile's epilogue is a scattered write, and more, narrower
        // tiles per CU overlap it better -- 3 x 96 beats 2 x 160 on the 288-channel stride-2 dgrad (1642 -> 1427 us)
        if (strided_out && g.bn == 160 && cprod % 96 == 0) g.bn = 96;
    }
    // Tile choice (measured on MI355X, tools/conv_bench.py).  The L2->CU operand stream limits the 128x128
    // tile to ~770 TFLOP/s (64 FLOP per byte pulled from L2):
    //   64-filter launches over many pixels              -> 256x64  (256 threads, 2 workgroups / CU: 2x work per barrier)
    //   bf16, filters fill 256-wide tiles, long reduction -> 256x256 (512 threads, 128 FLOP/B; +12..16 % on VGG conv3/conv4)
    //   everything else                                   -> 128x128 / 128x64 at 2 workgroups / CU (a 256x128 tile at one
    //                                                        workgroup / CU measured 8..25 % SLOWER: no prologue/epilogue overlap)
    g.nk = (taps * g.cpt + KC - 1) / KC;
    const int64_t tiles256 = ((int64_t)M + 255) / 256;
    const char* force = DIN_OPT("DIN_CONV_TILE");
    if (g.bn == 64) {
        // fp32: 256x64 (4 waves, 2 workgroups / CU).  bf16: 128x64 on 8 waves measured +6..14 % on the 1x1 / dgrad launches, -2.5 % on the
        // 5x5 forward (DIN_CONV_TILE=256 restores 256x64)
        if (M >= 256 * 1024 && (dtype == DIN_F32 || (force && atoi(force) == 256))) g.bm = 256;
    } else if (!(force && atoi(force) == 128)) {
        const int nco256 = (cprod + 255) / 256;
        if (dtype == DIN_BF16 && cprod >= 224 && nco256 * 256 * 100 <= cprod * 115 && g.nk >= 24 && tiles256 * nco256 >= 768) { g.bm = 256; g.bn = 256; }
        else if (dtype == DIN_BF16 && force && atoi(force) == 256 && tiles256 >= 512) g.bm = 256;      // experiment: 256 x {96..192}
    }
    g.cout_pad = pad_to(cprod, 128);
    g.n_co_tiles = (cprod + g.bn - 1) / g.bn;
    g.n_px_tiles = (M + g.bm - 1) / g.bm;
    // split-K only when the launch cannot fill the chip and the reduction is long
    int tiles = g.n_co_tiles * g.n_px_tiles;
    g.splitk = 1;
    if (tiles < 192 && g.nk >= 8) {
        int want = (512 + tiles - 1) / tiles;
        int maxs = g.nk / 2;
        g.splitk = want < maxs ? want : maxs;
        if (g.splitk < 1) g.splitk = 1;
        if (g.splitk > 64) g.splitk = 64;
    }
    g.ks_per_split = (g.nk + g.splitk - 1) / g.splitk;
    if (g.ks_per_split < 1) g.ks_per_split = 1;                    // nk == 0: launch still runs its epilogue (zeros / accumulate)
    g.splitk = g.nk > 0 ? (g.nk + g.ks_per_split - 1) / g.ks_per_split : 1;
    // partial sums: [splitk][M][filter tiles x tile].  A launch that leaves the buffer-addressed kernels is re-tiled by choose_gather to 128
    // filters and writes rows of that width (a 72-filter 7x7 launch planned on a 96-filter tile wrote 128-filter rows past a workspace
    // sized for 96); every other plan keeps its own tile's width (a split 256-pixel plan falls back to 128 filters: never wider)
    const int ws_cols = (retile && g.bn != 64 && g.bn != 128) ? g.cout_pad : g.n_co_tiles * g.bn;
    g.ws_bytes = g.splitk > 1 ? (int64_t)g.splitk * M * ws_cols * 4 : 0;
    return g;
}

}  // namespace

int din_conv::check_desc(const din_conv_desc* d) {
    DIN_REQUIRE(d != nullptr, "conv: null descriptor");
    DIN_REQUIRE(d->dtype == DIN_F32 || d->dtype == DIN_BF16, "conv: bad dtype %d", d->dtype);
    int epc = epc_of(d->dtype);
    DIN_REQUIRE(d->nb > 0 && d->h > 0 && d->w > 0 && d->cin > 0 && d->cout > 0, "conv: empty tensor");
    DIN_REQUIRE(d->ldi % epc == 0 && d->cioff % epc == 0, "conv: input pixel stride/offset must be multiples of %d", epc);
    DIN_REQUIRE(d->ldo % 4 == 0 && d->cooff % 4 == 0, "conv: output pixel stride/offset must be multiples of 4");
    // operands are read in whole 16-byte chunks: a channel count that is not a chunk multiple must be followed by
    // finite (zero) padding inside the pixel stride -- the packed filters hold zeros there
    DIN_REQUIRE(d->ldi >= d->cioff + pad_to(d->cin, epc), "conv: ldi %d too small for cin %d (+pad)", d->ldi, d->cin);
    DIN_REQUIRE(d->ldo >= d->cooff + d->cout, "conv: ldo too small");
    int eoh = (d->h + 2 * d->ph - d->dh * (d->kh - 1) - 1) / d->sh + 1;
    int eow = (d->w + 2 * d->pw - d->dw * (d->kw - 1) - 1) / d->sw + 1;
    DIN_REQUIRE(eoh == d->oh && eow == d->ow, "conv: output size %dx%d inconsistent (expected %dx%d)", d->oh, d->ow, eoh, eow);
    DIN_REQUIRE((int64_t)d->nb * d->h * d->w < (1ll << 31) && (int64_t)d->nb * d->oh * d->ow < (1ll << 31), "conv: too many pixels");
    DIN_REQUIRE(d->in_u8 == 0 || d->in_u8 == 1, "conv: in_u8 must be 0 or 1");
    return DIN_OK;
}

namespace {

template <typename T, int BMT, int BN, int WM, int WN, int KCS, int NS, bool MULTI, bool FASTK, bool XSRC, bool LANEK>
void launch_fast(const ConvK& k, dim3 grid, hipStream_t st) {
    constexpr int LR_ = 64 * WM * WN / KCS, BNP_ = (BN + LR_ - 1) / LR_ * LR_;       // filter rows padded to whole loader passes
    size_t stage = (size_t)NS * (BMT + BNP_) * KCS * 16 + (k.remap ? 128 : 0);   // stage ring (+ remap table)
    // a single k-step (1x1 layers with <= 64 input channels: Conv2d_3b, the 64-channel dgrads) only ever touches ring stage 0: ask for one
    // stage, so that more of these memory-bound workgroups are resident per CU and their loads / stores overlap (DIN_CONV_ONESTAGE=0: off)
    const bool one_stage_ok = !MULTI && !(DIN_OPT("DIN_CONV_ONESTAGE") && atoi(DIN_OPT("DIN_CONV_ONESTAGE")) == 0);
    if (one_stage_ok && !k.remap && k.xsteps == 0 && k.ks_per_split * (8 / KCS) <= 1) stage = (size_t)(BMT + BNP_) * KCS * 16;
    size_t epi = (size_t)BMT * (BN * sizeof(T) + 16);
    size_t lds = stage > epi ? stage : epi;
    auto kern = conv_gather_fast_kernel<T, BMT, BN, WM, WN, KCS, NS, MULTI, FASTK, XSRC, LANEK>;
    if (lds > 65536) raise_lds_limit(kern, lds);
    hipLaunchKernelGGL(kern, grid, dim3(64 * WM * WN), lds, st, k);
}

// ---- kernel selection of a forward / data-gradient launch: decided ONCE, in choose_gather ------------
// run_gather and din_conv1x1_dgrad_multi launch what it returns; din_conv_kernel_tile / din_conv_kernel_variant report what it returns.
enum GatherFamily { GATHER_REGW, GATHER_STREAM, GATHER_HALO, GATHER_SMALL, GATHER_PIPE, GATHER_GENERIC, GATHER_TILE };
// conv_gather_fast_kernel<T, BM, BN, WM, WN, KCS, NS, MULTI, FASTK, XSRC, LANEK>
struct TileInst { int bm, bn, wm, wn, kcs, ns; bool multi, fastk, xsrc, lanek; };
using din_gather::HaloPlan;
using din_gather::SmallVariant;
struct GatherChoice {
    GatherFamily family;
    GatherPlan g;               // the plan after the 256 -> 128 pixel fallbacks (bm, bn, n_px_tiles, n_co_tiles)
    int korder;                 // ConvK::korder of the launch
    int n_co_tiles;             // ConvK::n_co_tiles of the launch (the halo kernel counts its own filter tiles)
    int bn;                     // filter tile of the chosen kernel (regw: filters per class)
    TileInst tile;              // GATHER_TILE (GATHER_GENERIC: bm, bn only)
    HaloPlan halo;              // GATHER_HALO
    SmallVariant small;         // GATHER_SMALL
};

// the plan fields of a chosen launch, written into its argument block
static void set_plan_fields(ConvK& k, const GatherChoice& c) {
    if (k.nsrc == 0) { k.cpt = c.g.cpt; k.Q = c.g.Q; k.nk = c.g.nk; if (!k.remap) k.wld = c.g.nk * KC; }    // (a multi-source launch lays its reduction out itself)
    k.korder = c.korder; k.splitk = c.g.splitk; k.ks_per_split = c.g.ks_per_split; k.n_co_tiles = c.n_co_tiles;
}

// the instantiation of the 128- / 256-pixel tile kernel for a launch whose plan fields are set
static TileInst choose_tile(const ConvK& k, int bm, int bn, int dtype) {
    const bool bf16 = dtype == DIN_BF16;
    const int taps = k.kh * k.kw;
    // ring geometry per tile, from A/B runs of tools/conv_bench.py (DIN_CONV_PIPE=0/1 switches the alternatives; 4 / 8: four / eight waves):
    //   256x64  : 4 stages x 4 chunks (80 KiB)  -- short-K, latency-bound launches gain 9 % from the deeper ring
    //   others  : 2 stages x 8 chunks           -- MFMA-dense tiles lose 8-10 % when the stage (and the barrier interval) is halved
    const int pipe = opt_int(DIN_OPT("DIN_CONV_PIPE"), -1);
    TileInst t{bm, bn, 2, 2, 8, 2, k.nsrc > 0, false, false, false};
    auto shape = [&](int wm, int wn, int kcs, int ns) { t.wm = wm; t.wn = wn; t.kcs = kcs; t.ns = ns; };
    if (t.multi) {      // 8 waves (bf16) where the filter tile is whole 64-row loader passes
        if (bn != 64 && bn != 96 && bn != 160 && bn != 192) t.bn = 128;
        if (bf16 && (t.bn % 64 == 0 || pipe == 8) && pipe != 4) shape(4, 2, 8, 2);
        return t;
    }
    // the scalar-walk specialisation (FASTK) whenever the launch qualifies: bf16 8- / 16-wave tiles, whole k-steps per tap, no tap remap,
    // taps-inside-chunks k-order or a single tap; DIN_CONV_FASTK=0 keeps the general loop
    const bool fastk_on = opt_int(DIN_OPT("DIN_CONV_FASTK"), 1) != 0;
    const bool fastk = fastk_on && !k.remap && k.nsrc == 0 && (k.cpt % 8) == 0 && (k.korder || taps == 1);
    // the per-lane k-walk (LANEK) serves: bf16 8-wave 128-pixel tiles, single source, no tap remap, tap-major k-order, reduction channels that
    // are NOT whole k-steps per tap but at least one k-step wide (so a k-step crosses at most one tap boundary).
    // measured (tools/ab_lanek.sh, profiles/r06_lanek.txt): forward launches +4..7 % (Conv2d_4a 1929 -> 1858 us, the 160-channel 7-tap layers
    // 165 -> 155 us); data gradients (ReLU mask / accumulate operands in the epilogue, the register file full) 1-2 % SLOWER: forward only
    // unless DIN_CONV_LANEK=2
    const int lmode = opt_int(DIN_OPT("DIN_CONV_LANEK"), 1);
    const bool lanek = lmode != 0 && !(lmode == 1 && (k.flags & (DIN_CONV_MASK | DIN_CONV_ACCUM))) && fastk_on && !k.remap && k.nsrc == 0 &&
                       !k.korder && k.xsteps == 0 && (k.cpt % 8) != 0 && k.cpt >= 8 && taps > 1 && taps <= 31;
#ifdef DIN_EXPERIMENTS
    // DIN_CONV_WG3=1: four waves on a 4-chunk stage at three workgroups per CU; DIN_CONV_RING=3: three 32-deep stages (two in flight, one counted
    // vmcnt per barrier) instead of two 64-deep ones for the general loop's 8-wave tiles -- same LDS budget (72 vs 80 KiB per workgroup), half
    // the MFMAs per barrier; DIN_CONV_W16=1 with DIN_CONV_TILE=256: the 256-pixel sixteen-wave tile for the 128- / 160- / 192-filter layers
    // (Mixed_6b-6d: 98 / 85 instead of 71 / 64 FLOP per staged byte; ONE filter stage per 256 pixels)
    const bool wg3 = opt_int(DIN_OPT("DIN_CONV_WG3"), 0) == 1, ring3 = opt_int(DIN_OPT("DIN_CONV_RING"), 0) == 3, w16 = opt_int(DIN_OPT("DIN_CONV_W16"), 0) == 1;
#else
    constexpr bool wg3 = false, ring3 = false, w16 = false;
#endif
    // 8-wave 128 x BN tile (4 x 2, four waves per SIMD at two workgroups per CU) -- same LDS ring, more waves to hide the stage waits:
    // +8..12 % on the 7-tap layers, +24 % on thin-K dgrads (bf16 only; DIN_CONV_PIPE=4 restores the 4-wave form)
    auto wave8 = [&]() {
        // 128 x 192: wave grid 2 x 4 (64 pixels x 48 filters per wave: 4 + 3 fragments per 12 MFMAs) instead of 4 x 2 (32 x 96: 2 + 6): an eighth
        // fewer LDS fragment reads for the same tile (experiment switch DIN_CONV_WAVEGRID=24)
        if (bn == 192 && opt_int(DIN_OPT("DIN_CONV_WAVEGRID"), 0) == 24) { shape(2, 4, 8, 2); t.fastk = fastk; }
        else if (bn >= 128 && fastk && wg3) { shape(2, 2, 4, 2); t.fastk = true; }
        else if (fastk) { shape(4, 2, 8, 2); t.fastk = true; }
        else if (lanek) { shape(4, 2, 8, 2); t.fastk = t.lanek = true; }
        else if ((bn == 192 || bn == 160) && ring3 && !k.remap) shape(4, 2, 4, 3);
        else shape(4, 2, 8, 2);
    };
    if (bm == 256 && bn == 64) { if (pipe != 0) shape(4, 1, 4, 4); else shape(4, 1, 8, 2); }
    else if (bm == 256 && bn == 256) { if (pipe == 1) shape(4, 2, 4, 4); else shape(4, 2, 8, 2); }
    else if (bm == 256) {                                                   // (bf16 only: plan_gather)
        if (bn == 96 || (bn == 160 && !w16)) shape(2, 2, 8, 2);
        else if (w16) { shape(8, 2, 8, 2); t.fastk = fastk; }
        else if (bn == 192) shape(4, 2, 8, 2);
        else { t.bn = 128; if (pipe == 1) shape(4, 2, 4, 4); else shape(4, 2, 8, 2); }
    }
    else if (bn == 64) { if (pipe == 1) shape(2, 2, 8, 3); else if (pipe != 4 && bf16) wave8(); }
    // 128 x 96: four waves (eight measured 5-14 % slower on Conv2d_3b) -- except the parity classes of a strided dgrad, whose scattered,
    // epilogue-bound tiles gain 5 % from eight waves (Mixed_6a.branch3x3 dgrad 1379 -> 1312 us)
    else if (bn == 96) {
        if (bf16 && k.xsteps > 0) { shape(4, 2, 8, 2); t.xsrc = true; }
        else if ((pipe == 8 || (k.remap && pipe != 4)) && bf16) shape(4, 2, 8, 2);
    }
    else if (bn == 160 || bn == 192) { if (pipe != 4 && bf16) wave8(); }
    else { t.bn = 128; if (pipe == 1) shape(2, 2, 4, 4); else if (pipe != 4 && bf16) wave8(); }
    return t;
}

// 256-pixel software-pipelined tiles (conv_gather_pipe.hip): bf16 launches with whole 32-channel blocks per tap whose filter tile the
// planner set to 128 / 192 / 256 and that still give every CU at least two tiles.  OPT-IN (DIN_GATHER_PIPE=1; 2 = also on small launches,
// used by the tests): measured against the 128-pixel 8-wave kernels at two workgroups per CU it is +5 % on the 7x1 forward but -2..-10 %
// on 1x1 / 1x7 forwards and on every dgrad (one workgroup per CU: no prologue / epilogue overlap; 64-byte instead of 128-byte gather
// segments per pixel), 520 vs 523 clips/s end to end (profiles/r02_gather_pipe_experiment.txt).
bool want_gather_pipe(int dtype, int64_t M, int cred, int taps, int bn, int splitk, int n_co_tiles) {
    const char* ev = DIN_OPT("DIN_GATHER_PIPE");
    const int mode = ev ? atoi(ev) : 0;
    if (!mode || dtype != DIN_BF16 || cred % 32 != 0 || taps > 32 || taps < 1 || splitk != 1 || !din_gather::gather_pipe_tile_ok(bn)) return false;
    const int64_t tiles = (M + 255) / 256 * n_co_tiles;
    return tiles >= (mode == 2 ? 1 : 512);
}

// Which kernel a launch runs on: geometry, flags and options only -- no pointer is read (ConvK::u8 only as "raw uint8 frames"), nothing is
// launched.  `k0` carries the geometry and flags of the launch, `g` its plan.  Precedence: regw, stream, halo (unless a stem shape), small,
// gather-pipe, then the tile kernels.
GatherChoice choose_gather(const ConvK& k0, GatherPlan g, int dtype) {
    GatherChoice c{};
    const bool fast = k0.divy == 1 && k0.divx == 1 && k0.kh * k0.kw <= 32;
    if (!fast && g.bn != 64 && g.bn != 128) { g.bn = 128; g.n_co_tiles = (k0.Cout + 127) / 128; }
    if (k0.nsrc > 0 && g.bn == 256) g.bn = 128;
    if (g.bm == 256 && (!fast || k0.remap || g.splitk > 1 || k0.nsrc > 0)) { g.bm = 128; if (g.bn == 256) g.bn = 128; }
    g.n_px_tiles = (k0.M + g.bm - 1) / g.bm; g.n_co_tiles = (k0.Cout + g.bn - 1) / g.bn;
    c.g = g; c.bn = g.bn; c.n_co_tiles = g.n_co_tiles;
    c.korder = (opt_int(DIN_OPT("DIN_CONV_KORDER"), 1) != 0 && fast && !k0.remap && g.splitk == 1 && (g.cpt % KC) == 0 && k0.kh * k0.kw > 1) ? 1 : 0;
    ConvK k = k0;                                          // (the eligibility rules below read the plan fields from the argument block)
    set_plan_fields(k, c);
    const bool single = !k.remap && k.nsrc == 0 && k.csplit == 0;
    if (fast && g.splitk == 1 && k.xsteps == 0) {
        // 1x1 layers with a 640..768-channel reduction over a large map (the Mixed_6 block entries): filters resident in registers (conv_regw.hip)
        if (din_gather::conv1x1_regw_eligible(k, dtype)) {
            int nks = 0;                                   // 32-channel k-steps as launch_conv1x1_regw counts them: <= 10 -> classes of 128 filters
            for (int s = 0; s < (k.nsrc > 0 ? k.nsrc : 1); ++s) nks += ((k.nsrc > 0 ? k.src[s].cpt : k.cpt) + 7) / 8 * 2;
            c.family = GATHER_REGW; c.bn = nks <= 10 ? 128 : 192;
            return c;
        }
        // 1x1 layers with a short reduction over a large map: persistent streaming kernel (conv_stream.hip)
        if (din_gather::conv1x1_stream_eligible(k, dtype)) { c.family = GATHER_STREAM; c.bn = din_gather::conv1x1_stream_tile(k.Cout); return c; }
    }
    // mid-network multi-tap layers: halo tiles + filter-slab ring (conv_halo.hip); the stem shapes keep their own kernel below
    const bool stem_shape = k.kh == 3 && k.kw == 3 && (k.Cin == 32 || k.Cin == 64) && k.Cout <= 64 && !(k.Cin == 64 && k.Cout > 32) && (int64_t)k.M >= 256 * 1024;
    if (fast && single && g.splitk == 1 && !stem_shape && k.ay == 1 && k.ax == 1 && (k.cy == 1 || k.cy == -1) && (k.cx == 1 || k.cx == -1) && k.cy == k.cx &&
        k.out_sy == 0 && k.ldi % 8 == 0 && k.cioff % 8 == 0 && k.ldo % 4 == 0 && k.cooff % 4 == 0 &&
        (!(k.flags & DIN_CONV_MASK) || (k.ldm % 4 == 0 && k.moff % 4 == 0)) && din_gather::views_below_2g(k) &&
        din_gather::plan_halo(dtype, k.kh, k.kw, k.Cin, k.Cout, k.OH, k.OW, k.M, c.halo)) {
        c.family = GATHER_HALO; c.bn = c.halo.bn; c.n_co_tiles = c.halo.n_co_tiles;
        return c;
    }
    // stem layers: stationary filters + halo tiles (conv_small.hip)
    if (din_gather::conv_small_variant(k, dtype, c.small)) { c.family = GATHER_SMALL; c.bn = c.small.bn; return c; }
    if (fast && !k.remap && k.nsrc == 0 && want_gather_pipe(dtype, k.M, k.Cin, k.kh * k.kw, g.bn, g.splitk, g.n_co_tiles) &&
        g.cpt % 4 == 0 && k.Cout % 8 == 0 && k.cooff % 8 == 0 && k.ldo % 8 == 0 && din_gather::mask_views_aligned8(k) &&
        (k.csplit == 0 || (k.csplit % 8 == 0 && k.ldo2 % 8 == 0 && k.cooff2 % 8 == 0))) {
        c.family = GATHER_PIPE;
        return c;
    }
    c.family = fast ? GATHER_TILE : GATHER_GENERIC;
    c.tile = fast ? choose_tile(k, g.bm, g.bn, dtype) : TileInst{128, g.bn == 64 ? 64 : 128, 2, 2, 8, 2, false, false, false, false};
    c.bn = c.tile.bn;
    return c;
}

// Every conv_gather_fast_kernel the library holds, X(BM, BN, WM, WN, KCS, NS, MULTI, FASTK, XSRC, LANEK): DIN_CONV_TILE_TABLE for every operand
// type (four waves, the general loop on eight, the multi-source forms), DIN_CONV_TILE_BF16_TABLE for bf16 alone (256-pixel tiles, the extra
// 1x1 source of din_conv_dgrad_x, the scalar and per-lane k-walks, the three-stage ring), DIN_CONV_TILE_EXPERIMENTS_TABLE (bf16) for what only
// an experiment switch of a -DDIN_EXPERIMENTS build reaches.  The generic kernel: X(BN), every operand type.
#define DIN_CONV_TILE_TABLE(X)                                                                                                          \
    X(256, 64, 4, 1, 4, 4, 0, 0, 0, 0) X(256, 64, 4, 1, 8, 2, 0, 0, 0, 0)                                                               \
    X(128, 64, 2, 2, 8, 3, 0, 0, 0, 0) X(128, 64, 2, 2, 8, 2, 0, 0, 0, 0) X(128, 96, 2, 2, 8, 2, 0, 0, 0, 0) X(128, 128, 2, 2, 4, 4, 0, 0, 0, 0) \
    X(128, 128, 2, 2, 8, 2, 0, 0, 0, 0) X(128, 160, 2, 2, 8, 2, 0, 0, 0, 0) X(128, 192, 2, 2, 8, 2, 0, 0, 0, 0)                         \
    X(128, 64, 4, 2, 8, 2, 0, 0, 0, 0) X(128, 96, 4, 2, 8, 2, 0, 0, 0, 0) X(128, 128, 4, 2, 8, 2, 0, 0, 0, 0) X(128, 160, 4, 2, 8, 2, 0, 0, 0, 0) \
    X(128, 192, 4, 2, 8, 2, 0, 0, 0, 0)                                                                                                 \
    X(128, 64, 4, 2, 8, 2, 1, 0, 0, 0) X(128, 64, 2, 2, 8, 2, 1, 0, 0, 0) X(128, 96, 4, 2, 8, 2, 1, 0, 0, 0) X(128, 96, 2, 2, 8, 2, 1, 0, 0, 0) \
    X(128, 128, 4, 2, 8, 2, 1, 0, 0, 0) X(128, 128, 2, 2, 8, 2, 1, 0, 0, 0) X(128, 160, 4, 2, 8, 2, 1, 0, 0, 0) X(128, 160, 2, 2, 8, 2, 1, 0, 0, 0) \
    X(128, 192, 4, 2, 8, 2, 1, 0, 0, 0) X(128, 192, 2, 2, 8, 2, 1, 0, 0, 0)
#define DIN_CONV_TILE_BF16_TABLE(X)                                                                                                     \
    X(256, 256, 4, 2, 4, 4, 0, 0, 0, 0) X(256, 256, 4, 2, 8, 2, 0, 0, 0, 0) X(256, 128, 4, 2, 4, 4, 0, 0, 0, 0) X(256, 128, 4, 2, 8, 2, 0, 0, 0, 0) \
    X(256, 96, 2, 2, 8, 2, 0, 0, 0, 0) X(256, 160, 2, 2, 8, 2, 0, 0, 0, 0) X(256, 192, 4, 2, 8, 2, 0, 0, 0, 0)                          \
    X(256, 192, 8, 2, 8, 2, 0, 0, 0, 0) X(256, 192, 8, 2, 8, 2, 0, 1, 0, 0)                                                             \
    X(128, 96, 4, 2, 8, 2, 0, 0, 1, 0)                                                                                                  \
    X(128, 192, 2, 4, 8, 2, 0, 0, 0, 0) X(128, 192, 2, 4, 8, 2, 0, 1, 0, 0)                                                             \
    X(128, 64, 4, 2, 8, 2, 0, 1, 0, 0) X(128, 128, 4, 2, 8, 2, 0, 1, 0, 0) X(128, 160, 4, 2, 8, 2, 0, 1, 0, 0) X(128, 192, 4, 2, 8, 2, 0, 1, 0, 0) \
    X(128, 64, 4, 2, 8, 2, 0, 1, 0, 1) X(128, 128, 4, 2, 8, 2, 0, 1, 0, 1) X(128, 160, 4, 2, 8, 2, 0, 1, 0, 1) X(128, 192, 4, 2, 8, 2, 0, 1, 0, 1) \
    X(128, 160, 4, 2, 4, 3, 0, 0, 0, 0) X(128, 192, 4, 2, 4, 3, 0, 0, 0, 0)
#ifdef DIN_EXPERIMENTS
#define DIN_CONV_TILE_EXPERIMENTS_TABLE(X)                                                                                              \
    X(256, 160, 8, 2, 8, 2, 0, 0, 0, 0) X(256, 160, 8, 2, 8, 2, 0, 1, 0, 0) X(256, 128, 8, 2, 8, 2, 0, 0, 0, 0) X(256, 128, 8, 2, 8, 2, 0, 1, 0, 0) \
    X(128, 128, 2, 2, 4, 2, 0, 1, 0, 0) X(128, 160, 2, 2, 4, 2, 0, 1, 0, 0) X(128, 192, 2, 2, 4, 2, 0, 1, 0, 0)
#else
#define DIN_CONV_TILE_EXPERIMENTS_TABLE(X)
#endif
#define DIN_CONV_GENERIC_TABLE(X) X(64) X(128)

// The table row of a chosen tile / generic kernel for operand type T: launched when `k` is given, only looked up otherwise.  false: no row.
template <typename T>
bool tile_row(const TileInst& t, const ConvK* k, dim3 grid, hipStream_t st) {
#define DIN_ROW(BM_, BN_, WM_, WN_, KCS_, NS_, MULTI_, FASTK_, XSRC_, LANEK_)                                                            \
    if (t.bm == BM_ && t.bn == BN_ && t.wm == WM_ && t.wn == WN_ && t.kcs == KCS_ && t.ns == NS_ && t.multi == (bool)MULTI_ &&          \
        t.fastk == (bool)FASTK_ && t.xsrc == (bool)XSRC_ && t.lanek == (bool)LANEK_) {                                                  \
        if (k) launch_fast<T, BM_, BN_, WM_, WN_, KCS_, NS_, MULTI_, FASTK_, XSRC_, LANEK_>(*k, grid, st);                               \
        return true;                                                                                                                    \
    }
    DIN_CONV_TILE_TABLE(DIN_ROW)
    if constexpr (sizeof(T) == 2) {
        DIN_CONV_TILE_BF16_TABLE(DIN_ROW)
        DIN_CONV_TILE_EXPERIMENTS_TABLE(DIN_ROW)
    }
#undef DIN_ROW
    return false;
}
template <typename T>
bool generic_row(int bn, const ConvK* k, dim3 grid, hipStream_t st) {
#define DIN_ROW(BN_)                                                                                                                     \
    if (bn == BN_) {                                                                                                                     \
        if (k) hipLaunchKernelGGL((conv_gather_generic_kernel<T, BN_>), grid, dim3(NTHREADS), 2 * (BM + 128) * KC * 16, st, *k);         \
        return true;                                                                                                                     \
    }
    DIN_CONV_GENERIC_TABLE(DIN_ROW)
#undef DIN_ROW
    return false;
}

// a GATHER_TILE / GATHER_GENERIC choice as the reporters spell its kernel (k: the argument block with its plan fields set)
std::string tile_kernel_name(const ConvK& k, const GatherChoice& c, int dtype) {
    const char* T = k.mma ? "f32x3" : dtype == DIN_F32 ? "float" : "bf16";
    const TileInst& t = c.tile;
    char s[160];
    if (c.family == GATHER_GENERIC) snprintf(s, sizeof s, "conv_gather_generic_kernel<%s,%d>", T, t.bn);
    else snprintf(s, sizeof s, "conv_gather_fast_kernel<%s,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d>", T, t.bm, t.bn, t.wm, t.wn, t.kcs, t.ns, (int)t.multi,
                  (int)t.fastk, (int)t.xsrc, (int)t.lanek);
    return s;
}

// ... and its table row, launched (launch_choice) or only looked up (append_kernel_names): a tuple without a row is an error from both
int tile_choice_row(const ConvK& k, const GatherChoice& c, int dtype, bool launch, hipStream_t st, const char* what) {
    const dim3 grid(c.g.n_px_tiles * k.n_co_tiles, k.splitk);
    const ConvK* kl = launch ? &k : nullptr;
    auto row = [&](auto tag) {
        using T = decltype(tag);
        return c.family == GATHER_TILE ? tile_row<T>(c.tile, kl, grid, st) : generic_row<T>(c.tile.bn, kl, grid, st);
    };
    if (k.mma ? row(f32x3_t{}) : dtype == DIN_F32 ? row(float{}) : row(bf16_t{})) return DIN_OK;
    DIN_FAIL(DIN_E_ARG, "%s: %s is not instantiated", what, tile_kernel_name(k, c, dtype).c_str());
}

// launches the chosen kernel on an argument block whose plan fields are set (set_plan_fields)
int launch_choice(ConvK& k, const GatherChoice& c, int dtype, hipStream_t st, const char* what) {
    switch (c.family) {
    case GATHER_REGW:
        if (din_gather::launch_conv1x1_regw(k, st)) DIN_FAIL(DIN_E_LAUNCH, "%s: conv1x1_regw launch failed", what);
        return DIN_OK;
    case GATHER_STREAM:
        if (din_gather::launch_conv1x1_stream(k, st)) DIN_FAIL(DIN_E_LAUNCH, "%s: conv1x1_stream launch failed", what);
        return DIN_OK;
    case GATHER_HALO:
        if (int e = din_gather::launch_conv_halo(k, c.halo, st)) return e;
        break;
    case GATHER_SMALL:
        if (int e = din_gather::launch_conv_small(k, c.small, st)) return e;
        break;
    case GATHER_PIPE:
        if (int e = din_gather::launch_gather_pipe(k, c.g.bn, (k.M + 255) / 256, st)) return e;
        break;
    case GATHER_GENERIC:
    case GATHER_TILE:
        if (int e = tile_choice_row(k, c, dtype, true, st, what)) return e;
        break;
    }
    DIN_CHECK_LAUNCH(what);
    return DIN_OK;
}

// choose, check the workspace, launch the chosen kernel, finish a split reduction
int run_gather(ConvK& k, GatherPlan g0, int dtype, void* workspace, int64_t ws_bytes, hipStream_t st, const char* what) {
    const GatherChoice c = choose_gather(k, g0, dtype);
    const GatherPlan& g = c.g;
    set_plan_fields(k, c);
    if (const char* eb = DIN_OPT("DIN_CONV_EPI_BATCH")) { if (atoi(eb) == 0) k.flags |= 0x100; }
    // timing experiments only (results are WRONG): DIN_GATHER_KNOCK bit 0 = the pixel-tile transfers of the scalar-walk loop fetch nothing
    // (all lanes out of range: issued, landed as zeros, no cache / HBM access), bit 1 = the same for the filter tile, bit 2 = no MFMA
    // -- only in -DDIN_EXPERIMENTS builds (conv_gather.h)
#ifdef DIN_EXPERIMENTS
    if (const char* kn = DIN_OPT("DIN_GATHER_KNOCK")) k.flags |= (atoi(kn) & 7) << 9;
#endif
    if (DIN_OPT("DIN_DEBUG_PLAN"))
        fprintf(stderr, "[din] %s M=%d NB=%d HxW=%dx%d Cin=%d Cout=%d k=%dx%d ay=%d cy=%d tile=%dx%d splitk=%d korder=%d remap=%d flags=%d dtype=%d family=%d\n", what,
                k.M, k.NB, k.H, k.W, k.Cin, k.Cout, k.kh, k.kw, k.ay, k.cy, g.bm, g.bn, g.splitk, k.korder, k.remap, k.flags, dtype, (int)c.family);
    if (k.csplit > 0 && (c.family == GATHER_GENERIC || g.splitk > 1)) DIN_FAIL(DIN_E_ARG, "%s: two destinations need the staged epilogue of the buffer-addressed kernel", what);
    if (g.splitk > 1) {
        // what the chosen (possibly re-tiled) kernel writes: never more than the plan reported, or the launch is refused
        const int64_t written = (int64_t)g.splitk * k.M * g.n_co_tiles * g.bn * 4;
        const int64_t need = written > g.ws_bytes ? written : g.ws_bytes;
        if (ws_bytes < need || workspace == nullptr)
            DIN_FAIL(DIN_E_WORKSPACE, "%s: workspace %lld < %lld bytes", what, (long long)ws_bytes, (long long)need);
        k.partial = reinterpret_cast<float*>(workspace);
    }
    DIN_REQUIRE(!k.u8 || c.family == GATHER_SMALL, "%s: in_u8 is only served by the image-layer kernel (see din_conv_accepts_u8)", what);
    if (int e = launch_choice(k, c, dtype, st, what)) return e;
    if (g.splitk > 1) {
        int64_t total = (int64_t)k.M * k.Cout;
        int cpad = g.n_co_tiles * g.bn;
        if (dtype == DIN_F32) hipLaunchKernelGGL(conv_splitk_finish_kernel<float>, dim3(grid_1d(total, 256)), dim3(256), 0, st, k, cpad);
        else hipLaunchKernelGGL(conv_splitk_finish_kernel<bf16_t>, dim3(grid_1d(total, 256)), dim3(256), 0, st, k, cpad);
        DIN_CHECK_LAUNCH(what);
    }
    return DIN_OK;
}

// ---- descriptor -> launch ------------------------------------------------------------------------------
// A strided data gradient is decomposed by output parity (py, px).  Class (py, px) only sees the taps r = r0 + sh*r', s = s0 + sw*s' with
// r0 = (py+ph) % sh: a stride-1 gather oy = a + (py+ph-r0)/sh - r' over the sub-grid y = sh*a + py -- no structurally zero taps are
// multiplied, and it runs on the fast (buffer-addressed) kernel.
struct ParityClass { int py, px, Ha, Wa, r0c, s0c, khs, kws; };
static bool dgrad_by_parity(const din_conv_desc* d) { return (d->sh > 1 || d->sw > 1) && d->dh == 1 && d->dw == 1 && d->kh * d->kw <= 32; }
// f(class) for every non-empty parity class; stops at the first non-zero return and hands it back
template <typename F>
static int for_each_parity_class(const din_conv_desc* d, F f) {
    for (int py = 0; py < d->sh; ++py)
        for (int px = 0; px < d->sw; ++px) {
            ParityClass pc{py, px, (d->h - py + d->sh - 1) / d->sh, (d->w - px + d->sw - 1) / d->sw, (py + d->ph) % d->sh, (px + d->pw) % d->sw, 0, 0};
            if (pc.Ha <= 0 || pc.Wa <= 0) continue;
            pc.khs = pc.r0c < d->kh ? (d->kh - pc.r0c + d->sh - 1) / d->sh : 0;
            pc.kws = pc.s0c < d->kw ? (d->kw - pc.s0c + d->sw - 1) / d->sw : 0;
            if (int e = f(pc)) return e;
        }
    return 0;
}

// plan of the launch `which` (0 forward, 1 data gradient; pc: one parity class of a strided data gradient)
static GatherPlan plan_launch(const din_conv_desc* d, int which, const ParityClass* pc = nullptr) {
    // (the launches choose_gather calls !fast: more than 32 taps, or a data gradient that divides by its stride)
    const bool retile = d->kh * d->kw > 32 || (which == 1 && !pc && (d->sh > 1 || d->sw > 1));
    if (which == 0) return plan_gather(d->nb * d->oh * d->ow, d->cin, d->cout, d->kh * d->kw, d->dtype, false, retile);
    if (!pc) return plan_gather(d->nb * d->h * d->w, d->cout, d->cin, d->kh * d->kw, d->dtype, false, retile);
    return plan_gather(d->nb * pc->Ha * pc->Wa, d->cout, d->cin, pc->khs * pc->kws, d->dtype, true);
}

// Geometry of that launch as the kernels' argument block; the caller adds pointers, flags and the mask view.
// The CANONICAL LAUNCH of a descriptor -- the one din_conv_kernel_tile / din_conv_kernel_variant report -- is:
//   forward        single destination, no dgrad flags;
//   data gradient  DIN_CONV_MASK without DIN_CONV_ACCUM, the mask view equal to the layer's input view (ldm = ldi, moff = cioff);
//   strided dgrad  parity class (0, 0) of the above.
static ConvK conv_k_of(const din_conv_desc* d, int which, const ParityClass* pc = nullptr) {
    const int esz = d->dtype == DIN_F32 ? 4 : 2;
    ConvK k{};
    k.NB = d->nb; k.kh = d->kh; k.kw = d->kw;
    const PackGeom bank = pack_geom(d, which);
    k.w_bytes = (long long)bank.rows_pad * bank.kelems * esz;
    if (which == 0) {
        k.H = d->h; k.W = d->w; k.Cin = d->cin; k.ldi = d->ldi; k.cioff = d->cioff;
        k.OH = d->oh; k.OW = d->ow; k.Cout = d->cout; k.ldo = d->ldo; k.cooff = d->cooff;
        k.ay = d->sh; k.by = -d->ph; k.cy = d->dh; k.divy = 1;
        k.ax = d->sw; k.bx = -d->pw; k.cx = d->dw; k.divx = 1;
        k.M = d->nb * d->oh * d->ow;
        k.in_bytes = (long long)d->nb * d->h * d->w * d->ldi * esz;
        if (d->in_u8) { k.ldi = 8; k.cioff = 0; k.in_bytes = (long long)d->nb * d->h * d->w * 16; }   // raw uint8 frames: plan as the 8-channel prepared tensor the image layer would read
        return k;
    }
    // the "input" of the gather is dout (geometry oh x ow x cout), the "output" is din (h x w x cin)
    k.H = d->oh; k.W = d->ow; k.Cin = d->cout; k.ldi = d->ldo; k.cioff = d->cooff;
    k.OH = d->h; k.OW = d->w; k.Cout = d->cin; k.ldo = d->ldi; k.cooff = d->cioff;
    k.in_bytes = (long long)d->nb * d->oh * d->ow * d->ldo * esz;
    if (!pc) {
        // y_in = oy*sh - ph + r*dh  =>  oy = (y_in + ph - r*dh) / sh
        k.ay = 1; k.by = d->ph; k.cy = -d->dh; k.divy = d->sh;
        k.ax = 1; k.bx = d->pw; k.cx = -d->dw; k.divx = d->sw;
        k.M = d->nb * d->h * d->w;
        return k;
    }
    const bool taps = pc->khs > 0 && pc->kws > 0;
    k.kh = taps ? pc->khs : 0; k.kw = taps ? pc->kws : 1;
    k.ay = 1; k.by = (pc->py + d->ph - pc->r0c) / d->sh; k.cy = -1; k.divy = 1;
    k.ax = 1; k.bx = (pc->px + d->pw - pc->s0c) / d->sw; k.cx = -1; k.divx = 1;
    k.OH = pc->Ha; k.OW = pc->Wa; k.M = d->nb * pc->Ha * pc->Wa;
    k.out_sy = d->sh; k.out_sx = d->sw; k.out_y0 = pc->py; k.out_x0 = pc->px; k.out_H = d->h; k.out_W = d->w;
    k.remap = 1; k.wld = bank.nk * KC;                                                                // rows of the full packed bank
    for (int rr = 0; rr < pc->khs; ++rr)
        for (int ss = 0; ss < pc->kws; ++ss) k.wtap[rr * pc->kws + ss] = (unsigned char)((pc->r0c + d->sh * rr) * d->kw + (pc->s0c + d->sw * ss));
    return k;
}

// what the canonical launch of a descriptor (conv_k_of) resolves to
static GatherChoice canonical_choice(const din_conv_desc* d, int which) {
    ParityClass first{};
    const bool parity = which == 1 && dgrad_by_parity(d) && for_each_parity_class(d, [&](const ParityClass& pc) { first = pc; return 1; });
    ConvK k = conv_k_of(d, which, parity ? &first : nullptr);
    if (which == 1) { k.flags = DIN_CONV_MASK; k.ldm = d->ldi; k.moff = d->cioff; }
    return choose_gather(k, plan_launch(d, which, parity ? &first : nullptr), d->dtype);
}


// The launches din_conv_fwd (which 0) / din_conv_dgrad (which 1) make for a descriptor, flags and mask view, in launch order:
// f(argument block without pointers, plan, what) per launch -- a strided data gradient: one per non-empty parity class.  The entry points
// bind their pointers and launch from here; din_conv_kernel_names names the kernels from here.
template <typename F>
static int for_each_launch(const din_conv_desc* d, int which, int flags, int ldm, int moff, F f) {
    if (which == 0) {
        ConvK k = conv_k_of(d, 0);
        k.flags = flags;
        return f(k, plan_launch(d, 0), "conv_fwd");
    }
    if (!dgrad_by_parity(d)) {
        ConvK k = conv_k_of(d, 1);
        k.flags = flags; k.ldm = ldm; k.moff = moff;
        return f(k, plan_launch(d, 1), "conv_dgrad");
    }
    return for_each_parity_class(d, [&](const ParityClass& pc) {
        ConvK c = conv_k_of(d, 1, &pc);
        c.flags = flags; c.ldm = ldm; c.moff = moff;
        return f(c, plan_launch(d, 1, &pc), "conv_dgrad(strided)");
    });
}

// the kernels launch_choice / run_gather launch for a choice, spelled as their instantiations: one line each, appended to `out`.
// k: the argument block with its plan fields set (set_plan_fields).  The halo, stem, tile and generic families answer from the table their
// launcher walks: a chosen tuple the library does not hold is the launcher's error here too.
static int append_kernel_names(const ConvK& k, const GatherChoice& c, int dtype, std::string& out) {
    char line[160];
    switch (c.family) {
    case GATHER_REGW: {
        const din_gather::RegwInst i = din_gather::conv1x1_regw_inst(k);
        snprintf(line, sizeof line, "conv1x1_regw_kernel<%d,%d,%d,%d,%d>\n", i.nks, (int)i.masked, i.ns, i.occ, i.rt);
        out += line;
        break;
    }
    case GATHER_STREAM: {
        const din_gather::StreamInst i = din_gather::conv1x1_stream_inst(k);
        snprintf(line, sizeof line, "conv1x1_stream_kernel<%d,%d,%d,%d,%d>\n", i.bn, i.nsw, (int)i.multi, (int)i.epi, (int)i.split);
        out += line;
        break;
    }
    case GATHER_HALO:
        if (int e = din_gather::append_conv_halo_name(k, c.halo, out)) return e;
        break;
    case GATHER_SMALL:
        if (int e = din_gather::append_conv_small_name(c.small, out)) return e;
        break;
    case GATHER_PIPE: snprintf(line, sizeof line, "conv_gather_pipe_kernel<%d>\n", c.g.bn); out += line; break;
    case GATHER_GENERIC:
    case GATHER_TILE:
        if (int e = tile_choice_row(k, c, dtype, false, nullptr, "conv_kernel_names")) return e;
        out += tile_kernel_name(k, c, dtype); out += '\n';
        break;
    }
    if (c.g.splitk > 1) { out += "conv_splitk_finish_kernel<"; out += dtype == DIN_F32 ? "float" : "bf16"; out += ">\n"; }     // (f32x3 reuses <float>)
    return DIN_OK;
}

// one launch as append_kernel_names spells it: choose, set the plan fields, append
static int append_launch_names(ConvK& k, const GatherPlan& g, int dtype, std::string& out) {
    const GatherChoice c = choose_gather(k, g, dtype);
    set_plan_fields(k, c);
    return append_kernel_names(k, c, dtype, out);
}

// The launch din_conv_fwd2 makes for a checked descriptor (dtype normalised, split: it was DIN_F32_BF16X3): every argument check that reads
// no pointer, then f(argument block without pointers, plan).  din_conv_fwd2 binds its pointers and launches from here;
// din_conv_fwd2_kernel_names names the kernel from here.
template <typename F>
static int for_fwd2_launch(const din_conv_desc* d, bool split, int ldo2, int cooff2, int csplit, int craw, int flags, F f) {
    DIN_REQUIRE(!d->in_u8, "conv_fwd2: in_u8 is a din_conv_fwd / din_conv_wgrad option");
    DIN_REQUIRE(!(flags & (DIN_CONV_ACCUM | DIN_CONV_MASK)), "conv_fwd2: ACCUM/MASK are dgrad-only flags");
    const int epc = epc_of(d->dtype);
    DIN_REQUIRE(d->kh * d->kw <= 32 && d->dh == 1 && d->dw == 1, "conv_fwd2: needs the buffer-addressed gather kernel (<= 32 taps)");
    DIN_REQUIRE(csplit > 0 && csplit < d->cout && csplit % epc == 0 && d->cout % epc == 0 && d->ldo % epc == 0 && d->cooff % epc == 0 &&
                ldo2 % epc == 0 && cooff2 % epc == 0 && ldo2 >= cooff2 + (d->cout - csplit) && d->ldo >= d->cooff + csplit,
                "conv_fwd2: split / strides / offsets must be multiples of %d and the destinations must hold their channel ranges", epc);
    DIN_REQUIRE(craw == 0 || (craw >= csplit && craw < d->cout && craw % epc == 0), "conv_fwd2: craw must be 0 or a multiple of %d in [csplit, cout)", epc);
    ConvK k = conv_k_of(d, 0);
    k.flags = flags; k.mma = split;
    k.ldo2 = ldo2; k.cooff2 = cooff2; k.csplit = csplit; k.craw = craw;
    const GatherPlan g = plan_launch(d, 0);
    if (g.splitk > 1) DIN_FAIL(DIN_E_ARG, "conv_fwd2: this shape runs split-K (%d pixels): launch the sibling convs separately", k.M);
    return f(k, g);
}

// The launch din_conv1x1_dgrad_multi makes: every argument check that reads no pointer (of a source: cout, ldo, cooff), the argument block
// without pointers, its plan and choice, then f(argument block with its plan fields set, choice, storage dtype).  din_conv1x1_dgrad_multi
// binds its pointers and launches from here; din_conv1x1_dgrad_multi_kernel_names names the kernel from here.
template <typename F>
static int for_multi_launch(int nsrc, const din_conv_src* srcs, int dtype, int nb, int h, int w, int cin, int ldi, int cioff, int ldm, int moff,
                            int flags, F f) {
    DIN_REQUIRE(nsrc >= 1 && nsrc <= 4 && srcs, "conv1x1_dgrad_multi: 1..4 sources");
    const bool split = dtype == DIN_F32_BF16X3;
    dtype = storage_dtype(dtype);
    DIN_REQUIRE(dtype == DIN_F32 || dtype == DIN_BF16, "conv1x1_dgrad_multi: bad dtype");
    DIN_REQUIRE(!(flags & (DIN_CONV_BIAS | DIN_CONV_RELU)), "conv1x1_dgrad_multi: BIAS/RELU are fwd-only flags");
    const int epc = epc_of(dtype), esz = dtype == DIN_F32 ? 4 : 2;
    DIN_REQUIRE(nb > 0 && h > 0 && w > 0 && cin > 0 && ldi % 4 == 0 && cioff % 4 == 0 && ldi >= cioff + cin, "conv1x1_dgrad_multi: bad output geometry");
    DIN_REQUIRE((int64_t)nb * h * w < (1ll << 31), "conv1x1_dgrad_multi: too many pixels");
    ConvK k{};
    k.NB = nb; k.H = h; k.W = w; k.OH = h; k.OW = w; k.Cout = cin; k.ldo = ldi; k.cooff = cioff;
    k.kh = k.kw = 1; k.ay = k.ax = 1; k.by = k.bx = 0; k.cy = k.cx = 1; k.divy = k.divx = 1;
    k.M = nb * h * w; k.flags = flags; k.ldm = ldm; k.moff = moff; k.mma = split;
    int steps = 0;
    for (int b = 0; b < nsrc; ++b) {
        const din_conv_src& sc = srcs[b];
        DIN_REQUIRE(sc.cout > 0, "conv1x1_dgrad_multi: null source %d", b);
        DIN_REQUIRE(sc.ldo % epc == 0 && sc.cooff % epc == 0 && sc.ldo >= sc.cooff + pad_to(sc.cout, epc),
                    "conv1x1_dgrad_multi: source %d stride/offset must be multiples of %d and cover cout (+zero pad)", b, epc);
        ConvK::Src& o = k.src[b];
        o.ld = sc.ldo; o.coff = sc.cooff;
        o.cpt = pad_to(sc.cout, epc) / epc;
        o.wld = (o.cpt + KC - 1) / KC * KC;
        o.in_bytes = (long long)nb * h * w * sc.ldo * esz;
        o.w_bytes = (long long)pad_to(cin, 256) * o.wld * 16;
        steps += (o.cpt + KC - 1) / KC;
    }
    k.nsrc = nsrc;
    k.in_bytes = k.src[0].in_bytes; k.w_bytes = k.src[0].w_bytes;
    k.Cin = srcs[0].cout; k.ldi = srcs[0].ldo; k.cioff = srcs[0].cooff;
    // the reduction runs over the sources' k-steps, every source padded to whole k-steps; no tap remap, no split
    k.cpt = KC; k.Q = steps * KC; k.nk = steps; k.wld = k.src[0].wld;
    GatherPlan g = plan_gather(k.M, 64, cin, 1, dtype);
    g.ks_per_split = steps;
    const GatherChoice c = choose_gather(k, g, dtype);
    set_plan_fields(k, c);
    return f(k, c, dtype);
}

// the argument checks of a data-gradient launch that read no pointer (din_conv_dgrad, din_conv_dgrad_x and the latter's reporter)
static int check_dgrad_args(const din_conv_desc* d, int flags) {
    DIN_REQUIRE(!d->in_u8, "conv_dgrad: in_u8 is a din_conv_fwd / din_conv_wgrad option");
    DIN_REQUIRE(!(flags & (DIN_CONV_BIAS | DIN_CONV_RELU)), "conv_dgrad: BIAS/RELU are fwd-only flags");
    const int epc = epc_of(d->dtype);
    DIN_REQUIRE(d->ldo % epc == 0 && d->cooff % epc == 0 && d->ldo >= d->cooff + pad_to(d->cout, epc),
                "conv_dgrad: dout stride/offset must be multiples of %d and cover cout (+zero pad)", epc);
    DIN_REQUIRE(d->ldi % 4 == 0 && d->cioff % 4 == 0, "conv_dgrad: din stride/offset must be multiples of 4");
    return DIN_OK;
}
// ... and those of din_conv_dgrad_x's extra source (cout, ldo, cooff)
static int check_dgrad_xsrc(const din_conv_desc* d, const din_conv_src* x) {
    DIN_REQUIRE(x && x->cout > 0, "conv_dgrad_x: null extra source");
    const int epc = epc_of(d->dtype);
    DIN_REQUIRE(x->ldo % epc == 0 && x->cooff % epc == 0 && x->ldo >= x->cooff + pad_to(x->cout, epc),
                "conv_dgrad_x: extra source stride/offset must be multiples of %d and cover cout (+zero pad)", epc);
    return DIN_OK;
}

// The launches of a data gradient (for_each_launch), each with the geometry of the extra 1x1 source `x` at the output pixel where one is
// given (din_conv_dgrad_x's fused form: parity-class launches only); the pointers of x are not read.  din_conv_dgrad binds its pointers
// and launches from here; for_dgrad_x_launches walks it for din_conv_dgrad_x and its reporter.
template <typename F>
static int for_each_dgrad_launch(const din_conv_desc* d, int flags, int ldm, int moff, const din_conv_src* x, F f) {
    const int epc = epc_of(d->dtype);
    return for_each_launch(d, 1, flags, ldm, moff, [&](ConvK& c, const GatherPlan& g, const char* what) {
        if (x) {
            ConvK::Src& o = c.src[0];
            o.ld = x->ldo; o.coff = x->cooff;
            o.cpt = pad_to(x->cout, epc) / epc;
            o.wld = (o.cpt + KC - 1) / KC * KC;
            o.in_bytes = (long long)d->nb * d->h * d->w * x->ldo * 2;
            o.w_bytes = (long long)pad_to(d->cin, 256) * o.wld * 16;
            c.xsteps = (o.cpt + KC - 1) / KC;
        }
        return f(c, g, what);
    });
}

// whether the parity-class launches of this strided dgrad can carry an extra 1x1 source (conv_gather_fast_kernel<..., XSRC>: bf16, 128 x 96
// tiles, no split-K)
static bool dgrad_x_fused(const din_conv_desc* d) {
    if (DIN_OPT("DIN_DGRAD_X") && atoi(DIN_OPT("DIN_DGRAD_X")) == 0) return false;
    if (d->dtype != DIN_BF16 || !dgrad_by_parity(d)) return false;
    return !for_each_parity_class(d, [&](const ParityClass& pc) { const GatherPlan g = plan_launch(d, 1, &pc); return (g.bn != 96 || g.splitk != 1) ? 1 : 0; });
}

// The launches din_conv_dgrad_x makes for a checked descriptor (dtype normalised; dtype0: as the caller gave it): every argument check that
// reads no pointer, then the fused form -- dg(argument block without pointers, plan, what) per parity class, x's geometry in src[0] -- or,
// for a shape the fused kernel does not serve, the two launches it replaces: dg(...) per launch of the plain data gradient, then
// mu(argument block, choice, storage dtype) for the one-source multi launch, which accumulates (the mask is linear).  din_conv_dgrad_x binds
// its pointers and launches from here; din_conv_dgrad_x_kernel_names names the kernels from here.
template <typename DG, typename MU>
static int for_dgrad_x_launches(const din_conv_desc* d, int dtype0, const din_conv_src* x, int ldm, int moff, int flags, DG dg, MU mu) {
    if (int e = check_dgrad_xsrc(d, x)) return e;
    if (int e = check_dgrad_args(d, flags)) return e;
    const bool fused = dgrad_x_fused(d);
    if (int e = for_each_dgrad_launch(d, flags, ldm, moff, fused ? x : nullptr, dg)) return e;
    if (fused) return DIN_OK;
    return for_multi_launch(1, x, dtype0, d->nb, d->h, d->w, d->cin, d->ldi, d->cioff, ldm, moff, flags | DIN_CONV_ACCUM, mu);
}

// a data-gradient launch of for_each_dgrad_launch with its pointers bound (x: the extra 1x1 source where the launch carries one), run
static int run_dgrad_launch(ConvK& c, const GatherPlan& g, const char* what, int dtype, bool split, const void* dout, const void* wpk_t, void* din_,
                            const void* mask, const din_conv_src* x, void* workspace, int64_t workspace_bytes, hipStream_t st) {
    c.in = dout; c.w = wpk_t; c.out = din_; c.mask = mask; c.mma = split;
    if (c.xsteps > 0) { c.src[0].in = x->dout; c.src[0].w = x->wpk_t; }
    return run_gather(c, g, dtype, workspace, workspace_bytes, st, what);
}

// the launch of for_multi_launch with its pointers bound, launched
static int run_multi_launch(ConvK& k, const GatherChoice& c, int dtype, int nsrc, const din_conv_src* srcs, void* din_, const void* mask, hipStream_t st) {
    k.out = din_; k.mask = mask;
    for (int b = 0; b < nsrc; ++b) { k.src[b].in = srcs[b].dout; k.src[b].w = srcs[b].wpk_t; }
    k.in = srcs[0].dout; k.w = srcs[0].wpk_t;
    if (DIN_OPT("DIN_DEBUG_PLAN"))
        fprintf(stderr, "[din] conv1x1_dgrad_multi M=%d nsrc=%d couts=%d,%d,%d,%d ld=%d,%d,%d,%d coff=%d,%d,%d,%d cin=%d flags=%d regw=%d\n", k.M, nsrc, srcs[0].cout,
                nsrc > 1 ? srcs[1].cout : 0, nsrc > 2 ? srcs[2].cout : 0, nsrc > 3 ? srcs[3].cout : 0, srcs[0].ldo, nsrc > 1 ? srcs[1].ldo : 0,
                nsrc > 2 ? srcs[2].ldo : 0, nsrc > 3 ? srcs[3].ldo : 0, srcs[0].cooff, nsrc > 1 ? srcs[1].cooff : 0, nsrc > 2 ? srcs[2].cooff : 0,
                nsrc > 3 ? srcs[3].cooff : 0, k.Cout, k.flags, (int)(c.family == GATHER_REGW));
    return launch_choice(k, c, dtype, st, "conv1x1_dgrad_multi");
}

}  // namespace

extern "C" {

int din_conv_kernel_tile(const din_conv_desc* d, int which, int32_t* bm, int32_t* bn) {
    DIN_REQUIRE(d && bm && bn && which >= 0 && which <= 2, "conv_kernel_tile: bad argument");
    const SplitDesc sd(d);
    if (which == 2) { din_wgrad::wgrad_tile_code(din_wgrad::plan_wgrad(d, sd.split), bm, bn); return DIN_OK; }     // (the codes of the weight-gradient choice)
    // the canonical launch of the descriptor (conv_k_of), as choose_gather resolves it
    const GatherChoice c = canonical_choice(d, which);
    switch (c.family) {
    case GATHER_SMALL: *bm = 0; break;
    case GATHER_HALO: *bm = 1; break;
    case GATHER_PIPE: *bm = 2; break;
    case GATHER_STREAM: *bm = 4; break;
    case GATHER_REGW: *bm = 5; break;
    default: *bm = c.tile.bm; break;
    }
    *bn = c.bn;
    return DIN_OK;
}

int din_conv_kernel_variant(const din_conv_desc* d, int which, int32_t* flags) {
    DIN_REQUIRE(d && flags && which >= 0 && which <= 1, "conv_kernel_variant: bad argument");
    const SplitDesc sd(d);
    const GatherChoice c = canonical_choice(d, which);
    *flags = 0;
    if (c.family != GATHER_TILE || c.tile.bm != 128) return DIN_OK;     // (the 256-pixel tiles have one wave grid per filter tile)
    *flags = (c.tile.fastk ? 1 : 0) | (c.tile.wm * c.tile.wn == 8 ? 2 : 0) | (c.tile.lanek ? 4 : 0);
    return DIN_OK;
}

int din_conv_kernel_names(const din_conv_desc* d, int which, int flags, int ldm, int moff, char* buf, int buf_bytes) {
    const SplitDesc sd(d);
    if (int e = check_desc(d)) return e;
    DIN_REQUIRE(which >= 0 && which <= 2 && buf_bytes >= 0 && (buf || buf_bytes == 0), "conv_kernel_names: bad argument");
    std::string names;
    if (which == 2) {
        DIN_REQUIRE(!flags && !ldm && !moff, "conv_kernel_names: flags / ldm / moff are fwd / dgrad arguments");
        DIN_REQUIRE(!d->in_u8 || din_conv_accepts_u8(d), "conv_kernel_names: in_u8 on a layer din_conv_accepts_u8() rejects");
        din_wgrad::append_wgrad_names(d, din_wgrad::plan_wgrad(d, sd.split), names);
    } else if (which == 0) {
        DIN_REQUIRE(!(flags & (DIN_CONV_ACCUM | DIN_CONV_MASK)), "conv_kernel_names: ACCUM/MASK are dgrad-only flags");
        DIN_REQUIRE(!d->in_u8 || din_conv_accepts_u8(d), "conv_kernel_names: in_u8 on a layer din_conv_accepts_u8() rejects");
    } else {
        DIN_REQUIRE(!d->in_u8 && !(flags & (DIN_CONV_BIAS | DIN_CONV_RELU)), "conv_kernel_names: in_u8 / BIAS / RELU are fwd-only");
    }
    static const unsigned char raw_frames = 0;              // stands for the caller's uint8 frames: the selection only asks whether there are any
    if (which != 2) {
        if (int e = for_each_launch(d, which, flags, ldm, moff, [&](ConvK& k, const GatherPlan& g, const char*) {
                if (d->in_u8) k.u8 = &raw_frames;
                k.mma = sd.split;
                return append_launch_names(k, g, d->dtype, names);
            }))
            return e;
    }
    return copy_names(names, buf, buf_bytes);
}

int64_t din_conv_workspace_bytes(const din_conv_desc* d, int which) {
    if (!d) return 0;
    const SplitDesc sd(d);
    if (which != 0 && which != 1) return din_wgrad::plan_wgrad(d).ws_bytes;
    if (which == 0 || !dgrad_by_parity(d)) return plan_launch(d, which).ws_bytes;
    int64_t mx = 0;
    for_each_parity_class(d, [&](const ParityClass& pc) { const int64_t b = plan_launch(d, 1, &pc).ws_bytes; if (b > mx) mx = b; return 0; });
    return mx;
}

int din_conv_fwd(const din_conv_desc* d, const void* in, const void* wpk, const float* bias, void* out, int flags,
                 void* workspace, int64_t workspace_bytes, void* stream) {
    const SplitDesc sd(d);
    if (int e = check_desc(d)) return e;
    DIN_REQUIRE(in && wpk && out, "conv_fwd: null pointer");
    DIN_REQUIRE(!(flags & DIN_CONV_BIAS) || bias, "conv_fwd: BIAS flag without bias");
    DIN_REQUIRE(!(flags & (DIN_CONV_ACCUM | DIN_CONV_MASK)), "conv_fwd: ACCUM/MASK are dgrad-only flags");
    DIN_REQUIRE(!d->in_u8 || din_conv_accepts_u8(d), "conv_fwd: in_u8 on a layer din_conv_accepts_u8() rejects");
    return for_each_launch(d, 0, flags, 0, 0, [&](ConvK& k, const GatherPlan& g, const char* what) {
        k.in = in; k.w = wpk; k.out = out; k.bias = bias; k.mma = sd.split;
        if (d->in_u8) k.u8 = reinterpret_cast<const unsigned char*>(in);
        return run_gather(k, g, d->dtype, workspace, workspace_bytes, as_stream(stream), what);
    });
}

int din_conv_accepts_u8(const din_conv_desc* d) {
    if (!d || d->dtype != DIN_BF16 || d->kh != 3 || d->kw != 3 || d->sh != 2 || d->sw != 2 || d->dh != 1 || d->dw != 1) return 0;
    if (d->cin != 3 || d->cout > 32 || d->cout % 8 != 0 || d->ldo % 8 != 0 || d->cooff % 8 != 0) return 0;
    if ((int64_t)d->nb * d->oh * d->ow < 256 * 1024) return 0;
    if ((long long)d->h * d->w * 16 >= 0x7fffffffll || (long long)d->oh * d->ow * d->ldo * 2 >= 0x7fffffffll) return 0;
    if (!conv_small_wanted()) return 0;
    const char* uv = DIN_OPT("DIN_CONV_U8");
    if (uv && atoi(uv) == 0) return 0;
    din_conv_desc t = *d;
    t.in_u8 = 0; t.ldi = 8; t.cioff = 0;             // the plan of the prepared-tensor form must pick the image-layer wgrad kernel
    const din_wgrad::WgradChoice c = din_wgrad::plan_wgrad(&t);
    return c.family == din_wgrad::WGRAD_STEM && c.stem.cpp == 1 ? 1 : 0;
}

int din_conv_fwd2(const din_conv_desc* d, const void* in, const void* wpk, const float* bias, void* out, void* out2, int ldo2, int cooff2,
                  int csplit, int craw, int flags, void* workspace, int64_t workspace_bytes, void* stream) {
    const SplitDesc sd(d);
    if (int e = check_desc(d)) return e;
    DIN_REQUIRE(in && wpk && out && out2, "conv_fwd2: null pointer");
    DIN_REQUIRE(!(flags & DIN_CONV_BIAS) || bias, "conv_fwd2: BIAS flag without bias");
    return for_fwd2_launch(d, sd.split, ldo2, cooff2, csplit, craw, flags, [&](ConvK& k, const GatherPlan& g) {
        k.in = in; k.w = wpk; k.out = out; k.bias = bias; k.out2 = out2;
        return run_gather(k, g, d->dtype, workspace, workspace_bytes, as_stream(stream), "conv_fwd2");
    });
}

int din_conv_fwd2_kernel_names(const din_conv_desc* d, int ldo2, int cooff2, int csplit, int craw, int flags, char* buf, int buf_bytes) {
    const SplitDesc sd(d);
    if (int e = check_desc(d)) return e;
    DIN_REQUIRE(buf_bytes >= 0 && (buf || buf_bytes == 0), "conv_fwd2_kernel_names: bad argument");
    std::string names;
    if (int e = for_fwd2_launch(d, sd.split, ldo2, cooff2, csplit, craw, flags, [&](ConvK& k, const GatherPlan& g) {
            return append_launch_names(k, g, d->dtype, names);
        }))
        return e;
    return copy_names(names, buf, buf_bytes);
}

int din_conv_dgrad(const din_conv_desc* d, const void* dout, const void* wpk_t, void* din_, const void* mask, int ldm,
                   int moff, int flags, void* workspace, int64_t workspace_bytes, void* stream) {
    const SplitDesc sd(d);
    if (int e = check_desc(d)) return e;
    DIN_REQUIRE(dout && wpk_t && din_, "conv_dgrad: null pointer");
    DIN_REQUIRE(!(flags & DIN_CONV_MASK) || mask, "conv_dgrad: MASK flag without mask");
    if (int e = check_dgrad_args(d, flags)) return e;
    return for_each_dgrad_launch(d, flags, ldm, moff, nullptr, [&](ConvK& c, const GatherPlan& g, const char* what) {
        return run_dgrad_launch(c, g, what, d->dtype, sd.split, dout, wpk_t, din_, mask, nullptr, workspace, workspace_bytes, as_stream(stream));
    });
}

int din_conv_dgrad_x_fused(const din_conv_desc* d) { return (d && check_desc(d) == DIN_OK && dgrad_x_fused(d)) ? 1 : 0; }

int din_conv_dgrad_x(const din_conv_desc* d, const void* dout, const void* wpk_t, void* din_, const void* mask, int ldm, int moff, int flags,
                     const din_conv_src* x, void* workspace, int64_t workspace_bytes, void* stream) {
    const int dtype0 = d ? d->dtype : 0;
    const SplitDesc sd(d);
    if (int e = check_desc(d)) return e;
    DIN_REQUIRE(x && x->dout && x->wpk_t, "conv_dgrad_x: null extra source");
    DIN_REQUIRE(dout && wpk_t && din_, "conv_dgrad: null pointer");
    DIN_REQUIRE(!(flags & DIN_CONV_MASK) || mask, "conv_dgrad: MASK flag without mask");
    hipStream_t st = as_stream(stream);
    return for_dgrad_x_launches(d, dtype0, x, ldm, moff, flags,
        [&](ConvK& c, const GatherPlan& g, const char* what) {
            return run_dgrad_launch(c, g, what, d->dtype, sd.split, dout, wpk_t, din_, mask, x, workspace, workspace_bytes, st);
        },
        [&](ConvK& k, const GatherChoice& c, int sdt) { return run_multi_launch(k, c, sdt, 1, x, din_, mask, st); });
}

int din_conv_dgrad_x_kernel_names(const din_conv_desc* d, const din_conv_src* x, int ldm, int moff, int flags, char* buf, int buf_bytes) {
    const int dtype0 = d ? d->dtype : 0;
    const SplitDesc sd(d);
    if (int e = check_desc(d)) return e;
    DIN_REQUIRE(buf_bytes >= 0 && (buf || buf_bytes == 0), "conv_dgrad_x_kernel_names: bad argument");
    std::string names;
    if (int e = for_dgrad_x_launches(d, dtype0, x, ldm, moff, flags,
            [&](ConvK& k, const GatherPlan& g, const char*) { k.mma = sd.split; return append_launch_names(k, g, d->dtype, names); },
            [&](ConvK& k, const GatherChoice& c, int sdt) { return append_kernel_names(k, c, sdt, names); }))
        return e;
    return copy_names(names, buf, buf_bytes);
}

int din_conv1x1_dgrad_multi(int nsrc, const din_conv_src* srcs, int dtype, int nb, int h, int w, int cin, int ldi, int cioff,
                            void* din_, const void* mask, int ldm, int moff, int flags, void* stream) {
    DIN_REQUIRE(nsrc >= 1 && nsrc <= 4 && srcs && din_, "conv1x1_dgrad_multi: 1..4 sources");
    DIN_REQUIRE(!(flags & DIN_CONV_MASK) || mask, "conv1x1_dgrad_multi: MASK flag without mask");
    for (int b = 0; b < nsrc; ++b) DIN_REQUIRE(srcs[b].dout && srcs[b].wpk_t, "conv1x1_dgrad_multi: null source %d", b);
    return for_multi_launch(nsrc, srcs, dtype, nb, h, w, cin, ldi, cioff, ldm, moff, flags,
                            [&](ConvK& k, const GatherChoice& c, int sdt) { return run_multi_launch(k, c, sdt, nsrc, srcs, din_, mask, as_stream(stream)); });
}

int din_conv1x1_dgrad_multi_kernel_names(int nsrc, const din_conv_src* srcs, int dtype, int nb, int h, int w, int cin, int ldi, int cioff,
                                         int ldm, int moff, int flags, char* buf, int buf_bytes) {
    DIN_REQUIRE(buf_bytes >= 0 && (buf || buf_bytes == 0), "conv1x1_dgrad_multi_kernel_names: bad argument");
    std::string names;
    if (int e = for_multi_launch(nsrc, srcs, dtype, nb, h, w, cin, ldi, cioff, ldm, moff, flags,
                                 [&](ConvK& k, const GatherChoice& c, int sdt) { return append_kernel_names(k, c, sdt, names); }))
        return e;
    return copy_names(names, buf, buf_bytes);
}

}  // extern "C"
