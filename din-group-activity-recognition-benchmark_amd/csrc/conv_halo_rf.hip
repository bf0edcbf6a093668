// conv_halo_rf_kernel: the halo-tiled 3x3 convolution with the FILTERS RESIDENT IN REGISTERS -- the narrow 3x3 layers of the Inception-A
// blocks (Mixed_5b..5d branch3x3dbl_2 / _3, Mixed_6a.branch3x3dbl_2: 64 -> 96 and 96 -> 96 channels), forward and data gradient.
//
// Why another kernel: conv_halo_kernel (conv_halo.hip) streams one (tap, 64-channel block) filter slab per step through an LDS ring although
// the filter bank never changes during a launch: for 96 -> 96 channels 166 KB of constants land in LDS per 256-pixel tile next to 65 KB of
// pixels, three of the five fragment reads per six MFMAs fetch constants, and the ring costs one s_barrier per tap.  The banks are small
// (96 x 96 x 9 bf16 = 166 KB against a 512 KB register file per CU), so here they are loaded ONCE per persistent workgroup, straight from the
// layer's packed bank (forward: wpk, data gradient: the transposed wpt) as ready-made A fragments of v_mfma_f32_16x16x32_bf16.
//
// Wave layout: FOUR waves, one per SIMD, 512 registers each.  wave = (filter class wc, pixel half wp): 16 TI filters (TI = 2 | 3 row tiles:
// <= 64 | <= 96 produced channels in two classes) over the WHOLE reduction -- 9 taps x NKS 32-channel steps x TI fragments = up to 324
// registers -- times 128 pixels (four rows of the 8 x 32 tile = 8 pixel fragments, 8 TI accumulators).  One pixel fragment read feeds TI MFMAs;
// per 32-channel step a wave issues 8 reads for 8 TI MFMAs (the 16-wave halo kernel: 5 reads for 6).
// Pixels: the halo kernel's LDS image unchanged -- (8 + 2) x (32 + 2) pixels per 64-channel block at a 160-byte row pitch, filled by LDS-DMA
// with out-of-image taps as out-of-range buffer offsets (zeros), double-buffered by block with the next block / next item in flight.  A tap
// is an immediate offset on the fragment read.  The ONLY barrier is the halo-buffer hand-over, once per 64-channel block; there is no filter
// ring.  With one wave per SIMD nothing hides a wait and a wave issues one instruction per four clocks: next to a 16-clock MFMA that is a
// budget of three other instructions.  So (as conv1x1_regw_kernel) the fragment reads are inline asm with a rolling window of three or four
// reads ahead of the MFMAs and hand-counted lgkmcnt; the MFMAs are inline asm too, which fixes the register file of every filter fragment
// (rf_mfma); and the transfers of the next halo are issued one behind every second or fourth fragment of a block's first half from a
// per-lane plan made once (11 instructions per transfer), so that they sit between the MFMAs and have landed at the hand-over (vmcnt(0):
// nothing else is in flight there but stores a whole block old).
// MFMA row 4 g + e of row tile i is channel (class base) + 4 TI g + 4 i + e: a lane of the result holds 4 TI consecutive channels of a pixel.
// ReLU-backward mask: the tile's mask operand travels by LDS-DMA too, into a wave-private LDS region (each wave fetches exactly the 128 pixels
// x 16 TI channels its epilogue reads: no barrier of its own), issued during the item's first block -- no exposed memory latency in the
// epilogue.  It needs the mask view in whole 16-byte chunks (din_conv_rf_eligible).  Accumulate operands are requested one, two or four pixel
// fragments at a time before their stores (compiler-visible loads: nothing is in flight at that point; the planner keeps ACCUM launches on
// the old kernels).  The forward's bias sits in LDS behind the halo buffers.
// The 5x5 48 -> 64 layers of the same blocks have a kernel family of their own, conv_halo_rf5_kernel (conv_halo_rf5.hip): their 48-channel
// taps are 6 chunks, so a 32-channel step straddles taps, and the reduction is walked densely over (tap, chunk) there.  Conv2d_4a
// (80 -> 192) does not fit the register file.
#include "din_common.h"
#include "conv_wgrad.h"
#include "conv_gather.h"
#include "conv_shared.h"
#include <stdlib.h>
#include <type_traits>

using din_wgrad::lds_dma16;
using din_gather::ConvK;

namespace {

constexpr int RF_TH = 8, RF_TW = 32, RF_HWW = RF_TW + 2, RF_HWH = RF_TH + 2, RF_HPX = RF_HWW * RF_HWH;
constexpr int RF_PCH = 10, RF_PB = RF_PCH * 16;                                  // row pitch: 10 chunks = 160 bytes (conv_halo.hip)
constexpr int RF_NTR_H = (RF_HPX * RF_PCH + 255) / 256;                          // halo transfers per wave and block (14)
constexpr int RF_HB = RF_NTR_H * 4096;                                           // bytes of one halo buffer
constexpr unsigned RF_OOB = 0x80000000u;
// dynamic LDS: two halo buffers, then the four waves' mask regions (masked data gradient) or their bias values (forward)
constexpr size_t rf_lds(int ti, bool dg, bool mask) { return (size_t)2 * RF_HB + (dg ? (mask ? (size_t)4 * 4 * ti * 1024 : 0) : 1024); }

template <int I, int N, typename F>
__device__ __forceinline__ void rf_static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        rf_static_for<I + 1, N>(f);
    }
}
template <int OFF>
__device__ __forceinline__ void rf_read(u32x4& dst, uint32_t addr) {
    static_assert(OFF >= 0 && OFF < 65536, "ds_read offset field");
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF) : "memory");
}
template <bool ACC>
__device__ __forceinline__ void rf_pin(u32x4& x) {               // the value lives in an accumulation (ACC) or an architectural register from here on
    if constexpr (ACC) asm volatile("" : "+a"(x));
    else asm volatile("" : "+v"(x));
}
// c (+)= a x b.  Inline asm, with the register file of every operand chosen here (ACC: the filter fragment sits in an accumulation
// register): through the builtin the allocator keeps every fragment it can in architectural registers and copies the others there in
// front of their MFMA (904 v_accvgpr_read per tile in the first build of the 96 -> 96 form).  FIRST: the tile's first k-step, C = 0.
template <bool ACC, bool FIRST>
__device__ __forceinline__ void rf_mfma(f32x4& c, const u32x4& a, const u32x4& b) {
    if constexpr (FIRST) {
        if constexpr (ACC) asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, 0" : "=&a"(c) : "a"(a), "v"(b));
        else asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, 0" : "=&a"(c) : "v"(a), "v"(b));
    } else {
        if constexpr (ACC) asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(c) : "a"(a), "v"(b));
        else asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
    }
}
template <int N>
__device__ __forceinline__ void rf_wait(u32x4& x) { asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(x) : "n"(N)); }

// byte offset of pixel fragment j (row j >> 1 of the wave's four, columns (j & 1) * 16 ..) at tap (r, s), 32-channel step kk of the block,
// from the lane's base; the data gradient walks the taps backwards from the far corner of the halo
template <bool DG>
constexpr int rf_frag_off(int tap, int kk, int j) {
    const int r = tap / 3, s = tap - r * 3;
    const int ry = DG ? 2 - r : r, sx = DG ? 2 - s : s;
    return (((j >> 1) + ry) * RF_HWW + (j & 1) * 16 + sx) * RF_PB + kk * 64;
}

// TI: 16-row filter tiles per wave (two classes: 32 TI produced channels per workgroup); NKS: 32-channel steps per tap (2: <= 64 reduction
// channels, 3: <= 96); DG: data gradient (taps walked backwards)
template <int TI, int NKS, bool DG>
__global__ __launch_bounds__(256, 1) void conv_halo_rf_kernel(ConvK p) {
#if defined(__HIP_DEVICE_COMPILE__)
    static_assert((TI == 2 || TI == 3) && (NKS == 2 || NKS == 3), "filter registers: 9 NKS TI fragments <= 324");
    constexpr int NBLK = (NKS + 1) / 2;                                          // 64-channel blocks
    constexpr int NTR_M = 4 * TI, MBW = NTR_M * 1024;                            // mask transfers / bytes per wave: 128 pixels x 2 TI chunks
    constexpr int NA = (256 - 32 * TI) / 4;                                       // filter fragments in accumulation registers (beside the 32 TI accumulator registers)
    constexpr int D = TI == 3 ? 3 : 4;                                            // fragment reads in flight ahead of the MFMAs (>= 128 matrix-pipe cycles)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 15, g4 = lane >> 4;
    const int wc = wid & 1, wp = wid >> 1;
    const int cbase = wc * 16 * TI;                                               // first produced channel of the wave's class
    const uint32_t lds_base = (uint32_t)(uintptr_t)smem_raw;
    const uint32_t ldsWv = __builtin_amdgcn_readfirstlane(lds_base + (uint32_t)(wid * 1024));
    const uint32_t ldsMk = __builtin_amdgcn_readfirstlane(lds_base + (uint32_t)(2 * RF_HB + wid * MBW));

    // the launch's geometry in registers: nothing below reads the argument block again (a scalar load inside the walk would share lgkmcnt
    // with the counted fragment reads)
    const int W_ = p.W, H_ = p.H, ldi = p.ldi, OH = p.OH, OW = p.OW, Cout = p.Cout, ldo = p.ldo, cooff = p.cooff, cpt = p.cpt, flags = p.flags;
    const int ldm = p.ldm, moff = p.moff, cioff2 = p.cioff * 2;
    const int hy0 = p.by - (DG ? 2 : 0), hx0 = p.bx - (DG ? 2 : 0);
    const int tiles_x = (OW + RF_TW - 1) / RF_TW, tiles_y = (OH + RF_TH - 1) / RF_TH;
    const int tiles_img = tiles_x * tiles_y, nitems = tiles_img * p.NB;
    const long long img_bytes = (long long)H_ * W_ * ldi * 2ll;
    const long long oimg_bytes = (long long)OH * OW * ldo * 2ll, mimg_bytes = (long long)OH * OW * ldm * 2ll;
    const char* const inp = reinterpret_cast<const char*>(p.in);
    char* const outp = reinterpret_cast<char*>(p.out);
    const char* const maskp = reinterpret_cast<const char*>(p.mask);
    const bool masked = (flags & DIN_CONV_MASK) != 0;

    struct Item { int n, ty, tx; };
    auto decode_item = [&](int item) {
        Item it;
        it.n = item / tiles_img;
        const int tr = item - it.n * tiles_img;
        it.ty = tr / tiles_x; it.tx = tr - it.ty * tiles_x;
        return it;
    };
    // ---- halo transfers.  Halo chunk id = (wid + 4 i) * 64 + lane of transfer i, lane-linear in LDS (conv_halo.hip).  What a lane fetches in
    // transfer i never changes, so its plan is made once: rel[i] = byte offset of (halo pixel, chunk) from the halo's first pixel, pk = its
    // halo column and chunk (16 bits per transfer; chunk 15: a pad chunk or past the halo, never fetched).  Per transfer that leaves the column
    // test, the chunk test and one add: with one wave per SIMD every instruction of the plan is an issue slot the MFMAs do not get.  Rows
    // outside the image need no test: the buffer resource covers ONE image and the whole offset sits in the VGPR, so a row above it is a
    // negative (= huge unsigned) offset and a row below it one past the image's bytes -- both out of range, and such transfers land as zeros.
    int rel[RF_NTR_H];
    uint32_t pk[(RF_NTR_H + 1) / 2];
#pragma unroll
    for (int i = 0; i < (RF_NTR_H + 1) / 2; ++i) pk[i] = 0u;
#pragma unroll
    for (int i = 0; i < RF_NTR_H; ++i) {
        const int id = (wid + 4 * i) * 64 + lane;
        const int hp = id / RF_PCH, cc = id - hp * RF_PCH;
        const int hy = hp / RF_HWW, hx = hp - hy * RF_HWW;
        const bool real = hp < RF_HPX && cc < 8;
        rel[i] = real ? ((hy * W_ + hx) * ldi + cc * 8) * 2 : 0;
        pk[i >> 1] |= (uint32_t)((real ? hx : 0) | ((real ? cc : 15) << 8)) << (16 * (i & 1));
    }
    // what the transfers of one (item, block) share, computed once per block: the image's resource, the byte offset of the halo's first pixel
    // at the block's first channel, the columns left of the halo (gx0) and the chunks the block has
    struct HaloBlk { __amdgpu_buffer_rsrc_t rs; int base, gx0, nch; };
    auto halo_blk = [&](const Item& it, int b) __attribute__((always_inline)) {
        HaloBlk h;
        h.rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(inp) + (long long)it.n * img_bytes, 0, (int)img_bytes, 0x00020000);
        h.gx0 = it.tx * RF_TW + hx0;
        h.base = ((it.ty * RF_TH + hy0) * W_ + h.gx0) * ldi * 2 + cioff2 + b * 128;
        h.nch = cpt - b * 8;                                                      // (>= 8: all)
        return h;
    };
    auto halo_one = [&](int buf, const HaloBlk& h, int i) __attribute__((always_inline)) {
        asm volatile("" : "+v"(rel[i]));                                          // the transfer's instructions stay HERE, between the MFMAs around them
        const int hx = (int)__builtin_amdgcn_ubfe(pk[i >> 1], 16 * (i & 1), 6), cc = (int)__builtin_amdgcn_ubfe(pk[i >> 1], 16 * (i & 1) + 8, 4);
        const bool ok = (unsigned)(h.gx0 + hx) < (unsigned)W_ && cc < h.nch;
        int voff = rel[i] + h.base;
        voff = ok ? voff : (int)RF_OOB;
        lds_dma16(ldsWv + (uint32_t)(buf * RF_HB + i * 4096), h.rs, voff, 0);
    };
    // transfer i of the wave's own mask region: chunk id = i * 64 + lane = (pixel pl of the wave's 128, chunk c of its 2 TI)
    auto mask_one = [&](const Item& it, int i) __attribute__((always_inline)) {
        int ln = lane;
        asm volatile("" : "+v"(ln));
        __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(maskp) + (long long)it.n * mimg_bytes, 0, (int)mimg_bytes, 0x00020000);
        const unsigned id = (unsigned)(i * 64 + ln), pl = id / (unsigned)(2 * TI), c = id - pl * (unsigned)(2 * TI);
        const int gy = it.ty * RF_TH + 4 * wp + (int)(pl >> 5), gx = it.tx * RF_TW + (int)(pl & 31u);
        const int co = cbase + (int)c * 8;
        const bool ok = gy < OH && gx < OW && co < Cout;
        lds_dma16(ldsMk + (uint32_t)(i * 1024), rs, ok ? ((gy * OW + gx) * ldm + moff + co) * 2 : (int)RF_OOB, 0);
    };

    const int G = (int)gridDim.x;
    int item = xcd_remap((int)blockIdx.x, G);
    if (item >= nitems) return;
    Item cur = decode_item(item);
    {
        const HaloBlk h0 = halo_blk(cur, 0);
#pragma unroll
        for (int i = 0; i < RF_NTR_H; ++i) halo_one(0, h0, i);
    }

    // ---- the wave's filters as A fragments, once: MFMA row m of row tile i is channel cbase + (m >> 2) * 4 TI + 4 i + (m & 3)
    u32x4 Wf[9][NKS][TI];
    {
        __amdgpu_buffer_rsrc_t rsW = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.w), 0, (int)p.w_bytes, 0x00020000);
        const int wld16 = p.wld * 16;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
                for (int i = 0; i < TI; ++i) {
                    const int chan = cbase + (frow >> 2) * 4 * TI + i * 4 + (frow & 3);
                    const bool real = chan < Cout && ks * 4 + g4 < cpt;
                    Wf[tap][ks][i] = __builtin_amdgcn_raw_buffer_load_b128(rsW, real ? chan * wld16 + g4 * 16 : (int)RF_OOB, (tap * cpt + ks * 4) * 16, 0);
                }
        // where they live is decided HERE (rf_mfma): the first NA fragments in accumulation registers, the others in architectural ones
        rf_static_for<0, 9 * NKS * TI>([&](auto N_) __attribute__((always_inline)) {
            constexpr int n = decltype(N_)::value, tap = n / (NKS * TI), ks = (n / TI) % NKS, i = n % TI;
            rf_pin<(n < NA)>(Wf[tap][ks][i]);
        });
    }
    // forward: the wave's 16 TI bias values behind the halo buffers (in registers they would push filters out; read from global memory in
    // the epilogue they would cost a memory latency per item)
    if constexpr (!DG) {
        if (lane < 16 * TI) {
            const int co = cbase + lane;
            *reinterpret_cast<float*>(smem_raw + 2 * RF_HB + wid * 256 + lane * 4) = ((flags & DIN_CONV_BIAS) && co < Cout) ? p.bias[co] : 0.f;
        }
    }
    f32x4 acc[TI][8];                                                             // (the first k-step of a tile writes them: rf_mfma<.., FIRST>)

    // lane base of the fragment reads: first row of the wave's pixel half, pixel column frow, chunk g4
    const uint32_t xb0 = lds_base + (uint32_t)((4 * wp * RF_HWW + frow) * RF_PB + g4 * 16);
    u32x4 xf[D];

    // ---- epilogue straight from the accumulators: a lane holds channels cbase + 4 TI g4 .. + 4 TI of pixel frow of every fragment
    auto epilogue = [&](const Item& it) __attribute__((always_inline)) {
        int ln = lane;                                                             // (the lane's offsets are recomputed per item: hoisted out of the item
        asm volatile("" : "+v"(ln));                                              //  loop they cost registers the filters fill)
        const int frow_e = ln & 15, g4_e = ln >> 4;
        __amdgpu_buffer_rsrc_t rsO = __builtin_amdgcn_make_buffer_rsrc(outp + (long long)it.n * oimg_bytes, 0, (int)oimg_bytes, 0x00020000);
        constexpr int EB = TI * NKS == 9 ? 1 : TI == 3 ? 2 : 4;                                       // pixel fragments per batch of operand requests (register budget)
#pragma unroll
        for (int jb = 0; jb < 8; jb += EB) {
            [[maybe_unused]] u32x2 old[DG ? EB : 1][TI];                          // (BIAS / RELU are forward flags, MASK / ACCUM data-gradient flags: host)
            int pxo[EB];                                                           // byte offset of the fragment's pixel, or out of range
#pragma unroll
            for (int jj = 0; jj < EB; ++jj) {
                const int j = jb + jj;
                const int gy = it.ty * RF_TH + 4 * wp + (j >> 1), gx = it.tx * RF_TW + (j & 1) * 16 + frow_e;
                pxo[jj] = (gy < OH && gx < OW) ? ((gy * OW + gx) * ldo + cooff) * 2 : (int)RF_OOB;
#pragma unroll
                for (int i = 0; i < TI; ++i) {
                    const int co = cbase + g4_e * 4 * TI + i * 4;
                    if (DG && (flags & DIN_CONV_ACCUM)) old[DG ? jj : 0][i] = __builtin_amdgcn_raw_buffer_load_b64(rsO, co < Cout ? pxo[jj] + co * 2 : (int)RF_OOB, 0, 0);
                }
            }
#pragma unroll
            for (int jj = 0; jj < EB; ++jj) {
                const int j = jb + jj;
                const int pl = (j >> 1) * 32 + (j & 1) * 16 + frow_e;
#pragma unroll
                for (int i = 0; i < TI; ++i) {
                    const int co = cbase + g4_e * 4 * TI + i * 4;
                    f32x4 v = acc[i][j];
                    if constexpr (!DG) v += *reinterpret_cast<const f32x4*>(smem_raw + 2 * RF_HB + wid * 256 + (g4_e * 4 * TI + i * 4) * 4);
                    if (!DG && (flags & DIN_CONV_RELU)) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
                    }
                    if (DG && masked) {
                        const u32x2 mk = *reinterpret_cast<const u32x2*>(smem_raw + 2 * RF_HB + wid * MBW + pl * (2 * TI * 16) + g4_e * 8 * TI + i * 8);
                        if (!(__uint_as_float(mk[0] << 16) > 0.f)) v[0] = 0.f;
                        if (!(__uint_as_float(mk[0] & 0xffff0000u) > 0.f)) v[1] = 0.f;
                        if (!(__uint_as_float(mk[1] << 16) > 0.f)) v[2] = 0.f;
                        if (!(__uint_as_float(mk[1] & 0xffff0000u) > 0.f)) v[3] = 0.f;
                    }
                    if (DG && (flags & DIN_CONV_ACCUM)) {
                        v[0] += __uint_as_float(old[DG ? jj : 0][i][0] << 16); v[1] += __uint_as_float(old[DG ? jj : 0][i][0] & 0xffff0000u);
                        v[2] += __uint_as_float(old[DG ? jj : 0][i][1] << 16); v[3] += __uint_as_float(old[DG ? jj : 0][i][1] & 0xffff0000u);
                    }
                    // (out of range: pxo has bit 31 set and stays >= 2^31 as an unsigned offset; Cout % 8 == 0: a piece is whole or absent)
                    __builtin_amdgcn_raw_buffer_store_b64(u32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])}, rsO, co < Cout ? pxo[jj] + co * 2 : (int)RF_OOB, 0, 0);
                }
            }
            asm volatile("" ::: "memory");                                       // one batch at a time: the operands of both would push filters out
        }
    };

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    int hb = 0;
    for (;;) {
        const int item_n = item + G;
        const bool has_next_item = item_n < nitems;
        const Item nxt = has_next_item ? decode_item(item_n) : cur;
        rf_static_for<0, NBLK>([&](auto B_) __attribute__((always_inline)) {
            constexpr int b = decltype(B_)::value;
            constexpr int KB = b == NBLK - 1 ? NKS - 2 * b : 2;                  // 32-channel steps of this block per tap
            constexpr int NSTEP = 9 * KB, NF = NSTEP * 8;                        // steps = (tap, kk); fragments
            constexpr int SP = KB == 1 ? 2 : 4;                                   // fragments between two transfers: all issued in the block's first half
            static_assert(RF_NTR_H * SP <= NF / 2 + 8 && (RF_NTR_H + (b == 0 ? NTR_M : 0)) * SP <= NF, "every transfer of the block has a slot");
            constexpr bool last_blk = b == NBLK - 1;
            const bool hn = !last_blk || has_next_item;                           // a next (item, block) exists: its halo goes into buffer hb ^ 1
            const HaloBlk hnx = halo_blk(last_blk ? nxt : cur, last_blk ? 0 : b + 1);
            const uint32_t xa = xb0 + (uint32_t)(hb * RF_HB);
            rf_static_for<0, D>([&](auto F_) __attribute__((always_inline)) {
                constexpr int f = decltype(F_)::value;
                rf_read<rf_frag_off<DG>((f >> 3) / KB, (f >> 3) % KB, f & 7)>(xf[f], xa);
            });
            rf_static_for<0, NF>([&](auto F_) __attribute__((always_inline)) {
                constexpr int f = decltype(F_)::value;
                constexpr int step = f >> 3, j = f & 7, tap = step / KB, kk = step % KB, ks = 2 * b + kk;
                rf_wait<(NF - 1 - f < D - 1 ? NF - 1 - f : D - 1)>(xf[f % D]);
                rf_static_for<0, TI>([&](auto I_) __attribute__((always_inline)) {
                    constexpr int i = decltype(I_)::value;
                    rf_mfma<((tap * NKS + ks) * TI + i < NA), (b == 0 && step == 0)>(acc[i][j], Wf[tap][ks][i], xf[f % D]);
                });
                if constexpr (f + D < NF) {
                    constexpr int nf = f + D;
                    rf_read<rf_frag_off<DG>((nf >> 3) / KB, (nf >> 3) % KB, nf & 7)>(xf[f % D], xa);
                }
                if constexpr (f % SP == 0) {                                      // one transfer after the MFMAs of every SP-th fragment
                    constexpr int t = f / SP;
                    if constexpr (t < RF_NTR_H) { if (hn) halo_one(hb ^ 1, hnx, t); }
                    else if constexpr (DG && b == 0 && t - RF_NTR_H < NTR_M) { if (masked) mask_one(cur, t - RF_NTR_H); }
                }
            });
            asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");                    // (the last MFMAs' results: read by the epilogue's VALU, no hazard the compiler sees)
            // hand-over: this wave's transfers (next halo, the item's mask) have landed; the stores in flight are a block old
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if constexpr (last_blk) epilogue(cur);
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            hb ^= 1;
        });
        if (!has_next_item) break;
        item = item_n; cur = nxt;
    }
#endif
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
// the instantiations, X(TI, NKS, DG): both directions, <= 64 | <= 96 produced channels, <= 64 | <= 96 reduction channels
#define DIN_CONV_HALO_RF_TABLE(X)                                       \
    X(2, 2, false) X(2, 3, false) X(3, 2, false) X(3, 3, false)         \
    X(2, 2, true) X(2, 3, true) X(3, 2, true) X(3, 3, true)

struct RfInst { int ti, nks; bool dg; };

// the kernel of an instantiation as rocprofv3 prints it
std::string rf_kernel_name(const RfInst& r) {
    char s[64];
    snprintf(s, sizeof s, "conv_halo_rf_kernel<%d, %d, %s>", r.ti, r.nks, r.dg ? "true" : "false");
    return s;
}

// the table row of an instantiation: launched on `st` when `k` is given, only looked up otherwise; a tuple without a row is an error
int rf_row(const RfInst& r, const ConvK* k, hipStream_t st) {
    auto go = [&](auto kern) {
        if (!k) return DIN_OK;
        const int tiles = ((k->OH + RF_TH - 1) / RF_TH) * ((k->OW + RF_TW - 1) / RF_TW) * k->NB;
        const size_t lds = rf_lds(r.ti, r.dg, (k->flags & DIN_CONV_MASK) != 0);
        raise_lds_limit(kern, rf_lds(r.ti, r.dg, true));
        hipLaunchKernelGGL(kern, dim3(tiles < 256 ? tiles : 256), dim3(256), lds, st, *k);
        return DIN_OK;
    };
#define DIN_ROW(TI_, NKS_, DG_) \
    if (r.ti == TI_ && r.nks == NKS_ && r.dg == DG_) return go(conv_halo_rf_kernel<TI_, NKS_, DG_>);
    DIN_CONV_HALO_RF_TABLE(DIN_ROW)
#undef DIN_ROW
    DIN_FAIL(DIN_E_ARG, "conv_halo_rf: %s is not instantiated", rf_kernel_name(r).c_str());
}

// Eligibility, geometry and instantiation of the launch `which` (0 forward, 1 data gradient) of a descriptor: bf16, 3x3, stride 1,
// dilation 1, reduction and produced channels in 40 .. 96 and multiples of 8, views as conv_halo_kernel takes them except the mask view
// (whole 16-byte chunks: it travels by LDS-DMA).  Options: DIN_CONV_HALO=0 and DIN_CONV_HALO_RF=0 switch the kernel off, DIN_CONV_HALO_RF=2
// forces it on every eligible shape; unset, the planner's rule holds (rf_wanted: a floor on the pixels of the launch, no ACCUM).  Reads no pointer.
bool rf_wanted(int which, int flags, int cred, int cprod, int oh, int ow, int64_t M) {
    // padded-area waste of the 8 x 32 tile grid must stay moderate (plan_halo's rule)
    const int64_t padded = (int64_t)((oh + RF_TH - 1) / RF_TH * RF_TH) * ((ow + RF_TW - 1) / RF_TW * RF_TW);
    if (padded * 100 > (int64_t)oh * ow * 118) return false;
    // <= 64 -> <= 64 channels (VGG's conv1_2): the stem kernel's shape (conv_small.hip), never measured against this one
    if (cred <= 64 && cprod <= 64) return false;
    // accumulate operands are requested one or two pixel fragments at a time (the filters leave no registers for more): several exposed
    // memory round trips per tile, not measured against the old kernels -- no backbone layer asks for it
    if (flags & DIN_CONV_ACCUM) return false;
    // measured, old kernel against this one at 96 / 24 / 12 frames of 87 x 157 pixels (profiles/halo_rf_layers.txt): -21..-41 % at 96 frames,
    // -4..-32 % at 24, -5..-23 % at 12 except the forward with <= 64 reduction channels, which loses 9 % there (one wave per SIMD has
    // nothing to hide its prologue behind when a workgroup gets two or three tiles).  Below 12 frames nothing was measured: old kernels.
    const int64_t floor = (which == 0 && cred <= 64) ? 256 * 1024 : 160 * 1024;
    return M >= floor;
}

bool rf_plan(const din_conv_desc* d, int which, int flags, int ldm, int moff, ConvK& k, RfInst& r) {
    if (!d || (which != 0 && which != 1) || d->dtype != DIN_BF16 || d->in_u8) return false;
    if (d->nb <= 0 || d->h <= 0 || d->w <= 0 || d->cin <= 0 || d->cout <= 0) return false;
    if (d->kh != 3 || d->kw != 3 || d->sh != 1 || d->sw != 1 || d->dh != 1 || d->dw != 1) return false;
    if (d->oh != d->h + 2 * d->ph - 2 || d->ow != d->w + 2 * d->pw - 2 || d->oh <= 0 || d->ow <= 0) return false;
    if ((int64_t)d->nb * d->h * d->w >= (1ll << 31) || (int64_t)d->nb * d->oh * d->ow >= (1ll << 31)) return false;
    const int cred = which ? d->cout : d->cin, cprod = which ? d->cin : d->cout;
    if (cred % 8 != 0 || cprod % 8 != 0 || cred < 40 || cred > 96 || cprod < 40 || cprod > 96) return false;
    if (d->ldi % 8 != 0 || d->cioff % 8 != 0 || d->ldi < d->cioff + d->cin || d->ldo % 4 != 0 || d->cooff % 4 != 0 || d->ldo < d->cooff + d->cout) return false;
    if (which == 0 && (flags & ~(DIN_CONV_BIAS | DIN_CONV_RELU))) return false;
    if (which == 1) {
        if (flags & ~(DIN_CONV_MASK | DIN_CONV_ACCUM)) return false;
        if (d->ldo % 8 != 0 || d->cooff % 8 != 0) return false;                  // the gradient operand is read in whole chunks
        if ((flags & DIN_CONV_MASK) && (ldm % 8 != 0 || moff % 8 != 0 || moff < 0 || ldm < moff + cprod)) return false;
    }
    const char* hv = DIN_OPT("DIN_CONV_HALO");
    if (hv && atoi(hv) == 0) return false;
    const char* rv = DIN_OPT("DIN_CONV_HALO_RF");
    const int mode = rv ? atoi(rv) : 1;
    if (mode == 0) return false;
    k = ConvK{};
    k.NB = d->nb; k.kh = 3; k.kw = 3;
    const PackGeom bank = pack_geom(d, which);
    k.w_bytes = (long long)bank.rows_pad * bank.kelems * 2;
    k.ay = k.ax = 1; k.divy = k.divx = 1;
    if (which == 0) {
        k.H = d->h; k.W = d->w; k.Cin = d->cin; k.ldi = d->ldi; k.cioff = d->cioff;
        k.OH = d->oh; k.OW = d->ow; k.Cout = d->cout; k.ldo = d->ldo; k.cooff = d->cooff;
        k.by = -d->ph; k.bx = -d->pw; k.cy = k.cx = 1;
    } else {
        k.H = d->oh; k.W = d->ow; k.Cin = d->cout; k.ldi = d->ldo; k.cioff = d->cooff;
        k.OH = d->h; k.OW = d->w; k.Cout = d->cin; k.ldo = d->ldi; k.cooff = d->cioff;
        k.by = d->ph; k.bx = d->pw; k.cy = k.cx = -1;
    }
    k.M = k.NB * k.OH * k.OW;
    k.in_bytes = (long long)k.NB * k.H * k.W * k.ldi * 2;
    k.cpt = bank.cpt; k.Q = 9 * bank.cpt; k.nk = bank.nk; k.wld = bank.nk * KC;
    k.flags = flags; k.ldm = (flags & DIN_CONV_MASK) ? ldm : 0; k.moff = (flags & DIN_CONV_MASK) ? moff : 0;
    k.splitk = 1; k.ks_per_split = k.nk; k.n_co_tiles = 1;
    if (!din_gather::views_below_2g(k)) return false;
    if (mode != 2 && !rf_wanted(which, flags, cred, cprod, k.OH, k.OW, k.M)) return false;
    r.ti = cprod <= 64 ? 2 : 3; r.nks = cred <= 64 ? 2 : 3; r.dg = which == 1;
    return true;
}

}  // namespace

extern "C" {

int din_conv_rf_eligible(const din_conv_desc* d, int which, int flags, int ldm, int moff) {
    ConvK k; RfInst r;
    return rf_plan(d, which, flags, ldm, moff, k, r) && rf_row(r, nullptr, nullptr) == DIN_OK ? 1 : 0;
}

int din_conv_rf_fwd(const din_conv_desc* d, const void* in, const void* wpk, const float* bias, void* out, int flags,
                    void* workspace, int64_t workspace_bytes, void* stream) {
    (void)workspace; (void)workspace_bytes;                                      // (the argument list of din_conv_fwd: this kernel never splits its reduction)
    if (int e = din_conv::check_desc(d)) return e;
    DIN_REQUIRE(in && wpk && out, "conv_rf_fwd: null pointer");
    DIN_REQUIRE(!(flags & DIN_CONV_BIAS) || bias, "conv_rf_fwd: BIAS flag without bias");
    ConvK k; RfInst r;
    DIN_REQUIRE(rf_plan(d, 0, flags, 0, 0, k, r), "conv_rf_fwd: not eligible (ask din_conv_rf_eligible)");
    k.in = in; k.w = wpk; k.out = out; k.bias = bias;
    if (int e = rf_row(r, &k, as_stream(stream))) return e;
    DIN_CHECK_LAUNCH("conv_rf_fwd");
    return DIN_OK;
}

int din_conv_rf_dgrad(const din_conv_desc* d, const void* dout, const void* wpk_t, void* din_, const void* mask, int ldm, int moff, int flags,
                      void* workspace, int64_t workspace_bytes, void* stream) {
    (void)workspace; (void)workspace_bytes;
    if (int e = din_conv::check_desc(d)) return e;
    DIN_REQUIRE(dout && wpk_t && din_, "conv_rf_dgrad: null pointer");
    DIN_REQUIRE(!(flags & DIN_CONV_MASK) || mask, "conv_rf_dgrad: MASK flag without mask");
    ConvK k; RfInst r;
    DIN_REQUIRE(rf_plan(d, 1, flags, ldm, moff, k, r), "conv_rf_dgrad: not eligible (ask din_conv_rf_eligible)");
    k.in = dout; k.w = wpk_t; k.out = din_; k.mask = mask;
    if (int e = rf_row(r, &k, as_stream(stream))) return e;
    DIN_CHECK_LAUNCH("conv_rf_dgrad");
    return DIN_OK;
}

int din_conv_rf_kernel_names(const din_conv_desc* d, int which, int flags, int ldm, int moff, char* buf, int buf_bytes) {
    if (int e = din_conv::check_desc(d)) return e;
    DIN_REQUIRE(buf_bytes >= 0 && (buf || buf_bytes == 0), "conv_rf_kernel_names: bad argument");
    ConvK k; RfInst r;
    DIN_REQUIRE(rf_plan(d, which, flags, ldm, moff, k, r), "conv_rf_kernel_names: not eligible (ask din_conv_rf_eligible)");
    if (int e = rf_row(r, nullptr, nullptr)) return e;
    const std::string names = rf_kernel_name(r) + "\n";
    if (buf_bytes > 0) {
        const size_t n = names.size() < (size_t)buf_bytes - 1 ? names.size() : (size_t)buf_bytes - 1;
        memcpy(buf, names.data(), n);
        buf[n] = 0;
    }
    return (int)names.size() + 1;
}

}  // extern "C"
