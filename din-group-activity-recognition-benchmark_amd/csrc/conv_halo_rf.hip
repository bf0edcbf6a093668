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
// (rf::mfma); and the transfers of the next halo are issued one behind every second or fourth fragment of a block's first half from a
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
// (80 -> 192) does not fit the register file.  What the two families share -- the inline-asm primitives (rf::read, rf::mfma, rf::wait,
// rf::pin), the work items, the epilogue's mask / accumulate pieces, the planner's checks and the bodies of the entry points -- is in
// conv_halo_rf.h (namespace din_rf, rf:: below).
#include "din_common.h"
#include "conv_wgrad.h"
#include "conv_gather.h"
#include "conv_shared.h"
#include "conv_halo_rf.h"

using din_wgrad::lds_dma16;
using din_gather::ConvK;
namespace rf = din_rf;

namespace {

constexpr int RF_HWW = rf::TW + 2, RF_HWH = rf::TH + 2, RF_HPX = RF_HWW * RF_HWH;
constexpr int RF_PCH = 10, RF_PB = RF_PCH * 16;                                  // row pitch: 10 chunks = 160 bytes (conv_halo.hip)
constexpr int RF_NTR_H = (RF_HPX * RF_PCH + 255) / 256;                          // halo transfers per wave and block (14)
constexpr int RF_HB = RF_NTR_H * 4096;                                           // bytes of one halo buffer
// dynamic LDS: two halo buffers, then the four waves' mask regions (masked data gradient) or their bias values (forward)
constexpr size_t rf_lds(int ti, bool dg, bool mask) { return (size_t)2 * RF_HB + (dg ? (mask ? (size_t)4 * 4 * ti * 1024 : 0) : 1024); }

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
    const int tiles_x = (OW + rf::TW - 1) / rf::TW, tiles_y = (OH + rf::TH - 1) / rf::TH;
    const int tiles_img = tiles_x * tiles_y, nitems = tiles_img * p.NB;
    const long long img_bytes = (long long)H_ * W_ * ldi * 2ll;
    const long long oimg_bytes = (long long)OH * OW * ldo * 2ll, mimg_bytes = (long long)OH * OW * ldm * 2ll;
    const char* const inp = reinterpret_cast<const char*>(p.in);
    char* const outp = reinterpret_cast<char*>(p.out);
    const char* const maskp = reinterpret_cast<const char*>(p.mask);
    const bool masked = (flags & DIN_CONV_MASK) != 0;

    using rf::Item;
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
        h.gx0 = it.tx * rf::TW + hx0;
        h.base = ((it.ty * rf::TH + hy0) * W_ + h.gx0) * ldi * 2 + cioff2 + b * 128;
        h.nch = cpt - b * 8;                                                      // (>= 8: all)
        return h;
    };
    auto halo_one = [&](int buf, const HaloBlk& h, int i) __attribute__((always_inline)) {
        asm volatile("" : "+v"(rel[i]));                                          // the transfer's instructions stay HERE, between the MFMAs around them
        const int hx = (int)__builtin_amdgcn_ubfe(pk[i >> 1], 16 * (i & 1), 6), cc = (int)__builtin_amdgcn_ubfe(pk[i >> 1], 16 * (i & 1) + 8, 4);
        const bool ok = (unsigned)(h.gx0 + hx) < (unsigned)W_ && cc < h.nch;
        int voff = rel[i] + h.base;
        voff = ok ? voff : (int)rf::OOB;
        lds_dma16(ldsWv + (uint32_t)(buf * RF_HB + i * 4096), h.rs, voff, 0);
    };
    // transfer i of the wave's own mask region: chunk id = i * 64 + lane = (pixel pl of the wave's 128, chunk c of its 2 TI)
    auto mask_one = [&](const Item& it, int i) __attribute__((always_inline)) {
        int ln = lane;
        asm volatile("" : "+v"(ln));
        __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(maskp) + (long long)it.n * mimg_bytes, 0, (int)mimg_bytes, 0x00020000);
        const unsigned id = (unsigned)(i * 64 + ln), pl = id / (unsigned)(2 * TI), c = id - pl * (unsigned)(2 * TI);
        const int gy = it.ty * rf::TH + 4 * wp + (int)(pl >> 5), gx = it.tx * rf::TW + (int)(pl & 31u);
        const int co = cbase + (int)c * 8;
        const bool ok = gy < OH && gx < OW && co < Cout;
        lds_dma16(ldsMk + (uint32_t)(i * 1024), rs, ok ? ((gy * OW + gx) * ldm + moff + co) * 2 : (int)rf::OOB, 0);
    };

    const int G = (int)gridDim.x;
    int item = xcd_remap((int)blockIdx.x, G);
    if (item >= nitems) return;
    Item cur = rf::decode_item(item, tiles_img, tiles_x);
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
                    Wf[tap][ks][i] = __builtin_amdgcn_raw_buffer_load_b128(rsW, real ? chan * wld16 + g4 * 16 : (int)rf::OOB, (tap * cpt + ks * 4) * 16, 0);
                }
        // where they live is decided HERE (rf::mfma): the first NA fragments in accumulation registers, the others in architectural ones
        rf::static_for<0, 9 * NKS * TI>([&](auto N_) __attribute__((always_inline)) {
            constexpr int n = decltype(N_)::value, tap = n / (NKS * TI), ks = (n / TI) % NKS, i = n % TI;
            rf::pin<(n < NA)>(Wf[tap][ks][i]);
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
    f32x4 acc[TI][8];                                                             // (the first k-step of a tile writes them: rf::mfma<.., FIRST>)

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
                const int gy = it.ty * rf::TH + 4 * wp + (j >> 1), gx = it.tx * rf::TW + (j & 1) * 16 + frow_e;
                pxo[jj] = (gy < OH && gx < OW) ? ((gy * OW + gx) * ldo + cooff) * 2 : (int)rf::OOB;
#pragma unroll
                for (int i = 0; i < TI; ++i) {
                    const int co = cbase + g4_e * 4 * TI + i * 4;
                    if (DG && (flags & DIN_CONV_ACCUM)) old[DG ? jj : 0][i] = __builtin_amdgcn_raw_buffer_load_b64(rsO, rf::piece_off(pxo[jj], co, Cout), 0, 0);
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
                        rf::mask4(v, mk);
                    }
                    if (DG && (flags & DIN_CONV_ACCUM)) v = rf::accum4(v, old[DG ? jj : 0][i]);
                    __builtin_amdgcn_raw_buffer_store_b64(u32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])}, rsO, rf::piece_off(pxo[jj], co, Cout), 0, 0);
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
        const Item nxt = has_next_item ? rf::decode_item(item_n, tiles_img, tiles_x) : cur;
        rf::static_for<0, NBLK>([&](auto B_) __attribute__((always_inline)) {
            constexpr int b = decltype(B_)::value;
            constexpr int KB = b == NBLK - 1 ? NKS - 2 * b : 2;                  // 32-channel steps of this block per tap
            constexpr int NSTEP = 9 * KB, NF = NSTEP * 8;                        // steps = (tap, kk); fragments
            constexpr int SP = KB == 1 ? 2 : 4;                                   // fragments between two transfers: all issued in the block's first half
            static_assert(RF_NTR_H * SP <= NF / 2 + 8 && (RF_NTR_H + (b == 0 ? NTR_M : 0)) * SP <= NF, "every transfer of the block has a slot");
            constexpr bool last_blk = b == NBLK - 1;
            const bool hn = !last_blk || has_next_item;                           // a next (item, block) exists: its halo goes into buffer hb ^ 1
            const HaloBlk hnx = halo_blk(last_blk ? nxt : cur, last_blk ? 0 : b + 1);
            const uint32_t xa = xb0 + (uint32_t)(hb * RF_HB);
            rf::static_for<0, D>([&](auto F_) __attribute__((always_inline)) {
                constexpr int f = decltype(F_)::value;
                rf::read<rf_frag_off<DG>((f >> 3) / KB, (f >> 3) % KB, f & 7)>(xf[f], xa);
            });
            rf::static_for<0, NF>([&](auto F_) __attribute__((always_inline)) {
                constexpr int f = decltype(F_)::value;
                constexpr int step = f >> 3, j = f & 7, tap = step / KB, kk = step % KB, ks = 2 * b + kk;
                rf::wait<(NF - 1 - f < D - 1 ? NF - 1 - f : D - 1)>(xf[f % D]);
                rf::static_for<0, TI>([&](auto I_) __attribute__((always_inline)) {
                    constexpr int i = decltype(I_)::value;
                    rf::mfma<((tap * NKS + ks) * TI + i < NA), (b == 0 && step == 0)>(acc[i][j], Wf[tap][ks][i], xf[f % D]);
                });
                if constexpr (f + D < NF) {
                    constexpr int nf = f + D;
                    rf::read<rf_frag_off<DG>((nf >> 3) / KB, (nf >> 3) % KB, nf & 7)>(xf[f % D], xa);
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
        const int tiles = ((k->OH + rf::TH - 1) / rf::TH) * ((k->OW + rf::TW - 1) / rf::TW) * k->NB;
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

// the planner's rule (option unset): a floor on the pixels of the launch, no ACCUM
bool rf_wanted(int which, int flags, int cred, int cprod, int oh, int ow, int64_t M) {
    if (!rf::tile_waste_ok(oh, ow)) return false;
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

// Eligibility, geometry and instantiation of the launch `which` (0 forward, 1 data gradient) of a descriptor: what rf::plan_common asks of
// a 3x3 with 40 .. 96 channels.  Options: DIN_CONV_HALO=0 and DIN_CONV_HALO_RF=0 switch the kernel off, DIN_CONV_HALO_RF=2 forces it on
// every eligible shape; unset, the planner's rule holds (rf_wanted).  Reads no pointer.
bool rf_plan(const din_conv_desc* d, int which, int flags, int ldm, int moff, ConvK& k, RfInst& r) {
    if (!rf::plan_common(d, which, flags, ldm, moff, 3, 96, k)) return false;
    const char* rv = DIN_OPT("DIN_CONV_HALO_RF");
    const int mode = rv ? atoi(rv) : 1;
    const int cred = k.Cin, cprod = k.Cout;
    if (mode == 0 || (mode != 2 && !rf_wanted(which, flags, cred, cprod, k.OH, k.OW, k.M))) return false;
    r.ti = cprod <= 64 ? 2 : 3; r.nks = cred <= 64 ? 2 : 3; r.dg = which == 1;
    return true;
}

struct Rf3 {
    typedef RfInst Inst;
    static constexpr auto plan = rf_plan;
    static constexpr auto row = rf_row;
    static constexpr auto name = rf_kernel_name;
    static constexpr const char* prefix = "conv_rf";
};

}  // namespace

extern "C" {

int din_conv_rf_eligible(const din_conv_desc* d, int which, int flags, int ldm, int moff) { return rf::eligible<Rf3>(d, which, flags, ldm, moff); }

// (workspace: the argument list of din_conv_fwd / din_conv_dgrad; this kernel never splits its reduction)
int din_conv_rf_fwd(const din_conv_desc* d, const void* in, const void* wpk, const float* bias, void* out, int flags,
                    void* /*workspace*/, int64_t /*workspace_bytes*/, void* stream) {
    return rf::fwd<Rf3>(d, in, wpk, bias, out, flags, stream);
}

int din_conv_rf_dgrad(const din_conv_desc* d, const void* dout, const void* wpk_t, void* din_, const void* mask, int ldm, int moff, int flags,
                      void* /*workspace*/, int64_t /*workspace_bytes*/, void* stream) {
    return rf::dgrad<Rf3>(d, dout, wpk_t, din_, mask, ldm, moff, flags, stream);
}

int din_conv_rf_kernel_names(const din_conv_desc* d, int which, int flags, int ldm, int moff, char* buf, int buf_bytes) {
    return rf::kernel_names<Rf3>(d, which, flags, ldm, moff, buf, buf_bytes);
}

}  // extern "C"

